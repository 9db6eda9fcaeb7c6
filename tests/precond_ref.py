"""The multigrid and AMG preconditioners restated in fp64 with NumPy and
scipy.sparse, from what arcanefem_amd/csrc/multigrid.hip, amg.hip and
kcycle.hpp say they compute -- nothing is imported from the package:

  * the geometric prolongation P of nested Kuhn boxes (value 1 at fine node 2I,
    1/2 at the fine nodes 2I +- e, e in {0,1}^3 \\ 0, inside the box), expanded by
    kron(P, I_k); the 15-point Kuhn stencil of the coarse operator;
  * the algebraic prolongation of an `agg` array (P[i, agg[i]] = 1, a zero row
    where agg[i] < 0);
  * the Galerkin operator P^T A P and the bound |P|^T |A| |P| of its rounding;
  * one application z = F V(F r) + C D^-1 r of the cycle from explicit inputs
    (per level A, dinv, omega, P; sweeps; scale; dense coarsest level or sweeps;
    K-cycle levels with kcycle.hpp's coefficients), optionally with every
    level's values and every product's operand rounded to float32, or with the
    sums of every product taken in the reverse order.

tests/test_precond_ref.py checks this file on the CPU against the oracle's
assembly and against the theory of the symmetric V-cycle;
tests/test_gpu_precond_parts.py holds the kernels to it."""
import numpy as np
import scipy.sparse as sp

KUHN_E = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
# self + the 14 Kuhn edge directions
KUHN_STENCIL = [(0, 0, 0)] + KUHN_E + [(-a, -b, -c) for a, b, c in KUHN_E]


def node_id(dims, x, y, z):
    """Lexicographic node id on the box of dims = (nx, ny, nz) cells."""
    return x + (dims[0] + 1) * (y + (dims[1] + 1) * z)


def n_nodes(dims):
    return (dims[0] + 1) * (dims[1] + 1) * (dims[2] + 1)


def coarse_dims(dims):
    assert all(d % 2 == 0 and d >= 2 for d in dims), dims
    return tuple(d // 2 for d in dims)


def geometric_P(fine_dims, k=1):
    """Prolongation from the half-resolution box to the box of fine_dims cells:
    (k * fine nodes) x (k * coarse nodes), CSR."""
    cd = coarse_dims(fine_dims)
    X, Y, Z = np.meshgrid(np.arange(cd[0] + 1), np.arange(cd[1] + 1), np.arange(cd[2] + 1), indexing="ij")
    X, Y, Z = X.ravel(), Y.ravel(), Z.ravel()
    J = node_id(cd, X, Y, Z)
    rows, cols, vals = [], [], []
    for (a, b, c) in KUHN_STENCIL:
        fx, fy, fz = 2 * X + a, 2 * Y + b, 2 * Z + c
        ok = (fx >= 0) & (fy >= 0) & (fz >= 0) & (fx <= fine_dims[0]) & (fy <= fine_dims[1]) & (fz <= fine_dims[2])
        rows.append(node_id(fine_dims, fx[ok], fy[ok], fz[ok]))
        cols.append(J[ok])
        vals.append(np.full(int(ok.sum()), 1.0 if (a, b, c) == (0, 0, 0) else 0.5))
    P = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                      shape=(n_nodes(fine_dims), n_nodes(cd)))
    if k > 1:
        P = sp.kron(P, sp.identity(k), format="csr")
    P.sort_indices()
    return P


def kuhn_structure(dims):
    """Node CSR (row_ptr, sorted columns) of the 15-point Kuhn stencil on the box."""
    X, Y, Z = np.meshgrid(np.arange(dims[0] + 1), np.arange(dims[1] + 1), np.arange(dims[2] + 1), indexing="ij")
    X, Y, Z = X.ravel(), Y.ravel(), Z.ravel()
    rows, cols = [], []
    for (a, b, c) in KUHN_STENCIL:
        x, y, z = X + a, Y + b, Z + c
        ok = (x >= 0) & (y >= 0) & (z >= 0) & (x <= dims[0]) & (y <= dims[1]) & (z <= dims[2])
        rows.append(node_id(dims, X[ok], Y[ok], Z[ok]))
        cols.append(node_id(dims, x[ok], y[ok], z[ok]))
    n = n_nodes(dims)
    S = sp.csr_matrix((np.ones(sum(r.size for r in rows)), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    S.sort_indices()
    return S.indptr.astype(np.int64), S.indices.astype(np.int32)


def algebraic_P(agg, nc):
    """Piecewise-constant prolongation of an aggregate map: P[i, agg[i]] = 1,
    a zero row where agg[i] < 0."""
    agg = np.asarray(agg)
    i = np.nonzero(agg >= 0)[0]
    return sp.csr_matrix((np.ones(i.size), (i, agg[i])), shape=(agg.size, nc))


def level_matrix(row_ptr, columns, values, k=1, n_cols=None):
    """Scalar CSR of an operator in a level's own layout: node rows row_ptr /
    columns, and per node row r of len blocks k scalar rows of k * len values,
    values[k*k*row_ptr[r] + k*u*len + k*t + v] = entry (k*r + u, k*columns[t] + v).
    Duplicate columns are NOT summed away silently: see structure_of()."""
    row_ptr = np.asarray(row_ptr, np.int64)
    columns = np.asarray(columns, np.int64)
    nb = row_ptr.size - 1
    ln = np.diff(row_ptr)
    # scalar row k*r + u holds, in order, the k*len columns k*columns[t] + v
    sc_len = np.repeat(k * ln, k)
    indptr = np.concatenate([[0], np.cumsum(sc_len)])
    idx = np.empty(indptr[-1], np.int64)
    pos = 0
    for r in range(nb):
        c = (k * columns[row_ptr[r]:row_ptr[r + 1], None] + np.arange(k)[None, :]).ravel()
        for _ in range(k):
            idx[pos:pos + c.size] = c
            pos += c.size
    n = k * nb
    A = sp.csr_matrix((np.asarray(values, np.float64), idx, indptr), shape=(n, k * nb if n_cols is None else n_cols))
    return A


def galerkin(P, A):
    C = (P.T @ A @ P).tocsr()
    C.sort_indices()
    return C


def galerkin_bound(P, A):
    """|P|^T |A| |P|: the componentwise scale of the Galerkin sums' rounding."""
    C = (abs(P).T @ abs(A) @ abs(P)).tocsr()
    C.sort_indices()
    return C


def structural(A):
    """A's stored pattern as a matrix of ones (explicit zeros kept)."""
    S = sp.csr_matrix((np.ones(A.indices.size), A.indices.copy(), A.indptr.copy()), shape=A.shape)
    return S


def free_lambda_max(A, dinv, free=None):
    """lambda_max(D^-1 A) by a dense symmetric eigensolve of D^-1/2 A D^-1/2
    (rows with dinv <= 0, or outside `free`, left out)."""
    keep = dinv > 0 if free is None else (np.asarray(free, bool) & (dinv > 0))
    i = np.nonzero(keep)[0]
    s = np.sqrt(dinv[i])
    B = A[i][:, i].toarray() * s[:, None] * s[None, :]
    B = 0.5 * (B + B.T)
    return float(np.linalg.eigvalsh(B)[-1])


class Level:
    """One level of a replayed hierarchy.  P: prolongation from the next level
    (None on the coarsest); kcycle: this level's problem (as the coarse problem
    of the level above) is solved by the K-cycle's two Krylov steps."""

    def __init__(self, A, dinv, omega, P=None, kcycle=False):
        self.A = sp.csr_matrix(A)
        self.dinv = np.asarray(dinv, np.float64)
        self.omega = float(omega)
        self.P = None if P is None else sp.csr_matrix(P)
        self.kcycle = bool(kcycle)


def _reversed(M):
    """The same CSR matrix with every row's entries stored in the reverse order
    (scipy's product sums a row in storage order)."""
    M = sp.csr_matrix(M)
    order = np.empty(M.indices.size, np.int64)
    for r in range(M.shape[0]):
        a, e = M.indptr[r], M.indptr[r + 1]
        order[a:e] = np.arange(e - 1, a - 1, -1)
    R = sp.csr_matrix((M.data[order], M.indices[order], M.indptr.copy()), shape=M.shape)
    R.has_sorted_indices = False
    return R


class Cycle:
    """z = F V(F r) + C D^-1 r, as mg_apply / amg_apply order it.

    levels         list of Level, fine first
    sweeps         pre- and post-smoothing sweeps (damped Jacobi, the first from zero)
    scale          factor on the coarse correction of a level whose coarse problem is
                   one cycle (the AMG's AFEM_AMG_SCALE; 1 geometric); a K-cycle's
                   Krylov weights replace it
    dense_coarsest the coarsest level is solved exactly (np.linalg.solve), else
                   coarse_sweeps sweeps from zero (a one-level hierarchy: 2 * sweeps)
    cons, dinv_fix the constraint flags and the fine dinv of the exit fix
    f32            round the values of the levels in f32_levels (default: every
                   level) and the operand of each of their cycle products to float32
                   (f32_kcycle: also the K-cycle's own products A c1, A c2)
    reverse        every product's row sums in the reverse order
    After apply(): self.dropped lists the K-cycle steps that took a
    drop-the-step branch, self.coefs every (level, rho, alpha1, den, w1, w2)."""

    def __init__(self, levels, sweeps=1, scale=1.0, dense_coarsest=True, coarse_sweeps=16, cons=None, dinv_fix=None,
                 f32=False, f32_levels=None, f32_kcycle=False, reverse=False):
        self.lv = levels
        self.sweeps = sweeps
        self.scale = scale
        self.dense = dense_coarsest
        self.coarse_sweeps = coarse_sweeps
        n = levels[0].A.shape[0]
        self.cons = np.zeros(n, bool) if cons is None else np.asarray(cons, bool)
        self.dinv_fix = levels[0].dinv if dinv_fix is None else np.asarray(dinv_fix, np.float64)
        self.f32_kcycle = f32 and f32_kcycle
        self.dropped, self.coefs = [], []
        fl = set(range(len(levels))) if f32_levels is None else set(f32_levels)
        fix = _reversed if reverse else (lambda M: M)
        self.A, self.A32, self.P, self.PT = [], [], [], []
        for l, L in enumerate(levels):
            self.A.append(fix(L.A))
            if f32 and l in fl:
                with np.errstate(over="ignore"):  # a penalty above the fp32 range saturates
                    d32 = L.A.data.astype(np.float32).astype(np.float64)
                self.A32.append(fix(sp.csr_matrix((d32, L.A.indices, L.A.indptr), shape=L.A.shape)))
            else:
                self.A32.append(None)
            self.P.append(None if L.P is None else fix(L.P))
            self.PT.append(None if L.P is None else fix(sp.csr_matrix(L.P.T)))
        self._coarse_dense = None

    # the product of a cycle step (sweep, residual) on level l
    def _prod(self, l, x):
        if self.A32[l] is not None:
            return self.A32[l] @ x.astype(np.float32).astype(np.float64)
        return self.A[l] @ x

    # the K-cycle's own products
    def _kprod(self, l, x):
        if self.f32_kcycle and self.A32[l] is not None:
            return self.A32[l] @ x.astype(np.float32).astype(np.float64)
        return self.A[l] @ x

    def _smooth(self, l, b, x, sweeps):
        L = self.lv[l]
        s = 0
        if x is None:
            x = L.omega * L.dinv * b
            s = 1
        for _ in range(s, sweeps):
            x = x + L.omega * L.dinv * (b - self._prod(l, x))
        return x

    def _vcycle(self, l, b):
        last = l + 1 == len(self.lv)
        if last:
            if self.dense and l > 0:
                if self._coarse_dense is None:
                    self._coarse_dense = self.lv[l].A.toarray()
                return np.linalg.solve(self._coarse_dense, b)
            return self._smooth(l, b, None, 2 * self.sweeps if l == 0 else self.coarse_sweeps)
        x = self._smooth(l, b, None, self.sweeps)
        r = b - self._prod(l, x)
        bc = self.PT[l] @ r
        kc = self.lv[l + 1].kcycle
        xc = self._kcycle(l + 1, bc) if kc else self._vcycle(l + 1, bc)
        x = x + (1.0 if kc else self.scale) * (self.P[l] @ xc)
        return self._post(l, b, x)

    def _post(self, l, b, x):
        L = self.lv[l]
        for _ in range(self.sweeps):
            x = x + L.omega * L.dinv * (b - self._prod(l, x))
        return x

    def _kcycle(self, l, b):
        """kcycle.hpp: c1 = B b, v1 = A c1, rho = c1.v1, alpha1 = c1.b / rho,
        rt = b - alpha1 v1, c2 = B rt, v2 = A c2, gamma = c2.v1, beta = c2.v2,
        delta = c2.rt, alpha2 = delta / (beta - gamma^2 / rho),
        x = (alpha1 - gamma alpha2 / rho) c1 + alpha2 c2; a zero or non-positive
        curvature drops the step."""
        c1 = self._vcycle(l, b)
        v1 = self._kprod(l, c1)
        rho = float(c1 @ v1)
        a1 = float(c1 @ b) / rho if rho > 0.0 else 0.0
        rt = b - a1 * v1
        c2 = self._vcycle(l, rt)
        v2 = self._kprod(l, c2)
        gam, bet, dl = float(c2 @ v1), float(c2 @ v2), float(c2 @ rt)
        den = bet - gam * gam / rho if rho > 0.0 else bet
        a2 = dl / den if den > 0.0 else 0.0
        w1 = a1 - gam * a2 / rho if rho > 0.0 else a1
        if not rho > 0.0:
            self.dropped.append((l, "rho", rho))
        if not den > 0.0:
            self.dropped.append((l, "den", den))
        self.coefs.append((l, rho, a1, den, w1, a2))
        return w1 * c1 + a2 * c2

    def apply(self, r):
        r = np.asarray(r, np.float64)
        self.dropped, self.coefs = [], []
        b = np.where(self.cons, 0.0, r)
        z = self._vcycle(0, b)
        z = z.copy()
        z[self.cons] = r[self.cons] * self.dinv_fix[self.cons]
        return z

    def dense_inverse(self):
        """M^-1 column by column (a linear cycle: no K-cycle level)."""
        n = self.lv[0].A.shape[0]
        M = np.empty((n, n))
        e = np.zeros(n)
        for j in range(n):
            e[j] = 1.0
            M[:, j] = self.apply(e)
            e[j] = 0.0
        return M


def geometric_hierarchy(A, dims, k=1, dense_max=512, omega_of=None):
    """The one-rank geometric hierarchy of multigrid.hip from the fine operator:
    coarsen while the level has more than dense_max DoF and even cell counts
    (nx, nz >= 2); A_c = P^T A P; dinv = 1 / diag; omega_of(A, dinv) -> omega
    (default: 4 / (3 lambda_max) with the true lambda_max).  Returns (levels,
    dims per level, dense: the coarsest level is inverted densely)."""
    if omega_of is None:
        def omega_of(A, dinv):
            return 4.0 / (3.0 * free_lambda_max(A, dinv))
    mats, dl = [sp.csr_matrix(A)], [tuple(dims)]
    Ps = []
    while True:
        d = dl[-1]
        if mats[-1].shape[0] <= dense_max or any(x % 2 for x in d) or d[0] < 2 or d[2] < 2:
            break
        P = geometric_P(d, k)
        Ps.append(P)
        mats.append(galerkin(P, mats[-1]))
        dl.append(coarse_dims(d))
    levels = []
    for l, M in enumerate(mats):
        diag = M.diagonal()
        dinv = np.where(diag != 0.0, 1.0 / np.where(diag != 0.0, diag, 1.0), 0.0)
        levels.append(Level(M, dinv, omega_of(M, dinv), Ps[l] if l < len(Ps) else None))
    dense = len(mats) > 1 and mats[-1].shape[0] <= dense_max
    return levels, dl, dense


def hashed_vector(n, seed=1):
    """A dense deterministic vector in [-1, 1) (splitmix64 of the index)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (2.0 / 9007199254740992.0) - 1.0
