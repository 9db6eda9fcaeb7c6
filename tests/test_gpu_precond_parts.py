"""The multigrid (multigrid.hip) and AMG (amg.hip) preconditioners part by part:
every level's operator, D^-1, omega, the aggregates and one application of the
cycle are read through the diagnostic entries (afem_ls_precond_*) and held to the
fp64 restatement of tests/precond_ref.py, which tests/test_precond_ref.py checks
on the CPU.  A PCG repairs a wrong preconditioner by itself, so the solve tests
(test_gpu_multigrid.py, test_gpu_amg.py) cannot see any of this.

Shapes: the smallest that reach each branch (kDenseMax = 512 DoF; level 0 is
never dense) -- see GEO below.  Every system is jittered, has a Poisson
coefficient of 1.7 and a Dirichlet face (penalty 1e30; once row elimination),
so constraint rows exist.

Bounds (none of them measured on the code under test):
  * Galerkin: |A_gpu - P^T A P| <= 512 eps |P|^T |A| |P| componentwise (at most
    15 * 15 * 2 summands per entry of the geometric product);
  * omega lambda_max(D^-1 A) < 2 with lambda_max from a dense eigensolve: the
    damped-Jacobi sweep contracts;
  * one application, fp64 cycle: 64 x the largest difference, over the test's
    right-hand sides, of two CPU replays that differ only in the order of every
    row sum (CSR entries reversed), relative to max |z_ref|;
  * one application, fp32 cycle: 4 x the deviation of the replay's own fp32 mode
    (values and product operands rounded to float32) from its fp64 mode.
The measured figures are recorded in the docstrings of the tests."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csgraph

import arcanefem_amd as af
from arcanefem_amd.gmsh import read_gmsh
from oracle import oracle as O

import precond_ref as R
from golden_cases import path

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
COEF = 1.7
E, NU = 21e5, 0.28
LAM = E * NU / ((1 + NU) * (1 - 2 * NU))
MU2 = 2 * E / (2 * (1 + NU))

# name: (k, n, nz, level rows, coarsest level dense, Dirichlet method)
GEO = {
    "s8": (1, 8, 8, [729, 125], True, "penalty"),
    "s16": (1, 16, 16, [4913, 729, 125], True, "penalty"),
    "s16x4": (1, 16, 4, [1445, 243], True, "penalty"),       # an anisotropic box
    "s8elim": (1, 8, 8, [729, 125], True, "row-elimination"),
    "b8": (3, 8, 8, [2187, 375], True, "penalty"),
    "b12": (3, 12, 12, [6591, 1029, 192], True, "penalty"),
    # an odd 5-cell grid stops the coarsening above kDenseMax: 16 sweeps on the coarsest level
    "b10": (3, 10, 10, [3993, 648], False, "penalty"),
}
# name: (mesh, NB_DOF, AFEM_AMG_DENSE)
AMG = {
    "sphere": ("sphere_cut.msh", 1, "16"),
    "lshape": ("L-shape-3D.msh", 1, "16"),
    "sphere3": ("sphere_cut.msh", 3, "32"),
}
THETA = 0.05  # AFEM_AMG_THETA's default


# ------------------------------------------------------------------ systems
class System:
    """An assembled system with its Dirichlet rows set, kept for the session."""

    def __init__(self, ctx, name):
        self.ctx, self.name = ctx, name
        if name in GEO:
            self.k, n, nz, self.rows, self.dense, method = GEO[name]
            self.kind, self.pc, self.env = "geometric", "multigrid", {}
            self.dims = (n, n, nz)
            self.mesh = af.Mesh.structured(ctx, 3, n, nz, jitter=0.2, seed=17 + n)
            fixed = self.mesh.bottom_nodes()
        else:
            mesh_name, self.k, dense = AMG[name]
            self.kind, self.pc, self.env = "algebraic", "amg", {"AFEM_AMG_DENSE": dense}
            method = "penalty"
            gm = read_gmsh(path(mesh_name))
            self.mesh = af.Mesh.from_arrays(ctx, gm.dim, gm.cells, gm.coords)
            if self.k == 1:
                fixed = gm.group_nodes("horizontal" if mesh_name == "sphere_cut.msh" else "bot").astype(np.int32)
            else:
                z = gm.coords[:, 2]
                fixed = np.nonzero(z <= z.min() + 0.15 * (z.max() - z.min()))[0].astype(np.int32)
        mesh, k = self.mesh, self.k
        self.cells, self.coords, _ = mesh.download()
        self.nn = mesh.n_own_nodes
        self.n = k * self.nn
        self.bsr = af.BSRFormat(mesh, k).initialize(True)
        self.bsr.computeSparsity()
        self.ls = af.DoFLinearSystem().initialize(ctx, self.n, k * mesh.n_nodes)
        if k == 1:
            self.bsr.assemblePoissonP1(COEF, 5.5, self.ls.rhsVariable())
        else:
            self.bsr.assembleElasticityP1Ex(LAM, MU2, 0.0, (0.0, 0.0, -1.0), self.ls.rhsVariable(), rhs_mode="set")
        self.bsr.toLinearSystem(self.ls)
        self.fixed_nodes = np.asarray(fixed, np.int64)
        self.dofs = (k * self.fixed_nodes[:, None] + np.arange(k)[None, :]).ravel().astype(np.int32)
        self.method = method
        if method == "penalty":
            self.ls.applyDirichletViaPenalty(self.dofs, 0.5 if k == 1 else 0.0, 1e30)
        else:
            self.ls.applyDirichletViaRowElimination(self.dofs, 0.5)
        self.d_r = ctx.malloc(8 * self.n)
        self.d_z = ctx.malloc(8 * self.n)
        self._oracle = None

    def prepare(self, variant, **env):
        """Set the knobs, run the prelude, copy the hierarchy."""
        for key, val in {**self.env, **env}.items():
            variant(key, val)
        self.ls.setSolverOptions(rtol=1e-12, max_iter=5000, method="pcg", preconditioner=self.pc)
        assert self.ls.precondPrepare() == self.kind
        n_lv = self.ls.precondLevelInfo(0)["levels"]
        return [self.ls.precondLevel(l) for l in range(n_lv)]

    def apply(self, r):
        self.ctx.to_device(self.d_r, np.ascontiguousarray(r, np.float64))
        self.ls.precondApply(self.d_r, self.d_z)
        return self.ctx.to_host(self.d_z, self.n, np.float64)

    def oracle_matrix(self):
        """The oracle's assembly with the Dirichlet rows, as a scalar CSR."""
        if self._oracle is None:
            rp, cols = O.sparsity(self.mesh.n_nodes, self.nn, self.cells)
            if self.k == 1:
                vals, _ = O.assemble_poisson(self.nn, self.cells, self.coords, rp, cols, 0.0, with_rhs=False)
                A = sp.csr_matrix((COEF * vals, cols, rp), shape=(self.n, self.n))
            else:
                vals, _ = O.assemble_elasticity_tet(self.nn, self.cells, self.coords, rp, cols, LAM, MU2)
                A = sp.bsr_matrix((vals.reshape(-1, 3, 3), cols, rp), shape=(self.n, self.n)).tocsr()
            A.sort_indices()
            for d in self.dofs:  # in place: an eliminated row keeps its (zeroed) entries
                a, e = A.indptr[d], A.indptr[d + 1]
                on_diag = A.indices[a:e] == d
                if self.method == "penalty":
                    A.data[a:e][on_diag] = 1e30
                else:
                    A.data[a:e] = on_diag.astype(np.float64)
            self._oracle = A
        return self._oracle

    def rhs_set(self):
        """A hashed dense vector, unit vectors at a corner node, at an interior
        node and on a constraint row."""
        n, k = self.n, self.k
        free = np.setdiff1d(np.arange(n), self.dofs)
        corner = int(free[-1])  # the last free DoF: the box's far top corner
        if self.kind == "geometric":
            d = self.dims
            interior = k * int(R.node_id(d, d[0] // 2 + 1, d[1] // 2, d[2] // 2 + 1)) + (k - 1)
        else:
            interior = int(free[len(free) // 2])
        out = {"hashed": R.hashed_vector(n, 5)}
        for nm, i in (("corner", corner), ("interior", interior), ("cons", int(self.dofs[len(self.dofs) // 2]))):
            e = np.zeros(n)
            e[i] = 1.0
            out[nm] = e
        return out


@pytest.fixture(scope="module")
def systems(ctx):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = System(ctx, name)
        return cache[name]

    yield get
    for s in cache.values():
        ctx.free(s.d_r)
        ctx.free(s.d_z)
        s.bsr.close()
        s.mesh.close()


# ------------------------------------------------------------------ the replay from the copied levels
def _matrix(lv):
    return R.level_matrix(lv["row_ptr"], lv["columns"], lv["values"], lv["k"])


def _prolongation(levels, l):
    lv = levels[l]
    if lv["kind"] == "geometric":
        return R.geometric_P(lv["dims"], lv["k"])
    return R.algebraic_P(lv["agg"], lv["n_agg"])


def _cycle(levels, **kw):
    """precond_ref.Cycle fed with the device's own levels and omegas."""
    mats = [_matrix(lv) for lv in levels]
    L = [R.Level(mats[l], lv["dinv"], lv["omega"], _prolongation(levels, l) if l + 1 < len(levels) else None,
                 lv["kcycle"]) for l, lv in enumerate(levels)]
    d0 = mats[0].diagonal()
    dinv_fix = np.where(d0 != 0.0, 1.0 / np.where(d0 != 0.0, d0, 1.0), 0.0)  # the PCG's dinv (k_inv_diag)
    last = levels[-1]
    alg = last["kind"] == "algebraic"
    return R.Cycle(L, sweeps=last["sweeps"], scale=last["scale"], dense_coarsest=last["dense"],
                   coarse_sweeps=last["coarse_sweeps"], cons=levels[0]["cons"].astype(bool), dinv_fix=dinv_fix,
                   f32_levels=[l for l, lv in enumerate(levels) if lv["has_f32"]], f32_kcycle=alg, **kw)


def _order_gate(levels, rs):
    """64 x the largest relative difference of two CPU replays that differ only
    in the summation order, over the right-hand sides; and the references."""
    fwd, rev = _cycle(levels), _cycle(levels, reverse=True)
    refs, worst = {}, 0.0
    for nm, r in rs.items():
        z = fwd.apply(r)
        if r[~fwd.cons].any():
            assert not fwd.dropped, (nm, fwd.dropped)  # no K-cycle coefficient took a drop-the-step branch
        else:  # r on a constraint row only: the cycle's input F r is zero (rho = 0 is the exact answer, x = 0)
            assert not z[~fwd.cons].any()
        refs[nm] = z
        worst = max(worst, np.abs(rev.apply(r) - z).max() / np.abs(z).max())
    assert worst > 0.0
    return 64.0 * worst, worst, refs


# ------------------------------------------------------------------ hierarchy: shapes, Galerkin, dinv, omega
def _check_galerkin(levels, what):
    worst = 0.0
    for l in range(1, len(levels)):
        A = _matrix(levels[l - 1])
        P = _prolongation(levels, l - 1)
        C = _matrix(levels[l])
        cols = levels[l]["columns"]
        rp = levels[l]["row_ptr"]
        # no duplicate column: strictly increasing within every row
        inc = np.diff(cols.astype(np.int64)) > 0
        ends = rp[1:-1] - 1  # the last entry of a row is followed by the next row's first
        inc[ends[(ends >= 0) & (ends < inc.size)]] = True
        assert inc.all(), (what, l, "duplicate or unsorted column")
        # no missing and no extra column: the structure of the product of the structures
        S = R.galerkin(P, R.structural(A))
        Cs = C.copy()
        Cs.sort_indices()
        assert np.array_equal(Cs.indptr, S.indptr) and np.array_equal(Cs.indices, S.indices), (what, l)
        if levels[l]["kind"] == "geometric":
            krp, kc = R.kuhn_structure(levels[l]["dims"])
            assert np.array_equal(rp, krp) and np.array_equal(cols, kc), (what, l)
        G = R.galerkin(P, A)
        B = R.galerkin_bound(P, A)
        diff = abs(C - G).tocsr()
        over = (diff - 512 * EPS * B).tocsr()
        assert over.nnz == 0 or over.data.max() <= 0.0, (what, l, over.data.max())
        ratio = (diff.toarray() / np.maximum(B.toarray(), 1e-300)).max() / EPS
        worst = max(worst, ratio)
    return worst


def _check_dinv_omega(levels, what):
    ratios = []
    for l, lv in enumerate(levels):
        A = _matrix(lv)
        d = A.diagonal()
        alg = lv["kind"] == "algebraic"
        cons = lv["cons"].astype(bool)
        if alg:
            # (outside the strength graph -- constraint rows, no positive diagonal -- the AMG's D^-1 is 0)
            in_graph = lv["in_graph"].astype(bool)
            assert np.array_equal(in_graph, (d > 0) & ~cons), (what, l)
            expect = np.where(in_graph, 1.0 / np.where(in_graph, d, 1.0), 0.0)
        else:
            expect = np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 0.0)
        assert np.array_equal(lv["dinv"], expect), (what, l)
        lam = R.free_lambda_max(A, lv["dinv"], free=~cons)
        assert 0.0 < lv["omega"] and lv["omega"] * lam < 2.0, (what, l, lv["omega"], lam)
        est = 4.0 / (3.0 * (1.1 if alg else 1.05) * lv["omega"])  # the power iteration's estimate behind omega
        ratios.append(est / lam)
    return ratios


@pytest.mark.parametrize("name", list(GEO))
def test_geometric_hierarchy(systems, variant, name):
    """Level shapes, flags, A_0 against the oracle's assembly, every A_l against
    P^T A_{l-1} P of the device's own A_{l-1} (structure: the 15-point Kuhn
    stencil, no duplicate, no missing column), dinv = 1 / diag exactly and
    omega lambda_max < 2.

    Measured (MI355X): Galerkin |A_gpu - P^T A P| / (|P|^T |A| |P|) at most
    1.61 eps over the seven systems (bound 512 eps).  Power-iteration estimate
    (12 iterations) over the true lambda_max(D^-1 A), per level: s8 0.904 0.890;
    s16 0.907 0.860 0.929; s16x4 0.928 0.860; s8elim 0.904 0.968; b8 0.953 0.967;
    b12 0.939 0.962 0.949; b10 0.939 0.927 -- with the 5 % margin in omega,
    omega lambda_max lies between 1.31 and 1.48 (4/3 with the true value)."""
    s = systems(name)
    levels = s.prepare(variant, AFEM_MG_F32="0")
    k, n, nz, rows, dense, _ = GEO[name]
    assert [lv["rows"] for lv in levels] == rows
    for l, lv in enumerate(levels):
        assert lv["kind"] == "geometric" and lv["k"] == k and lv["levels"] == len(rows)
        assert lv["dims"] == (n >> l, n >> l, nz >> l) and lv["block_rows"] * k == lv["rows"]
        assert not lv["distributed"] and not lv["has_f32"] and not lv["kcycle"]
        assert lv["dense"] == (dense and l + 1 == len(rows))
        assert lv["sweeps"] == 1 and lv["scale"] == 1.0
    assert levels[-1]["coarse_sweeps"] == 16
    # level 0 is the system: the oracle's assembly with its Dirichlet rows
    A0, Ao = _matrix(levels[0]), s.oracle_matrix()
    A0.sort_indices()
    assert np.array_equal(A0.indptr, Ao.indptr) and np.array_equal(A0.indices, Ao.indices)
    assert np.abs(A0.data - Ao.data).max() <= 1e-12 * np.abs(Ao.data[Ao.data < 1e29]).max()
    assert np.array_equal(np.nonzero(levels[0]["cons"])[0], np.sort(s.dofs))
    worst = _check_galerkin(levels, name)
    ratios = _check_dinv_omega(levels, name)
    print(f"{name}: Galerkin error / bound-scale {worst:.2f} eps; power estimate / lambda_max "
          f"{' '.join(f'{r:.3f}' for r in ratios)}; omega lambda_max "
          f"{' '.join(f'{4 / (3 * 1.05 * r):.3f}' for r in ratios)}")


@pytest.mark.parametrize("name", list(AMG))
def test_amg_hierarchy(systems, variant, name):
    """The aggregates (agg = -1 exactly on the constraint rows and the rows
    without a positive diagonal; every id used; ap / mem the inverse of agg;
    every aggregate connected in the strength graph; nc = the next level's
    rows), every A_l against P^T A_{l-1} P, dinv and omega.

    Measured (MI355X): level rows sphere 194 18 3, lshape 108 9, sphere3 582 15;
    Galerkin error at most 1.46 eps of the bound's scale.  Power-iteration
    estimate (8 iterations, signed start) over the true lambda_max, per level:
    sphere 0.952 0.933 0.869; lshape 0.955 0.989; sphere3 0.876 0.992 (omega
    carries a 10 % margin: omega lambda_max up to 1.40)."""
    s = systems(name)
    levels = s.prepare(variant, AFEM_AMG_F32="0")
    assert len(levels) >= 2 and levels[0]["rows"] == s.n
    assert np.array_equal(np.nonzero(levels[0]["cons"])[0], np.sort(s.dofs))
    for l, lv in enumerate(levels):
        last = l + 1 == len(levels)
        assert lv["kind"] == "algebraic" and lv["k"] == 1 and not lv["distributed"] and not lv["has_f32"]
        assert lv["dense"] == last and lv["scale"] == 1.7 and lv["sweeps"] == 1
        A = _matrix(lv)
        d = A.diagonal()
        cons = lv["cons"].astype(bool)
        if last:
            assert lv["n_agg"] == 0 and lv["rows"] <= int(AMG[name][2])
            continue
        agg, ap, mem, nc = lv["agg"], lv["agg_ptr"], lv["members"], lv["n_agg"]
        assert nc == levels[l + 1]["rows"]
        assert np.array_equal(agg < 0, cons | ~(d > 0)), (name, l)
        assert agg.max() == nc - 1 and np.array_equal(np.unique(agg[agg >= 0]), np.arange(nc))
        # ap / mem: each aggregated row once, under its own aggregate
        assert ap[0] == 0 and (np.diff(ap) > 0).all() and ap[-1] == mem.size == int((agg >= 0).sum())
        assert np.array_equal(np.sort(mem), np.nonzero(agg >= 0)[0])
        assert np.array_equal(agg[mem], np.repeat(np.arange(nc), np.diff(ap)))
        # connected in the strength graph |a_ij| >= theta sqrt(|a_ii a_jj|)
        C = A.tocoo()
        strong = (C.row != C.col) & (agg[C.row] >= 0) & (agg[C.row] == agg[C.col]) & \
                 (np.abs(C.data) >= THETA * np.sqrt(np.abs(d[C.row] * d[C.col])))
        G = sp.csr_matrix((np.ones(int(strong.sum())), (C.row[strong], C.col[strong])), shape=A.shape)
        ncomp, label = csgraph.connected_components(G, directed=False)
        comp_of_agg = {}
        for i in np.nonzero(agg >= 0)[0]:
            assert comp_of_agg.setdefault(int(agg[i]), int(label[i])) == int(label[i]), (name, l, int(agg[i]))
    worst = _check_galerkin(levels, name)
    ratios = _check_dinv_omega(levels, name)
    print(f"{name}: rows {[lv['rows'] for lv in levels]}; Galerkin error / bound-scale {worst:.2f} eps; "
          f"power estimate / lambda_max {' '.join(f'{r:.3f}' for r in ratios)}")


# ------------------------------------------------------------------ one application
FP64_CASES = [(nm, kc, fu) for nm in ("s8", "s16", "s16x4", "s8elim", "b8", "b12", "b10", "sphere", "lshape", "sphere3")
              for kc in ("0", "2") for fu in ("0", "1")]


@pytest.mark.parametrize("name,kcyc,fuse", FP64_CASES)
def test_apply_fp64_cycle(systems, variant, name, kcyc, fuse):
    """One application with the cycle in fp64 (AFEM_*_F32=0), K-cycle off and on,
    AFEM_*_FUSE 0 and 1, for the four right-hand sides: equal to the replay fed
    with the copied levels and omegas, within 64 x the replays' own
    summation-order difference; the replay's K-cycle took no drop-the-step
    branch; the constraint rows are r * dinv exactly.

    Measured (MI355X), largest over the right-hand sides, relative to max |z_ref|,
    CPU order difference / GPU difference (the gate is 64 x the first; fuse 0 and
    1 give the same figures: without an fp32 copy there is nothing to fuse):
      system   V-cycle               K-cycle 2
      s8       2.68e-16 / 7.48e-16   = (level 1 is dense: no K-cycle level)
      s16      2.67e-16 / 8.23e-16   8.32e-16 / 7.19e-16
      s16x4    1.66e-16 / 4.36e-16   =
      s8elim   1.87e-16 / 1.88e-15   =
      b8       5.28e-16 / 2.37e-14   =   (the dense 375-row elasticity level)
      b12      9.52e-16 / 2.99e-15   5.38e-15 / 3.68e-15
      b10      3.18e-16 / 2.12e-16   6.25e-16 / 7.50e-16
      sphere   2.36e-16 / 2.77e-16   3.22e-16 / 4.02e-16
      lshape   2.70e-16 / 3.82e-15   =
      sphere3  3.06e-16 / 5.44e-16   =
    s8elim stood at 1.54e-02 before the coarsest level's dense inverse handled a
    non-symmetric operator (multigrid section)."""
    s = systems(name)
    p = "AFEM_MG" if s.kind == "geometric" else "AFEM_AMG"
    levels = s.prepare(variant, **{p + "_F32": "0", p + "_KCYCLE": kcyc, p + "_FUSE": fuse})
    assert not any(lv["has_f32"] for lv in levels)
    kc_levels = [l for l, lv in enumerate(levels) if lv["kcycle"]]
    # (a K-cycle level: 1..k, except a dense coarsest level, which is solved exactly)
    assert kc_levels == [l for l in range(1, len(levels)) if l <= int(kcyc) and not levels[l]["dense"]]
    rs = s.rhs_set()
    gate, order, refs = _order_gate(levels, rs)
    cons = levels[0]["cons"].astype(bool)
    d0 = _matrix(levels[0]).diagonal()
    worst = 0.0
    for nm, r in rs.items():
        z = s.apply(r)
        err = np.abs(z - refs[nm]).max() / np.abs(refs[nm]).max()
        worst = max(worst, err)
        assert np.array_equal(z[cons], r[cons] * (1.0 / d0[cons])), (name, nm)
    print(f"{name} kcycle={kcyc} fuse={fuse}: CPU order difference {order:.2e}, gate {gate:.2e}, GPU {worst:.2e}")
    assert worst <= gate, (name, worst, gate)


@pytest.mark.parametrize("name", ["b8", "b12", "b10", "sphere", "lshape", "sphere3"])
def test_apply_fp32_cycle(systems, variant, name):
    """The defaults (block-3 geometric: every level's cycle products on fp32
    copies; AMG: the same, with its default K-cycle), fused and unfused: against
    the fp64 replay, within 4 x the deviation of the replay's own fp32 mode from
    its fp64 mode on the same r; fused = unfused bits.

    Measured (MI355X), relative to max |z_ref|, the replay's fp32 deviation / the
    GPU's deviation from the fp64 replay (the margin is 4 x the first), hashed r:
    b8 5.47e-08 / 4.36e-08; b12 6.47e-08 / 5.25e-08; b10 4.56e-08 / 3.92e-08;
    sphere 5.65e-08 / 5.72e-08; lshape 7.68e-08 / 5.72e-08; sphere3 3.77e-08 /
    2.69e-08; the unit vectors: between 1.5e-08 and 5.7e-08 / 8.2e-09 and 5.4e-08;
    r on a constraint row: 0 / 0."""
    s = systems(name)
    p = "AFEM_MG" if s.kind == "geometric" else "AFEM_AMG"
    rs = s.rhs_set()
    zs = {}
    for fuse in ("0", "1"):
        levels = s.prepare(variant, **{p + "_FUSE": fuse})
        assert all(lv["has_f32"] for lv in levels)
        zs[fuse] = {nm: s.apply(r) for nm, r in rs.items()}
    c64, c32 = _cycle(levels), _cycle(levels, f32=True)
    for nm, r in rs.items():
        ref = c64.apply(r)
        sc = np.abs(ref).max()
        margin = 4.0 * np.abs(c32.apply(r) - ref).max() / sc
        err = np.abs(zs["1"][nm] - ref).max() / sc
        print(f"{name} {nm}: replay fp32 deviation {margin / 4:.2e}, margin {margin:.2e}, GPU {err:.2e}")
        # (r on a constraint row only: F r = 0, both replays and the device give exactly C D^-1 r)
        free_part = r[~c64.cons].any()
        assert (margin > 0.0 or not free_part) and err <= margin, (name, nm, err, margin)
        assert np.array_equal(zs["0"][nm], zs["1"][nm]), (name, nm)
        assert not free_part or (not c64.dropped and not c32.dropped)


# ------------------------------------------------------------------ SPD
def _dense_inverse(s):
    M = np.empty((s.n, s.n))
    e = np.zeros(s.n)
    for j in range(s.n):
        e[j] = 1.0
        M[:, j] = s.apply(e)
        e[j] = 0.0
    return M


@pytest.mark.parametrize("name", ["s8", "sphere"])
def test_dense_inverse_is_spd(systems, variant, name):
    """M^-1 column by column (scalar n = 8: 729 applications; the sphere AMG)
    with the V-cycle in fp64: symmetric within the fp64 gate, the symmetrised
    matrix positive definite, equal to the replay's dense M^-1; with the default
    cycle (fp32 on the AMG; the scalar geometric cycle has no fp32 copy) the
    asymmetry stays within the fp32 margin.

    Measured (MI355X): asymmetry max |M - M^T| / max |M| on the free rows: s8
    9.15e-17 (gate 1.72e-14), sphere 1.27e-16 (gate 1.51e-14); against the
    replay's dense M^-1 3.66e-16 / 1.69e-16; eigenvalues of the symmetrised free
    block 0.341 .. 171 (s8) and 0.115 .. 38.3 (sphere); the default cycle: s8 the
    same bits (a scalar geometric cycle has no fp32 copy), sphere with the fp32
    V-cycle 1.27e-16 (margin 2.78e-07)."""
    s = systems(name)
    p = "AFEM_MG" if s.kind == "geometric" else "AFEM_AMG"
    levels = s.prepare(variant, **{p + "_F32": "0", p + "_KCYCLE": "0"})
    cons = levels[0]["cons"].astype(bool)
    free = np.nonzero(~cons)[0]
    gate, order, _ = _order_gate(levels, s.rhs_set())
    M = _dense_inverse(s)
    Mf = M[np.ix_(free, free)]
    sc = np.abs(Mf).max()
    asym = np.abs(Mf - Mf.T).max() / sc
    Mr = _cycle(levels).dense_inverse()
    dev = np.abs(M - Mr)[np.ix_(free, free)].max() / sc
    w = np.linalg.eigvalsh(0.5 * (Mf + Mf.T))
    print(f"{name}: gate {gate:.2e}, asymmetry {asym:.2e}, against the replay {dev:.2e}, eigenvalues {w[0]:.3e} .. "
          f"{w[-1]:.3e}")
    assert asym <= gate and dev <= gate, (asym, dev, gate)
    assert w[0] > 0.0
    # the constraint block: C D^-1, coupled to nothing
    ci = np.nonzero(cons)[0]
    assert np.array_equal(M[np.ix_(ci, ci)], np.diag(1.0 / _matrix(levels[0]).diagonal()[ci]))
    assert not M[np.ix_(free, ci)].any() and not M[np.ix_(ci, free)].any()
    # the default cycle
    levels = s.prepare(variant, **{p + "_F32": None, p + "_KCYCLE": "0"})
    M2 = _dense_inverse(s)[np.ix_(free, free)]
    asym32 = np.abs(M2 - M2.T).max() / np.abs(M2).max()
    if any(lv["has_f32"] for lv in levels):
        c64, c32 = _cycle(levels), _cycle(levels, f32=True)
        margin = 0.0
        for r in s.rhs_set().values():
            ref = c64.apply(r)
            margin = max(margin, 4.0 * np.abs(c32.apply(r) - ref).max() / np.abs(ref).max())
    else:
        margin = gate
    print(f"{name}: default cycle asymmetry {asym32:.2e}, margin {margin:.2e}")
    assert asym32 <= margin


# ------------------------------------------------------------------ constraint rows
@pytest.mark.parametrize("name", ["s8", "s8elim", "b8", "sphere", "sphere3"])
def test_constraint_rows(systems, variant, name):
    """z[cons] == r[cons] * dinv[cons] exactly, and z on the free rows does not
    change when r on the constraint rows does (default cycle, fused and not)."""
    s = systems(name)
    p = "AFEM_MG" if s.kind == "geometric" else "AFEM_AMG"
    for fuse in ("0", "1"):
        levels = s.prepare(variant, **{p + "_FUSE": fuse})
        cons = levels[0]["cons"].astype(bool)
        assert cons.sum() == s.dofs.size
        dinv = 1.0 / _matrix(levels[0]).diagonal()
        r = R.hashed_vector(s.n, 11)
        z = s.apply(r)
        assert np.array_equal(z[cons], r[cons] * dinv[cons])
        r2 = r.copy()
        r2[cons] = 3.0 + R.hashed_vector(int(cons.sum()), 12)
        z2 = s.apply(r2)
        assert np.array_equal(z2[~cons], z[~cons])
        assert np.array_equal(z2[cons], r2[cons] * dinv[cons])


# ------------------------------------------------------------------ prepare + solve = solve
@pytest.mark.parametrize("name", ["s16", "b8", "sphere"])
def test_solve_after_prepare_is_the_plain_solve(systems, variant, name):
    """prepare, a few applications, then solve: the bits and the iteration count
    of the solve alone."""
    s = systems(name)
    for key, val in s.env.items():
        variant(key, val)
    rhs = s.ls.rhs_host().copy()
    s.ls.setSolverOptions(rtol=1e-12, max_iter=5000, method="pcg", preconditioner=s.pc)
    st0 = s.ls.solve()
    x0 = s.ls.solution_host().copy()
    assert st0["converged"]
    s.ls.set_rhs_host(rhs)
    assert s.ls.precondPrepare() == s.kind
    s.apply(R.hashed_vector(s.n, 2))
    s.apply(rhs)
    st1 = s.ls.solve()
    assert st1["converged"] and st1["iterations"] == st0["iterations"]
    assert np.array_equal(s.ls.solution_host(), x0)
    assert np.array_equal(s.ls.rhs_host(), rhs)


def test_diagnostic_entries_need_a_hierarchy(ctx):
    mesh = af.Mesh.structured(ctx, 3, 8)
    bsr = af.BSRFormat(mesh, 1).initialize(True)
    bsr.computeSparsity()
    ls = af.DoFLinearSystem().initialize(ctx, mesh.n_own_nodes, mesh.n_nodes)
    bsr.assemblePoissonP1(1.0, 1.0, ls.rhsVariable())
    bsr.toLinearSystem(ls)
    ls.applyDirichletViaPenalty(mesh.bottom_nodes(), 0.0, 1e30)
    ls.setSolverOptions(method="pcg", preconditioner="jacobi")
    assert ls.precondPrepare() is None
    d = ctx.malloc(8 * 2 * mesh.n_own_nodes)
    with pytest.raises(af.AfemError):
        ls.precondApply(d, d + 8 * mesh.n_own_nodes)
    with pytest.raises(af.AfemError):
        ls.precondLevelInfo(0)
    ls.setSolverOptions(preconditioner="multigrid")
    assert ls.precondPrepare() == "geometric"
    with pytest.raises(af.AfemError):
        ls.precondLevelInfo(2)
    with pytest.raises(af.AfemError):
        ls.precondApply(d, d)
    ctx.free(d)
    bsr.close()
    mesh.close()


# ------------------------------------------------------------------ the distributed geometric hierarchy
def _levels_of(res, prefix):
    """The level dicts a dist_worker "mg_parts" rank saved (DoFLinearSystem.precondLevel's)."""
    out = []
    for l in range(int(res[prefix + "levels"])):
        lv = {key[len(f"{prefix}L{l}_"):]: val for key, val in res.items() if key.startswith(f"{prefix}L{l}_")}
        for key in ("levels", "k", "rows", "block_rows", "nnz_blocks", "n_agg", "sweeps", "coarse_sweeps"):
            lv[key] = int(lv[key])
        for key in ("distributed", "dense", "has_f32", "kcycle"):
            lv[key] = bool(lv[key])
        lv.update(kind="geometric", dims=tuple(int(x) for x in lv["dims"]), omega=float(lv["omega"]),
                  scale=float(lv["scale"]), slab=tuple(int(x) for x in lv["slab"]))
        out.append(lv)
    return out


def _global_nodes(lv, l, l2g, n_local):
    """Global node id of every local node id of a rank's level: the mesh's own map on level 0;
    on a distributed coarse level the owned layers, then the ghost layer below, then above
    (multigrid.hip SlabMap); the identity on a replicated level."""
    if not lv["distributed"]:
        return np.arange(n_local)
    if l == 0:
        return l2g
    k0, nown, glo, _ = lv["slab"]
    L = (lv["dims"][0] + 1) * (lv["dims"][1] + 1)
    q = np.arange(n_local)
    li, pos = q // L, q % L
    gz = np.where(li < nown, k0 + li, np.where((li == nown) & (glo != 0), k0 - 1, k0 + nown))
    return pos + L * gz


@pytest.mark.parametrize("case,world", [("mg_parts", 2), ("mg_parts", 3), ("mg_parts_b3", 2)])
def test_distributed_geometric_hierarchy(case, world, tmp_path):
    """z-slabs of one box over the host transport (tests/dist_worker.py): mapped to
    global node ids, the owned rows of every distributed level (k_mg_fat_rows,
    k_mg_galerkin_dist) and every rank's copy of the gathered level
    (k_mg_galerkin_part, summed over the ranks) equal the one-rank hierarchy's
    rows under the Galerkin bound, omega agrees, and one global application of
    the same global r equals the one-rank application within the fp64 gate.

    omega: the distributed power iteration runs the one-rank sequence by global
    index; 12 normalised products that differ in summation order only -- held
    to 1e-10 relative.

    Measured (MI355X): level rows against the one-rank hierarchy, in eps of the
    bound's scale: scalar x2 and x3 0.00 (the gathered level's sums come out the
    same), block-3 x2 1.07.  One application, relative to max |z_ref|: CPU order
    difference 2.95e-16 (gate 1.89e-14), slabs against one rank 1.18e-15 (x2) and
    5.90e-16 (x3); block-3: 9.08e-16 (gate 5.81e-14), 4.55e-15."""
    import dist_worker as W
    import test_gpu_distributed as D

    res = D._run(case, world, tmp_path)
    k = 3 if case == "mg_parts_b3" else 1
    n, nz = W.MG_PARTS["n"], W.MG_PARTS["nz"]
    one = _levels_of(res[0], "one_")
    per_rank = [_levels_of(r, "") for r in res]
    assert [lv["rows"] for lv in one] == ([4131, 675, 135] if k == 3 else [1377, 225])
    assert [lv["distributed"] for lv in per_rank[0]] == ([True, True, False] if k == 3 else [True, False])
    assert one[-1]["dense"] and all(lv[-1]["dense"] for lv in per_rank)
    mats = [_matrix(lv) for lv in one]
    worst = 0.0
    for l, ref in enumerate(one):
        A1 = mats[l].tocsr()
        A1.sort_indices()
        N = A1.shape[0]
        if l == 0:
            tol = sp.csr_matrix(A1.shape)
            flat = 1e-12 * np.abs(A1.data[np.abs(A1.data) < 1e29]).max()
        else:
            tol = 512 * EPS * R.galerkin_bound(R.geometric_P(one[l - 1]["dims"], k), mats[l - 1])
            flat = 0.0
        parts = []
        for r, lvs in zip(res, per_rank):
            lv = lvs[l]
            assert lv["dims"] == ref["dims"] and lv["k"] == k and lv["dense"] == ref["dense"]
            assert abs(lv["omega"] - ref["omega"]) <= 1e-10 * ref["omega"], (l, lv["omega"], ref["omega"])
            n_local = max(int(lv["columns"].max()) + 1, lv["block_rows"])
            g = _global_nodes(lv, l, r["l2g"], n_local)
            M = R.level_matrix(lv["row_ptr"], lv["columns"], lv["values"], k, n_cols=k * n_local).tocoo()
            gdof = (k * np.asarray(g, np.int64)[:, None] + np.arange(k)[None, :]).ravel()
            G = sp.csr_matrix((M.data, (gdof[M.row], gdof[M.col])), shape=(N, N))
            if lv["distributed"]:
                parts.append(G)
            else:
                parts = [G]  # replicated: every rank's copy is checked on its own
                _cmp_level(G, A1, tol, flat, (case, world, l))
        if per_rank[0][l]["distributed"]:
            G = sum(parts[1:], parts[0]).tocsr()  # the ranks own disjoint rows
            assert sum(p.nnz for p in parts) == G.nnz
            worst = max(worst, _cmp_level(G, A1, tol, flat, (case, world, l)))
    # one application of the same global r
    r_glob = R.hashed_vector(k * (n + 1) * (n + 1) * (nz + 1), 7)
    z = np.full(r_glob.size, np.nan)
    for r in res:
        own = r["l2g"][:int(r["n_own"])].astype(np.int64)
        z[(k * own[:, None] + np.arange(k)[None, :]).ravel()] = r["z"]
    z1 = np.empty_like(z)
    own = res[0]["one_l2g"][:int(res[0]["one_n_own"])].astype(np.int64)
    z1[(k * own[:, None] + np.arange(k)[None, :]).ravel()] = res[0]["one_z"]
    gate, order, refs = _order_gate(one, {"hashed": r_glob})
    sc = np.abs(refs["hashed"]).max()
    e_dist, e_one = np.abs(z - z1).max() / sc, np.abs(z1 - refs["hashed"]).max() / sc
    print(f"{case} x{world}: level rows against one rank: worst {worst:.2f} eps of the bound's scale; apply: CPU order "
          f"difference {order:.2e}, gate {gate:.2e}, slabs against one rank {e_dist:.2e}, one rank against the "
          f"replay {e_one:.2e}")
    assert not np.isnan(z).any() and e_dist <= gate and e_one <= gate, (e_dist, e_one, gate)


def _cmp_level(G, A1, tol, flat, what):
    G = G.tocsr()
    G.sort_indices()
    assert np.array_equal(G.indptr, A1.indptr) and np.array_equal(G.indices, A1.indices), what
    diff = abs(G - A1).tocsr()
    over = diff - tol
    over = over.tocsr()
    assert over.nnz == 0 or over.data.max() <= flat, (what, over.data.max())
    T = tol.toarray() if tol.nnz else None
    return 0.0 if T is None else float((diff.toarray() / np.maximum(T, 1e-300)).max() * 512)
