"""tests/precond_ref.py checked on the CPU, so that the reference is not
validated by the kernels it will judge (tests/test_gpu_precond_parts.py):

  * on an unjittered Kuhn box the grids are nested, so the geometric P^T A P of
    the oracle's fine matrix IS the oracle's own assembly on the half-resolution
    box, up to rounding (Poisson and block-3 elasticity);
  * its sparsity is exactly the 15-point Kuhn stencil;
  * the replayed V-cycle with the true omega = 4 / (3 lambda_max) is a symmetric
    positive definite M^-1 with the spectrum of M^-1 A on the free rows in (0, 2)
    (theory: I - M^-1 A = S (I - P A_c^-1 P^T A) S is A-self-adjoint with
    eigenvalues in [0, 1), S = I - omega D^-1 A having its own in (-1/3, 1));
  * the K-cycle's coefficients are the two flexible-CG steps they claim to be,
    and its non-positive-curvature branches drop the step;
  * the fp32 and reversed-order modes move the result by rounding only."""
import numpy as np
import pytest
import scipy.sparse as sp

import precond_ref as R
from oracle import oracle as O

EPS = np.finfo(np.float64).eps
E, NU = 21e5, 0.28
LAM = E * NU / ((1 + NU) * (1 - 2 * NU))
MU2 = 2 * E / (2 * (1 + NU))


def _poisson(n, nz=None, jitter=0.0, seed=1):
    m = O.structured_mesh(3, n, nz, jitter=jitter, seed=seed)
    nn = m["n_own"]
    rp, cols = O.sparsity(nn, nn, m["cells"])
    vals, _ = O.assemble_poisson(nn, m["cells"], m["coords"], rp, cols, 0.0, with_rhs=False)
    return sp.csr_matrix((vals, cols, rp), shape=(nn, nn)), rp, cols


def _elasticity(n, nz=None, jitter=0.0, seed=1):
    m = O.structured_mesh(3, n, nz, jitter=jitter, seed=seed)
    nn = m["n_own"]
    rp, cols = O.sparsity(nn, nn, m["cells"])
    vals, _ = O.assemble_elasticity_tet(nn, m["cells"], m["coords"], rp, cols, LAM, MU2)
    A = sp.bsr_matrix((vals.reshape(-1, 3, 3), cols, rp), shape=(3 * nn, 3 * nn)).tocsr()
    A.sort_indices()
    return A, rp, cols


def _same_structure(A, B):
    A, B = sp.csr_matrix(A), sp.csr_matrix(B)
    A.sort_indices()
    B.sort_indices()
    return np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)


def test_prolongation_is_p1_interpolation():
    """P interpolates every function that is linear on the coarse box exactly,
    its columns are the coarse hat functions (value 1 at 2I, 15 entries inside),
    and kron(P, I_k) acts per component."""
    fd = (4, 4, 2)
    cd = R.coarse_dims(fd)
    P = R.geometric_P(fd)
    assert P.shape == (R.n_nodes(fd), R.n_nodes(cd))

    def coords(d, h):
        X, Y, Z = np.meshgrid(np.arange(d[0] + 1), np.arange(d[1] + 1), np.arange(d[2] + 1), indexing="ij")
        i = R.node_id(d, X, Y, Z).ravel()
        c = np.zeros((R.n_nodes(d), 3))
        c[i] = np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1) * h
        return c

    cf, cc = coords(fd, 1.0), coords(cd, 2.0)
    for w in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.3, -1.1, 0.7)):
        assert np.abs(P @ (cc @ w + 0.25) - (cf @ w + 0.25)).max() <= 8 * EPS * 5.0
    assert np.array_equal(np.asarray(P.sum(1)).ravel(), np.ones(P.shape[0]))  # a partition of unity
    # the hat function of the coarse node (1, 1, 0) on the bottom face of the 2 x 2 x 1 box: 1 at the
    # fine node (2, 2, 0), 1/2 at the 2I +- e inside the box (z >= 0 leaves the 7 e, and -e with e_z = 0: 3)
    col = P[:, R.node_id(cd, 1, 1, 0)].toarray().ravel()
    assert col[R.node_id(fd, 2, 2, 0)] == 1.0 and np.count_nonzero(col == 0.5) == 10 and np.count_nonzero(col) == 11
    assert set(np.unique(P.data)) == {0.5, 1.0}
    P3 = R.geometric_P(fd, 3)
    x = R.hashed_vector(3 * P.shape[1])
    assert np.array_equal((P3 @ x).reshape(-1, 3), np.stack([P @ x[c::3] for c in range(3)], 1))


@pytest.mark.parametrize("n,nz", [(8, 8), (8, 4)])
def test_geometric_galerkin_is_the_coarse_assembly_poisson(n, nz):
    A, _, _ = _poisson(n, nz)
    Ac, crp, ccols = _poisson(n // 2, nz // 2)
    P = R.geometric_P((n, n, nz))
    G = R.galerkin(P, A)
    bound = R.galerkin_bound(P, A)
    # structure: the product of the STRUCTURES (exact zeros of the Kuhn Laplacian kept)
    S = R.galerkin(P, R.structural(A))
    krp, kcols = R.kuhn_structure((n // 2, n // 2, nz // 2))
    assert np.array_equal(S.indptr, krp) and np.array_equal(S.indices, kcols)
    assert np.array_equal(crp, krp) and np.array_equal(ccols, kcols)  # ... and the oracle's own sparsity
    assert np.array_equal(np.diff(krp).max(), 15)
    diff = abs(G - Ac).toarray()
    assert (diff <= 512 * EPS * bound.toarray()).all(), (diff.max(), bound.max())
    assert abs(G).max() > 0.1  # (not a comparison of zeros)


def test_geometric_galerkin_is_the_coarse_assembly_elasticity():
    n = 8
    A, _, _ = _elasticity(n)
    Ac, crp, ccols = _elasticity(n // 2)
    P = R.geometric_P((n, n, n), 3)
    G = R.galerkin(P, A)
    bound = R.galerkin_bound(P, A).toarray()
    S = R.galerkin(P, R.structural(A))
    assert _same_structure(S, R.structural(Ac))
    krp, kcols = R.kuhn_structure((n // 2,) * 3)
    assert np.array_equal(crp, krp) and np.array_equal(ccols, kcols)
    diff = abs(G - Ac).toarray()
    assert (diff <= 512 * EPS * bound).all(), (diff / np.maximum(bound, 1e-300)).max() / EPS


def test_level_matrix_layout():
    """The level layout (k scalar rows of k * len values per node row) against
    the per-block layout of the oracle."""
    m = O.structured_mesh(3, 2, jitter=0.2, seed=3)
    nn = m["n_own"]
    rp, cols = O.sparsity(nn, nn, m["cells"])
    vals, _ = O.assemble_elasticity_tet(nn, m["cells"], m["coords"], rp, cols, LAM, MU2)
    A = sp.bsr_matrix((vals.reshape(-1, 3, 3), cols, rp), shape=(3 * nn, 3 * nn)).toarray()
    B = R.level_matrix(rp, cols, O.blocks_to_row_order_k(rp, vals, 3), 3)
    assert np.array_equal(B.toarray(), A)
    assert np.array_equal(R.level_matrix(rp, cols, np.arange(cols.size, dtype=float), 1).data, np.arange(cols.size))


def _penalised(A, dofs, penalty=1e30):
    A = sp.lil_matrix(A)
    for d in dofs:
        A[d, d] = penalty
    return sp.csr_matrix(A)


def _cons_of(A):
    d = A.diagonal()
    off = np.asarray(abs(A).sum(1)).ravel() - np.abs(d)
    return np.abs(d) > 1e10 * off


@pytest.mark.parametrize("n,dense_max", [(4, 64), (8, 512)])
def test_replayed_vcycle_is_spd_and_contracts(n, dense_max):
    """n = 4: 125 -> 27 rows (dense_max lowered so that a coarse level exists);
    n = 8: 729 -> 125, the library's own shape."""
    A, _, _ = _poisson(n, jitter=0.2, seed=11)
    A = 1.7 * A
    bottom = np.arange((n + 1) ** 2)
    A = _penalised(A, bottom)
    cons = _cons_of(A)
    assert np.array_equal(np.nonzero(cons)[0], bottom)
    levels, dims, dense = R.geometric_hierarchy(A, (n, n, n), 1, dense_max=dense_max)
    assert len(levels) == 2 and dense and dims[1] == (n // 2,) * 3
    for L in levels:
        lam = R.free_lambda_max(L.A, L.dinv)
        assert abs(L.omega * lam - 4.0 / 3.0) < 1e-12
    cyc = R.Cycle(levels, sweeps=1, dense_coarsest=dense, cons=cons)
    M = cyc.dense_inverse()
    scale = np.abs(M[~cons][:, ~cons]).max()
    free = np.nonzero(~cons)[0]
    Mf = M[np.ix_(free, free)]
    assert np.abs(Mf - Mf.T).max() <= 1e-13 * scale
    # the constraint block is C D^-1 and nothing couples it to the free rows
    assert np.array_equal(M[np.ix_(bottom, bottom)], np.diag(levels[0].dinv[bottom]))
    assert not M[np.ix_(free, bottom)].any() and not M[np.ix_(bottom, free)].any()
    w = np.linalg.eigvalsh(0.5 * (Mf + Mf.T))
    assert w[0] > 0
    Af = A[free][:, free].toarray()
    # M^-1 A ~ M^-1/2 A M^-1/2: symmetric, same spectrum
    Lc = np.linalg.cholesky(0.5 * (Mf + Mf.T))
    ev = np.linalg.eigvalsh(Lc.T @ Af @ Lc)
    assert ev[0] > 0 and ev[-1] < 2, (ev[0], ev[-1])
    assert ev[-1] <= 1 + 1e-10  # (the sharper statement of the theory above)
    assert ev[0] > 0.1  # and it is a preconditioner: kappa(M^-1 A) < 10 against kappa(A) ~ n^2


def test_replay_modes_move_the_result_by_rounding_only():
    n = 8
    A, _, _ = _elasticity(n, jitter=0.2, seed=5)
    dofs = np.arange(3 * (n + 1) ** 2)
    A = _penalised(A, dofs)
    cons = _cons_of(A)
    levels, _, dense = R.geometric_hierarchy(A, (n, n, n), 3)
    assert [L.A.shape[0] for L in levels] == [2187, 375] and dense
    r = R.hashed_vector(A.shape[0], 3)
    z = R.Cycle(levels, cons=cons).apply(r)
    zr = R.Cycle(levels, cons=cons, reverse=True).apply(r)
    z32 = R.Cycle(levels, cons=cons, f32=True).apply(r)
    s = np.abs(z).max()
    assert 0 < np.abs(zr - z).max() <= 1e-13 * s
    assert 1e-9 * s < np.abs(z32 - z).max() <= 1e-5 * s
    assert np.array_equal(z[cons], r[cons] * levels[0].dinv[cons])
    # z on the free rows does not see r on the constraint rows
    r2 = r.copy()
    r2[cons] = 7.0
    assert np.array_equal(R.Cycle(levels, cons=cons).apply(r2)[~cons], z[~cons])


def test_kcycle_is_two_flexible_cg_steps():
    """With B the cycle of a level, the K-cycle's x minimises the A-norm error
    over span{c1, c2} (c1 = B b, c2 = B (b - alpha1 A c1)): the Galerkin
    conditions c_i . (b - A x) = 0 hold; and it is never worse than c1 alone."""
    n = 16
    A, _, _ = _poisson(n, jitter=0.2, seed=2)
    A = _penalised(A, np.arange((n + 1) ** 2))
    cons = _cons_of(A)
    levels, _, dense = R.geometric_hierarchy(A, (n, n, n), 1)
    assert [L.A.shape[0] for L in levels] == [4913, 729, 125] and dense
    levels[1].kcycle = True
    cyc = R.Cycle(levels, cons=cons)
    b = R.hashed_vector(729, 9)
    A1 = levels[1].A
    x = cyc._kcycle(1, b)
    assert not cyc.dropped
    (_, rho, a1, den, w1, w2), = cyc.coefs
    c1 = cyc._vcycle(1, b)
    c2 = cyc._vcycle(1, b - a1 * (A1 @ c1))
    res = b - A1 @ x
    sc = np.abs(b).max() * max(np.abs(c1).max(), np.abs(c2).max()) * b.size
    assert abs(c1 @ res) <= 1e-12 * sc and abs(c2 @ res) <= 1e-12 * sc
    xs = np.linalg.solve(A1.toarray(), b)

    def enorm(e):
        return float(e @ (A1 @ e))

    assert enorm(x - xs) <= enorm(a1 * c1 - xs) <= enorm(c1 - xs) * (1 + 1e-12)
    # the branches: an indefinite "operator" gives rho <= 0 -> both weights as kcycle.hpp has them
    neg = [R.Level(-L.A, L.dinv, L.omega, L.P, L.kcycle) for L in levels]
    cn = R.Cycle(neg, cons=cons)
    xn = cn._kcycle(1, b)
    assert [d[1] for d in cn.dropped] == ["rho", "den"] or [d[1] for d in cn.dropped] == ["rho"]
    (_, rho, a1, den, w1, w2), = cn.coefs
    assert rho <= 0 and a1 == 0.0 and w1 == 0.0
    assert np.array_equal(xn, w2 * cn._vcycle(1, b))


def test_algebraic_prolongation_and_galerkin():
    A, _, _ = _poisson(4, jitter=0.2, seed=4)
    n = A.shape[0]
    agg = (np.arange(n) // 5).astype(np.int32)
    agg[::7] = -1
    nc = int(agg.max()) + 1
    P = R.algebraic_P(agg, nc)
    assert P.shape == (n, nc) and P.nnz == int((agg >= 0).sum())
    G = R.galerkin(P, A).toarray()
    D = A.toarray()
    ref = np.zeros((nc, nc))
    for i in range(n):
        for j in range(n):
            if agg[i] >= 0 and agg[j] >= 0:
                ref[agg[i], agg[j]] += D[i, j]
    assert np.abs(G - ref).max() <= 64 * EPS * np.abs(D).sum(1).max() * 5
