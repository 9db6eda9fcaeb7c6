"""CPU: pin tests/pcg_ref.py (the NumPy restatement of ls_solve's Jacobi-PCG)
and the generators of tests/csr_cases.py.

pcg_ref is held to three references: oracle.c's orc_pcg_jacobi (the same
constraint rule and x0 lift, written independently in C) on the reference's
own Poisson cases, np.linalg.solve on small dense systems, and the textbook
property that CG on an n x n SPD system has no residual left after n steps.
"""
import numpy as np
import pytest

import csr_cases as CC
import pcg_ref
from arcanefem_amd.gmsh import read_gmsh
from golden_cases import CASES, path
from oracle import oracle as O


def _golden_system(case, method="penalty"):
    mfile, f, bcs, _, P = CASES[case]
    m = read_gmsh(path(mfile))
    rp, cols = O.sparsity(m.n_nodes, m.n_nodes, m.cells)
    vals, rhs = O.assemble_poisson(m.n_nodes, m.cells, m.coords, rp, cols, 0.0 if f is None else f)
    for g, v in bcs:
        if method == "penalty":
            O.dirichlet_penalty(m.group_nodes(g), v, P, rp, cols, vals, rhs)
        else:
            O.row_elimination(m.group_nodes(g), v, rp, cols, vals, rhs)
    return rp, cols, vals, rhs


GOLDEN_SYSTEMS = [(c, "penalty") for c in CASES] + [("circle_2D", "row-elimination"), ("L-shape_3D", "row-elimination")]


@pytest.mark.parametrize("case,method", GOLDEN_SYSTEMS)
def test_restatement_matches_oracle_pcg(case, method):
    """After exactly k steps the iterate equals orc_pcg_jacobi's to rounding (1e-12 of max |x|: k <= 25
    steps of a recurrence whose steps each round at 2^-53), and a tolerance-stopped run tested every
    iteration stops at the oracle's iteration with the oracle's residual."""
    rp, cols, vals, rhs = _golden_system(case, method)
    for k in (1, 2, 7, 25):
        xo, ito, _, _ = O.pcg_jacobi(rp, cols, vals, rhs, max_iter=-k)
        res = pcg_ref.pcg(rp, cols, vals, rhs, fixed_iterations=k)
        assert ito == k and res["iterations"] == k
        assert np.abs(res["x"] - xo).max() <= 1e-12 * np.abs(xo).max()
    xo, ito, reso, _ = O.pcg_jacobi(rp, cols, vals, rhs, rtol=1e-10)
    res = pcg_ref.pcg(rp, cols, vals, rhs, rtol=1e-10, check_every=1)
    assert res["converged"] and res["iterations"] == ito
    assert abs(res["rel_residual"] - reso) <= 1e-6 * reso
    # check_every = 8: the first multiple of 8 at or after the oracle's stop
    res8 = pcg_ref.pcg(rp, cols, vals, rhs, rtol=1e-10, check_every=8)
    assert res8["converged"] and res8["iterations"] == -(-ito // 8) * 8


@pytest.mark.parametrize("n", [1, 2, 257, 1000, 1001])
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_restatement_solves_dense(n, dtype):
    """Penalty rows, row-eliminated rows (non-symmetric) and duplicate diagonal entries: the converged
    iterate is the dense solution; eliminated rows come back as their value exactly."""
    (rp, cols, vals, nc), b = CC.spd_system(n)
    res = pcg_ref.pcg(rp, cols, vals, b, rtol=1e-14, check_every=1, dtype=dtype)
    xd = np.linalg.solve(O.csr_to_dense(rp, cols, vals, nc), b)
    assert res["converged"]
    assert np.abs(res["x"].astype(np.float64) - xd).max() <= 1e-11 * np.abs(xd).max()
    ident = (np.diff(rp) >= 1) & (res["dinv"] == 1) & res["cons"]
    assert np.array_equal(res["x"][ident].astype(np.float64), b[ident])


@pytest.mark.parametrize("n", [1, 2, 5, 12])
def test_n_steps_leave_no_residual(n):
    """CG on an n x n SPD system: after n steps the residual is at rounding level (longdouble
    restatement: 1e-12 of |b| leaves room for the loss of orthogonality at n = 12)."""
    (rp, cols, vals, nc), b = CC.spd_system(n, name=f"tiny{n}", per_row=2, n_penalty=0, n_elim=0, n_dup=1)
    res = pcg_ref.pcg(rp, cols, vals, b, fixed_iterations=n, dtype=np.longdouble)
    r = b.astype(np.longdouble) - pcg_ref.spmv(rp, cols, vals.astype(np.longdouble), res["x"])
    assert np.abs(r).max() <= 1e-12 * np.abs(b).max()


def test_degenerate_inputs():
    (rp, cols, vals, nc), b = CC.spd_system(257)
    res = pcg_ref.pcg(rp, cols, vals, np.zeros(257))
    assert res["iterations"] == 0 and res["converged"] and not res["x"].any()
    # every row a constraint: x_i = b_i / a_ii, the stopping reference falls back to r.z over all rows
    n = 65
    rp = np.arange(n + 1, dtype=np.int64)
    cols = np.arange(n, dtype=np.int32)
    d = CC.values(CC.rng_for("diag"), n)
    b = CC.values(CC.rng_for("rhs"), n)
    res = pcg_ref.pcg(rp, cols, d, b)
    assert res["cons"].all() and res["iterations"] == 0 and res["converged"]
    assert np.array_equal(res["x"], b * (1 / d))
    # a zero diagonal in a free row: dinv = 0, no NaN, and never a success
    (rp, cols, vals, nc), b = CC.spd_system(257, n_penalty=0, n_elim=0, n_dup=0)
    ri = pcg_ref.row_index(rp)
    vals[(ri == 100) & (cols == 100)] = 0.0
    res = pcg_ref.pcg(rp, cols, vals, b, max_iter=200)
    assert res["dinv"][100] == 0 and not res["cons"][100]
    assert np.isfinite(res["x"]).all() and res["x"][100] == 0 and not res["converged"]


def test_block3_restatement_solves_dense():
    (rp, cols, vals, nc), b, _ = CC.block3_system()
    res = pcg_ref.pcg(rp, cols, vals, b, rtol=1e-14, check_every=1, block3=True)
    xd = np.linalg.solve(O.csr_to_dense(rp, cols, vals, nc), b)
    assert res["converged"] and np.abs(res["x"] - xd).max() <= 1e-11 * np.abs(xd).max()
    point = pcg_ref.pcg(rp, cols, vals, b, rtol=1e-14, check_every=1)
    assert res["iterations"] < point["iterations"]  # the blocks do precondition


# ---- the generators: each case sits on the boundary it was built for
def test_generators_are_deterministic_and_on_their_boundaries():
    a = CC.uniform(513, 16)
    b = CC.uniform(513, 16)
    assert all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3]))
    assert CC.max_segment(CC.uniform(513, 16)[0], 256) == 4096
    assert CC.max_segment(CC.uniform(513, 16, extra=(5, 300))[0], 256) == 4097
    assert CC.max_segment(CC.uniform(513, 32)[0], 256) == 8192
    assert CC.max_segment(CC.uniform(513, 32, extra=(300,))[0], 256) == 8193
    for m in range(4):
        rp = CC.aligned(m, (m + 3) % 4)[0]
        assert rp[256] % 4 == m and rp[-1] % 4 == (m + 3) % 4
    e = CC.empty_cases()
    rp = e["empty_300"][0]
    assert rp[512] == rp[256] and rp[-1] > rp[512]
    assert e["empty_all"][0][-1] == 0 and e["empty_last5"][0][-1] == e["empty_last5"][0][-6]
    assert 4096 < CC.max_segment(CC.skew([100])[0], 256) <= 8192 < CC.max_segment(CC.skew([300, 301])[0], 256)
    g = CC.ghosts()
    assert g[3] == 257 + 40 and (g[1] >= 257).any() and g[1].max() < g[3]
    for length in (1, 3, 15, 16, 17):
        (rp, cols, vals, nc), m = CC.toeplitz(513, CC.toeplitz_offsets(length))
        assert 513 - length <= m < 513 and np.diff(rp).max() == length and cols.min() >= 0 and cols.max() < 513
    for share in (490, 510):
        rp, cols, vals, nc = CC.pattern_share(share)
        lens = np.diff(rp)
        assert set(np.unique(lens)) == {0, 1, 3, 40}
        assert CC.max_segment(rp, 256) + 3 <= 4096 and CC.max_segment(rp, 64) + 3 <= 1024
    for seg in (1021, 1022):
        rp = CC.pattern_seg64(seg)[0]
        assert CC.max_segment(rp, 64) == seg and CC.max_segment(rp, 128) + 3 <= 2048
        assert CC.max_segment(rp, 256) + 3 <= 4096


def test_row_bound_reference():
    """spmv_longdouble against the dense product (duplicates add up)"""
    rp, cols, vals, nc = CC.skew([100])
    x = CC.values(CC.rng_for("x"), nc)
    y, mag = CC.spmv_longdouble(rp, cols, vals, x)
    yd = O.csr_to_dense(rp, cols, vals, nc) @ x
    assert np.all(np.abs(y.astype(np.float64) - yd) <= (np.diff(rp) + 2) * 2.0 ** -53 * mag.astype(np.float64) * 2)
