"""GPU: the SpMV kernels and their planner, the PCG iteration and the dense
direct solver of arcanefem_amd/csrc/linear_system.hip on CSR systems that no
mesh produces (tests/csr_cases.py), each held to a plain high-precision
restatement.

Part A, the product.  Every case asserts the plan it was built to reach
(DoFLinearSystem.spmvPlanInfo, the planner ls.spmv itself runs), then compares
ls.spmv with a np.longdouble row-by-row product under the bound that holds for
any summation order, with or without FMA:

    |y_r - yhat_r| <= (L_r + 2) 2^-53 sum_k |a_rk x_k|,   L_r the row length

(L_r products rounded once each, L_r - 1 additions; one more unit for the
rounding of the longdouble reference to fp64).  An empty row gives exactly 0.0
in a y pre-filled with NaN.  The bitwise claims of the kernels' comments are
assertions: pattern == stream at equal block size, stream blocks of 64 / 128
== 256, s4 == the unrolled kernel.

Part B, the iteration, against tests/pcg_ref.py (pinned on the CPU by
tests/test_pcg_ref.py).  Part C, the direct solver, by its backward error
against LAPACK's on the same matrix.
"""
from fractions import Fraction

import numpy as np
import pytest

import arcanefem_amd as af
import csr_cases as CC
import pcg_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SPMV_OTHER = 4  # AFEM_SPMV_OTHER (include/arcanefem_amd.h): row-per-thread / no-unroll variants, direct solver

MODES = {
    "default": {},
    "nopat": {"AFEM_SPMV": "nopat"},
    "stream": {"AFEM_SPMV": "stream"},
    "s4": {"AFEM_SPMV": "s4"},
    "v16": {"AFEM_SPMV": "v16"},
    "sbs64": {"AFEM_SPMV_STREAM_BS": 64},
    "sbs128": {"AFEM_SPMV_STREAM_BS": 128},
    "bs64": {"AFEM_SPMV_BS": 64},
    "bs128": {"AFEM_SPMV_BS": 128},
    "bs256": {"AFEM_SPMV_BS": 256},
}


def expected_plan(rp, mode, pat=None, aligned=True):
    """plan_spmv_ls restated for a scalar system.  pat = (offsets of the pattern, rows that match)."""
    n = rp.size - 1
    ceil = lambda a, b: -(-a // b)  # noqa: E731
    kind = mode.get("AFEM_SPMV")
    hm = CC.max_segment(rp, 256)
    if kind == "v16":
        return dict(rpb=-1, nblocks=ceil(n, 64))
    if hm > 8192:
        return dict(rpb=-1, nblocks=ceil(n, 64)) if kind in (None, "nopat") else dict(rpb=0, nblocks=ceil(n, 256))
    wide = aligned and kind != "stream"
    unroll = kind in (None, "nopat")
    p = dict(rpb=256, wide=wide, unroll=unroll, bs=256, max_seg=hm, nblocks=ceil(n, 256), pat_len=0, pat_rows=0)
    sbs = mode.get("AFEM_SPMV_STREAM_BS")
    if unroll and wide and sbs in (64, 128):
        p.update(bs=sbs, max_seg=CC.max_segment(rp, sbs), nblocks=ceil(n, sbs))
    if kind is None and pat and n > 64 and wide and hm + 3 <= 4096 and 2 * pat[1] >= n:
        p.update(rpb=-3, pat_len=pat[0], pat_rows=pat[1], bs=256, max_seg=hm, nblocks=ceil(n, 256))
        bs = mode.get("AFEM_SPMV_BS", 64)
        if bs in (64, 128) and CC.max_segment(rp, bs) + 3 <= 16 * bs:
            p.update(bs=bs, max_seg=CC.max_segment(rp, bs), nblocks=ceil(n, bs))
    return p


def kernel_of(p):
    if p["rpb"] == -3:
        return f"k_spmv_pat<{p['bs']}>"
    if p["rpb"] == -2:
        return f"k_spmv_blk<{p['blk_k']}>"
    if p["rpb"] == -1:
        return "k_spmv_v16"
    if p["rpb"] == 0:
        return "k_spmv_row"
    if p["wide"] and p["unroll"]:
        return f"k_spmv_stream4u<{p['bs']}>" + (" tail" if p["max_seg"] > 16 * p["bs"] else "")
    return "k_spmv_stream4" + (" tail" if p["max_seg"] > 1024 else "") if p["wide"] else "k_spmv_stream"


class Device:
    """device arrays that live as long as the test"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.ptrs = []

    def put(self, a, offset=0):
        a = np.ascontiguousarray(a)
        d = self.ctx.malloc(a.nbytes + offset + 16)
        self.ptrs.append(d)
        assert d % 16 == 0
        self.ctx.to_device(d + offset, a)
        return d + offset

    def close(self):
        for d in self.ptrs:
            self.ctx.free(d)
        self.ptrs = []


@pytest.fixture
def dev(ctx):
    d = Device(ctx)
    yield d
    d.close()


def make_ls(ctx, sysm):
    rp, cols, vals, nc = sysm
    ls = af.DoFLinearSystem().initialize(ctx, rp.size - 1, nc)
    rows, rnc = CC.rows_of(rp)
    ls.setCSRValues(rows, rnc, cols, vals.copy())
    return ls


def run_spmv(ctx, dev, ls, x, n):
    dx = dev.put(x)
    dy = dev.put(np.full(n, np.nan))
    ls.spmv(dx, dy)
    return ctx.to_host(dy, n, np.float64)


def check_product(y, sysm, x, what):
    rp, cols, vals, nc = sysm
    ref, mag = CC.spmv_longdouble(rp, cols, vals, x)
    lens = np.diff(rp)
    assert np.isfinite(y).all(), what
    assert np.all(y[lens == 0] == 0.0), f"{what}: an empty row is not exactly 0"
    err = np.abs(y.astype(np.longdouble) - ref)
    bound = (lens + 2) * np.longdouble(U) * mag
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, f"{what}: rows {bad[:8]} err {err[bad[:8]]} bound {bound[bad[:8]]}"


def product_in_modes(ctx, dev, variant, sysm, modes, pat=None, kernel=None):
    """Every mode: the plan (restated planner), the product (row bound); returns {mode: (plan, y)}."""
    rp, cols, vals, nc = sysm
    n = rp.size - 1
    x = CC.values(CC.rng_for("x"), nc)
    ls = make_ls(ctx, sysm)
    out = {}
    try:
        for m in modes:
            for k, v in MODES[m].items():
                variant(k, v)
            plan = ls.spmvPlanInfo()
            exp = expected_plan(rp, MODES[m], pat, aligned=cols.size > 0)
            assert {k: plan[k] for k in exp} == exp, f"{m}: planned {plan}, expected {exp}"
            if m == "default" and kernel:
                assert kernel_of(plan) == kernel, f"planned {plan}"
            y = run_spmv(ctx, dev, ls, x, n)
            check_product(y, sysm, x, f"{m} ({kernel_of(plan)})")
            out[m] = (plan, y)
            for k in MODES[m]:
                variant(k, None)
    finally:
        ls.reset()
    return out


def assert_bitwise_claims(out):
    """stream blocks of 64 / 128 == 256, s4 == the unrolled kernel; pattern == stream at equal block size"""
    base = out["nopat"][1]
    for m in ("sbs64", "sbs128", "s4"):
        if m in out and out["nopat"][0]["rpb"] == 256 and out[m][0]["rpb"] == 256:
            assert np.array_equal(out[m][1], base), f"{m} differs from nopat bitwise"
    for m in ("default", "bs64", "bs128", "bs256"):
        if m in out and out[m][0]["rpb"] == -3:
            assert np.array_equal(out[m][1], base), f"pattern ({m}) differs from the stream kernel bitwise"


ALL_MODES = list(MODES)

# name: (system, the kernel the default plan must be, pattern or None)
_E = CC.empty_cases()
PRODUCT_CASES = {
    **{f"rows{n}": (lambda n=n: CC.random_rows(n, lo=int(n == 1)), "k_spmv_stream4u<256>", None) for n in CC.ROW_COUNTS},
    # 256-row segments of 4096 (exactly the unrolled pass), 4097 (one group in the tail loop of
    # k_spmv_stream4u, and of k_spmv_stream4 under s4), 8192 (the 64 KiB LDS limit)
    "seg4096": (lambda: CC.uniform(513, 16), "k_spmv_stream4u<256>", None),
    "seg4097": (lambda: CC.uniform(513, 16, extra=(5, 300)), "k_spmv_stream4u<256> tail", None),
    "seg8192": (lambda: CC.uniform(513, 32), "k_spmv_stream4u<256> tail", None),
    # 8193: k_spmv_v16 by default, k_spmv_row under stream and s4
    "seg8193": (lambda: CC.uniform(513, 32, extra=(300,)), "k_spmv_v16", None),
    **{f"align{m}{(m + 3) % 4}": (lambda m=m: CC.aligned(m, (m + 3) % 4), "k_spmv_stream4u<256>", None)
       for m in range(4)},
    **{k: (lambda k=k: _E[k], "k_spmv_stream" if k == "empty_all" else "k_spmv_stream4u<256>", None) for k in _E},
    # one row of 5000 entries (duplicate columns): the tail loop by default, the long-row loop of
    # k_spmv_v16 under v16; two such rows in one block (10 000 > 8192): k_spmv_v16 with long rows by
    # default, k_spmv_row under stream / s4
    "skew": (lambda: CC.skew([100]), "k_spmv_stream4u<256> tail", None),
    "skew2": (lambda: CC.skew([300, 301]), "k_spmv_v16", None),
    "ghosts": (lambda: CC.ghosts(), "k_spmv_stream4u<256>", None),
}


@pytest.mark.parametrize("case", list(PRODUCT_CASES))
def test_product(ctx, dev, variant, case):
    """k_spmv_stream4u (with and without its tail loop, 256 / 128 / 64-row blocks), k_spmv_stream4
    (and its tail loop), k_spmv_stream (non-wide: AFEM_SPMV=stream), k_spmv_row (segments over 64 KiB
    in a diagnostic mode) and k_spmv_v16 with long rows, on random CSR systems: every row count
    around 64 / 256, segments on the 4096 / 8192 boundaries, segment starts and nnz at every residue
    mod 4, empty rows (first, scattered, a whole block, the last, the last 5, every row), one very
    long row, ghost columns."""
    build, kernel, pat = PRODUCT_CASES[case]
    sysm = build()
    out = product_in_modes(ctx, dev, variant, sysm, ALL_MODES, pat, kernel)
    assert_bitwise_claims(out)
    if case in ("seg8193", "skew2"):
        assert kernel_of(out["stream"][0]) == "k_spmv_row" and kernel_of(out["s4"][0]) == "k_spmv_row"
    if case == "seg4097":
        assert kernel_of(out["s4"][0]) == "k_spmv_stream4 tail" and kernel_of(out["stream"][0]) == "k_spmv_stream"


PATTERN_LENGTHS = [1, 3, 15, 16, 17]


@pytest.mark.parametrize("length", PATTERN_LENGTHS)
def test_pattern_product(ctx, dev, variant, length):
    """k_spmv_pat at bs 64 / 128 / 256: Toeplitz rows of 1, 3, 15 and 16 offsets (negative and
    positive: the first and last rows are clipped and do not match) plan the pattern kernel, 17
    offsets do not (k_spmv_stream4u tail).  16 offsets: 256 full rows are 4096 non-zeros, over the
    planner's max_seg + 3 <= 4096, so row 300 is given one entry; its 64- and 128-row blocks (1024
    / 2048 non-zeros) decline, the pattern runs in 256-row blocks."""
    sysm, matching = CC.toeplitz(513, CC.toeplitz_offsets(length), {300: 1} if length == 16 else None)
    pat = (length, matching) if length <= 16 else None
    kernel = "k_spmv_stream4u<256> tail" if not pat else "k_spmv_pat<256>" if length == 16 else "k_spmv_pat<64>"
    out = product_in_modes(ctx, dev, variant, sysm, ALL_MODES, pat, kernel)
    assert_bitwise_claims(out)
    if pat:
        want = [256, 256, 256] if length == 16 else [64, 128, 256]
        assert [out[m][0]["bs"] for m in ("bs64", "bs128", "bs256")] == want
        assert out["sbs64"][0]["rpb"] == -3 and out["sbs64"][0]["bs"] == want[0]


@pytest.mark.parametrize("n_match,kernel", [(490, "k_spmv_stream4u<256>"), (510, "k_spmv_pat<64>")])
def test_pattern_share_gate(ctx, dev, variant, n_match, kernel):
    """The hc * 2 >= n_rows gate of the pattern kernel: 49 % matching rows keep k_spmv_stream4u, 51 %
    plan k_spmv_pat; the other rows have lengths 0, 1 and 40."""
    sysm = CC.pattern_share(n_match)
    out = product_in_modes(ctx, dev, variant, sysm, ALL_MODES, (3, n_match), kernel)
    assert_bitwise_claims(out)


@pytest.mark.parametrize("seg", [1021, 1022])
def test_pattern_block_size_fallback(ctx, dev, variant, seg):
    """k_spmv_pat's block size: a largest 64-row segment of 1021 is accepted (hm + 3 <= 1024), 1022
    falls back to 256-row blocks; 128-row blocks take both.  Under AFEM_SPMV_STREAM_BS=64 the pattern
    plan is the same (the stream kernel's knob does not reach the pattern kernel)."""
    sysm = CC.pattern_seg64(seg)
    (rp, cols, vals, nc) = sysm
    ri = pcg_ref.row_index(rp)
    off = cols.astype(np.int64) - ri
    full = np.array([np.array_equal(off[rp[r]:rp[r + 1]], np.arange(-7, 8)) for r in range(rp.size - 1)])
    out = product_in_modes(ctx, dev, variant, sysm, ALL_MODES, (15, int(full.sum())),
                           "k_spmv_pat<64>" if seg == 1021 else "k_spmv_pat<256>")
    assert_bitwise_claims(out)
    assert out["bs128"][0]["bs"] == 128 and out["bs256"][0]["bs"] == 256
    assert out["bs64"][0]["bs"] == (64 if seg == 1021 else 256)
    assert out["sbs64"][0]["bs"] == (64 if seg == 1021 else 256) and out["sbs64"][0]["rpb"] == -3


def test_unaligned_device_view(ctx, dev, variant):
    """k_spmv_stream (non-wide) by default: a device view whose columns start 4 B and whose values
    start 8 B past a 16-B aligned allocation (setCSRValuesDevice) must plan wide = 0; the same
    matrix aligned plans k_spmv_stream4u and gives the same bits."""
    sysm = CC.uniform(513, 16, extra=(5, 300))
    rp, cols, vals, nc = sysm
    n = rp.size - 1
    x = CC.values(CC.rng_for("x"), nc)
    ys = {}
    for name, oc, ov in (("unaligned", 4, 8), ("aligned", 0, 0)):
        ls = af.DoFLinearSystem().initialize(ctx, n, nc)
        dc, dv = dev.put(cols, oc), dev.put(vals, ov)
        ls.setCSRValuesDevice(CC.rows_of(rp)[0], dc, dv, n, cols.size)
        plan = ls.spmvPlanInfo()
        assert plan["wide"] == (name == "aligned") and plan["rpb"] == 256, plan
        assert kernel_of(plan) == ("k_spmv_stream" if name == "unaligned" else "k_spmv_stream4u<256> tail")
        ys[name] = run_spmv(ctx, dev, ls, x, n)
        check_product(ys[name], sysm, x, name)
        ls.reset()
    assert np.array_equal(ys["unaligned"], ys["aligned"])


# ---- block systems: k_spmv_blk<2> / <3> with more than 16 blocks in a node row
def fan2d():
    """20 triangles about vertex 0: 21 nodes (odd: the kBlkRpg = 2 tail), node 0 has 21 blocks"""
    a = 2 * np.pi * np.arange(20) / 20
    coords = np.zeros((21, 3))
    coords[1:, 0], coords[1:, 1] = np.cos(a), np.sin(a)
    cells = np.array([[0, 1 + i, 1 + (i + 1) % 20] for i in range(20)], dtype=np.int32)
    return 2, cells, coords


def cone3d():
    """A fanned disc of 18 rim vertices about node 0 with an apex above (node 19) and, for an odd
    node count (21: the kBlkRpg = 2 tail), one below (node 20): node 0 has 21 blocks"""
    a = 2 * np.pi * np.arange(18) / 18
    coords = np.zeros((21, 3))
    coords[1:19, 0], coords[1:19, 1] = np.cos(a), np.sin(a)
    coords[19, 2], coords[20, 2] = 1.0, -1.0
    up = [[0, 1 + i, 1 + (i + 1) % 18, 19] for i in range(18)]
    down = [[0, 1 + (i + 1) % 18, 1 + i, 20] for i in range(18)]
    return 3, np.array(up + down, dtype=np.int32), coords


def block_system(ctx, dim, cells, coords):
    """Elasticity on the mesh (the BSR origin the block kernels need); returns mesh, bsr, ls and the
    scalar CSR of the assembled matrix in the device's value order"""
    mesh = af.Mesh.from_arrays(ctx, dim, cells, coords)
    bsr = af.BSRFormat(mesh, dim).initialize(True)
    bsr.computeSparsity()
    bsr.assembleElasticityP1Ex(1.3, 0.9)
    rows, rnc, cols, vals = bsr.export_csr32()
    ls = af.DoFLinearSystem().initialize(ctx, dim * mesh.n_own_nodes)
    rp = np.concatenate([rows.astype(np.int64), [cols.size]])
    return mesh, bsr, ls, (rp, cols, vals, dim * mesh.n_nodes)


@pytest.mark.parametrize("mesh_fn", [fan2d, cone3d])
def test_block_product(ctx, dev, variant, mesh_fn):
    """k_spmv_blk<2> (fan of 20 triangles) and k_spmv_blk<3> (cone over a disc of 18 rim vertices):
    21 nodes, the centre node's row holds 21 > 16 blocks (the t = l16 + 16 loop).  The assembled
    values are overwritten with random ones through the BSR view, so a transposed block shows; the
    diagnostic modes run the scalar kernels on the same CSR."""
    dim, cells, coords = mesh_fn()
    mesh, bsr, ls, (rp, cols, vals, nc) = block_system(ctx, dim, cells, coords)
    try:
        v = bsr.view()
        assert v.block_size == dim and v.nnz_blocks * dim * dim == vals.size
        bp = ctx.to_host(v.rows, v.n_block_rows + 1, np.int64)
        assert np.diff(bp).max() == 21 and v.n_block_rows == 21
        assert np.array_equal(ctx.to_host(v.values, vals.size, np.float64), vals)  # the CSR is the device order
        new = CC.values(CC.rng_for(mesh_fn.__name__), vals.size)
        ctx.to_device(v.values, new)
        bsr.toLinearSystem(ls)
        sysm = (rp, cols, new, nc)
        x = CC.values(CC.rng_for("x"), nc)
        n = rp.size - 1
        for m in ("default", "nopat", "stream", "s4", "v16"):
            for k, val in MODES[m].items():
                variant(k, val)
            plan = ls.spmvPlanInfo()
            if m == "default":
                assert plan["rpb"] == -2 and plan["blk_k"] == dim and plan["nblocks"] == 1, plan
                assert kernel_of(plan) == f"k_spmv_blk<{dim}>"
            else:
                exp = expected_plan(rp, MODES[m])  # the scalar kernels on the same CSR
                assert (plan["rpb"], plan["nblocks"]) == (exp["rpb"], exp["nblocks"]), f"{m}: {plan}"
            check_product(run_spmv(ctx, dev, ls, x, n), sysm, x, f"{mesh_fn.__name__} {m}")
            for k in MODES[m]:
                variant(k, None)
    finally:
        ls.reset()
        bsr.close()
        mesh.close()


# ---------------------------------------------------------------- part B: the iteration
def gpu_solve(ctx, sysm, b, **opts):
    ls = make_ls(ctx, sysm)
    try:
        ctx.to_device(ls.rhsVariable(), b)
        ls.setSolverOptions(method="pcg", **opts)
        st = ls.solve()
        return ls.solution_host(), st
    finally:
        ls.reset()


_REF = {}


def reference(key, sysm, b, **kw):
    """The longdouble restatement and the distance of the float64 one from it, over 3 random
    orderings of its dot-product sums (computed once per system and k).  Returns (ref, d_x, d_rel):
    d_x = max |x64 - xld| over the orderings, floored at 2^-53 max |x| (below that the float64
    result cannot resolve a difference at all), d_rel likewise for rel_residual."""
    if key in _REF:
        return _REF[key]
    rp, cols, vals, nc = sysm
    ld = pcg_ref.pcg(rp, cols, vals, b, n_cols=nc, dtype=np.longdouble, **kw)
    xl = ld["x"]
    dx, drel = 0.0, 0.0
    for s in range(3):
        perm = np.random.default_rng(s).permutation(rp.size - 1)

        def dot(u, v, perm=perm):
            w = u * v
            return w[perm[perm < w.size] if w.size < perm.size else perm].sum()

        f = pcg_ref.pcg(rp, cols, vals, b, n_cols=nc, dot=dot, **kw)
        dx = max(dx, float(np.abs(f["x"] - xl).max()))
        drel = max(drel, abs(f["rel_residual"] - ld["rel_residual"]))
        assert f["iterations"] == ld["iterations"] and f["converged"] == ld["converged"]
    dx = max(dx, U * float(np.abs(xl).max()))
    drel = max(drel, U * ld["rel_residual"])
    _REF[key] = (ld, dx, drel)
    return _REF[key]


PCG_SIZES = [1, 2, 257, 1000, 1001]


@pytest.mark.parametrize("n", PCG_SIZES)
def test_pcg_fixed_iterations(ctx, variant, n):
    """k_inv_diag, k_cg_x0, k_cg_init, k_cg_update_rz / k_cg_dir_x (scalar, V2 and V2 + U2 forms,
    the n & 1 tail at n = 1, 257, 1001) after exactly k = 1, 2, 7 steps on symmetric, diagonally
    dominant random systems with penalty rows, row-eliminated rows and duplicate diagonal entries.
    x is held to the longdouble restatement within 8 x the float64 restatement's own distance from
    it (3 orderings of the dot products); measured on the CPU, relative to max |x|:
    n = 1: the 2^-53 floor; n = 257: 4.3e-12 (k = 1), 8.9e-15 (k = 7) -- the 1e30 penalty rows leave
    1e30 * 2^-53 of rounding in r0, which r.z sees; n = 1001: 2.9e-16 (k = 1), 2.1e-16 (k = 7).  The
    GPU's own distance was 1/8 to 1/5 of what is allowed in every case.
    AFEM_CG_VEC2 unset and = 2 group the partial sums alike (one trip: the second access of U2 is
    empty): bitwise equal; = 0 groups them differently: the tolerance."""
    sysm, b = CC.spd_system(n)
    for k in (1, 2, 7):
        ld, dx, _ = reference(("spd", n, k), sysm, b, fixed_iterations=k)
        xs = {}
        for v2 in (None, 0, 2):
            variant("AFEM_CG_VEC2", v2)
            x, st = gpu_solve(ctx, sysm, b, fixed_iterations=k)
            variant("AFEM_CG_VEC2", None)
            assert st["iterations"] == k
            err = float(np.abs(x.astype(np.longdouble) - ld["x"]).max())
            print(f"n={n} k={k} VEC2={v2}: err {err:.3e} allowed {8 * dx:.3e}")
            assert err <= 8 * dx, f"n={n} k={k} VEC2={v2}: {err:.3e} > {8 * dx:.3e}"
            xs[v2] = x
        assert np.array_equal(xs[None], xs[2])
        # the row-eliminated rows keep their value exactly
        ident = ld["cons"] & (ld["dinv"] == 1)
        assert np.array_equal(xs[None][ident], b[ident])


def test_pcg_second_grid_stride_trip(ctx, variant):
    """n = 2 * 524288 + 257 rows (3 .. 5 non-zeros per row): the vector kernels' grid of 2048 x 256
    threads takes a second trip (V2: 128 threads; U2: its `two` arm is false for every thread past
    the first 128; scalar: every thread twice, 257 thrice) and the odd n leaves the n & 1 tail.
    Tolerance as test_pcg_fixed_iterations; measured 6.0e-16 (k = 1), 3.3e-16 (k = 7) of max |x|, the
    GPU at 1/12 .. 1/8 of what is allowed.  VEC2 unset and
    = 2 visit a thread's rows in the same order: bitwise equal."""
    n = 2 * 524288 + 257
    sysm, b = CC.banded_spd(n)
    for k in (1, 7):
        ld, dx, _ = reference(("band", n, k), sysm, b, fixed_iterations=k)
        xs = {}
        for v2 in (None, 0, 2):
            variant("AFEM_CG_VEC2", v2)
            x, st = gpu_solve(ctx, sysm, b, fixed_iterations=k)
            variant("AFEM_CG_VEC2", None)
            err = float(np.abs(x.astype(np.longdouble) - ld["x"]).max())
            print(f"k={k} VEC2={v2}: err {err:.3e} allowed {8 * dx:.3e}")
            assert st["iterations"] == k and err <= 8 * dx, f"k={k} VEC2={v2}: {err:.3e} > {8 * dx:.3e}"
            xs[v2] = x
        assert np.array_equal(xs[None], xs[2])


@pytest.mark.parametrize("n", [257, 1000])
def test_pcg_tolerance_stopped_and_graph(ctx, variant, n):
    """iterations, converged and rel_residual of a tolerance-stopped run (rtol 1e-6, tested every 8
    iterations) against the restatement's own values, launched and (AFEM_CG_GRAPH=1) replayed as a
    captured graph: the same kernels, so the same bits.  rel_residual within 8 x the float64
    restatement's distance from the longdouble one (measured: 1.3e-11 of rel_residual at n = 257,
    6.1e-11 at n = 1000; both stop after 16 iterations)."""
    sysm, b = CC.spd_system(n)
    ld, dx, drel = reference(("spd-tol", n), sysm, b, rtol=1e-6, check_every=8)
    assert ld["converged"] and ld["iterations"] % 8 == 0 and ld["iterations"] > 0
    res = {}
    for g in (None, 1):
        variant("AFEM_CG_GRAPH", g)
        x, st = gpu_solve(ctx, sysm, b, rtol=1e-6, check_every=8, max_iter=1000)
        variant("AFEM_CG_GRAPH", None)
        assert st["iterations"] == ld["iterations"] and st["converged"]
        assert abs(st["rel_residual"] - ld["rel_residual"]) <= 8 * drel
        assert float(np.abs(x.astype(np.longdouble) - ld["x"]).max()) <= 8 * dx
        res[g] = x
    assert np.array_equal(res[None], res[1])
    # 16 fixed iterations: one replayed batch of 16
    ld, dx, _ = reference(("spd", n, 16), sysm, b, fixed_iterations=16)
    for g in (None, 1):
        variant("AFEM_CG_GRAPH", g)
        x, st = gpu_solve(ctx, sysm, b, fixed_iterations=16)
        variant("AFEM_CG_GRAPH", None)
        assert st["iterations"] == 16
        assert float(np.abs(x.astype(np.longdouble) - ld["x"]).max()) <= 8 * dx
        res[g] = x
    assert np.array_equal(res[None], res[1])


def test_pcg_degenerate_inputs(ctx):
    """Exact expectations: b = 0; every row a constraint (the stopping reference's fallback); a zero
    diagonal in a free row (dinv = 0: no NaN, never a success); a matrix without entries."""
    sysm, b = CC.spd_system(257)
    x, st = gpu_solve(ctx, sysm, np.zeros(257))
    assert not x.any() and st["iterations"] == 0 and st["converged"]
    n = 65
    d = CC.values(CC.rng_for("diag"), n)
    b = CC.values(CC.rng_for("rhs"), n)
    x, st = gpu_solve(ctx, (np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), d, n), b)
    assert np.array_equal(x, b * (1 / d)) and st["iterations"] == 0 and st["converged"]
    (rp, cols, vals, nc), b = CC.spd_system(257, n_penalty=0, n_elim=0, n_dup=0)
    vals[(pcg_ref.row_index(rp) == 100) & (cols == 100)] = 0.0
    ref = pcg_ref.pcg(rp, cols, vals, b, max_iter=200)
    x, st = gpu_solve(ctx, (rp, cols, vals, nc), b, max_iter=200)
    assert np.isfinite(x).all() and x[100] == 0.0
    assert not st["converged"] and not ref["converged"]
    # nnz == 0: x = 0; converged only for b = 0 (include/arcanefem_amd.h, afem_ls_solve)
    empty = CC.empty_cases()["empty_all"]
    x, st = gpu_solve(ctx, empty, np.ones(65), max_iter=16)
    assert not x.any() and not st["converged"]
    x, st = gpu_solve(ctx, empty, np.zeros(65))
    assert not x.any() and st["converged"] and st["iterations"] == 0


def test_pcg_constraint_threshold(ctx):
    """k_inv_diag's rule |d| > 1e10 sum |off|: a row whose diagonal is 3e9 times its off-diagonal sum
    is a free row (x0 = 0 there, it enters the stopping reference), one at 3e10 is a constraint row
    (lifted into x0).  After 1 and 2 steps x follows the restatement (tolerance as
    test_pcg_fixed_iterations): a row classified the other way starts from another x0."""
    (rp, cols, vals, nc), b = CC.spd_system(257, n_penalty=0, n_elim=0, n_dup=0)
    ri = pcg_ref.row_index(rp)
    off = pcg_ref.row_sums(rp, np.where(cols == ri, 0, np.abs(vals)))
    vals[(ri == 40) & (cols == 40)] = 3e9 * off[40]
    vals[(ri == 90) & (cols == 90)] = 3e10 * off[90]
    b[[40, 90]] *= 1e9
    sysm = (rp, cols, vals, nc)
    for k in (1, 2):
        ld, dx, _ = reference(("threshold", k), sysm, b, fixed_iterations=k)
        assert not ld["cons"][40] and ld["cons"][90] and ld["cons"].sum() == 1
        x, st = gpu_solve(ctx, sysm, b, fixed_iterations=k)
        err = float(np.abs(x.astype(np.longdouble) - ld["x"]).max())
        print(f"threshold k={k}: err {err:.3e} allowed {8 * dx:.3e}")
        assert err <= 8 * dx


def test_pcg_block3(ctx):
    """precond="block3" (k_inv_block3, k_cg_init_b3, k_cg_update_b3) on a random SPD block-3 CSR with
    one and with two penalty rows inside a block, against the restatement with the dense 3 x 3
    inverse of the free sub-block; tolerance as test_pcg_fixed_iterations (measured 3.3e-9 of max
    |x| at k = 1, 7.8e-14 at k = 7: the penalty rows' rounding in r0, as there; the GPU at 1/8)."""
    sysm, b, pen = CC.block3_system()
    for k in (1, 2, 7):
        ld, dx, _ = reference(("b3", k), sysm, b, fixed_iterations=k, block3=True)
        x, st = gpu_solve(ctx, sysm, b, fixed_iterations=k, preconditioner="block3")
        err = float(np.abs(x.astype(np.longdouble) - ld["x"]).max())
        print(f"block3 k={k}: err {err:.3e} allowed {8 * dx:.3e}")
        assert st["iterations"] == k and err <= 8 * dx
    assert ld["cons"][pen].all() and ld["cons"].sum() == pen.size


def test_pcg_block_rows_long(ctx, variant):
    """k_inv_diag_blk<2> / <3> with a node row of 21 > 16 blocks (its second trip) and k_spmv_blk
    with DOT inside the loop: the elasticity fan and cone with penalty rows, 2 fixed iterations,
    against the restatement on the exported CSR; tolerance as test_pcg_fixed_iterations."""
    for mesh_fn in (fan2d, cone3d):
        dim, cells, coords = mesh_fn()
        mesh, bsr, ls, sysm = block_system(ctx, dim, cells, coords)
        try:
            rp, cols, vals, nc = sysm
            n = rp.size - 1
            b = CC.values(CC.rng_for("rhs" + mesh_fn.__name__), n)
            bsr.toLinearSystem(ls)
            ctx.to_device(ls.rhsVariable(), b)
            fixed = np.array([2, 3, 11], dtype=np.int32)
            ls.applyDirichletVectorial(fixed, [0.25] * dim, "penalty", 1e30)
            ls.setSolverOptions(method="pcg", fixed_iterations=2)
            assert ls.spmvPlanInfo()["rpb"] == -2
            st = ls.solve()
            x = ls.solution_host()
            vals = vals.copy()
            ri = pcg_ref.row_index(rp)
            for node in fixed:
                for c in range(dim):
                    d = dim * node + c
                    vals[(ri == d) & (cols == d)] = 1e30
                    b[d] = 1e30 * 0.25
            ld, dx, _ = reference(("blk", mesh_fn.__name__), (rp, cols, vals, nc), b, fixed_iterations=2)
            err = float(np.abs(x.astype(np.longdouble) - ld["x"]).max())
            print(f"{mesh_fn.__name__}: err {err:.3e} allowed {8 * dx:.3e}")
            assert st["iterations"] == 2 and err <= 8 * dx
        finally:
            ls.reset()
            bsr.close()
            mesh.close()


def test_two_stage_reduction(ctx, variant):
    """k_reduce_chunks: n_rows = 64 * 65537 with a tridiagonal pattern system, so the default 64-row
    pattern plan has 65537 > 65536 partials.  3 fixed iterations with AFEM_REDUCE_2STAGE unset and
    = 0, both held to the restatement, and to each other, within the tolerance of
    test_pcg_fixed_iterations (a dropped chunk is 1/128 of p.q).  Measured 5.5e-16 of max |x|; the GPU at 1/16."""
    n = 64 * 65537
    sysm, b = CC.banded_spd(n, offsets=(1,))
    ld, dx, _ = reference(("two-stage",), sysm, b, fixed_iterations=3)
    ls = make_ls(ctx, sysm)
    try:
        plan = ls.spmvPlanInfo()
        assert plan["rpb"] == -3 and plan["bs"] == 64 and plan["nblocks"] == 65537, plan
        ctx.to_device(ls.rhsVariable(), b)
        ls.setSolverOptions(method="pcg", fixed_iterations=3)
        xs = {}
        for two in (None, 0):
            variant("AFEM_REDUCE_2STAGE", two)
            st = ls.solve()
            variant("AFEM_REDUCE_2STAGE", None)
            xs[two] = ls.solution_host()
            err = float(np.abs(xs[two].astype(np.longdouble) - ld["x"]).max())
            print(f"2STAGE={two}: err {err:.3e} allowed {8 * dx:.3e}")
            assert st["iterations"] == 3 and err <= 8 * dx
        assert float(np.abs(xs[None] - xs[0]).max()) <= 8 * dx
    finally:
        ls.reset()


# ---------------------------------------------------------------- part C: the direct solver
def dense_to_csr(A, rng=None, dup=0):
    """CSR of the non-zeros of A; `dup` entries split into two that add up"""
    n = A.shape[0]
    r, c = np.nonzero(A)
    v = A[r, c]
    if dup:
        pick = rng.choice(r.size, dup, replace=False)
        half = v[pick] * 0.375
        v = v.copy()
        v[pick] -= half
        r, c, v = np.concatenate([r, r[pick]]), np.concatenate([c, c[pick]]), np.concatenate([v, half])
        order = np.argsort(r, kind="stable")
        r, c, v = r[order], c[order], v[order]
    rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int64)
    return rp, c.astype(np.int32), v, A.shape[1]


def random_matrix(n, name, density=None):
    """well scaled, non-symmetric, shifted on the diagonal: LAPACK's backward error stays < 1e-13"""
    rng = CC.rng_for(name)
    A = rng.uniform(-1.0, 1.0, (n, n))
    if density:
        A *= rng.random((n, n)) < density
    A[np.arange(n), np.arange(n)] += 0.25 * np.sqrt(n) * rng.choice([-1.0, 1.0], n)
    return A, rng.uniform(-1.0, 1.0, n), rng


def backward_error(A, x, b):
    r = b.astype(np.longdouble) - A.astype(np.longdouble) @ x.astype(np.longdouble)
    return float(np.abs(r).max() / (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()))


def gpu_direct(ctx, sysm, b, method="direct", elim=None):
    ls = make_ls(ctx, sysm)
    try:
        ctx.to_device(ls.rhsVariable(), b)
        for d, g in (elim or {}).items():
            ls.applyDirichletViaRowElimination(np.array([d], dtype=np.int32), g)
        ls.setSolverOptions(method=method, rtol=1e-12)
        st = ls.solve()
        return ls.solution_host(), st
    finally:
        ls.reset()


def check_direct(ctx, A, b, sysm, what, method="direct"):
    """eta = |b - A x|_inf / (|A|_inf |x|_inf + |b|_inf) in longdouble, allowed 16 x max(LAPACK's eta
    on the same matrix, 2^-53); st["rel_residual"] against the same longdouble residual"""
    x, st = gpu_direct(ctx, sysm, b, method)
    eta_l = backward_error(A, np.linalg.solve(A, b), b)
    eta = backward_error(A, x, b)
    print(f"{what}: eta {eta:.3e}, LAPACK {eta_l:.3e}")
    assert eta_l < 1e-13
    assert eta <= 16 * max(eta_l, U), f"{what}: eta {eta:.3e}, LAPACK {eta_l:.3e}"
    assert st["iterations"] == 0 and st["converged"] and st["spmv_kernel"] == SPMV_OTHER
    r = b.astype(np.longdouble) - A.astype(np.longdouble) @ x.astype(np.longdouble)
    rel = float(np.sqrt((r * r).sum() / (b.astype(np.longdouble) ** 2).sum()))
    # the kernel forms r in fp64: |r_i| carries up to (L + 2) 2^-53 sum |a_ij x_j| of its own rounding
    slack = float((A.shape[0] + 2) * U * np.sqrt(((np.abs(A) @ np.abs(x)) ** 2).sum() / (b ** 2).sum()))
    assert abs(st["rel_residual"] - rel) <= slack
    return x, st


@pytest.mark.parametrize("n", [1, 2, 1025, 1100])
def test_direct_solver(ctx, n):
    """k_csr_to_dense + k_dense_gauss under method="direct": n = 1; n = 2 with a zero leading diagonal
    (must swap rows); n = 1025 and 1100, more rows than the kernel's 1024 lanes, non-symmetric.
    Measured eta (LAPACK's in brackets): n = 1: 8.7e-18 (8.7e-18); n = 2: 0 (0); n = 1025: 7.2e-16
    (5.8e-16); n = 1100: 7.4e-16 (4.6e-16)."""
    if n == 2:
        A, b = np.array([[0.0, 2.0], [-3.0, 0.5]]), np.array([1.0, 7.0])
    else:
        A, b, _ = random_matrix(n, f"direct{n}")
    check_direct(ctx, A, b, dense_to_csr(A), f"n={n}")


def test_direct_duplicates_ghosts_sparse(ctx):
    """k_csr_to_dense: duplicate entries add up, ghost columns (>= n_rows) are dropped; a sparse
    non-symmetric matrix of 300 rows.  Measured eta 5.6e-16 (LAPACK 1.9e-16)."""
    n = 300
    A, b, rng = random_matrix(n, "direct-sparse", density=0.05)
    rp, cols, vals, _ = dense_to_csr(A, rng, dup=200)
    # ghost entries: 2 per row at the end of the row, columns in [n, n + 40)
    lens = np.diff(rp)
    gcols = rng.integers(n, n + 40, 2 * n).astype(np.int32)
    gvals = CC.values(rng, 2 * n)
    pos = np.repeat(rp[1:], 2) + np.arange(2 * n)
    cols = np.insert(cols, np.repeat(rp[1:], 2), gcols)
    vals = np.insert(vals, np.repeat(rp[1:], 2), gvals)
    rp = np.concatenate([[0], np.cumsum(lens + 2)]).astype(np.int64)
    assert cols.size == rp[-1] and pos.size == 2 * n and (cols >= n).sum() == 2 * n
    check_direct(ctx, A, b, (rp, cols, vals, n + 40), "duplicates + ghosts")


@pytest.mark.parametrize("n,direct", [(499, True), (500, False)])
def test_auto_threshold(ctx, n, direct):
    """method="auto": the direct solver below 500 rows (0 iterations, AFEM_SPMV_OTHER), the PCG from
    500 on (iterations > 0, a planned SpMV kernel)."""
    sysm, b = CC.spd_system(n, n_penalty=0, n_elim=0)
    rp, cols, vals, nc = sysm
    if direct:
        from oracle import oracle as O

        check_direct(ctx, O.csr_to_dense(rp, cols, vals, nc), b, sysm, f"auto n={n}", method="auto")
    else:
        x, st = gpu_direct(ctx, sysm, b, method="auto")
        assert st["iterations"] > 0 and st["converged"] and st["spmv_kernel"] != SPMV_OTHER


def _round(fr):
    return float(fr)  # Fraction -> nearest double (correctly rounded)


def gauss_lowest_index(A, b, fma, lowest=True):
    """k_dense_gauss restated with every operation rounded as the kernel's: pivot = largest |a_ik|,
    the lowest row index on ties; l = a_ik * (1 / a_kk); a_ij -= l a_kj either contracted to one
    rounding (fma) or as two; column-oriented back substitution."""
    n = A.shape[0]
    a = np.concatenate([A, b[:, None]], axis=1).astype(np.float64)
    F = Fraction

    def mulsub(c, l, u):  # c - l * u
        return _round(F(c) - F(l) * F(u)) if fma else c - l * u

    for k in range(n):
        col = np.abs(a[k:, k])
        m = col.max()
        idx = np.flatnonzero(col == m)
        p = k + (idx[0] if lowest else idx[-1])
        if p != k:
            a[[k, p], k:] = a[[p, k], k:]
        inv = 1.0 / a[k, k]
        for i in range(k + 1, n):
            l = a[i, k] * inv
            for j in range(k + 1, n + 1):
                a[i, j] = mulsub(a[i, j], l, a[k, j])
    x = np.zeros(n)
    for j in range(n - 1, -1, -1):
        x[j] = a[j, n] / a[j, j]
        for i in range(j):
            a[i, n] = mulsub(a[i, n], a[i, j], x[j])
    return x


def test_direct_pivot_ties(ctx):
    """Tied pivot magnitudes: the lowest row index wins, inside a wave (the shuffle reduction) and
    across waves (rows 64 apart).  Entries are multiples of 0.1 in [-0.4, 0.4], so the first columns
    tie many times.  x must equal, bit for bit, the NumPy restatement of the kernel's operations
    with the lowest-index rule -- with the elimination's a - l u either contracted to an FMA or not
    (the compiler's choice) -- and the restatements with the highest-index rule differ from both,
    so a flipped rule cannot pass."""
    n = 70
    rng = CC.rng_for("ties")
    A = rng.integers(-4, 5, (n, n)) * 0.1
    A[np.arange(n), np.arange(n)] = 0.4 * rng.choice([-1.0, 1.0], n)
    b = rng.integers(-9, 10, n) * 0.1
    col0 = np.abs(A[:, 0])
    tied = np.flatnonzero(col0 == col0.max())
    assert tied.size >= 4 and tied[0] < 64 <= tied[-1]
    lo = [gauss_lowest_index(A, b, fma) for fma in (True, False)]
    hi = [gauss_lowest_index(A, b, fma, lowest=False) for fma in (True, False)]
    assert not any(np.array_equal(u, v) for u in lo for v in hi)
    x, st = gpu_direct(ctx, dense_to_csr(A), b)
    assert any(np.array_equal(x, u) for u in lo), \
        f"max diff to the lowest-index restatements {[float(np.abs(x - u).max()) for u in lo]}"


def test_direct_row_eliminated_dof(ctx):
    """A row-eliminated DoF whose column keeps the other rows' entries: k_csr_to_dense moves the
    column to the right-hand side, x_d comes back as the stated value exactly, and the other
    unknowns solve the reduced system (backward error gate of check_direct on it)."""
    n = 40
    A, b, _ = random_matrix(n, "direct-elim")
    d, g = 17, 0.7312
    x, st = gpu_direct(ctx, dense_to_csr(A), b, elim={d: g})
    assert x[d] == g
    keep = np.arange(n) != d
    Ar, br = A[np.ix_(keep, keep)], b[keep] - A[keep, d] * g
    eta_l = backward_error(Ar, np.linalg.solve(Ar, br), br)
    eta = backward_error(Ar, x[keep], br)
    print(f"row-eliminated: eta {eta:.3e}, LAPACK {eta_l:.3e}")
    assert eta_l < 1e-13 and eta <= 16 * max(eta_l, U)


def test_direct_errors(ctx):
    """A singular matrix: AFEM_ERR_ARG with the solver's message; 4097 rows: AFEM_ERR_LIMIT before
    any launch; a matrix without entries is singular."""
    A = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.5, -1.0, 2.0]])
    with pytest.raises(af.AfemError, match="direct solver: the matrix is singular") as e:
        gpu_direct(ctx, dense_to_csr(A), np.ones(3))
    assert e.value.code == 1
    with pytest.raises(af.AfemError, match="direct solver: the matrix is singular"):
        gpu_direct(ctx, CC.empty_cases()["empty_all"], np.ones(65))
    n = 4097
    eye = (np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), np.ones(n), n)
    with pytest.raises(af.AfemError, match="more than 4096 rows") as e:
        gpu_direct(ctx, eye, np.ones(n))
    assert e.value.code == 7
