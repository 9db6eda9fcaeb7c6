"""The cube kernel's unit table (cubes.hip build_cube_units): each workgroup
loads its unit {column x, column y, z0, z1} from a table built once per
structure and plan.  AFEM_CUBES_SCHED=1 cuts the lattice-order list of units
into one contiguous region per XCD by modelled cost and runs each region most
expensive unit first (the lists then differ in length: the shorter ones end in
empty padding records); AFEM_CUBES_SCHED=0 keeps the lattice order and the
equal-count eighths the kernel computed itself before.  Every unit computes
what it computed, so values and RHS are bitwise the same under both plans.
AFEM_CUBES_ZS may be a list of segment lengths ("20/7": repeated up the box),
AFEM_CUBES_BAND=r sorts by cost within bands of r y-rows of units only (both
measurement knobs): bitwise the default too.

Checked here: the table partitions the box (every column and owned node layer
in exactly one record, z ranges inside the owned layers, block i on XCD i & 7
takes that XCD's (i >> 3)-th record of a contiguous region); plan 1 against
plan 0 bitwise, values and RHS, RHS set and add (add = 2 x set), with the
accumulators' NaN fill (AFEM_CUBES_ACC_INIT=nan: finite and equal), for
AFEM_CUBES_ZS in {1, 2, 3, default}; each against the oracle within 1e-12 of
its largest entry, per entry (as test_gpu_cubes_loops.py).

Shapes: n = 15 (three columns per line: a face column, an interior one, a
partial one) with nz in {1, 2, 3, 9}; n = 22, nz = 5 (four columns per line);
n = 6, nz = 2 (one column: with the default segment length one unit, so seven
XCDs get none); n = 15, nz = 9, zs = 2 gives 45 units, no multiple of 8;
z-slabs of n = 15, nz = 7 on 2 and 3 ranks; a natural-lattice arrays mesh and
a random-numbered one (the staged canonical instance)."""
import numpy as np
import pytest

import arcanefem_amd as af
from oracle import oracle as O

pytestmark = pytest.mark.gpu

VAL_TOL = 1e-12
KERNEL_CUBES = 10  # AFEM_KERNEL_CUBES
F = 5.5
KRUN = 7  # rows per x-run of a unit's column (cubes.hip kRun)
DEFAULT_SCHED = 1
ZS = [None, "1", "2", "3"]

_oracle = {}


def _oracle_for(key, mesh):
    """The oracle's system of one (sub)domain, computed once and shared by the
    cases that differ only in the kernel's segment length."""
    if key not in _oracle:
        cells, coords, _ = mesh.download()
        orp, ocols = O.sparsity(mesh.n_nodes, mesh.n_own_nodes, cells)
        ovals, orhs = O.assemble_poisson(mesh.n_own_nodes, cells, coords, orp, ocols, F)
        for a in (orp, ocols, ovals, orhs):
            a.setflags(write=False)
        _oracle[key] = (orp, ocols, ovals, orhs)
    return _oracle[key]


def _system(ctx, mesh):
    bsr = af.BSRFormat(mesh, 1).initialize(True)
    bsr.computeSparsity()
    ls = af.DoFLinearSystem().initialize(ctx, mesh.n_own_nodes, mesh.n_nodes)
    return bsr, ls


def _run(bsr, ls, mode="set"):
    """One cube run into cleared values and a cleared RHS: (values, RHS)."""
    bsr.resetMatrixValues()
    if mode == "add":  # onto the set run's RHS: 2 x set
        bsr.assemblePoissonP1(1.0, F, ls.rhsVariable(), rhs_mode="set")
        bsr.resetMatrixValues()
    bsr.assemblePoissonP1(1.0, F, ls.rhsVariable(), rhs_mode=mode)
    assert bsr.stats()["last_kernel"] == KERNEL_CUBES
    return bsr.download()[2], ls.rhs_host()


def _check_oracle(bsr, vals, rhs, ref):
    orp, ocols, ovals, orhs = ref
    rows, cols, _ = bsr.download()
    assert np.array_equal(rows, orp) and np.array_equal(cols, ocols)
    verr = np.abs(vals - ovals).max() / np.abs(ovals).max()
    rerr = np.abs(rhs - orhs).max() / np.abs(orhs).max()
    print(f"values {verr:.3e} rhs {rerr:.3e}")
    assert verr <= VAL_TOL, f"CSR values differ from the oracle: {verr:.3e}"
    assert rerr <= VAL_TOL, f"RHS differs from the oracle: {rerr:.3e}"


def _same(a, b, what):
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all(), f"{what}: not finite"
    assert np.array_equal(a[0], b[0]), f"{what}: values differ"
    assert np.array_equal(a[1], b[1]), f"{what}: RHS differs"


def _check_table(ctx, bsr, sched, npx, npy, k0, k1, zs):
    """The table of the last launch: a partition of the columns x owned layers."""
    st = bsr.stats()
    t = bsr.cube_unit_table(ctx).astype(np.int64)
    assert st["cube_sched"] == sched, st
    assert len(t) == st["cube_unit_records"] and len(t) > 0
    tx, ty = (npx + KRUN - 1) // KRUN, (npy + KRUN - 1) // KRUN
    # the segments' first layers and k1 (cubes.hip assemble_cubes: the lengths of AFEM_CUBES_ZS, repeated)
    pat = [int(x) for x in zs.split("/")] if zs else [min(48, max(8, max(npx, npy) // 16))]
    cuts = [k0]
    while cuts[-1] < k1:
        cuts.append(min(cuts[-1] + pat[(len(cuts) - 1) % len(pat)], k1))
    cuts = np.array(cuts)
    ns = len(cuts) - 1
    cx, cy, z0, z1 = t.T
    real = z1 > z0
    assert (z1 >= z0).all() and (z0 >= k0).all() and (z1 <= k1).all()
    assert (cx >= 0).all() and (cx < tx).all() and (cy >= 0).all() and (cy < ty).all()
    assert real.sum() == st["cube_units"] == tx * ty * ns, (real.sum(), st["cube_units"], tx * ty * ns)
    cover = np.zeros((tx, ty, k1 - k0), dtype=np.int64)
    for r in t[real]:
        cover[r[0], r[1], r[2] - k0:r[3] - k0] += 1
    assert (cover == 1).all(), "the records do not partition the columns x owned layers"
    seg = np.searchsorted(cuts, z0)
    assert ((cuts[np.minimum(seg, ns)] == z0) & (seg < ns))[real].all()
    assert (z1 == cuts[np.minimum(seg + 1, ns)])[real].all()
    # the units' lattice-order index; XCD x = the records bid & 7 == x
    u = cx + tx * (cy + ty * seg)
    bid = np.arange(len(t))
    assert st["cube_xcd_cost_spread"] >= 1.0
    if sched == 0:  # the mapping the kernel computed itself: no padding, equal-count eighths in lattice order
        n_units = tx * ty * ns
        assert len(t) == n_units
        qq, rem = n_units >> 3, n_units & 7
        xc, jj = bid & 7, bid >> 3
        assert np.array_equal(u, xc * qq + np.minimum(xc, rem) + jj)
        return st
    assert len(t) % 8 == 0
    nxt = 0
    longest = 0
    for x in range(8):
        m = (bid & 7) == x
        rx = real[m]
        cnt = int(rx.sum())
        assert rx[:cnt].all(), f"XCD {x}: a padding record before its last unit"
        longest = max(longest, cnt)
        ux = np.sort(u[m][rx])
        # a contiguous run of the lattice order, the runs in the order of the XCDs
        assert np.array_equal(ux, nxt + np.arange(cnt)), f"XCD {x}: not a contiguous region"
        nxt += cnt
    assert nxt == tx * ty * ns and len(t) == 8 * longest
    return st


def _both_plans(ctx, variant, bsr, ls, ref, what, dims, zs):
    """Plan 1 against the oracle; plan 0, RHS add (2 x set) under both plans,
    and all of these with the NaN fill: bitwise plan 1's set run.  The table of
    each plan checked after its first launch."""
    variant("AFEM_CUBES_SCHED", "1")
    new = _run(bsr, ls)
    _check_table(ctx, bsr, 1, *dims, zs)
    if ref is not None:
        _check_oracle(bsr, new[0], new[1], ref)
    twice = (new[0], new[1] + new[1])
    for sched in (0, 1):
        variant("AFEM_CUBES_SCHED", str(sched))
        for fill in (None, "nan"):
            variant("AFEM_CUBES_ACC_INIT", fill)
            _same(_run(bsr, ls), new, f"{what}: sched {sched} fill {fill} set")
            _same(_run(bsr, ls, "add"), twice, f"{what}: sched {sched} fill {fill} add")
        if sched == 0:
            _check_table(ctx, bsr, 0, *dims, zs)
    variant("AFEM_CUBES_ACC_INIT", None)
    variant("AFEM_CUBES_SCHED", None)
    _same(_run(bsr, ls), new, f"{what}: the default")
    assert bsr.stats()["cube_sched"] == DEFAULT_SCHED
    return new


@pytest.mark.parametrize("zs", ZS)
@pytest.mark.parametrize("n,nz", [(15, 1), (15, 2), (15, 3), (15, 9), (22, 5), (6, 2)])
def test_schedule_boxes(ctx, variant, n, nz, zs):
    variant("AFEM_CUBES_ZS", zs)
    mesh = af.Mesh.structured(ctx, 3, n, nz, jitter=0.2, seed=31)
    bsr, ls = _system(ctx, mesh)
    _both_plans(ctx, variant, bsr, ls, _oracle_for(("box", n, nz), mesh), f"box {n} x {nz}, zs {zs}",
                (n + 1, n + 1, 0, nz + 1), zs)
    if (n, nz, zs) == (15, 9, "2"):
        assert bsr.stats()["cube_units"] == 45  # no multiple of 8
    if (n, nz, zs) == (6, 2, None):
        assert bsr.stats()["cube_units"] == 1  # seven XCDs without a unit
    mesh.close()


@pytest.mark.parametrize("n,nz", [(15, 9), (22, 5)])
def test_schedule_graded_segments_and_bands(ctx, variant, n, nz):
    """Segments of unequal lengths (AFEM_CUBES_ZS a list, repeated up the box)
    and the cost order within bands of y-rows only (AFEM_CUBES_BAND): other
    partitions of the same box, other orders of the same units -- bitwise the
    uniform default's values and RHS under both plans."""
    mesh = af.Mesh.structured(ctx, 3, n, nz, jitter=0.2, seed=31)
    bsr, ls = _system(ctx, mesh)
    ref = _oracle_for(("box", n, nz), mesh)
    dims = (n + 1, n + 1, 0, nz + 1)
    uniform = _run(bsr, ls)
    for zs, band in (("2/1", None), ("3/1/2", None), ("1/4", "1"), (None, "1"), ("2", "2")):
        variant("AFEM_CUBES_ZS", zs)
        variant("AFEM_CUBES_BAND", band)
        _same(_both_plans(ctx, variant, bsr, ls, ref, f"box {n} x {nz}, zs {zs}, band {band}", dims, zs), uniform,
              f"zs {zs}, band {band} against the uniform default")
    mesh.close()


@pytest.mark.parametrize("zs", ZS)
@pytest.mark.parametrize("nranks", [2, 3])
def test_schedule_slabs(ctx, variant, nranks, zs):
    """z-slabs of one box: the table covers the rank's owned layers [k0, k1)."""
    variant("AFEM_CUBES_ZS", zs)
    n, nz = 15, 7
    L = (n + 1) * (n + 1)
    for rank in range(nranks):
        mesh = af.Mesh.structured(ctx, 3, n, nz=nz, jitter=0.2, seed=13, nranks=nranks, rank=rank)
        spec = O.structured_mesh(3, n, nz=nz, nranks=nranks, rank=rank)
        own = spec["local_to_global"][:spec["n_own"]]
        k0, k1 = int(own.min() // L), int(own.max() // L) + 1
        assert (k1 - k0) * L == mesh.n_own_nodes
        bsr, ls = _system(ctx, mesh)
        _both_plans(ctx, variant, bsr, ls, _oracle_for(("slab", nranks, rank), mesh),
                    f"slab {rank} of {nranks}, zs {zs}", (n + 1, n + 1, k0, k1), zs)
        mesh.close()


@pytest.mark.parametrize("zs", ZS)
@pytest.mark.parametrize("numbering", ["natural", "random"])
def test_schedule_array_lattices(ctx, variant, numbering, zs):
    """Lattices handed over as arrays, in their own lexicographic numbering
    (cube_lattice 2: the box instance) and in a random one (cube_lattice 3:
    the staged canonical instance): the same table, the same checks."""
    variant("AFEM_CUBES_ZS", zs)
    n = nz = 15  # a cube: the lattice's node counts are the same in whatever axis order it is recovered
    m0 = af.Mesh.structured(ctx, 3, n, nz=nz, jitter=0.2, seed=5)
    cells, coords, _ = m0.download()
    m0.close()
    rng = np.random.default_rng(5)
    if numbering == "random":
        p = rng.permutation(coords.shape[0])
        cells = p[cells].astype(np.int32)
        pc = np.empty_like(coords)
        pc[p] = coords
        coords = pc
    cells = np.ascontiguousarray(cells[rng.permutation(cells.shape[0])])
    m1 = af.Mesh.from_arrays(ctx, 3, cells, coords)
    b1, l1 = _system(ctx, m1)
    assert b1.stats()["cube_lattice"] == (2 if numbering == "natural" else 3), b1.stats()
    _both_plans(ctx, variant, b1, l1, _oracle_for(("arrays", numbering), m1), f"{numbering} arrays, zs {zs}",
                (n + 1, n + 1, 0, nz + 1), zs)
    m1.close()
