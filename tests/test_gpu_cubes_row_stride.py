"""The cube kernel's scalar row bases (cubes.hip, AFEM_CUBES_V bit 4096): where
a structure's row offsets grow by one constant from each node layer to the
next (checked on the device when the structure is built; afem_bsr_stats
cube_row_stride, 0 = not so), the complete-layer loop loads no row offsets --
the 7 x-runs' first values are loaded once per unit and advanced by the
constant.  The same stores go to the same places, so values and RHS are
bitwise those of the run without the bit.

Under single writer the accumulators are no longer filled at the kernel's
start; AFEM_CUBES_ACC_INIT=nan still fills them with a quiet NaN.  Every case
runs with it too: finite, bitwise equal outputs show that no flush reads a
slot its own layer cycle did not write.

Shapes: n = 15 has one column of units away from the box's x / y faces (the
only ones with a complete range), n = 22 has four; nz in {2, 3, 4, 9} with
AFEM_CUBES_ZS in {1, 2, 3, default} gives complete ranges of 0, 1, 2 and more
layers per unit, at the bottom, inside and at the top of the box.  z-slabs
start the range next to the ghost layer below.  A random-numbered lattice
(canonical maps) has no stride and keeps its path.

Gates as in test_gpu_cubes_single_writer.py: the structure bit-exact, values
and RHS within 1e-12 of the oracle's largest entry, everything between two
cube runs bitwise.

test_dispatch_fallback pins what assemble_cubes runs when AFEM_CUBES_V names
no compiled instance of the wanted family and RHS mode: the default one."""
import numpy as np
import pytest

import arcanefem_amd as af
from oracle import oracle as O

pytestmark = pytest.mark.gpu

VAL_TOL = 1e-12
KERNEL_CUBES = 10  # AFEM_KERNEL_CUBES
F = 5.5
V_BASE = 16 | 32 | 64 | 256 | 512 | 1024 | 2048  # cubes.hip kCubesBase
V_ON = V_BASE | 4096
V_OFF = V_BASE

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


def _on_off(variant, bsr, ls, ref, what):
    """Bit on against the oracle; bit off, RHS add (2 x set) with the bit on and
    off, and all of these with the NaN fill: bitwise the bit-on set run."""
    variant("AFEM_CUBES_V", str(V_ON))
    on = _run(bsr, ls)
    if ref is not None:
        _check_oracle(bsr, on[0], on[1], ref)
    twice = (on[0], on[1] + on[1])
    for v in (V_ON, V_OFF):
        variant("AFEM_CUBES_V", str(v))
        for fill in (None, "nan"):
            variant("AFEM_CUBES_ACC_INIT", fill)
            _same(_run(bsr, ls), on, f"{what}: V={v} fill={fill} set")
            _same(_run(bsr, ls, "add"), twice, f"{what}: V={v} fill={fill} add")
    variant("AFEM_CUBES_ACC_INIT", None)
    variant("AFEM_CUBES_V", None)
    _same(_run(bsr, ls), on, f"{what}: the default")
    return on


@pytest.mark.parametrize("zs", [None, "1", "2", "3"])
@pytest.mark.parametrize("nz", [2, 3, 4, 9])
@pytest.mark.parametrize("n", [15, 22])
def test_row_stride_boxes(ctx, variant, n, nz, zs):
    variant("AFEM_CUBES_ZS", zs)
    mesh = af.Mesh.structured(ctx, 3, n, nz, jitter=0.2, seed=31)
    bsr, ls = _system(ctx, mesh)
    rows = bsr.download()[0]
    L = (n + 1) * (n + 1)
    stride = bsr.stats()["cube_row_stride"]
    # layers 1 .. nz - 1 can be complete; the stride is their rows' distance
    assert stride == rows[2 * L] - rows[L] and stride > 0, stride
    for layer in range(1, nz - 1):
        assert np.array_equal(rows[(layer + 1) * L:(layer + 2) * L] - rows[layer * L:(layer + 1) * L],
                              np.full(L, stride))
    _on_off(variant, bsr, ls, _oracle_for(("box", n, nz), mesh), f"box {n} x {nz}, zs {zs}")
    mesh.close()


@pytest.mark.parametrize("nranks", [2, 3])
def test_row_stride_slabs(ctx, variant, nranks):
    """z-slabs of one box: the complete range starts at k0 + 1, next to the
    ghost layer below; every slab against the oracle on the same subdomain."""
    n, nz = 15, 9
    for rank in range(nranks):
        mesh = af.Mesh.structured(ctx, 3, n, nz=nz, jitter=0.2, seed=13, nranks=nranks, rank=rank)
        bsr, ls = _system(ctx, mesh)
        own_layers = mesh.n_own_nodes // ((n + 1) * (n + 1))
        stride = bsr.stats()["cube_row_stride"]
        print(f"slab {rank} of {nranks}: {own_layers} owned layers, stride {stride}")
        if own_layers >= 3:  # at least owned layers 1 and 2 below the box's top
            assert stride > 0
        _on_off(variant, bsr, ls, _oracle_for(("slab", nranks, rank), mesh), f"slab {rank} of {nranks}")
        mesh.close()


@pytest.mark.parametrize("numbering", ["natural", "random"])
def test_row_stride_array_lattices(ctx, variant, numbering):
    """Lattices handed over as arrays: in their own lexicographic numbering
    (cube_lattice 2: the box instance; whatever stride the device check finds)
    and in a random one (cube_lattice 3: canonical maps, no stride, the
    canonical path as it was).  Both bitwise the run without the bit."""
    n = 15
    m0 = af.Mesh.structured(ctx, 3, n, jitter=0.2, seed=5)
    cells, coords, _ = m0.download()
    b0, l0 = _system(ctx, m0)
    box = _run(b0, l0)
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
    st = b1.stats()
    print(f"{numbering}: cube_lattice {st['cube_lattice']} stride {st['cube_row_stride']}")
    if numbering == "random":
        assert st["cube_lattice"] == 3 and st["cube_row_stride"] == 0, st
    else:
        assert st["cube_lattice"] == 2, st
        assert b0.stats()["cube_row_stride"] > 0
        assert st["cube_row_stride"] == b0.stats()["cube_row_stride"]
    on = _on_off(variant, b1, l1, None, numbering)
    if numbering == "natural":  # the generator box's system, bitwise
        _same(on, box, "natural lattice against the generator box")
    else:
        assert np.array_equal(on[1][p], box[1]), "RHS is not the generator box's, permuted"
    m1.close()
    m0.close()


V_UNLISTED = 12345  # a value cubes.hip compiles no instance for
V_SET_ONLY = V_ON | 8  # compiled with RHS set only (an ablation: no complete-layer flush, wrong values if it ran)


def _values_only(bsr):
    """One cube run without an RHS: the values."""
    bsr.resetMatrixValues()
    bsr.assemblePoissonP1(1.0, F)
    assert bsr.stats()["last_kernel"] == KERNEL_CUBES
    return bsr.download()[2]


def _check_fallback(variant, bsr, ls, what):
    """AFEM_CUBES_V with a value no instance is compiled for (every RHS mode), or
    with one compiled for RHS set only (RHS add, no RHS): the default instance of
    the family runs, values and RHS bitwise the default's."""
    def run(v, mode):
        """The run under test with AFEM_CUBES_V = v; an add run goes onto the
        default's set run (V_SET_ONLY itself runs under RHS set)."""
        variant("AFEM_CUBES_V", None)
        bsr.resetMatrixValues()
        if mode == "add":
            bsr.assemblePoissonP1(1.0, F, ls.rhsVariable(), rhs_mode="set")
            bsr.resetMatrixValues()
        variant("AFEM_CUBES_V", v)
        bsr.assemblePoissonP1(1.0, F, ls.rhsVariable(), rhs_mode=mode)
        assert bsr.stats()["last_kernel"] == KERNEL_CUBES
        return bsr.download()[2], ls.rhs_host()

    ref = {"set": run(None, "set"), "add": run(None, "add")}
    ref_values = _values_only(bsr)
    assert np.isfinite(ref_values).all() and np.array_equal(ref_values, ref["set"][0])
    assert np.array_equal(ref["add"][1], ref["set"][1] + ref["set"][1])
    for v, modes in ((V_UNLISTED, ("set", "add")), (V_SET_ONLY, ("add",))):
        for mode in modes:
            _same(run(str(v), mode), ref[mode], f"{what}: V={v} {mode}")
        assert np.array_equal(_values_only(bsr), ref_values), f"{what}: V={v} no RHS: values differ"
    variant("AFEM_CUBES_V", None)


def test_dispatch_fallback(ctx, variant):
    """n = 16, nz = 5, segments of 3 layers: three columns of units per axis, the
    middle one complete, the outer ones on the box's faces with a partial
    column, two segments.  The generator box (the headline instance), then the
    same box as arrays in a random numbering (the canonical and staged ones)."""
    variant("AFEM_CUBES_ZS", "3")
    m0 = af.Mesh.structured(ctx, 3, 16, 5, jitter=0.2, seed=17)
    b0, l0 = _system(ctx, m0)
    _check_fallback(variant, b0, l0, "box")
    cells, coords, _ = m0.download()
    rng = np.random.default_rng(17)
    p = rng.permutation(coords.shape[0])
    pc = np.empty_like(coords)
    pc[p] = coords
    cells = np.ascontiguousarray(p[cells].astype(np.int32)[rng.permutation(cells.shape[0])])
    m1 = af.Mesh.from_arrays(ctx, 3, cells, pc)
    b1, l1 = _system(ctx, m1)
    assert b1.stats()["cube_lattice"] == 3, b1.stats()
    _check_fallback(variant, b1, l1, "random-numbered arrays")
    m1.close()
    m0.close()
