"""The cube kernel's single-writer dataflow (cubes.hip, AFEM_CUBES_V bit 2048,
the default): with the z carry, both exchanges and the dummy rows every
accumulator slot takes exactly one sum per layer cycle, so the sums are stored
into a buffer laid out as the image, flush_full writes back the diagonal alone
and nothing is zero-filled.  Without the bit the sums are added into zeroed
offset planes: 0.0 + x = x and no summation order changes, so both give the
same bits.

AFEM_CUBES_ACC_INIT=nan fills the accumulators with a quiet NaN once, at the
kernel's start: a flush that read a slot its own layer cycle did not write
would put the NaN (or stale data) into a value or the RHS.

Shapes as in test_gpu_cubes_loops.py: n = 15 gives one column away from the
faces (complete layers: flush_full), one face column and one partial column;
AFEM_CUBES_ZS and nz choose segments at the box's bottom, inside and at its
top (nz = 9 in segments of 3: a unit that runs flush_full and then add_top).

Gates as there: the structure bit-exact, values and RHS within 1e-12 of the
oracle's largest entry, everything between two cube runs bitwise."""
import numpy as np
import pytest

import arcanefem_amd as af
from oracle import oracle as O

pytestmark = pytest.mark.gpu

VAL_TOL = 1e-12
KERNEL_CUBES = 10  # AFEM_KERNEL_CUBES
F = 5.5
V_ON = 16 | 32 | 64 | 256 | 512 | 1024 | 2048  # cubes.hip kCubesV
V_OFF = V_ON & ~2048  # the adding instances

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


def _set_run(bsr, ls):
    """One cube run into cleared values, RHS set: (values, RHS)."""
    bsr.resetMatrixValues()
    bsr.assemblePoissonP1(1.0, F, ls.rhsVariable(), rhs_mode="set")
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


def _nan_fill_same(variant, bsr, ls, ref, what):
    """The run again with the accumulators NaN-filled at the kernel's start."""
    variant("AFEM_CUBES_ACC_INIT", "nan")
    got = _set_run(bsr, ls)
    variant("AFEM_CUBES_ACC_INIT", None)
    _same(got, ref, what + ", NaN fill")


@pytest.mark.parametrize("n,nz,zs", [(15, nz, zs) for nz in (1, 2, 3, 9) for zs in (None, "1", "3")] + [(8, 2, None)])
def test_stores_against_adds(ctx, variant, n, nz, zs):
    """Bit on against bit off, bitwise values and RHS; the new path against the
    oracle; RHS add = 2 x set on the new path, bitwise; the NaN fill changes
    nothing on the new path and is ignored by the adding one."""
    variant("AFEM_CUBES_ZS", zs)
    mesh = af.Mesh.structured(ctx, 3, n, nz, jitter=0.2, seed=31)
    bsr, ls = _system(ctx, mesh)
    on = _set_run(bsr, ls)
    _check_oracle(bsr, on[0], on[1], _oracle_for(("box", n, nz), mesh))
    bsr.resetMatrixValues()
    bsr.assemblePoissonP1(1.0, F, ls.rhsVariable(), rhs_mode="add")
    assert bsr.stats()["last_kernel"] == KERNEL_CUBES
    assert np.array_equal(ls.rhs_host(), on[1] + on[1]), "RHS add is not 2 x set"
    assert np.array_equal(bsr.download()[2], on[0])
    _nan_fill_same(variant, bsr, ls, on, "stores")
    # the NaN fill with RHS add (another instance of the kernel)
    variant("AFEM_CUBES_ACC_INIT", "nan")
    bsr.assemblePoissonP1(1.0, F, ls.rhsVariable(), rhs_mode="add")
    variant("AFEM_CUBES_ACC_INIT", None)
    assert np.array_equal(ls.rhs_host(), on[1] + on[1]) and np.array_equal(bsr.download()[2], on[0])
    # the general flush everywhere (no flush_full), NaN-filled too
    variant("AFEM_CUBES_FULL", "0")
    _same(_set_run(bsr, ls), on, "general flush")
    _nan_fill_same(variant, bsr, ls, on, "general flush")
    variant("AFEM_CUBES_FULL", None)
    variant("AFEM_CUBES_V", str(V_OFF))
    _same(_set_run(bsr, ls), on, "adds against stores")
    _nan_fill_same(variant, bsr, ls, on, "adds (the knob is ignored)")
    mesh.close()


@pytest.mark.parametrize("nranks", [2, 3])
def test_stores_on_slabs(ctx, variant, nranks):
    """z-slabs of one box (the ghost layer below, local layers out of id
    order): every slab against the oracle on the same subdomain, bit on
    against bit off and NaN-filled."""
    for rank in range(nranks):
        mesh = af.Mesh.structured(ctx, 3, 15, nz=7, jitter=0.2, seed=13, nranks=nranks, rank=rank)
        bsr, ls = _system(ctx, mesh)
        on = _set_run(bsr, ls)
        _check_oracle(bsr, on[0], on[1], _oracle_for(("slab", nranks, rank), mesh))
        _nan_fill_same(variant, bsr, ls, on, f"slab {rank} of {nranks}")
        variant("AFEM_CUBES_V", str(V_OFF))
        _same(_set_run(bsr, ls), on, f"slab {rank} of {nranks}, adds against stores")
        variant("AFEM_CUBES_V", None)
        mesh.close()


@pytest.mark.parametrize("n,nz,zs,seed", [(9, 4, None, 3), (9, 9, "3", 7)])
def test_stores_canonical(ctx, variant, n, nz, zs, seed):
    """Random-numbered arrays of a generator box (as test_staged_canonical_units):
    the staged canonical path and the single-pass one (V without 1024), each
    bitwise the generator box's system permuted, with and without the bit and
    NaN-filled."""
    variant("AFEM_CUBES_ZS", zs)
    m0 = af.Mesh.structured(ctx, 3, n, nz=nz, jitter=0.2, seed=seed)
    b0, l0 = _system(ctx, m0)
    v0, rhs0 = _set_run(b0, l0)
    cells0, coords0, _ = m0.download()
    rng = np.random.default_rng(seed)
    nn = coords0.shape[0]
    p = rng.permutation(nn)
    cells = p[cells0].astype(np.int32)[rng.permutation(cells0.shape[0])]
    coords = np.empty_like(coords0)
    coords[p] = coords0
    m1 = af.Mesh.from_arrays(ctx, 3, cells, coords)
    b1, l1 = _system(ctx, m1)
    r0, c0, _ = b0.download()
    first = None
    for v in (None, V_ON & ~1024, V_OFF, V_OFF & ~1024):
        variant("AFEM_CUBES_V", None if v is None else str(v))
        got = _set_run(b1, l1)
        if first is None:
            st = b1.stats()
            assert st["cube_lattice"] == 3, st
            r1, c1, _ = b1.download()
            key0 = p[np.repeat(np.arange(nn), np.diff(r0))].astype(np.int64) * nn + p[c0]
            key1 = np.repeat(np.arange(nn), np.diff(r1)).astype(np.int64) * nn + c1
            o0, o1 = np.argsort(key0), np.argsort(key1)
            assert np.array_equal(key0[o0], key1[o1])
            assert np.array_equal(v0[o0], got[0][o1]), "values are not the generator box's, permuted"
            assert np.array_equal(got[1][p], rhs0), "RHS is not the generator box's, permuted"
            first = got
        _same(got, first, f"V={v}")
        _nan_fill_same(variant, b1, l1, first, f"V={v}")
    variant("AFEM_CUBES_V", None)
    b1.assemblePoissonP1(1.0, F, l1.rhsVariable(), rhs_mode="add")
    assert np.array_equal(l1.rhs_host(), first[1] + first[1])
    m1.close()
    m0.close()


@pytest.mark.parametrize("knobs", [{"AFEM_CUBES_YEX": "0"}, {"AFEM_CUBES_STRIDE": "49"}])
def test_adding_paths_keep(ctx, variant, knobs):
    """Instances without the y exchange or with 49-row planes keep the adds,
    the offset planes and the zero fill: the oracle's system, and the same bits
    with the NaN knob set (ignored there)."""
    mesh = af.Mesh.structured(ctx, 3, 15, 3, jitter=0.2, seed=31)
    bsr, ls = _system(ctx, mesh)
    for k, v in knobs.items():
        variant(k, v)
    got = _set_run(bsr, ls)
    _check_oracle(bsr, got[0], got[1], _oracle_for(("box", 15, 3), mesh))
    _nan_fill_same(variant, bsr, ls, got, str(knobs))
    mesh.close()
