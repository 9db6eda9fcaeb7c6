"""The cube kernel's z walk split by flush kind (cubes.hip): a unit away from
the x / y faces runs [general layers] -> [complete layers: a loop of its own
with flush_full] -> [general layers, the box's top layer]; the other units run
the general loop only; the staged canonical flush issues a fixed 7 stores and
loads its ids one trip ahead.

n = 15 gives 16 nodes per line, so of the three 7-row columns column 1 is away
from the faces (complete layers), column 0 touches them and column 2 is
partial: all three kinds of unit in every box.  nz and AFEM_CUBES_ZS choose
complete-layer loops of 0, 1 and 2 or more trips, in segments that start at
the box's bottom, end at its top, or lie inside.

Tolerances as in test_gpu_parity.py: the structure bit-exact, values and RHS
within 1e-12 of the oracle's largest entry, per entry (the summation order
differs: ~1e-16 relative); everything between two runs of the cube kernel is
compared bitwise."""
import numpy as np
import pytest

import arcanefem_amd as af
from oracle import oracle as O

pytestmark = pytest.mark.gpu

VAL_TOL = 1e-12
KERNEL_CUBES = 10  # AFEM_KERNEL_CUBES
F = 5.5

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


def _assemble(ctx, mesh):
    bsr = af.BSRFormat(mesh, 1).initialize(True)
    bsr.computeSparsity()
    ls = af.DoFLinearSystem().initialize(ctx, mesh.n_own_nodes, mesh.n_nodes)
    bsr.assemblePoissonP1(1.0, F, ls.rhsVariable())
    bsr.toLinearSystem(ls)
    return bsr, ls


def _check_oracle(bsr, ls, ref):
    orp, ocols, ovals, orhs = ref
    rows, cols, vals = bsr.download()
    rhs = ls.rhs_host()
    assert np.array_equal(rows, orp) and np.array_equal(cols, ocols)
    verr = np.abs(vals - ovals).max() / np.abs(ovals).max()
    rerr = np.abs(rhs - orhs).max() / np.abs(orhs).max()
    print(f"values {verr:.3e} rhs {rerr:.3e}")
    assert verr <= VAL_TOL, f"CSR values differ from the oracle: {verr:.3e}"
    assert rerr <= VAL_TOL, f"RHS differs from the oracle: {rerr:.3e}"
    return vals, rhs


@pytest.mark.parametrize("zs", [None, "1", "2", "3"])
@pytest.mark.parametrize("nz", [1, 2, 3, 9])
def test_three_phase_units(ctx, variant, nz, zs):
    """Boxes whose middle column runs all three phases of the walk: values and
    RHS against the oracle; the general flush everywhere (AFEM_CUBES_FULL=0)
    gives the same bits; RHS add = 2 x set, bitwise; a second set run,
    bitwise."""
    variant("AFEM_CUBES_ZS", zs)
    mesh = af.Mesh.structured(ctx, 3, 15, nz, jitter=0.2, seed=31)
    bsr, ls = _assemble(ctx, mesh)
    assert bsr.stats()["last_kernel"] == KERNEL_CUBES
    vals, rhs = _check_oracle(bsr, ls, _oracle_for(("box", nz), mesh))
    variant("AFEM_CUBES_FULL", "0")
    bsr.assemblePoissonP1(1.0, F, ls.rhsVariable(), rhs_mode="set")
    assert bsr.stats()["last_kernel"] == KERNEL_CUBES
    assert np.array_equal(bsr.download()[2], vals), "the general flush and flush_full differ"
    assert np.array_equal(ls.rhs_host(), rhs)
    variant("AFEM_CUBES_FULL", None)
    bsr.assemblePoissonP1(1.0, F, ls.rhsVariable(), rhs_mode="add")
    assert np.array_equal(ls.rhs_host(), rhs + rhs)
    bsr.assemblePoissonP1(1.0, F, ls.rhsVariable(), rhs_mode="set")
    assert np.array_equal(bsr.download()[2], vals) and np.array_equal(ls.rhs_host(), rhs)
    mesh.close()


@pytest.mark.parametrize("zs", [None, "1"])
@pytest.mark.parametrize("nranks", [2, 3])
def test_three_phase_units_on_slabs(ctx, variant, nranks, zs):
    """z-slabs of the same box: the middle column's unit next to a slab's ghost
    layer below has its local layers out of id order on its first layer, which
    is where its complete range starts.  Every slab against the oracle on the
    same subdomain."""
    variant("AFEM_CUBES_ZS", zs)
    for rank in range(nranks):
        mesh = af.Mesh.structured(ctx, 3, 15, nz=7, jitter=0.2, seed=13, nranks=nranks, rank=rank)
        bsr, ls = _assemble(ctx, mesh)
        assert bsr.stats()["last_kernel"] == KERNEL_CUBES
        _check_oracle(bsr, ls, _oracle_for(("slab", nranks, rank), mesh))
        mesh.close()


# (9, 4), (15, 3), (8, 2): lines of 10, 16 and 9 nodes, no multiple of the 7-row
# columns, so the last column of units has x-runs past the box that repeat run
# 0's store.  (9, 8) and (9, 9) in segments of 3 layers: the top segment holds
# three layers / one layer, and the id prefetch reaches past the last layer.
@pytest.mark.parametrize("n,nz,zs,seed", [(9, 4, None, 3), (15, 3, None, 4), (8, 2, None, 5), (9, 8, "3", 6),
                                          (9, 9, "3", 7)])
def test_staged_canonical_units(ctx, variant, n, nz, zs, seed):
    """The staged canonical path on random-numbered arrays of a generator box:
    bitwise the generator box's matrix and RHS (also the cube kernel's),
    permuted, in set and add RHS modes."""
    variant("AFEM_CUBES_ZS", zs)
    m0 = af.Mesh.structured(ctx, 3, n, nz=nz, jitter=0.2, seed=seed)
    b0, l0 = _assemble(ctx, m0)
    assert b0.stats()["last_kernel"] == KERNEL_CUBES
    cells0, coords0, _ = m0.download()
    rng = np.random.default_rng(seed)
    nn = coords0.shape[0]
    p = rng.permutation(nn)
    cells = p[cells0].astype(np.int32)[rng.permutation(cells0.shape[0])]
    coords = np.empty_like(coords0)
    coords[p] = coords0
    m1 = af.Mesh.from_arrays(ctx, 3, cells, coords)
    b1, l1 = _assemble(ctx, m1)
    st = b1.stats()
    assert st["cube_lattice"] == 3 and st["last_kernel"] == KERNEL_CUBES, st
    r0, c0, v0 = b0.download()
    r1, c1, v1 = b1.download()
    key0 = p[np.repeat(np.arange(nn), np.diff(r0))].astype(np.int64) * nn + p[c0]
    key1 = np.repeat(np.arange(nn), np.diff(r1)).astype(np.int64) * nn + c1
    o0, o1 = np.argsort(key0), np.argsort(key1)
    assert np.array_equal(key0[o0], key1[o1])
    assert np.array_equal(v0[o0], v1[o1])
    rhs1 = l1.rhs_host()
    assert np.array_equal(rhs1[p], l0.rhs_host())
    b1.assemblePoissonP1(1.0, F, l1.rhsVariable(), rhs_mode="add")
    assert np.array_equal(l1.rhs_host(), rhs1 + rhs1)
    assert np.array_equal(b1.download()[2][o1], v0[o0])
    b1.assemblePoissonP1(1.0, F, l1.rhsVariable(), rhs_mode="set")
    assert np.array_equal(l1.rhs_host(), rhs1) and np.array_equal(b1.download()[2], v1)
    m1.close()
    m0.close()
