"""GPU tests of block-2 elasticity on triangles with mass, body force and
vectorial Dirichlet conditions (the reference's elasticity module,
modules/elasticity/FemModule.cc:146-241), through the C ABI.

  * the fused triangle kernel (stiffness + mass_coef x consistent mass + body
    force RHS) against the oracle's stiffness plus elasticity2d_ref.py;
  * afem_ls_dirichlet_vectorial (NULL components) and the list form of
    row+column elimination;
  * the reference's three body-force goldens on bar.msh, every deck of
    elasticity2d_cases.py, both value layouts, direct solver and PCG.

Tolerances: matrix / RHS entries 1e-12 x max|reference| (summation and
evaluation order only); solutions 1e-10 relative (max norm) against the
restatement's reduced-system solve; the goldens by the rule of
elasticity2d_cases.py (1e-8 on the entries of the relative comparison for the
direct solver: the restatement itself is within 1.8e-10 of them, and
golden_cases.py holds goldens of this provenance to 1e-8).
"""
import numpy as np
import pytest

import arcanefem_amd as af
from arcanefem_amd.gmsh import read_gmsh, read_node_result_file
from oracle import oracle as O

import elasticity2d_ref as R
from elasticity2d_cases import DECKS, E, MESH, NU, PENALTY, SMALL_ENTRIES
from golden_cases import lame, path

pytestmark = pytest.mark.gpu

VAL_TOL = 1e-12
SOL_TOL = 1e-10
# PCG (rtol 1e-15) against the reduced-system solve: the direct solver's gate holds
# (measured 7.0e-13 at worst; the penalty rows are constraint rows the PCG's start solves on their own)
PCG_SOL_TOL = SOL_TOL
GOLDEN_DIRECT = 1e-8
K_E2 = 7
LAM, MU2 = 1.2e5, 2 * 8.1e4
MASS, FORCE = 3.7e6, (0.5, -1.0)
METHODS = ["penalty", "row-elimination", "row-column-elimination"]


def _close(a, b, tol=VAL_TOL):
    scale = max(np.abs(b).max(), 1e-300)
    err = np.abs(a - b).max() / scale
    assert err <= tol, f"differ from the reference: {err:.3e}"
    return err


def fan_mesh(m, seed=4):
    """One hub node joined to m rim nodes, m triangles: the hub row has m + 1 blocks."""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * (np.arange(m) + 0.3 * rng.random(m)) / m
    r = 1.0 + 0.1 * rng.random(m)
    coords = np.vstack([[0.0, 0.0, 0.0], np.c_[r * np.cos(ang), r * np.sin(ang), np.zeros(m)]])
    cells = [[0, 1 + i, 1 + (i + 1) % m] for i in range(m)]
    return np.array(cells, dtype=np.int32), coords


_GM = []


def _gm():
    if not _GM:
        _GM.append(read_gmsh(path(MESH)))
    return _GM[0]


def _mesh(ctx, which):
    if which == "bar":
        return af.Mesh.from_arrays(ctx, 2, _gm().cells, _gm().coords)
    if which == "box":
        return af.Mesh.structured(ctx, 2, 37)
    if which == "slab":  # ghosts on both sides, owned rows that fill no whole brick
        return af.Mesh.structured(ctx, 2, 19, nranks=3, rank=1)
    cells, coords = fan_mesh(120)
    return af.Mesh.from_arrays(ctx, 2, cells, coords)


_REF = {}


def _ref(mesh, which):
    """Per mesh, once: structure, stiffness, unit mass (per block) and the body-force RHS."""
    if which not in _REF:
        cells, coords, _ = mesh.download()
        n_own = mesh.n_own_nodes
        orp, ocols = O.sparsity(mesh.n_nodes, n_own, cells)
        K = O.assemble_elasticity_tri(n_own, cells, coords, orp, ocols, LAM, MU2)
        M = R.mass_blocks(n_own, cells, coords, orp, ocols, 1.0)
        rhs = R.body_force_rhs(n_own, cells, coords, FORCE)
        for a in (orp, ocols, K, M, rhs):
            a.setflags(write=False)
        _REF[which] = dict(orp=orp, ocols=ocols, K=K, M=M, rhs=rhs, area=R.tri_areas(cells, coords).sum())
    return _REF[which]


def _assemble_ex(ctx, mesh, use_csr, mass, force=FORCE, mode="set", fill=7.0):
    bsr = af.BSRFormat(mesh, 2).initialize(use_csr)
    bsr.computeSparsity()
    n2 = 2 * mesh.n_own_nodes
    d = ctx.malloc(8 * n2)
    ctx.to_device(d, np.full(n2, fill))
    bsr.assembleElasticityP1Ex(LAM, MU2, mass, force, d, rhs_mode=mode)
    rhs = ctx.to_host(d, n2, np.float64)
    ctx.free(d)
    return bsr, rhs


def _check_assembly(bsr, rhs, ref, use_csr, mass):
    rows, cols, vals = bsr.download()
    assert np.array_equal(rows, ref["orp"]) and np.array_equal(cols, ref["ocols"])
    ovals = ref["K"] + mass * ref["M"]
    if use_csr:
        ovals = O.blocks_to_row_order(ref["orp"], ovals)
    ev = _close(vals, ovals)
    er = _close(rhs, ref["rhs"])
    return ev, er


# ---------------------------------------------------------------- assembly parity
@pytest.mark.parametrize("which", ["bar", "box", "slab"])
@pytest.mark.parametrize("use_csr", [False, True])
@pytest.mark.parametrize("mass", [0.0, MASS])
def test_fused_assembly_parity(ctx, which, use_csr, mass):
    mesh = _mesh(ctx, which)
    ref = _ref(mesh, which)
    bsr, rhs = _assemble_ex(ctx, mesh, use_csr, mass)
    st = bsr.stats()
    assert st["last_kernel"] == K_E2 and st["rows_per_block"] == 64  # the LDS tile instance
    ev, er = _check_assembly(bsr, rhs, ref, use_csr, mass)
    print(f"{which} csr={use_csr} mass={mass}: values {ev:.2e}, rhs {er:.2e}")
    if which != "slab":  # every node owned: the RHS sums to f x area
        for i in range(2):
            assert abs(rhs[i::2].sum() - FORCE[i] * ref["area"]) <= VAL_TOL * ref["area"]
    if which == "box":  # the unit square, boundary nodes moved by the jitter
        assert abs(rhs[1::2].sum() - FORCE[1]) < 0.05 * abs(FORCE[1])


@pytest.mark.parametrize("use_csr", [False, True])
def test_fused_assembly_on_a_fan_takes_the_global_instance(ctx, use_csr):
    # the hub row (121 blocks) is past the LDS tile budget (kTileLdsMax:
    # 8 B x 64 lanes x 4 x 121 slots = 242 KiB): accumulation in the value array
    mesh = _mesh(ctx, "fan")
    ref = _ref(mesh, "fan")
    bsr, rhs = _assemble_ex(ctx, mesh, use_csr, MASS)
    st = bsr.stats()
    assert st["last_kernel"] == K_E2 and st["rows_per_block"] == 0 and st["max_row_len"] == 121
    _check_assembly(bsr, rhs, ref, use_csr, MASS)


# ---------------------------------------------------------------- RHS modes, reproducibility
@pytest.mark.parametrize("which", ["slab", "fan"])
@pytest.mark.parametrize("use_csr", [False, True])
def test_rhs_modes_and_reproducibility(ctx, which, use_csr):
    mesh = _mesh(ctx, which)
    bsr = af.BSRFormat(mesh, 2).initialize(use_csr)
    bsr.computeSparsity()
    n2 = 2 * mesh.n_own_nodes
    d = ctx.malloc(8 * n2)
    ctx.to_device(d, np.ones(n2))
    runs = []
    for _ in range(3):
        bsr.assembleElasticityP1Ex(LAM, MU2, MASS, FORCE, d, rhs_mode="set")
        runs.append((bsr.download()[2], ctx.to_host(d, n2, np.float64)))
    for v, r in runs[1:]:
        assert np.array_equal(v, runs[0][0]) and np.array_equal(r, runs[0][1])
    ctx.to_device(d, np.ones(n2))
    bsr.assembleElasticityP1Ex(LAM, MU2, MASS, FORCE, d, rhs_mode="add")
    assert np.array_equal(ctx.to_host(d, n2, np.float64), 1.0 + runs[0][1])
    assert np.array_equal(bsr.download()[2], runs[0][0])
    # without mass and body force: the plain entry, bit for bit; the RHS is not touched
    ctx.to_device(d, np.ones(n2))
    bsr.assembleElasticityP1Ex(LAM, MU2, 0.0, None, None)
    assert bsr.stats()["last_kernel"] == K_E2
    v_ex = bsr.download()[2]
    bsr.assembleElasticityP1Ex(LAM, MU2, 0.0, None, d)
    assert np.array_equal(ctx.to_host(d, n2, np.float64), np.ones(n2))
    bsr.resetMatrixValues()
    bsr.assembleElasticityP1(LAM, MU2)
    assert bsr.stats()["last_kernel"] == K_E2
    assert np.array_equal(v_ex, bsr.download()[2])
    # mass 0 with a body force runs the fused form: the same stiffness, the same RHS bits
    bsr.assembleElasticityP1Ex(LAM, MU2, 0.0, FORCE, d, rhs_mode="set")
    _close(bsr.download()[2], v_ex)
    assert np.array_equal(ctx.to_host(d, n2, np.float64), runs[0][1])
    ctx.free(d)


def test_other_combinations_keep_their_error(ctx):
    for dim, k in ((2, 1), (3, 1)):
        mesh = af.Mesh.structured(ctx, dim, 4)
        bsr = af.BSRFormat(mesh, k).initialize(True)
        bsr.computeSparsity()
        with pytest.raises(af.AfemError) as e:
            bsr.assembleElasticityP1Ex(LAM, MU2, 0.0, None, None)
        assert e.value.code == 3  # AFEM_ERR_NOT_IMPL


# ---------------------------------------------------------------- vectorial Dirichlet flags
def _ls_arrays(ctx, ls):
    n = ls.n_rows
    return dict(finfo=ctx.to_host(ls.getForcedInfo(), n, np.uint8), fval=ctx.to_host(ls.getForcedValue(), n, np.float64),
                einfo=ctx.to_host(ls.getEliminationInfo(), n, np.uint8),
                eval=ctx.to_host(ls.getEliminationValue(), n, np.float64), rhs=ls.rhs_host())


@pytest.mark.parametrize("which", ["box9", "slab"])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("u", [(0.25, None), (None, -2.0), (1.0, 3.0)])
def test_vectorial_dirichlet_flags(ctx, which, method, u):
    mesh = af.Mesh.structured(ctx, 2, 9) if which == "box9" else _mesh(ctx, "slab")
    n_own, n_all = mesh.n_own_nodes, mesh.n_nodes
    ls = af.DoFLinearSystem().initialize(ctx, 2 * n_own, 2 * n_all)
    ls.set_rhs_host(np.full(2 * n_own, 7.0))
    before = _ls_arrays(ctx, ls)
    nodes = np.array([0, 5, 17, n_own // 2, n_own - 1], dtype=np.int32)
    if which == "slab":  # ghost ids in the list are ignored
        assert n_all > n_own
        nodes = np.concatenate([nodes, np.array([n_own, n_own + 3, n_all - 1], dtype=np.int32)])
    ls.applyDirichletVectorial(nodes, u, method, 1e30)
    after = _ls_arrays(ctx, ls)
    dofs, vals = R.expand_u(nodes, u, n_own=n_own)
    assert dofs.size == 5 * sum(x is not None for x in u)
    sel = np.zeros(2 * n_own, dtype=bool)
    sel[dofs] = True
    touched = ("finfo", "fval", "rhs") if method == "penalty" else ("einfo", "eval")
    for name in before:
        assert np.array_equal(after[name][~sel], before[name][~sel]), name
        if name not in touched:
            assert np.array_equal(after[name], before[name]), name
    if method == "penalty":
        assert np.all(after["finfo"][dofs] == 1) and np.all(after["fval"][dofs] == 1e30)
        assert np.array_equal(after["rhs"][dofs], 1e30 * vals)
    else:
        assert np.all(after["einfo"][dofs] == METHODS.index(method))
        assert np.array_equal(after["eval"][dofs], vals)


# ---------------------------------------------------------------- row+column elimination from a list
def test_row_column_elimination_from_a_list(ctx):
    gm = _gm()
    n = gm.n_nodes
    left, br = gm.group_nodes("left"), gm.group_nodes("botRight")
    dofs = np.concatenate([2 * left, 2 * left + 1, 2 * br + 1]).astype(np.int32)
    g = 0.25

    def system():
        mesh = af.Mesh.from_arrays(ctx, 2, gm.cells, gm.coords)
        bsr = af.BSRFormat(mesh, 2).initialize(True)  # the linear system's view is the BSR's own values
        bsr.computeSparsity()
        ls = af.DoFLinearSystem().initialize(ctx, 2 * n)
        bsr.assembleElasticityP1Ex(LAM, MU2, 0.0, FORCE, ls.rhsVariable(), rhs_mode="set")
        bsr.toLinearSystem(ls)
        return mesh, bsr, ls

    mesh, bsr, ls = system()
    ls.applyDirichletViaRowColumnElimination(dofs, g)
    ls.applyBoundaryConditions()
    vals, rhs = bsr.download()[2], ls.rhs_host()
    # the oracle's Aleph elimination on the scalar CSR
    ref = _ref(mesh, "bar")
    srp, scols, svals = R.scalar_csr(ref["orp"], ref["ocols"], np.array(ref["K"]))
    orhs = np.array(ref["rhs"])
    info, val = np.zeros(2 * n, np.uint8), np.zeros(2 * n)
    info[dofs], val[dofs] = 2, g
    before = svals.copy()
    O.eliminate(info, val, srp, scols, svals, orhs)
    free = np.setdiff1d(np.arange(2 * n), dofs)
    assert np.abs(orhs[free] - ref["rhs"][free]).max() > 0  # the column pass moved the RHS
    assert np.count_nonzero(svals != before) > dofs.size
    _close(vals, svals)
    _close(rhs, orhs)
    # the one-row host entry on the same list: bit for bit
    mesh2, bsr2, ls2 = system()
    for d in dofs:
        ls2.eliminateRowColumn(int(d), g)
    ls2.applyBoundaryConditions()
    assert np.array_equal(bsr2.download()[2], vals) and np.array_equal(ls2.rhs_host(), rhs)
    # and the solve keeps the eliminated values exactly
    ls.setSolverOptions(method="direct")
    ls.solve()
    x = ls.solution_host()
    assert np.all(x[dofs] == g)
    xo = np.linalg.solve(O.csr_to_dense(srp, scols, svals), orhs)
    assert np.abs(x - xo).max() / np.abs(xo).max() <= SOL_TOL


# ---------------------------------------------------------------- the three goldens
_UREF = {}


def _deck_reference(deck):
    if deck not in _UREF:
        _UREF[deck] = R.deck_reference(_gm(), DECKS[deck])
        _UREF[deck].setflags(write=False)
    return _UREF[deck]


@pytest.mark.parametrize("deck", list(DECKS))
@pytest.mark.parametrize("use_csr", [False, True])
@pytest.mark.parametrize("solver", ["direct", "pcg"])
def test_elasticity_goldens(ctx, deck, use_csr, solver):
    c = DECKS[deck]
    gm = _gm()
    n = gm.n_nodes
    lam, mu2 = lame(E, NU)
    mesh = af.Mesh.from_arrays(ctx, 2, gm.cells, gm.coords)
    bsr = af.BSRFormat(mesh, 2).initialize(use_csr)
    bsr.computeSparsity()
    ls = af.DoFLinearSystem().initialize(ctx, 2 * n)
    f = tuple(0.0 if x is None else x for x in c["f"])
    bsr.assembleElasticityP1Ex(lam, mu2, 0.0, f, ls.rhsVariable(), rhs_mode="set")
    assert bsr.stats()["last_kernel"] == K_E2
    bsr.toLinearSystem(ls)
    for group, t in c["traction"]:
        af.applyNeumannToRhs(mesh, ls.rhsVariable(), gm.group_faces(group), t, "traction", nb_dof=2)
    for group, u in c["dirichlet"] + c["points"]:
        ls.applyDirichletVectorial(gm.group_nodes(group), u, c["method"], PENALTY)
    ls.setSolverOptions(method=solver, rtol=1e-15, max_iter=50000)
    st = ls.solve()
    x = ls.solution_host()
    xr = _deck_reference(deck)
    err = np.abs(x - xr).max() / np.abs(xr).max()
    r = R.golden_compare(x, read_node_result_file(path(c["golden"])), gm.node_tags)
    print(f"{deck} [{solver}, csr={use_csr}]: vs reduced solve {err:.3e}, golden {r}, "
          f"{st['iterations']} iterations, residual {st['rel_residual']:.2e}")
    assert err <= (SOL_TOL if solver == "direct" else PCG_SOL_TOL)
    if c["method"] != "penalty":
        dofs, values = R.deck_constraints(gm, c)
        assert np.all(x[dofs] == values)
    assert r["n_small"] == SMALL_ENTRIES[c["golden"]]
    assert r["small_ok"], r
    assert r["nerr"] == 0
    if solver == "direct":
        assert r["rel"] <= GOLDEN_DIRECT
