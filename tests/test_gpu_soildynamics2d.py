"""GPU tests of the soildynamics module (modules/soildynamics, TRIA3, block 2)
through the C ABI: the paraxial edge kernel (afem_bsr_add_paraxial_p1) and the
time loop (Soildynamics2D: paraxial boundaries + double-couple source on the
Elastodynamics2D step), against the fp64 restatement soildynamics2d_ref.py that
test_soildynamics2d_ref.py pins with the module's golden files.

Kernel entry (the square with its four groups: corner nodes in two blocks; the
semi-circle's curved `lower` group; the boundary of the jittered 37 x 37 box,
148 nodes = more than two wavefronts, its list cut into four pieces in shuffled order;
a ghosted slab's two physical sides, whose end edges join an owned and a
ghost node and whose ghost-ghost edges are dropped; both value layouts; random
U, V, A and a random fixed mask of 15 % with one node fixed in one component):
values and RHS at VAL_TOL = 1e-12 x max against paraxial_lhs / paraxial_rhs,
fixed DoFs' RHS bit-untouched, on a prefilled matrix every value outside the
touched blocks keeps its bits and the RHS is prefill + the zero-based result
bit for bit, two runs bitwise equal, an edge listed twice = two
calls (at VAL_TOL: the diagonal block is accumulated over the node's edges
before it is added, so the two sums round differently).
Measured worst over the 8 cases: values 3.6e-16 (the slab), RHS 2.7e-16 (the box).

Loop: the five decks of soildynamics2d_cases.py for their own step counts,
direct solver and PCG (rtol 1e-15), through _run_against's gates of
test_gpu_elastodynamics2d.py: |U - U_ref| <= N_steps x SOL_TOL x max|U|, V and A
at that bound x gamma / (beta dt) and 1 / (beta dt^2), constrained DoFs
bit-exact every step.  The two golden decks are also checked against their
golden files by the reference's checker (zero failures at 1e-4).
Measured worst errors as fractions of those gates over the ten cases: U 3.1e-3
(Soildynamics.arc, direct), V 4.4e-4 (the same), A 2.5e-4 (the soil constants
on the square, PCG); the paraxial decks alone: U 5.7e-5, V 1.4e-5, A 2.5e-4.
The PCG needs no wider gate on the paraxial decks (the LHS stays symmetric
positive definite; 32 iterations per solve on the square and the semi-circle).
Goldens on the GPU: zero checker failures; max|U - G| / max|G| 7.0e-11 /
3.5e-11 (bar, direct / PCG) and 3.7e-13 / 4.0e-13 (square).
operators(): (LHS - the kernel entry's LHS) - paraxial_lhs = 5.5e-16 of
max|paraxial|.  dt change mid-run: U 1.7e-5, V 9.6e-6, A 7.5e-5 of the gates.
"""
import ctypes

import numpy as np
import pytest

import arcanefem_amd as af
from arcanefem_amd import _capi as C
from arcanefem_amd.gmsh import read_gmsh, read_node_result_file
from oracle import oracle as O

import elastodynamics2d_ref as R
import soildynamics2d_ref as S
from golden_cases import path
from soildynamics2d_cases import DECKS, GOLDEN, SEMI_SOIL, SQUARE
from test_gpu_elasticity2d import VAL_TOL
from test_gpu_elastodynamics2d import _Dev, _rel, _run_against

pytestmark = pytest.mark.gpu

RHO, DT, CP, CS = 1.3, 0.01, 4.0, 2.0
LAM, MU2 = 576.9230769, 2 * 384.6153846  # the prefilled values: a stiffness matrix
MESHES = ["square", "semi", "box", "slab"]

_GM = {}


def _gm(name):
    if name not in _GM:
        _GM[name] = read_gmsh(path(name))
    return _GM[name]


def _boundary_edges(cells):
    """Edges that belong to one cell, in cell order."""
    e = np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [2, 0]]])
    key = np.sort(e, axis=1)
    _, idx, cnt = np.unique(key, axis=0, return_index=True, return_counts=True)
    return e[np.sort(idx[cnt == 1])].astype(np.int32)


def _mesh_and_faces(ctx, which):
    if which == "square":
        gm = _gm(SQUARE)
        return (af.Mesh.from_arrays(ctx, 2, gm.cells, gm.coords),
                np.concatenate([gm.group_faces(g) for g in ("left", "top", "right", "bottom")]))
    if which == "semi":
        gm = _gm(SEMI_SOIL)
        return af.Mesh.from_arrays(ctx, 2, gm.cells, gm.coords), gm.group_faces("lower")
    if which == "box":
        mesh = af.Mesh.structured(ctx, 2, 37)
        faces = _boundary_edges(mesh.download()[0])
        assert np.unique(faces).size == 148  # 4 x 37: more than two wavefronts
        q = np.array_split(np.arange(faces.shape[0]), 4)
        return mesh, np.concatenate([faces[q[i]] for i in (2, 0, 3, 1)])
    mesh = af.Mesh.structured(ctx, 2, 19, nranks=3, rank=1)  # ghosts on both sides
    cells, coords, _ = mesh.download()
    faces = _boundary_edges(cells)
    col = faces % 20  # local ids run along x within a node layer of 20 (owned layers, then the ghost layers)
    faces = faces[(col[:, 0] == col[:, 1]) & ((col[:, 0] == 0) | (col[:, 0] == 19))]
    x = coords[:, 0]
    assert faces.shape[0] > 8 and np.all((np.abs(x[faces]) < 0.02) | (np.abs(x[faces] - 1.0) < 0.02))
    own = faces < mesh.n_own_nodes
    assert (own[:, 0] != own[:, 1]).any()  # an owned and a ghost end
    ghost = cells[:, :2][(cells[:, :2] >= mesh.n_own_nodes).all(1)][:1]  # and one edge between two ghosts: ignored
    assert ghost.shape == (1, 2)
    faces = np.concatenate([faces, ghost])
    return mesh, faces


_REF = {}


def _ref(ctx, which):
    """Per mesh, once: structure, the random state, the paraxial LHS blocks and RHS."""
    if which not in _REF:
        mesh, faces = _mesh_and_faces(ctx, which)
        cells, coords, _ = mesh.download()
        n_own = mesh.n_own_nodes
        orp, ocols = O.sparsity(mesh.n_nodes, n_own, cells)
        rng = np.random.default_rng(7)
        n = 2 * mesh.n_nodes
        U, V, A = rng.standard_normal(n) * 1e-3, rng.standard_normal(n) * 1e-2, rng.standard_normal(n)
        fixed = rng.random(2 * n_own) < 0.15
        v0 = int(faces[faces < n_own][0])
        fixed[2 * v0:2 * v0 + 2] = (True, False)  # a boundary node with one component flagged
        p = S.paraxial_constants(RHO, DT)
        lhs = S.paraxial_lhs(n_own, coords, faces, orp, ocols, p[0], CP, CS)
        rhs = S.paraxial_rhs(n_own, coords, faces, p, CP, CS, U, V, A, fixed)
        # the values of the touched blocks: (v, v) and (v, other end) for every owned end v of every edge
        tb = np.zeros(ocols.shape[0])
        for a, b in faces:
            for i, j in ((a, a), (a, b), (b, b), (b, a)):
                if i < n_own:
                    row = ocols[orp[i]:orp[i + 1]]
                    tb[orp[i] + int(np.searchsorted(row, j))] = 1.0
        touched = np.repeat(tb, 4)
        for a in (lhs, rhs, U, V, A, fixed, faces):
            a.setflags(write=False)
        _REF[which] = dict(mesh=mesh, faces=faces, orp=orp, ocols=ocols, U=U, V=V, A=A, fixed=fixed, p=p, lhs=lhs,
                           rhs=rhs)
        _REF[which]["touched", False] = touched != 0.0
        _REF[which]["touched", True] = O.blocks_to_row_order(orp, touched) != 0.0
    return _REF[which]


# ---------------------------------------------------------------- the kernel entry
@pytest.mark.parametrize("which", MESHES)
@pytest.mark.parametrize("use_csr", [False, True])
def test_paraxial_kernel(ctx, which, use_csr):
    """Measured worst over the 8 cases: values 3.6e-16, RHS 2.7e-16 of max."""
    r = _ref(ctx, which)
    mesh, faces, fixed, p = r["mesh"], r["faces"], r["fixed"], r["p"]
    n2 = 2 * mesh.n_own_nodes
    bsr = af.BSRFormat(mesh, 2).initialize(use_csr)
    bsr.computeSparsity()
    rows, cols, _ = bsr.download()
    assert np.array_equal(rows, r["orp"]) and np.array_equal(cols, r["ocols"])
    dev = _Dev(ctx)
    dU, dV, dA = dev.put(r["U"]), dev.put(r["V"]), dev.put(r["A"])
    dfix = dev.put(fixed.astype(np.uint8))
    drhs = dev.put(np.zeros(n2))

    def run(fc, fill=None, reset=True, fix=dfix):
        if reset:
            bsr.resetMatrixValues()
        ctx.to_device(drhs, np.zeros(n2) if fill is None else fill)
        bsr.addParaxialP1(fc, CP, CS, p, dU, dV, dA, fix, drhs)
        return bsr.download()[2], ctx.to_host(drhs, n2, np.float64)

    # from zero: the paraxial LHS and RHS themselves
    vals, rhs = run(faces)
    ovals = O.blocks_to_row_order(r["orp"], np.array(r["lhs"])) if use_csr else r["lhs"]
    ev, er = _rel(vals, ovals), _rel(rhs, r["rhs"])
    print(f"{which} csr={use_csr}: values {ev:.2e}, rhs {er:.2e} of max (gate {VAL_TOL:.0e})")
    assert ev <= VAL_TOL and er <= VAL_TOL
    assert np.all(rhs[fixed] == 0.0) and np.abs(r["rhs"]).max() > 0
    assert np.all(vals[~r["touched", use_csr]] == 0.0)
    # two runs: bit for bit
    vals2, rhs2 = run(faces)
    assert np.array_equal(vals, vals2) and np.array_equal(rhs, rhs2)
    # on a prefilled matrix and RHS: prefill + the result above, bit for bit -- the untouched values and the
    # fixed DoFs keep their bits
    bsr.assembleElasticityP1(LAM, MU2)
    before = bsr.download()[2]
    prefill = np.random.default_rng(9).standard_normal(n2)
    vals3, rhs3 = run(faces, fill=prefill, reset=False)
    untouched = ~r["touched", use_csr]
    assert untouched.any() and (~untouched).any()
    assert np.array_equal(vals3[untouched].view(np.uint64), before[untouched].view(np.uint64))
    # (the touched ones at VAL_TOL: the kernel's `+=` of a product is one fused multiply-add on the old value)
    assert _rel(vals3, before + vals) <= VAL_TOL
    assert np.array_equal(rhs3[fixed].view(np.uint64), prefill[fixed].view(np.uint64))
    assert np.array_equal(rhs3, prefill + rhs)
    # no mask: the flagged DoFs get their terms too, the others do not change
    _, rhs4 = run(faces, fix=None)
    assert np.array_equal(rhs4[~fixed], rhs[~fixed])
    on_boundary = np.zeros(n2, dtype=bool)
    own = np.unique(faces[faces < mesh.n_own_nodes])
    on_boundary[2 * own], on_boundary[2 * own + 1] = True, True
    assert np.abs(rhs4[fixed & on_boundary]).min() > 0
    # an edge listed twice counts twice: one call with the longer list against two calls
    twice = np.concatenate([faces, faces[:3]])
    va, ra = run(twice)
    run(faces)
    bsr.addParaxialP1(faces[:3], CP, CS, p, dU, dV, dA, dfix, drhs)
    vb, rb = bsr.download()[2], ctx.to_host(drhs, n2, np.float64)
    assert _rel(va, vb) <= VAL_TOL and _rel(ra, rb) <= VAL_TOL and np.abs(va - vals).max() > 0
    dev.free()
    bsr.close()


def test_paraxial_other_combinations_keep_their_error(ctx):
    for dim, k in ((2, 1), (3, 1), (3, 3)):
        mesh = af.Mesh.structured(ctx, dim, 4)
        bsr = af.BSRFormat(mesh, k).initialize(True)
        bsr.computeSparsity()
        d = ctx.malloc(8 * 3 * mesh.n_nodes)
        with pytest.raises(af.AfemError) as e:
            bsr.addParaxialP1(np.array([[0, 1]]), CP, CS, (1.0, 1.0, 1.0), d, d, d, None, d)
        assert e.value.code == 3  # AFEM_ERR_NOT_IMPL
        ctx.free(d)
    # an edge that is no edge of the mesh, a node id out of range
    mesh = af.Mesh.structured(ctx, 2, 4)
    bsr = af.BSRFormat(mesh, 2).initialize(True)
    bsr.computeSparsity()
    d = ctx.malloc(8 * 2 * mesh.n_nodes)
    for bad in ([[0, mesh.n_nodes - 1]], [[0, mesh.n_nodes]], [[3, 3]]):
        with pytest.raises(af.AfemError) as e:
            bsr.addParaxialP1(np.array(bad), CP, CS, (1.0, 1.0, 1.0), d, d, d, None, d)
        assert e.value.code == 1  # AFEM_ERR_ARG
    ctx.free(d)


# ---------------------------------------------------------------- the time loop
def _sim(ctx, gm, deck, solver, mesh=None, cls=None, **over):
    d = dict(deck, **over)
    mesh = mesh or af.Mesh.from_arrays(ctx, 2, gm.cells, gm.coords)
    mat = {k: d[k] for k in ("cp", "cs", "lam", "mu", "E", "nu") if d[k] is not None}
    sim = (cls or af.Soildynamics2D)(ctx, mesh, d["rho"], d["dt"], body_force=d["f"], alpm=d["alpm"], alpf=d["alpf"],
                                     time_discretization=d["scheme"], enforce_dirichlet_method=d["method"],
                                     penalty=d["penalty"], rtol=1e-15, max_iter=50000, solver=solver, **mat)
    for g in d["paraxial"]:
        sim.setParaxial(gm.group_faces(g))
    for group, t, tab in d["traction"]:
        sim.setTraction(gm.group_faces(group), t, table=R.read_table(path(tab)) if tab else None)
    for group, u in d["dirichlet"] + d["points"]:
        sim.setDirichlet(gm.group_nodes(group), u)
    for n, s, e, w, tab in d["double_couple"]:
        sim.setDoubleCouple(gm.group_nodes(n), gm.group_nodes(s), gm.group_nodes(e), gm.group_nodes(w),
                            table=S.read_force_table(path(tab)))
    return sim, mesh


@pytest.mark.parametrize("deck", list(DECKS))
@pytest.mark.parametrize("solver", ["direct", "pcg"])
def test_decks(ctx, deck, solver):
    """Measured worst fractions of the gates over the ten cases: U 3.1e-3, V 4.4e-4, A 2.5e-4."""
    d = DECKS[deck]
    gm = _gm(d["mesh"])
    sim, mesh = _sim(ctx, gm, d, solver)
    L = S.deck_loop(gm, d, path)
    dofs, values = R.deck_constraints(gm, d)
    fu, fv, fa = _run_against(sim, L, S.steps(d), dofs, values)
    print(f"{deck} [{solver}]: {S.steps(d)} steps, error / gate U {fu:.2e}, V {fv:.2e}, A {fa:.2e}; "
          f"last solve {sim.last_stats['iterations']} iterations")
    U = sim.state_host()[0]
    sim.close()
    assert fu <= 1.0 and fv <= 1.0 and fa <= 1.0
    if deck in GOLDEN:  # the module's own check of its result file (:1630-1638)
        g = S.golden_compare(U, read_node_result_file(path(GOLDEN[deck])), gm.node_tags)
        print(f"{deck} [{solver}]: golden checker failures {g['nerr']}, max|U - G| / max|G| {g['frac']:.2e}")
        assert g["nerr"] == 0


def test_operators_contain_the_paraxial_terms(ctx):
    d = DECKS["constant-traction.arc"]  # the curved boundary: cross terms
    gm = _gm(d["mesh"])
    sim, mesh = _sim(ctx, gm, d, "pcg")
    sim.step()
    v = sim.operators()["lhs"]
    assert v.block_size == 2 and v.ordered_per_block == 0
    vals, c = ctx.to_host(v.values, 4 * v.nnz_blocks, np.float64), sim.operators()["c"]
    bsr = af.BSRFormat(mesh, 2).initialize(True)
    bsr.computeSparsity()
    dev = _Dev(ctx)
    z = dev.put(np.zeros(2 * gm.n_nodes))
    rhs = dev.put(np.zeros(2 * gm.n_nodes))
    bsr.assembleElastodynamicsP1(c, None, z, z, z, None, rhs)
    rows, cols, kv = bsr.download()
    lam, mu, cp, cs = S.deck_material(d)
    p = S.paraxial_constants(d["rho"], d["dt"])
    ref = O.blocks_to_row_order(rows, S.paraxial_lhs(gm.n_nodes, gm.coords, gm.group_faces("lower"), rows, cols, p[0],
                                                    cp, cs))
    err = np.abs((vals - kv) - ref).max() / np.abs(ref).max()
    print(f"operators: |(LHS - kernel LHS) - paraxial| {err:.2e} of max|paraxial| (gate {VAL_TOL:.0e})")
    assert err <= VAL_TOL
    touched = ref != 0.0
    assert np.array_equal(vals[~touched], kv[~touched])
    sim.close()
    dev.free()
    bsr.close()


def test_set_time_step_mid_run(ctx):
    d = DECKS["double-couple.paraxial.arc"]  # p7 .. p9 and the table's time follow the new dt
    gm = _gm(d["mesh"])
    sim, _ = _sim(ctx, gm, d, "pcg")
    L = S.deck_loop(gm, d, path)
    dofs, values = R.deck_constraints(gm, d)
    fu, fv, fa = _run_against(sim, L, 12, dofs, values, dt_change=(5, 0.004))
    print(f"dt 0.01 -> 0.004 after 5 steps: error / gate U {fu:.2e}, V {fv:.2e}, A {fa:.2e}")
    assert sim.t == pytest.approx(L.t, abs=1e-12) and L.dt == 0.004
    sim.close()
    assert fu <= 1.0 and fv <= 1.0 and fa <= 1.0


@pytest.mark.parametrize("solver", ["direct", "pcg"])
def test_without_paraxial_and_source_it_is_elastodynamics2d(ctx, solver):
    d = DECKS["Soildynamics.arc"]
    gm = _gm(d["mesh"])
    a, _ = _sim(ctx, gm, d, solver)
    b, _ = _sim(ctx, gm, d, solver, cls=af.Elastodynamics2D)
    for _ in range(5):
        a.step()
        b.step()
        for x, y in zip(a.state_host(), b.state_host()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    assert np.abs(a.state_host()[0]).max() > 0
    a.close()
    b.close()


def test_profiled_step_times_the_new_launches_and_changes_nothing(ctx):
    d = DECKS["double-couple.paraxial.arc"]
    gm = _gm(d["mesh"])
    a, _ = _sim(ctx, gm, d, "pcg")
    b, _ = _sim(ctx, gm, d, "pcg")
    a.profile(True)
    for _ in range(3):
        a.step()
        b.step()
        t = a.step_timing()
        # the paraxial launch and the source's assignment are the only work between those events here
        assert t["rhs_ms"] > 0 and t["bc_ms"] >= 0 and t["assemble_ms"] > 0
    for x, y in zip(a.state_host(), b.state_host()):
        assert np.array_equal(x, y)
    a.close()
    b.close()


# ---------------------------------------------------------------- documented errors
def test_documented_errors(ctx):
    d = DECKS["double-couple.paraxial.arc"]
    gm = _gm(d["mesh"])
    mesh = af.Mesh.from_arrays(ctx, 2, gm.cells, gm.coords)
    faces = np.ascontiguousarray(gm.group_faces("left"), dtype=np.int32)
    north = np.ascontiguousarray(gm.group_nodes("sourceT"), dtype=np.int32)
    t, f = S.read_force_table(path(d["double_couple"][0][4]))

    def c_entries(h):
        yield "afem_elastodynamics_set_wave_speeds", (h, 4.0, 2.0)
        yield "afem_elastodynamics_set_paraxial", (h, ctypes.c_void_p(faces.ctypes.data), faces.shape[0], C.AFEM_MEM_HOST)
        yield "afem_elastodynamics_set_double_couple", (h, ctypes.c_void_p(north.ctypes.data), north.size, None, 0, None,
                                                        0, None, 0, ctypes.c_void_p(t.ctypes.data),
                                                        ctypes.c_void_p(f.ctypes.data), t.size, C.AFEM_MEM_HOST)

    # a 3D handle
    sim3 = af.Elastodynamics3D(ctx, af.Mesh.structured(ctx, 3, 3), 1.0e3, 0.3, 1.0, 0.01)
    for name, args in c_entries(sim3.h):
        with pytest.raises(af.AfemError) as e:
            C.call(name, *args)
        assert e.value.code == 3, name
    sim3.close()
    with pytest.raises(ValueError):
        af.Soildynamics2D(ctx, af.Mesh.structured(ctx, 3, 3), 1.0, 0.01, cp=4.0, cs=2.0)
    # damping, generalized-alpha: the module's own FATAL
    for kw in (dict(etak=0.01), dict(etam=0.01), dict(time_discretization="Generalized-alpha", alpm=0.2, alpf=0.4)):
        sim = af.Elastodynamics2D(ctx, mesh, 1.0, 0.01, lam=8.0, mu=4.0, **kw)
        for name, args in list(c_entries(sim.h))[1:]:
            with pytest.raises(af.AfemError) as e:
                C.call(name, *args)
            assert e.value.code == 3, (name, kw)
        sim.close()
    sim = af.Soildynamics2D(ctx, mesh, 1.0, 0.01, cp=4.0, cs=2.0, etak=0.01)
    with pytest.raises(af.AfemError) as e:
        sim.setParaxial(faces)
    assert e.value.code == 3
    sim.close()
    with pytest.raises(ValueError, match="Only Newmark-beta works"):
        af.Soildynamics2D(ctx, mesh, 1.0, 0.01, cp=4.0, cs=2.0, time_discretization="Generalized-alpha")
    with pytest.raises(ValueError):
        af.Soildynamics2D(ctx, mesh, 1.0, 0.01, cp=4.0, cs=2.0, time_discretization="Euler")
    # a double couple on a constrained DoF, registered in either order: refused when the step runs
    for first in ("dirichlet", "source"):
        sim = af.Soildynamics2D(ctx, mesh, 1.0, 0.01, cp=4.0, cs=2.0, enforce_dirichlet_method="RowElimination")
        for what in (("dirichlet", "source") if first == "dirichlet" else ("source", "dirichlet")):
            if what == "dirichlet":
                sim.setDirichlet(north, (0.0, None))
            else:
                sim.setDoubleCouple(north, [], [], [], table=(t, f))
        with pytest.raises(af.AfemError) as e:
            sim.step()
        assert e.value.code == 1
        sim.close()
    # the other component of the same node is free to be constrained
    sim = af.Soildynamics2D(ctx, mesh, 1.0, 0.01, cp=4.0, cs=2.0, enforce_dirichlet_method="RowElimination")
    sim.setDirichlet(north, (None, 0.0))
    sim.setDoubleCouple(north, [], [], [], table=(t, f))
    sim.step()
    sim.close()
    # the material: exactly one pair
    for kw in (dict(), dict(cp=4.0), dict(cp=4.0, cs=2.0, lam=8.0, mu=4.0), dict(lam=8.0, mu=4.0, E=1.0, nu=0.3),
               dict(cp=4.0, cs=2.0, E=1.0, nu=0.3)):
        with pytest.raises(ValueError):
            af.Soildynamics2D(ctx, mesh, 1.0, 0.01, **kw)
