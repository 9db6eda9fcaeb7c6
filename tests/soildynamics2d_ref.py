"""CPU restatement (numpy, float64) of the reference's soildynamics module
(modules/soildynamics/FemModule.cc; TRIA3, block 2), on top of
elastodynamics2d_ref.py: the checker of test_soildynamics2d_ref.py (against the
module's golden files) and of test_gpu_soildynamics2d.py (against the GPU).

  * material (:261-280): cp, cs (mu = cs^2 rho, lambda = cp^2 rho - 2 mu), or
    lambda, mu, or E, nu (then cs = sqrt(mu / rho), cp = sqrt((lambda + 2 mu) / rho));
  * constants (:283-300): Newmark-beta, gamma = 1/2, beta = 1/4; c0 .. c4 are
    the elastodynamics module's undamped values, c5 .. c10 of the cell loop are
    zero; the module's c7 .. c9 are the PARAXIAL constants, kept apart here as
    p7 = rho gamma / (beta dt), p8 = rho (1 - gamma / beta),
    p9 = rho dt (1 - gamma / (2 beta));
  * cell loop and LHS: elastodynamics2d_ref's (rhs_cell_loop, Operators);
  * paraxial LHS: the EDGE2 element matrix (:1376-1486) assembled on owned rows
    (:1540-1577); paraxial RHS: the edge loop over U, V, A (:870-936);
  * double couple (:946-987): after everything else rhs[2 north] = F,
    rhs[2 south] = -F, rhs[2 east + 1] = -F, rhs[2 west + 1] = F, F the
    one-column CaseTable at the step's time;
  * the time loop (:454-480, :150-180): t = dt, 2 dt, ...; exact reduced
    solves; the update of elastodynamics2d_ref.newmark_update.
"""
import numpy as np

from oracle import oracle as O

import elastodynamics2d_ref as R
from elastodynamics2d_ref import (Operators, interp_table, newmark_update, rhs_cell_loop,  # noqa: F401
                                  traction_rhs)
from elasticity2d_ref import reduced_solve  # noqa: F401

CHECK_EPSILON = 1.0e-4  # _checkResultFile, :1636


def material(rho, cp=None, cs=None, lam=None, mu=None, E=None, nu=None):
    """(lambda, mu, cp, cs) of :261-280."""
    if E is not None:
        mu = E / (2 * (1 + nu))
        lam = E * nu / ((1 + nu) * (1 - 2 * nu))
    if cp is not None:
        mu = cs * cs * rho
        lam = cp * cp * rho - 2 * mu
    else:
        cs = np.sqrt(mu / rho)
        cp = np.sqrt((lam + (2. * mu)) / rho)
    return float(lam), float(mu), float(cp), float(cs)


def deck_material(deck):
    return material(deck["rho"], deck["cp"], deck["cs"], deck["lam"], deck["mu"], deck["E"], deck["nu"])


def paraxial_constants(rho, dt, gamma=0.5, beta=0.25):
    """The module's c7, c8, c9 (:297-299)."""
    return rho * gamma / beta / dt, rho * (1. - gamma / beta), rho * dt * (1. - gamma / (2. * beta))


def steps(deck):
    """Steps of a run: compute() solves at t, updates t += dt and ends the run
    with the first step whose updated time exceeds tmax + dt - 1e-8 (:173-179)."""
    t, n = deck["dt"], 0
    while True:
        n += 1
        t += deck["dt"]
        if t > deck["tmax"] + deck["dt"] - 1e-8:
            return n


def read_force_table(path):
    """(times[n], values[n]) of a double-couple-input-file: rows of t, F."""
    a = np.loadtxt(path, dtype=np.float64).reshape(-1, 2)
    return a[:, 0].copy(), a[:, 1].copy()


def interp_force(times, values, t):
    return float(interp_table(times, values.reshape(-1, 1), t)[0])


def edge_geometry(coords, a, b):
    """Length and unit normal of edge (a, b); only nx^2, ny^2 and nx ny are used."""
    xy = np.asarray(coords, dtype=np.float64)[:, :2]
    d = xy[b] - xy[a]
    length = np.hypot(d[0], d[1])
    return length, d[1] / length, -d[0] / length


def paraxial_lhs(n_own, coords, faces, row_ptr, cols, p7, cp, cs):
    """The EDGE2 element matrices of `faces` on the owned rows, per block
    (4 values per block of the structure, like O.assemble_elasticity_tri)."""
    vals = np.zeros(4 * cols.shape[0])
    slot = {}
    for r in range(n_own):
        for k in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            slot[(r, int(cols[k]))] = k
    for a, b in np.asarray(faces).reshape(-1, 2):
        a, b = int(a), int(b)
        L, nx, ny = edge_geometry(coords, a, b)
        k11 = p7 * (nx * nx * cp + ny * ny * cs)
        k22 = p7 * (ny * ny * cp + nx * nx * cs)
        k12 = p7 * (nx * ny * (cp - cs))
        for i in (a, b):
            if i >= n_own:
                continue
            for j in (a, b):
                m = L / 3 if i == j else L / 6
                k = slot[(i, j)]
                vals[4 * k] += k11 * m
                vals[4 * k + 3] += k22 * m
                vals[4 * k + 1] += k12 * L / 6  # the cross terms carry L/6 on the diagonal block too (:1445-1483)
                vals[4 * k + 2] += k12 * L / 6
    return vals


def paraxial_rhs(n_own, coords, faces, p, cp, cs, U, V, A, fixed=None):
    """The paraxial edge loop (:875-935) as written: owned, unfixed DoFs."""
    p7, p8, p9 = p
    fixed = np.zeros(2 * n_own, dtype=bool) if fixed is None else np.asarray(fixed, dtype=bool)
    U2, V2, A2 = (np.asarray(x, dtype=np.float64).reshape(-1, 2) for x in (U, V, A))
    rhs = np.zeros(2 * n_own)
    for a, b in np.asarray(faces).reshape(-1, 2):
        a, b = int(a), int(b)
        L, nx, ny = edge_geometry(coords, a, b)
        old = [W[a] + W[b] for W in (U2, V2, A2)]
        for v in (a, b):
            if v >= n_own:
                continue
            S = [o + W[v] for o, W in zip(old, (U2, V2, A2))]

            def f1(s):
                return cp * (nx * nx * s[0] + nx * ny * s[1]) + cs * (ny * ny * s[0] - nx * ny * s[1])

            def f2(s):
                return cp * (nx * ny * s[0] + ny * ny * s[1]) + cs * (-nx * ny * s[0] + nx * nx * s[1])

            if not fixed[2 * v]:
                rhs[2 * v] += (p7 * f1(S[0]) - p8 * f1(S[1]) - p9 * f1(S[2])) * L / 6.
            if not fixed[2 * v + 1]:
                rhs[2 * v + 1] += (p7 * f2(S[0]) - p8 * f2(S[1]) - p9 * f2(S[2])) * L / 6.
    return rhs


def double_couple_assign(rhs, north, south, east, west, F, flip_east_west=False):
    """:966-985, in place."""
    s = -1.0 if flip_east_west else 1.0
    rhs[2 * np.asarray(north, dtype=np.int64)] = F
    rhs[2 * np.asarray(south, dtype=np.int64)] = -F
    rhs[2 * np.asarray(east, dtype=np.int64) + 1] = -F * s
    rhs[2 * np.asarray(west, dtype=np.int64) + 1] = F * s
    return rhs


class Loop(R.Loop):
    """The module's time loop on a mesh without ghosts, with exact reduced solves.
    paraxial: one face array per block; double_couples: (north, south, east,
    west, (times, values)) per block.  The drop_* / flip_* switches are the
    mutations of test_soildynamics2d_ref.py."""

    def __init__(self, n_nodes, cells, coords, rho, dt, cp=None, cs=None, lam=None, mu=None, E=None, nu=None,
                 f=(None, None), dofs=(), values=(), tractions=(), paraxial=(), double_couples=(),
                 drop_paraxial_lhs=False, drop_paraxial_rhs=False, flip_east_west=False):
        self.rho = rho
        self.lam, self.mu, self.cp, self.cs = material(rho, cp, cs, lam, mu, E, nu)
        self.par_faces = (np.concatenate([np.asarray(x).reshape(-1, 2) for x in paraxial]) if len(paraxial)
                          else np.zeros((0, 2), dtype=np.int32))
        self.double_couples = list(double_couples)
        self.drop_paraxial_lhs, self.drop_paraxial_rhs = drop_paraxial_lhs, drop_paraxial_rhs
        self.flip_east_west = flip_east_west
        super().__init__(n_nodes, cells, coords, self.lam, self.mu, rho, dt, f=f, dofs=dofs, values=values,
                         tractions=tractions)

    def paraxial_blocks(self):
        o = self.ops
        return paraxial_lhs(o.n_own, o.coords, self.par_faces, o.orp, o.ocols, self.p[0], self.cp, self.cs)

    def setTimeStep(self, dt):
        super().setTimeStep(dt)
        assert all(x == 0.0 for x in self.c[5:])
        self.p = paraxial_constants(self.rho, dt, self.gamma, self.beta)
        if len(self.par_faces) and not self.drop_paraxial_lhs:
            self.lhs = self.lhs + self.ops.dense(self.paraxial_blocks())

    def rhs(self):
        o = self.ops
        b = super().rhs()  # cell loop + tractions
        if len(self.par_faces) and not self.drop_paraxial_rhs:
            b += paraxial_rhs(o.n_own, o.coords, self.par_faces, self.p, self.cp, self.cs, self.U, self.V, self.A,
                              self.fixed)
        for north, south, east, west, (times, values) in self.double_couples:
            double_couple_assign(b, north, south, east, west, interp_force(times, values, self.t),
                                 self.flip_east_west)
        return b


def deck_loop(gm, deck, table_path, **mutations):
    """The Loop of a deck of soildynamics2d_cases.py (table_path: where its tables are)."""
    dofs, values = R.deck_constraints(gm, deck)
    tractions = [(gm.group_faces(g), t, R.read_table(table_path(tab)) if tab else None)
                 for g, t, tab in deck["traction"]]
    dcs = [(gm.group_nodes(n), gm.group_nodes(s), gm.group_nodes(e), gm.group_nodes(w),
            read_force_table(table_path(tab))) for n, s, e, w, tab in deck["double_couple"]]
    return Loop(gm.n_nodes, gm.cells, gm.coords, deck["rho"], deck["dt"], deck["cp"], deck["cs"], deck["lam"],
                deck["mu"], deck["E"], deck["nu"], deck["f"], dofs, values, tractions,
                [gm.group_faces(g) for g in deck["paraxial"]], dcs, **mutations)


def golden_compare(U, gold, node_tags):
    """U (2 per node, in mesh order) against a golden file (uid -> x, y, z):
    the reference checker's failures at CHECK_EPSILON (per component, Arcane's
    isNearlyEqualWithEpsilon, femutils/FemUtils.cc:84-102), max|U - G| /
    max|G|, and the worst relative error on the entries above 1e-3 max|G|."""
    g = np.array([gold[int(t)][:2] for t in node_tags]).ravel()
    U = np.asarray(U)
    nerr = 0
    for comp in range(2):
        e, _ = O.check_node_result({int(t): v for t, v in zip(node_tags, U[comp::2])},
                                   {int(t): gold[int(t)][comp] for t in node_tags}, CHECK_EPSILON)
        nerr += e
    gmax = np.abs(g).max()
    big = np.abs(g) >= 1e-3 * gmax
    d = np.abs(U - g)
    return dict(nerr=nerr, frac=float(d.max() / gmax), n_small=int((~big).sum()),
                rel_big=float((d[big] / np.abs(g[big])).max()))
