"""CPU restatement (numpy, float64) of the reference's 2D elastodynamics module
(modules/elastodynamics/FemModule.cc; TRIA3, block 2), on top of the oracle and
of elasticity2d_ref.py, which the elasticity goldens pin: the checker of
test_elastodynamics2d_ref.py and of test_gpu_elastodynamics2d.py.

  * LHS = O.assemble_elasticity_tri(c1, c2) + c0 x mass_blocks (:1130-1340);
  * the right-hand side twice: `rhs_cell_loop`, the module's loops as written
    (body force :645-669, cell loop over U, V, A :671-867, with the
    m_u1_fixed / m_u2_fixed and isOwn() guards), and `rhs_operators`,
    M Wm + K_lambda Wl + K_mu Wu from the pinned operators;
  * tractions t_i |e| / 2 per face node on unfixed owned DoFs (:880-967) and
    the CaseTable of a traction-input-file (piecewise linear, constant outside;
    CaseTable::CurveLinear, femutils/FemUtils.cc:175-220: rows t, t1, t2, t3);
  * the time loop: t = dt, 2 dt, ... (:175, :189), exact reduced solves (the
    constrained values exact, what Penalty 1e64 / RowElimination /
    RowColumnElimination + the re-imposition of :1416-1417 all give) and the
    update _updateVariables (:429-455).
"""
import numpy as np

from oracle import oracle as O

import elasticity2d_ref as R2


def scheme_name(deck_scheme):
    return deck_scheme.lower()


def constants(lam, mu, rho, dt, etam=0.0, etak=0.0, alpm=0.0, alpf=0.0, scheme="newmark-beta"):
    """gamma, beta, c0 .. c10 (FemModule.cc:255-290, the oracle's restatement)."""
    return O.elastodynamics_constants(lam, mu, rho, dt, etam, etak, alpm, alpf, scheme_name(scheme))


def deck_constants(deck, dt=None):
    return constants(deck["lam"], deck["mu"], deck["rho"], deck["dt"] if dt is None else dt, deck["etam"],
                     deck["etak"], deck["alpm"], deck["alpf"], deck["scheme"])


def steps(deck):
    """Steps the module's time loop takes: compute() runs at t and stops once
    t >= tmax - dt (startInit :175-176, compute :144-145, _updateTime :189)."""
    t, tmax, n = deck["dt"], deck["tmax"] - deck["dt"], 0
    while True:
        n += 1
        if t >= tmax:
            return n
        t += deck["dt"]


# ---------------------------------------------------------------- CaseTable
def read_table(path):
    """(times[n], values[n, 2]) of a traction-input-file: rows of t, t1, t2, t3."""
    a = np.loadtxt(path, dtype=np.float64).reshape(-1, 4)
    return a[:, 0].copy(), a[:, 1:3].copy()


def interp_table(times, values, t):
    """CaseTable::CurveLinear: linear between the table's times, constant outside."""
    if t <= times[0]:
        return values[0].copy()
    if t >= times[-1]:
        return values[-1].copy()
    k = int(np.searchsorted(times, t, side="right"))  # times[k-1] <= t < times[k]
    w = (t - times[k - 1]) / (times[k] - times[k - 1])
    return values[k - 1] + w * (values[k] - values[k - 1])


# ---------------------------------------------------------------- right-hand side
def rhs_cell_loop(n_own, cells, coords, c, f, U, V, A, fixed=None):
    """The module's body-force loops and cell loop, cell by cell in cell order.
    U, V, A: 2 per local node; fixed: bool per owned DoF (m_u1_fixed / m_u2_fixed)."""
    cells = np.asarray(cells)
    xy = np.asarray(coords, dtype=np.float64)[:, :2]
    fx = [0.0 if x is None else float(x) for x in (f if f is not None else (None, None))]
    fixed = np.zeros(2 * n_own, dtype=bool) if fixed is None else np.asarray(fixed, dtype=bool)
    rhs = np.zeros(2 * n_own)
    U2, V2, A2 = (np.asarray(x, dtype=np.float64).reshape(-1, 2) for x in (U, V, A))
    for cell in cells:
        m0, m1, m2 = xy[cell[0]], xy[cell[1]], xy[cell[2]]
        area = 0.5 * abs((m1[0] - m0[0]) * (m2[1] - m0[1]) - (m2[0] - m0[0]) * (m1[1] - m0[1]))
        for comp in range(2):
            for v in cell:
                if v < n_own and not fixed[2 * v + comp]:
                    rhs[2 * v + comp] += fx[comp] * area / 3
        dphi = np.array([[m1[1] - m2[1], m2[0] - m1[0]], [m2[1] - m0[1], m0[0] - m2[0]], [m0[1] - m1[1], m1[0] - m0[0]]])
        DXV, DYV = dphi[:, 0] / (2. * area), dphi[:, 1] / (2. * area)

        def grads(W):  # (sum of the nodal values, d/dx, d/dy) of both components
            w = W[cell]
            return w.sum(0), DXV @ w, DYV @ w

        (Uo, DXU, DYU), (Vo, DXVv, DYVv), (Ao, DXA, DYA) = grads(U2), grads(V2), grads(A2)
        for i, v in enumerate(cell):
            if v >= n_own:
                continue
            if not fixed[2 * v]:
                rhs[2 * v] += ((Uo[0] + U2[v, 0]) * (area / 12.) * c[0] + (Vo[0] + V2[v, 0]) * (area / 12.) * c[3]
                               + (Ao[0] + A2[v, 0]) * (area / 12.) * c[4]
                               - ((DXU[0] + DYU[1]) * DXV[i] * area) * c[5]
                               - ((DXU[0] * DXV[i] * area) + 0.5 * (DYU[0] + DXU[1]) * DYV[i] * area) * c[6]
                               + ((DXVv[0] + DYVv[1]) * DXV[i] * area) * c[7]
                               + ((DXVv[0] * DXV[i] * area) + 0.5 * (DYVv[0] + DXVv[1]) * DYV[i] * area) * c[9]
                               + ((DXA[0] + DYA[1]) * DXV[i] * area) * c[8]
                               + ((DXA[0] * DXV[i] * area) + 0.5 * (DYA[0] + DXA[1]) * DYV[i] * area) * c[10])
            if not fixed[2 * v + 1]:
                rhs[2 * v + 1] += ((Uo[1] + U2[v, 1]) * (area / 12.) * c[0] + (Vo[1] + V2[v, 1]) * (area / 12.) * c[3]
                                   + (Ao[1] + A2[v, 1]) * (area / 12.) * c[4]
                                   - ((DXU[0] + DYU[1]) * DYV[i] * area) * c[5]
                                   - ((DYU[1] * DYV[i] * area) + 0.5 * (DYU[0] + DXU[1]) * DXV[i] * area) * c[6]
                                   + ((DXVv[0] + DYVv[1]) * DYV[i] * area) * c[7]
                                   + ((DYVv[1] * DYV[i] * area) + 0.5 * (DYVv[0] + DXVv[1]) * DXV[i] * area) * c[9]
                                   + ((DXA[0] + DYA[1]) * DYV[i] * area) * c[8]
                                   + ((DYA[1] * DYV[i] * area) + 0.5 * (DYA[0] + DXA[1]) * DXV[i] * area) * c[10])
    return rhs


def traction_rhs(n_own, coords, faces, t, fixed=None):
    """t_i |e| / 2 to both nodes of every edge, owned and unfixed DoFs (:899-963)."""
    xy = np.asarray(coords, dtype=np.float64)[:, :2]
    fixed = np.zeros(2 * n_own, dtype=bool) if fixed is None else np.asarray(fixed, dtype=bool)
    rhs = np.zeros(2 * n_own)
    for a, b in np.asarray(faces):
        length = np.hypot(*(xy[a] - xy[b]))
        for v in (a, b):
            for i in range(2):
                if t[i] is not None and v < n_own and not fixed[2 * v + i]:
                    rhs[2 * v + i] += float(t[i]) * length / 2.
    return rhs


class Operators:
    """Structure, K_lambda (lambda = 1, 2 mu = 0), K_mu (0, 1) and the unit
    consistent mass of a mesh, per block (the pinned oracle / elasticity2d_ref
    routines), and their dense forms on a mesh without ghosts."""

    def __init__(self, n_nodes, n_own, cells, coords):
        self.n_nodes, self.n_own, self.cells, self.coords = n_nodes, n_own, np.asarray(cells), np.asarray(coords)
        self.orp, self.ocols = O.sparsity(n_nodes, n_own, cells)
        asm = lambda lam, mu2: O.assemble_elasticity_tri(n_own, cells, coords, self.orp, self.ocols, lam, mu2)  # noqa: E731
        self.Kl, self.Km = asm(1.0, 0.0), asm(0.0, 1.0)
        self.M = R2.mass_blocks(n_own, cells, coords, self.orp, self.ocols, 1.0)
        for a in (self.orp, self.ocols, self.Kl, self.Km, self.M):
            a.setflags(write=False)
        self._dense = {}

    def lhs_blocks(self, c):
        """c0 M + K(c1, c2) per block, K by the oracle's own assembly."""
        return O.assemble_elasticity_tri(self.n_own, self.cells, self.coords, self.orp, self.ocols, c[1],
                                         c[2]) + c[0] * self.M

    def dense(self, blocks):
        return O.csr_to_dense(*R2.scalar_csr(self.orp, self.ocols, np.array(blocks)), n_cols=2 * self.n_nodes)

    def dense_of(self, name):
        if name not in self._dense:
            self._dense[name] = self.dense(getattr(self, name))
        return self._dense[name]


def rhs_operators(ops, c, f, U, V, A, fixed=None):
    """Body force + M Wm + K_lambda Wl + K_mu Wu, fixed DoFs zeroed."""
    U, V, A = (np.asarray(x, dtype=np.float64) for x in (U, V, A))
    Wm = c[0] * U + c[3] * V + c[4] * A
    Wl = -c[5] * U + c[7] * V + c[8] * A
    Wu = -c[6] * U + c[9] * V + c[10] * A
    rhs = (R2.body_force_rhs(ops.n_own, ops.cells, ops.coords, f if f is not None else (None, None))
           + ops.dense_of("M") @ Wm + ops.dense_of("Kl") @ Wl + ops.dense_of("Km") @ Wu)
    if fixed is not None:
        rhs[np.asarray(fixed, dtype=bool)] = 0.0
    return rhs


# ---------------------------------------------------------------- the time loop
def newmark_update(U, V, A, dU, dt, beta, gamma):
    """_updateVariables (:429-455); returns the new (U, V, A)."""
    a = (dU - U - dt * V) / beta / (dt * dt) - (1. - 2. * beta) / 2. / beta * A
    v = V + dt * ((1. - gamma) * A + gamma * a)
    return dU.copy(), v, a


def deck_constraints(gm, deck):
    """(dofs, values) of the deck's Dirichlet blocks, later blocks overriding earlier ones."""
    return R2.deck_constraints(gm, deck)


class Loop:
    """The module's time loop on a mesh without ghosts, with exact reduced solves."""

    def __init__(self, n_nodes, cells, coords, lam, mu, rho, dt, etam=0.0, etak=0.0, alpm=0.0, alpf=0.0,
                 scheme="newmark-beta", f=(None, None), dofs=(), values=(), tractions=(), gamma=None):
        self.ops = Operators(n_nodes, n_nodes, cells, coords)
        self.par = dict(lam=lam, mu=mu, rho=rho, etam=etam, etak=etak, alpm=alpm, alpf=alpf, scheme=scheme)
        self.f = f
        self.dofs, self.values = np.asarray(dofs, dtype=np.int64), np.asarray(values, dtype=np.float64)
        self.fixed = np.zeros(2 * n_nodes, dtype=bool)
        self.fixed[self.dofs] = True
        self.tractions = list(tractions)  # (faces, t, table or None)
        self.gamma_override = gamma  # mutation check of the energy test only
        n = 2 * n_nodes
        self.U, self.V, self.A = np.zeros(n), np.zeros(n), np.zeros(n)
        self.t = dt
        self.setTimeStep(dt)

    def setTimeStep(self, dt):
        self.dt = dt
        self.gamma, self.beta, self.c = constants(dt=dt, **self.par)
        if self.gamma_override is not None:
            self.gamma = self.gamma_override
        self.lhs = self.ops.dense(self.ops.lhs_blocks(self.c))

    def rhs(self):
        o = self.ops
        b = rhs_cell_loop(o.n_own, o.cells, o.coords, self.c, self.f, self.U, self.V, self.A, self.fixed)
        for faces, t, table in self.tractions:
            tv = tuple(interp_table(table[0], table[1], self.t)) if table is not None else t
            b += traction_rhs(o.n_own, o.coords, faces, tv, self.fixed)
        return b

    def step(self):
        dU = R2.reduced_solve(self.lhs, self.rhs(), self.dofs, self.values)
        self.U, self.V, self.A = newmark_update(self.U, self.V, self.A, dU, self.dt, self.beta, self.gamma)
        self.t += self.dt
        return self.U


def deck_loop(gm, deck, table_path=None):
    """The Loop of a deck of elastodynamics2d_cases.py (table_path: where its traction tables are)."""
    dofs, values = deck_constraints(gm, deck)
    tractions = [(gm.group_faces(g), t, read_table(table_path(tab)) if tab else None) for g, t, tab in deck["traction"]]
    return Loop(gm.n_nodes, gm.cells, gm.coords, deck["lam"], deck["mu"], deck["rho"], deck["dt"], deck["etam"],
                deck["etak"], deck["alpm"], deck["alpf"], deck["scheme"], deck["f"], dofs, values, tractions)


def energy(ops, lam, mu, rho, U, V):
    """1/2 V^T M V + 1/2 U^T K U with M = rho x the unit mass, K = K(lam, 2 mu)."""
    K = lam * ops.dense_of("Kl") + 2 * mu * ops.dense_of("Km")
    return 0.5 * rho * V @ (ops.dense_of("M") @ V) + 0.5 * U @ (K @ U)
