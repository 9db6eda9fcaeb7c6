"""Elastodynamics time stepping on the assembly + CG path: 3D (BASELINE config C5)
and the reference module's own 2D case (Elastodynamics2D, at the end), with the
soil-dynamics module on top of it (Soildynamics2D: paraxial boundaries and a
double-couple source, modules/soildynamics/FemModule.cc).

Thin host mirror of the native time loop behind the C ABI
(``afem_elastodynamics_*``, arcanefem_amd/csrc/elastodynamics.cpp), which
restates the reference's time-stepping callers of the linear-system path:

* ``modules/elastodynamics/FemModule.cc`` (2D TRIA3): Newmark-beta with
  gamma = 1/2, beta = (gamma + 1/2)^2 / 4 (:256-270) or generalized-alpha
  (gamma = 1/2 + alpf - alpm, :275-290), Rayleigh damping etam / etak; LHS
  ``c1 div-div + c2 strain + c0 consistent mass`` (:1130-1340); RHS
  ``M (c0 U + c3 V + c4 A) - K(c5, c6) U + K(c7, c9) V + K(c8, c10) A`` + body
  force (:842-862); state update ``_updateVariables`` (:429-455); the matrix
  re-assembled every step (:149-153).
* ``modules/passmo/ElastodynamicModule.cc`` (3D): re-assembly every step on a
  fixed structure (:469-536).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _capi as C
from ._capi import call
from .core import Context, Mesh


SCHEMES = {"newmark-beta": 0, "generalized-alpha": 1}


def newmark_coefficients(rho: float, dt: float):
    """Newmark-beta constants of modules/elastodynamics/FemModule.cc:255-264
    (etam = etak = 0): returns gamma, beta, c0, c3, c4."""
    gamma = 0.5
    beta = 0.25 * (gamma + 0.5) ** 2
    c0 = rho / (beta * dt * dt)
    c3 = rho / beta / dt
    c4 = rho * ((1.0 - 2.0 * beta) / 2.0 / beta)
    return gamma, beta, c0, c3, c4


def young_from_lame(lam: float, mu: float):
    """(E, nu) of Lame parameters the way passmo converts its "lame" input
    (modules/passmo/ElastodynamicModule.cc:270-277): x = lambda/mu,
    nu = x/2/(1+x), E = 2 mu (1+nu)."""
    x = lam / mu
    nu = x / 2.0 / (1.0 + x)
    return 2.0 * mu * (1.0 + nu), nu


class _Elastodynamics:
    """The native handle and what both loops do with it; a subclass gives NB (DoFs per node) and MESH (dim, word)."""

    def _check(self, mesh: Mesh, time_discretization: str):
        if mesh.dim != self.MESH[0]:
            raise ValueError(f"{type(self).__name__} needs a {self.MESH[1]} mesh")
        if time_discretization.lower() not in SCHEMES:
            raise ValueError("Only Newmark-beta | Generalized-alpha are supported for time-discretization")

    def _open(self, ctx, mesh, E, nu, rho, dt, body_force, penalty, etam, etak, alpm, alpf, time_discretization,
              comm, fixed_nodes, opts, t0):
        """Fills NewmarkParams, creates the handle and sets the solver options; t0: the time of the first step."""
        self.ctx, self.mesh, self.dt, self.t = ctx, mesh, dt, t0
        self.n = self.NB * mesh.n_own_nodes
        self.last_stats = None
        p = C.NewmarkParams(E, nu, rho, dt, (ctypes.c_double * 3)(*[float(x) for x in body_force]), penalty, 0.0, 0.0,
                            etam, etak, alpm, alpf, SCHEMES[time_discretization.lower()], 0)
        fixed = np.ascontiguousarray([] if fixed_nodes is None else fixed_nodes, dtype=np.int32)
        self.h = ctypes.c_void_p()
        call("afem_elastodynamics_create", mesh.h, comm.h if comm is not None else None, ctypes.byref(p),
             ctypes.c_void_p(fixed.ctypes.data) if fixed.size else None, fixed.size, C.AFEM_MEM_HOST,
             ctypes.byref(self.h))
        call("afem_elastodynamics_set_solver_options", self.h, ctypes.byref(opts))

    def step(self) -> dict:
        st = C.SolveStats()
        call("afem_elastodynamics_step", self.h, ctypes.byref(st))
        self.t += self.dt
        self.last_stats = dict(iterations=st.iterations, converged=bool(st.converged), rel_residual=st.rel_residual,
                               residual_norm=st.residual_norm, solve_ms=st.solve_ms, amg_levels=st.amg_levels,
                               amg_setup_ms=st.amg_setup_ms, precond_ms=st.precond_ms)
        return self.last_stats

    def setTimeStep(self, dt: float):
        """dt from the next step on (passmo's shortened final step, :525-530)."""
        call("afem_elastodynamics_set_time_step", self.h, float(dt))
        self.dt = float(dt)

    def profile(self, on: bool = True):
        """Per-phase HIP-event times of every following step (step_timing())."""
        call("afem_elastodynamics_profile", self.h, 1 if on else 0)

    def step_timing(self) -> dict:
        t = C.StepTiming()
        call("afem_elastodynamics_step_timing", self.h, ctypes.byref(t))
        return {f: getattr(t, f) for f, _ in C.StepTiming._fields_ if f != "reserved0"}

    def operators(self):
        """The last step's operators on the device: dict(lhs = CsrView of c0 M +
        K (block 3, CSR-row order), scalar_rows / scalar_cols = device pointers
        of the scalar CSR structure of those values, mass = device pointer of
        the mass values on it, c = the constants c0 .. c10)."""
        v = C.CsrView()
        sr, sc, mp = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        c = (ctypes.c_double * 11)()
        call("afem_elastodynamics_operators", self.h, ctypes.byref(v), ctypes.byref(sr), ctypes.byref(sc),
             ctypes.byref(mp), c)
        return dict(lhs=v, scalar_rows=sr.value, scalar_cols=sc.value, mass=mp.value, c=list(c))

    def state_dptrs(self):
        u, v, a = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        call("afem_elastodynamics_state", self.h, ctypes.byref(u), ctypes.byref(v), ctypes.byref(a))
        return u.value, v.value, a.value

    def state_host(self):
        return tuple(self.ctx.to_host(p, self.n, np.float64) for p in self.state_dptrs())

    def close(self):
        if self.h:
            call("afem_elastodynamics_destroy", self.h)
            self.h = None


class Elastodynamics3D(_Elastodynamics):
    """The same scheme in 3D on P1 tetrahedra with block-3 BSR, on one
    subdomain or on one ghosted z-slab per rank (``comm``: RCCL ``Communicator`` or
    ``parallel.HostCommunicator``): each step re-assembles ``c0 M + K`` and the
    body-force RHS in one fused HIP kernel on the fixed sparsity, adds
    ``M (c0 U + c3 V + c4 A)`` (the mass operator shares the structure; its SpMV
    exchanges the ghost values of the operand), clamps the fixed nodes by
    penalty, solves with the PCG (Jacobi by default, warm started from the
    Newmark predictor; halo + all-reduces over the ranks) and applies the
    Newmark update on the device.  The handle and the step are the base's."""
    NB, MESH = 3, (3, "tetrahedral")

    def __init__(self, ctx: Context, mesh: Mesh, E: float, nu: float, rho: float, dt: float,
                 body_force=(0.0, 0.0, 0.0), fixed_nodes=None, penalty: float = 1.0e30, rtol: float = 1e-12,
                 comm=None, max_iter: int = 20000, preconditioner: str = "jacobi", etam: float = 0.0,
                 etak: float = 0.0, alpm: float = 0.0, alpf: float = 0.0, time_discretization: str = "newmark-beta"):
        """time_discretization, etam, etak, alpm, alpf: the module's
        timeDiscretization and damping options (Fem.axl of
        modules/elastodynamics; FemModule.cc:222-296)."""
        self._check(mesh, time_discretization)
        # "multigrid": the geometric multigrid V-cycle on structured boxes (one rank or z-slabs), built at
        # the first step and reused (the Newmark operator c0 M + K is the same every step)
        # "amg-reuse": the algebraic multigrid (any mesh; rebuilt when dt changes the operator)
        blk, mgm, amg = {"jacobi": (0, 0, 0), "block3": (3, 0, 0), "multigrid": (0, 2, 0),
                         "amg-reuse": (0, 0, 2)}[preconditioner]
        o = C.SolverOpts(C.AFEM_SOLVER_PCG, max_iter, rtol, 0.0, 8, 0, 0, blk, mgm)
        o.amg = amg
        self._open(ctx, mesh, E, nu, rho, dt, body_force, penalty, etam, etak, alpm, alpf, time_discretization, comm,
                   fixed_nodes, o, 0.0)

    def setDirichlet(self, dofs, values):
        """Imposed displacements by penalty (passmo's dirichlet-surface /
        point conditions, modules/passmo/ElastodynamicModule.cc:1923-1939 and
        the re-application after the solve :2369-2371): local DoF ids
        (3 node + component) and their values; replaces the previous list."""
        d = np.ascontiguousarray(dofs, dtype=np.int32).ravel()
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(values, dtype=np.float64), d.shape))
        call("afem_elastodynamics_set_dirichlet", self.h, ctypes.c_void_p(d.ctypes.data) if d.size else None,
             ctypes.c_void_p(v.ctypes.data) if v.size else None, d.size, C.AFEM_MEM_HOST)


DIRICHLET_METHODS = {"penalty": C.AFEM_DIRICHLET_PENALTY, "rowelimination": C.AFEM_DIRICHLET_ROW_ELIMINATION,
                     "rowcolumnelimination": C.AFEM_DIRICHLET_ROW_COLUMN_ELIMINATION, "weakpenalty": -1}


def _mask_values(x):
    """(component mask, 2 doubles) of a tuple whose None entries are the decks' missing components."""
    if len(x) != 2:
        raise ValueError("2 components (None for a component the deck leaves out)")
    return (sum(1 << i for i, c in enumerate(x) if c is not None),
            (ctypes.c_double * 2)(*[0.0 if c is None else float(c) for c in x]))


class Elastodynamics2D(_Elastodynamics):
    """The module modules/elastodynamics itself: TRIA3, block 2, one subdomain.

    Each step is one fused HIP kernel for the LHS c0 M + K(c1, c2) and the
    complete right-hand side (body force + the cell loop over U, V, A,
    FemModule.cc:645-867; no stored M / K operators, no SpMV), the tractions
    (:880-967), the Dirichlet blocks, the solve (Jacobi-PCG, or the direct
    solver: solver="direct", or "auto" below 500 rows), the re-imposition of
    the constrained values (:1416-1417) and the Newmark update (:429-455).
    Material: lam and mu (the decks' lambda / mu, :242-246) or E and nu.
    enforce_dirichlet_method: "Penalty" (the decks give penalty = 1e64),
    "RowElimination" or "RowColumnElimination" (the stated value is imposed;
    "WeakPenalty" is not implemented).
    """
    NB, MESH = 2, (2, "triangle")

    def __init__(self, ctx: Context, mesh: Mesh, rho: float, dt: float, lam: float | None = None,
                 mu: float | None = None, E: float | None = None, nu: float | None = None, body_force=(None, None),
                 etam: float = 0.0, etak: float = 0.0, alpm: float = 0.0, alpf: float = 0.0,
                 time_discretization: str = "newmark-beta", enforce_dirichlet_method: str = "Penalty",
                 penalty: float = 1.0e30, rtol: float = 1e-12, max_iter: int = 20000, solver: str = "pcg",
                 preconditioner: str = "jacobi", comm=None):
        self._check(mesh, time_discretization)
        if preconditioner != "jacobi":
            raise ValueError("Elastodynamics2D solves with the Jacobi-PCG or the direct solver "
                             f"(preconditioner {preconditioner!r} is the 3D loop's)")
        method = enforce_dirichlet_method.lower().replace("-", "")
        if method not in DIRICHLET_METHODS:
            raise ValueError("enforce-Dirichlet-method only supports Penalty, WeakPenalty, RowElimination, "
                             "RowColumnElimination")
        if (lam is None) != (mu is None) or (E is None) != (nu is None) or (lam is None) == (E is None):
            raise ValueError("give the material as lam and mu, or as E and nu")
        self.method = DIRICHLET_METHODS[method]
        if lam is not None:
            E, nu = young_from_lame(lam, mu)
        _, f = _mask_values(body_force)
        o = C.SolverOpts({"auto": C.AFEM_SOLVER_AUTO, "pcg": C.AFEM_SOLVER_PCG, "direct": C.AFEM_SOLVER_DIRECT}[solver],
                         max_iter, rtol, 0.0, 8, 0, 0, 0, 0)
        self._open(ctx, mesh, E, nu, rho, dt, (f[0], f[1], 0.0), penalty, etam, etak, alpm, alpf, time_discretization,
                   comm, None, o, dt)  # t0 = dt: the time of the next step (FemModule.cc:175)
        self.n_tractions = 0
        try:
            if lam is not None:
                call("afem_elastodynamics_set_lame", self.h, float(lam), float(mu))
            if self.method < 0:  # WeakPenalty: the library's own refusal
                self.setDirichlet(np.zeros(0, dtype=np.int32), (0.0, 0.0))
        except Exception:
            self.close()
            raise

    def setDirichlet(self, nodes, u):
        """One dirichlet-boundary-condition / dirichlet-point-condition block:
        the group's nodes and u = (u1, u2), None for a component the block
        leaves out.  Blocks accumulate; a later one overrides per DoF."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int32).ravel()
        mask, v = _mask_values(u)
        call("afem_elastodynamics_set_dirichlet_vectorial", self.h, ctypes.c_void_p(nodes.ctypes.data) if nodes.size else
             None, nodes.size, v, mask, self.method, C.AFEM_MEM_HOST)

    def setTraction(self, faces, t, table=None):
        """One traction-boundary-condition block on boundary edges
        (faces[n, 2], local node ids): t = (t1, t2), None for a missing
        component; table = (times[n], values[n, 2]) makes it the CaseTable of
        a traction-input-file (t is then ignored, both components are read).
        Returns the block's index."""
        faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 2)
        mask, v = _mask_values((0.0, 0.0) if table is not None else t)
        call("afem_elastodynamics_set_traction", self.h, ctypes.c_void_p(faces.ctypes.data) if faces.size else None,
             faces.shape[0], v, mask, C.AFEM_MEM_HOST)
        k = self.n_tractions
        self.n_tractions += 1
        if table is not None:
            times = np.ascontiguousarray(table[0], dtype=np.float64).ravel()
            vals = np.ascontiguousarray(table[1], dtype=np.float64).reshape(-1, 2)
            if vals.shape[0] != times.size:
                raise ValueError("the table needs one (t1, t2) per time")
            call("afem_elastodynamics_set_traction_table", self.h, k, ctypes.c_void_p(times.ctypes.data),
                 ctypes.c_void_p(vals.ctypes.data), times.size)
        return k

    def operators(self):
        """The last step's LHS on the device: dict(lhs = CsrView of c0 M +
        K(c1, c2) with the Dirichlet rows as the solve saw them (block 2,
        CSR-row order), scalar_rows / scalar_cols = its scalar CSR structure,
        c = the constants c0 .. c10).  No mass operator is stored."""
        d = super().operators()
        d.pop("mass")
        return d


class Soildynamics2D(Elastodynamics2D):
    """The module modules/soildynamics: the block-2 TRIA3 step of
    Elastodynamics2D plus paraxial (absorbing) boundaries -- an EDGE2 matrix on
    the LHS (FemModule.cc:1376-1486) and an edge loop over U, V, A on the RHS
    (:870-936), one HIP launch per step for all blocks -- and a force-based
    double-couple source (:946-987).  Material: cp and cs (mu = cs^2 rho,
    lambda = cp^2 rho - 2 mu, :275-278), lam and mu, or E and nu (:261-273).
    Newmark-beta without damping only, as the module (:321).  setTraction and
    setDirichlet are Elastodynamics2D's.
    """

    def __init__(self, ctx: Context, mesh: Mesh, rho: float, dt: float, cp: float | None = None,
                 cs: float | None = None, lam: float | None = None, mu: float | None = None, E: float | None = None,
                 nu: float | None = None, body_force=(None, None), time_discretization: str = "newmark-beta",
                 alpm: float = 0.0, alpf: float = 0.0, **kw):
        self._check(mesh, time_discretization)
        if SCHEMES[time_discretization.lower()] != 0:
            raise ValueError("Only Newmark-beta works for time-discretization Generalized-alpha WIP")
        pairs = [(cp, cs), (lam, mu), (E, nu)]
        if any((a is None) != (b is None) for a, b in pairs) or sum(a is not None for a, _ in pairs) != 1:
            raise ValueError("give the material as cp and cs, as lam and mu, or as E and nu")
        if cp is not None:
            mu = float(cs) * float(cs) * rho
            lam = float(cp) * float(cp) * rho - 2.0 * mu
        # alpm / alpf of a deck are ignored by Newmark-beta (FemModule.cc:283-300)
        super().__init__(ctx, mesh, rho, dt, lam=lam, mu=mu, E=E, nu=nu, body_force=body_force,
                         time_discretization=time_discretization, **kw)
        if cp is not None:
            try:
                call("afem_elastodynamics_set_wave_speeds", self.h, float(cp), float(cs))
            except Exception:
                self.close()
                raise

    def setParaxial(self, faces):
        """One paraxial-boundary-condition block: the group's boundary edges
        (faces[n, 2], local node ids).  Blocks accumulate."""
        faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 2)
        call("afem_elastodynamics_set_paraxial", self.h, ctypes.c_void_p(faces.ctypes.data) if faces.size else None,
             faces.shape[0], C.AFEM_MEM_HOST)

    def setDoubleCouple(self, north, south, east, west, table):
        """One double-couple block (force-based): the four node groups (any may
        be empty) and table = (times[n], values[n]), the force F of the
        double-couple-input-file; each step assigns rhs[2 north] = F,
        rhs[2 south] = -F, rhs[2 east + 1] = -F, rhs[2 west + 1] = F at the
        step's time.  Sources accumulate in order."""
        lists = [np.ascontiguousarray(x, dtype=np.int32).ravel() for x in (north, south, east, west)]
        times = np.ascontiguousarray(table[0], dtype=np.float64).ravel()
        vals = np.ascontiguousarray(table[1], dtype=np.float64).ravel()
        if vals.size != times.size:
            raise ValueError("the table needs one force per time")
        args = []
        for a in lists:
            args += [ctypes.c_void_p(a.ctypes.data) if a.size else None, a.size]
        call("afem_elastodynamics_set_double_couple", self.h, *args, ctypes.c_void_p(times.ctypes.data) if times.size
             else None, ctypes.c_void_p(vals.ctypes.data) if vals.size else None, times.size, C.AFEM_MEM_HOST)
