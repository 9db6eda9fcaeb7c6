"""The reference's six elastodynamics decks (2D, TRIA3, block 2), as data:
replayed by the CPU restatement (test_elastodynamics2d_ref.py) and by the GPU
tests (test_gpu_elastodynamics2d.py).

Sources (toutane/arcanefem @ 2025-02-20, modules/elastodynamics):
  inputs/*.arc                     the decks (names below, without the directory)
  CMakeLists.txt:34-42             the six registered tests
  data/traction_bar_test_1.txt     the transient-traction table (tests/golden/)
  meshes/msh/bar_dynamic.msh, meshes/msh/semi-circle.msh   (tests/golden/)
The module has no golden result files (_checkResultFile is a TODO,
FemModule.cc:1443-1452): the decks are checked against the restatement.

All decks: rho = 1, dt = 0.08, lambda = 576.9230769, mu = 384.6153846 (given
as Lame parameters, FemModule.cc:242-246).  `f`, every `u` and every `t` are
tuples with None for a component the deck leaves out.  `dirichlet` holds
(face group, u) applied to the group's nodes, `points` the same for point
groups, `traction` (face group, t, table file or None).  `method` is the
deck's enforce-Dirichlet-method (RowColumnElimination decks give no penalty:
the Fem.axl default).  The time loop runs steps at t = dt, 2 dt, ... until
t >= tmax - dt (startInit :175-176, compute :144-145): 24 steps for tmax = 2,
12 for tmax = 1 (elastodynamics2d_ref.steps).
"""
RHO, DT, LAM, MU = 1.0, 0.08, 576.9230769, 384.6153846
BAR, SEMI = "bar_dynamic.msh", "semi-circle.msh"
TABLE = "traction_bar_test_1.txt"

_CLAMP = [("surfaceleft", (0.0, 0.0))]


def _deck(mesh=BAR, tmax=2.0, scheme="Newmark-beta", method="Penalty", penalty=1.0e64, f=(None, None), etam=0.0,
          etak=0.0, alpm=0.0, alpf=0.0, dirichlet=_CLAMP, points=(), traction=()):
    return dict(mesh=mesh, tmax=tmax, dt=DT, rho=RHO, lam=LAM, mu=MU, scheme=scheme, method=method, penalty=penalty,
                f=f, etam=etam, etak=etak, alpm=alpm, alpf=alpf, dirichlet=list(dirichlet), points=list(points),
                traction=list(traction))


_T_CONST = [("surfaceright", (None, 0.01), None)]

DECKS = {
    "bar.arc": _deck(traction=_T_CONST),
    # Newmark-beta with alpm / alpf present: the scheme ignores them (:252-270)
    "bar.transient-traction.arc": _deck(alpm=0.20, alpf=0.40, traction=[("surfaceright", (None, None), TABLE)]),
    "bar.damping.arc": _deck(etam=0.01, etak=0.01, traction=_T_CONST),
    "bar.Galpha.arc": _deck(scheme="Generalized-alpha", method="RowColumnElimination", penalty=1.0e30, alpm=0.20,
                            alpf=0.40, traction=_T_CONST),
    "bar.dirichlet.traction.bodyforce.arc": _deck(tmax=1.0, f=(None, -2000.0),
                                                  traction=[("surfaceright", (None, -1.0), None)]),
    "semi-circle.pointBC.arc": _deck(mesh=SEMI, tmax=1.0, method="RowColumnElimination", penalty=1.0e30,
                                     dirichlet=[("boderCircle", (0.0, 0.0))], points=[("source", (10.0, 10.0))]),
}

