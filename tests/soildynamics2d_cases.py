"""The reference's soildynamics decks (2D, TRIA3, block 2) on the small meshes,
as data: replayed by the CPU restatement (test_soildynamics2d_ref.py) and by
the GPU tests (test_gpu_soildynamics2d.py).

Sources (toutane/arcanefem @ 2025-02-20, modules/soildynamics):
  inputs/*.arc                          the decks (names below, without the directory)
  CMakeLists.txt                        the five registered decks
  check/test_paraxial_results.txt       golden of double-couple.paraxial.arc   (tests/golden/)
  check/test_soildynamics_results.txt   golden of Soildynamics.arc             (tests/golden/)
  data/force_loading_dc.txt             the double couple's force table        (tests/golden/)
  data/semi-circle-soil-traction.txt    the transient traction table           (tests/golden/)
  meshes/msh/square_double-couple.msh, semi-circle-soil.msh, bar_dynamic.msh   (tests/golden/)

The material is one of (cp, cs), (lam, mu), (E, nu): the keys a deck does not
give are None.  `paraxial` lists the face groups of the deck's
paraxial-boundary-condition blocks, `double_couple` (north, south, east, west
node groups, table file) per double-couple block; `dirichlet`, `points`,
`traction`, `f`, `method`, `penalty` as in elastodynamics2d_cases.py.  All decks
are Newmark-beta; the alpm / alpf of Soildynamics.arc are ignored by it
(FemModule.cc:283-300).

A run ends with the first step whose updated time exceeds tmax + dt - 1e-8
(compute, :176; soildynamics2d_ref.steps): 20 steps for the square deck, 25
for the bar, 8 for the semi-circle decks.

The fifth registered deck, double-couple.paraxial.soil.arc, runs on
soil_2d.msh (261 kB, not committed) and has no golden; it differs from the
square deck in the mesh, the constants (cp = 20, cs = 11.5, rho = 9) and in
leaving the top side free.  "double-couple.paraxial.soil.arc@square" below is
that deck's constants and its three paraxial sides on the square mesh's groups.
"""
BAR, SQUARE, SEMI_SOIL = "bar_dynamic.msh", "square_double-couple.msh", "semi-circle-soil.msh"
DC_TABLE, SOIL_TABLE = "force_loading_dc.txt", "semi-circle-soil-traction.txt"
GOLDEN = {"Soildynamics.arc": "test_soildynamics_results.txt",
          "double-couple.paraxial.arc": "test_paraxial_results.txt"}


def _deck(mesh, tmax, dt, rho, cp=None, cs=None, lam=None, mu=None, E=None, nu=None, method="Penalty", penalty=1.0e30,
          f=(None, None), alpm=0.0, alpf=0.0, dirichlet=(), points=(), traction=(), paraxial=(), double_couple=()):
    return dict(mesh=mesh, tmax=tmax, dt=dt, rho=rho, cp=cp, cs=cs, lam=lam, mu=mu, E=E, nu=nu, scheme="Newmark-beta",
                method=method, penalty=penalty, f=f, etam=0.0, etak=0.0, alpm=alpm, alpf=alpf, dirichlet=list(dirichlet),
                points=list(points), traction=list(traction), paraxial=list(paraxial),
                double_couple=list(double_couple))


_SOURCE = [("sourceT", "sourceB", "sourceR", "sourceL", DC_TABLE)]
_SEMI = dict(mesh=SEMI_SOIL, tmax=0.08, dt=0.01, rho=2500.0, E=6.62e6, nu=0.45, paraxial=["lower"])

DECKS = {
    "Soildynamics.arc": _deck(BAR, 2.0, 0.08, 1.0, lam=576.9230769, mu=384.6153846, penalty=1.0e64, alpm=0.20,
                              alpf=0.40, dirichlet=[("surfaceleft", (0.0, 0.0))],
                              traction=[("surfaceright", (None, 0.01), None)]),
    "double-couple.paraxial.arc": _deck(SQUARE, 0.2, 0.01, 1.0, cp=4.0, cs=2.0, method="RowColumnElimination",
                                        paraxial=["left", "top", "right", "bottom"], double_couple=_SOURCE),
    "double-couple.paraxial.soil.arc@square": _deck(SQUARE, 0.2, 0.01, 9.0, cp=20.0, cs=11.5,
                                                    method="RowColumnElimination",
                                                    paraxial=["left", "right", "bottom"], double_couple=_SOURCE),
    "constant-traction.arc": _deck(traction=[("input", (0.01, 0.01), None)], **_SEMI),
    "transient-traction.arc": _deck(traction=[("input", (None, None), SOIL_TABLE)], **_SEMI),
}
