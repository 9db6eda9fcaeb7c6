"""The reference's 2D elasticity regression decks on bar.msh that carry a body
force (block-2, TRIA3), as data: replayed by the CPU restatement
(test_elasticity2d_ref.py) and by the GPU tests (test_gpu_elasticity2d.py).

Sources (toutane/arcanefem @ 2025-02-20, modules/elasticity):
  inputs/bar.2D*.arc                 the decks (names below, without the directory)
  check/test_elasticity_results.txt, check/elasticity_traction_bodyforce_bar_test_ref.txt,
  check/elasticity_point-dirichlet_bar_test_ref.txt      the three goldens (tests/golden/)
All decks: E = 21e5, nu = 0.28; the penalty defaults to 1e30 (Fem.axl:37);
checked by the reference with checkNodeResultFile at epsilon 1e-3, minimum
1e-16 (FemModule.cc:547-553).

`f` and every `u` are tuples with None for the decks' NULL.  `dirichlet` holds
(group, u) for face groups (applied to the group's nodes), `points` the same
for point groups.  `method` is what the deck's enforce-Dirichlet-method
CONTAINS (default Penalty).
"""
E, NU, PENALTY = 21.0e5, 0.28, 1.0e30
MESH = "bar.msh"

G_BODY = "test_elasticity_results.txt"
G_TRACTION = "elasticity_traction_bodyforce_bar_test_ref.txt"
G_POINT = "elasticity_point-dirichlet_bar_test_ref.txt"

_CLAMP = [("left", (0.0, 0.0))]
_POINT_FACES = [("left", (0.0, None)), ("right", (1.0, None))]
_POINT_NODES = [("botLeft", (0.0, 0.0)), ("botRight", (None, 0.0))]


def _deck(golden, f, method="penalty", traction=(), dirichlet=_CLAMP, points=()):
    return dict(golden=golden, f=f, traction=list(traction), dirichlet=list(dirichlet), points=list(points),
                method=method)


_TB = dict(f=(3.33, -6.66), traction=[("right", (1.33, 2.13))])
_PD = dict(f=(None, -1.0), dirichlet=_POINT_FACES, points=_POINT_NODES)

DECKS = {
    "bar.2D.arc": _deck(G_BODY, (None, -1.0)),
    "bar.2D.DirichletViaRowElimination.arc": _deck(G_BODY, (None, -1.0), "row-elimination"),
    "bar.2D.DirichletViaRowColumnElimination.arc": _deck(G_BODY, (None, -1.0), "row-column-elimination"),
    "bar.2D.traction.bodyforce.arc": _deck(G_TRACTION, **_TB),
    "bar.2D.traction.bodyforce.bsr.arc": _deck(G_TRACTION, **_TB),
    "bar.2D.traction.bodyforce.bsr.atomic-free.arc": _deck(G_TRACTION, **_TB),
    "bar.2D.PointDirichlet.arc": _deck(G_POINT, **_PD),
    "bar.2D.PointDirichlet.bsr.arc": _deck(G_POINT, **_PD),
    "bar.2D.PointDirichlet.bsr.hypre.arc": _deck(G_POINT, **_PD),
    # the next two deck names are swapped against their contents in the
    # reference: ...PointDirichlet.DirichletViaRowElimination.arc says
    # RowColumnElimination and ...DirichletViaRowColumnElimination.arc says
    # RowElimination; recorded here is what each file contains
    "bar.2D.PointDirichlet.DirichletViaRowElimination.arc": _deck(G_POINT, method="row-column-elimination", **_PD),
    "bar.2D.PointDirichlet.DirichletViaRowColumnElimination.arc": _deck(G_POINT, method="row-elimination", **_PD),
}

# entries of each golden (of 160 = 80 nodes x 2 components) below 1e-6 x its
# largest: clamped DoFs (1e-30 from the penalty) and, in G_BODY, ten symmetry
# zeros (6e-16 .. 7.7e-11) that move by 1e-3 relative under rounding-size
# perturbations of the matrix; left out of the relative comparison and held
# to an absolute 1e-9 x max|golden| instead
SMALL_ENTRIES = {G_BODY: 20, G_TRACTION: 8, G_POINT: 6}
SMALL_REL, SMALL_ABS = 1.0e-6, 1.0e-9
