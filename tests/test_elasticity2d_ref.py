"""The CPU restatement of the 2D elasticity decks (elasticity2d_ref.py)
reproduces the reference's three body-force goldens on bar.msh, for every deck
of elasticity2d_cases.py, under the golden rule stated there.  This pins the
helper before the GPU is compared against it (test_gpu_elasticity2d.py).

Measured worst |d| / (|ref| + |v|) on the entries of the relative comparison,
reduced-system and penalty solves: 1.3e-10 (test_elasticity_results), 7.1e-13
(traction + body force), 1.8e-10 (point Dirichlet); gate 1e-8, the bound
golden_cases.py uses for goldens that an iterative solver produced.
"""
import os

import numpy as np
import pytest

from arcanefem_amd.gmsh import read_gmsh, read_node_result_file
from oracle import oracle as O

import elasticity2d_ref as R
from elasticity2d_cases import DECKS, MESH, PENALTY, SMALL_ENTRIES
from golden_cases import path

GOLDEN_GATE = 1e-8


@pytest.fixture(scope="module")
def gm():
    return read_gmsh(path(MESH))


@pytest.mark.parametrize("deck", list(DECKS))
def test_restatement_reproduces_golden(gm, deck):
    c = DECKS[deck]
    srp, scols, svals, rhs = R.deck_system(gm, c)
    A = O.csr_to_dense(srp, scols, svals)
    dofs, values = R.deck_constraints(gm, c)
    gold = read_node_result_file(path(c["golden"]))
    sols = {"reduced": R.reduced_solve(A, rhs, dofs, values)}
    if c["method"] == "penalty":
        sols["penalty"] = R.penalty_solve(A, rhs, dofs, values, PENALTY)
    else:
        assert np.array_equal(sols["reduced"][dofs], values)
    for name, u in sols.items():
        r = R.golden_compare(u, gold, gm.node_tags)
        print(f"{deck} [{name}]: {r}")
        assert r["n_small"] == SMALL_ENTRIES[c["golden"]]
        assert r["small_ok"], r
        assert r["nerr"] == 0
        assert r["rel"] <= GOLDEN_GATE


def test_every_golden_has_its_decks():
    by_golden = {}
    for c in DECKS.values():
        by_golden.setdefault(c["golden"], []).append(c["method"])
    assert {g: sorted(m) for g, m in by_golden.items()} == {
        "test_elasticity_results.txt": ["penalty", "row-column-elimination", "row-elimination"],
        "elasticity_traction_bodyforce_bar_test_ref.txt": ["penalty"] * 3,
        "elasticity_point-dirichlet_bar_test_ref.txt": ["penalty"] * 3 + ["row-column-elimination", "row-elimination"]}
    for g in by_golden:
        assert len(read_node_result_file(path(g))) == 80 and os.path.getsize(path(g)) < 8192


def test_null_component_expansion():
    d, v = R.expand_u([3, 7, 40], (0.25, None))
    assert d.tolist() == [6, 14, 80] and v.tolist() == [0.25] * 3
    d, v = R.expand_u([3, 7, 40], (None, -2.0), n_own=10)
    assert d.tolist() == [7, 15] and v.tolist() == [-2.0] * 2
    d, v = R.expand_u([3], (1.0, 3.0))
    assert d.tolist() == [6, 7] and v.tolist() == [1.0, 3.0]
    assert R.expand_u([3], (None, None))[0].size == 0


def test_body_force_and_mass_sum_to_the_area(gm):
    n = gm.n_nodes
    area = R.tri_areas(gm.cells, gm.coords).sum()
    rhs = R.body_force_rhs(n, gm.cells, gm.coords, (None, -1.0))
    assert np.all(rhs[0::2] == 0.0) and abs(rhs[1::2].sum() + area) <= 1e-13 * area
    orp, ocols = O.sparsity(n, n, gm.cells)
    m = R.mass_blocks(n, gm.cells, gm.coords, orp, ocols, 2.0)
    assert abs(m[0::4].sum() - 2.0 * area) <= 1e-13 * area and np.array_equal(m[0::4], m[3::4])
    assert not m[1::4].any() and not m[2::4].any()
