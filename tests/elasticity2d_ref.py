"""CPU restatement (numpy, float64) of what the reference's 2D elasticity module
adds around the stiffness matrix, on top of the oracle's routines: the
checker of test_elasticity2d_ref.py (against the reference goldens) and of
test_gpu_elasticity2d.py (against the GPU).

  * body force: the per-cell loop of modules/elasticity/FemModule.cc:230-241,
    rhs[2 v + i] += f_i |K| / 3 on owned nodes, NULL components as 0;
  * consistent P1 mass blocks: |K|/6 on a node's own block, |K|/12 on a
    neighbour's, on the component diagonal;
  * the NULL-component expansion of a Dirichlet `u` tuple into DoF lists
    (femutils/ArcaneFemFunctionsGpu.h:514-586);
  * the reference solution: a dense solve with the constrained DoFs taken out,
    A_ff x_f = b_f - A_fc g, so the clamped values are exact (a dense LU with
    identity rows left in leaves 1e-10-sized noise in DoFs that must be 0);
  * the golden rule of the elasticity goldens (elasticity2d_cases.py).
"""
import numpy as np

from oracle import oracle as O

from elasticity2d_cases import E, NU, SMALL_ABS, SMALL_REL
from golden_cases import lame


def tri_areas(cells, coords):
    p = np.asarray(coords, dtype=np.float64)[np.asarray(cells)]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    return 0.5 * np.abs(e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1])


def body_force_rhs(n_own, cells, coords, f):
    """rhs[2 v + i] = sum over the cells of owned node v of f_i |K| / 3, cell by cell."""
    fv = [0.0 if x is None else float(x) for x in f]
    rhs = np.zeros(2 * n_own)
    for c, a in zip(np.asarray(cells), tri_areas(cells, coords)):
        for v in c:
            if v < n_own:
                rhs[2 * v] += fv[0] * a / 3
                rhs[2 * v + 1] += fv[1] * a / 3
    return rhs


def mass_blocks(n_own, cells, coords, row_ptr, cols, mass_coef):
    """mass_coef x consistent P1 mass, ordered per block like O.assemble_elasticity_tri."""
    vals = np.zeros(4 * cols.shape[0])
    slot = {}
    for r in range(n_own):
        for k in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            slot[(r, int(cols[k]))] = k
    for c, a in zip(np.asarray(cells), tri_areas(cells, coords)):
        for r in c:
            if r >= n_own:
                continue
            for b in c:
                m = mass_coef * a / (6.0 if b == r else 12.0)
                k = slot[(int(r), int(b))]
                vals[4 * k] += m
                vals[4 * k + 3] += m
    return vals


def scalar_csr(row_ptr, cols, vals4):
    """Per-block values -> the scalar CSR (rows, columns, values) of the
    per-scalar-row layout rb*4 + i*2*len + 2*slot + j."""
    n = row_ptr.shape[0] - 1
    ln = np.diff(row_ptr)
    srp = np.zeros(2 * n + 1, dtype=np.int64)
    srp[1:] = np.cumsum(np.repeat(2 * ln, 2))
    scols = np.empty(4 * cols.shape[0], dtype=np.int32)
    for r in range(n):
        c2 = np.stack([2 * cols[row_ptr[r]:row_ptr[r + 1]], 2 * cols[row_ptr[r]:row_ptr[r + 1]] + 1], 1).ravel()
        scols[srp[2 * r]:srp[2 * r + 1]] = c2
        scols[srp[2 * r + 1]:srp[2 * r + 2]] = c2
    return srp, scols, O.blocks_to_row_order(row_ptr, vals4)


def expand_u(nodes, u, n_own=None):
    """DoFs and values a `u` tuple (None = NULL) constrains on `nodes`."""
    nodes = np.asarray(nodes, dtype=np.int64)
    if n_own is not None:
        nodes = nodes[nodes < n_own]
    k = len(u)
    dofs = [k * nodes + i for i, x in enumerate(u) if x is not None]
    vals = [np.full(nodes.shape[0], float(x)) for x in u if x is not None]
    if not dofs:
        return np.zeros(0, np.int32), np.zeros(0)
    return np.concatenate(dofs).astype(np.int32), np.concatenate(vals)


def deck_constraints(gm, deck):
    """(dofs, values) of all Dirichlet blocks of a deck, later blocks overriding earlier ones."""
    g = {}
    for group, u in deck["dirichlet"] + deck["points"]:
        d, v = expand_u(gm.group_nodes(group), u)
        g.update(zip(d.tolist(), v.tolist()))
    dofs = np.array(sorted(g), dtype=np.int32)
    return dofs, np.array([g[d] for d in dofs])


def deck_system(gm, deck):
    """Scalar CSR (rows, columns, values) and RHS of a deck before its Dirichlet conditions."""
    n = gm.n_nodes
    lam, mu2 = lame(E, NU)
    orp, ocols = O.sparsity(n, n, gm.cells)
    srp, scols, svals = scalar_csr(orp, ocols, O.assemble_elasticity_tri(n, gm.cells, gm.coords, orp, ocols, lam, mu2))
    rhs = body_force_rhs(n, gm.cells, gm.coords, deck["f"])
    for group, t in deck["traction"]:
        O.neumann(2, n, 2, O.NEUMANN_TRACTION, t, gm.group_faces(group), None, gm.cells, gm.coords, rhs)
    return srp, scols, svals, rhs


def reduced_solve(A, b, dofs, values):
    """x with x[dofs] = values exactly and A_ff x_f = b_f - A_fc g."""
    n = A.shape[0]
    free = np.setdiff1d(np.arange(n), dofs)
    x = np.zeros(n)
    x[dofs] = values
    x[free] = np.linalg.solve(A[np.ix_(free, free)], b[free] - A[np.ix_(free, dofs)] @ values)
    return x


def penalty_solve(A, b, dofs, values, penalty):
    A, b = A.copy(), b.copy()
    A[dofs, dofs] = penalty
    b[dofs] = penalty * values
    return np.linalg.solve(A, b)


def deck_reference(gm, deck):
    srp, scols, svals, rhs = deck_system(gm, deck)
    dofs, values = deck_constraints(gm, deck)
    return reduced_solve(O.csr_to_dense(srp, scols, svals), rhs, dofs, values)


def golden_compare(u, gold, node_tags):
    """The golden rule: entries with |golden| < SMALL_REL max|golden| are counted
    and compared absolutely (returned relative to max|golden|); on the others
    the worst |d| / (|ref| + |v|) and the number failing the reference's own
    check (epsilon 1e-3, minimum 1e-16, per component)."""
    g = np.array([gold[int(t)][:2] for t in node_tags]).ravel()  # the files carry x, y and a zero z
    u = np.asarray(u)
    gmax = np.abs(g).max()
    small = np.abs(g) < SMALL_REL * gmax
    d = np.abs(u - g)
    rel = d[~small] / (np.abs(g[~small]) + np.abs(u[~small]))
    nerr = 0
    for comp in range(2):
        sel = ~small[comp::2]
        tags = np.asarray(node_tags)[sel]
        e, _ = O.check_node_result({int(t): v for t, v in zip(tags, u[comp::2][sel])},
                                   {int(t): gold[int(t)][comp] for t in tags}, 1e-3, 1e-16)
        nerr += e
    return dict(n_small=int(small.sum()), small_abs=float(d[small].max() / gmax) if small.any() else 0.0,
                rel=float(rel.max()), nerr=nerr, small_ok=bool(d[small].max() <= SMALL_ABS * gmax) if small.any() else True)
