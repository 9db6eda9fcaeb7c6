"""The Jacobi-PCG of ls_solve (arcanefem_amd/csrc/linear_system.hip) restated
in NumPy, in float64 or np.longdouble: the one restatement the tests share
(tests/test_pcg_ref.py pins it, tests/test_distributed_gloo.py runs it over
gloo, tests/test_gpu_linear_system_csr.py holds the GPU loop to it).

  k_inv_diag    dinv = 1 / sum of the row's diagonal entries (0 if that sum is
                0), cons = |d| > 1e10 * sum |off-diagonal|
  k_cg_x0       x0 = b * dinv on constraint rows, 0 elsewhere (the lift)
  k_cg_init     r = b - A x0, z = M^-1 r, p = z; r.z over all rows and over the
                free rows: the stopping reference is the latter, the former
                when the latter is not positive
  the loop      alpha = rz / pq (0 if pq == 0), beta = rz_new / rz (0 if
                rz == 0), the test every `check_every` iterations and at
                max_iter; fixed_iterations = k runs exactly k steps
  block3        M^-1 = inverse of the 3 x 3 node blocks with their constraint
                rows decoupled (k_inv_block3), point Jacobi for a singular block

`allsum` and `halo` are the two places where ranks talk (identity on one
rank); `dot` lets a test choose the summation order of the dot products.
"""
import numpy as np


def row_index(row_ptr):
    return np.repeat(np.arange(row_ptr.size - 1), np.diff(row_ptr))


def row_sums(row_ptr, a):
    out = np.zeros(row_ptr.size - 1, dtype=a.dtype)
    ne = row_ptr[:-1] < row_ptr[1:]
    if ne.any():
        out[ne] = np.add.reduceat(a, row_ptr[:-1][ne])
    return out


def spmv(row_ptr, cols, vals, x):
    """y = A x in the dtype of vals / x (rows may be empty, columns may repeat)"""
    return row_sums(row_ptr, vals * x[cols])


def inv_diag(row_ptr, cols, vals):
    """k_inv_diag: (dinv, cons)"""
    n = row_ptr.size - 1
    on = cols == row_index(row_ptr)
    d = row_sums(row_ptr, np.where(on, vals, 0))
    off = row_sums(row_ptr, np.where(on, 0, np.abs(vals)))
    dinv = np.zeros(n, dtype=vals.dtype)
    nz = d != 0
    dinv[nz] = 1 / d[nz]
    return dinv, np.abs(d) > 1e10 * off


def inv_block3(row_ptr, cols, vals, cons, dinv):
    """k_inv_block3: the 3 x 3 inverses [nb, 3, 3] (constraint rows decoupled)"""
    n = row_ptr.size - 1
    nb = n // 3
    ri = row_index(row_ptr)
    B = np.zeros((nb, 3, 3), dtype=vals.dtype)
    d = cols.astype(np.int64) - 3 * (ri // 3)
    inb = (d >= 0) & (d < 3)
    B[ri[inb] // 3, ri[inb] % 3, d[inb]] = vals[inb]  # (no duplicate inside a block)
    c = cons.reshape(nb, 3)
    dec = c[:, :, None] | c[:, None, :]
    dec[:, [0, 1, 2], [0, 1, 2]] = False
    B[dec] = 0
    out = np.zeros_like(B)
    for b in range(nb):
        M = B[b]
        c00 = M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1]
        c01 = M[1, 2] * M[2, 0] - M[1, 0] * M[2, 2]
        c02 = M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0]
        det = M[0, 0] * c00 + M[0, 1] * c01 + M[0, 2] * c02
        if det == 0 or not np.isfinite(det):
            out[b] = np.diag(dinv[3 * b:3 * b + 3])
            continue
        adj = np.array([[c00, M[0, 2] * M[2, 1] - M[0, 1] * M[2, 2], M[0, 1] * M[1, 2] - M[0, 2] * M[1, 1]],
                        [c01, M[0, 0] * M[2, 2] - M[0, 2] * M[2, 0], M[0, 2] * M[1, 0] - M[0, 0] * M[1, 2]],
                        [c02, M[0, 1] * M[2, 0] - M[0, 0] * M[2, 1], M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]]],
                       dtype=vals.dtype)
        out[b] = adj / det
    return out


def pcg(row_ptr, cols, vals, b, n_cols=None, rtol=1e-12, max_iter=10000, check_every=8, fixed_iterations=0,
        dtype=np.float64, dot=None, allsum=None, halo=None, block3=False):
    """The iteration of ls_solve on the owned rows [0, n) of a system with
    n_cols >= n local columns.  Returns a dict: x, r, z, p (owned part),
    iterations, converged, rel_residual, rz0, dinv, cons."""
    n = row_ptr.size - 1
    n_cols = n if n_cols is None else n_cols
    vals = np.asarray(vals).astype(dtype)
    b = np.asarray(b).astype(dtype)
    dot = dot or (lambda u, v: (u * v).sum())
    allsum = allsum or (lambda s: s)
    halo = halo or (lambda v: None)
    dinv, cons = inv_diag(row_ptr, cols, vals)
    if block3:
        binv = inv_block3(row_ptr, cols, vals, cons, dinv)
        precond = lambda r: np.einsum("bij,bj->bi", binv, r.reshape(-1, 3)).reshape(-1)  # noqa: E731
    else:
        precond = lambda r: r * dinv  # noqa: E731
    p = np.zeros(n_cols, dtype=dtype)
    x = np.where(cons, b * dinv, 0).astype(dtype)               # k_cg_x0
    p[:n] = x
    halo(p)
    r = b - spmv(row_ptr, cols, vals, p)                        # k_cg_init
    z = precond(r)
    p[:n] = z
    stuck = bool(allsum(float(np.any(~cons & (dinv == 0) & (r != 0)))) and not block3)
    rz = allsum(dot(r, z))
    rzf = allsum(dot(r[~cons], z[~cons]))
    rz0 = rzf if rzf > 0 else rz
    fixed = fixed_iterations > 0
    max_it = fixed_iterations if fixed else max_iter
    rel = np.sqrt(abs(rz / rz0)) if rz0 > 0 else 0.0
    converged = False if fixed else bool(rz == 0 or rel <= rtol)
    it = 0
    while not converged and it < max_it:
        halo(p)
        q = spmv(row_ptr, cols, vals, p)
        pq = allsum(dot(p[:n], q))
        alpha = rz / pq if pq != 0 else 0 * rz                  # k_cg_update_rz
        r = r - alpha * q
        z = precond(r)
        rzn = allsum(dot(r, z))
        beta = rzn / rz if rz != 0 else 0 * rz                  # k_cg_dir_x
        x = x + alpha * p[:n]
        p[:n] = z + beta * p[:n]
        rz = rzn
        it += 1
        if not fixed and (it % check_every == 0 or it == max_it):
            rel = np.sqrt(abs(rz / rz0))
            converged = bool(rel <= rtol)
    rel = np.sqrt(abs(rz / rz0)) if rz0 > 0 else 0.0
    converged = bool(rel <= rtol) if fixed else converged
    return dict(x=x, r=r, z=z, p=p[:n].copy(), iterations=it, converged=converged and not stuck,
                rel_residual=float(rel), rz0=rz0, dinv=dinv, cons=cons)
