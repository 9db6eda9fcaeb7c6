"""Seeded generators of small CSR systems that no mesh produces (pure NumPy).

Each generator returns (row_ptr int64[n+1], cols int32, vals float64, n_cols);
the columns of a row may repeat (duplicates add up, as O.csr_to_dense and the
SpMV treat them) and need not be sorted.  Values have mixed signs and
magnitudes over about 6 decades, so a misplaced product shows.  The shapes are
the smallest that cross each boundary of arcanefem_amd/csrc/linear_system.hip:
the 4096 non-zeros of k_spmv_stream4u's unrolled pass, the 8192 non-zeros
(64 KiB of LDS) of a 256-row segment, the 16-lane chunks of k_spmv_v16, the
4-aligned groups of the 16-B loads, the 50 % gate and the 64/128/256-row
blocks of the pattern kernel.
"""
import numpy as np

SEED = 20250220


def rng_for(name):
    return np.random.default_rng([SEED] + [ord(c) for c in name])


def values(rng, m):
    """mixed signs, magnitudes 1e-3 .. 1e3"""
    return rng.choice([-1.0, 1.0], m) * 10.0 ** rng.uniform(-3.0, 3.0, m)


def rows_of(row_ptr):
    """setCSRValues' (rows, rows_nb_column): row starts without sentinel, row lengths"""
    return row_ptr[:-1].astype(np.int32), np.diff(row_ptr).astype(np.int32)


def from_lengths(lens, n_cols, rng):
    """random columns in [0, n_cols) (repeats allowed), random values"""
    lens = np.asarray(lens, dtype=np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    m = int(rp[-1])
    return rp, rng.integers(0, n_cols, m).astype(np.int32), values(rng, m), n_cols


def random_rows(n, rng=None, lo=0, hi=6, n_cols=None):
    rng = rng or rng_for(f"random{n}")
    return from_lengths(rng.integers(lo, hi + 1, n), n_cols or n, rng)


ROW_COUNTS = [1, 63, 64, 65, 255, 256, 257, 513, 1000]


def uniform(n, per_row, extra=()):
    """`per_row` entries in every row, one more in each row of `extra`"""
    lens = np.full(n, per_row, dtype=np.int64)
    for r in extra:
        lens[r] += 1
    return from_lengths(lens, n, rng_for(f"uniform{n}_{per_row}_{len(extra)}"))


def aligned(start_mod4, nnz_mod4, n=513):
    """the second 256-row block starts at a = start_mod4 (mod 4), nnz = nnz_mod4 (mod 4)"""
    rng = rng_for(f"aligned{start_mod4}{nnz_mod4}")
    lens = rng.integers(1, 9, n)
    lens[0] += (start_mod4 - lens[:256].sum()) % 4
    lens[n - 1] += (nnz_mod4 - lens.sum()) % 4
    rp, cols, vals, nc = from_lengths(lens, n, rng)
    assert rp[256] % 4 == start_mod4 and rp[-1] % 4 == nnz_mod4
    return rp, cols, vals, nc


def with_empty(n, empty, name):
    rng = rng_for(name)
    lens = rng.integers(1, 7, n)
    lens[np.asarray(empty, dtype=np.int64)] = 0
    return from_lengths(lens, n, rng)


def empty_cases():
    rng = rng_for("scatter")
    return {
        "empty_first": with_empty(257, [0], "empty_first"),
        "empty_scattered": with_empty(513, np.unique(rng.integers(0, 513, 120)), "empty_scattered"),
        # rows 250 .. 549: the 256-row block 1 and four 64-row blocks have seglen == 0
        "empty_300": with_empty(1000, np.arange(250, 550), "empty_300"),
        "empty_last": with_empty(257, [256], "empty_last"),
        "empty_last5": with_empty(513, np.arange(508, 513), "empty_last5"),
        "empty_all": (np.zeros(66, np.int64), np.zeros(0, np.int32), np.zeros(0), 65),
    }


def skew(long_rows, n=513, long_len=5000):
    """rows of 1 .. 3 entries and `long_rows` of long_len entries each (more
    entries than columns: duplicate columns)"""
    rng = rng_for(f"skew{len(long_rows)}")
    lens = rng.integers(1, 4, n)
    lens[list(long_rows)] = long_len
    return from_lengths(lens, n, rng)


def ghosts(n=257, n_ghost=40):
    """n_cols = n + n_ghost with entries in [n, n_cols)"""
    rng = rng_for("ghosts")
    rp, cols, vals, nc = from_lengths(rng.integers(1, 9, n), n + n_ghost, rng)
    cols[::3] = rng.integers(n, n + n_ghost, cols[::3].size)
    return rp, cols, vals, nc


def toeplitz_offsets(length):
    """negative and positive offsets: the first and the last rows are clipped"""
    return {1: [1], 3: [-1, 0, 1]}.get(length) or list(range(-(length // 2), length - length // 2))


def toeplitz(n, offsets, other=None, name=None):
    """Row r holds the columns r + off that fall in [0, n) (a clipped row is
    shorter: it does not match the pattern).  other: {row: length} rows with
    random columns instead."""
    rng = rng_for(name or f"toeplitz{n}_{len(offsets)}")
    offsets = np.asarray(offsets, dtype=np.int64)
    other = other or {}
    lens = np.zeros(n, dtype=np.int64)
    r = np.arange(n)[:, None] + offsets[None, :]
    ok = (r >= 0) & (r < n)
    for o in other:
        ok[o, :] = False
    lens[:] = ok.sum(axis=1)
    flat = r[ok].astype(np.int32)  # row-major: the rows' columns in offset order
    for o, ln in other.items():
        lens[o] = ln
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cols = np.zeros(int(rp[-1]), dtype=np.int32)
    tl = ok.sum(axis=1)
    pos = np.repeat(rp[:-1], tl) + (np.arange(int(tl.sum())) - np.repeat(np.cumsum(tl) - tl, tl))
    cols[pos] = flat
    for o, ln in other.items():
        cols[rp[o]:rp[o] + ln] = rng.integers(0, n, ln)
    matching = int((ok.all(axis=1)).sum())
    return (rp, cols, values(rng, int(rp[-1])), n), matching


def pattern_share(n_match, n=1000):
    """offsets (-1, 0, 1) in exactly n_match rows; the other rows have lengths
    0, 1 and 40 in turn (random columns)"""
    rng = rng_for(f"share{n_match}")
    match = set(rng.choice(np.arange(1, n - 1), n_match, replace=False).tolist())
    other = {}
    for i, r in enumerate(r for r in range(n) if r not in match):
        other[r] = (0, 1, 40)[i % 3]
    (rp, cols, vals, nc), m = toeplitz(n, [-1, 0, 1], other, name=f"share{n_match}")
    assert m == n_match
    return rp, cols, vals, nc


def pattern_seg64(seg, n=513):
    """15 offsets per row and one row of random columns in the 64-row block
    128 .. 191 that makes that block's segment exactly `seg` non-zeros (every
    other 64-row block holds at most 960)"""
    (rp, cols, vals, nc), _ = toeplitz(n, toeplitz_offsets(15), {150: seg - 63 * 15}, name=f"seg{seg}")
    assert rp[192] - rp[128] == seg
    return rp, cols, vals, nc


def max_segment(row_ptr, bs):
    n = row_ptr.size - 1
    starts = np.arange(0, n, bs)
    return int((row_ptr[np.minimum(starts + bs, n)] - row_ptr[starts]).max())


def spmv_longdouble(row_ptr, cols, vals, x):
    """y = A x and the row sums of |a_rk x_k| in np.longdouble"""
    prod = vals.astype(np.longdouble) * x.astype(np.longdouble)[cols]
    n = row_ptr.size - 1
    y = np.zeros(n, dtype=np.longdouble)
    mag = np.zeros(n, dtype=np.longdouble)
    ne = row_ptr[:-1] < row_ptr[1:]
    if ne.any():
        y[ne] = np.add.reduceat(prod, row_ptr[:-1][ne])
        mag[ne] = np.add.reduceat(np.abs(prod), row_ptr[:-1][ne])
    return y, mag


# ---- symmetric systems for the PCG (tests/pcg_ref.py)
def spd_system(n, name=None, per_row=3, n_penalty=3, n_elim=3, n_dup=3):
    """Symmetric, strictly diagonally dominant, random sparse (row i coupled to
    `per_row` random rows, symmetrised; duplicates add up), then: n_dup rows
    with the diagonal split into two entries, n_penalty penalty rows (diagonal
    1e30, b = 1e30 g) and n_elim row-eliminated identity rows (b = g) whose
    column keeps the other rows' entries: the matrix is no longer symmetric,
    its free block is.  Returns (row_ptr, cols, vals, n), b."""
    rng = rng_for(name or f"spd{n}")
    i = np.repeat(np.arange(n), per_row)
    j = rng.integers(0, n, i.size)
    keep = i != j
    i, j = i[keep], j[keep]
    w = rng.choice([-1.0, 1.0], i.size) * 10.0 ** rng.uniform(-2.0, 1.0, i.size)
    r = np.concatenate([i, j])
    c = np.concatenate([j, i])
    v = np.concatenate([w, w])
    off = np.bincount(r, np.abs(v), n)
    d = off * rng.uniform(1.2, 3.0, n) + 10.0 ** rng.uniform(-2.0, 1.0, n)
    special = rng.permutation(n)
    dup = special[:min(n_dup, n)]
    rest = special[min(n_dup, n):] if n > 4 else special[:0]
    pen = rest[:n_penalty]
    eli = rest[n_penalty:n_penalty + n_elim]
    d2 = np.zeros(0)
    if dup.size:
        d2 = d[dup] * 0.25
        d[dup] -= d2
    d[pen] = 1e30
    r = np.concatenate([r, np.arange(n), dup])
    c = np.concatenate([c, np.arange(n), dup])
    v = np.concatenate([v, d, d2])
    if eli.size:
        is_e = np.zeros(n, bool)
        is_e[eli] = True
        e_row = is_e[r]
        v[e_row] = np.where(c[e_row] == r[e_row], 1.0, 0.0)
        # one diagonal entry of 1 per eliminated row (a split diagonal would give 2)
        first = np.zeros(n, bool)
        for t in np.flatnonzero(e_row & (c == r)):
            if first[r[t]]:
                v[t] = 0.0
            first[r[t]] = True
    order = np.lexsort((rng.random(r.size), r))  # rows in order, a row's entries shuffled
    r, c, v = r[order], c[order], v[order]
    rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int64)
    b = values(rng, n)
    g = rng.uniform(-2.0, 2.0, n)
    b[pen] = 1e30 * g[pen]
    b[eli] = g[eli]
    return (rp, c.astype(np.int32), v, n), b


def banded_spd(n, offsets=(1, 7), name=None):
    """Symmetric bands at +-offsets with random weights and a dominant diagonal,
    built without a loop over rows (3 .. 2 len(offsets) + 1 non-zeros per row);
    columns sorted."""
    rng = rng_for(name or f"band{n}")
    rs, cs, vs = [np.arange(n)], [np.arange(n)], [np.zeros(n)]
    off = np.zeros(n)
    for o in offsets:
        w = rng.choice([-1.0, 1.0], n - o) * 10.0 ** rng.uniform(-1.0, 1.0, n - o)
        i = np.arange(n - o)
        rs += [i, i + o]
        cs += [i + o, i]
        vs += [w, w]
        off[:n - o] += np.abs(w)
        off[o:] += np.abs(w)
    vs[0] = off * rng.uniform(1.2, 2.0, n) + 0.1
    r, c, v = np.concatenate(rs), np.concatenate(cs), np.concatenate(vs)
    order = np.lexsort((c, r))
    r, c, v = r[order], c[order], v[order]
    rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int64)
    return (rp, c.astype(np.int32), v, n), values(rng, n)


def block3_system(nb=67, per_node=3, name="block3"):
    """Random SPD block-3 CSR (3 nb rows): node i coupled to `per_node` random
    nodes by full 3 x 3 blocks W (and W^T on the other side), dominant
    symmetric diagonal blocks with off-diagonal entries, no duplicates, columns
    sorted.  Node 5 has one penalty row (row 16), node 9 two (rows 27, 29).
    Returns (row_ptr, cols, vals, n), b, penalty rows."""
    rng = rng_for(name)
    n = 3 * nb
    A = np.zeros((n, n))
    for i in range(nb):
        for j in rng.integers(0, nb, per_node):
            if j == i:
                continue
            W = rng.uniform(-1.0, 1.0, (3, 3))
            A[3 * i:3 * i + 3, 3 * j:3 * j + 3] = W
            A[3 * j:3 * j + 3, 3 * i:3 * i + 3] = W.T
    for i in range(nb):
        S = rng.uniform(-1.0, 1.0, (3, 3))
        A[3 * i:3 * i + 3, 3 * i:3 * i + 3] = S + S.T
    off = np.abs(A).sum(axis=1)
    A[np.arange(n), np.arange(n)] = off * rng.uniform(1.1, 1.5, n) + 0.1
    pen = np.array([16, 27, 29])
    A[pen, pen] = 1e30
    r, c = np.nonzero(A)
    rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int64)
    b = values(rng, n)
    b[pen] = 1e30 * rng.uniform(-2.0, 2.0, 3)
    return (rp, c.astype(np.int32), A[r, c], n), b, pen
