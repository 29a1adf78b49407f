"""Matrices and reference arithmetic for the IC(0) tests (test_ic0.py, test_gpu_ic0.py).

Stencils give IC(0) short rows (<= 14 entries of L), regular wavefront levels and grids that fit
on the device at once.  The matrices here do not: random sparsity, hub rows as long as the matrix,
a chain with one row per level, and a grid of more waves than the device holds.  All are symmetric
with ascending columns and diagonal = sum |off-diagonal| + 1: strictly diagonally dominant, so an
H-matrix, so IC(0) exists with shift 0.  Every generator is seeded; numpy only (fem150 is the
library's own stencil generator).

The reference side is plain numpy in np.longdouble over the CSR arrays: the factor identity on L's
pattern and the componentwise residual of one triangular solve.
"""
import functools

import numpy as np

EPS = 2.0 ** -53


def _csr_from_mask(mask, vals):
    """(row_offsets, column_indices, values) of the entries where mask holds, columns ascending."""
    r, c = np.nonzero(mask)  # row-major: rows ascending, columns ascending within a row
    ro = np.zeros(mask.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=mask.shape[0]), out=ro[1:])
    return ro.astype(np.int32), c.astype(np.int32), vals[r, c]


def _dominant_symmetric(n, mask_upper, vals_upper):
    """Mirror a strict upper triangle and set the diagonal to sum |off-diagonal| + 1."""
    mask = np.triu(mask_upper, 1)
    vals = np.where(mask, vals_upper, 0.0)
    mask = mask | mask.T
    vals = vals + vals.T
    np.fill_diagonal(vals, np.abs(vals).sum(axis=1) + 1.0)
    np.fill_diagonal(mask, True)
    return n, *_csr_from_mask(mask, vals)


def _random_draws(rng, n, draws):
    mask = np.zeros((n, n), bool)
    vals = np.zeros((n, n))
    cols = rng.integers(0, n, (n, draws))
    v = rng.uniform(-1.0, 1.0, (n, draws))
    rows = np.repeat(np.arange(n), draws)
    mask[rows, cols.ravel()] = True
    vals[rows, cols.ravel()] = v.ravel()  # a column drawn twice keeps its last value
    return mask, vals


def randsym777():
    """n = 777, 6 random columns per row: irregular rows and levels."""
    n = 777
    mask, vals = _random_draws(np.random.default_rng(777), n, 6)
    return _dominant_symmetric(n, mask, vals)


def hubs600():
    """n = 600, 3 random columns per row, rows / columns 200 and 599 dense: L's rows 200 and 599 hold
    201 and 600 entries (several trips of the solve's chunk loop at every width), and every row of
    L^T awaits row 599."""
    n = 600
    rng = np.random.default_rng(600)
    mask, vals = _random_draws(rng, n, 3)
    mask, vals = np.triu(mask, 1), np.triu(vals, 1)
    for h in (200, 599):
        v = rng.uniform(-1.0, 1.0, n)
        mask[:h, h], vals[:h, h] = True, v[:h]
        mask[h, h + 1:], vals[h, h + 1:] = True, v[h + 1:]
    return _dominant_symmetric(n, mask, vals)


def tridiag2000():
    """Diagonal 2.5, off-diagonals -1: 2,000 levels of one row, each wave awaits the one before."""
    n = 2000
    i = np.arange(n)
    cand = np.stack([i - 1, i, i + 1], axis=1)
    ok = (cand >= 0) & (cand < n)
    lens = ok.sum(axis=1)
    ro = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=ro[1:])
    ci = cand[ok]
    va = np.where(ci == np.repeat(i, lens), 2.5, -1.0)
    return n, ro.astype(np.int32), ci.astype(np.int32), va


SMALL = {"randsym777": randsym777, "hubs600": hubs600, "tridiag2000": tridiag2000}


@functools.lru_cache(maxsize=None)
def matrix(name):
    """The named case as an mspmv.CsrMatrix (built once per session; do not modify)."""
    import mspmv

    if name == "fem150":  # 22,500 rows: more waves than 256 CUs x 32 hold at once
        return mspmv.CsrMatrix.synth_stencil(0, 22500, 150)
    n, ro, ci, va = SMALL[name]()
    return mspmv.CsrMatrix.from_arrays(n, ro, ci, va)


@functools.lru_cache(maxsize=None)
def factor(name):
    """(L, shift, L^T) of matrix(name): mspmv.ic0_factor and mspmv.csr_transpose."""
    import mspmv

    l, shift = mspmv.ic0_factor(matrix(name))
    return l, shift, mspmv.csr_transpose(l)


def rows_of(t):
    return np.repeat(np.arange(t.num_rows), np.diff(t.row_offsets.astype(np.int64)))


def lower_levels(l):
    """Dependency levels of the forward solve with lower-triangular l: 1 + the deepest level read."""
    ro, ci = l.row_offsets, l.column_indices
    lev = np.zeros(l.num_rows, np.int64)
    for i in range(l.num_rows):
        c = ci[ro[i]:ro[i + 1]]
        c = c[c < i]
        if c.size:
            lev[i] = lev[c].max() + 1
    return int(lev.max()) + 1 if l.num_rows else 0


def factor_identity_ratio(a, l, shift):
    """max over L's pattern of |(L L^T)_ij - A_ij - shift d_ij| / (2 (len_i + 2) 2^-53 (|L||L|^T)_ij),
    both sides formed in np.longdouble on the pattern's entries only.  The bound is the rounding
    bound of IC(0)'s defining recurrence: a sum of at most len_i products, one subtraction, one
    sqrt or division."""
    ro = l.row_offsets.astype(np.int64)
    ci = l.column_indices
    lv = l.values.astype(np.longdouble)
    ar = rows_of(a)
    low = a.column_indices <= ar
    # L keeps A's lower pattern in A's order: entry k of L sits on the k-th lower entry of A
    assert np.array_equal(a.column_indices[low], ci) and np.array_equal(ar[low], rows_of(l))
    target = a.values[low].astype(np.longdouble)
    target = target + np.where(ci == rows_of(l), np.longdouble(shift), np.longdouble(0))
    w = np.zeros(l.num_rows, np.longdouble)
    worst = 0.0
    for i in range(l.num_rows):
        s, e = ro[i], ro[i + 1]
        w[ci[s:e]] = lv[s:e]
        for k in range(s, e):
            j = ci[k]
            cj, vj = ci[ro[j]:ro[j + 1]], lv[ro[j]:ro[j + 1]]
            prod = vj * w[cj]
            err = abs(prod.sum() - target[k])
            bound = 2 * (e - s + 2) * np.longdouble(EPS) * np.abs(prod).sum()
            assert bound > 0
            worst = max(worst, float(err / bound))
        w[ci[s:e]] = 0
    return worst


def solve_residual_ratio(t, X, B):
    """max over rows i and columns c of |B - T X|_ic / (2 (len_i + 2) 2^-53 (|T||X|)_ic) for a
    triangular CSR T with every diagonal present: the componentwise backward-error bound of
    substitution, which holds for any order of summing a row.  Residual and bound in np.longdouble,
    segment sums over the CSR.  An entry with a zero bound must have a zero residual (ratio 0);
    a nonzero residual over a zero bound gives inf."""
    X = np.asarray(X, np.float64).reshape(t.num_rows, -1)
    B = np.asarray(B, np.float64).reshape(t.num_rows, -1)
    ro = t.row_offsets.astype(np.int64)
    lens = np.diff(ro)
    assert lens.min() >= 1
    prod = t.values.astype(np.longdouble)[:, None] * X.astype(np.longdouble)[t.column_indices]
    tx = np.add.reduceat(prod, ro[:-1], axis=0)
    ab = np.add.reduceat(np.abs(prod), ro[:-1], axis=0)
    res = np.abs(B.astype(np.longdouble) - tx)
    bound = 2 * (lens[:, None] + 2) * np.longdouble(EPS) * ab
    ratio = np.where(res == 0, np.longdouble(0), res / np.where(bound > 0, bound, np.longdouble(1)))
    ratio = np.where((bound == 0) & (res > 0), np.longdouble(np.inf), ratio)
    return float(ratio.max())
