"""Matrices for the register-resident CG's instantiated shapes (test_resident_cases.py,
test_gpu_cg_resident_shapes.py), and a numpy restatement of the choice resident_build
(csrc/mspmv_cg_resident.hip) makes among them.

The stencils of test_gpu_cg_resident.py reach two of the nine (rows per thread, slots per row) shapes
and have regular rows, columns at a few common offsets and equal, non-empty row blocks.  mixed() has
none of that: rows of 1..maxlen entries whose columns are scattered over the whole matrix by a random
relabelling, and a run of diagonal-only rows that makes some merge-path row blocks hold about twice
the rows of the others, so 2 and 3 rows per thread are reached at a fraction of the rows a uniform
matrix needs.  Every matrix is symmetric, strictly diagonally dominant (so SPD) with ascending
columns; every generator is seeded; numpy only.
"""
import functools
import re

import numpy as np

# kResShapes of csrc/mspmv_cg_resident.hip, in its order (the first of equal rpt * nzr wins)
SHAPES = [(1, 4), (2, 4), (1, 8), (3, 4), (2, 7), (3, 7), (2, 8), (1, 16), (3, 8)]
ROWS_PER_BLOCK = 1024  # kRB: threads of a workgroup, one row slot each per rpt


def _csr(n, rows, cols, vals):
    """mspmv.CsrMatrix of the n x n entries (rows, cols, vals), no duplicates; columns ascending."""
    import mspmv

    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    ro = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=ro[1:])
    return mspmv.CsrMatrix.from_arrays(n, ro, cols, vals)


def mixed(n_diag, n_long, maxlen, seed, drop=0.15):
    """n_long 'long' rows carrying a wrapped band of (maxlen - 1) // 2 distinct random offsets d in
    [1, n_long/2 - 1) -- pairs (i, (i + d) mod n_long) -- plus, for even maxlen, the self-paired
    offset n_long / 2; every pair is dropped with probability `drop`, so rows hold 1..maxlen entries.
    The long rows are relabelled by a random permutation (columns all over the matrix), and n_diag
    diagonal-only rows are inserted as one run starting at row n_long // 3.  Off-diagonals U(-1, 1),
    mirrored; diagonal sum |off| + 1 + U(0, 1)."""
    rng = np.random.default_rng(seed)
    half = (maxlen - 1) // 2
    offs = 1 + rng.choice(n_long // 2 - 2, size=half, replace=False) if half else np.zeros(0, np.int64)
    i = np.arange(n_long, dtype=np.int64)
    pi = [i] * half
    pj = [(i + d) % n_long for d in offs]
    if maxlen % 2 == 0:
        assert n_long % 2 == 0, "an even maxlen needs the self-paired offset n_long / 2"
        pi.append(i[: n_long // 2])
        pj.append(i[: n_long // 2] + n_long // 2)
    pi = np.concatenate(pi) if pi else np.zeros(0, np.int64)
    pj = np.concatenate(pj) if pj else np.zeros(0, np.int64)
    keep = rng.uniform(0, 1, pi.size) >= drop
    pi, pj = pi[keep], pj[keep]
    v = rng.uniform(-1.0, 1.0, pi.size)
    perm = rng.permutation(n_long)
    at = n_long // 3
    label = np.where(perm < at, perm, perm + n_diag)  # the long rows' final numbers, around the run
    pi, pj = label[pi], label[pj]
    n = n_long + n_diag
    absum = np.bincount(pi, np.abs(v), n) + np.bincount(pj, np.abs(v), n)
    diag = absum + 1.0 + rng.uniform(0.0, 1.0, n)
    d = np.arange(n, dtype=np.int64)
    a = _csr(n, np.concatenate([pi, pj, d]), np.concatenate([pj, pi, d]), np.concatenate([v, v, diag]))
    assert np.diff(a.row_offsets).max() == maxlen, (np.diff(a.row_offsets).max(), maxlen)
    return a


def row_blocks(a, G):
    """resident_build's merge-path row bounds: block j starts at the last row i with
    i + row_offsets[i] <= (m + nnz) j // G; the last bound is m."""
    m, nnz = a.num_rows, a.num_nonzeros
    key = np.arange(m + 1, dtype=np.int64) + a.row_offsets.astype(np.int64)  # strictly ascending
    d = np.array([(m + nnz) * j // G for j in range(G + 1)], np.int64)
    rb = np.searchsorted(key, d, side="right") - 1
    rb[G] = m
    return rb


def predict_shape(a, G):
    """((rpt, nzr) or None, number of empty row blocks): the SHAPES entry with rpt >= ceil(largest
    block / 1024), nzr >= longest row and the smallest rpt * nzr, the first of equals."""
    rows = np.diff(row_blocks(a, G))
    rpt_need = max(-(-int(rows.max()) // ROWS_PER_BLOCK), 1)
    maxlen = int(np.diff(a.row_offsets).max())
    best = None
    for rpt, nzr in SHAPES:
        if rpt >= rpt_need and nzr >= maxlen and (best is None or rpt * nzr < best[0] * best[1]):
            best = (rpt, nzr)
    return best, int((rows == 0).sum())


# name: (n_diag, n_long, maxlen, seed, the shape resident_build selects with one row block per CU of
# a 256-CU device, None: no shape fits and the solve runs the two-kernel pipelined CG)
CASES = {
    "s14": (0, 3000, 4, 14, (1, 4)),
    "s18": (0, 3000, 8, 18, (1, 8)),
    "s116_12": (0, 3000, 12, 112, (1, 16)),
    "s116": (0, 3000, 16, 116, (1, 16)),
    "s24": (3000, 125000, 4, 24, (2, 4)),
    "s34": (6000, 245000, 4, 34, (3, 4)),
    "s27": (3000, 80000, 7, 27, (2, 7)),
    "s37": (6000, 160000, 7, 37, (3, 7)),
    "s28": (3000, 70000, 8, 28, (2, 8)),
    "s38": (6000, 140000, 8, 38, (3, 8)),
    "none_2x16": (3000, 56000, 12, 212, None),   # 2 rows per thread, 12 slots: no (2, >= 12) shape
    "none_3x16": (6000, 90000, 16, 316, None),   # 3 rows per thread, 16 slots
    "none_17": (0, 3000, 17, 17, None),          # a row of 17 entries
}
ACCEPTED = [k for k, c in CASES.items() if c[4] is not None]
DECLINED = [k for k, c in CASES.items() if c[4] is None]

# Few rows: with m < 256 most row blocks are empty (their workgroups publish zero partials); around
# 64, 256 and 1024 rows the blocks' sizes change.  An odd m has no self-paired offset: maxlen 3.
TINY_M = [6, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
TINY = ["one", "two"] + [f"m{m}" for m in TINY_M]


@functools.lru_cache(maxsize=None)
def matrix(name):
    """The named case (of CASES or TINY) as an mspmv.CsrMatrix, built once per session; do not modify."""
    import mspmv

    if name == "one":
        a = mspmv.CsrMatrix.from_arrays(1, [0, 1], [0], [2.0])
    elif name == "two":
        a = mspmv.CsrMatrix.from_arrays(2, [0, 2, 4], [0, 1, 0, 1], [2.0, -1.0, -1.0, 2.0])
    elif name in CASES:
        n_diag, n_long, maxlen, seed, _ = CASES[name]
        a = mixed(n_diag, n_long, maxlen, seed)
    else:
        m = int(name[1:])
        a = mixed(0, m, 4 if m % 2 == 0 else 3, 1000 + m)
    for arr in (a.row_offsets, a.column_indices, a.values):
        arr.setflags(write=False)
    return a


def maxlen_of(name):
    if name in CASES:
        return CASES[name][2]
    return {"one": 1, "two": 2}.get(name) or (4 if int(name[1:]) % 2 == 0 else 3)


def rhs(m):
    return np.random.default_rng(1).uniform(0, 1, m)


TOL = 1e-10
MAX_ITERS = 500
_RESIDENT_NAME = re.compile(r"^k_cg_resident<(\d+),(\d+),(\w+)> x (\d+)$")


def resident_shape(kname, form):
    """(rpt, nzr, G) of a resident kernel's name, "k_cg_resident<rpt,nzr,form> x G"; fails on any
    other name: a solve the resident path declined or that fell back after a stall reports the
    pipelined kernels."""
    assert "stall" not in kname, kname
    m = _RESIDENT_NAME.match(kname)
    assert m, kname
    assert m.group(3) == form, kname
    return int(m.group(1)), int(m.group(2)), int(m.group(4))


def _solve_reference(orc, a):
    b = rhs(a.num_rows)
    x, it, hist = orc.cg_single(a, b, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
    res = float(np.linalg.norm(b - orc.spmv_gold(a, x)) / np.linalg.norm(b))
    for arr in (b, x, hist):
        arr.setflags(write=False)
    return b, x, it, hist, res


@functools.lru_cache(maxsize=None)
def reference(orc, name):
    """(b, x, iterations, history, true residual) of the oracle's fp64 CGSolveSingle on the
    named case (tolerance 1e-10, at most 500 iterations), solved once per session and shared; the
    arrays are read-only."""
    return _solve_reference(orc, matrix(name))


@functools.lru_cache(maxsize=None)
def perturbed_reference(orc, name, eps=1e-6):
    """reference() of the named case with its first off-diagonal pair -- (0, j) and (j, 0), j the
    first off-diagonal column of row 0 -- changed by eps: what a kernel that got one value slightly
    wrong would compute.  The bars must tell it from the unperturbed solve."""
    import mspmv

    a = matrix(name)
    ro, ci = a.row_offsets, a.column_indices
    k = next(k for k in range(ro[0], ro[1]) if ci[k] != 0)
    j = int(ci[k])
    k2 = int(ro[j]) + int(np.nonzero(ci[ro[j]:ro[j + 1]] == 0)[0][0])
    va = a.values.copy()
    va[k] += eps
    va[k2] += eps
    return _solve_reference(orc, mspmv.CsrMatrix.from_arrays(a.num_rows, ro, ci, va))


def check_bars(orc, label, a, ref, x, it, hist, st):
    """A solve (x, iterations, history, status) of matrix a against ref = reference(...).  The bars
    of test_gpu_cg.py and test_gpu_cg_resident.py: status 0, iteration counts equal (iter_match),
    every recorded ||r_k||/||b|| within 1e-10 of the oracle's, x within 1e-8 relative, true residual
    <= max(10 x the oracle's, 1e-13).  One bar more: x within 1e-8 of the oracle's in the maximum
    norm too.  Both solves run the same iterations and stop at the same one, so their x differ by the
    rounding of differently ordered dot products carried through at most 43 iterations of a matrix
    whose condition number is below 40 (diagonal dominance: eigenvalues in [1, 2 sum|off| + 2]) --
    orders below 1e-8 in any norm; but a change confined to a row or two of 70,000, which a wrong
    value or row slot makes, moves the 2-norm bars by 1/sqrt(m) of its size and this one in full.
    The figures are printed before they are asserted."""
    from test_gpu_cg import iter_match

    b, xo, it_o, ho, res_o = ref
    k = min(len(hist), len(ho))
    dev = float(np.max(np.abs(hist[:k] - ho[:k]))) if k else 0.0
    xerr = float(np.linalg.norm(x - xo) / np.linalg.norm(xo))
    xmax = float(np.max(np.abs(x - xo)) / np.max(np.abs(xo)))
    res = float(np.linalg.norm(b - orc.spmv_gold(a, x)) / np.linalg.norm(b))
    ratio = res / res_o if res_o else float("inf")
    print(f"\n{label}: status {st}, iterations {it} (oracle {it_o}), worst history deviation {dev:.3e}, "
          f"x error {xerr:.3e} (max norm {xmax:.3e}), true residual {res:.3e} = {ratio:.3f} x the oracle's")
    assert st == 0, f"status {st}"
    assert it_o < MAX_ITERS
    assert iter_match(it, it_o, ho, TOL), f"iterations {it} against the oracle's {it_o}"
    assert len(hist) == it and k >= min(it, it_o), f"history length {len(hist)} of {it} iterations"
    assert dev <= 1e-10, f"history deviation {dev:.3e}"
    assert xerr <= 1e-8, f"x error {xerr:.3e}"
    assert xmax <= 1e-8, f"x error in the maximum norm {xmax:.3e}"
    assert res <= max(10 * res_o, 1e-13), f"true residual {res:.3e} against the oracle's {res_o:.3e}"
    return dev, xerr, ratio
