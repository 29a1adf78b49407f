"""Non-finite x / X under the product kernels: which entries are poisoned, and the rule a product must meet.

Every product kernel pads and clamps for speed -- pad slots of value 0 at column 0, gathers clamped to a tile's
last nonzero or its column base, pair loads clamped to column n - 2, a run's longer rows' columns fetched for the
shorter rows too -- and selects the padding out, so that a row comes out non-finite exactly where the reference's
does: where it holds a nonzero in a column whose x is Inf or NaN (0.0 * Inf = NaN would show any pad that slipped
through).  bad_columns picks the columns the kernels pad and clamp to, poison puts one non-finite value into each
(in one panel column only, so that a row's other panel columns -- the other half of its double2 among them -- must
stay bit-exact), and check_nonfinite holds a product to the rule of test_gpu_slab.py::test_slab_nonfinite_x per
panel entry.  test_nonfinite_cases.py pins all three on the CPU; test_gpu_nonfinite.py runs the kernels.
"""
import numpy as np

from gpu_common import check_parity

VALUES = (np.inf, -np.inf, np.nan)  # bad column k of the list gets VALUES[k % 3]: column 0 gets +Inf
NUM_RANDOM = 4
MAX_PAIRS = 4


def prefix_pairs(a):
    """Every (shorter, longer, column): adjacent rows where the shorter's column list is a proper prefix of the
    longer's, and the first column the longer row has beyond it.  In row order of the pair's first row."""
    ro = a.row_offsets.astype(np.int64)
    ci = a.column_indices
    lens = np.diff(ro)
    if a.num_rows < 2:
        return []
    k = np.minimum(lens[:-1], lens[1:])
    cand = lens[:-1] != lens[1:]
    first = ci[np.minimum(ro[:-1], max(a.num_nonzeros - 1, 0))] if a.num_nonzeros else np.zeros(a.num_rows, ci.dtype)
    both = cand & (k > 0)
    same_first = np.zeros(a.num_rows - 1, bool)
    same_first[both] = first[:-1][both] == first[1:][both]
    out = []
    for i in np.flatnonzero(cand & ((k == 0) | same_first)):
        kk = int(k[i])
        if np.array_equal(ci[ro[i]:ro[i] + kk], ci[ro[i + 1]:ro[i + 1] + kk]):
            s, l = (i, i + 1) if lens[i] < lens[i + 1] else (i + 1, i)
            out.append((int(s), int(l), int(ci[ro[l] + kk])))
    return out


def pick_pairs(pairs, count=MAX_PAIRS):
    """Up to `count` of the pairs, evenly spaced over the list (so over the matrix's tiles), pairs whose shorter
    row is not empty before the others."""
    full = [p for p in pairs if p[3]] or pairs
    if len(full) <= count:
        return [p[:3] for p in full]
    idx = np.unique(np.linspace(0, len(full) - 1, count).round().astype(int))
    return [full[i][:3] for i in idx]


def bad_columns(a, plan, seed=0, num_random=NUM_RANDOM):
    """(columns, pairs): the columns of x to poison, in order, duplicates removed, and the prefix pairs
    [(shorter row, longer row, column)] behind the prefix-only ones.

    1. columns 0, n - 1 and n - 2 (pad slots hold column 0; the column-pair load is clamped to n - 2 and the last
       pair has one column left at n - 1);
    2. of the first, the middle and the last tile of `plan` that holds nonzeros: the smallest column among the
       tile's nonzeros (its column base: where elements outside the tile and records without a chunk gather) and
       the column of its last nonzero (where indices past the tile's end are clamped);
    3. of up to four pairs of adjacent rows of which one's column list is a proper prefix of the other's: the
       first column the longer row has beyond the prefix (a column "a shorter row lacks");
    4. num_random columns from default_rng(seed).  A case whose share of non-finite rows passes the cap of
       check_nonfinite lowers num_random; nothing else gives.
    """
    n = a.num_cols
    ci = a.column_indices
    cols = [c for c in (0, n - 1, n - 2) if 0 <= c < n]
    bounds = plan["bounds"]
    tiles = [t for t in range(plan["num_tiles"]) if int(bounds[t + 1][1]) > int(bounds[t][1])]
    for t in ([tiles[0], tiles[len(tiles) // 2], tiles[-1]] if tiles else []):
        n0, n1 = int(bounds[t][1]), int(bounds[t + 1][1])
        cols += [int(ci[n0:n1].min()), int(ci[n1 - 1])]
    lens = np.diff(a.row_offsets)
    pairs = pick_pairs([p + (int(lens[p[0]]),) for p in prefix_pairs(a)])
    cols += [c for _, _, c in pairs]
    if n:
        cols += [int(c) for c in np.random.default_rng(seed).integers(0, n, num_random)]
    return list(dict.fromkeys(cols)), pairs


def poison(X, cols):
    """A copy of X (n, or n x L) with one entry per bad column made non-finite: column cols[k] gets VALUES[k % 3]
    in panel column k % L; every other entry is X's."""
    P = np.array(X, np.float64, copy=True)
    V = P.reshape(P.shape[0], -1)
    L = V.shape[1]
    for k, c in enumerate(cols):
        V[c, k % L] = VALUES[k % 3]
    return P


def cleaned(X):
    """X with its non-finite entries replaced by 0.0."""
    return np.where(np.isfinite(X), X, 0.0)


def predicted_nonfinite(a, cols, L):
    """m x L bool: row i is non-finite in panel column j iff it holds a nonzero in a bad column poisoned in j."""
    hit = np.zeros((a.num_rows, L), bool)
    rows = np.repeat(np.arange(a.num_rows), np.diff(a.row_offsets))
    for k, c in enumerate(cols):
        hit[rows[a.column_indices == c], k % L] = True
    return hit


def input_conditions(a, gold, L, pairs=()):
    """The conditions on the oracle's output that keep a case from passing empty; (non-finite rows, mixed rows,
    prefix pairs split).  At least one non-finite row and at most a quarter of the rows (the quarter rounded up
    to a whole row: a one-row matrix's one row is its case); at L >= 2 a row non-finite in some panel columns
    and finite in others; of the prefix pairs at least one whose shorter row is finite while its longer is not.
    The all-empty matrix is exempt."""
    gold = np.asarray(gold).reshape(a.num_rows, -1)
    bad = ~np.isfinite(gold)
    rows_bad = bad.any(axis=1)
    mixed = rows_bad & ~bad.all(axis=1)
    split = sum(1 for s, l, _ in pairs if not rows_bad[s] and rows_bad[l])
    counts = (int(rows_bad.sum()), int(mixed.sum()), split)
    if a.num_nonzeros == 0:
        return counts
    assert 1 <= counts[0] <= -(-a.num_rows // 4), f"{counts[0]} of {a.num_rows} rows non-finite"
    if L >= 2:
        assert counts[1] >= 1, "no row non-finite in some panel columns and finite in others"
    if pairs:
        assert split >= 1, f"no prefix pair of {pairs} has a finite shorter and a non-finite longer row"
    return counts


def check_nonfinite(a, Y, gold, Yclean, gold_clean, X_clean, plan, L, pairs=()):
    """Y = A X of a poisoned X against the oracle's `gold`, entry by entry of the panel: NaN where gold has NaN,
    gold's infinities with their signs, and every entry finite in gold bit-equal to Yclean, the same handle's
    product of X_clean (X with its bad entries replaced by 0.0), which itself passes check_parity against
    gold_clean.  NaN bit patterns are not compared (x86 and the GPU sign them differently).

    plan: the tile plan the product ran on, or for a chunked width the list [(c0, c1, plan, width)] of its column
    chunks.  Returns input_conditions' counts."""
    m = a.num_rows
    Y, gold, Yclean, gold_clean = (np.asarray(v, np.float64).reshape(m, -1) for v in (Y, gold, Yclean, gold_clean))
    X_clean = np.asarray(X_clean, np.float64).reshape(a.num_cols, -1)
    assert Y.shape == gold.shape == Yclean.shape == gold_clean.shape == (m, L)
    assert np.all(np.isfinite(X_clean))
    counts = input_conditions(a, gold, L, pairs)
    if a.num_nonzeros == 0:  # whatever x holds, y is +0.0
        for v in (Y, Yclean):
            assert np.all(v == 0.0) and not np.signbit(v).any()
        return counts
    for c0, c1, p, w in (plan if isinstance(plan, list) else [(0, L, plan, L)]):
        check_parity(a, Yclean[:, c0:c1], gold_clean[:, c0:c1], X_clean[:, c0:c1], p, w)
    nan, fin = np.isnan(gold), np.isfinite(gold)
    wrong = np.argwhere(np.isnan(Y) != nan)
    assert wrong.size == 0, f"{len(wrong)} entries NaN on one side only, e.g. (row, column) {wrong[:3].tolist()}"
    wrong = np.argwhere(np.isfinite(Y) != fin)
    assert wrong.size == 0, f"{len(wrong)} entries finite on one side only, e.g. (row, column) {wrong[:3].tolist()}"
    inf = ~fin & ~nan
    wrong = np.argwhere(inf & (Y != gold))
    assert wrong.size == 0, f"{len(wrong)} infinities of the wrong sign, e.g. (row, column) {wrong[:3].tolist()}"
    wrong = np.argwhere(fin & (Y.view(np.uint64) != Yclean.view(np.uint64)))
    assert wrong.size == 0, (f"{len(wrong)} finite entries differ from the cleaned product, e.g. (row, column) "
                             f"{wrong[:3].tolist()}")
    return counts


# ---- shapes that need no GPU: generators in numpy (and scipy) alone -------------------------------------------------
def cpu_shapes():
    """name -> matrix maker, for test_nonfinite_cases.py."""
    from test_gpu_blk_records import boundary_matrix
    from test_gpu_blocks import kron_fem9
    from test_gpu_slab import with_rows
    from test_gpu_slab_mm import CASES as SLAB_MM
    from test_gpu_spmv import edge_case

    return {
        "short_first_r12_odd": lambda: boundary_matrix("short_first_r12_odd")[0],
        "short_first_r13": lambda: boundary_matrix("short_first_r13")[0],
        "kron9_6": lambda: kron_fem9(60, 50, 6),
        "kron9_8": lambda: kron_fem9(25, 20, 8),
        "hub_rect": SLAB_MM["hub_rect"],
        "long_rows_many_tiles": lambda: edge_case("long_rows_many_tiles"),
        "rows50": lambda: with_rows(12000, 12000, [50] * 12000, 3),
    }


def whole_row_plan(a, items=2048):
    """A hand-made plan of whole-row tiles: a tile ends at the first row end at or past `items` merge items."""
    ro = a.row_offsets.astype(np.int64)
    bounds = [(0, 0)]
    r = 0
    while r < a.num_rows:
        r1 = r + 1
        while r1 < a.num_rows and (r1 - r) + (ro[r1] - ro[r]) < items:
            r1 += 1
        bounds.append((r1, int(ro[r1])))
        r = r1
    return {"num_tiles": len(bounds) - 1, "bounds": np.array(bounds, np.int32), "modes": np.ones(len(bounds) - 1, np.uint8),
            "lanes": 256, "num_carries": 0}
