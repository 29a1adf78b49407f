"""CPU: what test_gpu_slab_edges.py relies on, pinned without a plan -- every case of slab_cases.py is a valid CSR
matrix with the row lengths, run lengths and dimensions it claims, a finite gold product and a bound that is not
vacuous; the features of slab_chunks lie inside one merge-path block each and its hub row over four; the numpy
model of k_spmv_sell's order is a reordered sum (exact on short runs); and the lanes-per-run rule of the planners,
enumerated, can choose the lg values the cases claim and no others.
"""
import numpy as np
import pytest

import slab_cases as sc
from gpu_common import abs_bound

WIDE = {"sell_segs_255", "sell_segs_256"}


def test_cases_are_all_listed():
    assert sorted(sc.CASES) == sorted([
        "sell_packed", "sell_one_seg", "sell_edges", "sell_segs_255", "sell_segs_256", "sell_pieces_1024",
        "sell_pieces_1025", "slab_chunks", "slab_empty_rows", "slab_chunks_255", "slab_chunks_256", "mm_edges",
        "mm_short_rows", "mm_dense", "mm_hub", "mm_chunks_127", "mm_chunks_128"] + [f"mm_chunks_{k}" for k in (1, 2, 3, 4, 5, 9)])
    assert all(c.purpose and c.n > 0 for c in sc.CASES.values())


@pytest.mark.parametrize("name", list(sc.CASES))
def test_case_is_what_it_claims(orc, name):
    case, a = sc.CASES[name], sc.matrix(name)
    ro, ci = a.row_offsets.astype(np.int64), a.column_indices.astype(np.int64)
    lens = np.diff(ro)
    assert a.num_cols == case.n and ro[0] == 0 and ro[-1] == ci.size == a.values.size and np.all(lens >= 0)
    assert ci.min() >= 0 and ci.max() < a.num_cols
    inner = np.ones(ci.size, bool)
    inner[ro[:-1][lens > 0]] = False                     # not a row's first nonzero: larger than the one before
    assert np.all(np.diff(ci)[inner[1:]] > 0), "columns not sorted and distinct within a row"
    assert a.num_nonzeros <= 250000 or name in WIDE, a.num_nonzeros
    assert case.row_lengths <= set(lens.tolist()), sorted(case.row_lengths - set(lens.tolist()))
    if case.run_w:
        have = sc.run_lengths(a, case.run_w, case.groups)
        assert case.run_lengths <= have, sorted(case.run_lengths - have)
    x = sc.x_for(a)
    gold = orc.spmv_gold(a, x)
    assert np.all(np.isfinite(gold)) and np.all(np.abs(a.values) < 1) and np.all(a.values != 0)
    bound, _ = abs_bound(a, x)
    assert 2 * int((bound[:, 0] > 0).sum()) >= a.num_rows


def rows_with(a, col):
    return set((np.searchsorted(a.row_offsets, np.flatnonzero(a.column_indices == col), side="right") - 1).tolist())


def test_sell_packed_edges():
    a = sc.matrix("sell_packed")
    n, W = a.num_cols, sc.SELL_W
    lo = sc.group_lo(n, 4)
    assert n >= 43009 and -(-n // W) == 4 and a.num_rows == 3 * 4095
    assert all(lo[g + 1] - lo[g] <= W for g in range(4))          # one segment per (block, group)
    ro, ci = a.row_offsets, a.column_indices
    lens = np.diff(ro)
    b0 = ci[:ro[4095]]
    assert b0.max() < lo[1]                                       # row block 0 lies in group 0
    assert 1 <= lens[4094] <= 4 and np.all(lens[2048:4095] <= 8)  # packed runs in local rows >= 2,048 and 4,094
    for k, need in ((1, 512), (2, 256), (3, 128), (4, 128), (5, 64), (6, 64), (7, 64), (8, 64)):
        assert (lens[:4095] == k).sum() > need + 64, k            # each length leads a slice of its own form
    assert (lens[:4095] == 1).sum() > 2 * 512                     # and the 8 x 1 form a second one
    assert ((lens[:4095] > 8) & (lens[:4095] <= 64)).sum() == 57  # 7 full medium slices and one run alone
    for g in (1, 2, 3):                                           # rows across every group boundary
        assert rows_with(a, lo[g] - 1) & rows_with(a, lo[g])
    assert ci[ro[8190]:].max() < lo[3]                            # row block 2: nothing in the last group
    one_group = (lens <= 8) & (lens > 0)
    first, last = ci[ro[:-1]], ci[ro[1:] - 1]
    g_of = lambda c: np.searchsorted(np.asarray(lo[1:4]), c, side="right")
    assert (one_group & (g_of(first) == g_of(last))).sum() >= 1000


def test_sell_one_group_edges():
    a = sc.matrix("sell_edges")
    n, W = a.num_cols, sc.SELL_W
    assert n == 7 * W + 1 and rows_with(a, n - 1) and min(rows_with(a, n - 1)) < sc.SELL_EDGES_RICH
    assert rows_with(a, 0) == {0}                                 # block 0's slabs start at column 0
    assert rows_with(a, 3 * W - 1) & rows_with(a, 3 * W)          # offsets 14,335 and 0 of neighbouring segments
    ro, ci = a.row_offsets.astype(np.int64), a.column_indices.astype(np.int64)
    rich = ci[:ro[sc.SELL_EDGES_RICH]]
    rows = np.repeat(np.arange(sc.SELL_EDGES_RICH), np.diff(ro[:sc.SELL_EDGES_RICH + 1]))
    runs = [np.unique(rows[rich // W == s], return_counts=True)[1] for s in range(8)]
    assert [len(r) for r in runs] == [10, 2, 1025, 961, 129, 0, 1, 1]
    assert [-(-len(r) // 64) for r in runs[2:5]] == [17, 16, 3] and runs[1].min() > 64 and runs[0].max() <= 8
    rest = ci[ro[sc.SELL_EDGES_RICH]:]
    assert rest.min() >= 6 * W and rest.max() < 7 * W             # the later rows add to segment 6 alone
    total = a.num_rows + a.num_nonzeros                           # the rich rows fit the first of eight row blocks
    assert sc.SELL_EDGES_RICH + ro[sc.SELL_EDGES_RICH] <= -(-total // 8)
    b = sc.matrix("sell_one_seg")
    assert b.num_cols == W and set(np.diff(b.row_offsets).tolist()) >= set(range(1, 65))


@pytest.mark.parametrize("name,k,stride", [("sell_segs_255", 255, sc.SELL_W), ("sell_segs_256", 256, sc.SELL_W),
                                           ("slab_chunks_255", 255, sc.SLAB_W), ("slab_chunks_256", 256, sc.SLAB_W),
                                           ("mm_chunks_127", 127, 1024), ("mm_chunks_128", 128, 1024)]
                         + [(f"mm_chunks_{k}", k, 1024) for k in (1, 2, 3, 4, 5, 9)])
def test_limit_cases(name, k, stride):
    """Row 0 holds one entry in each of k slabs (segments), every other row one entry within 100 columns of one of
    them, and row 0 lies whole in the first block of a 16-block (and any coarser) merge-path plan."""
    a = sc.matrix(name)
    ro, ci = a.row_offsets, a.column_indices
    assert a.num_cols == k * stride and np.array_equal(ci[:ro[1]], np.arange(k) * stride)
    assert np.all(ci % stride < 100) and set((ci // stride).tolist()) == set(range(k))
    assert np.all(np.diff(ro)[1:] == 1)
    assert (a.num_rows + a.num_nonzeros) // 24 > k + 1            # a block's merge items, down to 24 blocks


def test_sell_pieces_cases():
    for name, k in (("sell_pieces_1024", 1024), ("sell_pieces_1025", 1025)):
        a = sc.matrix(name)
        assert a.num_rows == k <= 4095 and -(-a.num_cols // sc.SELL_W) == 8
        assert a.column_indices.max() < a.num_cols // 8 <= sc.SELL_W and np.all(np.diff(a.row_offsets) == 65)


def test_slab_chunks_layout():
    """Each feature's rows lie strictly inside one block of the 16-block merge path (step 8,192 exactly), each in a
    block and a slab of its own; the hub row starts inside a block and covers the next two whole."""
    rows, n, spans = sc.slab_chunks_layout()
    a = sc.matrix("slab_chunks")
    S = sc.SLAB_STEP
    ro = a.row_offsets.astype(np.int64)
    assert n % sc.SLAB_W == 1 and rows_with(a, n - 1) and rows_with(a, 4095) & rows_with(a, 4096)
    assert a.num_rows + a.num_nonzeros == 16 * S and a.num_rows <= 16 * 2047
    blocks = {}
    for t, (name, slab, lens) in enumerate(sc._features(), start=1):
        r0, r1 = spans[name]
        i0, i1 = r0 + ro[r0], r1 + ro[r1]                         # the rows' merge items [i0, i1)
        assert t * S + 64 < i0 and i1 < (t + 1) * S - 64, name
        c = a.column_indices[ro[r0]:ro[r1]]
        assert c.min() // sc.SLAB_W == c.max() // sc.SLAB_W == slab and np.array_equal(np.diff(ro[r0:r1 + 1]), lens)
        blocks[name] = t
        rb0, rb1 = np.searchsorted(np.arange(a.num_rows) + ro[:-1], [t * S, (t + 1) * S])
        others = np.concatenate([a.column_indices[ro[rb0]:ro[r0]], a.column_indices[ro[r1]:ro[rb1]]])
        assert others.max() < 2 * sc.SLAB_W                       # the block's other rows stay in the first two slabs
        assert rb1 - rb0 <= 2047
    r0, r1 = spans["long_runs"]
    assert r0 // 4095 == (r1 - 1) // 4095                         # ... and inside one 4,095-row block of mode 2
    h = spans["hub"][0]
    i0, i1 = h + ro[h], h + 1 + ro[h + 1]
    assert i0 // S == sc.HUB_BLOCK and i1 // S == sc.HUB_BLOCK + 3 and i0 % S > S // 8 and i1 % S > S // 8
    assert ro[h] > ro[h - 1] and ro[h + 2] > ro[h + 1]            # short rows before and after it
    # the lg each feature's chunk gets (mode 1: 512 threads): 0, 1, 2, 3 and 4 all occur
    lg = {name: sc.lg_choice(sum(k <= 64 for k in lens), -(-sum(k for k in lens if k <= 64) // max(1, sum(k <= 64 for k in lens))), 512)
          for name, _, lens in sc._features()}
    assert lg["full_chunk"] == 4 and lg["entries_1024"] == 0 and lg["lg1"] == 1 and lg["lg2"] == 2 and lg["lg3"] == 3


def test_lg_rule_reach():
    """Which lg the planners' cost rule can choose at all.  k_spmv_slab sums runs of <= 64 by groups (longer ones by
    whole waves), so the mean run is <= 64 and 32 or 64 lanes per run never cost less than 16: lg 5 and 6 are
    unreachable in both shapes.  k_spmm_slab has no long-run path: every lg up to its butterfly's width occurs."""
    for threads, entries in ((512, 1024), (1024, 2048)):
        reach = {sc.lg_choice(r, mean, threads) for r in range(1, entries + 1) for mean in range(1, 65)}
        assert reach == {0, 1, 2, 3, 4}, (threads, reach)
    for cfg, (L, threads, chunk) in {0: (8, 512, 1024), 1: (8, 1024, 2048), 2: (16, 1024, 2048), 3: (16, 512, 1024)}.items():
        lg_max = 4 if L == 8 else 3
        reach = {sc.lg_choice(r, -(-nz // r), threads, L // 2, lg_max)
                 for r in (1, 2, 3, 5, 8, 16, 32, 64, 128, 256, sc.MM_ENTRIES[cfg]) for nz in range(r, chunk + 1, 7)}
        assert reach == set(range(lg_max + 1)), (cfg, reach)


def test_mm_cases_shapes():
    a = sc.matrix("mm_edges")
    lens = np.diff(a.row_offsets)
    assert set(lens.tolist()) >= set(range(1, 10)) | {15, 16, 17, 63, 64, 65}
    assert rows_with(a, a.num_cols - 1) == {a.num_rows - 1} and lens[-1] == 1
    assert a.column_indices[:-1].max() < a.num_cols - 300        # a gap wider than any segment before column n - 1
    touched = np.zeros(a.num_cols, bool)
    touched[a.column_indices] = True
    assert touched[:3 * 3000].mean() > 0.95                       # (nearly) contiguous: segments fill to cfg.cols
    h = sc.matrix("mm_hub")
    hl = np.diff(h.row_offsets)
    r = int(np.argmax(hl))
    c = h.column_indices[h.row_offsets[r]:h.row_offsets[r + 1]]
    assert hl[r] == 5000 and c[-1] - c[0] == 4999 and 0 < r < h.num_rows - 1
    assert hl[r] > 2 * -(-(h.num_rows + h.num_nonzeros) // 8) + 300   # over three blocks even at 8 blocks
    s = sc.matrix("mm_short_rows")
    for cfg in (0, 1):                                            # a block at the row cap lists more runs than a chunk
        assert sc.MM_ROWS[cfg] > sc.MM_ENTRIES[cfg]
    for cfg in (2, 3):                                            # ... which 2 and 3 cannot: a segment holds <= rows + 1 runs
        assert sc.MM_ROWS[cfg] + 1 < sc.MM_ENTRIES[cfg]
    assert np.all(np.diff(s.row_offsets) == 1) and s.num_rows == 6000


def test_sell_model_is_a_reordered_sum(orc):
    """The numpy model of k_spmv_sell's order: exact against the sequential sum on short runs, within the
    reordering bound on medium and long ones, and different from it somewhere (the order matters)."""
    rng = np.random.default_rng(3)
    differs = 0
    for k in [1, 2, 7, 8, 9, 16, 17, 33, 64, 65, 511, 512, 513, 1025, 5000]:
        p = rng.uniform(-1, 1, k)
        seq = np.float64(0.0)
        for v in p:
            seq = seq + v
        got = sc.sell_run_sum(p)
        if k <= 8:
            assert got == seq
        assert abs(got - seq) <= 2 * (k + 1) * 2.0 ** -53 * np.abs(p).sum()
        differs += got != seq
    assert differs >= 3
    a = sc.matrix("sell_one_seg")
    x = sc.x_for(a)
    y, gold = sc.sell_model(a, x), orc.spmv_gold(a, x)
    short = np.diff(a.row_offsets) <= 8
    assert np.array_equal(y[short], gold[short]) and short.sum() >= 2400
    bound, lens = abs_bound(a, x)
    assert np.all(np.abs(y - gold) <= 2 * (lens + 1) * 2.0 ** -53 * bound[:, 0])
    assert (y[~short] != gold[~short]).sum() >= 20


def test_stat_names_follow_the_header():
    """mspmv.SLAB_STATS spells out include/mspmv.h's MSPMV_SLAB_STAT_* in order: each enumerator's name, lower case,
    sits at its value, and the ranged ones (LG0, PACK_1X5, UNPACKED_1, MEDIUM_2) are followed by their successors."""
    import os
    import re

    import mspmv

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mspmv.h")).read()
    body = text[text.index("enum mspmv_slab_stat {"):text.index("MSPMV_API mspmv_status mspmv_slab_plan_stats")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    values, nxt = {}, 0
    for name, expr in re.findall(r"MSPMV_SLAB_STAT_(\w+)\s*(?:=\s*([^,}]+))?[,}\s]", body):
        if expr.strip():
            nxt = eval(re.sub(r"MSPMV_SLAB_STAT_(\w+)", lambda m: str(values[m.group(1)]), expr))
        values[name] = nxt
        nxt += 1
    assert values.pop("COUNT") == len(mspmv.SLAB_STATS) == len(set(mspmv.SLAB_STATS)) and len(values) >= 30
    for name, v in values.items():
        assert mspmv.SLAB_STATS[v] == name.lower(), (name, v)
    i = values["LG0"]
    assert mspmv.SLAB_STATS[i:i + 7] == [f"lg{k}" for k in range(7)] and values["SEGMENTS"] == i + 7
    i = values["PACK_1X5"]
    assert mspmv.SLAB_STATS[i:i + 4] == [f"pack_1x{k}" for k in range(5, 9)] and values["UNPACKED_1"] == i + 4
    i = values["UNPACKED_1"]
    assert mspmv.SLAB_STATS[i:i + 8] == [f"unpacked_{k}" for k in range(1, 9)] and values["MEDIUM_2"] == i + 8
    i = values["MEDIUM_2"]
    assert mspmv.SLAB_STATS[i:i + 7] == [f"medium_{k}" for k in range(2, 9)] and values["SLICES_ODD"] == i + 7
