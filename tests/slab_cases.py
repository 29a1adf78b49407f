"""Small matrices cut to the layout edges of the column-slab and sliced-ELL products (mspmv_slab.hip).

Each case is a deterministic generator with a stated purpose: which packed field, table or pipeline edge of
k_spmv_sell, k_spmv_slab or k_spmm_slab it is built to reach.  What a case claims without a plan -- its row
lengths, the run lengths per (row, column group, slab), its dimensions -- test_slab_cases.py checks on the CPU;
that the plan really took the form, test_gpu_slab_edges.py reads from GpuCsr.slab_plan_stats.  The GPU tests size
blocks with set_cu_limit(8): eight CUs give the merge-path plans 16 blocks (8 for the one-block-per-CU SpMM
shapes), the column-group plans 8 / groups row blocks, so a small matrix puts many rows into one block.

The numbers the cases are cut to (mspmv_internal.h, kSlabMmCfgs): k_spmv_slab mode 1 -- slabs of 4,096 columns,
chunks of 2,048 nonzeros and 1,024 runs, runs over 64 by whole waves (8 per block), 2,047 rows and 255 chunks per
block; mode 2 -- 8,192 / 4,096 / 2,048, 16 waves, 4,095 rows.  k_spmv_sell -- slabs of 14,336 columns from the
block's first column, runs <= 8 short, <= 64 medium, longer in pieces of 512; 4,095 rows, 255 segments per block,
1,024 pieces per segment.  k_spmm_slab -- configurations (L, threads, rows, cols, chunk, entries): 0 (8, 512, 384,
256, 1024, 256), 1 (8, 1024, 768, 512, 2048, 512), 2 (16, 1024, 256, 320, 2048, 512), 3 (16, 512, 192, 128, 1024,
256); 127 chunks per block.
"""
import functools
from typing import Callable, NamedTuple

import numpy as np

import mspmv

SELL_W = 14336       # kSlabCfgs[2].cols
SLAB_W = 4096        # kSlabCfgs[0].cols
SLAB_STEP = 8192     # slab_chunks: merge items per block of the 16-block plan
MM_COLS = {0: 256, 1: 512, 2: 320, 3: 128}
MM_ENTRIES = {0: 256, 1: 512, 2: 512, 3: 256}
MM_ROWS = {0: 384, 1: 768, 2: 256, 3: 192}
MM_L = {0: 8, 1: 8, 2: 16, 3: 16}


class Case(NamedTuple):
    purpose: str
    make: Callable              # () -> mspmv.CsrMatrix
    row_lengths: frozenset      # row lengths the case claims to hold (a subset of its rows' lengths)
    run_lengths: frozenset      # run lengths per (row, group, slab of run_w columns from the group's first)
    run_w: int = 0              # 0: no run claim
    groups: int = 1             # column groups the run claim is cut by: group g = [g n / G, (g + 1) n / G)
    n: int = 0                  # the column count the case claims


def build(n, rows, seed):
    """CSR from a list of per-row column arrays (sorted here), values uniform in (-1, 1)."""
    lens = np.fromiter((len(r) for r in rows), np.int64, len(rows))
    ro = np.zeros(len(rows) + 1, np.int64)
    ro[1:] = np.cumsum(lens)
    ci = np.concatenate([np.sort(np.asarray(r, np.int64)) for r in rows if len(r)] or [np.zeros(0, np.int64)])
    va = np.random.default_rng(seed).uniform(-1, 1, ci.size)
    return mspmv.CsrMatrix.from_arrays(n, ro.astype(np.int32), ci.astype(np.int32), va)


def pick(rng, lo, hi, k):
    """k distinct columns of [lo, hi)."""
    return lo + rng.choice(hi - lo, k, replace=False)


def group_lo(n, G):
    return [g * n // G for g in range(G + 1)]


def run_lengths(a, W, G=1):
    """The set of run lengths: nonzeros of one row in one slab of W columns counted from its group's first column."""
    n = a.num_cols
    lo = np.asarray(group_lo(n, G)[:-1], np.int64)
    ci = a.column_indices.astype(np.int64)
    rows = np.repeat(np.arange(a.num_rows, dtype=np.int64), np.diff(a.row_offsets))
    g = np.searchsorted(lo, ci, side="right") - 1
    slab = (ci - lo[g]) // W
    key = (rows * G + g) * (n // W + 2) + slab
    return set(np.unique(key, return_counts=True)[1].tolist())


# ---- k_spmv_sell ------------------------------------------------------------------------------------------------------
SHORT_CYCLE = [1] * 8 + [2] * 3 + [3] * 2 + [4] * 2 + [5, 6, 7, 8]   # 19 rows: enough of each length for every form
MEDIUMS = list(range(64, 8, -1)) + [9]   # eight per slice, longest first: slots per lane 8, 7, .., 2, then one run alone
SELL_LONGS = [65, 512, 513, 1025]        # one piece, one full piece, two, three


def sell_packed():
    n, G = 43009, 4                      # four slabs' worth of columns: four groups of 10,752 (one slab each)
    lo = group_lo(n, G)
    rng = np.random.default_rng(11)
    rows = [pick(rng, 0, lo[1], k) for k in MEDIUMS + SELL_LONGS]
    while len(rows) < 4095:              # row block 0, all in group 0: short runs of every length, up to row 4,094
        rows.append(pick(rng, 0, lo[1], SHORT_CYCLE[len(rows) % 19]))
    for i in range(4095):                # row block 1: rows across the group boundaries, then scattered rows
        if i < 300:
            b = lo[1 + i % 3]
            rows.append(np.array([b - 2, b - 1, b, b + 1]))
        else:
            rows.append(pick(rng, 0, n, 12))
    for i in range(4095):                # row block 2: nothing in the last group
        rows.append(pick(rng, 0, lo[3], 5))
    return build(n, rows, 12)


def sell_one_seg():
    n = SELL_W
    rng = np.random.default_rng(21)
    rows = []
    for k in (8, 7, 6, 5):
        rows += [pick(rng, 0, n, k) for _ in range(300)]
    rows += [pick(rng, 0, n, k) for k in MEDIUMS + SELL_LONGS + [1024, 1536, 2049]]
    rows.append(np.arange(n))            # the whole slab: 28 pieces, the last offset 14,335
    for k in (4, 3, 2, 1):
        rows += [pick(rng, 0, n, k) for _ in range(300)]
    return build(n, rows, 22)


SELL_EDGES_RICH = 1028   # rows 0 .. 1,027 hold the targeted segments; they lie in block 0


def sell_edges():
    W = SELL_W
    n = 7 * W + 1                        # the last segment of a block that starts at column 0 holds one column
    rng = np.random.default_rng(31)
    rows = []
    for i in range(1025):
        c = [2 * W + (i * 13) % (W - 1)]              # segment 2: 1,025 runs, 17 slices
        if i < 10:
            c.append(i * 7)                           # segment 0 (column 0 in row 0): 1 slice
        if i < 961:
            c.append(3 * W + 1 + (i * 11) % (W - 1))  # segment 3: 961 runs, 16 slices
        if i < 129:
            c.append(4 * W + i)                       # segment 4: 129 runs, 3 slices
        if i == 1:
            c += [3 * W - 1, 3 * W]                   # a segment's last offset, 14,335, and the next one's first
        rows.append(np.array(c))
    rows.append(pick(rng, W, 2 * W, 100))             # segment 1: long runs only (one piece, two pieces)
    rows.append(pick(rng, W, 2 * W, 600))
    rows.append(np.array([6 * W + 5, n - 1]))         # segments 6 and 7; segment 5 stays untouched
    assert len(rows) == SELL_EDGES_RICH
    for _ in range(5000):                             # the other blocks' work, in segment 6 alone
        rows.append(pick(rng, 6 * W, 7 * W, 8))
    return build(n, rows, 32)


def one_row_at_stride(k, stride, seed, extra=4000):
    """Row 0 with k entries at the given stride; `extra` one-element rows inside 100 columns of row 0's entries."""
    rows = [np.arange(k) * stride] + [np.array([(i % k) * stride + (i * 7) % 100]) for i in range(1, extra + 1)]
    return build(k * stride, rows, seed)


def sell_pieces(k):
    """k runs of 65 in one segment of a plan of eight column groups and one row block: k one-piece long runs."""
    n = 7 * SELL_W + 1
    rng = np.random.default_rng(41)
    return build(n, [pick(rng, 0, n // 8, 65) for _ in range(k)], 42)


# ---- k_spmv_slab ------------------------------------------------------------------------------------------------------
def _features():
    """(name, slab, [row lengths]) of slab_chunks, one per block 1, 2, ...: each in a slab of its own."""
    return [
        ("full_chunk", 2, [64] * 32),                 # a chunk of exactly 2,048 nonzeros, runs of 64, lg 4
        ("chunk_plus_one", 3, [65] + [64] * 31),      # 2,049: a long run of 65, a run cut at the chunk's end
        ("entries_1024", 4, [1] * 1024),              # exactly 1,024 runs, lg 0
        ("entries_1025", 5, [1] * 1025),              # cut at the entry limit
        ("long_runs", 6, [70] * 20),                  # more long runs in a chunk than a block has waves (8, 16)
        ("lg2", 7, [16] * 128),
        ("lg1", 8, [8] * 256),
        ("lg3", 9, [32] * 64),
    ]


HUB_BLOCK = 10           # slab_chunks: the hub row starts in the middle of this block and spans 3.2 blocks


@functools.lru_cache(maxsize=None)
def slab_chunks_layout():
    """(rows, n, spans): the matrix's rows, and per feature (and "hub") its [first, last) row."""
    S = SLAB_STEP
    n = 16 * SLAB_W + 1                               # n = 4096 k + 1: the last slab holds column n - 1 alone
    rng = np.random.default_rng(51)
    rows = [np.array([4095, 4096])]                   # a slab's last column and the next one's first
    items = [3]
    spans = {}

    def put(r):
        rows.append(r)
        items[0] += len(r) + 1

    def fill_to(target):                              # filler: rows of 8 in the first two slabs
        while items[0] + 9 <= target:
            put(pick(rng, 0, 2 * SLAB_W, 8))

    for t, (name, slab, lens) in enumerate(_features(), start=1):
        size = sum(lens) + len(lens)
        fill_to(t * S + (S - size) // 2)
        spans[name] = (len(rows), len(rows) + len(lens))
        for k in lens:
            put(pick(rng, slab * SLAB_W, (slab + 1) * SLAB_W, k))
    fill_to(HUB_BLOCK * S + S // 2)
    spans["hub"] = (len(rows), len(rows) + 1)
    put(pick(rng, 0, n, 3 * S + S // 5))              # blocks 10 .. 13: two of them hold only its middle
    fill_to(16 * S - 11)
    rem = 16 * S - items[0]                           # the last row brings the total to 16 S: the step is S exactly
    put(np.concatenate([pick(rng, 0, 2 * SLAB_W, rem - 2), [n - 1]]))
    assert items[0] == 16 * S
    return rows, n, spans


def slab_chunks():
    rows, n, _ = slab_chunks_layout()
    return build(n, rows, 52)


def slab_empty_rows():
    """Leading, trailing and a long stretch of empty rows: the 2,047-row cap (4,095 in mode 2), not the work, sets the
    block count."""
    n = 2 * SLAB_W + 1
    rng = np.random.default_rng(61)
    e = np.zeros(0, np.int64)
    rows = [e] * 5000 + [pick(rng, 0, n, 3) for _ in range(10000)] + [e] * 10000
    rows += [pick(rng, 0, n, 3) for _ in range(10000)] + [e] * 5000
    return build(n, rows, 62)


# ---- k_spmm_slab ------------------------------------------------------------------------------------------------------
MM_CYCLE = [3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1, 2]   # every lg's 4-deep loop and its remainder


def mm_edges():
    """Row i holds MM_CYCLE[i % 15] consecutive columns from 3 i: a block's columns are (nearly) one contiguous
    range a few segments wide, so segments of exactly cfg.cols columns are followed by one that starts at the next
    column; 300 untouched columns, then column n - 1 in the last row alone: a one-column segment."""
    m = 4000
    n = 3 * m + 300
    rows = [np.arange(3 * i, min(3 * i + MM_CYCLE[i % 15], 3 * m)) for i in range(m - 1)] + [np.array([n - 1])]
    return build(n, rows, 71)


def mm_short_rows():
    """6,000 one-element rows, two to a column: blocks at the row cap, a segment with more runs than a chunk lists."""
    return build(3000, [np.array([i // 2]) for i in range(6000)], 72)


def mm_dense():
    """Forty consecutive rows share the same 65 consecutive columns: a segment holds several chunks' worth of
    nonzeros at every configuration, full chunks, and (1,024 and 2,048 are no multiples of 65) runs cut by their ends."""
    return build(15 * 65, [np.arange((i // 40) * 65, (i // 40) * 65 + 65) for i in range(600)], 74)


def mm_hub():
    """Rows of four, and in their middle a hub row of 5,000 consecutive columns: over three blocks at every
    configuration (the step is at most 1,875 merge items), 8 to 40 segments per block, far below the table."""
    m = 2000
    rows = [np.arange(2 * i, 2 * i + 4) for i in range(m)]
    rows[m // 2] = np.arange(1000, 6000)
    return build(6000, rows, 73)


CASES = {
    "sell_packed": Case(
        "k_spmv_sell, four groups: all five packed forms, full and partial slices, every medium slot count, long runs "
        "of 1, 2 and 3 pieces, a 4,095-row block with a packed run in row 4,094, rows across group boundaries, an "
        "empty (row block, group)",
        sell_packed, frozenset(range(1, 65)) | frozenset(SELL_LONGS), frozenset(range(1, 65)) | frozenset(SELL_LONGS),
        SELL_W, 4, 43009),
    "sell_one_seg": Case(
        "k_spmv_sell, one group, one segment per block: every row is one run (unpacked short 1..8, medium 9..64, "
        "long up to 28 pieces), so a numpy model of the documented order gives y bit for bit",
        sell_one_seg, frozenset(range(1, 65)) | frozenset(SELL_LONGS + [1024, 1536, 2049, SELL_W]),
        frozenset(range(1, 65)) | frozenset(SELL_LONGS + [1024, 1536, 2049, SELL_W]), SELL_W, 1, SELL_W),
    "sell_edges": Case(
        "k_spmv_sell, one group, seven segments in block 0 with 1, 0 (long runs only), 17, 16, 3 slices in a row, "
        "an untouched slab, offsets 14,335 / 0 across a segment edge, a last segment of one column",
        sell_edges, frozenset([1, 2, 3, 4, 6, 8, 100, 600]), frozenset([1, 2, 8, 100, 600]), SELL_W, 1, 7 * SELL_W + 1),
    "sell_segs_255": Case("k_spmv_sell: 255 segments in a block, the table's limit (a wide x: n = 255 x 14,336)",
                          lambda: one_row_at_stride(255, SELL_W, 81), frozenset([1, 255]), frozenset([1]), SELL_W, 1,
                          255 * SELL_W),
    "sell_segs_256": Case("k_spmv_sell: 256 segments in a block, one past the table: the plan declines",
                          lambda: one_row_at_stride(256, SELL_W, 82), frozenset([1, 256]), frozenset([1]), SELL_W, 1,
                          256 * SELL_W),
    "sell_pieces_1024": Case("k_spmv_sell: 1,024 long-run pieces in one segment, the table's limit",
                             lambda: sell_pieces(1024), frozenset([65]), frozenset([65]), SELL_W, 8, 7 * SELL_W + 1),
    "sell_pieces_1025": Case("k_spmv_sell: 1,025 pieces in one segment: the plan declines",
                             lambda: sell_pieces(1025), frozenset([65]), frozenset([65]), SELL_W, 8, 7 * SELL_W + 1),
    "slab_chunks": Case(
        "k_spmv_slab: chunks of 2,048 and 2,049 nonzeros and of 1,024 and 1,025 runs, runs of 64 and 65, 20 long runs "
        "in a chunk, lg 0..4, columns 4,095 / 4,096, n = 4096 k + 1, a hub row over four merge-path blocks",
        slab_chunks, frozenset([1, 2, 8, 16, 32, 64, 65, 70, 3 * SLAB_STEP + SLAB_STEP // 5]),
        frozenset([1, 16, 32, 64, 65, 70]), SLAB_W, 1, 16 * SLAB_W + 1),
    "slab_empty_rows": Case("k_spmv_slab: 20,000 empty rows of 40,000 in three stretches, so the row cap adds blocks and "
                            "some of them hold no nonzero",
                            slab_empty_rows, frozenset([0, 3]), frozenset(), 0, 1, 2 * SLAB_W + 1),
    "slab_chunks_255": Case("k_spmv_slab: 255 chunks in a block, the table's limit",
                            lambda: one_row_at_stride(255, SLAB_W, 83), frozenset([1, 255]), frozenset([1]), SLAB_W, 1,
                            255 * SLAB_W),
    "slab_chunks_256": Case("k_spmv_slab: 256 chunks in a block: the plan declines",
                            lambda: one_row_at_stride(256, SLAB_W, 84), frozenset([1, 256]), frozenset([1]), SLAB_W, 1,
                            256 * SLAB_W),
    "mm_edges": Case(
        "k_spmm_slab: runs of 1..9, 15..17 and 63..65, three and more segments per block, segments of exactly "
        "cfg.cols columns and the next one a column later, full chunks and runs cut by them, a one-column segment at "
        "panel row n - 1",
        mm_edges, frozenset(MM_CYCLE), frozenset(), 0, 1, 12300),
    "mm_short_rows": Case("k_spmm_slab: one-element rows against the row cap; more runs in a segment than a chunk lists "
                          "(configurations 0 and 1; the row caps of 2 and 3 are below their entry limits)",
                          mm_short_rows, frozenset([1]), frozenset(), 0, 1, 3000),
    "mm_dense": Case("k_spmm_slab: a segment spanning several chunks, full chunks, runs cut by a chunk's end, at every "
                     "configuration", mm_dense, frozenset([65]), frozenset(), 0, 1, 975),
    "mm_hub": Case("k_spmm_slab: a hub row of 5,000 consecutive columns split across three and more blocks (carries, "
                   "heads), which must not decline",
                   mm_hub, frozenset([4, 5000]), frozenset(), 0, 1, 6000),
    "mm_chunks_127": Case("k_spmm_slab: 127 chunks (one-column-cluster segments) in a block, the table's limit",
                          lambda: one_row_at_stride(127, 1024, 85), frozenset([1, 127]), frozenset(), 0, 1, 127 * 1024),
    "mm_chunks_128": Case("k_spmm_slab: 128 chunks in a block: the plan declines",
                          lambda: one_row_at_stride(128, 1024, 86), frozenset([1, 128]), frozenset(), 0, 1, 128 * 1024),
}

for _k in (1, 2, 3, 4, 5, 9):   # the stream pipeline is four chunks deep: every remainder, and a third round
    CASES[f"mm_chunks_{_k}"] = Case(f"k_spmm_slab: a block of exactly {_k} chunks (and none of more)",
                                    functools.partial(one_row_at_stride, _k, 1024, 90 + _k), frozenset([1, _k]),
                                    frozenset(), 0, 1, _k * 1024)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """The case's matrix, built once and shared (left unchanged)."""
    return CASES[name].make()


def x_for(a, L=1, seed=1):
    return np.random.default_rng(seed).uniform(-1, 1, a.num_cols if L == 1 else (a.num_cols, L))


# ---- the documented summation order of k_spmv_sell, for a row that is one run ---------------------------------------
def sell_run_sum(p):
    """The sum k_spmv_sell forms of one run's products p (in CSR order) onto a row sum of +0.0.

    Short (<= 8): sequential.  Medium (<= 64): lane j of 8 sums products j, j + 8, ... in order, then
    ((s0+s1)+(s2+s3))+((s4+s5)+(s6+s7)).  Long: pieces of <= 512, in each lane l of 64 sums products l, l + 64, ...,
    the lanes fold by xor 32, 16, 8, 4, 2, 1 (own + other), and the pieces are added in order."""
    p = np.asarray(p, np.float64)
    k = p.size
    if k <= 8:
        s = np.float64(0.0)
        for v in p:
            s = s + v
        return s
    if k <= 64:
        q = np.zeros(64)
        q[:k] = p
        lanes = np.zeros(8)
        for j in range(8):                  # slot j of every lane, in order
            lanes = lanes + q[8 * j:8 * j + 8]
        return np.float64(0.0) + (((lanes[0] + lanes[1]) + (lanes[2] + lanes[3])) + ((lanes[4] + lanes[5]) + (lanes[6] + lanes[7])))
    s = np.float64(0.0)
    idx = np.arange(64)
    for b in range(0, k, 512):
        q = np.zeros(512)
        q[:min(512, k - b)] = p[b:b + 512]
        lanes = np.zeros(64)
        for j in range(8):
            lanes = lanes + q[64 * j:64 * j + 64]
        for o in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[idx ^ o]
        s = s + lanes[0]
    return s


def sell_model(a, x):
    """y of a matrix whose every row is one run of k_spmv_sell (one group, n <= 14,336)."""
    ro = a.row_offsets.astype(np.int64)
    prod = a.values * x[a.column_indices]
    return np.array([sell_run_sum(prod[ro[i]:ro[i + 1]]) for i in range(a.num_rows)])


# ---- the lanes-per-run rule of slab_block / slab_mm_block, restated to enumerate what it can choose ------------------
def lg_choice(runs, mean, threads, lanes_per_group=1, lg_max=6):
    best, lg = 1 << 30, 0
    for l in range(lg_max + 1):
        groups = threads // (lanes_per_group << l)
        cost = -(-runs // groups) * (-(-mean // (1 << l)) + 2 * l + 8)
        if cost < best:
            best, lg = cost, l
    return lg
