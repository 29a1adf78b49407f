"""k_spmv_sell, k_spmv_slab and k_spmm_slab (mspmv_slab.hip) at their layout edges: the cases of slab_cases.py, each
under set_cu_limit(8) so that a small matrix fills a block.

Every case: the forced kernel's name (a decline the case was not built for fails), GpuCsr.slab_plan_stats showing the
form the case was cut for, check_parity against the oracle (orc.spmv_gold / orc.csr_spmm_t), repeats bit-identical,
carries where the case claims split rows.  Each table limit (255 chunks, 255 segments, 1,024 pieces, 127 SpMM chunks)
has a case exactly at it -- accepted, the statistic equal to the limit -- and one past it, which must come out right
on a tile kernel.  Two exact checks hold k_spmv_sell to the order its header documents (no FMA contraction, so no
tolerance): rows of <= 8 nonzeros inside one column group equal SpmvGold bit for bit, and where every row is one run
(one group, n <= 14,336) the numpy model slab_cases.sell_model reproduces y bit for bit.  Non-finite x / X at a
segment's first and last column and at column 0 follow the rule of nonfinite_cases.check_nonfinite.
"""
import numpy as np
import pytest

import mspmv
import nonfinite_cases as nf
import slab_cases as sc
from gpu_common import check_parity, check_parity_chunked, chunk_widths

pytestmark = pytest.mark.gpu

CUS = 8
_GOLD = {}


def gold_of(orc, name, L=1):
    """(matrix, X, oracle product), computed once per (case, width) and shared."""
    if (name, L) not in _GOLD:
        a = sc.matrix(name)
        X = sc.x_for(a, L)
        _GOLD[name, L] = (a, X, orc.spmv_gold(a, X) if L == 1 else orc.csr_spmm_t(a, X))
    return _GOLD[name, L]


def bits(v):
    return np.ascontiguousarray(v, np.float64).view(np.uint64)


def spmv_env(monkeypatch, mode, groups=None):
    monkeypatch.setenv("MSPMV_SPMV_SLAB", mode)
    if groups is None:
        monkeypatch.delenv("MSPMV_SLAB_GROUPS", raising=False)
    else:
        monkeypatch.setenv("MSPMV_SLAB_GROUPS", str(groups))


def is_kernel(name, stem, tail):
    """stem<true|false,tail>: the SpMV kernels' nontemporal flag comes first; k_spmm_slab<tail,true|false>."""
    if stem == "k_spmm_slab":
        return name in (f"{stem}<{tail},true>", f"{stem}<{tail},false>")
    return name in (f"{stem}<true,{tail}>", f"{stem}<false,{tail}>")


def run_spmv(orc, name, stem, tail):
    """The case's product on eight CUs: (y, statistics, plan) after the checks every case gets.  stem None: the plan
    must have declined -- a tile kernel, no statistics -- and the product must still be right."""
    a, x, gold = gold_of(orc, name)
    with mspmv.GpuCsr(a) as g:
        g.set_cu_limit(CUS)
        y = g.spmv(x)
        k, st, plan = g.kernel_name(), g.slab_plan_stats(1), g.tile_plan(1)
        print(f"{name}: {k} {({n: v for n, v in st.items() if v} if st else None)}")
        if stem is None:
            assert st is None and not k.startswith(("k_spmv_slab<", "k_spmv_sell<")), k
        else:
            assert is_kernel(k, stem, tail), k
            assert st is not None and np.all(plan["modes"] == 255)
            assert st["blocks"] == plan["num_tiles"] and st["carries"] == plan["num_carries"]
        check_parity(a, y, gold, x, plan, 1)
        assert y.tobytes() == g.spmv(x).tobytes()
    return y, st, plan


def positive(st, names):
    missing = [n for n in names if st[n] <= 0]
    assert not missing, f"forms the case was built for and the plan does not hold: {missing}"


# ---- k_spmv_sell ------------------------------------------------------------------------------------------------------
MEDIUM = [f"medium_{i}" for i in range(2, 9)]
LONGS = ["long_1", "long_2", "long_3plus"]


def test_sell_packed_forms_and_short_rows(orc, monkeypatch):
    spmv_env(monkeypatch, "4")
    y, st, _ = run_spmv(orc, "sell_packed", "k_spmv_sell", "true")
    positive(st, ["pack_8x1", "pack_4x2", "pack_2x3", "pack_2x4"] + [f"pack_1x{i}" for i in range(5, 9)] + MEDIUM + LONGS
             + ["slices_odd", "slices_partial"])
    assert st["groups"] == 4 and st["blocks"] == 12 and st["rows_max"] == 4095 and st["units_max"] == 1
    assert st["packed_row_max"] == 4094 and st["pack_8x1"] >= 2 and st["pieces_max"] == 7
    assert st["empty_blocks"] >= 4 and st["carries"] == 0 and st["unpacked_1"] == 0
    # rows of <= 8 nonzeros inside one group: the CSR-order sum from +0.0, plus the other groups' +0.0
    a, x, gold = gold_of(orc, "sell_packed")
    lens = np.diff(a.row_offsets)
    lo = np.asarray(sc.group_lo(a.num_cols, 4)[1:4])
    first, last = a.column_indices[a.row_offsets[:-1]], a.column_indices[a.row_offsets[1:] - 1]
    exact = (lens <= 8) & (np.searchsorted(lo, first, side="right") == np.searchsorted(lo, last, side="right"))
    assert exact.sum() >= 1000
    bad = np.flatnonzero(exact & (bits(y) != bits(gold)))
    assert bad.size == 0, f"{bad.size} of {exact.sum()} short rows differ from SpmvGold, e.g. rows {bad[:5]} of length {lens[bad[:5]]}"


def test_sell_one_segment_matches_the_documented_order(orc, monkeypatch):
    spmv_env(monkeypatch, "4")
    y, st, _ = run_spmv(orc, "sell_one_seg", "k_spmv_sell", "false")
    positive(st, [f"unpacked_{i}" for i in range(1, 9)] + MEDIUM + LONGS + ["slices_odd", "slices_partial"])
    assert st["groups"] == 1 and st["units_max"] == 1 and st["pieces_max"] >= 28 and st["pack_8x1"] == 0
    a, x, gold = gold_of(orc, "sell_one_seg")
    lens = np.diff(a.row_offsets)
    short = lens <= 8
    assert np.array_equal(bits(y[short]), bits(gold[short]))
    model = sc.sell_model(a, x)
    bad = np.flatnonzero(bits(y) != bits(model))
    assert bad.size == 0, f"{bad.size} rows differ from the documented order, e.g. rows {bad[:5]} of length {lens[bad[:5]]}"


def test_sell_one_group_segment_edges(orc, monkeypatch):
    spmv_env(monkeypatch, "4", 1)
    y, st, _ = run_spmv(orc, "sell_edges", "k_spmv_sell", "false")
    positive(st, ["unpacked_1", "unpacked_2", "unpacked_8", "long_1", "long_2", "segs_pieces_only", "segs_refill"])
    assert st["groups"] == 1 and st["blocks"] == 8 and st["units_max"] == 7 and st["empty_blocks"] == 0
    a, x, gold = gold_of(orc, "sell_edges")
    short = np.diff(a.row_offsets) <= 8   # a row's runs follow slab order, so column order: the CSR-order sum
    assert short.sum() >= 6000 and np.array_equal(bits(y[short]), bits(gold[short]))


@pytest.mark.parametrize("name,groups,stat,limit", [("sell_segs_255", 1, "units_max", 255), ("sell_segs_256", 1, None, 0),
                                                    ("sell_pieces_1024", 8, "pieces_max", 1024),
                                                    ("sell_pieces_1025", 8, None, 0)])
def test_sell_table_limits(orc, monkeypatch, name, groups, stat, limit):
    """sseg holds 255 segments and the next one's piece start (256 entries), lpart 1,024 piece sums."""
    spmv_env(monkeypatch, "4", groups)
    if stat is None:
        run_spmv(orc, name, None, None)
        return
    _, st, _ = run_spmv(orc, name, "k_spmv_sell", "true" if groups > 1 else "false")
    assert st[stat] == limit and st["groups"] == groups
    if groups == 8:
        assert st["blocks"] == 8 and st["empty_blocks"] == 7 and st["long_1"] == 1024 and st["segs_pieces_only"] == 1


def test_sell_packed_nonfinite(orc, monkeypatch):
    """Inf and NaN at column 0, at the first and last column of block 0's segment, on both sides of a group boundary
    that is a segment's first column in row block 1, and at n - 1."""
    spmv_env(monkeypatch, "4")
    a, x, _ = gold_of(orc, "sell_packed")
    b0 = a.column_indices[:a.row_offsets[4095]]
    lo = sc.group_lo(a.num_cols, 4)
    cols = list(dict.fromkeys([0, int(b0.min()), int(b0.max()), lo[1] - 1, lo[1], lo[2], a.num_cols - 1]))
    xp = nf.poison(x, cols)
    xc = nf.cleaned(xp)
    with mspmv.GpuCsr(a) as g:
        g.set_cu_limit(CUS)
        y, yc = g.spmv(xp), g.spmv(xc)
        assert is_kernel(g.kernel_name(), "k_spmv_sell", "true")
        nf.check_nonfinite(a, y, orc.spmv_gold(a, xp), yc, orc.spmv_gold(a, xc), xc, g.tile_plan(1), 1)


# ---- k_spmv_slab ------------------------------------------------------------------------------------------------------
SLAB_MODES = {"1": ("k_spmv_slab", "0"), "2": ("k_spmv_slab", "1")}


@pytest.mark.parametrize("mode", ["1", "2"])
def test_slab_chunk_edges(orc, monkeypatch, mode):
    spmv_env(monkeypatch, mode)
    _, st, _ = run_spmv(orc, "slab_chunks", *SLAB_MODES[mode])
    positive(st, ["chunks_full", "runs_cut", "chunks_long", "lg0"])
    assert st["lg5"] == st["lg6"] == 0
    if mode == "1":   # the features are cut to this shape's 4,096 / 2,048 / 1,024
        positive(st, ["chunks_entry_cut", "lg1", "lg2", "lg3", "lg4"])
        assert st["blocks"] == 16 and st["groups"] == 1 and st["carries"] >= 3 and st["long_runs_max"] == 20
        assert st["rows_max"] <= 2047 and st["units_max"] <= 255
    else:             # four groups of three 8,192-column slabs over nine: the last group is empty
        assert st["groups"] == 4 and st["carries"] == 0 and st["rows_max"] == 4095 and st["long_runs_max"] > 16
        assert st["empty_blocks"] >= st["blocks"] // 4


@pytest.mark.parametrize("mode", ["1", "2"])
def test_slab_empty_row_stretches(orc, monkeypatch, mode):
    spmv_env(monkeypatch, mode)
    _, st, _ = run_spmv(orc, "slab_empty_rows", *SLAB_MODES[mode])
    cap = 2047 if mode == "1" else 4095
    assert st["empty_blocks"] >= 1 and cap // 2 < st["rows_max"] <= cap
    assert st["blocks"] > (16 if mode == "1" else 8) and st["blocks"] >= -(-40000 // cap)


@pytest.mark.parametrize("want,groups", [(2, 2), (8, 8), (9, 8)])
def test_slab_group_counts(orc, monkeypatch, want, groups):
    spmv_env(monkeypatch, "2", want)
    _, st, _ = run_spmv(orc, "slab_chunks", "k_spmv_slab", "1")
    assert st["groups"] == groups and st["blocks"] % groups == 0
    if groups == 8:   # nine slabs of 8,192 in groups of two: groups 5, 6 and 7 hold no column
        assert st["empty_blocks"] >= 3 * st["blocks"] // 8


@pytest.mark.parametrize("name,limit", [("slab_chunks_255", 255), ("slab_chunks_256", 0)])
def test_slab_table_limit(orc, monkeypatch, name, limit):
    """schunk holds 255 chunks and the next one's entry start (256 entries)."""
    spmv_env(monkeypatch, "1")
    if not limit:
        run_spmv(orc, name, None, None)
        return
    _, st, _ = run_spmv(orc, name, "k_spmv_slab", "0")
    assert st["units_max"] == limit and st["blocks"] == 16


# ---- k_spmm_slab ------------------------------------------------------------------------------------------------------
MM_RUNS = [(8, None, 0), (16, None, 2), (8, "1", 1), (16, "3", 3)]   # (L, MSPMV_SPMM_SLAB_CFG, configuration)
MM_IDS = ["L8_cfg0", "L16_cfg2", "L8_cfg1", "L16_cfg3"]


def mm_env(monkeypatch, lab):
    monkeypatch.setenv("MSPMV_SPMM_SLAB", "1")
    if lab is None:
        monkeypatch.delenv("MSPMV_SPMM_SLAB_CFG", raising=False)
    else:
        monkeypatch.setenv("MSPMV_SPMM_SLAB_CFG", lab)


def run_spmm(orc, name, L, cfg):
    """As run_spmv; cfg None: the plan must have declined."""
    a, X, gold = gold_of(orc, name, L)
    with mspmv.GpuCsr(a) as g:
        g.set_cu_limit(CUS)
        Y = g.spmm(X)
        k, st, plan = g.spmm_kernel_name(L), g.slab_plan_stats(L), g.tile_plan(L)
        print(f"{name} L={L}: {k} {({n: v for n, v in st.items() if v} if st else None)}")
        if cfg is None:
            assert st is None and not k.startswith("k_spmm_slab<"), k
        else:
            assert is_kernel(k, "k_spmm_slab", str(cfg)), k
            assert st is not None and np.all(plan["modes"] == 255)
            assert st["blocks"] == plan["num_tiles"] and st["carries"] == plan["num_carries"]
            assert st["units_max"] <= 127 and st["rows_max"] <= sc.MM_ROWS[cfg] and st["lg5"] == st["lg6"] == 0
        check_parity(a, Y, gold, X, plan, L)
        assert Y.tobytes() == g.spmm(X).tobytes()
    return Y, st, plan


@pytest.mark.parametrize("L,lab,cfg", MM_RUNS, ids=MM_IDS)
@pytest.mark.parametrize("name", ["mm_edges", "mm_short_rows", "mm_dense", "mm_hub"])
def test_slab_mm_edges(orc, monkeypatch, name, L, lab, cfg):
    mm_env(monkeypatch, lab)
    _, st, _ = run_spmm(orc, name, L, cfg)
    if name == "mm_edges":
        positive(st, ["segments", "segments_full", "segments_ragged"])
        assert st["segments_max"] >= 3 and st["units"] >= st["segments"]
    elif name == "mm_short_rows":
        positive(st, ["lg0"])
        assert st["rows_max"] > 0.9 * sc.MM_ROWS[cfg]
        # a segment holds at most rows + 1 runs: configurations 2 and 3 cannot reach their entry limit
        assert (st["chunks_entry_cut"] > 0) == (cfg in (0, 1))
    elif name == "mm_dense":
        positive(st, ["chunks_full", "runs_cut"])
        assert st["units"] > st["segments"] and st["lg2"] + st["lg3"] + st["lg4"] > 0
    else:
        assert st["carries"] >= 2


@pytest.mark.parametrize("L,lab,cfg", MM_RUNS, ids=MM_IDS)
@pytest.mark.parametrize("name,limit", [("mm_chunks_127", 127), ("mm_chunks_128", 0)])
def test_slab_mm_table_limit(orc, monkeypatch, name, limit, L, lab, cfg):
    """schunk holds 127 chunks and the next one's entry start (128 entries)."""
    mm_env(monkeypatch, lab)
    _, st, _ = run_spmm(orc, name, L, cfg if limit else None)
    if limit:
        assert st["units_max"] == limit and st["segments_max"] == limit


@pytest.mark.parametrize("L,lab,cfg", MM_RUNS, ids=MM_IDS)
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 9])
def test_slab_mm_block_chunk_counts(orc, monkeypatch, k, L, lab, cfg):
    """A block of exactly k chunks, and none of more: each remainder of the four-deep stream pipeline, and k = 9."""
    mm_env(monkeypatch, lab)
    _, st, _ = run_spmm(orc, f"mm_chunks_{k}", L, cfg)
    assert st["units_max"] == k == st["segments_max"]


@pytest.mark.parametrize("L", [24, 12])
def test_slab_mm_hub_column_chunks(orc, monkeypatch, L):
    """Widths outside {8, 16} on the split hub row: chunks of 16 / 8 (and 4) columns, panel stride L."""
    mm_env(monkeypatch, None)
    a, X, gold = gold_of(orc, "mm_hub", L)
    with mspmv.GpuCsr(a) as g:
        g.set_cu_limit(CUS)
        Y = g.spmm(X)
        check_parity_chunked(a, g, Y, gold, X, L)
        for _, w in chunk_widths(L):
            if w >= 8:
                assert g.spmm_kernel_name(w).startswith("k_spmm_slab<"), (w, g.spmm_kernel_name(w))
                assert g.slab_plan_stats(w)["carries"] >= 2
        assert Y.tobytes() == g.spmm(X).tobytes()


@pytest.mark.parametrize("L,lab,cfg", MM_RUNS, ids=MM_IDS)
def test_slab_mm_nonfinite(orc, monkeypatch, L, lab, cfg):
    """Inf and NaN at column 0, at the last column of the first block's first segment and the first of its second
    (columns 3 i .. are contiguous from 0, so the first segment is [0, cfg.cols)), and at the one-column segment n - 1."""
    mm_env(monkeypatch, lab)
    a, X, _ = gold_of(orc, "mm_edges", L)
    w = sc.MM_COLS[cfg]
    cols = [0, w - 1, w, a.num_cols - 1]
    Xp = nf.poison(X, cols)
    Xc = nf.cleaned(Xp)
    with mspmv.GpuCsr(a) as g:
        g.set_cu_limit(CUS)
        Y, Yc = g.spmm(Xp), g.spmm(Xc)
        assert is_kernel(g.spmm_kernel_name(L), "k_spmm_slab", str(cfg))
        nf.check_nonfinite(a, Y, orc.csr_spmm_t(a, Xp), Yc, orc.csr_spmm_t(a, Xc), Xc, g.tile_plan(L), L)
