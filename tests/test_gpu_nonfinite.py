"""GPU: Inf and NaN in x / X under every tile, node-block and slab product kernel (nonfinite_cases.py).

The kernels pad and clamp -- pad slots of value 0 at column 0, gathers clamped to a tile's column base or to its
last nonzero, the column-pair load clamped to n - 2, a run's longer rows' panel entries fetched for its shorter rows
too -- and select the padding out, so that a row is non-finite exactly where the oracle's is (SpmvGold,
cpu_spmv.cpp:241-265; OmpCsrSpmmT, row_splitting.hpp:15-54): where it holds a nonzero in a column whose x is
non-finite.  With finite x a pad slot's 0.0 * x[0] is invisible; here x[0] = +Inf turns it into NaN.

Each case poisons the columns bad_columns derives from the plan the product runs on (one entry per column, in one
panel column), multiplies the poisoned and the cleaned input on one handle and holds both to check_nonfinite: the
oracle's NaNs and signed infinities exactly, every other entry bit-equal to the cleaned product, the cleaned
product within check_parity of the oracle.  Each case asserts the kernel or plan feature it is here for and prints
its kernel and its counts of non-finite rows, mixed rows (non-finite in some panel columns only) and prefix pairs
split (shorter row finite, longer not).  The switches set here (MSPMV_SPMV_RUNS, MSPMV_SPMM_SLAB) are read at each
handle's decision (mspmv_plan.hip), so monkeypatch sets them; none that is read once per process is needed.

Measured on an MI355X (all 59 cases pass; non-finite rows of m, mixed rows at L >= 2, prefix pairs split):
  SpMV  k_spmv_tile<8,0,false,64,true,true>   walk_onewave 264 of 60,000
        k_spmv_tile<8,0,false,256,true,true>  split_rows 6 of 3,000
        k_spmv_tile<8,0,false,256,true,false> rowgroup_thread 64 of 40,000; rowgroup_wide 591 of 12,000; dictionary 711 of
                                              6,000; all_empty 0; single_entry, one_row_matrix 1 of 1; leading_empty 165,
                                              trailing_empty 150 of 9,000 (1 of 1 pair each); two_chunk_lds 552 of 4,000
        k_spmv_blk<0,false,6,false>           pair_compact 708, _runs0 700, pair_escaped 679 of 4,198 (3 of 4 pairs each);
                                              pair_two_rounds 414, pair_odd_runs 425, mixed_plan 746 (3 of 4) of 4,200;
                                              pair_r13 326, pair_w63 350, pair_short_first 383 (4 of 4),
                                              pair_short_first_escaped 408 (4 of 4) of 4,196; empty_in_runs 560 of 12,000
                                              (4 of 4); pair_dof7 518 of 14,000
        k_spmv_blk<0,false,6,true>            fallback 671 of 5,398 (3 of 4)
  SpMM  k_spmm_tile<L,..,false,true>          powerlaw L = 2, 4, 8, 16, 3: 341-361 of 20,000, all but 0-4 mixed; hub_rect
                                              L = 8, 16 (the slab plan declines it): 43 of 20,000, 42-43 mixed, 4 of 4
        k_spmm_tile<L,..,false,false>         fem2d L = 2..16: 65 of 10,007, 62-65 mixed
        k_spmm_tile<16,32,0,false,true,true>  dict16: 288 of 6,000, all mixed (182 dictionary tiles)
        k_spmm_blk<L,0,false,6>               kron9_6 444-462 of 18,000; kron12 504-540 of 10,800; fem_52_53 (and L = 3 on
                                              k_spmm_blk<4,..>) 725-758 of 4,198, 2-3 of 4 pairs; short_first_r12_odd 383-464
                                              of 4,196, 4 of 4; kron9_7 539 of 14,000; all mixed but 1-69 rows at L = 2
        k_spmm_slab<0 | 2,false>              band L = 8 | 16: 481 | 459 of 30,000; short_rows 437 | 397 of 200,000 (4 of 4)
With the column-pair SpMV's and the node-block SpMM's selects replaced by a multiplication by 0.0 (a lab build, not
kept) all 29 k_spmv_blk and k_spmm_blk cases of the 54 then here failed and none of the other 25.
"""
import functools

import numpy as np
import pytest

import mspmv
import nonfinite_cases as nf
from gpu_common import chunk_widths
from test_gpu_blk_records import boundary_matrix, escape_matrix, fallback_matrix
from test_gpu_blocks import kron9_emptied, kron_fem, kron_fem9
from test_gpu_slab import scatter_band, with_rows
from test_gpu_slab_mm import CASES as SLAB_MM_CASES
from test_gpu_slab_mm import MAY_DECLINE
from test_gpu_spmv import LONG_ROWS, edge_case, synth_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    return gpu_available


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for name in ("MSPMV_SPMV_RUNS", "MSPMV_SPMV_SLAB", "MSPMV_SLAB_GROUPS", "MSPMV_SPMM_SLAB"):
        monkeypatch.delenv(name, raising=False)


def fem(m, nnz, block):
    return mspmv.CsrMatrix.synth_fem_blocked(m, nnz, block, 60, seed=5)


MATRICES = {
    "powerlaw_onewave": lambda: mspmv.CsrMatrix.synth_powerlaw(60000, 60000, 1800000, exponent=1.2, seed=7),
    "stencil_rows": lambda: mspmv.CsrMatrix.synth_stencil(0, 40000, 200, 0, 0, seed=3),
    "rows50": lambda: with_rows(12000, 12000, [50] * 12000, 3),
    "cant_small": synth_cases()["cant_small"],
    "powerlaw": synth_cases()["powerlaw"],
    "fem2d": synth_cases()["fem2d"],
    "long_rows_many_tiles": lambda: edge_case("long_rows_many_tiles"),
    "all_empty": lambda: edge_case("all_empty"),
    "single_entry": lambda: edge_case("single_entry"),
    "one_row_matrix": lambda: edge_case("one_row_matrix"),
    "leading_empty": lambda: edge_case("leading_empty"),
    "trailing_empty": lambda: edge_case("trailing_empty"),
    "fem_52_53": lambda: fem(4198, 222000, 6),
    "fem_36": lambda: fem(4200, 151200, 6),
    "fem_dof5": lambda: fem(4200, 210000, 5),
    "escape": escape_matrix,
    "r13": lambda: boundary_matrix("r13")[0],
    "short_first_r12_odd": lambda: boundary_matrix("short_first_r12_odd")[0],
    "short_first_r13": lambda: boundary_matrix("short_first_r13")[0],
    "w63": lambda: boundary_matrix("w63")[0],
    "fallback": fallback_matrix,
    "perturbed": lambda: mspmv.CsrMatrix.synth_fem_perturbed(4200, 222000, 6, 60, 0.05, 0.02, seed=5),
    "kron9_8": lambda: kron_fem9(25, 20, 8),
    "kron9_emptied": lambda: kron9_emptied()[0],
    "dict16": lambda: mspmv.CsrMatrix.synth_fem_blocked(6000, 180000, 6, 3, seed=4),
    "kron9_6": lambda: kron_fem9(60, 50, 6),
    "kron12": lambda: kron_fem(30, 30, 12),
    "kron9_7": lambda: kron_fem9(50, 40, 7),
    "band": lambda: scatter_band(30000, 40, 2000, 3),
    "hub_rect": SLAB_MM_CASES["hub_rect"],
    "short_rows": SLAB_MM_CASES["short_rows"],
}


@functools.lru_cache(maxsize=4)
def matrix(name):
    """The named matrix, shared by the cases that follow each other on it and left unchanged."""
    return MATRICES[name]()


def run_case(orc, label, a, L, num_random=nf.NUM_RANDOM):
    """One handle: the plan, the poisoned and the cleaned product, check_nonfinite.  Returns what the case's own
    assertions need."""
    w = chunk_widths(L)[0][1]  # the plan the (first chunk of the) product runs on
    with mspmv.GpuCsr(a) as g:
        plan = g.tile_plan(w)
        cols, pairs = nf.bad_columns(a, plan, seed=L, num_random=num_random)
        X = nf.poison(np.random.default_rng(100 + L).uniform(-1, 1, (a.num_cols, L)), cols)
        Xc = nf.cleaned(X)
        if L == 1:
            Y, Yc = g.spmv(X[:, 0].copy()), g.spmv(Xc[:, 0].copy())
            kname = g.kernel_name()
        else:
            Y, Yc = g.spmm(X), g.spmm(Xc)
            kname = g.spmm_kernel_name(L)
        info = {"kname": kname, "plan": plan, "nb": g.plan_block_tiles(w), "rounds": g.plan_block_rounds(w),
                "records": g.plan_block_records(w), "streams": g.tile_streams(), "dict_tiles": g.dict_tiles(w),
                "pairs": pairs, "cols": cols, "Y": Y}
        chunks = plan if w == L else [(c0, min(c0 + cw, L), g.tile_plan(cw), cw) for c0, cw in chunk_widths(L)]
    if L == 1:
        gold, gold_c = orc.spmv_gold(a, X[:, 0].copy()), orc.spmv_gold(a, Xc[:, 0].copy())
    else:
        gold, gold_c = orc.csr_spmm_t(a, X), orc.csr_spmm_t(a, Xc)
    info["gold"] = gold
    print(f"{label} L={L}: {kname}, modes {np.unique(plan['modes']).tolist()}, lanes {plan['lanes']}, "
          f"carries {plan['num_carries']}, node-block tiles {info['nb']} of {plan['num_tiles']} "
          f"({info['rounds']} of two rounds), records (compact, escaped) {info['records']}, "
          f"streams (16-bit, dictionary) {info['streams']}, dictionary tiles {info['dict_tiles']}; "
          f"{len(cols)} bad columns", end="")
    bad, mixed, split = nf.check_nonfinite(a, Y, gold, Yc, gold_c, Xc, chunks, L, pairs)
    print(f": {bad} of {a.num_rows} rows non-finite, {mixed} mixed, {split} of {len(pairs)} prefix pairs split")
    return info


# ---- SpMV --------------------------------------------------------------------------------------------------------
def is_pair(i):
    return i["kname"].startswith("k_spmv_blk<0,") and i["kname"].endswith(",6,false>")


def is_tile(i):
    return i["kname"].startswith("k_spmv_tile<")


# name: (matrix, MSPMV_SPMV_RUNS, what the case is here for)
SPMV_CASES = {
    # merge-walk tiles with cross-tile carries on the one-wave plan
    "walk_onewave": ("powerlaw_onewave", None, lambda i: is_tile(i) and ",64," in i["kname"] and i["plan"]["lanes"] == 64
                     and (i["plan"]["modes"] == 0).any() and i["plan"]["num_carries"] > 0),
    # row-group tiles: one row per thread, and groups of >= 4 lanes on rows that share no column list
    "rowgroup_thread": ("stencil_rows", None, lambda i: is_tile(i) and set(i["plan"]["modes"].tolist()) == {1}),
    "rowgroup_wide": ("rows50", None, lambda i: is_tile(i) and i["plan"]["modes"].min() >= 3 and i["nb"] == 0),
    # 16-bit column stream, grouped staging, column dictionaries
    "dictionary": ("cant_small", None, lambda i: is_tile(i) and i["streams"][0] > 0 and i["streams"][1] > 0),
    # rows split between tiles (see test_spmv_split_rows_neighbours too)
    "split_rows": ("long_rows_many_tiles", None, lambda i: is_tile(i) and i["plan"]["num_carries"] > 0),
    "all_empty": ("all_empty", None, is_tile),
    "single_entry": ("single_entry", None, is_tile),
    "one_row_matrix": ("one_row_matrix", None, is_tile),
    "leading_empty": ("leading_empty", None, is_tile),
    "trailing_empty": ("trailing_empty", None, is_tile),
    # the column-pair kernel on compact records, run-balanced and merge-path plans
    "pair_compact": ("fem_52_53", None, lambda i: is_pair(i) and i["nb"] == i["plan"]["num_tiles"]
                     and i["records"][0] > 0 and i["records"][1] == 0),
    "pair_compact_runs0": ("fem_52_53", "0", lambda i: is_pair(i) and i["nb"] == i["plan"]["num_tiles"]
                           and i["records"][0] > 0 and i["records"][1] == 0),
    "pair_two_rounds": ("fem_36", "0", lambda i: is_pair(i) and i["rounds"] > 0 and i["records"][1] == 0),
    "pair_odd_runs": ("fem_dof5", None, lambda i: is_pair(i) and i["records"][0] > 0 and i["records"][1] == 0),
    # escaped records, beside compact ones and alone
    "pair_escaped": ("escape", None, lambda i: is_pair(i) and i["records"][0] > i["records"][1] > 0),
    "pair_r13": ("r13", None, lambda i: i["kname"].startswith("k_spmv_blk<0,") and i["records"][0] == 0
                 and i["records"][1] > 0),
    # a pattern row that is not the run's first: the prefix-only columns
    "pair_short_first": ("short_first_r12_odd", None, lambda i: i["kname"].startswith("k_spmv_blk<0,")
                         and i["records"][0] > 0 and i["records"][1] == 0 and len(i["pairs"]) == 4),
    "pair_short_first_escaped": ("short_first_r13", None, lambda i: i["kname"].startswith("k_spmv_blk<0,")
                                 and i["records"][1] > 0 and len(i["pairs"]) == 4),
    # the last pair has one column left, at column n - 1
    "pair_w63": ("w63", None, lambda i: i["kname"].startswith("k_spmv_blk<0,") and i["records"][0] > 0
                 and i["records"][1] == 0),
    # the register fallback beside records
    "fallback": ("fallback", None, lambda i: i["kname"].startswith("k_spmv_blk<0,") and i["kname"].endswith(",6,true>")
                 and 0 < i["nb"] < i["plan"]["num_tiles"] and i["records"][0] > 0),
    "mixed_plan": ("perturbed", None, lambda i: i["kname"].startswith("k_spmv_blk<0,") and i["records"][0] > 0),
    # two-chunk runs on k_spmv_tile's LDS path; empty rows inside runs
    "two_chunk_lds": ("kron9_8", None, lambda i: is_tile(i) and i["nb"] > 0),
    "empty_in_runs": ("kron9_emptied", None, lambda i: i["nb"] > 0),
    # nodes of 7 unknowns: runs of 6 + 1 rows, 63 columns wide
    "pair_dof7": ("kron9_7", None, lambda i: i["kname"].startswith("k_spmv_blk<0,") and i["records"][0] > 0),
}


@pytest.mark.parametrize("name", list(SPMV_CASES))
def test_spmv_nonfinite(orc, monkeypatch, name):
    mat, runs, covers = SPMV_CASES[name]
    if runs is not None:
        monkeypatch.setenv("MSPMV_SPMV_RUNS", runs)
    a = matrix(mat)
    info = run_case(orc, name, a, 1)
    assert covers(info), (info["kname"], {k: info[k] for k in ("nb", "rounds", "records", "streams")},
                          np.unique(info["plan"]["modes"]), info["plan"]["lanes"], info["plan"]["num_carries"])
    if mat in ("w63", "r13", "short_first_r12_odd", "short_first_r13"):
        assert a.column_indices[-1] == a.num_cols - 1 and not np.isfinite(info["gold"][-1])
    if name == "split_rows":
        # the hub rows are non-finite; the one-entry rows beside them stay finite unless their one column is a bad
        # one (the last nonzero of a tile that ends where a hub row starts is such a row's), and each hub row has
        # a finite neighbour
        hubs = np.array(LONG_ROWS)
        beside = np.setdiff1d(np.concatenate([hubs - 1, hubs + 1]), [a.num_rows])
        hit = nf.predicted_nonfinite(a, info["cols"], 1)[:, 0]
        assert hit[hubs].all() and not np.isfinite(info["gold"][hubs]).any()
        assert all(not hit[[r for r in (h - 1, h + 1) if r < a.num_rows]].all() for h in hubs)
        assert np.array_equal(np.isfinite(info["Y"][beside]), ~hit[beside])
    if name == "empty_in_runs":
        keep = kron9_emptied()[1]
        assert np.all(info["Y"][~keep] == 0.0) and not np.signbit(info["Y"][~keep]).any()


# ---- SpMM --------------------------------------------------------------------------------------------------------
def spmm_tile(L, dictionary=False):
    def covers(i):
        return i["kname"].startswith(f"k_spmm_tile<{L},") and (not dictionary or (
            i["kname"].endswith(",true,true>") and i["dict_tiles"] > 0))
    return covers


def spmm_blk(L):
    return lambda i: i["kname"].startswith(f"k_spmm_blk<{L},") and i["nb"] == i["plan"]["num_tiles"]


WIDTHS = (2, 4, 8, 16)
# (matrix, L, MSPMV_SPMM_SLAB, what the case is here for)
SPMM_CASES = (
    # k_spmm_tile: the merge walk (power-law rows) and row groups (7 per row)
    [("powerlaw", L, None, lambda i, L=L: spmm_tile(L)(i) and (i["plan"]["modes"] == 0).any()) for L in WIDTHS]
    + [("fem2d", L, None, lambda i, L=L: spmm_tile(L)(i) and (i["plan"]["modes"] > 0).any()) for L in WIDTHS]
    + [("dict16", 16, None, spmm_tile(16, dictionary=True))]
    # k_spmm_blk: equal rows, one wide chunk, 52 / 53-long prefix rows (fused passes against select passes), and
    # a pattern row that is not its run's first
    + [(mat, L, None, spmm_blk(L)) for mat in ("kron9_6", "kron12", "fem_52_53", "short_first_r12_odd") for L in WIDTHS]
    # nodes of 7 unknowns: runs of 6 + 1 rows (a run holds at most kBlkRunRows = 6 rows, so the plans here never
    # reach the kernel's form for taller runs, k_spmm_blk<.., 8>)
    + [("kron9_7", L, None, lambda i, L=L: spmm_blk(L)(i) and i["kname"].endswith(",6>")) for L in (2, 16)]
    # k_spmm_slab where the plan takes the shape (the band; one-entry and empty rows), the tiles where it declines
    + [(mat, L, "1", lambda i, L=L, mat=mat: i["kname"].startswith("k_spmm_slab<") and np.all(i["plan"]["modes"] == 255)
        or (mat in MAY_DECLINE and spmm_tile(L)(i))) for mat in ("band", "hub_rect", "short_rows") for L in (8, 16)]
    # an odd width: one chunk of four columns on a zero-padded panel
    + [("powerlaw", 3, None, spmm_tile(4)), ("fem_52_53", 3, None, spmm_blk(4))]
)


@pytest.mark.parametrize("mat,L,slab,covers", SPMM_CASES, ids=[f"{c[0]}-{c[1]}" for c in SPMM_CASES])
def test_spmm_nonfinite(orc, monkeypatch, mat, L, slab, covers):
    """short_first_r12_odd takes the node-block SpMM like the other FEM shapes (asserted: k_spmm_blk<L,..>)."""
    if slab is not None:
        monkeypatch.setenv("MSPMV_SPMM_SLAB", slab)
    a = matrix(mat)
    info = run_case(orc, mat, a, L)
    assert covers(info), (info["kname"], {k: info[k] for k in ("nb", "rounds", "records", "dict_tiles")},
                          np.unique(info["plan"]["modes"]), info["plan"]["num_carries"])
    if mat in ("fem_52_53", "short_first_r12_odd"):
        assert info["pairs"], "no prefix pairs: the select passes after the fused ones go unchecked"
