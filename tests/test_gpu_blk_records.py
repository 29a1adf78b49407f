"""GPU: the column-pair node-block SpMV on 64-B records (TilePlan::d_recs).

k_spmv_blk<0, NT, 6, FB> reads a run's descriptor and its pattern columns, run-length coded as at
most 12 runs of consecutive columns, from one 64-B record per run slot; a pattern of more such runs
escapes to its row of the 16-bit column stream.  Products, sums and their order are what they were, so
on plans of register run tiles alone (kernel name ending ",6,false>") y is the pair tree of each row,
restated in numpy here and required bit for bit: prod[k] = val[k] * x[col[k]] padded with +0.0 to 64,
pair[l] = prod[2l] + prod[2l+1], then halves of 16, 8, 4, 2, 1.  Mixed plans are checked against the
oracle under check_parity.

test_record_boundary runs the boundary itself on the device -- rows of exactly 11, 12 and 13 column-runs, patterns 63
and 64 columns wide, a pattern row that is not its run's first -- on generated FEM nodes (fem_nodes)."""
import numpy as np
import pytest

import mspmv
from gpu_common import check_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    return gpu_available


def pair_tree_spmv(a, x):
    """y of the column-pair kernel for a matrix whose rows hold <= 64 entries, bit for bit."""
    ro = a.row_offsets.astype(np.int64)
    lens = np.diff(ro)
    assert lens.max() <= 64
    prod = np.zeros((a.num_rows, 64))
    row = np.repeat(np.arange(a.num_rows), lens)
    pos = np.arange(a.num_nonzeros) - ro[row]
    prod[row, pos] = a.values * x[a.column_indices]
    s = prod[:, 0::2] + prod[:, 1::2]
    while s.shape[1] > 1:
        w = s.shape[1] // 2
        s = s[:, :w] + s[:, w:]
    return s[:, 0]


def count_chunks(a, bounds):
    """Run chunks of a plan of whole-row tiles, as the plan forms them: within a tile, up to 6 consecutive
    rows whose column lists are prefixes of one list (rows of <= 64 columns: one chunk per run)."""
    ro, ci = a.row_offsets, a.column_indices
    chunks = 0
    for t in range(len(bounds) - 1):
        r, r1 = int(bounds[t][0]), int(bounds[t + 1][0])
        assert ro[r] == bounds[t][1] and ro[r1] == bounds[t + 1][1]
        while r < r1:
            pat = ci[ro[r]:ro[r + 1]]
            h = 1
            while r + h < r1 and h < 6:
                row = ci[ro[r + h]:ro[r + h + 1]]
                k = min(len(row), len(pat))
                if not np.array_equal(row[:k], pat[:k]):
                    break
                pat = row if len(row) > len(pat) else pat
                h += 1
            chunks += 1
            r += h
    return chunks


def column_runs_per_row(a):
    """Runs of consecutive columns in each row."""
    ro, ci = a.row_offsets.astype(np.int64), a.column_indices.astype(np.int64)
    brk = np.ones(a.num_nonzeros, bool)
    brk[1:] = np.diff(ci) != 1
    brk[ro[:-1]] = True
    return np.add.reduceat(brk.astype(np.int64), ro[:-1])


def run_pair(a, seed, runs_env, monkeypatch):
    if runs_env is None:
        monkeypatch.delenv("MSPMV_SPMV_RUNS", raising=False)
    else:
        monkeypatch.setenv("MSPMV_SPMV_RUNS", runs_env)
    x = np.random.default_rng(seed).uniform(-1, 1, a.num_cols)
    with mspmv.GpuCsr(a) as g:
        plan = g.tile_plan(1)
        y = g.spmv(x)
        info = {"kname": g.kernel_name(), "plan": plan, "nb": g.plan_block_tiles(1),
                "rounds": g.plan_block_rounds(1), "records": g.plan_block_records(1)}
    return x, y, info


def assert_pair_tree(name, a, x, y, info):
    want = pair_tree_spmv(a, x)
    bad = np.flatnonzero(y.view(np.uint64) != want.view(np.uint64))
    print(f"{name}: {info['kname']}, {info['nb']} of {info['plan']['num_tiles']} tiles on node blocks, "
          f"{info['rounds']} of two rounds, records (compact, escaped) {info['records']}, "
          f"{bad.size} of {a.num_rows} rows differ")
    assert info["kname"].startswith("k_spmv_blk<0,") and info["kname"].endswith(",6,false>"), info["kname"]
    assert bad.size == 0, (bad[:5], y[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("runs_env", [None, "0"])
def test_compact_records_bit_exact(monkeypatch, runs_env):
    """Shape 1: rows of 7-10 column-runs; every chunk has a compact record."""
    a = mspmv.CsrMatrix.synth_fem_blocked(4198, 222000, 6, 60, seed=5)
    cr = column_runs_per_row(a)
    assert cr.max() <= 10, np.bincount(cr)
    x, y, info = run_pair(a, 41, runs_env, monkeypatch)
    assert_pair_tree(f"shape1-runs{runs_env}", a, x, y, info)
    assert info["nb"] == info["plan"]["num_tiles"]
    compact, escaped = info["records"]
    assert escaped == 0
    assert compact == count_chunks(a, info["plan"]["bounds"])


def test_two_rounds_bit_exact(monkeypatch):
    """Shape 2: 36 per row on the merge-path plan, tiles of more than 8 chunks: records 8-15."""
    a = mspmv.CsrMatrix.synth_fem_blocked(4200, 151200, 6, 60, seed=5)
    x, y, info = run_pair(a, 42, "0", monkeypatch)
    assert_pair_tree("shape2", a, x, y, info)
    assert info["rounds"] > 0
    compact, escaped = info["records"]
    assert escaped == 0 and compact == count_chunks(a, info["plan"]["bounds"])


def test_odd_column_runs_bit_exact(monkeypatch):
    """Shape 3: nodes of 5 unknowns, column-runs of odd length, so lanes' pairs straddle two runs."""
    a = mspmv.CsrMatrix.synth_fem_blocked(4200, 210000, 5, 60, seed=5)
    ro, ci = a.row_offsets.astype(np.int64), a.column_indices.astype(np.int64)
    pos = np.arange(a.num_nonzeros) - np.repeat(ro[:-1], np.diff(ro))
    first = (pos % 2 == 0) & (np.arange(a.num_nonzeros) + 1 < np.repeat(ro[1:], np.diff(ro)))
    straddled = int(np.count_nonzero(ci[np.flatnonzero(first) + 1] != ci[first] + 1))
    assert straddled > a.num_rows  # more than one such pair per row
    x, y, info = run_pair(a, 43, None, monkeypatch)
    assert_pair_tree("shape3", a, x, y, info)
    assert info["records"][0] > 0 and info["records"][1] == 0


def test_mixed_plan_records(monkeypatch, orc):
    """Shape 4: odd nodes and off-pattern rows (1,250 rows with a pair straddling two column-runs; at this
    size every tile is still a register run tile), against the oracle."""
    monkeypatch.delenv("MSPMV_SPMV_RUNS", raising=False)
    a = mspmv.CsrMatrix.synth_fem_perturbed(4200, 222000, 6, 60, 0.05, 0.02, seed=5)
    x = np.random.default_rng(44).uniform(-1, 1, a.num_cols)
    with mspmv.GpuCsr(a) as g:
        plan = g.tile_plan(1)
        y = g.spmv(x)
        kname = g.kernel_name()
        compact, escaped = g.plan_block_records(1)
        check_parity(a, y, orc.spmv_gold(a, x), x, plan, 1)
    print(f"shape4: {kname}, records (compact, escaped) ({compact}, {escaped})")
    assert kname.startswith("k_spmv_blk<0,"), kname
    assert compact > 0


def fallback_matrix():
    """Shape 1 with 1,200 stencil rows (7 per row, no runs) below it."""
    f = mspmv.CsrMatrix.synth_fem_blocked(4198, 222000, 6, 60, seed=5)
    rng = np.random.default_rng(9)
    ms = 1200
    base = rng.integers(0, f.num_cols - 40, ms)
    ci = (base[:, None] + np.arange(0, 35, 5)[None, :]).astype(np.int32).reshape(-1)
    ro = np.concatenate([f.row_offsets, f.row_offsets[-1] + np.arange(7, 7 * ms + 1, 7)]).astype(np.int32)
    return mspmv.CsrMatrix.from_arrays(f.num_cols, ro, np.concatenate([f.column_indices, ci]),
                                       np.concatenate([f.values, rng.uniform(0.5, 1.5, 7 * ms)]))


def test_fallback_tiles_beside_records(monkeypatch, orc):
    """Shape 1 with 1,200 stencil rows (7 per row, no runs) below it: k_spmv_blk<.., true>, whose tiles
    without runs have all-zero records (count 0) and take the register fallback."""
    monkeypatch.delenv("MSPMV_SPMV_RUNS", raising=False)
    a = fallback_matrix()
    x = np.random.default_rng(47).uniform(-1, 1, a.num_cols)
    with mspmv.GpuCsr(a) as g:
        plan = g.tile_plan(1)
        y = g.spmv(x)
        kname = g.kernel_name()
        nb = g.plan_block_tiles(1)
        compact, escaped = g.plan_block_records(1)
        check_parity(a, y, orc.spmv_gold(a, x), x, plan, 1)
    print(f"fallback: {kname}, {nb} of {plan['num_tiles']} tiles on node blocks, records ({compact}, {escaped})")
    assert kname.startswith("k_spmv_blk<0,") and kname.endswith(",6,true>"), kname
    assert 0 < nb < plan["num_tiles"]
    assert compact > 0 and escaped == 0


def escape_matrix():
    """Shape 1 with every seventh node's rows on pairs of columns two apart over a window twice as wide:
    26-27 column-runs, the row lengths and the one list per node kept."""
    a = mspmv.CsrMatrix.synth_fem_blocked(4198, 222000, 6, 60, seed=5)
    ro = a.row_offsets.astype(np.int64)
    ci = a.column_indices.copy()
    for node in range(0, (a.num_rows + 5) // 6, 7):
        rows = range(6 * node, min(6 * node + 6, a.num_rows))
        j = np.arange(max(int(ro[r + 1] - ro[r]) for r in rows))
        rel = 4 * (j // 2) + (j % 2)
        start = max(min(int(ci[ro[rows[0]]]), a.num_cols - 1 - int(rel[-1])), 0)
        for r in rows:  # a shorter row keeps a prefix of the node's list
            ci[ro[r]:ro[r + 1]] = (start + rel)[: ro[r + 1] - ro[r]]
    assert ci.max() < a.num_cols
    return mspmv.CsrMatrix.from_arrays(a.num_cols, a.row_offsets, ci, a.values)


def test_escaped_records_bit_exact(monkeypatch):
    """Shape 5: chunks of 26-27 column-runs escape to the column stream, sharing tiles with compact ones."""
    a = escape_matrix()
    cr = column_runs_per_row(a)
    assert set(np.unique(cr[cr > 12])) <= {26, 27} and np.count_nonzero(cr > 12) >= 600
    x, y, info = run_pair(a, 45, None, monkeypatch)
    assert_pair_tree("shape5", a, x, y, info)
    compact, escaped = info["records"]
    assert escaped > 0 and compact > escaped
    assert compact + escaped == count_chunks(a, info["plan"]["bounds"])


def test_wide_column_range(monkeypatch, orc):
    """Shape 6: tiles whose columns span about 60,000: `start` uses its top bit."""
    monkeypatch.delenv("MSPMV_SPMV_RUNS", raising=False)
    a = mspmv.CsrMatrix.synth_fem_blocked(66000, 3498000, 6, 5000, seed=5)
    ro = a.row_offsets.astype(np.int64)
    span = a.column_indices[ro[1:] - 1].astype(np.int64) - a.column_indices[ro[:-1]]
    assert span.max() > 40000  # beyond 15 bits within single rows, let alone tiles
    x = np.random.default_rng(46).uniform(-1, 1, a.num_cols)
    with mspmv.GpuCsr(a) as g:
        plan = g.tile_plan(1)
        y = g.spmv(x)
        info = {"kname": g.kernel_name(), "plan": plan, "nb": g.plan_block_tiles(1),
                "rounds": g.plan_block_rounds(1), "records": g.plan_block_records(1)}
        if info["kname"].endswith(",6,false>"):
            assert_pair_tree("shape6", a, x, y, info)
        else:
            print(f"shape6: {info['kname']}, records {info['records']}")
            check_parity(a, y, orc.spmv_gold(a, x), x, plan, 1)
    assert info["kname"].startswith("k_spmv_blk<0,"), info["kname"]
    assert info["records"][0] > 0


# ---- the record boundary: 11, 12 and 13 column-runs, 63 and 64 columns, a pattern row that is not the run's first ----
R12_ODD = (3, 5) * 6                  # 48 columns in 12 runs; every run odd, so a lane's pair straddles every entry
R13 = R12_ODD + (4,)                  # 52 columns in 13 runs: one more than a record holds
BOUNDARY_SHAPES = {
    # name: (run lengths per node, cycled over the nodes; columns each node's first row is short by)
    "r11": ([(3, 5) * 5 + (3,)], 0),
    "r12_odd": ([R12_ODD], 0),
    "r12_ones_first": ([(1,) * 11 + (37,)], 0),
    "r12_ones_last": ([(37,) + (1,) * 11], 0),
    "r13": ([R13], 0),
    "mixed": ([R12_ODD, R13], 0),
    "w64": ([(5,) * 11 + (9,)], 0),
    "w63": ([(5,) * 11 + (8,)], 0),
    "short_first_r12_odd": ([R12_ODD], 5),
    "short_first_r13": ([R13], 5),
}
ESCAPING = {"r13", "mixed", "short_first_r13"}


def fem_nodes(run_lengths, short_first=0, nodes=700, n=6000, seed=0):
    """nodes - 1 FEM nodes of 6 rows and a last one of 2, the rows of a node sharing one column list: runs of
    consecutive columns of the lengths run_lengths[node % len(run_lengths)], separated by gaps of 1-3 columns, from a
    random first column (never equal to the node before's, so the two nodes' rows never agree on a prefix and no
    run of the plan joins them; the last node's list ends at column n - 1).  short_first > 0: each node's first row is the list less its last short_first columns, so the row that
    holds the run's pattern is not the run's first.  n = 6,000 keeps every tile on 16-bit columns."""
    rng = np.random.default_rng(seed)
    ro, ci = [0], []
    prev = -1
    for node in range(nodes):
        lens = run_lengths[node % len(run_lengths)]
        gaps = rng.integers(1, 4, len(lens) - 1)
        rel = np.concatenate([np.arange(ln) + off for ln, off in
                              zip(lens, np.concatenate([[0], np.cumsum(np.asarray(lens[:-1]) + gaps)]))])
        span = int(rel[-1]) + 1
        start = n - span if node == nodes - 1 else int(rng.integers(0, n - span + 1))
        if start == prev:
            start = start - 1 if start > 0 else start + 1
        prev = start
        for r in range(6 if node < nodes - 1 else 2):
            row = start + (rel[:-short_first] if short_first and r == 0 else rel)
            ci.append(row)
            ro.append(ro[-1] + row.size)
    ci = np.concatenate(ci).astype(np.int32)
    assert ci.min() >= 0 and ci.max() == n - 1
    va = rng.uniform(-1, 1, ci.size)
    return mspmv.CsrMatrix.from_arrays(n, np.asarray(ro, np.int32), ci, va)


def boundary_matrix(name):
    """The named boundary shape, its runs-per-row and widths asserted on the CPU (before any handle is made)."""
    run_lengths, short = BOUNDARY_SHAPES[name]
    a = fem_nodes(run_lengths, short_first=short, seed=sorted(BOUNDARY_SHAPES).index(name))
    cr = column_runs_per_row(a)
    lens = np.diff(a.row_offsets)
    node = np.arange(a.num_rows) // 6
    first = np.arange(a.num_rows) % 6 == 0
    want_runs = np.array([len(run_lengths[k % len(run_lengths)]) for k in node])
    want_len = np.array([sum(run_lengths[k % len(run_lengths)]) for k in node])
    if short:  # the first row lacks its last 5 columns: of R12_ODD's and of R13's list that is one run fewer
        assert np.array_equal(lens[first], want_len[first] - short) and np.array_equal(cr[first], want_runs[first] - 1)
    else:
        assert np.array_equal(lens[first], want_len[first]) and np.array_equal(cr[first], want_runs[first])
    assert np.array_equal(lens[~first], want_len[~first]) and np.array_equal(cr[~first], want_runs[~first])
    assert 32 <= lens.min() and lens.max() <= 64  # k_build_blocks: patterns >= 32 columns wide pay, <= 64 are one chunk
    assert a.num_rows % 6 == 2  # the last node has 2 rows
    assert a.column_indices[-1] == a.num_cols - 1
    return a, cr


@pytest.mark.parametrize("name,runs_env", [(k, None) for k in BOUNDARY_SHAPES] + [("mixed", "0"), ("r12_odd", "0")])
def test_record_boundary(monkeypatch, orc, name, runs_env):
    """Rows of exactly 11, 12 and 13 column-runs (a record holds 12: En = dword(4 + min(e + 1, 11)) reads the twelfth
    entry as its own successor), pairs that straddle every entry boundary, single-column runs first and last,
    patterns 64 and 63 columns wide (w63 and the others' last node end at column n - 1: the pair's lane with one
    column left), compact and escaped records in one tile (mixed), and a pattern row that is not the run's first,
    compact and escaped (pstart > 0) -- on the run-balanced plan and, for two shapes, on the merge-path plan
    (MSPMV_SPMV_RUNS=0: tiles of more than one round)."""
    a, cr = boundary_matrix(name)
    assert (cr.max() > 12) == (name in ESCAPING), np.bincount(cr)
    x, y, info = run_pair(a, 50, runs_env, monkeypatch)
    kname = info["kname"]
    compact, escaped = info["records"]
    print(f"{name} runs={runs_env}: {kname}, {info['nb']} of {info['plan']['num_tiles']} tiles on node blocks, "
          f"{info['rounds']} of two rounds, records (compact, escaped) ({compact}, {escaped}), "
          f"runs per row {np.flatnonzero(np.bincount(cr)).tolist()}")
    assert kname.startswith("k_spmv_blk<0,"), kname
    if name in ESCAPING:
        assert escaped > 0
        if name == "r13":
            assert compact == 0  # every chunk's pattern has 13 runs
        if name == "mixed":
            assert compact > 0
    else:
        assert compact > 0 and escaped == 0
    assert compact + escaped == count_chunks(a, info["plan"]["bounds"])
    if kname.endswith(",6,false>"):
        assert_pair_tree(f"{name}-runs{runs_env}", a, x, y, info)
    check_parity(a, y, orc.spmv_gold(a, x), x, info["plan"], 1)
