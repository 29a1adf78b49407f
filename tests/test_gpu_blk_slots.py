"""GPU: the node-block kernels' pattern-column slots (TilePlan::d_pcols).

Every reader of a run's pattern columns takes them from the chunk's 128-B slot instead of the CSR-ordered
16-bit stream; the products, the sums and their order are what they were.  So the tests here state
behaviour, not layout:

* the column-pair kernel (k_spmv_blk<0, NT, 6, false>) sums a row of <= 64 entries by a tree that depends
  on the row alone -- prod[k] = val[k] * x[col[k]] padded with +0.0 to 64, pair[l] = prod[2l] + prod[2l+1],
  then halves of 16, 8, 4, 2, 1 -- restated in numpy below and required bit for bit, on plans of one round
  of run slots per tile (descriptor stride 8), of run heights below 6 and of two rounds (slots 8-15);
* the other readers (k_spmv_tile's LDS staging of two-chunk runs, the mixed plan's fallback tiles, which
  stay on the 16-bit stream, and k_spmm_blk at L = 2 and 16) against the oracle under check_parity.
"""
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


# (m, nnz, MSPMV_SPMV_RUNS, tiles of more than 8 chunks expected)
PAIR_CASES = {
    # rows of 52 and 53 as in pwtk, the last node 4 rows, the last columns at n - 1
    "pwtk_like-auto": (4198, 222000, None, False),
    # the merge-path plan: runs cut at tile ends (heights below 6), descriptor strides above 8
    "pwtk_like-runs0": (4198, 222000, "0", False),
    # 36 per row, ~9.5 runs per 2,048 items: a second round of run slots (slots 8-15)
    "narrow-runs0": (4200, 151200, "0", True),
}


@pytest.mark.parametrize("name", list(PAIR_CASES))
def test_pair_kernel_bit_exact(monkeypatch, name):
    m, nnz, runs, two_rounds = PAIR_CASES[name]
    if runs is None:
        monkeypatch.delenv("MSPMV_SPMV_RUNS", raising=False)
    else:
        monkeypatch.setenv("MSPMV_SPMV_RUNS", runs)
    a = mspmv.CsrMatrix.synth_fem_blocked(m, nnz, 6, 60, seed=5)
    x = np.random.default_rng(31).uniform(-1, 1, a.num_cols)
    with mspmv.GpuCsr(a) as g:
        plan = g.tile_plan(1)
        y = g.spmv(x)
        kname = g.kernel_name()
        nb = g.plan_block_tiles(1)
        rounds = g.plan_block_rounds(1)
    want = pair_tree_spmv(a, x)
    bad = np.flatnonzero(y.view(np.uint64) != want.view(np.uint64))
    print(f"{name}: {kname}, {nb} of {plan['num_tiles']} tiles on node blocks, {rounds} of two rounds, "
          f"{bad.size} of {a.num_rows} rows differ")
    assert kname.startswith("k_spmv_blk<0,") and kname.endswith(",6,false>"), kname
    assert nb == plan["num_tiles"], (nb, plan["num_tiles"])
    if two_rounds:
        assert rounds > 0
    assert bad.size == 0, (bad[:5], y[bad[:5]], want[bad[:5]])


def test_two_chunk_runs_tile_kernel(orc):
    """100 columns per row: two chunks per run, the second slot starting at pattern column 64
    (k_spmv_tile's node-block staging)."""
    a = mspmv.CsrMatrix.synth_fem_blocked(4200, 420000, 6, 60, seed=5)
    x = np.random.default_rng(32).uniform(-1, 1, a.num_cols)
    with mspmv.GpuCsr(a) as g:
        y = g.spmv(x)
        kname = g.kernel_name()
        nb = g.plan_block_tiles(1)
        check_parity(a, y, orc.spmv_gold(a, x), x, g.tile_plan(1), 1)
    assert kname.startswith("k_spmv_tile<"), kname
    assert nb > 0


def test_mixed_plan_fallback_tiles(orc):
    """Odd nodes and off-pattern rows: the fallback tiles of k_spmv_blk<.., true> read the 16-bit stream."""
    a = mspmv.CsrMatrix.synth_fem_perturbed(4200, 222000, 6, 60, 0.05, 0.02, seed=5)
    x = np.random.default_rng(33).uniform(-1, 1, a.num_cols)
    with mspmv.GpuCsr(a) as g:
        plan = g.tile_plan(1)
        y = g.spmv(x)
        kname = g.kernel_name()
        nb = g.plan_block_tiles(1)
        check_parity(a, y, orc.spmv_gold(a, x), x, plan, 1)
    assert kname.startswith("k_spmv_blk<0,"), kname
    assert 0 < nb <= plan["num_tiles"]


@pytest.mark.parametrize("L", [2, 16])
def test_spmm_blk_slots(orc, L):
    a = mspmv.CsrMatrix.synth_fem_blocked(4198, 222000, 6, 60, seed=5)
    X = np.random.default_rng(34 + L).uniform(-1, 1, (a.num_cols, L))
    with mspmv.GpuCsr(a) as g:
        Y = g.spmm(X)
        kname = g.spmm_kernel_name(L)
        check_parity(a, Y, orc.csr_spmm_t(a, X), X, g.tile_plan(L), L)
    assert kname.startswith(f"k_spmm_blk<{L},"), kname

