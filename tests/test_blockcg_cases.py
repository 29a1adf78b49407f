"""CPU: what test_gpu_blockcg.py relies on in blockcg_cases.py -- the cases are SPD and keep their shapes, both
summation orders of the BCGrQ restatement converge on every case and stop within one iteration of each other, the
block iteration beats the lock-step CG where the GPU test says it does, and a rank-deficient block breaks down at
the init.  Numpy only."""
import numpy as np
import pytest

import blockcg_cases as kc
from blockcg_cases import TOL

CPU_WIDTHS = (2, 8, 16)


def dense(a):
    ro, ci, va = a
    n = len(ro) - 1
    d = np.zeros((n, n))
    d[np.repeat(np.arange(n), np.diff(ro)), ci] = va
    return d


@pytest.mark.parametrize("name", kc.NAMES)
def test_cases_are_spd(name):
    a = kc.matrix(name)
    d = dense(a)
    assert np.array_equal(d, d.T)
    assert np.linalg.eigvalsh(d).min() > 0.0
    ro, ci, _ = a
    assert all(np.all(np.diff(ci[ro[i]:ro[i + 1]]) > 0) for i in range(len(ro) - 1))


def test_case_shapes():
    """The laplacian is 48 x 47 = 2,256 rows of at most 5; the node cases hold 54 columns per interior row; hubs
    keeps its three hub rows, long enough to be split between merge tiles at every width."""
    assert len(kc.matrix("laplacian")[0]) - 1 == 48 * 47
    assert np.diff(kc.matrix("laplacian")[0]).max() == 5
    assert np.diff(kc.matrix("node_blocks")[0]).max() == 54
    assert set(np.diff(kc.matrix("node_torus")[0])) == {54}
    row_len = np.diff(kc.matrix("hubs")[0])
    assert all(row_len[h] > 1500 for h in kc.HUBS)


@pytest.mark.parametrize("L", CPU_WIDTHS)
@pytest.mark.parametrize("name", kc.NAMES)
def test_both_orders_converge(name, L):
    """Status 0 inside the iteration limit, the true residual within 2 TOL per column (the recurrence's residual
    norm is below TOL; the true one drifts from it by rounding), and the two counts at most 1 apart."""
    a, B = kc.system(name, L)
    refs = kc.reference(name, L)
    counts = [refs[o][1] for o in kc.ORDERS]
    for o in kc.ORDERS:
        X, it, hist, st, broke = refs[o]
        tr = kc.true_residual(a, B, X)
        print(f"{name} L={L} {o}: {it} iterations, worst true residual {tr.max():.3e}")
        assert st == 0 and broke is None and it < kc.MAX_ITERS and len(hist) == it
        assert hist[-1] < TOL and np.all(hist[:-1] >= TOL)
        assert np.all(tr <= 2 * TOL), tr
    assert abs(counts[0] - counts[1]) <= 1, counts


@pytest.mark.parametrize("L", kc.WIDTHS)
@pytest.mark.parametrize("name", kc.NAMES)
def test_history_bar_is_a_yardstick(name, L):
    """What admits a case: a further legitimate order of the Gram sums (chunks of 64 rows; on the scaled case also of
    37 and 100) meets the GPU test's own bars against the two orders -- the count within theirs widened by one, and
    over the prefix on which they agree to 1e-3 relative, the history within 4 x their largest difference so far
    + 1e-14.  A case on which the restatement's own reorderings miss that bar cannot hold the GPU to it."""
    a, B = kc.system(name, L)
    refs = kc.reference(name, L)
    (ia, ib), k, diff = kc.spread(refs)
    for chunk in ("64", "37", "100") if name == "scaled" else ("64",):
        _, it, hist, st, _ = kc.bcgrq(a, B, TOL, kc.MAX_ITERS, chunk)
        q = min(k, len(hist))
        ratio = np.abs(hist[:q] - refs[kc.ORDERS[0]][2][:q]) / (4.0 * np.maximum.accumulate(diff[:q]) + 1e-14)
        print(f"{name} L={L} chunks of {chunk}: {it} iterations ({ia}, {ib}), worst {ratio.max():.3g} of the bar over {q}")
        assert st == 0 and min(ia, ib) - 1 <= it <= max(ia, ib) + 1
        assert q > 0 and np.all(ratio <= 1.0)


def test_hard_case_converges():
    """scaled_hard: both orders converge within one iteration of each other at every width, far ahead of the
    lock-step CG at L = 16 -- and a third order misses the history bar, which is why it is no case of NAMES."""
    a, B = kc.system(kc.HARD, 16)
    _, it_lock, _ = kc.cg_lockstep(a, B, TOL, kc.MAX_ITERS)
    for L in kc.WIDTHS:
        refs = kc.reference(kc.HARD, L)
        counts = [refs[o][1] for o in kc.ORDERS]
        assert all(refs[o][3] == 0 for o in kc.ORDERS) and abs(counts[0] - counts[1]) <= 1
        a, B = kc.system(kc.HARD, L)
        assert all(np.all(kc.true_residual(a, B, refs[o][0]) <= 2 * TOL) for o in kc.ORDERS)
    assert 3 * max(counts) < it_lock


@pytest.mark.parametrize("L", [8, 16])
def test_block_needs_fewer_iterations_than_lockstep(L):
    refs = kc.reference("laplacian", L)
    _, it_lock, _ = kc.lockstep("laplacian", L)
    counts = [refs[o][1] for o in kc.ORDERS]
    print(f"laplacian L={L}: block {counts}, lock step {it_lock}")
    assert max(counts) < it_lock


def test_single_column_is_cg():
    """L = 1: the block recurrence is CG in another normalisation -- the same iteration count as the lock-step
    restatement's (within one) and the same history to rounding."""
    refs = kc.reference("laplacian", 1)
    _, it_lock, h_lock = kc.lockstep("laplacian", 1)
    for o in kc.ORDERS:
        _, it, hist, st, _ = refs[o]
        assert st == 0 and abs(it - it_lock) <= 1
        k = min(it, it_lock) - 1
        assert np.all(np.abs(hist[:k] - h_lock[:k]) <= 1e-9 * h_lock[:k] + 1e-14)


@pytest.mark.parametrize("order", kc.ORDERS)
@pytest.mark.parametrize("L", [2, 8])
def test_dependent_and_zero_columns_break_down_at_init(L, order):
    a, B = kc.system("node_blocks", L)
    dup = B.copy()
    dup[:, L - 1] = dup[:, 0]
    zero = B.copy()
    zero[:, 1] = 0.0
    for panel, pivot in ((dup, L - 1), (zero, 1)):
        X, it, hist, st, broke = kc.bcgrq(a, panel, TOL, 50, order)
        assert st == kc.BREAKDOWN and it == 0 and len(hist) == 0 and np.all(X == 0.0)
        assert broke == ("H", pivot)


def test_one_row_and_exhausted_space():
    """n = 1 (A = 16): the first iteration converges exactly, V = 0, so H's pivot 0 fails after X took its update:
    BREAKDOWN with one completed iteration, X = b / 16 and the history entry 0.  n = 129 converges at L = 16 in 7
    iterations, one short of the 8 that exhaust the block Krylov space."""
    a, B = kc.system(("chain", 1), 1)
    for o in kc.ORDERS:
        X, it, hist, st, broke = kc.reference_n(("chain", 1), 1)[o]
        assert st == kc.BREAKDOWN and it == 1 and broke == ("H", 0) and list(hist) == [0.0]
        np.testing.assert_array_equal(X, B / 16)
        assert kc.reference_n(("chain", 129), 16)[o][1] == 7 and kc.reference_n(("chain", 129), 16)[o][3] == 0


def test_small_algebra():
    """chol_upper, upper_inverse and mm against numpy on a random SPD 16 x 16, from the upper triangle alone."""
    rng = np.random.default_rng(3)
    M = rng.uniform(-1, 1, (40, 16))
    G = M.T @ M
    U, piv = kc.chol_upper(np.triu(G) + np.tril(rng.uniform(-1, 1, (16, 16)), -1))  # the lower triangle is ignored
    assert piv == -1 and np.allclose(U.T @ U, G, rtol=1e-13, atol=1e-13) and np.all(np.tril(U, -1) == 0.0)
    inv = kc.upper_inverse(U)
    assert np.allclose(inv @ U, np.eye(16), atol=1e-12) and np.all(np.tril(inv, -1) == 0.0)
    assert np.allclose(kc.mm(inv, inv.T.copy()), np.linalg.inv(G), rtol=1e-10, atol=1e-10)
    G[5, 5] = -1.0
    assert kc.chol_upper(G)[1] <= 5
    assert kc.chol_upper(np.full((2, 2), np.nan))[1] == 0


def test_gram_orders_differ_only_by_rounding():
    U = kc.rhs_n(2256, 8)
    V = kc.rhs_n(2256, 8, seed=9)
    a, b = kc.gram(U, V, "pairwise"), kc.gram(U, V, "chunks")
    assert np.allclose(a, U.T @ V, rtol=1e-13) and np.allclose(a, b, rtol=1e-13)
    assert np.any(a != b)  # two orders, not one


def test_entry_points_exported(mspmv):
    """The library exports both entry points, the header declares them and the binding wraps them (no device)."""
    import os

    for sym in ("mspmv_dbcg_multi", "mspmv_dbcg_multi_dev"):
        assert hasattr(mspmv.lib, sym)
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mspmv.h")) as f:
            assert f"mspmv_status {sym}(" in f.read()
    assert callable(mspmv.GpuCsr.block_cg) and callable(mspmv.GpuCsr.block_cg_dev)
