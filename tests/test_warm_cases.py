"""What test_gpu_warm_start.py relies on, pinned on the CPU: the exact-product systems of warm_cases.py are what
they claim (products exact in every order, R0 = E, ||B|| / ||R0|| in the thousands, each matrix of the shape that
takes its plan), and the numpy restatements of warm CG and warm BiCGSTAB meet the bars the GPU solvers are held to --
the X identity, the history shift, the entry test.

Which plan a handle takes is a device-side decision (mspmv_tile_plan needs a handle): here the host-side half is
checked -- mspmv_offset_windows accepts `windows`, the hub rows are longer than any tile, a node-block row holds 72
columns, the band lies in its half band -- and test_gpu_warm_start.py asserts the kernel each product ran."""
import numpy as np
import pytest

import warm_cases as wc

LD = np.longdouble


@pytest.mark.parametrize("sym", [True, False], ids=["sym", "nonsym"])
@pytest.mark.parametrize("name", wc.CASES)
def test_matrix_follows_the_value_rule(name, sym):
    ro, ci, va = wc.system(name, sym)
    n = len(ro) - 1
    r = np.repeat(np.arange(n), np.diff(ro))
    off = r != ci
    assert np.all(np.diff(ro) > 0) and np.all(va[off] != 0) and np.all(np.abs(va[off]) <= 1.0)
    assert np.array_equal(va * 64, np.round(va * 64))
    assert np.array_equal(va[~off], np.bincount(r[off], np.abs(va[off]), n) + 1.0)
    # the pattern is closed under transposition; sym: so are the values
    key = r.astype(np.int64) * n + ci
    order = np.argsort(ci.astype(np.int64) * n + r, kind="stable")
    assert np.array_equal(key, (ci.astype(np.int64) * n + r)[order])
    assert np.array_equal(va, va[order]) == sym


@pytest.mark.parametrize("sym", [True, False], ids=["sym", "nonsym"])
@pytest.mark.parametrize("name", wc.CASES)
def test_products_are_exact_in_every_order(name, sym):
    """float64 row sums against np.longdouble ones, bit for bit; R0 is E; the norms' ratio."""
    L = 4
    a, X0 = wc.system(name, sym), wc.guess(name, L)
    Bs, B = wc.exact_rhs(name, sym, L)
    assert np.array_equal(X0, np.round(X0)) and np.max(np.abs(X0)) <= 8
    assert np.array_equal(Bs.astype(LD), wc.csr_mm(a, X0, LD))
    # ... and in another order: the rows' entries reversed
    ro, ci, va = a
    rev = np.concatenate([np.arange(ro[i + 1] - 1, ro[i] - 1, -1) for i in range(len(ro) - 1)])
    assert np.array_equal(Bs, wc.csr_mm((ro, ci[rev], va[rev]), X0))
    R0 = wc.residual0(name, sym, L)
    assert np.array_equal(np.abs(R0), np.full(R0.shape, 1.0 / 64.0))
    assert np.array_equal((B.astype(LD) - wc.csr_mm(a, X0, LD)).astype(np.float64), R0)
    ratio = wc.col_norms(B) / wc.col_norms(R0)
    print(f"{name} {'sym' if sym else 'nonsym'}: ||B|| / ||R0|| = {ratio}")
    assert np.all(ratio >= 1e3)


def test_patterns_are_the_ones_named(mspmv):
    w = mspmv.offset_windows(wc.csr(wc.system("windows")))
    assert w is not None
    ro = wc.system("long_rows")[0]
    assert np.all(np.diff(ro)[list(wc.bc.HUBS)] >= 3000)   # a tile holds at most 2,048 + 256 merge items
    ro, ci, _ = wc.system("node_blocks")
    assert np.diff(ro).max() == 72 and np.all(np.diff(ro) % 8 == 0)
    ro, ci, _ = wc.system("band")
    r = np.repeat(np.arange(len(ro) - 1), np.diff(ro))
    assert len(ro) - 1 == 30000 and np.max(np.abs(ci - r)) <= 2000 and 40 <= np.diff(ro).mean() <= 81  # 40, their transposes, the diagonal


STENCILS = [(sym, k, seed) for sym in (True, False) for k in (4, 8, 16) for seed in range(5)]


def _stencil_system(sym, seed, L=4, nx=23, ny=19):
    a = wc.stencil5_dyadic(nx, ny, seed, sym)
    rng = np.random.default_rng(100 + seed)
    X0 = rng.integers(-8, 9, (nx * ny, L)).astype(np.float64)
    B = wc.csr_mm(a, X0) + rng.choice([-1.0, 1.0], X0.shape) / 64.0
    return a, B, X0


@pytest.mark.parametrize("sym,k,seed", STENCILS)
def test_restatements_meet_the_x_identity(sym, k, seed):
    """A warm solve of (B, X0) against X0 + the cold solve of (R0, 0), tol = 0, k iterations: the bar of the GPU test,
    on the symmetric and the convection-diffusion stencil; the L = 1 history against the cold one, by ||B|| / ||R0||."""
    a, B, X0 = _stencil_system(sym, seed)
    R0 = B - wc.csr_mm(a, X0)
    assert np.array_equal(np.abs(R0), np.full(R0.shape, 1.0 / 64.0))
    zero = np.zeros_like(X0)
    solvers = [(wc.bicgstab_warm, 2)] + ([(wc.cg_warm, 1)] if sym else [])
    for solve, adds in solvers:
        D = [zero] + [solve(a, R0, zero, i, 0.0)[0] for i in range(1, k + 1)]
        Xw, it, hw = solve(a, B, X0, k, 0.0)
        assert it == k and len(hw) == k
        room = wc.check_x_identity(f"{solve.__name__} sym={sym} k={k} seed={seed}", Xw, X0, D, adds)
        assert room <= 0.5   # (measured: 5 to 10 times inside the bar)
        _, _, h1 = solve(a, B[:, :1], X0[:, :1], k, 0.0)
        _, _, c1 = solve(a, R0[:, :1], zero[:, :1], k, 0.0)
        wc.check_history_shift(solve.__name__, len(B), h1, wc.col_norms(B[:, :1])[0], c1, wc.col_norms(R0[:, :1])[0])
        # normalised by the wrong norm the same figures miss by the norms' ratio
        with pytest.raises(AssertionError):
            wc.check_history_shift(solve.__name__, len(B), h1, wc.col_norms(R0[:, :1])[0], c1, wc.col_norms(R0[:, :1])[0])


@pytest.mark.parametrize("solve", [wc.cg_warm, wc.bicgstab_warm], ids=["cg", "bicgstab"])
def test_restatements_entry_test(solve):
    a, _, X0 = _stencil_system(True, 0)
    Bs = wc.csr_mm(a, X0)
    X, it, hist = solve(a, Bs, X0, 50, 1e-9)
    assert it == 0 and len(hist) == 0 and np.array_equal(X, X0)
    # one exact column among four: it stays bit for bit, the others are solved from the warm start
    B = Bs.copy()
    B[:, [0, 1, 3]] += np.random.default_rng(3).choice([-1.0, 1.0], (len(B), 3)) / 64.0
    X, it, hist = solve(a, B, X0, 200, 1e-9)
    _, it_cold, _ = solve(a, B, np.zeros_like(X0), 200, 1e-9)
    assert 0 < it < it_cold and np.array_equal(X[:, 2], X0[:, 2])
    res = wc.col_norms(B - wc.csr_mm(a, X)) / wc.col_norms(B)
    assert np.all(res <= 2e-9)
    # the stop test is relative to ||B||, not ||R0||: the first history entry is far below 1
    assert hist[0] < 1e-2


def test_inputs_are_shared_and_read_only():
    for arr in (*wc.system("windows"), wc.guess("windows", 4), wc.rhs("windows", True, 4), wc.residual0("windows", True, 4)):
        assert not arr.flags.writeable
    assert wc.rhs("windows", True, 4) is wc.rhs("windows", True, 4)
