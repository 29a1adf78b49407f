"""GPU: BiCGSTAB and ILU(0)-BiCGSTAB (csrc/mspmv_bicgstab.hip) on every product path of launch_solver_product --
offset windows with and without a remainder, column slabs, node blocks, merge tiles with split rows -- and in the
per-column freezes, on the matrices of bicgstab_cases.py against the numpy restatements (test_bicgstab.py,
test_ilu0.py; what these tests rely on is pinned by test_bicgstab_cases.py).  The product kernel is asserted by name
(mspmv_solver_product_kernel_name), never skipped on; every solve runs twice on its handle (the second replays the
cached graph) and must repeat bit for bit; the bars are bicgstab_cases.check_bars, which prints each figure.

This module is not among conftest's DEFAULT_PLAN_MODULES, so MSPMV_DIA=0 is set for it: the window cases unset it.
Every switch is set before the handle is created (a handle reads it at its first plan decision).

Measured on an MI355X, worst over each test's cases (bar): test_every_plan history 9.0e-16 (1e-10; windows 0.02 of the
spread bar), true residual 9.98e-10 (2e-9), |X - X_ref|_inf 3.3e-16 = 7.3e-4 of the rounding bar and 0.08 of the
residuals' sum (windows 1.4e-8 of 2 TOL cond); the declined slab 1.5e-19, 2.3e-10, 1.4e-4; test_cu_limit 1.9e-16,
9.8e-10, 3.1e-4, the same on 64 CUs; staggered 0.04 of the spread bar, 6.8e-10, 1.5e-9 of 2 TOL cond; freeze2x2's
live columns 7.7e-17, 3.8e-10, 1.2e-4, with ILU(0) 2.5e-16, 6.8e-10, 2.9e-4."""
import numpy as np
import pytest

import bicgstab_cases as bc
import test_bicgstab as tb
import test_ilu0 as ti
from test_bicgstab import TOL

pytestmark = pytest.mark.gpu
BREAKDOWN = 4
MAX_ITERS = 200
SOLVERS = ["bicgstab", "ilu0"]
FULL_REFERENCE = ("windows", "staggered", "freeze2x2")  # cheap, or judged by the spread of their orders


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    return gpu_available


class Run:
    """The case's handle, with its ILU(0) factor on the device for solver "ilu0"."""

    def __init__(self, mspmv, name, solver):
        self.mspmv, self.name, self.ilu = mspmv, name, solver == "ilu0"
        self.a = ti.matrix(name)
        self.g = mspmv.GpuCsr(ti.csr(self.a), device=0)
        self.m = None
        if self.ilu:
            ro, ci, _ = self.a
            self.m = mspmv.GpuIlu0(mspmv.CsrMatrix.from_arrays(len(ro) - 1, ro, ci, ti.factor(name)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.m is not None:
            self.m.close()
        self.g.close()

    def solve(self, B, max_iters=MAX_ITERS):
        if self.ilu:
            out = self.mspmv.pbicgstab_ilu0(self.g, self.m, B, max_iters, TOL, hist_cap=MAX_ITERS)
            assert self.g.cg_kernel_name() == "ILU0-BiCGSTAB (2 SpMM + 4 trsv + 5 passes)"
        else:
            out = self.g.bicgstab(B, max_iters, TOL, hist_cap=MAX_ITERS)
            assert self.g.cg_kernel_name() == "BiCGSTAB (2 SpMM + 5 passes)"
        return out

    def product(self, X0):
        return self.g.spmv(X0[:, 0])[:, None] if X0.shape[1] == 1 else self.g.spmm(X0)

    def refs(self, L):
        if self.name in FULL_REFERENCE:
            return bc.ilu_reference(self.name, L) if self.ilu else bc.reference(self.name, L)
        return bc.reference_order(self.name, L, self.ilu)

    def bars(self, label, B, out, **kw):
        X, it, hist, st = out
        if self.name in ("windows", "staggered"):  # no dominance margin: the stencil bars of test_gpu_bicgstab
            kw = dict(kw, cond=bc.cond(self.name), spread_history=True)
        return bc.check_bars(f"{label} {'ILU0-' if self.ilu else ''}BiCGSTAB", self.a, B, self.refs(B.shape[1]), X, it,
                             hist, st, **kw)


def same_bits(out, out2):
    (X, it, hist, st), (X2, it2, hist2, st2) = out, out2
    assert it2 == it and st2 == st
    np.testing.assert_array_equal(X2, X)
    np.testing.assert_array_equal(hist2, hist)


def check_kernel(g, name, L):
    """The solve's product kernel, by name; the plan's split rows (long_rows) and node-block tiles too."""
    k = g.solver_product_kernel_name()
    print(f"{name} L={L}: the solver's products ran {k}")
    if name in ("windows", "windows_rem"):
        assert k.startswith(f"k_spmm_dia<{L},"), k
    elif name == "band":
        assert k.startswith("k_spmm_slab<"), k
    elif name == "node_blocks6":  # every tile a register run tile: the node-block kernels
        assert k.startswith(f"k_spmm_blk<{L}," if L > 1 else "k_spmv_blk<"), k
        assert g.plan_block_tiles(L) > 0
    elif name == "node_blocks":
        # 72 columns per row, and boundary nodes: at L = 1 the tile kernel stages the node blocks itself, the
        # L-wide products keep their merge tiles (solver_plan: k_spmm_blk needs every tile a register run tile)
        assert k.startswith(f"k_spmm_tile<{L}," if L > 1 else "k_spmv_tile<"), k
        if L == 1:
            assert g.plan_block_tiles(1) > 0
    elif name == "long_rows":
        # the tile kernel in its form that closes split rows (the last template flag), on a plan that has some
        assert k.startswith(f"k_spmm_tile<{L}," if L > 1 else "k_spmv_tile<") and k.endswith(",true>"), k
        if L > 1:  # the plain L-wide product of this matrix runs on the same merge tiles
            assert g.tile_plan(L)["num_carries"] > 0
    return k


PLAN_CASES = [(name, L) for name in ("windows", "windows_rem", "long_rows", "node_blocks", "node_blocks6")
              for L in (1, 4, 16)]
PLAN_CASES += [("band", 8), ("band", 16)]


def set_switches(monkeypatch, name):
    if name in ("windows", "windows_rem"):
        monkeypatch.delenv("MSPMV_DIA", raising=False)
    if name == "band":
        monkeypatch.setenv("MSPMV_SPMM_SLAB", "1")


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name,L", PLAN_CASES)
def test_every_plan(mspmv, monkeypatch, name, L, solver):
    """Both solvers on each product path, with the control word, the workspace sized for the plan multiplied on, the
    prologue's ticket zeroing and the cached graph.  The handle's plain product is taken before the first solve,
    between the two and after the second, and never changes: a solve leaves no split-row ticket, carry or window
    state behind, and a plain product leaves none that a solve trips over."""
    set_switches(monkeypatch, name)
    B = bc.rhs(name, L)
    X0 = np.random.default_rng(100 + L).uniform(-1, 1, B.shape)
    with Run(mspmv, name, solver) as s:
        Y0 = s.product(X0)
        out = s.solve(B)
        check_kernel(s.g, name, L)
        Y1 = s.product(X0)
        out2 = s.solve(B)  # the cached graph, replayed, after a plain product
        Y2 = s.product(X0)
    s.bars(f"{name} L={L}", B, out)
    same_bits(out, out2)
    np.testing.assert_array_equal(Y1, Y0)
    np.testing.assert_array_equal(Y2, Y0)
    # (and it is the product: within the worst-case rounding of a 3,004-term row sum, twice -- here and there)
    mag = tb.csr_mm((s.a[0], s.a[1], np.abs(s.a[2])), np.abs(X0))
    assert np.all(np.abs(Y0 - tb.csr_mm(s.a, X0)) <= 2 * 3004 * 2.0 ** -53 * mag)


@pytest.mark.parametrize("solver", SOLVERS)
def test_single_rhs_declines_the_slab(mspmv, monkeypatch, solver):
    """MSPMV_SPMV_SLAB=4 puts the plain SpMV of the banded matrix on the sliced-ELL plan, which takes no control
    word: the L = 1 solve must multiply on the merge tiles instead."""
    monkeypatch.setenv("MSPMV_SPMV_SLAB", "4")
    B = bc.rhs("band", 1)
    with Run(mspmv, "band", solver) as s:
        assert s.g.kernel_name().startswith("k_spmv_sell<"), s.g.kernel_name()
        out = s.solve(B)
        k = s.g.solver_product_kernel_name()
        out2 = s.solve(B)
        assert s.g.kernel_name().startswith("k_spmv_sell<"), s.g.kernel_name()
    print(f"band L=1 with the plain SpMV on sliced ELL: the solver's products ran {k}")
    assert k.startswith("k_spmv_tile<"), k
    s.bars("band L=1, slab declined", B, out)
    same_bits(out, out2)


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", ["long_rows", "windows_rem"])
def test_cu_limit(mspmv, monkeypatch, name, solver):
    """After set_cu_limit(64) the plans are rebuilt for 64 CUs (split rows fall elsewhere, so the bits may differ
    from the full device's: test_split_rows_spmv): the solve meets the bars again and repeats itself."""
    set_switches(monkeypatch, name)
    L = 8
    B = bc.rhs(name, L)
    with Run(mspmv, name, solver) as s:
        out = s.solve(B)
        check_kernel(s.g, name, L)
        s.g.set_cu_limit(64)
        lim = s.solve(B)
        check_kernel(s.g, name, L)
        lim2 = s.solve(B)
    s.bars(f"{name} L={L}", B, out)
    s.bars(f"{name} L={L} on 64 CUs", B, lim)
    same_bits(lim, lim2)


@pytest.mark.parametrize("solver", SOLVERS)
def test_frozen_columns_stay_frozen(mspmv, solver):
    """staggered: columns 0 and 2 converge within 4 iterations (3 with ILU(0)), columns 1 and 3 dozens (at least 5)
    later.  A solve cut at 8 iterations runs the same kernels in the same order as the full one's first 8
    (test_max_iters relies on that for the history), so its columns 0 and 2 must hold the full solve's bits: a
    pass that lacked the converged-column mask would go on moving them -- towards the solution, past every other
    bar."""
    B = bc.rhs("staggered", 4)
    with Run(mspmv, "staggered", solver) as s:
        out = s.solve(B)
        out2 = s.solve(B)
        X8, it8, h8, st8 = s.solve(B, max_iters=8)
    s.bars("staggered L=4", B, out)
    same_bits(out, out2)
    X, it, hist, st = out
    assert st8 == 0 and it8 == 8 and it > 8 + 2
    np.testing.assert_array_equal(h8, hist[:8])
    np.testing.assert_array_equal(X8[:, [0, 2]], X[:, [0, 2]])
    moved = np.abs(X8[:, [1, 3]] - X[:, [1, 3]]).max()
    print(f"staggered: columns 1 and 3 moved by {moved:.3e} after iteration 8, columns 0 and 2 by nothing")
    assert moved > 0.0


def test_freeze_in_the_update(mspmv):
    """freeze2x2, unpreconditioned: column 0's omega is 0 with T.T != 0 and its beta 0 (-1 / 0) = NaN, so it freezes
    in k_bicg_update after the first iteration -- in small integers, so exactly -- and the other columns are
    solved: MSPMV_ERR_BREAKDOWN.  Alone, the column leaves no live column after one iteration."""
    a = tb.matrix("freeze2x2")
    B = bc.rhs("freeze2x2", 4)
    refs = bc.reference("freeze2x2", 4)
    with Run(mspmv, "freeze2x2", "bicgstab") as s:
        out = s.solve(B)
        out2 = s.solve(B)
        X1, it1, h1, st1 = s.solve(B[:, :1])
    X, it, hist, st = out
    assert st == BREAKDOWN and abs(it - refs["fsum"][1]) <= 1, (st, it)
    assert hist[0] == 4.0
    assert np.all(X[:bc.N_2X2, 0] == -1.0) and np.all(X[bc.N_2X2:, 0] == 0.0)
    bc.check_bars("freeze2x2 L=4 BiCGSTAB, columns 1..3", a, B, refs, X, it, hist, st, cols=[1, 2, 3])
    same_bits(out, out2)
    assert st1 == BREAKDOWN and it1 == 1 and list(h1) == [4.0]
    assert np.all(X1[:bc.N_2X2, 0] == -1.0) and np.all(X1[bc.N_2X2:, 0] == 0.0)


def test_freeze_case_with_ilu0_converges(mspmv):
    """freeze2x2 with ILU(0): the factor of a 2 x 2 block is exact, so column 0 converges in the first iteration
    instead of breaking down -- what the restatement gives in all four variants
    (test_bicgstab_cases.test_freeze2x2_with_ilu0_converges_instead) -- status 0, and the full bars hold."""
    B = bc.rhs("freeze2x2", 4)
    with Run(mspmv, "freeze2x2", "ilu0") as s:
        out = s.solve(B)
        out2 = s.solve(B)
        out1 = s.solve(B[:, :1])
    assert out[3] == 0 and out1[3] == 0 and out1[1] == 1
    s.bars("freeze2x2 L=4", B, out)
    s.bars("freeze2x2 L=1", B[:, :1], out1)
    same_bits(out, out2)
