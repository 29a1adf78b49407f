"""GPU: the block CG (mspmv_dbcg_multi, csrc/mspmv_blockcg.hip) against the numpy restatement of blockcg_cases.py,
whose two summation orders of the Gram sums measure how far a legitimate reordering moves the iterates
(test_blockcg_cases.py pins what is relied on here).  The bars, each a multiple of the restatement's own spread:
  status 0; iterations within the two orders' counts widened by one on either side;
  history: over the prefix on which the two orders agree to 1e-3 relative, |h - h_pairwise| <= 4 x the largest
    |h_pairwise - h_chunks| met so far + 1e-14 (the running maximum, as test_gpu_bicgstab.check_history's);
  true residual ||B_j - A X_j|| / ||B_j|| in np.longdouble: per column <= 4 x the larger of the two orders' own.
Every figure is printed before it is asserted.

Measured on an MI355X, worst over all cases and widths: history 0.23 of its bar (laplacian L = 1, 3.1e-15; the node
and hub cases 0.02 of it), true residual 0.25 of its bar everywhere (the restatement's own, to three digits),
iteration counts equal to the restatement's in every case; scaled_hard: 143 iterations for the restatement's 145 at
L = 1, 69 for 70 / 69 at L = 8, true residual at most 0.33 of its bar.

This module is not among conftest's DEFAULT_PLAN_MODULES, so MSPMV_DIA=0 is set for it: the laplacian unsets it (the
switch is read at the handle's first plan decision)."""
import numpy as np
import pytest

import blockcg_cases as kc
from blockcg_cases import TOL

pytestmark = pytest.mark.gpu
BREAKDOWN, INVALID, UNSUPPORTED = 4, 1, 6
MAX_ITERS = 400
K_SLOT_GROUP = 32  # csrc/mspmv_internal.h kSlotGroup: the fan-in of a fold level


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    return gpu_available


def csr(mspmv, a):
    ro, ci, va = a
    return mspmv.CsrMatrix.from_arrays(len(ro) - 1, ro, ci, va)


def set_switches(monkeypatch, key):
    if key == "laplacian":
        monkeypatch.delenv("MSPMV_DIA", raising=False)


def check_bars(label, key, L, out):
    """A solve (X, it, hist, st) of system(key, L) against reference_n(key, L); returns the printed figures."""
    X, it, hist, st = out
    a, B = kc.system(key, L)
    refs = kc.reference_n(key, L)
    (ia, ib), k, diff = kc.spread(refs)
    h_ref = refs[kc.ORDERS[0]][2]
    tr = kc.true_residual(a, B, X)
    tr_ref = np.maximum(*(kc.true_residual(a, B, refs[o][0]) for o in kc.ORDERS))
    q = min(k, len(hist))
    err = np.abs(hist[:q] - h_ref[:q])
    bar = 4.0 * np.maximum.accumulate(diff[:q]) + 1e-14
    hratio = float(np.max(err / bar)) if q else 0.0
    print(f"\n{label}: status {st}, iterations {it} (restatement {ia}, {ib}), history prefix {q} of {len(hist)}: worst "
          f"deviation {float(err.max()) if q else 0.0:.3e} = {hratio:.3g} of its bar, worst true residual "
          f"{tr.max():.3e} = {float(np.max(tr / (4 * tr_ref))):.3g} of its bar")
    assert st == 0, f"status {st}"
    assert min(ia, ib) - 1 <= it <= max(ia, ib) + 1, f"iterations {it} against {ia}, {ib}"
    assert len(hist) == it, f"history length {len(hist)} of {it} iterations"
    assert q > 0 and np.all(err <= bar), f"history deviation {hratio:.3g} of its bar"
    assert np.all(np.isfinite(X)) and np.all(tr <= 4 * tr_ref), f"true residual {tr} against {tr_ref}"
    return hratio, float(np.max(tr / (4 * tr_ref)))


def check_kernel(g, key, L):
    k = g.solver_product_kernel_name()
    print(f"{key} L={L}: the product ran {k}")
    if key == "laplacian":
        assert k.startswith(f"k_spmm_dia<{L},"), k
    elif key in ("node_blocks", "node_torus"):
        assert k.startswith(f"k_spmm_blk<{L}," if L > 1 else "k_spmv_blk<"), k
    elif key == "hubs":
        assert k.startswith(f"k_spmm_tile<{L}," if L > 1 else "k_spmv_tile<"), k
        if L > 1:
            assert k.endswith(",true>") and g.tile_plan(L)["num_carries"] > 0, k  # rows split between tiles


def same_bits(out, out2):
    (X, it, hist, st), (X2, it2, hist2, st2) = out, out2
    assert it2 == it and st2 == st
    np.testing.assert_array_equal(X2, X)
    np.testing.assert_array_equal(hist2, hist)


CASES = [(name, L) for name in kc.NAMES for L in kc.WIDTHS]
CASES += [(("chain", 129), 16), (("chain", 129), 1)]  # (n = 1: test_one_row)


@pytest.mark.parametrize("key,L", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_against_restatement(mspmv, monkeypatch, key, L):
    """Every case and width, and n = 129 at L = 16 and at L = 1 (odd: the L = 1 passes' last single row) -- solved
    twice on the handle, the second solve replaying the cached graph bit for bit."""
    set_switches(monkeypatch, key)
    a, B = kc.system(key, L)
    with mspmv.GpuCsr(csr(mspmv, a), device=0) as g:
        out = g.block_cg(B, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
        assert g.cg_kernel_name() == "BlockCG-rQ (1 SpMM + 3 passes)"
        check_kernel(g, key, L)
        out2 = g.block_cg(B, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
    check_bars(f"{key} L={L}", key, L, out)
    same_bits(out, out2)


def test_fold_depth(mspmv, monkeypatch):
    """The laplacian's 2,256 rows at L = 8 are 9,024 pairs: 36 pass blocks, over one fold group, so the Gram folds
    run two levels; n = 129 at L = 1 is one block, whose fold is a single arrival."""
    set_switches(monkeypatch, "laplacian")
    a, _ = kc.system("laplacian", 8)
    with mspmv.GpuCsr(csr(mspmv, a), device=0) as g:
        blocks, _ = g.solver_pass_shape(8)
        assert K_SLOT_GROUP < blocks <= K_SLOT_GROUP ** 2, blocks
        check_bars("laplacian L=8, two fold levels", "laplacian", 8, g.block_cg(kc.rhs("laplacian", 8), MAX_ITERS, TOL,
                                                                                hist_cap=MAX_ITERS))
    a1, B1 = kc.system(("chain", 129), 1)
    with mspmv.GpuCsr(csr(mspmv, a1), device=0) as g:
        assert g.solver_pass_shape(1)[0] == 1
        check_bars("chain129 L=1, one block", ("chain", 129), 1, g.block_cg(B1, MAX_ITERS, TOL, hist_cap=MAX_ITERS))


@pytest.mark.parametrize("L", [8, 16])
def test_fewer_iterations_than_lockstep_cg(mspmv, monkeypatch, L):
    set_switches(monkeypatch, "laplacian")
    a, B = kc.system("laplacian", L)
    with mspmv.GpuCsr(csr(mspmv, a), device=0) as g:
        _, it_block, _, st = g.block_cg(B, MAX_ITERS, TOL)
        _, it_cg, _, st_cg = g.cg_multi(B, MAX_ITERS, TOL)
    print(f"\nlaplacian L={L}: block CG {it_block} iterations, cg_multi {it_cg}")
    assert st == 0 and st_cg == 0 and it_block < it_cg


@pytest.mark.parametrize("key", ["laplacian", "node_blocks"])
def test_single_column_agrees_with_cg(mspmv, monkeypatch, key):
    """L = 1: the block recurrence is CG in another normalisation -- cg_multi's iteration count or one off, and the
    true residual within the restatement's bar."""
    set_switches(monkeypatch, key)
    a, B = kc.system(key, 1)
    with mspmv.GpuCsr(csr(mspmv, a), device=0) as g:
        out = g.block_cg(B, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
        _, it_cg, _, st_cg = g.cg_multi(B, MAX_ITERS, TOL)
    print(f"\n{key} L=1: block CG {out[1]} iterations, cg_multi {it_cg}")
    assert st_cg == 0 and abs(out[1] - it_cg) <= 1
    check_bars(f"{key} L=1", key, 1, out)


def test_graphed_and_ungraphed(mspmv, monkeypatch):
    """max_iters below a batch runs ungraphed and stops there, above it replays the cached graph: the short solve's
    history is the long one's head, bit for bit (the same kernels in the same order)."""
    set_switches(monkeypatch, "laplacian")
    a, B = kc.system("laplacian", 4)
    with mspmv.GpuCsr(csr(mspmv, a), device=0) as g:
        _, K = g.solver_pass_shape(4)
        assert 5 < K < 100
        full = g.block_cg(B, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
        X5, it5, h5, st5 = g.block_cg(B, 5, TOL, hist_cap=MAX_ITERS)
        XK, itK, hK, stK = g.block_cg(B, K + 3, TOL, hist_cap=MAX_ITERS)  # one replay, then three launched singly
    check_bars("laplacian L=4", "laplacian", 4, full)
    assert full[1] > K + 3
    assert st5 == 0 and it5 == 5 and len(h5) == 5 and stK == 0 and itK == K + 3
    np.testing.assert_array_equal(h5, full[2][:5])
    np.testing.assert_array_equal(hK, full[2][:K + 3])
    assert np.all(np.isfinite(X5)) and np.all(np.isfinite(XK))


def test_repeated_and_alternating_solves(mspmv):
    """A second solve repeats the first bit for bit; so does a third after a cg_multi and a bicgstab solve on the
    same handle, which share the workspace and keep graphs of their own."""
    a, B = kc.system("hubs", 8)
    with mspmv.GpuCsr(csr(mspmv, a), device=0) as g:
        out = g.block_cg(B, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
        out2 = g.block_cg(B, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
        Xc, _, _, stc = g.cg_multi(B, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
        Xb, _, _, stb = g.bicgstab(B, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
        out3 = g.block_cg(B, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
        Xc2, _, _, _ = g.cg_multi(B, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
    check_bars("hubs L=8", "hubs", 8, out)
    assert stc == 0 and stb == 0
    same_bits(out, out2)
    same_bits(out, out3)
    np.testing.assert_array_equal(Xc2, Xc)
    assert np.all(kc.true_residual(a, B, Xc) <= 2 * TOL) and np.all(kc.true_residual(a, B, Xb) <= 2 * TOL)


@pytest.mark.parametrize("L", [2, 16])
def test_breakdown_at_init(mspmv, L):
    """A duplicated column, then a zero column: H = B^T B has a zero pivot, MSPMV_ERR_BREAKDOWN with no iteration
    run and X = 0; the error text names the matrix and the pivot.  The next solve on the handle is clean."""
    a, B = kc.system("node_blocks", L)
    dup = B.copy()
    dup[:, L - 1] = dup[:, 0]
    zero = B.copy()
    zero[:, 1] = 0.0
    with mspmv.GpuCsr(csr(mspmv, a), device=0) as g:
        for panel, pivot in ((dup, L - 1), (zero, 1)):
            X, it, hist, st = g.block_cg(panel, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
            msg = mspmv.lib.mspmv_last_error().decode()
            print(f"\nL={L}: {msg}")
            assert st == BREAKDOWN and it == 0 and len(hist) == 0
            assert np.all(X == 0.0)  # and so no NaN
            assert f"pivot {pivot} of H" in msg and "mspmv_dcg_multi" in msg and "init" in msg
        out = g.block_cg(B, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
    check_bars(f"node_blocks L={L} after two breakdowns", "node_blocks", L, out)


@pytest.mark.parametrize("L", [1, 2, 16])
def test_one_row(mspmv, L):
    """n = 1, A = 16.  L = 1: the first iteration converges exactly -- every quantity a power of two times b -- so
    V = 0 and H's pivot fails after X took its update: MSPMV_ERR_BREAKDOWN by the one rule, one iteration completed,
    X = b / 16, the history entry 0 (the restatement's outcome, test_blockcg_cases).  L > 1: a 1 x L block has rank 1,
    so the init breaks down on pivot 1 of H, X = 0."""
    a, B = kc.system(("chain", 1), L)
    with mspmv.GpuCsr(csr(mspmv, a), device=0) as g:
        X, it, hist, st = g.block_cg(B, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
        msg = mspmv.lib.mspmv_last_error().decode()
    print(f"\nn=1 L={L}: {msg}")
    assert st == BREAKDOWN
    if L == 1:
        assert it == 1 and list(hist) == [0.0] and "pivot 0 of H" in msg and "iteration 0" in msg, msg
        np.testing.assert_array_equal(X, B / 16)
    else:
        assert it == 0 and len(hist) == 0 and np.all(X == 0.0) and "pivot 1 of H" in msg, msg


def test_rounding_sensitive_solve(mspmv):
    """scaled_hard (blockcg_cases: the restatement's own reorderings part too far for the history bar there): the
    bars that hold regardless -- status 0 and, per column, the true residual within 4 x the two orders' own -- and
    the solve repeats bit for bit."""
    for L in (1, 8, 16):
        a, B = kc.system(kc.HARD, L)
        refs = kc.reference(kc.HARD, L)
        with mspmv.GpuCsr(csr(mspmv, a), device=0) as g:
            out = g.block_cg(B, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
            out2 = g.block_cg(B, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
        tr = kc.true_residual(a, B, out[0])
        tr_ref = np.maximum(*(kc.true_residual(a, B, refs[o][0]) for o in kc.ORDERS))
        print(f"\n{kc.HARD} L={L}: status {out[3]}, iterations {out[1]} (restatement "
              f"{[refs[o][1] for o in kc.ORDERS]}), worst true residual {tr.max():.3e} = "
              f"{float(np.max(tr / (4 * tr_ref))):.3g} of its bar")
        assert out[3] == 0 and len(out[2]) == out[1] and np.all(tr <= 4 * tr_ref)
        same_bits(out, out2)


def test_argument_contract(mspmv):
    a, B = kc.system("scaled", 2)
    n = B.shape[0]
    with mspmv.GpuCsr(csr(mspmv, a), device=0) as g:
        with pytest.raises(mspmv.MspmvError) as ei:
            g.block_cg(np.ones((n, 3)), 10, TOL)
        assert ei.value.status == UNSUPPORTED
        with pytest.raises(mspmv.MspmvError) as ei:
            g.block_cg(B, -1, TOL)
        assert ei.value.status == INVALID
        dB, dX = mspmv.DeviceBuffer.from_array(B), mspmv.DeviceBuffer.from_array(np.full(2 * n + 2, 7.0))

        class Null:
            ptr = None

        class Shifted:
            ptr = dX.ptr + 8

        for bad_b, bad_x, L, iters, status in ((dB, dX, 3, 10, UNSUPPORTED), (Null, dX, 2, 10, INVALID),
                                               (dB, Null, 2, 10, INVALID), (dB, Shifted, 2, 10, INVALID),
                                               (dB, dX, 2, -1, INVALID)):
            with pytest.raises(mspmv.MspmvError) as ei:
                g.block_cg_dev(bad_b, bad_x, L, iters, TOL)
            assert ei.value.status == status, (L, iters, ei.value.status)
            assert np.all(dX.download((2 * n + 2,)) == 7.0)  # X untouched
        it, hist, st = g.block_cg_dev(dB, dX, 2, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
        Xd = dX.download((2 * n + 2,))
        X, it_h, hist_h, st_h = g.block_cg(B, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
        dB.free()
        dX.free()
    assert st == 0 and st_h == 0 and it == it_h
    np.testing.assert_array_equal(Xd[:2 * n].reshape(n, 2), X)
    assert np.all(Xd[2 * n:] == 7.0)
    np.testing.assert_array_equal(hist, hist_h)
    ro = np.arange(0, 11, dtype=np.int32)
    rect = mspmv.CsrMatrix.from_arrays(12, ro, np.arange(10, dtype=np.int32), np.ones(10))
    with mspmv.GpuCsr(rect, device=0) as g:
        with pytest.raises(mspmv.MspmvError) as ei:
            g.block_cg(np.ones((10, 2)), 10, TOL)
        assert ei.value.status == INVALID


def test_limits(mspmv):
    """max_iters = 0: X = 0 and no history.  hist_cap below the iteration count: that many entries are written, and
    they are the full history's head."""
    a, B = kc.system("hubs", 4)
    with mspmv.GpuCsr(csr(mspmv, a), device=0) as g:
        X0, it0, h0, st0 = g.block_cg(B, 0, TOL, hist_cap=50)
        full = g.block_cg(B, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
        cap = 5
        it = ctypes_solve_with_guard(mspmv, g, B, cap)
    assert st0 == 0 and it0 == 0 and len(h0) == 0 and np.all(X0 == 0.0)
    assert full[3] == 0 and full[1] > cap
    assert it[0] == full[1]
    np.testing.assert_array_equal(it[1][:cap], full[2][:cap])
    assert np.all(it[1][cap:] == -1.0)  # nothing written past hist_cap


def ctypes_solve_with_guard(mspmv, g, B, cap):
    """mspmv_dbcg_multi with hist_cap = cap into a longer history buffer filled with -1: (iterations, buffer)."""
    import ctypes

    B = np.ascontiguousarray(B, np.float64)
    X = np.empty_like(B)
    hist = np.full(cap + 16, -1.0)
    it = ctypes.c_int()
    st = mspmv.lib.mspmv_dbcg_multi(g.h, B.ctypes.data_as(ctypes.c_void_p), X.ctypes.data_as(ctypes.c_void_p),
                                    B.shape[1], MAX_ITERS, TOL, ctypes.byref(it),
                                    hist.ctypes.data_as(ctypes.c_void_p), cap)
    assert st == 0
    return it.value, hist


@pytest.mark.parametrize("value", [32, 0x7FFFFFFF, 0xFFFFFFFF])
def test_poisoned_tickets(mspmv, value):
    """test_gpu_faults' hook and values on this solver's folds: dirty tickets when the iterations begin make an
    arrival draw past its group, and the solve stops with MSPMV_ERR_FAULT instead of hanging or returning a stale
    sum; the next solve starts from re-zeroed tickets and meets the bars."""
    a, B = kc.system("hubs", 8)
    with mspmv.GpuCsr(csr(mspmv, a), device=0) as g:
        g.test_poison_tickets(value, mspmv.POISON_FILL)
        with pytest.raises(mspmv.MspmvError) as ei:
            g.block_cg(B, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
        assert ei.value.status == mspmv.FAULT
        out = g.block_cg(B, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
    check_bars(f"hubs L=8 after poison {value:#x}", "hubs", 8, out)
