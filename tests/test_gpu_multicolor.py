"""GPU: the multi-colour ILU(0) factor (mspmv_ilu0_create_colored, csrc/mspmv_color.hip) -- its triangular solves
alone and its apply, bit for bit against the numpy restatement (multicolor_cases.py: test_ilu0.TriPlan on the
permuted factor, rows summed in CSR order), and mspmv_dpbicgstab_ilu0_multi on such a factor against the
restated recurrence under test_gpu_ilu0's bars."""
import numpy as np
import pytest

import multicolor_cases as mc
import test_bicgstab as tb
import test_gpu_ilu0 as tg
import test_ilu0 as ti
from test_bicgstab import TOL

pytestmark = pytest.mark.gpu
INVALID, BREAKDOWN, UNSUPPORTED = 1, 4, 6
MAX_ITERS = 200


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    return gpu_available


def kernel_name(name):
    return f"MC-ILU0-BiCGSTAB (2 SpMM + 4 sweeps of {mc.ordering(name)[1]} colours + 5 passes)"


class Solver:
    """The matrix's handle and its multi-colour ILU(0) factor on the device."""

    def __init__(self, mspmv, name):
        self.mspmv = mspmv
        self.g = mspmv.GpuCsr(mc.csr(mc.matrix(name)), device=0)
        self.m = mspmv.GpuIlu0.colored(mc.csr(mc.matrix(name)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.m.close()
        self.g.close()

    def solve(self, B, max_iters=MAX_ITERS, hist_cap=MAX_ITERS, tol=TOL):
        return self.mspmv.pbicgstab_ilu0(self.g, self.m, B, max_iters, tol, hist_cap=hist_cap)


def panel(n, L, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (n, L))


# ---- the solves alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("upper", [0, 1])
@pytest.mark.parametrize("L", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("name", ["randdd", "hubs", "chain515"])
def test_solve_is_the_restatement(mspmv, name, L, upper):
    """One triangle of the permuted factor, in the colour ordering: TriPlan's bits, and the same on a repeat.
    hubs: a row of 599 entries alone in its colour (the split pairwise sum); chain515: colours of 258 and 257
    rows, past one workgroup at L = 1."""
    n = len(mc.matrix(name)[0]) - 1
    B = panel(n, L, 3000 + 10 * L + upper)
    want = mc.tri_plans(name, "csr")[upper].solve(B)
    with Solver(mspmv, name) as s:
        assert s.m.num_colors == mc.ordering(name)[1]
        np.testing.assert_array_equal(s.m.perm, mc.ordering(name)[2])
        X = s.m.solve(s.g, B, upper=bool(upper))
        X2 = s.m.solve(s.g, B, upper=bool(upper))
    np.testing.assert_array_equal(X, want)
    np.testing.assert_array_equal(X2, X)


# ---- the apply ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 8])
@pytest.mark.parametrize("name", ["randdd", "hubs", "chain515"])
def test_apply_is_the_restatement(mspmv, name, L):
    n = len(mc.matrix(name)[0]) - 1
    B = panel(n, L, 4000 + L)
    with Solver(mspmv, name) as s:
        Z = s.m.apply(s.g, B)
        Z2 = s.m.apply(s.g, B)
    np.testing.assert_array_equal(Z, mc.apply_ref(name, B))  # gather, L^-1, U^-1, scatter
    np.testing.assert_array_equal(Z2, Z)


@pytest.mark.parametrize("L", [1, 8])
@pytest.mark.parametrize("name", ["randdd", "hubs"])
def test_apply_on_a_natural_order_factor_is_its_two_solves(mspmv, name, L):
    n = len(mc.matrix(name)[0]) - 1
    B = panel(n, L, 5000 + L)
    with tg.Solver(mspmv, name) as s:
        assert s.m.num_colors == 0 and s.m.perm is None and s.m.num_rows == n
        Z = s.m.apply(s.g, B)
        want = s.m.solve(s.g, s.m.solve(s.g, B, upper=False), upper=True)
    np.testing.assert_array_equal(Z, want)


@pytest.mark.parametrize("colored", [True, False])
def test_apply_argument_checks(mspmv, colored):
    """test_gpu_ilu0.test_solve_argument_checks on mspmv_ilu0_apply_dev, for both kinds of factor: each bad call
    returns its documented status and leaves X as it was."""
    n, L = 600, 4
    nbytes = 8 * n * L
    apply = mspmv.lib.mspmv_ilu0_apply_dev
    B = panel(n, L, 5)
    other_a = mc.csr(mc.matrix("randdd"))
    with (Solver(mspmv, "hubs") if colored else tg.Solver(mspmv, "hubs")) as s, \
            (mspmv.GpuIlu0.colored(other_a) if colored else mspmv.GpuIlu0(tg.lu_csr(mspmv, "randdd"))) as other:
        g, m = s.g, s.m
        dB = mspmv.DeviceBuffer(2 * nbytes)
        dX = mspmv.DeviceBuffer(nbytes + 16)
        try:
            dB.upload(np.concatenate([B, B]))
            calls = {
                "X is B": (INVALID, lambda: apply(g.h, m.h, dB.ptr, dB.ptr, L)),
                "X overlaps B's tail": (INVALID, lambda: apply(g.h, m.h, dB.ptr, dB.ptr + nbytes - 16, L)),
                "B overlaps X's tail": (INVALID, lambda: apply(g.h, m.h, dB.ptr + nbytes - 16, dB.ptr, L)),
                "misaligned X": (INVALID, lambda: apply(g.h, m.h, dB.ptr, dX.ptr + 8, L)),
                "misaligned B": (INVALID, lambda: apply(g.h, m.h, dB.ptr + 8, dX.ptr, L)),
                "null X": (INVALID, lambda: apply(g.h, m.h, dB.ptr, None, L)),
                "null factor": (INVALID, lambda: apply(g.h, None, dB.ptr, dX.ptr, L)),
                "L = 3": (UNSUPPORTED, lambda: apply(g.h, m.h, dB.ptr, dX.ptr, 3)),
                "factor of another size": (INVALID, lambda: apply(g.h, other.h, dB.ptr, dX.ptr, L)),
            }
            for what, (want, call) in calls.items():
                dX.fill_bytes(0x5A)
                assert call() == want, what
                assert np.all(dX.download(dX.nbytes, np.uint8) == 0x5A), what
                np.testing.assert_array_equal(dB.download((2 * n, L)), np.concatenate([B, B]), err_msg=what)
            # and the same buffers, apart and aligned, apply
            assert apply(g.h, m.h, dB.ptr, dX.ptr, L) == 0
            if colored:
                np.testing.assert_array_equal(dX.download((n, L)), mc.apply_ref("hubs", B))
        finally:
            dB.free()
            dX.free()


# ---- the solver -------------------------------------------------------------------------------------------------
def check_solve(name, B, X, it, hist, st, ref):
    assert st == 0
    tg.check_counts(it, ref)
    assert len(hist) == it
    tg.check_true_residual(mc.matrix(name), B, X)
    tg.check_history(hist, ref)


@pytest.mark.parametrize("L", [1, 2, 4, 8, 6, 16])
@pytest.mark.parametrize("name", ["convdiff30", "randdd"])
def test_against_restatement(mspmv, name, L):
    B = tb.rhs(len(mc.matrix(name)[0]) - 1, L)
    ref = mc.reference(name, L)
    with Solver(mspmv, name) as s:
        X, it, hist, st = s.solve(B)
        assert s.g.cg_kernel_name() == kernel_name(name)
        X2, it2, hist2, st2 = s.solve(B)  # the cached graph, replayed
    check_solve(name, B, X, it, hist, st, ref)
    assert st2 == 0 and it2 == it
    np.testing.assert_array_equal(X2, X)
    np.testing.assert_array_equal(hist2, hist)


@pytest.mark.parametrize("name,L", [("convdiff60", 8), ("convdiff60", 16),  # the two-level folds
                                    ("hubs", 1), ("hubs", 4),               # one-row colours, long sequential rows
                                    ("chain515", 1), ("chain515", 16)])     # colours past a workgroup's rows
def test_further_shapes(mspmv, name, L):
    B = tb.rhs(len(mc.matrix(name)[0]) - 1, L)
    with Solver(mspmv, name) as s:
        X, it, hist, st = s.solve(B)
        assert s.g.cg_kernel_name() == kernel_name(name)
    check_solve(name, B, X, it, hist, st, mc.reference(name, L))


@pytest.mark.parametrize("L", [1, 8])
def test_default_plan_offset_windows(mspmv, monkeypatch, L):
    """Without MSPMV_DIA=0 the stencil takes the offset-window plan, and the solver's two products run on it."""
    monkeypatch.delenv("MSPMV_DIA", raising=False)
    B = tb.rhs(len(mc.matrix("convdiff60")[0]) - 1, L)
    with Solver(mspmv, "convdiff60") as s:
        X, it, hist, st = s.solve(B)
        kernel = s.g.solver_product_kernel_name()
    assert kernel.startswith(f"k_spmm_dia<{L},"), kernel
    check_solve("convdiff60", B, X, it, hist, st, mc.reference("convdiff60", L))


def test_zero_rhs_column(mspmv):
    a = mc.matrix("randdd")
    B = tb.rhs(777, 4).copy()
    B[:, 2] = 0.0
    with Solver(mspmv, "randdd") as s:
        X, it, hist, st = s.solve(B)
    assert st == BREAKDOWN
    assert np.all(X[:, 2] == 0.0) and np.all(np.isfinite(X))
    tg.check_true_residual(a, B[:, [0, 1, 3]], X[:, [0, 1, 3]])


def test_natural_order_untouched(mspmv):
    """A natural-order factor's solve on the same handle returns the same bits before and after a multi-colour
    one, and so does the multi-colour one around it: the cached graphs are kept apart.  A multi-colour factor of
    another size is MSPMV_ERR_INVALID."""
    B = tb.rhs(930, 4)
    with Solver(mspmv, "convdiff30") as s, mspmv.GpuIlu0(tg.lu_csr(mspmv, "convdiff30")) as nat, \
            mspmv.GpuIlu0.colored(mc.csr(mc.matrix("randdd"))) as other:
        X0, it0, h0, st0 = mspmv.pbicgstab_ilu0(s.g, nat, B, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
        assert s.g.cg_kernel_name() == tg.NAME
        Xc, itc, hc, stc = s.solve(B)
        assert s.g.cg_kernel_name() == kernel_name("convdiff30")
        X1, it1, h1, st1 = mspmv.pbicgstab_ilu0(s.g, nat, B, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
        assert s.g.cg_kernel_name() == tg.NAME
        Xd, itd, hd, std = s.solve(B)
        with pytest.raises(mspmv.MspmvError, match="shape") as ei:
            mspmv.pbicgstab_ilu0(s.g, other, B, 10, TOL)
        assert ei.value.status == INVALID
    assert st0 == 0 and st1 == 0 and stc == 0 and std == 0
    assert it1 == it0 and itd == itc and it0 < itc  # red-black ordering weakens ILU(0)
    np.testing.assert_array_equal(X1, X0)
    np.testing.assert_array_equal(h1, h0)
    np.testing.assert_array_equal(Xd, Xc)
    np.testing.assert_array_equal(hd, hc)
