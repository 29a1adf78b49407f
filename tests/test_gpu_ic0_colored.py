"""GPU: the multi-colour IC(0) factor (mspmv_ic0_create_colored, csrc/mspmv_color.hip) -- its triangular solves alone
and its apply with the fused turn-around colour, bit for bit against the numpy restatement (ic0_color_cases.py:
test_ilu0.TriPlan on the permuted factor, rows summed in CSR order), and mspmv_dpcg_ic0_multi on such a factor
against pcg_cases.pcg_reference under pcg_cases.check_bars."""
import numpy as np
import pytest

import ic0_color_cases as cc
import pcg_cases as pc
import test_gpu_ilu0 as tg
from ic0_color_cases import MAX_ITERS, TOL

pytestmark = pytest.mark.gpu
INVALID, BREAKDOWN, UNSUPPORTED = 1, 4, 6
NATURAL_NAME = "IC0-PCG (split)"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    return gpu_available


def kernel_name(name):
    C = cc.ordering(name)[1]
    return f"MC-IC0-PCG (split, {2 * C - 1} sweeps of {C} colours)"


class Solver:
    """The matrix's handle and its multi-colour IC(0) factor on the device."""

    def __init__(self, mspmv, name):
        self.mspmv = mspmv
        self.g = mspmv.GpuCsr(cc.matrix(name), device=0)
        self.m = mspmv.GpuIc0.colored(cc.matrix(name))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.m.close()
        self.g.close()

    def solve(self, B, m=None, max_iters=MAX_ITERS):
        return self.mspmv.pcg_ic0(self.g, m or self.m, B, max_iters, TOL, hist_cap=max_iters)


def natural(mspmv, name):
    """The natural-order factor of the case on the device."""
    return mspmv.GpuIc0(mspmv.ic0_factor(cc.matrix(name))[0])


def panel(n, L, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (n, L))


# ---- the solves alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("name,L", [(name, L) for name in ("randsym777", "hubs600", "stencil5_23")
                                    for L in (1, 2, 4, 8, 16)] + [("tridiag2000", 1), ("tridiag2000", 16)])
def test_solve_is_the_restatement(mspmv, name, L, transpose):
    """One triangle of the permuted factor, in the colour ordering: TriPlan's bits, and the same on a repeat.
    hubs600: rows of L of 201 and 600 entries, the diagonal last (the split pairwise sum over the entries before
    it); stencil5_23, tridiag2000: colours past one workgroup's rows."""
    n = cc.matrix(name).num_rows
    B = panel(n, L, 6000 + 10 * L + transpose)
    want = cc.tri_plans(name)[transpose].solve(B)
    with Solver(mspmv, name) as s:
        assert s.m.num_colors == cc.ordering(name)[1]
        np.testing.assert_array_equal(s.m.perm, cc.ordering(name)[2])
        assert s.m.shift == 0.0
        X = s.m.solve(s.g, B, transpose=bool(transpose))
        X2 = s.m.solve(s.g, B, transpose=bool(transpose))
    np.testing.assert_array_equal(X, want)
    np.testing.assert_array_equal(X2, X)


# ---- the apply ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 8])
@pytest.mark.parametrize("name", cc.CASES)
def test_apply_is_the_restatement(mspmv, name, L):
    """Gather, L^-1, L^-T, scatter: the fused last colour rounds twice, as the two launches it replaces (diag300:
    that launch alone; hubs600: a one-row LONG one)."""
    n = cc.matrix(name).num_rows
    B = panel(n, L, 7000 + L)
    with Solver(mspmv, name) as s:
        Z = s.m.apply(s.g, B)
        Z2 = s.m.apply(s.g, B)
    np.testing.assert_array_equal(Z, cc.apply_ref(name, B))
    np.testing.assert_array_equal(Z2, Z)


@pytest.mark.parametrize("L", [1, 8])
@pytest.mark.parametrize("name", ["randsym777", "hubs600"])
def test_apply_on_a_natural_order_factor_is_its_two_solves(mspmv, name, L):
    n = cc.matrix(name).num_rows
    B = panel(n, L, 8000 + L)
    with mspmv.GpuCsr(cc.matrix(name), device=0) as g, natural(mspmv, name) as m:
        assert m.num_colors == 0 and m.perm is None and m.shift is None
        Z = m.apply(g, B)
        want = m.solve(g, m.solve(g, B, transpose=False), transpose=True)
    np.testing.assert_array_equal(Z, want)


@pytest.mark.parametrize("colored", [True, False])
def test_apply_argument_checks(mspmv, colored):
    """test_gpu_multicolor.test_apply_argument_checks on mspmv_ic0_apply_dev, for both kinds of factor: each bad call
    returns its documented status and leaves X as it was."""
    n, L = 600, 4
    nbytes = 8 * n * L
    apply = mspmv.lib.mspmv_ic0_apply_dev
    B = panel(n, L, 5)
    other_a = cc.matrix("randsym777")
    with mspmv.GpuCsr(cc.matrix("hubs600"), device=0) as g, \
            (mspmv.GpuIc0.colored(cc.matrix("hubs600")) if colored else natural(mspmv, "hubs600")) as m, \
            (mspmv.GpuIc0.colored(other_a) if colored else natural(mspmv, "randsym777")) as other:
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
                np.testing.assert_array_equal(dX.download((n, L)), cc.apply_ref("hubs600", B))
        finally:
            dB.free()
            dX.free()


# ---- the solver -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,L", cc.SOLVES)
def test_against_restatement(mspmv, name, L):
    B = cc.rhs(name, L)
    with Solver(mspmv, name) as s:
        out = s.solve(B)
        assert s.g.cg_kernel_name() == kernel_name(name)
        X2, it2, hist2, st2 = s.solve(B)  # the cached graph, replayed
    pc.check_bars(f"MC-IC0-PCG {name} L={L}", cc.reference(name, L), out)
    assert st2 == 0 and it2 == out[1]
    np.testing.assert_array_equal(X2, out[0])
    np.testing.assert_array_equal(hist2, out[2])


def test_red_black_costs_iterations_on_the_chain(mspmv):
    """tridiag2000: the natural-order IC(0) is the exact factor, the red-black one is not."""
    B = cc.rhs("tridiag2000", 1)
    with Solver(mspmv, "tridiag2000") as s, natural(mspmv, "tridiag2000") as nat:
        _, itc, _, stc = s.solve(B)
        _, itn, _, stn = s.solve(B, nat)
    print(f"tridiag2000: {itn} natural-order iterations, {itc} coloured")
    assert stc == 0 and stn == 0 and itn < itc


def test_zero_rhs_column(mspmv):
    B = cc.rhs("randsym777", 4).copy()
    B[:, 2] = 0.0
    with Solver(mspmv, "randsym777") as s:
        X, it, hist, st = s.solve(B)
    assert st == BREAKDOWN
    assert np.all(X[:, 2] == 0.0) and np.all(np.isfinite(X))
    tg.check_true_residual(cc.arrays("randsym777"), B[:, [0, 1, 3]], X[:, [0, 1, 3]])


# ---- untouched ----------------------------------------------------------------------------------------------------
def test_natural_order_untouched(mspmv):
    """A natural-order factor's PCG on the same handle returns the same bits before and after a multi-colour one,
    and so does the multi-colour one around it: the cached graphs are kept apart.  A multi-colour factor of another
    size is MSPMV_ERR_INVALID."""
    name = "stencil5_23"
    B = cc.rhs(name, 4)
    with Solver(mspmv, name) as s, natural(mspmv, name) as nat, mspmv.GpuIc0.colored(cc.matrix("diag300")) as other:
        X0, it0, h0, st0 = s.solve(B, nat)
        assert s.g.cg_kernel_name() == NATURAL_NAME
        Xc, itc, hc, stc = s.solve(B)
        assert s.g.cg_kernel_name() == kernel_name(name)
        X1, it1, h1, st1 = s.solve(B, nat)
        assert s.g.cg_kernel_name() == NATURAL_NAME
        Xd, itd, hd, std = s.solve(B)
        with pytest.raises(mspmv.MspmvError, match="shape") as ei:
            s.solve(B, other, max_iters=10)
        assert ei.value.status == INVALID
    assert st0 == 0 and st1 == 0 and stc == 0 and std == 0
    assert it1 == it0 and itd == itc and it0 < itc  # red-black ordering weakens IC(0)
    pc.check_bars("natural order beside it", cc.reference(name, 4, colored=False), (X0, it0, h0, st0))
    np.testing.assert_array_equal(X1, X0)
    np.testing.assert_array_equal(h1, h0)
    np.testing.assert_array_equal(Xd, Xc)
    np.testing.assert_array_equal(hd, hc)
