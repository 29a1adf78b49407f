"""The IC(0) triangular solves on their own (mspmv_ic0_solve_dev: the pass tri_apply runs twice per
preconditioner application), on factors no stencil gives -- tests/ic0_cases.py: random rows, hub rows
as long as the matrix, a 2,000-deep chain, a grid of more waves than the device holds at once.

Each solve is checked against the definition, not against another solver: the componentwise
backward-error bound of substitution, |B - T X|_ic <= 2 (len_i + 2) 2^-53 (|T||X|)_ic, which holds
whatever order a row's products are summed in (the kernel folds them in a tree), with residual and
bound formed in long double.  A float64 simulation of the kernel's fold order stays near 0.2 of the
bound, and one x value off by a relative 1e-13 already misses it.
"""
import numpy as np
import pytest

import ic0_cases
import mspmv
from test_ic0 import _iter_match

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 6


def _solve(g, ic, B, transpose):
    """(status, X) of one mspmv_ic0_solve_dev on host panels; X starts as zero bytes."""
    B = np.ascontiguousarray(B, np.float64)
    dB = mspmv.DeviceBuffer.from_array(B)
    dX = mspmv.DeviceBuffer(B.nbytes)
    try:
        dX.fill_bytes(0)
        st = mspmv.lib.mspmv_ic0_solve_dev(g.h, ic.h, transpose, dB.ptr, dX.ptr, B.shape[1])
        return st, dX.download(B.shape)
    finally:
        dB.free()
        dX.free()


def _check_solve(name, g, ic, B, transpose):
    l, _, u = ic0_cases.factor(name)
    st, X = _solve(g, ic, B, transpose)
    assert st == 0, mspmv.lib.mspmv_last_error().decode()
    assert np.all(np.isfinite(X))
    ratio = ic0_cases.solve_residual_ratio(u if transpose else l, X, B)
    print(f"{name} L={B.shape[1]} transpose={transpose}: worst |B - T X| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    return X


@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("L", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("name", list(ic0_cases.SMALL))
def test_gpu_ic0_solve_residual(gpu_available, name, L, transpose):
    a = ic0_cases.matrix(name)
    B = np.random.default_rng(1000 + 10 * L + transpose).uniform(-1, 1, (a.num_rows, L))
    with mspmv.GpuCsr(a) as g, mspmv.GpuIc0(ic0_cases.factor(name)[0]) as ic:
        X = _check_solve(name, g, ic, B, transpose)
        np.testing.assert_array_equal(ic.solve(g, B, transpose=bool(transpose)), X)  # fixed fold order


@pytest.mark.parametrize("transpose", [0, 1])
def test_gpu_ic0_solve_columns_independent(gpu_available, transpose):
    """A NaN and an inf in two columns of B stay in those columns: a NaN is not the pending pattern,
    so nothing stalls, and every other column is bit-identical to the clean solve."""
    name, L = "hubs600", 8
    a = ic0_cases.matrix(name)
    n = a.num_rows
    B = np.random.default_rng(77).uniform(-1, 1, (n, L))
    Bd = B.copy()
    Bd[0, 2] = np.nan
    Bd[n - 1, 5] = np.inf
    with mspmv.GpuCsr(a) as g, mspmv.GpuIc0(ic0_cases.factor(name)[0]) as ic:
        st, X = _solve(g, ic, B, transpose)
        std, Xd = _solve(g, ic, Bd, transpose)
    assert st == 0 and std == 0
    clean = [c for c in range(L) if c not in (2, 5)]
    np.testing.assert_array_equal(Xd[:, clean].view(np.uint64), X[:, clean].view(np.uint64))
    assert np.isnan(Xd[0, 2]) and not np.isfinite(Xd[n - 1, 5])


@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("L", [1, 16])
def test_gpu_ic0_solve_grid_larger_than_device(gpu_available, L, transpose):
    """22,500 waves, 8,192 resident at once (2,048 on 64 CUs): a wave may wait on a row whose wave is
    resident or finished only because waves are dispatched in level order."""
    name = "fem150"
    a = ic0_cases.matrix(name)
    B = np.random.default_rng(150 + L + transpose).uniform(-1, 1, (a.num_rows, L))
    with mspmv.GpuCsr(a) as g, mspmv.GpuIc0(ic0_cases.factor(name)[0]) as ic:
        X = _check_solve(name, g, ic, B, transpose)
        g.set_cu_limit(64)
        st, X64 = _solve(g, ic, B, transpose)
    assert st == 0, mspmv.lib.mspmv_last_error().decode()
    np.testing.assert_array_equal(X64, X)


def test_gpu_ic0_solve_argument_checks(gpu_available):
    """Each bad call returns its documented status and leaves X as it was."""
    a = ic0_cases.matrix("hubs600")
    n, L = a.num_rows, 4
    nbytes = 8 * n * L
    solve = mspmv.lib.mspmv_ic0_solve_dev
    B = np.random.default_rng(5).uniform(-1, 1, (n, L))
    with mspmv.GpuCsr(a) as g, mspmv.GpuIc0(ic0_cases.factor("hubs600")[0]) as ic, \
            mspmv.GpuIc0(ic0_cases.factor("tridiag2000")[0]) as other:
        dB = mspmv.DeviceBuffer(2 * nbytes)
        dX = mspmv.DeviceBuffer(nbytes + 16)
        try:
            dB.upload(np.concatenate([B, B]))
            calls = {
                "X is B": (INVALID, lambda: solve(g.h, ic.h, 0, dB.ptr, dB.ptr, L)),
                "X overlaps B's tail": (INVALID, lambda: solve(g.h, ic.h, 0, dB.ptr, dB.ptr + nbytes - 16, L)),
                "B overlaps X's tail": (INVALID, lambda: solve(g.h, ic.h, 1, dB.ptr + nbytes - 16, dB.ptr, L)),
                "misaligned X": (INVALID, lambda: solve(g.h, ic.h, 0, dB.ptr, dX.ptr + 8, L)),
                "misaligned B": (INVALID, lambda: solve(g.h, ic.h, 0, dB.ptr + 8, dX.ptr, L)),
                "null X": (INVALID, lambda: solve(g.h, ic.h, 0, dB.ptr, None, L)),
                "L = 3": (UNSUPPORTED, lambda: solve(g.h, ic.h, 0, dB.ptr, dX.ptr, 3)),
                "factor of another size": (INVALID, lambda: solve(g.h, other.h, 0, dB.ptr, dX.ptr, L)),
            }
            for what, (want, call) in calls.items():
                dX.fill_bytes(0x5A)
                assert call() == want, what
                assert np.all(dX.download(dX.nbytes, np.uint8) == 0x5A), what
                np.testing.assert_array_equal(dB.download((2 * n, L)), np.concatenate([B, B]), err_msg=what)
            # and the same buffers, apart and aligned, solve
            assert solve(g.h, ic.h, 0, dB.ptr, dX.ptr, L) == 0
            X = dX.download((n, L))
            assert ic0_cases.solve_residual_ratio(ic0_cases.factor("hubs600")[0], X, B) <= 1.0
        finally:
            dB.free()
            dX.free()


@pytest.mark.parametrize("L", [1, 16])
@pytest.mark.parametrize("name", ["randsym777", "hubs600"])
def test_gpu_pcg_ic0_irregular_vs_oracle(gpu_available, orc, name, L):
    """The whole PCG on the irregular factors: what test_ic0.test_gpu_pcg_ic0_vs_oracle asserts on the
    stencils, bars unchanged."""
    a = ic0_cases.matrix(name)
    l = ic0_cases.factor(name)[0]
    B = np.random.default_rng(11 + L).uniform(0, 1, (a.num_rows, L))
    tol = 1e-9
    Xo, it_o, ho = orc.pcg_ic0_multi(a, l.row_offsets, l.column_indices, l.values, B, 2000, tol, hist_cap=2000)
    with mspmv.GpuCsr(a) as ga, mspmv.GpuIc0(l) as ic:
        X, it, h, st = mspmv.pcg_ic0(ga, ic, B, 2000, tol, hist_cap=2000)
        X2, it2, h2, _ = mspmv.pcg_ic0(ga, ic, B, 2000, tol, hist_cap=2000)
    print(f"{name} L={L}: {it} iterations (oracle {it_o})")
    assert st == 0 and _iter_match(it, it_o, ho, tol)
    k = min(len(h), len(ho))
    np.testing.assert_allclose(h[:k], ho[:k], rtol=0, atol=1e-10)
    assert np.linalg.norm(X - Xo) <= 1e-8 * np.linalg.norm(Xo)
    assert it2 == it
    np.testing.assert_array_equal(X2, X)
    np.testing.assert_array_equal(h2, h)
