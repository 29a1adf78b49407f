"""IC(0)-preconditioned block CG.

Setup (IncompleteCholesky, work_2025/cg/incomplete_cholesky_decomp.hpp:84-201) runs on the host in
the reference and here.  That header includes <mkl.h>, absent from this image, so the reference
cannot be built: the factorization is checked bit for bit against the oracle's restatement
(oracle/mspmv_oracle.c orc_ic0_factor, same sequential operation order) -- **parity pinned to the
restatement only**.  Independently of any restatement, L L^T = A + shift I is checked on L's
pattern to the recurrence's rounding bound, on the stencils and on the irregular matrices of
ic0_cases.py, and inputs the recurrence cannot factor must be refused.  The solve (PCGSolveMultiple, work_2025/main/incomplete_cholesky.hpp:33-199)
runs on the GPU with sync-free triangular solves; it is compared with the oracle's restatement
(orc_pcg_ic0_multi) under the CG tolerances of test_gpu_cg.py.
"""
import numpy as np
import pytest

import ic0_cases
import mspmv

INVALID = 1  # MSPMV_ERR_INVALID


def spd_small():
    return {
        "fem2d": lambda: mspmv.CsrMatrix.synth_stencil(0, 900, 30),
        "stencil27": lambda: mspmv.CsrMatrix.synth_stencil(1, 8 * 9 * 10, 8, 9, 10),
        "fem2d_partial_row": lambda: mspmv.CsrMatrix.synth_stencil(0, 1003, 41),
    }


def factor_cases():
    """The stencils and the irregular matrices of ic0_cases (random rows, hub rows, a chain)."""
    return {**spd_small(), **{name: (lambda name=name: ic0_cases.matrix(name)) for name in ic0_cases.SMALL}}


@pytest.mark.parametrize("name", list(factor_cases()))
def test_ic0_factor_bitexact_with_oracle(orc, name):
    a = factor_cases()[name]()
    l, shift = mspmv.ic0_factor(a)
    lro, lci, lva, sh = orc.ic0_factor(a)
    assert shift == sh
    np.testing.assert_array_equal(l.row_offsets, lro)
    np.testing.assert_array_equal(l.column_indices, lci)
    np.testing.assert_array_equal(l.values, lva)


def test_ic0_factor_shift_retries(orc):
    """[[1, 2], [2, 1]] is indefinite: pivots fail until the diagonal shift (1e-3, 1e-2, 0.1,
    1, ... -- incomplete_cholesky_decomp.hpp:150-225) makes them positive; the product and the
    oracle agree on the shift and on every value."""
    a = mspmv.CsrMatrix.from_arrays(2, [0, 2, 4], [0, 1, 0, 1], [1.0, 2.0, 2.0, 1.0])
    l, shift = mspmv.ic0_factor(a)
    lro, lci, lva, sh = orc.ic0_factor(a)
    assert shift == sh and shift >= 0.1
    np.testing.assert_array_equal(l.values, lva)
    r = mspmv.CsrMatrix.from_arrays(3, [0, 1], [2], [1.0])
    with pytest.raises(mspmv.MspmvError):
        mspmv.ic0_factor(r)


@pytest.mark.parametrize("name", list(factor_cases()) + ["shift_retry_2x2"])
def test_ic0_factor_identity(name):
    """L L^T = A + shift I on L's pattern -- IC(0)'s definition, checked against nothing but A:
    |(L L^T)_ij - A_ij - shift d_ij| <= 2 (len_i + 2) 2^-53 (|L||L|^T)_ij for every (i, j) of the
    pattern, both sides in long double (ic0_cases.factor_identity_ratio).  The oracle restates the
    same recurrence and shares its assumptions; this does not."""
    if name == "shift_retry_2x2":
        a = mspmv.CsrMatrix.from_arrays(2, [0, 2, 4], [0, 1, 0, 1], [1.0, 2.0, 2.0, 1.0])
    else:
        a = factor_cases()[name]()
    l, shift = mspmv.ic0_factor(a)
    if name in ic0_cases.SMALL:
        assert shift == 0.0  # strictly diagonally dominant: IC(0) exists unshifted
    if name == "shift_retry_2x2":
        assert shift >= 0.1
    ratio = ic0_cases.factor_identity_ratio(a, l, shift)
    print(f"{name}: worst |L L^T - A - shift I| / bound = {ratio:.3f}")
    assert ratio <= 1.0


def test_ic0_cases_are_what_they_claim():
    """The irregular matrices exercise what the stencils cannot: a row of L as long as the matrix,
    a chain of one row per level, irregular levels."""
    shape = {}
    for name in ic0_cases.SMALL:
        l, _, u = ic0_cases.factor(name)
        shape[name] = (int(np.diff(l.row_offsets).max()), ic0_cases.lower_levels(l))
        for t in (l, u):  # both triangles: ascending columns, the diagonal at the row's end / start
            rows = ic0_cases.rows_of(t)
            same_row = rows[1:] == rows[:-1]
            assert np.all(np.diff(t.column_indices.astype(np.int64))[same_row] > 0)
        assert np.array_equal(l.column_indices[l.row_offsets[1:] - 1], np.arange(l.num_rows))
        assert np.array_equal(u.column_indices[u.row_offsets[:-1]], np.arange(l.num_rows))
    assert shape["hubs600"][0] == 600 and shape["tridiag2000"] == (2, 2000)
    assert shape["randsym777"][0] > 8 and 8 < shape["randsym777"][1] < 100


# The row each defect goes into: rows on which the unchecked recurrence returned MSPMV_OK (without its
# diagonal, row 396 "factored" with a shift of 10; on other rows it happened to end in BREAKDOWN).
BROKEN_ROW = {"reversed": 400, "duplicate": 400, "no_diagonal": 396}


def _randsym_broken(kind):
    """randsym777 with one defect in the lower part (columns <= row) of row BROKEN_ROW[kind]."""
    a = ic0_cases.matrix("randsym777")
    ro, ci, va = a.row_offsets.copy(), a.column_indices.copy(), a.values.copy()
    r = BROKEN_ROW[kind]
    s = int(ro[r])
    nlow = int(np.sum(ci[s:ro[r + 1]] <= r))
    assert nlow >= 3 and ci[s + nlow - 1] == r
    if kind == "reversed":
        ci[s:s + nlow] = ci[s:s + nlow][::-1].copy()
        va[s:s + nlow] = va[s:s + nlow][::-1].copy()
    elif kind == "duplicate":  # the first lower entry twice
        ci, va = np.insert(ci, s, ci[s]), np.insert(va, s, va[s])
        ro[r + 1:] += 1
    elif kind == "no_diagonal":
        ci, va = np.delete(ci, s + nlow - 1), np.delete(va, s + nlow - 1)
        ro[r + 1:] -= 1
    return mspmv.CsrMatrix.from_arrays(a.num_cols, ro, ci, va)


@pytest.mark.parametrize("kind", ["reversed", "duplicate", "no_diagonal", "descending_3x3"])
def test_ic0_factor_rejects_what_it_cannot_factor(kind):
    """The recurrence merges rows in ascending column order and takes a row's last lower entry as its
    diagonal: unsorted or duplicate columns or a missing diagonal used to factor to garbage with
    MSPMV_OK (descending [[4,1,0],[1,4,1],[0,1,4]] gave L(1,1) = L(2,1) = 2 for 1.9365, 0.5164)."""
    if kind == "descending_3x3":
        a = mspmv.CsrMatrix.from_arrays(3, [0, 2, 5, 7], [1, 0, 2, 1, 0, 2, 1], [1.0, 4.0, 1.0, 4.0, 1.0, 4.0, 1.0])
        row = 1
    else:
        a, row = _randsym_broken(kind), BROKEN_ROW[kind]
    with pytest.raises(mspmv.MspmvError, match=f"row {row}\\b") as e:
        mspmv.ic0_factor(a)
    assert e.value.status == INVALID


@pytest.mark.parametrize("kind", ["above_diagonal", "no_diagonal", "non_square", "column_out_of_range"])
def test_ic0_create_rejects_before_touching_the_device(kind):
    """mspmv_ic0_create validates on the host first (an entry above the diagonal or a missing diagonal
    would make a solve wait forever): MSPMV_ERR_INVALID with or without a device."""
    ro, ci, va = [0, 1, 3, 5], [0, 0, 1, 1, 2], [2.0, 1.0, 2.0, 1.0, 2.0]
    ncols, what = 3, None
    if kind == "above_diagonal":
        ro, ci, va = [0, 2, 4, 6], [0, 2, 0, 1, 1, 2], [2.0, 1.0, 1.0, 2.0, 1.0, 2.0]
        what = "above the diagonal in row 0"
    elif kind == "no_diagonal":
        ro, ci, va = [0, 1, 2, 4], [0, 0, 1, 2], [2.0, 1.0, 1.0, 2.0]
        what = "row 1 has no diagonal"
    elif kind == "non_square":
        ncols, what = 4, "square"
    elif kind == "column_out_of_range":
        ci = [0, 0, 1, -1, 2]
        what = "column index out of range"
    with pytest.raises(mspmv.MspmvError, match=what) as e:
        mspmv.GpuIc0(mspmv.CsrMatrix.from_arrays(ncols, ro, ci, va))
    assert e.value.status == INVALID


def test_oracle_pcg_ic0_beats_cg(orc):
    a = spd_small()["fem2d"]()
    lro, lci, lva, _ = orc.ic0_factor(a)
    B = np.random.default_rng(3).uniform(0, 1, (a.num_rows, 2))
    _, itp, hp = orc.pcg_ic0_multi(a, lro, lci, lva, B, 1000, 1e-10, hist_cap=1000)
    _, itc, _ = orc.cg_multi(a, B, 1000, 1e-10, hist_cap=1000)
    assert hp[-1] < 1e-10 and itp < itc


def _iter_match(it_g, it_o, hist_o, tol):
    if it_g == it_o:
        return True
    if abs(it_g - it_o) == 1 and len(hist_o):
        k = min(it_g, it_o) - 1
        return abs(hist_o[k] - tol) <= 1e-9 * tol
    return False


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(spd_small()))
@pytest.mark.parametrize("L", [1, 2, 4, 8, 32])
def test_gpu_pcg_ic0_vs_oracle(gpu_available, orc, name, L):
    a = spd_small()[name]()
    l, _ = mspmv.ic0_factor(a)
    B = np.random.default_rng(11 + L).uniform(0, 1, (a.num_rows, L))
    tol = 1e-9
    Xo, it_o, ho = orc.pcg_ic0_multi(a, l.row_offsets, l.column_indices, l.values, B, 2000, tol, hist_cap=2000)
    with mspmv.GpuCsr(a) as ga, mspmv.GpuIc0(l) as ic:
        X, it, h, st = mspmv.pcg_ic0(ga, ic, B, 2000, tol, hist_cap=2000)
        X2, it2, h2, _ = mspmv.pcg_ic0(ga, ic, B, 2000, tol, hist_cap=2000)
    assert st == 0 and _iter_match(it, it_o, ho, tol)
    k = min(len(h), len(ho))
    np.testing.assert_allclose(h[:k], ho[:k], rtol=0, atol=1e-10)
    assert np.linalg.norm(X - Xo) <= 1e-8 * np.linalg.norm(Xo)
    # the sync-free solves fold each row in a fixed order: a repeat is bitwise identical
    assert it2 == it
    np.testing.assert_array_equal(X2, X)
    np.testing.assert_array_equal(h2, h)


@pytest.mark.gpu
def test_gpu_ic0_facade_names(gpu_available, orc):
    a = spd_small()["stencil27"]()
    l = mspmv.IncompleteCholesky(a)
    L = 8
    B = np.random.default_rng(12).uniform(0, 1, a.num_rows * L)
    X = np.zeros_like(B)
    errs = []
    it = mspmv.PCGSolveMultiple(a, l, None, B, X, L, 1000, 1e-8, mspmv.MERGE, errs)
    _, it_o, _ = orc.pcg_ic0_multi(a, l.row_offsets, l.column_indices, l.values, B.reshape(-1, L), 1000, 1e-8)
    assert abs(it - it_o) <= 1 and len(errs) == it and errs[-1] < 1e-8
