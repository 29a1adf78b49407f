"""Multi-colour IC(0) on the CPU: the restated ordering against mspmv_color_greedy and mspmv_csr_permute_sym, the
property the ordering exists for -- the permuted factor has at most as many dependency levels as colours -- the
factor identity of the permuted factor, the inputs mspmv_ic0_create_colored must refuse before it touches a device,
and the restatement itself held to the bars the GPU is held to (test_gpu_ic0_colored.py): a float64 run of the
recurrence against the np.longdouble one, on every (case, width) the GPU file solves."""
import ctypes

import numpy as np
import pytest

import ic0_cases
import ic0_color_cases as cc
import mspmv
import pcg_cases as pc
import test_bicgstab as tb

INVALID = 1


# ---- the ordering ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.CASES)
def test_ordering_is_the_library_s(name):
    a = cc.matrix(name)
    colors_ref, num_ref, perm, ap, _, shift, _ = cc.ordering(name)
    colors, num = mspmv.color_greedy(a)
    rows = np.bincount(colors).tolist()
    print(f"{name}: {num} colours, rows per colour {rows}, shift {shift}")
    assert num == num_ref
    np.testing.assert_array_equal(colors, colors_ref)
    if name in cc.COLOUR_ROWS:
        assert rows == cc.COLOUR_ROWS[name]
    else:  # hubs600: the two hub rows, and one row more, alone in their colours; the last colour is one of them
        assert num == 7 and rows.count(1) == 3 and rows[-1] == 1
        assert rows[colors[200]] == 1 and rows[colors[599]] == 1
    p = mspmv.csr_permute_sym(a, perm)
    np.testing.assert_array_equal(p.row_offsets, ap.row_offsets)
    np.testing.assert_array_equal(p.column_indices, ap.column_indices)
    np.testing.assert_array_equal(p.values, ap.values)
    assert shift == 0.0  # an H-matrix (or a diagonal one): IC(0) exists in any ordering


@pytest.mark.parametrize("name", cc.CASES)
def test_permuted_factor_levels_and_identity(name):
    _, num, _, ap, l, shift, lt = cc.ordering(name)
    lev = ic0_cases.lower_levels(l)
    ratio = ic0_cases.factor_identity_ratio(ap, l, shift)
    natural = ic0_cases.lower_levels(mspmv.ic0_factor(cc.matrix(name))[0])
    longest = int(np.diff(l.row_offsets).max())
    print(f"{name}: {num} colours, {lev} levels (natural order {natural}), longest row of L {longest} entries, "
          f"factor identity ratio {ratio:.3f}")
    assert lev <= num
    assert ratio <= 1.0
    # L ends every row in its diagonal, L^T starts every row with it: what the sweeps take for granted
    n = l.num_rows
    np.testing.assert_array_equal(l.column_indices[l.row_offsets[1:] - 1], np.arange(n))
    np.testing.assert_array_equal(lt.column_indices[lt.row_offsets[:-1]], np.arange(n))
    np.testing.assert_array_equal(lt.values[lt.row_offsets[:-1]], l.values[l.row_offsets[1:] - 1])
    # the last colour's rows of L^T hold the diagonal alone: the fused launch's premise
    last = np.arange(n)[np.sort(cc.ordering(name)[0], kind="stable") == num - 1]
    assert np.all(np.diff(lt.row_offsets)[last] == 1)
    if name == "hubs600":  # rows past 129 entries, the last colour's row among them
        assert longest > 129 and np.diff(l.row_offsets)[last].max() > 129


# ---- rejections, no device needed ----------------------------------------------------------------------------
def _colored(a, colors):
    return mspmv.GpuIc0.colored(a, None if colors is None else np.asarray(colors, np.int32))


def test_create_colored_rejects_bad_colours():
    a = cc.matrix("tridiag2000")
    n = 2000
    good = np.arange(n) % 2
    who = "ic0_create_colored: "
    cases = {"adjacent equal": (np.where(np.arange(n) == 41, 0, good), who + "row 40 shares colour 0"),  # 40, 41, 42
             "negative": (np.where(np.arange(n) == 77, -1, good), who + "row 77: colour -1 is outside"),
             "not below n": (np.where(np.arange(n) == 78, n, good), who + "row 78: colour 2000 is outside"),
             "gap": (np.where(good == 1, 2, good), who + "row 1: colour 2 is in use but colour 1 is not")}
    for what, (colors, msg) in cases.items():
        with pytest.raises(mspmv.MspmvError, match=msg) as e:
            _colored(a, colors)
        assert e.value.status == INVALID, what


def test_create_colored_rejects_non_square():
    a = mspmv.CsrMatrix.from_arrays(3, [0, 1, 2], [0, 1], [1.0, 1.0])
    for colors in (None, [0, 0]):
        with pytest.raises(mspmv.MspmvError, match="square") as e:
            _colored(a, colors)
        assert e.value.status == INVALID


def test_create_colored_rejects_a_row_without_its_diagonal():
    """Row 1 of [[2, 1, 0], [1, 0, 1], [0, 1, 2]] holds no diagonal: rows 0 and 2 take colour 0, row 1 colour 1, so
    it is row 2 of the colour ordering that mspmv_ic0_factor refuses."""
    a = mspmv.CsrMatrix.from_arrays(3, [0, 2, 4, 6], [0, 1, 0, 2, 1, 2], [2.0, 1.0, 1.0, 1.0, 1.0, 2.0])
    for colors in (None, [0, 1, 0]):
        with pytest.raises(mspmv.MspmvError, match=r"row 2 has no diagonal entry.*colour ordering") as e:
            _colored(a, colors)
        assert e.value.status == INVALID


def test_create_colored_rejects_a_column_out_of_range():
    a = mspmv.CsrMatrix.from_arrays(3, [0, 1, 3, 5], [0, 0, 1, 3, 2], [2.0, 1.0, 2.0, 1.0, 2.0])
    with pytest.raises(mspmv.MspmvError, match="column index out of range") as e:
        _colored(a, None)
    assert e.value.status == INVALID


def test_abi_symbols():
    lib = ctypes.CDLL(tb.LIB)
    for name in ("mspmv_ic0_create_colored", "mspmv_ic0_colors", "mspmv_ic0_apply_dev"):
        assert hasattr(lib, name), name
    for attr in ("colored", "num_colors", "perm", "apply", "apply_dev", "solve"):
        assert hasattr(mspmv.GpuIc0, attr), attr


# ---- the restatement alone, under the GPU's bars -------------------------------------------------------------
@pytest.mark.parametrize("name,L", cc.SOLVES)
def test_float64_restatement_stays_inside_the_bars(name, L):
    ref = cc.reference(name, L)
    out = cc.pcg_float64(name, L)
    pc.check_bars(f"{name} L={L} float64 against longdouble", ref, out)
    gap = np.min(np.abs(ref[2] - cc.TOL)) / cc.TOL
    print(f"  the residual nearest the tolerance lies {gap:.2e} of it away")
    tr = tb.true_residual(cc.arrays(name), cc.rhs(name, L), ref[0])
    assert np.all(tr <= 2 * cc.TOL), tr.max()


def test_red_black_costs_iterations():
    """tridiag2000: the natural-order IC(0) is the exact factor (1 iteration), the red-black one is not; the stencil
    loses too."""
    counts = {name: (cc.reference(name, 1)[1], cc.reference(name, 1, colored=False)[1])
              for name in ("tridiag2000", "stencil5_23")}
    print(counts)
    assert counts["tridiag2000"][1] == 1 and counts["tridiag2000"][0] > 1
    assert counts["stencil5_23"][1] < counts["stencil5_23"][0]
