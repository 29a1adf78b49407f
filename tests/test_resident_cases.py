"""The inputs of test_gpu_cg_resident_shapes.py, pinned without a GPU: every matrix of
resident_cases.py is symmetric, strictly diagonally dominant with ascending columns and a row of
exactly its maxlen entries, and resident_build's choice -- restated in numpy by predict_shape -- is,
with one row block per CU of a 256-CU device, the (rows per thread, slots per row) shape the case is
meant to reach.  (resident_build itself reads the CU count from the device and is not callable on
the host, so the restatement is held to the library by the GPU module: the shape in the launched
kernel's name must equal predict_shape's.)
"""
import numpy as np
import pytest

import resident_cases as rc

G = 256  # CUs of an MI355X: one row block each


def dense_rows(a):
    return np.repeat(np.arange(a.num_rows), np.diff(a.row_offsets.astype(np.int64)))


@pytest.mark.parametrize("name", list(rc.CASES) + rc.TINY)
def test_case_is_symmetric_dominant_sorted(name):
    a = rc.matrix(name)
    m = a.num_rows
    assert a.num_cols == m and a.row_offsets[0] == 0 and a.row_offsets[-1] == a.num_nonzeros == len(a.values)
    rows, cols = dense_rows(a), a.column_indices.astype(np.int64)
    assert cols.min() >= 0 and cols.max() < m
    # columns strictly ascending within every row: (row, column) keys strictly ascending overall
    key = rows * m + cols
    assert np.all(np.diff(key) > 0)
    # A == A^T exactly: the transposed entries, sorted, are the same keys with the same values
    order = np.argsort(cols * m + rows, kind="stable")
    assert np.array_equal((cols * m + rows)[order], key)
    assert np.array_equal(a.values[order], a.values)
    # strict diagonal dominance, every diagonal present and positive
    on = rows == cols
    assert on.sum() == m
    diag = a.values[on]
    off = np.bincount(rows[~on], np.abs(a.values[~on]), m)
    assert np.all(diag > off) and np.all(diag > 0)
    # rows of at most maxlen entries, one of exactly maxlen
    assert np.diff(a.row_offsets).max() == rc.maxlen_of(name)
    assert np.diff(a.row_offsets).min() >= 1


def test_mixed_cases_have_unequal_rows_and_scattered_columns():
    """What the stencils lack: rows of different lengths, columns far from the row, unequal blocks."""
    for name in rc.CASES:
        a = rc.matrix(name)
        lens = np.diff(a.row_offsets)
        assert lens.min() < lens.max()
        far = np.abs(a.column_indices.astype(np.int64) - dense_rows(a))
        assert far.max() > a.num_rows // 2
        if rc.CASES[name][0]:  # a diagonal-only run: its blocks hold about twice the rows of the others
            rows = np.diff(rc.row_blocks(a, G))
            assert rows.max() > 1.8 * np.median(rows)


@pytest.mark.parametrize("name", list(rc.CASES))
def test_predicted_shape_is_the_table(name):
    shape, empty = rc.predict_shape(rc.matrix(name), G)
    assert shape == rc.CASES[name][4]
    assert empty == 0
    if shape is not None and shape[0] > 1:
        # the threshold is cleared with room: another seed's draw does not flip the shape
        rows = np.diff(rc.row_blocks(rc.matrix(name), G))
        assert rows.max() >= 1.05 * (shape[0] - 1) * rc.ROWS_PER_BLOCK
        assert rows.max() <= shape[0] * rc.ROWS_PER_BLOCK


def test_every_instantiated_shape_has_a_case():
    assert sorted({rc.CASES[k][4] for k in rc.ACCEPTED}) == sorted(rc.SHAPES)
    assert len(rc.ACCEPTED) == 10 and len(rc.DECLINED) == 3


@pytest.mark.parametrize("name", rc.TINY)
def test_tiny_cases_select_1x4_and_leave_blocks_empty(name):
    a = rc.matrix(name)
    shape, empty = rc.predict_shape(a, G)
    assert shape == (1, 4)
    if a.num_rows < G:
        assert empty >= G - a.num_rows >= 1
    rb = rc.row_blocks(a, G)
    assert rb[0] == 0 and rb[-1] == a.num_rows and np.all(np.diff(rb) >= 0)


def test_row_blocks_is_the_search_resident_build_runs():
    """row_blocks (searchsorted) against the definition spelled out row by row: block j starts at the
    last row i with i + row_offsets[i] <= (m + nnz) j // G."""
    for name, g in (("m65", 256), ("m1025", 256), ("s14", 256), ("s14", 304), ("two", 256), ("m257", 7)):
        a = rc.matrix(name)
        m, nnz, ro = a.num_rows, a.num_nonzeros, a.row_offsets
        want = []
        for j in range(g + 1):
            d = (m + nnz) * j // g
            want.append(max(i for i in range(m + 1) if i + int(ro[i]) <= d))
        want[g] = m
        assert np.array_equal(rc.row_blocks(a, g), want)


def test_each_bar_bites(orc):
    """check_bars passes the oracle's own solve and fails when any one figure is off by a little more
    than its bar; resident_shape fails on every name that is not the resident kernel of that form."""
    a = rc.matrix("s18")
    ref = rc.reference(orc, "s18")
    b, xo, it, ho, res = ref
    rc.check_bars(orc, "s18 oracle", a, ref, xo, it, ho, 0)
    bump = np.zeros_like(ho)
    bump[it // 2] = 2e-10
    one_row = np.zeros_like(xo)
    one_row[7] = 2e-8 * np.max(np.abs(xo))
    wrong = {  # the bar's message: a solve off by a little more than that bar
        "status 4": (xo, it, ho, 4),
        "iterations": (xo, it - 2, ho[:it - 2], 0),
        "history length": (xo, it, ho[:it - 1], 0),
        "history deviation": (xo, it, ho + bump, 0),
        "x error 2": (xo * (1 + 2e-8), it, ho, 0),
        "x error in the maximum norm": (xo + one_row, it, ho, 0),
        "true residual": (xo + 5e-10 * np.sign(xo - xo.mean()), it, ho, 0),
    }
    for what, (x, i, h, st) in wrong.items():
        with pytest.raises(AssertionError, match="^" + what):
            rc.check_bars(orc, f"s18 with a wrong {what}", a, ref, x, i, h, st)
    assert rc.resident_shape("k_cg_resident<2,8,classic> x 256", "classic") == (2, 8, 256)
    for kname, form in (("pipelined (k_spmv_tile MODE 1 + k_cg1_update)", "classic"),
                        ("pipelined (k_spmv_tile MODE 1 + k_cg1_update) after a resident-CG stall", "classic"),
                        ("k_cg_resident<2,8,classic> x 256", "single_reduction"),
                        ("k_cg_resident<2,8> x 256", "classic")):
        with pytest.raises(AssertionError):
            rc.resident_shape(kname, form)


def test_bars_tell_a_perturbed_matrix_apart(orc):
    """s28 with one off-diagonal pair of its 73,000 rows changed by 1e-6, both solved by the oracle:
    the history moves by 4e-12 and x by 1.3e-9 in the 2-norm -- inside the 1e-10 and 1e-8 bars, which
    weigh a change in two rows by 1 / sqrt(m) -- and x by 5e-8 in the maximum norm, which the
    maximum-norm bar of check_bars refuses."""
    a = rc.matrix("s28")
    ref = rc.reference(orc, "s28")
    b, xo, it, ho, res = ref
    pert = rc.perturbed_reference(orc, "s28")
    rc.check_bars(orc, "s28 oracle", a, ref, xo, it, ho, 0)
    with pytest.raises(AssertionError, match="^x error in the maximum norm"):
        rc.check_bars(orc, "s28 oracle against the perturbed matrix's solve", a, pert, xo, it, ho, 0)
    _, xp, itp, hp, _ = pert
    assert itp == it
    assert np.max(np.abs(hp - ho)) < 1e-10 and np.linalg.norm(xp - xo) < 1e-8 * np.linalg.norm(xo)
    assert np.max(np.abs(xp - xo)) > 3e-8 * np.max(np.abs(xo))


def test_reference_inputs_are_shared_and_read_only():
    a = rc.matrix("s14")
    assert rc.matrix("s14") is a
    with pytest.raises(ValueError):
        a.values[0] = 0.0
    b = rc.rhs(a.num_rows)
    assert np.array_equal(b, np.random.default_rng(1).uniform(0, 1, a.num_rows))
