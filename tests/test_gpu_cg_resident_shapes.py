"""The register-resident CG (csrc/mspmv_cg_resident.hip) on every instantiated (rows per thread, slots
per row) shape, in both iteration forms, on matrices that are not stencils (resident_cases.py: rows
of unequal length, columns scattered over the whole matrix, row blocks of unequal size, and -- with
fewer rows than CUs -- row blocks with no rows at all), and the two-kernel pipelined CG
(k_spmv_tile MODE 1 + k_cg1_update) on the same matrices and on those no shape fits.

Reference: the oracle's fp64 restatement of CGSolveSingle (orc.cg_single: rows summed in CSR order,
dot products as OpenMP reductions, so its last bits depend on the thread count), SpmvGold for true
residuals.  Bars (resident_cases.check_bars) as test_gpu_cg.py and test_gpu_cg_resident.py:
status 0, iteration counts equal (iter_match), every recorded ||r_k||/||b|| within 1e-10 of the
oracle's, x within 1e-8 relative, true residual <= max(10 x the oracle's, 1e-13); and x within 1e-8
in the maximum norm as well, which is what notices one slightly wrong value among 73,000 rows
(test_bars_tell_a_perturbed_matrix_apart).  On these inputs (21-42 iterations, diagonally dominant)
another summation order of the dot products moves the history by about 1e-14, so the 1e-10 bar is
not consumed by rounding.

The shape in the launched kernel's name must be the one resident_cases.predict_shape restates from
resident_build, and on a 256-CU device the one the case was built to reach: a shape that is wrong,
declined by the occupancy query or stalled fails by name, not silently on the two-kernel path.
Each test prints its worst history deviation, x error and true-residual ratio (pytest -s).
"""
import numpy as np
import pytest

import mspmv
import resident_cases as rc
from test_gpu_cg_resident import FORMS, solve

pytestmark = pytest.mark.gpu

TOL, MAX_ITERS = rc.TOL, rc.MAX_ITERS
TWO_KERNEL = "pipelined (k_spmv_tile MODE 1"
check_bars, resident_shape = rc.check_bars, rc.resident_shape


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    return gpu_available


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", rc.ACCEPTED)
def test_every_shape_vs_oracle(orc, monkeypatch, name, form):
    """The case's shape is the one launched; the bars hold; a second solve on the same handle and a
    solve on a fresh handle repeat the first bit for bit."""
    a = rc.matrix(name)
    ref = rc.reference(orc, name)
    b = ref[0]
    monkeypatch.setenv("MSPMV_CG_RESIDENT", "1")
    monkeypatch.setenv("MSPMV_CG_RESIDENT_FORM", form)
    with mspmv.GpuCsr(a) as g:
        x1, it1, h1, st1 = g.cg_single(b, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
        kname = g.cg_kernel_name()
        x2, it2, h2, st2 = g.cg_single(b, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
        kname2 = g.cg_kernel_name()
    rpt, nzr, G = resident_shape(kname, form)
    predicted, _ = rc.predict_shape(a, G)
    table = rc.CASES[name][4]
    assert (rpt, nzr) == predicted, (kname, predicted)
    if G != 256 and predicted != table:  # never on an MI355X
        pytest.skip(f"{name}: on {G} CUs resident_build selects {predicted}, not the {table} the case reaches on 256")
    assert (rpt, nzr) == table, (kname, table)
    check_bars(orc, f"{name} {kname}", a, ref, x1, it1, h1, st1)
    assert kname2 == kname and st2 == st1 and it2 == it1
    np.testing.assert_array_equal(x2, x1)
    np.testing.assert_array_equal(h2, h1)
    x3, it3, h3, st3, kname3 = solve(a, b, MAX_ITERS, TOL, True, form=form)
    assert kname3 == kname and st3 == st1 and it3 == it1
    np.testing.assert_array_equal(x3, x1)
    np.testing.assert_array_equal(h3, h1)


@pytest.mark.parametrize("name", rc.ACCEPTED)
def test_two_kernel_path_on_irregular_rows(orc, name):
    """MSPMV_CG_RESIDENT=0: the merge-tile SpMV with the fused dot and k_cg1_update on matrices with
    unequal rows and scattered columns, held to the oracle's history and x (not only a residual)."""
    a = rc.matrix(name)
    ref = rc.reference(orc, name)
    x, it, h, st, kname = solve(a, ref[0], MAX_ITERS, TOL, False)
    assert kname.startswith(TWO_KERNEL) and "stall" not in kname, kname
    check_bars(orc, f"{name} {kname}", a, ref, x, it, h, st)


@pytest.mark.parametrize("name", rc.DECLINED)
def test_no_fitting_shape_runs_the_two_kernel_path(orc, name):
    """Rows too long for the rows per thread the blocks need (or for any shape): with the resident
    path enabled the solve runs the two-kernel CG from the start -- not after a stall -- and is right."""
    a = rc.matrix(name)
    assert rc.predict_shape(a, 256)[0] is None
    ref = rc.reference(orc, name)
    x, it, h, st, kname = solve(a, ref[0], MAX_ITERS, TOL, True)
    assert kname.startswith("pipelined") and "stall" not in kname, kname
    assert kname.startswith(TWO_KERNEL), kname
    check_bars(orc, f"{name} {kname}", a, ref, x, it, h, st)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", rc.TINY)
def test_tiny_matrices_with_empty_row_blocks(orc, name, form):
    a = rc.matrix(name)
    ref = rc.reference(orc, name)
    b = ref[0]
    x, it, h, st, kname = solve(a, b, MAX_ITERS, TOL, True, form=form)
    rpt, nzr, G = resident_shape(kname, form)
    assert (rpt, nzr) == (1, 4) == rc.predict_shape(a, G)[0], kname
    check_bars(orc, f"{name} {kname}", a, ref, x, it, h, st)
    assert len(h) == it
    if name == "one":  # 2 x = b: one iteration, alpha = b.b / (b 2 b), x = alpha b
        assert it == 1
        assert abs(x[0] - b[0] / 2) <= 2 * np.spacing(b[0] / 2)


@pytest.mark.parametrize("form", FORMS)
def test_tiny_max_iters(orc, form):
    """m = 65 (191 of 256 row blocks empty): max_iters caps the count and the capped run's history is
    the head of the long run's bit for bit; max_iters = 0 leaves x = 0."""
    a = rc.matrix("m65")
    b = rc.rhs(a.num_rows)
    _, it_long, h_long, st_long, k_long = solve(a, b, MAX_ITERS, TOL, True, form=form)
    x3, it3, h3, st3, k3 = solve(a, b, 3, TOL, True, form=form)
    resident_shape(k_long, form)
    resident_shape(k3, form)
    assert st_long == 0 and it_long > 3
    assert st3 == 0 and it3 == 3 and len(h3) == 3
    np.testing.assert_array_equal(h3, h_long[:3])
    x0, it0, h0, st0, k0 = solve(a, b, 0, TOL, True, form=form)
    resident_shape(k0, form)
    assert st0 == 0 and it0 == 0 and len(h0) == 0
    assert x0.shape == b.shape and not np.any(x0)


@pytest.mark.parametrize("form", FORMS)
def test_bars_tell_a_perturbed_matrix_apart(orc, form):
    """The bars bite, shown without running a wrong kernel: the GPU's solve of s28 passes against the
    oracle's solve of s28 and fails against the oracle's solve of s28 with one off-diagonal pair
    changed by 1e-6 (test_resident_cases.py shows the same with the oracle's own solve, and which
    bars notice)."""
    a = rc.matrix("s28")
    ref = rc.reference(orc, "s28")
    x, it, h, st, kname = solve(a, ref[0], MAX_ITERS, TOL, True, form=form)
    resident_shape(kname, form)
    check_bars(orc, f"s28 {kname}", a, ref, x, it, h, st)
    with pytest.raises(AssertionError, match="^x error in the maximum norm"):
        check_bars(orc, f"s28 {kname} against the perturbed matrix's solve", a, rc.perturbed_reference(orc, "s28"),
                   x, it, h, st)


@pytest.mark.parametrize("form", FORMS)
def test_breakdown_with_two_rows_per_thread(orc, form):
    """b = 0 on s28 (the (2, 8) shape): p.Ap = 0, alpha = 0/0 at the first iteration: status 4, one
    iteration, x stays 0 in every row slot."""
    a = rc.matrix("s28")
    x, it, h, st, kname = solve(a, np.zeros(a.num_rows), 10, 1e-8, True, form=form)
    rpt, nzr, _ = resident_shape(kname, form)
    assert rpt >= 2
    assert st == 4 and it == 1
    assert x.shape == (a.num_rows,) and not np.any(x)
