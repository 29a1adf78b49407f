"""What test_gpu_bicgstab_plans.py relies on, pinned on the CPU (as test_bicgstab.test_orders_agree_and_true_residual
does for the stencils): on the matrices of bicgstab_cases.py the restatements stop at the same iteration in every
summation order, the matrices have the margin the X bars assume, the window cases fit the offset-window plan, the
breakdown case breaks down exactly as described, and the bars tell a slightly wrong matrix apart."""
import numpy as np
import pytest

import bicgstab_cases as bc
import mspmv
import test_bicgstab as tb
import test_ilu0 as ti
from test_bicgstab import TOL

# (case, the widths the GPU tests solve it at)
WIDTHS = {"windows": (1, 4, 16), "windows_rem": (1, 4, 8, 16), "long_rows": (1, 4, 8, 16), "node_blocks": (1, 4, 16),
          "node_blocks6": (1, 4, 16), "band": (1, 8, 16), "staggered": (4,)}
CASES = [(name, L) for name, Ls in WIDTHS.items() for L in Ls]
# iterations of the restatement when the inputs were chosen: unpreconditioned, with ILU(0)
COUNT_RANGE = {"windows": ((68, 69), (12, 13)), "windows_rem": ((14, 16), (4, 5)), "long_rows": ((15, 16), (4, 5)),
               "node_blocks": ((6, 7), (2, 3)), "node_blocks6": ((6, 7), (2, 3)), "band": ((7, 8), (3, 4)), "staggered": ((48, 48), (11, 11))}


def _xbar(name):
    return dict(cond=bc.cond(name), spread_history=True) if name in ("windows", "staggered") else {}


@pytest.mark.parametrize("name,L", CASES)
def test_orders_agree_and_bars_hold_among_them(name, L):
    """The three dot orders -- with ILU(0) the reversed triangular-solve order too -- stop at the same iteration,
    every column's true residual is below TOL, and each order passes the GPU tests' bars against the reference
    order: rounding does not consume them."""
    a = tb.matrix(name)
    B = bc.rhs(name, L)
    for what, refs, (lo, hi) in (("plain", bc.reference(name, L), COUNT_RANGE[name][0]),
                                 ("ilu0", bc.ilu_reference(name, L), COUNT_RANGE[name][1])):
        counts = [r[1] for r in refs.values()]
        print(f"{name} L={L} {what}: iterations {counts}")
        assert len(set(counts)) == 1 and lo <= counts[0] <= hi, (name, L, what, counts)
        for v, (X, it, hist, st, conv) in refs.items():
            assert st == 0 and np.all(conv == 1) and len(hist) == it
            tr = tb.true_residual(a, B, X)
            assert np.all(tr <= TOL), (name, L, what, v, tr.max())
            hdev, _, _ = bc.check_bars(f"{name} L={L} {what} {v}", a, B, refs, X, it, hist, st, **_xbar(name))
            if name not in ("windows", "staggered"):  # (bicgstab_cases.reference_order relies on it)
                assert hdev <= 1e-13, (name, L, what, v, hdev)


@pytest.mark.parametrize("name", bc.DOMINANT)
def test_dominant_margin_and_ascending_columns(name):
    ro, ci, va = tb.matrix(name)
    n = len(ro) - 1
    rows = np.repeat(np.arange(n), np.diff(ro))
    same = rows[1:] == rows[:-1]
    assert np.all(np.diff(ci.astype(np.int64))[same] > 0)
    assert np.count_nonzero(ci == rows) == n  # every diagonal present
    off = np.bincount(rows, np.where(ci == rows, 0.0, np.abs(va)), n)
    diag = va[ci == rows]
    margin = (diag - off).min()
    print(f"{name}: n {n}, longest row {np.diff(ro).max()}, margin 1 - {1.0 - margin:.3g}")
    # 1 up to the rounding of the row's sum of magnitudes, here and in the generator (worst case 3,004 x 2^-53 x 4)
    assert margin >= 1.0 - 2e-12


def test_patterns_are_the_ones_named():
    """long_rows keeps its hub rows, node_blocks is kron_fem9(25, 20, 8)'s 72 columns per interior row, band is
    test_gpu_slab_mm's band with a diagonal, freeze2x2's blocks are dominant with margin 1 as well."""
    ro, ci, va = tb.matrix("long_rows")
    lens = np.diff(ro)
    assert len(ro) - 1 == 8000 and all(lens[h] >= 3000 for h in bc.HUBS) and np.sort(lens)[-4] <= 6
    ro, ci, va = tb.matrix("node_blocks")
    assert len(ro) - 1 == 4000 and np.diff(ro).max() == 72 and np.diff(ro).min() == 32
    ro, ci, va = tb.matrix("node_blocks6")
    assert len(ro) - 1 == 3600 and np.all(np.diff(ro) == 54)
    runs = ci.reshape(3600, 9, 6)  # nine runs of the six unknowns of one node, in every row
    assert np.all(runs[:, :, 0] % 6 == 0) and np.all(np.diff(runs, axis=2) == 1)
    ro, ci, va = tb.matrix("band")
    s = mspmv.CsrMatrix.synth_banded(30000, 30000 * 40, 2000, seed=3)
    assert len(ro) - 1 == 30000 and len(ci) >= s.num_nonzeros and np.diff(ro).max() <= 42
    rows = np.repeat(np.arange(30000), np.diff(ro))
    assert np.abs(ci - rows).max() <= 2000
    d = tb.dense(tb.matrix("freeze2x2"))
    np.testing.assert_array_equal(d[:4, :4], [[-3, -2, 0, 0], [1, 2, 0, 0], [0, 0, -3, -2], [0, 0, 1, 2]])
    assert d.shape == (1077, 1077) and not d[:300, 300:].any() and not d[300:, :300].any()
    assert (np.abs(np.diag(d)) - (np.abs(d).sum(axis=1) - np.abs(np.diag(d)))).min() >= 1.0 - 2e-12


def test_offset_windows_accepts_the_window_cases():
    w = mspmv.offset_windows(ti.csr(tb.matrix("windows")))
    assert w is not None and w["windows"] == 45 and w["remainder"] == 0
    w = mspmv.offset_windows(ti.csr(tb.matrix("windows_rem")))
    assert w is not None and w["windows"] == 45 and w["remainder"] > 0
    print(f"windows_rem: remainder {w['remainder']} of {len(tb.matrix('windows_rem')[1])} entries")
    for name in ("long_rows", "node_blocks", "node_blocks6", "band"):
        assert mspmv.offset_windows(ti.csr(tb.matrix(name))) is None, name


@pytest.mark.parametrize("name", bc.NAMES)
def test_ilu0_exists_without_a_shift(name):
    lu = ti.factor(name)
    ro, ci, _ = tb.matrix(name)
    rows = np.repeat(np.arange(len(ro) - 1), np.diff(ro))
    assert np.all(np.isfinite(lu))
    piv = np.abs(lu[ci == rows]).min()
    print(f"{name}: smallest |pivot| {piv:.3f}")
    assert piv >= (1.0 if name in bc.DOMINANT else 0.5)


def test_freeze2x2_breaks_down_in_the_update():
    """Column 0 in all three orders: hist[0] = 4 exactly (alpha = -1, omega = 0), then beta = NaN freezes it with
    X = -1 on the blocks' rows; the other columns are solved; status 4.  Alone (L = 1) the solve stops after one
    iteration with no live column."""
    a = tb.matrix("freeze2x2")
    B = bc.rhs("freeze2x2", 4)
    for o, (X, it, hist, st, conv) in bc.reference("freeze2x2", 4).items():
        assert st == 4 and list(conv) == [2, 1, 1, 1] and it == 12 and len(hist) == 12, (o, st, conv, it)
        assert hist[0] == 4.0
        assert np.all(X[:bc.N_2X2, 0] == -1.0) and np.all(X[bc.N_2X2:, 0] == 0.0)
        assert np.all(tb.true_residual(a, B[:, 1:], X[:, 1:]) <= TOL)
    for o, (X, it, hist, st, conv) in bc.reference("freeze2x2", 1).items():
        assert st == 4 and list(conv) == [2] and it == 1 and list(hist) == [4.0], (o, st, conv, it, hist)
        assert np.all(X[:bc.N_2X2, 0] == -1.0) and np.all(X[bc.N_2X2:, 0] == 0.0)


def test_freeze2x2_with_ilu0_converges_instead():
    """The ILU(0) factor of a 2 x 2 block is its LU factorisation, so the preconditioned column 0 converges in the
    first iteration in every variant: no breakdown, status 0.  The GPU test asserts this outcome."""
    a = tb.matrix("freeze2x2")
    for L, want in ((4, 5), (1, 1)):
        B = bc.rhs("freeze2x2", L)
        refs = bc.ilu_reference("freeze2x2", L)
        for v, (X, it, hist, st, conv) in refs.items():
            assert st == 0 and np.all(conv == 1) and it == want, (v, st, conv, it)
            assert np.all(tb.true_residual(a, B, X) <= TOL)
            bc.check_bars(f"freeze2x2 L={L} ilu0 {v}", a, B, refs, X, it, hist, st)
        x0 = refs[ti.VARIANTS[0]][0][:, 0]
        assert np.all(np.abs(x0[:bc.N_2X2:2] + 1.0) <= 4 * 2.0 ** -53) and np.all(np.abs(x0[1:bc.N_2X2:2] - 1.0) <= 4 * 2.0 ** -53)


def test_staggered_columns_converge_far_apart():
    """The recurrences are per column, so a column alone stops where it converges inside the panel: E's columns in
    a few iterations, the stencil's at least 30 later -- unpreconditioned, and 5 later with ILU(0)."""
    a = tb.matrix("staggered")
    B = bc.rhs("staggered", 4)
    alone = [tb.bicgstab_ref(a, B[:, [j]], 200, TOL)[1] for j in range(4)]
    palone = [ti.pbicgstab_ref(a, ti.apply_plans("staggered", "csr"), B[:, [j]], 200, TOL)[1] for j in range(4)]
    print(f"staggered: a column alone converges in {alone} iterations, with ILU(0) in {palone}")
    assert max(alone[0], alone[2]) <= 4 and min(alone[1], alone[3]) >= max(alone[0], alone[2]) + 30
    assert max(alone) == bc.reference("staggered", 4)["fsum"][1]
    assert max(palone[0], palone[2]) <= 3 and min(palone[1], palone[3]) >= max(palone[0], palone[2]) + 5
    # the early columns do not move again: the panel's solve holds the bits the column alone stopped with
    X = bc.reference("staggered", 4)["fsum"][0]
    for j in (0, 2):
        np.testing.assert_array_equal(X[:, [j]], tb.bicgstab_ref(a, B[:, [j]], 200, TOL)[0])


@pytest.mark.parametrize("L", [1, 4, 8, 16])
def test_bars_tell_a_perturbed_matrix_apart(L):
    """long_rows with the largest off-diagonal of hub row 3000 changed by 1e-6 of itself (about 3e-9 in a row whose
    diagonal is 5), solved by the restatement: the iteration count, the history (1e-12) and both residual bars
    accept it -- the residual sum bounds |X - X_ref| for any X -- and the rounding bar on |X - X_ref|_inf refuses
    it.  A bar that accepted it could not tell a slightly wrong split-row sum from a right one."""
    a = tb.matrix("long_rows")
    ro, ci, va = a
    r = bc.HUBS[1]
    ks = np.arange(ro[r], ro[r + 1])
    ks = ks[ci[ks] != r]
    k = ks[np.argmax(np.abs(va[ks]))]
    vp = va.copy()
    vp[k] *= 1.0 + 1e-6
    B = bc.rhs("long_rows", L)
    refs = bc.reference("long_rows", L)
    X, it, hist, st, _ = tb.bicgstab_ref((ro, ci, vp), B, 200, TOL)
    with pytest.raises(AssertionError, match=r"^x error .* of the rounding bar"):
        bc.check_bars(f"long_rows L={L}, one hub entry off by 1e-6", a, B, refs, X, it, hist, st)
    X0, it0, h0 = refs["fsum"][:3]
    assert it == it0 and np.abs(hist - h0).max() <= 1e-11
    moved = np.abs(X - X0).max(axis=0)
    bar = bc.rounding_bar(a, X0, it0)
    print(f"L={L}: X moved by {moved.max():.3e}, {np.max(moved / bar):.3g} of the rounding bar")
    assert np.max(moved / bar) >= 3.0


def test_inputs_are_shared_and_read_only():
    a = tb.matrix("long_rows")
    assert ti.matrix("long_rows") is a and tb.matrix("long_rows") is a
    with pytest.raises(ValueError):
        a[2][0] = 0.0
    with pytest.raises(ValueError):
        bc.rhs("staggered", 4)[0, 0] = 1.0
    B = bc.rhs("staggered", 4)
    assert not B[bc.N_EASY:, [0, 2]].any() and not B[:bc.N_EASY, [1, 3]].any() and B[:bc.N_EASY, 0].all()
    B = bc.rhs("freeze2x2", 4)
    assert np.all(B[:bc.N_2X2, 0] == 1.0) and not B[bc.N_2X2:, 0].any() and not B[:bc.N_2X2, 1:].any()
