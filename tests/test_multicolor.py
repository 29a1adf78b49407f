"""Multi-colour ILU(0) on the CPU: the greedy colouring and the symmetric permutation against their numpy
restatements (multicolor_cases.py), the property the ordering exists for -- the permuted factor has at most as
many dependency levels as colours -- the restated preconditioned BiCGSTAB's iteration counts, and the inputs
mspmv_ilu0_create_colored must refuse before it touches a device."""
import ctypes

import numpy as np
import pytest

import mspmv
import multicolor_cases as mc
import test_bicgstab as tb
import test_ilu0 as ti
from test_bicgstab import TOL

INVALID, BREAKDOWN = 1, 4


# ---- colouring -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["convdiff30", "convdiff60s", "randdd", "hubs", "chain515"])
def test_color_greedy_is_the_restatement(name):
    a = mc.matrix(name)
    ro, ci, _ = a
    n = len(ro) - 1
    colors, num = mspmv.color_greedy(mc.csr(a))
    ref, num_ref = mc.greedy_ref(a)
    print(f"{name}: {num} colours, rows per colour {np.bincount(colors).tolist()}")
    assert colors.dtype == np.int32 and num == num_ref
    np.testing.assert_array_equal(colors, ref)
    rows = np.repeat(np.arange(n), np.diff(ro))
    off = rows != ci
    assert np.all(colors[rows[off]] != colors[ci[off]])  # every stored (i, j), i != j, joins two colours
    assert np.array_equal(np.unique(colors), np.arange(num))
    assert num <= mc.max_degree(a) + 1
    if name.startswith("convdiff") or name == "chain515":
        assert num == 2
    if name == "chain515":
        assert np.bincount(colors).tolist() == [258, 257]
    if name == "randdd":  # structurally nonsymmetric: some (j, i) is stored without (i, j) -- the A + A^T rule
        d = tb.dense(a) != 0
        assert not np.array_equal(d, d.T)
    if name == "hubs":  # the two dense rows sit alone in their colours
        count = np.bincount(colors)
        assert count[colors[200]] == 1 and count[colors[599]] == 1


# ---- permutation -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["randdd", "hubs", "chain515"])
def test_csr_permute_sym_against_dense(name):
    a = mc.matrix(name)
    n = len(a[0]) - 1
    for perm in (mc.ordering(name)[2], np.random.default_rng(3).permutation(n).astype(np.int32)):
        p = mspmv.csr_permute_sym(mc.csr(a), perm)
        d = tb.dense(a)
        np.testing.assert_array_equal(tb.dense((p.row_offsets, p.column_indices, p.values)), d[np.ix_(perm, perm)])
        assert p.num_nonzeros == len(a[1])
        rows = np.repeat(np.arange(n), np.diff(p.row_offsets))
        same = rows[1:] == rows[:-1]
        assert np.all(np.diff(p.column_indices.astype(np.int64))[same] > 0)  # strictly ascending
    ro, ci, va = mc.permuted(a, mc.ordering(name)[2])
    p = mspmv.csr_permute_sym(mc.csr(a), mc.ordering(name)[2])
    np.testing.assert_array_equal(p.row_offsets, ro)
    np.testing.assert_array_equal(p.column_indices, ci)
    np.testing.assert_array_equal(p.values, va)


def test_csr_permute_sym_rejects_what_is_no_permutation():
    a = mc.csr(mc.matrix("chain515"))
    for bad, what in ((3, "repeat"), (515, "out of range"), (-1, "out of range")):
        perm = np.arange(515, dtype=np.int32)
        perm[4] = bad
        with pytest.raises(mspmv.MspmvError, match=what) as e:
            mspmv.csr_permute_sym(a, perm)
        assert e.value.status == INVALID


# ---- levels: the property the feature exists for ----------------------------------------------------------
@pytest.mark.parametrize("name", ["convdiff30", "convdiff60", "convdiff60s", "randdd", "hubs", "chain515"])
def test_permuted_factor_has_at_most_one_level_per_colour(name):
    num = mc.ordering(name)[1]
    pl, pu = mc.tri_plans(name, "csr")
    natural = [len(p.levels) + 1 for p in ti.apply_plans(name, "csr")] if name != "chain515" else None
    print(f"{name}: {num} colours, levels L {len(pl.levels) + 1}, U {len(pu.levels) + 1}; natural order {natural}")
    assert len(pl.levels) + 1 <= num and len(pu.levels) + 1 <= num
    # the factor create_colored uploads is the library's ILU(0) of the permuted matrix: the restatement's bits
    ap = mc.csr(mc.ordering(name)[3])
    np.testing.assert_array_equal(mspmv.ilu0_values(ap), mc.ordering(name)[4])


# ---- the restated solver ----------------------------------------------------------------------------------
# fsum iteration counts at TOL; the stencils' are the issue's table (23 / 25, 33 / 35, 47 / 48), randdd's is what
# the restatement gives
COUNTS = {("convdiff30", 1): 23, ("convdiff30", 8): 25, ("convdiff60", 1): 33, ("convdiff60", 8): 35,
          ("convdiff60s", 1): 47, ("convdiff60s", 8): 48, ("randdd", 1): 5, ("randdd", 8): 5}


@pytest.mark.parametrize("name,L", sorted(COUNTS))
def test_variants_agree_and_true_residual(name, L):
    a = mc.matrix(name)
    B = tb.rhs(len(a[0]) - 1, L)
    ref = mc.reference(name, L)
    counts = [ref[v][1] for v in ti.VARIANTS]
    print(f"{name} L={L}: iterations {counts}")
    assert max(counts) - min(counts) <= 1, counts
    assert counts[0] == COUNTS[(name, L)], counts
    for v in ti.VARIANTS:
        X, it, hist, st, conv = ref[v]
        assert st == 0 and np.all(conv == 1) and len(hist) == it
        tr = tb.true_residual(a, B, X)
        print(f"  {v}: worst true residual {tr.max():.3e}")
        assert np.all(tr <= 2 * TOL), (v, tr.max())


# ---- rejections, no device needed ---------------------------------------------------------------------------
def _colored(a, colors):
    return mspmv.GpuIlu0.colored(a, None if colors is None else np.asarray(colors, np.int32))


def test_create_colored_rejects_bad_colours():
    a = mc.csr(mc.matrix("chain515"))
    good = np.arange(515) % 2
    cases = {"adjacent equal": (np.where(np.arange(515) == 41, 0, good), r"row 40\b"),  # rows 40, 41, 42 share 0
             "negative": (np.where(np.arange(515) == 77, -1, good), r"row 77\b"),
             "not below n": (np.where(np.arange(515) == 78, 515, good), r"row 78\b"),
             "gap": (np.where(good == 1, 2, good), r"row 1\b")}
    for what, (colors, row) in cases.items():
        with pytest.raises(mspmv.MspmvError, match=row) as e:
            _colored(a, colors)
        assert e.value.status == INVALID, what


@pytest.mark.parametrize("kind", ["unsorted", "no_diagonal"])
def test_create_colored_rejects_rows_it_cannot_factor(kind):
    with pytest.raises(mspmv.MspmvError, match=r"row 400\b") as e:
        _colored(ti._broken(kind), None)
    assert e.value.status == INVALID
    with pytest.raises(mspmv.MspmvError, match=r"row 400\b") as e:
        mspmv.color_greedy(ti._broken(kind))
    assert e.value.status == INVALID


def test_create_colored_rejects_non_square():
    a = mspmv.CsrMatrix.from_arrays(3, [0, 1, 2], [0, 1], [1.0, 1.0])
    with pytest.raises(mspmv.MspmvError, match="square") as e:
        _colored(a, None)
    assert e.value.status == INVALID


def test_create_colored_zero_pivot_is_a_breakdown():
    """[[1, 1], [1, 1]]: two colours, and the second row's pivot cancels in the permuted factorisation just as in
    the natural one; with the colours swapped it is the first row's (the second of the ordering) that does."""
    a = mspmv.CsrMatrix.from_arrays(2, [0, 2, 4], [0, 1, 0, 1], [1.0, 1.0, 1.0, 1.0])
    for colors in (None, [0, 1], [1, 0]):
        with pytest.raises(mspmv.MspmvError, match=r"row 1\b") as e:
            _colored(a, colors)
        assert e.value.status == BREAKDOWN


def test_abi_symbols():
    lib = ctypes.CDLL(tb.LIB)
    for name in ("mspmv_color_greedy", "mspmv_csr_permute_sym", "mspmv_ilu0_create_colored", "mspmv_ilu0_colors",
                 "mspmv_ilu0_apply_dev"):
        assert hasattr(lib, name), name
    assert callable(mspmv.color_greedy) and callable(mspmv.csr_permute_sym)
    for attr in ("colored", "num_colors", "perm", "apply", "apply_dev"):
        assert hasattr(mspmv.GpuIlu0, attr), attr
