"""CPU: what test_gpu_nonfinite.py relies on, pinned -- bad_columns picks the columns its docstring says (restated
here on a hand-made plan of whole-row tiles), poison touches exactly one entry per bad column, the oracle's products
of a poisoned input are non-finite exactly where a row holds a nonzero in a column poisoned in that panel column,
the caps of input_conditions hold on the shapes that need no GPU, and check_nonfinite passes the oracle's own output
and rejects it with a finite row turned NaN, with an infinity of the wrong sign and with a finite entry one ulp off.
"""
import functools

import numpy as np
import pytest

import nonfinite_cases as nf

SHAPES = ["short_first_r12_odd", "short_first_r13", "kron9_6", "kron9_8", "hub_rect", "long_rows_many_tiles", "rows50"]
WIDTHS = [1, 2, 8]


@functools.lru_cache(maxsize=None)
def shape(name):
    a = nf.cpu_shapes()[name]()
    return a, nf.whole_row_plan(a)


@functools.lru_cache(maxsize=None)
def products(orc, name, L):
    """(a, plan, cols, pairs, X, gold, X_clean, gold_clean), shared and left unchanged."""
    a, plan = shape(name)
    cols, pairs = nf.bad_columns(a, plan)
    X = nf.poison(np.random.default_rng(5 + L).uniform(-1, 1, (a.num_cols, L)), cols)
    Xc = nf.cleaned(X)
    mul = (lambda V: orc.spmv_gold(a, V[:, 0].copy())[:, None]) if L == 1 else (lambda V: orc.csr_spmm_t(a, V))
    return a, plan, cols, pairs, X, mul(X), Xc, mul(Xc)


def test_cpu_shapes_are_all_listed():
    assert sorted(nf.cpu_shapes()) == sorted(SHAPES)


@pytest.mark.parametrize("name", SHAPES)
def test_bad_columns(name):
    a, plan = shape(name)
    cols, pairs = nf.bad_columns(a, plan)
    n, ro, ci = a.num_cols, a.row_offsets.astype(np.int64), a.column_indices
    assert len(set(cols)) == len(cols) and all(0 <= c < n for c in cols)
    assert cols[:3] == [0, n - 1, n - 2]
    b = plan["bounds"]
    assert np.array_equal(ro[b[:, 0]], b[:, 1]) and plan["num_tiles"] >= 3  # whole rows, several tiles
    want = [0, n - 1, n - 2]
    nt = plan["num_tiles"]
    for t in (0, nt // 2, nt - 1):  # every tile of these shapes holds nonzeros
        tile = ci[b[t][1]:b[t + 1][1]]
        assert tile.size
        want += [int(tile.min()), int(tile[-1])]
    # the prefix pairs, one pair of rows at a time
    every = []
    for i in range(a.num_rows - 1):
        p, q = ci[ro[i]:ro[i + 1]], ci[ro[i + 1]:ro[i + 2]]
        if p.size != q.size:
            s, l = (p, q) if p.size < q.size else (q, p)
            if np.array_equal(s, l[: s.size]):
                every.append(((i, i + 1) if p.size < q.size else (i + 1, i)) + (int(l[s.size]),))
    assert nf.prefix_pairs(a) == every
    assert len(pairs) == min(nf.MAX_PAIRS, len(every)) and set(pairs) <= set(every)
    if name.startswith("short_first"):  # every node's first row lacks the node's last five columns
        assert len(every) == a.num_rows // 6 + 1 and all(s % 6 == 0 and l == s + 1 for s, l, _ in every)
        assert pairs[0] == every[0] and pairs[-1] == every[-1] and len(pairs) == 4
        for s, l, c in pairs:
            assert c == ci[ro[l + 1] - 5] and c not in ci[ro[s]:ro[s + 1]]
    want += [c for _, _, c in pairs]
    chosen = list(dict.fromkeys(want))
    want += [int(c) for c in np.random.default_rng(0).integers(0, n, 4)]
    assert cols == list(dict.fromkeys(want))
    none, _ = nf.bad_columns(a, plan, num_random=0)  # a case over the cap gives up random columns, nothing else
    assert none == chosen


def test_bad_columns_tiny():
    """n = 1 and n = 2: the columns that do not exist are skipped; a plan without nonzeros gives no tile columns."""
    import mspmv

    one = mspmv.CsrMatrix.from_arrays(1, np.array([0, 1], np.int32), np.zeros(1, np.int32), np.ones(1))
    assert nf.bad_columns(one, nf.whole_row_plan(one)) == ([0], [])
    two = mspmv.CsrMatrix.from_arrays(2, np.array([0, 1, 3], np.int32), np.array([1, 0, 1], np.int32), np.ones(3))
    cols, pairs = nf.bad_columns(two, nf.whole_row_plan(two))
    assert sorted(cols) == [0, 1] and cols[:2] == [0, 1] and pairs == []
    empty = mspmv.CsrMatrix.from_arrays(7, np.zeros(4, np.int32), np.zeros(0, np.int32), np.zeros(0))
    cols, pairs = nf.bad_columns(empty, {"num_tiles": 1, "bounds": np.array([[0, 0], [3, 0]], np.int32)})
    assert cols[:3] == [0, 6, 5] and len(cols) <= 7 and pairs == []
    # an empty row is a proper prefix too, but pairs with a non-empty shorter row go first
    ro = np.array([0, 0, 2, 5, 7], np.int32)
    ci = np.array([3, 4, 3, 4, 6, 1, 2], np.int32)
    pre = mspmv.CsrMatrix.from_arrays(8, ro, ci, np.ones(7))
    assert nf.prefix_pairs(pre) == [(0, 1, 3), (1, 2, 6)]
    assert nf.bad_columns(pre, nf.whole_row_plan(pre))[1] == [(1, 2, 6)]


@pytest.mark.parametrize("L", [1, 2, 3, 16])
def test_poison_touches_one_entry_per_column(L):
    n = 50
    X = np.random.default_rng(L).uniform(-1, 1, (n, L) if L > 1 else n)
    cols = [0, 49, 48, 7, 21, 30, 11]
    P = nf.poison(X, cols)
    assert P.shape == X.shape and P is not X and np.all(np.isfinite(X))
    changed = np.argwhere((P != X).reshape(n, -1))
    assert changed.tolist() == sorted([c, k % L] for k, c in enumerate(cols))
    V = P.reshape(n, -1)
    assert V[0, 0] == np.inf and V[49, 1 % L] == -np.inf and np.isnan(V[48, 2 % L]) and V[7, 3 % L] == np.inf
    C = nf.cleaned(P)
    assert np.array_equal(C != X, P != X) and np.all(C.reshape(n, -1)[cols, [k % L for k in range(len(cols))]] == 0.0)


@pytest.mark.parametrize("L", WIDTHS)
@pytest.mark.parametrize("name", SHAPES)
def test_oracle_pattern_and_caps(orc, name, L):
    """The oracle's non-finite entries are where the numpy restatement puts them, and the caps hold: 1 .. m / 4
    non-finite rows, a mixed row at L >= 2, a prefix pair split where there are pairs."""
    a, plan, cols, pairs, X, gold, Xc, gold_clean = products(orc, name, L)
    assert np.array_equal(~np.isfinite(gold), nf.predicted_nonfinite(a, cols, L))
    assert np.all(np.isfinite(gold_clean))
    bad, mixed, split = nf.input_conditions(a, gold, L, pairs)
    print(f"{name} L={L}: {len(cols)} bad columns, {bad} of {a.num_rows} rows non-finite, {mixed} mixed, "
          f"{split} of {len(pairs)} prefix pairs split")
    assert 1 <= bad <= a.num_rows // 4
    assert (mixed >= 1) == (L >= 2)
    assert split == len(pairs) or not name.startswith("short_first")


def test_input_conditions_reject_empty_cases(orc):
    a, plan, cols, pairs, X, gold, Xc, gold_clean = products(orc, "short_first_r12_odd", 2)
    with pytest.raises(AssertionError, match="rows non-finite"):
        nf.input_conditions(a, gold_clean, 2, pairs)          # no non-finite row
    with pytest.raises(AssertionError, match="rows non-finite"):
        nf.input_conditions(a, np.where(np.arange(a.num_rows)[:, None] % 3 == 0, np.nan, gold_clean), 2)  # a third
    whole = np.where(np.isfinite(gold).all(axis=1, keepdims=True), gold_clean, np.nan)
    with pytest.raises(AssertionError, match="panel columns"):
        nf.input_conditions(a, whole, 2, pairs)                # no mixed row
    with pytest.raises(AssertionError, match="prefix pair"):
        nf.input_conditions(a, gold, 2, [(l, s, c) for s, l, c in pairs])  # no pair split the right way round


def ulp_up(v):
    return np.nextafter(v, np.inf)


@pytest.mark.parametrize("L", WIDTHS)
@pytest.mark.parametrize("name", ["short_first_r13", "hub_rect", "kron9_8"])
def test_check_nonfinite_rejects_doctored_outputs(orc, name, L):
    a, plan, cols, pairs, X, gold, Xc, gold_clean = products(orc, name, L)
    args = (gold_clean, gold_clean, Xc, plan, L, pairs)
    counts = nf.check_nonfinite(a, gold, gold, *args)  # the oracle's own output passes
    assert counts == nf.input_conditions(a, gold, L, pairs)
    fin = np.argwhere(np.isfinite(gold))
    inf = np.argwhere(np.isinf(gold))
    assert len(inf), "no infinity in the oracle's output"

    Y = gold.copy()                      # a finite row turned NaN (a pad slot's 0.0 * Inf)
    Y[tuple(fin[len(fin) // 2])] = np.nan
    with pytest.raises(AssertionError, match="NaN on one side"):
        nf.check_nonfinite(a, Y, gold, *args)

    Y = gold.copy()                      # an infinity of the wrong sign
    Y[tuple(inf[0])] *= -1.0
    with pytest.raises(AssertionError, match="wrong sign"):
        nf.check_nonfinite(a, Y, gold, *args)

    Y = gold.copy()                      # a finite entry one ulp off
    i = tuple(fin[len(fin) // 3])
    Y[i] = ulp_up(Y[i])
    with pytest.raises(AssertionError, match="differ from the cleaned product"):
        nf.check_nonfinite(a, Y, gold, *args)

    Y = gold.copy()                      # ... and an Inf where the oracle has NaN, a finite entry where it has Inf
    nan = np.argwhere(np.isnan(gold))
    if len(nan):
        Y[tuple(nan[0])] = np.inf
        with pytest.raises(AssertionError, match="NaN on one side"):
            nf.check_nonfinite(a, Y, gold, *args)
    Y = gold.copy()
    Y[tuple(inf[0])] = 1.0
    with pytest.raises(AssertionError, match="finite on one side"):
        nf.check_nonfinite(a, Y, gold, *args)


def test_check_nonfinite_all_empty(orc):
    """The all-empty matrix: y is +0.0 whatever x holds; -0.0 or NaN is rejected."""
    from test_gpu_spmv import edge_case

    a = edge_case("all_empty")
    plan = {"num_tiles": 1, "bounds": np.array([[0, 0], [a.num_rows, 0]], np.int32), "modes": np.ones(1, np.uint8)}
    cols, pairs = nf.bad_columns(a, plan)
    x = nf.poison(np.random.default_rng(1).uniform(-1, 1, a.num_cols), cols)
    gold = orc.spmv_gold(a, x)
    z = np.zeros(a.num_rows)
    assert nf.check_nonfinite(a, gold, gold, z, z, nf.cleaned(x), plan, 1, pairs) == (0, 0, 0)
    for v in (-0.0, np.nan):
        y = z.copy()
        y[17] = v
        with pytest.raises(AssertionError):
            nf.check_nonfinite(a, y, gold, z, z, nf.cleaned(x), plan, 1, pairs)
