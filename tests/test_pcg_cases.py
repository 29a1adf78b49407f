"""CPU: what test_gpu_pcg_forms.py relies on, pinned -- the matrices of pcg_cases.py are SPD of the row profile each
form needs, the preconditioners are symmetric with b^T M b > 0, the longdouble restatement pcg_reference agrees with
the oracle wherever the oracle can take the preconditioner (which licenses it for "jacobi" and "wide", where it
cannot), staggered has its stagger, a zero column does in the oracle what the GPU tests assert, and the one-iteration
probe would see one hub row's share of either dot go missing.

Measured, worst over test_restatement_matches_oracle's cases, restatement against oracle (bar): iterations equal in
every case, history 8.9e-16 (1e-10), ||X - Xo|| / ||Xo|| 4.2e-16 per column (1e-8).
test_probe_sensitivity: the smallest |alpha shift| / alpha bound over the hub rows and cases is 5.1e+6 (bar 100),
and every element of X then moves past its bound (bar: half of them).
"""
import numpy as np
import pytest

import pcg_cases as pc
from pcg_cases import LD, TOL

ON_PATTERN = [c for c in pc.solves() if c[2] not in pc.OFF_PATTERN]
MATRICES = [(name, L) for name, widths in pc.WIDTHS.items() for L in (widths if name == "many_tiles" else widths[:1])]
TILE_ITEMS = {1: 2048, 4: 1024, 8: 1536, 16: 1024}  # tile_items_for (csrc/mspmv_kernels.hip)


def _id(case):
    return "-".join(str(v) for v in case)


def dense_or_sparse(a):
    import scipy.sparse as sp

    return sp.csr_matrix((a.values, a.column_indices, a.row_offsets), shape=(a.num_rows, a.num_cols))


@pytest.mark.parametrize("case", MATRICES, ids=_id)
def test_matrices_are_what_they_claim(case):
    name, L = case
    a = pc.matrix(name, L)
    A = dense_or_sparse(a)
    n = a.num_rows
    rows = pc.rows_of(a)
    same_row = rows[1:] == rows[:-1]
    assert np.all(np.diff(a.column_indices.astype(np.int64))[same_row] > 0)  # ascending columns, no duplicates
    assert abs(A - A.T).max() == 0.0
    d = pc.diagonal(a)
    off = np.bincount(rows, np.abs(a.values), n) - np.abs(d)
    assert np.all(d > 0) and np.all(d > off)  # strictly dominant, positive diagonal: SPD
    lens = np.diff(a.row_offsets)
    if name in pc.HUBS:
        hubs = np.array(pc.HUBS[name])
        assert np.all(lens[hubs] >= pc.HUB_LEN[name])
        for w in pc.WIDTHS[name] + (8,):  # a hub row is split at every width: longer than an eighth of a tile
            assert pc.HUB_LEN[name] > TILE_ITEMS[w] // 8
        rest = np.delete(lens, hubs)
        assert rest.max() <= (10 if name == "long_rows" else 54 + len(hubs))
    if name == "many_tiles":
        tiles = -(-(n + a.num_nonzeros) // TILE_ITEMS[L])
        assert 65 <= tiles <= 127 and tiles % 2 == 1, tiles  # two fold blocks (64 tiles each at most), the last short
        assert lens.max() == 7
    if name == "dict16":
        assert lens.max() == 30 and lens.min() == 18
    if name in ("node_blocks6", "node_blocks_mixed"):
        clean = np.arange(n) >= (n // 3 if name == "node_blocks_mixed" else 0)
        if name in pc.HUBS:
            clean[list(pc.HUBS[name])] = False
        assert np.all(lens[clean] == 54)
        # the six rows of a node list the same columns
        first = (np.arange(n) // 6) * 6
        ok = clean & clean[first]
        ro = a.row_offsets[:-1].astype(np.int64)
        cols = np.stack([a.column_indices[ro[ok] + k] for k in range(54)])
        cols0 = np.stack([a.column_indices[ro[first[ok]] + k] for k in range(54)])
        assert np.array_equal(cols, cols0)
    if name == "staggered":
        assert A[:pc.N_EASY, pc.N_EASY:].nnz == 0 and n == pc.N_EASY + 30 * 31


@pytest.mark.parametrize("case", [c for c in pc.solves() if c[2] != "ic0"], ids=_id)
def test_preconditioners_are_symmetric_and_positive_on_the_rhs(case):
    name, L, kind = case
    a, m = pc.matrix(name, L), pc.preconditioner(name, L, kind)
    M = dense_or_sparse(m)
    assert m.num_rows == m.num_cols == a.num_rows
    assert abs(M - M.T).max() <= 1e-15 * abs(M).max()
    B = pc.rhs(name, L)
    bmb = np.sum(B * (M @ B), axis=0)
    assert np.all(bmb > 0), bmb
    if kind in ("spai", "neumann"):
        assert np.array_equal(m.row_offsets, a.row_offsets) and np.array_equal(m.column_indices, a.column_indices)
    if kind == "jacobi":
        assert m.num_nonzeros == a.num_rows
    if kind == "wide":
        assert 1.9 * a.num_nonzeros < m.num_nonzeros < 2.3 * a.num_nonzeros and np.all(pc.diagonal(m) == 1.0)
        rows = pc.rows_of(m)
        assert np.all(np.bincount(rows, np.abs(m.values), m.num_rows) < 2.0)  # strictly dominant: SPD


@pytest.mark.parametrize("kind", ["ic0"])
@pytest.mark.parametrize("name", list(pc.WIDTHS))
def test_ic0_is_unshifted_and_inexact_where_claimed(name, kind):
    L = pc.WIDTHS[name][0]
    l = pc.ic0(name, L)  # (asserts shift == 0)
    assert l.num_rows == pc.matrix(name, L).num_rows
    if name == "dict16":  # not the exact factor: the solve takes more than one iteration
        assert pc.reference(name, L, kind)[1] > 2


@pytest.mark.parametrize("case", ON_PATTERN, ids=_id)
def test_restatement_matches_oracle(orc, case):
    """pcg_reference (np.longdouble) against orc_pcg_spai_multi / orc_pcg_ic0_multi under the project's parity bars
    (pcg_cases.check_bars): the same iterations, the history within 1e-10, X within 1e-8 per column."""
    name, L, kind = case
    X, it, hist, _ = pc.reference(name, L, kind)
    ref = pc.oracle_solve(orc, name, L, kind)
    assert it == ref[1]
    pc.check_bars(f"restatement, {name} L={L} {kind}", ref, (X, it, hist, 0))


@pytest.mark.parametrize("kind", [pc.SPAI_KIND["staggered"], "ic0"])
def test_staggered_has_its_stagger(orc, kind):
    conv_at = pc.reference("staggered", 4, kind)[3]
    print(f"staggered {kind}: columns converge at iterations {conv_at}")
    assert np.all(conv_at >= 0)
    assert conv_at[[1, 3]].min() - conv_at[[0, 2]].max() >= 5
    # (and the cut of test_frozen_columns_stay_frozen lies between them)
    assert conv_at[[0, 2]].max() + 1 + 3 <= 8 <= conv_at[[1, 3]].min() - 2


def test_zero_column_in_the_oracle(orc):
    """long_rows, L = 4, column 1 of B zero.  SPAISolveMultiple's guards give alpha = beta = 0 there: the column
    converges at the first iteration with X exactly 0, and the solve ends as without it.  PCGSolveMultiple has no
    guard: 0 / 0, a NaN column that the history skips and that never converges, so it runs to max_iters.  Alone the
    column does the same: one iteration and X = 0, or max_iters of NaN.  pcg_reference restates both."""
    name, L = "long_rows", 4
    B = pc.rhs(name, L).copy()
    B[:, 1] = 0.0
    spai = pc.SPAI_KIND[name]
    X, it, hist = pc.oracle_solve(orc, name, L, spai, B)
    assert it < pc.MAX_ITERS and hist[-1] < TOL and np.all(X[:, 1] == 0.0) and np.all(np.isfinite(X))
    Xr, itr, hr, conv_at = pc.pcg_reference(pc.matrix(name), pc.applier(name, L, spai), B, pc.MAX_ITERS, TOL, True)
    assert itr == it and conv_at[1] == 0 and np.all(Xr[:, 1] == 0.0) and np.max(np.abs(hr - hist)) <= 1e-10
    X1, it1, h1 = pc.oracle_solve(orc, name, 1, spai, B[:, 1:2])
    assert it1 == 1 and list(h1) == [0.0] and np.all(X1 == 0.0)
    cap = 12
    X, it, hist = pc.oracle_solve(orc, name, L, "ic0", B, max_iters=cap)
    assert it == cap and np.all(np.isnan(X[:, 1])) and np.all(np.isfinite(X[:, [0, 2, 3]]))
    done = int(np.flatnonzero(hist < TOL)[0])
    assert done < 10 and np.all(hist[done:] == hist[done])  # the other columns converge, then stay frozen
    Xr, itr, hr, conv_at = pc.pcg_reference(pc.matrix(name), pc.applier(name, L, "ic0"), B, cap, TOL, False)
    assert itr == cap and conv_at[1] == -1 and np.all(np.isnan(Xr[:, 1])) and np.max(np.abs(hr - hist)) <= 1e-10
    X1, it1, h1 = pc.oracle_solve(orc, name, 1, "ic0", B[:, 1:2], max_iters=cap)
    assert it1 == cap and np.all(np.isnan(X1)) and np.all(h1 == 0.0)


@pytest.mark.parametrize("case", [c for c in pc.solves() if c[0] in pc.HUBS], ids=_id)
def test_probe_sensitivity(case):
    """A condition on the inputs of test_one_iteration_dots, computed on the reference side alone: with the hub
    rows of B at 20 + U(0, 1), leaving any one hub row's term Z*_i (A Z*)_i out of the denominator, or B_i Z*_i out
    of the numerator, moves alpha* by at least 100 times the probe's bound on alpha -- and then moves most of X past
    its elementwise bound.  (A carry counted twice or not at all is a share of such a term; a whole term is what
    the bound is sized against.)"""
    name, L, kind = case
    p = pc.probe(name, L, kind)
    B = np.asarray(pc.rhs(name, L), LD)
    worst, moved = np.inf, 1.0
    for i in pc.HUBS[name]:
        shifts = [p["num"] / (p["den"] - p["Z"][i] * p["AZ"][i]) - p["alpha"],
                  (p["num"] - B[i] * p["Z"][i]) / p["den"] - p["alpha"]]
        for shift in shifts:
            worst = min(worst, float(np.min(np.abs(shift) / p["alpha_bound"])))
            moved = min(moved, float(np.mean(np.abs(shift) * np.abs(p["Z"]) > p["x_bound"])))
    print(f"{name} L={L} {kind}: smallest |alpha shift| / alpha bound {worst:.3g}; at least {moved:.0%} of X moves "
          f"past its bound; relative alpha bound {float(np.max(p['alpha_bound'] / np.abs(p['alpha']))):.3e}")
    assert worst >= 100.0
    assert moved >= 0.5
