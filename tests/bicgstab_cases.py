"""Matrices and right-hand sides that take BiCGSTAB and ILU(0)-BiCGSTAB (csrc/mspmv_bicgstab.hip) off the plain
merge tiles and into the per-column freezes (test_bicgstab_cases.py, test_gpu_bicgstab_plans.py).  One case per
product path of launch_solver_product -- offset windows with and without a remainder, the column-slab SpMM, the
node-block kernel, merge tiles with rows split across tiles -- and two for the per-column logic: columns that
converge dozens of iterations apart, and a column whose omega and then beta break down in exact arithmetic.

CSR as (row_offsets int32, column_indices int32, values float64), columns ascending, as test_bicgstab's.  Seeded,
built once, numpy only (band's pattern is the library's host-side synth_banded, test_gpu_slab_mm's "band").

All but freeze2x2 share one value rule, dominant(): off-diagonals U(-1, 1) x min(1, 8 / the row's off-diagonal
count), the diagonal added where absent and set to sum |off-diagonal| + 1.  So the matrix is strictly row diagonally
dominant with margin 1 -- ||A^-1||_inf <= 1 (Varah), the X bar of the GPU tests -- ILU(0) exists without a shift,
and the pattern is kept.  The row scaling keeps a hub row's sum |off-diagonal| near 4 instead of near 1,500: with
unscaled hub rows the iteration count wandered between the restatement's own summation orders.
"""
import functools

import numpy as np

import test_bicgstab as tb

TOL = tb.TOL


def _csr(n, rows, cols, vals):
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    ro = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=ro[1:])
    return ro.astype(np.int32), cols.astype(np.int32), vals.astype(np.float64)


def dominant(n, rows, cols, seed):
    """The value rule of this file's docstring on the pattern {(rows, cols)} of an n x n matrix (duplicates and
    diagonal entries in the input are harmless: the pattern is the set, plus the diagonal)."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    key = np.unique(rows[rows != cols] * n + cols[rows != cols])
    rows, cols = key // n, key % n
    cnt = np.bincount(rows, minlength=n)
    vals = np.random.default_rng(seed).uniform(-1.0, 1.0, rows.size) * np.minimum(1.0, 8.0 / np.maximum(cnt, 1))[rows]
    diag = np.bincount(rows, np.abs(vals), n) + 1.0
    d = np.arange(n, dtype=np.int64)
    return _csr(n, np.concatenate([rows, d]), np.concatenate([cols, d]), np.concatenate([vals, diag]))


def _offsets_pattern(n, offsets):
    r = np.arange(n, dtype=np.int64)
    rows = np.concatenate([r[(r + o >= 0) & (r + o < n)] for o in offsets])
    cols = np.concatenate([r[(r + o >= 0) & (r + o < n)] + o for o in offsets])
    return rows, cols


def blockdiag(a, b):
    na = len(a[0]) - 1
    return (np.concatenate([a[0], b[0][1:] + a[0][-1]]).astype(np.int32),
            np.concatenate([a[1], b[1] + na]).astype(np.int32), np.concatenate([a[2], b[2]]))


def windows_rem():
    """Six common offsets on 44 windows of 64 rows and one of 13, and 2 % as many entries again at uniformly random
    places, which no window lists among its offsets: they go to the plan's remainder."""
    n = 64 * 44 + 13
    rows, cols = _offsets_pattern(n, (-70, -3, 0, 2, 9, 70))
    rng = np.random.default_rng(41)
    extra = int(0.02 * rows.size)
    return dominant(n, np.concatenate([rows, rng.integers(0, n, extra)]),
                    np.concatenate([cols, rng.integers(0, n, extra)]), 42)


HUBS = (5, 3000, 6000)


def long_rows(n=8000, per_hub=3000):
    """Five offsets and three hub rows of per_hub random columns: a hub row spans several merge tiles at every
    width, so its tiles carry into the one that completes it (TilePlan::d_fix, d_fix_cnt)."""
    rows, cols = _offsets_pattern(n, (1, 2, 7, -3, -40))
    rng = np.random.default_rng(43)
    hub_cols = [rng.choice(n, per_hub, replace=False) for _ in HUBS]
    rows = np.concatenate([rows] + [np.full(per_hub, h, np.int64) for h in HUBS])
    return dominant(n, rows, np.concatenate([cols] + hub_cols), 44)


def kron9_pattern(nx, ny, dof):
    """The pattern of test_gpu_blocks.kron_fem9(nx, ny, dof): a 9-point node stencil on an nx x ny grid, every
    node pair a dense dof x dof block."""
    rows, cols = [], []
    k = np.arange(dof, dtype=np.int64)
    for i in range(ny):
        for j in range(nx):
            for di in (-1, 0, 1):
                for dj in (-1, 0, 1):
                    if 0 <= i + di < ny and 0 <= j + dj < nx:
                        a, b = i * nx + j, (i + di) * nx + j + dj
                        rows.append(np.repeat(a * dof + k, dof))
                        cols.append(np.tile(b * dof + k, dof))
    return nx * ny * dof, np.concatenate(rows), np.concatenate(cols)


def node_blocks():
    """72 columns per interior row: two pattern chunks per run, so the single-RHS tile kernel stages the node blocks
    through LDS, and the L-wide products keep their own merge tiles (with column dictionaries at L = 16)."""
    n, rows, cols = kron9_pattern(25, 20, 8)
    return dominant(n, rows, cols, 45)


def torus9_pattern(nx, ny, dof):
    """kron9_pattern's node stencil on a periodic nx x ny grid: no boundary nodes, every row 9 dof columns."""
    N = nx * ny
    k = np.arange(dof, dtype=np.int64)
    node = np.arange(N, dtype=np.int64)
    i, j = node // nx, node % nx
    rows, cols = [], []
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            other = ((i + di) % ny) * nx + (j + dj) % nx
            rows.append(np.repeat(node * dof, dof * dof) + np.tile(np.repeat(k, dof), N))
            cols.append(np.repeat(other * dof, dof * dof) + np.tile(np.tile(k, dof), N))
    return N * dof, np.concatenate(rows), np.concatenate(cols)


def node_blocks6():
    """The second, smaller-dof pattern: 6 unknowns per node on a 30 x 20 torus, 54 columns in every row.  Every
    single-RHS tile is then a register run tile, which is what puts the L-wide products on k_spmm_blk (and the
    single-RHS one on k_spmv_blk); a grid with boundary nodes, like node_blocks', leaves a tile or two out."""
    n, rows, cols = torus9_pattern(30, 20, 6)
    return dominant(n, rows, cols, 49)


def band():
    """test_gpu_slab_mm's "band" (30,000 rows, 40 per row inside a half band of 2,000), square, with a diagonal."""
    import mspmv

    a = mspmv.CsrMatrix.synth_banded(30000, 30000 * 40, 2000, seed=3)
    rows = np.repeat(np.arange(a.num_rows, dtype=np.int64), np.diff(a.row_offsets))
    return dominant(a.num_rows, rows, a.column_indices, 46)


N_EASY = 400


def staggered():
    """blockdiag(E, convdiff(30, 31)), E = randdd(400, 6, seed 9) with 50 added to its diagonal: a column supported
    on E's rows converges in a few iterations, one on the stencil's rows in about fifty."""
    ro, ci, va = tb.randdd(N_EASY, 6, seed=9)
    va = va.copy()
    va[ci == np.repeat(np.arange(N_EASY), np.diff(ro))] += 50.0
    return blockdiag((ro, ci, va), tb.convdiff(30, 31))


N_2X2 = 300


def freeze2x2():
    """blockdiag(150 copies of [[-3, -2], [1, 2]], randdd()), n = 1,077 (see rhs("freeze2x2", ...))."""
    k = N_2X2 // 2
    ro = np.arange(0, 2 * N_2X2 + 1, 2, dtype=np.int32)
    ci = (np.repeat(np.arange(k) * 2, 4) + np.tile([0, 1, 0, 1], k)).astype(np.int32)
    return blockdiag((ro, ci, np.tile([-3.0, -2.0, 1.0, 2.0], k)), tb.randdd())


BUILDERS = {"windows": lambda: tb.convdiff(60, 47), "windows_rem": windows_rem, "long_rows": long_rows,
            "node_blocks": node_blocks, "node_blocks6": node_blocks6,
            "band": band, "staggered": staggered, "freeze2x2": freeze2x2}
NAMES = tuple(BUILDERS)
DOMINANT = ("windows_rem", "long_rows", "node_blocks", "node_blocks6", "band")


def build(name):
    """The named case, arrays read-only (test_bicgstab.matrix / test_ilu0.matrix cache it)."""
    a = BUILDERS[name]()
    for arr in a:
        arr.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def rhs(name, L):
    """The case's n x L right-hand side, read-only.  staggered: columns 0 and 2 supported on E's rows, 1 and 3 on
    the stencil's.  freeze2x2: column 0 is 1 on the 2 x 2 blocks' rows and 0 elsewhere -- in it every quantity of
    the first iteration is a small integer: alpha = -1, s = (-4, 4) per block, T = (4, 4), T.s = 0 with T.T != 0 so
    omega = 0, then rho' = 0 and beta = 0 (-1 / 0) is NaN, which freezes the column in the update pass with
    X = -1 on those rows; columns 1..3 (L = 4) are U(0, 1) on randdd's rows and 0 on the blocks'."""
    n = len(tb.matrix(name)[0]) - 1
    if name == "staggered":
        assert L == 4
        B = np.random.default_rng(47).uniform(0, 1, (n, L))
        B[N_EASY:, [0, 2]] = 0.0
        B[:N_EASY, [1, 3]] = 0.0
    elif name == "freeze2x2":
        assert L in (1, 4)
        B = np.random.default_rng(48).uniform(0, 1, (n, L))
        B[:N_2X2, :] = 0.0
        B[:, 0] = 0.0
        B[:N_2X2, 0] = 1.0
    else:
        B = tb.rhs(n, L).copy()
    B.setflags(write=False)
    return B


def _frozen(ref):
    for run in ref.values():
        for arr in run:
            if isinstance(arr, np.ndarray):
                arr.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(name, L, max_iters=200):
    """test_bicgstab.reference with this file's right-hand sides: {order: (X, iters, hist, status, conv)}."""
    a = tb.matrix(name)
    return _frozen({o: tb.bicgstab_ref(a, rhs(name, L), max_iters, TOL, dot=o) for o in tb.ORDERS})


@functools.lru_cache(maxsize=None)
def ilu_reference(name, L, max_iters=200):
    """test_ilu0.reference with this file's right-hand sides: {variant: (X, iters, hist, status, conv)}."""
    import test_ilu0 as ti

    a = ti.matrix(name)
    return _frozen({v: ti.pbicgstab_ref(a, ti.apply_plans(name, v[1]), rhs(name, L), max_iters, TOL, dot=v[0])
                    for v in ti.VARIANTS})


@functools.lru_cache(maxsize=None)
def cond(name):
    """The 2-norm condition number of a case without the dominance margin (windows, staggered), computed once."""
    return float(np.linalg.cond(tb.dense(tb.matrix(name))))


@functools.lru_cache(maxsize=None)
def reference_order(name, L, ilu=False, max_iters=200):
    """The reference order's solve alone, {order: run}: all a GPU test needs of a case on which
    test_bicgstab_cases.py has pinned that the other orders stop at the same iteration and stay within 1e-13 of its
    history (the large cases; the others' solves cost as much again each)."""
    if ilu:
        import test_ilu0 as ti

        v = ti.VARIANTS[0]
        run = ti.pbicgstab_ref(ti.matrix(name), ti.apply_plans(name, v[1]), rhs(name, L), max_iters, TOL, dot=v[0])
        return _frozen({v: run})
    o = tb.ORDERS[0]
    return _frozen({o: tb.bicgstab_ref(tb.matrix(name), rhs(name, L), max_iters, TOL, dot=o)})


# ---- the bars of test_gpu_bicgstab_plans.py, kept here so that the CPU tests can hold a wrong solve to them ----
def residuals_inf(a, B, X):
    """||B - A X||_inf per column, in np.longdouble."""
    ro, ci, va = a
    AX = tb.csr_mm((ro, ci, va.astype(np.longdouble)), np.asarray(X, np.longdouble))
    return np.max(np.abs(np.asarray(B, np.longdouble) - AX), axis=0)


def rounding_bar(a, X_ref, it):
    """Per column, 10 it sqrt(longest row + n) 2^-53 max_i (|A| |X_ref|)_i: how far rounding may move X between
    two runs of the same recurrence on a matrix of dominance margin 1.  An iteration's products and dot products
    sum at most (longest row) and n terms; summed in another order, or fused, a sum of k terms moves by about
    sqrt(k) 2^-53 of the sum of its terms' magnitudes (the probabilistic rounding model; the worst case is k 2^-53
    and is not attained by a tree or a blocked sum).  Such an error in a product is an error of that size in the
    residual, ||A^-1||_inf <= 1 carries it into X undamped at worst, and the it iterations' errors add; 10 is the
    margin.  The restatement's own three orders differ by about 4e-16 in X on these matrices, four decades inside
    the bar (test_bicgstab_cases.py pins that), and a single hub-row entry wrong by 1e-6 of itself moves X by
    2e-11 .. 1e-10, a decade outside it -- which the residual and history bars all accept."""
    ro, ci, va = a
    scale = np.max(tb.csr_mm((ro, ci, np.abs(va)), np.abs(X_ref)), axis=0)
    return 10.0 * it * np.sqrt(float(np.diff(ro).max()) + len(ro) - 1) * 2.0 ** -53 * scale


def check_bars(label, a, B, refs, X, it, hist, st, cols=None, spread_history=False, cond=None):
    """A solve (X, it, hist, st) against refs = reference(...) or ilu_reference(...), whose first entry is the
    reference order.  Status 0; the iteration count within one of the restatement's orders; len(hist) == it; the
    history within 1e-10 of the reference's (spread_history: test_gpu_bicgstab.check_history's spread rule, for the
    stencil, whose own orders drift apart); per column a true residual <= 2 TOL and, for a matrix of dominance
    margin 1, |X - X_ref|_inf <= |B - A X|_inf + |B - A X_ref|_inf: A (X - X_ref) is the difference of the two
    residuals and ||A^-1||_inf <= 1.  That bound holds for any X whatever, so with it goes the bar that tells a
    slightly wrong product apart: |X - X_ref|_inf <= rounding_bar().  cond: the matrix has no such margin (the
    stencils); the X bar is then test_gpu_bicgstab's, |X - X_ref|_2 <= 2 TOL cond |X_ref|_2 per column.  cols: the
    columns the residual and X bars apply to (default all; status and counts are then the caller's).  Prints each
    figure before it asserts; returns (history deviation, true residual, x error over the rounding or cond bar)."""
    runs = list(refs.values())
    X_ref, _, h_ref = runs[0][0], runs[0][1], runs[0][2]
    counts = [r[1] for r in runs]
    k = min(len(hist), len(h_ref))
    err = np.abs(hist[:k] - h_ref[:k])
    if spread_history:
        spread = np.zeros(k)
        for r in runs[1:]:
            q = min(k, len(r[2]))
            spread[:q] = np.maximum(spread[:q], np.abs(r[2][:q] - h_ref[:q]))
        bar = 10.0 * np.maximum.accumulate(spread) + 64.0 * 2.0 ** -53 * h_ref.max()
    else:
        bar = np.full(k, 1e-10)
    sel = np.arange(B.shape[1]) if cols is None else np.asarray(cols)
    tr = tb.true_residual(a, B[:, sel], X[:, sel])
    res, res_ref = residuals_inf(a, B[:, sel], X[:, sel]), residuals_inf(a, B[:, sel], X_ref[:, sel])
    xerr = np.max(np.abs(X[:, sel].astype(np.longdouble) - X_ref[:, sel]), axis=0)
    hdev = float(err.max()) if k else 0.0
    hratio = float(np.max(err / bar)) if k else 0.0
    if cond is not None:
        x2 = np.linalg.norm(X[:, sel] - X_ref[:, sel], axis=0) / np.linalg.norm(X_ref[:, sel], axis=0)
        xratio = float(np.max(x2) / (2 * TOL * cond))
    else:
        xratio = float(np.max(xerr / np.maximum(res + res_ref, np.finfo(np.float64).tiny)))
        rbar = rounding_bar(a, X_ref[:, sel], runs[0][1])
        rratio = float(np.max(xerr / rbar))
    print(f"\n{label}: status {st}, iterations {it} (restatement {counts}), worst history deviation {hdev:.3e} "
          f"({hratio:.3g} of its bar), worst true residual {tr.max():.3e} (bar {2 * TOL:.1e}), worst |X - X_ref|_inf "
          f"{float(xerr.max()):.3e} = {xratio:.3g} of its bar"
          + ("" if cond is not None else f" and {rratio:.3g} of the rounding bar"))
    if cols is None:
        assert st == 0, f"status {st}"
        assert min(counts) - 1 <= it <= max(counts) + 1, f"iterations {it} against {counts}"
    assert len(hist) == it, f"history length {len(hist)} of {it} iterations"
    assert k > 0 and np.all(err <= bar), f"history deviation {hdev:.3e}, {hratio:.3g} of its bar"
    assert np.all(np.isfinite(X)) and np.all(tr <= 2 * TOL), f"true residual {tr.max():.3e}"
    if cond is not None:
        assert xratio <= 1.0, f"x error {xratio:.3g} of 2 TOL cond"
    else:
        assert np.all(xerr <= res + res_ref), f"x error {float(xerr.max()):.3e}, {xratio:.3g} of the residuals' sum"
        assert np.all(xerr <= rbar), f"x error {float(xerr.max()):.3e}, {rratio:.3g} of the rounding bar"
    return hdev, float(tr.max()), xratio if cond is not None else rratio
