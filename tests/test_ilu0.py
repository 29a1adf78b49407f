"""ILU(0) and the ILU(0)-preconditioned BiCGSTAB, pinned on the CPU: the numpy restatement of the
factorisation mspmv_ilu0_values runs (bit for bit), the factor identity A = L U on A's pattern checked
against nothing but A, the inputs the factorisation must refuse, and the restatement of the recurrence
mspmv_dpbicgstab_ilu0_multi runs (include/mspmv.h) with what the GPU tests (test_gpu_ilu0.py) rely on --
that on these inputs the iteration count depends neither on the summation order of the dot products nor on
the order a triangular-solve row is summed in, and that the stop means a true residual below the tolerance.

The recurrence, per column j of a row-major n x L panel, fp64, no fused multiply-adds, M = L U:

    X = 0; R = Rhat = P = B; bnorm_j = sqrt(B_j.B_j) (0 -> 1); rho_j = Rhat_j.R_j; conv_j = 0
    for it = 0 .. max_iters-1:
        Phat = U^-1 L^-1 P ; V = A Phat
        alpha_j = conv_j ? 0 : rho_j / (Rhat_j.V_j)
        R -= alpha V ; X += alpha Phat               # R now holds s
        Shat = U^-1 L^-1 R ; T = A Shat
        omega_j = conv_j ? 0 : (T_j.T_j == 0 ? 0 : T_j.R_j / T_j.T_j)
        X += omega Shat ; R -= omega T
        rel_j = sqrt(R_j.R_j)/bnorm_j ; hist[it] = max_j rel_j (broken columns left out)
        conv_j |= rel_j < tol ; all converged -> return it+1
        beta_j = conv_j ? 0 : (rho'_j/rho_j)(alpha_j/omega_j), rho'_j = Rhat_j.R_j ; rho_j = rho'_j (unconverged)
        P = R + beta (P - omega V)                   # unconverged columns only
    return max_iters

with test_bicgstab.bicgstab_ref's guard (a non-finite alpha, omega or beta freezes the column, status 4).
A triangular solve is substitution, x_i = (b_i - sum_j t_ij x_j) / t_ii, the row's products summed in CSR
order ("csr") or in reversed CSR order ("rev": the kernel folds a row in a tree, and this variant measures
how far a legitimate reordering of the solves moves the iterates).
"""
import ctypes
import functools

import numpy as np
import pytest

import ic0_cases
import mspmv
import test_bicgstab as tb
from test_bicgstab import TOL

INVALID, BREAKDOWN = 1, 4  # MSPMV_ERR_INVALID, MSPMV_ERR_BREAKDOWN
EPS = 2.0 ** -53


# ---- matrices ------------------------------------------------------------------------------------
def hubs_nonsym():
    """ic0_cases.hubs600's pattern (n = 600, rows / columns 200 and 599 dense) with every off-diagonal
    value scaled by its own factor in (0.5, 1.5) -- no longer symmetric -- and the diagonal reset to
    sum |off-diagonal| + 1: strictly row diagonally dominant, so ILU(0) exists."""
    n, ro, ci, va = ic0_cases.hubs600()
    rows = np.repeat(np.arange(n), np.diff(ro))
    off = ci != rows
    va = va.copy()
    va[off] *= 1.0 + 0.5 * np.random.default_rng(601).uniform(-1.0, 1.0, int(off.sum()))
    va[~off] = np.add.reduceat(np.where(off, np.abs(va), 0.0), ro[:-1].astype(np.int64)) + 1.0
    return ro, ci, va


@functools.lru_cache(maxsize=None)
def matrix(name):
    """(row_offsets, column_indices, values); built once per session, do not modify."""
    if name == "convdiff60s":  # the strongly convective one of the issue's table
        return tb.convdiff(60, 47, c=0.9, d=0.8)
    if name == "hubs":
        return hubs_nonsym()
    return tb.matrix(name)


def csr(a):
    ro, ci, va = a
    return mspmv.CsrMatrix.from_arrays(len(ro) - 1, ro, ci, va)


# ---- the factorisation, restated -------------------------------------------------------------------
def ilu0_ref(a):
    """IKJ ILU(0) in A's pattern, values in A's CSR order: python floats, one rounding per operation.
    Returns (lu, smallest |pivot|)."""
    ro, ci, va = a
    n = len(ro) - 1
    ro = [int(v) for v in ro]
    ci = [int(v) for v in ci]
    lu = [float(v) for v in va]
    diag = [0] * n
    for i in range(n):
        pos = {}
        for k in range(ro[i], ro[i + 1]):
            pos[ci[k]] = k
        diag[i] = pos[i]
        for ko in range(ro[i], diag[i]):
            k = ci[ko]
            l = lu[ko] / lu[diag[k]]
            lu[ko] = l
            for jo in range(diag[k] + 1, ro[k + 1]):
                p = pos.get(ci[jo])
                if p is not None:
                    lu[p] = lu[p] - l * lu[jo]
    lu = np.array(lu)
    return lu, float(np.abs(lu[diag]).min())


@functools.lru_cache(maxsize=None)
def factor(name):
    """mspmv.ilu0_values(matrix(name)), computed once (the GPU tests read it too); do not modify."""
    return mspmv.ilu0_values(csr(matrix(name)))


def triangles(a, lu):
    """(L, U) as mspmv.CsrMatrix: L the strictly lower entries with a unit diagonal last in the row, U the
    diagonal and the upper entries -- the two triangles mspmv_ilu0_create uploads."""
    ro, ci, _ = a
    n = len(ro) - 1
    rows = np.repeat(np.arange(n), np.diff(ro))
    low, up = ci < rows, ci >= rows
    lro = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows[low], minlength=n) + 1, out=lro[1:])
    lci = np.zeros(lro[-1], np.int32)
    lva = np.ones(lro[-1])
    dpos = lro[1:] - 1
    keep = np.ones(lro[-1], bool)
    keep[dpos] = False
    lci[dpos] = np.arange(n)
    lci[keep], lva[keep] = ci[low], lu[low]
    uro = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows[up], minlength=n), out=uro[1:])
    return (mspmv.CsrMatrix.from_arrays(n, lro.astype(np.int32), lci, lva),
            mspmv.CsrMatrix.from_arrays(n, uro.astype(np.int32), ci[up], lu[up]))


def factor_identity_ratio(a, lu):
    """max over A's pattern of |A - L U|_ij / (2 (k_ij + 2) 2^-53 (|L||U|)_ij), k_ij the number of products
    L_ik U_kj in the entry (k <= min(i, j), both factors on the pattern, L_ii = 1 included), both sides in
    np.longdouble.  The bound is the rounding bound of the defining recurrence: k_ij - 1 products and
    subtractions, then nothing (an entry of U) or one division (an entry of L)."""
    ro, ci, va = a
    n = len(ro) - 1
    ro = ro.astype(np.int64)
    v = lu.astype(np.longdouble)
    rows = np.repeat(np.arange(n), np.diff(ro))
    dpos = np.flatnonzero(ci == rows)
    tot, ab = np.zeros(n, np.longdouble), np.zeros(n, np.longdouble)
    cnt = np.zeros(n, np.int64)
    worst = 0.0
    for i in range(n):
        s, e = ro[i], ro[i + 1]
        # row i of L (unit diagonal included) times U: U_kj is on the pattern only for j >= k
        for k, lik in zip(np.append(ci[s:dpos[i]], i), np.append(v[s:dpos[i]], np.longdouble(1))):
            c = ci[dpos[k]:ro[k + 1]]
            t = lik * v[dpos[k]:ro[k + 1]]
            tot[c] += t
            ab[c] += np.abs(t)
            cnt[c] += 1
        c = ci[s:e]
        bound = 2 * (cnt[c] + 2) * np.longdouble(EPS) * ab[c]
        assert np.all(cnt[c] >= 1) and np.all(bound > 0)
        worst = max(worst, float(np.max(np.abs(tot[c] - va[s:e].astype(np.longdouble)) / bound)))
        tot[:], ab[:], cnt[:] = 0, 0, 0
    return worst


# ---- triangular solves by substitution, a level at a time -------------------------------------------
class TriPlan:
    """Substitution with a triangular CSR (mspmv.CsrMatrix, every diagonal present), rows grouped by
    dependency level so that a level is one vectorised step; a row's products are summed sequentially in
    CSR order, or in reversed CSR order (reverse)."""

    def __init__(self, t, lower, reverse):
        n = t.num_rows
        ro, ci, va = t.row_offsets.astype(np.int64), t.column_indices, t.values
        rows = np.repeat(np.arange(n), np.diff(ro))
        self.diag = va[ci == rows]
        assert self.diag.size == n
        lev = np.zeros(n, np.int64)
        entries = [None] * n
        for i in (range(n) if lower else range(n - 1, -1, -1)):
            k = np.arange(ro[i], ro[i + 1])
            k = k[ci[k] != i]
            entries[i] = k[::-1] if reverse else k
            if k.size:
                lev[i] = lev[ci[k]].max() + 1
        self.level0 = np.flatnonzero(lev == 0)
        self.levels = []
        for lv in range(1, int(lev.max()) + 1 if n else 0):
            r = np.flatnonzero(lev == lv)
            ks = np.concatenate([entries[i] for i in r])
            starts = np.zeros(r.size, np.int64)
            np.cumsum([entries[i].size for i in r[:-1]], out=starts[1:])
            self.levels.append((r, ci[ks], va[ks][:, None], starts))

    def solve(self, B):
        X = np.empty_like(B)
        X[self.level0] = B[self.level0] / self.diag[self.level0, None]
        for r, cols, vals, starts in self.levels:
            X[r] = (B[r] - np.add.reduceat(vals * X[cols], starts, axis=0)) / self.diag[r, None]
        return X


@functools.lru_cache(maxsize=None)
def apply_plans(name, solve_order):
    l, u = triangles(matrix(name), factor(name))
    rev = solve_order == "rev"
    return TriPlan(l, True, rev), TriPlan(u, False, rev)


# ---- the preconditioned recurrence, restated ---------------------------------------------------------
def pbicgstab_ref(a, plans, B, max_iters, tol, dot="fsum", guard=True):
    """The recurrence of this file's docstring: (X, iterations, history, status, conv).  tb.bicgstab_ref with
    the two applies; plans = (TriPlan of L, TriPlan of U)."""
    dotf = tb.DOTS[dot]
    pl, pu = plans
    B = np.asarray(B, np.float64)
    L = B.shape[1]
    X = np.zeros_like(B)
    R, Rh, P = B.copy(), B.copy(), B.copy()
    bb = dotf(B, B)
    bnorm = np.sqrt(bb)
    bnorm[bnorm == 0.0] = 1.0
    rho = bb.copy()
    conv = np.zeros(L, np.int64)
    rs_new = np.zeros(L)
    hist = []
    status = 0

    def freeze(q):
        nonlocal status
        bad = (conv == 0) & ~np.isfinite(q)
        if guard and bad.any():
            conv[bad] = 2
            status = 4
            return np.where(bad, 0.0, q), True
        return q, False

    def maxrel(rel, which):
        h = 0.0
        for j in np.flatnonzero(which):
            if rel[j] > h:
                h = rel[j]
        return h

    with np.errstate(all="ignore"):
        for it in range(max_iters):
            Ph = pu.solve(pl.solve(P))
            V = tb.csr_mm(a, Ph)
            alpha, froze = freeze(np.where(conv != 0, 0.0, rho / dotf(Rh, V)))
            if froze and not (conv == 0).any():
                hist.append(maxrel(np.sqrt(rs_new) / bnorm, conv == 1))
                return X, it + 1, np.array(hist), status, conv
            R = R - alpha * V
            X = X + alpha * Ph
            Sh = pu.solve(pl.solve(R))
            T = tb.csr_mm(a, Sh)
            tt, ts = dotf(T, T), dotf(T, R)
            omega, froze = freeze(np.where((conv != 0) | (tt == 0.0), 0.0, ts / tt))
            if froze and not (conv == 0).any():
                hist.append(maxrel(np.sqrt(rs_new) / bnorm, conv == 1))
                return X, it + 1, np.array(hist), status, conv
            X = X + omega * Sh
            R = R - omega * T
            rs_new, rho_new = dotf(R, R), dotf(Rh, R)
            rel = np.sqrt(rs_new) / bnorm
            hist.append(maxrel(rel, conv != 2))
            conv[(conv == 0) & (rel < tol)] = 1
            if (conv != 0).all():
                return X, it + 1, np.array(hist), status, conv
            beta, _ = freeze(np.where(conv != 0, 0.0, (rho_new / rho) * (alpha / omega)))
            live = conv == 0
            rho = np.where(live, rho_new, rho)
            if guard and not live.any():
                return X, it + 1, np.array(hist), status, conv
            P = np.where(live, R + beta * (P - omega * V), P)
    return X, max_iters, np.array(hist), status, conv


# (dot order, solve order); the first is the reference, the rest measure legitimate reorderings
VARIANTS = (("fsum", "csr"), ("einsum", "csr"), ("reversed", "csr"), ("fsum", "rev"))


@functools.lru_cache(maxsize=None)
def reference(name, L, max_iters=200):
    """The four variants' solves of matrix(name) with tb.rhs(n, L) at TOL: {variant: (X, iters, hist, status,
    conv)}.  Computed once and shared (the GPU tests read it too); callers leave the arrays unchanged."""
    a = matrix(name)
    B = tb.rhs(len(a[0]) - 1, L)
    return {v: pbicgstab_ref(a, apply_plans(name, v[1]), B, max_iters, TOL, dot=v[0]) for v in VARIANTS}


# ---- tests ---------------------------------------------------------------------------------------------
FACTOR_CASES = ["convdiff30", "randdd", "convdiff60s", "hubs"]
# smallest |pivot|: the issue's table; hubs: elimination keeps a row's dominance margin, here 1
MIN_PIVOT = {"convdiff30": 3.5, "randdd": 2.6, "convdiff60s": 3.8, "hubs": 1.0}


@pytest.mark.parametrize("name", FACTOR_CASES)
def test_ilu0_values_bitexact_with_restatement(name):
    a = matrix(name)
    lu = factor(name)
    ref, min_pivot = ilu0_ref(a)
    print(f"{name}: smallest pivot {min_pivot:.3f}")
    np.testing.assert_array_equal(lu.view(np.uint64), ref.view(np.uint64))
    assert min_pivot >= MIN_PIVOT[name]
    if name == "hubs":
        d = tb.dense(a)
        assert not np.array_equal(d, d.T) and np.array_equal(d != 0, (d != 0).T)
        assert int(np.diff(a[0]).max()) == 600  # a row as long as the matrix
        off = np.abs(d).sum(axis=1) - np.abs(np.diag(d))
        assert np.all(np.diag(d) > off)


@pytest.mark.parametrize("name", FACTOR_CASES)
def test_ilu0_factor_identity(name):
    """A = L U on A's pattern -- ILU(0)'s definition, checked against nothing but A:
    |A - L U|_ij <= 2 (k_ij + 2) 2^-53 (|L||U|)_ij for every (i, j) of the pattern, k_ij the number of
    products in the entry, both sides in long double.  The restatement meets the bound as stated (it is the
    library's values bit for bit), so the constant is not widened."""
    ratio = factor_identity_ratio(matrix(name), factor(name))
    print(f"{name}: worst |A - L U| / bound = {ratio:.3f}")
    assert ratio <= 1.0


def test_triangles_are_what_create_uploads():
    a = matrix("hubs")
    l, u = triangles(a, factor("hubs"))
    n = l.num_rows
    assert np.array_equal(l.column_indices[l.row_offsets[1:] - 1], np.arange(n))
    assert np.all(l.values[l.row_offsets[1:] - 1] == 1.0)
    assert np.array_equal(u.column_indices[u.row_offsets[:-1]], np.arange(n))
    assert l.num_nonzeros + u.num_nonzeros == len(a[1]) + n
    for t in (l, u):
        rows = ic0_cases.rows_of(t)
        same = rows[1:] == rows[:-1]
        assert np.all(np.diff(t.column_indices.astype(np.int64))[same] > 0)
    # L U restores A on the pattern to rounding (dense, float64: a sanity check of the split itself)
    d = tb.dense((l.row_offsets, l.column_indices, l.values)) @ tb.dense((u.row_offsets, u.column_indices, u.values))
    ad = tb.dense(a)
    assert np.max(np.abs(d - ad)[ad != 0]) <= 1e-12 * np.abs(ad).max()


def _broken(kind):
    """randdd with one defect in row 400."""
    ro, ci, va = (x.copy() for x in tb.matrix("randdd"))
    r = 400
    s, e = int(ro[r]), int(ro[r + 1])
    if kind == "unsorted":
        ci[s:e], va[s:e] = ci[s:e][::-1].copy(), va[s:e][::-1].copy()
    elif kind == "duplicate":
        ci, va = np.insert(ci, s, ci[s]), np.insert(va, s, va[s])
        ro[r + 1:] += 1
    elif kind == "no_diagonal":
        d = s + int(np.flatnonzero(ci[s:e] == r)[0])
        ci, va = np.delete(ci, d), np.delete(va, d)
        ro[r + 1:] -= 1
    return mspmv.CsrMatrix.from_arrays(777, ro, ci, va)


@pytest.mark.parametrize("kind", ["unsorted", "duplicate", "no_diagonal"])
def test_ilu0_values_rejects_rows_it_cannot_factor(kind):
    a = _broken(kind)
    with pytest.raises(mspmv.MspmvError, match=r"row 400\b") as e:
        mspmv.ilu0_values(a)
    assert e.value.status == INVALID
    with pytest.raises(mspmv.MspmvError, match=r"row 400\b") as e:  # create applies the same row checks
        mspmv.GpuIlu0(a)
    assert e.value.status == INVALID


def test_ilu0_values_rejects_non_square():
    a = mspmv.CsrMatrix.from_arrays(3, [0, 1, 2], [0, 1], [1.0, 1.0])
    for call in (mspmv.ilu0_values, mspmv.GpuIlu0):
        with pytest.raises(mspmv.MspmvError, match="square") as e:
            call(a)
        assert e.value.status == INVALID


def test_ilu0_zero_pivot_is_a_breakdown():
    """[[0, 1], [1, 0]] with its diagonal entries stored: row 0's pivot is 0, and nothing shifts it."""
    a = mspmv.CsrMatrix.from_arrays(2, [0, 2, 4], [0, 1, 0, 1], [0.0, 1.0, 1.0, 0.0])
    with pytest.raises(mspmv.MspmvError, match=r"row 0\b") as e:
        mspmv.ilu0_values(a)
    assert e.value.status == BREAKDOWN
    # a pivot that cancels during the elimination: row 1's becomes 1 - (1/1) 1 = 0
    a = mspmv.CsrMatrix.from_arrays(2, [0, 2, 4], [0, 1, 0, 1], [1.0, 1.0, 1.0, 1.0])
    with pytest.raises(mspmv.MspmvError, match=r"row 1\b") as e:
        mspmv.ilu0_values(a)
    assert e.value.status == BREAKDOWN
    a = mspmv.CsrMatrix.from_arrays(2, [0, 2, 4], [0, 1, 0, 1], [1.0, 1.0, 1.0, np.inf])
    with pytest.raises(mspmv.MspmvError, match=r"row 1\b") as e:
        mspmv.ilu0_values(a)
    assert e.value.status == BREAKDOWN


@pytest.mark.parametrize("bad", [0.0, np.nan, np.inf])
def test_ilu0_create_rejects_a_diagonal_no_solve_may_divide_by(bad):
    """Checked on the host before the device is touched: MSPMV_ERR_INVALID with or without a device."""
    lu = mspmv.CsrMatrix.from_arrays(3, [0, 2, 4, 6], [0, 1, 0, 1, 1, 2], [2.0, 1.0, 0.5, bad, 0.5, 2.0])
    with pytest.raises(mspmv.MspmvError, match=r"row 1\b.*diagonal") as e:
        mspmv.GpuIlu0(lu)
    assert e.value.status == INVALID


# The issue's table: iterations to TOL at L = 1 / 8, unpreconditioned and with ILU(0).
CASES = [(name, L) for name in ("convdiff30", "convdiff60", "randdd", "convdiff60s") for L in (1, 8, 6, 4)]
COUNTS = {("convdiff30", 1): 11, ("convdiff30", 8): 11, ("convdiff60", 1): 12, ("convdiff60", 8): 13,
          ("randdd", 1): 5, ("randdd", 8): 6, ("convdiff60s", 1): 6, ("convdiff60s", 8): 7}


@pytest.mark.parametrize("name,L", CASES)
def test_variants_agree_and_true_residual(name, L):
    """The three dot orders and the reversed triangular-solve order stop at the same iteration, at the counts
    measured when the inputs were chosen; every column's true residual is below the tolerance; and the
    preconditioned solve takes fewer iterations than the unpreconditioned one."""
    a = matrix(name)
    B = tb.rhs(len(a[0]) - 1, L)
    ref = reference(name, L)
    counts = [ref[v][1] for v in VARIANTS]
    print(f"{name} L={L}: iterations {counts}")
    assert len(set(counts)) == 1, (name, L, counts)
    if (name, L) in COUNTS:
        assert counts[0] == COUNTS[(name, L)], (name, L, counts)
    for v in VARIANTS:
        X, it, hist, st, conv = ref[v]
        assert st == 0 and np.all(conv == 1) and len(hist) == it
        tr = tb.true_residual(a, B, X)
        print(f"  {v}: worst true residual {tr.max():.3e}")
        assert np.all(tr <= 1e-9), (name, L, v, tr.max())
    if name == "convdiff60s":
        plain = tb.bicgstab_ref(a, B, 200, TOL)[1]
    else:
        plain = tb.reference(name, L)["fsum"][1]
    print(f"  unpreconditioned: {plain}")
    assert counts[0] < plain


def test_tri_plan_is_substitution():
    """The level-at-a-time solve is substitution: the componentwise residual bound of ic0_cases holds for
    both orders, and the two orders differ (the variant is not a no-op) on rows of several entries."""
    l, u = triangles(matrix("hubs"), factor("hubs"))
    B = np.random.default_rng(9).uniform(-1, 1, (l.num_rows, 3))
    for t, lower in ((l, True), (u, False)):
        xs = [TriPlan(t, lower, rev).solve(B) for rev in (False, True)]
        for X in xs:
            assert ic0_cases.solve_residual_ratio(t, X, B) <= 1.0
        assert not np.array_equal(xs[0], xs[1])


def test_abi_symbols():
    lib = ctypes.CDLL(tb.LIB)
    for name in ("mspmv_ilu0_values", "mspmv_ilu0_create", "mspmv_ilu0_destroy", "mspmv_ilu0_solve_dev",
                 "mspmv_dpbicgstab_ilu0_multi", "mspmv_dpbicgstab_ilu0_multi_dev"):
        assert hasattr(lib, name), name
    assert callable(mspmv.ILU0BiCGStabSolveMultiple) and callable(mspmv.pbicgstab_ilu0)
    assert hasattr(mspmv.GpuIlu0, "solve") and hasattr(mspmv.GpuIlu0, "solve_dev")
