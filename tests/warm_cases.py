"""Systems and numpy restatements for the warm start (mspmv_set_initial_guess) and the fused true residual
(mspmv_dresidual): test_warm_cases.py (CPU), test_gpu_warm_start.py.

Exact-product systems.  One per product path of launch_solver_product, on the patterns of the existing builders:

  windows      bicgstab_cases._offsets_pattern, six offsets on 44 windows of 64 rows and one of 13 (n = 2,829)
  node_blocks  bicgstab_cases.kron9_pattern(25, 20, 8): dense 8 x 8 node blocks, 72 columns per interior row (n = 4,000)
  long_rows    bicgstab_cases.long_rows' pattern: five offsets and three hub rows of 3,000 columns, which every
               width's merge tiles split (n = 8,000)
  band         bicgstab_cases.band's pattern, 40 per row inside a half band of 2,000 (n = 30,000: the smallest the
               column-slab SpMM's plan has been built on)

each closed under transposition.  Off-diagonal values are nonzero multiples of 1/64 in [-1, 1] -- one per unordered
pair (sym, for the CG families) or one per entry (for the BiCGSTABs) -- and the diagonal is sum |off-diagonal| + 1, so
the matrix is strictly diagonally dominant with a positive diagonal.  X0 has integer entries in [-8, 8] and
B = A X0 + E with E = +-1/64: every product a_ij x0_j and every partial sum of a row is a multiple of 1/64 far below
2^53 / 64, so A X0 and R0 = B - A X0 = E are exact in every summation order, and the host and every kernel hold the
same R0 bits.  ||B|| / ||R0|| = 64 rms(A X0) is in the thousands: a stop test normalised by the wrong norm shows.

Restatements.  cg_warm and bicgstab_warm are the lock-step multi-RHS recurrences continued from X0 with b_norm from B
and the entry test, in float64, every statement one rounding (no fused multiply-add), so that with the same inputs they
repeat bit for bit.
"""
import functools

import numpy as np

import bicgstab_cases as bc
import test_bicgstab as tb

CASES = ("windows", "node_blocks", "long_rows", "band")
WIDTHS = (1, 4, 16, 3)  # 3: through the column groups (2 + 1)
K = 8                   # iterations of the shift identity
LD = np.longdouble


def _band_pattern():
    import mspmv

    a = mspmv.CsrMatrix.synth_banded(30000, 30000 * 40, 2000, seed=3)
    rows = np.repeat(np.arange(a.num_rows, dtype=np.int64), np.diff(a.row_offsets.astype(np.int64)))
    return a.num_rows, rows, a.column_indices.astype(np.int64)


def _long_rows_pattern(n=8000, per_hub=3000):
    rows, cols = bc._offsets_pattern(n, (1, 2, 7, -3, -40))
    rng = np.random.default_rng(43)
    hub_cols = [rng.choice(n, per_hub, replace=False) for _ in bc.HUBS]
    rows = np.concatenate([rows] + [np.full(per_hub, h, np.int64) for h in bc.HUBS])
    return n, rows, np.concatenate([cols] + hub_cols)


def _windows_pattern():
    n = 64 * 44 + 13
    return (n,) + bc._offsets_pattern(n, (-70, -3, 0, 2, 9, 70))


PATTERNS = {"windows": _windows_pattern, "node_blocks": lambda: bc.kron9_pattern(25, 20, 8),
            "long_rows": _long_rows_pattern, "band": _band_pattern}


def exact_matrix(n, rows, cols, seed, sym):
    """The value rule of the module docstring on the symmetric closure of the pattern {(rows, cols)}: CSR arrays."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    key = np.unique(lo[lo != hi] * n + hi[lo != hi])
    lo, hi = key // n, key % n
    rng = np.random.default_rng(seed)

    def draw():
        return rng.choice(np.concatenate([np.arange(-64, 0), np.arange(1, 65)]), key.size) / 64.0

    v_up = draw()
    v_dn = v_up if sym else draw()
    diag = np.bincount(lo, np.abs(v_up), n) + np.bincount(hi, np.abs(v_dn), n) + 1.0
    d = np.arange(n, dtype=np.int64)
    return bc._csr(n, np.concatenate([lo, hi, d]), np.concatenate([hi, lo, d]), np.concatenate([v_up, v_dn, diag]))


@functools.lru_cache(maxsize=None)
def system(name, sym=True):
    """(row_offsets, column_indices, values) of the named case, read-only, built once."""
    n, rows, cols = PATTERNS[name]()
    a = exact_matrix(n, rows, cols, 80 + CASES.index(name), sym)
    for arr in a:
        arr.setflags(write=False)
    return a


def csr(a):
    import mspmv

    ro, ci, va = a
    return mspmv.CsrMatrix.from_arrays(len(ro) - 1, ro, ci, va)


def csr_mm(a, X, dtype=np.float64):
    """A X by row segment sums (test_bicgstab.csr_mm), in `dtype`."""
    ro, ci, va = a
    return tb.csr_mm((ro, ci, va.astype(dtype)), np.asarray(X, dtype))


def _readonly(*arrs):
    for arr in arrs:
        arr.setflags(write=False)
    return arrs if len(arrs) > 1 else arrs[0]


@functools.lru_cache(maxsize=None)
def guess(name, L):
    """X0: integers in [-8, 8], n x L, read-only."""
    n = len(system(name)[0]) - 1
    return _readonly(np.random.default_rng(90 + 7 * L + CASES.index(name)).integers(-8, 9, (n, L)).astype(np.float64))


@functools.lru_cache(maxsize=None)
def exact_rhs(name, sym, L):
    """(B*, B): B* = A X0 exactly (X0 solves it: the converged-at-entry cases) and B = B* + E, E = +-1/64."""
    X0 = guess(name, L)
    Bs = csr_mm(system(name, sym), X0)
    E = np.random.default_rng(91 + 7 * L + CASES.index(name)).choice([-1.0, 1.0], X0.shape) / 64.0
    return _readonly(Bs, Bs + E)


def rhs(name, sym, L):
    return exact_rhs(name, sym, L)[1]


@functools.lru_cache(maxsize=None)
def residual0(name, sym, L):
    """R0 = B - A X0 as float64 computes it (exact: test_warm_cases.py), read-only."""
    return _readonly(rhs(name, sym, L) - csr_mm(system(name, sym), guess(name, L)))


@functools.lru_cache(maxsize=None)
def random_system(name, L, seed=5):
    """An inexact system on the case's matrix, for mspmv_dresidual: (B, X), U(-1, 1), read-only."""
    n = len(system(name)[0]) - 1
    rng = np.random.default_rng(seed + L + CASES.index(name))
    return _readonly(rng.uniform(-1, 1, (n, L)), rng.uniform(-1, 1, (n, L)))


def switches(name):
    """The plan switches a case's handle is created under, {variable: value or None (unset)}: the offset windows for
    `windows` alone, the column-slab SpMM for `band` alone, no slab SpMV (the single-RHS products stay on the tiles)."""
    return {"MSPMV_DIA": None if name == "windows" else "0", "MSPMV_SPMM_SLAB": "1" if name == "band" else "0",
            "MSPMV_SPMV_SLAB": "0"}


def col_norms(V):
    return np.sqrt(np.sum(np.asarray(V, LD) ** 2, axis=0)).astype(np.float64)


# ---- the bars of test_gpu_warm_start.py, kept here so that the CPU tests hold the restatements to them ---------------
def x_identity_bar(X0, D, adds_per_iteration=1):
    """(2 k + 2) 2^-52 (||X0||_inf + sum_i ||D_i - D_(i-1)||_inf), D = [D_0 = 0, D_1, .., D_k] the cold solves of
    (R0, 0) cut at i iterations: a warm solve of (B, X0) adds the same k updates to X0 that the cold one adds to 0,
    one rounding per addition in each run (BiCGSTAB makes two additions per iteration: adds_per_iteration = 2)."""
    k = len(D) - 1
    steps = sum(float(np.max(np.abs(D[i] - D[i - 1]))) for i in range(1, k + 1))
    return (2 * k * adds_per_iteration + 2) * 2.0 ** -52 * (float(np.max(np.abs(X0))) + steps)


def check_x_identity(label, Xw, X0, D, adds_per_iteration=1):
    bar = x_identity_bar(X0, D, adds_per_iteration)
    err = float(np.max(np.abs(Xw - (X0 + D[-1]))))
    print(f"{label}: ||X_warm - (X0 + D_k)||_inf = {err:.3e}, {err / bar:.3g} of its bar {bar:.3e}")
    assert np.all(np.isfinite(Xw)) and err <= bar, f"{label}: {err:.3e} over {bar:.3e}"
    return err / bar


def check_history_shift(label, n, hw, normB, hc, normR0):
    """hist_warm[i] ||B|| against hist_cold[i] ||R0||, (n + 8) 2^-53 relative: two sums of n squares in possibly
    different orders, a square root and a division."""
    assert len(hw) == len(hc) and len(hw) > 0, f"{label}: history lengths {len(hw)} and {len(hc)}"
    lhs, rhs_ = np.asarray(hw, LD) * LD(normB), np.asarray(hc, LD) * LD(normR0)
    rel = float(np.max(np.abs(lhs - rhs_) / np.abs(rhs_)))
    bar = (n + 8) * 2.0 ** -53
    print(f"{label}: hist_warm ||B|| against hist_cold ||R0||: {rel:.3e} relative, {rel / bar:.3g} of its bar {bar:.3e}")
    assert rel <= bar, f"{label}: {rel:.3e} over {bar:.3e}"
    return rel / bar


# ---- numpy restatements ----------------------------------------------------------------------------------------------
def _bnorm(B):
    bn = np.sqrt(np.sum(B * B, axis=0))
    return np.where(bn == 0.0, 1.0, bn)


def cg_warm(a, B, X0, max_iters, tol):
    """The lock-step multi-RHS CG (mspmv_dcg_multi) continued from X0: R0 = B - A X0, rs = R0.R0, b_norm from B, the
    entry test, then the cold recurrence.  Returns (X, iterations, history)."""
    X = np.array(X0, np.float64)
    R = B - csr_mm(a, X)
    bn = _bnorm(B)
    rs = np.sum(R * R, axis=0)
    conv = np.sqrt(rs) / bn < tol
    hist = []
    if conv.all():
        return X, 0, np.array(hist)
    P = R.copy()
    it = 0
    with np.errstate(invalid="ignore", divide="ignore"):
        while it < max_iters:
            AP = csr_mm(a, P)
            alpha = np.where(conv, 0.0, rs / np.sum(P * AP, axis=0))
            X = X + alpha * P
            R = R + (-alpha) * AP
            rs_new = np.sum(R * R, axis=0)
            rel = np.sqrt(rs_new) / bn
            hist.append(float(np.max(rel)))
            conv = conv | (rel < tol)
            it += 1
            if conv.all():
                break
            beta = np.where(conv, 0.0, rs_new / rs)
            rs = rs_new
            P = R + beta * P
    return X, it, np.array(hist)


def bicgstab_warm(a, B, X0, max_iters, tol):
    """The lock-step multi-RHS BiCGSTAB (mspmv_dbicgstab_multi) continued from X0: Rhat = P = R0, rho = R0.R0, b_norm
    from B, the entry test.  Returns (X, iterations, history)."""
    X = np.array(X0, np.float64)
    R = B - csr_mm(a, X)
    bn = _bnorm(B)
    rho = np.sum(R * R, axis=0)
    conv = np.sqrt(rho) / bn < tol
    hist = []
    if conv.all():
        return X, 0, np.array(hist)
    Rhat, P = R.copy(), R.copy()
    it = 0
    with np.errstate(invalid="ignore", divide="ignore"):
        while it < max_iters:
            V = csr_mm(a, P)
            alpha = np.where(conv, 0.0, rho / np.sum(Rhat * V, axis=0))
            S = R - alpha * V
            X = X + alpha * P
            T = csr_mm(a, S)
            tt = np.sum(T * T, axis=0)
            omega = np.where(conv | (tt == 0.0), 0.0, np.sum(T * S, axis=0) / np.where(tt == 0.0, 1.0, tt))
            X = X + omega * S
            R = S - omega * T
            rel = np.sqrt(np.sum(R * R, axis=0)) / bn
            hist.append(float(np.max(rel)))
            conv = conv | (rel < tol)
            it += 1
            if conv.all():
                break
            rho_new = np.sum(Rhat * R, axis=0)
            beta = np.where(conv, 0.0, (rho_new / rho) * (alpha / np.where(omega == 0.0, 1.0, omega)))
            rho = np.where(conv, rho, rho_new)
            P = np.where(conv, P, R + beta * (P - omega * V))
    return X, it, np.array(hist)


def stencil5_dyadic(nx, ny, seed, sym):
    """A 5-point stencil with dyadic entries: symmetric (-1, diagonal 4 + u) or convection-diffusion (-1 -+ 1/4 west /
    east, -1 -+ 1/8 south / north, diagonal 4 + u), u a multiple of 1/8 in [1/8, 1]: strictly dominant, and exact on
    integer vectors."""
    n = nx * ny
    g = np.arange(n, dtype=np.int64).reshape(ny, nx)
    c, d = (0.0, 0.0) if sym else (0.25, 0.125)
    rows = [g.ravel(), g[:, 1:].ravel(), g[:, :-1].ravel(), g[1:].ravel(), g[:-1].ravel()]
    cols = [g.ravel(), g[:, :-1].ravel(), g[:, 1:].ravel(), g[:-1].ravel(), g[1:].ravel()]
    u = np.random.default_rng(seed).integers(1, 9, n) / 8.0
    vals = [4.0 + u, np.full(rows[1].size, -1.0 - c), np.full(rows[2].size, -1.0 + c),
            np.full(rows[3].size, -1.0 - d), np.full(rows[4].size, -1.0 + d)]
    return bc._csr(n, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))
