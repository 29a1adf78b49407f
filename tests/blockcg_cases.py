"""Matrices, right-hand sides and numpy restatements for the block CG (mspmv_dbcg_multi, csrc/mspmv_blockcg.hip;
test_blockcg_cases.py, test_gpu_blockcg.py).  Numpy only, seeded, built once.

bcgrq() restates Dubrulle's BCGrQ recurrence with the library's own small-matrix arithmetic -- the Cholesky factor
row by row from the upper triangle, the factor's inverse by back substitution, every L x L and 1 x L by L x L
product with k ascending, a multiply and an add each -- so that what separates it from the GPU is the order of the
two Gram sums (and of the product's row sums) alone.  Those Gram sums come in two orders, ORDERS: "pairwise"
(np.add.reduce along the contiguous row axis) and "chunks" (chunks of 256 rows summed one after the other).  How far
the two runs drift apart is the rounding yardstick of the GPU tests, as bicgstab_cases.rounding_bar is BiCGSTAB's.
cg_lockstep() is the lock-step CG (L independent recurrences, each column frozen once it converges) the block
iteration counts are compared with.

CSR as (row_offsets int32, column_indices int32, values float64), columns ascending.  Cases (all SPD):
  laplacian    the 5-point Laplacian on a 48 x 47 grid (2,256 rows): takes the offset windows
  node_blocks  bicgstab_cases.kron9_pattern(20, 15, 6), 54 columns per interior row, values by sym_dominant()
  node_torus   bicgstab_cases.torus9_pattern(20, 15, 6): no boundary nodes, so every single-RHS tile is a register
               run tile and the L-wide products run k_spmm_blk (a grid with boundary nodes leaves a tile or two out)
  hubs         five offsets and three hub rows / columns of 1,500 entries on 4,000 rows: merge tiles, the hub rows
               split between them
  scaled       D A D for a 20 x 21 5-point stencil A of diagonal 6 and D = diag(10^U(-0.15, 0.15)).  The widest
               scaling that is still a yardstick: block CG amplifies rounding once some directions have converged
               ahead of others (H turns ill-conditioned), and on a badly scaled matrix the two orders' histories then
               part by 1e-3 relative within a third of the solve.  Candidates were judged on the CPU alone, by
               whether further Gram orders (chunks of 37, 64, 100 rows) meet the GPU test's history bar against the
               two orders: at 10^U(-3, 3) nothing converged within 2,000 iterations at L <= 8 and the two orders
               stopped 33 iterations apart at L = 16; at 10^U(-1, 1) they stopped 14 apart at L = 2; at 10^U(-0.5,
               0.5) (HARD, below: lock-step CG 145 iterations, block CG 35 at L = 16) they stop within one iteration
               at every width, but a third order misses the history bar by 2x at L = 8; at 10^U(-0.25, 0.25) still by
               6x .. 175x at L = 8.  At 10^U(-0.15, 0.15) every order stays within 0.03 of the bar at every width.
  HARD         ("scaled_hard", not among NAMES): the 10^U(-0.5, 0.5) form on the diagonal-4.5 stencil, for the bars that
               hold on a rounding-sensitive solve too (status, true residual)
"""
import functools

import numpy as np

import bicgstab_cases as bc

TOL = 1e-8
MAX_ITERS = 2000
ORDERS = ("pairwise", "chunks")
WIDTHS = (1, 2, 4, 8, 16)
BREAKDOWN = 4
CHUNK = 256


# ---- matrices ----------------------------------------------------------------------------------------------------
def stencil5(nx, ny, diag=4.0):
    g = np.arange(nx * ny, dtype=np.int64).reshape(ny, nx)
    rows = [g.ravel(), g[:, :-1].ravel(), g[:, 1:].ravel(), g[:-1].ravel(), g[1:].ravel()]
    cols = [g.ravel(), g[:, 1:].ravel(), g[:, :-1].ravel(), g[1:].ravel(), g[:-1].ravel()]
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return bc._csr(nx * ny, rows, cols, np.where(rows == cols, diag, -1.0))


def sym_dominant(n, rows, cols, seed):
    """The symmetric closure of the pattern {(rows, cols)}: one U(-1, 1) value per unordered pair, scaled by
    min(1, 8 / the longer of its two rows' off-diagonal counts), the diagonal sum |off-diagonal| + 1: symmetric and
    strictly diagonally dominant with a positive diagonal, so SPD (pcg_cases.sym_dominant's rule, in numpy alone)."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    key = np.unique(lo[lo != hi] * n + hi[lo != hi])
    lo, hi = key // n, key % n
    cnt = np.bincount(lo, minlength=n) + np.bincount(hi, minlength=n)
    v = np.random.default_rng(seed).uniform(-1.0, 1.0, key.size) * np.minimum(1.0, 8.0 / np.maximum(cnt[lo], cnt[hi]))
    diag = np.bincount(lo, np.abs(v), n) + np.bincount(hi, np.abs(v), n) + 1.0
    d = np.arange(n, dtype=np.int64)
    return bc._csr(n, np.concatenate([lo, hi, d]), np.concatenate([hi, lo, d]), np.concatenate([v, v, diag]))


HUBS = (5, 1500, 3000)


def hubs(n=4000, per_hub=1500):
    rows, cols = bc._offsets_pattern(n, (1, 2, 7, -3, -40))
    rng = np.random.default_rng(71)
    hub_cols = [rng.choice(n, per_hub, replace=False) for _ in HUBS]
    rows = np.concatenate([rows] + [np.full(per_hub, h, np.int64) for h in HUBS])
    return sym_dominant(n, rows, np.concatenate([cols] + hub_cols), 72)


def scaled(nx=20, ny=21, diag=6.0, spread=0.15):
    ro, ci, va = stencil5(nx, ny, diag=diag)
    d = 10.0 ** np.random.default_rng(73).uniform(-spread, spread, nx * ny)
    r = np.repeat(np.arange(nx * ny), np.diff(ro))
    return ro, ci, d[r] * va * d[ci]


BUILDERS = {
    "laplacian": lambda: stencil5(48, 47),
    "node_blocks": lambda: sym_dominant(*bc.kron9_pattern(20, 15, 6), 74),
    "node_torus": lambda: sym_dominant(*bc.torus9_pattern(20, 15, 6), 75),
    "hubs": hubs,
    "scaled": scaled,
}
NAMES = tuple(BUILDERS)
HARD = "scaled_hard"
BUILDERS[HARD] = lambda: scaled(diag=4.5, spread=0.5)


@functools.lru_cache(maxsize=None)
def matrix(name):
    a = BUILDERS[name]()
    for arr in a:
        arr.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def rhs_n(n, L, seed=7):
    B = np.random.default_rng(seed + 100 * L + n).uniform(0.0, 1.0, (n, L))
    B.setflags(write=False)
    return B


def rhs(name, L):
    return rhs_n(len(matrix(name)[0]) - 1, L)


# ---- arithmetic --------------------------------------------------------------------------------------------------
def csr_mm(a, X):
    """A X, each row's products summed by np.add.reduceat (every row of every case holds its diagonal)."""
    ro, ci, va = a
    return np.add.reduceat(va[:, None] * X[ci], ro[:-1].astype(np.int64), axis=0)


def gram(U, V, order):
    """U^T V, the sums over the rows in the named order ("pairwise", "chunks", or a chunk length)."""
    P = np.ascontiguousarray(U.T)[:, None, :] * np.ascontiguousarray(V.T)[None, :, :]  # [L][L][n]
    if order == "pairwise":
        return np.add.reduce(P, axis=-1)
    chunk = CHUNK if order == "chunks" else int(order)  # (further orders, for test_blockcg_cases: chunks of `order` rows)
    acc = np.zeros(P.shape[:2])
    for c in range(0, P.shape[2], chunk):
        acc = acc + np.add.reduce(P[:, :, c:c + chunk], axis=-1)
    return acc


def chol_upper(G):
    """(zeta, pivot): the upper factor of G = zeta^T zeta from G's upper triangle, row k as G[k][q] - sum_{p<k}
    zeta[p][k] zeta[p][q] with p ascending; pivot: the first one <= 0 or non-finite (zeta is then None), else -1."""
    L = G.shape[0]
    U = np.zeros((L, L))
    for k in range(L):
        s = G[k, k:].copy()
        for p in range(k):
            s = s - U[p, k] * U[p, k:]
        if not (s[0] > 0.0 and s[0] < np.inf):
            return None, k
        r = np.sqrt(s[0])
        U[k, k:] = s / r
        U[k, k] = r
    return U, -1


def upper_inverse(U):
    """U^-1 by back substitution per column: x_i = -(sum_{k>i} U[i][k] x_k) / U[i][i], k ascending."""
    L = U.shape[0]
    inv = np.zeros((L, L))
    for i in range(L - 1, -1, -1):
        if i + 1 < L:
            s = U[i, i + 1] * inv[i + 1, :]
            for k in range(i + 2, L):
                s = s + U[i, k] * inv[k, :]
            inv[i, i + 1:] = -s[i + 1:] / U[i, i]
        inv[i, i] = 1.0 / U[i, i]
    return inv


def mm(A, B):
    """A B with k ascending from the k = 0 product, a multiply and an add each (A: n x L or L x L, B: L x L)."""
    s = A[:, [0]] * B[[0], :]
    for k in range(1, B.shape[0]):
        s = s + A[:, [k]] * B[[k], :]
    return s


def col_norms(C):
    s = C[0] * C[0]
    for p in range(1, C.shape[0]):
        s = s + C[p] * C[p]
    return np.sqrt(s)


def bcgrq(a, B, tol, max_iters, order):
    """(X, iterations, history, status, (matrix, pivot)): the recurrence of include/mspmv.h's mspmv_dbcg_multi.
    status BREAKDOWN with X the iterate of the last completed iteration when a pivot of H or G fails."""
    B = np.asarray(B, np.float64)
    n, L = B.shape
    X = np.zeros((n, L))
    hist = []
    zeta, piv = chol_upper(gram(B, B, order))
    if piv >= 0:
        return X, 0, np.array(hist), BREAKDOWN, ("H", piv)
    C = zeta
    bnorm = col_norms(C)
    bnorm[bnorm == 0.0] = 1.0
    W = mm(B, upper_inverse(zeta))
    S = W
    for k in range(max_iters):
        Q = csr_mm(a, S)
        gamma, piv = chol_upper(gram(S, Q, order))
        if piv >= 0:
            return X, k, np.array(hist), BREAKDOWN, ("G", piv)
        ginv = upper_inverse(gamma)
        xi = mm(ginv, ginv.T.copy())
        X = X + mm(S, mm(xi, C))
        V = W - mm(Q, xi)
        H = gram(V, V, order)
        zeta, piv = chol_upper(H)
        if piv >= 0:
            Hs = np.triu(H) + np.triu(H, 1).T
            HC = mm(Hs, C)
            s = C[0] * HC[0]
            for p in range(1, L):
                s = s + C[p] * HC[p]
            with np.errstate(invalid="ignore"):
                hist.append(np.nanmax(np.sqrt(s) / bnorm))
            return X, k + 1, np.array(hist), BREAKDOWN, ("H", piv)
        C = mm(zeta, C)
        rel = col_norms(C) / bnorm
        hist.append(rel.max())
        if np.all(rel < tol):
            return X, k + 1, np.array(hist), 0, None
        W = mm(V, upper_inverse(zeta))
        S = W + mm(S, zeta.T.copy())
    return X, max_iters, np.array(hist), 0, None


def cg_lockstep(a, B, tol, max_iters):
    """(X, iterations, history): L independent CG recurrences in lock step, a column frozen once
    sqrt(r.r) / ||b|| < tol; the count is the last column's."""
    B = np.asarray(B, np.float64)
    X = np.zeros_like(B)
    R = B.copy()
    P = B.copy()
    rs = np.sum(R * R, axis=0)
    bnorm = np.sqrt(rs)
    bnorm[bnorm == 0.0] = 1.0
    live = np.ones(B.shape[1], bool)
    hist = []
    for k in range(max_iters):
        AP = csr_mm(a, P)
        alpha = np.where(live, rs / np.where(live, np.sum(P * AP, axis=0), 1.0), 0.0)
        X = X + alpha * P
        R = R - alpha * AP
        rs_new = np.sum(R * R, axis=0)
        rel = np.sqrt(rs_new) / bnorm
        hist.append(rel.max())
        live = live & ~(rel < tol)
        if not live.any():
            return X, k + 1, np.array(hist)
        P = R + (rs_new / rs) * P
        rs = rs_new
    return X, max_iters, np.array(hist)


def true_residual(a, B, X):
    """||B_j - A X_j||_2 / ||B_j||_2 per column, in np.longdouble."""
    ro, ci, va = a
    LD = np.longdouble
    AX = np.add.reduceat(va.astype(LD)[:, None] * np.asarray(X, LD)[ci], ro[:-1].astype(np.int64), axis=0)
    R = np.asarray(B, LD) - AX
    bn = np.sqrt(np.sum(np.asarray(B, LD) ** 2, axis=0))
    return (np.sqrt(np.sum(R * R, axis=0)) / np.where(bn == 0, 1, bn)).astype(np.float64)


def _frozen(run):
    for arr in run:
        if isinstance(arr, np.ndarray):
            arr.setflags(write=False)
    return run


@functools.lru_cache(maxsize=None)
def reference_n(key, L, max_iters=MAX_ITERS):
    """{order: bcgrq(...)} for system(key, L) -- a named case or ("chain", n); computed once, read-only."""
    a, B = system(key, L)
    return {o: _frozen(bcgrq(a, B, TOL, max_iters, o)) for o in ORDERS}


def reference(name, L, max_iters=MAX_ITERS):
    return reference_n(name, L, max_iters)


@functools.lru_cache(maxsize=None)
def lockstep(name, L):
    a, B = system(name, L)
    return _frozen(cg_lockstep(a, B, TOL, MAX_ITERS))


def chain(n):
    """tridiag(-1, 16, -1) on n rows: so well conditioned that 129 rows converge at L = 16 before the 8 iterations
    that exhaust the block Krylov space (a singular H: breakdown).  n = 1: the 1 x 1 matrix 16, on which every
    quantity is a power of two times b."""
    rows, cols = bc._offsets_pattern(n, (-1, 0, 1))
    return bc._csr(n, rows, cols, np.where(rows == cols, 16.0, -1.0))


@functools.lru_cache(maxsize=None)
def system(key, L):
    """(matrix, right-hand side) of a named case, or of ("chain", n)."""
    if isinstance(key, tuple):
        a = chain(key[1])
        for arr in a:
            arr.setflags(write=False)
        return a, rhs_n(key[1], L)
    return matrix(key), rhs(key, L)


def spread(refs):
    """(counts, history prefix length, |h_a - h_b| over it): the two orders' iteration counts, and the prefix of
    their histories over which they agree to 1e-3 relative."""
    (_, ia, ha, _, _), (_, ib, hb, _, _) = (refs[o] for o in ORDERS)
    k = min(len(ha), len(hb))
    diff = np.abs(ha[:k] - hb[:k])
    off = np.nonzero(diff > 1e-3 * np.maximum(np.abs(ha[:k]), np.abs(hb[:k])))[0]
    k = int(off[0]) if off.size else k
    return (ia, ib), k, diff[:k]
