"""Matrices, preconditioners and reference arithmetic that take SPAI-PCG and IC(0)-PCG (launch_pcg_init,
launch_pcg_iteration, launch_pcg_ic0_iteration: csrc/mspmv_cg_passes.hip) onto every dot-mode form of the tile
kernels and into the per-column freezes of their folds (test_pcg_cases.py, test_gpu_pcg_forms.py).

Every matrix is symmetric and strictly row diagonally dominant with a positive diagonal, so SPD; each is the
smallest that still shows its form; all are generated, seeded and built once.

  long_rows          test_gpu_split_rows.spd_with_long_rows(): 20,000 rows of 7 and three hub rows / columns of
                     6,000, far over a tile's snap distance at every width (tiles hold 2,048 / 1,024 / 1,536 / 1,024
                     merge items at L = 1 / 4 / 8 / 16, tile_items_for, and a row longer than an eighth of that is
                     split between tiles)
  many_tiles         a 3-D 7-point stencil, diagonal 6.5: 26^3 rows at L = 1 (67 tiles of 2,048 items) and 22^3 at
                     L = 4 (81 tiles of 1,024 items; 26^3 would make 134, past the 65..127 of a two-block fold):
                     k_fold_dot then runs two blocks, the second one short
  dict16             a chain of 1,000 nodes of 6 unknowns, each coupled to the nodes 1 and 3 away on either side (30
                     columns per row; IC(0) drops the fill between them, so it is not the exact factor): at L = 16 a
                     1,024-item tile holds about 70 distinct columns, under the 128 of a column dictionary, and 30
                     columns are too few for node blocks.  (The matrix of test_spmm16_column_dictionary_tiles has an unsymmetric
                     pattern, and its symmetric closure is 42 columns wide, which takes node blocks instead.)
  node_blocks6       bicgstab_cases.torus9_pattern(30, 20, 6): 54 columns in every row, every single-RHS tile a
                     register run tile, so the products run k_spmv_blk<kModeDot> and k_spmm_blk<L, kModeDot, NT, 6>
  node_blocks_mixed  the same torus, 40 x 30 nodes, with two hub rows / columns of 1,500 entries whose columns lie
                     in the first third of the matrix: tiles of the other two thirds keep their node blocks, the hub
                     rows are split between tiles (test_gpu_blocks.fem_with_long_rows replaces rows only, which is
                     not symmetric: this is its symmetric form)
  staggered          blockdiag(E, a 30 x 31 5-point stencil of diagonal 4.02), E 400 rows of 6 random columns with
                     50 added to the diagonal: a column supported on E's rows converges in a few iterations, one on
                     the stencil's rows dozens later

There is no node_blocks8: k_build_blocks closes a run after kBlkRunRows = 6 rows whatever the node size, so
TilePlan::blk_rows_max never exceeds 6 and launch_spmm_L never takes k_spmm_blk<L, MODE, NT> without the 6 -- no
matrix reaches that instantiation.

Preconditioners for SPAI-PCG (any SPD M of A's shape): mspmv.spai_values on the stencil, chain and node-block cases;
on the hub cases, where its dense least squares per column is ruinous, "neumann" M = D^-1 (2 D - A) D^-1 on A's
pattern (SPD, 2 D - A being strictly dominant, and with split rows of its own); and on many_tiles two more on other
patterns, "jacobi" M = D^-1 (a fraction of A's tiles) and "wide", a seeded band of 14 off-diagonals of magnitude
<= 0.03 beside a unit diagonal (more than twice A's tiles).  IC(0)-PCG takes mspmv.ic0_factor of the case's A.

The reference arithmetic is np.longdouble over the CSR arrays: pcg_reference restates SPAISolveMultiple and
PCGSolveMultiple with their guards (oracle/mspmv_oracle.c orc_pcg_spai_multi, orc_pcg_ic0_multi), one_iteration gives
the first iteration's Z, alpha and the rounding bound the GPU's X = alpha Z must meet.
"""
import functools

import numpy as np

import bicgstab_cases as bc

EPS = 2.0 ** -53
TOL = 1e-9
MAX_ITERS = 400
LD = np.longdouble

# case -> widths (the table of the module docstring); (case, preconditioner) pairs of the SPAI-PCG
WIDTHS = {"long_rows": (1, 4, 16), "many_tiles": (1, 4), "dict16": (16,), "node_blocks6": (1, 8),
          "node_blocks_mixed": (1, 8), "staggered": (4,)}
SPAI_KIND = {"long_rows": "neumann", "many_tiles": "spai", "dict16": "spai", "node_blocks6": "spai",
             "node_blocks_mixed": "neumann", "staggered": "spai"}
OFF_PATTERN = ("jacobi", "wide")  # on many_tiles only: M's pattern is not A's, the oracle cannot take it
HUBS = {"long_rows": (5, 9000, 15000), "node_blocks_mixed": (3000, 5001)}
HUB_LEN = {"long_rows": 6000, "node_blocks_mixed": 1500}
N_EASY = 400
MANY_SIDE = {1: 26, 4: 22}


def solves():
    """Every (case, L, kind) the GPU tests run: kind "ic0", or the SPAI-PCG's preconditioner."""
    out = []
    for name, widths in WIDTHS.items():
        for L in widths:
            out.append((name, L, SPAI_KIND[name]))
            out.append((name, L, "ic0"))
            if name == "many_tiles":
                out += [(name, L, k) for k in OFF_PATTERN]
    return out


# ---- matrices ----------------------------------------------------------------------------------------------------
def _csr_matrix(n, ro, ci, va):
    import mspmv

    for arr in (ro, ci, va):
        arr.setflags(write=False)
    return mspmv.CsrMatrix.from_arrays(n, ro, ci, va)


def sym_dominant(n, rows, cols, seed):
    """The symmetric closure of the pattern {(rows, cols)}: one U(-1, 1) value per unordered pair, scaled by
    min(1, 8 / the longer of its two rows' off-diagonal counts) so that a hub row's sum stays near 4, the diagonal
    sum |off-diagonal| + 1 (bicgstab_cases.dominant's rule, made symmetric)."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    key = np.unique(lo[lo != hi] * n + hi[lo != hi])
    lo, hi = key // n, key % n
    cnt = np.bincount(lo, minlength=n) + np.bincount(hi, minlength=n)
    v = np.random.default_rng(seed).uniform(-1.0, 1.0, key.size) * np.minimum(1.0, 8.0 / np.maximum(cnt[lo], cnt[hi]))
    diag = np.bincount(lo, np.abs(v), n) + np.bincount(hi, np.abs(v), n) + 1.0
    d = np.arange(n, dtype=np.int64)
    ro, ci, va = bc._csr(n, np.concatenate([lo, hi, d]), np.concatenate([hi, lo, d]), np.concatenate([v, v, diag]))
    return _csr_matrix(n, ro, ci, va)


def stencil7(side, diag=6.5):
    n = side ** 3
    idx = np.arange(n, dtype=np.int64).reshape(side, side, side)
    rows, cols = [np.arange(n, dtype=np.int64)], [np.arange(n, dtype=np.int64)]
    for ax in range(3):
        a = np.take(idx, np.arange(side - 1), axis=ax).ravel()
        b = np.take(idx, np.arange(1, side), axis=ax).ravel()
        rows += [a, b]
        cols += [b, a]
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    ro, ci, va = bc._csr(n, rows, cols, np.where(rows == cols, diag, -1.0))
    return _csr_matrix(n, ro, ci, va)


def node_chain(nodes=1000, dof=6, reach=(0, 1, 3), seed=61):
    k = np.arange(dof, dtype=np.int64)
    rows, cols = [], []
    for d in reach:
        a = np.arange(nodes - d, dtype=np.int64)
        rows.append((np.repeat(a * dof, dof * dof) + np.tile(np.repeat(k, dof), a.size)))
        cols.append((np.repeat((a + d) * dof, dof * dof) + np.tile(np.tile(k, dof), a.size)))
    return sym_dominant(nodes * dof, np.concatenate(rows), np.concatenate(cols), seed)


def node_blocks_mixed():
    n, rows, cols = bc.torus9_pattern(40, 30, 6)
    rng = np.random.default_rng(63)
    for h in HUBS["node_blocks_mixed"]:
        c = rng.choice(n // 3, HUB_LEN["node_blocks_mixed"], replace=False)
        rows = np.concatenate([rows, np.full(c.size, h, np.int64)])
        cols = np.concatenate([cols, c])
    return sym_dominant(n, rows, cols, 64)


def staggered():
    import test_bicgstab as tb

    ro, ci, _ = tb.randdd(N_EASY, 6, seed=9)
    er = np.repeat(np.arange(N_EASY, dtype=np.int64), np.diff(ro))
    e = sym_dominant(N_EASY, er, ci, 65)
    ev = e.values.copy()
    ev[e.column_indices == np.repeat(np.arange(N_EASY), np.diff(e.row_offsets))] += 50.0
    nx, ny = 30, 31
    g = np.arange(nx * ny, dtype=np.int64).reshape(ny, nx)
    rows = [g.ravel(), g[:, :-1].ravel(), g[:, 1:].ravel(), g[:-1].ravel(), g[1:].ravel()]
    cols = [g.ravel(), g[:, 1:].ravel(), g[:, :-1].ravel(), g[1:].ravel(), g[:-1].ravel()]
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    s = bc._csr(nx * ny, rows, cols, np.where(rows == cols, 4.02, -1.0))
    ro, ci, va = bc.blockdiag((e.row_offsets, e.column_indices, ev), s)
    return _csr_matrix(N_EASY + nx * ny, ro, ci, va.copy())


@functools.lru_cache(maxsize=None)
def matrix(name, L=1):
    """The named case as an mspmv.CsrMatrix (L matters to many_tiles alone); built once, read-only."""
    if name == "many_tiles":
        return _many_tiles(MANY_SIDE[L])
    return _matrix(name)


@functools.lru_cache(maxsize=None)
def _many_tiles(side):
    return stencil7(side)


@functools.lru_cache(maxsize=None)
def _matrix(name):
    if name == "long_rows":
        import test_gpu_split_rows as tsr

        a = tsr.spd_with_long_rows()
        return _csr_matrix(a.num_cols, a.row_offsets, a.column_indices, a.values)
    if name == "dict16":
        return node_chain()
    if name == "node_blocks6":
        n, rows, cols = bc.torus9_pattern(30, 20, 6)
        return sym_dominant(n, rows, cols, 62)
    if name == "node_blocks_mixed":
        return node_blocks_mixed()
    if name == "staggered":
        return staggered()
    raise KeyError(name)


def rows_of(a):
    return np.repeat(np.arange(a.num_rows, dtype=np.int64), np.diff(a.row_offsets.astype(np.int64)))


def diagonal(a):
    d = np.zeros(a.num_rows)
    on = rows_of(a) == a.column_indices
    d[a.column_indices[on]] = a.values[on]
    return d


# ---- preconditioners ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def preconditioner(name, L, kind):
    """M of SPAI-PCG as an mspmv.CsrMatrix: "spai" and "neumann" on A's pattern, "jacobi" and "wide" on their own."""
    import mspmv

    a = matrix(name, L)
    n, d = a.num_rows, diagonal(matrix(name, L))
    if kind == "spai":
        return _csr_matrix(n, a.row_offsets, a.column_indices, mspmv.spai_values(a))
    if kind == "neumann":
        r = rows_of(a)
        off = -a.values / (d[r] * d[a.column_indices])
        return _csr_matrix(n, a.row_offsets, a.column_indices, np.where(r == a.column_indices, 1.0 / d[r], off))
    if kind == "jacobi":
        return _csr_matrix(n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), 1.0 / d)
    if kind == "wide":
        rows, cols = bc._offsets_pattern(n, tuple(o for o in range(-7, 8) if o))
        up = rows < cols
        key = rows[up] * n + cols[up]
        v = np.random.default_rng(66).uniform(-0.03, 0.03, key.size)
        i = np.arange(n, dtype=np.int64)
        ro, ci, va = bc._csr(n, np.concatenate([rows[up], cols[up], i]), np.concatenate([cols[up], rows[up], i]),
                             np.concatenate([v, v, np.ones(n)]))
        return _csr_matrix(n, ro, ci, va)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def ic0(name, L=1):
    """mspmv.ic0_factor of the case's A: the factor as an mspmv.CsrMatrix (the shift is 0: A is an H-matrix)."""
    import mspmv

    l, shift = mspmv.ic0_factor(matrix(name, L))
    assert shift == 0.0
    return l


# ---- right-hand sides --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rhs(name, L):
    """The case's n x L right-hand side, U(0, 1), read-only.  long_rows, node_blocks_mixed: the hub rows hold
    20 + U(0, 1), which makes each hub row's own term a visible share of both dots of the first iteration
    (test_pcg_cases.test_probe_sensitivity).  staggered: columns 0 and 2 supported on E's rows, 1 and 3 on the
    stencil's."""
    n = matrix(name, L).num_rows
    B = np.random.default_rng(70 + 7 * L + sorted(WIDTHS).index(name)).uniform(0.0, 1.0, (n, L))
    if name in HUBS:
        B[list(HUBS[name])] += 20.0
    if name == "staggered":
        assert L == 4
        B[N_EASY:, [0, 2]] = 0.0
        B[:N_EASY, [1, 3]] = 0.0
    B.setflags(write=False)
    return B


# ---- reference arithmetic ----------------------------------------------------------------------------------------
def gamma(k):
    """k eps / (1 - k eps), eps = 2^-53: the bound on the relative error of k successive roundings."""
    k = np.asarray(k, LD)
    return k * LD(EPS) / (1 - k * LD(EPS))


def csr_mm(a, X, absolute=False):
    """A X (|A| X with absolute) in np.longdouble, segment sums over the CSR arrays; every row has its diagonal."""
    va = a.values.astype(LD)
    prod = (np.abs(va) if absolute else va)[:, None] * np.asarray(X, LD)[a.column_indices]
    return np.add.reduceat(prod, a.row_offsets[:-1].astype(np.int64), axis=0)


class CsrApply:
    """Z = M R as a CSR product."""

    def __init__(self, m):
        self.m = m
        self.longest = int(np.diff(m.row_offsets).max())

    def __call__(self, R):
        return csr_mm(self.m, R)

    def error(self, B, Z):
        """(E, Zmaj): |fl(M B) - M B| <= E elementwise for a row sum in any order (gamma_len |M||B|), and
        Zmaj = |M||B| >= |Z|, which also bounds every partial sum the dot-mode kernels multiply by B."""
        zmaj = csr_mm(self.m, np.abs(B), absolute=True)
        return gamma(np.diff(self.m.row_offsets))[:, None] * zmaj, zmaj


class Ic0Apply:
    """Z = L^-T (L^-1 R): two substitutions in np.longdouble, row by row."""

    def __init__(self, l):
        self.n = n = l.num_rows
        ro = l.row_offsets.astype(np.int64)
        self.longest = 0  # (the dots of IC(0)-PCG are streaming passes over stored vectors)
        self.lens = np.diff(ro)
        assert np.array_equal(l.column_indices[ro[1:] - 1], np.arange(n))  # the diagonal ends each row of L
        self.diag = l.values[ro[1:] - 1].astype(LD)
        lv = l.values.astype(LD)
        self.low = [(l.column_indices[ro[i]:ro[i + 1] - 1], lv[ro[i]:ro[i + 1] - 1]) for i in range(n)]
        # L^T by rows: row j holds L(i, j), i > j
        r = np.repeat(np.arange(n, dtype=np.int64), self.lens)
        strict = l.column_indices != r
        order = np.lexsort((r[strict], l.column_indices[strict]))
        tc, tr, tv = l.column_indices[strict][order], r[strict][order], lv[strict][order]
        tro = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(tc, minlength=n), out=tro[1:])
        self.up = [(tr[tro[j]:tro[j + 1]], tv[tro[j]:tro[j + 1]]) for j in range(n)]
        self.tlens = np.diff(tro) + 1

    def _solve(self, tri, order, B, comparison=False):
        X = np.zeros(B.shape, LD)
        for i in order:
            c, v = tri[i]
            s = (np.abs(v) if comparison else -v) @ X[c] if c.size else 0
            X[i] = (B[i] + s) / self.diag[i]
        return X

    def forward(self, B, comparison=False):
        return self._solve(self.low, range(self.n), np.asarray(B, LD), comparison)

    def backward(self, B, comparison=False):
        return self._solve(self.up, range(self.n - 1, -1, -1), np.asarray(B, LD), comparison)

    def __call__(self, R):
        return self.backward(self.forward(R))

    def _abs_product(self, tri, X):
        out = np.abs(X) * self.diag[:, None]
        for i, (c, v) in enumerate(tri):
            if c.size:
                out[i] += np.abs(v) @ np.abs(X[c])
        return out

    def error(self, B, Z):
        """(E, Zmaj).  Substitution in any summation order solves (T + dT) x^ = b with |dT| <= gamma_(len + 2) |T|
        row by row (ic0_cases.solve_residual_ratio's bound), so to first order |x^ - x| <= C(T)^-1 (gamma |T||x| +
        |db|), C(T) the comparison matrix (|diagonal|, -|off-diagonal|), whose inverse dominates |T^-1|: a
        substitution with -|off-diagonal| on a nonnegative right-hand side.  Forward, then backward with the forward
        error as db.  Zmaj = |Z| + E."""
        Y = self.forward(B)
        ey = self.forward(gamma(self.lens + 2)[:, None] * self._abs_product(self.low, Y), comparison=True)
        ez = self.backward(gamma(self.tlens + 2)[:, None] * self._abs_product(self.up, Z) + ey, comparison=True)
        return ez, np.abs(Z) + ez


@functools.lru_cache(maxsize=None)
def applier(name, L, kind):
    return Ic0Apply(ic0(name, L)) if kind == "ic0" else CsrApply(preconditioner(name, L, kind))


def pcg_reference(a, apply_m, B, max_iters, tol, guards):
    """SPAISolveMultiple (guards=True: alpha = 0 for a converged column or when P.AP = 0, beta = 0 for a converged
    column or when rs_old = 0) and PCGSolveMultiple (guards=False: only the converged mask, so 0 / 0 is NaN) as
    oracle/mspmv_oracle.c restates them, in np.longdouble: per-column alpha, beta and masks, the max-relative-residual
    history with std::max's rule (a NaN is skipped).  Returns (X, iterations, history, the iteration at which each
    column converged or -1), X and the history rounded to double."""
    n, L = B.shape
    B = np.asarray(B, LD)
    X = np.zeros((n, L), LD)
    R = B.copy()
    bn = np.sqrt(np.sum(B * B, axis=0))
    bn[bn == 0] = 1
    conv = np.zeros(L, bool)
    conv_at = np.full(L, -1)
    Z = apply_m(R)
    P = Z.copy()
    rs_old = np.sum(R * Z, axis=0)
    hist = []
    it = 0
    with np.errstate(invalid="ignore", divide="ignore"):
        while it < max_iters:
            AP = csr_mm(a, P)
            pap = np.sum(P * AP, axis=0)
            live = ~conv & (pap != 0) if guards else ~conv
            alpha = np.zeros(L, LD)
            alpha[live] = rs_old[live] / pap[live]
            X += alpha * P
            R -= alpha * AP
            rel = np.sqrt(np.sum(R * R, axis=0)) / bn
            hist.append(float(np.fmax.reduce(np.concatenate([[LD(0)], rel]))))
            newly = ~conv & (rel < tol)
            conv_at[newly] = it
            conv |= newly
            it += 1
            if conv.all():
                break
            Z = apply_m(R)
            rs_new = np.sum(R * Z, axis=0)
            live = ~conv & (rs_old != 0) if guards else ~conv
            beta = np.zeros(L, LD)
            beta[live] = rs_new[live] / rs_old[live]
            rs_old = rs_new
            P = Z + beta * P
    return X.astype(np.float64), it, np.array(hist), conv_at


def one_iteration(a, apply_m, B):
    """The first iteration in np.longdouble: Z* = M B, alpha*_j = (B_j . Z*_j) / (Z*_j . (A Z*)_j), and how far a
    solve cut at one iteration, X^ = fl(alpha^ Z^) (P = Z, X = 0 + alpha P: one rounded multiply per element), may lie
    from alpha* Z*.  With E >= |Z^ - Z*| and Zmaj >= |Z^| from apply_m.error, n rows, lenM / lenA the longest rows
    of M (0 for IC(0), whose dots stream over stored vectors) and A:

      numerator     |B|^T Zmaj gamma_(n + lenM + 2) + |B|^T E        a dot of n terms, each a row sum of lenM, in
                                                                     any order (the tile kernels count split rows'
                                                                     carries piecewise), and Z's own error
      denominator   Zmaj^T |A| Zmaj gamma_(n + lenA + 2) + 2 E^T |A| Zmaj        likewise, and Z^ for Z* to first
                                                                                 order (A symmetric)
      alpha         |alpha*| rel,  rel = numerator / |B.Z*| + denominator / (Z*.A Z*) + eps     (the division)
      X             2 (|alpha*| |Z*| (rel + eps) + |alpha*| E)       the final multiply; doubled for the second order

    Returns a dict: Z, alpha, alpha_bound (|alpha*| rel, undoubled), x (alpha* Z*), x_bound, and the pieces a
    sensitivity test needs (num, den, AZ)."""
    n = a.num_rows
    Bl = np.asarray(B, LD)
    Z = apply_m(Bl)
    E, zmaj = apply_m.error(Bl, Z)
    AZ = csr_mm(a, Z)
    absA = csr_mm(a, zmaj, absolute=True)
    num, den = np.sum(Bl * Z, axis=0), np.sum(Z * AZ, axis=0)
    num_err = gamma(n + apply_m.longest + 2) * np.sum(np.abs(Bl) * zmaj, axis=0) + np.sum(np.abs(Bl) * E, axis=0)
    len_a = int(np.diff(a.row_offsets).max())
    den_err = gamma(n + len_a + 2) * np.sum(zmaj * absA, axis=0) + 2 * np.sum(E * absA, axis=0)
    rel = num_err / np.abs(num) + den_err / den + LD(EPS)
    alpha = num / den
    x_bound = 2 * (np.abs(alpha) * np.abs(Z) * (rel + LD(EPS)) + np.abs(alpha) * E)
    return {"Z": Z, "AZ": AZ, "num": num, "den": den, "alpha": alpha, "alpha_bound": np.abs(alpha) * rel,
            "x": alpha * Z, "x_bound": x_bound}


@functools.lru_cache(maxsize=None)
def probe(name, L, kind):
    """one_iteration of a case, and the restatement's residual after that iteration; computed once."""
    a, ap, B = matrix(name, L), applier(name, L, kind), rhs(name, L)
    out = one_iteration(a, ap, B)
    out["hist0"] = pcg_reference(a, ap, B, 1, TOL, guards=kind != "ic0")[2][0]
    return out


@functools.lru_cache(maxsize=None)
def reference(name, L, kind, max_iters=MAX_ITERS):
    """pcg_reference of a case: (X, iterations, history, conv_at), read-only."""
    out = pcg_reference(matrix(name, L), applier(name, L, kind), rhs(name, L), max_iters, TOL, guards=kind != "ic0")
    for arr in out:
        if isinstance(arr, np.ndarray):
            arr.setflags(write=False)
    return out


def oracle_solve(orc, name, L, kind, B=None, max_iters=MAX_ITERS):
    """The oracle's solve of a case (M on A's pattern, or the IC(0) factor): (X, iterations, history)."""
    a = matrix(name, L)
    B = rhs(name, L) if B is None else B
    if kind == "ic0":
        l = ic0(name, L)
        return orc.pcg_ic0_multi(a, l.row_offsets, l.column_indices, l.values, B, max_iters, TOL, hist_cap=max_iters)
    assert kind not in OFF_PATTERN
    return orc.pcg_spai_multi(a, preconditioner(name, L, kind).values, B, max_iters, TOL, hist_cap=max_iters)


# ---- the project's parity bars (test_spai.py, test_ic0.py), kept here so that the CPU tests hold the restatement
# ---- to them too
def iter_match(it_g, it_o, hist_o, tol):
    if it_g == it_o:
        return True
    if abs(it_g - it_o) == 1 and len(hist_o):
        k = min(it_g, it_o) - 1
        return abs(hist_o[k] - tol) <= 1e-9 * tol
    return False


def check_bars(label, ref, out, cols=None, status=0):
    """A solve out = (X, iterations, history, status) against ref = (X, iterations, history, ...): the status; the
    same iteration count under iter_match; len(history) == iterations; the history within 1e-10; per column
    ||X - X_ref|| <= 1e-8 ||X_ref|| (cols: those columns only).  Prints each figure before it asserts; returns (the
    worst history difference, the worst relative X difference)."""
    X, it, hist, st = out
    Xo, it_o, ho = ref[0], ref[1], ref[2]
    k = min(len(hist), len(ho))
    hdev = float(np.max(np.abs(hist[:k] - ho[:k]))) if k else 0.0
    sel = np.arange(X.shape[1]) if cols is None else np.asarray(cols)
    xrel = np.linalg.norm(X[:, sel] - Xo[:, sel], axis=0) / np.linalg.norm(Xo[:, sel], axis=0)
    print(f"\n{label}: status {st}, iterations {it} (reference {it_o}), worst history difference {hdev:.3e} "
          f"(bar 1e-10), worst ||X - X_ref|| / ||X_ref|| {float(xrel.max()):.3e} (bar 1e-8)")
    assert st == status, f"status {st}"
    assert iter_match(it, it_o, ho, TOL), f"iterations {it} against {it_o}"
    assert len(hist) == it, f"history length {len(hist)} of {it} iterations"
    assert k > 0 and hdev <= 1e-10, f"history difference {hdev:.3e}"
    assert np.all(np.isfinite(X[:, sel])) and np.all(xrel <= 1e-8), f"x difference {float(xrel.max()):.3e}"
    return hdev, float(xrel.max())
