"""Multi-colour IC(0), restated in numpy for test_ic0_colored.py and test_gpu_ic0_colored.py: the cases, the ordering
mspmv_ic0_create_colored builds (multicolor_cases.greedy_ref, perm_of, permuted), the factor of the permuted matrix
(mspmv.ic0_factor, mspmv.csr_transpose: host code, the library's own), its two solves as test_ilu0.TriPlan and the
apply Z = P^T L^-T L^-1 P R as gather, solve, solve, scatter.  The solver's reference is pcg_cases.pcg_reference in
np.longdouble with pcg_cases.Ic0Apply of the permuted factor between the gather and the scatter.  Everything is
computed once per session and shared; callers leave the arrays unchanged.

  randsym777    777 rows, 6 colours: irregular rows, several colours
  hubs600       600 rows, 7 colours, three of a single row: the hub rows alone in their colours, rows of L past 129
                entries with the diagonal last (the LONG instantiation), the last colour a one-row LONG turn-around
  tridiag2000   2 x 1,000 rows: colours past one workgroup at every width; the natural-order IC(0) is the exact
                factor (1 iteration), the red-black one is not
  stencil5_23   the 5-point Laplacian on a 23 x 23 grid (diagonal 4, off-diagonals -1): colours of 265 and 264 rows,
                9 and 8 past a 256-row workgroup at L = 1, no multiple of the 32 rows a workgroup covers at L = 16
  diag300       a diagonal matrix of 300 positive entries: one colour, the fused launch alone
"""
import functools

import numpy as np

import ic0_cases
import multicolor_cases as mc
import pcg_cases as pc
import test_ilu0 as ti

TOL = 1e-9
MAX_ITERS = 200
LD = np.longdouble
CASES = ("randsym777", "hubs600", "tridiag2000", "stencil5_23", "diag300")
# rows per colour of the greedy colouring (hubs600: seven colours, three of them one row)
COLOUR_ROWS = {"randsym777": [255, 204, 156, 108, 42, 12], "tridiag2000": [1000, 1000], "stencil5_23": [265, 264],
               "diag300": [300]}
# (case, width) of every solve of test_gpu_ic0_colored.py; the CPU file holds the restatement to the same bars
SOLVES = ([(name, L) for name in ("randsym777", "stencil5_23") for L in (1, 2, 4, 8, 6, 16)] +
          [("hubs600", 1), ("hubs600", 4), ("tridiag2000", 1), ("tridiag2000", 16), ("diag300", 8)])


def stencil5_23():
    side = 23
    n = side * side
    g = np.arange(n, dtype=np.int64).reshape(side, side)
    rows = [g.ravel(), g[:, :-1].ravel(), g[:, 1:].ravel(), g[:-1].ravel(), g[1:].ravel()]
    cols = [g.ravel(), g[:, 1:].ravel(), g[:, :-1].ravel(), g[1:].ravel(), g[:-1].ravel()]
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    order = np.lexsort((cols, rows))
    ro = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=ro[1:])
    rows, cols = rows[order], cols[order]
    return n, ro.astype(np.int32), cols.astype(np.int32), np.where(rows == cols, 4.0, -1.0)


def diag300():
    n = 300
    d = np.random.default_rng(300).uniform(0.5, 4.0, n)
    return n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), d


@functools.lru_cache(maxsize=None)
def arrays(name):
    """(row_offsets, column_indices, values) of the case, read-only."""
    if name in ic0_cases.SMALL:
        _, ro, ci, va = ic0_cases.SMALL[name]()
    else:
        _, ro, ci, va = {"stencil5_23": stencil5_23, "diag300": diag300}[name]()
    for arr in (ro, ci, va):
        arr.setflags(write=False)
    return ro, ci, va


@functools.lru_cache(maxsize=None)
def matrix(name):
    """The case as an mspmv.CsrMatrix."""
    return mc.csr(arrays(name))


@functools.lru_cache(maxsize=None)
def ordering(name):
    """(colors, number of colours, perm, the permuted matrix, its L by mspmv.ic0_factor, the shift, L^T by
    mspmv.csr_transpose), the last four as mspmv.CsrMatrix."""
    import mspmv

    a = arrays(name)
    colors, num = mc.greedy_ref(a)
    perm = mc.perm_of(colors)
    ap = mc.csr(mc.permuted(a, perm))
    l, shift = mspmv.ic0_factor(ap)
    return colors, num, perm, ap, l, shift, mspmv.csr_transpose(l)


@functools.lru_cache(maxsize=None)
def tri_plans(name):
    """test_ilu0.TriPlan of the permuted L and L^T, rows summed in CSR order: the solves in the colour ordering."""
    _, _, _, _, l, _, lt = ordering(name)
    return ti.TriPlan(l, True, False), ti.TriPlan(lt, False, False)


def apply_ref(name, B):
    """Gather, L^-1, L^-T, scatter, in float64 (what the GPU's apply must equal bit for bit)."""
    perm = ordering(name)[2]
    pl, pu = tri_plans(name)
    Z = np.empty_like(B)
    Z[perm] = pu.solve(pl.solve(np.ascontiguousarray(B[perm])))
    return Z


class ColoredApply:
    """Z = P^T L^-T L^-1 P R in np.longdouble: pcg_cases.Ic0Apply of the permuted factor between the gather and
    the scatter."""

    def __init__(self, name):
        self.perm = ordering(name)[2]
        self.inner = pc.Ic0Apply(ordering(name)[4])

    def __call__(self, R):
        Z = np.empty(R.shape, LD)
        Z[self.perm] = self.inner(np.asarray(R, LD)[self.perm])
        return Z


@functools.lru_cache(maxsize=None)
def natural_apply(name):
    """pcg_cases.Ic0Apply of the natural-order factor of the case."""
    import mspmv

    return pc.Ic0Apply(mspmv.ic0_factor(matrix(name))[0])


@functools.lru_cache(maxsize=None)
def rhs(name, L):
    """The case's n x L right-hand side, U(0, 1), read-only."""
    n = matrix(name).num_rows
    B = np.random.default_rng(900 + 13 * L + CASES.index(name)).uniform(0.0, 1.0, (n, L))
    B.setflags(write=False)
    return B


@functools.lru_cache(maxsize=None)
def reference(name, L, colored=True):
    """pcg_cases.pcg_reference (PCGSolveMultiple, np.longdouble) of the case with the multi-colour apply, or the
    natural-order one: (X, iterations, history, conv_at), read-only."""
    ap = ColoredApply(name) if colored else natural_apply(name)
    out = pc.pcg_reference(matrix(name), ap, rhs(name, L), MAX_ITERS, TOL, guards=False)
    for arr in out:
        if isinstance(arr, np.ndarray):
            arr.setflags(write=False)
    return out


def pcg_float64(name, L, max_iters=MAX_ITERS, tol=TOL):
    """pcg_reference's recurrence (guards=False) in float64 throughout, the apply being apply_ref: what a device
    that rounds every operation to double computes, up to the summation order of its products and dots.  Returns
    (X, iterations, history, status 0)."""
    a, B = matrix(name), rhs(name, L)
    ro = a.row_offsets[:-1].astype(np.int64)

    def mm(X):
        return np.add.reduceat(a.values[:, None] * X[a.column_indices], ro, axis=0)

    X = np.zeros(B.shape)
    R = B.copy()
    bn = np.sqrt(np.sum(B * B, axis=0))
    bn[bn == 0] = 1
    conv = np.zeros(L, bool)
    Z = apply_ref(name, R)
    P = Z.copy()
    rs_old = np.sum(R * Z, axis=0)
    hist = []
    it = 0
    while it < max_iters:
        AP = mm(P)
        alpha = np.where(conv, 0.0, rs_old / np.sum(P * AP, axis=0))
        X += alpha * P
        R -= alpha * AP
        rel = np.sqrt(np.sum(R * R, axis=0)) / bn
        hist.append(float(rel.max()))
        conv |= rel < tol
        it += 1
        if conv.all():
            break
        Z = apply_ref(name, R)
        rs_new = np.sum(R * Z, axis=0)
        beta = np.where(conv, 0.0, rs_new / rs_old)
        rs_old = rs_new
        P = Z + beta * P
    return X, it, np.array(hist), 0
