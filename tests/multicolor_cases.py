"""Multi-colour ILU(0), restated in numpy for test_multicolor.py and test_gpu_multicolor.py: the greedy colouring
mspmv_color_greedy runs, the ordering and the permuted matrix mspmv_ilu0_create_colored factors, and the
preconditioner apply Z = P^T U^-1 L^-1 P R as a pair of plans with .solve(B), so that test_ilu0.pbicgstab_ref runs
unchanged on them.  Everything is computed once per session and shared; callers leave the arrays unchanged."""
import functools

import numpy as np

import mspmv
import test_bicgstab as tb
import test_ilu0 as ti
from test_bicgstab import TOL


def chain515():
    """A nonsymmetric, strictly row diagonally dominant tridiagonal matrix, n = 515.  Two colours (even rows,
    odd rows) of 258 and 257 rows: two rows and one row past a 256-row workgroup at L = 1, and no multiple of
    the 32 rows a workgroup covers at L = 16."""
    n = 515
    i = np.arange(n)
    sub, sup = -1.0 - 0.3 * np.sin(i), -0.5 + 0.2 * np.cos(i)
    diag = np.abs(sub) + np.abs(sup) + 1.0
    rows = np.concatenate([i[1:], i, i[:-1]])
    cols = np.concatenate([i[1:] - 1, i, i[:-1] + 1])
    vals = np.concatenate([sub[1:], diag, sup[:-1]])
    order = np.lexsort((cols, rows))
    ro = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=ro[1:])
    return ro, cols[order].astype(np.int32), vals[order]


@functools.lru_cache(maxsize=None)
def matrix(name):
    """(row_offsets, column_indices, values): chain515, else test_ilu0.matrix(name)."""
    return chain515() if name == "chain515" else ti.matrix(name)


def greedy_ref(a):
    """mspmv_color_greedy restated: rows 0..n-1 in turn take the smallest colour no already-coloured neighbour
    in A + A^T's off-diagonal pattern holds.  (colors int32 [n], number of colours)."""
    ro, ci, _ = a
    n = len(ro) - 1
    nbr = [set() for _ in range(n)]
    for i in range(n):
        for j in ci[ro[i]:ro[i + 1]]:
            j = int(j)
            if j != i:
                nbr[i].add(j)
                nbr[j].add(i)
    colors = np.full(n, -1, np.int32)
    for i in range(n):
        held = {int(colors[j]) for j in nbr[i] if j < i}
        c = 0
        while c in held:
            c += 1
        colors[i] = c
    return colors, int(colors.max()) + 1 if n else 0


def max_degree(a):
    """Largest degree of the symmetrised off-diagonal pattern."""
    ro, ci, _ = a
    n = len(ro) - 1
    rows = np.repeat(np.arange(n), np.diff(ro))
    off = rows != ci
    pairs = {(int(r), int(c)) for r, c in zip(rows[off], ci[off])}
    pairs |= {(c, r) for r, c in pairs}
    return int(np.bincount([r for r, _ in pairs], minlength=n).max())


def perm_of(colors):
    """Rows stably sorted by colour: row i of the permuted matrix is row perm[i] of A."""
    return np.argsort(colors, kind="stable").astype(np.int32)


def permuted(a, perm):
    """P A P^T in CSR, every row's columns ascending (numpy only)."""
    ro, ci, va = a
    n = len(ro) - 1
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    rows = np.repeat(np.arange(n), np.diff(ro))
    r2, c2 = inv[rows], inv[ci]
    order = np.lexsort((c2, r2))
    pro = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(r2, minlength=n), out=pro[1:])
    return pro, c2[order].astype(np.int32), va[order]


@functools.lru_cache(maxsize=None)
def ordering(name):
    """(colors, number of colours, perm, the permuted matrix, its ILU(0) by test_ilu0.ilu0_ref)."""
    a = matrix(name)
    colors, num = greedy_ref(a)
    perm = perm_of(colors)
    ap = permuted(a, perm)
    return colors, num, perm, ap, ti.ilu0_ref(ap)[0]


@functools.lru_cache(maxsize=None)
def triangles(name):
    """(L with its unit diagonal, U) of the permuted matrix's factor, as test_ilu0.triangles builds them."""
    _, _, _, ap, lu = ordering(name)
    return ti.triangles(ap, lu)


@functools.lru_cache(maxsize=None)
def tri_plans(name, solve_order):
    """test_ilu0.TriPlan of the permuted L and U: the solves in the colour ordering."""
    l, u = triangles(name)
    rev = solve_order == "rev"
    return ti.TriPlan(l, True, rev), ti.TriPlan(u, False, rev)


class _Lower:
    def __init__(self, plan, perm):
        self.plan, self.perm = plan, perm

    def solve(self, B):  # gather into the colour ordering, then L^-1
        return self.plan.solve(np.ascontiguousarray(B[self.perm]))


class _Upper:
    def __init__(self, plan, perm):
        self.plan, self.perm = plan, perm

    def solve(self, Y):  # U^-1, then scatter back to A's ordering
        X = np.empty_like(Y)
        X[self.perm] = self.plan.solve(Y)
        return X


@functools.lru_cache(maxsize=None)
def plans(name, solve_order):
    """The apply Z = P^T U^-1 L^-1 P R as the (lower, upper) pair test_ilu0.pbicgstab_ref takes."""
    perm = ordering(name)[2]
    pl, pu = tri_plans(name, solve_order)
    return _Lower(pl, perm), _Upper(pu, perm)


def apply_ref(name, B):
    """The restatement's gather - solve - solve - scatter, rows summed in CSR order."""
    pl, pu = plans(name, "csr")
    return pu.solve(pl.solve(B))


@functools.lru_cache(maxsize=None)
def reference(name, L, max_iters=200):
    """test_ilu0.reference with the multi-colour apply: {variant: (X, iters, hist, status, conv)}."""
    a = matrix(name)
    B = tb.rhs(len(a[0]) - 1, L)
    return {v: ti.pbicgstab_ref(a, plans(name, v[1]), B, max_iters, TOL, dot=v[0]) for v in ti.VARIANTS}


def csr(a):
    ro, ci, va = a
    return mspmv.CsrMatrix.from_arrays(len(ro) - 1, ro, ci, va)
