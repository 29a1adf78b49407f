#!/usr/bin/env python3
"""Block CG (mspmv_dbcg_multi_dev) next to the lock-step multi-RHS CG (mspmv_dcg_multi_dev) on one handle:
iterations, ms per iteration and ms per solve of each, one JSON line per width.  A warm call (plans, workspace and
the cached graph), then the median of `reps` solves to 1e-9.  Both calls return after their stream has drained, so a
solve is timed by the host clock around the call: launches past convergence and the last control-word copy are
included, as in pbicgstab_probe.py.
    blockcg_probe.py stencil [nx ny] [L ...] [--reps=5] [--shift=0.01]     default 2000 2000, widths 2 4 8 16
    blockcg_probe.py nodes [nx ny] [L ...] [--reps=5] [--shift=0.02]       default 191 190 (217,740 rows, pwtk's size)
stencil: the 5-point Laplacian on an nx x ny grid with `shift` added to its diagonal of 4 (SPD, condition about
8 / shift).  nodes: 6 unknowns per node of a periodic nx x ny grid, every node coupled to its 8 neighbours and
itself by dense 6 x 6 blocks (54 columns in every row: the node-block product kernels), one value -U(0, 1) 8 / 53 per
unordered pair and the diagonal sum |off-diagonal| + shift (a weighted graph Laplacian plus shift: SPD, its smallest
eigenvalue near shift, as ill conditioned as a stiffness matrix is).
MSPMV_LIB selects the library; MSPMV_DIA=0 keeps the stencil's products on the merge tiles."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "sparse-matrix-linear-equations_amd")]
import mspmv  # noqa: E402

TOL = 1e-9
MAX_ITERS = 100000


def csr(n, rows, cols, vals):
    order = np.lexsort((cols, rows))
    ro = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=ro[1:])
    return mspmv.CsrMatrix.from_arrays(n, ro.astype(np.int32), cols[order].astype(np.int32), vals[order])


def stencil(nx, ny, shift):
    g = np.arange(nx * ny, dtype=np.int64).reshape(ny, nx)
    rows = np.concatenate([g.ravel(), g[:, :-1].ravel(), g[:, 1:].ravel(), g[:-1].ravel(), g[1:].ravel()])
    cols = np.concatenate([g.ravel(), g[:, 1:].ravel(), g[:, :-1].ravel(), g[1:].ravel(), g[:-1].ravel()])
    return csr(nx * ny, rows, cols, np.where(rows == cols, 4.0 + shift, -1.0))


def nodes(nx, ny, shift, dof=6, seed=5):
    N = nx * ny
    n = N * dof
    k = np.arange(dof, dtype=np.int64)
    node = np.arange(N, dtype=np.int64)
    i, j = node // nx, node % nx
    rows, cols = [], []
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            other = ((i + di) % ny) * nx + (j + dj) % nx
            rows.append(np.repeat(node * dof, dof * dof) + np.tile(np.repeat(k, dof), N))
            cols.append(np.repeat(other * dof, dof * dof) + np.tile(np.tile(k, dof), N))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    up = rows < cols
    lo, hi = rows[up], cols[up]  # the pattern is symmetric: one value per unordered pair, mirrored
    v = -np.random.default_rng(seed).uniform(0.0, 1.0, lo.size) * (8.0 / 53.0)
    diag = np.bincount(lo, np.abs(v), n) + np.bincount(hi, np.abs(v), n) + shift
    d = np.arange(n, dtype=np.int64)
    return csr(n, np.concatenate([lo, hi, d]), np.concatenate([hi, lo, d]), np.concatenate([v, v, diag]))


def main():
    opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    shape = args[0] if args else "stencil"
    nums = [int(v) for v in args[1:]]
    nx, ny = nums[:2] if len(nums) >= 2 else ((2000, 2000) if shape == "stencil" else (191, 190))
    widths = nums[2:] or [2, 4, 8, 16]
    reps = int(opts.get("reps", 5))
    shift = float(opts.get("shift", 0.01 if shape == "stencil" else 0.02))
    a = stencil(nx, ny, shift) if shape == "stencil" else nodes(nx, ny, shift)
    n = a.num_rows
    with mspmv.GpuCsr(a) as g:
        solvers = {"block_cg": lambda dB, dX, L: g.block_cg_dev(dB, dX, L, MAX_ITERS, TOL),
                   "cg_multi": lambda dB, dX, L: g.cg_dev(dB, dX, L, MAX_ITERS, TOL)}
        for L in widths:
            B = np.random.default_rng(7 + L).uniform(0, 1, (n, L))
            dB, dX = mspmv.DeviceBuffer.from_array(B), mspmv.DeviceBuffer(8 * n * L)
            line = {"lib": os.path.basename(os.environ.get("MSPMV_LIB", "libmspmv.so")), "shape": shape,
                    "grid": [nx, ny], "shift": shift, "rows": n, "nnz": a.num_nonzeros, "L": L, "reps": reps,
                    "tolerance": TOL}
            for name, solve in solvers.items():
                solve(dB, dX, L)  # plans, workspace, the graph
                times, it, st = [], 0, 0
                for _ in range(reps):
                    t0 = time.perf_counter()
                    it, _, st = solve(dB, dX, L)
                    times.append(time.perf_counter() - t0)
                med = statistics.median(times)
                X = dX.download((n, L))
                res = float(np.max(np.linalg.norm(B - g.spmm(X), axis=0) / np.linalg.norm(B, axis=0)))
                line[name] = {"status": st, "iterations": it, "ms_per_solve": round(med * 1e3, 3),
                              "ms_per_iter": round(med * 1e3 / max(it, 1), 4),
                              "min_ms_per_solve": round(min(times) * 1e3, 3), "true_residual": res,
                              "kernel": g.cg_kernel_name()}
            line["product"] = g.solver_product_kernel_name()
            line["solve_speedup"] = round(line["cg_multi"]["ms_per_solve"] / line["block_cg"]["ms_per_solve"], 3)
            print(json.dumps(line), flush=True)
            dB.free()
            dX.free()


if __name__ == "__main__":
    main()
