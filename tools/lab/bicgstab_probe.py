#!/usr/bin/env python3
"""Multi-RHS BiCGSTAB (mspmv_dbicgstab_multi_dev) on a convection-diffusion stencil: iterations, ms per
iteration and bytes/s against the algorithmic count of DESIGN 4.4a -- two products (12 B per nonzero each)
and 24 reads or writes of an n x L vector per iteration -- one JSON line per width.
    bicgstab_probe.py [nx ny [L ...]]        default 1000 1000 1 8 16
MSPMV_LIB selects the library; MSPMV_DIA=0 keeps the products on the merge tiles."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "sparse-matrix-linear-equations_amd")]
import mspmv  # noqa: E402

VECTOR_TOUCHES = 24  # rhat.V 2, s pass 6, T.T/T.s 2, update 6, p pass 4, and each product's X read and Y write


def convdiff(nx, ny, c=0.4, d=0.3, seed=3):
    """tests/test_bicgstab.py's 5-point stencil (values -1-d, -1-c, 4 + 0.5 u, -1+c, -1+d), vectorised."""
    n = nx * ny
    r = np.arange(n)
    i, j = r % nx, r // nx
    u = np.random.default_rng(seed).uniform(size=n)
    cols = np.stack([r - nx, r - 1, r, r + 1, r + nx], axis=1)
    vals = np.stack([np.full(n, -1.0 - d), np.full(n, -1.0 - c), 4.0 + 0.5 * u, np.full(n, -1.0 + c),
                     np.full(n, -1.0 + d)], axis=1)
    keep = np.stack([j > 0, i > 0, np.ones(n, bool), i < nx - 1, j < ny - 1], axis=1)
    ro = np.concatenate([[0], np.cumsum(keep.sum(axis=1))])
    return mspmv.CsrMatrix.from_arrays(n, ro, cols[keep], vals[keep])


def main():
    args = [int(v) for v in sys.argv[1:]]
    nx, ny = args[:2] if len(args) >= 2 else (1000, 1000)
    widths = args[2:] or [1, 8, 16]
    a = convdiff(nx, ny)
    n = a.num_rows
    with mspmv.GpuCsr(a) as g:
        for L in widths:
            B = np.random.default_rng(7 + L).uniform(0, 1, (n, L))
            dB, dX = mspmv.DeviceBuffer.from_array(B), mspmv.DeviceBuffer(8 * n * L)
            g.bicgstab_dev(dB, dX, L, 100000, 1e-9)  # plans, workspace, the graph
            best, it, st = None, 0, 0
            for _ in range(3):
                t0 = time.perf_counter()
                it, _, st = g.bicgstab_dev(dB, dX, L, 100000, 1e-9)
                el = time.perf_counter() - t0
                best = el / max(it, 1) if best is None else min(best, el / max(it, 1))
            X = dX.download((n, L))
            Y = g.spmm(X) if L > 1 else g.spmv(X[:, 0]).reshape(n, 1)
            res = float(np.max(np.linalg.norm(B - Y, axis=0) / np.linalg.norm(B, axis=0)))
            bytes_it = 2 * 12 * a.num_nonzeros + 8 * n * L * VECTOR_TOUCHES
            print(json.dumps({"lib": os.path.basename(os.environ.get("MSPMV_LIB", "libmspmv.so")), "grid": [nx, ny],
                              "rows": n, "nnz": a.num_nonzeros, "L": L, "status": st, "iterations": it,
                              "ms_per_iter": round(best * 1e3, 4), "bytes_per_iter": bytes_it,
                              "TB_per_s": round(bytes_it / best / 1e12, 3), "true_residual": res,
                              "product": g.spmm_kernel_name(L), "solver": g.cg_kernel_name()}), flush=True)
            dB.free()
            dX.free()


if __name__ == "__main__":
    main()
