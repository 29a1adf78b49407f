#!/usr/bin/env python3
"""Warm start (mspmv_set_initial_guess) against cold solves over implicit heat-equation steps on one handle:
(I + dt K) u_(k+1) = u_k, K the 5-point Laplacian (stencil) or the node-block graph Laplacian of blockcg_probe.py
(nodes), each step solved twice from the same right-hand side -- cold (x0 = 0) and warm (x0 = u_k, the previous
step's solution) -- with mspmv_dcg_multi_dev to 1e-9.  u_0 is smooth -- per column 144 low sine modes of the grid
with decaying amplitudes, zero on the stencil's (Dirichlet) boundary, periodic on the nodes' torus -- so a step
changes u by little and the warm start's residual ("x0_residual", ||u_k - A u_k|| / ||u_k||) is small against
||u_k||.  Per step and width: the iterations and the median ms per solve of each, and the warm init's own cost measured
as mspmv_dresidual_dev without R (the plain product and the pass, one host sync and a 2 L-value copy included: an
upper estimate).  One JSON line per (shape, width) on stdout and, with
--out=FILE, the list of them in FILE.  The solver calls return after their stream has drained, so a solve is timed by
the host clock around the call, as in blockcg_probe.py; every timed call follows a warm-up call of the same kind.
    warm_start_probe.py stencil [nx ny] [L ...] [--steps=5] [--reps=5] [--dt=20] [--out=FILE]   default 2000 2000, L 1 8
    warm_start_probe.py nodes [nx ny] [L ...] ...                                                default 191 190, L 1 8
MSPMV_LIB selects the library; MSPMV_DIA=0 keeps the stencil's products on the merge tiles."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blockcg_probe as bp  # noqa: E402  (the matrices; it puts the package on the path)

mspmv = bp.mspmv
TOL = 1e-9
MAX_ITERS = 100000


def heat_matrix(shape, nx, ny, dt):
    """I + dt K as a CsrMatrix: K = the shape's matrix with a zero diagonal shift (a graph Laplacian, K 1 = 0 up to
    the stencil's boundary rows)."""
    k = bp.stencil(nx, ny, 0.0) if shape == "stencil" else bp.nodes(nx, ny, 0.0)
    r = np.repeat(np.arange(k.num_rows), np.diff(k.row_offsets))
    return mspmv.CsrMatrix.from_arrays(k.num_cols, k.row_offsets, k.column_indices,
                                       dt * k.values + (r == k.column_indices))


def smooth_field(shape, nx, ny, n, L, modes=12):
    """n x L: per column a sum of the modes^2 lowest sine modes of the grid with amplitudes (a^2 + b^2)^-1.5 and seeded
    random signs -- smooth, but not a handful of eigenvectors (CG would finish those in as many iterations)."""
    if shape == "stencil":
        x, y, w = (np.arange(nx) + 1.0) / (nx + 1), (np.arange(ny) + 1.0) / (ny + 1), np.pi
    else:
        x, y, w = np.arange(nx) / nx, np.arange(ny) / ny, 2 * np.pi
    k = 1.0 + np.arange(modes)
    sx, sy = np.sin(w * np.outer(x, k) + 0.3 * (shape != "stencil")), np.sin(w * np.outer(y, k))
    amp = (k[:, None] ** 2 + k[None, :] ** 2) ** -1.5
    dof = n // (nx * ny)
    U = np.empty((n, L))
    for c in range(L):
        sign = np.random.default_rng(11 + c).choice([-1.0, 1.0], amp.shape)
        U[:, c] = np.repeat((sy @ (amp * sign) @ sx.T).ravel(), dof)
    return U


def timed(call, reps):
    call()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return out, statistics.median(times) * 1e3


def main():
    opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    shape = args[0] if args else "stencil"
    nums = [int(v) for v in args[1:]]
    nx, ny = nums[:2] if len(nums) >= 2 else ((2000, 2000) if shape == "stencil" else (191, 190))
    widths = nums[2:] or [1, 8]
    steps, reps, dt = int(opts.get("steps", 5)), int(opts.get("reps", 5)), float(opts.get("dt", 20.0))
    a = heat_matrix(shape, nx, ny, dt)
    n = a.num_rows
    lines = []
    with mspmv.GpuCsr(a) as g:
        for L in widths:
            U = smooth_field(shape, nx, ny, n, L)
            probe = np.zeros(1)

            def copy_x0():
                # hipMemcpy device to device returns before the copy is done and runs on the null stream, which the
                # handle's non-blocking stream does not wait for: the 8-byte read back, queued behind it, does
                mspmv.lib.mspmv_memcpy_d2d(dX.ptr, dB.ptr, 8 * n * L)
                mspmv.lib.mspmv_memcpy_d2h(probe.ctypes.data, dX.ptr, 8)

            dB, dX = mspmv.DeviceBuffer.from_array(U), mspmv.DeviceBuffer(8 * n * L)
            line = {"lib": os.path.basename(os.environ.get("MSPMV_LIB", "libmspmv.so")), "shape": shape,
                    "grid": [nx, ny], "dt": dt, "rows": n, "nnz": a.num_nonzeros, "L": L, "reps": reps,
                    "tolerance": TOL, "steps": []}
            for k in range(steps):
                dB.upload(U)   # the step's right-hand side, and its warm start
                _, ms_copy = timed(copy_x0, reps)
                r0 = g.residual_dev(dB, dB, None, L)[1]   # ||B - A X0|| of the warm start X0 = B
                (itc, _, stc), ms_c = timed(lambda: g.cg_dev(dB, dX, L, MAX_ITERS, TOL, warm=False), reps)
                kc = g.cg_kernel_name()

                def warm():
                    copy_x0()
                    return g.cg_dev(dB, dX, L, MAX_ITERS, TOL, warm=True)

                (itw, _, stw), ms_w = timed(warm, reps)
                kw = g.cg_kernel_name()   # (dX now holds the warm solve's result: the next step's right-hand side)
                (nb, nr), ms_init = timed(lambda: g.residual_dev(dB, dX, None, L), reps)
                U = dX.download((n, L))
                line["steps"].append({"step": k, "cold_iters": itc, "warm_iters": itw, "cold_ms": round(ms_c, 3),
                                      "warm_ms": round(ms_w - ms_copy, 3), "x0_copy_ms": round(ms_copy, 3),
                                      "warm_init_ms": round(ms_init, 3),
                                      "cold_ms_per_iter": round(ms_c / max(itc, 1), 4),
                                      "status": [stc, stw], "true_residual": float(np.max(nr / nb)),
                                      "x0_residual": float(np.max(r0 / nb))})
            line["kernels"] = {"cold": kc, "warm": kw}
            print(json.dumps(line), flush=True)
            lines.append(line)
            dB.free()
            dX.free()
    if "out" in opts:
        with open(opts["out"], "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
