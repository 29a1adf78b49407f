#!/usr/bin/env python3
"""Multi-colour IC(0)-PCG (mspmv_ic0_create_colored) next to the natural-order IC(0)-PCG and plain CG on the
parabolic_fem shape, synth_stencil(0, 525825, 725, diag_shift=1e-4), all in one process (tools/pcg_probe.py's
protocol: a warm call, then the host clock around synchronous *_dev solves).  One JSON line per (width, solver):
ms per iteration at a fixed iteration count (tolerance 0), iterations to 1e-8, ms per solve (median of `reps`),
the true residual, and the host seconds of the factor (ic0: mspmv_ic0_factor alone; colored:
mspmv_ic0_create_colored whole -- colouring, ordering, factorisation, transpose, upload).
    pcg_ic0_colored_probe.py [L ...] [--iters=20] [--reps=3] [--only=cg|ic0|colored] [--fixed-only]   default 1 8 16
The sweeps' share of a solve and the time of the fused launch come from a kernel trace of this script:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o p -- python pcg_ic0_colored_probe.py 8 \\
        --only=colored --fixed-only
    pcg_ic0_colored_probe.py --stats=DIR/.../p_kernel_stats.csv
prints the summed duration per kernel family and, per k_trsv_color instantiation, calls and the average launch
(TriForm 1: backward, 2: forward, 3: the fused last colour).
MSPMV_LIB selects the library; MSPMV_DIA=0 keeps the products on the merge tiles."""
import csv
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "sparse-matrix-linear-equations_amd")]
import mspmv  # noqa: E402

TOL = 1e-8
SHAPE = (0, 525825, 725)


def kernel_shares(path):
    fam = {"trsv": 0.0, "sweep": 0.0, "product": 0.0, "passes": 0.0, "fill": 0.0, "other": 0.0}
    sweeps = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name, ns = row["Name"], float(row["TotalDurationNs"])
            key = ("trsv" if "k_trsv_tagged" in name else "sweep" if "k_trsv_color" in name else
                   "product" if any(k in name for k in ("k_spmm", "k_spmv", "k_dia", "k_slab")) else
                   "passes" if any(k in name for k in ("k_dist_", "k_cg", "k_pcg", "k_fold")) else
                   "fill" if "fill" in name.lower() or "memset" in name.lower() else "other")
            fam[key] += ns
            if key == "sweep":
                calls = int(row["Calls"])
                sweeps.append({"kernel": name[name.index("k_trsv_color"):name.index(">(") + 1], "calls": calls,
                               "avg_us": round(ns / calls / 1e3, 3)})
    total = sum(fam.values())
    print(json.dumps({"stats": os.path.basename(path), "total_ms": round(total / 1e6, 3),
                      **{k + "_share": round(v / total, 4) for k, v in fam.items()}, "sweeps": sweeps}))


def main():
    opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    if "stats" in opts:
        return kernel_shares(opts["stats"])
    widths = [int(v) for v in sys.argv[1:] if not v.startswith("--")] or [1, 8, 16]
    its, reps, only = int(opts.get("iters", 20)), int(opts.get("reps", 3)), opts.get("only", "")
    fixed_only = "--fixed-only" in sys.argv[1:]
    a = mspmv.CsrMatrix.synth_stencil(*SHAPE, diag_shift=1e-4)
    n = a.num_rows
    t0 = time.perf_counter()
    l, shift = mspmv.ic0_factor(a)
    factor_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    mc = mspmv.GpuIc0.colored(a)
    colored_s = time.perf_counter() - t0
    with mspmv.GpuCsr(a) as g, mspmv.GpuIc0(l) as ic, mc:
        def pcg(m):
            def run(dB, dX, L, iters, tol):
                it = ctypes.c_int()
                st = mspmv.lib.mspmv_dpcg_ic0_multi_dev(g.h, m.h, dB.ptr, dX.ptr, L, iters, tol, mspmv.MERGE,
                                                        ctypes.byref(it), None, 0)
                return it.value, st
            return run

        def cg(dB, dX, L, iters, tol):
            it, _, st = g.cg_dev(dB, dX, L, iters, tol)
            return it, st

        solvers = {"cg": cg, "ic0": pcg(ic), "colored": pcg(mc)}
        for L in widths:
            B = np.random.default_rng(1).uniform(0, 1, (n, L))
            dB, dX = mspmv.DeviceBuffer.from_array(B), mspmv.DeviceBuffer(8 * n * L)
            for name, solve in solvers.items():
                if only and name != only:
                    continue
                solve(dB, dX, L, its, 0.0)  # plans, workspace, the graph
                t0 = time.perf_counter()
                solve(dB, dX, L, its, 0.0)
                out = {"lib": os.path.basename(os.environ.get("MSPMV_LIB", "libmspmv.so")), "rows": n,
                       "nnz": a.num_nonzeros, "L": L, "solver": name, "fixed_iters": its,
                       "ms_per_iter_fixed": round((time.perf_counter() - t0) / its * 1e3, 4),
                       "kernel": g.cg_kernel_name(), "colors": mc.num_colors if name == "colored" else 0,
                       "host_factor_s": round({"cg": 0.0, "ic0": factor_s, "colored": colored_s}[name], 3),
                       "shift": {"cg": None, "ic0": shift, "colored": mc.shift}[name]}
                if not fixed_only:
                    solve(dB, dX, L, 20000, TOL)
                    times, it, st = [], 0, 0
                    for _ in range(reps):
                        t0 = time.perf_counter()
                        it, st = solve(dB, dX, L, 20000, TOL)
                        times.append(time.perf_counter() - t0)
                    med = statistics.median(times)
                    X = dX.download((n, L))
                    Y = g.spmm(X) if L > 1 else g.spmv(X[:, 0]).reshape(n, 1)
                    out.update({"status": st, "iterations": it, "reps": reps, "ms_per_solve": round(med * 1e3, 3),
                                "min_ms_per_solve": round(min(times) * 1e3, 3),
                                "ms_per_iter_solve": round(med * 1e3 / max(it, 1), 4),
                                "true_residual": float(np.max(np.linalg.norm(B - Y, axis=0) /
                                                              np.linalg.norm(B, axis=0)))})
                print(json.dumps(out), flush=True)
            dB.free()
            dX.free()


if __name__ == "__main__":
    main()
