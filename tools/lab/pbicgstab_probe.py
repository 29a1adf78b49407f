#!/usr/bin/env python3
"""ILU(0)-preconditioned multi-RHS BiCGSTAB (mspmv_dpbicgstab_ilu0_multi_dev) next to the unpreconditioned
solver (mspmv_dbicgstab_multi_dev) on one convection-diffusion stencil: iterations, ms per solve and ms per
iteration of each, one JSON line per (width, solver).  Warm runs (plans, workspace and the cached graph built by
a first solve), then the median of `reps` solves.  Both calls return after their stream has drained, so a solve
is timed by the host clock around the call: launches past convergence and the last control-word copy are
included, as in bicgstab_probe.py.
    pbicgstab_probe.py [nx ny [L ...]] [--reps=5] [--c=0.4] [--d=0.3] [--colored]      default 2000 2000 1 16
--colored adds the multi-colour ILU(0) factor (mspmv_ilu0_create_colored, greedy colours: one parallel sweep per
colour instead of a dependency chain) as a third solver, "colored", beside "plain" and "ilu0".
The share of an iteration spent in the triangular solves comes from a kernel trace of this script:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o p -- python pbicgstab_probe.py ... --only=ilu0
    pbicgstab_probe.py --stats=DIR/.../p_kernel_stats.csv
prints the summed duration per kernel family (k_trsv_tagged, the colour sweeps k_trsv_color, the products, the
k_bicg_* passes, the fills).
MSPMV_LIB selects the library; MSPMV_DIA=0 keeps the products on the merge tiles."""
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "sparse-matrix-linear-equations_amd"), os.path.dirname(os.path.abspath(__file__))]
import mspmv  # noqa: E402
from bicgstab_probe import convdiff  # noqa: E402

TOL = 1e-9


def kernel_shares(path):
    """Summed duration per kernel family from rocprofv3's *_kernel_stats.csv."""
    fam = {"trsv": 0.0, "sweep": 0.0, "product": 0.0, "passes": 0.0, "fill": 0.0, "other": 0.0}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name, ns = row["Name"], float(row["TotalDurationNs"])
            key = ("trsv" if "k_trsv_tagged" in name else "sweep" if "k_trsv_color" in name else
                   "passes" if "k_bicg_" in name else
                   "product" if any(k in name for k in ("k_spmm", "k_spmv", "k_dia", "k_slab")) else
                   "fill" if "fill" in name.lower() or "memset" in name.lower() else "other")
            fam[key] += ns
    total = sum(fam.values())
    print(json.dumps({"stats": os.path.basename(path), "total_ms": round(total / 1e6, 3),
                      **{k + "_share": round(v / total, 4) for k, v in fam.items()}}))


def main():
    opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    if "stats" in opts:
        return kernel_shares(opts["stats"])
    args = [int(v) for v in sys.argv[1:] if not v.startswith("--")]
    nx, ny = args[:2] if len(args) >= 2 else (2000, 2000)
    widths = args[2:] or [1, 16]
    reps = int(opts.get("reps", 5))
    only = opts.get("only", "")
    a = convdiff(nx, ny, c=float(opts.get("c", 0.4)), d=float(opts.get("d", 0.3)))
    n = a.num_rows
    t0 = time.perf_counter()
    lu = mspmv.CsrMatrix.from_arrays(n, a.row_offsets, a.column_indices, mspmv.ilu0_values(a))
    factor_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    mc = mspmv.GpuIlu0.colored(a) if "--colored" in sys.argv[1:] else None  # colouring, ordering, factor, upload
    colored_ms = (time.perf_counter() - t0) * 1e3
    with mspmv.GpuCsr(a) as g, mspmv.GpuIlu0(lu) as m:
        solvers = {"plain": lambda dB, dX, L: g.bicgstab_dev(dB, dX, L, 100000, TOL),
                   "ilu0": lambda dB, dX, L: mspmv.pbicgstab_ilu0_dev(g, m, dB, dX, L, 100000, TOL)}
        if mc is not None:
            solvers["colored"] = lambda dB, dX, L: mspmv.pbicgstab_ilu0_dev(g, mc, dB, dX, L, 100000, TOL)
        for L in widths:
            B = np.random.default_rng(7 + L).uniform(0, 1, (n, L))
            dB, dX = mspmv.DeviceBuffer.from_array(B), mspmv.DeviceBuffer(8 * n * L)
            for name, solve in solvers.items():
                if only and name != only:
                    continue
                solve(dB, dX, L)  # plans, workspace, the graph
                times, it, st = [], 0, 0
                for _ in range(reps):
                    t0 = time.perf_counter()
                    it, _, st = solve(dB, dX, L)
                    times.append(time.perf_counter() - t0)
                med = statistics.median(times)
                X = dX.download((n, L))
                Y = g.spmm(X) if L > 1 else g.spmv(X[:, 0]).reshape(n, 1)
                res = float(np.max(np.linalg.norm(B - Y, axis=0) / np.linalg.norm(B, axis=0)))
                print(json.dumps({"lib": os.path.basename(os.environ.get("MSPMV_LIB", "libmspmv.so")),
                                  "grid": [nx, ny], "rows": n, "nnz": a.num_nonzeros, "L": L, "solver": name,
                                  "status": st, "iterations": it, "reps": reps,
                                  "ms_per_solve": round(med * 1e3, 3), "ms_per_iter": round(med * 1e3 / max(it, 1), 4),
                                  "min_ms_per_solve": round(min(times) * 1e3, 3), "true_residual": res,
                                  "host_factor_ms": round(colored_ms if name == "colored" else factor_ms, 1),
                                  "colors": mc.num_colors if name == "colored" else 0,
                                  "product": g.spmm_kernel_name(L),
                                  "kernel": g.cg_kernel_name()}), flush=True)
            dB.free()
            dX.free()
    if mc is not None:
        mc.close()


if __name__ == "__main__":
    main()
