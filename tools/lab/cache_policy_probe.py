#!/usr/bin/env python3
"""What the Infinity Cache is worth to the product kernels, per handle policy (mspmv_set_cache_policy), on
bench.py's own shapes and through its own timing entry (mspmv.time_spmm_batch), all in one process:

  (a) one pwtk-shaped matrix back to back (bench.py's hot_single_matrix), STREAM against RESIDENT;
  (b) the headline batch of four with the first k = 0..4 handles RESIDENT and the rest STREAM, 200 steps after
      10 warm-up steps;
  (c) bench.py's CG_LARGE stencil through cg_dev in the two-kernel pipelined form (MSPMV_CG_RESIDENT=0), both
      policies: us per iteration, median of 3 solves after a warm one.

The whole sweep runs twice, the second pass in the opposite order.  One JSON document on stdout (and in the
file named by the first argument, if any)."""
import json
import os
import sys
import time

import numpy as np

os.environ["MSPMV_CG_RESIDENT"] = "0"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sparse-matrix-linear-equations_amd")]
import mspmv  # noqa: E402
from bench import CG_LARGE, PWTK, glibc_rhs  # noqa: E402

STEPS, WARMUP, DEV = 200, 10, 0
POLICY = {"stream": mspmv.CACHE_STREAM, "resident": mspmv.CACHE_RESIDENT}


def timed(gs, dxs, dys):
    mspmv.time_spmm_batch(gs, dxs, dys, 1, WARMUP)
    step_ms, kern_ms, _ = mspmv.time_spmm_batch(gs, dxs, dys, 1, STEPS)
    return round(step_ms * 1e3, 3), round(kern_ms * 1e3, 3)


def main():
    out = {"steps": STEPS, "warmup": WARMUP, "budget_bytes": mspmv.cache_budget(DEV), "passes": []}
    mats = [mspmv.CsrMatrix.synth_fem_blocked(PWTK["m"], PWTK["nnz"], PWTK["block"], PWTK["half_band_nodes"], seed=1 + i)
            for i in range(4)]
    gs = [mspmv.GpuCsr(a, device=DEV) for a in mats]
    dxs = [mspmv.DeviceBuffer.from_array(np.random.default_rng(2 + i).uniform(0.0, 1.0, a.num_cols), DEV)
           for i, a in enumerate(mats)]
    dys = [mspmv.DeviceBuffer(8 * a.num_rows, DEV) for a in mats]
    out["auto"] = [dict(zip(("resident", "bytes"), g.cache_info())) for g in gs]
    nx, ny, nz = CG_LARGE["dims"]
    st = mspmv.CsrMatrix.synth_stencil(1, nx * ny * nz, nx, ny, nz, seed=9, diag_shift=CG_LARGE["shift"])
    b = glibc_rhs(42, st.num_rows)
    thr = float(np.sqrt(np.sum(b * b)) * 1e-5)

    for p in range(2):
        rec = {"order": "ascending" if p == 0 else "descending", "single": {}, "batch": {}, "cg_large": {}}
        names = list(POLICY) if p == 0 else list(POLICY)[::-1]
        for g in gs:
            g.set_cache_policy(mspmv.CACHE_STREAM)
        for name in names:  # (a)
            gs[0].set_cache_policy(POLICY[name])
            step, kern = timed(gs[:1], dxs[:1], dys[:1])
            rec["single"][name] = {"us_per_call": step, "kernel_us": kern, "kernel": gs[0].kernel_name()}
        for k in (range(5) if p == 0 else range(4, -1, -1)):  # (b)
            for i, g in enumerate(gs):
                g.set_cache_policy(mspmv.CACHE_RESIDENT if i < k else mspmv.CACHE_STREAM)
            step, kern = timed(gs, dxs, dys)
            rec["batch"][str(k)] = {"us_per_step": step, "kernel_us": kern,
                                    "resident_bytes": sum(g.cache_info()[1] for g in gs[:k]),
                                    "leased_bytes": mspmv.cache_leased(DEV)}
        for g in gs:  # the stencil's handle is alone in the cache
            g.set_cache_policy(mspmv.CACHE_STREAM)
        with mspmv.GpuCsr(st, device=DEV) as g:  # (c)
            db, dx = mspmv.DeviceBuffer.from_array(b, DEV), mspmv.DeviceBuffer(8 * st.num_rows, DEV)
            for name in names:
                g.set_cache_policy(POLICY[name])
                g.cg_dev(db, dx, 1, 10000, thr)
                els = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    it, _, status = g.cg_dev(db, dx, 1, 10000, thr)
                    els.append(time.perf_counter() - t0)
                rec["cg_large"][name] = {"us_per_iter": round(float(np.median(els)) / max(it, 1) * 1e6, 3),
                                         "iterations": it, "status": status, "kernel": g.cg_kernel_name(),
                                         "bytes": g.cache_info()[1]}
            db.free()
            dx.free()
        out["passes"].append(rec)
    for g in gs:
        g.close()
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
