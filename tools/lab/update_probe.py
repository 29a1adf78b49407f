#!/usr/bin/env python3
"""What a change of values on a fixed pattern costs: mspmv_csr_update_values next to the only path there was before
it, destroy + create + the first products' plan builds.  One JSON line per shape, and all of them as a list in --out.
    update_probe.py [shape ...] [--reps=20] [--L=8] [--out=profiles/update_values_probe.json]
Shapes (default all four): pwtk (the pwtk-size node-block FEM matrix of bench.py's headline), nlpkkt120 (the
nlpkkt120-size 27-point stencil: offset windows), powerlaw (pwtk-size power-law rows: sliced ELL, column groups),
band (pwtk-size scattered band: sliced ELL, one group).  Per shape, with the plans of the L = 1 and the L-wide
product built:
  recreate_ms      (a) wall ms of destroy + GpuCsr(A') + the first product at L = 1 and at L (host clock; the products
                   are the host-pointer calls, which return after their stream has drained)
  update_ms        (b) GpuCsr.update_values(v1) via update_ms(): the host-pointer form, upload of the values included
                   (the first one, which also uploads the source maps, and the median of `reps` more)
  update_dev_ms    (c) GpuCsr.update_values_dev: `reps` updates enqueued back to back after one warm-up, host clock from
                   a drained stream to the sync after the last, per update; the first (map-upload) update apart
  floor_ms         (d) the bytes the update cannot avoid -- the values read and written into the CSR array (16 B per
                   nonzero), and per derived copy the values read again (8 B), its slots written (>= 8 B per nonzero:
                   padding slots are not counted) and, where the copy is a reordering, its 4-B source map read --
                   over time_stream_read's measured ceiling on this device
  dev_over_floor   (c) / (d);  recreate_over_dev  (a) / (c)
MSPMV_LIB selects the library."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "sparse-matrix-linear-equations_amd")]
import mspmv  # noqa: E402

PWTK = dict(m=217918, nnz=11524432)

SHAPES = {
    "pwtk": lambda: mspmv.CsrMatrix.synth_fem_blocked(PWTK["m"], PWTK["nnz"], 6, 1700, seed=3),
    "nlpkkt120": lambda: mspmv.CsrMatrix.synth_stencil(1, 160 * 135 * 164, 160, 135, 164, diag_shift=1e-2),
    "powerlaw": lambda: mspmv.CsrMatrix.synth_powerlaw(PWTK["m"], PWTK["m"], PWTK["nnz"], 1.2, 3),
    "band": lambda: mspmv.CsrMatrix.synth_banded(PWTK["m"], PWTK["nnz"], 10000, seed=77),
}


def derived_copies(g, L):
    """[(what, reordered through a source map)] of the value copies the handle's L = 1 and L-wide plans hold."""
    k1, kL = g.kernel_name(), g.spmm_kernel_name(L)
    out = []
    if k1.startswith("k_spmm_dia<") or kL.startswith("k_spmm_dia<"):
        out.append(("window panels", False))   # one plan for every width
    if k1.startswith(("k_spmv_slab<", "k_spmv_sell<")):
        out.append((k1.split("<")[0], True))
    if kL.startswith("k_spmm_slab<"):
        out.append(("k_spmm_slab", True))
    return out


def probe(name, L, reps, ceiling_gbs):
    a = SHAPES[name]()
    nnz = a.num_nonzeros
    v1 = a.values * 1.0625
    a1 = mspmv.CsrMatrix.from_arrays(a.num_cols, a.row_offsets, a.column_indices, v1)
    x = np.random.default_rng(1).uniform(-1, 1, a.num_cols)
    X = np.random.default_rng(2).uniform(-1, 1, (a.num_cols, L))
    g = mspmv.GpuCsr(a)
    g.spmv(x)
    g.spmm(X)
    k1, kL = g.kernel_name(), g.spmm_kernel_name(L)
    # (a) the path without an update: a new handle on the new values, its plans built by the first products
    t0 = time.perf_counter()
    g.close()
    g = mspmv.GpuCsr(a1)
    g.spmv(x)
    g.spmm(X)
    recreate = (time.perf_counter() - t0) * 1e3
    assert (g.kernel_name(), g.spmm_kernel_name(L)) == (k1, kL)
    copies = derived_copies(g, L)
    # (b) the host-pointer form; the first update moves the source maps to the device
    g.update_values(a.values)
    host_first = g.update_ms()
    host = []
    for i in range(reps):
        g.update_values(v1 if i % 2 == 0 else a.values)
        host.append(g.update_ms())
    g.close()
    # (c) the device-pointer form, on a handle that has not been updated yet
    g = mspmv.GpuCsr(a)
    g.spmv(x)
    g.spmm(X)
    dV = mspmv.DeviceBuffer.from_array(v1)
    g.sync()
    t0 = time.perf_counter()
    g.update_values_dev(dV, sync=True)
    dev_first = (time.perf_counter() - t0) * 1e3
    g.update_values_dev(dV, sync=True)   # warm-up
    t0 = time.perf_counter()
    for _ in range(reps):
        g.update_values_dev(dV, sync=False)
    g.sync()
    dev = (time.perf_counter() - t0) * 1e3 / reps
    y = g.spmv(x)
    g.close()
    dV.free()
    with mspmv.GpuCsr(a1) as f:   # and it is the update: the fresh handle's product, bit for bit
        same = bool(np.array_equal(f.spmv(x).view(np.uint64), y.view(np.uint64)))
    floor_bytes = 16 * nnz + sum(16 * nnz + (4 * nnz if mapped else 0) for _, mapped in copies)
    floor = floor_bytes / (ceiling_gbs * 1e9) * 1e3
    return {"shape": name, "rows": a.num_rows, "nnz": nnz, "L": L, "reps": reps, "spmv_kernel": k1, "spmm_kernel": kL,
            "derived_copies": [c[0] for c in copies], "recreate_ms": round(recreate, 3),
            "update_first_ms": round(host_first, 3), "update_ms": round(statistics.median(host), 3),
            "update_dev_first_ms": round(dev_first, 3), "update_dev_ms": round(dev, 4),
            "floor_bytes": floor_bytes, "stream_read_gbs": round(ceiling_gbs, 1), "floor_ms": round(floor, 4),
            "dev_over_floor": round(dev / floor, 2), "recreate_over_dev": round(recreate / dev, 1),
            "matches_fresh_handle": same}


def main():
    opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or list(SHAPES)
    reps, L = int(opts.get("reps", 20)), int(opts.get("L", 8))
    out = opts.get("out", os.path.join(ROOT, "profiles", "update_values_probe.json"))
    ceiling = mspmv.time_stream_read(0)
    lines = []
    for name in names:
        lines.append(probe(name, L, reps, ceiling))
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(lines, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
