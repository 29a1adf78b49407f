"""GPU: a plain bench.py run (headline only, --steps honoured, ms_per_step) and --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mspmv

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# everything a plain run leaves to --full
FULL_ONLY = ("cpu_baseline", "speedup_vs_cpu", "hot_single_matrix", "merge_path", "scatter_band_stress",
             "spmv_pwtk_perturbed", "spmm16", "spmv_shapes", "window_shapes", "cg_single", "cg_multi",
             "spmv_nlpkkt120_size")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    return gpu_available


def test_plain_run_is_the_headline_alone_and_dumps_its_outputs(tmp_path):
    """`bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR`: one JSON line with the contract's fields,
    steps = 3, ms_per_step consistent with value, none of the --full legs; DIR/y<i>.npy hold the batch's y
    vectors, and y0 is A0 x0 for the seeded inputs: each row within 2 gamma_n (|A0| |x0|) of a float64 numpy
    product (gamma_n = n u / (1 - n u), n = the longest row, u = 2^-53: the bound of either summation order)."""
    import bench
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items()  # a plain run: no launcher, and the library's default plans
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK") and not k.startswith("MSPMV_")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["unit"] == "GFLOP/s" and d["higher_is_better"] is True and d["dtype"] == "f64" and d["metric"] == bench.METRIC
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["roofline"]["kernels_per_step"] == 4
    assert d["ms_per_step"] > 0
    flops_step = 2.0 * bench.PWTK["nnz"] * 4
    assert d["value"] == pytest.approx(flops_step / d["ms_per_step"] / 1e6, rel=1e-3)
    assert not [k for k in FULL_ONLY if k in d]
    assert "measured_read_GBps" not in d["roofline"]

    ys = [np.load(out / f"y{i}.npy") for i in range(4)]
    assert sorted(os.listdir(out)) == [f"y{i}.npy" for i in range(4)]
    for y in ys:
        assert y.dtype == np.float64 and y.shape == (bench.PWTK["m"],) and np.isfinite(y).all()
    p = bench.PWTK
    a = mspmv.CsrMatrix.synth_fem_blocked(p["m"], p["nnz"], p["block"], p["half_band_nodes"], seed=1)
    x = np.random.default_rng(2).uniform(0.0, 1.0, a.num_cols)
    lens = np.diff(a.row_offsets)
    assert lens.min() > 0
    prod = a.values * x[a.column_indices]
    ref = np.add.reduceat(prod, a.row_offsets[:-1])
    mag = np.add.reduceat(np.abs(prod), a.row_offsets[:-1])
    n, u = int(lens.max()), 2.0 ** -53
    assert np.all(np.abs(ys[0] - ref) <= 2 * n * u / (1 - n * u) * mag)
    assert not np.array_equal(ys[0], ys[1])  # distinct matrices of the batch
