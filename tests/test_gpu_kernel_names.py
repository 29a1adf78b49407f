"""GPU: the exact kernel names the library reports, one case per branch of each kernel pick.

mspmv_spmv_kernel_name, mspmv_spmm_kernel_name and mspmv_solver_product_kernel_name format the same pick the launchers
launch from (pick_tile_kernel / tile_kernel_name in mspmv_kernels.hip, the offset-window and column-slab picks in
mspmv_dia.hip and mspmv_slab.hip, product_kernel_name over them).  The coverage assertions of some twenty GPU test
files, bench.py's traffic attribution and smoke() read these strings, so the table below holds each one whole, as
recorded on an MI355X before the names were moved onto the picks: a change of a launcher that changes a name shows
here, on purpose or not.

The switches set here (MSPMV_DIA, MSPMV_SPMV_RUNS, MSPMV_SPMV_SLAB, MSPMV_SPMM_SLAB) are read at each handle's
decision, so monkeypatch sets them.  No case runs a nontemporal (`true`) form: those need a matrix above 128 MiB and
stay covered by test_gpu_fullsize.py and the benchmark alone; the flag reaches both pick and name from the same
stream_nt call.
"""
import numpy as np
import pytest

import mspmv
import slab_cases as sc
from test_gpu_nonfinite import matrix as nf_matrix

pytestmark = pytest.mark.gpu

SWITCHES = ("MSPMV_DIA", "MSPMV_SPMV_RUNS", "MSPMV_SPMV_SLAB", "MSPMV_SLAB_GROUPS", "MSPMV_SPMM_SLAB")
SLAB_CUS = 8  # the slab_cases matrices fill a block on eight CUs (test_gpu_slab_edges.py)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    return gpu_available


def matrix(name):
    if name == "stencil":  # smoke()'s: SPD, takes the offset windows
        return mspmv.CsrMatrix.synth_stencil(0, 3000, 55)
    if name == "no_rows":
        return mspmv.CsrMatrix(0, 0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    if name.startswith("slab:"):
        return sc.matrix(name[5:])
    return nf_matrix(name)


# (matrix, environment, query, the whole name).  Queries: ("spmv",), ("spmm", L), and the solver product after two
# iterations of ("bicgstab", L) or ("block_cg", L).
CASES = [
    # ---- SpMV: windows, one-wave tiles, tiles with and without split rows, node blocks, slabs, sliced ELL, no rows
    ("stencil", {}, ("spmv",), "k_spmm_dia<1,false>"),
    ("powerlaw_onewave", {}, ("spmv",), "k_spmv_tile<8,0,false,64,true,true>"),
    ("long_rows_many_tiles", {}, ("spmv",), "k_spmv_tile<8,0,false,256,true,true>"),
    ("stencil_rows", {"MSPMV_DIA": "0"}, ("spmv",), "k_spmv_tile<8,0,false,256,true,false>"),
    ("fem_52_53", {}, ("spmv",), "k_spmv_blk<0,false,6,false>"),
    ("fem_52_53", {"MSPMV_SPMV_RUNS": "0"}, ("spmv",), "k_spmv_blk<0,false,6,false>"),
    ("fallback", {}, ("spmv",), "k_spmv_blk<0,false,6,true>"),
    ("slab:slab_chunks", {"MSPMV_SPMV_SLAB": "1"}, ("spmv",), "k_spmv_slab<false,0>"),
    ("slab:slab_chunks", {"MSPMV_SPMV_SLAB": "2"}, ("spmv",), "k_spmv_slab<false,1>"),
    ("slab:sell_packed", {"MSPMV_SPMV_SLAB": "4"}, ("spmv",), "k_spmv_sell<false,true>"),
    ("slab:sell_one_seg", {"MSPMV_SPMV_SLAB": "4"}, ("spmv",), "k_spmv_sell<false,false>"),
    ("no_rows", {}, ("spmv",), "k_spmv_tile<8,0,false,256,true,false>"),
    # ---- SpMM: the tile depths 8, 8, 24, 32 with split rows (powerlaw) and without (fem2d), the dictionary form,
    # node blocks, windows, slabs, and the chunk width of widths that are not native
    ("powerlaw", {}, ("spmm", 2), "k_spmm_tile<2,8,0,false,false,true>"),
    ("powerlaw", {}, ("spmm", 4), "k_spmm_tile<4,8,0,false,false,true>"),
    ("powerlaw", {}, ("spmm", 8), "k_spmm_tile<8,24,0,false,false,true>"),
    ("powerlaw", {}, ("spmm", 16), "k_spmm_tile<16,32,0,false,false,true>"),
    ("powerlaw", {}, ("spmm", 3), "k_spmm_tile<4,8,0,false,false,true>"),
    ("powerlaw", {}, ("spmm", 32), "k_spmm_tile<16,32,0,false,false,true>"),
    ("fem2d", {"MSPMV_DIA": "0"}, ("spmm", 4), "k_spmm_tile<4,8,0,false,false,false>"),
    ("fem2d", {"MSPMV_DIA": "0"}, ("spmm", 8), "k_spmm_tile<8,24,0,false,false,false>"),
    ("dict16", {}, ("spmm", 16), "k_spmm_tile<16,32,0,false,true,true>"),
    ("kron9_6", {}, ("spmm", 2), "k_spmm_blk<2,0,false,6>"),
    ("kron9_6", {}, ("spmm", 16), "k_spmm_blk<16,0,false,6>"),
    ("stencil", {}, ("spmm", 8), "k_spmm_dia<8,false>"),
    ("band", {"MSPMV_SPMM_SLAB": "1"}, ("spmm", 8), "k_spmm_slab<0,false>"),
    ("band", {"MSPMV_SPMM_SLAB": "1"}, ("spmm", 16), "k_spmm_slab<2,false>"),
    # ---- the solvers' product: windows, slab, node blocks, tiles
    ("stencil", {}, ("bicgstab", 4), "k_spmm_dia<4,false>"),
    ("stencil", {}, ("block_cg", 4), "k_spmm_dia<4,false>"),
    ("band", {"MSPMV_SPMM_SLAB": "1"}, ("bicgstab", 8), "k_spmm_slab<0,false>"),
    ("kron9_6", {}, ("bicgstab", 1), "k_spmv_blk<0,false,6,false>"),
    ("kron9_6", {}, ("bicgstab", 4), "k_spmm_blk<4,0,false,6>"),
    ("powerlaw", {}, ("bicgstab", 1), "k_spmv_tile<8,0,false,256,true,true>"),
    ("powerlaw", {}, ("bicgstab", 4), "k_spmm_tile<4,8,0,false,false,true>"),
]


def case_id(c):
    env = "".join(f"-{k[6:].lower()}{v}" for k, v in c[1].items())
    return f"{c[0]}{env}-{'-'.join(str(q) for q in c[2])}"


def reported(a, query, g):
    """The name `query` reports on handle g of matrix a."""
    if query[0] == "spmv":
        return g.kernel_name()
    if query[0] == "spmm":
        return g.spmm_kernel_name(query[1])
    B = np.random.default_rng(5).uniform(-1, 1, (a.num_rows, query[1]))
    getattr(g, query[0])(B, 2, 1e-30)
    return g.solver_product_kernel_name()


def observe(mat, env, query, setenv, delenv):
    for name in SWITCHES:
        delenv(name)
    for name, value in env.items():
        setenv(name, value)
    a = matrix(mat)
    with mspmv.GpuCsr(a) as g:
        if mat.startswith("slab:"):
            g.set_cu_limit(SLAB_CUS)
        return reported(a, query, g)


@pytest.mark.parametrize("mat,env,query,want", CASES, ids=[case_id(c) for c in CASES])
def test_reported_kernel_name(monkeypatch, mat, env, query, want):
    got = observe(mat, env, query, monkeypatch.setenv, lambda n: monkeypatch.delenv(n, raising=False))
    assert got == want
