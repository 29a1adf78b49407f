"""GPU: mspmv_csr_update_values -- a handle whose values were replaced on the same pattern against a handle freshly
created on the new values, bit for bit (view(np.uint64) equality), on every layout that keeps a copy of the values
(offset windows and their remainder, k_spmv_slab, k_spmv_sell packed and unpacked, k_spmm_slab, the register-resident
CG) and on those that keep none (merge tiles with split rows, node blocks, the run-balanced and one-wave plans).

The yardstick is always GpuCsr(A'), never a recomputation by the updated handle.  Every case first checks that two
fresh handles on A' agree bit for bit with each other; only a plan whose own result is not stable is compared within
gpu_common.check_parity's reordering bound instead (and the case prints which).

A' = perturbed(A): every unordered pair {i, j} of the pattern gets one factor 1 + 0.25 u, u ~ U[0, 1), shared by (i, j)
and (j, i), and the diagonal the factor 1.3 -- so a symmetric matrix stays symmetric and a diagonally dominant one
(sum |off-diagonal| + margin <= diagonal) stays so: 1.3 d >= 1.3 sum + 1.3 margin > 1.25 sum + margin.

This module is not among conftest's DEFAULT_PLAN_MODULES, so MSPMV_DIA=0 is set for it: the window cases unset it.
Every switch is set before the handle is created."""
import numpy as np
import pytest

import bicgstab_cases as bc
import blockcg_cases as bcg
import mspmv
import pcg_cases as pc
import resident_cases as rc
import slab_cases as sc
import test_bicgstab as tb
from gpu_common import check_parity

pytestmark = pytest.mark.gpu
CUS = 8  # the slab cases of slab_cases.py are cut for eight CUs (test_gpu_slab_edges.py)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    return gpu_available


# ---- matrices ------------------------------------------------------------------------------------------------------
def as_csr(a):
    """mspmv.CsrMatrix of a case given as one, or as (row_offsets, column_indices, values) of a square matrix."""
    if isinstance(a, mspmv.CsrMatrix):
        return a
    ro, ci, va = a
    return mspmv.CsrMatrix.from_arrays(len(ro) - 1, ro, ci, va)


def perturbed(a, seed=1):
    """The values of A' (module docstring), float64[nnz], in A's CSR order."""
    n = max(a.num_rows, a.num_cols)
    r = np.repeat(np.arange(a.num_rows, dtype=np.int64), np.diff(a.row_offsets.astype(np.int64)))
    c = a.column_indices.astype(np.int64)
    key, inv = np.unique(np.minimum(r, c) * n + np.maximum(r, c), return_inverse=True)
    f = 1.0 + 0.25 * np.random.default_rng(seed).uniform(0.0, 1.0, key.size)
    return np.where(r == c, 1.3, f[inv]) * a.values


def with_values(a, v):
    return mspmv.CsrMatrix.from_arrays(a.num_cols, a.row_offsets, a.column_indices, v)


def symmetrized(a):
    """The matrix with entry (i, j), i > j, replaced by entry (j, i) (a symmetric pattern): symmetric values."""
    n = a.num_rows
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(a.row_offsets.astype(np.int64)))
    c = a.column_indices.astype(np.int64)
    key = np.minimum(r, c) * n + np.maximum(r, c)
    up = r <= c
    order = np.argsort(key[up])
    pos = np.searchsorted(key[up][order], key)
    assert np.array_equal(key[up][order][pos], key)
    return with_values(a, a.values[up][order][pos])


_CASES = {}


def case(name):
    """(A, v1) of a named case, built once: bicgstab_cases, slab_cases, resident_cases and pcg_cases names, and
    "windows_sym" (bicgstab_cases' windows made symmetric, for the CG), "onewave" (test_gpu_spmv's skewed rows),
    "node_blocks6_spd" (pcg_cases' symmetric node_blocks6, for the block CG)."""
    if name not in _CASES:
        if name == "windows_sym":
            a = symmetrized(as_csr(tb.matrix("windows")))
        elif name == "onewave":
            a = mspmv.CsrMatrix.synth_powerlaw(60000, 60000, 1800000, exponent=1.2, seed=7)
        elif name == "node_blocks6_spd":
            a = pc.matrix("node_blocks6")
        elif name in bc.NAMES:
            a = as_csr(tb.matrix(name))
        elif name in sc.CASES:
            a = sc.matrix(name)
        elif name in rc.CASES:
            a = rc.matrix(name)
        elif name == "many_tiles":
            a = pc.matrix(name, 4)
        else:
            a = pc.matrix(name)
        v1 = perturbed(a)
        v1.setflags(write=False)
        _CASES[name] = (a, v1)
    return _CASES[name]


def x_for(a, L, seed=5):
    return np.random.default_rng(seed + L).uniform(-1, 1, a.num_cols if L == 1 else (a.num_cols, L))


# ---- comparisons ---------------------------------------------------------------------------------------------------
def bits(v):
    return np.ascontiguousarray(v, np.float64).view(np.uint64)


def same(label, got, want):
    diff = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert diff.size == 0, f"{label}: {diff.size} of {np.size(want)} entries differ in bits, first at {diff[:4]}"


def same_solve(label, got, want):
    (X, it, hist, st), (Xw, itw, histw, stw) = got, want
    assert (it, st) == (itw, stw), f"{label}: iterations / status {(it, st)} against {(itw, stw)}"
    same(label + " history", hist, histw)
    same(label + " X", X, Xw)


class Fresh:
    """Two fresh handles' product on (A', X): the yardstick, and whether the plan repeats itself across handles."""

    def __init__(self, label, a1, X, L, prepare=None):
        self.label, self.a1, self.X, self.L = label, a1, X, L
        outs = []
        for _ in range(2):
            with mspmv.GpuCsr(a1) as g:
                if prepare:
                    prepare(g)
                outs.append(product(g, X, L))
                self.plan = g.tile_plan(L)
        self.Y = outs[0]
        self.stable = bool(np.array_equal(bits(outs[0]), bits(outs[1])))
        if not self.stable:
            print(f"{label}: two fresh handles differ in bits -- this plan's own result is not stable; the updated "
                  f"handle is held to the reordering bound instead")

    def check(self, what, Y, orc):
        if self.stable:
            same(f"{self.label} {what}", Y, self.Y)
        else:
            X = self.X
            seq = orc.spmv_gold(self.a1, X) if self.L == 1 else orc.csr_spmm_t(self.a1, X)
            check_parity(self.a1, Y, seq, X, self.plan, self.L)


def product(g, X, L):
    return g.spmv(X) if L == 1 else g.spmm(X)


def kernel(g, L):
    return g.kernel_name() if L == 1 else g.spmm_kernel_name(L)


def queries(g, widths):
    """Everything the plan queries answer, for equality before and after an update."""
    out = {"spmv": g.kernel_name(), "setup_ms": g.setup_ms}
    for L in widths:
        p = g.tile_plan(L)
        out[L] = (g.spmm_kernel_name(L), p["num_tiles"], p["tile_items"], p["num_carries"], p["lanes"],
                  p["bounds"].tobytes(), p["modes"].tobytes(), g.slab_plan_stats(L))
    return out


def limit(g):
    g.set_cu_limit(CUS)


# ---- 1-3. the products, plan by plan ------------------------------------------------------------------------------
def set_switches(monkeypatch, name):
    if name.startswith("windows"):
        monkeypatch.delenv("MSPMV_DIA", raising=False)
    monkeypatch.setenv("MSPMV_SPMM_SLAB", "1" if name == "band" else "0")
    for v in ("MSPMV_SPMV_RUNS", "MSPMV_SPMV_SLAB", "MSPMV_SLAB_GROUPS"):
        monkeypatch.delenv(v, raising=False)
    if name != "onewave":   # (its plan is the default choice for skewed rows; nothing else here is a slab by default)
        monkeypatch.setenv("MSPMV_SPMV_SLAB", "0")


def expect_kernel(name, L, k, g):
    if name.startswith("windows"):
        assert k.startswith(f"k_spmm_dia<{L},"), k
    elif name == "band":
        assert k.startswith("k_spmm_slab<"), k
    elif name == "long_rows":
        assert k.startswith("k_spmv_tile<" if L == 1 else f"k_spmm_tile<{L},"), k
        assert g.tile_plan(L)["num_carries"] > 0
    elif name == "node_blocks":
        assert k.startswith("k_spmv_tile<" if L == 1 else f"k_spmm_tile<{L},"), k
        if L == 1:
            assert g.plan_block_tiles(1) > 0
    elif name == "node_blocks6":  # L = 1: the run-balanced node-block plan (tiles cut at run starts)
        assert k.startswith("k_spmv_blk<" if L == 1 else f"k_spmm_blk<{L},"), k
        if L == 1:
            p = g.tile_plan(1)
            assert p["num_carries"] == 0 and np.array_equal(case(name)[0].row_offsets[p["bounds"][:, 0]], p["bounds"][:, 1])
    elif name == "onewave":
        assert ",64," in k and g.tile_plan(1)["lanes"] == 64, k


PLAN_CASES = [(n, L) for n in ("windows", "windows_rem", "long_rows", "node_blocks", "node_blocks6") for L in (1, 8, 16)]
PLAN_CASES += [("band", 8), ("band", 16), ("onewave", 1)]


@pytest.mark.parametrize("name,L", PLAN_CASES)
def test_products(orc, monkeypatch, name, L):
    set_switches(monkeypatch, name)
    a, v1 = case(name)
    X = x_for(a, L)
    fresh = Fresh(f"{name} L={L}", with_values(a, v1), X, L)
    with mspmv.GpuCsr(a) as g:
        Y0 = product(g, X, L)   # builds the plan under test, on the old values
        k = kernel(g, L)
        expect_kernel(name, L, k, g)
        if name == "windows_rem":
            assert (g.tile_plan(L)["modes"] == 255).any()   # windows with remainder entries
        g.update_values(v1)
        Y1 = product(g, X, L)
        assert kernel(g, L) == k and g.update_ms() > 0.0
    print(f"{name} L={L}: {k}")
    assert not np.array_equal(bits(Y0), bits(Y1))
    fresh.check("after the update", Y1, orc)


# (case, MSPMV_SPMV_SLAB, MSPMV_SLAB_GROUPS, kernel stem, its second template argument, statistics that must be positive)
SLAB_CASES = [("slab_chunks", "1", None, "k_spmv_slab", "0", ["chunks_full", "chunks_long"]),
              ("slab_chunks", "2", None, "k_spmv_slab", "1", ["chunks_full"]),
              ("sell_edges", "4", 1, "k_spmv_sell", "false", ["unpacked_1", "long_1", "long_2"]),
              ("sell_one_seg", "4", None, "k_spmv_sell", "false", ["unpacked_8", "medium_2", "long_3plus"]),
              ("sell_packed", "4", None, "k_spmv_sell", "true", ["pack_8x1", "pack_2x4", "medium_8", "long_3plus",
                                                                 "slices_odd", "slices_partial"])]


def slab_env(monkeypatch, mode, groups):
    monkeypatch.setenv("MSPMV_SPMV_SLAB", mode)
    if groups is None:
        monkeypatch.delenv("MSPMV_SLAB_GROUPS", raising=False)
    else:
        monkeypatch.setenv("MSPMV_SLAB_GROUPS", str(groups))


@pytest.mark.parametrize("name,mode,groups,stem,tail,forms", SLAB_CASES, ids=[f"{c[0]}-{c[1]}" for c in SLAB_CASES])
def test_slab_spmv_forms(orc, monkeypatch, name, mode, groups, stem, tail, forms):
    slab_env(monkeypatch, mode, groups)
    a, v1 = case(name)
    x = x_for(a, 1)
    fresh = Fresh(f"{name} mode {mode}", with_values(a, v1), x, 1, prepare=limit)
    with mspmv.GpuCsr(a) as g:
        limit(g)
        y0 = g.spmv(x)
        k, st = g.kernel_name(), g.slab_plan_stats(1)
        assert k in (f"{stem}<true,{tail}>", f"{stem}<false,{tail}>"), k
        assert st is not None and not [f for f in forms if st[f] <= 0], st
        g.update_values(v1)
        y1 = g.spmv(x)
        assert g.kernel_name() == k and g.slab_plan_stats(1) == st
    assert not np.array_equal(bits(y0), bits(y1))
    fresh.check("after the update", y1, orc)


# ---- 4. lifecycle, one case per layout family ----------------------------------------------------------------------
LIFE = [("windows_rem", None, None), ("sell_packed", "4", limit), ("band", None, None), ("long_rows", None, None)]


@pytest.mark.parametrize("name,mode,prepare", LIFE, ids=[c[0] for c in LIFE])
def test_lifecycle(orc, monkeypatch, name, mode, prepare):
    set_switches(monkeypatch, name)
    if mode:
        slab_env(monkeypatch, mode, None)
    a, v1 = case(name)
    v0 = a.values
    x, X = x_for(a, 1), x_for(a, 16)
    a1 = with_values(a, v1)
    f1, f16 = Fresh(f"{name} L=1", a1, x, 1, prepare), Fresh(f"{name} L=16", a1, X, 16, prepare)
    # an update before any product has run, right after the create
    with mspmv.GpuCsr(a) as g:
        if prepare:
            prepare(g)
        g.update_values(v1)
        f1.check("updated before any product", g.spmv(x), orc)
        f16.check("updated before any product", g.spmm(X), orc)
    with mspmv.GpuCsr(a) as g:
        if prepare:
            prepare(g)
        y0 = g.spmv(x)                 # the L = 1 plan, built on v0
        before = queries(g, (1,))
        g.update_values(v1)
        y1, Y1 = g.spmv(x), g.spmm(X)  # ... refreshed; the L = 16 plan, built on v1
        after = queries(g, (1, 16))
        g.update_values(np.array(v0))
        y2, Y2 = g.spmv(x), g.spmm(X)  # both refreshed back
        back = queries(g, (1, 16))
        g.check_faults()
    f1.check("plan built before the update", y1, orc)
    f16.check("plan built after the update", Y1, orc)
    assert before["spmv"] == after["spmv"] and before[1] == after[1] and before["setup_ms"] == after["setup_ms"]
    want_k = {"windows_rem": ("k_spmm_dia<1,", "k_spmm_dia<16,"), "sell_packed": ("k_spmv_sell<", ""),
              "band": ("", "k_spmm_slab<"), "long_rows": ("k_spmv_tile<", "k_spmm_tile<16,")}[name]
    assert after["spmv"].startswith(want_k[0]) and after[16][0].startswith(want_k[1]), (after["spmv"], after[16][0])
    assert after == back
    # v0 -> v1 -> v0: the original outputs, against the untouched handle's own
    if f1.stable:
        same(f"{name} L=1 back on v0", y2, y0)
    with mspmv.GpuCsr(a) as g:
        if prepare:
            prepare(g)
        Y0 = g.spmm(X)
    if f16.stable:
        same(f"{name} L=16 back on v0", Y2, Y0)
    assert not np.array_equal(bits(y0), bits(y1))


# ---- 5. non-finite values ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode,prepare", LIFE[:2], ids=[c[0] for c in LIFE[:2]])
def test_nonfinite_values(monkeypatch, name, mode, prepare):
    """One Inf and one NaN among the new values: the update does not look at them.  NaN positions equal the fresh
    handle's, everything else bit for bit."""
    set_switches(monkeypatch, name)
    if mode:
        slab_env(monkeypatch, mode, None)
    a, v1 = case(name)
    vp = np.array(v1)
    vp[a.row_offsets[a.num_rows // 3]] = np.inf
    vp[a.row_offsets[2 * a.num_rows // 3 + 1] - 1] = np.nan
    x = x_for(a, 1)
    outs = []
    for _ in range(2):
        with mspmv.GpuCsr(with_values(a, vp)) as g:
            if prepare:
                prepare(g)
            outs.append(g.spmv(x))
    with mspmv.GpuCsr(a) as g:
        if prepare:
            prepare(g)
        g.spmv(x)
        g.update_values(vp)
        y = g.spmv(x)
    want = outs[0]
    assert np.isnan(want).any() and np.isinf(want).any()
    assert np.array_equal(np.isnan(outs[1]), np.isnan(want)) and np.array_equal(np.isnan(y), np.isnan(want))
    ok = ~np.isnan(want)
    same(f"{name} with Inf and NaN: two fresh handles", outs[1][ok], want[ok])   # the yardstick repeats itself
    same(f"{name} with Inf and NaN", y[ok], want[ok])


# ---- 6. stream order -----------------------------------------------------------------------------------------------
ORDER = [("windows_rem", 8, None, None), ("sell_packed", 1, "4", limit), ("band", 16, None, None),
         ("node_blocks6", 8, None, None)]


@pytest.mark.parametrize("name,L,mode,prepare", ORDER, ids=[c[0] for c in ORDER])
def test_stream_order(monkeypatch, name, L, mode, prepare):
    """product (old values), update, product (new values) enqueued with no sync in between: after one sync the first
    output is a fresh handle's on A and the second a fresh handle's on A'."""
    set_switches(monkeypatch, name)
    if mode:
        slab_env(monkeypatch, mode, None)
    a, v1 = case(name)
    X = x_for(a, L)
    want = []
    for m in (a, with_values(a, v1)):
        with mspmv.GpuCsr(m) as g:
            if prepare:
                prepare(g)
            want.append(product(g, X, L))
    shape = X.shape if L > 1 else (a.num_rows,)
    with mspmv.GpuCsr(a) as g:
        if prepare:
            prepare(g)
        dX, dV = mspmv.DeviceBuffer.from_array(X), mspmv.DeviceBuffer.from_array(v1)
        dY = [mspmv.DeviceBuffer(8 * a.num_rows * L) for _ in range(2)]
        g.spmm_dev(dX, dY[0], L, sync=True)   # the plan exists before the sequence: nothing below builds one
        dY[0].fill_bytes(0)
        g.spmm_dev(dX, dY[0], L, sync=False)
        g.update_values_dev(dV, sync=False)
        g.spmm_dev(dX, dY[1], L, sync=False)
        g.sync()
        got = [d.download(shape) for d in dY]
        g.check_faults()
        for d in [dX, dV] + dY:
            d.free()
    same(f"{name} L={L} enqueued before the update", got[0], want[0])
    same(f"{name} L={L} enqueued after the update", got[1], want[1])


# ---- 7. solvers over their cached graphs ---------------------------------------------------------------------------
def solve_cg(g, m, B, iters):
    return g.cg_multi(B, iters, pc.TOL, hist_cap=iters)


def solve_bicgstab(g, m, B, iters):
    return g.bicgstab(B, iters, bc.TOL, hist_cap=iters)


def solve_bcg(g, m, B, iters):
    return g.block_cg(B, iters, bcg.TOL, hist_cap=iters)


def solve_pcg(g, m, B, iters):
    return g.pcg_spai(m, B, iters, pc.TOL, hist_cap=iters)


def jacobi(a, v):
    """The Jacobi preconditioner of (a's pattern, values v) as pcg_cases.preconditioner(.., "jacobi") builds it."""
    n = a.num_rows
    return mspmv.CsrMatrix.from_arrays(n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32),
                                       1.0 / pc.diagonal(with_values(a, v)))


SOLVES = [("cg_multi", "windows_sym", 8, solve_cg, "k_spmm_dia<8,"), ("bicgstab", "band", 8, solve_bicgstab, "k_spmm_slab<"),
          ("block_cg", "node_blocks6_spd", 4, solve_bcg, "k_spmm_blk<4,"), ("pcg_spai", "many_tiles", 4, solve_pcg, None)]


@pytest.mark.parametrize("solver,name,L,solve,kstem", SOLVES, ids=[c[0] for c in SOLVES])
def test_solvers_replay_their_graph(monkeypatch, solver, name, L, solve, kstem):
    """Solve on A, update, solve again (the cached graph, replayed): iterations, history and X of a fresh handle's
    solve on A', bit for bit."""
    set_switches(monkeypatch, name)
    a, v1 = case(name)
    B = np.random.default_rng(70 + L).uniform(0.0, 1.0, (a.num_rows, L))
    pre = solver == "pcg_spai"
    fresh = []
    for _ in range(2):
        with mspmv.GpuCsr(with_values(a, v1)) as g:
            iters = max(200, g.solver_pass_shape(L)[1])
            m = mspmv.GpuCsr(jacobi(a, v1)) if pre else None
            fresh.append(solve(g, m, B, iters))
            if m:
                m.close()
    same_solve(f"{solver} {name}: two fresh handles on A'", fresh[1], fresh[0])   # the yardstick repeats itself
    with mspmv.GpuCsr(a) as g:
        assert iters >= g.solver_pass_shape(L)[1]   # whole batches: the graph path
        m = mspmv.GpuCsr(jacobi(a, a.values)) if pre else None
        out0 = solve(g, m, B, iters)
        k0 = (g.cg_kernel_name(), g.solver_product_kernel_name(), g.spmm_kernel_name(L))
        g.update_values(v1)
        if m:
            m.update_values(jacobi(a, v1).values)
        out1 = solve(g, m, B, iters)
        assert (g.cg_kernel_name(), g.solver_product_kernel_name(), g.spmm_kernel_name(L)) == k0
        if m:
            m.close()
    print(f"{solver} on {name} L={L}: {k0}, {out0[1]} iterations on A, {out1[1]} on A' (fresh {fresh[0][1]})")
    if kstem:
        assert any(k.startswith(kstem) for k in k0[1:]), k0
    assert out0[3] == 0 and out1[3] == 0 and out0[1] > 1
    assert not np.array_equal(bits(out0[0]), bits(out1[0]))
    same_solve(f"{solver} {name}", out1, fresh[0])


# ---- 8. the register-resident CG -----------------------------------------------------------------------------------
def test_resident_cg():
    a, v1 = case("s14")   # the smallest shape of resident_cases that takes k_cg_resident
    b = rc.rhs(a.num_rows)
    with mspmv.GpuCsr(with_values(a, v1)) as g:
        want = g.cg_single(b, rc.MAX_ITERS, rc.TOL, hist_cap=rc.MAX_ITERS)
        assert g.cg_kernel_name().startswith("k_cg_resident<"), g.cg_kernel_name()
    with mspmv.GpuCsr(with_values(a, v1)) as g:
        again = g.cg_single(b, rc.MAX_ITERS, rc.TOL, hist_cap=rc.MAX_ITERS)
    with mspmv.GpuCsr(a) as g:
        out0 = g.cg_single(b, rc.MAX_ITERS, rc.TOL, hist_cap=rc.MAX_ITERS)
        k = g.cg_kernel_name()
        g.update_values(v1)
        out1 = g.cg_single(b, rc.MAX_ITERS, rc.TOL, hist_cap=rc.MAX_ITERS)
        assert g.cg_kernel_name() == k and k.startswith("k_cg_resident<"), (k, g.cg_kernel_name())
    assert out0[3] == 0 and out1[3] == 0 and not np.array_equal(bits(out0[0]), bits(out1[0]))
    same_solve("resident CG: two fresh handles on A'", again, want)   # the yardstick repeats itself
    same_solve("resident CG", out1, want)


# ---- 9. no nonzeros ------------------------------------------------------------------------------------------------
def test_empty_matrix():
    a = mspmv.CsrMatrix.from_arrays(5, np.zeros(4, np.int32), np.zeros(0, np.int32), np.zeros(0))
    with mspmv.GpuCsr(a) as g:
        g.update_values(np.zeros(0))
        d = mspmv.DeviceBuffer(8)
        g.update_values_dev(d)
        d.free()
        assert g.update_ms() >= 0.0
