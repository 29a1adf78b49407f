"""GPU: SPAI-PCG and IC(0)-PCG on every dot-mode form of the tile kernels -- the only single-GPU callers of
launch_spmm_dot (plain multi-RHS CG takes the plain SpMM and a streaming p.Ap pass) -- on the matrices and
preconditioners of pcg_cases.py, against the oracle's restatements (orc_pcg_spai_multi, orc_pcg_ic0_multi) and, where
M's pattern is not A's, against pcg_cases.pcg_reference (what these tests rely on is pinned by test_pcg_cases.py).

Each case asserts its form from the plan queries before it is used, never skips on it:
  long_rows          num_carries > 0 at L = 1, 4, 16 (and 8 under the CU limit), on A and on the M of its pattern:
                     k_spmv_tile<kModeDot> and k_spmm_tile<L, I, kModeDot> with split rows
  many_tiles         65 <= num_tiles <= 127 and odd at L = 1 and 4: k_fold_dot on two blocks, the second short;
                     "jacobi" has fewer tiles than A and "wide" more (partials sized by the larger plan)
  dict16             dict_tiles(16) > 0: k_spmm_tile<16, 32, kModeDot, NT, true>
  node_blocks6       plan_block_tiles(L) == num_tiles: k_spmv_blk<kModeDot> at L = 1, k_spmm_blk<8, kModeDot, NT, 6>
                     at L = 8 (the form without the 6 is unreachable: see pcg_cases.py)
  node_blocks_mixed  plan_block_tiles(1) > 0 and num_carries > 0: the tile kernel staging node blocks, with carries
                     (L = 1), and the L = 8 merge tiles with carries
The queries answer for the plain product's plan (product_plan(h, L)); the solvers call solver_plan(h, L).
At L > 1 the two differ only by windows and slabs (and the run-balanced node-block plan, which
is taken only where every tile of the solver's plan is a register run tile already); at L = 1 also by the one-wave
plan, which the L = 1 cases rule out by asserting 256 lanes.

This module is not among conftest's DEFAULT_PLAN_MODULES, so MSPMV_DIA=0 is set for it.  That changes nothing the
solvers do: both PCGs call solver_plan(h, L) and solver_plan(hm, L) (cg_solve_native), which
never returns the offset windows or a column slab; it only keeps the handles of the stencil cases from taking
windows for the plain products these tests interleave.

Measured on an MI355X, worst over each test's cases and over two runs (bar): test_one_iteration_dots |X - alpha* Z*|
0.033 of the bound (long_rows L = 16 "neumann"; the stencils 1e-5, the bound being the worst case of an n-term dot),
first residual 4.4e-16 (1e-10); test_every_form history 1.3e-15 (1e-10), ||X - X_ref|| / ||X_ref|| 3.2e-16 per column
(1e-8), every iteration count the reference's; test_cu_limit 1.5e-16, 1.4e-16, the same on 64 CUs;
test_frozen_columns_stay_frozen 1.3e-15, 2.6e-16; test_zero_column 4.9e-16, 1.4e-16 on the live columns.  Plans seen:
long_rows 6 / 15 / 10 / 15 carries at L = 1 / 4 / 8 / 16, many_tiles 67 and 81 tiles (M: 18 and 21 "jacobi", 138 and
167 "wide"), dict16 182 of 182 tiles on dictionaries, node_blocks6 86 of 86 tiles node blocks, node_blocks_mixed 160
of 197 with 1 carry at L = 1 and 2 carries at L = 8.

test_zero_column found a defect, fixed with it: when the p.Ap test freezes the last live column (cg_alpha_finish) the
solve stops before the update that records the iteration's history entry, and the entry returned was whatever an
earlier solve had left in the buffer (cg_solve_native now writes the reference's value).
"""
import numpy as np
import pytest

import pcg_cases as pc
from gpu_common import EPS, abs_bound
from pcg_cases import MAX_ITERS, TOL

pytestmark = pytest.mark.gpu
BREAKDOWN = 4
SOLVES = pc.solves()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    return gpu_available


def _id(case):
    return "-".join(str(v) for v in case)


class Run:
    """A's handle and the preconditioner's: M's handle (SPAI-PCG) or the IC(0) factor on the device."""

    def __init__(self, mspmv, name, L, kind):
        self.mspmv, self.name, self.L, self.kind = mspmv, name, L, kind
        self.a = pc.matrix(name, L)
        self.m = None if kind == "ic0" else pc.preconditioner(name, L, kind)
        self.ga = mspmv.GpuCsr(self.a)
        self.gm = self.ic = None
        if kind == "ic0":
            self.ic = mspmv.GpuIc0(pc.ic0(name, L))
        else:
            self.gm = mspmv.GpuCsr(self.m)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for h in (self.ic, self.gm, self.ga):
            if h is not None:
                h.close()

    def solve(self, B, max_iters=MAX_ITERS):
        if self.ic is not None:
            out = self.mspmv.pcg_ic0(self.ga, self.ic, B, max_iters, TOL, hist_cap=MAX_ITERS)
            assert self.ga.cg_kernel_name() == "IC0-PCG (split)"
        else:
            out = self.ga.pcg_spai(self.gm, B, max_iters, TOL, hist_cap=MAX_ITERS)
            assert self.ga.cg_kernel_name() == "SPAI-PCG (split)"
        return out

    def products(self, X0):
        """The plain products A X0 and M X0 (None with IC(0)) on the two handles."""
        one = X0.shape[1] == 1
        return [None if g is None else g.spmv(X0[:, 0])[:, None] if one else g.spmm(X0) for g in (self.ga, self.gm)]

    def reference(self, orc, B=None):
        if self.kind in pc.OFF_PATTERN:
            assert B is None
            return pc.reference(self.name, self.L, self.kind)
        return pc.oracle_solve(orc, self.name, self.L, self.kind, B)


def check_form(s, L=None):
    """The form the case is in the table for, from the plan queries, on A's handle (and on M's where M is on A's
    pattern); returns what it printed."""
    L = s.L if L is None else L
    name = s.name
    on_pattern = [g for g in (s.ga, s.gm if s.kind in ("spai", "neumann") else None) if g is not None]
    plans = [g.tile_plan(L) for g in on_pattern]
    said = f"{name} L={L} {s.kind}: " + ", ".join(
        f"{p['num_tiles']} tiles / {p['num_carries']} carries / {g.plan_block_tiles(L)} node-block tiles / "
        f"{g.dict_tiles(L)} dictionary tiles ({g.kernel_name() if L == 1 else g.spmm_kernel_name(L)})"
        for g, p in zip(on_pattern, plans))
    if s.kind in pc.OFF_PATTERN:
        said += f"; M {s.gm.tile_plan(L)['num_tiles']} tiles"
    print(said)
    for g, p in zip(on_pattern, plans):
        if L == 1 and name != "staggered":
            # tile_plan(1) then answers for a workgroup plan of merge tiles, as the solver's is
            assert p["lanes"] == 256 and g.kernel_name().startswith(("k_spmv_tile<", "k_spmv_blk<")), g.kernel_name()
        if name == "long_rows":
            assert p["num_carries"] > 0
        elif name == "many_tiles":
            assert 65 <= p["num_tiles"] <= 127 and p["num_tiles"] % 2 == 1, p["num_tiles"]
        elif name == "dict16":
            assert g.dict_tiles(16) > 0
        elif name == "node_blocks6":
            assert g.plan_block_tiles(L) == p["num_tiles"] > 0 and np.all(p["modes"] == 255)
            if L > 1:
                assert g.spmm_kernel_name(L).startswith(f"k_spmm_blk<{L},") and g.spmm_kernel_name(L).endswith(",6>")
        elif name == "node_blocks_mixed":
            assert g.plan_block_tiles(1) > 0 and g.tile_plan(1)["num_carries"] > 0
            assert g.plan_block_tiles(1) < g.tile_plan(1)["num_tiles"]
            if L > 1:
                assert p["num_carries"] > 0 and g.spmm_kernel_name(L).startswith(f"k_spmm_tile<{L},")
    if s.kind == "jacobi":
        assert s.gm.tile_plan(L)["num_tiles"] < plans[0]["num_tiles"]
    if s.kind == "wide":
        assert s.gm.tile_plan(L)["num_tiles"] > plans[0]["num_tiles"]
    return said


def same_bits(out, out2):
    (X, it, hist, st), (X2, it2, hist2, st2) = out, out2
    assert it2 == it and st2 == st
    np.testing.assert_array_equal(X2, X)
    np.testing.assert_array_equal(hist2, hist)


@pytest.mark.parametrize("case", SOLVES, ids=_id)
def test_one_iteration_dots(mspmv, case):
    """A solve cut at one iteration (below cg_batch_iters: no graph) returns X = alpha Z, one rounded multiply per
    element: the two dot-mode products and their folds, isolated.  |X - alpha* Z*| <= pcg_cases.one_iteration's
    bound elementwise -- derived there, not tuned; a hub row's share of either dot counted twice or not at all moves
    alpha by over 100 times the bound (test_pcg_cases.test_probe_sensitivity) -- and the first residual within 1e-10 of
    the restatement's.  With IC(0) only the denominator is a dot-mode product (Z comes from the triangular solves).
    Measured: at worst 0.033 of the bound (long_rows, L = 16, "neumann"), first residual within 4.4e-16."""
    name, L, kind = case
    B = pc.rhs(name, L)
    with Run(mspmv, name, L, kind) as s:
        X, it, hist, st = s.solve(B, max_iters=1)
        check_form(s)
    p = pc.probe(name, L, kind)
    err = np.abs(X.astype(pc.LD) - p["x"])
    ratio = float(np.max(np.where(p["x_bound"] > 0, err / np.where(p["x_bound"] > 0, p["x_bound"], 1), 0)))
    hdev = abs(hist[0] - p["hist0"]) if len(hist) else np.inf
    print(f"{name} L={L} {kind}: worst |X - alpha* Z*| / bound = {ratio:.3g}, first residual {hist[:1]} against "
          f"{p['hist0']:.17g} ({hdev:.3e}, bar 1e-10)")
    assert st == 0 and it == 1 and len(hist) == 1
    assert np.all(err <= p["x_bound"]), f"{int(np.sum(err > p['x_bound']))} elements past the bound, worst {ratio:.3g}"
    assert hdev <= 1e-10


@pytest.mark.parametrize("case", SOLVES, ids=_id)
def test_every_form(mspmv, orc, case):
    """The full solve on each form, against the oracle (pcg_reference for "jacobi" and "wide") under the project's
    parity bars, twice on its handles -- the second replays the cached graph and must repeat bit for bit.  The plain
    products of A's handle and of M's are taken before, between and after the solves and never change by a bit: the
    stream swap, the tickets and the carries of a solve leave nothing behind, and a plain product leaves nothing a
    solve trips over.  (And they are the products: within gpu_common.check_parity's reordering bound.)"""
    name, L, kind = case
    B = pc.rhs(name, L)
    X0 = np.random.default_rng(200 + L).uniform(-1, 1, B.shape)
    with Run(mspmv, name, L, kind) as s:
        check_form(s)
        Y0 = s.products(X0)
        out = s.solve(B)
        Y1 = s.products(X0)
        out2 = s.solve(B)
        Y2 = s.products(X0)
        ref = s.reference(orc)
    pc.check_bars(f"{name} L={L} {kind}", ref, out)
    same_bits(out, out2)
    for mat, y0, y1, y2 in zip((s.a, s.m), Y0, Y1, Y2):
        if mat is None:
            continue
        np.testing.assert_array_equal(y1, y0)
        np.testing.assert_array_equal(y2, y0)
        bound, lens = abs_bound(mat, X0)
        assert np.all(np.abs(y0 - pc.csr_mm(mat, X0)) <= 2.0 * (lens[:, None] + 1) * EPS * bound + 1e-300)


def test_preconditioner_swap(mspmv):
    """One A handle solved with M1 (SPAI), then M2 (the Neumann M: other values on the same pattern), then M1 again:
    each result equals, bit for bit, what fresh handles give.  The graph key holds hm, hm->d_vals, hm->gen and
    mplan; a stale graph would apply the old M and still converge."""
    name, L = "many_tiles", 4
    B = pc.rhs(name, L)
    a = pc.matrix(name, L)
    ms = [pc.preconditioner(name, L, "spai"), pc.preconditioner(name, L, "neumann")]
    fresh = []
    for m in ms:
        with mspmv.GpuCsr(a) as ga, mspmv.GpuCsr(m) as gm:
            fresh.append(ga.pcg_spai(gm, B, MAX_ITERS, TOL, hist_cap=MAX_ITERS))
    with mspmv.GpuCsr(a) as ga, mspmv.GpuCsr(ms[0]) as g1, mspmv.GpuCsr(ms[1]) as g2:
        shared = [ga.pcg_spai(g, B, MAX_ITERS, TOL, hist_cap=MAX_ITERS) for g in (g1, g2, g1)]
    print(f"swap: iterations {[o[1] for o in shared]} on the shared handle, {[o[1] for o in fresh]} on fresh ones")
    assert fresh[0][3] == 0 and fresh[1][3] == 0
    assert not np.array_equal(fresh[0][0], fresh[1][0])  # the two preconditioners do give different solves
    same_bits(shared[0], fresh[0])
    same_bits(shared[1], fresh[1])
    same_bits(shared[2], fresh[0])


@pytest.mark.parametrize("kind", [pc.SPAI_KIND["long_rows"], "ic0"])
def test_cu_limit(mspmv, orc, kind):
    """long_rows at L = 8: after set_cu_limit(64) on both handles the plans are rebuilt for 64 CUs (the split rows
    may fall elsewhere, so the bits may differ from the full device's): the bars hold again and the solve repeats."""
    name, L = "long_rows", 8
    B = pc.rhs(name, L)
    with Run(mspmv, name, L, kind) as s:
        out = s.solve(B)
        check_form(s)
        for g in (s.ga, s.gm):
            if g is not None:
                g.set_cu_limit(64)
        lim = s.solve(B)
        check_form(s)
        lim2 = s.solve(B)
        ref = s.reference(orc)
    pc.check_bars(f"{name} L={L} {kind}", ref, out)
    pc.check_bars(f"{name} L={L} {kind} on 64 CUs", ref, lim)
    same_bits(lim, lim2)


@pytest.mark.parametrize("kind", [pc.SPAI_KIND["staggered"], "ic0"])
def test_frozen_columns_stay_frozen(mspmv, orc, kind):
    """staggered: columns 0 and 2 converge in 3 iterations, columns 1 and 3 dozens later.  A solve cut at 8
    iterations launches what the full solve's first 8 launch, kernel for kernel (solve_batches: a batch below
    cg_batch_iters is launched one iteration at a time through the same launch_pcg_iteration / launch_pcg_ic0_iteration
    the graph captured), so its columns 0 and 2 hold the full solve's bits: a fold or a pass that lacked the
    converged-column mask would go on moving them -- towards the solution, past every other bar."""
    name, L, cut = "staggered", 4, 8
    B = pc.rhs(name, L)
    conv_at = pc.reference(name, L, kind)[3]
    assert conv_at[[0, 2]].max() + 1 + 3 <= cut <= conv_at[[1, 3]].min() - 2
    with Run(mspmv, name, L, kind) as s:
        out = s.solve(B)
        out2 = s.solve(B)
        X8, it8, h8, st8 = s.solve(B, max_iters=cut)
        ref = s.reference(orc)
    pc.check_bars(f"{name} L={L} {kind}", ref, out)
    same_bits(out, out2)
    X, it, hist, st = out
    assert st8 == 0 and it8 == cut and it > cut + 2
    np.testing.assert_array_equal(h8, hist[:cut])
    np.testing.assert_array_equal(X8[:, [0, 2]], X[:, [0, 2]])
    moved = np.abs(X8[:, [1, 3]] - X[:, [1, 3]]).max()
    print(f"staggered {kind}: columns 1 and 3 moved by {moved:.3e} after iteration {cut}, columns 0 and 2 by nothing")
    assert moved > 0.0


def zero_column_spai(mspmv, orc):
    """long_rows, L = 4, column 1 of B zero, SPAI-PCG: R.Z = P.AP = 0 there, kFoldPcgAlpha gives alpha = 0 and
    kFoldPcgBeta beta = 0, the column's residual is 0 < tol at the first iteration -- what the oracle does: status 0,
    its iterations and history, X exactly 0 in that column.  Alone (L = 1) it converges in one iteration, as in the
    oracle."""
    name, L, kind = "long_rows", 4, pc.SPAI_KIND["long_rows"]
    B = pc.rhs(name, L).copy()
    B[:, 1] = 0.0
    with Run(mspmv, name, L, kind) as s:
        out = s.solve(B)
        out2 = s.solve(B)
        alone = s.solve(B[:, 1:2])
        ref, ref1 = s.reference(orc, B), s.reference(orc, B[:, 1:2])
    assert np.all(ref[0][:, 1] == 0.0) and ref1[1] == 1 and list(ref1[2]) == [0.0] and np.all(ref1[0] == 0.0)
    pc.check_bars(f"{name} L={L} {kind}, column 1 zero", ref, out, cols=[0, 2, 3])
    same_bits(out, out2)
    assert np.all(out[0][:, 1] == 0.0)
    X1, it1, h1, st1 = alone
    assert st1 == 0 and it1 == 1 and list(h1) == [0.0] and np.all(X1 == 0.0)


def zero_column_ic0(mspmv, orc):
    """The same right-hand side under IC(0)-PCG, which has no guard (PCGSolveMultiple): the oracle's column 1 is
    0 / 0 = NaN from the first alpha on, skipped by the max-residual history (std::max) and never converged, so
    the oracle runs to max_iters.  Here cg_alpha_column freezes the column (kConvBroken) at X = 0, its exact solution,
    the solve stops when the other columns have converged and reports MSPMV_ERR_BREAKDOWN; the history is the
    oracle's on those iterations and the other columns meet the bars (test_cg_multi_zero_column_breaks_down_alone's
    rule for the plain CG).  Alone (L = 1), on a handle whose history buffer holds an earlier solve's residuals, the
    column breaks down in the first iteration: one iteration, X = 0 and the oracle's history entry, 0."""
    name, L, kind = "long_rows", 4, "ic0"
    cap = 40
    B = pc.rhs(name, L).copy()
    B[:, 1] = 0.0
    Xo, it_o, ho = pc.oracle_solve(orc, name, L, kind, B, max_iters=cap)
    assert it_o == cap and np.all(np.isnan(Xo[:, 1]))  # the reference never converges the NaN column
    expect = int(np.flatnonzero(ho < TOL)[0]) + 1
    X1o, it1_o, h1o = pc.oracle_solve(orc, name, 1, kind, B[:, 1:2], max_iters=cap)
    assert it1_o == cap and np.all(np.isnan(X1o)) and np.all(h1o == 0.0)
    with Run(mspmv, name, L, kind) as s:
        out = s.solve(B)
        out2 = s.solve(B)
        alone = s.solve(B[:, 1:2])
    X, it, hist, st = out
    print(f"{name} L={L} ic0, column 1 zero: status {st}, iterations {it} (the oracle's other columns {expect})")
    assert st == BREAKDOWN and pc.iter_match(it, expect, ho, TOL)
    assert np.all(X[:, 1] == 0.0)
    pc.check_bars(f"{name} L={L} ic0, columns 0, 2, 3", (Xo, it, ho[:it]), out, cols=[0, 2, 3], status=BREAKDOWN)
    assert hist[-1] < TOL
    same_bits(out, out2)
    X1, it1, h1, st1 = alone
    print(f"alone: status {st1}, iterations {it1}, history {h1}")
    assert st1 == BREAKDOWN and it1 == 1 and np.all(X1 == 0.0)
    assert list(h1) == [0.0]


@pytest.mark.parametrize("solver", ["spai", "ic0"])
def test_zero_column(mspmv, orc, solver):
    """L = 4 with column 1 of B zero, on long_rows: what the oracle does with it, under each solver (above)."""
    (zero_column_spai if solver == "spai" else zero_column_ic0)(mspmv, orc)


def test_breakdown_history_entry_plain_cg(mspmv):
    """The alpha test that ends test_zero_column's lone IC(0)-PCG column is shared with the plain split CG
    (cg_alpha_finish): after an ordinary solve has filled the handle's history buffer, a right-hand side of zeros
    breaks every column down in the first iteration -- one iteration, X = 0, and the history entry the reference
    records for it, 0 (its NaN columns are skipped), not the earlier solve's first residual."""
    name, L = "long_rows", 4
    B = pc.rhs(name, L)
    with mspmv.GpuCsr(pc.matrix(name, L)) as g:
        X, it, hist, st = g.cg_multi(B, MAX_ITERS, TOL, hist_cap=MAX_ITERS)
        X0, it0, h0, st0 = g.cg_multi(np.zeros_like(B), MAX_ITERS, TOL, hist_cap=MAX_ITERS)
    assert st == 0 and hist[0] > 0.0 and hist[-1] < TOL
    assert st0 == BREAKDOWN and it0 == 1 and np.all(X0 == 0.0)
    assert list(h0) == [0.0]
