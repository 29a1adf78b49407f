"""GPU: the Infinity-Cache policy of a handle (mspmv_set_cache_policy, mspmv_cache_info) and the leases the handles
of one device share (mspmv_cache_budget; the ledger alone: test_cache_lease.py).

The policy picks the instantiation of every product kernel -- default-policy or nontemporal loads of the matrix's
own arrays -- and nothing else: the same handle computes the same bytes under either.  These are also the runs
of the nontemporal instantiations at small sizes, by the policy the library ships (below the ledger's floor a
matrix is resident unless told otherwise).

Shapes, one per kernel family: FEM node blocks in the lean and the fallback form of k_spmv_blk (the latter on
test_gpu_blk_records.py's fallback matrix: the perturbed FEM shape's plan holds register tiles only), a band on
k_spmv_tile, power-law rows on the sliced-ELL kernel (forced: at this size the tiles are the default) and a
27-point stencil on the offset windows at L = 1 and L = 8.  One oracle product per shape and width, shared."""
import re

import numpy as np
import pytest

import mspmv
from gpu_common import EPS, abs_bound, check_parity
from test_gpu_blk_records import fallback_matrix

pytestmark = pytest.mark.gpu

STREAM, RESIDENT, AUTO = mspmv.CACHE_STREAM, mspmv.CACHE_RESIDENT, mspmv.CACHE_AUTO
FORM = {STREAM: "true", RESIDENT: "false"}

# name -> (matrix, environment at the handle's plan decision, the kernel's name with NT for its policy flag)
SHAPES = {
    "fem": (lambda: mspmv.CsrMatrix.synth_fem_blocked(6000, 318000, 6, 200, seed=1), {}, "k_spmv_blk<0,NT,6,false>"),
    # (at this size the run-balanced plan leaves no tile to the register fallback, so this one runs the lean form
    # too; the fallback form is the `fallback` shape's, whose plan mixes both kinds of tile)
    "fem_perturbed": (lambda: mspmv.CsrMatrix.synth_fem_perturbed(6000, 318000, 6, 200, 0.02, 0.01, seed=1), {},
                      "k_spmv_blk<0,NT,6,false>"),
    "fallback": (fallback_matrix, {}, "k_spmv_blk<0,NT,6,true>"),
    "cant_small": (lambda: mspmv.CsrMatrix.synth_banded(6000, 380000, 2000, seed=1), {}, r"k_spmv_tile<8,0,NT,256,\w+,\w+>"),
    "powerlaw": (lambda: mspmv.CsrMatrix.synth_powerlaw(20000, 20000, 600000, exponent=1.3, seed=3),
                 {"MSPMV_SPMV_SLAB": "4"}, r"k_spmv_sell<NT,\w+>"),
    "stencil": (lambda: mspmv.CsrMatrix.synth_stencil(1, 20 * 20 * 20, 20, 20, 20), {"MSPMV_DIA": None},
                "k_spmm_dia<1,NT>"),
}
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    return gpu_available


def case(orc, name, L=1):
    """(matrix, X, the oracle's product), computed once per shape and width and never written to."""
    if (name, L) not in _cache:
        a = _cache.get((name, "a")) or SHAPES[name][0]()
        _cache[(name, "a")] = a
        X = np.random.default_rng(11 + L).uniform(-1, 1, a.num_cols if L == 1 else (a.num_cols, L))
        ref = orc.spmv_gold(a, X) if L == 1 else orc.csr_spmm_t(a, X)
        for v in (X, ref):
            v.setflags(write=False)
        _cache[(name, L)] = (a, X, ref)
    return _cache[(name, L)]


def handle(monkeypatch, name, a):
    for k, v in SHAPES[name][1].items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    return mspmv.GpuCsr(a)


def name_matches(pattern, policy, got):
    rx = re.escape(pattern).replace(r"\\w\+", r"\w+").replace("NT", FORM[policy])
    return re.fullmatch(rx, got) is not None


@pytest.mark.parametrize("name", list(SHAPES))
def test_policy_leaves_the_bits_alone(orc, monkeypatch, name):
    a, x, ref = case(orc, name)
    widths = [(1, x, ref)]
    if name == "stencil":
        widths.append((8,) + case(orc, name, 8)[1:])
    with handle(monkeypatch, name, a) as g:
        assert g.cache_info()[0], "below the floor a matrix is resident by default"
        for L, X, want in widths:
            pattern = SHAPES[name][2].replace("<1,", f"<{L},") if name == "stencil" else SHAPES[name][2]
            got = {}
            for policy in (STREAM, RESIDENT, STREAM):
                g.set_cache_policy(policy)
                assert g.cache_info()[0] == (policy == RESIDENT)
                kname = g.kernel_name() if L == 1 else g.spmm_kernel_name(L)
                assert name_matches(pattern, policy, kname), (kname, pattern, FORM[policy])
                Y = g.spmv(X) if L == 1 else g.spmm(X)
                check_parity(a, Y, want, X, g.tile_plan(L), L)
                got.setdefault(policy, []).append(Y.tobytes())
            assert got[STREAM][0] == got[RESIDENT][0] == got[STREAM][1], f"{name} L={L}: the policy changed the result"
        g.set_cache_policy(AUTO)
        assert g.cache_info()[0] and mspmv.cache_leased(0) == 0


@pytest.mark.parametrize("name", list(SHAPES))
def test_reported_stream_bytes(orc, monkeypatch, name):
    a = case(orc, name)[0]
    nnz, m = a.num_nonzeros, a.num_rows
    with handle(monkeypatch, name, a) as g:
        resident, nbytes = g.cache_info()
        tiles = g.tile_plan(1)["num_tiles"]
        # a tile's dictionary holds at most one entry per nonzero (4 B) and a 16-bit index per nonzero
        dictionary = 6 * nnz if g.dict_tiles(1) > 0 and not g.kernel_name().startswith(("k_spmv_blk", "k_spmm_dia")) else 0
        print(f"{name}: {g.kernel_name()} streams {nbytes} B = {nbytes / nnz:.3f} B/nnz, {tiles} tiles, "
              f"upper bound {12 * nnz + 4 * (m + 1) + dictionary}")
        assert resident
        assert 8 * nnz <= nbytes <= 12 * nnz + 4 * (m + 1) + dictionary
        if name == "fem":
            # the run-balanced plan: every tile one round of eight record slots, every tile a node-block tile
            assert g.plan_block_rounds(1) == 0 and g.plan_block_tiles(1) == tiles
            slots = 8 * tiles
            assert nbytes == 8 * nnz + 64 * slots + 12 * tiles


def test_leases_in_creation_order(orc):
    a, x, ref = case(orc, "fem")
    with mspmv.GpuCsr(a) as g:
        nbytes = g.cache_info()[1]
    assert mspmv.cache_leased(0) == 0
    budget, floor = mspmv.cache_budget(0), mspmv.cache_floor(0)
    gs, bufs = [], []
    try:
        mspmv.cache_floor(0, 0)  # the shape is far below the 32 MiB floor: every stream asks
        mspmv.cache_budget(0, nbytes * 3 // 2)
        gs = [mspmv.GpuCsr(a) for _ in range(3)]
        assert [g.cache_info()[0] for g in gs] == [True, False, False]
        assert [g.kernel_name() for g in gs] == ["k_spmv_blk<0,false,6,false>"] + 2 * ["k_spmv_blk<0,true,6,false>"]
        assert nbytes <= mspmv.cache_leased(0) <= nbytes * 3 // 2
        xs = [np.random.default_rng(20 + i).uniform(-1, 1, a.num_cols) for i in range(3)]
        dxs = [mspmv.DeviceBuffer.from_array(v) for v in xs]
        dys = [mspmv.DeviceBuffer(8 * a.num_rows) for _ in range(3)]
        bufs = dxs + dys
        single = []
        for g, dx, dy in zip(gs, dxs, dys):
            g.spmm_dev(dx, dy, 1)
            single.append(dy.download(a.num_rows).tobytes())
            dy.fill_bytes(0)
        mspmv.spmm_batch_dev(gs, dxs, dys, 1)
        assert [dy.download(a.num_rows).tobytes() for dy in dys] == single
        check_parity(a, np.frombuffer(single[1]), orc.spmv_gold(a, xs[1]), xs[1], gs[1].tile_plan(1), 1)
        gs[0].close()
        assert mspmv.cache_leased(0) == 0
        gs.append(mspmv.GpuCsr(a))
        assert gs[3].cache_info()[0] and gs[3].kernel_name() == "k_spmv_blk<0,false,6,false>"
        assert [g.cache_info()[0] for g in gs[1:3]] == [False, False], "a decision made is not revisited"
        gs[1].set_cache_policy(RESIDENT)   # an override is booked over the budget ...
        assert gs[1].cache_info()[0] and mspmv.cache_leased(0) > nbytes * 3 // 2
        gs[1].set_cache_policy(AUTO)       # ... and AUTO asks again: refused, the lease returned
        assert not gs[1].cache_info()[0] and nbytes <= mspmv.cache_leased(0) <= nbytes * 3 // 2
    finally:
        for g in gs:
            g.close()
        for b in bufs:
            b.free()
        mspmv.cache_budget(0, budget)
        mspmv.cache_floor(0, floor)
    assert mspmv.cache_leased(0) == 0


@pytest.mark.parametrize("L", [1, 8])
def test_policy_drops_the_solver_graphs(orc, monkeypatch, L):
    """cg_dev, set_cache_policy, cg_dev: the second solve captures its iteration graph again, on the other
    instantiation of the window kernels, and arrives where the first did."""
    monkeypatch.setenv("MSPMV_CG_RESIDENT", "0")  # L = 1: the two-kernel pipelined form, which replays a graph
    a = case(orc, "stencil")[0]
    n = a.num_rows
    B = orc.glibc_rand(42, n * L).reshape(n, L)
    thr = float(np.sqrt(np.sum(B[:, 0] ** 2)) * 1e-8)
    with handle(monkeypatch, "stencil", a) as g:
        db, dx = mspmv.DeviceBuffer.from_array(B), mspmv.DeviceBuffer(8 * n * L)
        runs = []
        for policy in (RESIDENT, STREAM, RESIDENT):
            g.set_cache_policy(policy)
            dx.fill_bytes(0xff)
            it, _, st = g.cg_dev(db, dx, L, 2000, thr)
            g.sync()
            runs.append((it, st, dx.download((n, L)).tobytes(), g.cg_kernel_name()))
        db.free()
        dx.free()
    assert runs[0][1] == 0 and 10 < runs[0][0] < 2000
    assert runs[0][:3] == runs[1][:3] == runs[2][:3], [r[:2] for r in runs]
    assert runs[0][3] == runs[2][3] and "nontemporal" not in runs[0][3]
    assert runs[1][3] == runs[0][3] + ", nontemporal matrix loads"
    assert ("k_cg1_dia" in runs[0][3]) == (L == 1)


def test_sharded_handles_keep_out_of_the_ledger(orc):
    """A DistCsr's handles (on the communicator's stream; row-range views at N > 1) take no lease under AUTO,
    where a plain handle of the same matrix does, and multiply as before."""
    a, x, ref = case(orc, "fem")
    floor = mspmv.cache_floor(0, 0)  # every plain handle's stream asks
    d = dx = dy = None
    try:
        with mspmv.GpuCsr(a) as g:
            assert g.cache_info()[0] and mspmv.cache_leased(0) >= g.cache_info()[1] > 0
        assert mspmv.cache_leased(0) == 0
        rb = mspmv.dist_partition(a, 1)
        d = mspmv.DistCsr(mspmv.comm_unique_id(), 1, 0, 0, rb, mspmv.local_rows(a, rb, 0))
        assert mspmv.cache_leased(0) == 0
        dx, dy = mspmv.DeviceBuffer.from_array(x), mspmv.DeviceBuffer(8 * a.num_rows)
        d.spmm_dev(dx, dy, 1)
        y = dy.download(a.num_rows)
        bound, lens = abs_bound(a, x)
        assert np.all(np.abs(y - ref) <= 2.0 * (lens + 1) * EPS * bound[:, 0] + 1e-300)
        assert mspmv.cache_leased(0) == 0
    finally:
        if d is not None:
            d.close()
        for b in (dx, dy):
            if b is not None:
                b.free()
        mspmv.cache_floor(0, floor)
