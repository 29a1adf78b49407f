"""GPU: the batched product (mspmv_spmm_batch_dev / mspmv_sync_batch) and the batch timing entry on the same
path: product i on handle i's own stream, so independent products may overlap.

Four handles, one per launch path of a plain product: node blocks (the headline kernel), merge tiles,
offset windows, and a 0-row matrix (no launch); a fifth, with rows split between tiles, for the fault check.  Every check is bit for bit: the
batch runs the kernel, plan and order of sums of the handle's own spmm_dev.
"""
import os

import numpy as np
import pytest

import mspmv

pytestmark = pytest.mark.gpu

WIDTHS = (1, 8)
SENTINEL = 0x7F
INVALID = 1  # MSPMV_ERR_INVALID


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    return gpu_available


class Case:
    def __init__(self, name, a):
        self.name, self.a = name, a
        self.g = mspmv.GpuCsr(a, device=0)
        self.x, self.dx, self.ref = {}, {}, {}


@pytest.fixture(scope="module")
def cases():
    """The four handles with their plans settled under the library's default plan choice (MSPMV_DIA unset:
    the stencil on its offset windows), x panels on the device, and each handle's own spmm_dev result per
    width -- computed once, never modified."""
    mats = [("fem", mspmv.CsrMatrix.synth_fem_blocked(21792, 1152443, 6, 170, seed=3)),
            ("banded", mspmv.CsrMatrix.synth_banded(6000, 380000, 2000, seed=1)),
            ("stencil", mspmv.CsrMatrix.synth_stencil(1, 12 * 13 * 14, 12, 13, 14)),
            ("empty", mspmv.CsrMatrix(0, 0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0)))]
    saved = os.environ.pop("MSPMV_DIA", None)
    try:
        cs = [Case(n, a) for n, a in mats]
        rng = np.random.default_rng(11)
        for c in cs:
            for L in WIDTHS:
                c.x[L] = rng.uniform(-1, 1, (c.a.num_cols, L))
                c.dx[L] = mspmv.DeviceBuffer.from_array(c.x[L]) if c.a.num_cols else mspmv.DeviceBuffer(16)
                dy = ybuf(c, L)
                c.g.spmm_dev(c.dx[L], dy, L)  # settles the plan for L
                c.g.check_faults()
                c.ref[L] = dy.download((c.a.num_rows, L))
                dy.free()
    finally:
        if saved is not None:
            os.environ["MSPMV_DIA"] = saved
    by = {c.name: c for c in cs}
    assert by["fem"].g.kernel_name().startswith("k_spmv_blk"), by["fem"].g.kernel_name()
    assert by["stencil"].g.kernel_name().startswith("k_spmm_dia<1,"), by["stencil"].g.kernel_name()
    yield cs
    for c in cs:
        c.g.close()


@pytest.fixture(scope="module")
def long_rows():
    """A fifth handle whose single-RHS plan does split rows between tiles (the banded case's 63-nonzero rows
    all snap to tile boundaries): 2,000 rows of 12 columns, three of them 1,900 long."""
    rng = np.random.default_rng(5)
    m = 2000
    lens = np.full(m, 12, np.int64)
    lens[[3, 700, 1500]] = 1900
    ro = np.zeros(m + 1, np.int64)
    ro[1:] = np.cumsum(lens)
    ci = np.concatenate([np.sort(rng.choice(m, n, replace=False)) for n in lens]).astype(np.int32)
    c = Case("long", mspmv.CsrMatrix.from_arrays(m, ro.astype(np.int32), ci, rng.uniform(-1, 1, ci.size)))
    c.x[1] = rng.uniform(-1, 1, (m, 1))
    c.dx[1] = mspmv.DeviceBuffer.from_array(c.x[1])
    dy = ybuf(c, 1)
    c.g.spmm_dev(c.dx[1], dy, 1)
    c.g.check_faults()
    c.ref[1] = dy.download((m, 1))
    dy.free()
    assert c.g.tile_plan(1)["num_carries"] > 0
    yield c
    c.g.close()


def ybuf(c, L):
    """A y panel filled with the sentinel byte (a 0-row matrix gets a small one: nothing writes it)."""
    b = mspmv.DeviceBuffer(max(8 * c.a.num_rows * L, 16))
    b.fill_bytes(SENTINEL)
    return b


def untouched(b):
    return bool(np.all(b.download((b.nbytes,), np.uint8) == SENTINEL))


def same_bits(y, ref):
    return y.shape == ref.shape and y.tobytes() == ref.tobytes()


@pytest.mark.parametrize("overlap", [None, "0"])
@pytest.mark.parametrize("L", WIDTHS)
def test_batch_is_bit_identical_to_single_products(cases, monkeypatch, L, overlap):
    """spmm_batch_dev over the four handles: every y bit-identical to the handle's own spmm_dev on the same
    inputs, with MSPMV_BATCH_OVERLAP unset and = 0; the timing entry, which launches on the same path in
    either form of the switch, leaves the same y."""
    if overlap is None:
        monkeypatch.delenv("MSPMV_BATCH_OVERLAP", raising=False)
    else:
        monkeypatch.setenv("MSPMV_BATCH_OVERLAP", overlap)
    gs = [c.g for c in cases]
    dxs = [c.dx[L] for c in cases]
    dys = [ybuf(c, L) for c in cases]
    mspmv.spmm_batch_dev(gs, dxs, dys, L)
    for c, dy in zip(cases, dys):
        assert same_bits(dy.download((c.a.num_rows, L)), c.ref[L]), c.name
    assert untouched(dys[3])
    for dy in dys:
        dy.fill_bytes(SENTINEL)
    step_ms, kern_ms, kps = mspmv.time_spmm_batch(gs, dxs, dys, L, 3)
    assert kps == 3 and step_ms > 0 and kern_ms > 0
    for c, dy in zip(cases, dys):
        assert same_bits(dy.download((c.a.num_rows, L)), c.ref[L]), c.name
    for dy in dys:
        dy.free()


def test_one_handle_timing_batch(cases):
    """A batch of one handle (the hot-single-matrix form): the same y, one kernel per step."""
    c = cases[0]
    dy = ybuf(c, 1)
    step_ms, kern_ms, kps = mspmv.time_spmm_batch([c.g], [c.dx[1]], [dy], 1, 3)
    assert kps == 1 and step_ms > 0
    assert kern_ms == pytest.approx(step_ms)
    assert same_bits(dy.download((c.a.num_rows, 1)), c.ref[1])
    dy.free()


def test_batch_keeps_the_handle_stream_order(cases):
    """Nothing synchronised in between: spmm_dev(x0 -> y0), then a batch in which the same handle computes
    y1 = A y0 (beside the other handles' products), then spmm_dev(y1 -> y2), all enqueued before one
    sync_batch.  y2 equals the three products run with a sync after each, bit for bit (square matrix)."""
    fem, others = cases[0], cases[1:]
    assert fem.a.num_rows == fem.a.num_cols
    g, x0 = fem.g, fem.dx[1]
    want = [ybuf(fem, 1) for _ in range(3)]
    g.spmm_dev(x0, want[0], 1)
    g.spmm_dev(want[0], want[1], 1)
    g.spmm_dev(want[1], want[2], 1)
    y = [ybuf(fem, 1) for _ in range(3)]
    oy = [ybuf(c, 1) for c in others]
    g.spmm_dev(x0, y[0], 1, sync=False)
    mspmv.spmm_batch_dev([c.g for c in others] + [g], [c.dx[1] for c in others] + [y[0]], oy + [y[1]], 1, sync=False)
    g.spmm_dev(y[1], y[2], 1, sync=False)
    mspmv.sync_batch([c.g for c in cases])
    for k in range(3):
        assert same_bits(y[k].download((fem.a.num_rows,)), want[k].download((fem.a.num_rows,))), k
    for c, b in zip(others, oy):
        assert same_bits(b.download((c.a.num_rows, 1)), c.ref[1]), c.name
    for b in want + y + oy:
        b.free()


def test_a_handle_listed_twice_and_a_shared_x(cases):
    """A handle listed twice is legal (its two products run in stream order), and products may share an x
    when their y ranges are disjoint."""
    fem = cases[0]
    ya, yb = ybuf(fem, 1), ybuf(fem, 1)
    mspmv.spmm_batch_dev([fem.g, fem.g], [fem.dx[1], fem.dx[1]], [ya, yb], 1)
    for b in (ya, yb):
        assert same_bits(b.download((fem.a.num_rows, 1)), fem.ref[1])
        b.free()


class _View:
    """A device pointer inside another buffer."""

    def __init__(self, buf, offset_bytes):
        self.ptr = buf.ptr + offset_bytes


def _refused(gs, dxs, dys, L, names, ys):
    with pytest.raises(mspmv.MspmvError) as ei:
        mspmv.spmm_batch_dev(gs, dxs, dys, L, sync=False)
    assert ei.value.status == INVALID, ei.value
    for n in names:
        assert n in str(ei.value), ei.value
    mspmv.sync_batch(gs)
    for b in ys:
        assert untouched(b)


def test_argument_checks_launch_nothing(cases):
    """Each refused with MSPMV_ERR_INVALID before anything is enqueued (every y keeps its sentinel)."""
    fem, banded = cases[0], cases[1]
    m, n = fem.a.num_rows, fem.a.num_cols
    # two products sharing a y; and partially overlapping y ranges
    y0, y1 = ybuf(fem, 1), ybuf(banded, 1)
    _refused([fem.g, fem.g], [fem.dx[1], fem.dx[1]], [y0, y0], 1, ("0 and 1",), [y0])
    big = mspmv.DeviceBuffer(8 * (m + n) + 64)
    big.fill_bytes(SENTINEL)
    _refused([fem.g, fem.g], [fem.dx[1], fem.dx[1]], [big, _View(big, 8 * (m - 1))], 1, ("0 and 1",), [big])
    # y of product 1 overlapping the x of product 0 (the x's last element)
    _refused([fem.g, banded.g], [_View(big, 0), banded.dx[1]], [y0, _View(big, 8 * (n - 1))], 1,
             ("product 1", "product 0"), [big, y0])
    # y aliasing its own x
    _refused([banded.g, fem.g], [banded.dx[1], big], [y1, big], 1, ("product 1",), [big, y1])
    # an unsupported width (panels large enough for it)
    y3 = mspmv.DeviceBuffer(8 * m * 3)
    y3.fill_bytes(SENTINEL)
    x3 = mspmv.DeviceBuffer(8 * n * 3)
    _refused([fem.g], [x3], [y3], 3, ("L",), [y3])
    # a misaligned panel for L > 1
    y8 = mspmv.DeviceBuffer(8 * m * 8 + 16)
    y8.fill_bytes(SENTINEL)
    _refused([fem.g], [fem.dx[8]], [_View(y8, 8)], 8, ("aligned",), [y8])
    for b in (y0, y1, big, y3, x3, y8):
        b.free()


def test_handles_on_different_devices_are_refused(cases):
    if mspmv.device_count() < 2:
        pytest.skip("one device visible")
    fem = cases[0]
    with mspmv.GpuCsr(fem.a, device=1) as g1:
        x1 = mspmv.DeviceBuffer.from_array(fem.x[1], 1)
        y1 = mspmv.DeviceBuffer(8 * fem.a.num_rows, 1)
        y1.fill_bytes(SENTINEL)
        y0 = ybuf(fem, 1)
        _refused([fem.g, g1], [fem.dx[1], x1], [y0, y1], 1, ("device",), [y0, y1])
        for b in (x1, y1, y0):
            b.free()


def test_sync_batch_reports_a_ticket_fault(cases, long_rows):
    """A handle with rows split between tiles starts one batched product from split-row tickets of 2^31 - 1
    (the hook and a value of tests/test_gpu_faults.py): no tile draws its row's last ticket, every arrival
    draws past its group, and sync_batch returns MSPMV_ERR_FAULT instead of the fault lying unread.  The
    tickets are zeroed behind that product, so the next batch is clean and bit-identical again.  Once: the
    guard reports, nothing waits."""
    cs = list(cases) + [long_rows]
    gs = [c.g for c in cs]
    dxs = [c.dx[1] for c in cs]
    dys = [ybuf(c, 1) for c in cs]
    mspmv.spmm_batch_dev(gs, dxs, dys, 1)  # clean first: the fifth handle's split rows close in a batch too
    for c, dy in zip(cs, dys):
        assert same_bits(dy.download((c.a.num_rows, 1)), c.ref[1]), c.name
    long_rows.g.test_poison_tickets(0x7FFFFFFF, mspmv.POISON_FILL)
    mspmv.spmm_batch_dev(gs, dxs, dys, 1, sync=False)
    with pytest.raises(mspmv.MspmvError) as ei:
        mspmv.sync_batch(gs)
    assert ei.value.status == mspmv.FAULT and "product 4" in str(ei.value)
    for c, dy in zip(cs, dys):  # the other products of that batch are whole
        if c.name != "long":
            assert same_bits(dy.download((c.a.num_rows, 1)), c.ref[1]), c.name
    mspmv.spmm_batch_dev(gs, dxs, dys, 1)
    for c, dy in zip(cs, dys):
        assert same_bits(dy.download((c.a.num_rows, 1)), c.ref[1]), c.name
    for dy in dys:
        dy.free()
