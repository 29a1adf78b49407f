"""Node-block records: the codec of a chunk's pattern columns (blk_rec_encode / blk_rec_decode, the
one definition the plan-time fill, the column-pair SpMV and these host hooks share).  No GPU.

The contract: decode(encode(P), q) == P[min(q, wc - 1)] for every position q of a 64-wide slot,
unless P has more than 12 runs of consecutive columns, when the escape flag is set and no entry is
kept; an all-zero record decodes to offset 0 everywhere."""
import numpy as np
import pytest

import mspmv


def _record(ent, wc):
    """The 16 dwords: a descriptor of width wc (dword 0, bits 24-31), then the entries."""
    rec = np.zeros(16, np.uint32)
    rec[0] = wc << 24
    rec[4:] = ent
    return rec


def _roundtrip(P):
    P = np.asarray(P, np.uint16)
    ent, esc = mspmv.block_record_encode(P)
    assert not esc
    rec = _record(ent, P.size)
    got = [mspmv.block_record_decode(rec, q) for q in range(64)]
    want = [int(P[min(q, P.size - 1)]) for q in range(64)]
    assert got == want
    return ent


def _runs(P):
    return 1 + int(np.count_nonzero(np.diff(np.asarray(P, np.int64)) != 1))


def test_single_column():
    for c in (0, 7, 65535):
        ent = _roundtrip([c])
        assert ent[0] == c | (1 << 16) and not ent[1:].any()


def test_64_consecutive_columns():
    ent = _roundtrip(np.arange(100, 164))
    assert ent[0] == 100 | (64 << 16) and not ent[1:].any()
    _roundtrip(np.arange(65535 - 63, 65536))
    _roundtrip(np.arange(0, 64))


def test_entry_fields():
    ent = _roundtrip([5, 6, 7, 20, 21, 40])
    assert list(ent[:3]) == [5 | (3 << 16), 20 | (2 << 16) | (3 << 24), 40 | (1 << 16) | (5 << 24)]
    assert not ent[3:].any()


def test_exactly_12_runs():
    P = np.concatenate([np.arange(10 * k, 10 * k + 5) for k in range(12)])  # 12 runs of 5: wc = 60
    assert _runs(P) == 12
    ent = _roundtrip(P)
    assert ent.all()
    P = np.concatenate([np.arange(10 * k, 10 * k + 1 + k % 3) for k in range(12)])  # lengths 1, 2, 3
    assert _runs(P) == 12
    _roundtrip(P)


def test_13_runs_escape():
    P = np.concatenate([np.arange(10 * k, 10 * k + 4) for k in range(13)]).astype(np.uint16)
    assert _runs(P) == 13
    ent, esc = mspmv.block_record_encode(P)
    assert esc and not ent.any()
    ent, esc = mspmv.block_record_encode(np.arange(0, 128, 2, dtype=np.uint16))  # 64 runs of 1
    assert esc and not ent.any()


def test_runs_of_length_1():
    _roundtrip(np.arange(0, 24, 2))  # 12 runs of one column
    _roundtrip([3, 5, 9, 65535])
    _roundtrip([0, 2, 3, 4, 6])


def test_offsets_0_and_65535():
    _roundtrip([0, 65535])
    _roundtrip([0, 1, 2, 65533, 65534, 65535])
    _roundtrip([65534, 65535])  # one run ending at the top of the range


def test_all_zero_record():
    assert all(mspmv.block_record_decode(np.zeros(16, np.uint32), q) == 0 for q in range(64))
    ent, esc = mspmv.block_record_encode(np.zeros(0, np.uint16))
    assert not esc and not ent.any()


@pytest.mark.parametrize("seed", range(4))
def test_random_patterns(seed):
    rng = np.random.default_rng(seed)
    compact = escaped = 0
    for _ in range(100):
        wc = int(rng.integers(1, 65))
        nruns = int(rng.integers(1, min(wc, 16) + 1))
        # nruns runs of consecutive columns: cut wc positions into nruns lengths, separate them by gaps >= 1
        cuts = np.sort(rng.choice(np.arange(1, wc), nruns - 1, replace=False)) if nruns > 1 else np.zeros(0, int)
        lens = np.diff(np.concatenate([[0], cuts, [wc]]))
        span = 65536 if rng.random() < 0.5 else 4 * wc + 2 * nruns
        slack = span - wc - (nruns - 1)
        gaps = rng.multinomial(int(rng.integers(0, slack + 1)), np.ones(nruns) / nruns)
        P, c = [], 0
        for k in range(nruns):
            c += int(gaps[k]) + (k > 0)
            P += list(range(c, c + int(lens[k])))
            c += int(lens[k])
        P = np.asarray(P)
        assert P.size == wc and P[-1] <= 65535 and np.all(np.diff(P) > 0) and _runs(P) == nruns
        if nruns <= 12:
            _roundtrip(P)
            compact += 1
        else:
            ent, esc = mspmv.block_record_encode(P.astype(np.uint16))
            assert esc and not ent.any()
            escaped += 1
    assert compact > 50 and escaped > 0
