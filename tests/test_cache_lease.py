"""The per-device Infinity-Cache ledger (csrc/mspmv_cache.cpp) through its host-only entry points: the exchange
every handle makes (mspmv_cache_lease), the budget and the floor.  No GPU, no handle.

The rules under test: a request above the floor is granted while the live leases plus the request stay within the
budget, first come, first served, and a refused request holds nothing; a stream of at most the floor (32 MiB by
default) stays resident and books nothing; MSPMV_CACHE_RESIDENT books whatever the budget says and later requests
see it; MSPMV_CACHE_STREAM returns what was held; the same sequence always gives the same answers.

Each test works on a ledger of its own (a device ordinal nothing else uses) so that nothing a GPU test of the same
process booked on device 0 is in the way."""
import itertools
import os
import subprocess
import sys

import pytest

import mspmv

MIB = 1 << 20
_ordinals = itertools.count(900)


@pytest.fixture
def dev():
    """A fresh ledger at a known budget, its defaults put back afterwards."""
    d = next(_ordinals)
    budget, floor = mspmv.cache_budget(d, 200 * MIB), mspmv.cache_floor(d)
    yield d
    assert mspmv.cache_leased(d) == 0, "a test left a lease behind"
    mspmv.cache_budget(d, budget)
    mspmv.cache_floor(d, floor)


def test_defaults():
    d = next(_ordinals)
    assert mspmv.cache_floor(d) == 32 * MIB
    budget = mspmv.cache_budget(d)
    if "MSPMV_CACHE_MIB" not in os.environ:  # the built-in value: a multiple of 16 MiB within the cache
        assert budget > 32 * MIB and budget % (16 * MIB) == 0 and budget <= 256 * MIB
    assert mspmv.cache_leased(d) == 0


def test_budget_from_the_environment():
    """MSPMV_CACHE_MIB, read once per process: a fresh process starts every ledger there."""
    code = "import mspmv; print(mspmv.cache_budget(0), mspmv.cache_budget(3), mspmv.cache_floor(0))"
    env = dict(os.environ, MSPMV_CACHE_MIB="48", PYTHONPATH=os.path.dirname(os.path.dirname(mspmv.__file__)))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout
    assert out.split() == [str(48 * MIB), str(48 * MIB), str(32 * MIB)]


def test_grant_refuse_release_in_creation_order(dev):
    a, b, c = 90 * MIB, 95 * MIB, 60 * MIB
    assert mspmv.cache_lease(dev, 0, a) == (a, True)
    assert mspmv.cache_lease(dev, 0, b) == (b, True)      # 185 of 200
    assert mspmv.cache_lease(dev, 0, c) == (0, False)     # 245 > 200: refused, holds nothing
    assert mspmv.cache_leased(dev) == a + b
    assert mspmv.cache_lease(dev, 0, 15 * MIB) == (0, True)   # at most the floor: resident, nothing booked
    assert mspmv.cache_lease(dev, a, 0, mspmv.CACHE_STREAM) == (0, False)  # the first one is destroyed
    assert mspmv.cache_leased(dev) == b
    assert mspmv.cache_lease(dev, 0, c) == (c, True)      # 155 of 200: a later one fits again
    assert mspmv.cache_lease(dev, b, 0, mspmv.CACHE_STREAM) == (0, False)
    assert mspmv.cache_lease(dev, c, 0, mspmv.CACHE_STREAM) == (0, False)


def test_exact_fit_and_one_byte_over(dev):
    assert mspmv.cache_lease(dev, 0, 200 * MIB) == (200 * MIB, True)
    assert mspmv.cache_lease(dev, 200 * MIB, 200 * MIB + 1) == (0, False)  # its own lease does not count against it
    assert mspmv.cache_leased(dev) == 0


def test_lease_grows_or_is_lost(dev):
    assert mspmv.cache_lease(dev, 0, 80 * MIB) == (80 * MIB, True)
    assert mspmv.cache_lease(dev, 0, 100 * MIB) == (100 * MIB, True)
    assert mspmv.cache_lease(dev, 80 * MIB, 100 * MIB) == (100 * MIB, True)   # a later plan streams more: grows
    assert mspmv.cache_leased(dev) == 200 * MIB
    assert mspmv.cache_lease(dev, 100 * MIB, 101 * MIB) == (0, False)         # no room to grow: dropped to STREAM
    assert mspmv.cache_leased(dev) == 100 * MIB
    assert mspmv.cache_lease(dev, 100 * MIB, 0, mspmv.CACHE_STREAM) == (0, False)


def test_override_booking(dev):
    big = 300 * MIB
    assert mspmv.cache_lease(dev, 0, big, mspmv.CACHE_RESIDENT) == (big, True)     # over the budget, and booked
    assert mspmv.cache_leased(dev) == big
    assert mspmv.cache_lease(dev, 0, 40 * MIB) == (0, False)                       # the others see it
    assert mspmv.cache_lease(dev, big, big, mspmv.CACHE_STREAM) == (0, False)      # STREAM returns the lease
    assert mspmv.cache_leased(dev) == 0
    assert mspmv.cache_lease(dev, 0, 40 * MIB) == (40 * MIB, True)
    assert mspmv.cache_lease(dev, 40 * MIB, 40 * MIB, mspmv.CACHE_STREAM) == (0, False)
    assert mspmv.cache_lease(dev, 0, MIB, mspmv.CACHE_STREAM) == (0, False)        # STREAM holds below the floor too
    assert mspmv.cache_lease(dev, 0, MIB, mspmv.CACHE_RESIDENT) == (MIB, True)     # RESIDENT books below it
    assert mspmv.cache_lease(dev, MIB, MIB, mspmv.CACHE_AUTO) == (0, True)         # back to AUTO: the floor again
    assert mspmv.cache_leased(dev) == 0


def test_floor(dev):
    assert mspmv.cache_lease(dev, 0, 200 * MIB) == (200 * MIB, True)   # the budget is spent
    for n in range(3):                                                 # however many small ones follow
        assert mspmv.cache_lease(dev, 0, 32 * MIB) == (0, True)
    assert mspmv.cache_lease(dev, 0, 32 * MIB + 1) == (0, False)
    assert mspmv.cache_floor(dev, 0) == 32 * MIB                       # no floor: every stream asks
    assert mspmv.cache_lease(dev, 0, 1) == (0, False)
    assert mspmv.cache_lease(dev, 200 * MIB, 0, mspmv.CACHE_STREAM) == (0, False)
    assert mspmv.cache_lease(dev, 0, 1) == (1, True)
    assert mspmv.cache_lease(dev, 1, 0, mspmv.CACHE_STREAM) == (0, False)


def test_budget_set_query_restore(dev):
    assert mspmv.cache_budget(dev) == 200 * MIB          # query only
    assert mspmv.cache_budget(dev, -5) == 200 * MIB      # any negative value
    assert mspmv.cache_budget(dev, 50 * MIB) == 200 * MIB
    assert mspmv.cache_lease(dev, 0, 60 * MIB) == (0, False)
    assert mspmv.cache_lease(dev, 0, 50 * MIB) == (50 * MIB, True)
    assert mspmv.cache_budget(dev, 40 * MIB) == 50 * MIB  # a smaller budget leaves the decisions made alone
    assert mspmv.cache_leased(dev) == 50 * MIB
    assert mspmv.cache_lease(dev, 50 * MIB, 0, mspmv.CACHE_STREAM) == (0, False)
    assert mspmv.cache_budget(dev, 200 * MIB) == 40 * MIB
    other = next(_ordinals)                               # ledgers are per device
    assert mspmv.cache_budget(other) == mspmv.cache_budget(next(_ordinals))
    assert mspmv.cache_leased(other) == 0


def test_same_sequence_same_answers(dev):
    wants = [70, 33, 90, 32, 64, 10, 41]

    def run():
        held, answers = [], []
        for w in wants:
            g, r = mspmv.cache_lease(dev, 0, w * MIB)
            held.append(g)
            answers.append((g, r))
        for g in held:
            mspmv.cache_lease(dev, g, 0, mspmv.CACHE_STREAM)
        return answers

    first = run()
    assert first == run()
    assert [r for _, r in first] == [True, True, True, True, False, True, False]


def test_bad_arguments(dev):
    for args in ((-1, 0, 1, 0), (dev, -1, 1, 0), (dev, 0, -1, 0), (dev, 0, 1, 7), (dev, 1, 0, 0)):
        with pytest.raises(mspmv.MspmvError):
            mspmv.cache_lease(*args)
    with pytest.raises(mspmv.MspmvError):
        mspmv.cache_budget(-1)
