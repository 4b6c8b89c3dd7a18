"""k_dups_insert / k_dups_lookup (genrich_amd/csrc/gx_dups.h) through gx_dups_first, on their own: the raw owner words against
a dict and np.unique (tests/dups_ref.py), exactly, at the table's edges -- the two sides of a capacity step and a load of exactly
one half, one key claimed by 100,000 lanes at once, keys that differ in one word, a probe chain of 600 slots that wraps past the
last slot (built with the library's own hash, gx_dups_geometry), both trips of the grid-stride loop, a second call on a context."""
import ctypes as C

import numpy as np
import pytest

import backends as B
import dups_ref as R
from genrich_amd.lib import DUP_CONTESTED, dups_geometry

pytestmark = pytest.mark.gpu

ORDER = -10
GRID_LANES = 8192 * 256          # the most lanes of a launch (gx_dups_first): records beyond take a lane's second trip


@pytest.fixture(scope="module")
def ctx():
    import genrich_amd
    h = genrich_amd.Genrich(B.make_params(pq=0.01, min_auc=20.0))
    yield h
    h.close()


def _check(h, keys, multi, ref=R.owner_dict):
    got = h.dups_first(keys, multi)
    want = ref(keys, multi)
    assert got.dtype == np.uint32 and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert not len(bad), (len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    return got


def test_contested_bit_is_the_librarys():
    assert DUP_CONTESTED == R.CONTESTED == 1 << 31


def test_no_record_and_one(ctx):
    lib = ctx.lib
    owner = np.full(4, 0xDEADBEEF, dtype=np.uint32)
    k, m = R.distinct(4)
    assert lib.gx_dups_first(ctx.ctx, k.ctypes.data, m.ctypes.data, 0, owner.ctypes.data) == 0
    assert lib.gx_dups_first(ctx.ctx, None, None, 0, None) == 0
    assert (owner == 0xDEADBEEF).all()                               # n = 0: nothing written
    assert len(ctx.dups_first(np.zeros((0, 4), dtype=np.uint32), np.zeros(0, dtype=np.uint8))) == 0
    assert lib.gx_dups_first(ctx.ctx, k.ctypes.data, m.ctypes.data, 1, owner.ctypes.data) == 0
    assert owner.tolist() == [0, 0xDEADBEEF, 0xDEADBEEF, 0xDEADBEEF]  # n = 1: one word
    for flag in (0, 1, 255):
        assert ctx.dups_first(k[:1], [flag]).tolist() == [DUP_CONTESTED if flag else 0]


def test_refusals_come_before_anything_is_allocated(ctx):
    lib = ctx.lib
    owner = np.full(4, 0xDEADBEEF, dtype=np.uint32)
    k, m = R.distinct(4)
    for args in ((None, m.ctypes.data, 4, owner.ctypes.data), (k.ctypes.data, None, 4, owner.ctypes.data),
                 (k.ctypes.data, m.ctypes.data, 4, None),
                 (k.ctypes.data, m.ctypes.data, (1 << 30) + 1, owner.ctypes.data)):    # (four records' room: refused unread)
        assert lib.gx_dups_first(ctx.ctx, *args) == ORDER
    assert lib.gx_dups_first(None, k.ctypes.data, m.ctypes.data, 4, owner.ctypes.data) == ORDER
    assert (owner == 0xDEADBEEF).all()
    _check(ctx, k, m)                                                # the context is as good as before


@pytest.mark.parametrize("n", [511, 512, 513, 65536, 65537])
def test_all_distinct_on_both_sides_of_a_capacity_step(ctx, n):
    k, m = R.distinct(n, n)
    cap = dups_geometry(k)[0]
    assert cap == {511: 1024, 512: 1024, 513: 2048, 65536: 1 << 17, 65537: 1 << 18}[n]   # 512, 65536: exactly half full
    got = _check(ctx, k, m)
    assert np.array_equal(got, np.arange(n, dtype=np.uint32))


@pytest.mark.parametrize("flag_last", [False, True])
def test_one_key_a_hundred_thousand_times(ctx, flag_last):
    n = 100_000
    k, m = R.one_key(n, flag_last)
    got = ctx.dups_first(k, m)
    assert (got == (DUP_CONTESTED if flag_last else 0)).all(), np.unique(got)[:5]


def test_heavy_duplication(ctx):
    k, m = R.heavy(200_000)
    got = _check(ctx, k, m)
    first = got & ~np.uint32(DUP_CONTESTED)
    assert (first != np.arange(len(k))).sum() > 140_000 and 10_000 < ((got & DUP_CONTESTED) != 0).sum() < 100_000
    # (a slot's claimer is whichever lane wins: with 782 workgroups the first holder is often not in the claimer's)


def test_near_equal_keys(ctx):
    k, m = R.near_equal()
    _check(ctx, k, m)
    _check(ctx, k, np.zeros(len(k), dtype=np.uint8))
    _check(ctx, k, np.ones(len(k), dtype=np.uint8))


def test_a_chain_of_600_that_wraps_past_the_last_slot(ctx):
    k, m, is_cl, cap = R.cluster(dups_geometry)
    assert cap == 4096 and (dups_geometry(k)[1][is_cl] == cap - 1).all() and is_cl.sum() == 1200
    got = _check(ctx, k, m)
    flagged = (got & DUP_CONTESTED) != 0
    assert 12 <= flagged.sum() <= 24 and not flagged[~is_cl].any()   # no neighbour in the chain inherits the bit
    _check(ctx, k[::-1].copy(), m[::-1].copy())                      # the same chain claimed in another order


def test_both_trips_of_the_grid_stride_loop(ctx):
    n = GRID_LANES + 300
    k, m = R.strided(n, GRID_LANES)
    got = _check(ctx, k, m, R.owner_np)
    first = got[GRID_LANES:] & ~np.uint32(DUP_CONTESTED)
    assert (first < GRID_LANES).sum() >= 140 and (first == np.arange(GRID_LANES, n)).sum() >= 60


def test_a_second_call_knows_nothing_of_the_first(ctx):
    big, mb = R.heavy(200_000, 3)
    _check(ctx, big, np.ones(len(big), dtype=np.uint8), R.owner_np)  # every key flagged
    small, ms = big[:700].copy(), np.zeros(700, dtype=np.uint8)      # the same keys, fewer and unflagged, in a smaller table
    got = _check(ctx, small, ms)
    assert not (got & DUP_CONTESTED).any()
    k, m = R.distinct(513, 1)
    assert np.array_equal(_check(ctx, k, m), np.arange(513, dtype=np.uint32))
