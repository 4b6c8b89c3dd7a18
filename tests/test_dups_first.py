"""The -r table without a GPU: the two references of gx_dups_first (tests/dups_ref.py: a dict, np.unique) against each other
on every key set of tests/test_hip_dups_first.py, and gx_dups_geometry -- the capacity gx_dups_first uses and the kernels' own
hash on the host, from which the GPU tests build their collision cluster."""
import ctypes as C

import numpy as np
import pytest

import dups_ref as R
from genrich_amd.lib import dups_geometry, load_library

ORDER = -10


def _sets():
    """(name, keys, multi) of every generator, at the GPU tests' sizes where a dict can walk them in a moment."""
    yield ("empty",) + R.distinct(0)
    yield ("one",) + R.distinct(1)
    for n in (511, 512, 513, 65536, 65537):
        yield (f"distinct{n}",) + R.distinct(n, n)
    for flag in (False, True):
        yield (f"one_key{int(flag)}",) + R.one_key(100_000, flag)
    yield ("heavy",) + R.heavy(200_000)
    yield ("near_equal",) + R.near_equal()
    yield ("cluster",) + R.cluster(dups_geometry)[:2]
    yield ("strided",) + R.strided(5_000, 4_096)                  # (the generator of the grid-stride case, at a dict's size)


@pytest.mark.parametrize("name,keys,multi", list(_sets()), ids=lambda v: v if isinstance(v, str) else "")
def test_the_two_references_agree(name, keys, multi):
    assert keys.dtype == np.uint32 and keys.shape == (len(multi), 4) and multi.dtype == np.uint8
    a, b = R.owner_dict(keys, multi), R.owner_np(keys, multi)
    assert a.dtype == b.dtype == np.uint32 and np.array_equal(a, b)
    first = a & ~np.uint32(R.CONTESTED)
    assert (first <= np.arange(len(a))).all()                       # the first holder never comes later
    assert np.array_equal(first[first], first)                     # ... and is its own first holder
    if len(a):
        assert (keys[first] == keys).all()                         # ... of the same key


def test_the_sets_hold_what_they_are_for():
    k, m = R.distinct(65537)
    assert len(np.unique(k, axis=0)) == len(k) and not m.any()
    k, m = R.heavy(200_000)
    assert len(np.unique(k, axis=0)) <= 50_000 and 4_000 < m.sum() < 8_000
    k, m = R.near_equal()
    u = np.unique(k, axis=0)
    assert len(k) == 3 * len(u) and m.any()
    for w in range(4):                                             # pairs of keys that differ in word w alone
        others = [c for c in range(4) if c != w]
        assert len(np.unique(u[:, others], axis=0)) < len(u)
    srt = np.unique(np.sort(u, axis=1), axis=0)                    # permutations of the same four words
    assert len(srt) < len(u)
    assert all((u == v).any() for v in R.EDGE_WORDS)
    k, m, is_cl, cap = R.cluster(dups_geometry)
    assert cap == 4096 and len(k) == 1500 and is_cl.sum() == 1200 and len(np.unique(k[is_cl], axis=0)) == 600
    assert m[is_cl].sum() == 12 and not m[~is_cl].any()
    own = R.owner_dict(k, m)
    flagged = (own & R.CONTESTED) != 0
    assert 12 <= flagged.sum() <= 24 and not flagged[~is_cl].any() and not flagged[is_cl].all()
    n, stride = 8192 * 256 + 300, 8192 * 256
    k, m = R.strided(n, stride)
    first = R.owner_np(k, m) & ~np.uint32(R.CONTESTED)
    dup = first != np.arange(n)
    assert n // 5 < dup.sum() < n // 3
    assert (first[stride:][dup[stride:]] < stride).sum() >= 140    # second-trip records whose first holder is in the first trip
    assert (first[stride:][dup[stride:]] >= stride).sum() >= 20 and (~dup[stride:]).sum() >= 60


@pytest.mark.parametrize("n", [0, 1, 511, 512, 513, 1000, 65535, 65536, 65537, 100_000, 1 << 20, (1 << 20) + 1])
def test_capacity_is_the_least_power_of_two_that_holds_2n(n):
    cap, home = dups_geometry(np.zeros((n, 4), dtype=np.uint32))
    want = 1024
    while want < 2 * n:
        want *= 2
    assert cap == want and cap >= 1024 and cap >= 2 * n and cap & (cap - 1) == 0 and (cap == 1024 or cap // 2 < 2 * n)
    assert len(home) == n


def test_capacity_alone_and_the_refusals():
    lib = load_library()
    cap = C.c_uint32(0)
    for n, want in ((512, 1024), (513, 2048), (65536, 1 << 17), (65537, 1 << 18), (1 << 30, 1 << 31)):
        assert lib.gx_dups_geometry(None, n, C.byref(cap), None) == 0 and cap.value == want      # (no keys: the capacity only)
    cap.value = 7
    assert lib.gx_dups_geometry(None, (1 << 30) + 1, C.byref(cap), None) == ORDER and cap.value == 7
    home = np.zeros(4, dtype=np.uint32)
    assert lib.gx_dups_geometry(None, 4, C.byref(cap), home.ctypes.data) == ORDER                # home without keys
    k = R.distinct(4)[0]
    assert lib.gx_dups_geometry(k.ctypes.data, 4, None, home.ctypes.data) == 0                   # home without capacity
    assert np.array_equal(home, dups_geometry(k)[1])


def test_home_slots():
    k, _ = R.heavy(200_000)
    cap, home = dups_geometry(k)
    assert cap == 1 << 19 and home.dtype == np.uint32 and (home < cap).all()
    _, inv = np.unique(k, axis=0, return_inverse=True)
    inv = inv.ravel()
    per_key = np.full(inv.max() + 1, -1, dtype=np.int64)
    per_key[inv] = home
    assert np.array_equal(per_key[inv], home)                       # equal keys, equal homes
    assert len(np.unique(home)) > 40_000                            # ... and the 50,000 keys are spread over the table
    # the home in a smaller table is the home in a larger one, masked (the hash's low bits)
    small_cap, small = dups_geometry(k[:1000])
    assert small_cap == 2048 and np.array_equal(small, home[:1000] & 2047)
    # every word, and every bit of the last one, reaches the hash
    base = np.tile(np.array([[1, 2, 3, 4]], dtype=np.uint32), (1 << 16, 1))
    for w in range(4):
        v = base.copy()
        v[:, w] = np.arange(1 << 16)
        assert len(np.unique(dups_geometry(v)[1])) > 1 << 12, w     # (1 if the word were ignored)
    k, _ = R.near_equal()
    cap, home = dups_geometry(k)
    assert (home < cap).all()
