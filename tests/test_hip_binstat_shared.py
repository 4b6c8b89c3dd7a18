"""What the correlation, the fingerprint and the rank correlation share on a context (gx_host_binstat.h): one staging buffer for
the hooks' rows, one table of row pointers, one check of the hooks' domain.  The statistics' own suites call one hook after the
same hook; here the hooks follow each other on one context, in sizes that make every call resize or reuse what the call before
it left, between real passes over the bins, and every refusal is held to its code and its text."""
import ctypes as C

import numpy as np
import pytest

import fingerprint_ref as F
import gram_ref as R
import rank_ref as K
from genrich_amd.lib import (FP_NC, GX_PATH_FINGERPRINT, GX_PATH_GRAM, GX_PATH_SPEARMAN, RankTable, U128_DTYPE,
                             coverage_spearman_group, gram_geometry)
from test_hip_coverage import C0, LENS, ORDER, T0, _ctx, _run   # noqa: F401 (T0, C0: fixtures)
from test_hip_spearman import _new, _tied

pytestmark = pytest.mark.gpu

_, LANES, _ = gram_geometry()            # the lanes of k_gram's workgroup, from the library as built
ODD = 2 * LANES + 1                      # an odd row: a padded pitch, and with 32 rows the largest pointer table


def _plain(a):
    return np.asarray(a).tolist()


def _gram(h, rows):
    nz, s, g = h.gram_u64(rows)
    n, enz, es, eg = R.gram(list(rows))
    got = (nz, [int(v) for v in s], [[int(v) for v in row] for row in g])
    assert got == (enz, es, eg)
    return got


def _fp(h, rows):
    count, total = h.fp_u64(rows)
    exp = F.hist(list(rows))
    assert count.shape == total.shape == (len(rows), FP_NC)
    got = (_plain(count), _plain(total))
    assert got == (exp[0], exp[1])
    return got


def _rank(h, rows, skip):
    got, nz = h.rank_u64(rows, 0, skip)
    N, enz, exp = K.rank_rows(list(rows), skip)
    assert nz == enz and np.array_equal(got, exp)
    return _plain(got), nz


def _distinct(h, row):
    v, c = h.distinct_u64(row)
    ev, ec = K.distinct(row)
    assert v.dtype == np.uint64 and _plain(v) == _plain(ev) and _plain(c) == _plain(ec)
    return _plain(v), _plain(c)


# ---- 1. the hooks after each other on one context ---------------------------------------------------------------------------

def test_the_hooks_interleaved_on_one_context():
    rng = np.random.default_rng(31)
    r32, r1 = _tied(rng, 32, ODD), _tied(rng, 1, 1, zeros=0)
    f5, d1 = _tied(rng, 5, 65), _tied(rng, 1, 64)[0]
    g32, k5, f32 = _tied(rng, 32, ODD), _tied(rng, 5, 63), _tied(rng, 32, 1)
    dead = (k5 == 0).all(axis=0)
    assert dead.any() and not dead.all()
    h = _new()
    runs = []
    for _ in range(2):
        out = [_rank(h, r32, False), _gram(h, r1), _fp(h, f5), _distinct(h, d1), _gram(h, g32), _rank(h, k5, True), _fp(h, f32)]
        assert (np.asarray(out[5][0])[:, dead] == 0).all() and out[5][1] == int(dead.sum())
        runs.append(out)
    assert runs[0] == runs[1]
    h.close()


# ---- 2. the hooks between real passes ---------------------------------------------------------------------------------------

def _passes(h):
    n, nz, s, g = h.coverage_gram()
    fn, count, total = h.coverage_fingerprint()
    N, rs, rg, nd = coverage_spearman_group([h])
    return ((n, nz, _plain(s), _plain(g)), (fn, _plain(count), _plain(total)), (N, _plain(rs), _plain(rg), nd))


def test_the_hooks_between_real_passes_leave_the_bins_and_the_results(T0, C0):
    h = _ctx(50)
    _run(h, [(T0, C0)])
    bins = [[h.coverage(i, c).sum120.copy() for c in range(len(LENS))] for i in range(2)]
    first = _passes(h)
    rows = _tied(np.random.default_rng(32), 5, 65)
    _gram(h, rows)
    _fp(h, rows)
    _rank(h, rows, False)
    assert _passes(h) == first
    for i in range(2):
        for c in range(len(LENS)):
            assert np.array_equal(h.coverage(i, c).sum120, bins[i][c]), (i, c)
    h.close()


# ---- 3. every refusal's code and text -----------------------------------------------------------------------------------------
# (the texts are the library's before the statistics shared anything: what the shared check is held to)

def test_refusal_codes_and_texts(T0, C0):
    g = _new()
    lib, ctx = g.lib, g.ctx
    bits = g.path_info()
    nz, nd = C.c_uint64(0), C.c_size_t(0)
    ok = np.ones((33, 4), dtype=np.uint64)
    bad = ok[:2].copy()
    bad[1, 3] = 1 << 51
    big = np.zeros((1, (1 << 24) + 1), dtype=np.uint64)
    out = np.zeros((33, max(4, FP_NC)), dtype=np.uint64)
    s1, g1 = np.zeros(33, dtype=U128_DTYPE), np.zeros((33, 33), dtype=U128_DTYPE)
    hooks = {
        "gx_gram_u64": lambda p, S, n, grid: lib.gx_gram_u64(ctx, p, S, n, grid, C.byref(nz), s1.ctypes.data, g1.ctypes.data),
        "gx_fp_u64": lambda p, S, n, grid: lib.gx_fp_u64(ctx, p, S, n, grid, out.ctypes.data, out.ctypes.data),
        "gx_rank_u64": lambda p, S, n, grid: lib.gx_rank_u64(ctx, p, S, n, grid, 0, out.ctypes.data, C.byref(nz)),
        "gx_distinct_u64": lambda p, S, n, grid: lib.gx_distinct_u64(ctx, p, n, grid, None, None, 0, C.byref(nd)),
    }

    def refused(rc, text):
        assert rc == ORDER and lib.gx_last_error(ctx).decode() == text, (rc, lib.gx_last_error(ctx), text)
        assert g.path_info() == bits, text

    for name, call in hooks.items():
        if name != "gx_distinct_u64":                            # (it takes one row)
            refused(call(ok.ctypes.data, 0, 4, 0), name + ": the number of rows is outside [1, 32]")
            refused(call(ok.ctypes.data, 33, 4, 0), name + ": the number of rows is outside [1, 32]")
        refused(call(big.ctypes.data, 1, (1 << 24) + 1, 0), name + ": more than 2^24 values a row")
        refused(call(ok.ctypes.data, 1, 4, 65536), name + ": a grid of more than 65535 workgroups")
        refused(call(None, 1, 4, 0), name + ": no rows")
        if name != "gx_fp_u64":                                  # (its domain is the row's total)
            refused(call(bad[1].ctypes.data, 1, 4, 0), name + ": a value of 2^51 or more")
    total = np.array([[1, 2, 3, 4], [1 << 63, 1 << 62, 1 << 62, 0]], dtype=np.uint64)   # the second row's total is exactly 2^64
    refused(hooks["gx_fp_u64"](total.ctypes.data, 2, 4, 0), "gx_fp_u64: a row's total of 2^64 or more")
    assert not out.any() and not s1["lo"].any() and not g1["lo"].any()
    g.close()

    h = _ctx(50)
    _run(h, [(T0, C0)])
    lib, ctx = h.lib, h.ctx
    bits = h.path_info()
    assert not bits & (GX_PATH_GRAM | GX_PATH_FINGERPRINT | GX_PATH_SPEARMAN)
    ns, n = C.c_int(0), C.c_uint64(0)
    luts = (RankTable * 2)()                                     # two empty tables: in order
    calls = {
        "gx_coverage_gram": lambda: lib.gx_coverage_gram(ctx, C.byref(ns), C.byref(n), C.byref(nz), s1.ctypes.data, g1.ctypes.data, 1),
        "gx_coverage_fingerprint": lambda: lib.gx_coverage_fingerprint(ctx, C.byref(ns), C.byref(n), out.ctypes.data, out.ctypes.data, 1),
        "gx_coverage_rank_gram": lambda: lib.gx_coverage_rank_gram(ctx, C.addressof(luts), 0, C.byref(ns), C.byref(n), C.byref(nz),
                                                                   s1.ctypes.data, g1.ctypes.data, 1),
    }
    for name, call in calls.items():
        assert call() == ORDER and lib.gx_last_error(ctx).decode() == name + ": cap is smaller than the number of samples", name
        assert h.path_info() == bits, name
    assert not out.any() and not s1["lo"].any() and not g1["lo"].any()
    h.close()
