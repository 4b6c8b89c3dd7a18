"""The samples' rank rows on the GPU (gx_distinct_u64 / gx_rank_u64 / gx_coverage_distinct / gx_coverage_spearman_group:
k_rank_distinct, k_rank_compact, k_rank_nzero, k_rank, then k_gram) and genrich-amd --spearman: exact equality with numpy and
Python integers (tests/rank_ref.py) at the edges of the kernels' geometry, of the LDS cache and of the table that grows, on real
runs in every form the coverage tests know, and over two contexts, where the ranking must be one over both."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import backends as B
import coverage_ref as CR
import golden_cases as G
import gram_ref as R
import rank_ref as K
from genrich_amd.lib import GX_PATH_GRAM, GX_PATH_SPEARMAN, coverage_spearman_group, rank_geometry, spearman_text
from test_hip_counts import _cli_inputs
from test_hip_coverage import BEDS, C0, LENS, ORDER, PARAMS, T0, _ctx, _events, _run   # noqa: F401 (T0, C0: fixtures)
from test_host_cli import _binary

pytestmark = pytest.mark.gpu

LANES, GRID, CACHE, CAP, LIMIT = rank_geometry()   # the kernels' own constants, from the library as built
FULL = GRID * LANES                                # one full pass of k_rank's default grid.  k_rank_distinct's default grid has a
                                                   # workgroup per 2 * LANES values: 2 * FULL values are one 16-byte load a lane on the
                                                   # full grid, 4 * FULL one whole step of its loop (two loads a lane)
SMALL_LOG = 10                                     # GX_RANK_CAP_LOG of the context whose table grows
SMALL_CAP = 1 << SMALL_LOG
SMALL_LIMIT = SMALL_CAP * LIMIT // CAP


def _new(knobs=()):
    import genrich_amd
    ctx = genrich_amd.Genrich(B.make_params(**PARAMS))
    ctx.set_chroms(LENS)
    for k, v in knobs:
        ctx.set_knob(k, v)
    return ctx


@pytest.fixture(scope="module")
def h():
    ctx = _new()
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def small():
    """A context whose table starts with 2^10 slots."""
    ctx = _new([("GX_RANK_CAP_LOG", SMALL_LOG)])
    yield ctx
    ctx.close()


def _same_table(got, exp, what=""):
    assert got[0].dtype == np.uint64 and got[0].tolist() == exp[0].tolist(), what
    assert got[1].tolist() == exp[1].tolist(), what


def _check_rows(h, rows, grid=0, what=""):
    """Every row's table and the rank rows, with and without the all-zero bins, against the definition."""
    rows = np.asarray(rows, dtype=np.uint64)
    for r in rows:
        _same_table(h.distinct_u64(r, grid), K.distinct(r), what)
    out = []
    for skip in (False, True):
        got, nz = h.rank_u64(rows, grid, skip)
        N, enz, exp = K.rank_rows(list(rows), skip)
        assert nz == enz, (what, skip, nz, enz)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, (what, skip, bad[:4], got[tuple(bad[0])], exp[tuple(bad[0])])
        out.append(got)
    assert rows.shape[1] == 0 or h.path_info() & GX_PATH_SPEARMAN     # (no bins: nothing is launched)
    return out


def _tied(rng, S, n, zeros=0.6, values=300):
    """Rows of a few hundred distinct values (up to the domain's end) with many ties; `zeros` of every row is 0, half of that
    in all rows at once."""
    pool = np.concatenate([rng.integers(1, 1 << 51, values // 2), rng.integers(1, 2000, values - values // 2)]).astype(np.uint64)
    rows = pool[rng.integers(0, len(pool), (S, n))]
    rows[:, rng.random(n) < zeros / 2] = 0
    rows[rng.random((S, n)) < zeros / 2] = 0
    return rows


# ---- 1. the edges of the geometry -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, LANES - 1, LANES, LANES + 1, 2 * LANES - 1, 2 * LANES, 2 * LANES + 1])
def test_small_sizes(h, n):
    rng = np.random.default_rng(100 + n)
    for S in (1, 2, 5):
        rows = _tied(rng, S, n)
        if n:
            rows[rng.integers(0, S), rng.integers(0, n)] = (1 << 51) - 1
        _check_rows(h, rows, what=(n, S))


@pytest.mark.parametrize("n", [FULL - 1, FULL, FULL + 1, 2 * FULL - 1, 2 * FULL, 2 * FULL + 1, 4 * FULL - 1, 4 * FULL, 4 * FULL + 1])
def test_one_full_pass_of_the_default_grid(h, n):
    rng = np.random.default_rng(n)
    rows = _tied(rng, 2, n)
    rows[:, -1] = (3, 1 << 50)                                   # the last bin counts
    _check_rows(h, rows, what=n)


# ---- 2. ties, the cache and the table -------------------------------------------------------------------------------------

def test_all_values_equal(h):
    n = 100_003
    for v in (7, (1 << 51) - 1, 0):
        rows = np.full((2, n), v, dtype=np.uint64)
        a, b = _check_rows(h, rows, what=v)
        assert (a == n + 1).all()                                # one tie group of n: twice the mean rank (n + 1) / 2
        assert (b == (0 if v == 0 else n + 1)).all()


def test_all_values_distinct_fill_the_table_to_its_load_limit(h):
    assert LIMIT == 1 << 16
    rng = np.random.default_rng(21)
    row = rng.permutation(np.arange(1, LIMIT + 1, dtype=np.uint64) * 977)
    _check_rows(h, [row])
    h.distinct_u64(row)
    assert h.rank_last() == (CAP, 0)                             # D = n = the load limit: no growth
    more = np.concatenate([row, [5]]).astype(np.uint64)
    _same_table(h.distinct_u64(more), K.distinct(more))
    assert h.rank_last() == (4 * CAP, 1)                         # one more: the table grew once


def test_the_growth_path_gives_the_default_capacitys_result(h, small):
    rng = np.random.default_rng(22)
    for d, grown in ((SMALL_LIMIT, 0), (SMALL_LIMIT + 1, 1), (5 * SMALL_LIMIT, 2)):
        vals = rng.choice(np.arange(1, 1 << 20), d, replace=False).astype(np.uint64)
        row = np.concatenate([vals, vals[rng.integers(0, d, 3000)], np.zeros(500, dtype=np.uint64)])
        rng.shuffle(row)
        assert len(np.unique(row)) == d + 1                      # (0 never enters the table)
        got = small.distinct_u64(row)
        cap, g = small.rank_last()
        assert g == grown and cap == SMALL_CAP << (2 * grown), (d, cap, g)
        _same_table(got, K.distinct(row), d)
        _same_table(h.distinct_u64(row), got, d)
        assert h.rank_last() == (CAP, 0)
        two = np.asarray([row, np.roll(row, 7)])
        for skip in (False, True):
            a, b = small.rank_u64(two, 0, skip), h.rank_u64(two, 0, skip)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1]
            assert np.array_equal(a[0], K.rank_rows(list(two), skip)[2])


def test_values_that_differ_in_one_half_only_and_multiples_of_the_capacity(h, small):
    rng = np.random.default_rng(23)
    n = 20_000
    high = ((rng.integers(0, 1 << 19, n) << 32) | 5).astype(np.uint64)             # equal low words
    low = ((7 << 40) | rng.integers(0, 1 << 12, n)).astype(np.uint64)              # equal high words
    mult = (rng.integers(1, 1000, n) * CAP).astype(np.uint64)                      # one slot under a masked identity hash
    mult_small = (rng.integers(1, 400, n) * SMALL_CAP).astype(np.uint64)
    top = ((1 << 51) - 1 - rng.integers(0, 50, n)).astype(np.uint64)               # up to the domain's end
    rows = np.asarray([high, low, mult, mult_small, top])
    _check_rows(h, rows)
    _check_rows(small, rows)


def test_more_distinct_values_than_the_cache_holds_in_one_workgroup(h):
    rng = np.random.default_rng(24)
    d = 3 * CACHE
    vals = np.unique(rng.integers(1, 1 << 30, 2 * d))[:d].astype(np.uint64)
    assert len(vals) == d
    row = np.concatenate([vals, vals[rng.integers(0, d, 4 * d)]])
    rng.shuffle(row)
    _check_rows(h, [row, np.roll(row, 1)], grid=1)


def test_mostly_zeros_and_one_value_among_zeros_in_a_wavefront(h):
    rng = np.random.default_rng(25)
    rows = _tied(rng, 3, 50_001)
    rows[rng.random(rows.shape) < 0.9] = 0
    assert 0.9 < (rows == 0).mean() < 0.99
    _check_rows(h, rows)
    n = 64 * 8
    one = np.zeros(n, dtype=np.uint64)
    one[70] = (1 << 50) + 3                                      # lane 6 of the second wavefront
    zero = np.zeros(n, dtype=np.uint64)
    a, b = _check_rows(h, [one, zero])
    assert a[0, 70] == 2 * n and a[0, 0] == n and (a[1] == n + 1).all()
    assert b[0, 70] == 2 and b[1, 70] == 2 and b.sum() == 4      # one bin is ranked
    _same_table(h.distinct_u64(one), (np.array([0, (1 << 50) + 3], dtype=np.uint64), np.array([n - 1, 1])))


# ---- 3. geometry and repeatability ------------------------------------------------------------------------------------------

def test_the_grid_does_not_matter_and_a_second_run_gives_the_same(h):
    rng = np.random.default_rng(26)
    rows = _tied(rng, 4, 100_003, values=5000)
    first = None
    for grid in (1, 7, 0, 0):
        tabs = [h.distinct_u64(r, grid) for r in rows]
        ranks = [h.rank_u64(rows, grid, skip) for skip in (False, True)]
        key = ([(v.tobytes(), c.tobytes()) for v, c in tabs], [(a.tobytes(), nz) for a, nz in ranks])
        first = first or key
        assert key == first, grid
    _check_rows(h, rows)


@pytest.mark.parametrize("lookup", [1, 2])
def test_both_lookups_of_k_rank(h, lookup):
    """k_rank by binary search in the sorted table (GX_RANK_LOOKUP=1) and by probing the hashed one (2): whichever the default
    is, both give the definition's ranks."""
    ctx = _new([("GX_RANK_LOOKUP", lookup)])
    rng = np.random.default_rng(40)
    try:
        for n in (0, 1, 65, 4099):
            _check_rows(ctx, _tied(rng, 3, n), what=(lookup, n))
        _check_rows(ctx, _tied(rng, 32, 1027), what=lookup)
        _check_rows(ctx, np.array([[0, 5, 5, 0, 9, 0], [0, 0, 0, 0, 0, 0], [7, 7, 7, 7, 7, 7]], dtype=np.uint64))   # tables of 1 and 2 entries
        # D = n: a table of 2^16 entries (the probed one exactly half full), values up to the domain's end and multiples of a capacity
        row = rng.permutation(np.arange(1, LIMIT + 1, dtype=np.uint64) * 977)
        row[:3] = ((1 << 51) - 1, CAP, 2 * CAP)
        row[3] = 0
        a = _check_rows(ctx, [row, np.roll(row, 5)], what=lookup)
        b = [h.rank_u64(np.asarray([row, np.roll(row, 5)]), 0, skip)[0] for skip in (False, True)]
        assert all(np.array_equal(x, y) for x, y in zip(a, b))   # ... and the default's
    finally:
        ctx.close()


# ---- 4. the bins that are 0 in every row ------------------------------------------------------------------------------------

def test_skip_zeros_by_hand(h):
    rows = np.array([[0, 5, 5, 0, 9, 0], [0, 1, 0, 0, 2, 3]], dtype=np.uint64)
    got, nz = h.rank_u64(rows, 0, False)
    assert nz == 2 and got.tolist() == [[4, 9, 9, 4, 12, 4], [4, 8, 4, 4, 10, 12]]
    got, nz = h.rank_u64(rows, 0, True)
    # bins 0 and 3 are 0 in both rows: 0 everywhere; bin 5 is kept, and the first row's 0 there is a tie group of one now
    assert nz == 2 and got.tolist() == [[0, 5, 5, 0, 8, 2], [0, 4, 2, 0, 6, 8]]


def test_32_rows(h):
    rng = np.random.default_rng(27)
    rows = _tied(rng, 32, 4099)
    a, b = _check_rows(h, rows)
    dead = (rows == 0).all(axis=0)
    assert dead.any() and (b[:, dead] == 0).all() and (b[:, ~dead] > 0).all() and (a > 0).all()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(T0):
    g = _new()
    lib, ctx = g.lib, g.ctx
    nz, nd = C.c_uint64(0), C.c_size_t(0)
    ok = np.ones((33, 4), dtype=np.uint64)
    bad = ok[:2].copy()
    bad[1, 3] = 1 << 51
    big = np.zeros((1, (1 << 24) + 1), dtype=np.uint64)
    out = np.zeros((33, 4), dtype=np.uint64)
    assert lib.gx_rank_u64(ctx, bad.ctypes.data, 2, 4, 0, 0, out.ctypes.data, C.byref(nz)) == ORDER          # a value of 2^51
    assert lib.gx_distinct_u64(ctx, bad[1].ctypes.data, 4, 0, None, None, 0, C.byref(nd)) == ORDER
    assert lib.gx_rank_u64(ctx, big.ctypes.data, 1, (1 << 24) + 1, 0, 0, None, C.byref(nz)) == ORDER         # n = 2^24 + 1
    assert lib.gx_distinct_u64(ctx, big.ctypes.data, (1 << 24) + 1, 0, None, None, 0, C.byref(nd)) == ORDER
    assert lib.gx_rank_u64(ctx, ok.ctypes.data, 0, 4, 0, 0, out.ctypes.data, C.byref(nz)) == ORDER           # no row
    assert lib.gx_rank_u64(ctx, ok.ctypes.data, 33, 4, 0, 0, out.ctypes.data, C.byref(nz)) == ORDER          # 33 rows
    assert lib.gx_rank_u64(ctx, ok.ctypes.data, 2, 4, 65536, 0, out.ctypes.data, C.byref(nz)) == ORDER       # a grid beyond the limit
    assert lib.gx_distinct_u64(ctx, ok.ctypes.data, 4, 65536, None, None, 0, C.byref(nd)) == ORDER
    # through the context: coverage off, before any sample, a sample open
    assert lib.gx_coverage_distinct(ctx, 0, None, None, 0, C.byref(nd)) == ORDER
    arr = (C.c_void_p * 1)(ctx)
    s1, g1 = np.zeros(1, dtype=[("lo", "<u8"), ("hi", "<u8")]), np.zeros(1, dtype=[("lo", "<u8"), ("hi", "<u8")])
    group = lambda: lib.gx_coverage_spearman_group(arr, 1, 1, 0, C.byref(nz), s1.ctypes.data, g1.ctypes.data, None)
    assert group() == ORDER                                      # coverage off
    g.sample_begin(0, None)
    g.push_events(T0)
    g.sample_end()
    assert group() == ORDER                                      # ... still off, with a closed sample
    g.reset()
    g.set_coverage_bins(50)
    assert group() == ORDER                                      # on, no sample yet
    g.sample_begin(0, None)
    assert group() == ORDER and lib.gx_coverage_distinct(ctx, 0, None, None, 0, C.byref(nd)) == ORDER   # a sample is open
    g.push_events(T0)
    g.sample_end()
    assert lib.gx_coverage_distinct(ctx, 1, None, None, 0, C.byref(nd)) == ORDER                        # no such sample
    assert not g.path_info() & GX_PATH_SPEARMAN and g.rank_last() == (0, 0)                              # nothing ran
    assert group() == 0 and g.path_info() & GX_PATH_SPEARMAN and g.rank_last()[0] == CAP
    g.reset()
    assert not g.path_info() & GX_PATH_SPEARMAN
    bad[1, 3] = (1 << 51) - 1
    assert lib.gx_rank_u64(ctx, bad.ctypes.data, 2, 4, 0, 0, out.ctypes.data, C.byref(nz)) == 0 and nz.value == 0
    assert g.path_info() & GX_PATH_SPEARMAN
    g.close()


# ---- 6. real runs through the context -----------------------------------------------------------------------------------------

def _dev_rows(h):
    return [np.concatenate([h.coverage(i, c).sum120 for c in range(len(LENS))]).astype(np.uint64) for i in range(h.coverage_samples())]


def _plain(res):
    N, s, g, nd = res
    return N, [int(v) for v in s], [[int(v) for v in row] for row in g], nd


def _check_run(h):
    """gx_coverage_distinct and the Spearman sums of one context against the definition over the bins gx_get_coverage returns."""
    rows = _dev_rows(h)
    for i, r in enumerate(rows):
        _same_table(h.coverage_distinct(i), K.distinct(r), i)
    out = []
    for skip in (False, True):
        N, s, g, nd = _plain(coverage_spearman_group([h], skip))
        eN, enz, es, eg = K.spearman(rows, skip)
        assert (N, s, g) == (eN, es, eg), skip
        assert nd == [len(v) for v, _ in K.tables(rows, skip)]
        assert N == len(rows[0]) - (enz if skip else 0)
        out.append((N, s, g))
    assert h.path_info() & GX_PATH_SPEARMAN and h.path_info() & GX_PATH_GRAM
    return rows, out


@pytest.mark.parametrize("W", [1, 50, 4096, 1 << 20])
def test_a_treatment_and_a_control(W, T0, C0):
    h = _ctx(W)
    _run(h, [(T0, C0)])
    rows, out = _check_run(h)
    assert len(rows) == 2 and len(rows[0]) == sum(CR.n_bins(x, W) for x in LENS)
    assert (out[0][0] > out[1][0]) == (W <= 4096)                # bins that are 0 in both, up to 4096 bases
    h.close()


def test_three_replicates_with_controls(T0, C0):
    T1, T2, C1 = _events(6), _events(7, n=30_000), _events(9, n=10_000)
    h = _ctx(50)
    _run(h, [(T0, C0), (T1, C1), (T2, C0)])
    rows, _ = _check_run(h)
    assert len(rows) == 6                                        # more than one tile of the pair matrix
    h.close()


def test_excluded_regions_a_skipped_chromosome_and_a_save_mask(T0, C0):
    h = _ctx(50, beds=BEDS)
    _run(h, [(T0, C0)])
    _check_run(h)
    h.close()
    h = _ctx(100, skip=[0, 0, 1, 0, 0])
    _run(h, [(T0, None)])
    rows, _ = _check_run(h)
    assert len(rows[0]) == sum(CR.n_bins(x, 100) for c, x in enumerate(LENS) if c != 2)
    h.close()
    h = _ctx(64)
    _run(h, [(T0, None), (T0, None)], saves=[[1, 1, 1, 1, 0], None])
    rows, _ = _check_run(h)
    assert (rows[0] != rows[1]).any() and (rows[0][-CR.n_bins(LENS[4], 64):] == 0).all()
    h.close()


def test_fractional_weights():
    ev = _events(4, counts=(2, 3, 4, 5, 6, 8, 10))
    h = _ctx(50, frac=True)
    _run(h, [(ev, None)])
    rows, _ = _check_run(h)
    assert (rows[0] % 120 != 0).any()
    h.close()


def test_tables_a_caller_gives_are_checked_before_anything_runs(T0):
    """gx_coverage_rank_gram with its own tables: out of order, a rank of 0 or of 2^42, and the value 2^64 - 1 (the probed
    table's free slot) are refused and k_rank is not launched; the definition's tables give the definition's sums."""
    h = _ctx(4096)
    _run(h, [(T0, None)])
    rows = _dev_rows(h)
    (v, r), = [(np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)) for a, b in K.tables(rows)]
    assert len(v) > 2
    top = np.uint64(0xFFFFFFFFFFFFFFFF)
    zero_rank, big_rank = r.copy(), r.copy()
    zero_rank[1], big_rank[1] = 0, 1 << 42
    for bad in ((v[::-1].copy(), r), (np.append(v, top), np.append(r, r[-1])), (np.append(v[:-1], top), r), (v, zero_rank), (v, big_rank)):
        with pytest.raises(RuntimeError, match="gx_coverage_rank_gram"):
            h.coverage_rank_gram([bad])
    assert not h.path_info() & GX_PATH_SPEARMAN
    n, nz, s, g = h.coverage_rank_gram([(v, r)])
    eN, enz, es, eg = K.spearman(rows, False)
    assert (n, nz, [int(x) for x in s], [[int(x) for x in row] for row in g]) == (eN, enz, es, eg)
    assert h.path_info() & GX_PATH_SPEARMAN
    h.close()


# ---- 7. two contexts: one ranking over both -------------------------------------------------------------------------------------

def test_two_contexts_with_complementary_chromosomes_give_the_one_context_sums(T0, C0):
    owned = [1, 0, 1, 0, 0]
    other = [1 - x for x in owned]
    a, b, whole = _ctx(50, owned=owned), _ctx(50, owned=other), _ctx(50)
    for h in (a, b, whole):
        _run(h, [(T0, C0)])
    ra, rb, rw = _dev_rows(a), _dev_rows(b), _dev_rows(whole)
    assert len(ra[0]) + len(rb[0]) == len(rw[0]) and len(ra[0]) > 100 and len(rb[0]) > 100
    for skip in (False, True):
        one = _plain(coverage_spearman_group([whole], skip))
        two = _plain(coverage_spearman_group([a, b], skip))
        assert two == one, skip
        assert _plain(coverage_spearman_group([b, a], skip)) == one
        exp = K.spearman(rw, skip)
        assert one[:3] == (exp[0], exp[2], exp[3])
        # ranking each half by itself gives other sums: the halves' values are distributed differently
        ha, hb = K.spearman(ra, skip), K.spearman(rb, skip)
        alone = ([x + y for x, y in zip(ha[2], hb[2])], [[x + y for x, y in zip(p, q)] for p, q in zip(ha[3], hb[3])])
        assert ha[0] + hb[0] == exp[0] and alone[0] != exp[2] and alone[1] != exp[3]
    names = ["t0", "c0"]
    assert spearman_text([a, b], names).decode() == K.spearman_text(names, rw) == spearman_text([whole], names).decode()
    for h in (a, b, whole):
        h.close()


# ---- 8. state ---------------------------------------------------------------------------------------------------------------------

def test_the_pass_changes_nothing_else(T0, C0):
    plain, asked = _ctx(50), _ctx(50)
    _run(plain, [(T0, C0)])
    asked.sample_begin(0, None)
    asked.push_events(T0)
    asked.sample_end()
    coverage_spearman_group([asked], True)                       # between the samples ...
    asked.sample_begin(1, None)
    asked.push_events(C0)
    asked.sample_end()
    asked.pvalues()
    asked.find_peaks()
    gram0, fp0 = asked.coverage_gram(), asked.coverage_fingerprint()
    one = _plain(coverage_spearman_group([asked], False))        # ... and after the peaks, twice
    assert _plain(coverage_spearman_group([asked], False)) == one
    gram1, fp1 = asked.coverage_gram(), asked.coverage_fingerprint()
    assert (gram0[0], gram0[1], gram0[2].tolist(), gram0[3].tolist()) == (gram1[0], gram1[1], gram1[2].tolist(), gram1[3].tolist())
    assert fp0[0] == fp1[0] and np.array_equal(fp0[1], fp1[1]) and np.array_equal(fp0[2], fp1[2])
    ref = plain.coverage_gram()
    assert (ref[0], ref[1], ref[2].tolist(), ref[3].tolist()) == (gram1[0], gram1[1], gram1[2].tolist(), gram1[3].tolist())
    assert plain.get_peaks().tobytes() == asked.get_peaks().tobytes()
    for c in range(len(LENS)):
        e0, c0 = plain.get_intervals(-1, c)
        e1, c1 = asked.get_intervals(-1, c)
        assert np.array_equal(e0, e1)
        for k in ("expt", "ctrl", "p"):
            assert np.array_equal(c0[k].view(np.uint32), c1[k].view(np.uint32)), k
        for i in range(2):
            assert np.array_equal(plain.coverage(i, c).sum120, asked.coverage(i, c).sum120)
    plain.coverage_fingerprint()
    assert asked.path_info() == plain.path_info() | GX_PATH_SPEARMAN
    plain.close()
    asked.close()


# ---- 9. the command line ------------------------------------------------------------------------------------------------------------

def _cli_rows(name, W):
    """(the samples' rows, their labels) from the case's events alone."""
    meta, case, _, names = G.load_case(name)
    rows, labels = [], []
    for r, rep in enumerate(case["replicates"]):
        for ctrl, ev in ((False, rep["treat"]), (True, rep["ctrl"])):
            if ev is None:
                continue
            cov = CR.coverage(ev, case["lens"], W, skip=case["skip"], beds=case["beds"], save=rep["save"])
            rows.append(np.concatenate([cov[c] for c in sorted(cov)]))
            labels.append(f"{'c' if ctrl else 't'}{r}")
    return rows, labels


@pytest.mark.parametrize("name", ["basic", "ctrl_q"])
def test_cli_spearman(name):
    meta, args, tmp, _ = _cli_inputs(name)
    out = os.path.join(tmp, "rho_out")
    res = subprocess.run([_binary(), "-v", "-o", out + ".narrowPeak", "--spearman", out + ".tsv"] + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    rows, labels = _cli_rows(name, 50)
    assert K.min_boundary_distance(rows) > 1e-9                  # no printed value sits on a rounding boundary
    assert open(out + ".tsv").read() == K.spearman_text(labels, rows)
    most = max(len(v) for v, _ in K.tables(rows))
    line = [l for l in res.stderr.splitlines() if l.startswith("  Spearman: ")]
    assert len(line) == 1 and line[0].startswith(f"  Spearman: {len(rows[0])} bins ranked, at most {most} distinct values a sample; "), res.stderr
    assert open(out + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")
    assert not os.path.exists(out + ".t0.bedgraph")              # the bins are on, no track is written


def test_cli_two_contexts_skip_zeros_X_gzip_and_next_to_correlation():
    name = "ctrl_q"
    meta, args, tmp, _ = _cli_inputs(name)
    run = lambda extra: subprocess.run([_binary()] + extra + args, capture_output=True, text=True)
    rows7, labels = _cli_rows(name, 7)
    rows50, _ = _cli_rows(name, 50)
    skipped, plain7, plain50 = K.spearman_text(labels, rows7, True), K.spearman_text(labels, rows7), K.spearman_text(labels, rows50)
    assert K.kept(rows7, True)[1] > 0 and skipped != plain7       # bins that are 0 in both samples: leaving them out shows
    assert min(K.min_boundary_distance(rows7, True), K.min_boundary_distance(rows7), K.min_boundary_distance(rows50)) > 1e-9
    g7 = R.gram(rows7)
    assert R.min_boundary_distance(*g7, True) > 1e-9
    out = os.path.join(tmp, "rho2_out")
    res = run(["--devices", "0,0", "-o", out + ".narrowPeak", "--spearman", out + ".tsv", "--correlation", out + ".r.tsv", "--corr-skip-zeros",
               "--bin-size", "7"])
    assert res.returncode == 0, res.stderr
    assert open(out + ".tsv").read() == skipped
    assert open(out + ".r.tsv").read() == R.correlation_text(labels, *g7, True)
    assert open(out + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")
    out = os.path.join(tmp, "rho3_out")
    res = run(["--devices", "0,0", "-o", out + ".narrowPeak", "--spearman", out + ".tsv", "--bin-size", "7"])
    assert res.returncode == 0, res.stderr
    assert open(out + ".tsv").read() == plain7
    out = os.path.join(tmp, "rho4_out")
    res = run(["-X", "-f", out + ".log", "--spearman", out + ".tsv"])
    assert res.returncode == 0, res.stderr
    assert open(out + ".tsv").read() == plain50
    out = os.path.join(tmp, "rho5_out")
    res = run(["-z", "-o", out + ".narrowPeak", "--spearman", out + ".tsv", "--corr-skip-zeros"])
    assert res.returncode == 0, res.stderr
    assert gzip.open(out + ".tsv.gz", "rb").read().decode() == K.spearman_text(labels, rows50, True)
