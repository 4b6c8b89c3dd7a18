"""The samples' Gram sums on the GPU (gx_gram_u64 / gx_coverage_gram: k_gram, k_gram_sum) and genrich-amd --correlation: exact
equality with Python integers (tests/gram_ref.py) at the edges of the kernel's geometry, where carries cross lanes, wavefronts
and workgroups, on real runs in every form the coverage tests know, and over two contexts."""
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
from genrich_amd.lib import GX_PATH_GRAM, gram_geometry
from test_hip_counts import _cli_inputs
from test_hip_coverage import BEDS, C0, LENS, ORDER, PARAMS, T0, _ctx, _events, _expected, _run   # noqa: F401 (T0, C0: fixtures)
from test_host_cli import _binary

pytestmark = pytest.mark.gpu

GRAM_TILE, GRAM_LANES, GRAM_GRID = gram_geometry()   # the kernel's own constants, from the library as built
FULL = GRAM_GRID * GRAM_LANES            # one full pass of the default grid
ROWS = sorted({1, 2, 3, GRAM_TILE - 1, GRAM_TILE, GRAM_TILE + 1, 32})


@pytest.fixture(scope="module")
def h():
    import genrich_amd
    ctx = genrich_amd.Genrich(B.make_params(**PARAMS))
    ctx.set_chroms(LENS)
    yield ctx
    ctx.close()


def _same(got, exp, what=""):
    nz, s, g = got
    n, enz, es, eg = exp
    assert nz == enz, (what, nz, enz)
    assert [int(v) for v in s] == es, what
    assert [[int(v) for v in row] for row in g] == eg, what


# ---- 1. gx_gram_u64 at the edges of the geometry ---------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, GRAM_LANES - 1, GRAM_LANES, GRAM_LANES + 1])
def test_small_sizes_with_values_up_to_the_domains_end(h, n):
    rng = np.random.default_rng(100 + n)
    for S in ROWS:
        rows = rng.integers(0, 1 << 51, (S, n)).astype(np.uint64)
        rows[:, rng.random(n) < 0.2] = 0                         # all-zero bins
        if n:
            rows[rng.integers(0, S), rng.integers(0, n)] = (1 << 51) - 1
        _same(h.gram_u64(rows), R.gram(list(rows)), (n, S))


@pytest.mark.parametrize("n", [FULL - 1, FULL, FULL + 1])
def test_one_full_pass_of_the_default_grid(h, n):
    rng = np.random.default_rng(n)
    X = rng.integers(0, 1 << 20, (32, n))                        # (2^40 * 2^19 bins < 2^63: the reference is an int64 product)
    X[:, rng.random(n) < 0.3] = 0
    X[:, -1] = (1 << 20) - 1                                     # the last bin counts
    for S in ROWS:
        _same(h.gram_u64(X[:S].astype(np.uint64)), R.gram_int64(X[:S]), (n, S))


# ---- 2. carries -------------------------------------------------------------------------------------------------------

def test_carries_in_a_lane_across_lanes_and_across_workgroups(h):
    n, v = (1 << 13) + 1, (1 << 51) - 1
    rows = np.full((2, n), v, dtype=np.uint64)
    nz, s, g = h.gram_u64(rows)
    assert nz == 0 and [int(x) for x in s] == [n * v] * 2
    assert all(int(x) == n * v * v for x in g.reshape(-1)) and (n * v * v) >> 114
    nz, s, g = h.gram_u64(rows, grid=1)                         # 33 steps of one workgroup: the high word is non-zero in a lane
    assert all(int(x) == n * v * v for x in g.reshape(-1))
    assert v * v * 33 >> 64 and v * v * 64 * 4 >> 64


def test_values_around_2_to_the_32(h):
    n = 1000
    rng = np.random.default_rng(5)
    alt = np.where(np.arange(n) % 2 == 0, (1 << 32) - 1, 1 << 32).astype(np.uint64)
    below = np.full(n, (1 << 32) - 1, dtype=np.uint64)           # (the high words of this row are all 0)
    small = rng.integers(0, 1 << 32, n).astype(np.uint64)
    for rows in ([alt, small], [below, small], [below, below], [alt, alt, small, below, small]):
        _same(h.gram_u64(np.asarray(rows)), R.gram(rows))


def test_one_large_value_among_zeros_in_a_wavefront(h):
    n = 64 * 8
    rng = np.random.default_rng(6)
    one = np.zeros(n, dtype=np.uint64)
    one[70] = (1 << 50) + 3                                      # lane 6 of the second wavefront's step
    small = rng.integers(0, 1 << 32, n).astype(np.uint64)
    small[70] = (1 << 32) - 1
    zero = np.zeros(n, dtype=np.uint64)
    _same(h.gram_u64(np.asarray([one, small])), R.gram([one, small]))
    _same(h.gram_u64(np.asarray([small, one, zero, small, one])), R.gram([small, one, zero, small, one]))


# ---- 3. geometry ------------------------------------------------------------------------------------------------------

def test_the_grid_does_not_matter(h):
    n = 100_003
    rng = np.random.default_rng(8)
    rows = rng.integers(0, 1 << 51, (5, n)).astype(np.uint64)
    rows[:, rng.random(n) < 0.1] = 0
    exp = R.gram(list(rows))
    first = None
    for grid in (1, 2, 7, 0):
        got = h.gram_u64(rows, grid=grid)
        _same(got, exp, grid)
        key = (got[0], got[1].tolist(), got[2].tolist())
        first = first or key
        assert key == first


# ---- 4. refusals of gx_gram_u64 -----------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    import genrich_amd
    g = genrich_amd.Genrich(B.make_params(**PARAMS))
    g.set_chroms(LENS)
    lib, ctx = g.lib, g.ctx
    nz = C.c_uint64(0)
    ok = np.ones((33, 4), dtype=np.uint64)
    bad = ok[:2].copy()
    bad[1, 3] = 1 << 51
    big = np.zeros((1, (1 << 24) + 1), dtype=np.uint64)
    assert lib.gx_gram_u64(ctx, bad.ctypes.data, 2, 4, 0, C.byref(nz), None, None) == ORDER          # a value of 2^51
    assert lib.gx_gram_u64(ctx, big.ctypes.data, 1, (1 << 24) + 1, 0, C.byref(nz), None, None) == ORDER   # n = 2^24 + 1
    assert lib.gx_gram_u64(ctx, ok.ctypes.data, 0, 4, 0, C.byref(nz), None, None) == ORDER           # no row
    assert lib.gx_gram_u64(ctx, ok.ctypes.data, 33, 4, 0, C.byref(nz), None, None) == ORDER          # 33 rows
    assert lib.gx_gram_u64(ctx, ok.ctypes.data, 2, 4, 65536, C.byref(nz), None, None) == ORDER       # a grid beyond the limit
    assert not g.path_info() & GX_PATH_GRAM
    bad[1, 3] = (1 << 51) - 1
    assert lib.gx_gram_u64(ctx, bad.ctypes.data, 2, 4, 0, C.byref(nz), None, None) == 0 and nz.value == 0
    assert g.path_info() & GX_PATH_GRAM
    g.close()


# ---- 5. gx_coverage_gram on real runs -------------------------------------------------------------------------------------

def _dev_rows(h, S):
    return [np.concatenate([h.coverage(i, c).sum120 for c in range(len(LENS))]) for i in range(S)]


def _ref_rows(expected):
    return [np.concatenate([e[c] for c in sorted(e)]) for e in expected]


def _check_run(h, order, expected):
    """gx_coverage_gram against the definition over the device's own bins and over coverage_ref's."""
    S = len(order)
    n, nz, s, g = h.coverage_gram()
    dev = R.gram(_dev_rows(h, S))
    ref = R.gram(_ref_rows(expected))
    assert dev == ref
    assert n == ref[0] == sum(len(x) for x in expected[0].values())
    _same((nz, s, g), ref)
    assert h.path_info() & GX_PATH_GRAM
    return n, nz, s, g


@pytest.mark.parametrize("W", [1, 50, 4096, 1 << 20])
def test_a_treatment_and_a_control(W, T0, C0):
    h = _ctx(W)
    order, _ = _run(h, [(T0, C0)])
    n, nz, s, g = _check_run(h, order, [_expected("T0", T0, W), _expected("C0", C0, W)])
    assert n == sum(CR.n_bins(x, W) for x in LENS) and int(g[0][1]) > 0 and (nz > 0) == (W <= 4096)
    h.close()


def test_three_replicates_with_controls(T0, C0):
    T1, T2, C1 = _events(6), _events(7, n=30_000), _events(9, n=10_000)
    h = _ctx(50)
    order, _ = _run(h, [(T0, C0), (T1, C1), (T2, C0)])
    assert len(order) == 6                                       # more than one tile of the pair matrix
    _check_run(h, order, [_expected("T0", T0, 50), _expected("C0", C0, 50), _expected("T1", T1, 50), _expected("C1", C1, 50),
                          _expected("T2", T2, 50), _expected("C0", C0, 50)])
    h.close()


def test_excluded_regions(T0, C0):
    h = _ctx(50, beds=BEDS)
    order, _ = _run(h, [(T0, C0)])
    plain = R.gram(_ref_rows([_expected("T0", T0, 50), _expected("C0", C0, 50)]))
    n, nz, s, g = _check_run(h, order, [_expected("T0bed", T0, 50, beds=BEDS), _expected("C0bed", C0, 50, beds=BEDS)])
    assert nz > plain[1] and int(s[0]) < plain[2][0]
    h.close()


def test_a_skipped_chromosome(T0):
    skip = [0, 0, 1, 0, 0]
    h = _ctx(100, skip=skip)
    order, _ = _run(h, [(T0, None)])
    n, _, _, _ = _check_run(h, order, [_expected("T0", T0, 100, skip=skip)])
    assert n == sum(CR.n_bins(x, 100) for c, x in enumerate(LENS) if not skip[c])
    h.close()


def test_a_save_mask_that_omits_a_chromosome_for_one_replicate(T0, C0):
    save = [1, 1, 1, 1, 0]
    h = _ctx(64)
    order, _ = _run(h, [(T0, None), (T0, None)], saves=[save, None])
    exp = [_expected("T0", T0, 64, save=save), _expected("T0", T0, 64)]
    n, nz, s, g = _check_run(h, order, exp)
    # chromosome 4's bins are 0 in the first sample; they count as all zero only where the second is 0 too
    both = int(((exp[0][4] == 0) & (exp[1][4] == 0)).sum())
    assert 0 < both < len(exp[0][4]) and nz == both + sum(int((exp[1][c] == 0).sum()) for c in range(4))
    h.close()


def test_fractional_weights():
    ev = _events(4, counts=(2, 3, 4, 5, 6, 8, 10))
    h = _ctx(50, frac=True)
    order, _ = _run(h, [(ev, None)])
    _, _, s, _ = _check_run(h, order, [_expected("frac", ev, 50)])
    assert int(s[0]) % 120
    h.close()


# ---- 6. two contexts ------------------------------------------------------------------------------------------------------

def test_two_contexts_with_complementary_chromosomes_add_up(T0, C0):
    owned = [1, 0, 1, 0, 0]
    other = [1 - x for x in owned]
    parts = []
    for own in (owned, other, None):
        h = _ctx(50, owned=own)
        order, _ = _run(h, [(T0, C0)])
        n, nz, s, g = _check_run(h, order, [_expected("T0", T0, 50, owned=own), _expected("C0", C0, 50, owned=own)])
        parts.append((n, nz, [int(v) for v in s], [[int(v) for v in row] for row in g]))
        h.close()
    assert R.add(parts[0], parts[1]) == parts[2]


# ---- 7. order and state ---------------------------------------------------------------------------------------------------

def _gram_rc(h):
    return h.lib.gx_coverage_gram(h.ctx, None, None, None, None, None, 0)


def test_order_errors_and_repeatability(T0, C0):
    off = _ctx(0)
    _run(off, [(T0, None)])
    assert _gram_rc(off) == ORDER                                # coverage off
    off.close()
    h = _ctx(50)
    assert _gram_rc(h) == ORDER                                  # before any sample
    h.sample_begin(0, None)
    assert _gram_rc(h) == ORDER                                  # a sample is open
    h.push_events(T0)
    h.sample_end()
    assert _gram_rc(h) == 0                                      # no gx_pvalues, no gx_find_peaks needed
    one = h.coverage_gram()
    _same(one[1:], R.gram(_ref_rows([_expected("T0", T0, 50)])))
    small = np.zeros(1, dtype=[("lo", "<u8"), ("hi", "<u8")])
    assert h.lib.gx_coverage_gram(h.ctx, None, None, None, small.ctypes.data, None, 0) == ORDER      # cap < S with an array
    h.sample_begin(1, None)
    assert _gram_rc(h) == ORDER
    h.push_events(C0)
    h.sample_end()
    h.pvalues()
    h.find_peaks()
    a, b = h.coverage_gram(), h.coverage_gram()                  # twice: the same
    assert (a[0], a[1], a[2].tolist(), a[3].tolist()) == (b[0], b[1], b[2].tolist(), b[3].tolist())
    h.reset()
    assert _gram_rc(h) == ORDER and not h.path_info() & GX_PATH_GRAM
    _run(h, [(T0, C0)])
    c = h.coverage_gram()
    assert (a[0], a[1], a[2].tolist(), a[3].tolist()) == (c[0], c[1], c[2].tolist(), c[3].tolist())
    h.close()


def test_the_pass_changes_nothing_else(T0, C0):
    plain, asked = _ctx(50), _ctx(50)
    _run(plain, [(T0, C0)])
    asked.sample_begin(0, None)
    asked.push_events(T0)
    asked.sample_end()
    asked.coverage_gram()                                        # between the samples ...
    asked.sample_begin(1, None)
    asked.push_events(C0)
    asked.sample_end()
    asked.coverage_gram()
    asked.pvalues()
    asked.find_peaks()
    asked.coverage_gram()                                        # ... and after the peaks
    assert plain.get_peaks().tobytes() == asked.get_peaks().tobytes()
    for c in range(len(LENS)):
        e0, c0 = plain.get_intervals(-1, c)
        e1, c1 = asked.get_intervals(-1, c)
        assert np.array_equal(e0, e1)
        for k in ("expt", "ctrl", "p"):
            assert np.array_equal(c0[k].view(np.uint32), c1[k].view(np.uint32)), k
        for i in range(2):
            assert np.array_equal(plain.coverage(i, c).sum120, asked.coverage(i, c).sum120)
    assert asked.path_info() == plain.path_info() | GX_PATH_GRAM
    plain.close()
    asked.close()


# ---- 8. the command line --------------------------------------------------------------------------------------------------

def _cli_expected(name, W, skip_zeros=False):
    """(--correlation's text, n, n_zero) from the case's events alone."""
    meta, case, _, names = G.load_case(name)
    rows, labels = [], []
    for r, rep in enumerate(case["replicates"]):
        for ctrl, ev in ((False, rep["treat"]), (True, rep["ctrl"])):
            if ev is None:
                continue
            cov = CR.coverage(ev, case["lens"], W, skip=case["skip"], beds=case["beds"], save=rep["save"])
            rows.append(np.concatenate([cov[c] for c in sorted(cov)]))
            labels.append(f"{'c' if ctrl else 't'}{r}")
    g = R.gram(rows)
    return R.correlation_text(labels, *g, skip_zeros), g[0], g[1]


@pytest.mark.parametrize("name", ["basic", "ctrl_q"])
def test_cli_correlation(name):
    meta, args, tmp, _ = _cli_inputs(name)
    out = os.path.join(tmp, "corr_out")
    res = subprocess.run([_binary(), "-v", "-o", out + ".narrowPeak", "--correlation", out + ".tsv"] + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    text, n, nz = _cli_expected(name, 50)
    assert open(out + ".tsv").read() == text
    assert (name == "ctrl_q") == ("\tc0" in text.splitlines()[0])
    line = [l for l in res.stderr.splitlines() if l.startswith("  Correlation: ")]
    assert len(line) == 1 and line[0].startswith(f"  Correlation: {n} bins, {nz} all zero; "), res.stderr
    assert open(out + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")
    assert not os.path.exists(out + ".t0.bedgraph")              # the bins are on, no track is written


def test_cli_two_contexts_skip_zeros_X_gzip_and_next_to_coverage():
    name = "ctrl_q"
    meta, args, tmp, _ = _cli_inputs(name)
    text, _, nz = _cli_expected(name, 50)
    run = lambda extra: subprocess.run([_binary()] + extra + args, capture_output=True, text=True)
    out = os.path.join(tmp, "corr2_out")
    res = run(["--devices", "0,0", "-o", out + ".narrowPeak", "--correlation", out + ".tsv"])
    assert res.returncode == 0, res.stderr
    assert open(out + ".tsv").read() == text
    assert open(out + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")
    text7, _, nz7 = _cli_expected(name, 7)                       # (at 50 bases no bin of this case is 0 in both samples)
    skipped, _, _ = _cli_expected(name, 7, skip_zeros=True)
    assert nz == 0 and nz7 > 0 and skipped != text7
    out = os.path.join(tmp, "corr3_out")
    res = run(["-o", out + ".narrowPeak", "--correlation", out + ".tsv", "--corr-skip-zeros", "--bin-size", "7"])
    assert res.returncode == 0, res.stderr
    assert open(out + ".tsv").read() == skipped
    out = os.path.join(tmp, "corr4_out")
    res = run(["-X", "-f", out + ".log", "--correlation", out + ".tsv"])
    assert res.returncode == 0, res.stderr
    assert open(out + ".tsv").read() == text
    out = os.path.join(tmp, "corr5_out")
    res = run(["-z", "-o", out + ".narrowPeak", "--correlation", out + ".tsv"])
    assert res.returncode == 0, res.stderr
    assert gzip.open(out + ".tsv.gz", "rb").read().decode() == text
    out = os.path.join(tmp, "corr6_out")
    res = run(["-o", out + ".narrowPeak", "--correlation", out + ".tsv", "--coverage", out, "--bin-size", "7"])
    assert res.returncode == 0, res.stderr
    assert open(out + ".tsv").read() == text7 and text7 != text
    case = G.load_case(name)[1]
    names = G.load_case(name)[3]
    cov = CR.coverage(case["replicates"][0]["treat"], case["lens"], 7, skip=case["skip"], beds=case["beds"], save=case["replicates"][0]["save"])
    assert open(out + ".t0.bedgraph").read() == CR.coverage_text(names, case["lens"], 7, cov)
