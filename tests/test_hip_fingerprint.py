"""The samples' fingerprint histograms on the GPU (gx_fp_u64 / gx_coverage_fingerprint: k_fp_hist) and genrich-amd --fingerprint:
exact equality with Python integers (tests/fingerprint_ref.py) at the edges of the kernel's geometry, in every class, where a
wavefront's lanes collide on one class and a sum carries across its dwords, on real runs in every form the coverage tests know,
and over two contexts."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import backends as B
import coverage_ref as CR
import fingerprint_ref as R
import golden_cases as G
from genrich_amd.lib import FP_NC, GX_PATH_FINGERPRINT, fp_geometry
from test_hip_counts import _cli_inputs
from test_hip_coverage import BEDS, C0, LENS, ORDER, PARAMS, T0, _ctx, _events, _expected, _run   # noqa: F401 (T0, C0: fixtures)
from test_host_cli import _binary

pytestmark = pytest.mark.gpu

_, _, LANES, GRID = fp_geometry()        # the kernel's own constants, from the library as built
FULL = GRID * LANES                      # the default grid x the lanes of a workgroup
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def h():
    import genrich_amd
    ctx = genrich_amd.Genrich(B.make_params(**PARAMS))
    ctx.set_chroms(LENS)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def agg():
    """A context whose k_fp_hist aggregates equal classes inside the wavefront (GX_FP_AGG): the variant that is not the default."""
    import genrich_amd
    ctx = genrich_amd.Genrich(B.make_params(**PARAMS))
    ctx.set_chroms(LENS)
    assert ctx.lib.gx_set_knob(ctx.ctx, b"GX_FP_AGG", b"1") == 0
    yield ctx
    ctx.close()


def _same(got, exp, what=""):
    count, total = got
    assert count.shape == total.shape == (len(exp[0]), FP_NC), what
    for s in range(len(exp[0])):
        assert count[s].tolist() == exp[0][s], (what, s)
        assert total[s].tolist() == exp[1][s], (what, s)


# ---- 1. gx_fp_u64 at the edges of the geometry -----------------------------------------------------------------------------

def _edge_rows(rng, S, n):
    rows = rng.integers(0, 1 << 39, (S, n)).astype(np.uint64)     # (2^24 values below 2^39 cannot reach 2^64)
    rows >>= rng.integers(0, 39, (S, n)).astype(np.uint64)        # every magnitude, the classes below 128 too
    rows[rng.random((S, n)) < 0.2] = 0
    if n:
        rows[:, -1] = (1 << 39) - 1 - np.arange(S, dtype=np.uint64)   # the last value counts
    return rows


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, LANES - 1, LANES, LANES + 1, 2 * LANES - 1, 2 * LANES, 2 * LANES + 1])
def test_small_sizes(h, agg, n):
    rng = np.random.default_rng(100 + n)
    for S in (1, 2, 3, 32):
        rows = _edge_rows(rng, S, n)
        exp = R.hist(list(rows))
        _same(h.fp_u64(rows), exp, (n, S))
        _same(agg.fp_u64(rows), exp, (n, S, "agg"))


EDGES = [FULL - 1, FULL, FULL + 1, 2 * FULL - 1, 2 * FULL, 2 * FULL + 1]


@pytest.fixture(scope="module")
def full_rows():
    """32 rows of 2 FULL + 1 values, none of the values an edge ends on zero; the histograms of their first FULL - 1 and
    2 FULL - 1 values, computed once: an edge's expectation is one of them plus the histogram of at most two values more."""
    rows = _edge_rows(np.random.default_rng(9), 32, 2 * FULL + 1)
    for n in EDGES:
        rows[:, n - 1] = 12345 + 1000 * n + np.arange(32, dtype=np.uint64)
    first = R.hist(list(rows[:, :FULL - 1]))
    return rows, {FULL - 1: first, 2 * FULL - 1: R.add(first, R.hist(list(rows[:, FULL - 1:2 * FULL - 1])))}


@pytest.mark.parametrize("n", EDGES)
def test_full_passes_of_the_default_grid(h, full_rows, n):
    """FULL values: every lane of the default grid has one; 2 FULL: a full step (a lane takes two values a step)."""
    rows, bases = full_rows
    b = max(x for x in bases if x <= n)
    exp = R.add(bases[b], R.hist(list(rows[:, b:n])))
    for S in (1, 2, 3, 32):
        _same(h.fp_u64(rows[:S, :n]), (exp[0][:S], exp[1][:S]), (n, S))


# ---- 2. every class ------------------------------------------------------------------------------------------------------------

def test_every_class(h, agg):
    top = R.cls(1 << 50)
    row = np.array([f(k) for k in range(top + 1) for f in (R.lo, R.hi)], dtype=np.uint64)
    assert int(row.astype(object).sum()) < 1 << 64
    exp = R.hist([row])
    assert all(exp[0][0][k] == 2 for k in range(top + 1)) and exp[1][0][top] == R.lo(top) + R.hi(top)
    for ctx in (h, agg):
        _same(ctx.fp_u64(row[None, :]), exp)
        _same(ctx.fp_u64(row[None, :], grid=1), exp)
    # above: the first and last class of every octave, one value a row; 2^63, 2^64 - 1 and the row [2^64 - 1, 0, 0, ...]
    values = []
    for e in range(51, 64):
        first, last = R.cls(1 << e), R.cls((2 << e) - 1)
        values += [R.lo(first), R.hi(first), R.lo(last), R.hi(last)]
    assert 1 << 63 in values and U64 in values
    for at in range(0, len(values), 32):
        part = values[at:at + 32]
        rows = np.zeros((len(part), 70), dtype=np.uint64)
        for r, v in enumerate(part):
            rows[r, 0 if v == U64 else (7 * r) % 70] = v
        exp = R.hist(list(rows))
        _same(h.fp_u64(rows), exp, at)
        _same(agg.fp_u64(rows, grid=1), exp, at)


# ---- 3. collisions and carries -----------------------------------------------------------------------------------------------

def _collision_rows():
    n = 1 << 14
    same = np.full(n, (1 << 50) - 1, dtype=np.uint64)              # the total is 2^64 - 2^14: the sum carries across its dwords
    zeros = np.zeros(n, dtype=np.uint64)
    two = np.where(np.arange(n) % 2 == 0, 1000, (1 << 33) + 5).astype(np.uint64)   # two classes, lane by lane
    one = np.zeros(64 * 8, dtype=np.uint64)
    one[70] = (1 << 50) + 3                                        # lane 6 of the second wavefront's step
    return dict(same=same, zeros=zeros, two=two, one=one)


@pytest.mark.parametrize("which", ["same", "zeros", "two", "one"])
def test_collisions_and_carries(h, agg, which):
    row = _collision_rows()[which]
    exp = R.hist([row])
    if which == "same":
        assert exp[1][0][R.cls((1 << 50) - 1)] == (1 << 64) - (1 << 14) and exp[0][0][R.cls((1 << 50) - 1)] == 1 << 14
    if which == "zeros":
        assert exp[0][0][0] == len(row) and sum(exp[1][0]) == 0
    for ctx in (h, agg):
        for grid in (0, 1):
            _same(ctx.fp_u64(row[None, :], grid=grid), exp, (which, grid))


# ---- 4. geometry -------------------------------------------------------------------------------------------------------------

def test_the_grid_does_not_matter(h, agg):
    n = 100_003
    rng = np.random.default_rng(8)
    rows = _edge_rows(rng, 5, n)
    rows[:, ::3] <<= np.uint64(8)
    exp = R.hist(list(rows))
    first = None
    for ctx in (h, agg):
        for grid in (1, 2, 7, 0):
            got = ctx.fp_u64(rows, grid=grid)
            _same(got, exp, grid)
            key = (got[0].tobytes(), got[1].tobytes())
            first = first or key
            assert key == first


# ---- 5. refusals of gx_fp_u64 ------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    import genrich_amd
    g = genrich_amd.Genrich(B.make_params(**PARAMS))
    g.set_chroms(LENS)
    lib, ctx = g.lib, g.ctx
    ok = np.ones((33, 4), dtype=np.uint64)
    bad = np.array([[1, 2, 3, 4], [1 << 63, 1 << 62, 1 << 62, 0]], dtype=np.uint64)      # the second row's total is exactly 2^64
    big = np.zeros((1, (1 << 24) + 1), dtype=np.uint64)
    c, t = np.zeros((33, FP_NC), dtype=np.uint64), np.zeros((33, FP_NC), dtype=np.uint64)
    assert lib.gx_fp_u64(ctx, bad.ctypes.data, 2, 4, 0, c.ctypes.data, t.ctypes.data) == ORDER
    assert lib.gx_fp_u64(ctx, ok.ctypes.data, 0, 4, 0, c.ctypes.data, t.ctypes.data) == ORDER            # no row
    assert lib.gx_fp_u64(ctx, ok.ctypes.data, 33, 4, 0, c.ctypes.data, t.ctypes.data) == ORDER           # 33 rows
    assert lib.gx_fp_u64(ctx, big.ctypes.data, 1, (1 << 24) + 1, 0, c.ctypes.data, t.ctypes.data) == ORDER   # n = 2^24 + 1
    assert lib.gx_fp_u64(ctx, ok.ctypes.data, 2, 4, 65536, c.ctypes.data, t.ctypes.data) == ORDER        # a grid beyond the limit
    assert not g.path_info() & GX_PATH_FINGERPRINT and not c.any() and not t.any()
    bad[1, 3] = 0
    bad[1, 2] -= np.uint64(1)                                                                             # 2^64 - 1
    assert lib.gx_fp_u64(ctx, bad.ctypes.data, 2, 4, 0, c.ctypes.data, t.ctypes.data) == 0
    assert g.path_info() & GX_PATH_FINGERPRINT
    _same((c[:2], t[:2]), R.hist(list(bad)))
    g.close()


# ---- 6. gx_coverage_fingerprint on real runs ---------------------------------------------------------------------------------------

def _dev_rows(h, S):
    return [np.concatenate([h.coverage(i, c).sum120 for c in range(len(LENS))]) for i in range(S)]


def _ref_rows(expected):
    return [np.concatenate([e[c] for c in sorted(e)]) for e in expected]


def _check_run(h, order, expected):
    """gx_coverage_fingerprint against the definition over the device's own bins and over coverage_ref's."""
    S = len(order)
    n, count, total = h.coverage_fingerprint()
    dev = R.hist(_dev_rows(h, S))
    ref = R.hist(_ref_rows(expected))
    assert dev == ref
    assert n == sum(len(x) for x in expected[0].values())
    _same((count, total), ref)
    assert all(int(count[s].sum()) == n for s in range(S))
    assert h.path_info() & GX_PATH_FINGERPRINT
    return n, count, total


@pytest.mark.parametrize("W", [1, 50, 4096, 1 << 20])
def test_a_treatment_and_a_control(W, T0, C0):
    h = _ctx(W)
    order, _ = _run(h, [(T0, C0)])
    n, count, total = _check_run(h, order, [_expected("T0", T0, W), _expected("C0", C0, W)])
    assert n == sum(CR.n_bins(x, W) for x in LENS) and (count[0][0] > 0) == (W <= 4096)
    h.close()


def test_three_replicates_with_controls(T0, C0):
    T1, T2, C1 = _events(6), _events(7, n=30_000), _events(9, n=10_000)
    h = _ctx(50)
    order, _ = _run(h, [(T0, C0), (T1, C1), (T2, C0)])
    assert len(order) == 6
    _check_run(h, order, [_expected("T0", T0, 50), _expected("C0", C0, 50), _expected("T1", T1, 50), _expected("C1", C1, 50),
                          _expected("T2", T2, 50), _expected("C0", C0, 50)])
    h.close()


def test_excluded_regions(T0, C0):
    h = _ctx(50, beds=BEDS)
    order, _ = _run(h, [(T0, C0)])
    plain = R.hist(_ref_rows([_expected("T0", T0, 50), _expected("C0", C0, 50)]))
    n, count, total = _check_run(h, order, [_expected("T0bed", T0, 50, beds=BEDS), _expected("C0bed", C0, 50, beds=BEDS)])
    assert count[0][0] > plain[0][0][0] and int(total[0].astype(object).sum()) < sum(plain[1][0])
    h.close()


def test_a_skipped_chromosome(T0):
    skip = [0, 0, 1, 0, 0]
    h = _ctx(100, skip=skip)
    order, _ = _run(h, [(T0, None)])
    n, _, _ = _check_run(h, order, [_expected("T0", T0, 100, skip=skip)])
    assert n == sum(CR.n_bins(x, 100) for c, x in enumerate(LENS) if not skip[c])
    h.close()


def test_a_save_mask_that_omits_a_chromosome_for_one_replicate(T0, C0):
    save = [1, 1, 1, 1, 0]
    h = _ctx(64)
    order, _ = _run(h, [(T0, None), (T0, None)], saves=[save, None])
    exp = [_expected("T0", T0, 64, save=save), _expected("T0", T0, 64)]
    n, count, total = _check_run(h, order, exp)
    assert count[0][0] - count[1][0] == int((exp[1][4] != 0).sum()) > 0     # chromosome 4's bins are 0 in the first sample
    h.close()


def test_fractional_weights():
    ev = _events(4, counts=(2, 3, 4, 5, 6, 8, 10))
    h = _ctx(50, frac=True)
    order, _ = _run(h, [(ev, None)])
    _, _, total = _check_run(h, order, [_expected("frac", ev, 50)])
    assert any(int(v) % 120 for v in total[0])
    h.close()


# ---- 7. two contexts ---------------------------------------------------------------------------------------------------------

def test_two_contexts_with_complementary_chromosomes_add_up(T0, C0):
    owned = [1, 0, 1, 0, 0]
    other = [1 - x for x in owned]
    parts, ctxs = [], []
    for own in (owned, other, None):
        h = _ctx(50, owned=own)
        order, _ = _run(h, [(T0, C0)])
        n, count, total = _check_run(h, order, [_expected("T0", T0, 50, owned=own), _expected("C0", C0, 50, owned=own)])
        parts.append((n, (count.tolist(), total.tolist())))
        ctxs.append(h)
    assert R.add(parts[0][1], parts[1][1]) == parts[2][1] and parts[0][0] + parts[1][0] == parts[2][0]
    # ... and the library's own adding
    c, t, n = np.zeros((2, FP_NC), dtype=np.uint64), np.zeros((2, FP_NC), dtype=np.uint64), C.c_uint64(0)
    arr = (C.c_void_p * 2)(ctxs[0].ctx.value, ctxs[1].ctx.value)
    assert ctxs[0].lib.gx_coverage_fingerprint_group(arr, 2, 2, C.byref(n), c.ctypes.data, t.ctypes.data) == 0
    assert n.value == parts[2][0] and (c.tolist(), t.tolist()) == parts[2][1]
    for h in ctxs:
        h.close()


# ---- 8. order and state --------------------------------------------------------------------------------------------------------

def _fp_rc(h):
    return h.lib.gx_coverage_fingerprint(h.ctx, None, None, None, None, 0)


def test_order_errors_and_repeatability(T0, C0):
    off = _ctx(0)
    _run(off, [(T0, None)])
    assert _fp_rc(off) == ORDER                                  # coverage off
    off.close()
    h = _ctx(50)
    assert _fp_rc(h) == ORDER                                    # before any sample
    h.sample_begin(0, None)
    assert _fp_rc(h) == ORDER                                    # a sample is open
    h.push_events(T0)
    h.sample_end()
    assert _fp_rc(h) == 0                                        # no gx_pvalues, no gx_find_peaks needed
    one = h.coverage_fingerprint()
    _same(one[1:], R.hist(_ref_rows([_expected("T0", T0, 50)])))
    small = np.zeros(FP_NC, dtype=np.uint64)
    assert h.lib.gx_coverage_fingerprint(h.ctx, None, None, small.ctypes.data, None, 0) == ORDER     # cap < S with an array
    assert h.lib.gx_coverage_fingerprint(h.ctx, None, None, None, small.ctypes.data, 0) == ORDER
    h.sample_begin(1, None)
    assert _fp_rc(h) == ORDER
    h.push_events(C0)
    h.sample_end()
    h.pvalues()
    h.find_peaks()
    a, b = h.coverage_fingerprint(), h.coverage_fingerprint()    # twice: the same
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert a[1][0].tolist() == one[1][0].tolist()                # the first sample's as between the samples
    h.reset()
    assert _fp_rc(h) == ORDER and not h.path_info() & GX_PATH_FINGERPRINT
    _run(h, [(T0, C0)])
    c = h.coverage_fingerprint()
    assert a[0] == c[0] and a[1].tobytes() == c[1].tobytes() and a[2].tobytes() == c[2].tobytes()
    h.close()


def test_the_pass_changes_nothing_else(T0, C0):
    plain, asked = _ctx(50), _ctx(50)
    _run(plain, [(T0, C0)])
    asked.sample_begin(0, None)
    asked.push_events(T0)
    asked.sample_end()
    asked.coverage_fingerprint()                                 # between the samples ...
    asked.sample_begin(1, None)
    asked.push_events(C0)
    asked.sample_end()
    asked.coverage_fingerprint()
    asked.pvalues()
    asked.find_peaks()
    asked.coverage_fingerprint()                                 # ... and after the peaks
    assert plain.get_peaks().tobytes() == asked.get_peaks().tobytes()
    for c in range(len(LENS)):
        e0, c0 = plain.get_intervals(-1, c)
        e1, c1 = asked.get_intervals(-1, c)
        assert np.array_equal(e0, e1)
        for k in ("expt", "ctrl", "p"):
            assert np.array_equal(c0[k].view(np.uint32), c1[k].view(np.uint32)), k
        for i in range(2):
            assert np.array_equal(plain.coverage(i, c).sum120, asked.coverage(i, c).sum120)
    assert asked.path_info() == plain.path_info() | GX_PATH_FINGERPRINT
    plain.close()
    asked.close()


# ---- 9. the command line -------------------------------------------------------------------------------------------------------

_CLI = {}


def _cli_expected(name, W):
    """(labels, (count, sum), ctrl_of) from the case's events alone."""
    if (name, W) not in _CLI:
        meta, case, _, names = G.load_case(name)
        rows, labels = [], []
        for r, rep in enumerate(case["replicates"]):
            for ctrl, ev in ((False, rep["treat"]), (True, rep["ctrl"])):
                if ev is None:
                    continue
                cov = CR.coverage(ev, case["lens"], W, skip=case["skip"], beds=case["beds"], save=rep["save"])
                rows.append(np.concatenate([cov[c] for c in sorted(cov)]))
                labels.append(f"{'c' if ctrl else 't'}{r}")
        ctrl_of = [labels.index("c" + l[1:]) if l[0] == "t" and "c" + l[1:] in labels else -1 for l in labels]
        _CLI[(name, W)] = labels, R.hist(rows), ctrl_of
    return _CLI[(name, W)]


def _check_files(name, W, curve, metrics):
    labels, h, ctrl_of = _cli_expected(name, W)
    assert R.check_curve(curve, labels, *h) is None, R.check_curve(curve, labels, *h)
    assert R.check_metrics(metrics, labels, *h, ctrl_of) is None, R.check_metrics(metrics, labels, *h, ctrl_of)


@pytest.mark.parametrize("name", ["ctrl_q", "reps3"])
def test_cli_fingerprint(name):
    meta, args, tmp, _ = _cli_inputs(name)
    out = os.path.join(tmp, "fp_out")
    res = subprocess.run([_binary(), "-v", "-o", out + ".narrowPeak", "--fingerprint", out + ".tsv", "--fingerprint-metrics", out + ".m.tsv"] + args,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    _check_files(name, 50, open(out + ".tsv").read(), open(out + ".m.tsv").read())
    labels, _, ctrl_of = _cli_expected(name, 50)
    assert labels == (["t0", "c0"] if name == "ctrl_q" else ["t0", "c0", "t1", "t2", "c2"])
    assert ctrl_of == ([1, -1] if name == "ctrl_q" else [1, -1, -1, 4, -1])
    lines = [l for l in res.stderr.splitlines() if l.startswith("  Fingerprint ")]
    assert [l.split()[1] for l in lines] == [l + ":" for l in labels], res.stderr
    rows = open(out + ".m.tsv").read().splitlines()[1:]
    for line, row in zip(lines, rows):                           # the same figures on stderr
        f = row.split("\t")
        assert f"zero fraction {f[4]}," in line and f"gini {f[6]}," in line and line.endswith(f"jsd to control {f[9]}"), (line, row)
    assert open(out + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")
    assert not os.path.exists(out + ".t0.bedgraph")              # the bins are on, no track is written


def test_cli_two_contexts_X_gzip_and_next_to_the_other_outputs():
    name = "ctrl_q"
    meta, args, tmp, _ = _cli_inputs(name)
    run = lambda extra: subprocess.run([_binary()] + extra + args, capture_output=True, text=True)
    out = os.path.join(tmp, "fp2_out")
    res = run(["--devices", "0,0", "-o", out + ".narrowPeak", "--fingerprint", out + ".tsv", "--fingerprint-metrics", out + ".m.tsv"])
    assert res.returncode == 0, res.stderr
    _check_files(name, 50, open(out + ".tsv").read(), open(out + ".m.tsv").read())
    assert open(out + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")
    out = os.path.join(tmp, "fp3_out")
    res = run(["-X", "-f", out + ".log", "--fingerprint", out + ".tsv", "--fingerprint-metrics", out + ".m.tsv", "--bin-size", "7"])
    assert res.returncode == 0, res.stderr
    _check_files(name, 7, open(out + ".tsv").read(), open(out + ".m.tsv").read())
    out = os.path.join(tmp, "fp4_out")
    res = run(["-z", "-o", out + ".narrowPeak", "--fingerprint", out + ".tsv", "--fingerprint-metrics", out + ".m.tsv"])
    assert res.returncode == 0, res.stderr
    _check_files(name, 50, gzip.open(out + ".tsv.gz", "rb").read().decode(), gzip.open(out + ".m.tsv.gz", "rb").read().decode())
    # next to --coverage --correlation --counts: their files are the bytes they are without --fingerprint
    others = lambda o: ["-o", o + ".narrowPeak", "--coverage", o, "--correlation", o + ".corr", "--counts", o + ".counts"]
    a, b = os.path.join(tmp, "fp5_out"), os.path.join(tmp, "fp6_out")
    res = run(others(a))
    assert res.returncode == 0, res.stderr
    res = run(others(b) + ["--fingerprint", b + ".tsv", "--fingerprint-metrics", b + ".m.tsv"])
    assert res.returncode == 0, res.stderr
    _check_files(name, 50, open(b + ".tsv").read(), open(b + ".m.tsv").read())
    for suffix in (".narrowPeak", ".t0.bedgraph", ".c0.bedgraph", ".corr", ".counts"):
        assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix
    assert not os.path.exists(a + ".tsv")
