"""Binned coverage of every sample's pileup on the GPU (gx_set_coverage_bins / k_cov_bins, genrich-amd --coverage): exact
equality with the numpy definition (tests/coverage_ref.py) of every sample and chromosome, for every class of bin size, on
every tile-stage path, in every form the sample can be in when it is closed."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import backends as B
import coverage_ref as R
import golden_cases as G
from genrich_amd.lib import GX_PATH_COVERAGE
from test_hip_counts import Mem, _cli_inputs, _push
from test_host_cli import _binary

pytestmark = pytest.mark.gpu

LENS = [3 * 4096 + 17, 4096, 4097, 37, 200_000]
ORDER = -10
BIN_SIZES = [1, 7, 16, 50, 64, 100, 1000, 4096, 5000, 65536, 1 << 20]
PARAMS = dict(pq=0.01, min_auc=20.0)


def _events(seed, n=24_000, counts=(1,)):
    """n short fragments in clusters that leave long stretches of chromosome 4 empty, plus intervals longer than two tiles
    (some across the empty stretches: tiles without a breakpoint under a non-zero pileup) and ends beyond the lengths."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(LENS, dtype=np.int64)
    ev = np.zeros(n, dtype=B.EVENT_DTYPE)
    ev["chrom"] = rng.choice(len(LENS), n, p=[0.2, 0.1, 0.1, 0.02, 0.58])
    ch = ev["chrom"].astype(np.int64)
    start = rng.integers(0, lens[ch])
    on4 = ch == 4
    zone = rng.choice([0, 30_000, 110_000, 190_000], int(on4.sum()))          # nothing starts in [40 000, 110 000) or [120 000, 190 000)
    start[on4] = zone + rng.integers(0, 10_000, int(on4.sum()))
    ev["start"] = start
    ev["end"] = start + rng.integers(1, 400, n)                                # (beyond the length now and then: clamped)
    ev["count"] = rng.choice(counts, n)
    long_ = np.zeros(40, dtype=B.EVENT_DTYPE)
    long_["chrom"] = [4] * 30 + [0] * 10
    long_["start"] = np.concatenate([rng.integers(35_000, 100_000, 30), rng.integers(0, 3000, 10)])
    long_["end"] = long_["start"] + np.concatenate([rng.integers(2 * 4096 + 1, 70_000, 30), rng.integers(2 * 4096 + 1, 12_000, 10)])
    long_["count"] = rng.choice(counts, 40)
    ev = np.concatenate([ev, long_])
    return ev[rng.permutation(len(ev))]


_PILES = {}


def _expected(key, ev, W, skip=None, beds=None, save=None, owned=None):
    """coverage_ref's bins; the per-base pileups of a sample are computed once (`key` names the sample and its masks)."""
    if key not in _PILES:
        _PILES[key] = {c: R.pileup120(ev, c, LENS[c], beds[c] if beds is not None else ()) for c in range(len(LENS))}
    out = {}
    for c, length in enumerate(LENS):
        if (skip is not None and skip[c]) or (owned is not None and not owned[c]):
            continue
        live = save is None or save[c]
        out[c] = R.bin_sums(_PILES[key][c], W) if live else np.zeros(R.n_bins(length, W), dtype=np.int64)
    return out


def _ctx(W, skip=None, beds=None, owned=None, knobs=(), frac=False, params=None):
    import genrich_amd
    h = genrich_amd.Genrich(B.make_params(**(params or PARAMS)))
    h.set_chroms(LENS, skip, beds)
    if owned is not None:
        h.set_owned(owned)
    for k, v in knobs:
        h.set_knob(k, v)
    if frac:
        h.expect_fractional(True)
    if W:
        h.set_coverage_bins(W)
    return h


def _run(h, reps, mode="host", saves=None, mem=None):
    """reps = [(treatment events, control events | None)]; -> the samples in gx_sample_end order as (rep, is_ctrl)."""
    mem = mem or Mem()
    order = []
    for r, (t, c) in enumerate(reps):
        h.sample_begin(0, saves[r] if saves else None)
        _push(h, t, mode, mem)
        h.sample_end()
        order.append((r, False))
        if c is not None:
            h.sample_begin(1, None)
            _push(h, c, mode, mem)
            h.sample_end()
            order.append((r, True))
        else:
            h.sample_no_control()
        h.pvalues()
    h.find_peaks()
    return order, mem


def _check(h, order, expected):
    """expected[i] = {chrom: bins} of sample i: every sample and every chromosome, exactly."""
    assert h.coverage_samples() == len(order) == len(expected)
    for i, ((r, ctrl), exp) in enumerate(zip(order, expected)):
        for c in range(len(LENS)):
            got = h.coverage(i, c)
            assert (got.rep, got.is_ctrl) == (r, ctrl)
            if c not in exp:
                assert h.coverage_bin_count(c) == 0 and got.sum120.size == 0
                continue
            assert got.sum120.dtype == np.int64 and got.sum120.shape == exp[c].shape, (i, c)
            bad = np.flatnonzero(got.sum120 != exp[c])
            assert bad.size == 0, (i, c, bad[:8], got.sum120[bad[:8]], exp[c][bad[:8]])


@pytest.fixture(scope="module")
def T0():
    return _events(1)


@pytest.fixture(scope="module")
def C0():
    return _events(2, n=20_000)


@pytest.mark.parametrize("W", BIN_SIZES)
def test_every_bin_size_on_the_default_path(W, T0):
    h = _ctx(W)
    order, _ = _run(h, [(T0, None)])
    exp = _expected("T0", T0, W)
    assert any(x.any() for x in exp.values()) and sum(len(x) for x in exp.values()) == sum(R.n_bins(n, W) for n in LENS)
    _check(h, order, [exp])
    assert h.path_info() & GX_PATH_COVERAGE
    h.close()


@pytest.mark.parametrize("W", [50, 4096])
@pytest.mark.parametrize("knob", [("GX_NO_FUSED", 1), ("GX_NO_PAIRS", 1), ("GX_SBT_GRID", 1)])
def test_forced_tile_stage_paths(knob, W, T0, C0):
    h = _ctx(W, knobs=[knob])
    order, _ = _run(h, [(T0, C0)])
    _check(h, order, [_expected("T0", T0, W), _expected("C0", C0, W)])
    flags = h.path_info()
    assert not (knob[0] == "GX_NO_FUSED" and flags & 1) and not (knob[0] == "GX_NO_PAIRS" and flags & 16), flags   # (the path was forced)
    h.close()


@pytest.mark.parametrize("W", [50, 5000])
def test_a_pile_of_5000_fragments_in_one_tile(W, T0):
    tower = np.zeros(5000, dtype=B.EVENT_DTYPE)
    rng = np.random.default_rng(3)
    tower["chrom"] = 4
    tower["start"] = 2 * 4096 + 100 + rng.integers(0, 300, 5000)
    tower["end"] = tower["start"] + rng.integers(50, 900, 5000)
    tower["count"] = 1
    ev = np.concatenate([T0[:12_000], tower, T0[12_000:]])
    h = _ctx(W)
    order, _ = _run(h, [(ev, None)])
    exp = _expected("tower", ev, W)
    assert exp[4].max() >= 120 * 2000 * min(W, 50)
    _check(h, order, [exp])
    h.close()


def test_fractional_weights():
    ev = _events(4, counts=(2, 3, 4, 5, 6, 8, 10))
    for W in (50, 4096):
        h = _ctx(W, frac=True)
        order, _ = _run(h, [(ev, None)])
        exp = _expected("frac", ev, W)
        assert any((x % 120 != 0).any() for x in exp.values())
        _check(h, order, [exp])
        h.close()


# -E regions: one from base 0, one that ends at a tile edge, one inside one bin of 50, one to the chromosome's end
BEDS = [[0, 100, 5000, 8192], [], [4090, 4097], [], [20_010, 20_030, 36_000, 45_000, 199_000, 200_000]]


@pytest.mark.parametrize("W", [50, 4096])
def test_excluded_regions(W, T0, C0):
    h = _ctx(W, beds=BEDS)
    order, _ = _run(h, [(T0, C0)])
    et, ec = _expected("T0bed", T0, W, beds=BEDS), _expected("C0bed", C0, W, beds=BEDS)
    plain = _expected("T0", T0, W)
    assert any((et[c] != plain[c]).any() for c in et)
    _check(h, order, [et, ec])
    h.close()
    h = _ctx(W, beds=BEDS)   # ... and without a control
    order, _ = _run(h, [(T0, None)])
    _check(h, order, [et])
    h.close()


def test_a_skipped_chromosome(T0):
    skip = [0, 0, 1, 0, 0]
    h = _ctx(100, skip=skip)
    order, _ = _run(h, [(T0, None)])
    exp = _expected("T0", T0, 100, skip=skip)
    assert sorted(exp) == [0, 1, 3, 4]
    _check(h, order, [exp])
    h.close()


def test_a_save_mask_that_omits_a_chromosome_for_one_replicate(T0, C0):
    save = [1, 1, 0, 1, 1]
    h = _ctx(64)
    order, _ = _run(h, [(T0, C0), (T0, None)], saves=[save, None])
    exp = [_expected("T0", T0, 64, save=save), _expected("C0", C0, 64, save=save), _expected("T0", T0, 64)]
    assert not exp[0][2].any() and exp[2][2].any()
    _check(h, order, exp)
    h.close()


def test_treatment_and_control_raw_pileups(T0, C0):
    h = _ctx(50, params=dict(pq=0.05, qval=True, min_auc=20.0))
    order, _ = _run(h, [(T0, C0)])
    assert order == [(0, False), (0, True)]
    _check(h, order, [_expected("T0", T0, 50), _expected("C0", C0, 50)])   # (the control's own pileup: no factor, no lambda)
    h.close()


def test_three_replicates_reuse_the_loose_slots(T0, C0):
    T1, T2 = _events(6), _events(7, n=30_000)
    h = _ctx(50)
    order, _ = _run(h, [(T0, C0), (T1, None), (T2, C0)])
    assert order == [(0, False), (0, True), (1, False), (2, False), (2, True)]
    _check(h, order, [_expected("T0", T0, 50), _expected("C0", C0, 50), _expected("T1", T1, 50), _expected("T2", T2, 50),
                      _expected("C0", C0, 50)])
    h.close()


@pytest.mark.parametrize("mode", ["packed_host", "packed_device", "device"])
def test_packed_and_device_pushes(mode, T0, C0):
    h = _ctx(50)
    order, mem = _run(h, [(T0, C0)], mode=mode)
    _check(h, order, [_expected("T0", T0, 50), _expected("C0", C0, 50)])
    h.close()
    mem.free()


@pytest.mark.parametrize("W", [50, 5000])
def test_two_contexts_with_complementary_chromosomes(W, T0, C0):
    owned = [1, 0, 1, 0, 0]
    other = [1 - x for x in owned]
    ha, hb = _ctx(W, owned=owned), _ctx(W, owned=other)
    ev = [(T0, C0)]
    # (no collectives between them: each is a run of its own on its chromosomes, which is all the bins depend on)
    oa, _ = _run(ha, ev)
    ob, _ = _run(hb, ev)
    _check(ha, oa, [_expected("T0", T0, W, owned=owned), _expected("C0", C0, W, owned=owned)])
    _check(hb, ob, [_expected("T0", T0, W, owned=other), _expected("C0", C0, W, owned=other)])
    one = _ctx(W)
    o1, _ = _run(one, ev)
    for i in range(2):
        for c in range(len(LENS)):
            parts = np.concatenate([ha.coverage(i, c).sum120, hb.coverage(i, c).sum120])
            assert np.array_equal(parts, one.coverage(i, c).sum120), (i, c)
    for h in (ha, hb, one):
        h.close()


def test_reset_keeps_the_switch_and_a_second_run_equals_the_first(T0, C0):
    h = _ctx(100)
    order, _ = _run(h, [(T0, C0)])
    first = [[h.coverage(i, c).sum120.copy() for c in range(len(LENS))] for i in range(2)]
    _check(h, order, [_expected("T0", T0, 100), _expected("C0", C0, 100)])
    h.reset()
    assert h.coverage_samples() == 0 and not h.path_info() & GX_PATH_COVERAGE
    assert h.lib.gx_get_coverage(h.ctx, 0, 0, None, None, None, 0) == ORDER     # the results are gone ...
    assert h.coverage_bin_count(4) == R.n_bins(LENS[4], 100)                    # ... the switch is not
    order, _ = _run(h, [(T0, C0)])
    assert h.coverage_samples() == 2
    for i in range(2):
        for c in range(len(LENS)):
            assert np.array_equal(h.coverage(i, c).sum120, first[i][c])
    h.close()


@pytest.mark.parametrize("with_ctrl", [False, True])
def test_the_switch_changes_nothing_else(with_ctrl, T0, C0):
    reps = [(T0, C0 if with_ctrl else None)]
    off, on = _ctx(0), _ctx(50)
    _run(off, reps)
    _run(on, reps)
    assert off.get_peaks().tobytes() == on.get_peaks().tobytes()
    for c in range(len(LENS)):
        e0, c0 = off.get_intervals(-1, c)
        e1, c1 = on.get_intervals(-1, c)
        assert np.array_equal(e0, e1)
        for k in ("expt", "ctrl", "p"):
            assert np.array_equal(c0[k].view(np.uint32), c1[k].view(np.uint32)), k
    f0, f1 = off.path_info(), on.path_info()
    assert not f0 & GX_PATH_COVERAGE and f1 == f0 | GX_PATH_COVERAGE, (f0, f1)
    assert off.coverage_samples() == 0
    off.close()
    on.close()


def test_order_errors(T0):
    import genrich_amd
    h = genrich_amd.Genrich(B.make_params(**PARAMS))
    lib, ctx = h.lib, h.ctx
    assert lib.gx_set_coverage_bins(ctx, 50) == ORDER                  # before gx_set_chroms
    h.set_chroms(LENS)
    assert lib.gx_set_coverage_bins(ctx, (1 << 20) + 1) == ORDER       # bin_size out of range
    assert lib.gx_set_coverage_bins(ctx, 1 << 20) == 0
    assert lib.gx_set_coverage_bins(ctx, 50) == 0
    h.sample_begin(0, None)
    assert lib.gx_set_coverage_bins(ctx, 10) == ORDER                  # a sample is open
    assert lib.gx_get_coverage(ctx, 0, 0, None, None, None, 0) == ORDER
    h.push_events(T0)
    h.sample_end()
    assert lib.gx_set_coverage_bins(ctx, 10) == ORDER                  # not idle
    assert lib.gx_get_coverage(ctx, 0, 0, None, None, None, 0) == 0    # no gx_pvalues, no gx_find_peaks needed
    assert np.array_equal(h.coverage(0, 4).sum120, _expected("T0", T0, 50)[4])
    assert lib.gx_get_coverage(ctx, 1, 0, None, None, None, 0) == ORDER   # no such sample
    assert lib.gx_get_coverage(ctx, -1, 0, None, None, None, 0) == ORDER
    assert lib.gx_get_coverage(ctx, 0, len(LENS), None, None, None, 0) == ORDER   # no such chromosome
    buf = np.zeros(4, dtype=np.int64)
    assert lib.gx_get_coverage(ctx, 0, 4, None, None, None, 4) == ORDER   # cap without an array
    assert lib.gx_get_coverage(ctx, 0, 4, None, None, buf.ctypes.data, 4) == 0
    assert np.array_equal(buf, _expected("T0", T0, 50)[4][:4])
    h.sample_begin(1, None)
    assert lib.gx_get_coverage(ctx, 0, 0, None, None, None, 0) == ORDER   # a sample is open
    h.push_events(T0[:1000])
    h.sample_end()
    h.pvalues()
    h.find_peaks()
    assert lib.gx_set_coverage_bins(ctx, 10) == ORDER                  # until gx_reset
    h.reset()
    assert lib.gx_set_coverage_bins(ctx, 0) == 0
    assert h.coverage_bin_count(4) == 0
    h.close()


def test_too_many_bins():
    import genrich_amd
    h = genrich_amd.Genrich(B.make_params(**PARAMS))
    h.set_chroms([4_000_000_000, 100], skip=[0, 0])
    assert h.lib.gx_set_coverage_bins(h.ctx, 1) == ORDER      # 4 x 10^9 bins > 2^30
    assert h.lib.gx_set_coverage_bins(h.ctx, 4) == 0          # 10^9 + 25 <= 2^30
    h.close()


# ---- the command line -------------------------------------------------------------------------------------------------

def _cli_expected(name, W, scale=1.0):
    """{file suffix: text}, the -v lines: from the case's events alone."""
    meta, case, _, names = G.load_case(name)
    files, lines = {}, []
    for r, rep in enumerate(case["replicates"]):
        for ctrl, ev in ((False, rep["treat"]), (True, rep["ctrl"])):
            if ev is None:
                continue
            cov = R.coverage(ev, case["lens"], W, skip=case["skip"], beds=case["beds"], save=rep["save"])
            files[f".{'c' if ctrl else 't'}{r}.bedgraph"] = R.coverage_text(names, case["lens"], W, cov, scale)
            lines.append(R.mean_line(r, ctrl, case["lens"], cov))
    return files, lines


@pytest.mark.parametrize("name", ["basic", "ctrl_q", "bedx"])
def test_cli_coverage(name):
    meta, args, tmp, _ = _cli_inputs(name)
    out = os.path.join(tmp, "cov_out")
    res = subprocess.run([_binary(), "-v", "-o", out + ".narrowPeak", "--coverage", out] + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    files, lines = _cli_expected(name, 50)
    assert files and all(t for t in files.values())
    for suffix, text in files.items():
        assert open(out + suffix).read() == text, suffix
    assert [l for l in res.stderr.splitlines() if l.startswith("  Coverage, ")] == lines
    assert open(out + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")


def test_cli_bin_size_scale_gzip_two_contexts_and_X():
    name = "ctrl_q"
    meta, args, tmp, _ = _cli_inputs(name)
    out = os.path.join(tmp, "covz_out")
    res = subprocess.run([_binary(), "-z", "-o", out + ".narrowPeak", "--coverage", out, "--bin-size", "7", "--coverage-scale", "0.25"] + args,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    files, _ = _cli_expected(name, 7, 0.25)
    for suffix, text in files.items():
        assert gzip.open(out + suffix + ".gz", "rb").read().decode() == text, suffix
    assert gzip.open(out + ".narrowPeak.gz", "rb").read() == G.read_gz(name, "out.narrowPeak")
    files, _ = _cli_expected(name, 4096)
    out2 = os.path.join(tmp, "cov2_out")
    res = subprocess.run([_binary(), "--devices", "0,0", "-o", out2 + ".narrowPeak", "--coverage", out2, "--bin-size", "4096"] + args,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    for suffix, text in files.items():
        assert open(out2 + suffix).read() == text, suffix
    assert open(out2 + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")
    out3 = os.path.join(tmp, "cov3_out")
    res = subprocess.run([_binary(), "-X", "-f", out3 + ".log", "--coverage", out3, "--bin-size", "4096"] + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    for suffix, text in files.items():
        assert open(out3 + suffix).read() == text, suffix


def test_cli_refusals(tmp_path):
    meta, args, tmp, _ = _cli_inputs("basic")
    pre = str(tmp_path / "cov")
    for extra in (["--coverage", pre, "-P", "-f", os.path.join(tmp, "nonexistent.log")], ["--coverage", pre, "--events-only"]):
        res = subprocess.run([_binary(), "-o", str(tmp_path / "o.np")] + args + extra, capture_output=True, text=True)
        assert res.returncode == 1 and "--coverage" in res.stderr, res.stderr
    for extra in (["--bin-size", "10"], ["--coverage-scale", "2"]):
        res = subprocess.run([_binary(), "-o", str(tmp_path / "o.np")] + args + extra, capture_output=True, text=True)
        assert res.returncode == 1 and "--coverage" in res.stderr, res.stderr
    for bad in ("0", "1048577"):
        res = subprocess.run([_binary(), "-o", str(tmp_path / "o.np"), "--coverage", pre, "--bin-size", bad] + args, capture_output=True, text=True)
        assert res.returncode == 1 and "--bin-size" in res.stderr, res.stderr
    assert not list(tmp_path.iterdir())
