"""Lengths and per-chromosome tallies of each sample's intervals on the GPU (gx_interval_stats, genrich-amd --lengths /
--chrom-stats): against the reference's own -b interval lists of the golden fixtures through the command line, and against
tests/lengths_ref.py on planted synthetic events in every push mode, launch geometry and list capacity.

A sample that is built rejects an event with an invalid count, an unknown chromosome or a start beyond an active chromosome, so
those three kinds reach the kernel through gx_interval_stats_events only; everything else of the planted set goes through real
samples as well.  Every comparison is == on integers, or on bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import backends as B
import golden_cases as G
import lengths_ref as R
from genrich_amd import synth
from genrich_amd.lib import (GX_PATH_COMPLEXITY, GX_PATH_IVSTAT, filter_saturation, interval_stats_geometry, interval_stats_group,
                             interval_stats_text)
from test_hip_complexity import ACTIVE6, FIXTURES, LENS6, MODES, OWNED6, SKIP6, _events, _hook_events, _repeat, _run3, _run6
from test_hip_counts import LENS, _cli_inputs
from test_host_cli import _binary

pytestmark = pytest.mark.gpu

ORDER = -10
HOOK_ACTIVE6 = [1, 1, 1, 0, 1, 0]      # (the hook's sample lists every chromosome in its save mask; -e and ownership hold)


def _planted():
    """About 300,000 events a sample takes: see the list in test_planted_events_in_every_push_mode.  The two runs of 70,000 stay
    in one piece behind the shuffled rest, so that whole wavefronts, batches and chunks hold nothing else."""
    bound = interval_stats_geometry()[2]
    rng = np.random.default_rng(37)
    parts = [synth.make_fragments(LENS, 150_000, 61, peak_every=20_000, tower_every=3_000_000)]
    for i, L in enumerate((bound - 1, bound, bound + 1)):            # the last LDS class, the list's first two entries
        parts.append(_repeat(1, 2_000_000 + 50_000 * i, 2_000_000 + 50_000 * i + L, [1, 2] if L == bound else [1], 5))
    parts.append(_repeat(0, 9_000_000, 9_070_000, [1], 3))           # too long to travel packed
    parts.append(_events([(0, 7_000_000, 7_000_000, 1), (0, 7_000_000, 7_000_000, 3), (1, 7_000_000, 7_000_000, 1),            # length 0
                          (2, LENS[2] - 100, LENS[2] + 50, 1), (2, LENS[2] - 100, LENS[2] + 7, 1), (2, LENS[2] - 100, LENS[2], 1)]))  # one length after clamping
    inv = _events([(0, 8_000_000 + 1000 * i, 8_000_000 + 1000 * i - 40, 1 + (i & 1)) for i in range(30)])       # end before start
    cover = inv.copy()                                               # (a fragment over each inverted one: no pileup below zero)
    cover["start"], cover["end"], cover["count"] = inv["end"] - 10, inv["start"] + 10, 1
    parts += [inv, cover]
    parts.append(_repeat(0, 10_000_000, 10_000_180, list(R.VALID_COUNTS), 24))   # all eight count classes
    for c in (3, 4, 5):                                              # skipped, outside the save mask, not owned: never counted
        parts.append(_repeat(c, 500_000, 500_200, [1], 500))
        far = synth.make_fragments([LENS6[c]], 2000, 70 + c)
        far["chrom"] = c
        parts.append(far)
    ev = np.concatenate(parts)
    ev = ev[rng.permutation(len(ev))]
    uniform = _repeat(2, 3_000_000, 3_000_190, [10], 70_000)         # one (L, w): more than a chunk, more than a batch
    mixed = _repeat(2, 4_000_000, 4_000_190, [10], 70_000)           # the same with two alternating lengths
    mixed["end"][1::2] += 40
    return np.concatenate([ev, uniform, mixed])


@pytest.fixture(scope="module")
def planted():
    ev = _planted()
    keep, dropped = filter_saturation(ev, LENS6)
    assert dropped == 0 and 280_000 < len(ev) < 330_000
    exp = R.of_events(ev, LENS6, ACTIVE6)
    bound = interval_stats_geometry()[2]
    by = {L: (n, w) for L, n, w in exp.lengths}
    assert by[bound - 1] == (5, 600) and by[bound] == (5, 3 * 120 + 2 * 60) and by[bound + 1] == (5, 600) and by[70_000] == (3, 360)
    assert by[0] == (3, 280) and by[100][0] >= 3 and exp.n_inverted == 30 and exp.w120_inverted == 15 * 120 + 15 * 60
    assert by[190][0] >= 105_000 and by[230][0] >= 35_000 and by[180][1] >= 3 * sum(120 // c for c in R.VALID_COUNTS)
    assert exp.cn[3:] == [0, 0, 0] and min(exp.cn[:3]) > 0 and R.invariants(exp)
    return ev, exp


def _stats(got):
    return R.Stats(*got[:6])


def _hook(lens=LENS6, skip=SKIP6, owned=OWNED6):
    import genrich_amd
    h = genrich_amd.Genrich(B.make_params(pq=0.01, min_auc=20.0))
    h.set_chroms(lens, skip)
    if owned is not None:
        h.set_owned(owned)
    return h


# ---- planted events ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_planted_events_in_every_push_mode(planted, mode):
    """The LDS bound's edges (one with two counts), a length that cannot travel packed, length 0, three ends that clamp to one
    length, inverted intervals, all eight count classes, 70,000 copies of one (L, w) and 70,000 of two alternating lengths, a
    skipped chromosome, one outside the save mask, one not owned."""
    ev, exp = planted
    h, mem = _run6(ev, mode)
    assert h.interval_stats() == 1
    got = h.get_interval_stats(0)
    assert _stats(got) == exp and (got.rep, got.is_ctrl) == (0, False)
    assert h.path_info() & GX_PATH_IVSTAT
    assert h.interval_stats() == 1 and h.get_interval_stats(0) == got            # again: the same
    h.close()
    mem.free()


def test_geometry_and_list_capacity_through_the_hook(planted):
    ev, _ = planted
    h = _hook()
    lib, ctx = h.lib, h.ctx
    args = (None, None, None, 0, None, None, None, None, None, None, 0)
    assert lib.gx_interval_stats_events(ctx, ev.ctypes.data, len(ev), 1 << 16, 0, *args) == ORDER
    assert "65535" in lib.gx_last_error(ctx).decode()
    assert not h.path_info() & GX_PATH_IVSTAT and h.interval_stats_last() == (0, 0)        # refused before any launch
    allev = np.concatenate([ev, _hook_events(3000, 9)])     # with the kinds a sample refuses mixed in
    exp = R.of_events(allev, LENS6, HOOK_ACTIVE6)
    assert R.invariants(exp) and exp.cn[4] > 0 and exp.cn[3] == exp.cn[5] == 0
    cap0 = interval_stats_geometry()[4]
    for grid in (1, 3, 0):
        assert _stats(h.interval_stats_events(allev, grid)) == exp, grid
        assert h.interval_stats_last() == (cap0, 0)
    assert _stats(h.interval_stats_events(allev, 0, 1)) == exp
    cap, reruns = h.interval_stats_last()
    assert reruns == 1 and 1 < cap <= 5 + 5 + 5 + 3 + 64          # the counted size: at most one entry per long interval
    assert _stats(h.interval_stats_events(allev, 3, cap)) == exp and h.interval_stats_last() == (cap, 0)
    for n in (0, 1, 63, 64, 65, (1 << 16) - 1, (1 << 16) + 1):
        small = _hook_events(n, 100 + n)
        want = R.of_events(small, LENS6, HOOK_ACTIVE6)
        for grid in (1, 3, 0):
            assert _stats(h.interval_stats_events(small, grid)) == want, (n, grid)
    assert h.path_info() & GX_PATH_IVSTAT
    h.reset()
    assert not h.path_info() & GX_PATH_IVSTAT
    h.close()


def test_chromosomes_beyond_the_lds_window():
    win = interval_stats_geometry()[3]
    lens = [1000] * (win + 3)
    rows = []
    for k, c in enumerate((0, win - 1, win, win + 1, win + 2)):
        rows += [(c, 10 + i, 10 + i + 50 * (k + 1), (1, 2, 3)[i % 3]) for i in range(40 + k)]
        rows += [(c, 900, 1100, 1), (c, 500, 400, 2)]               # a clamped end, an inverted interval
    rng = np.random.default_rng(5)
    ev = _events(rows)
    ev = ev[rng.permutation(len(ev))]
    exp = R.of_events(ev, lens)
    assert R.invariants(exp) and exp.cn[win + 2] == 46 and exp.n_inverted == 5
    h = _hook(lens=lens, skip=None, owned=None)
    for grid in (1, 0):
        assert _stats(h.interval_stats_events(ev, grid)) == exp
    whole = np.concatenate([ev] + [_repeat(c, 100, 300, [1], 5000) for c in (win - 1, win + 1)])     # whole wavefronts on one chromosome
    assert _stats(h.interval_stats_events(whole)) == R.of_events(whole, lens)
    h.close()


def test_a_treatment_a_control_and_a_sample_without_events():
    import genrich_amd
    lens = [2_000_000]
    ev = synth.make_fragments(lens, 50_000, 13, peak_every=20_000)
    h = genrich_amd.Genrich(B.make_params(pq=0.01, min_auc=20.0))
    h.set_chroms(lens)
    h.set_count_in_peaks(True)
    assert _stats(h.interval_stats_events(ev[:0])) == R.of_events(ev[:0], lens)
    h.sample_begin(0, None)
    h.push_events(ev)
    h.sample_end()
    h.sample_begin(1, None)                                          # a control without events
    h.sample_end()
    assert h.interval_stats() == 2
    t, c = h.get_interval_stats(0), h.get_interval_stats(1)
    assert _stats(t) == R.of_events(ev, lens) and (t.rep, t.is_ctrl) == (0, False)
    assert _stats(c) == R.of_events(ev[:0], lens) == R.Stats([], 0, 0, [0], [0], [0]) and (c.rep, c.is_ctrl) == (0, True)
    lt, mt, ct = interval_stats_text([h], ["chrZ"])
    samples = [(g.rep, g.is_ctrl, _stats(g)) for g in (t, c)]
    assert lt.decode() == R.lengths_text(samples) and mt.decode() == R.metrics_text(samples) and ct.decode() == R.chrom_text(["chrZ"], lens, samples)
    assert "c0\t0\t0\tNA\tNA\t0" in mt.decode()
    h.close()
    h = genrich_amd.Genrich(B.make_params(pq=0.01, min_auc=20.0))    # a control with events, then a second replicate without one
    h.set_chroms(lens)
    h.set_count_in_peaks(True)
    for is_ctrl, part in ((0, ev[:30_000]), (1, ev[30_000:])):
        h.sample_begin(is_ctrl, None)
        h.push_events(part)
        h.sample_end()
    h.pvalues()
    h.sample_begin(0, None)
    h.push_events(ev[10_000:])
    h.sample_end()
    assert h.interval_stats() == 3
    got = [h.get_interval_stats(i) for i in range(3)]
    assert [(g.rep, g.is_ctrl) for g in got] == [(0, False), (0, True), (1, False)]
    assert [_stats(g) for g in got] == [R.of_events(x, lens) for x in (ev[:30_000], ev[30_000:], ev[10_000:])]
    h.close()


def test_two_contexts_add_up():
    rng = np.random.default_rng(41)
    ev = synth.make_fragments(LENS, 150_000, 49, peak_every=20_000, tower_every=3_000_000)
    ev["count"] = rng.choice(R.VALID_COUNTS, len(ev))
    whole = R.of_events(ev, LENS)
    hs = []
    for owned in ([1, 0, 1], [0, 1, 0]):
        h = _run3(ev, owned)
        assert h.interval_stats() == 1
        assert _stats(h.get_interval_stats(0)) == R.of_events(ev, LENS, owned)
        hs.append(h)
    got = interval_stats_group(hs, 0)
    assert _stats(got) == whole == R.add([_stats(h.get_interval_stats(0)) for h in hs]) and (got.rep, got.is_ctrl) == (0, False)
    one = _run3(ev, [1, 1, 1])
    assert one.interval_stats() == 1 and _stats(one.get_interval_stats(0)) == whole
    names = ["chrA", "chrB", "chrC"]
    sample = [(0, False, whole)]
    for ctxs in (hs, [one]):
        lt, mt, ct = interval_stats_text(ctxs, names, cuts=(100, 200))
        assert lt.decode() == R.lengths_text(sample) and mt.decode() == R.metrics_text(sample, (100, 200)) and ct.decode() == R.chrom_text(names, LENS, sample)
    fresh = _hook()                                                   # a context without a result
    assert hs[0].lib.gx_interval_stats_group((C.c_void_p * 2)(hs[0].ctx, fresh.ctx), 2, 0, *([None] * 5), 0, *([None] * 6), 0) == ORDER
    for h in hs + [one, fresh]:
        h.close()


def test_the_tally_is_the_integral_of_the_pileup():
    """Without -E regions and inverted intervals, cbases120[c] is the sum of the sample's --coverage bins of chromosome c."""
    rng = np.random.default_rng(3)
    ev = synth.make_fragments(LENS, 200_000, 17, peak_every=20_000, tower_every=3_000_000)
    ev["count"] = rng.choice([1, 1, 1, 2, 3, 5, 10], len(ev))
    ev = np.concatenate([ev, _events([(2, LENS[2] - 100, LENS[2] + 50, 1), (0, 5000, 5000, 1)])])
    h, mem = _run6(ev, coverage=1000)
    assert h.interval_stats() == 1
    got = h.get_interval_stats(0)
    assert got.n_inverted == 0 and _stats(got) == R.of_events(ev, LENS6, ACTIVE6)
    for c in range(3):
        assert int(h.coverage(0, c).sum120.astype(object).sum()) == got.cbases120[c] > 0
    h.close()
    mem.free()


def test_order_rules_and_what_survives():
    import genrich_amd
    lens = [2_000_000]
    ev = synth.make_fragments(lens, 50_000, 13, peak_every=20_000)
    h = genrich_amd.Genrich(B.make_params(pq=0.01, min_auc=20.0))
    h.set_chroms(lens)
    lib, ctx = h.lib, h.ctx
    n = C.c_int(0)
    err = lambda: lib.gx_last_error(ctx).decode()
    assert lib.gx_interval_stats(ctx, C.byref(n)) == ORDER and "gx_set_count_in_peaks" in err()       # counting off
    h.set_count_in_peaks(True)
    assert lib.gx_interval_stats(ctx, C.byref(n)) == ORDER and "no closed sample" in err()
    h.sample_begin(0, None)
    assert lib.gx_interval_stats(ctx, C.byref(n)) == ORDER and "a sample is open" in err()
    assert lib.gx_interval_stats_events(ctx, ev.ctypes.data, 10, 0, 0, None, None, None, 0, None, None, None, None, None, None, 0) == ORDER
    assert "a sample is open" in err()
    h.push_events(ev)
    h.sample_end()
    assert lib.gx_get_interval_lengths(ctx, 0, None, None, None, None, None, 0, None, None, None) == ORDER    # no pass yet
    assert lib.gx_get_chrom_stats(ctx, 0, None, None, None, 0) == ORDER
    assert not h.path_info() & GX_PATH_IVSTAT
    h.sample_no_control()
    h.pvalues()
    h.find_peaks()
    assert h.count_in_peaks() == 1 and h.complexity() == 1
    pk, cpx = h.peak_counts(0), h.get_complexity(0)
    assert h.interval_stats() == 1
    first = h.get_interval_stats(0)
    assert _stats(first) == R.of_events(ev, lens)
    again, cpx2 = h.peak_counts(0), h.get_complexity(0)                     # the earlier results stay readable
    assert np.array_equal(pk.count, again.count) and pk[1:] == again[1:] and cpx2 == cpx
    flags = h.path_info()
    assert flags & GX_PATH_IVSTAT and flags & GX_PATH_COMPLEXITY
    assert lib.gx_get_interval_lengths(ctx, 1, None, None, None, None, None, 0, None, None, None) == ORDER    # no such sample
    assert lib.gx_get_interval_lengths(ctx, -1, None, None, None, None, None, 0, None, None, None) == ORDER
    nc = C.c_size_t(0)
    assert lib.gx_get_interval_lengths(ctx, 0, None, None, None, None, None, 0, C.byref(nc), None, None) == 0 and nc.value == len(first.lengths)
    a = [np.zeros(2, dtype=np.uint64) for _ in range(3)]                       # cap < n_classes: the first one
    assert lib.gx_get_interval_lengths(ctx, 0, None, None, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, 1, None, None, None) == 0
    assert (int(a[0][0]), int(a[1][0]), int(a[2][0]), int(a[0][1])) == first.lengths[0] + (0,)
    h.reset()
    assert lib.gx_get_interval_lengths(ctx, 0, None, None, None, None, None, 0, None, None, None) == ORDER    # gx_reset drops the result
    assert lib.gx_interval_stats(ctx, C.byref(n)) == ORDER and "no closed sample" in err()
    assert not h.path_info() & GX_PATH_IVSTAT
    h.close()


# ---- the reference's own intervals, through the command line -------------------------------------------------------------

def _golden_samples(name):
    """[(rep, is_ctrl, Stats)] from the fixture's events.bed alone, in run order."""
    meta, case, params, names = G.load_case(name)
    per = R.of_bed_rows(G.read_gz(name, "events.bed").decode().splitlines(), names, case["lens"])
    out = []
    for r, rep in enumerate(case["replicates"]):
        for ctrl in ([False, True] if rep["ctrl"] is not None else [False]):
            out.append((r, ctrl, per.get((r, ctrl), R.of_intervals([], len(names)))))
    return out, meta, names, case["lens"]


@pytest.mark.parametrize("name", FIXTURES)
def test_cli_lengths_of_the_golden_fixtures(name):
    samples, meta, names, lens = _golden_samples(name)
    assert all(R.invariants(st) for _, _, st in samples)
    _, args, tmp, _ = _cli_inputs(name)
    atac = "-j" in meta["args"]
    exp = (R.lengths_text(samples, atac), R.metrics_text(samples), R.chrom_text(names, lens, samples))
    assert exp[0].startswith("# an interval is a cut-site window of -j") == atac
    for tag, extra in (("len", []), ("len2", ["--devices", "0,0"])):     # one context; two contexts on one GPU: the same bytes
        out = os.path.join(tmp, tag + "_out")
        res = subprocess.run([_binary(), "-v", "-o", out + ".narrowPeak", "--lengths", out + ".tsv", "--lengths-metrics", out + ".met",
                              "--chrom-stats", out + ".chr"] + extra + args, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        assert (open(out + ".tsv").read(), open(out + ".met").read(), open(out + ".chr").read()) == exp
        if "-X" not in meta["args"]:
            assert open(out + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")
        lines = [l for l in res.stderr.splitlines() if l.startswith("  Interval lengths")]
        assert len(lines) == len(samples)
        for l, (r, c, st) in zip(lines, samples):
            m = R.metrics(st.lengths)
            assert f"{'control' if c else 'experimental'} file #{r}: {m['n']} intervals, median {m['median']}, mode {m['mode']};" in l, l
            assert ("(cut-site windows)" in l) == atac


def test_cli_alone_gzip_and_the_refusals():
    import gzip
    name = "reps3_p_missing"
    samples, meta, names, lens = _golden_samples(name)
    _, args, tmp, _ = _cli_inputs(name)
    out = os.path.join(tmp, "lenz_out")
    res = subprocess.run([_binary(), "-z", "-X", "-f", out + ".log", "--chrom-stats", out + ".chr"] + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert gzip.open(out + ".chr.gz", "rb").read().decode() == R.chrom_text(names, lens, samples) and not os.path.exists(out + ".tsv")
    res = subprocess.run([_binary(), "-o", out + ".np", "--lengths-metrics", out + ".met", "--lengths-cuts", "100,147,1000"] + args,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert open(out + ".met").read() == R.metrics_text(samples, (100, 147, 1000))
    msg = "--lengths, --lengths-metrics and --chrom-stats need the intervals of this run (not with -P or --events-only)"
    for extra in (["--events-only", "-b", out + ".bed"], ["-P", "-f", out + ".log"]):
        res = subprocess.run([_binary(), "-o", out + ".np2", "--lengths", out + ".no"] + extra + args, capture_output=True, text=True)
        assert res.returncode == 1 and msg in res.stderr and not os.path.exists(out + ".no")
