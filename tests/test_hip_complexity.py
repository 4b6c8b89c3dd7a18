"""Library complexity of each sample's intervals on the GPU (gx_complexity, genrich-amd --complexity): against the reference's
own -b interval lists of the golden fixtures through the command line, and against collections.Counter (tests/complexity_ref.py)
on planted synthetic events in every push mode, launch geometry and table capacity.

A sample that is built rejects an event with an invalid count, an unknown chromosome or a start beyond an active chromosome
(gx_sample_end fails on it, as the reference does), so those three kinds reach the kernels through gx_complexity_events only;
everything else of the planted set goes through real samples as well."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import backends as B
import complexity_ref as R
import golden_cases as G
from genrich_amd import synth
from genrich_amd.lib import GX_PATH_COMPLEXITY, complexity_geometry, complexity_group, complexity_text, filter_saturation
from test_hip_counts import LENS, Mem, _cli_inputs, _push
from test_host_cli import _binary

pytestmark = pytest.mark.gpu

ORDER = -10
MODES = ["host", "pinned", "device", "packed_host", "packed_pinned", "packed_device"]
# chromosomes 0-2 as everywhere; 3 is skipped (-e), 4 is outside the sample's save mask, 5 is not owned by the context
LENS6 = LENS + [1_000_000, 1_000_000, 1_000_000]
SKIP6, SAVE6, OWNED6 = [0, 0, 0, 1, 0, 0], [1, 1, 1, 1, 0, 1], [1, 1, 1, 1, 1, 0]
ACTIVE6 = [1, 1, 1, 0, 0, 0]


def _events(rows):
    ev = np.zeros(len(rows), dtype=B.EVENT_DTYPE)
    if len(rows):
        a = np.asarray(rows, dtype=np.int64)
        ev["chrom"], ev["start"], ev["end"], ev["count"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    return ev


def _repeat(chrom, start, end, counts, times):
    ev = np.zeros(times, dtype=B.EVENT_DTYPE)
    ev["chrom"], ev["start"], ev["end"] = chrom, start, end
    ev["count"] = np.resize(np.asarray(counts), times)
    return ev


def _planted():
    """About 300,000 events a sample takes: see the module's list in test_planted_events_in_every_push_mode."""
    bound = complexity_geometry()[2]
    rng = np.random.default_rng(31)
    parts = [synth.make_fragments(LENS, 200_000, 61, peak_every=20_000, tower_every=3_000_000)]
    parts.append(_repeat(0, 1_000_000, 1_000_200, [1], 2))
    parts.append(_repeat(0, 1_010_000, 1_010_200, [1], 3))
    for i, m in enumerate((bound - 1, bound, bound + 1)):           # the LDS histogram's last class, the list's first two
        parts.append(_repeat(1, 2_000_000 + 50_000 * i, 2_000_150 + 50_000 * i, [2], m))
    parts.append(_repeat(2, 3_000_000, 3_000_190, [10, 5], 70_000))  # more than one chunk; two counts, one key; no int16 saturation
    parts.append(_events([(0, 5_000_000, 5_000_100, 1), (1, 5_000_000, 5_000_100, 1),        # the same (start, end) on two chromosomes
                          (0, 6_000_000, 6_000_100, 1), (0, 6_000_000, 6_000_101, 1),        # the same start with two ends
                          (2, LENS[2] - 100, LENS[2] + 50, 1), (2, LENS[2] - 100, LENS[2] + 7, 1), (2, LENS[2] - 100, LENS[2], 1),   # one key after clamping
                          (0, 7_000_000, 7_000_000, 1), (0, 7_000_000, 7_000_000, 3), (1, 7_000_000, 7_000_000, 1)]))              # empty intervals
    inv = _events([(0, 8_000_000 + 1000 * i, 8_000_000 + 1000 * i - 40, 1) for i in range(30)] * 2)     # end before start, each twice
    cover = inv.copy()                                               # (a fragment over each inverted one: no pileup below zero)
    cover["start"], cover["end"] = inv["end"] - 10, inv["start"] + 10
    parts += [inv, cover]
    for c in (3, 4, 5):                                              # skipped, outside the save mask, not owned: never counted
        parts.append(_repeat(c, 500_000, 500_200, [1], 500))
        far = synth.make_fragments([LENS6[c]], 2000, 70 + c)
        far["chrom"] = c
        parts.append(far)
    ev = np.concatenate(parts)
    return ev[rng.permutation(len(ev))]


@pytest.fixture(scope="module")
def planted():
    ev = _planted()
    keep, dropped = filter_saturation(ev, LENS6)
    assert dropped == 0 and 280_000 < len(ev) < 330_000
    exp = R.of_events(ev, LENS6, ACTIVE6)
    bound = complexity_geometry()[2]
    h = dict(exp[2])
    assert h[bound - 1] == h[bound] == h[bound + 1] == h[70_000] == 1 and h[3] >= 2 and h[2] >= 30 and max(h) == 70_000
    return ev, exp


def _run6(ev, mode="host", owned=OWNED6, count=True, coverage=0):
    """One treatment sample of `ev` over LENS6, closed; no p-values, no peaks."""
    import genrich_amd
    mem = Mem()
    h = genrich_amd.Genrich(B.make_params(pq=0.01, min_auc=20.0))
    h.set_chroms(LENS6, SKIP6)
    h.set_owned(owned)
    h.expect_fractional(True)
    if coverage:
        h.set_coverage_bins(coverage)
    if count:
        h.set_count_in_peaks(True)
    h.sample_begin(0, SAVE6)
    _push(h, ev, mode, mem)
    h.sample_end()
    return h, mem


def _result(c):
    return (c.n_obs, c.n_distinct, c.pairs)


# ---- the reference's own intervals, through the command line -------------------------------------------------------------

# a control (-q); -r -y -s; ATAC -j; unpaired -y; -r on pairs; -e; three replicates with a missing chromosome
FIXTURES = ["ctrl_q", "dups_y", "atac", "unpaired_y", "dups_pairs", "bedx", "reps3_p_missing"]


def _golden_samples(name):
    """[(rep, is_ctrl, N, D, pairs)] from the fixture's events.bed alone, in run order."""
    meta, case, params, names = G.load_case(name)
    rows = {}
    for line in G.read_gz(name, "events.bed").decode().splitlines():
        c, s, e, nm = line.split("\t")
        _, cnt, kind, smp = nm.rsplit("_", 3)
        rows.setdefault((int(smp), kind == "C"), []).append((c, int(s), int(e)))
    out = []
    for r, rep in enumerate(case["replicates"]):
        for ctrl in ([False, True] if rep["ctrl"] is not None else [False]):
            out.append((r, ctrl) + R.histogram(rows.get((r, ctrl), [])))
    return out, meta


def test_the_fixtures_cover_what_they_are_chosen_for():
    args = {n: G.load_case(n)[0]["args"] for n in FIXTURES}
    assert "-j" in args["atac"] and "-y" in args["unpaired_y"] and "-e" in args["bedx"] and "-r" in args["dups_pairs"]
    assert {"-r", "-y", "-s"} <= set(args["dups_y"])
    assert [s[:2] for s in _golden_samples("ctrl_q")[0]] == [(0, False), (0, True)]
    assert len(_golden_samples("reps3_p_missing")[0]) == 3
    assert any(m > 1 for s in _golden_samples("atac")[0] for m, _ in s[4])     # the fixtures do hold repeated keys


@pytest.mark.parametrize("name", FIXTURES)
def test_cli_complexity_of_the_golden_fixtures(name):
    samples, meta = _golden_samples(name)
    _, args, tmp, _ = _cli_inputs(name)
    out = os.path.join(tmp, "cpx_out")
    res = subprocess.run([_binary(), "-v", "-o", out + ".narrowPeak", "--complexity", out + ".tsv", "--complexity-hist", out + ".hist"] + args,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    text, hist = open(out + ".tsv").read(), open(out + ".hist").read()
    assert hist == R.hist_text(samples)
    assert R.check_metrics(text, samples) is None, R.check_metrics(text, samples)
    if "-X" not in meta["args"]:
        assert open(out + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")
    lines = [l for l in res.stderr.splitlines() if l.startswith("  Library complexity")]
    assert len(lines) == len(samples)
    for l, (r, c, N, D, pairs) in zip(lines, samples):
        assert l.startswith(R.verbose_prefix(r, c, N, D)), l
    # two contexts on one GPU: the same bytes
    out2 = os.path.join(tmp, "cpx2_out")
    res = subprocess.run([_binary(), "--devices", "0,0", "-o", out2 + ".narrowPeak", "--complexity", out2 + ".tsv", "--complexity-hist",
                          out2 + ".hist"] + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert open(out2 + ".tsv").read() == text and open(out2 + ".hist").read() == hist


def test_cli_gzip_without_peaks_and_next_to_counts():
    name = "reps3_p_missing"
    samples, meta = _golden_samples(name)
    _, args, tmp, _ = _cli_inputs(name)
    out = os.path.join(tmp, "cpxz_out")
    res = subprocess.run([_binary(), "-z", "-X", "-f", out + ".log", "--complexity", out + ".tsv"] + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert R.check_metrics(gzip.open(out + ".tsv.gz", "rb").read().decode(), samples) is None
    plain = os.path.join(tmp, "cpxc_out")
    for extra in ([], ["--complexity", plain + ".tsv", "--complexity-hist", plain + ".hist"]):
        res = subprocess.run([_binary(), "-o", plain + ".narrowPeak", "--counts", plain + ".counts" + str(len(extra))] + extra + args,
                             capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
    assert open(plain + ".counts0", "rb").read() == open(plain + ".counts4", "rb").read()
    assert open(plain + ".hist").read() == R.hist_text(samples)


# ---- planted events ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_planted_events_in_every_push_mode(planted, mode):
    """Multiplicities 1, 2, 3 and the LDS bound's edges, one key 70,000 times (more than one chunk), the same (start, end) on two
    chromosomes, the same start with two ends, the same coordinates with different counts, three ends that clamp to one, empty
    intervals, intervals that end before they start, a skipped chromosome, one outside the save mask, one not owned."""
    ev, exp = planted
    h, mem = _run6(ev, mode)
    assert h.complexity() == 1
    got = h.get_complexity(0)
    assert _result(got) == exp and (got.rep, got.is_ctrl) == (0, False)
    assert h.path_info() & GX_PATH_COMPLEXITY
    assert h.complexity_last() == complexity_geometry(len(ev))[3]
    h.close()
    mem.free()


def _hook_events(n, seed, distinct=False):
    """n events for gx_complexity_events: every kind a sample takes, and those it refuses (an invalid count, an unknown chromosome,
    a start at or beyond the chromosome's length); `distinct`: n different legal keys."""
    rng = np.random.default_rng(seed)
    ev = np.zeros(n, dtype=B.EVENT_DTYPE)
    if distinct:
        ev["chrom"], ev["start"], ev["count"] = 0, 1000 + 3 * np.arange(n), 1
        ev["end"] = ev["start"] + 100
        return ev
    pool = max(1, n // 3)                                          # (few places: most keys repeat)
    ev["chrom"] = rng.integers(0, len(LENS6) + 1, n)               # (one beyond the table)
    ln = np.asarray(LENS6 + [1 << 20])[ev["chrom"]]
    ev["start"] = (ln - 40) + rng.integers(0, pool, n) % 60        # around the chromosome's end: some start at or beyond it
    ev["end"] = ev["start"] + rng.integers(0, 3, n) * 30           # empty ones; ends that clamp
    ev["count"] = rng.choice([1, 2, 3, 4, 5, 6, 8, 10, 0, 7, 9, 11, 200], n)
    return ev


def test_geometry_and_capacity_through_the_hook(planted):
    import genrich_amd
    h = genrich_amd.Genrich(B.make_params(pq=0.01, min_auc=20.0))
    h.set_chroms(LENS6, SKIP6)
    h.set_owned(OWNED6)
    active = [1, 1, 1, 0, 1, 0]            # (the hook's sample lists every chromosome in its save mask; -e and ownership hold)
    lib, ctx = h.lib, h.ctx
    big = _hook_events(1 << 16, 5, distinct=True)
    least = complexity_geometry(len(big))[3].bit_length() - 1
    assert 1 << least == 2 * len(big)
    assert lib.gx_complexity_events(ctx, big.ctypes.data, len(big), 0, least - 1, None, None, None, None, 0, None) == ORDER
    assert "2 n slots" in lib.gx_last_error(ctx).decode()
    assert lib.gx_complexity_events(ctx, big.ctypes.data, len(big), 1 << 16, 0, None, None, None, None, 0, None) == ORDER
    assert not h.path_info() & GX_PATH_COMPLEXITY and h.complexity_last() == 0      # refused before any launch
    cases = [(_hook_events(n, 100 + n), n) for n in (0, 1, 63, 64, 65, (1 << 16) - 1, (1 << 16) + 1)]
    cases += [(_hook_events(64, 1, distinct=True), 64), (big, len(big))]            # the table exactly half full at the least capacity
    for ev, n in cases:
        exp = R.of_events(ev, LENS6, active)
        least = complexity_geometry(n)[3].bit_length() - 1
        for grid in (1, 3, 0):
            for cap_log in (least, least + 4):
                assert h.complexity_events(ev, grid, cap_log) == exp, (n, grid, cap_log)
                assert h.complexity_last() == (1 << cap_log if n else h.complexity_last())
        assert h.complexity_events(ev) == exp
    assert h.complexity_events(big)[:2] == (len(big), len(big))
    assert h.path_info() & GX_PATH_COMPLEXITY
    ev, exp = planted                       # the planted set with the kinds a sample refuses mixed in
    bad = _hook_events(3000, 9)
    allev = np.concatenate([ev, bad])
    assert h.complexity_events(allev, 3) == R.of_events(allev, LENS6, active) == h.complexity_events(allev, 0, 22)
    h.reset()
    assert not h.path_info() & GX_PATH_COMPLEXITY
    h.close()


def _run3(ev, owned):
    """One treatment sample of `ev` over LENS in a context that owns some of the chromosomes, closed."""
    import genrich_amd
    h = genrich_amd.Genrich(B.make_params(pq=0.01, min_auc=20.0))
    h.set_chroms(LENS)
    h.set_owned(owned)
    h.set_count_in_peaks(True)
    h.sample_begin(0, None)
    h.push_events(ev)
    h.sample_end()
    return h


def test_two_contexts_add_up():
    rng = np.random.default_rng(41)
    ev = synth.make_fragments(LENS, 150_000, 49, peak_every=20_000, tower_every=3_000_000)
    ev[rng.choice(len(ev), 30_000, replace=False)] = ev[rng.integers(0, len(ev), 30_000)]     # a fifth are copies of others
    whole = R.of_events(ev, LENS)
    assert whole[1] < whole[0] and len(whole[2]) > 2
    hs = []
    for owned in ([1, 0, 1], [0, 1, 0]):
        h = _run3(ev, owned)
        assert h.complexity() == 1
        assert _result(h.get_complexity(0)) == R.of_events(ev, LENS, owned)
        hs.append(h)
    got = complexity_group(hs, 0)
    assert _result(got) == whole == R.add([_result(h.get_complexity(0)) for h in hs]) and (got.rep, got.is_ctrl) == (0, False)
    met, hist = complexity_text(hs)
    sample = [(0, False) + whole]
    assert hist.decode() == R.hist_text(sample) and R.check_metrics(met.decode(), sample) is None
    for h in hs:
        h.close()


def test_order_rules():
    import genrich_amd
    lens = [2_000_000]
    ev = synth.make_fragments(lens, 50_000, 13, peak_every=20_000)
    h = genrich_amd.Genrich(B.make_params(pq=0.01, min_auc=20.0))
    h.set_chroms(lens)
    lib, ctx = h.lib, h.ctx
    n = C.c_int(0)
    err = lambda: lib.gx_last_error(ctx).decode()
    assert lib.gx_complexity(ctx, C.byref(n)) == ORDER and "gx_set_count_in_peaks" in err()       # counting off
    h.set_count_in_peaks(True)
    assert lib.gx_complexity(ctx, C.byref(n)) == ORDER and "no closed sample" in err()
    h.sample_begin(0, None)
    assert lib.gx_complexity(ctx, C.byref(n)) == ORDER and "a sample is open" in err()
    assert lib.gx_complexity_events(ctx, ev.ctypes.data, 10, 0, 0, None, None, None, None, 0, None) == ORDER and "a sample is open" in err()
    h.push_events(ev)
    h.sample_end()
    assert lib.gx_get_complexity(ctx, 0, None, None, None, None, None, None, 0, None) == ORDER    # no pass yet
    assert not h.path_info() & GX_PATH_COMPLEXITY
    assert h.complexity() == 1
    first = h.get_complexity(0)
    assert _result(first) == R.of_events(ev, lens)
    assert lib.gx_get_complexity(ctx, 1, None, None, None, None, None, None, 0, None) == ORDER    # no such sample
    assert lib.gx_get_complexity(ctx, -1, None, None, None, None, None, None, 0, None) == ORDER
    nc = C.c_size_t(0)
    assert lib.gx_get_complexity(ctx, 0, None, None, None, None, None, None, 0, C.byref(nc)) == 0 and nc.value == len(first.pairs)
    m2, k2 = np.zeros(2, dtype=np.uint64), np.zeros(2, dtype=np.uint64)                           # cap < n_classes: the first two
    assert lib.gx_get_complexity(ctx, 0, None, None, None, None, m2.ctypes.data, k2.ctypes.data, 1, None) == 0
    assert (int(m2[0]), int(k2[0]), int(m2[1])) == (first.pairs[0][0], first.pairs[0][1], 0)
    assert h.complexity() == 1 and h.get_complexity(0) == first                                   # again: the same
    h.sample_begin(1, None)                                                                       # a control: a second sample
    h.push_events(ev[:20_000])
    assert lib.gx_complexity(ctx, C.byref(n)) == ORDER and "a sample is open" in err()
    h.sample_end()
    assert h.complexity() == 2
    assert h.get_complexity(0) == first
    second = h.get_complexity(1)
    assert _result(second) == R.of_events(ev[:20_000], lens) and (second.rep, second.is_ctrl) == (0, True)
    h.pvalues()
    h.find_peaks()
    h.reset()
    assert lib.gx_get_complexity(ctx, 0, None, None, None, None, None, None, 0, None) == ORDER    # gx_reset drops the result
    assert lib.gx_complexity(ctx, C.byref(n)) == ORDER and "no closed sample" in err()            # ... and the samples
    assert not h.path_info() & GX_PATH_COMPLEXITY
    h.close()


def test_complexity_changes_nothing_else():
    ev = synth.make_fragments(LENS, 300_000, 17, peak_every=20_000, tower_every=3_000_000)
    reg = np.zeros(200, dtype=[("chrom", "<u4"), ("start", "<u4"), ("end", "<u4")])
    reg["chrom"], reg["start"] = np.arange(200) % 3, 10_000 * np.arange(200)
    reg["end"] = reg["start"] + 30_000
    runs = []
    for with_cpx in (False, True):
        h, mem = _run6(ev, coverage=1000)
        assert h.count_in_regions(reg) == 1
        before = h.region_counts(0)
        if with_cpx:
            assert h.complexity() == 1 and _result(h.get_complexity(0)) == R.of_events(ev, LENS6, ACTIVE6)
            after = h.region_counts(0)                      # the last gx_count_in_regions result stays readable
            assert np.array_equal(before.count, after.count) and before[1:] == after[1:]
        h.sample_no_control()
        h.pvalues()
        h.find_peaks()
        assert h.count_in_peaks() == 1
        pk = h.peak_counts(0)
        if with_cpx:
            assert h.complexity() == 1                      # after the peaks as well
            again = h.peak_counts(0)
            assert np.array_equal(pk.count, again.count) and pk[1:] == again[1:]
        runs.append((h, pk, before))
    (off, pk0, rg0), (on, pk1, rg1) = runs
    assert len(off.get_peaks()) > 50 and off.get_peaks().tobytes() == on.get_peaks().tobytes()
    assert np.array_equal(pk0.count, pk1.count) and pk0[1:] == pk1[1:] and np.array_equal(rg0.count, rg1.count) and rg0[1:] == rg1[1:]
    for c in range(3):
        assert np.array_equal(off.coverage(0, c).sum120, on.coverage(0, c).sum120)
    f0, f1 = off.path_info(), on.path_info()
    assert not f0 & GX_PATH_COMPLEXITY and f1 == f0 | GX_PATH_COMPLEXITY, (f0, f1)
    off.close()
    on.close()
