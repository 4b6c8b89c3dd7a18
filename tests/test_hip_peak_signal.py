"""Each sample's own depth inside the peaks on the GPU (gx_peak_signal, gx_peak_signal_events, genrich-amd --peak-signal):
k_psig_scatter / k_psig_reduce on constructed peaks (tests/peaksig_cases.py) and on runs of a few hundred thousand intervals in
every push mode against numpy (tests/peaksig_ref.py), with ==; one golden fixture through the command line against the
reference's own -b interval lists and narrowPeak file."""
import ctypes as C
import gzip
import os
import subprocess
import threading

import numpy as np
import pytest

import backends as B
import counts_ref as CR
import golden_cases as G
import peaksig_cases as K
import peaksig_ref as R
from genrich_amd import synth
from genrich_amd.lib import pack_events, peak_signal_geometry
from ranks import ThreadAllreduce
from test_hip_counts import Mem, _cli_inputs, _push
from test_host_cli import _binary

pytestmark = pytest.mark.gpu

LENS = [3_000_000, 2_000_000, 1_000_000]
ORDER = -10
STEP = peak_signal_geometry()[2]
MOST = peak_signal_geometry()[4]


def _ctx(lens, skip=None, owned=None, params=None):
    import genrich_amd
    h = genrich_amd.Genrich(params or B.make_params(pq=0.01, min_auc=20.0))
    h.set_chroms(lens, skip)
    if owned is not None:
        h.set_owned(owned)
    return h


# ---- the two kernels on constructed peaks -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def constructed():
    """label -> (lens, peaks, summit offsets, events, the reference's figures): the reference is computed once"""
    return {label: (lens, peaks, so, ev, R.signal(ev, lens, peaks, so)) for label, lens, peaks, so, ev in K.device_cases(STEP)}


@pytest.mark.parametrize("grid", [0, 1])
@pytest.mark.parametrize("label", ["lengths", "edges", "plateaus", "tiny_peaks"])
def test_constructed_peaks(constructed, label, grid):
    lens, peaks, so, ev, exp = constructed[label]
    h = _ctx(lens)
    got = h.peak_signal_events(ev, peaks, so, grid)
    assert R.same(got, exp) is None, R.same(got, exp)
    if label == "lengths":
        L = [e - s for _, s, e in peaks]
        assert L == [1, 3, 4, 5, 63, 64, 65, STEP - 1, STEP, STEP + 1, 3 * STEP + 7, 200_000]
        assert (exp.max > 0).all()
        assert h.peak_signal_events(ev[::-1], peaks, so, grid).area.tolist() == exp.area.tolist()   # the order of the adds
    if label == "tiny_peaks":
        assert len(peaks) == 100_000 and (exp.max > 0).sum() > 10_000 and (exp.max < 0).sum() > 10_000
    h.close()


@pytest.mark.parametrize("grid", [0, 1])
def test_no_peaks_and_no_events(constructed, grid):
    lens, peaks, so, ev, exp = constructed["edges"]
    h = _ctx(lens)
    none = h.peak_signal_events(ev, [], None, grid)
    assert all(len(x) == 0 for x in none[:5])
    got = h.peak_signal_events(ev[:0], peaks, so, grid)
    for f in got[:5]:
        assert not f.any()
    assert R.same(h.peak_signal_events(ev, peaks, so, grid), exp) is None
    h.close()


def test_the_deepest_base_of_the_domain():
    """2^31 / 120 - 1 copies of one interval of weight 120: the final entries fit 31 bits while the sum wraps nowhere; one
    event more is refused by its number alone."""
    n = MOST
    ev = np.zeros(n + 1, dtype=B.EVENT_DTYPE)
    ev["start"], ev["end"], ev["count"] = 100, 103, 1
    h = _ctx([1000])
    got = h.peak_signal_events(ev[:n], [(0, 90, 110), (0, 110, 120)], [11, 0])
    assert got.max.tolist() == [120 * n, 0] and got.summit.tolist() == [10, 0] and got.area.tolist() == [360 * n, 0]
    assert got.covered.tolist() == [3, 0] and got.at_summit.tolist() == [120 * n, 0] and 120 * n < 1 << 31 <= 120 * (n + 2)
    reg = np.zeros(1, dtype=[("chrom", "<u4"), ("start", "<u4"), ("end", "<u4")])
    reg["start"], reg["end"] = 90, 110
    assert h.lib.gx_peak_signal_events(h.ctx, ev.ctypes.data, n + 1, reg.ctypes.data, 1, None, 0, None, None, None, None, None) == ORDER
    assert b"2^31 / 120" in h.lib.gx_last_error(h.ctx)
    h.close()


def test_refusals_of_the_events_call():
    h = _ctx([1000, 500, 300], skip=[0, 0, 1])
    ev = K.events([(0, 5, 50, 1)])
    for bad in ([(0, 100, 200), (0, 50, 80)],            # unsorted
                [(1, 0, 10), (0, 0, 10)],                # chromosomes out of order
                [(0, 100, 200), (0, 199, 300)],          # overlapping
                [(0, 100, 100)],                         # empty
                [(0, 900, 1001)],                        # beyond its chromosome
                [(3, 0, 10)],                            # a chromosome the table does not have
                [(2, 0, 10)]):                           # a skipped chromosome
        with pytest.raises(RuntimeError, match=f"error {ORDER}:"):
            h.peak_signal_events(ev, bad)
    with pytest.raises(RuntimeError, match=f"error {ORDER}:"):
        h.peak_signal_events(ev, [(0, 100, 200)], [100])   # the summit outside its peak
    with pytest.raises(RuntimeError, match=f"error {ORDER}:"):
        h.peak_signal_events(ev, [(0, 100, 200)], None, 1 << 16)
    assert h.peak_signal_events(ev, [(0, 0, 100), (0, 100, 200), (1, 0, 500)]).covered.tolist() == [45, 0, 0]
    h.sample_begin(0, None)
    with pytest.raises(RuntimeError, match=f"error {ORDER}:"):
        h.peak_signal_events(ev, [(0, 0, 100)])            # a sample is open
    h.close()


# ---- runs ---------------------------------------------------------------------------------------------------------------

def _run(lens, reps, mode="host", skip=None, owned=None, frac=False, params=None, saves=None, keep=True):
    """reps = [(treat events, ctrl events | None)] -> the context after find_peaks, and the device / pinned memory it reads"""
    h = _ctx(lens, skip, owned, params)
    mem = Mem()
    if frac:
        h.expect_fractional(True)
    if keep:
        h.set_count_in_peaks(True)
    for r, (t, c) in enumerate(reps):
        h.sample_begin(0, None if saves is None else saves[r])
        _push(h, t, mode, mem)
        h.sample_end()
        if c is not None:
            h.sample_begin(1, None)
            _push(h, c, mode, mem)
            h.sample_end()
        else:
            h.sample_no_control()
        h.pvalues()
    h.find_peaks()
    return h, mem


def _peaks(h):
    pk = h.get_peaks()
    return np.stack([pk["chrom"], pk["start"], pk["end"]], axis=1).astype(np.int64), pk["summit"].astype(np.int64)


def _check(h, lens, samples, active=None):
    """every sample of the context against numpy on the context's own peaks; samples = [(events, rep, is_ctrl, active | None)]"""
    peaks, so = _peaks(h)
    assert h.peak_signal() == len(samples)
    out = []
    for i, (ev, rep, ctrl, act) in enumerate(samples):
        got = h.peak_signal_of(i)
        assert (got.rep, got.is_ctrl) == (rep, ctrl)
        exp = R.signal(ev, lens, peaks, so, act if act is not None else active)
        assert R.same(got, exp) is None, (i, R.same(got, exp))
        out.append(got)
    return out


def _long_events(rng, n):
    """16-byte events: 65,536 bases or more (several peaks each), a few reaching beyond a chromosome's end"""
    ev = np.zeros(n, dtype=B.EVENT_DTYPE)
    ev["chrom"] = rng.integers(0, len(LENS), n)
    ln = rng.integers(65_536, 200_000, n)
    ev["start"] = rng.integers(0, np.asarray(LENS)[ev["chrom"]] - 1)
    ev["end"] = np.minimum(ev["start"].astype(np.int64) + ln, np.asarray(LENS)[ev["chrom"]] + (np.arange(n) % 7 == 0) * 50)
    ev["count"] = 1
    return ev


@pytest.mark.parametrize("n_rep,ctrl", [(1, False), (1, True), (3, False), (3, True)])
def test_replicates_and_controls(n_rep, ctrl):
    ts = [synth.make_fragments(LENS, 250_000, 40 + r, peak_every=20_000, tower_every=3_000_000) for r in range(n_rep)]
    cs = [synth.make_fragments(LENS, 200_000, 50 + r, uniform_only=True) if ctrl and r != 1 else None for r in range(n_rep)]
    h, mem = _run(LENS, list(zip(ts, cs)), params=B.make_params(pq=0.05, qval=ctrl, min_auc=20.0))
    assert h.n_peaks > (2 if ctrl else 20)               # (-q against a control leaves a few peaks of a run this small)
    samples = []
    for r in range(n_rep):
        samples.append((ts[r], r, False, None))
        if cs[r] is not None:
            samples.append((cs[r], r, True, None))
    got = _check(h, LENS, samples)
    assert (got[0].max > 0).all() and (got[0].covered > 0).all()
    h.close()
    mem.free()


@pytest.mark.parametrize("mode", ["host", "pinned", "device", "packed_host", "packed_pinned", "packed_device"])
def test_every_push_mode(mode):
    rng = np.random.default_rng(21)
    ev = synth.make_fragments(LENS, 300_000, 3, peak_every=20_000, tower_every=3_000_000)
    ev = synth.add_multimap(ev, LENS, 0.1, 6)
    ev = np.concatenate([ev, _long_events(rng, 400)])
    ev = ev[rng.permutation(len(ev))]
    if mode.startswith("packed"):
        p8, rest = pack_events(ev)
        assert len(p8) and len(rest)                        # 8-byte events, and 16-byte ones for the long
    h, mem = _run(LENS, [(ev, None)], mode=mode, frac=True)
    assert h.n_peaks > 20
    got = _check(h, LENS, [(ev, 0, False, None)])
    assert (got[0].max % 120 != 0).any() and (got[0].area % 120 != 0).any()
    h.close()
    mem.free()


def test_a_skipped_and_an_unsaved_chromosome():
    t = synth.make_fragments(LENS, 300_000, 60, peak_every=20_000, tower_every=3_000_000)
    c = synth.make_fragments(LENS, 200_000, 61, uniform_only=True)
    h, mem = _run(LENS, [(t, c)], skip=[0, 1, 0], saves=[[1, 1, 0]])
    assert h.n_peaks > 5 and set(h.get_peaks()["chrom"].tolist()) == {0}
    _check(h, LENS, [(t, 0, False, [1, 0, 0]), (c, 0, True, [1, 0, 0])])
    h.close()


def test_owned_split_over_two_contexts():
    ev = synth.make_fragments(LENS, 300_000, 62, peak_every=20_000, tower_every=3_000_000)
    one, _ = _run(LENS, [(ev, None)])
    whole = _check(one, LENS, [(ev, 0, False, None)])[0]
    owns = [[1, 0, 1], [0, 1, 0]]
    coll = ThreadAllreduce(2)
    parts, errors = [None, None], []

    def rank(r):
        try:
            h = _ctx(LENS, owned=owns[r])
            h.set_collectives(r, 2, coll.callback(r))
            h.set_count_in_peaks(True)
            h.sample_begin(0, None)
            h.push_events(ev)
            h.sample_end()
            h.sample_no_control()
            h.pvalues()
            h.find_peaks()
            assert set(h.get_peaks()["chrom"].tolist()) <= {c for c in range(3) if owns[r][c]}
            parts[r] = (_peaks(h)[0], _check(h, LENS, [(ev, 0, False, owns[r])])[0])
            h.close()
        except BaseException as e:
            errors.append(e)
            coll.bar.abort()

    threads = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    pk = np.concatenate([p for p, _ in parts])
    order = np.lexsort((pk[:, 1], pk[:, 0]))
    assert len(parts[0][0]) and len(parts[1][0]) and np.array_equal(pk[order], _peaks(one)[0])
    for f in ("area", "max", "summit", "covered", "at_summit"):
        assert np.array_equal(np.concatenate([getattr(sg, f) for _, sg in parts])[order], getattr(whole, f)), f
    one.close()


def test_again_next_to_the_counts_and_after_reset():
    ev = synth.make_fragments(LENS, 300_000, 63, peak_every=20_000, tower_every=3_000_000)
    h, _ = _run(LENS, [(ev, ev[:100_000])], keep=False)
    lib, ctx = h.lib, h.ctx
    n = C.c_int(0)
    assert lib.gx_peak_signal(ctx, C.byref(n)) == ORDER                    # the intervals were not kept
    assert lib.gx_get_peak_signal(ctx, 0, None, None, None, None, None, None, None, 0) == ORDER
    h.close()
    h, _ = _run(LENS, [(ev, ev[:100_000])])
    lib, ctx = h.lib, h.ctx
    h.set_phase_timing(2)
    assert lib.gx_get_peak_signal(ctx, 0, None, None, None, None, None, None, None, 0) == ORDER   # not taken yet
    assert h.count_in_peaks() == 2
    regions = _peaks(h)[0][::3]
    assert h.count_in_regions(regions) == 2
    counts = [(h.peak_counts(i), h.region_counts(i)) for i in range(2)]
    assert "peaksig" not in [name for name, _ in h.phase_times()]          # nothing of it ran so far
    first = _check(h, LENS, [(ev, 0, False, None), (ev[:100_000], 0, True, None)])
    assert [name for name, _ in h.phase_times()].count("peaksig") == 1
    again = _check(h, LENS, [(ev, 0, False, None), (ev[:100_000], 0, True, None)])
    for a, b in zip(first, again):
        assert R.same(a, b) is None
    for i, (pc, rc) in enumerate(counts):                                  # both counts are still what they were
        a, b = h.peak_counts(i), h.region_counts(i)
        assert np.array_equal(a.count, pc.count) and (a.total, a.in_peaks) == (pc.total, pc.in_peaks)
        assert np.array_equal(b.count, rc.count) and (b.total, b.in_regions) == (rc.total, rc.in_regions)
        exp = CR.count_in_peaks(*[(ev if i == 0 else ev[:100_000])[f].astype(np.int64) for f in ("chrom", "start", "end")],
                                CR.weights((ev if i == 0 else ev[:100_000])["count"]), *[h.get_peaks()[f] for f in ("chrom", "start", "end")])
        assert np.array_equal(a.count, exp[0])
    assert lib.gx_get_peak_signal(ctx, 2, None, None, None, None, None, None, None, 0) == ORDER   # no such sample
    h.reset()
    assert lib.gx_peak_signal(ctx, C.byref(n)) == ORDER
    assert lib.gx_get_peak_signal(ctx, 0, None, None, None, None, None, None, None, 0) == ORDER
    h.close()


def test_against_the_pileup_of_the_run():
    """One replicate, whole weights, no -E: the sample's depth IS the treatment pileup gx_get_intervals reports."""
    ev = synth.make_fragments(LENS, 300_000, 64, peak_every=20_000, tower_every=3_000_000)
    h, _ = _run(LENS, [(ev, None)])
    peaks, so = _peaks(h)
    assert h.peak_signal() == 1 and len(peaks) > 20
    got = h.peak_signal_of(0)
    for c in range(len(LENS)):
        end, cols = h.get_intervals(0, c)
        start = np.concatenate([[0], end[:-1]]).astype(np.int64)
        for k in np.flatnonzero(peaks[:, 0] == c):
            ps, pe = peaks[k, 1], peaks[k, 2]
            inside = (start < pe) & (end.astype(np.int64) > ps)
            assert got.max[k] == 120 * int(cols["expt"][inside].max()) and got.max[k] % 120 == 0
            at = int(np.searchsorted(end, ps + so[k], side="right"))
            assert got.at_summit[k] == 120 * int(cols["expt"][at])
    h.close()


# ---- the command line -------------------------------------------------------------------------------------------------

def _golden_text(name):
    """--peak-signal's text from events.bed and out.narrowPeak alone"""
    meta, case, params, names = G.load_case(name)
    idx = {n: i for i, n in enumerate(names)}
    rows = [l.split("\t") for l in G.read_gz(name, "out.narrowPeak").decode().splitlines()]
    peaks = [(idx[r[0]], int(r[1]), int(r[2])) for r in rows]
    so = [int(r[9]) for r in rows]
    by = {}
    for line in G.read_gz(name, "events.bed").decode().splitlines():
        c, s, e, nm = line.split("\t")
        _, cnt, kind, smp = nm.rsplit("_", 3)
        by.setdefault((int(smp), kind == "C"), []).append((idx[c], int(s), int(e), int(cnt)))
    samples = []
    for r, rep in enumerate(case["replicates"]):
        samples.append(R.signal(K.events(by.get((r, False), [])), case["lens"], peaks, so, rep=r, is_ctrl=False))
        if rep["ctrl"] is not None:
            samples.append(R.signal(K.events(by.get((r, True), [])), case["lens"], peaks, so, rep=r, is_ctrl=True))
    return R.peak_signal_text(names, peaks, samples), samples


def test_cli_on_a_golden_fixture_and_two_contexts():
    name = "reps3"                                        # three replicates, two of them with a control
    meta, args, tmp, _ = _cli_inputs(name)
    txt, samples = _golden_text(name)
    assert len(samples) == 5 and txt.count("\n") > 5
    out = os.path.join(tmp, "sig_out")
    res = subprocess.run([_binary(), "-v", "-o", out + ".narrowPeak", "--peak-signal", out + ".sig", "--counts", out + ".counts"] + args,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert open(out + ".sig").read() == txt
    assert open(out + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")
    lines = [l for l in res.stderr.splitlines() if l.startswith("  Signal in peaks")]
    so = [int(l.split("\t")[9]) for l in G.read_gz(name, "out.narrowPeak").decode().splitlines()]
    assert lines == [f"  Signal in peaks, {'control' if s.is_ctrl else 'experimental'} file #{s.rep}: no depth in {int((s.max == 0).sum())} of "
                     f"{len(so)} peaks, summit shared in {int((s.summit == np.asarray(so)).sum())}" for s in samples]
    out2 = os.path.join(tmp, "sig2_out")
    res = subprocess.run([_binary(), "-z", "--devices", "0,0", "-o", out2 + ".narrowPeak", "--peak-signal", out2 + ".sig"] + args,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert gzip.open(out2 + ".sig.gz", "rb").read().decode() == txt
    assert gzip.open(out2 + ".narrowPeak.gz", "rb").read() == G.read_gz(name, "out.narrowPeak")
