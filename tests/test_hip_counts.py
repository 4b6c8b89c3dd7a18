"""Each sample's intervals counted in the called peaks on the GPU (gx_count_in_peaks, genrich-amd --counts): against the
reference's own -b interval lists and narrowPeak files of the golden fixtures, and against numpy (tests/counts_ref.py) on
synthetic runs of a few million intervals, in every push mode."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import backends as B
import counts_ref as R
import golden_cases as G
from genrich_amd import synth
from genrich_amd.lib import GX_PATH_COUNTS, pack_events, filter_saturation
from test_host_cli import _binary, _cases, _write_inputs

pytestmark = pytest.mark.gpu

LENS = [24_000_000, 16_000_000, 6_000_000]
ORDER = -10


def _hip():
    # (memory from the HIP runtime the library runs on: a second runtime in the process -- torch's -- sees no GPU)
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipHostFree.argtypes = [C.c_void_p]
    return hip


class Mem:
    """Device / pinned copies of event arrays, freed after the run's last count."""

    def __init__(self):
        self.hip = _hip()
        self.dev, self.pin = [], []

    def device(self, a):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(16, a.nbytes)) == 0
        assert self.hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        self.dev.append(p)
        return p.value

    def pinned(self, a):
        p = C.c_void_p()
        assert self.hip.hipHostMalloc(C.byref(p), max(16, a.nbytes), 0) == 0
        C.memmove(p, a.ctypes.data, a.nbytes)
        self.pin.append(p)
        return p.value

    def free(self):
        for p in self.dev:
            assert self.hip.hipFree(p) == 0
        for p in self.pin:
            assert self.hip.hipHostFree(p) == 0


def _push(h, ev, mode, mem):
    if mode == "host":
        h.push_events(ev)
    elif mode == "pinned":
        h.push_events_ptr(mem.pinned(np.ascontiguousarray(ev)), len(ev), pinned=True)
    elif mode == "device":
        h.push_events_device(mem.device(np.ascontiguousarray(ev)), len(ev))
    else:   # packed_host / packed_pinned / packed_device: 8-byte events, the rest (long ones) as gx_event
        p8, rest = pack_events(ev)
        where = mode.split("_")[1]
        if where == "host":
            h.push_events_packed(p8)
        else:
            h.push_events_packed(mem.pinned(p8) if where == "pinned" else mem.device(p8), where=1 if where == "pinned" else 2, n=len(p8))
        if len(rest):
            h.push_events(rest)


def _run(params, lens, reps, mode="host", count=True, skip=None, owned=None, h=None, frac=False):
    """reps = [(treat events, ctrl events | None)] -> the context after find_peaks (and count_in_peaks)."""
    import genrich_amd
    mem = Mem()
    if h is None:
        h = genrich_amd.Genrich(params)
        h.set_chroms(lens, skip)
        if owned is not None:
            h.set_owned(owned)
    if frac:
        h.expect_fractional(True)
    if count:
        h.set_count_in_peaks(True)
    for t, c in reps:
        h.sample_begin(0, None)
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
    n = h.count_in_peaks() if count else 0
    return h, n, mem


def _expected(h, lens, samples, active=None):
    """numpy counts of each sample's events (ends clamped, inactive chromosomes left out) in the context's own peaks."""
    pk = h.get_peaks()
    lens = np.asarray(lens, dtype=np.int64)
    out = []
    for ev in samples:
        ch = ev["chrom"].astype(np.int64)
        keep = np.ones(len(ev), bool) if active is None else np.asarray(active, bool)[ch]
        ev, ch = ev[keep], ch[keep]
        e = np.minimum(ev["end"].astype(np.int64), lens[ch])
        out.append(R.count_in_peaks(ch, ev["start"], e, R.weights(ev["count"]), pk["chrom"], pk["start"], pk["end"]))
    return out


def _check(h, n, exp):
    assert n == len(exp)
    for i, (cnt, tot, inp) in enumerate(exp):
        got = h.peak_counts(i)
        assert got.total == tot and got.in_peaks == inp, (i, got.total, tot, got.in_peaks, inp)
        assert np.array_equal(got.count, cnt), i
    return [h.peak_counts(i) for i in range(n)]


def _long_events(rng, n):
    """16-byte events: 65,536 bases or more (several peaks each), a few reaching a chromosome's end."""
    ev = np.zeros(n, dtype=B.EVENT_DTYPE)
    ev["chrom"] = rng.integers(0, len(LENS), n)
    ln = rng.integers(65_536, 400_000, n)
    ev["start"] = rng.integers(0, np.asarray(LENS)[ev["chrom"]] - 1)
    ev["end"] = np.minimum(ev["start"].astype(np.int64) + ln, np.asarray(LENS)[ev["chrom"]] + (np.arange(n) % 7 == 0) * 50)
    ev["count"] = 1
    return ev


# ---- the reference's own intervals and peaks ----------------------------------------------------------------------------

def _golden_cases():
    return [n for n in G.case_names() if G.read_gz(n, "out.narrowPeak") is not None and G.read_gz(n, "events.bed") is not None]


def _golden_peaks(name, names):
    idx = {n: i for i, n in enumerate(names)}
    rows = [l.split("\t") for l in G.read_gz(name, "out.narrowPeak").decode().splitlines()]
    return [(idx[r[0]], int(r[1]), int(r[2])) for r in rows]


def _golden_expected(name):
    """(sample (rep, is_ctrl) list, counts per sample) from events.bed and out.narrowPeak alone."""
    meta, case, params, names = G.load_case(name)
    pk = _golden_peaks(name, names)
    pc, ps, pe = (np.array([p[i] for p in pk], dtype=np.int64) for i in range(3))
    idx = {n: i for i, n in enumerate(names)}
    rows = {}
    for line in G.read_gz(name, "events.bed").decode().splitlines():
        c, s, e, nm = line.split("\t")
        _, cnt, kind, smp = nm.rsplit("_", 3)
        rows.setdefault((int(smp), kind == "C"), []).append((idx[c], int(s), int(e), int(cnt)))
    samples = []
    for r, rep in enumerate(case["replicates"]):
        samples.append((r, False))
        if rep["ctrl"] is not None:
            samples.append((r, True))
    exp = []
    for key in samples:
        a = np.array(rows.get(key, []), dtype=np.int64).reshape(-1, 4)
        exp.append(R.count_in_peaks(a[:, 0], a[:, 1], a[:, 2], R.weights(a[:, 3]) if len(a) else a[:, 3], pc, ps, pe))
    return meta, case, params, names, pk, samples, exp


@pytest.mark.parametrize("name", _golden_cases())
def test_golden_counts_from_the_reference_files(name):
    import genrich_amd
    meta, case, params, names, pk, samples, exp = _golden_expected(name)
    h = genrich_amd.Genrich(params)
    h.set_count_in_peaks(True)
    B.run_case(h, case)
    got_pk = h.get_peaks()
    assert [(int(p["chrom"]), int(p["start"]), int(p["end"])) for p in got_pk] == pk
    n = h.count_in_peaks()
    assert n == len(samples)
    for i, ((r, c), (cnt, tot, inp)) in enumerate(zip(samples, exp)):
        got = h.peak_counts(i)
        assert (got.rep, got.is_ctrl) == (r, c)
        assert (got.total, got.in_peaks) == (tot, inp), (i, got.total, tot, got.in_peaks, inp)
        assert np.array_equal(got.count, cnt), i
    assert h.path_info() & GX_PATH_COUNTS
    h.close()


# ---- synthetic runs of a few million intervals --------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["host", "pinned", "device", "packed_host", "packed_pinned", "packed_device", "mixed"])
def test_every_push_mode(mode):
    rng = np.random.default_rng(11)
    ev = synth.make_fragments(LENS, 2_000_000, 3, peak_every=20_000, tower_every=3_000_000)
    if mode == "mixed":
        ev = np.concatenate([ev, _long_events(rng, 3000)])
        ev = ev[rng.permutation(len(ev))]
    h, n, mem = _run(B.make_params(pq=0.01, min_auc=20.0), LENS, [(ev, None)], mode="packed_device" if mode == "mixed" else mode)
    assert h.n_peaks > 1000
    got = _check(h, n, _expected(h, LENS, [ev]))
    assert 0 < got[0].in_peaks < got[0].total
    if mode == "mixed":
        assert _check(h, h.count_in_peaks(), _expected(h, LENS, [ev]))   # again: the same
    h.close()
    mem.free()


def test_fractional_weights():
    ev = synth.make_fragments(LENS, 1_500_000, 5, peak_every=20_000, tower_every=3_000_000)
    ev = synth.add_multimap(ev, LENS, 0.1, 6)
    assert (ev["count"] > 1).any()
    h, n, mem = _run(B.make_params(pq=0.01, min_auc=20.0), LENS, [(ev, None)], mode="packed_host", frac=True)
    got = _check(h, n, _expected(h, LENS, [ev]))
    assert got[0].total % 120 != 0 or got[0].in_peaks % 120 != 0 or (got[0].count % 120 != 0).any()
    h.close()


def test_atac_towers():
    ev = synth.make_fragments(LENS, 1_500_000, 7, peak_every=20_000, tower_every=200_000, frac_tower=0.2)
    cut = synth.atac_events(ev, LENS)
    h, n, mem = _run(B.make_params(pq=0.01, min_auc=20.0), LENS, [(cut, None)], mode="packed_device")
    got = _check(h, n, _expected(h, LENS, [cut]))
    assert got[0].count.max() >= 120 * 1000   # one peak hit by many intervals
    h.close()
    mem.free()


def test_control_and_q():
    t = synth.make_fragments(LENS, 1_500_000, 9, peak_every=20_000, tower_every=3_000_000)
    c = synth.make_fragments(LENS, 1_500_000, 10, uniform_only=True)
    h, n, mem = _run(B.make_params(pq=0.05, qval=True, min_auc=20.0), LENS, [(t, c)])
    assert h.n_peaks > 0
    got = _check(h, n, _expected(h, LENS, [t, c]))
    assert [(g.rep, g.is_ctrl) for g in got] == [(0, False), (0, True)]
    h.close()


def test_three_replicates_with_a_missing_control():
    ts = [synth.make_fragments(LENS, 700_000, 20 + r, peak_every=20_000, tower_every=3_000_000) for r in range(3)]
    cs = [synth.make_fragments(LENS, 500_000, 30 + r, uniform_only=True) for r in range(3)]
    reps = [(ts[0], cs[0]), (ts[1], None), (ts[2], cs[2])]
    h, n, mem = _run(B.make_params(pq=0.05, qval=True, min_auc=20.0), LENS, reps, mode="packed_pinned")
    got = _check(h, n, _expected(h, LENS, [ts[0], cs[0], ts[1], ts[2], cs[2]]))
    assert [(g.rep, g.is_ctrl) for g in got] == [(0, False), (0, True), (1, False), (2, False), (2, True)]
    h.close()
    mem.free()


def test_int16_saturating_tower():
    lens = [3_000_000, 1_000_000]
    ev = synth.make_fragments(lens, 300_000, 12, peak_every=20_000, tower_every=3_000_000)
    tower = np.zeros(40_000, dtype=B.EVENT_DTYPE)
    tower["chrom"], tower["start"], tower["end"], tower["count"] = 0, 1_000_000, 1_000_180, 1
    ev = np.concatenate([ev[:100_000], tower, ev[100_000:]])
    keep, dropped = filter_saturation(ev, lens)
    assert dropped > 0
    h, n, mem = _run(B.make_params(pq=0.01, min_auc=20.0), lens, [(ev, None)])
    _check(h, n, _expected(h, lens, [ev[keep.astype(bool)]]))
    h.close()


def test_order_errors():
    import genrich_amd
    lens = [2_000_000]
    ev = synth.make_fragments(lens, 100_000, 13, peak_every=20_000)
    h = genrich_amd.Genrich(B.make_params(pq=0.01, min_auc=20.0))
    h.set_chroms(lens)
    lib, ctx = h.lib, h.ctx
    n = C.c_int(0)
    assert lib.gx_count_in_peaks(ctx, C.byref(n)) == ORDER          # counting off
    h.set_count_in_peaks(True)
    h.sample_begin(0, None)
    assert lib.gx_set_count_in_peaks(ctx, 0) == ORDER              # not idle
    h.push_events(ev)
    h.sample_end()
    assert lib.gx_set_count_in_peaks(ctx, 1) == ORDER
    h.sample_no_control()
    h.pvalues()
    assert lib.gx_count_in_peaks(ctx, C.byref(n)) == ORDER          # before gx_find_peaks
    assert lib.gx_get_peak_counts(ctx, 0, None, None, None, 0, None, None) == ORDER
    h.find_peaks()
    assert lib.gx_get_peak_counts(ctx, 0, None, None, None, 0, None, None) == ORDER   # not counted yet
    assert h.count_in_peaks() == 1
    assert lib.gx_get_peak_counts(ctx, 1, None, None, None, 0, None, None) == ORDER   # no such sample
    h.reset()
    assert lib.gx_count_in_peaks(ctx, C.byref(n)) == ORDER          # gx_reset drops what was kept
    assert not h.path_info() & GX_PATH_COUNTS
    h.close()


def test_two_runs_separated_by_reset():
    import genrich_amd
    a = synth.make_fragments(LENS, 1_000_000, 14, peak_every=20_000, tower_every=3_000_000)
    b = synth.make_fragments(LENS, 1_200_000, 15, peak_every=30_000, tower_every=3_000_000)
    params = B.make_params(pq=0.01, min_auc=20.0)
    h = genrich_amd.Genrich(params)
    h.set_chroms(LENS)
    h, n, mem = _run(params, LENS, [(a, None)], h=h)
    _check(h, n, _expected(h, LENS, [a]))
    h.reset()   # (the switch stays on)
    h, n, mem = _run(params, LENS, [(b, b[:300_000])], h=h, count=False)
    _check(h, h.count_in_peaks(), _expected(h, LENS, [b, b[:300_000]]))
    h.close()


def test_owned_chromosomes_only():
    ev = synth.make_fragments(LENS, 1_000_000, 16, peak_every=20_000, tower_every=3_000_000)
    owned = [1, 0, 1]
    h, n, mem = _run(B.make_params(pq=0.01, min_auc=20.0), LENS, [(ev, None)], owned=owned)
    assert set(h.get_peaks()["chrom"].tolist()) <= {0, 2}
    got = _check(h, n, _expected(h, LENS, [ev], active=owned))
    assert got[0].total == 120 * int(np.isin(ev["chrom"], [0, 2]).sum())
    h.close()


def test_counting_changes_nothing_else():
    ev = synth.make_fragments(LENS, 1_000_000, 17, peak_every=20_000, tower_every=3_000_000)
    params = B.make_params(pq=0.01, min_auc=20.0)
    off, _, _ = _run(params, LENS, [(ev, None)], count=False)
    on, n, _ = _run(params, LENS, [(ev, None)])
    assert off.get_peaks().tobytes() == on.get_peaks().tobytes()
    for c in range(len(LENS)):
        e0, c0 = off.get_intervals(-1, c, piles=False)
        e1, c1 = on.get_intervals(-1, c, piles=False)
        assert np.array_equal(e0, e1) and np.array_equal(c0["p"].view(np.uint32), c1["p"].view(np.uint32))
    f0, f1 = off.path_info(), on.path_info()
    assert not f0 & GX_PATH_COUNTS and f1 == f0 | GX_PATH_COUNTS, (f0, f1)
    off.close()
    on.close()


# ---- the command line -------------------------------------------------------------------------------------------------

def _cli_inputs(name):
    cases, mg = _cases()
    meta, _, _, _ = G.load_case(name)
    tmp = meta["tmp_prefix"].rstrip("/")   # same input paths as when the fixture was made (-k names them)
    args = _write_inputs(cases[name], mg, tmp)
    t = args[args.index("-t") + 1].split(",")
    c = args[args.index("-c") + 1].split(",") if "-c" in args else []
    names = t[:0]
    for r, tf in enumerate(t):
        names.append(tf)
        if r < len(c) and c[r] != "null":
            names.append(c[r])
    return meta, args, tmp, names


def _cli_expected(name, sample_names):
    meta, case, params, names, pk, samples, exp = _golden_expected(name)
    assert len(sample_names) == len(samples)
    return R.counts_text(names, pk, sample_names, [e[0] for e in exp]), samples, exp


@pytest.mark.parametrize("name", [n for n in _golden_cases() if "-X" not in G.load_case(n)[0]["args"]])
def test_cli_counts_and_the_other_outputs(name):
    meta, args, tmp, sample_names = _cli_inputs(name)
    out = os.path.join(tmp, "cnt_out")
    cmd = [_binary(), "-v", "-f", out + ".log", "-k", out + ".pile", "-b", out + ".bed", "-o", out + ".narrowPeak",
           "--counts", out + ".counts"] + args
    if "-r" in args:
        cmd += ["-R", out + ".dups"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert open(out + ".bed", "rb").read() == G.read_gz(name, "events.bed")
    assert open(out + ".pile", "rb").read() == G.read_gz(name, "out.pile")
    assert open(out + ".log", "rb").read() == G.read_gz(name, "out.log")
    assert open(out + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")
    txt, samples, exp = _cli_expected(name, sample_names)
    assert open(out + ".counts").read() == txt
    lines = res.stderr.splitlines()
    frip = [l for l in lines if l.startswith("  Intervals in peaks")]
    assert frip == [R.frip_line(r, c, e[1], e[2]) for (r, c), e in zip(samples, exp)]
    pi = [i for i, l in enumerate(lines) if l.startswith("Peaks identified:")]
    assert pi and lines[pi[-1] + 1] == frip[0]


@pytest.mark.parametrize("name", ["reps3", "ctrl_q"])
def test_cli_counts_gzip_and_two_contexts(name):
    meta, args, tmp, sample_names = _cli_inputs(name)
    txt, _, _ = _cli_expected(name, sample_names)
    out = os.path.join(tmp, "cntz_out")
    res = subprocess.run([_binary(), "-z", "-o", out + ".narrowPeak", "--counts", out + ".counts"] + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert gzip.open(out + ".counts.gz", "rb").read().decode() == txt
    assert gzip.open(out + ".narrowPeak.gz", "rb").read() == G.read_gz(name, "out.narrowPeak")
    out2 = os.path.join(tmp, "cnt2_out")
    res = subprocess.run([_binary(), "--devices", "0,0", "-o", out2 + ".narrowPeak", "--counts", out2 + ".counts"] + args,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert open(out2 + ".counts").read() == txt
    assert open(out2 + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")


def test_cli_counts_refused_with_P_or_X(tmp_path):
    meta, args, tmp, _ = _cli_inputs("basic")
    for extra in (["-X"], ["-P", "-f", os.path.join(tmp, "nonexistent.log")]):
        out = tmp_path / "c.counts"
        res = subprocess.run([_binary(), "-o", str(tmp_path / "o.np"), "--counts", str(out)] + args + extra,
                             capture_output=True, text=True)
        assert res.returncode == 1 and "--counts" in res.stderr, res.stderr
        assert not out.exists() and not (tmp_path / "o.np").exists()
