"""Each sample's intervals counted in a given region set on the GPU (gx_count_in_regions, genrich-amd --count-regions): region
sets that overlap, nest, repeat and come unsorted, against numpy (tests/regions_ref.py) on synthetic runs in every push mode,
against gx_count_in_peaks when the regions are the called peaks, and the command line on the golden fixtures."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import backends as B
import golden_cases as G
import regions_ref as R
from genrich_amd import synth
from genrich_amd.lib import GX_PATH_COUNTS, GX_PATH_REGION_COUNTS, REGION_DTYPE, pack_events
from test_host_cli import _binary, _cases, _write_inputs

pytestmark = pytest.mark.gpu

LENS = [3_000_000, 1_000_000, 500_000]
ORDER = -10
TILE = 4096              # gx_kernels.h TILE: the grain of the regions' tile index
CNT_LDS_MAX = 36_864     # gx_count.h: histogram entries one launch keeps in LDS; a set of n live regions has 2 (n + 1)
REG_WIN_MAX = 1          # gx_regions.h: LDS windows per sample; more entries than that go to global atomics
REG_INV_CAP = 1 << 14    # gx_regions.h: inverted intervals one pass lists before it has to run again


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


def _run(params, lens, reps, mode="host", count=True, skip=None, owned=None, frac=False, peaks=True):
    """reps = [(treat events, ctrl events | None)] -> the context after find_peaks (peaks=False: after the last sample_end /
    sample_no_control, with no pvalues and no find_peaks at all)."""
    import genrich_amd
    mem = Mem()
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
        elif peaks:
            h.sample_no_control()
        if peaks:
            h.pvalues()
    if peaks:
        h.find_peaks()
    return h, mem


def _expected(reg, lens, samples, active=None):
    """numpy counts of each sample's events (ends clamped, inactive chromosomes left out) in the regions as given."""
    lens = np.asarray(lens, dtype=np.int64)
    out = []
    for ev in samples:
        ch = ev["chrom"].astype(np.int64)
        keep = np.ones(len(ev), bool) if active is None else np.asarray(active, bool)[ch]
        ev, ch = ev[keep], ch[keep]
        e = np.minimum(ev["end"].astype(np.int64), lens[ch])
        out.append(R.count_in_regions(ch, ev["start"], e, R.weights(ev["count"]), reg["chrom"], reg["start"], reg["end"]))
    return out


def _check(h, n, exp):
    assert n == len(exp)
    for i, (cnt, tot, inr) in enumerate(exp):
        got = h.region_counts(i)
        assert got.total == tot and got.in_regions == inr, (i, got.total, tot, got.in_regions, inr)
        bad = np.flatnonzero(got.count != cnt)
        assert not len(bad), (i, len(bad), bad[:5], got.count[bad[:5]], cnt[bad[:5]])
    return [h.region_counts(i) for i in range(n)]


def _regions(rows):
    reg = np.zeros(len(rows), dtype=REGION_DTYPE)
    a = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    reg["chrom"], reg["start"], reg["end"] = a[:, 0], a[:, 1], a[:, 2]
    return reg


def _random_regions(rng, lens, n, chroms=None, short=False):
    """n regions on `chroms` (default: all), chromosome in proportion to its length, lengths from 1 base to 100 kb: they
    overlap and nest by themselves (short: up to 2 kb, so that about half of the genome lies in no region)."""
    lens = np.asarray(lens, dtype=np.int64)
    chroms = np.arange(len(lens)) if chroms is None else np.asarray(chroms)
    c = chroms[np.searchsorted(np.cumsum(lens[chroms]), rng.integers(0, lens[chroms].sum(), n), "right")]
    s = rng.integers(0, lens[c])
    ln = rng.choice([1, 40, 300, 2_000, 20_000, 100_000], n, p=[0.05, 0.25, 0.45, 0.25, 0, 0] if short else [0.05, 0.2, 0.4, 0.2, 0.1, 0.05])
    return _regions(np.stack([c, s, np.minimum(s + ln, lens[c])], axis=1))


def _all_kinds(rng, lens, skip, n):
    """About n regions of every kind the definition names; -> (regions in a shuffled order, {kind: row indices})."""
    lens = np.asarray(lens, dtype=np.int64)
    known = [c for c in range(len(lens)) if not skip[c]]
    parts, labels = [_random_regions(rng, lens, n, known, short=True)], [np.full(n, "random")]

    def add(kind, rows):
        parts.append(_regions(rows))
        labels.append(np.full(len(rows), kind))

    base = parts[0]
    k = rng.integers(0, n, 200)
    add("duplicate", [(base["chrom"][i], base["start"][i], base["end"][i]) for i in k])
    k = np.flatnonzero(base["end"] - base["start"] >= 300)[:200]
    add("nested", [(base["chrom"][i], base["start"][i] + 100, base["end"][i] - 100) for i in k])
    c = rng.choice(known, 100)
    s = rng.integers(0, lens[c])
    add("one_base", np.stack([c, s, s + 1], axis=1))
    add("whole", [(c, 0, lens[c]) for c in known[1:]])   # (not the first: some intervals shall lie in no region)
    t = rng.integers(1, lens[c] // TILE) * TILE
    add("straddle", np.stack([c, t - rng.integers(1, 300, 100), t + rng.integers(1, 300, 100)], axis=1))
    add("on_border", np.concatenate([np.stack([c, t, t + rng.integers(1, 5000, 100)], axis=1),
                                     np.stack([c, t - rng.integers(1, 4000, 100), t], axis=1)]))
    add("beyond", np.stack([c, lens[c] - rng.integers(1, 5000, 100), lens[c] + rng.integers(1, 10_000, 100)], axis=1))
    add("unknown", [(len(lens) + i % 3, 1000 * i, 1000 * i + 500) for i in range(50)] + [(0xFFFFFFFF, 0, 10)])
    sk = [c for c in range(len(lens)) if skip[c]]
    add("skipped", [(sk[0], 1000 * i, 1000 * i + 700) for i in range(50)])
    add("past", np.stack([c, lens[c] + rng.integers(0, 1000, 100), lens[c] + 5000], axis=1))
    reg, lab = np.concatenate(parts), np.concatenate(labels)
    p = rng.permutation(len(reg))
    reg, lab = reg[p], lab[p]
    return reg, {kind: np.flatnonzero(lab == kind) for kind in np.unique(lab)}


# ---- region sets of every kind ------------------------------------------------------------------------------------------------

def test_random_overlapping_regions():
    rng = np.random.default_rng(1)
    lens, skip = LENS + [200_000], [0, 0, 0, 1]
    L = np.asarray(lens, dtype=np.int64)
    ev = synth.make_fragments(lens, 300_000, 41, peak_every=20_000, tower_every=3_000_000)
    reg, kinds = _all_kinds(rng, lens, skip, 4000)
    # the set really holds each kind
    c, s, e = (reg[f].astype(np.int64) for f in ("chrom", "start", "end"))
    assert 4500 < len(reg) < 5500 and (s < e).all()
    assert len(reg) - len(np.unique(reg)) >= 100                                     # exact duplicates
    o = np.lexsort((s, c))
    assert ((c[o][1:] == c[o][:-1]) & (s[o][1:] < e[o][:-1])).sum() > 1000          # overlapping neighbours
    assert (np.diff(np.lexsort((s, c))) < 0).any()                                  # unsorted
    for k in kinds["nested"][:20]:
        assert ((c == c[k]) & (s < s[k]) & (e[k] < e)).any()
    assert len(kinds["one_base"]) and (e[kinds["one_base"]] - s[kinds["one_base"]] == 1).all()
    k = kinds["whole"]
    assert len(k) == 2 and (s[k] == 0).all() and (e[k] == L[c[k]]).all()
    k = kinds["straddle"]
    assert len(k) and (s[k] // TILE != (e[k] - 1) // TILE).all()
    k = kinds["on_border"]
    assert (s[k] % TILE == 0).any() and (e[k] % TILE == 0).any()
    k = kinds["beyond"]
    assert len(k) and (e[k] > L[c[k]]).all() and (s[k] < L[c[k]]).all()
    assert (c[kinds["unknown"]] >= len(lens)).all() and len(kinds["unknown"]) > 3
    assert (c[kinds["skipped"]] == 3).all() and len(kinds["skipped"])
    k = kinds["past"]
    assert len(k) and (s[k] >= L[c[k]]).all()

    h, mem = _run(B.make_params(pq=0.01, min_auc=20.0), lens, [(ev, None)], skip=skip)
    n = h.count_in_regions(reg)
    got = _check(h, n, _expected(reg, lens, [ev], active=[1, 1, 1, 0]))[0]
    assert 0 < got.in_regions < got.total
    for k in kinds["whole"]:
        assert got.count[k] == 120 * int((ev["chrom"] == c[k]).sum()) > 0
    for kind in ("unknown", "skipped", "past"):
        assert not got.count[kinds[kind]].any()
    assert got.count[kinds["beyond"]].any() and got.count[kinds["one_base"]].any()
    assert h.path_info() & GX_PATH_REGION_COUNTS
    h.close()
    mem.free()


def test_regions_equal_to_the_called_peaks():
    rng = np.random.default_rng(2)
    ev = synth.make_fragments(LENS, 300_000, 42, peak_every=20_000, tower_every=3_000_000)
    h, mem = _run(B.make_params(pq=0.01, min_auc=20.0), LENS, [(ev, None)], mode="packed_device")
    pk = h.get_peaks()
    assert len(pk) > 100
    assert h.count_in_peaks() == 1
    want = h.peak_counts(0)
    reg = _regions(np.stack([pk["chrom"], pk["start"], pk["end"]], axis=1))
    assert h.count_in_regions(reg) == 1
    got = h.region_counts(0)
    assert got.count.tobytes() == want.count.tobytes() and (got.total, got.in_regions) == (want.total, want.in_peaks)
    assert (got.rep, got.is_ctrl) == (want.rep, want.is_ctrl) == (0, False)
    p = rng.permutation(len(reg))
    assert h.count_in_regions(reg[p]) == 1
    got = h.region_counts(0)
    assert got.count.tobytes() == want.count[p].tobytes() and (got.total, got.in_regions) == (want.total, want.in_peaks)
    # both results stay readable, and a new peak count leaves the regions' alone
    assert h.peak_counts(0).count.tobytes() == want.count.tobytes()
    assert h.count_in_peaks() == 1
    assert h.region_counts(0).count.tobytes() == want.count[p].tobytes()
    assert h.path_info() & GX_PATH_COUNTS and h.path_info() & GX_PATH_REGION_COUNTS
    h.close()
    mem.free()


def test_without_peak_calling_and_twice():
    rng = np.random.default_rng(3)
    ev = synth.make_fragments(LENS, 200_000, 43, peak_every=20_000, tower_every=3_000_000)
    h, mem = _run(B.make_params(pq=0.01, min_auc=20.0), LENS, [(ev, None)], mode="device", peaks=False)
    a, b = _random_regions(rng, LENS, 3000), _random_regions(rng, LENS, 700)
    ea, eb = _expected(a, LENS, [ev]), _expected(b, LENS, [ev])
    _check(h, h.count_in_regions(a), ea)
    _check(h, h.count_in_regions(b), eb)
    _check(h, h.count_in_regions(a), ea)
    h.close()
    mem.free()


@pytest.mark.parametrize("n", [40_000, REG_WIN_MAX * CNT_LDS_MAX // 2 - 1, REG_WIN_MAX * CNT_LDS_MAX // 2])
def test_more_entries_than_one_lds_window(n):
    """40,000 regions: 2 (n + 1) entries > CNT_LDS_MAX.  2 (n + 1) = REG_WIN_MAX * CNT_LDS_MAX is the largest set whose
    histograms stay in LDS, one region more takes global atomics.  Every region is live, so n is the n of the threshold."""
    rng = np.random.default_rng(4)
    assert 2 * (40_000 + 1) > CNT_LDS_MAX
    ev = synth.make_fragments(LENS, 300_000, 44, peak_every=20_000, tower_every=3_000_000)
    reg = _random_regions(rng, LENS, n)
    h, mem = _run(B.make_params(pq=0.01, min_auc=20.0), LENS, [(ev, None)], peaks=False)
    got = _check(h, h.count_in_regions(reg), _expected(reg, LENS, [ev]))[0]
    assert 0 < got.in_regions <= got.total and got.count.any()
    h.close()


@pytest.mark.parametrize("windows,n", [(1000, 40_000), (-1, 3000)])
def test_forced_histogram_placement(windows, n):
    """GX_REG_WINDOWS: 40,000 regions in three LDS windows (a launch each), and a small set by global atomics."""
    rng = np.random.default_rng(11)
    ev = synth.make_fragments(LENS, 300_000, 51, peak_every=20_000, tower_every=3_000_000)
    reg = _random_regions(rng, LENS, n)
    h, mem = _run(B.make_params(pq=0.01, min_auc=20.0), LENS, [(ev, None)], mode="packed_host", peaks=False)
    h.set_knob("GX_REG_WINDOWS", windows)
    _check(h, h.count_in_regions(reg), _expected(reg, LENS, [ev]))
    h.close()


@pytest.mark.parametrize("n_inv", [300, REG_INV_CAP + 3000])
def test_inverted_and_empty_intervals(n_inv):
    """Intervals that end before they start (and empty ones) among the events: inside regions, around one, outside all.  More
    than REG_INV_CAP of them: the pass runs a second time with a longer list."""
    rng = np.random.default_rng(5)
    ev = synth.make_fragments(LENS, 150_000, 45, peak_every=20_000, tower_every=3_000_000)
    reg = _random_regions(rng, LENS, 5000, short=True)
    odd = np.zeros(n_inv + 300, dtype=B.EVENT_DTYPE)
    k = rng.integers(0, len(reg), len(odd))
    mid = (reg["start"][k].astype(np.int64) + reg["end"][k]) // 2
    back = rng.choice([1, 5, 60, 3000], len(odd))            # (s - e: small ones lie inside a region, long ones reach around one)
    odd["chrom"], odd["start"], odd["count"] = reg["chrom"][k], mid, rng.choice([1, 2, 3], len(odd))
    odd["end"] = np.maximum(0, mid - back)
    odd["end"][n_inv:] = odd["start"][n_inv:]                # the last 300: empty
    odd["start"][:20] = reg["end"][k[:20]]                   # s == a region's end: not in it
    odd = odd[odd["start"] < np.asarray(LENS)[odd["chrom"]]]
    assert (odd["end"] < odd["start"]).sum() > 0.9 * n_inv and (odd["end"] == odd["start"]).sum() > 250
    cover = odd[odd["end"] < odd["start"]].copy()            # (a fragment over each inverted one: no pileup below zero)
    cover["start"], cover["end"], cover["count"] = np.maximum(cover["end"], 10) - 10, cover["start"] + 10, 1
    ev = np.concatenate([ev, odd, cover])
    ev = ev[rng.permutation(len(ev))]
    h, mem = _run(B.make_params(pq=0.01, min_auc=20.0), LENS, [(ev, None)], frac=True)
    exp = _expected(reg, LENS, [ev])
    only = _expected(reg, LENS, [odd[odd["end"] < odd["start"]]])[0]
    assert only[0].any() and 0 < only[2] < only[1]           # some inverted intervals count, some do not
    _check(h, h.count_in_regions(reg), exp)
    _check(h, h.count_in_regions(reg), exp)                  # (again: the longer list is kept)
    h.close()


def test_fractional_weights():
    rng = np.random.default_rng(6)
    ev = synth.make_fragments(LENS, 200_000, 46, peak_every=20_000, tower_every=3_000_000)
    ev = synth.add_multimap(ev, LENS, 0.1, 6)
    assert (ev["count"] > 1).any()
    reg = _random_regions(rng, LENS, 5000)
    h, mem = _run(B.make_params(pq=0.01, min_auc=20.0), LENS, [(ev, None)], mode="packed_host", frac=True)
    got = _check(h, h.count_in_regions(reg), _expected(reg, LENS, [ev]))[0]
    assert (got.count % 120 != 0).any()
    h.close()


def test_treatment_and_control():
    rng = np.random.default_rng(7)
    t = synth.make_fragments(LENS, 200_000, 47, peak_every=20_000, tower_every=3_000_000)
    c = synth.make_fragments(LENS, 150_000, 48, uniform_only=True)
    reg = _random_regions(rng, LENS, 5000)
    h, mem = _run(B.make_params(pq=0.05, qval=True, min_auc=20.0), LENS, [(t, c)], mode="pinned")
    got = _check(h, h.count_in_regions(reg), _expected(reg, LENS, [t, c]))
    assert [(g.rep, g.is_ctrl) for g in got] == [(0, False), (0, True)]
    h.close()
    mem.free()


def test_three_replicates_with_a_missing_control():
    rng = np.random.default_rng(8)
    ts = [synth.make_fragments(LENS, 100_000, 50 + r, peak_every=20_000, tower_every=3_000_000) for r in range(3)]
    cs = [synth.make_fragments(LENS, 80_000, 60 + r, uniform_only=True) for r in range(3)]
    reps = [(ts[0], cs[0]), (ts[1], None), (ts[2], cs[2])]
    reg = _random_regions(rng, LENS, 5000)
    h, mem = _run(B.make_params(pq=0.05, qval=True, min_auc=20.0), LENS, reps, mode="packed_pinned")
    got = _check(h, h.count_in_regions(reg), _expected(reg, LENS, [ts[0], cs[0], ts[1], ts[2], cs[2]]))
    assert [(g.rep, g.is_ctrl) for g in got] == [(0, False), (0, True), (1, False), (2, False), (2, True)]
    h.close()
    mem.free()


def test_owned_chromosomes_and_two_contexts():
    rng = np.random.default_rng(9)
    ev = synth.make_fragments(LENS, 200_000, 49, peak_every=20_000, tower_every=3_000_000)
    reg = _random_regions(rng, LENS, 5000)
    whole = _expected(reg, LENS, [ev])[0]
    total = np.zeros(len(reg), dtype=np.int64)
    tot = inr = 0
    for owned in ([1, 0, 1], [0, 1, 0]):
        h, mem = _run(B.make_params(pq=0.01, min_auc=20.0), LENS, [(ev, None)], owned=owned, peaks=False)
        got = _check(h, h.count_in_regions(reg), _expected(reg, LENS, [ev], active=owned))[0]
        assert got.total == 120 * int(np.asarray(owned, bool)[ev["chrom"]].sum())
        assert not got.count[~np.asarray(owned, bool)[reg["chrom"]]].any()
        total += got.count
        tot += got.total
        inr += got.in_regions
        h.close()
    assert np.array_equal(total, whole[0]) and (tot, inr) == whole[1:]


def test_order_errors():
    import genrich_amd
    lens = [2_000_000]
    ev = synth.make_fragments(lens, 50_000, 13, peak_every=20_000)
    reg = _regions([(0, 100, 5000), (0, 1000, 1_000_000)])
    h = genrich_amd.Genrich(B.make_params(pq=0.01, min_auc=20.0))
    h.set_chroms(lens)
    lib, ctx = h.lib, h.ctx
    n = C.c_int(0)
    assert lib.gx_count_in_regions(ctx, reg.ctypes.data, len(reg), C.byref(n)) == ORDER      # the switch is off
    h.set_count_in_peaks(True)
    h.sample_begin(0, None)
    assert lib.gx_count_in_regions(ctx, reg.ctypes.data, len(reg), C.byref(n)) == ORDER      # a sample is open
    h.push_events(ev)
    h.sample_end()
    assert lib.gx_get_region_counts(ctx, 0, None, None, None, 0, None, None) == ORDER        # not counted yet
    for bad in ([(0, 100, 5000), (0, 700, 700)], [(0, 900, 100)]):
        b = _regions(bad)
        assert lib.gx_count_in_regions(ctx, b.ctypes.data, len(b), C.byref(n)) == ORDER      # start >= end
        assert lib.gx_get_region_counts(ctx, 0, None, None, None, 0, None, None) == ORDER    # ... and nothing was counted
    assert h.count_in_regions(reg) == 1
    assert lib.gx_get_region_counts(ctx, 1, None, None, None, 0, None, None) == ORDER        # no such sample
    assert lib.gx_get_region_counts(ctx, -1, None, None, None, 0, None, None) == ORDER
    assert h.region_counts(0).total == 120 * len(ev)
    h.sample_no_control()
    h.pvalues()
    h.find_peaks()
    h.reset()
    assert lib.gx_get_region_counts(ctx, 0, None, None, None, 0, None, None) == ORDER        # gx_reset drops the result
    assert not h.path_info() & GX_PATH_REGION_COUNTS
    assert h.count_in_regions(reg) == 0                                                      # ... and the samples
    h.close()


def test_no_regions():
    ev = synth.make_fragments(LENS, 50_000, 14, peak_every=20_000)
    h, mem = _run(B.make_params(pq=0.01, min_auc=20.0), LENS, [(ev, None)], peaks=False)
    assert h.count_in_regions(np.zeros(0, dtype=REGION_DTYPE)) == 1
    got = h.region_counts(0)
    assert got.count.size == 0 and got.total == 120 * len(ev) and got.in_regions == 0
    dead = _regions([(7, 0, 100), (0, LENS[0], LENS[0] + 5)])      # regions, but none that can count
    assert h.count_in_regions(dead) == 1
    got = h.region_counts(0)
    assert got.count.tolist() == [0, 0] and got.total == 120 * len(ev) and got.in_regions == 0
    h.close()


def test_counting_regions_changes_nothing_else():
    rng = np.random.default_rng(10)
    ev = synth.make_fragments(LENS, 300_000, 17, peak_every=20_000, tower_every=3_000_000)
    params = B.make_params(pq=0.01, min_auc=20.0)
    reg = _random_regions(rng, LENS, 5000)
    off, _ = _run(params, LENS, [(ev, None)], peaks=False)
    on, _ = _run(params, LENS, [(ev, None)], peaks=False)
    assert on.count_in_regions(reg) == 1           # between sample_end and the rest of the run
    for h in (off, on):
        h.sample_no_control()
        h.pvalues()
        h.find_peaks()
    assert on.count_in_regions(reg) == 1
    assert len(off.get_peaks()) > 50 and off.get_peaks().tobytes() == on.get_peaks().tobytes()
    for c in range(len(LENS)):
        e0, c0 = off.get_intervals(-1, c, piles=False)
        e1, c1 = on.get_intervals(-1, c, piles=False)
        assert np.array_equal(e0, e1) and np.array_equal(c0["p"].view(np.uint32), c1["p"].view(np.uint32))
    f0, f1 = off.path_info(), on.path_info()
    assert not f0 & GX_PATH_REGION_COUNTS and f1 == f0 | GX_PATH_REGION_COUNTS, (f0, f1)
    off.close()
    on.close()


# ---- the command line -------------------------------------------------------------------------------------------------

CLI_CASES = ["basic", "ctrl_q", "reps3"]


def _cli_inputs(name):
    cases, mg = _cases()
    meta, _, _, _ = G.load_case(name)
    tmp = meta["tmp_prefix"].rstrip("/")   # same input paths as when the fixture was made (-k names them)
    args = _write_inputs(cases[name], mg, tmp)
    t = args[args.index("-t") + 1].split(",")
    c = args[args.index("-c") + 1].split(",") if "-c" in args else []
    names = []
    for r, tf in enumerate(t):
        names.append(tf)
        if r < len(c) and c[r] != "null":
            names.append(c[r])
    return meta, args, tmp, names


def _cli_bed(name, tmp):
    """A BED made of the fixture's narrowPeak lines: shuffled, every third row widened (so rows overlap), some rows with a name
    (and the narrowPeak's further columns), one row on a chromosome no header names.  -> (path, rows as the text has them)."""
    rng = np.random.default_rng(len(name))
    rows, lines = [], []
    for i, l in enumerate(G.read_gz(name, "out.narrowPeak").decode().splitlines()):
        f = l.split("\t")
        s, e = int(f[1]), int(f[2])
        if i % 3 == 0:
            s, e = max(0, s - 400), e + 900
        if i % 4 == 0:
            rows.append((f[0], s, e, None))
            lines.append(f"{f[0]}\t{s}\t{e}")
        elif i % 4 == 1:
            rows.append((f[0], s, e, f"site{i}"))
            lines.append(f"{f[0]}\t{s}\t{e}\tsite{i}")
        else:
            rows.append((f[0], s, e, f[3]))
            lines.append("\t".join([f[0], str(s), str(e)] + f[3:]))
    rows.append(("chrNowhere", 5, 5000, None))
    lines.append("chrNowhere\t5\t5000")
    for ch in G.load_case(name)[0]["chroms"]:     # overlapping 9-kb bins over the first half, one beyond the chromosome's end
        for s in list(range(0, ch["len"] // 2, 7000)) + [ch["len"] - 3000]:
            rows.append((ch["name"], s, s + 9000, None))
            lines.append(f"{ch['name']}\t{s}\t{s + 9000}")
    assert len(rows) > 15
    p = rng.permutation(len(rows))
    rows, lines = [rows[i] for i in p], [lines[i] for i in p]
    path = os.path.join(tmp, "regions.bed")
    with open(path, "w") as f:
        f.write("".join(l + "\n" for l in lines))
    return path, rows


def _cli_expected(name, rows, sample_names):
    """The expected text and -v lines, from events.bed (the -b lines of the fixture) through regions_ref."""
    meta, case, params, names = G.load_case(name)
    idx = {n: i for i, n in enumerate(names)}
    by = {}
    for line in G.read_gz(name, "events.bed").decode().splitlines():
        c, s, e, nm = line.split("\t")
        _, cnt, kind, smp = nm.rsplit("_", 3)
        by.setdefault((int(smp), kind == "C"), []).append((idx[c], int(s), int(e), int(cnt)))
    samples = []
    for r, rep in enumerate(case["replicates"]):
        samples.append((r, False))
        if rep["ctrl"] is not None:
            samples.append((r, True))
    assert len(samples) == len(sample_names)
    rc = [idx.get(r[0], len(names) + 5) for r in rows]
    exp = []
    for key in samples:
        a = np.array(by.get(key, []), dtype=np.int64).reshape(-1, 4)
        exp.append(R.count_in_regions(a[:, 0], a[:, 1], a[:, 2], R.weights(a[:, 3]) if len(a) else a[:, 3], rc,
                                      [r[1] for r in rows], [r[2] for r in rows]))
    assert any(e[0].any() for e in exp)
    txt = R.region_counts_text(rows, sample_names, [e[0] for e in exp])
    return txt, [R.fraction_line(r, c, e[1], e[2]) for (r, c), e in zip(samples, exp)]


@pytest.mark.parametrize("name", CLI_CASES)
def test_cli_region_counts_and_the_other_outputs(name):
    meta, args, tmp, sample_names = _cli_inputs(name)
    assert "-X" not in args
    bed, rows = _cli_bed(name, tmp)
    txt, vlines = _cli_expected(name, rows, sample_names)
    out = os.path.join(tmp, "reg_out")
    cmd = [_binary(), "-v", "-f", out + ".log", "-k", out + ".pile", "-b", out + ".bed", "-o", out + ".narrowPeak",
           "--count-regions", bed, "--region-counts", out + ".regions"] + args
    if "-r" in args:
        cmd += ["-R", out + ".dups"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert open(out + ".regions").read() == txt
    assert open(out + ".bed", "rb").read() == G.read_gz(name, "events.bed")
    assert open(out + ".pile", "rb").read() == G.read_gz(name, "out.pile")
    assert open(out + ".log", "rb").read() == G.read_gz(name, "out.log")
    assert open(out + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")
    assert [l for l in res.stderr.splitlines() if l.startswith("  Intervals in regions")] == vlines
    assert "Intervals in peaks" not in res.stderr


@pytest.mark.parametrize("name", CLI_CASES)
def test_cli_region_counts_gzip_two_contexts_no_peaks_and_with_counts(name):
    meta, args, tmp, sample_names = _cli_inputs(name)
    bed, rows = _cli_bed(name, tmp)
    txt, vlines = _cli_expected(name, rows, sample_names)
    run = lambda extra: subprocess.run([_binary()] + extra + args, capture_output=True, text=True)
    # -z, with the BED itself gzipped
    out = os.path.join(tmp, "regz_out")
    with gzip.open(bed + ".gz", "wb") as f:
        f.write(open(bed, "rb").read())
    res = run(["-z", "-o", out + ".narrowPeak", "--count-regions", bed + ".gz", "--region-counts", out + ".regions"])
    assert res.returncode == 0, res.stderr
    assert gzip.open(out + ".regions.gz", "rb").read().decode() == txt
    assert gzip.open(out + ".narrowPeak.gz", "rb").read() == G.read_gz(name, "out.narrowPeak")
    # two contexts on the one GPU, chromosomes sharded between them
    out = os.path.join(tmp, "reg2_out")
    res = run(["--devices", "0,0", "-o", out + ".narrowPeak", "--count-regions", bed, "--region-counts", out + ".regions"])
    assert res.returncode == 0, res.stderr
    assert open(out + ".regions").read() == txt
    assert open(out + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")
    # -X: no peak calling at all
    out = os.path.join(tmp, "regX_out")
    res = run(["-X", "-v", "--count-regions", bed, "--region-counts", out + ".regions"])
    assert res.returncode == 0, res.stderr
    assert open(out + ".regions").read() == txt
    assert [l for l in res.stderr.splitlines() if l.startswith("  Intervals in regions")] == vlines
    # together with --counts, whose file is what --counts alone writes; -v: the regions' lines after the FRiP lines
    out = os.path.join(tmp, "regc_out")
    res = run(["-o", out + ".narrowPeak", "--counts", out + ".alone"])
    assert res.returncode == 0, res.stderr
    res = run(["-v", "-o", out + ".narrowPeak", "--counts", out + ".counts", "--count-regions", bed, "--region-counts", out + ".regions"])
    assert res.returncode == 0, res.stderr
    assert open(out + ".regions").read() == txt
    assert open(out + ".counts", "rb").read() == open(out + ".alone", "rb").read() and os.path.getsize(out + ".alone") > 100
    lines = res.stderr.splitlines()
    frip = [i for i, l in enumerate(lines) if l.startswith("  Intervals in peaks")]
    regs = [i for i, l in enumerate(lines) if l.startswith("  Intervals in regions")]
    assert len(frip) == len(regs) == len(vlines) and regs[0] == frip[-1] + 1 and [lines[i] for i in regs] == vlines


def test_cli_region_bed_errors(tmp_path):
    """-E's rules: end <= start and a missing field die with loadBED's message, before any output file exists."""
    meta, args, tmp, _ = _cli_inputs("basic")
    for text in ("chrA\t100\t100\n", "chrA\t500\t20\tname\n", "chrA\n", "chrA\t7"):
        bed = tmp_path / "bad.bed"
        bed.write_text(text)
        out = tmp_path / "r.tsv"
        res = subprocess.run([_binary(), "-o", str(tmp_path / "o.np"), "--count-regions", str(bed), "--region-counts", str(out)] + args,
                             capture_output=True, text=True)
        assert res.returncode == 1 and "poorly formatted BED record" in res.stderr, res.stderr
        assert not out.exists() and not (tmp_path / "o.np").exists()
