"""The subsample kernels and the peak saturation curve on the GPU (gx_subsample_events, gx_subsample_kept, gx_saturation,
genrich-amd --saturation): the kernels' bytes against numpy (tests/saturation_ref.py) at the block and chunk edges, in every
push mode and launch geometry; every point's re-call against the CPU oracle on the numpy-subsampled events, field by field;
the edges of the call; the command line on two golden fixtures.

The synthetic depths are chosen (with the oracle, which runs on the CPU) so that the curve rises: the oracle calls at least 10
peaks at the 10 % point and strictly fewer than at 100 % in every shape, which the test asserts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import backends as B
import golden_cases as G
import saturation_ref as R
from genrich_amd import synth
from genrich_amd.lib import (EVENT_DTYPE, GX_ERR_EXPT, GX_PATH_SATURATION, GX_SAT_CONTROLS, pack_events, saturation_thresholds,
                             subsample_geometry)
from test_hip_complexity import MODES
from test_hip_counts import LENS, Mem, _cli_inputs, _push
from test_host_cli import _binary

pytestmark = pytest.mark.gpu

ORDER = -10
FULL = R.FULL
T10, T50 = FULL // 10, FULL // 2
CHUNK = 1 << 16          # CNT_CHUNK: the events of one entry of the chunk list


def _ctx(lens=LENS, params=None, count=True):
    import genrich_amd
    h = genrich_amd.Genrich(params or B.make_params(pq=0.01, min_auc=20.0))
    h.set_chroms(lens)
    if count:
        h.set_count_in_peaks(True)
    return h


# ---- the kernels, bytes against numpy ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def frags():
    ev = synth.make_fragments(LENS, 200_003, 77, peak_every=20_000)
    p8, rest = pack_events(ev)
    assert len(rest) == 0 and len(p8) == len(ev)          # (fragments are short: every one has an 8-byte form)
    return ev, p8


def test_kernels_at_the_block_and_chunk_edges(frags):
    ev, p8 = frags
    lanes, grid, block = subsample_geometry()
    assert lanes % 64 == 0 and grid >= 1 and block % lanes == 0 and CHUNK % block == 0
    h = _ctx(count=False)
    assert not h.path_info() & GX_PATH_SATURATION
    sizes = [0, 1, 63, 64, 65, block - 1, block, block + 1, CHUNK - 1, CHUNK, CHUNK + 1]
    seen = 0
    for n in sizes:
        for packed, src in ((False, ev), (True, p8)):
            for k, T in ((0, 3 * FULL // 10), (5, FULL)):
                want = R.subsample(ev[:n], 9, k, T).tobytes()
                for g in (1, 2, 0):
                    got = h.subsample_events(src[:n], 9, k, T, grid=g, packed=packed)
                    assert got.dtype == EVENT_DTYPE and got.tobytes() == want, (n, packed, k, T, g)
                seen += len(want) > 0
    assert seen > 30
    assert h.path_info() & GX_PATH_SATURATION
    h.reset()
    assert not h.path_info() & GX_PATH_SATURATION
    h.close()


def test_kernels_at_every_threshold(frags):
    ev, p8 = frags
    h = _ctx(count=False)
    kept = []
    for T in (0, 1, 1 << 31, FULL - 1, FULL):
        want = R.subsample(ev, 3, 1, T)
        for packed, src in ((False, ev), (True, p8)):
            outs = [h.subsample_events(src, 3, 1, T, grid=g, packed=packed).tobytes() for g in (1, 2, 0)]
            assert outs[0] == outs[1] == outs[2] == want.tobytes(), (T, packed)
        kept.append(len(want))
    assert kept[0] == 0 and kept[1] <= 1 and 0.49 < kept[2] / len(ev) < 0.51 and kept[3] >= len(ev) - 1 and kept[4] == len(ev)
    assert h.subsample_events(ev, 3, 1, T10).tobytes() != h.subsample_events(ev, 3, 2, T10).tobytes()      # the sample matters
    assert h.subsample_events(ev, 3, 1, T10).tobytes() != h.subsample_events(ev, 4, 1, T10).tobytes()      # ... and the seed
    lib, ctx = h.lib, h.ctx
    n = C.c_size_t(0)
    assert lib.gx_subsample_events(ctx, ev.ctypes.data, 10, 0, 1, 0, FULL + 1, 0, None, 0, C.byref(n)) == ORDER
    assert "threshold" in lib.gx_last_error(ctx).decode()
    assert lib.gx_subsample_events(ctx, ev.ctypes.data, 10, 0, 1, 0, FULL, 1 << 16, None, 0, C.byref(n)) == ORDER
    assert lib.gx_subsample_events(ctx, ev.ctypes.data, 1000, 0, 1, 0, T50, 0, None, 0, C.byref(n)) == 0     # cap 0: the count alone
    assert n.value == len(R.subsample(ev[:1000], 1, 0, T50))
    h.close()


# ---- kept samples in every push mode ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES + ["mixed"])
def test_kept_samples_in_every_push_mode(mode):
    """Two samples in one run (a treatment and its control: k = 0 and 1), more than one chunk each; `mixed`: a packed device
    piece of odd length followed by an unpacked host piece."""
    t = synth.make_fragments(LENS, 150_001, 21, peak_every=20_000)
    c = synth.make_fragments(LENS, 70_001, 22, uniform_only=True)
    h, mem = _ctx(), Mem()
    for is_ctrl, ev in ((0, t), (1, c)):
        h.sample_begin(is_ctrl, None)
        if mode == "mixed":
            odd = 40_001
            p8, rest = pack_events(ev[:odd])
            assert len(rest) == 0
            h.push_events_packed(mem.device(p8), where=2, n=len(p8))
            h.push_events(ev[odd:])
        else:
            _push(h, ev, mode, mem)
        h.sample_end()
    for k, ev in ((0, t), (1, c)):
        for T in (T10, 7 * FULL // 10):
            want = R.subsample(ev, 5, k, T)
            assert 0 < len(want) < len(ev)
            assert h.subsample_kept(k, 5, T).tobytes() == want.tobytes(), (mode, k, T)
    assert h.subsample_kept(1, 5, T10).tobytes() != R.subsample(c, 5, 0, T10).tobytes()      # k matters
    assert h.subsample_kept(0, 5, FULL).tobytes() == t.tobytes() and len(h.subsample_kept(0, 5, 0)) == 0
    n = C.c_size_t(0)
    assert h.lib.gx_subsample_kept(h.ctx, 2, 5, T10, None, 0, C.byref(n)) == ORDER                  # no such sample
    assert h.path_info() & GX_PATH_SATURATION
    h.close()
    mem.free()


# ---- the re-call against the oracle ------------------------------------------------------------------------------------------

def _shape(name):
    """(params, [(treat, ctrl | None, save | None)]): depths at which the oracle's peak count rises from 10 % to 100 %."""
    if name == "noctrl":
        a = synth.make_fragments(LENS, 1_500_000, 5, peak_every=20_000, frac_peak=0.1)
        return B.make_params(pq=0.01, min_auc=20.0), [(a, None, None)]
    if name == "ctrl_q":   # (-q calls the towers alone: 46 weak ones, some of which the subsamples lose)
        a = np.concatenate([synth.make_fragments(LENS, 1_400_000, 5, peak_every=20_000, frac_peak=0.1),
                            synth.make_fragments(LENS, 46 * 400, 8, frac_peak=0.0, frac_tower=1.0, tower_every=1_000_000)])
        a = a[np.random.default_rng(1).permutation(len(a))]
        c = synth.make_fragments(LENS, 1_000_000, 7, uniform_only=True)
        return B.make_params(pq=0.01, qval=True, min_auc=20.0), [(a, c, None)]
    a = synth.make_fragments(LENS, 2_000_000, 5, peak_every=20_000, frac_peak=0.06)
    b = synth.make_fragments(LENS, 2_000_000, 6, peak_every=20_000, frac_peak=0.06)
    c = synth.make_fragments(LENS, 300_000, 7, uniform_only=True)
    return B.make_params(pq=0.01, min_auc=20.0), [(a, c, None), (b, None, [1, 1, 0])]


def _drive(be, reps):
    """tests/backends.py run_case's sequence, with each replicate's save mask."""
    for t, c, save in reps:
        be.sample_begin(0, save)
        be.push_events(t)
        be.sample_end()
        if c is not None:
            be.sample_begin(1, None)
            be.push_events(c)
            be.sample_end()
        else:
            be.sample_no_control()
        be.pvalues()
    be.find_peaks()


def _subsampled(reps, seed, T, controls):
    """The replicates with sample k = 0, 1, .. (gx_sample_end order) subsampled at T; the controls only with `controls`."""
    out, k, n_total, n_kept = [], 0, 0, 0
    for t, c, save in reps:
        ts = R.subsample(t, seed, k, T)
        n_total, n_kept, k = n_total + len(t), n_kept + len(ts), k + 1
        cs = c
        if c is not None:
            if controls:
                cs = R.subsample(c, seed, k, T)
                n_total, n_kept = n_total + len(c), n_kept + len(cs)
            k += 1
        out.append((ts, cs, save))
    return out, n_total, n_kept


def _same_peaks(po, ph):
    """tests/test_hip_parity.py's comparison of two peak lists."""
    assert len(po) == len(ph), (len(po), len(ph))
    for f in ("chrom", "start", "end", "summit"):
        assert np.array_equal(po[f], ph[f]), f
    for f in ("auc", "p", "q"):
        assert np.array_equal(po[f].view(np.uint32), ph[f].view(np.uint32)), f


@pytest.mark.parametrize("name,controls", [("noctrl", False), ("ctrl_q", False), ("reps2", False), ("ctrl_q", True)])
def test_recall_against_the_oracle(name, controls):
    params, reps = _shape(name)
    h = _ctx(params=params)
    _drive(h, reps)
    own = h.get_peaks()
    thr = [T10, T50, FULL]
    pts = h.saturation(thr, seed=1, flags=GX_SAT_CONTROLS if controls else 0)
    counts = []
    for j, T in enumerate(thr):
        sub, n_total, n_kept = _subsampled(reps, 1, T, controls)
        o = B.Oracle(params)
        o.set_chroms(LENS)
        _drive(o, sub)
        got = h.saturation_peaks(j)
        print(name, controls, T, "oracle", o.n_peaks, o.peak_bp, "device", int(pts[j]["n_peaks"]), int(pts[j]["peak_bp"]))
        _same_peaks(o.get_peaks(), got)
        p = pts[j]
        assert (int(p["threshold"]), int(p["status"])) == (T, 0)
        assert (int(p["n_peaks"]), int(p["peak_bp"]), int(p["genome_len"])) == (o.n_peaks, o.peak_bp, o.genome_len)
        assert (int(p["n_total"]), int(p["n_kept"])) == (n_total, n_kept)
        counts.append(o.n_peaks)
        o.close()
    assert 10 <= counts[0] < counts[2], counts             # no comparison of two empty lists; the curve rises
    assert h.saturation_peaks(2).tobytes() == own.tobytes()    # the whole sample: the run's own peaks, byte for byte
    assert h.get_peaks().tobytes() == own.tobytes()
    h.close()


# ---- edges -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small():
    t = synth.make_fragments(LENS, 400_000, 33, peak_every=20_000)
    c = synth.make_fragments(LENS, 200_000, 34, uniform_only=True)
    return t, c


def test_a_point_that_keeps_nothing_and_the_points_after_it(small):
    t, c = small
    h = _ctx()
    _drive(h, [(t, c, None)])
    assert len(R.subsample(t, 1, 0, 1)) == 0
    pts = h.saturation([1, T50, 0, FULL])
    assert [int(s) for s in pts["status"]] == [GX_ERR_EXPT, 0, GX_ERR_EXPT, 0]
    assert [int(pts[j][f]) for j in (0, 2) for f in ("n_kept", "n_peaks", "peak_bp")] == [0] * 6
    assert len(h.saturation_peaks(0)) == 0 and int(pts[0]["n_total"]) == len(t)
    mid, last = h.saturation_peaks(1).copy(), h.saturation_peaks(3).copy()
    alone = h.saturation([T50])
    assert h.saturation_peaks(0).tobytes() == mid.tobytes() and len(mid) > 10
    assert alone[0].tobytes() == pts[1].tobytes()
    assert last.tobytes() == h.get_peaks().tobytes()
    text = h.saturation_text().decode().splitlines()
    assert text[0] == f"# run: {h.n_peaks} peaks, {h.peak_bp} bp" and len(text) == 3
    h.close()


def test_a_point_that_ends_early_counts_every_subsampled_sample(small):
    """Two replicates, the first with a control: a point whose first treatment keeps nothing still reports the events of all the
    subsampled samples."""
    t, c = small
    t2 = t[::2].copy()
    h = _ctx()
    _drive(h, [(t, c, None), (t2, None, None)])
    plain = h.saturation([0, FULL])
    assert [int(x) for x in plain["status"]] == [GX_ERR_EXPT, 0]
    assert [int(x) for x in plain["n_total"]] == [len(t) + len(t2)] * 2 and [int(x) for x in plain["n_kept"]] == [0, len(t) + len(t2)]
    both = h.saturation([0, FULL], flags=GX_SAT_CONTROLS)
    assert [int(x) for x in both["status"]] == [GX_ERR_EXPT, 0]
    assert [int(x) for x in both["n_total"]] == [len(t) + len(c) + len(t2)] * 2 and int(both[1]["n_kept"]) == len(t) + len(c) + len(t2)
    assert h.saturation_peaks(1).tobytes() == h.get_peaks().tobytes()
    h.close()


def test_order_rules_twice_the_same_and_nothing_else_changes(small):
    t, c = small
    h = _ctx(count=False)
    lib, ctx = h.lib, h.ctx
    thr = np.array([T10, FULL], dtype=np.uint64)
    out = np.zeros(2, dtype=[("w", "<u8", (7,))])
    call = lambda: lib.gx_saturation(ctx, thr.ctypes.data, 2, 1, 0, out.ctypes.data)
    err = lambda: lib.gx_last_error(ctx).decode()
    _drive(h, [(t, None, None)])
    assert call() == ORDER and "gx_set_count_in_peaks" in err()                  # counting off
    h.reset()
    h.set_count_in_peaks(True)
    h.sample_begin(0, None)
    h.push_events(t)
    assert call() == ORDER and "after gx_find_peaks" in err()                    # a sample is open
    h.sample_end()
    h.sample_begin(1, None)
    h.push_events(c)
    h.sample_end()
    h.pvalues()
    assert call() == ORDER and "after gx_find_peaks" in err()                    # no peaks yet
    assert lib.gx_get_saturation_peaks(ctx, 0, None, 0) == ORDER                 # no result yet
    h.find_peaks()
    bad = np.array([FULL + 1], dtype=np.uint64)
    assert lib.gx_saturation(ctx, bad.ctypes.data, 1, 1, 0, out.ctypes.data) == ORDER and "threshold" in err()
    assert lib.gx_saturation(ctx, thr.ctypes.data, 2, 1, 2, out.ctypes.data) == ORDER       # an unknown flag
    assert h.count_in_peaks() == 2 and h.complexity() == 2
    own, flags = h.get_peaks(), h.path_info()
    cnt = [h.peak_counts(i) for i in range(2)]
    cpx = [h.get_complexity(i) for i in range(2)]
    assert not flags & GX_PATH_SATURATION
    first = h.saturation([T10, FULL])
    peaks = [h.saturation_peaks(j).tobytes() for j in range(2)]
    again = h.saturation([T10, FULL])
    assert first.tobytes() == again.tobytes() and peaks == [h.saturation_peaks(j).tobytes() for j in range(2)]
    assert 0 < int(first[0]["n_kept"]) < int(first[1]["n_kept"]) == len(t) and int(first[0]["n_peaks"]) > 10
    assert lib.gx_get_saturation_peaks(ctx, 2, None, 0) == ORDER                 # no such point
    # the parent's results are what they were
    assert h.get_peaks().tobytes() == own.tobytes() == peaks[1]
    for i in range(2):
        now = h.peak_counts(i)
        assert np.array_equal(now.count, cnt[i].count) and now[1:] == cnt[i][1:]
        assert h.get_complexity(i) == cpx[i]
    assert h.count_in_peaks() == 2 and np.array_equal(h.peak_counts(0).count, cnt[0].count)
    assert h.path_info() == flags | GX_PATH_SATURATION                           # the other bits as without the feature
    h.reset()
    assert not h.path_info() & GX_PATH_SATURATION
    assert lib.gx_get_saturation_peaks(ctx, 0, None, 0) == ORDER                 # gx_reset drops the result
    _drive(h, [(t, None, None)])                                                 # a second run on the context, and its curve
    pts = h.saturation([FULL])
    assert h.saturation_peaks(0).tobytes() == h.get_peaks().tobytes() and int(pts[0]["n_peaks"]) == h.n_peaks
    h.close()


# ---- the command line --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ctrl_q", "atac"])
def test_cli_saturation_of_the_golden_fixtures(name):
    meta, case, params, names = G.load_case(name)
    _, args, tmp, _ = _cli_inputs(name)
    out = os.path.join(tmp, "sat_out")
    res = subprocess.run([_binary(), "-v", "-o", out + ".narrowPeak", "--saturation", out + ".tsv", "--saturation-steps", "4"] + args,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert open(out + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")
    lines = open(out + ".tsv").read().splitlines()
    assert lines[0].startswith("# run: ") and lines[1].split("\t")[:4] == ["fraction", "threshold", "kept", "peaks"] and len(lines) == 6
    rows = [dict(zip(lines[1].split("\t"), l.split("\t"))) for l in lines[2:]]
    thr = saturation_thresholds(4)
    assert [int(r["threshold"]) for r in rows] == thr and [r["fraction"] for r in rows] == ["0.250000", "0.500000", "0.750000", "1.000000"]
    # the same curve through the library on the fixture's events
    import genrich_amd
    h = genrich_amd.Genrich(params)
    h.set_chroms(case["lens"], case.get("skip"), case.get("beds"))
    h.set_count_in_peaks(True)
    _drive(h, [(r["treat"], r.get("ctrl"), r.get("save")) for r in case["replicates"]])
    pts = h.saturation(thr, seed=1)
    assert [int(r["peaks"]) for r in rows] == [int(p) for p in pts["n_peaks"]]
    assert [int(r["kept"]) for r in rows] == [int(p) for p in pts["n_kept"]]
    assert [int(r["peak_bp"]) for r in rows] == [int(p) for p in pts["peak_bp"]]
    assert h.saturation_text().decode().splitlines() == lines
    last = rows[-1]
    assert lines[0] == f"# run: {h.n_peaks} peaks, {h.peak_bp} bp" and h.n_peaks > 0
    assert int(last["recovered"]) == int(last["peaks"]) == int(last["in_run"]) == h.n_peaks and last["recovered_share"] == "1.000000"
    assert int(last["shared_bp"]) == int(last["peak_bp"]) == h.peak_bp and last["status"] == "ok"
    sat = [l for l in res.stderr.splitlines() if l.startswith("  Saturation")]
    assert len(sat) == 4 + 2 and "recover 90 %" in sat[4] and "the last step" in sat[5], sat
    h.close()
