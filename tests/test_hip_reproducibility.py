"""The split kernel and the reproducibility calls on the GPU (gx_subsample_split_events, gx_subsample_split_kept,
gx_reproducibility, genrich-amd --reproducibility): the split's bytes against numpy (tests/saturation_ref.py's draw) at the block
and chunk edges, in every push mode and launch geometry; every call against the CPU oracle on the numpy-split events, field by
field, and the figures against the brute force of tests/reproducibility_ref.py; one replicate, where the calls must repeat the
run and each other; the edges of the call; the command line on two golden fixtures.

The synthetic depths are the issue's: the oracle (on the CPU) calls about 2,000 peaks in every call of the two-replicate shape,
and the test asserts that no compared list has fewer than 100."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import backends as B
import golden_cases as G
import reproducibility_ref as RR
import saturation_ref as R
from genrich_amd import synth
from genrich_amd.lib import (EVENT_DTYPE, GX_ERR_EXPT, GX_PATH_SATURATION, GX_PATH_SPLIT, GX_REPRO_ALONE, GX_REPRO_POOLED, GX_REPRO_SELF,
                             REPRO_VERDICTS, pack_events, repro_label, reproducibility_figures, subsample_geometry)
from test_hip_complexity import MODES
from test_hip_counts import LENS, Mem, _cli_inputs, _push
from test_hip_saturation import _ctx, _drive, _same_peaks, _shape
from test_host_cli import _binary

pytestmark = pytest.mark.gpu

ORDER = -10
FULL = R.FULL
HALF = 1 << 31
CHUNK = 1 << 16          # CNT_CHUNK: the events of one entry of the chunk list


def _split(ev, seed, k, T):
    """(A then B, n_a): the stable partition in numpy."""
    m = R.keep_mask(len(ev), seed, k, T)
    return np.concatenate([ev[m], ev[~m]]), int(m.sum())


# ---- the kernel, bytes against numpy -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def frags():
    ev = synth.make_fragments(LENS, 200_003, 77, peak_every=20_000)
    p8, rest = pack_events(ev)
    assert len(rest) == 0 and len(p8) == len(ev)          # (fragments are short: every one has an 8-byte form)
    return ev, p8


def test_split_at_the_block_and_chunk_edges(frags):
    ev, p8 = frags
    lanes, grid, block = subsample_geometry()
    h = _ctx(count=False)
    assert not h.path_info() & GX_PATH_SPLIT
    sizes = [0, 1, 63, 64, 65, block - 1, block, block + 1, CHUNK - 1, CHUNK, CHUNK + 1]
    seen = 0
    for n in sizes:
        for packed, src in ((False, ev), (True, p8)):
            for k, T in ((0, 0), (5, 1), (0, HALF), (5, HALF), (0, FULL - 1), (5, FULL), (0, 3 * FULL // 10)):
                want, na = _split(ev[:n], 9, k, T)
                for g in (1, 2, 0):
                    got, got_na = h.subsample_split_events(src[:n], 9, k, T, grid=g, packed=packed)
                    assert got.dtype == EVENT_DTYPE and got_na == na and got.tobytes() == want.tobytes(), (n, packed, k, T, g)
                seen += 0 < na < n
    assert seen > 40
    assert h.path_info() & GX_PATH_SPLIT and not h.path_info() & GX_PATH_SATURATION     # k_sub_write did not run
    for n in sizes:                                      # half A is the subsample at the same seed, sample and T
        for k, T in ((0, 0), (5, 1), (0, HALF), (0, FULL - 1), (5, FULL)):
            got, na = h.subsample_split_events(ev[:n], 9, k, T)
            assert got[:na].tobytes() == h.subsample_events(ev[:n], 9, k, T).tobytes(), (n, k, T)
    h.reset()
    assert not h.path_info() & GX_PATH_SPLIT
    h.close()


def test_split_at_every_threshold(frags):
    ev, p8 = frags
    h = _ctx(count=False)
    sizes = []
    for T in (0, 1, HALF, FULL - 1, FULL):
        want, na = _split(ev, 3, 1, T)
        for packed, src in ((False, ev), (True, p8)):
            outs = [h.subsample_split_events(src, 3, 1, T, grid=g, packed=packed) for g in (1, 2, 0)]
            assert all(o[1] == na and o[0].tobytes() == want.tobytes() for o in outs), (T, packed)
        assert want[:na].tobytes() == h.subsample_events(ev, 3, 1, T).tobytes()          # half A is the subsample at T
        assert np.array_equal(np.sort(want, order=["chrom", "start", "end", "count"]), np.sort(ev, order=["chrom", "start", "end", "count"]))
        sizes.append(na)
    assert sizes[0] == 0 and sizes[1] <= 1 and 0.49 < sizes[2] / len(ev) < 0.51 and sizes[3] >= len(ev) - 1 and sizes[4] == len(ev)
    assert h.subsample_split_events(ev, 3, 1, HALF)[0].tobytes() != h.subsample_split_events(ev, 3, 2, HALF)[0].tobytes()    # the sample matters
    assert h.subsample_split_events(ev, 3, 1, HALF)[0].tobytes() != h.subsample_split_events(ev, 4, 1, HALF)[0].tobytes()    # ... and the seed
    lib, ctx = h.lib, h.ctx
    n = C.c_size_t(0)
    assert lib.gx_subsample_split_events(ctx, ev.ctypes.data, 10, 0, 1, 0, FULL + 1, 0, None, 0, C.byref(n)) == ORDER
    assert "threshold" in lib.gx_last_error(ctx).decode()
    assert lib.gx_subsample_split_events(ctx, ev.ctypes.data, 10, 0, 1, 0, FULL, 1 << 16, None, 0, C.byref(n)) == ORDER
    assert lib.gx_subsample_split_events(ctx, ev.ctypes.data, 1000, 0, 1, 0, HALF, 0, None, 0, C.byref(n)) == 0      # cap 0: the count alone
    assert n.value == _split(ev[:1000], 1, 0, HALF)[1]
    h.sample_begin(0, None)
    assert lib.gx_subsample_split_events(ctx, ev.ctypes.data, 10, 0, 1, 0, HALF, 0, None, 0, C.byref(n)) == ORDER    # a sample is open
    h.close()


# ---- kept samples in every push mode ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES + ["mixed"])
def test_split_kept_in_every_push_mode(mode):
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
        for T in (FULL // 10, HALF):
            want, na = _split(ev, 5, k, T)
            assert 0 < na < len(ev)
            got, got_na = h.subsample_split_kept(k, 5, T, len(ev))
            assert got_na == na and got.tobytes() == want.tobytes(), (mode, k, T)
    assert h.subsample_split_kept(1, 5, HALF, len(c))[0].tobytes() != _split(c, 5, 0, HALF)[0].tobytes()      # k matters
    assert h.subsample_split_kept(0, 5, HALF, len(t))[0][:_split(t, 5, 0, HALF)[1]].tobytes() == h.subsample_kept(0, 5, HALF).tobytes()
    n = C.c_size_t(0)
    assert h.lib.gx_subsample_split_kept(h.ctx, 2, 5, HALF, None, 0, C.byref(n)) == ORDER                     # no such sample
    assert h.lib.gx_subsample_split_kept(h.ctx, 0, 5, FULL + 1, None, 0, C.byref(n)) == ORDER
    assert h.path_info() & GX_PATH_SPLIT
    h.close()
    mem.free()


# ---- every call against the oracle -----------------------------------------------------------------------------------------------

def _parts(reps, seed):
    """reps = [(treat, ctrl | None, save)] -> the 3 R + 2 calls as (kind, rep, half, [(treat part, ctrl, save)]), the library's order;
    the kept index of a treatment counts the controls before it."""
    halves, k = [], 0
    for t, c, save in reps:
        both, na = _split(t, seed, k, HALF)
        halves.append((both[:na], both[na:]))
        k += 1 if c is None else 2
    calls = [(GX_REPRO_ALONE, r, -1, [reps[r]]) for r in range(len(reps))]
    calls += [(GX_REPRO_SELF, r, h, [(halves[r][h], reps[r][1], reps[r][2])]) for r in range(len(reps)) for h in range(2)]
    calls += [(GX_REPRO_POOLED, -1, h, [(halves[r][h], reps[r][1], reps[r][2]) for r in range(len(reps))]) for h in range(2)]
    return calls


def _oracle(params, lens, reps):
    o = B.Oracle(params)
    o.set_chroms(lens)
    try:
        _drive(o, reps)
    except Exception:
        o.close()
        raise
    res = (o.get_peaks().copy(), o.n_peaks, o.peak_bp)
    o.close()
    return res


def test_every_call_against_the_oracle_and_the_figures_against_brute_force():
    params = B.make_params(pq=0.01, min_auc=20.0)
    reps = [(synth.make_fragments(LENS, 300_000, 5, peak_every=20_000, frac_peak=0.15), synth.make_fragments(LENS, 50_000, 7, uniform_only=True), None),
            (synth.make_fragments(LENS, 300_000, 6, peak_every=20_000, frac_peak=0.15), None, [1, 1, 0])]
    h = _ctx(params=params)
    _drive(h, reps)
    own = h.get_peaks()
    run_o = _oracle(params, LENS, reps)
    _same_peaks(run_o[0], own)
    calls = h.reproducibility(seed=1)
    want = _parts(reps, 1)
    assert len(calls) == len(want) == 8
    lists = []
    for i, (kind, rep, half, parts) in enumerate(want):
        po, n_peaks, bp = _oracle(params, LENS, parts)
        got = h.reproducibility_peaks(i)
        c = calls[i]
        print(repro_label(c), "oracle", n_peaks, bp, "device", int(c["n_peaks"]), int(c["peak_bp"]))
        _same_peaks(po, got)
        assert (int(c["kind"]), int(c["rep"]), int(c["half"]), int(c["status"])) == (kind, rep, half, 0)
        assert (int(c["n_events"]), int(c["n_peaks"]), int(c["peak_bp"])) == (sum(len(p[0]) for p in parts), n_peaks, bp)
        assert len(got) >= 100                                  # no comparison of near-empty lists
        lists.append(got)
    assert h.get_peaks().tobytes() == own.tobytes() and len(own) >= 100
    seen = []
    for pct in (0, 50, 100):
        ref = RR.figures(own, lists, pct)
        got = reproducibility_figures(own, calls, lists, pct)
        fig = got["fig"]
        print("pct", pct, "Nt", ref["nt"], "Np", ref["np"], "N_self", ref["n_self"], ref["verdict"])
        assert (int(fig["nt"]), int(fig["np"]), got["n_self"].tolist(), got["nt_pair"].tolist()) == (ref["nt"], ref["np"], ref["n_self"], ref["nt_pair"])
        assert got["in_run"].tolist() == ref["in_run"] and got["run_supported"].tolist() == ref["run_supported"]
        assert REPRO_VERDICTS[int(fig["verdict"])] == ref["verdict"]
        assert got["conservative"].tolist() == [int(x) for x in ref["conservative"]] and got["optimal"].tolist() == [int(x) for x in ref["optimal"]]
        text, metrics = h.reproducibility_text(pct)
        assert metrics.decode() == RR.metrics_text(ref)
        rows = text.decode().splitlines()
        assert rows[0] == f"# run: {h.n_peaks} peaks, {h.peak_bp} bp; overlap {pct} %; seed 1"
        assert [r.split("\t")[0] for r in rows[2:]] == RR.labels(2)
        assert [int(r.split("\t")[6]) for r in rows[2:]] == ref["in_run"] and [int(r.split("\t")[7]) for r in rows[2:]] == ref["run_supported"]
        assert min(ref["nt"], ref["np"], *ref["n_self"]) >= 100
        seen.append((ref["nt"], ref["np"], tuple(ref["n_self"])))
    assert len(set(seen)) == 3 and all(len({s[i] for s in seen}) == 3 for i in range(3))      # the predicate reads PCT
    h.close()


def test_one_replicate_repeats_the_run_and_itself():
    params, reps = _shape("noctrl")
    reps = [(reps[0][0][:400_000].copy(), None, None)]
    both, na = _split(reps[0][0], 1, 0, HALF)
    for half in (both[:na], both[na:]):
        assert _oracle(params, LENS, [(half, None, None)])[1] >= 10
    h = _ctx(params=params)
    _drive(h, reps)
    own = h.get_peaks()
    calls = h.reproducibility(seed=1)
    assert len(calls) == 5 and [int(c["n_events"]) for c in calls] == [len(both), na, len(both) - na, na, len(both) - na]
    pk = [h.reproducibility_peaks(i) for i in range(5)]
    assert pk[0].tobytes() == own.tobytes() and len(own) >= 10                        # ALONE 0 is the run itself
    assert pk[3].tobytes() == pk[1].tobytes() and pk[4].tobytes() == pk[2].tobytes()    # POOLED h is SELF 0 h
    assert min(len(p) for p in pk) >= 10 and pk[1].tobytes() != pk[2].tobytes()
    _, metrics = h.reproducibility_text(50)
    rows = dict(l.split("\t") for l in metrics.decode().splitlines())
    assert (rows["replicates"], rows["Nt"], rows["rescue_ratio"], rows["self_consistency_ratio"], rows["verdict"]) == ("1", "NA", "NA", "NA", "NA")
    assert int(rows["Np"]) > 0 and int(rows["N_self.t1"]) > 0
    pts = h.saturation([HALF], seed=1)                                                # SELF 0 0 is the saturation point at 2^31
    assert h.saturation_peaks(0).tobytes() == pk[1].tobytes() and int(pts[0]["n_kept"]) == na
    h.close()


# ---- edges -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small():
    t = synth.make_fragments(LENS, 400_000, 33, peak_every=20_000)
    c = synth.make_fragments(LENS, 200_000, 34, uniform_only=True)
    return t, c


def test_order_rules_twice_the_same_and_nothing_else_changes(small):
    t, c = small
    h = _ctx(count=False)
    lib, ctx = h.lib, h.ctx
    out = np.zeros(5, dtype=[("w", "<u8", (5,))])
    n = C.c_size_t(0)
    call = lambda flags=0: lib.gx_reproducibility(ctx, 1, flags, out.ctypes.data, 5, C.byref(n))
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
    assert lib.gx_get_reproducibility_peaks(ctx, 0, None, 0) == ORDER            # no result yet
    h.find_peaks()
    assert call(1) == ORDER and call(2) == ORDER                                 # a flag other than 0
    assert h.count_in_peaks() == 2 and h.complexity() == 2
    own, flags = h.get_peaks(), h.path_info()
    cnt = [h.peak_counts(i) for i in range(2)]
    cpx = [h.get_complexity(i) for i in range(2)]
    assert not flags & (GX_PATH_SPLIT | GX_PATH_SATURATION)
    sat_alone = h.saturation([FULL // 10, FULL])
    sat_peaks = [h.saturation_peaks(j).tobytes() for j in range(2)]
    h.reset()                                                                    # (the same run again, without the curve's bit)
    h.set_count_in_peaks(True)
    _drive(h, [(t, c, None)])
    assert h.count_in_peaks() == 2 and h.complexity() == 2
    assert h.get_peaks().tobytes() == own.tobytes() and h.path_info() == flags
    first = h.reproducibility()
    peaks = [h.reproducibility_peaks(i).tobytes() for i in range(5)]
    texts = h.reproducibility_text(50)
    assert h.path_info() == flags | GX_PATH_SPLIT                                # the other bits as without the feature
    again = h.reproducibility()
    assert first.tobytes() == again.tobytes() and peaks == [h.reproducibility_peaks(i).tobytes() for i in range(5)]
    assert texts == h.reproducibility_text(50) and texts != h.reproducibility_text(100)
    assert int(first[0]["n_events"]) == len(t) and int(first[1]["n_events"]) + int(first[2]["n_events"]) == len(t)
    assert all(int(x) > 10 for x in first["n_peaks"]) and all(int(x) == 0 for x in first["status"])
    assert lib.gx_get_reproducibility_peaks(ctx, 5, None, 0) == ORDER            # no such call
    assert lib.gx_reproducibility(ctx, 1, 0, None, 0, C.byref(n)) == 0 and n.value == 5      # cap 0: the count alone
    # the parent's results are what they were
    assert h.get_peaks().tobytes() == own.tobytes() == peaks[0]
    for i in range(2):
        now = h.peak_counts(i)
        assert np.array_equal(now.count, cnt[i].count) and now[1:] == cnt[i][1:]
        assert h.get_complexity(i) == cpx[i]
    assert h.count_in_peaks() == 2 and np.array_equal(h.peak_counts(0).count, cnt[0].count)
    # the curve before and after gives what it gives alone, and the calls are still there
    sat = h.saturation([FULL // 10, FULL])
    assert sat.tobytes() == sat_alone.tobytes() and [h.saturation_peaks(j).tobytes() for j in range(2)] == sat_peaks
    assert h.path_info() == flags | GX_PATH_SPLIT | GX_PATH_SATURATION
    assert h.reproducibility().tobytes() == first.tobytes() and [h.reproducibility_peaks(i).tobytes() for i in range(5)] == peaks
    assert h.saturation([FULL // 10, FULL]).tobytes() == sat_alone.tobytes() and h.saturation_peaks(0).tobytes() == sat_peaks[0]
    h.reset()
    assert not h.path_info() & (GX_PATH_SPLIT | GX_PATH_SATURATION)
    assert lib.gx_get_reproducibility_peaks(ctx, 0, None, 0) == ORDER            # gx_reset drops the result
    h.close()


def test_a_half_with_no_fragment_and_the_calls_after_it():
    """One treatment of one event: one half is empty, and the call on it is a result of its own."""
    ev = np.zeros(1, dtype=EVENT_DTYPE)
    ev[0] = (0, 1000, 1200, 1)
    in_a = bool(R.keep_mask(1, 1, 0, HALF)[0])
    h = _ctx(params=B.make_params(pq=0.01, min_auc=0.0))
    _drive(h, [(ev, None, None)])
    calls = h.reproducibility(seed=1)
    empty = [2, 4] if in_a else [1, 3]
    assert [int(c["n_events"]) for c in calls] == ([1, 1, 0, 1, 0] if in_a else [1, 0, 1, 0, 1])
    for i in range(5):
        c = calls[i]
        if i in empty:
            assert (int(c["status"]), int(c["n_peaks"]), int(c["peak_bp"])) == (GX_ERR_EXPT, 0, 0) and len(h.reproducibility_peaks(i)) == 0
        else:
            assert int(c["status"]) == 0 and h.reproducibility_peaks(i).tobytes() == h.get_peaks().tobytes()
    rows = h.reproducibility_text(50)[0].decode().splitlines()[2:]
    assert [r.split("\t")[-1] for r in rows] == ["no_fragments" if i in empty else "ok" for i in range(5)]
    h.close()


# ---- the command line --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ctrl_q", "atac"])
def test_cli_reproducibility_of_the_golden_fixtures(name):
    meta, case, params, names = G.load_case(name)
    _, args, tmp, _ = _cli_inputs(name)
    out = os.path.join(tmp, "repro_out")
    res = subprocess.run([_binary(), "-v", "-o", out + ".narrowPeak", "--reproducibility", out + ".tsv", "--reproducibility-metrics", out + ".metrics.tsv",
                          "--reproducibility-peaks", out + ".pk", "--reproducibility-overlap", "30", "--reproducibility-seed", "3"] + args,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    narrow = open(out + ".narrowPeak", "rb").read()
    assert narrow == G.read_gz(name, "out.narrowPeak")
    # the same tables through the library on the fixture's events
    import genrich_amd
    h = genrich_amd.Genrich(params)
    h.set_chroms(case["lens"], case.get("skip"), case.get("beds"))
    h.set_count_in_peaks(True)
    reps = [(r["treat"], r.get("ctrl"), r.get("save")) for r in case["replicates"]]
    _drive(h, reps)
    calls = h.reproducibility(seed=3)
    text, metrics = h.reproducibility_text(30)
    assert open(out + ".tsv", "rb").read() == text and open(out + ".metrics.tsv", "rb").read() == metrics
    lines = text.decode().splitlines()
    assert lines[0] == f"# run: {h.n_peaks} peaks, {h.peak_bp} bp; overlap 30 %; seed 3" and h.n_peaks > 0
    assert lines[1].split("\t") == ["call", "rep", "half", "intervals", "peaks", "peak_bp", "in_run", "run_supported", "status"]
    assert len(lines) == 2 + len(calls) == 2 + 3 * len(reps) + 2
    labels = RR.labels(len(reps))
    for i, label in enumerate(labels):
        got = open(f"{out}.pk.{label}.narrowPeak", "rb").read()
        assert got.count(b"\n") == int(calls[i]["n_peaks"]), label
    if len(reps) == 1:
        assert open(f"{out}.pk.t1.narrowPeak", "rb").read() == narrow
    own = set(narrow.splitlines())
    for which in ("conservative", "optimal"):
        sel = open(f"{out}.pk.{which}.narrowPeak", "rb").read().splitlines()
        assert all(l in own for l in sel) and len(set(sel)) == len(sel), which
    rows = dict(l.split("\t") for l in metrics.decode().splitlines())
    assert len(open(f"{out}.pk.optimal.narrowPeak", "rb").read().splitlines()) == int(rows["optimal_peaks"])
    rep = [l for l in res.stderr.splitlines() if l.startswith("  Reproducibility")]
    assert len(rep) == len(calls) + 3 and all(f"Reproducibility, {lab}:" in l for lab, l in zip(labels, rep)), rep
    assert "verdict" in rep[-2] and "conservative set" in rep[-1]
    h.close()
