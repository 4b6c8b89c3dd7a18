"""Depth distribution (gx_set_depth_hist, k_depth_hist) at benchmark size: config 2 (hg38, 50 M fragments, -p 0.01).

  python tools/depth_bench.py [--frags N] [--steps K] [--warmup W] [--no-check]

In ONE run, per form of the sample, it reports the device time per sample of
  * the depth pass: the library's "depth" phase (HIP events on its stream, bracketing the zeroing of 48 KiB, k_depth_hist and
    the read-back of those 48 KiB; gx_set_phase_filter), in the default instance (an LDS atomic per piece) and with GX_DEPTH_PRIV=1
    (the pieces of whole depth 1 .. 4 summed in registers, one LDS atomic per class and wavefront: the contention measure);
  * the yardstick, the "cover" phase at N = 50 (the zeroing of the bins and k_cov_bins), which reads the same intervals;
each as min / median / max over K steps after a warm-up, the two switches on together, one phase timed per step.  The forms:
  loose    the benchmark's track, read in its loose slots;
  tight    the same with a one-base -E region: the first pass of gx_sample_end makes the tight arrays (k_pack) -- timed once
           inside "depth" (coverage off) and once outside it (coverage on: k_pack is k_cov_bins' then); the difference is k_pack;
  weighted the track with 10 % of its fragments multimapped (-s weights 1/k): the remainder adds are live.
It also times the step (reset, sample from device memory, find_peaks: bench.py's step) with the switch off and on, alternating,
and checks the loose and the weighted result at full size against numpy (tests/depth_ref.py's definition, from a difference
array per chromosome).  One JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def note(msg):
    print(f"[depth_bench] {msg}", file=sys.stderr, flush=True)


def mmm(xs):
    return dict(min=round(min(xs), 4), median=round(statistics.median(xs), 4), max=round(max(xs), 4), n=len(xs))


def numpy_hist(ev, lens, beds=None):
    """tests/depth_ref.py's Hist at full size: one difference array per chromosome (float64 sums of multiples of 1/120 below
    2^53: exact), the pileups counted by value."""
    import depth_ref as R
    ev = ev[np.argsort(ev["chrom"], kind="stable")]
    cuts = np.searchsorted(ev["chrom"], np.arange(len(lens) + 1))
    by_v = np.zeros(1, dtype=np.int64)
    total = excluded = 0
    for c in range(len(lens)):
        e = ev[cuts[c]:cuts[c + 1]]
        e = e[e["start"] < lens[c]]
        w = (120 // e["count"].astype(np.int64)).astype(np.float64)
        diff = np.bincount(e["start"], weights=w, minlength=lens[c] + 1)
        diff -= np.bincount(np.minimum(e["end"], lens[c]), weights=w, minlength=lens[c] + 1)
        pile = np.cumsum(diff)[:lens[c]].astype(np.int64)
        total += lens[c]
        for a, b in zip(*(np.asarray(beds[c] if beds else [], dtype=np.int64).reshape(-1, 2).T)):
            pile[a:b] = 0          # (counted at 0 here, taken out of the zeros below)
            excluded += int(min(b, lens[c]) - a)
        n = np.bincount(pile)
        if len(n) > len(by_v):
            by_v = np.concatenate([by_v, np.zeros(len(n) - len(by_v), dtype=np.int64)])
        by_v[:len(n)] += n
    v = np.flatnonzero(by_v)
    v = v[v > 0]
    bases, rsum, rsq = (np.zeros(R.DEPTH_BOUND, dtype=np.uint64) for _ in range(3))
    deep = []
    for x in v.tolist():
        d, r = divmod(x, 120)
        k = int(by_v[x])
        if d < R.DEPTH_BOUND:
            bases[d] += np.uint64(k)
            rsum[d] += np.uint64(r * k)
            rsq[d] += np.uint64(r * r * k)
        else:
            deep.append((x, k))
    covered = int(by_v[1:].sum())
    return R.Hist(0, False, total, excluded, total - excluded - covered, int(v[0]) if len(v) else 0, int(v[-1]) if len(v) else 0, bases, rsum, rsq, deep)


def run(frags, steps, warmup, check):
    import torch

    import bench
    import depth_ref as R
    from genrich_amd import synth
    from genrich_amd.lib import GX_PATH_DEPTH, Genrich, GxParams, minus_log10f

    cfg = dict(bench.CONFIGS[2])
    lens = synth.HG38_LENS
    (tv, _), = bench.build_workload(cfg, frags, lens)
    par = GxParams(minus_log10f(0.01), 0, 200.0, 0, 100, 0, 0)
    dev = torch.device("cuda:0")

    def upload(ev):
        d = torch.from_numpy(ev.view(np.uint32).reshape(-1, 4).copy()).to(dev)
        torch.cuda.synchronize()
        return d

    def make(beds=None, frac=False):
        gx = Genrich(par)
        gx.set_chroms(lens, None, beds)
        gx.set_keep_pileups(False)
        if frac:
            gx.expect_fractional(True)
        return gx

    def step(gx, d_ev, depth, W):
        gx.reset()
        gx.set_coverage_bins(W)
        gx.set_depth_hist(depth)
        gx.sample_begin(0, None)
        gx.push_events_device(d_ev.data_ptr(), d_ev.shape[0])
        gx.sample_end()
        gx.sample_no_control()
        gx.pvalues()
        return gx.find_peaks()

    def phase(gx, d_ev, name, depth=True, W=50):
        """device ms of the phase t.<name>, `steps` times after `warmup`"""
        for _ in range(warmup):
            step(gx, d_ev, depth, W)
        out = []
        for _ in range(steps):
            gx.set_phase_filter(name)
            step(gx, d_ev, depth, W)
            out.append([ms for n, ms in gx.phase_times() if n == "t." + name][-1])
            gx.set_phase_timing(0)
        return out

    def form(gx, d_ev):
        res = {}
        gx.set_knob("GX_DEPTH_PRIV", 0)
        res["depth_ms"] = mmm(phase(gx, d_ev, "depth"))
        res["cover50_ms"] = mmm(phase(gx, d_ev, "cover"))
        gx.set_knob("GX_DEPTH_PRIV", 1)
        res["depth_priv_ms"] = mmm(phase(gx, d_ev, "depth"))
        gx.set_knob("GX_DEPTH_PRIV", 0)
        res["depth_over_cover50"] = round(res["depth_ms"]["median"] / res["cover50_ms"]["median"], 3)
        res["priv_over_default"] = round(res["depth_priv_ms"]["median"] / res["depth_ms"]["median"], 3)
        return res

    out = dict(config=2, desc=cfg["desc"], fragments=frags)
    note("workload built")
    # loose slots
    d_tv = upload(tv)
    gx = make()
    out["loose"] = form(gx, d_tv)
    assert gx.path_info() & GX_PATH_DEPTH
    n_iv = gx.interval_total(0)
    out["loose"]["intervals"] = int(n_iv)
    out["loose"]["gb_per_s"] = round(8 * n_iv / (out["loose"]["depth_ms"]["median"] * 1e-3) / 1e9, 1)
    got = gx.depth(0)
    out["loose"]["list_capacity_reruns"] = list(gx.depth_last())
    t_off, t_on = [], []
    for i in range(2 * steps):
        t0 = time.perf_counter()
        step(gx, d_tv, i % 2 == 1, 0)
        (t_on if i % 2 else t_off).append((time.perf_counter() - t0) * 1e3)
    out["step_off_ms"], out["step_on_ms"] = mmm(t_off), mmm(t_on)
    out["added_on_pct"] = round(100.0 * (statistics.median(t_on) / statistics.median(t_off) - 1.0), 2)
    gx.close()
    note("loose form timed")
    if check:
        why = R.same(got, numpy_hist(tv, lens))
        assert why is None, why
        out["loose"]["checked_against_numpy"] = True
    m = R.metrics(got)
    out["loose"]["figures"] = dict(mean=round(m["mean"], 4), median=m["median"], covered_fraction=round(m["covered_fraction"], 4), max=m["max_v"] // 120,
                                   deep_entries=len(got.deep))
    # tight arrays: one excluded base on the last chromosome
    beds = [[] for _ in lens]
    beds[-1] = [lens[-1] - 1, lens[-1]]
    gx = make(beds)
    out["tight"] = form(gx, d_tv)
    alone = phase(gx, d_tv, "depth", True, 0)          # (coverage off: k_pack is inside "depth")
    out["tight"]["depth_with_k_pack_ms"] = mmm(alone)
    out["tight"]["k_pack_ms"] = round(statistics.median(alone) - out["tight"]["depth_ms"]["median"], 4)
    out["tight"]["depth_over_k_pack"] = round(out["tight"]["depth_ms"]["median"] / max(out["tight"]["k_pack_ms"], 1e-9), 3)
    gx.close()
    note("tight form timed")
    del d_tv
    # -s weights: 10 % of the fragments multimapped
    tw = synth.add_multimap(tv, lens, 0.10, seed=11)
    d_tw = upload(tw)
    gx = make(frac=True)
    out["weighted"] = form(gx, d_tw)
    got = gx.depth(0)
    assert got.rsum.any()
    out["weighted"]["intervals"] = int(gx.interval_total(0))
    gx.close()
    note("weighted form timed")
    if check:
        why = R.same(got, numpy_hist(tw, lens))
        assert why is None, why
        out["weighted"]["checked_against_numpy"] = True
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-check", action="store_true", help="skip the full-size comparison with numpy")
    a = ap.parse_args()
    print(json.dumps(run(a.frags, a.steps, a.warmup, not a.no_check)), flush=True)


if __name__ == "__main__":
    main()
