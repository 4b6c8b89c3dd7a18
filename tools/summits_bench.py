"""The summits of the pooled treatment depth inside the peaks (gx_peak_summits) at benchmark size: config 2 (hg38, 50 M
fragments, -p 0.01), next to gx_peak_signal in the same process -- the yardstick: the same staging, the same scatter, and
k_psig_reduce reads the bytes that are k_summits' floor.

  python tools/summits_bench.py [--config 2|4] [--frags N] [--steps K] [--warmup W] [--check-chroms C]
  python tools/summits_bench.py --summarise KERNEL_STATS_CSV

It shares the set-up and the timing loop with tools/count_bench.py and reports
  * the library's "summits" phase (HIP events on its stream: the upload of the peak tables, k_cnt_index, the clear of the peak
    space, one k_psig_scatter per treatment, k_summits, the read of its control words) and the host's wall time of the whole
    call (the list read back and sorted);
  * the same two figures of gx_peak_signal ("peaksig"), and the ratio;
  * the summits: how many, the peaks with more than one, the most in a peak, the second launch's peaks, the list's reruns;
  * a constructed worst case through gx_peak_summits_events: sawtooth peaks of equal teeth, every base a run, so that every
    tooth's walk crosses its whole peak (n / 64 rounds of a wavefront of up to 2 (128 + n / 64) steps each for n runs) --
    `--saw-peaks` peaks of RUN_CAP runs
    (in LDS) and of RUN_CAP + 1 runs (the second launch, in HBM), and one peak of `--saw-long` runs;
as min / median / max over K calls each, and checks the summits of the C shortest chromosomes against numpy
(tests/summits_ref.py) at full size.  One JSON line.

The kernels one by one (k_summits, k_psig_reduce, k_psig_scatter, the clears): the same run under
`rocprofv3 --kernel-trace --stats`, in a run of its own; --summarise prints their rows of its kernel_stats CSV."""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def sawtooth_case(n_peaks, runs, first=1000, gap=16):
    """n_peaks peaks of `runs` bases, depth 12 and 24 in turn: (chromosome length, peaks, events)"""
    import summits_cases as K
    peaks, rows, pos = [], [], first
    odd = np.arange(1, runs, 2)
    for _ in range(n_peaks):
        peaks.append((0, pos, pos + runs))
        rows.append(np.array([[0, pos, pos + runs, 10]], dtype=np.int64))
        rows.append(np.stack([np.zeros_like(odd), pos + odd, pos + odd + 1, np.full_like(odd, 10)], axis=1))
        pos += runs + gap
    return pos + 1000, peaks, K.events(np.concatenate(rows))


def worst_cases(gx_factory, saw_peaks, saw_long, steps, warmup):
    import count_bench as CB
    from genrich_amd.lib import peak_summits_geometry
    run_cap = peak_summits_geometry()[3]
    out = {}
    for label, n_peaks, runs in (("lds_at_run_cap", saw_peaks, run_cap), ("hbm_beyond_run_cap", saw_peaks, run_cap + 1), ("hbm_one_long_peak", 1, saw_long)):
        length, peaks, ev = sawtooth_case(n_peaks, runs)
        gx = gx_factory([length])
        dev, wall, n = [], [], 0
        for it in range(warmup + steps):
            gx.set_phase_filter("summits")
            t0 = time.perf_counter()
            n = len(gx.peak_summits_events(ev, peaks))
            t1 = time.perf_counter()
            gx.set_phase_timing(0)
            if it >= warmup:
                wall.append((t1 - t0) * 1e3)
                dev.append([ms for name, ms in gx.phase_times() if name == "summits"][-1])
        assert n == n_peaks * (runs // 2), (label, n)
        out[label] = dict(peaks=n_peaks, runs_per_peak=runs, events=int(len(ev)), summits=n, second_launch_peaks=gx.peak_summits_last()[1],
                          device_ms=CB.mmm(dev), call_wall_ms=CB.mmm(wall),
                          wavefront_walk_steps_bound=int(n_peaks * ((runs + 63) // 64) * 2 * (128 + runs // 64)))
        gx.close()
    return out


def run(config, frags, steps, warmup, check_chroms, saw_peaks, saw_long):
    import count_bench as CB
    import summits_ref as R
    from genrich_amd.lib import Genrich, GxParams, minus_log10f, peak_signal_geometry

    cfg, lens, reps, gx, step = CB.setup(config, frags)
    step(True)
    pk = gx.get_peaks()
    treatments = [t for t, c in reps]
    d_sig, w_sig = CB.timed(gx, "peaksig", gx.peak_signal, steps, warmup)
    d_sum, w_sum = CB.timed(gx, "summits", gx.peak_summits, steps, warmup)
    sm = gx.peak_summits()
    reruns, big = gx.peak_summits_last()
    per = np.bincount(sm["peak"], minlength=len(pk))
    pad = peak_signal_geometry()[3]
    plen = pk["end"].astype(np.int64) - pk["start"].astype(np.int64)
    slots = int(((plen + pad - 1) // pad * pad).sum())
    out = dict(config=config, desc=cfg["desc"], fragments=frags, treatments=len(treatments), samples=sum(1 + (c is not None) for t, c in reps),
               peaks=int(len(pk)), peak_bp=int(plen.sum()), peak_space_bytes=4 * slots,
               summits=int(len(sm)), peaks_with_more_than_one=int((per > 1).sum()), most_in_a_peak=int(per.max()) if len(per) else 0,
               peaks_without_pooled_depth=int((per == 0).sum()), second_launch_peaks=int(big), list_reruns=int(reruns),
               summits_device_ms=d_sum, summits_call_wall_ms=w_sum, peaksig_device_ms=d_sig, peaksig_call_wall_ms=w_sig,
               device_ratio_to_peaksig=round(d_sum["median"] / d_sig["median"], 3), wall_ratio_to_peaksig=round(w_sum["median"] / w_sig["median"], 3))
    chroms = sorted(range(len(lens)), key=lambda c: lens[c])[:check_chroms]
    sel = np.flatnonzero(np.isin(pk["chrom"], chroms))
    if len(sel):
        peaks = np.stack([pk["chrom"], pk["start"], pk["end"]], axis=1).astype(np.int64)[sel]
        exp = R.summits([t[np.isin(t["chrom"], chroms)] for t in treatments], lens, peaks)
        got = sm[np.isin(sm["peak"], sel)].copy()
        got["peak"] = np.searchsorted(sel, got["peak"])
        assert R.same(got, exp) is None, R.same(got, exp)
    out["checked_against_numpy"] = dict(chromosomes=len(chroms), peaks=int(len(sel)))
    gx.close()

    def factory(lens1):
        g = Genrich(GxParams(minus_log10f(0.01), 0, 200.0, 0, 100, 0, 0))
        g.set_chroms(lens1)
        return g
    out["sawtooth"] = worst_cases(factory, saw_peaks, saw_long, steps, warmup)
    return out


def summarise(path):
    """the rows of a rocprofv3 kernel_stats CSV that belong to the two passes"""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    for r in rows:
        name = r.get("Name") or r.get("name") or ""
        if any(k in name for k in ("k_summits", "k_psig", "k_cnt_index", "fillBuffer")):
            print("\t".join(f"{k}={v}" for k, v in r.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2, help="2 (the benchmark's 50 M hg38 fragments) or 4")
    ap.add_argument("--frags", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check-chroms", type=int, default=3, help="the shortest chromosomes whose summits are compared with numpy (0: none)")
    ap.add_argument("--saw-peaks", type=int, default=256, help="sawtooth peaks at and just beyond the run capacity")
    ap.add_argument("--saw-long", type=int, default=16384, help="runs of the one long sawtooth peak")
    ap.add_argument("--summarise", metavar="CSV", default=None, help="a rocprofv3 --kernel-trace --stats kernel_stats CSV of a run of this tool")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise)
        return
    print(json.dumps(run(a.config, a.frags, a.steps, a.warmup, a.check_chroms, a.saw_peaks, a.saw_long)), flush=True)


if __name__ == "__main__":
    main()
