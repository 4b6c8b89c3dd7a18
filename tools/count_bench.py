"""Counting in peaks (gx_count_in_peaks) at benchmark size: config 2 (hg38, 50 M fragments, -p 0.01) and config 4 (ATAC cut
sites, -s weights).

  python tools/count_bench.py [--config 2|4] [--frags N] [--steps K] [--warmup W]

Per config it reports
  * the count pass: the library's "count" phase (HIP events on its stream, bracketing the upload of the peak tables, the
    kernels and the scan; gx_set_phase_filter), after a warm-up, and the host's wall time of the whole call (one read-back);
  * the step (reset, samples from device memory, find_peaks -- bench.py's step) with counting off and on, alternating
    in the same process, and the step followed by the count;
as min / median / max over K steps each, and checks one full-size count against numpy (tests/counts_ref.py).  One JSON line."""
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

import torch  # noqa: E402

import bench  # noqa: E402
import counts_ref as R  # noqa: E402
from genrich_amd import synth  # noqa: E402
from genrich_amd.lib import GX_PATH_COUNTS, Genrich, GxParams, minus_log10f  # noqa: E402


def mmm(xs):
    return dict(min=round(min(xs), 4), median=round(statistics.median(xs), 4), max=round(max(xs), 4), n=len(xs))


def run(config, frags, steps, warmup):
    cfg = dict(bench.CONFIGS[config])
    lens = synth.HG38_LENS
    reps = bench.build_workload(cfg, frags, lens)
    dev = torch.device("cuda:0")
    d_reps = [(torch.from_numpy(t.view(np.uint32).reshape(-1, 4).copy()).to(dev),
               None if c is None else torch.from_numpy(c.view(np.uint32).reshape(-1, 4).copy()).to(dev)) for t, c in reps]
    torch.cuda.synchronize()
    gx = Genrich(GxParams(minus_log10f(0.05 if cfg["qval"] else 0.01), int(cfg["qval"]), 200.0, 0, 100, 0, 0))
    gx.set_chroms(lens)
    gx.set_keep_pileups(False)
    if cfg["multimap"]:
        gx.expect_fractional(True)

    def step(count):
        gx.reset()
        gx.set_count_in_peaks(count)
        for d_tv, d_cv in d_reps:
            gx.sample_begin(0, None)
            gx.push_events_device(d_tv.data_ptr(), d_tv.shape[0])
            gx.sample_end()
            if d_cv is not None:
                gx.sample_begin(1, None)
                gx.push_events_device(d_cv.data_ptr(), d_cv.shape[0])
                gx.sample_end()
            else:
                gx.sample_no_control()
            gx.pvalues()
        return gx.find_peaks()

    for _ in range(warmup):
        step(False)
        step(True)
        gx.count_in_peaks()
    t_off, t_on, t_on_count, t_call, t_dev = [], [], [], [], []
    flags = {}
    for i in range(2 * steps):
        on = i % 2 == 1
        t0 = time.perf_counter()
        step(on)
        t1 = time.perf_counter()
        flags[on] = gx.path_info()
        if not on:
            t_off.append((t1 - t0) * 1e3)
            continue
        t_on.append((t1 - t0) * 1e3)
        gx.set_phase_filter("count")
        t2 = time.perf_counter()
        gx.count_in_peaks()
        t3 = time.perf_counter()
        gx.set_phase_timing(0)
        t_call.append((t3 - t2) * 1e3)
        t_on_count.append((t3 - t0) * 1e3)
        t_dev.append([ms for name, ms in gx.phase_times() if name == "count"][-1])
    # one full-size check against numpy
    n = gx.count_in_peaks()
    pk = gx.get_peaks()
    samples = [ev for t, c in reps for ev in (t, c) if ev is not None]
    assert n == len(samples)
    for k, ev in enumerate(samples):
        got = gx.peak_counts(k)
        cnt, tot, inp = R.count_in_peaks(ev["chrom"], ev["start"], ev["end"], R.weights(ev["count"]), pk["chrom"], pk["start"], pk["end"])
        assert got.total == tot and got.in_peaks == inp and np.array_equal(got.count, cnt), k
    med_off = statistics.median(t_off)
    out = dict(config=config, desc=cfg["desc"], fragments=frags, intervals=int(sum(len(e) for e in samples)), peaks=int(len(pk)),
               count_pass_device_ms=mmm(t_dev), count_call_wall_ms=mmm(t_call),
               step_off_ms=mmm(t_off), step_on_ms=mmm(t_on), step_on_plus_count_ms=mmm(t_on_count),
               added_on_pct=round(100.0 * (statistics.median(t_on) / med_off - 1.0), 2),
               added_on_plus_count_pct=round(100.0 * (statistics.median(t_on_count) / med_off - 1.0), 2),
               frip=[round(gx.peak_counts(k).in_peaks / max(1, gx.peak_counts(k).total), 4) for k in range(n)],
               path_off=flags[False], path_on=flags[True], counts_bit_on=bool(flags[True] & GX_PATH_COUNTS),
               checked_against_numpy=True)
    gx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=0, help="2 or 4 (default: both)")
    ap.add_argument("--frags", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    for c in ([a.config] if a.config else [2, 4]):
        print(json.dumps(run(c, a.frags, a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
