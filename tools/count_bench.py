"""Counting in peaks (gx_count_in_peaks) at benchmark size: config 2 (hg38, 50 M fragments, -p 0.01) and config 4 (ATAC cut
sites, -s weights).

  python tools/count_bench.py [--config 2|4] [--frags N] [--steps K] [--warmup W] [--regions]

Per config it reports
  * the count pass: the library's "count" phase (HIP events on its stream, bracketing the upload of the peak tables, the
    kernels and the scan; gx_set_phase_filter), after a warm-up, and the host's wall time of the whole call (one read-back);
  * the step (reset, samples from device memory, find_peaks -- bench.py's step) with counting off and on, alternating
    in the same process, and the step followed by the count;
as min / median / max over K steps each, and checks one full-size count against numpy (tests/counts_ref.py).  One JSON line.

--regions: counting in a given region set (gx_count_in_regions) on the same kept events instead: the run's own peaks as regions
(next to gx_count_in_peaks on the same peaks, the yardstick, in the same process), every 3rd and every 10th of them, and
genome-wide 1-kb bins; per set the
library's "regions" phase (the upload of the region tables, the kernels, the scans), the host's wall time of the whole call (it
also sorts the regions) and a full-size check (the peaks against gx_count_in_peaks, the bins against numpy).  One JSON line."""
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


def setup(config, frags):
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

    return cfg, lens, reps, gx, step


def run(config, frags, steps, warmup):
    cfg, lens, reps, gx, step = setup(config, frags)
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


def timed(gx, phase, call, steps, warmup):
    """-> (device ms of `phase`, wall ms of call()) over `steps` calls after `warmup`"""
    for _ in range(warmup):
        call()
    dev, wall = [], []
    for _ in range(steps):
        gx.set_phase_filter(phase)
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        gx.set_phase_timing(0)
        wall.append((t1 - t0) * 1e3)
        dev.append([ms for name, ms in gx.phase_times() if name == phase][-1])
    return mmm(dev), mmm(wall)


def run_regions(config, frags, steps, warmup):
    from genrich_amd.lib import REGION_DTYPE
    cfg, lens, reps, gx, step = setup(config, frags)
    step(True)
    pk = gx.get_peaks()
    samples = [ev for t, c in reps for ev in (t, c) if ev is not None]
    peaks = np.zeros(len(pk), dtype=REGION_DTYPE)
    for f in ("chrom", "start", "end"):
        peaks[f] = pk[f]
    bins = np.concatenate([np.stack([np.full((n + 999) // 1000, c), np.arange(0, n, 1000), np.arange(0, n, 1000) + 1000], axis=1)
                           for c, n in enumerate(lens)])
    reg_bins = np.zeros(len(bins), dtype=REGION_DTYPE)
    reg_bins["chrom"], reg_bins["start"], reg_bins["end"] = bins[:, 0], bins[:, 1], bins[:, 2]
    out = dict(config=config, desc=cfg["desc"], fragments=frags, intervals=int(sum(len(e) for e in samples)), mode="regions")
    d, w = timed(gx, "count", gx.count_in_peaks, steps, warmup)
    out["peaks_by_count_in_peaks"] = dict(regions=int(len(pk)), device_ms=d, call_wall_ms=w)
    d, w = timed(gx, "regions", lambda: gx.count_in_regions(peaks), steps, warmup)
    out["peaks_as_regions"] = dict(regions=int(len(pk)), device_ms=d, call_wall_ms=w)
    out["peaks_as_regions"]["device_ratio_to_count_in_peaks"] = round(d["median"] / out["peaks_by_count_in_peaks"]["device_ms"]["median"], 3)
    for k in range(len(samples)):
        a, b = gx.peak_counts(k), gx.region_counts(k)
        assert a.count.tobytes() == b.count.tobytes() and (a.total, a.in_peaks) == (b.total, b.in_regions), k
    for every in (3, 10):   # smaller sets (fewer histogram entries, more adds per entry): every 3rd / 10th peak
        sub = np.ascontiguousarray(peaks[::every])
        d, w = timed(gx, "regions", lambda: gx.count_in_regions(sub), steps, warmup)
        out[f"every_{every}th_peak"] = dict(regions=int(len(sub)), device_ms=d, call_wall_ms=w)
        for k in range(len(samples)):
            assert np.array_equal(gx.peak_counts(k).count[::every], gx.region_counts(k).count), (every, k)
    d, w = timed(gx, "regions", lambda: gx.count_in_regions(reg_bins), steps, warmup)
    out["bins_1kb"] = dict(regions=int(len(reg_bins)), device_ms=d, call_wall_ms=w)
    lens_a = np.asarray(lens, dtype=np.int64)
    base = np.concatenate([[0], np.cumsum((lens_a + 999) // 1000)])[:-1]
    for k, ev in enumerate(samples):   # bin b of a chromosome holds the intervals with s // 1000 <= b <= (e - 1) // 1000
        got = gx.region_counts(k)
        c, s0 = ev["chrom"].astype(np.int64), ev["start"].astype(np.int64)
        e0 = np.minimum(ev["end"].astype(np.int64), lens_a[c])
        assert (e0 > s0).all()
        wgt = R.weights(ev["count"]).astype(np.float64)      # (sums below 2^53: exact)
        diff = np.bincount(base[c] + s0 // 1000, weights=wgt, minlength=len(reg_bins) + 1)
        diff -= np.bincount(base[c] + (e0 - 1) // 1000 + 1, weights=wgt, minlength=len(reg_bins) + 1)
        cnt = np.cumsum(diff)[:-1].astype(np.int64)
        assert got.total == int(wgt.sum()) == got.in_regions and np.array_equal(got.count, cnt), k
    out["checked"] = True
    out["path"] = gx.path_info()
    gx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=0, help="2 or 4 (default: both)")
    ap.add_argument("--frags", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--regions", action="store_true", help="gx_count_in_regions: the run's peaks as regions, and 1-kb bins")
    a = ap.parse_args()
    for c in ([a.config] if a.config else [2, 4]):
        print(json.dumps((run_regions if a.regions else run)(c, a.frags, a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
