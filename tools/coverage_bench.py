"""Binned coverage (gx_set_coverage_bins, k_cov_bins) at benchmark size: config 2 (hg38, 50 M fragments, -p 0.01).

  python tools/coverage_bench.py [--frags N] [--steps K] [--warmup W] [--bins 10,50,200] [--plan FILE]
  python tools/coverage_bench.py --summarise KERNEL_TRACE.csv --plan FILE

Per bin size W it reports
  * the pass's device time per sample: the library's "cover" phase (HIP events on its stream, bracketing the zeroing of the
    bins and k_cov_bins; gx_set_phase_filter) after a warm-up, as min / median / max over K steps;
  * the bytes moved -- 8 B per interval read + 8 B per bin written + 8 B per bin zeroed -- and the TB/s that makes;
  * the step (reset, sample from device memory, find_peaks: bench.py's step) with the switch off and on, alternating in the
    same process;
and checks one full-size result per W against numpy (tests/coverage_ref.py's definition, from a difference array per
chromosome).  Then the yardstick: the same sample with a one-base -E region, where gx_sample_end makes the tight arrays
(k_pack: the same slots, the same tile walk, 8 B read + 8 B written per interval) ahead of k_cov_bins.  One JSON line.

Under `rocprofv3 --kernel-trace` the same run yields every launch of k_cov_bins and k_pack; --plan FILE writes the order of
the k_cov_bins launches (W, form) and the byte counts, and --summarise reads the trace's CSV with that plan: median of the last
five launches of each kind, ns per byte moved, k_pack's run-to-run spread.  One JSON line."""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def mmm(xs):
    return dict(min=round(min(xs), 4), median=round(statistics.median(xs), 4), max=round(max(xs), 4), n=len(xs))


def numpy_bins(ev, lens, bin_sizes, beds=None, only=None):
    """{W: {chrom: int64 bins}}: tests/coverage_ref.py's definition at full size, one difference array per chromosome for all
    the bin sizes (float64 sums of multiples of 1/120 below 2^53: exact)."""
    import coverage_ref as R
    ev = ev[np.argsort(ev["chrom"], kind="stable")]
    cuts = np.searchsorted(ev["chrom"], np.arange(len(lens) + 1))
    out = {W: {} for W in bin_sizes}
    for c in (range(len(lens)) if only is None else only):
        e = ev[cuts[c]:cuts[c + 1]]
        e = e[e["start"] < lens[c]]
        w = (120 // e["count"].astype(np.int64)).astype(np.float64)
        diff = np.bincount(e["start"], weights=w, minlength=lens[c] + 1)
        diff -= np.bincount(np.minimum(e["end"], lens[c]), weights=w, minlength=lens[c] + 1)
        pile = np.cumsum(diff)[:lens[c]].astype(np.int64)
        for a, b in zip(*(np.asarray(beds[c] if beds else [], dtype=np.int64).reshape(-1, 2).T)):
            pile[a:b] = 0
        for W in bin_sizes:
            out[W][c] = R.bin_sums(pile, W)
    return out


def run(frags, steps, warmup, bin_sizes, plan_path):
    import torch

    import bench
    from genrich_amd import synth
    from genrich_amd.lib import GX_PATH_COVERAGE, Genrich, GxParams, minus_log10f

    cfg = dict(bench.CONFIGS[2])
    lens = synth.HG38_LENS
    (tv, _), = bench.build_workload(cfg, frags, lens)
    d_tv = torch.from_numpy(tv.view(np.uint32).reshape(-1, 4).copy()).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    par = GxParams(minus_log10f(0.01), 0, 200.0, 0, 100, 0, 0)

    def make(beds=None):
        gx = Genrich(par)
        gx.set_chroms(lens, None, beds)
        gx.set_keep_pileups(False)
        return gx

    def step(gx, W):
        gx.reset()
        gx.set_coverage_bins(W)
        gx.sample_begin(0, None)
        gx.push_events_device(d_tv.data_ptr(), d_tv.shape[0])
        gx.sample_end()
        gx.sample_no_control()
        gx.pvalues()
        return gx.find_peaks()

    def measure(gx, W):
        for _ in range(warmup):
            step(gx, 0)
            step(gx, W)
        t_off, t_on, t_dev = [], [], []
        for i in range(2 * steps):
            on = i % 2 == 1
            if on:
                gx.set_phase_filter("cover")
            t0 = time.perf_counter()
            step(gx, W if on else 0)
            t1 = time.perf_counter()
            if on:
                t_dev.append([ms for name, ms in gx.phase_times() if name == "t.cover"][-1])
                gx.set_phase_timing(0)
            (t_on if on else t_off).append((t1 - t0) * 1e3)
        return t_off, t_on, t_dev

    out = dict(config=2, desc=cfg["desc"], fragments=frags, bins={})
    plan = []
    gx = make()
    exp_all = numpy_bins(tv, lens, bin_sizes)
    for W in bin_sizes:
        t_off, t_on, t_dev = measure(gx, W)
        plan += [dict(W=W, form="loose")] * (warmup + steps)
        assert gx.path_info() & GX_PATH_COVERAGE
        n_iv = gx.interval_total(0)
        n_bins = sum(gx.coverage_bin_count(c) for c in range(len(lens)))
        for c in range(len(lens)):
            assert np.array_equal(gx.coverage(0, c).sum120, exp_all[W][c]), (W, c)
        moved = 8 * n_iv + 16 * n_bins
        med = statistics.median(t_dev)
        out["bins"][str(W)] = dict(intervals=int(n_iv), n_bins=int(n_bins), bytes_moved=int(moved), cover_device_ms=mmm(t_dev),
                                   tb_per_s=round(moved / (med * 1e-3) / 1e12, 3), step_off_ms=mmm(t_off), step_on_ms=mmm(t_on),
                                   added_on_pct=round(100.0 * (statistics.median(t_on) / statistics.median(t_off) - 1.0), 2),
                                   checked_against_numpy=True)
    gx.close()
    # the yardstick's run: one excluded base on the last chromosome -> tight arrays (k_pack), then k_cov_bins on them
    beds = [[] for _ in lens]
    beds[-1] = [lens[-1] - 1, lens[-1]]
    gx = make(beds)
    W = 50 if 50 in bin_sizes else bin_sizes[0]
    t_off, t_on, t_dev = measure(gx, W)
    plan += [dict(W=W, form="tight")] * (warmup + steps)
    n_iv = gx.interval_total(0)
    n_bins = sum(gx.coverage_bin_count(c) for c in range(len(lens)))
    last = len(lens) - 1
    exp_all[W][last] = numpy_bins(tv, lens, [W], beds, only=[last])[W][last]
    for c in range(len(lens)):
        assert np.array_equal(gx.coverage(0, c).sum120, exp_all[W][c]), ("tight", c)
    out["with_one_excluded_base"] = dict(W=W, intervals=int(n_iv), n_bins=int(n_bins), cover_device_ms_with_k_pack=mmm(t_dev),
                                        k_pack_bytes=int(16 * n_iv), checked_against_numpy=True)
    gx.close()
    if plan_path:
        sizes = {k: dict(intervals=v["intervals"], n_bins=v["n_bins"]) for k, v in out["bins"].items()}
        json.dump(dict(launches=plan, sizes=sizes, tight=dict(intervals=int(n_iv), n_bins=int(n_bins)), last=steps), open(plan_path, "w"))
    return out


def summarise(trace_csv, plan_path):
    plan = json.load(open(plan_path))
    rows = list(csv.DictReader(open(trace_csv)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6   # ms
    cov = [dur(r) for r in rows if "k_cov_bins" in r["Kernel_Name"]]
    pack = [dur(r) for r in rows if "k_pack(" in r["Kernel_Name"] or r["Kernel_Name"].endswith("k_pack")]
    assert len(cov) == len(plan["launches"]), (len(cov), len(plan["launches"]))
    last = min(5, plan["last"])
    out = dict(k_cov_bins={}, launches=len(cov))
    by = {}
    for ms, l in zip(cov, plan["launches"]):
        by.setdefault((l["W"], l["form"]), []).append(ms)
    for (W, form), xs in by.items():
        sz = plan["tight"] if form == "tight" else plan["sizes"][str(W)]
        kernel_bytes = 8 * sz["intervals"] + 8 * sz["n_bins"]   # (the zeroing is a fill of its own: not in this kernel's time)
        med = statistics.median(xs[-last:])
        out["k_cov_bins"][f"{W}/{form}"] = dict(ms=mmm(xs[-last:]), kernel_bytes=kernel_bytes, ns_per_kb=round(med * 1e6 / (kernel_bytes / 1e3), 4),
                                                tb_per_s=round(kernel_bytes / (med * 1e-3) / 1e12, 3))
    if pack:
        xs = pack[-last:]
        b = 16 * plan["tight"]["intervals"]
        med = statistics.median(xs)
        out["k_pack"] = dict(ms=mmm(xs), bytes=b, ns_per_kb=round(med * 1e6 / (b / 1e3), 4), tb_per_s=round(b / (med * 1e-3) / 1e12, 3),
                             spread_pct=round(100.0 * (max(xs) - min(xs)) / med, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bins", default="10,50,200")
    ap.add_argument("--plan", default=None, help="write the order of the k_cov_bins launches here (for --summarise)")
    ap.add_argument("--summarise", metavar="CSV", default=None, help="a rocprofv3 kernel trace of a run made with --plan")
    a = ap.parse_args()
    if a.summarise:
        print(json.dumps(summarise(a.summarise, a.plan)), flush=True)
    else:
        print(json.dumps(run(a.frags, a.steps, a.warmup, [int(x) for x in a.bins.split(",")], a.plan)), flush=True)


if __name__ == "__main__":
    main()
