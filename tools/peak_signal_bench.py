"""Each sample's signal inside the peaks (gx_peak_signal) at benchmark size: config 2 (hg38, 50 M fragments, -p 0.01), next to the
count pass (gx_count_in_peaks) in the same process -- the yardstick: it reads the same events and makes the same peak search.

  python tools/peak_signal_bench.py [--config 2|4] [--frags N] [--steps K] [--warmup W] [--check-chroms C]
  python tools/peak_signal_bench.py --summarise KERNEL_STATS_CSV

It shares the set-up, the step and the timing loop with tools/count_bench.py and reports
  * the library's "peaksig" phase (HIP events on its stream: the upload of the peak tables, k_cnt_index, and per sample the
    clear of the peak space, k_psig_scatter and k_psig_reduce) and the host's wall time of the whole call (one read-back);
  * the same two figures of the count pass ("count": k_cnt_index, k_cnt_count per sample, k_cnt_scan), and the ratio;
  * the peak space (slots, bytes) and the bytes a sample moves: its events read once, the space cleared once and read once,
    two 4-byte atomic adds per interval end that falls into a peak, one 32-byte record per peak;
as min / median / max over K calls each, and checks the figures of the C shortest chromosomes against numpy
(tests/peaksig_ref.py) at full size.  One JSON line.

The kernels one by one (k_psig_scatter, k_psig_reduce, the clears, k_cnt_count, k_cnt_index, k_cnt_scan): the same run under
`rocprofv3 --kernel-trace --stats`, in a run of its own; --summarise prints their rows of its kernel_stats CSV."""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def run(config, frags, steps, warmup, check_chroms):
    import count_bench as CB
    import peaksig_ref as R
    from genrich_amd.lib import peak_signal_geometry

    cfg, lens, reps, gx, step = CB.setup(config, frags)
    step(True)
    pk = gx.get_peaks()
    samples = [ev for t, c in reps for ev in (t, c) if ev is not None]
    d_cnt, w_cnt = CB.timed(gx, "count", gx.count_in_peaks, steps, warmup)
    d_sig, w_sig = CB.timed(gx, "peaksig", gx.peak_signal, steps, warmup)
    pad = peak_signal_geometry()[3]
    plen = pk["end"].astype(np.int64) - pk["start"].astype(np.int64)
    slots = int(((plen + pad - 1) // pad * pad).sum())
    n_ev = int(sum(len(e) for e in samples))
    in_peaks = int(sum(gx.peak_counts(k).in_peaks for k in range(len(samples))))
    total = int(sum(gx.peak_counts(k).total for k in range(len(samples))))
    moved = 16 * n_ev + 2 * 4 * slots + 32 * len(pk) * len(samples)
    out = dict(config=config, desc=cfg["desc"], fragments=frags, intervals=n_ev, samples=len(samples), peaks=int(len(pk)),
               peak_bp=int(plen.sum()), peak_space_slots=slots, peak_space_bytes=4 * slots,
               peaksig_device_ms=d_sig, peaksig_call_wall_ms=w_sig, count_device_ms=d_cnt, count_call_wall_ms=w_cnt,
               device_ratio_to_count=round(d_sig["median"] / d_cnt["median"], 3),
               wall_ratio_to_count=round(w_sig["median"] / w_cnt["median"], 3),
               bytes_events_read=16 * n_ev, bytes_space_cleared_and_read=2 * 4 * slots, bytes_records=32 * int(len(pk)) * len(samples),
               bytes_moved_without_atomics=moved, fraction_of_weight_in_peaks=round(in_peaks / max(1, total), 4),
               gb_per_s_of_moved_bytes=round(moved / (d_sig["median"] * 1e-3) / 1e9, 1))
    # the figures of the shortest chromosomes against numpy, at full size
    chroms = sorted(range(len(lens)), key=lambda c: lens[c])[:check_chroms]
    sel = np.isin(pk["chrom"], chroms)
    if sel.any():
        peaks = np.stack([pk["chrom"], pk["start"], pk["end"]], axis=1).astype(np.int64)[sel]
        for k, ev in enumerate(samples):
            got = gx.peak_signal_of(k)
            exp = R.signal(ev[np.isin(ev["chrom"], chroms)], lens, peaks, pk["summit"].astype(np.int64)[sel])
            got = R.Signal(*[np.asarray(x)[sel] for x in got[:5]])
            assert R.same(got, exp) is None, (k, R.same(got, exp))
    out["checked_against_numpy"] = dict(chromosomes=len(chroms), peaks=int(sel.sum()))
    gx.close()
    return out


def summarise(path):
    """the rows of a rocprofv3 kernel_stats CSV that belong to the two passes"""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    for r in rows:
        name = r.get("Name") or r.get("name") or ""
        if any(k in name for k in ("k_psig", "k_cnt_", "fillBuffer")):
            print("\t".join(f"{k}={v}" for k, v in r.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2, help="2 (the benchmark's 50 M hg38 fragments) or 4")
    ap.add_argument("--frags", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check-chroms", type=int, default=3, help="the shortest chromosomes whose figures are compared with numpy (0: none)")
    ap.add_argument("--summarise", metavar="CSV", default=None, help="a rocprofv3 --kernel-trace --stats kernel_stats CSV of a run of this tool")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise)
        return
    print(json.dumps(run(a.config, a.frags, a.steps, a.warmup, a.check_chroms)), flush=True)


if __name__ == "__main__":
    main()
