"""Interval lengths and chromosome tallies (gx_interval_stats) at benchmark size: config 2's workload (hg38, 50 M fragments), and
the same fragments once more with every length made equal, so that every wavefront takes the one-lane path for its lengths,
and once more ordered by chromosome, so that a wavefront's chromosome tallies stay in registers (config 2 itself comes in no
order: nearly every wavefront holds several chromosomes and tallies them per lane).

  python tools/lengths_bench.py [--frags N] [--steps K] [--warmup W] [--out FILE]

It reports, per workload, as min / median / max over K calls after a warm-up,
  * the pass ("ivstat": the counters cleared and k_ivstat; HIP events on the library's stream, gx_set_phase_timing(2)) and the
    host's wall time of the whole gx_interval_stats call (staging, the kernel, the read-back, the merged list, the three sums);
  * on the same kept events in the same run the library's "count" phase (gx_count_in_peaks) and the "subsample" phase of
    gx_subsample_kept at 100 % (--saturation's pass: the nearest pure streaming pass, it reads every event and writes it again);
  * each per GB of events read (16 bytes an event) and the ratios.
The lengths and the tallies are checked at full size against numpy (bincount).  One JSON line per workload; --out also writes a
text table."""
from __future__ import annotations

import argparse
import ctypes as C
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
from genrich_amd import synth  # noqa: E402
from genrich_amd.lib import GX_PATH_IVSTAT, Genrich, GxParams, minus_log10f  # noqa: E402


def mmm(xs):
    return dict(min=round(min(xs), 4), median=round(statistics.median(xs), 4), max=round(max(xs), 4), n=len(xs))


def numpy_stats(ev, lens):
    """([(L, n, w120)], cn, cw120, cbases120) of events that are all intervals with a length (checked), by bincount."""
    lens_a = np.asarray(lens, dtype=np.int64)
    c = ev["chrom"].astype(np.int64)
    s, e = ev["start"].astype(np.int64), np.minimum(ev["end"].astype(np.int64), lens_a[c])
    assert np.isin(ev["count"], (1, 2, 3, 4, 5, 6, 8, 10)).all() and (s < lens_a[c]).all() and (e >= s).all()
    L, w = e - s, 120 // ev["count"].astype(np.int64)
    n_l = np.bincount(L)
    w_l = np.bincount(L, weights=w).astype(np.int64)            # (integers below 2^53: exact)
    at = np.nonzero(n_l)[0]
    nc = len(lens)
    return (list(zip(at.tolist(), n_l[at].tolist(), w_l[at].tolist())), np.bincount(c, minlength=nc).tolist(),
            np.bincount(c, weights=w, minlength=nc).astype(np.int64).tolist(), np.bincount(c, weights=w * L, minlength=nc).astype(np.int64).tolist())


def run(name, ev, lens, frags, steps, warmup):
    d_ev = torch.from_numpy(ev.view(np.uint32).reshape(-1, 4).copy()).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    gx = Genrich(GxParams(minus_log10f(0.01), 0, 200.0, 0, 100, 0, 0))
    gx.set_chroms(lens)
    gx.set_keep_pileups(False)
    gx.set_count_in_peaks(True)
    gx.sample_begin(0, None)
    gx.push_events_device(d_ev.data_ptr(), d_ev.shape[0])
    gx.sample_end()
    gx.sample_no_control()
    gx.pvalues()
    gx.find_peaks()
    n_out = C.c_size_t(0)

    def subsample_all():
        gx._check(gx.lib.gx_subsample_kept(gx.ctx, 0, 1, 1 << 32, None, 0, C.byref(n_out)))
    for _ in range(warmup):
        gx.interval_stats()
        gx.count_in_peaks()
        subsample_all()
    t_ivs, t_wall, t_cnt, t_sub = [], [], [], []
    for _ in range(steps):
        gx.set_phase_timing(2)
        t0 = time.perf_counter()
        gx.interval_stats()
        t1 = time.perf_counter()
        gx.count_in_peaks()
        subsample_all()
        gx.set_phase_timing(0)
        ph = gx.phase_times()
        t_ivs.append([ms for nm, ms in ph if nm == "ivstat"][-1])
        t_cnt.append([ms for nm, ms in ph if nm == "count"][-1])
        t_sub.append([ms for nm, ms in ph if nm == "subsample"][-1])
        t_wall.append((t1 - t0) * 1e3)
    assert n_out.value == len(ev)
    got = gx.get_interval_stats(0)
    lengths, cn, cw, cb = numpy_stats(ev, lens)
    assert got.lengths == lengths and (got.n_inverted, got.w120_inverted) == (0, 0) and (got.cn, got.cw120, got.cbases120) == (cn, cw, cb)
    nbytes = 16 * len(ev)
    med = statistics.median
    per_gb = lambda ms: round(ms / (nbytes / 1e9), 4)
    out = dict(workload=name, fragments=frags, events=len(ev), classes=len(lengths), longest=lengths[-1][0], list_capacity=gx.interval_stats_last()[0],
               reruns=gx.interval_stats_last()[1], event_bytes=nbytes, ivstat_ms=mmm(t_ivs), interval_stats_call_wall_ms=mmm(t_wall),
               count_phase_ms=mmm(t_cnt), subsample_phase_ms=mmm(t_sub),
               ms_per_gb_of_events=dict(ivstat=per_gb(med(t_ivs)), count=per_gb(med(t_cnt)), subsample=per_gb(med(t_sub))),
               million_events_per_s=round(len(ev) / med(t_ivs) / 1e3, 1), gb_per_s=round(nbytes / med(t_ivs) / 1e6, 1),
               ratio_to_count=round(med(t_ivs) / med(t_cnt), 2), ratio_to_subsample=round(med(t_ivs) / med(t_sub), 2),
               path_bit=bool(gx.path_info() & GX_PATH_IVSTAT), checked_against_numpy=True)
    gx.close()
    return out


def table(o):
    rows = [("ivstat (counters cleared + k_ivstat)", o["ivstat_ms"], o["ms_per_gb_of_events"]["ivstat"]),
            ("count (k_cnt_index, k_cnt_count, k_cnt_scan)", o["count_phase_ms"], o["ms_per_gb_of_events"]["count"]),
            ("subsample at 100 % (k_sub_count, scan, k_sub_write)", o["subsample_phase_ms"], o["ms_per_gb_of_events"]["subsample"])]
    out = [f"interval lengths pass, {o['workload']}: {o['events']} events ({o['event_bytes'] / 1e9:.2f} GB), {o['classes']} lengths, the longest "
           f"{o['longest']}, list capacity {o['list_capacity']}, reruns {o['reruns']}",
           f"{'phase':<54}{'min ms':>10}{'median ms':>11}{'max ms':>10}{'ms per GB of events':>22}"]
    for name, t, g in rows:
        out.append(f"{name:<54}{t['min']:>10.3f}{t['median']:>11.3f}{t['max']:>10.3f}{g:>22.3f}")
    out.append(f"whole gx_interval_stats call, host wall: median {o['interval_stats_call_wall_ms']['median']:.3f} ms over "
               f"{o['interval_stats_call_wall_ms']['n']} calls")
    out.append(f"k_ivstat: {o['million_events_per_s']} million events a second, {o['gb_per_s']} GB/s of events; the pass is {o['ratio_to_count']} times "
               f"the count phase and {o['ratio_to_subsample']} times the subsample pass")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", help="also write the text tables there")
    a = ap.parse_args()
    cfg = dict(bench.CONFIGS[2])
    lens = synth.HG38_LENS
    (tv, _), = bench.build_workload(cfg, a.frags, lens)
    same = tv.copy()                                   # every length 200: the start moved down where the chromosome ends sooner
    ln = np.asarray(lens, dtype=np.int64)[same["chrom"].astype(np.int64)]
    same["start"] = np.minimum(same["start"].astype(np.int64), ln - 200)
    same["end"] = same["start"] + 200
    text = []
    by_chrom = tv[np.argsort(tv["chrom"], kind="stable")]   # one chromosome per wavefront nearly everywhere: no per-lane tallies
    for name, ev in (("config 2", tv), ("config 2 with every length 200", same), ("config 2 ordered by chromosome", by_chrom)):
        o = run(name, ev, lens, a.frags, a.steps, a.warmup)
        print(json.dumps(o), flush=True)
        text.append(table(o))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(text))


if __name__ == "__main__":
    main()
