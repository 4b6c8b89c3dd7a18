"""The subsample pass and the peak saturation curve (gx_subsample_kept, gx_saturation) at benchmark size: config 2's workload
(hg38, 50 M fragments), one treatment without control.

  python tools/saturation_bench.py [--frags N] [--steps K] [--warmup W] [--points P] [--out FILE]

It reports, as min / median / max over K calls after a warm-up,
  * the subsample pass alone (k_sub_count, k_sub_scan, k_sub_write: the "subsample" phase, HIP events on the library's stream,
    gx_set_phase_timing(2)) at thresholds 10 %, 50 % and 100 %, by events and per byte of events read (16 bytes an event);
  * on the same kept events in the same run the library's "count" phase (k_cnt_count with its index and scan:
    gx_count_in_peaks), the one other pass that streams every kept event once;
  * the whole P-point gx_saturation call (10 by default) on the host's clock, and its points.
The kept counts are checked at full size against numpy (tests/saturation_ref.py) and the 100 % subsample against the events
themselves.  One JSON line; --out also writes a text table."""
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
import saturation_ref as R  # noqa: E402
from genrich_amd import synth  # noqa: E402
from genrich_amd.lib import GX_PATH_SATURATION, Genrich, GxParams, minus_log10f, saturation_thresholds, subsample_geometry  # noqa: E402


def mmm(xs):
    return dict(min=round(min(xs), 4), median=round(statistics.median(xs), 4), max=round(max(xs), 4), n=len(xs))


def run(frags, steps, warmup, points):
    cfg = dict(bench.CONFIGS[2])
    lens = synth.HG38_LENS
    (ev, _), = bench.build_workload(cfg, frags, lens)
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
    n = len(ev)
    count = lambda T: int(C_count(gx, T))
    fracs = {"10": R.FULL // 10, "50": R.FULL // 2, "100": R.FULL}
    for _ in range(warmup):
        for T in fracs.values():
            count(T)
        gx.count_in_peaks()
    t_sub = {k: [] for k in fracs}
    t_cnt = []
    kept = {}
    for _ in range(steps):
        for k, T in fracs.items():
            gx.set_phase_timing(2)
            kept[k] = count(T)
            gx.set_phase_timing(0)
            t_sub[k].append([ms for name, ms in gx.phase_times() if name == "subsample"][-1])
        gx.set_phase_timing(2)
        gx.count_in_peaks()
        gx.set_phase_timing(0)
        t_cnt.append([ms for name, ms in gx.phase_times() if name == "count"][-1])
    for k, T in fracs.items():   # full size against numpy
        assert kept[k] == int(R.keep_mask(n, 1, 0, T).sum()), (k, kept[k])
    assert gx.subsample_kept(0, 1, R.FULL).tobytes() == ev.tobytes()
    thr = saturation_thresholds(points)
    gx.saturation(thr)   # (warm-up: the child context is made here)
    t_wall = []
    for _ in range(steps):
        t0 = time.perf_counter()
        pts = gx.saturation(thr)
        t_wall.append((time.perf_counter() - t0) * 1e3)
    assert gx.saturation_peaks(points - 1).tobytes() == gx.get_peaks().tobytes()
    nbytes = 16 * n
    med = statistics.median
    per_gb = lambda ms: round(ms / (nbytes / 1e9), 4)
    lanes, grid, block = subsample_geometry()
    out = dict(workload="config 2, one treatment without control", fragments=frags, events=n, event_bytes=nbytes,
               geometry=dict(lanes=lanes, grid=grid, block_events=block),
               kept={k: kept[k] for k in fracs}, subsample_ms={k: mmm(t_sub[k]) for k in fracs}, count_phase_ms=mmm(t_cnt),
               ms_per_gb_of_events=dict(count=per_gb(med(t_cnt)), **{"subsample_" + k: per_gb(med(t_sub[k])) for k in fracs}),
               million_events_per_s={k: round(n / med(t_sub[k]) / 1e3, 1) for k in fracs},
               ratio_subsample100_to_count=round(med(t_sub["100"]) / med(t_cnt), 2),
               saturation_points=points, saturation_call_wall_ms=mmm(t_wall),
               curve=[dict(fraction=round(int(p["threshold"]) / R.FULL, 4), kept=int(p["n_kept"]), peaks=int(p["n_peaks"]), peak_bp=int(p["peak_bp"]),
                           status=int(p["status"])) for p in pts],
               run_peaks=gx.n_peaks, path_bit=bool(gx.path_info() & GX_PATH_SATURATION), checked_against_numpy=True)
    gx.close()
    return out


def C_count(gx, T):
    """The kept count of sample 0 at T through gx_subsample_kept with no read-back of the events."""
    import ctypes as C
    n = C.c_size_t(0)
    gx._check(gx.lib.gx_subsample_kept(gx.ctx, 0, 1, int(T), None, 0, C.byref(n)))
    return n.value


def table(o):
    out = [f"subsample pass, {o['workload']}: {o['events']} events ({o['event_bytes'] / 1e9:.2f} GB), {o['geometry']['lanes']} lanes, "
           f"blocks of {o['geometry']['block_events']} events, at most {o['geometry']['grid']} workgroups",
           f"{'phase':<52}{'min ms':>10}{'median ms':>11}{'max ms':>10}{'ms per GB of events':>22}{'kept':>12}"]
    for k in ("10", "50", "100"):
        t = o["subsample_ms"][k]
        out.append(f"{'subsample at ' + k + ' % (k_sub_count, k_sub_scan, k_sub_write)':<52}{t['min']:>10.3f}{t['median']:>11.3f}{t['max']:>10.3f}"
                   f"{o['ms_per_gb_of_events']['subsample_' + k]:>22.3f}{o['kept'][k]:>12}")
    t = o["count_phase_ms"]
    out.append(f"{'count (k_cnt_index, k_cnt_count, k_cnt_scan)':<52}{t['min']:>10.3f}{t['median']:>11.3f}{t['max']:>10.3f}{o['ms_per_gb_of_events']['count']:>22.3f}")
    out.append(f"the pass at 100 % is {o['ratio_subsample100_to_count']} times the count phase; "
               f"{o['million_events_per_s']['100']} million events a second at 100 %, {o['million_events_per_s']['10']} at 10 %")
    w = o["saturation_call_wall_ms"]
    out.append(f"whole {o['saturation_points']}-point gx_saturation call, host wall: min {w['min']:.3f}, median {w['median']:.3f}, max {w['max']:.3f} ms over {w['n']} calls")
    out.append("curve (fraction: kept, peaks, peak bp): " + "; ".join(f"{p['fraction']}: {p['kept']}, {p['peaks']}, {p['peak_bp']}" for p in o["curve"])
               + f"; the run: {o['run_peaks']} peaks")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--points", type=int, default=10)
    ap.add_argument("--out", help="also write the text table there")
    a = ap.parse_args()
    o = run(a.frags, a.steps, a.warmup, a.points)
    print(json.dumps(o), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table(o))


if __name__ == "__main__":
    main()
