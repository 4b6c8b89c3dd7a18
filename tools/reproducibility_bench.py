"""The split pass and the reproducibility calls (gx_subsample_split_kept, gx_reproducibility) at benchmark size: config 2's
workload (hg38, 50 M fragments), one treatment without control.

  python tools/reproducibility_bench.py [--frags N] [--steps K] [--warmup W] [--out FILE]

It reports, as min / median / max over K calls after a warm-up,
  * the split alone (k_sub_count, k_sub_scan, k_sub_split: the "split" phase, HIP events on the library's stream,
    gx_set_phase_timing(2)) at T = 2^31, by events and per byte of events read (16 bytes an event);
  * what two halves cost without it: two subsample passes (k_sub_count, k_sub_scan, k_sub_write: the "subsample" phase) at
    T = 2^31, the second one keyed as another sample -- the library cannot draw the complement, and a pass that did would keep
    as many events --, and their sum;
  * the subsample pass at 100 %, which reads and writes what the split reads and writes;
  * the whole gx_reproducibility call on the host's clock for one replicate (the 50 M fragments: 5 calls) and for two (the same
    fragments cut into two replicates of half the size: 8 calls), with the calls' peaks.
The split is checked at full size against numpy (tests/saturation_ref.py's draw), and ALONE 0 of one replicate against the
run's own peaks.  One JSON line; --out also writes a text table."""
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
import saturation_ref as R  # noqa: E402
from genrich_amd import synth  # noqa: E402
from genrich_amd.lib import GX_PATH_SATURATION, GX_PATH_SPLIT, Genrich, GxParams, minus_log10f, repro_label, subsample_geometry  # noqa: E402

HALF = 1 << 31


def mmm(xs):
    return dict(min=round(min(xs), 4), median=round(statistics.median(xs), 4), max=round(max(xs), 4), n=len(xs))


def drive(gx, ptr, sizes):
    """One run: a replicate per size, read in place from consecutive parts of the device array."""
    at = 0
    for n in sizes:
        gx.sample_begin(0, None)
        gx.push_events_device(ptr + 16 * at, n)
        gx.sample_end()
        gx.sample_no_control()
        gx.pvalues()
        at += n
    gx.find_peaks()


def timed_phase(gx, name, call):
    gx.set_phase_timing(2)
    res = call()
    gx.set_phase_timing(0)
    return res, [ms for nm, ms in gx.phase_times() if nm == name][-1]


def n_a_of_split(gx, T):
    """Half A's size of sample 0 through gx_subsample_split_kept with no read-back of the events."""
    n = C.c_size_t(0)
    gx._check(gx.lib.gx_subsample_split_kept(gx.ctx, 0, 1, int(T), None, 0, C.byref(n)))
    return n.value


def kept_of_pass(gx, seed, T):
    n = C.c_size_t(0)
    gx._check(gx.lib.gx_subsample_kept(gx.ctx, 0, int(seed), int(T), None, 0, C.byref(n)))
    return n.value


def wall(gx, steps):
    gx.reproducibility()   # (warm-up: the child context is made here)
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        calls = gx.reproducibility()
        t.append((time.perf_counter() - t0) * 1e3)
    return t, calls


def run(frags, steps, warmup):
    cfg = dict(bench.CONFIGS[2])
    lens = synth.HG38_LENS
    (ev, _), = bench.build_workload(cfg, frags, lens)
    d_ev = torch.from_numpy(ev.view(np.uint32).reshape(-1, 4).copy()).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    gx = Genrich(GxParams(minus_log10f(0.01), 0, 200.0, 0, 100, 0, 0))
    gx.set_chroms(lens)
    gx.set_keep_pileups(False)
    gx.set_count_in_peaks(True)
    n = len(ev)
    drive(gx, d_ev.data_ptr(), [n])
    for _ in range(warmup):
        n_a_of_split(gx, HALF)
        kept_of_pass(gx, 1, HALF)
        kept_of_pass(gx, 1, R.FULL)
    t_split, t_a, t_b, t_full = [], [], [], []
    for _ in range(steps):
        n_a, ms = timed_phase(gx, "split", lambda: n_a_of_split(gx, HALF))
        t_split.append(ms)
        kept_a, ms = timed_phase(gx, "subsample", lambda: kept_of_pass(gx, 1, HALF))
        t_a.append(ms)
        kept_b, ms = timed_phase(gx, "subsample", lambda: kept_of_pass(gx, 2, HALF))   # (another draw of the same share: the complement's cost)
        t_b.append(ms)
        kept_full, ms = timed_phase(gx, "subsample", lambda: kept_of_pass(gx, 1, R.FULL))
        t_full.append(ms)
    mask = R.keep_mask(n, 1, 0, HALF)   # full size against numpy
    assert n_a == kept_a == int(mask.sum()) and kept_full == n, (n_a, kept_a, kept_full)
    both, got_na = gx.subsample_split_kept(0, 1, HALF, n)
    assert got_na == n_a and both[:n_a].tobytes() == ev[mask].tobytes() and both[n_a:].tobytes() == ev[~mask].tobytes()
    del both
    t_two = [a + b for a, b in zip(t_a, t_b)]
    bits = gx.path_info()
    w1, calls1 = wall(gx, steps)
    assert gx.reproducibility_peaks(0).tobytes() == gx.get_peaks().tobytes()
    run1 = gx.n_peaks
    gx.reset()
    gx.set_count_in_peaks(True)
    drive(gx, d_ev.data_ptr(), [n // 2, n - n // 2])
    w2, calls2 = wall(gx, steps)
    run2 = gx.n_peaks
    nbytes = 16 * n
    med = statistics.median
    per_gb = lambda ms: round(ms / (nbytes / 1e9), 4)
    lanes, grid, block = subsample_geometry()
    rows = lambda calls: [dict(call=repro_label(c), intervals=int(c["n_events"]), peaks=int(c["n_peaks"]), peak_bp=int(c["peak_bp"]), status=int(c["status"]))
                          for c in calls]
    out = dict(workload="config 2, one treatment without control", fragments=frags, events=n, event_bytes=nbytes,
               geometry=dict(lanes=lanes, grid=grid, block_events=block), half_a=n_a,
               split_ms=mmm(t_split), pass_half_ms=mmm(t_a), pass_other_half_ms=mmm(t_b), two_passes_ms=mmm(t_two), pass_full_ms=mmm(t_full),
               ms_per_gb_of_events=dict(split=per_gb(med(t_split)), two_passes=per_gb(med(t_two)), pass_full=per_gb(med(t_full))),
               million_events_per_s=dict(split=round(n / med(t_split) / 1e3, 1), pass_full=round(n / med(t_full) / 1e3, 1)),
               ratio_split_to_two_passes=round(med(t_split) / med(t_two), 3), ratio_split_to_pass_full=round(med(t_split) / med(t_full), 3),
               reproducibility_r1_wall_ms=mmm(w1), reproducibility_r2_wall_ms=mmm(w2), calls_r1=rows(calls1), calls_r2=rows(calls2),
               run_peaks_r1=run1, run_peaks_r2=run2, path_bits=dict(split=bool(bits & GX_PATH_SPLIT), saturation=bool(bits & GX_PATH_SATURATION)),
               checked_against_numpy=True)
    gx.close()
    return out


def table(o):
    out = [f"split pass, {o['workload']}: {o['events']} events ({o['event_bytes'] / 1e9:.2f} GB), {o['geometry']['lanes']} lanes, "
           f"blocks of {o['geometry']['block_events']} events, at most {o['geometry']['grid']} workgroups; half A: {o['half_a']} events",
           f"{'phase':<64}{'min ms':>10}{'median ms':>11}{'max ms':>10}{'ms per GB of events':>22}"]
    for label, key, gb in (("split at 2^31 (k_sub_count, k_sub_scan, k_sub_split)", "split_ms", "split"),
                           ("subsample at 2^31 (k_sub_count, k_sub_scan, k_sub_write)", "pass_half_ms", None),
                           ("... once more, keyed as another sample", "pass_other_half_ms", None),
                           ("the two passes together", "two_passes_ms", "two_passes"),
                           ("subsample at 100 %", "pass_full_ms", "pass_full")):
        t = o[key]
        out.append(f"{label:<64}{t['min']:>10.3f}{t['median']:>11.3f}{t['max']:>10.3f}" + (f"{o['ms_per_gb_of_events'][gb]:>22.3f}" if gb else ""))
    r = o["ratio_split_to_two_passes"]
    out.append(f"the split is {r} times the two passes together" + ("" if r < 1 else " -- not where it should be: one reading of the events was expected to cost less than two")
               + f" and {o['ratio_split_to_pass_full']} times the pass at 100 %; {o['million_events_per_s']['split']} million events a second")
    for k, what in (("r1", "one replicate, 5 calls"), ("r2", "two replicates of half the size, 8 calls")):
        w = o[f"reproducibility_{k}_wall_ms"]
        out.append(f"whole gx_reproducibility call, {what}, host wall: min {w['min']:.3f}, median {w['median']:.3f}, max {w['max']:.3f} ms over {w['n']} calls")
        out.append("  calls (intervals, peaks, peak bp): " + "; ".join(f"{c['call']}: {c['intervals']}, {c['peaks']}, {c['peak_bp']}" for c in o[f"calls_{k}"])
                   + f"; the run: {o['run_peaks_' + k]} peaks")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", help="also write the text table there")
    a = ap.parse_args()
    o = run(a.frags, a.steps, a.warmup)
    print(json.dumps(o), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table(o))


if __name__ == "__main__":
    main()
