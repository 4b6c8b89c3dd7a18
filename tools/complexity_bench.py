"""Library complexity (gx_complexity) at benchmark size: config 2's workload (hg38, 50 M fragments) with a fifth of the
fragments replaced by copies of earlier ones, as a library with 20 % duplicates.

  python tools/complexity_bench.py [--frags N] [--steps K] [--warmup W] [--out FILE]

It reports, as min / median / max over K calls after a warm-up,
  * the pass split into its two phases (HIP events on the library's stream, gx_set_phase_timing(2)): "cpx_insert" (the table
    cleared and k_cpx_insert) and "cpx_hist" (k_cpx_hist), and the host's wall time of the whole call (staging, both kernels, the
    read-back of the histogram);
  * on the same kept events in the same run the library's "count" phase (k_cnt_count with its index and scan: gx_count_in_peaks),
    the one other pass that reads every kept event once;
  * each per byte of events read (16 bytes an event) and the ratios.
k_pack (the pileup's tight copy) reads no events and runs only ahead of a control merge with -E regions: this workload never
launches it, and it has no phase of its own to time, so it is not in the table.
N and D are checked at full size against numpy (np.unique over the packed keys).  One JSON line; --out also writes a text table."""
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
from genrich_amd import synth  # noqa: E402
from genrich_amd.lib import GX_PATH_COMPLEXITY, Genrich, GxParams, minus_log10f  # noqa: E402


def mmm(xs):
    return dict(min=round(min(xs), 4), median=round(statistics.median(xs), 4), max=round(max(xs), 4), n=len(xs))


def with_duplicates(ev, fraction, seed):
    """A fifth (fraction) of the fragments overwritten by copies of other ones."""
    rng = np.random.default_rng(seed)
    n = len(ev)
    k = int(n * fraction)
    dst = rng.choice(n, k, replace=False)
    src = rng.integers(0, n, k)
    out = ev.copy()
    out[dst] = ev[src]
    return out


def run(frags, steps, warmup):
    cfg = dict(bench.CONFIGS[2])
    lens = synth.HG38_LENS
    (tv, _), = bench.build_workload(cfg, frags, lens)
    ev = with_duplicates(tv, 0.2, 99)
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
    for _ in range(warmup):
        gx.complexity()
        gx.count_in_peaks()
    t_ins, t_hist, t_wall, t_cnt = [], [], [], []
    for _ in range(steps):
        gx.set_phase_timing(2)
        t0 = time.perf_counter()
        gx.complexity()
        t1 = time.perf_counter()
        gx.count_in_peaks()
        gx.set_phase_timing(0)
        ph = gx.phase_times()
        t_ins.append([ms for name, ms in ph if name == "cpx_insert"][-1])
        t_hist.append([ms for name, ms in ph if name == "cpx_hist"][-1])
        t_cnt.append([ms for name, ms in ph if name == "count"][-1])
        t_wall.append((t1 - t0) * 1e3)
    got = gx.get_complexity(0)
    # full size against numpy: the key as (chromosome, start) and the clamped end
    lens_a = np.asarray(lens, dtype=np.uint64)
    base = np.concatenate([[0], np.cumsum(lens_a)])[:-1].astype(np.uint64)
    c = ev["chrom"].astype(np.int64)
    key = ((base[c] + ev["start"].astype(np.uint64)) << np.uint64(32)) | np.minimum(ev["end"].astype(np.uint64), lens_a[c])
    _, counts = np.unique(key, return_counts=True)
    m, k = np.unique(counts, return_counts=True)
    assert (got.n_obs, got.n_distinct) == (len(ev), len(counts)) and got.pairs == list(zip(m.tolist(), k.tolist()))
    nbytes = 16 * len(ev)
    med = lambda xs: statistics.median(xs)
    per_gb = lambda ms: round(ms / (nbytes / 1e9), 4)
    out = dict(workload="config 2 with 20 % of the fragments copies of others", fragments=frags, events=len(ev), n_obs=got.n_obs,
               n_distinct=got.n_distinct, classes=len(got.pairs), max_multiplicity=got.pairs[-1][0], table_slots=gx.complexity_last(),
               table_bytes=16 * gx.complexity_last(), event_bytes=nbytes,
               cpx_insert_ms=mmm(t_ins), cpx_hist_ms=mmm(t_hist), complexity_call_wall_ms=mmm(t_wall), count_phase_ms=mmm(t_cnt),
               ms_per_gb_of_events=dict(cpx_insert=per_gb(med(t_ins)), cpx_hist=per_gb(med(t_hist)), cpx_both=per_gb(med(t_ins) + med(t_hist)),
                                        count=per_gb(med(t_cnt))),
               insert_million_events_per_s=round(len(ev) / med(t_ins) / 1e3, 1),
               ratio_pass_to_count=round((med(t_ins) + med(t_hist)) / med(t_cnt), 2),
               ratio_insert_to_hist=round(med(t_ins) / med(t_hist), 2),
               path_bit=bool(gx.path_info() & GX_PATH_COMPLEXITY), checked_against_numpy=True)
    gx.close()
    return out


def table(o):
    rows = [("cpx_insert (table cleared + k_cpx_insert)", o["cpx_insert_ms"], o["ms_per_gb_of_events"]["cpx_insert"]),
            ("cpx_hist (k_cpx_hist)", o["cpx_hist_ms"], o["ms_per_gb_of_events"]["cpx_hist"]),
            ("count (k_cnt_index, k_cnt_count, k_cnt_scan)", o["count_phase_ms"], o["ms_per_gb_of_events"]["count"])]
    out = [f"library complexity pass, {o['workload']}: {o['events']} events ({o['event_bytes'] / 1e9:.2f} GB), "
           f"{o['n_distinct']} distinct keys, table {o['table_slots']} slots ({o['table_bytes'] / 2 ** 30:.2f} GiB)",
           f"{'phase':<48}{'min ms':>10}{'median ms':>11}{'max ms':>10}{'ms per GB of events':>22}"]
    for name, t, g in rows:
        out.append(f"{name:<48}{t['min']:>10.3f}{t['median']:>11.3f}{t['max']:>10.3f}{g:>22.3f}")
    out.append(f"whole gx_complexity call, host wall: median {o['complexity_call_wall_ms']['median']:.3f} ms over {o['complexity_call_wall_ms']['n']} calls")
    out.append(f"k_cpx_insert: {o['insert_million_events_per_s']} million events a second; the pass is {o['ratio_pass_to_count']} times the count phase; "
               f"insert / hist = {o['ratio_insert_to_hist']}")
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
