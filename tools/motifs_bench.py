"""The motif scan (gx_motif_scan_peaks, gx_motif_scan_genome) at benchmark size: hg38's chromosome lengths, a synthetic genome (one
random block of bases with a few N, pushed again and again: no FASTA is needed), config 2's 50 M fragments and the peaks called
on them, 10, 100 and 1,000 random motifs of width 12 at p = 1e-4.

  python tools/motifs_bench.py [--frags N] [--steps K] [--warmup W] [--motifs 10,100,1000] [--genome-motifs 10,100] [--out FILE]

It reports, as min / median / max over K calls after a warm-up (HIP events on the library's stream, gx_set_phase_timing(2)),
  * k_motif_scan over the called peaks ("motifs", the list instance; a pass that ran full is both of its runs) per motif count;
  * k_motif_scan over the whole genome (the count-only instance) per motif count of --genome-motifs;
  * next to them, in the same run, the whole peak-signal pass ("peaksig": staging, scatter and k_psig_reduce, which reads the
    same peak space) and a plain read of three vectors of the genome's size (a device sum).
The counts are checked at full size: hits_fwd + hits_rev of the peaks is the hit list's length.  One JSON line; --out also writes
a text table."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import bench  # noqa: E402
from gcbias_bench import Phases, device_ms, mmm, push_genome, random_block  # noqa: E402
from genrich_amd import synth  # noqa: E402
from genrich_amd.lib import GX_PATH_MOTIFS, Genrich, GxParams, minus_log10f, motif_pssm, motif_threshold  # noqa: E402

WIDTH, P = 12, 1e-4


def random_motifs(n, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        counts = rng.integers(0, 40, (4, WIDTH)) + 30 * (rng.integers(0, 4, WIDTH)[None, :] == np.arange(4)[:, None])   # a preferred base per column
        s, lo, hi = motif_pssm(counts, 1.0)
        out.append((s, motif_threshold(s, P)[0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--motifs", default="10,100,1000")
    ap.add_argument("--genome-motifs", default="10,100")
    ap.add_argument("--out", help="also write the text table there")
    a = ap.parse_args()
    lens = synth.HG38_LENS
    genome = sum(lens)
    (tv, _), = bench.build_workload(dict(bench.CONFIGS[2]), a.frags, lens)
    d_ev = torch.from_numpy(tv.view(np.uint32).reshape(-1, 4).copy()).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    gx = Genrich(GxParams(minus_log10f(0.01), 0, 200.0, 0, 100, 0, 0))
    gx.set_chroms(lens)
    gx.set_keep_pileups(False)
    gx.set_count_in_peaks(True)
    gx.set_genome(True)
    gx.set_genome_bases(True)
    push_genome(gx, lens, random_block())
    gx.sample_begin(0, None)
    gx.push_events_device(d_ev.data_ptr(), d_ev.shape[0])
    gx.sample_end()
    gx.sample_no_control()
    gx.pvalues()
    gx.find_peaks()
    pk = gx.get_peaks()
    peak_bp = int((pk["end"] - pk["start"]).sum())
    vec = torch.ones(3 * ((genome + 63) // 64), dtype=torch.int64, device="cuda:0")      # three vectors' words
    t_read = device_ms(lambda: vec.sum(), a.warmup + a.steps)[a.warmup:]
    del vec
    ph = Phases(gx)
    o = dict(genome_bases=genome, fragments=a.frags, peaks=int(len(pk)), peak_bp=peak_bp, width=WIDTH, p=P, plain_read_three_vectors_ms=mmm(t_read),
             peaks_ms={}, genome_ms={}, hits={}, reruns={})
    t_sig = []
    for i in range(a.warmup + a.steps):
        gx.set_phase_timing(2)
        gx.peak_signal()
        gx.set_phase_timing(0)
        t_sig.append(ph.take("peaksig"))
    o["peak_signal_pass_ms"] = mmm(t_sig[a.warmup:])
    for n in [int(x) for x in a.motifs.split(",") if x]:
        gx.set_motifs(random_motifs(n))
        ts = []
        for i in range(a.warmup + a.steps):
            gx.set_phase_timing(2)
            hits = gx.motif_scan_peaks()
            gx.set_phase_timing(0)
            ts.append(ph.take("motifs"))
        cnt = gx.get_motif_counts()
        assert int(cnt[1].sum() + cnt[2].sum()) == hits and gx.path_info() & GX_PATH_MOTIFS
        o["peaks_ms"][n], o["hits"][n], o["reruns"][n] = mmm(ts[a.warmup:]), hits, gx.motif_last()[0]
        if str(n) in a.genome_motifs.split(","):
            ts = []
            for i in range(a.warmup + a.steps):
                gx.set_phase_timing(2)
                g = gx.motif_scan_genome()
                gx.set_phase_timing(0)
                ts.append(ph.take("motifs"))
            assert int(g[0].min()) > genome // 2
            o["genome_ms"][n] = mmm(ts[a.warmup:])
    gx.close()
    med = statistics.median
    o["peaks_over_peak_signal_pass"] = {n: round(t["median"] / med(t_sig[a.warmup:]), 2) for n, t in o["peaks_ms"].items()}
    o["genome_over_plain_read"] = {n: round(t["median"] / med(t_read), 1) for n, t in o["genome_ms"].items()}
    o["peaks_column_steps_per_ns"] = {n: round(peak_bp * n * WIDTH * 2 / t["median"] / 1e6, 1) for n, t in o["peaks_ms"].items()}
    o["genome_column_steps_per_ns"] = {n: round(genome * n * WIDTH * 2 / t["median"] / 1e6, 1) for n, t in o["genome_ms"].items()}
    print(json.dumps(o), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"motif scan: hg38's lengths ({genome} bases), {len(tv)} events, {len(pk)} peaks of {peak_bp} bp, width {WIDTH}, p = {P}\n")
            f.write(f"{'pass':<52}{'min ms':>12}{'median ms':>12}{'max ms':>12}\n")
            rows = [("plain read of three vectors (device sum)", o["plain_read_three_vectors_ms"]), ("peak-signal pass (peaksig: scatter + k_psig_reduce)", o["peak_signal_pass_ms"])]
            rows += [(f"k_motif_scan, peaks, {n} motifs ({o['hits'][n]} hits, {o['reruns'][n]} rerun)", t) for n, t in o["peaks_ms"].items()]
            rows += [(f"k_motif_scan, genome, {n} motifs (count only)", t) for n, t in o["genome_ms"].items()]
            for name, t in rows:
                f.write(f"{name:<52}{t['min']:>12.3f}{t['median']:>12.3f}{t['max']:>12.3f}\n")
            f.write(f"column steps (position x motif x column x strand) per ns: peaks {o['peaks_column_steps_per_ns']}, genome {o['genome_column_steps_per_ns']}\n")
            f.write(f"peaks over the peak-signal pass: {o['peaks_over_peak_signal_pass']}; genome over the plain read: {o['genome_over_plain_read']}\n")
            f.write("the pair-table variant (two columns per lookup) was not tried\n")


if __name__ == "__main__":
    main()
