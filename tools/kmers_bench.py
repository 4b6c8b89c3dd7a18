"""The k-mer count (gx_kmer_count_peaks, gx_kmer_count_genome) at benchmark size: hg38's chromosome lengths, a synthetic genome (one
random block of bases with a few N, pushed again and again: no FASTA is needed), config 2's 50 M fragments and the peaks called
on them, k = 6, 7, 8, 10 and 12.

  python tools/kmers_bench.py [--frags N] [--steps K] [--warmup W] [--ks 6,7,8,10,12] [--out FILE]

It reports, as min / median / max over K calls after a warm-up (HIP events on the library's stream, gx_set_phase_timing(2)),
  * k_kmer_count over the called peaks and over the whole genome per k (phase "kmers": the table's clearing and the kernel), on
    the path the library takes and, up to k = 7, once more with the global-atomic path forced (the 7 | 8 split);
  * the whole call's wall time next to it (the table read back, permuted to the public order and checked on the host);
  * next to them, in the same run, a plain read of three vectors of the genome's size (a device sum: the floor) and the
    count-only k_motif_scan with one motif of width k over the genome (the pass it must beat clearly).
The counts are checked at full size: sum(counts) == windows (the library does), and the forced path gives the same table.  One
JSON line; --out also writes a text table."""
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
from gcbias_bench import Phases, device_ms, mmm, push_genome, random_block  # noqa: E402
from genrich_amd import synth  # noqa: E402
from genrich_amd.lib import GX_PATH_KMERS, KMER_LDS_MAX_K, Genrich, GxParams, minus_log10f  # noqa: E402


def timed(gx, ph, call, n, phase="kmers"):
    """(device ms of the phase, wall ms, the last result) of n calls."""
    dev, wall, res = [], [], None
    for _ in range(n):
        gx.set_phase_timing(2)
        t0 = time.perf_counter()
        res = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        gx.set_phase_timing(0)
        dev.append(ph.take(phase))
    return dev, wall, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ks", default="6,7,8,10,12")
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
    n, w = a.warmup + a.steps, a.warmup
    o = dict(genome_bases=genome, fragments=a.frags, peaks=int(len(pk)), peak_bp=peak_bp, plain_read_three_vectors_ms=mmm(t_read), rows=[])
    med = statistics.median
    for k in [int(x) for x in a.ks.split(",") if x]:
        gx.set_motifs([(np.zeros((k, 4), dtype=np.int16), 1)])                            # one motif of width k that never hits: count only
        dev, wall, _ = timed(gx, ph, gx.motif_scan_genome, n, "motifs")
        motif_ms = mmm(dev[w:])
        kept = {}
        for forced in ([False, True] if k <= KMER_LDS_MAX_K else [False]):
            gx.kmer_force_hbm(forced)
            dp, wp, _ = timed(gx, ph, lambda: gx.kmer_count_peaks(k), n)
            cp = gx.get_kmer_counts()
            dg, wg, (cg, win) = timed(gx, ph, lambda: gx.kmer_count_genome(k), n)
            path, flushes = gx.kmer_last()
            assert path == (1 if forced or k > KMER_LDS_MAX_K else 0) and int(cg.sum()) == win > genome // 2 and gx.path_info() & GX_PATH_KMERS
            kept[forced] = (cp, cg)
            o["rows"].append(dict(k=k, path="HBM" if path else "LDS", forced=forced, peaks_ms=mmm(dp[w:]), peaks_wall_ms=mmm(wp[w:]), genome_ms=mmm(dg[w:]),
                                  genome_wall_ms=mmm(wg[w:]), genome_flushes=flushes, windows_genome=int(win), motif_scan_genome_one_motif_ms=motif_ms,
                                  genome_over_plain_read=round(med(dg[w:]) / med(t_read), 2), motif_over_kmers=round(motif_ms["median"] / med(dg[w:]), 2)))
        gx.kmer_force_hbm(False)
        if True in kept:
            assert np.array_equal(kept[False][0], kept[True][0]) and np.array_equal(kept[False][1], kept[True][1])
    gx.close()
    print(json.dumps(o), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"k-mer count: hg38's lengths ({genome} bases), {len(tv)} events, {len(pk)} peaks of {peak_bp} bp\n")
            f.write(f"plain read of three vectors (device sum): {o['plain_read_three_vectors_ms']['median']:.3f} ms median\n")
            f.write(f"{'k':>3} {'path':<12}{'peaks ms':>10}{'peaks wall':>12}{'genome ms':>11}{'genome wall':>13}{'flushes':>9}{'motif ms':>10}{'/read':>7}{'motif/':>8}\n")
            for r in o["rows"]:
                f.write(f"{r['k']:>3} {r['path'] + (' (forced)' if r['forced'] else ''):<12}{r['peaks_ms']['median']:>10.3f}{r['peaks_wall_ms']['median']:>12.3f}"
                        f"{r['genome_ms']['median']:>11.3f}{r['genome_wall_ms']['median']:>13.3f}{r['genome_flushes']:>9}"
                        f"{r['motif_scan_genome_one_motif_ms']['median']:>10.3f}{r['genome_over_plain_read']:>7.2f}{r['motif_over_kmers']:>8.2f}\n")
            f.write("ms: device time of the phase (the table's clearing and the kernel), median; wall: the whole call with the read-back, the\n"
                    "permutation to the public order and the check on the host; /read: genome ms over the plain read; motif/: the count-only\n"
                    "k_motif_scan with one motif of width k over the genome, over the k-mer pass\n")


if __name__ == "__main__":
    main()
