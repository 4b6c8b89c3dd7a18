"""The genome and GC bias passes (gx_push_sequence, gx_gc_bias) at benchmark size: hg38's chromosome lengths, a synthetic genome
(one random block of bases with a few N, pushed again and again: no FASTA is needed), config 2's 50 M fragments, W = 200.

  python tools/gcbias_bench.py [--frags N] [--steps K] [--warmup W] [--window W] [--fasta-mb M] [--out FILE]

It reports, as min / median / max over K calls after a warm-up,
  * k_gc_pack ("gc.pack": HIP events on the library's stream, gx_set_phase_timing(2), summed over the launches of one genome) next
    to a pinned host-to-device copy of the same bytes in the same run, and the host's wall time of pushing the whole genome;
  * the directory ("gc.dir": k_gc_dir_count + k_gc_dir_scan);
  * k_gc_expected ("gc.expected") next to a plain read of two vectors of the same size (a device sum);
  * k_gc_observed ("gc.observed") next to k_ivstat ("ivstat") and --saturation's subsample pass at 100 % ("subsample") over the
    same kept events;
  * the command line's --genome from a FASTA of M megabases (a file written here) to the device, in seconds per GB, as -v says it.
The tables are checked at full size: the classed and unclassed windows add up to the genome, the classed and unclassed intervals
to the events.  One JSON line; --out also writes a text table."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import bench  # noqa: E402
from genrich_amd import build, synth  # noqa: E402
from genrich_amd.lib import GX_PATH_GC, Genrich, GxParams, minus_log10f  # noqa: E402

BLOCK = 1 << 26


def mmm(xs):
    return dict(min=round(min(xs), 4), median=round(statistics.median(xs), 4), max=round(max(xs), 4), n=len(xs))


def random_block(seed=1):
    rng = np.random.default_rng(seed)
    b = np.frombuffer(b"ACGTacgt", dtype=np.uint8)[rng.integers(0, 8, BLOCK)].copy()
    for at in rng.integers(0, BLOCK - 50_000, 40):           # a few runs of N, as an assembly's gaps
        b[at:at + int(rng.integers(100, 50_000))] = ord("N")
    return b


def push_genome(gx, lens, block):
    for c, n in enumerate(lens):
        for first in range(0, n, BLOCK):
            k = min(BLOCK, n - first)
            gx._check(gx.lib.gx_push_sequence(gx.ctx, c, first, block.ctypes.data, k))


class Phases:
    """The time a named phase took since the last look (the library's list grows until the next sample begins)."""
    def __init__(self, gx):
        self.gx, self.seen = gx, {}

    def take(self, name):
        total = sum(ms for nm, ms in self.gx.phase_times() if nm == name)
        delta = total - self.seen.get(name, 0.0)
        self.seen[name] = total
        return delta


def device_ms(fn, steps):
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def cli_genome_seconds(mb, block):
    """--genome of one chromosome of `mb` megabases through the command line: the seconds -v reports, per GB of FASTA."""
    n = mb * 1_000_000
    with tempfile.TemporaryDirectory() as tmp:
        fa, sam = os.path.join(tmp, "g.fa"), os.path.join(tmp, "t.sam")
        seq = np.resize(block, n)
        lines = np.full((n // 60, 61), ord("\n"), dtype=np.uint8)
        lines[:, :60] = seq[:n // 60 * 60].reshape(-1, 60)
        with open(fa, "wb") as f:
            f.write(b">chrG\n")
            f.write(lines.tobytes())
            f.write(seq[n // 60 * 60:].tobytes() + b"\n")
        rng = np.random.default_rng(2)
        with open(sam, "w") as f:
            f.write("@HD\tVN:1.0\tSO:unsorted\n@SQ\tSN:chrG\tLN:%d\n" % n)
            for i, p in enumerate(rng.integers(1, n - 200, 20_000)):
                f.write("r%07d\t0\tchrG\t%d\t60\t100M\t*\t0\t0\t*\t*\n" % (i, p))
        res = subprocess.run([build.build_host(), "-v", "-y", "-X", "-t", sam, "--genome", fa, "--gc-bias", os.path.join(tmp, "gc.tsv")],
                             capture_output=True, text=True)
        m = re.search(r"^Genome .* in ([0-9.]+) s$", res.stderr, re.M)
        if not m:                                            # (the genome is loaded before an alignment is read: its line stands on its own)
            raise RuntimeError(res.stderr[-2000:])
        size = os.path.getsize(fa)
        return dict(fasta_bytes=size, seconds=float(m.group(1)), seconds_per_gb=round(float(m.group(1)) / (size / 1e9), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--fasta-mb", type=int, default=500)
    ap.add_argument("--out", help="also write the text table there")
    a = ap.parse_args()
    lens, W = synth.HG38_LENS, a.window
    genome = sum(lens)
    block = random_block()
    (tv, _), = bench.build_workload(dict(bench.CONFIGS[2]), a.frags, lens)
    d_ev = torch.from_numpy(tv.view(np.uint32).reshape(-1, 4).copy()).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    gx = Genrich(GxParams(minus_log10f(0.01), 0, 200.0, 0, 100, 0, 0))
    gx.set_chroms(lens)
    gx.set_keep_pileups(False)
    gx.set_count_in_peaks(True)
    gx.set_genome(True)
    # the pack: the whole genome pushed K times (the same words stored again)
    t_pack, t_push_wall = [], []
    ph = Phases(gx)
    for i in range(a.warmup + a.steps):
        gx.set_phase_timing(2)
        t0 = time.perf_counter()
        push_genome(gx, lens, block)
        pushed, gc, acgt = gx.genome_info()                  # (drains the stream; builds the directory)
        t1 = time.perf_counter()
        gx.set_phase_timing(0)
        packed = ph.take("gc.pack")
        if i >= a.warmup:
            t_pack.append(packed)
            t_push_wall.append((t1 - t0) * 1e3)
    assert pushed == genome and 0 < gc < acgt < genome
    pinned = torch.empty(BLOCK, dtype=torch.uint8).pin_memory()
    dev = torch.empty(BLOCK, dtype=torch.uint8, device="cuda:0")
    t_h2d = [t * genome / BLOCK for t in device_ms(lambda: dev.copy_(pinned, non_blocking=True), a.warmup + a.steps)[a.warmup:]]
    vec = torch.ones(2 * ((genome + 63) // 64), dtype=torch.int64, device="cuda:0")      # two vectors' words
    t_read = device_ms(lambda: vec.sum(), a.warmup + a.steps)[a.warmup:]
    del vec, dev
    gx.sample_begin(0, None)
    gx.push_events_device(d_ev.data_ptr(), d_ev.shape[0])
    gx.sample_end()
    n_out = C.c_size_t(0)
    ph = Phases(gx)                                          # (gx_sample_begin emptied the list)
    t_dir, t_exp, t_obs, t_wall, t_ivs, t_sub = [], [], [], [], [], []
    for i in range(a.warmup + a.steps):
        gx._check(gx.lib.gx_push_sequence(gx.ctx, 0, 0, block.ctypes.data, 64))      # (dirties the directory: it is built again)
        gx.set_phase_timing(2)
        t0 = time.perf_counter()
        assert gx.gc_bias(W) == 1
        t1 = time.perf_counter()
        gx.interval_stats()
        gx._check(gx.lib.gx_subsample_kept(gx.ctx, 0, 1, 1 << 32, None, 0, C.byref(n_out)))
        gx.set_phase_timing(0)
        for lst, nm in ((t_dir, "gc.dir"), (t_exp, "gc.expected"), (t_obs, "gc.observed"), (t_ivs, "ivstat"), (t_sub, "subsample")):
            lst.append(ph.take(nm))
        t_wall.append((t1 - t0) * 1e3)
    t_dir, t_exp, t_obs, t_ivs, t_sub, t_wall = (x[a.warmup:] for x in (t_dir, t_exp, t_obs, t_ivs, t_sub, t_wall))
    r = gx.get_gc_bias(0)
    assert int(r.F.sum()) + r.f_unclassed == genome and int(r.Nn.sum()) + r.n_unclassed == len(tv) and gx.path_info() & GX_PATH_GC
    gx.close()
    med = statistics.median
    vec_bytes = 2 * 8 * ((genome + 63) // 64)
    o = dict(genome_bases=genome, window=W, fragments=a.frags, events=len(tv), vector_bytes=vec_bytes,
             classed_windows=int(r.F.sum()), unclassed_windows=r.f_unclassed, classed_intervals=int(r.Nn.sum()), unclassed_intervals=r.n_unclassed,
             pack_ms=mmm(t_pack), h2d_copy_same_bytes_ms=mmm(t_h2d), push_genome_wall_ms=mmm(t_push_wall), dir_ms=mmm(t_dir),
             expected_ms=mmm(t_exp), plain_read_two_vectors_ms=mmm(t_read), observed_ms=mmm(t_obs), ivstat_ms=mmm(t_ivs), subsample_ms=mmm(t_sub),
             gc_bias_call_wall_ms=mmm(t_wall),
             pack_gb_per_s=round(genome / med(t_pack) / 1e6, 1), expected_gb_per_s=round(vec_bytes / med(t_exp) / 1e6, 1),
             expected_over_plain_read=round(med(t_exp) / med(t_read), 2), pack_over_h2d=round(med(t_pack) / med(t_h2d), 3),
             observed_over_ivstat=round(med(t_obs) / med(t_ivs), 2), observed_over_subsample=round(med(t_obs) / med(t_sub), 2),
             observed_million_events_per_s=round(len(tv) / med(t_obs) / 1e3, 1))
    if a.fasta_mb:
        try:
            o["cli_genome"] = cli_genome_seconds(a.fasta_mb, block)
        except RuntimeError as e:
            o["cli_genome_error"] = str(e)[-500:]
            a.fasta_mb = 0
    print(json.dumps(o), flush=True)
    if a.out:
        rows = [("k_gc_pack, whole genome (gc.pack)", o["pack_ms"]), ("pinned H2D copy of the same bytes", o["h2d_copy_same_bytes_ms"]),
                ("pushing the genome, host wall", o["push_genome_wall_ms"]), ("directory (gc.dir)", o["dir_ms"]),
                ("k_gc_expected (gc.expected)", o["expected_ms"]), ("plain read of two vectors (device sum)", o["plain_read_two_vectors_ms"]),
                ("k_gc_observed (gc.observed)", o["observed_ms"]), ("k_ivstat (ivstat)", o["ivstat_ms"]), ("subsample at 100 % (subsample)", o["subsample_ms"]),
                ("whole gx_gc_bias call, host wall", o["gc_bias_call_wall_ms"])]
        with open(a.out, "w") as f:
            f.write(f"genome and GC bias passes: hg38's lengths ({genome} bases, {vec_bytes / 1e9:.2f} GB in two vectors), W = {W}, {len(tv)} events\n")
            f.write(f"{'phase':<44}{'min ms':>12}{'median ms':>12}{'max ms':>12}\n")
            for name, t in rows:
                f.write(f"{name:<44}{t['min']:>12.3f}{t['median']:>12.3f}{t['max']:>12.3f}\n")
            f.write(f"k_gc_pack {o['pack_gb_per_s']} GB/s of bases, {o['pack_over_h2d']} times the copy; k_gc_expected {o['expected_gb_per_s']} GB/s of vector "
                    f"words, {o['expected_over_plain_read']} times the plain read; k_gc_observed {o['observed_million_events_per_s']} million events a second, "
                    f"{o['observed_over_ivstat']} times k_ivstat and {o['observed_over_subsample']} times the subsample pass\n")
            f.write(f"windows: {o['classed_windows']} classed, {o['unclassed_windows']} not; intervals: {o['classed_intervals']} classed, {o['unclassed_intervals']} not\n")
            if a.fasta_mb:
                g = o["cli_genome"]
                f.write(f"--genome on the command line: {g['fasta_bytes'] / 1e9:.3f} GB of FASTA to the device in {g['seconds']:.3f} s, {g['seconds_per_gb']} s per GB\n")


if __name__ == "__main__":
    main()
