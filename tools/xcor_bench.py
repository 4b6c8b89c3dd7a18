"""Strand cross-correlation (gx_set_xcor) at benchmark size: config 2's workload (hg38, 50 M fragments) as 100 M tags -- every
fragment's first base on the plus strand, its last on the minus strand -- over the default shifts -100 .. 600, and once more with
a fifth of the tags, which shows how the cost follows the number of non-zero plus words.

  python tools/xcor_bench.py [--frags N] [--steps K] [--warmup W] [--out FILE]

It reports, per workload, as min / median / max over K calls of gx_xcor_tags after a warm-up (HIP events on the library's stream,
gx_set_phase_timing(2)),
  * "xcor.set": k_xc_set over the tags on the device (one 64-bit atomic OR per tag into the cleared vectors);
  * "xcor.corr": k_xc_corr, the whole pass over the two vectors with its final adds;
  * the non-zero plus words, the pairs (non-zero plus word, block of 64 shifts) a second, and the bytes of the two vectors;
  * on the same fragments in the same run the library's "count" phase (gx_count_in_peaks) and the "subsample" phase of
    gx_subsample_kept at 100 % (--saturation's pass), for comparison.
nP and nM are checked at full size against numpy (distinct positions), n11 at two shifts against a sorted intersection.  One JSON
line per workload; --out also writes a text table."""
from __future__ import annotations

import argparse
import ctypes as C
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
from genrich_amd import synth  # noqa: E402
from genrich_amd.lib import GX_PATH_XCOR, TAG_DTYPE, Genrich, GxParams, minus_log10f, xcor_geometry  # noqa: E402

LO, HI = -100, 600


def mmm(xs):
    return dict(min=round(min(xs), 4), median=round(statistics.median(xs), 4), max=round(max(xs), 4), n=len(xs))


def tags_of(ev):
    t = np.zeros(2 * len(ev), dtype=TAG_DTYPE)
    t["chrom"][0::2], t["pos"][0::2], t["strand"][0::2] = ev["chrom"], ev["start"], 1
    t["chrom"][1::2], t["pos"][1::2], t["strand"][1::2] = ev["chrom"], ev["end"] - 1, 0
    return t


def numpy_counts(tags, shifts):
    """(nP, nM, {d: n11(d)}, non-zero plus words) from sorted keys chrom << 32 | pos."""
    key = (tags["chrom"].astype(np.uint64) << np.uint64(32)) | tags["pos"].astype(np.uint64)
    plus, minus = np.unique(key[tags["strand"] == 1]), np.unique(key[tags["strand"] == 0])
    n11 = {d: int(np.intersect1d(plus + np.uint64(d), minus, assume_unique=True).size) for d in shifts}
    return int(plus.size), int(minus.size), n11, int(np.unique(plus >> np.uint64(6)).size)


def kept_passes(gx, ev, lens, steps, warmup):
    """The count phase and the subsample pass at 100 % over the same fragments as one kept sample: (count ms, subsample ms)."""
    d_ev = torch.from_numpy(ev.view(np.uint32).reshape(-1, 4).copy()).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    gx.set_keep_pileups(False)
    gx.set_count_in_peaks(True)
    gx.sample_begin(0, None)
    gx.push_events_device(d_ev.data_ptr(), d_ev.shape[0])
    gx.sample_end()
    gx.sample_no_control()
    gx.pvalues()
    gx.find_peaks()
    n_out = C.c_size_t(0)
    t_cnt, t_sub = [], []
    for k in range(warmup + steps):
        gx.set_phase_timing(2)
        gx.count_in_peaks()
        gx._check(gx.lib.gx_subsample_kept(gx.ctx, 0, 1, 1 << 32, None, 0, C.byref(n_out)))
        gx.set_phase_timing(0)
        ph = gx.phase_times()
        if k >= warmup:
            t_cnt.append([ms for nm, ms in ph if nm == "count"][-1])
            t_sub.append([ms for nm, ms in ph if nm == "subsample"][-1])
    assert n_out.value == len(ev)
    gx.reset()
    return t_cnt, t_sub


def run(gx, name, tags, lens, steps, warmup, t_cnt, t_sub):
    t_set, t_corr = [], []
    got = None
    for k in range(warmup + steps):
        gx.set_phase_timing(2)
        got = gx.xcor_tags(lens, tags, LO, HI)
        gx.set_phase_timing(0)
        ph = gx.phase_times()
        if k >= warmup:
            t_set.append([ms for nm, ms in ph if nm == "xcor.set"][-1])
            t_corr.append([ms for nm, ms in ph if nm == "xcor.corr"][-1])
    nP, nM, n11, nz = numpy_counts(tags, (0, 200))
    assert (got.n_plus, got.n_minus, got.rejected, got.n_pos) == (nP, nM, 0, sum(lens)) and all(got.n11[d - LO] == v for d, v in n11.items())
    med = statistics.median
    blocks = (HI - LO + 1 + 63) // 64
    words = (sum(lens) + 63) // 64
    out = dict(workload=name, tags=int(len(tags)), n_plus=nP, n_minus=nM, shifts=HI - LO + 1, shift_blocks=blocks, genome_words=words,
               nonzero_plus_words=nz, nonzero_share=round(nz / words, 4), vector_bytes=2 * 8 * words, set_ms=mmm(t_set), corr_ms=mmm(t_corr),
               count_phase_ms=mmm(t_cnt), subsample_phase_ms=mmm(t_sub), million_tags_per_s_set=round(len(tags) / med(t_set) / 1e3, 1),
               word_blocks_per_ns=round(nz * blocks / med(t_corr) / 1e6, 3), vectors_gb_per_s_corr=round(2 * 8 * words / med(t_corr) / 1e6, 1),
               corr_to_count=round(med(t_corr) / med(t_cnt), 2), corr_to_subsample=round(med(t_corr) / med(t_sub), 2),
               set_to_subsample=round(med(t_set) / med(t_sub), 2), path_bit=bool(gx.path_info() & GX_PATH_XCOR), checked_against_numpy=True)
    return out


def table(o):
    rows = [("xcor.set (k_xc_set, tags on the device)", o["set_ms"]), ("xcor.corr (k_xc_corr, %d shifts)" % o["shifts"], o["corr_ms"]),
            ("count (k_cnt_index, k_cnt_count, k_cnt_scan), all fragments", o["count_phase_ms"]),
            ("subsample at 100 % (k_sub_count, scan, k_sub_write), all fragments", o["subsample_phase_ms"])]
    out = [f"strand cross-correlation, {o['workload']}: {o['tags']} tags, {o['n_plus']} + {o['n_minus']} positions, {o['nonzero_plus_words']} of "
           f"{o['genome_words']} plus words non-zero ({100 * o['nonzero_share']:.1f} %), vectors {o['vector_bytes'] / 1e6:.0f} MB",
           f"{'phase':<70}{'min ms':>10}{'median ms':>11}{'max ms':>10}"]
    for name, t in rows:
        out.append(f"{name:<70}{t['min']:>10.3f}{t['median']:>11.3f}{t['max']:>10.3f}")
    out.append(f"k_xc_set: {o['million_tags_per_s_set']} million tags a second; k_xc_corr: {o['word_blocks_per_ns']} (non-zero plus word, block of 64 shifts) "
               f"pairs per ns over {o['shift_blocks']} blocks, {o['vectors_gb_per_s_corr']} GB/s of the two vectors; the pass is {o['corr_to_count']} times the count "
               f"phase and {o['corr_to_subsample']} times the subsample pass of all fragments")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", help="also write the text tables there")
    a = ap.parse_args()
    cfg = dict(bench.CONFIGS[2])
    lens = synth.HG38_LENS
    (tv, _), = bench.build_workload(cfg, a.frags, lens)
    ln = np.asarray(lens, dtype=np.int64)[tv["chrom"].astype(np.int64)]
    tv = tv[(tv["end"].astype(np.int64) <= ln) & (tv["end"] > tv["start"])]          # (whole fragments: the last base lies on the chromosome)
    gx = Genrich(GxParams(minus_log10f(0.01), 0, 200.0, 0, 100, 0, 0))
    gx.set_chroms(lens)
    t_cnt, t_sub = kept_passes(gx, tv, lens, a.steps, a.warmup)
    tags = tags_of(tv)
    geo = dict(zip(("lanes", "grid", "tile_words", "pad_words_for_4096", "flush_words"), xcor_geometry()))
    text = [f"geometry: {json.dumps(geo)}\n"]
    for name, t in ((f"config 2, {len(tv)} fragments", tags), ("a fifth of the tags", tags[: 2 * (len(tv) // 5)])):
        o = run(gx, name, t, lens, a.steps, a.warmup, t_cnt, t_sub)
        print(json.dumps(o), flush=True)
        text.append(table(o))
    gx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(text))


if __name__ == "__main__":
    main()
