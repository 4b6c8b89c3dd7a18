"""The samples' fingerprint histograms (gx_coverage_fingerprint: one fill + k_fp_hist) at benchmark size: config 2's sample (hg38,
50 M fragments) closed S times with 50-base bins -- 61.8 M bins per sample, sparse as a real track is -- for S = 1, 2, 4, 8, 16.

  python tools/fingerprint_bench.py [--frags N] [--steps K] [--warmup W] [--samples 1,2,4,8,16]

Per S it reports
  * the pass's device time: the library's "fingerprint" phase (HIP events on its stream, bracketing exactly the fill and
    k_fp_hist; gx_set_phase_filter) after a warm-up, as min / median / max over K calls (K >= 20);
  * the bytes the pass must read, 8 S n, the TB/s that makes, and the ns per KB;
  * the ratio of that per-byte cost to k_pack's on the same device in the same process.
At S = 2 both collision variants are timed: an atomic pair per lane (the default) and aggregation inside the wavefront
(GX_FP_AGG), with the number of distinct non-zero classes of a 64-value step that decides between them.
k_pack (8 B read + 8 B written per run-length interval: a plain streaming kernel over the same memory) is timed by events too:
the "cover" phase of the same sample with a one-base -E region (gx_sample_end then makes the tight arrays with k_pack ahead of
k_cov_bins) minus the "cover" phase without one.
One S = 2 result is checked against numpy at full size, exactly.  One JSON line."""
from __future__ import annotations

import argparse
import json
import statistics

import numpy as np

from binstat_bench_common import Workload, mmm


def run(frags, steps, warmup, sample_counts):
    import fingerprint_ref as R
    from genrich_amd.lib import GX_PATH_FINGERPRINT

    w = Workload(frags, warmup)

    def pass_ms(gx):
        gx.set_phase_filter("fingerprint")
        for _ in range(warmup + steps):
            n, _, _ = gx.coverage_fingerprint()
        ms = [t for name, t in gx.phase_times() if name == "fingerprint"][-steps:]
        gx.set_phase_timing(0)
        assert len(ms) == steps and gx.path_info() & GX_PATH_FINGERPRINT
        return n, ms

    out = w.header()
    gx, out["k_pack"], pack_ns_per_kb = w.k_pack()
    for S in sample_counts:
        w.close_up_to(gx, S)
        n, ms = pass_ms(gx)
        must_read = 8 * S * n
        med = statistics.median(ms)
        ns_per_kb = med * 1e6 / (must_read / 1e3)
        res = dict(n_bins=int(n), bytes_must_read=int(must_read), fingerprint_device_ms=mmm(ms),
                   tb_per_s=round(must_read / (med * 1e-3) / 1e12, 3), ns_per_kb=round(ns_per_kb, 4),
                   vs_k_pack_per_byte=round(ns_per_kb / pack_ns_per_kb, 2))
        if S == 2:
            gx.set_knob("GX_FP_AGG", 1)
            _, ms_agg = pass_ms(gx)
            n2, c_agg, t_agg = gx.coverage_fingerprint()
            gx.set_knob("GX_FP_AGG", 0)
            n1, count, total = gx.coverage_fingerprint()
            assert np.array_equal(count, c_agg) and np.array_equal(total, t_agg)
            res["variants_ms"] = dict(atomics_per_lane=mmm(ms), aggregated_in_the_wavefront=mmm(ms_agg))
            rows = w.rows(gx, S)
            assert n1 == len(rows[0])
            for i in range(S):
                a = rows[i].astype(np.uint64)
                k = R.cls_array(a)
                assert np.array_equal(np.bincount(k, minlength=R.NC).astype(np.uint64), count[i]), i
                want = np.zeros(R.NC, dtype=np.uint64)    # by 16-bit pieces: every piece's sums are exact in a float64
                for sh in (0, 16, 32, 48):
                    piece = np.bincount(k, weights=((a >> np.uint64(sh)) & np.uint64(0xFFFF)).astype(np.float64), minlength=R.NC)
                    want += piece.astype(np.uint64) << np.uint64(sh)
                assert np.array_equal(want, total[i]), i
            res["checked_against_numpy"] = True
            # what the collision variants see: distinct non-zero classes among the 64 values of a wavefront's slot
            k0 = R.cls_array(rows[0].astype(np.uint64))[: (len(rows[0]) // 64) * 64].reshape(-1, 64)[::97]
            srt = np.sort(k0, axis=1)
            distinct = ((srt[:, 1:] != srt[:, :-1]) & (srt[:, 1:] != 0)).sum(axis=1) + (srt[:, 0] != 0)
            res["per_64_values"] = dict(zero=round(float((k0 == 0).mean() * 64), 2), distinct_nonzero_classes=round(float(distinct.mean()), 2),
                                        nonempty_classes_of_the_sample=int((count[0] != 0).sum()))
        out["samples"][str(S)] = res
    gx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", default="1,2,4,8,16")
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps: the median of at least 20")
    print(json.dumps(run(a.frags, a.steps, a.warmup, [int(x) for x in a.samples.split(",")])), flush=True)


if __name__ == "__main__":
    main()
