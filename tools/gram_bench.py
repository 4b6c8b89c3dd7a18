"""The samples' Gram sums (gx_coverage_gram: k_gram + k_gram_sum) at benchmark size: config 2's sample (hg38, 50 M fragments)
closed S times with 50-base bins -- 61.8 M bins per sample, sparse as a real track is -- for S = 2, 4, 8, 16.

  python tools/gram_bench.py [--frags N] [--steps K] [--warmup W] [--samples 2,4,8,16]

Per S it reports
  * the pass's device time: the library's "gram" phase (HIP events on its stream, bracketing exactly k_gram and k_gram_sum;
    gx_set_phase_filter) after a warm-up, as min / median / max over K calls (K >= 20);
  * the bytes the pass must read, 8 S n, the TB/s that makes, and the ns per KB;
  * the ratio of that per-byte cost to k_pack's on the same device in the same process.
k_pack (8 B read + 8 B written per run-length interval: a plain streaming kernel over the same memory) is timed by events too:
the "cover" phase of the same sample with a one-base -E region (gx_sample_end then makes the tight arrays with k_pack ahead of
k_cov_bins) minus the "cover" phase without one.
One S = 2 result is checked against numpy at full size (float64 sums of products are not exact there: to 1e-9 relative), the
counters exactly.  One JSON line."""
from __future__ import annotations

import argparse
import json
import statistics

import numpy as np

from binstat_bench_common import Workload, mmm


def run(frags, steps, warmup, sample_counts):
    from genrich_amd.lib import GX_PATH_GRAM

    w = Workload(frags, warmup)
    out = w.header()
    gx, out["k_pack"], pack_ns_per_kb = w.k_pack()
    for S in sample_counts:
        w.close_up_to(gx, S)
        gx.set_phase_filter("gram")
        for _ in range(warmup + steps):
            n, n_zero, _, _ = gx.coverage_gram()
        ms = [t for name, t in gx.phase_times() if name == "gram"][-steps:]
        gx.set_phase_timing(0)
        assert len(ms) == steps and gx.path_info() & GX_PATH_GRAM
        must_read = 8 * S * n
        med = statistics.median(ms)
        ns_per_kb = med * 1e6 / (must_read / 1e3)
        out["samples"][str(S)] = dict(n_bins=int(n), n_zero=int(n_zero), bytes_must_read=int(must_read), gram_device_ms=mmm(ms),
                                      tb_per_s=round(must_read / (med * 1e-3) / 1e12, 3), ns_per_kb=round(ns_per_kb, 4),
                                      vs_k_pack_per_byte=round(ns_per_kb / pack_ns_per_kb, 2))
        if S == sample_counts[0]:
            n, n_zero, s, g = gx.coverage_gram()
            rows = w.rows(gx, S)
            assert n == len(rows[0]) and n_zero == int((np.bitwise_or.reduce(rows) == 0).sum())
            for i in range(S):
                assert int(s[i]) == int(rows[i].sum())
                for j in range(S):
                    want = float(np.dot(rows[i].astype(np.float64), rows[j].astype(np.float64)))
                    assert abs(float(int(g[i][j])) - want) <= 1e-9 * want, (i, j)
            out["samples"][str(S)]["checked_against_numpy"] = True
    gx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", default="2,4,8,16")
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps: the median of at least 20")
    print(json.dumps(run(a.frags, a.steps, a.warmup, [int(x) for x in a.samples.split(",")])), flush=True)


if __name__ == "__main__":
    main()
