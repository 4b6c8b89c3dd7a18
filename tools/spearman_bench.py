"""The samples' rank correlation (gx_coverage_spearman_group: per sample k_rank_distinct + k_rank_compact, the host's merge,
k_rank, then k_gram / k_gram_sum over the rank rows) at benchmark size: config 2's sample (hg38, 50 M fragments) closed S times
with 50-base bins -- 61.8 M bins per sample, sparse as a real track is -- for S = 2, 4, 8, 16.

  python tools/spearman_bench.py [--frags N] [--steps K] [--warmup W] [--samples 2,4,8,16]

Per S it reports
  * the whole pass on the host's clock (it has host work in it: the tables' sort and merge, their upload), as min / median / max
    over K calls;
  * each kernel's device time per pass (the library's phases, HIP events on its stream: gx_set_phase_timing(2)), the median of
    the K passes' totals per phase: rank_distinct (its fills included), rank_compact, rank_nzero (with --corr-skip-zeros only),
    rank, gram;
  * the bytes a phase must move -- rank_distinct reads 8 S n, rank reads 8 S n (twice) and writes 8 S n -- and its ns per KB
    relative to k_pack's on the same device in the same process;
  * the Pearson pass (gx_coverage_gram's "gram" phase) over the same samples' bins;
  * D: the distinct values of the sample that has the most, and how often a table grew;
  * both of k_rank's lookups (GX_RANK_LOOKUP: 1 binary search in the sorted table, 2 probing a hashed one) in the same process,
    the same integers asserted from both.
k_pack (8 B read + 8 B written per run-length interval: a plain streaming kernel over the same memory) is timed as
tools/fingerprint_bench.py times it.  The S = 2 result is checked against numpy at full size, exactly.  One JSON line."""
from __future__ import annotations

import argparse
import json
import statistics
import time

import numpy as np

from binstat_bench_common import Workload, mmm


def run(frags, steps, warmup, sample_counts):
    from genrich_amd.lib import GX_PATH_SPEARMAN, coverage_spearman_group

    w = Workload(frags, warmup)

    def spearman_ms(gx, skip):
        """(the passes' wall ms, {phase: the passes' device ms}, the last result)"""
        wall, per = [], {}
        seen = len(gx.phase_times())
        res = None
        for i in range(warmup + steps):
            gx.set_phase_timing(2)
            t0 = time.perf_counter()
            res = coverage_spearman_group([gx], skip)
            t1 = time.perf_counter()
            gx.set_phase_timing(0)
            ph = gx.phase_times()
            new, seen = ph[seen:], len(ph)
            if i < warmup:
                continue
            wall.append((t1 - t0) * 1e3)
            tot = {}
            for name, ms in new:
                tot[name] = tot.get(name, 0.0) + ms
            for name, ms in tot.items():
                per.setdefault(name, []).append(ms)
        assert gx.path_info() & GX_PATH_SPEARMAN
        return wall, per, res

    def pearson_ms(gx):
        gx.set_phase_filter("gram")
        seen = len(gx.phase_times())
        for _ in range(warmup + steps):
            gx.coverage_gram()
        ms = [t for name, t in gx.phase_times()[seen:] if name == "gram"][-steps:]
        gx.set_phase_timing(0)
        return ms

    out = w.header()
    gx, pack, pack_ns_per_kb = w.k_pack()
    out["k_pack"] = {k: pack[k] for k in ("ms", "bytes", "ns_per_kb", "tb_per_s")}
    for S in sample_counts:
        w.close_up_to(gx, S)
        res = {}
        for skip in (False, True):
            by_lookup = {}
            for name, knob in (("binary_search", 1), ("probe", 2), ("default", 0)):
                gx.set_knob("GX_RANK_LOOKUP", knob)
                wall, per, (N, s, g, nd) = spearman_ms(gx, skip)
                by_lookup[name] = dict(rank_device_ms=mmm(per["rank"]), pass_wall_ms=mmm(wall))
                sums = ([int(v) for v in s], [[int(v) for v in row] for row in g])
                assert name == "binary_search" or sums == first, name
                first = sums
            entry = dict(rank_lookup=by_lookup, bins_ranked=int(N), most_distinct_values=int(max(nd)), table_grew=int(gx.rank_last()[1]), pass_wall_ms=mmm(wall),
                         device_ms={k: mmm(v) for k, v in sorted(per.items())})
            res["skip_zeros" if skip else "all_bins"] = entry
            if not skip:
                n_bins = int(N)
                moved = dict(rank_distinct=8 * S * n_bins, rank=24 * S * n_bins, gram=8 * S * n_bins)
                entry["vs_k_pack_per_byte"] = {k: round(statistics.median(per[k]) * 1e6 / (moved[k] / 1e3) / pack_ns_per_kb, 2) for k in moved if k in per}
                entry["bytes_moved"] = {k: int(v) for k, v in moved.items()}
                if S == 2:
                    import rank_ref as K
                    rows = [r.astype(np.uint64) for r in w.rows(gx, S)]
                    _, _, R = K.rank_rows(rows)
                    es = [int(r.astype(object).sum()) for r in R]
                    # (13-bit pieces: products below 2^26, 2^26 of them stay inside a float64's 2^53)
                    eg = sum(int(np.dot(((R[0] >> np.uint64(a)) & np.uint64(0x1FFF)).astype(np.float64),
                                        ((R[1] >> np.uint64(b)) & np.uint64(0x1FFF)).astype(np.float64))) << (a + b)
                             for a in (0, 13, 26) for b in (0, 13, 26))
                    assert int(R.max()) < 1 << 39 and R.shape[1] <= 1 << 26 and [int(v) for v in s] == es and int(g[0][1]) == eg
                    entry["checked_against_numpy"] = True
        res["pearson_gram_device_ms"] = mmm(pearson_ms(gx))
        out["samples"][str(S)] = res
    gx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--samples", default="2,4,8,16")
    a = ap.parse_args()
    if a.steps < 3:
        ap.error("--steps: the median of at least 3")
    print(json.dumps(run(a.frags, a.steps, a.warmup, [int(x) for x in a.samples.split(",")])), flush=True)


if __name__ == "__main__":
    main()
