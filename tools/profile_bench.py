"""Profiles around anchors (gx_set_profile, k_profile) at benchmark size: config 2 (hg38, 50 M fragments, -p 0.01).

  python tools/profile_bench.py [--frags N] [--steps K] [--warmup W] [--cases 20000,1000000] [--plan FILE]
  python tools/profile_bench.py --summarise KERNEL_TRACE.csv --plan FILE

Two cases at F = 2000, B = 10 (400 bins), the anchors drawn uniformly over the genome on either strand: 20,000 anchors with the
matrix kept, 1,000,000 anchors with the aggregate alone.  Per case it reports
  * the pass's device time per sample: the library's "profile" phase (HIP events on its stream, bracketing k_profile and
    k_profile_sum; gx_set_phase_filter) after a warm-up, as min / median / max over K steps;
  * the bytes the pass reads -- 8 B per interval of every tile an anchor's window overlaps, a tile counted once per anchor
    that reaches it (the intervals per tile: the change points of the numpy pileup) -- plus 8 B per cell written, and the TB/s
    that makes;
  * the step (reset, sample from device memory, find_peaks: bench.py's step) with the switch off and on, alternating in the
    same process;
and checks the full-size result against numpy (tests/profile_ref.py's definition by prefix sums per chromosome: the matrix of
the first case, the aggregate of both).  Then the yardstick: the first case with a one-base -E region, where gx_sample_end makes
the tight arrays (k_pack: every slot once, 8 B read + 8 B written per interval) ahead of k_profile.  One JSON line.

Under `rocprofv3 --kernel-trace` the same run yields every launch of k_profile and k_pack; --plan FILE writes the order of the
k_profile launches and the byte counts, and --summarise reads the trace's CSV with that plan: median of the last five launches
of each kind, ns per byte, k_pack's run-to-run spread.  One JSON line."""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F, BIN, TB = 2000, 10, 12
NB = 2 * F // BIN


def mmm(xs):
    return dict(min=round(min(xs), 4), median=round(statistics.median(xs), 4), max=round(max(xs), 4), n=len(xs))


def make_anchors(lens, n, seed):
    from genrich_amd.lib import ANCHOR_DTYPE
    rng = np.random.default_rng(seed)
    a = np.zeros(n, dtype=ANCHOR_DTYPE)
    p = np.asarray(lens, dtype=np.float64)
    a["chrom"] = rng.choice(len(lens), n, p=p / p.sum())
    a["pos"] = (rng.random(n) * np.asarray(lens)[a["chrom"]]).astype(np.int64)
    a["strand"] = rng.choice([1, -1], n)
    return a


def numpy_profiles(ev, lens, anchor_sets, beds=None):
    """Per anchor set: (cell120 int64[n, NB] or None for a set of more than 100,000 anchors, agg120, bytes of intervals read),
    and the intervals of the numpy pileup; one pass over the chromosomes for all the sets."""
    ev = ev[np.argsort(ev["chrom"], kind="stable")]
    cuts = np.searchsorted(ev["chrom"], np.arange(len(lens) + 1))
    cells = [np.zeros((len(a), NB), dtype=np.int64) if len(a) <= 100_000 else None for a in anchor_sets]
    aggs = [np.zeros(NB, dtype=np.int64) for _ in anchor_sets]
    read = [0 for _ in anchor_sets]
    n_iv = 0
    off = np.arange(NB + 1, dtype=np.int64) * BIN
    for c, L in enumerate(lens):
        e = ev[cuts[c]:cuts[c + 1]]
        e = e[e["start"] < L]
        w = (120 // e["count"].astype(np.int64)).astype(np.float64)
        diff = np.bincount(e["start"], weights=w, minlength=L + 1)
        diff -= np.bincount(np.minimum(e["end"], L), weights=w, minlength=L + 1)
        pile = np.cumsum(diff)[:L].astype(np.int64)   # (float64 sums of multiples of 1/120 below 2^53: exact)
        del diff
        for a, b in zip(*(np.asarray(beds[c] if beds else [], dtype=np.int64).reshape(-1, 2).T)):
            pile[a:b] = 0
        ends = np.flatnonzero(pile[1:] != pile[:-1]) + 1          # an interval ends where the pileup changes, and at L
        per_tile = np.bincount((ends - 1) >> TB, minlength=((L - 1) >> TB) + 1)
        per_tile[(L - 1) >> TB] += 1
        n_iv += len(ends) + 1
        tile_cs = np.concatenate([[0], np.cumsum(per_tile)])
        cs = np.concatenate([[0], np.cumsum(pile)])
        del pile
        for k, anchors in enumerate(anchor_sets):
            at = np.flatnonzero(anchors["chrom"] == c)
            if not len(at):
                continue
            lo = anchors["pos"][at].astype(np.int64) - F + (anchors["strand"][at] < 0)
            clo, chi = np.clip(lo, 0, L), np.clip(lo + 2 * F, 0, L)
            live = clo < chi
            read[k] += 8 * int((tile_cs[((chi[live] - 1) >> TB) + 1] - tile_cs[clo[live] >> TB]).sum())
            for s in range(0, len(at), 50_000):                   # (401 prefix sums per anchor: in slices)
                sl = slice(s, s + 50_000)
                edges = np.clip(lo[sl, None] + off[None, :], 0, L)
                rows = cs[edges[:, 1:]] - cs[edges[:, :-1]]
                minus = anchors["strand"][at[sl]] < 0
                rows[minus] = rows[minus, ::-1]
                aggs[k] += rows.sum(axis=0)
                if cells[k] is not None:
                    cells[k][at[sl]] = rows
    return cells, aggs, read, n_iv


def run(frags, steps, warmup, cases, plan_path):
    import torch

    import bench
    from genrich_amd import synth
    from genrich_amd.lib import GX_PATH_PROFILE, Genrich, GxParams, minus_log10f

    cfg = dict(bench.CONFIGS[2])
    lens = synth.HG38_LENS
    (tv, _), = bench.build_workload(cfg, frags, lens)
    d_tv = torch.from_numpy(tv.view(np.uint32).reshape(-1, 4).copy()).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    par = GxParams(minus_log10f(0.01), 0, 200.0, 0, 100, 0, 0)
    sets = [make_anchors(lens, n, 100 + i) for i, n in enumerate(cases)]
    keep = [n <= 100_000 for n in cases]

    def make(beds=None):
        gx = Genrich(par)
        gx.set_chroms(lens, None, beds)
        gx.set_keep_pileups(False)
        return gx

    def step(gx, k):
        gx.reset()
        if k is None:
            gx.set_profile(sets[0][:0], 0, 0)
        else:
            gx.set_profile(sets[k], F, BIN, keep[k])
        gx.sample_begin(0, None)
        gx.push_events_device(d_tv.data_ptr(), d_tv.shape[0])
        gx.sample_end()
        gx.sample_no_control()
        gx.pvalues()
        return gx.find_peaks()

    def measure(gx, k):
        for _ in range(warmup):
            step(gx, None)
            step(gx, k)
        t_off, t_on, t_dev = [], [], []
        for i in range(2 * steps):
            on = i % 2 == 1
            if on:
                gx.set_phase_filter("profile")
            t0 = time.perf_counter()
            step(gx, k if on else None)
            t1 = time.perf_counter()
            if on:
                t_dev.append([ms for name, ms in gx.phase_times() if name == "t.profile"][-1])
                gx.set_phase_timing(0)
            (t_on if on else t_off).append((t1 - t0) * 1e3)
        return t_off, t_on, t_dev

    exp_cells, exp_aggs, read, n_iv_numpy = numpy_profiles(tv, lens, sets)
    out = dict(config=2, desc=cfg["desc"], fragments=frags, flank=F, bin_size=BIN, intervals_numpy=int(n_iv_numpy), cases={})
    plan = []
    gx = make()
    for k, n in enumerate(cases):
        t_off, t_on, t_dev = measure(gx, k)
        plan += [dict(case=str(n), form="loose")] * (warmup + steps)
        assert gx.path_info() & GX_PATH_PROFILE
        got = gx.profile(0)
        assert np.array_equal(got.agg120, exp_aggs[k]), n
        if keep[k]:
            assert np.array_equal(got.cell120, exp_cells[k]), n
        written = 8 * n * NB if keep[k] else 0
        med = statistics.median(t_dev)
        out["cases"][str(n)] = dict(anchors=n, matrix=keep[k], intervals=int(gx.interval_total(0)), bytes_read=int(read[k]),
                                    bytes_written=int(written), profile_device_ms=mmm(t_dev),
                                    tb_per_s=round((read[k] + written) / (med * 1e-3) / 1e12, 4), step_off_ms=mmm(t_off),
                                    step_on_ms=mmm(t_on), checked_against_numpy=True)
    gx.close()
    # the yardstick's run: one excluded base on the last chromosome -> tight arrays (k_pack), then k_profile on them
    beds = [[] for _ in lens]
    beds[-1] = [lens[-1] - 1, lens[-1]]
    gx = make(beds)
    t_off, t_on, t_dev = measure(gx, 0)
    plan += [dict(case=str(cases[0]), form="tight")] * (warmup + steps)
    n_iv = gx.interval_total(0)
    got = gx.profile(0)
    hit = sets[0]["chrom"] == len(lens) - 1   # (an anchor whose window holds the excluded base may differ: compare the others)
    assert np.array_equal(got.cell120[~hit], exp_cells[0][~hit])
    out["with_one_excluded_base"] = dict(case=str(cases[0]), intervals=int(n_iv), profile_device_ms_with_k_pack=mmm(t_dev),
                                        k_pack_bytes=int(16 * n_iv), checked_against_numpy=True)
    gx.close()
    if plan_path:
        sizes = {k: dict(bytes_read=v["bytes_read"], bytes_written=v["bytes_written"]) for k, v in out["cases"].items()}
        json.dump(dict(launches=plan, sizes=sizes, tight_intervals=int(n_iv), last=steps), open(plan_path, "w"))
    return out


def summarise(trace_csv, plan_path):
    plan = json.load(open(plan_path))
    rows = list(csv.DictReader(open(trace_csv)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6   # ms
    prof = [dur(r) for r in rows if "k_profile" in r["Kernel_Name"] and "k_profile_sum" not in r["Kernel_Name"]]
    psum = [dur(r) for r in rows if "k_profile_sum" in r["Kernel_Name"]]
    pack = [dur(r) for r in rows if "k_pack(" in r["Kernel_Name"] or r["Kernel_Name"].endswith("k_pack")]
    assert len(prof) == len(plan["launches"]) == len(psum), (len(prof), len(psum), len(plan["launches"]))
    last = min(5, plan["last"])
    out = dict(k_profile={}, k_profile_sum={}, launches=len(prof))
    by, by_sum = {}, {}
    for ms, ms2, l in zip(prof, psum, plan["launches"]):
        by.setdefault((l["case"], l["form"]), []).append(ms)
        by_sum.setdefault((l["case"], l["form"]), []).append(ms2)
    for (case, form), xs in by.items():
        sz = plan["sizes"][case]
        b = sz["bytes_read"] + sz["bytes_written"]
        med = statistics.median(xs[-last:])
        out["k_profile"][f"{case}/{form}"] = dict(ms=mmm(xs[-last:]), bytes=b, ns_per_kb=round(med * 1e6 / (b / 1e3), 4),
                                                  tb_per_s=round(b / (med * 1e-3) / 1e12, 4))
        out["k_profile_sum"][f"{case}/{form}"] = mmm(by_sum[(case, form)][-last:])
    if pack:
        xs = pack[-last:]
        b = 16 * plan["tight_intervals"]
        med = statistics.median(xs)
        out["k_pack"] = dict(ms=mmm(xs), bytes=b, ns_per_kb=round(med * 1e6 / (b / 1e3), 4), tb_per_s=round(b / (med * 1e-3) / 1e12, 3),
                             spread_pct=round(100.0 * (max(xs) - min(xs)) / med, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="20000,1000000", help="anchor counts; a case of at most 100,000 anchors keeps its matrix")
    ap.add_argument("--plan", default=None, help="write the order of the k_profile launches here (for --summarise)")
    ap.add_argument("--summarise", metavar="CSV", default=None, help="a rocprofv3 kernel trace of a run made with --plan")
    a = ap.parse_args()
    if a.summarise:
        print(json.dumps(summarise(a.summarise, a.plan)), flush=True)
    else:
        print(json.dumps(run(a.frags, a.steps, a.warmup, [int(x) for x in a.cases.split(",")], a.plan)), flush=True)


if __name__ == "__main__":
    main()
