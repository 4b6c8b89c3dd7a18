"""What tools/gram_bench.py, tools/fingerprint_bench.py and tools/spearman_bench.py share: config 2's sample (hg38) on the
device, contexts with 50-base coverage bins that close it S times, and the yardstick -- k_pack (8 B read + 8 B written per
run-length interval: a plain streaming kernel over the same memory), timed by events: the "cover" phase of the sample with a
one-base -E region (gx_sample_end then makes the tight arrays with k_pack ahead of k_cov_bins) minus the "cover" phase without
one."""
from __future__ import annotations

import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W = 50   # the bins' bases


def mmm(xs):
    return dict(min=round(min(xs), 4), median=round(statistics.median(xs), 4), max=round(max(xs), 4), n=len(xs))


class Workload:
    def __init__(self, frags, warmup):
        import torch

        import bench
        from genrich_amd import synth
        from genrich_amd.lib import GxParams, minus_log10f

        self.frags, self.warmup = frags, warmup
        self.cfg = dict(bench.CONFIGS[2])
        self.lens = synth.HG38_LENS
        (tv, _), = bench.build_workload(self.cfg, frags, self.lens)
        self.d_tv = torch.from_numpy(tv.view(np.uint32).reshape(-1, 4).copy()).to(torch.device("cuda:0"))
        torch.cuda.synchronize()
        self.par = GxParams(minus_log10f(0.01), 0, 200.0, 0, 100, 0, 0)
        self.closed = 0

    def header(self):
        """The JSON line's first keys."""
        return dict(config=2, desc=self.cfg["desc"], fragments=self.frags, bin_size=W, samples={})

    def make(self, beds=None):
        from genrich_amd.lib import Genrich
        gx = Genrich(self.par)
        gx.set_chroms(self.lens, None, beds)
        gx.set_keep_pileups(False)
        gx.set_coverage_bins(W)
        return gx

    def close_sample(self, gx, n_events):
        gx.sample_begin(0, None)
        gx.push_events_device(self.d_tv.data_ptr(), n_events)
        gx.sample_end()
        gx.sample_no_control()
        gx.pvalues()

    def cover_ms(self, gx):
        out = []
        for i in range(self.warmup + 5):
            gx.reset()
            gx.set_phase_filter("cover")
            self.close_sample(gx, self.d_tv.shape[0])
            if i >= self.warmup:
                out.append([ms for name, ms in gx.phase_times() if name == "t.cover"][-1])
            gx.set_phase_timing(0)
        return out

    def k_pack(self):
        """(an idle context without regions, k_pack's record, its ns per KB): the difference of two event-timed phases."""
        beds = [[] for _ in self.lens]
        beds[-1] = [self.lens[-1] - 1, self.lens[-1]]
        gx = self.make(beds)
        with_pack = self.cover_ms(gx)
        n_iv = gx.interval_total(0)
        gx.close()
        gx = self.make()
        without = self.cover_ms(gx)
        pack_ms = statistics.median(with_pack) - statistics.median(without)
        pack_bytes = 16 * n_iv
        ns_per_kb = pack_ms * 1e6 / (pack_bytes / 1e3)
        rec = dict(cover_ms_with=mmm(with_pack), cover_ms_without=mmm(without), ms=round(pack_ms, 4), bytes=int(pack_bytes),
                   ns_per_kb=round(ns_per_kb, 4), tb_per_s=round(pack_bytes / (pack_ms * 1e-3) / 1e12, 3))
        gx.reset()
        self.closed = 0
        return gx, rec, ns_per_kb

    def close_up_to(self, gx, S):
        """S samples of one run: every one the same fragments but for its last r * 1000."""
        while self.closed < S:
            self.close_sample(gx, self.d_tv.shape[0] - 1000 * self.closed)
            self.closed += 1

    def rows(self, gx, S):
        """The S samples' bins as the library gives them, chromosome after chromosome."""
        return [np.concatenate([gx.coverage(i, c).sum120 for c in range(len(self.lens))]) for i in range(S)]
