"""The four *_events hooks (gx_complexity_events, gx_interval_stats_events, gx_peak_signal_events, gx_subsample_events) read a
caller's events from ONE upload buffer of the context, and the kept samples' staging area with them.  Called back to back on
one context -- with a little more than two reader chunks of events, then 5, then none -- each gives what it gives on a fresh
context, and the short rounds show nothing of the long one.  A normal two-sample run on the same context afterwards equals the
Python references (complexity_ref, lengths_ref, depth_ref), and the counted lists of the interval lengths and of the depth
distribution, started with room for one entry, run exactly once more with the counted size.  Every figure is an integer: ==."""
import numpy as np
import pytest

import backends as B
import complexity_ref as CR
import depth_ref as DR
import lengths_ref as LR
import peaksig_ref as PR
from genrich_amd.lib import depth_geometry, interval_stats_geometry
from test_hip_kept_reader import CHUNK           # gx_kept.h CNT_CHUNK: the events of one reader chunk

pytestmark = pytest.mark.gpu

LENS = [5000, 3000]
PEAKS = [(0, 1000, 2000), (1, 500, 1500)]
KEEP_ALL = 1 << 32                               # every draw lies below it
LONG = [(0, 0, 4096, 1), (0, 100, 4300, 2), (0, 400, 4900, 1), (0, 450, 4950, 3), (0, 0, 5000, 1)]   # lengths the interval pass lists (>= its LDS bound)


def _events(n, seed):
    rng = np.random.default_rng(seed)
    ev = np.zeros(n, dtype=B.EVENT_DTYPE)
    ev["chrom"] = rng.random(n) < 3 / 8
    length = np.asarray(LENS)[ev["chrom"]]
    ev["start"] = rng.integers(0, length - 60)
    ev["end"] = np.minimum(ev["start"] + rng.integers(30, 600, n), length)
    ev["count"] = rng.choice((1, 2, 3), n)
    return ev


def _rows(rows):
    ev = np.zeros(len(rows), dtype=B.EVENT_DTYPE)
    for f, col in zip(("chrom", "start", "end", "count"), zip(*rows)):
        ev[f] = col
    return ev


def _ctx():
    import genrich_amd
    h = genrich_amd.Genrich(B.make_params(pq=0.01, min_auc=20.0))
    h.set_chroms(LENS)
    return h


HOOKS = {
    "complexity": lambda h, ev, list_cap=0: h.complexity_events(ev),
    "lengths": lambda h, ev, list_cap=0: h.interval_stats_events(ev, 0, list_cap),
    "peak signal": lambda h, ev, list_cap=0: h.peak_signal_events(ev, PEAKS),
    "subsample": lambda h, ev, list_cap=0: h.subsample_events(ev, 7, 0, KEEP_ALL),
}


def _same(name, a, b):
    if name == "peak signal":
        return PR.same(a, b) is None
    if name == "subsample":
        return a.dtype == b.dtype and np.array_equal(a, b)
    return a == b


def test_hooks_back_to_back_then_a_normal_run():
    assert interval_stats_geometry()[2] <= 4096 and DR.DEPTH_BOUND < 3000      # (what LONG and the tower below rely on)
    long_ev = _rows(LONG)
    big = np.concatenate([_events(2 * CHUNK + 100, 11), long_ev])
    big = big[np.random.default_rng(12).permutation(len(big))]
    five = _rows([(1, 10, 90, 1), (1, 10, 90, 1), (0, 4000, 4700, 2), (1, 2000, 2600, 3), (0, 1500, 1501, 1)])
    h = _ctx()
    for label, ev in (("two chunks and a little", big), ("five", five), ("none", big[:0])):
        got = {}
        for name, hook in HOOKS.items():           # back to back on the one context; the long round's list starts with one entry
            got[name] = hook(h, ev, 1 if ev is big else 0)
            if name == "lengths" and ev is big:
                cap, reruns = h.interval_stats_last()
                assert reruns == 1 and len({e - s for _, s, e, _ in LONG}) <= cap <= len(LONG), (cap, reruns)
        for name, hook in HOOKS.items():
            fresh = _ctx()
            assert _same(name, got[name], hook(fresh, ev)), (label, name)
            fresh.close()
        # ... and what the references say, so that a round cannot agree with a fresh context on the wrong figures
        assert got["complexity"] == CR.of_events(ev, LENS), label
        assert LR.Stats(*got["lengths"][:6]) == LR.of_events(ev, LENS), label
        assert np.array_equal(got["subsample"], ev), label
        assert got["complexity"][0] == len(ev) == sum(got["lengths"].cn), label      # nothing of an earlier round
        if ev is five:
            assert got["peak signal"].covered.tolist() == [1, 0] and got["peak signal"].area.tolist() == [120, 0]
        if not len(ev):
            assert not got["peak signal"].area.any() and not got["peak signal"].covered.any()

    # a normal run on the same context: a treatment with a pile deeper than the depth pass counts in LDS, and a control
    rng = np.random.default_rng(5)
    tower = np.zeros(4000, dtype=B.EVENT_DTYPE)
    tower["start"] = 1000 + rng.integers(0, 300, len(tower))
    tower["end"] = tower["start"] + rng.integers(50, 900, len(tower))
    tower["count"] = 1
    treat = np.concatenate([_events(20_000, 21), long_ev, tower])
    treat = treat[rng.permutation(len(treat))]
    ctrl = _events(9000, 22)
    exp_t, exp_c = DR.hist(treat, LENS), DR.hist(ctrl, LENS, is_ctrl=True)
    assert len(exp_t.deep) > 1 and not exp_c.deep
    h.set_count_in_peaks(True)
    h.set_depth_hist(True)
    h.set_knob("GX_DEPTH_LIST_CAP", 1)
    h.sample_begin(0, None)
    h.push_events(treat)
    h.sample_end()
    cap, reruns = h.depth_last()
    assert reruns == 1 and len(exp_t.deep) <= cap < depth_geometry()[3], (cap, reruns)   # (one entry per piece: at least one per distinct v)
    h.sample_begin(1, None)
    h.push_events(ctrl)
    h.sample_end()
    assert h.depth_last() == (1, 0)
    assert DR.same(h.depth(0), exp_t) is None and DR.same(h.depth(1), exp_c) is None
    assert h.complexity() == 2 and h.interval_stats() == 2
    for i, (ev, is_ctrl) in enumerate(((treat, False), (ctrl, True))):
        c, s = h.get_complexity(i), h.get_interval_stats(i)
        assert (c.n_obs, c.n_distinct, c.pairs) == CR.of_events(ev, LENS) and (c.rep, c.is_ctrl) == (0, is_ctrl)
        assert LR.Stats(*s[:6]) == LR.of_events(ev, LENS) and (s.rep, s.is_ctrl) == (0, is_ctrl)
    assert h.interval_stats_last() == (interval_stats_geometry()[4], 0)
    h.close()
