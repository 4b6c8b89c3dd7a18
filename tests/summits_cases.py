"""Constructed peaks and events for gx_peak_summits_events (tests/test_summits.py checks tests/summits_ref.py on them against
the brute force, tests/test_hip_summits.py the kernels against tests/summits_ref.py).  A depth profile is a list of small
integers u: the depth is 12 u (weight 12 = 120 / 10) on the peak's bases, made of one interval per maximal stretch and level --
below zero of intervals that end before they start.  A case is (lens, peaks, events)."""
import numpy as np

import backends as B

UNIT = 12


def events(rows):
    a = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    ev = np.zeros(len(a), dtype=B.EVENT_DTYPE)
    ev["chrom"], ev["start"], ev["end"], ev["count"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    return ev


def profile_rows(chrom, start, u):
    """event rows whose depth is 12 u[x] at start + x and 0 around"""
    u = np.asarray(u, dtype=np.int64)
    rows = []
    for sign in (1, -1):
        lv = np.maximum(sign * u, 0)
        for level in range(1, int(lv.max()) + 1 if len(lv) else 1):
            m = np.diff(np.concatenate([[0], (lv >= level).astype(np.int64), [0]]))
            for a, b in zip(np.flatnonzero(m == 1), np.flatnonzero(m == -1)):
                rows.append((chrom, start + int(a), start + int(b), 10) if sign > 0 else (chrom, start + int(b), start + int(a), 10))
    return rows


def layout(profiles, gap=9, chrom_tail=50, adjacent=()):
    """profiles one after another on chromosome 0 from base 7 on, `gap` bases apart (index in `adjacent`: none before it)"""
    peaks, rows, pos = [], [], 7
    for i, u in enumerate(profiles):
        if i in adjacent:
            pos -= gap
        peaks.append((0, pos, pos + len(u)))
        rows += profile_rows(0, pos, u)
        pos += len(u) + gap
    return [pos + chrom_tail, 100], peaks, events(rows)


def sawtooth(n, run=1, lo=1, hi=2):
    """n runs of `run` bases each, lo and hi in turn"""
    return np.repeat(np.where(np.arange(n) % 2 == 0, lo, hi), run)


def walk(rng, L, top=5):
    """a random profile of length L in [-1, top] with plateaus"""
    steps = rng.choice([-1, 0, 0, 1], L)
    return np.clip(np.cumsum(steps) + int(rng.integers(0, top)), -1, top)


def noise(rng, n, top):
    """a random profile of about n runs of one or two bases in [-1, top)"""
    return np.repeat(rng.integers(-1, top, n), rng.integers(1, 3, n))


def constructed(step):
    """label -> (lens, peaks, events); step: the bases a wavefront covers per step"""
    rng = np.random.default_rng(5)
    out = {}
    out["lengths"] = layout([walk(rng, L) for L in (1, 3, 4, 5, step - 1, step, step + 1, 3 * step + 7)] + [[3], [0], [-2]])
    flat = np.full(300, 3)
    left = np.concatenate([np.full(6, 4), np.full(100, 2), [3], np.full(20, 1)])
    right = np.concatenate([np.full(20, 1), [3], np.full(100, 2), np.full(7, 4)])
    lane = np.concatenate([np.full(3, 1), np.full(3, 5), np.full(10, 2)])                    # a plateau over bases 3..5
    stepb = np.concatenate([np.full(step - 6, 1), np.full(12, 4), np.full(30, 0), [2, 2], np.full(9, 1)])   # one over step - 6 .. step + 5
    last = np.concatenate([np.full(step + 2, 2), [5]])                                        # L = step + 3, the maximum at L - 1
    twins = np.concatenate([[1, 1], np.full(5, 6), [2, 2, 2], np.full(4, 6), [0]])
    stairs = np.concatenate([np.repeat(np.arange(1, 6), 3), np.repeat(np.arange(4, 0, -1), 2)])
    out["plateaus"] = layout([flat, left, right, lane, stepb, last, twins, stairs])
    out["thresholds"] = layout([[8, 3, 4, 0],       # prominence * 100 == 25 * h and h * 100 == 50 * hmax
                                [10, 4, 5, 0],      # the prominence one unit short
                                [9, 3, 4, 0],       # the height one unit short
                                [0, 4, 3, 8],       # mirrored
                                [4, 3, 8, 3, 4, 3, 4, 0]])
    out["negative"] = layout([[-2, -1, -3], [0, 0, 0], [-1, 2, -1, 1, -2], [-3, 0, -3], [0, 1, 0], [-1, -1, 3, 3, -2, 1]])
    lens, peaks, ev = layout([walk(rng, 40), walk(rng, 70)])
    span = events([(0, peaks[0][1] - 3, peaks[0][2] + 3, 1), (0, peaks[1][1], peaks[1][2], 2), (0, peaks[1][2] + 2, peaks[0][1] - 2, 3)])
    out["spanning"] = (lens, peaks, np.concatenate([ev, span]))
    a = np.concatenate([[1, 2, 1], np.full(4, 5)])
    b = np.concatenate([np.full(3, 5), [1, 3, 0]])
    out["adjacent"] = layout([a, b, [2, 7], [7, 7, 1]], adjacent=(1, 3))                    # a plateau across either border
    out["many"] = layout([walk(rng, int(rng.integers(1, 40))) for _ in range(300)], gap=3)
    return out


def limits(run_cap, lib_cap):
    """sawtooth peaks around run_cap runs and far beyond it, around the library's capacity, and one of longer runs; two random
    profiles of many runs, whose walks cross blocks of runs and end inside them"""
    rng = np.random.default_rng(11)
    return layout([sawtooth(run_cap - 1), sawtooth(run_cap), sawtooth(run_cap + 1), sawtooth(1000), sawtooth(run_cap + 1, run=3, lo=2, hi=1),
                   sawtooth(lib_cap), sawtooth(lib_cap + 1), [1, 2, 1], noise(rng, 700, 9), noise(rng, 2500, 12)])


def five():
    """one peak with five summits, a second without depth"""
    return layout([[1, 3, 1, 3, 1, 4, 1, 3, 1, 3, 1], [0, 0]])
