"""Constructed peaks and events for gx_peak_signal_events (tests/test_peak_signal.py checks tests/peaksig_ref.py on them against
the brute force, tests/test_hip_peak_signal.py the kernels against tests/peaksig_ref.py).  A case is (label, lens, peaks, summit
offsets, events); S is the number of bases a wavefront of k_psig_reduce covers per step (gx_peak_signal_geometry)."""
import numpy as np

import backends as B

COUNTS = [1, 2, 3, 4, 5, 6, 8, 10]   # the weights 120, 60, 40, 30, 24, 20, 15, 12


def events(rows):
    a = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    ev = np.zeros(len(a), dtype=B.EVENT_DTYPE)
    ev["chrom"], ev["start"], ev["end"], ev["count"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    return ev


def around(peaks, length):
    """per peak, an interval of each kind: inside, clipped at either edge, spanning, touching nothing (from pe on, up to ps),
    empty, reversed inside and across either edge; the eight weights in turn"""
    rows, k = [], 0

    def add(c, s, e):
        nonlocal k
        if 0 <= s < length and e >= 0:
            rows.append((c, s, e, COUNTS[k % 8]))
            k += 1
    for c, ps, pe in peaks:
        L, mid = pe - ps, ps + (pe - ps) // 2
        add(c, ps + L // 4, max(ps + L // 4 + 1, pe - L // 4))
        add(c, ps - 5, mid + 1)
        add(c, mid, pe + 9)
        add(c, ps - 3, pe + 3)
        add(c, ps, pe)
        add(c, pe, pe + 20)
        add(c, ps - 20, ps)
        add(c, mid, mid)
        add(c, pe - 1, ps)        # reversed, inside (empty when the peak has one base)
        add(c, mid, ps - 4)       # reversed, across the start
        add(c, pe + 3, mid)       # reversed, across the end
    return rows


def lengths_case(S, big=200_000):
    """the peak lengths around a lane's 4 slots, the wavefront's 64 lanes and its step; two pairs of adjacent peaks"""
    length = 3_000 + 6 * S + big
    peaks, pos = [], 10
    for L in [1, 3, 4, 5, 63, 64, 65, S - 1, S, S + 1, 3 * S + 7, big]:
        peaks.append((0, pos, pos + L))
        pos += L + (0 if L in (4, 64) else 37)
    rng = np.random.default_rng(3)
    n = 4000
    s = rng.integers(0, pos + 100, n)
    ln = rng.integers(0, 600, n)
    e = np.where(rng.random(n) < 0.05, np.maximum(s - ln, 0), s + ln)
    rows = around(peaks, length) + [(0, int(a), int(b), int(c)) for a, b, c in zip(s, e, rng.choice(COUNTS + [7, 0, 11], n))]
    rows += [(0, peaks[1][1] - 2, peaks[5][2] + 2, 2), (0, peaks[6][1] + 1, peaks[10][2] - 1, 3)]   # across five peaks each
    rows += [(1, 5, 50, 1), (2, 5, 50, 1)]       # a chromosome without peaks; one the table does not have
    so = [(pe - ps) // 3 for _, ps, pe in peaks]
    return "lengths", [length, 400], peaks, so, events(rows)


def edges_case(S):
    """a peak from base 0, peaks up to the chromosomes' ends with intervals clamped there, adjacent peaks, a whole chromosome"""
    lens = [1000, 300, 7]
    peaks = [(0, 0, 50), (0, 100, 200), (0, 200, 260), (0, 260, 261), (0, 900, 1000), (1, 0, 300), (2, 6, 7)]
    rows = around(peaks[:5], 1000) + [(0, 950, 1200, 1), (0, 990, 1000, 2), (0, 999, 5000, 3), (0, 0, 1, 4), (0, 0, 5000, 5),
                                      (0, 1000, 1010, 1),                       # start at the length: not an interval
                                      (1, 0, 300, 6), (1, 299, 400, 8), (1, 150, 0, 10), (1, 299, 299, 1), (2, 6, 9, 1), (2, 0, 7, 2)]
    return "edges", lens, peaks, [49, 0, 59, 0, 99, 299, 0], events(rows)


def plateaus_case(S):
    """the maximum reached on two separate plateaus, at a peak's last base, in the last lane of a step and across two steps;
    a peak below zero everywhere, one without any interval"""
    peaks, rows, pos = [], [], 100
    for kind in range(7):
        ps, pe = pos, pos + 3 * S
        peaks.append((0, ps, pe))
        if kind == 0:
            rows += [(0, ps + 10, ps + 20, 1)] * 2 + [(0, ps + S + 5, ps + S + 15, 1)] * 2 + [(0, ps + 2 * S + 1, ps + 2 * S + 2, 2)] * 4
        elif kind == 1:
            rows += [(0, pe - 1, pe + 5, 3), (0, ps, pe, 4)]
        elif kind == 2:
            rows += [(0, ps + S - 1, ps + S, 5)]
        elif kind == 3:
            rows += [(0, ps + S - 1, ps + S + 1, 6), (0, ps + 2 * S, ps + 2 * S + 2, 6)]
        elif kind == 4:
            rows += [(0, pe + 10, ps - 10, 8)]
        elif kind == 5:
            rows += [(0, ps + 2 * S - 1, ps + 2 * S + 1, 10), (0, ps + 7, ps + 5, 1)]
        pos = pe + 50
    return "plateaus", [pos + 100], peaks, [10, 3 * S - 1, S - 1, S, 0, 6, 5], events(rows)


def tiny_peaks_case(S, n=100_000):
    """100,000 peaks of 1-4 bases: the padding and the offsets dominate"""
    i = np.arange(n)
    ps = 10 * i + i % 3
    pe = ps + 1 + i % 4
    length = 10 * n + 50
    rng = np.random.default_rng(9)
    m = 60_000
    s = rng.integers(0, length, m)
    e = s + rng.integers(0, 40, m)
    ev = np.zeros(m + 3, dtype=B.EVENT_DTYPE)
    ev["chrom"] = 0
    ev["start"][:m], ev["end"][:m], ev["count"][:m] = s, e, rng.choice(COUNTS, m)
    ev["start"][m:], ev["end"][m:], ev["count"][m:] = [0, 5000, length - 1], [length + 5, 300_000, 0], [2, 2, 1]   # across thousands of peaks; the last one reversed: below zero where nothing else is
    peaks = np.stack([np.zeros(n, dtype=np.int64), ps, pe], axis=1)
    return "tiny_peaks", [length], peaks, (i % 4) // 2, ev


def small_cases(S):
    """the cases small enough for the brute force when `big` is"""
    return [lengths_case(S, big=2000), edges_case(S), plateaus_case(S)]


def device_cases(S):
    return [lengths_case(S), edges_case(S), plateaus_case(S), tiny_peaks_case(S)]
