"""Each sample's own depth inside the peaks (gx_peak_signal, genrich-amd --peak-signal) restated in numpy, a brute force that
applies the definition base by base and interval by interval, and the text of --peak-signal.

A sample's intervals are those gx_count_in_peaks counts: count in {1, 2, 3, 4, 5, 6, 8, 10}, a chromosome of the table that is
active, start below its length, the end clamped to the length; weight 120 / count.  depth = the prefix sum of +w at s, -w at e:
an empty interval adds nothing, one with e < s adds -w over [e, s).  Per peak [ps, pe): area, max, the first base of the max
(from ps), the bases with depth > 0, the depth at ps + summit_off."""
from typing import NamedTuple

import numpy as np

VALID = np.zeros(11, dtype=bool)
VALID[[1, 2, 3, 4, 5, 6, 8, 10]] = True


class Signal(NamedTuple):
    area: np.ndarray       # int64, 1/120 units
    max: np.ndarray        # int64
    summit: np.ndarray     # int64 (bases from the peak's start)
    covered: np.ndarray    # int64 (bases)
    at_summit: np.ndarray  # int64
    rep: int = 0
    is_ctrl: bool = False


def intervals(ev, lens, active=None):
    """(chrom, start, clamped end, weight) int64 arrays of the events that are the sample's intervals."""
    lens = np.asarray(lens, dtype=np.int64)
    c, s, e, n = (ev[f].astype(np.int64) for f in ("chrom", "start", "end", "count"))
    ok = (n <= 10) & VALID[np.minimum(n, 10)] & (c < len(lens))
    cc = np.minimum(c, len(lens) - 1)
    ok &= s < lens[cc]
    if active is not None:
        ok &= np.asarray(active, dtype=bool)[cc]
    c, s, e, n = c[ok], s[ok], e[ok], n[ok]
    return c, s, np.minimum(e, lens[c]), 120 // n


def depth_of(c, s, e, w, chrom, length):
    """the depth of one chromosome, int64[length]"""
    m = c == chrom
    wf = w[m].astype(np.float64)
    assert wf.sum() < 2.0 ** 53   # (bincount adds doubles: exact below 2^53)
    d = np.bincount(s[m], weights=wf, minlength=length + 1) - np.bincount(e[m], weights=wf, minlength=length + 1)
    return np.cumsum(np.rint(d).astype(np.int64))[:length]


def signal(ev, lens, peaks, summit_off=None, active=None, rep=0, is_ctrl=False):
    """Signal of the events in `peaks` (rows of (chrom, start, end), sorted and disjoint)."""
    pk = np.asarray(peaks, dtype=np.int64).reshape(-1, 3)
    n = len(pk)
    so = np.zeros(n, dtype=np.int64) if summit_off is None else np.asarray(summit_off, dtype=np.int64)
    out = [np.zeros(n, dtype=np.int64) for _ in range(5)]
    c, s, e, w = intervals(ev, lens, active)
    for chrom in np.unique(pk[:, 0]):
        sel = np.flatnonzero(pk[:, 0] == chrom)
        ps, pe = pk[sel, 1], pk[sel, 2]
        L = pe - ps
        assert (L > 0).all() and (pe <= lens[chrom]).all() and (ps[1:] >= pe[:-1]).all()
        depth = depth_of(c, s, e, w, chrom, int(lens[chrom]))
        first = np.concatenate([[0], np.cumsum(L)[:-1]])           # each peak's first entry in the peaks' bases laid end to end
        x = np.repeat(ps - first, L) + np.arange(L.sum())          # their positions
        d = depth[x]
        mx = np.maximum.reduceat(d, first)
        out[0][sel] = np.add.reduceat(d, first)
        out[1][sel] = mx
        out[2][sel] = np.minimum.reduceat(np.where(d == np.repeat(mx, L), x - np.repeat(ps, L), 1 << 40), first)
        out[3][sel] = np.add.reduceat((d > 0).astype(np.int64), first)
        out[4][sel] = depth[ps + so[sel]]
    return Signal(*out, rep, is_ctrl)


def brute(ev, lens, peaks, summit_off=None, active=None):
    """The definition itself: per peak and base, the sum over the intervals of w [s <= x < e] - w [e <= x < s]."""
    pk = np.asarray(peaks, dtype=np.int64).reshape(-1, 3)
    so = np.zeros(len(pk), dtype=np.int64) if summit_off is None else np.asarray(summit_off, dtype=np.int64)
    c, s, e, w = intervals(ev, lens, active)
    out = [np.zeros(len(pk), dtype=np.int64) for _ in range(5)]
    for k, (chrom, ps, pe) in enumerate(pk):
        m = c == chrom
        x = np.arange(ps, pe)[:, None]
        si, ei, wi = s[m][None, :], e[m][None, :], w[m][None, :]
        d = (wi * ((si <= x) & (x < ei))).sum(axis=1) - (wi * ((ei <= x) & (x < si))).sum(axis=1)
        out[0][k] = d.sum()
        out[1][k] = d.max()
        out[2][k] = int(np.flatnonzero(d == d.max())[0])
        out[3][k] = int((d > 0).sum())
        out[4][k] = d[so[k]]
    return Signal(*out)


def same(a, b):
    """None, or the first figure in which two Signals differ"""
    for f in ("area", "max", "summit", "covered", "at_summit"):
        x, y = np.asarray(getattr(a, f), dtype=np.int64), np.asarray(getattr(b, f), dtype=np.int64)
        if x.shape != y.shape:
            return f, x.shape, y.shape
        if not np.array_equal(x, y):
            k = int(np.flatnonzero(x != y)[0])
            return f, k, int(x[k]), int(y[k])
    return None


def value_text(n):
    n = int(n)
    return str(n // 120) if n % 120 == 0 else "%.2f" % (n / 120.0)


def peak_signal_text(names, peaks, samples):
    """--peak-signal's text: samples = Signals (with rep and is_ctrl) over `peaks` (rows of (chrom, start, end))."""
    head = ["chr", "start", "end", "name"]
    for sm in samples:
        lab = ("c" if sm.is_ctrl else "t") + str(sm.rep)
        head += [f"{lab}.{col}" for col in ("max", "summit", "area", "covered", "at_summit")]
    lines = ["\t".join(head)]
    for k, (c, s, e) in enumerate(peaks):
        row = [names[int(c)], str(int(s)), str(int(e)), f"peak_{k}"]
        for sm in samples:
            row += [value_text(sm.max[k]), str(int(sm.summit[k])), value_text(sm.area[k]), str(int(sm.covered[k])), value_text(sm.at_summit[k])]
        lines.append("\t".join(row))
    return "\n".join(lines) + "\n"
