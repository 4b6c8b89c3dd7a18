"""The samples' fingerprint (include/genrich_amd.h, gx_coverage_fingerprint) in Python integers and fractions, for the tests.

class(x): x < 64: x; else e = floor(log2 x), (e - 6) 64 + (x >> (e - 6)).  hist(rows) -> per row count[k] and sum[k] over the
NC = 3776 classes, Python ints.  The curve passes through (C_k / n, T_k / T) for every non-empty class in ascending order;
metrics() makes the figures from those as fractions.Fraction (jsd_control: a float, the logarithms are not rational)."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

SUB_LOG = 6
NC = (64 - SUB_LOG + 1) << SUB_LOG
HEADER = "sample\tlo120\thi120\tbins\tsum120\tcum_bins\tcum_signal"
METRICS_HEADER = "sample\tbins\tzero_bins\tsum120\tzero_fraction\tauc\tgini\telbow_bins\telbow_gap\tjsd_control"
FIGURES = ("zero_fraction", "auc", "gini", "elbow_bins", "elbow_gap", "jsd_control")


def cls(x):
    x = int(x)
    assert 0 <= x < 1 << 64
    if x < 1 << SUB_LOG:
        return x
    e = x.bit_length() - 1
    return (e - SUB_LOG) * (1 << SUB_LOG) + (x >> (e - SUB_LOG))


def lo(k):
    assert 0 <= k < NC
    if k < 2 << SUB_LOG:
        return k
    q = k // (1 << SUB_LOG) - 1
    return (k - (q << SUB_LOG)) << q


def hi(k):
    if k < 2 << SUB_LOG:
        return k
    q = k // (1 << SUB_LOG) - 1
    return lo(k) + (1 << q) - 1


def cls_array(a):
    """cls() of a uint64 array, in numpy."""
    a = np.asarray(a, dtype=np.uint64)
    e = np.zeros(a.shape, dtype=np.int64)
    t = a.copy()
    for s in (32, 16, 8, 4, 2, 1):
        m = (t >> np.uint64(s)) != 0
        e[m] += s
        t[m] >>= np.uint64(s)
    sh = np.maximum(e - SUB_LOG, 0)
    return np.where(a < (1 << SUB_LOG), a.astype(np.int64), sh * (1 << SUB_LOG) + (a >> sh.astype(np.uint64)).astype(np.int64))


def hist(rows):
    """rows: a list of non-negative integer arrays -> (count, sum): per row a list of NC Python ints each.  The sums are taken
    over the values' 32-bit halves (fewer than 2^32 values: no uint64 sum can wrap) and joined as Python ints."""
    count, total = [], []
    for r in rows:
        a = np.asarray(r).astype(np.uint64)
        assert a.size < 1 << 32
        k = cls_array(a)
        order = np.argsort(k, kind="stable")
        a, k = a[order], k[order]
        c = np.bincount(k, minlength=NC)
        t = [0] * NC
        present = np.flatnonzero(c)
        if len(present):
            starts = np.searchsorted(k, present)
            low = np.add.reduceat(a & np.uint64(0xFFFFFFFF), starts)
            high = np.add.reduceat(a >> np.uint64(32), starts)
            for kk, l, h in zip(present, low, high):
                t[kk] = int(l) + (int(h) << 32)
        count.append([int(v) for v in c])
        total.append(t)
    return count, total


def add(a, b):
    """The histograms of two contexts (or of two sets of bins), added."""
    return ([[x + y for x, y in zip(ra, rb)] for ra, rb in zip(a[0], b[0])],
            [[x + y for x, y in zip(ra, rb)] for ra, rb in zip(a[1], b[1])])


def points(count, total):
    """One sample's [(k, C_k, T_k)] over its non-empty classes, and (n, T)."""
    out, C, T = [], 0, 0
    for k in range(NC):
        if count[k]:
            C += count[k]
            T += total[k]
            out.append((k, C, T))
    return out, C, T


def metrics(count, total, ctrl_of=None):
    """Per sample a dict of the figures: Fractions, None where the definition divides by 0; jsd_control a float or None."""
    S = len(count)
    ctrl_of = [-1] * S if ctrl_of is None else ctrl_of
    out = []
    for s in range(S):
        pts, n, T = points(count[s], total[s])
        m = dict.fromkeys(FIGURES)
        m["bins"], m["zero_bins"], m["sum120"] = n, count[s][0], T
        if n:
            m["zero_fraction"] = Fraction(count[s][0], n)
        if n and T:
            auc, p0, l0, best = Fraction(0), Fraction(0), Fraction(0), None
            for k, C, L in pts:
                p, l = Fraction(C, n), Fraction(L, T)
                auc += (p - p0) * (l + l0) / 2
                if best is None or p - l > best:
                    best = p - l
                    m["elbow_bins"], m["elbow_gap"] = p, p - l
                p0, l0 = p, l
            m["auc"], m["gini"] = auc, 1 - 2 * auc
        c = ctrl_of[s]
        if c >= 0 and n and sum(count[c]):
            nc = sum(count[c])
            js = 0.0
            for k in range(NC):
                p, q = Fraction(count[s][k], n), Fraction(count[c][k], nc)
                mid = (p + q) / 2
                for v in (p, q):
                    if v:
                        js += float(v) * math.log2(v / mid) / 2
            m["jsd_control"] = math.sqrt(max(js, 0.0))
        out.append(m)
    return out


def curve_rows(names, count, total):
    """[(name, lo, hi, bins, sum, cum_bins, cum_signal)]: integers, then two Fractions (cum_signal None with T == 0)."""
    rows = []
    for s, name in enumerate(names):
        pts, n, T = points(count[s], total[s])
        for k, C, L in pts:
            rows.append((name, lo(k), hi(k), count[s][k], total[s][k], Fraction(C, n), Fraction(L, T) if T else None))
    return rows


def _frac(v):
    return "nan" if v is None else f"{float(v):.6f}"


def curve_text(names, count, total):
    return "\n".join([HEADER] + ["\t".join([r[0]] + [str(x) for x in r[1:5]] + [_frac(r[5]), _frac(r[6])])
                                 for r in curve_rows(names, count, total)]) + "\n"


def metrics_text(names, count, total, ctrl_of=None):
    ms = metrics(count, total, ctrl_of)
    return "\n".join([METRICS_HEADER] + ["\t".join([name, str(m["bins"]), str(m["zero_bins"]), str(m["sum120"])] + [_frac(m[f]) for f in FIGURES])
                                         for name, m in zip(names, ms)]) + "\n"


TOL = Fraction(1, 10 ** 6)   # one unit of the last printed digit


def _check(text, header, want_rows, n_int):
    """want_rows: per row the n_int integer columns' texts (the name first), then the exact values of the others (None: nan).
    The integer columns byte-equal, every printed fraction within TOL of its exact value.  -> None or a message."""
    lines = text.split("\n")
    if lines[-1] != "" or lines[0] != header or len(lines) - 2 != len(want_rows):
        return f"{len(lines) - 2} rows for {len(want_rows)}, or another header: {lines[0]!r}"
    for line, want in zip(lines[1:-1], want_rows):
        f = line.split("\t")
        if len(f) != len(want) or f[:n_int] != [str(x) for x in want[:n_int]]:
            return f"{line!r} for {want!r}"
        for x, y in zip(f[n_int:], want[n_int:]):
            if (x == "nan") != (y is None):
                return f"{line!r} for {want!r}"
            if y is not None and (len(x.split(".")[-1]) != 6 or abs(Fraction(x) - Fraction(y)) > TOL):
                return f"{line!r} for {want!r}: {x} is not within 1e-6 of {float(y)!r}"
    return None


def check_curve(text, names, count, total):
    return _check(text, HEADER, curve_rows(names, count, total), 5)


def check_metrics(text, names, count, total, ctrl_of=None):
    ms = metrics(count, total, ctrl_of)
    return _check(text, METRICS_HEADER, [[name, m["bins"], m["zero_bins"], m["sum120"]] + [m[f] for f in FIGURES] for name, m in zip(names, ms)], 4)
