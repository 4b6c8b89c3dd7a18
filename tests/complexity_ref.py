"""Python restatement of gx_complexity (include/genrich_amd.h) and of the --complexity / --complexity-hist text, for the tests.

A sample's intervals are those gx_count_in_peaks counts (the filter tests/test_hip_counts.py applies before counts_ref: a valid
count, an active chromosome, start < len, the end clamped to len).  Each is one observation of the key (chrom, start, clamped
end); N = observations, D = distinct keys, h[m] = keys seen m times, reported as ascending (m, h[m]) pairs.  The figures are
exact: ratios as fractions.Fraction, the curve as rationals good to 2^-256 of each product, the library size's root bracketed
with decimal at 60 digits."""
from __future__ import annotations

import decimal
from collections import Counter
from fractions import Fraction

import numpy as np

CURVE = 20
VALID_COUNTS = (1, 2, 3, 4, 5, 6, 8, 10)
RATIOS = ("nrf", "pbc1", "pbc2", "dup_fraction")
HEADER = "\t".join(["sample", "N", "D", "h1", "h2", "NRF", "PBC1", "PBC2", "dup_fraction", "library_size"]
                   + [f"c{5 * k:03d}" for k in range(1, CURVE + 1)])
HIST_HEADER = "sample\tmultiplicity\tkeys"


def intervals(ev, lens, active=None):
    """(chrom, start, clamped end) int64 arrays of the events that are a sample's intervals; active: per chromosome, default all."""
    lens = np.asarray(lens, dtype=np.int64)
    ch = ev["chrom"].astype(np.int64)
    ok = np.isin(ev["count"], VALID_COUNTS) & (ch < len(lens))
    chs = np.where(ok, ch, 0)
    if active is not None:
        ok &= np.asarray(active, bool)[chs]
    ok &= ev["start"].astype(np.int64) < lens[chs]
    ch, s, e = ch[ok], ev["start"].astype(np.int64)[ok], ev["end"].astype(np.int64)[ok]
    return ch, s, np.minimum(e, lens[ch])


def histogram(keys):
    """keys: an iterable of hashable keys -> (N, D, [(m, h[m])] ascending)."""
    c = Counter(keys)
    h = Counter(c.values())
    return sum(c.values()), len(c), sorted(h.items())


def of_events(ev, lens, active=None):
    ch, s, e = intervals(ev, lens, active)
    return histogram(zip(ch.tolist(), s.tolist(), e.tolist()))


def add(results):
    """(N, D, pairs) of several contexts, added."""
    h = Counter()
    for _, _, pairs in results:
        for m, k in pairs:
            h[m] += k
    return sum(r[0] for r in results), sum(r[1] for r in results), sorted(h.items())


def curve_depth(N, k):
    """n of the k-th point: round(k N / 20), halves up."""
    return (k * N + CURVE // 2) // CURVE


def curve(N, pairs):
    """E_n for the 20 depths: sum_m h[m] (1 - falling(N - n, m) / falling(N, m)), each quotient to 2^-256."""
    out = []
    for k in range(1, CURVE + 1):
        n = curve_depth(N, k)
        num = den = 1
        done = 0
        E = Fraction(0)
        for m, h in pairs:          # ascending: the products are extended, not begun again
            while done < m:
                num *= max(N - n - done, 0)
                den *= N - done
                done += 1
            p = Fraction((num << 256) // den, 1 << 256)
            E += h * (1 - p)
        out.append(E)
    return out


def library_size(N, D):
    """(lo, hi) Decimals around the X with D / X = 1 - exp(-N / X), hi - lo < 1e-20; None when D == N or N == 0."""
    if N == 0 or D >= N:
        return None
    with decimal.localcontext() as c:
        c.prec = 60
        n, d = decimal.Decimal(N), decimal.Decimal(D)
        g = lambda X: X * (1 - (-n / X).exp()) - d
        lo = hi = d
        while g(hi) < 0:
            hi *= 2
        while hi - lo > decimal.Decimal("1e-20"):
            mid = (lo + hi) / 2
            if g(mid) < 0:
                lo = mid
            else:
                hi = mid
        return lo, hi


def figures(N, D, pairs):
    """The figures as exact numbers; None where one is not defined."""
    h = dict(pairs)
    h1, h2 = h.get(1, 0), h.get(2, 0)
    return {"h1": h1, "h2": h2,
            "nrf": Fraction(D, N) if N else None,
            "pbc1": Fraction(h1, D) if D else None,
            "pbc2": Fraction(h1, h2) if h2 else None,
            "dup_fraction": Fraction(N - D, N) if N else None,
            "library_size": library_size(N, D),
            "curve": curve(N, pairs)}


def label(rep, is_ctrl):
    return f"{'c' if is_ctrl else 't'}{rep}"


def hist_text(samples):
    """samples: [(rep, is_ctrl, N, D, pairs)] -> --complexity-hist's text."""
    out = [HIST_HEADER]
    for rep, ctrl, N, D, pairs in samples:
        out += [f"{label(rep, ctrl)}\t{m}\t{k}" for m, k in pairs]
    return "".join(l + "\n" for l in out)


def check_metrics(text, samples, curve_rel=Fraction(1, 10 ** 10)):
    """None when `text` is --complexity's table of the samples, else what is wrong.  Integers and labels exactly; a ratio as the
    %.6f of the correctly rounded double; the library size within 1 of the bracketed root; a curve point within curve_rel
    relative plus half a unit of the third printed digit."""
    lines = text.split("\n")
    if lines[-1] != "" or lines[0] != HEADER or len(lines) != len(samples) + 2:
        return "shape"
    for line, (rep, ctrl, N, D, pairs) in zip(lines[1:], samples):
        f = line.split("\t")
        want = figures(N, D, pairs)
        if len(f) != 10 + CURVE or f[:5] != [label(rep, ctrl), str(N), str(D), str(want["h1"]), str(want["h2"])]:
            return f"integers: {f[:5]}"
        for col, name in zip(f[5:9], RATIOS):
            exp = "NA" if want[name] is None else f"{float(want[name]):.6f}"      # (Fraction -> float rounds correctly)
            if col != exp:
                return f"{name}: {col} != {exp}"
        if want["library_size"] is None:
            if f[9] != "NA":
                return f"library_size: {f[9]}"
        else:
            lo, hi = want["library_size"]
            if not f[9].isdigit() or not (lo - 1 <= int(f[9]) <= hi + 1):
                return f"library_size: {f[9]} not within 1 of {lo}"
        for k, (col, E) in enumerate(zip(f[10:], want["curve"])):
            if abs(Fraction(col) - E) > curve_rel * E + Fraction(1, 2000):
                return f"curve[{k}]: {col} != {float(E)}"
    return None


def verbose_prefix(rep, is_ctrl, N, D):
    """How -v's line of a sample begins (the figures follow in brackets)."""
    return f"  Library complexity, {'control' if is_ctrl else 'experimental'} file #{rep}: {N} intervals, {D} distinct (NRF "
