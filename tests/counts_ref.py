"""numpy restatement of gx_count_in_peaks (include/genrich_amd.h) and of the --counts text, for the tests.

An interval [s, e) (end clamped to the chromosome's length) overlaps peak [ps, pe) of its chromosome iff s < pe && ps < e.
Per chromosome, with the peaks sorted and disjoint: k0 = first peak with pe > s, k1 = first peak with ps >= e; the interval
overlaps peaks k0 .. k1-1.  Weights are 120 / count (1/120 units), sums are exact int64."""
from __future__ import annotations

import numpy as np


def weights(count):
    return (120 // np.asarray(count, dtype=np.int64)).astype(np.int64)


def count_in_peaks(chrom, s, e, w, pchrom, ps, pe):
    """-> (count int64[n_peaks], total, in_peaks) for one sample's intervals against peaks in (chrom, start) order."""
    chrom = np.asarray(chrom, dtype=np.int64)
    s = np.asarray(s, dtype=np.int64)
    e = np.asarray(e, dtype=np.int64)
    w = np.asarray(w, dtype=np.int64)
    pchrom = np.asarray(pchrom, dtype=np.int64)
    ps = np.asarray(ps, dtype=np.int64)
    pe = np.asarray(pe, dtype=np.int64)
    n = len(ps)
    diff = np.zeros(n + 1, dtype=np.int64)
    inp = 0
    for c in np.unique(chrom):
        a, b = np.searchsorted(pchrom, c, "left"), np.searchsorted(pchrom, c, "right")
        sel = chrom == c
        k0 = a + np.searchsorted(pe[a:b], s[sel], "right")
        k1 = a + np.searchsorted(ps[a:b], e[sel], "left")
        m = k0 < k1
        ww = w[sel][m]
        inp += int(ww.sum())
        np.add.at(diff, k0[m], ww)
        np.add.at(diff, k1[m], -ww)
    return np.cumsum(diff)[:n], int(w.sum()), int(inp)


def count_brute(chrom, s, e, w, pchrom, ps, pe):
    """The definition itself, interval by interval and peak by peak."""
    cnt = np.zeros(len(ps), dtype=np.int64)
    tot = inp = 0
    for c, a, b, x in zip(chrom, s, e, w):
        tot += int(x)
        hit = False
        for k in range(len(ps)):
            if pchrom[k] == c and a < pe[k] and ps[k] < b:
                cnt[k] += int(x)
                hit = True
        inp += int(x) if hit else 0
    return cnt, tot, inp


def value_text(n):
    n = int(n)
    return f"{n // 120}" if n % 120 == 0 else f"{n / 120.0:.2f}"


def counts_text(names, peaks, sample_names, counts):
    """--counts: header, then one row per peak (chrom, start, end, peak_N) with one value per sample; counts[i][k]."""
    out = ["\t".join(["chr", "start", "end", "name"] + list(sample_names))]
    for k, (c, a, b) in enumerate(peaks):
        out.append("\t".join([names[c], str(a), str(b), f"peak_{k}"] + [value_text(cs[k]) for cs in counts]))
    return "".join(line + "\n" for line in out)


def frip_line(rep, is_ctrl, total, in_peaks):
    kind = "control" if is_ctrl else "experimental"
    frip = in_peaks / total if total else 0.0
    return f"  Intervals in peaks, {kind} file #{rep}: {value_text(in_peaks)} of {value_text(total)} (FRiP {frip:f})"
