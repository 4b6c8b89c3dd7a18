"""numpy restatement of gx_count_in_regions (include/genrich_amd.h) and of the --region-counts text, for the tests.

Region k = (chrom, start, end), start < end; the set may overlap, nest, repeat and come in any order.  An interval [s, e) on the
same chromosome overlaps it iff s < end && start < e, and counts in every region it overlaps.  Per chromosome, with A the sorted
starts and B the sorted ends: a = #{A < e}, b = #{B <= s}; for s <= e the interval overlaps a - b regions, and with region k at
rank i in A and rank j in B, count[k] = W{b <= j} - W{a <= i}.  Inverted intervals (e < s) are tested directly.  Weights are
120 / count (1/120 units), sums are exact int64.  The caller passes intervals as gx_count_in_peaks sees them (ends clamped to the
chromosome's length, inactive chromosomes left out) and leaves the regions as they are."""
from __future__ import annotations

import numpy as np

from counts_ref import value_text, weights  # noqa: F401  (the same weights and the same value text as --counts)


def count_in_regions(chrom, s, e, w, rchrom, rs, re):
    """-> (count int64[n_regions], total, in_regions) for one sample's intervals."""
    chrom, s, e, w = (np.asarray(x, dtype=np.int64) for x in (chrom, s, e, w))
    rchrom, rs, re = (np.asarray(x, dtype=np.int64) for x in (rchrom, rs, re))
    cnt = np.zeros(len(rs), dtype=np.int64)
    inr = 0
    for c in np.unique(chrom):
        rk = np.flatnonzero(rchrom == c)
        if not len(rk):
            continue
        sel = chrom == c
        cs, ce, cw = s[sel], e[sel], w[sel]
        fwd = cs <= ce
        A, B = np.sort(rs[rk]), np.sort(re[rk])
        a = np.searchsorted(A, ce[fwd], "left")
        b = np.searchsorted(B, cs[fwd], "right")
        assert (a >= b).all()
        inr += int(cw[fwd][a > b].sum())
        ha = np.zeros(len(rk) + 1, dtype=np.int64)
        hb = np.zeros(len(rk) + 1, dtype=np.int64)
        np.add.at(ha, a, cw[fwd])
        np.add.at(hb, b, cw[fwd])
        pa, pb = np.cumsum(ha), np.cumsum(hb)
        i = np.argsort(np.argsort(rs[rk], kind="stable"), kind="stable")
        j = np.argsort(np.argsort(re[rk], kind="stable"), kind="stable")
        cnt[rk] += pb[j] - pa[i]
        for x, y, z in zip(cs[~fwd], ce[~fwd], cw[~fwd]):   # inverted: the predicate itself
            hit = (x < re[rk]) & (rs[rk] < y)
            cnt[rk[hit]] += z
            inr += int(z) if hit.any() else 0
    return cnt, int(w.sum()), int(inr)


def count_brute(chrom, s, e, w, rchrom, rs, re):
    """The definition itself, interval by interval and region by region."""
    cnt = np.zeros(len(rs), dtype=np.int64)
    tot = inr = 0
    for c, a, b, x in zip(chrom, s, e, w):
        tot += int(x)
        hit = False
        for k in range(len(rs)):
            if rchrom[k] == c and a < re[k] and rs[k] < b:
                cnt[k] += int(x)
                hit = True
        inr += int(x) if hit else 0
    return cnt, tot, inr


def region_counts_text(rows, sample_names, counts):
    """--region-counts: header, then one row per BED line; rows[k] = (chrom text, start, end, name | None); counts[i][k]."""
    out = ["\t".join(["chr", "start", "end", "name"] + list(sample_names))]
    for k, (c, a, b, nm) in enumerate(rows):
        out.append("\t".join([c, str(a), str(b), nm if nm is not None else f"region_{k}"] + [value_text(cs[k]) for cs in counts]))
    return "".join(line + "\n" for line in out)


def fraction_line(rep, is_ctrl, total, in_regions):
    kind = "control" if is_ctrl else "experimental"
    frac = in_regions / total if total else 0.0
    return f"  Intervals in regions, {kind} file #{rep}: {value_text(in_regions)} of {value_text(total)} (fraction {frac:f})"
