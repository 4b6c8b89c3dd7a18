"""numpy restatement of the binned coverage (include/genrich_amd.h, gx_set_coverage_bins) and of the --coverage text, for the tests.

A sample's pileup at a base, in 1/120 units, is the sum of the weights 120 / count of its events [start, end) that cover the
base -- the events that enter the pileup: a valid count, a chromosome the context computes and the replicate's treatment header
lists, start < len, end clamped to len (the rules of gx_count_in_peaks) --, 0 inside -E regions.  Bin b of a chromosome covers
[b W, min((b + 1) W, len)); sum120[b] is the sum of the pileup over its bases, an exact int64."""
from __future__ import annotations

import numpy as np

VALID_COUNTS = (1, 2, 3, 4, 5, 6, 8, 10)


def n_bins(length, W):
    return (int(length) + int(W) - 1) // int(W)


def pileup120(ev, chrom, length, bed=()):
    """Per-base pileup (int64[length], 1/120 units) of one chromosome from a sample's events."""
    ev = ev[(ev["chrom"] == chrom) & np.isin(ev["count"], VALID_COUNTS) & (ev["start"] < length)]
    w = 120 // ev["count"].astype(np.int64)
    diff = np.zeros(int(length) + 1, dtype=np.int64)
    np.add.at(diff, ev["start"].astype(np.int64), w)
    np.add.at(diff, np.minimum(ev["end"].astype(np.int64), int(length)), -w)
    pile = np.cumsum(diff)[:int(length)]
    bed = np.asarray(bed, dtype=np.int64).ravel()
    for a, b in zip(bed[0::2], bed[1::2]):
        pile[a:min(b, int(length))] = 0
    return pile


def bin_sums(pile, W):
    """The per-base pileup summed over bins of W bases (the last one may be short)."""
    n = n_bins(len(pile), W)
    pad = np.zeros(n * int(W), dtype=np.int64)
    pad[:len(pile)] = pile
    return pad.reshape(n, int(W)).sum(axis=1)


def coverage(ev, lens, W, skip=None, beds=None, save=None, owned=None):
    """{chrom: sum120 int64[n_bins]} of one sample: the chromosomes that have bins (not skipped, not empty, owned); one the
    treatment header does not list (save) has bins that are all 0."""
    out = {}
    for c, length in enumerate(lens):
        if length == 0 or (skip is not None and skip[c]) or (owned is not None and not owned[c]):
            continue
        if save is not None and not save[c]:
            out[c] = np.zeros(n_bins(length, W), dtype=np.int64)
            continue
        out[c] = bin_sums(pileup120(ev, c, length, beds[c] if beds is not None else ()), W)
    return out


def coverage_brute(ev, lens, W):
    """The definition itself, event by event and base by base (no -E, every chromosome)."""
    out = {c: np.zeros(n_bins(length, W), dtype=np.int64) for c, length in enumerate(lens) if length}
    for e in ev:
        c, s, t, k = int(e["chrom"]), int(e["start"]), int(e["end"]), int(e["count"])
        if k not in VALID_COUNTS or s >= lens[c]:
            continue
        for x in range(s, min(t, lens[c])):
            out[c][x // W] += 120 // k
    return out


def value_text(total, bases, scale=1.0):
    total, bases = int(total), int(bases)
    if scale == 1.0 and total % (120 * bases) == 0:
        return f"{total // (120 * bases)}"
    return "%.4f" % ((float(total) / (120.0 * float(bases))) * scale)


def format_chrom(name, length, W, sum120, scale=1.0):
    """bedGraph lines of one chromosome: adjacent bins with exactly equal means (cross-multiplied integers) share a line."""
    length, W = int(length), int(W)
    sums = [int(x) for x in sum120]
    assert len(sums) == n_bins(length, W)
    bases = [min((b + 1) * W, length) - b * W for b in range(len(sums))]
    out = []
    a = 0
    while a < len(sums):
        b = a + 1
        while b < len(sums) and sums[a] * bases[b] == sums[b] * bases[a]:
            b += 1
        tot, nb = sum(sums[a:b]), sum(bases[a:b])
        out.append(f"{name}\t{a * W}\t{a * W + nb}\t{value_text(tot, nb, scale)}\n")
        a = b
    return "".join(out)


def coverage_text(names, lens, W, cov, scale=1.0):
    """--coverage's file of one sample: the chromosomes that have bins, in table order."""
    return "".join(format_chrom(names[c], lens[c], W, cov[c], scale) for c in range(len(lens)) if c in cov)


def mean_line(rep, is_ctrl, lens, cov):
    kind = "control" if is_ctrl else "experimental"
    total = sum(float(sum(int(x) for x in cov[c])) / 120.0 for c in sorted(cov))
    bp = sum(int(lens[c]) for c in cov)
    return f"  Coverage, {kind} file #{rep}: mean {(total / float(bp) if bp else 0.0):f} over {bp} bp"
