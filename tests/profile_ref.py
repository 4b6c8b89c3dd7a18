"""numpy restatement of the profiles around anchors (include/genrich_amd.h, gx_set_profile) and of the --profile text, for the tests.

An anchor is (chrom, pos, strand), strand +1 or -1.  With the flank F and the bin size B (F % B == 0) it has nb = 2 F / B bins;
bin j covers the bases x with
    strand +:  pos - F + j B       <= x <  pos - F + (j + 1) B
    strand -:  pos + F - (j + 1) B <  x <= pos + F - j B
and cell120[a][j] is the sum of the sample's per-base pileup (coverage_ref.pileup120: 1/120 units, 0 inside -E regions) over
them, bases outside [0, len) counting 0.  A row is all zeros when the anchor's chromosome is skipped, empty, not owned, left out
by the save mask or behind the table.  agg120[j] = the sum of cell120[a][j] over all anchors."""
from __future__ import annotations

import math

import numpy as np

import coverage_ref as R

ANCHOR_DTYPE = np.dtype([("chrom", "<u4"), ("pos", "<u4"), ("strand", "<i4")])


def n_bins(F, B):
    assert B >= 1 and F % B == 0
    return 2 * int(F) // int(B)


def rows_of(pile, pos, strand, F, B):
    """The rows of anchors (pos[i], strand[i]) on one chromosome whose per-base pileup is `pile`: pad with zeros, slice the
    window, reverse it for strand -, reshape to (nb, B) and sum."""
    F, B = int(F), int(B)
    nb = n_bins(F, B)
    pos = np.asarray(pos, dtype=np.int64)
    over = max(0, int(pos.max()) + 2 - len(pile)) if len(pos) else 0     # (anchors at or beyond the length)
    pad = np.zeros(F + len(pile) + F + over, dtype=np.int64)
    pad[F:F + len(pile)] = pile
    out = np.zeros((len(pos), nb), dtype=np.int64)
    for i, (p, s) in enumerate(zip(pos, strand)):
        lo = int(p) - F + (1 if s < 0 else 0)                            # the window [lo, lo + 2 F) in chromosome coordinates
        w = pad[lo + F:lo + F + 2 * F]
        if s < 0:
            w = w[::-1]
        out[i] = w.reshape(nb, B).sum(axis=1)
    return out


def live_chrom(c, lens, skip=None, save=None, owned=None):
    return (c < len(lens) and lens[c] != 0 and not (skip is not None and skip[c]) and not (owned is not None and not owned[c])
            and not (save is not None and not save[c]))


def profile(ev, lens, anchors, F, B, skip=None, beds=None, save=None, owned=None, piles=None):
    """cell120 int64[n_anchors, nb] of one sample, in the anchors' order (piles: {chrom: pileup120} computed before)."""
    anchors = np.asarray(anchors, dtype=ANCHOR_DTYPE)
    out = np.zeros((len(anchors), n_bins(F, B)), dtype=np.int64)
    for c in np.unique(anchors["chrom"]):
        c = int(c)
        if not live_chrom(c, lens, skip, save, owned):
            continue
        pile = piles[c] if piles is not None else R.pileup120(ev, c, lens[c], beds[c] if beds is not None else ())
        at = np.flatnonzero(anchors["chrom"] == c)
        out[at] = rows_of(pile, anchors["pos"][at], anchors["strand"][at], F, B)
    return out


def rows_brute(pile, pos, strand, F, B):
    """The definition itself, bin by bin and base by base."""
    F, B = int(F), int(B)
    nb = n_bins(F, B)
    out = np.zeros((len(pos), nb), dtype=np.int64)
    for i, (p, s) in enumerate(zip(pos, strand)):
        p = int(p)
        for j in range(nb):
            if s > 0:
                xs = range(p - F + j * B, p - F + (j + 1) * B)
            else:
                xs = range(p + F - (j + 1) * B + 1, p + F - j * B + 1)
            out[i, j] = sum(int(pile[x]) for x in xs if 0 <= x < len(pile))
    return out


def n_counted(anchors, lens, skip=None):
    """Anchors on chromosomes the run computes: known, not skipped, not empty."""
    return sum(1 for a in anchors if a["chrom"] < len(lens) and lens[a["chrom"]] != 0 and not (skip is not None and skip[a["chrom"]]))


def profile_text(sample_names, aggs, counted, F, B):
    """PREFIX.profile.tsv: the mean per base and anchor at every offset, one column per sample."""
    out = ["offset" + "".join("\t" + n for n in sample_names) + "\n"]
    for j in range(n_bins(F, B)):
        vals = "".join("\t%.6f" % (float(int(a[j])) / (120.0 * B * counted) if counted else 0.0) for a in aggs)
        out.append(f"{-F + j * B}{vals}\n")
    return "".join(out)


def rows_text(names, regions, row_names, strands, first, cells, B):
    """Rows of PREFIX.t<rep>.matrix.tsv: chrom start end name strand of the anchor's BED line, then its nb values."""
    out = []
    for i, row in enumerate(cells):
        a = first + i
        c, s, e = regions[a]
        name = row_names[a] if row_names is not None and row_names[a] is not None else f"anchor_{a}"
        vals = "".join("\t" + R.value_text(int(x), B) for x in row)
        out.append(f"{names[c]}\t{s}\t{e}\t{name}\t{'-' if strands[a] < 0 else '+'}{vals}\n")
    return "".join(out)


def enrichment(agg, B):
    nb = len(agg)
    ne = max(1, min(nb // 4, math.ceil(100 / B)))
    edge = sum(int(x) for x in agg[:ne]) + sum(int(x) for x in agg[nb - ne:])
    return float(max(int(x) for x in agg)) * (2.0 * ne) / float(edge) if edge else 0.0


def enrichment_line(rep, is_ctrl, agg, counted, B):
    kind = "control" if is_ctrl else "experimental"
    return f"  Profile, {kind} file #{rep}: enrichment {enrichment(agg, B):f} over {counted} anchors"


def parse_bed(text, names, at="tss"):
    """--profile's BED -> (all names, regions [(chrom, start, end)], row names, strands, anchors): a chromosome that no header
    names gets an index behind the table; column 4 names the row; column 6 is the strand (. or none: +)."""
    all_names = list(names)
    idx = {n: i for i, n in enumerate(all_names)}
    regions, row_names, strands = [], [], []
    for line in text.splitlines():
        f = line.split("\t")
        if f[0] not in idx:
            idx[f[0]] = len(all_names)
            all_names.append(f[0])
        regions.append((idx[f[0]], int(f[1]), int(f[2])))
        row_names.append(f[3] if len(f) > 3 else None)
        strands.append(-1 if len(f) > 5 and f[5] == "-" else 1)
    anchors = np.zeros(len(regions), dtype=ANCHOR_DTYPE)
    for k, ((c, s, e), st) in enumerate(zip(regions, strands)):
        anchors[k] = (c, (s + e) // 2 if at == "center" else (s if st > 0 else e - 1), st)
    return all_names, regions, row_names, strands, anchors
