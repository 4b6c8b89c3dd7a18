"""Plain Python / numpy restatement of the k-mer definitions of include/genrich_amd.h (gx_kmer_count_regions .. gx_format_kmers)
over motifs_ref.genome's codes: the counts of the forward codes and the counted windows of a set of regions, of the peaks with a
flank and of the genome, the strand collapse, the figures per canonical k-mer in Python integers (converted to doubles by the
same steps as the library's) and the table's text."""
import math

import numpy as np

import motifs_ref as MR

MAX_K = 12
LDS_MAX_K = 7


def code_of(word):
    """ACGT letters to the public code: the first base most significant, A 0, C 1, G 2, T 3."""
    c = 0
    for ch in word:
        c = c * 4 + "ACGT".index(ch)
    return c


def word_of(k, code):
    return "".join("ACGT"[(code >> (2 * (k - 1 - j))) & 3] for j in range(k))


def revcomp(k, code):
    """The code of the reverse complement: the last base first, every digit b as 3 - b."""
    r = 0
    for _ in range(k):
        r = r * 4 + (3 - code % 4)
        code //= 4
    return r


def count(gen, regions, k, active=None):
    """(counts int64[4^k], windows, regions counted) of regions = [(chrom, start, end)] of the genome `gen` (codes per chromosome): a
    window [x, x + k) is counted iff start <= x, x + k <= min(end, length) and all k bases are known; active[c] = 0: the
    chromosome has no words here and counts nothing.  A region is `counted` when it holds at least k bases after the clamp."""
    found = [np.zeros(0, dtype=np.int64)]
    n_reg = 0
    for c, start, end in regions:
        if c >= len(gen) or (active is not None and not active[c]):
            continue
        e = min(end, len(gen[c]))
        if start >= e or e - start < k:
            continue
        n_reg += 1
        code = gen[c][start:e].astype(np.int64)
        n = len(code) - k + 1
        bad = np.concatenate([[0], np.cumsum(code < 0)])
        ok = (bad[k:k + n] - bad[:n]) == 0
        safe = np.where(code < 0, 0, code)
        idx = np.zeros(n, dtype=np.int64)
        for j in range(k):
            idx = idx * 4 + safe[j:j + n]
        found.append(idx[ok])
    found = np.concatenate(found)
    return np.bincount(found, minlength=4 ** k).astype(np.int64), len(found), n_reg


def count_genome(gen, k, active=None):
    return count(gen, [(c, 0, len(g)) for c, g in enumerate(gen)], k, active)[:2]


def flank_regions(peaks, summit_off, flank):
    """[(chrom, start, end)] of the peaks: whole (flank < 0) or [max(start, summit - flank), min(end, summit + flank + 1))."""
    if flank < 0:
        return [tuple(p) for p in peaks]
    out = []
    for (c, s, e), so in zip(peaks, summit_off):
        at = s + so
        out.append((c, max(s, at - flank), min(e, at + flank + 1)))
    return out


def collapse(k, counts):
    """{canonical code: count}: counts[c] + counts[rc(c)], or counts[c] alone for a palindrome; every canonical code is there."""
    out = {}
    for c in range(4 ** k):
        rc = revcomp(k, c)
        if rc < c:
            continue
        out[c] = int(counts[c]) + (int(counts[rc]) if rc != c else 0)
    return out


def _signed(x):
    return -MR._to_double(-x) if x < 0 else MR._to_double(x)


def stats(k, cp, wp, cg, wg):
    """[(code, revcomp, count_peaks, count_genome, enrichment or None, z or None)] of the canonical k-mers with count_peaks > 0,
    sorted by z descending with None last, then count_peaks descending, then code ascending."""
    p, g = collapse(k, cp), collapse(k, cg)
    rows = []
    for c in sorted(p):
        if not p[c]:
            continue
        enr = z = None
        if g[c]:
            enr = MR._to_double(p[c] * wg) / MR._to_double(g[c] * wp)
            if g[c] != wg:
                z = _signed(p[c] * wg - g[c] * wp) / math.sqrt(MR._to_double(wp * g[c] * (wg - g[c])))
        rows.append((c, revcomp(k, c), p[c], g[c], enr, z))
    rows.sort(key=lambda r: (r[5] is None, -(r[5] or 0.0), -r[2], r[0]))
    return rows


def text(k, flank, n_reg, wp, wg, cp, cg, top=100):
    rows = stats(k, cp, wp, cg, wg)
    out = ["# k=%d flank=%s regions=%d windows_peaks=%d windows_genome=%d kmers=%d\n" % (k, "whole" if flank < 0 else str(flank), n_reg, wp, wg, len(rows)),
           "kmer\trevcomp\tcount_peaks\tcount_genome\tenrichment\tz\n"]
    for c, rc, a, b, enr, z in rows[:top] if top else rows:
        out.append("%s\t%s\t%d\t%d\t%s\t%s\n" % (word_of(k, c), word_of(k, rc), a, b, "NA" if enr is None else "%.6f" % enr, "NA" if z is None else "%.4f" % z))
    return "".join(out)
