"""The summits of the pooled treatment depth inside the peaks (gx_peak_summits, genrich-amd --summits) restated in numpy over
runs of equal depth, a brute force that applies the definition base by base, and the text of --summits.

Pooled depth: the sum over the treatment samples of tests/peaksig_ref.py's depth (+w at s, -w at the clamped e, w = 120 /
count; an empty interval adds nothing, one with e < s adds -w over [e, s)).  Per peak d(x), x in [0, L).  A plateau is a maximal
run [a, b) of equal d, a local maximum when d is strictly lower on both sides (outside the peak counts as lower).  Per local
maximum of height h: pos = a + (b - a - 1) // 2, width = b - a, prominence = h - max(baseL, baseR); a side's base is the minimum
of d between the plateau and the nearest base with d > h (none: up to the peak's end); an empty side is left out, both empty: the
base is 0.  Reported: the highest (leftmost of equals) when h > 0; every other one with h > 0, prominence * 100 >= P * h and
h * 100 >= R * hmax."""
import numpy as np

import peaksig_ref as PR

SUMMIT_DTYPE = np.dtype([("peak", "<u4"), ("pos", "<u4"), ("width", "<u4"), ("pad", "<u4"), ("height", "<i8"), ("prominence", "<i8")])


def pooled_depth(samples, lens, chrom, actives=None):
    """int64[lens[chrom]]: the samples' (event arrays) depths added; actives[i]: sample i's active chromosomes or None"""
    d = np.zeros(int(lens[chrom]), dtype=np.int64)
    for i, ev in enumerate(samples):
        c, s, e, w = PR.intervals(ev, lens, None if actives is None else actives[i])
        d += PR.depth_of(c, s, e, w, chrom, int(lens[chrom]))
    return d


def _select(cands, P, R):
    """cands = [(pos, width, h, prom)] of all local maxima, left to right -> those reported"""
    pos = [c for c in cands if c[2] > 0]
    if not pos:
        return []
    hmax = max(c[2] for c in pos)
    top = next(c for c in pos if c[2] == hmax)
    return [c for c in pos if c is top or (c[3] * 100 >= P * c[2] and c[2] * 100 >= R * hmax)]


def of_depth(d, P=25, R=50):
    """the restatement over runs: d = int64[L] -> [(pos, width, height, prominence)]"""
    d = np.asarray(d, dtype=np.int64)
    L = len(d)
    st = np.concatenate([[0], np.flatnonzero(d[1:] != d[:-1]) + 1])
    en = np.concatenate([st[1:], [L]])
    v = d[st]
    n = len(v)
    lo_left = np.concatenate([[True], v[1:] > v[:-1]])
    lo_right = np.concatenate([v[:-1] > v[1:], [True]])
    cands = []
    for i in np.flatnonzero(lo_left & lo_right):
        h = int(v[i])
        left, right = v[:i][::-1], v[i + 1:]
        sides = []
        for side in (left, right):
            if len(side):
                hi = np.flatnonzero(side > h)
                sides.append(int(side[:hi[0] if len(hi) else len(side)].min()))
        base = max(sides) if sides else 0
        a, b = int(st[i]), int(en[i])
        cands.append((a + (b - a - 1) // 2, b - a, h, h - base))
    assert n >= 1
    return _select(cands, P, R)


def brute_of_depth(d, P=25, R=50):
    """the definition base by base (plain Python integers)"""
    d = [int(x) for x in d]
    L = len(d)
    cands = []
    a = 0
    while a < L:
        b = a
        while b < L and d[b] == d[a]:
            b += 1
        h = d[a]
        if (a == 0 or d[a - 1] < h) and (b == L or d[b] < h):
            bases = []
            if a > 0:
                m, x = None, a - 1
                while x >= 0 and d[x] <= h:
                    m = d[x] if m is None else min(m, d[x])
                    x -= 1
                bases.append(m)
            if b < L:
                m, x = None, b
                while x < L and d[x] <= h:
                    m = d[x] if m is None else min(m, d[x])
                    x += 1
                bases.append(m)
            cands.append((a + (b - a - 1) // 2, b - a, h, h - (max(bases) if bases else 0)))
        a = b
    return _select(cands, P, R)


def summits(samples, lens, peaks, P=25, R=50, actives=None, of=of_depth):
    """SUMMIT_DTYPE records, ascending in (peak, pos), of the treatment samples' pooled depth in `peaks` (rows of (chrom, start,
    end))"""
    pk = np.asarray(peaks, dtype=np.int64).reshape(-1, 3)
    rows, depth = [], {}
    for k, (c, ps, pe) in enumerate(pk):
        if int(c) not in depth:
            depth[int(c)] = pooled_depth(samples, lens, int(c), actives)
        for pos, width, h, prom in of(depth[int(c)][ps:pe], P, R):
            rows.append((k, pos, width, 0, h, prom))
    return np.array(rows, dtype=SUMMIT_DTYPE) if rows else np.zeros(0, dtype=SUMMIT_DTYPE)


def same(a, b):
    """None, or the first record in which two summit lists differ"""
    a, b = np.asarray(a, dtype=SUMMIT_DTYPE), np.asarray(b, dtype=SUMMIT_DTYPE)
    if len(a) != len(b):
        return "length", len(a), len(b)
    for f in ("peak", "pos", "width", "height", "prominence"):
        if not np.array_equal(a[f], b[f]):
            k = int(np.flatnonzero(a[f] != b[f])[0])
            return f, k, a[k].tolist(), b[k].tolist()
    return None


HEADER = "chr\tstart\tend\tname\theight\tstrand\tplateau_start\tplateau_end\tprominence\tpeak_start\tpeak_end"


def summits_text(names, peaks, sm):
    """--summits' text: sm = SUMMIT_DTYPE records ascending in (peak, pos) over `peaks` (rows of (chrom, start, end))"""
    lines, j, last = [HEADER], 0, None
    for r in sm:
        k, pos, width = int(r["peak"]), int(r["pos"]), int(r["width"])
        c, ps, pe = (int(x) for x in peaks[k])
        j = j + 1 if last == k else 1
        last = k
        a = ps + pos - (width - 1) // 2
        lines.append("\t".join([names[c], str(ps + pos), str(ps + pos + 1), f"peak_{k}.{j}", PR.value_text(r["height"]), ".", str(a), str(a + width),
                                PR.value_text(r["prominence"]), str(ps), str(pe)]))
    return "\n".join(lines) + "\n"
