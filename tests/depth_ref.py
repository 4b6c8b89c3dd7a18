"""numpy restatement of the depth distribution (include/genrich_amd.h, gx_set_depth_hist) and of the --depth / --depth-metrics
texts, for the tests; the figures with Python integers.

For one closed sample on one context: a chromosome counts iff it is not skipped, owned and not empty; one the replicate's
treatment header does not list has pileup 0 everywhere.  total = the counting chromosomes' lengths, excluded = the union of their
-E regions clipped to the chromosome, B = total - excluded.  A non-excluded base of pileup v (1/120 units, coverage_ref.pileup120)
has whole depth d = v // 120 and remainder r = v % 120; for v > 0 and d < DEPTH_BOUND: bases[d], rsum[d], rsq[d]; for d >=
DEPTH_BOUND: the deep list {v: bases}; zero = B - the bases with v > 0; min_v / max_v the extreme v > 0."""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

import coverage_ref as CR

DEPTH_BOUND = 2048
GE = (1, 2, 5, 10, 20, 50, 100)
QS = (25, 50, 75, 95, 99)
HEADER = "#sample\tdepth\tbases\tbases_at_least\tfraction_at_least\n"
METRICS_HEADER = ("sample\tbases\texcluded\tcovered\tcovered_fraction\tmean\tsd\tmin\tq25\tmedian\tq75\tp95\tp99\tmax\t"
                  + "\t".join(f"ge{k}" for k in GE) + "\n")


class Hist(NamedTuple):
    rep: int
    is_ctrl: bool
    total: int
    excluded: int
    zero: int
    min_v: int
    max_v: int
    bases: np.ndarray      # uint64[DEPTH_BOUND]
    rsum: np.ndarray
    rsq: np.ndarray
    deep: list             # [(v, bases)] ascending


def excluded_mask(length, bed=()):
    m = np.zeros(int(length), dtype=bool)
    bed = np.asarray(bed, dtype=np.int64).ravel()
    for a, b in zip(bed[0::2], bed[1::2]):
        m[a:min(b, int(length))] = True
    return m


def from_values(v, total, excluded, rep=0, is_ctrl=False):
    """The histogram of the pileups `v` (int64, one per non-excluded base that was visited; zeros allowed)."""
    v = np.asarray(v, dtype=np.int64)
    v = v[v > 0]
    d, r = v // 120, v % 120
    low = d < DEPTH_BOUND
    bases, rsum, rsq = (np.zeros(DEPTH_BOUND, dtype=np.int64) for _ in range(3))
    np.add.at(bases, d[low], 1)
    np.add.at(rsum, d[low], r[low])
    np.add.at(rsq, d[low], r[low] * r[low])
    dv, dn = np.unique(v[~low], return_counts=True)
    B = int(total) - int(excluded)
    return Hist(rep, bool(is_ctrl), int(total), int(excluded), B - int(v.size), int(v.min()) if v.size else 0, int(v.max()) if v.size else 0,
                bases.astype(np.uint64), rsum.astype(np.uint64), rsq.astype(np.uint64), [(int(a), int(b)) for a, b in zip(dv, dn)])


def hist(ev, lens, skip=None, beds=None, save=None, owned=None, rep=0, is_ctrl=False, piles=None):
    """One sample's Hist; piles: {chrom: pileup120 with the -E regions zeroed} computed before, if the caller has them."""
    total = excluded = 0
    vals = []
    for c, length in enumerate(lens):
        if length == 0 or (skip is not None and skip[c]) or (owned is not None and not owned[c]):
            continue
        total += int(length)
        bed = beds[c] if beds is not None else ()
        mask = excluded_mask(length, bed)
        excluded += int(mask.sum())
        if save is not None and not save[c]:
            continue
        pile = piles[c] if piles is not None else CR.pileup120(ev, c, length, bed)
        vals.append(pile[~mask])
    return from_values(np.concatenate(vals) if vals else np.zeros(0, dtype=np.int64), total, excluded, rep, is_ctrl)


def brute(ev, lens, beds=None):
    """The definition itself, event by event and base by base (every chromosome counts), as a Hist."""
    total = excluded = 0
    counts = {}
    for c, length in enumerate(lens):
        total += length
        pile = [0] * length
        for e in ev:
            k = int(e["count"])
            if int(e["chrom"]) != c or k not in CR.VALID_COUNTS or int(e["start"]) >= length:
                continue
            for x in range(int(e["start"]), min(int(e["end"]), length)):
                pile[x] += 120 // k
        out = set()
        bed = list(beds[c]) if beds is not None else []
        for a, b in zip(bed[0::2], bed[1::2]):
            out.update(range(a, min(b, length)))
        excluded += len(out)
        for x in range(length):
            if x not in out and pile[x] > 0:
                counts[pile[x]] = counts.get(pile[x], 0) + 1
    bases, rsum, rsq = (np.zeros(DEPTH_BOUND, dtype=np.uint64) for _ in range(3))
    deep = []
    for v in sorted(counts):
        d, r = divmod(v, 120)
        if d < DEPTH_BOUND:
            bases[d] += counts[v]
            rsum[d] += r * counts[v]
            rsq[d] += r * r * counts[v]
        else:
            deep.append((v, counts[v]))
    covered = sum(counts.values())
    return Hist(0, False, total, excluded, total - excluded - covered, min(counts) if counts else 0, max(counts) if counts else 0, bases, rsum, rsq, deep)


def add(a, b):
    """Two contexts' results of one sample, added."""
    deep = dict(a.deep)
    for v, n in b.deep:
        deep[v] = deep.get(v, 0) + n
    mins = [x for x in (a.min_v, b.min_v) if x]
    return Hist(a.rep, a.is_ctrl, a.total + b.total, a.excluded + b.excluded, a.zero + b.zero, min(mins) if mins else 0, max(a.max_v, b.max_v),
                a.bases + b.bases, a.rsum + b.rsum, a.rsq + b.rsq, sorted(deep.items()))


def same(got, exp):
    """None, or the first field in which two histograms differ (every integer, exactly)."""
    for f in ("rep", "is_ctrl", "total", "excluded", "zero", "min_v", "max_v"):
        if int(getattr(got, f)) != int(getattr(exp, f)):
            return f"{f}: {getattr(got, f)} != {getattr(exp, f)}"
    for f in ("bases", "rsum", "rsq"):
        g, e = np.asarray(getattr(got, f), dtype=np.uint64), np.asarray(getattr(exp, f), dtype=np.uint64)
        if g.shape != (DEPTH_BOUND,) or not np.array_equal(g, e):
            bad = np.flatnonzero(g != e)[:6] if g.shape == e.shape else []
            return f"{f}: classes {list(bad)}: {[int(g[i]) for i in bad]} != {[int(e[i]) for i in bad]}"
    if [tuple(map(int, p)) for p in got.deep] != [tuple(map(int, p)) for p in exp.deep]:
        return f"deep: {got.deep[:4]} ({len(got.deep)}) != {exp.deep[:4]} ({len(exp.deep)})"
    return None


def rows(h):
    """[(whole depth, bases)] ascending: the depth-0 row first and always there, deep entries grouped by v // 120."""
    out = {0: int(h.zero) + int(h.bases[0])}
    for d in range(1, DEPTH_BOUND):
        if int(h.bases[d]):
            out[d] = int(h.bases[d])
    for v, n in h.deep:
        out[v // 120] = out.get(v // 120, 0) + int(n)
    return sorted(out.items())


def label(h):
    return f"{'c' if h.is_ctrl else 't'}{h.rep}"


def depth_text(samples):
    out = [HEADER]
    for h in samples:
        B = h.total - h.excluded
        at_least = B
        for d, n in rows(h):
            out.append(f"{label(h)}\t{d}\t{n}\t{at_least}\t{'%.6f' % (at_least / B if B else 0.0)}\n")
            at_least -= n
        assert at_least == 0
    return "".join(out)


def to_double(x):
    """An exact non-negative integer as the library makes it a double: its leading 64 bits, converted once, scaled."""
    bl = int(x).bit_length()
    if bl <= 64:
        return float(int(x))
    return math.ldexp(float(int(x) >> (bl - 64)), bl - 64)


def sums(h):
    """(sum v, sum v^2) over the bases, Python integers."""
    sv = sv2 = 0
    for d in range(DEPTH_BOUND):
        n, a, q = int(h.bases[d]), int(h.rsum[d]), int(h.rsq[d])
        sv += 120 * d * n + a
        sv2 += 14400 * d * d * n + 240 * d * a + q
    for v, n in h.deep:
        sv += v * n
        sv2 += v * v * n
    return sv, sv2


def metrics(h):
    """The figures as a dict: integers exact, doubles made as the library makes them."""
    B = h.total - h.excluded
    r = rows(h)
    covered = B - h.zero
    sv, sv2 = sums(h)
    m = dict(bases=B, excluded=h.excluded, covered=covered, min_v=0 if (h.zero or not covered) else h.min_v, max_v=h.max_v if covered else 0)
    if B:
        nb = 120.0 * float(B)
        m.update(covered_fraction=covered / B, mean=to_double(sv) / nb, sd=math.sqrt(to_double(B * sv2 - sv * sv)) / nb)
    else:
        m.update(covered_fraction=0.0, mean=math.nan, sd=math.nan)
    for name, q in zip(("q25", "median", "q75", "p95", "p99"), QS):
        below = 0
        for d, n in r:
            below += n
            if 100 * below >= q * B:
                m[name] = d
                break
    m["ge"] = [(sum(n for d, n in r if d >= k) / B if B else 0.0) for k in GE]
    return m


def value_text(v):
    return CR.value_text(v, 1)


def metrics_text(samples):
    out = [METRICS_HEADER]
    for h in samples:
        m = metrics(h)
        f = lambda x: "NA" if math.isnan(x) else "%.6f" % x
        out.append("\t".join([label(h), str(m["bases"]), str(m["excluded"]), str(m["covered"]), f(m["covered_fraction"]), f(m["mean"]), f(m["sd"]),
                              value_text(m["min_v"])] + [str(m[k]) for k in ("q25", "median", "q75", "p95", "p99")] + [value_text(m["max_v"])]
                             + [f(x) for x in m["ge"]]) + "\n")
    return "".join(out)


def verbose_line(h):
    m = metrics(h)
    return (f"  Depth, {'control' if h.is_ctrl else 'experimental'} file #{h.rep}: mean {m['mean']:f}, median {m['median']}, "
            f"{100.0 * m['covered_fraction']:f}% of {m['bases']} bp covered")
