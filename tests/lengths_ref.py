"""Python restatement of gx_interval_stats (include/genrich_amd.h) and of the --lengths / --lengths-metrics / --chrom-stats text,
for the tests.

A sample's intervals are those gx_count_in_peaks counts (a valid count, an active chromosome, start < len, the end clamped to
len).  One whose clamped end lies below its start is inverted and has no length; every other has L = end - start and the weight
w = 120 / count.  Everything is an exact Python integer; the doubles of the text are made of them as the library makes them:
one division of two integers below 2^53 (correctly rounded on both sides), or the leading 64 bits of a big integer converted
once and scaled (to_double), one square root, one division."""
from __future__ import annotations

import math
from collections import Counter
from typing import NamedTuple

import numpy as np

VALID_COUNTS = (1, 2, 3, 4, 5, 6, 8, 10)
CUTS = (150, 300, 500)
QS = (("p5", 5), ("q25", 25), ("median", 50), ("q75", 75), ("p95", 95))
LENGTHS_HEADER = "sample\tlength\tintervals\tweight\tcum_weight_share\n"
LENGTHS_COMMENT = ("# an interval is one of the sample's -b lines: a fragment, or an unpaired read as -y / -w extend it (with -j: cut-site "
                   "windows instead); length = end (clamped to the chromosome) - start; weight = 1 / alignments\n")
LENGTHS_COMMENT_J = ("# an interval is a cut-site window of -j (ATAC mode), not a fragment: nearly all have one length; length = end "
                     "(clamped to the chromosome) - start; weight = 1 / alignments\n")
CHROM_COMMENT = ("# intervals, weight and share count every interval of the sample on the chromosome; mean_depth = sum of weight x "
                 "length / chromosome length; a chromosome skipped with -e never reaches the library: its row is zeros\n")


class Stats(NamedTuple):
    lengths: list          # [(L, n, w120)] ascending
    n_inverted: int
    w120_inverted: int
    cn: list               # per chromosome of the table
    cw120: list
    cbases120: list


def of_intervals(rows, n_chrom):
    """rows: an iterable of (chromosome index, start, clamped end, count) that ARE a sample's intervals."""
    n, w = Counter(), Counter()
    ni = wi = 0
    cn, cw, cb = [0] * n_chrom, [0] * n_chrom, [0] * n_chrom
    for c, s, e, cnt in rows:
        wt = 120 // cnt
        cn[c] += 1
        cw[c] += wt
        if e < s:
            ni += 1
            wi += wt
            continue
        n[e - s] += 1
        w[e - s] += wt
        cb[c] += wt * (e - s)
    return Stats([(L, n[L], w[L]) for L in sorted(n)], ni, wi, cn, cw, cb)


def of_events(ev, lens, active=None):
    """Stats of EVENT_DTYPE events over the table `lens`; active: per chromosome (not skipped, saved, owned), default all."""
    lens = np.asarray(lens, dtype=np.int64)
    ch = ev["chrom"].astype(np.int64)
    ok = np.isin(ev["count"], VALID_COUNTS) & (ch < len(lens))
    chs = np.where(ok, ch, 0)
    if active is not None:
        ok &= np.asarray(active, bool)[chs]
    ok &= ev["start"].astype(np.int64) < lens[chs]
    ch, s, e, cnt = ch[ok], ev["start"].astype(np.int64)[ok], ev["end"].astype(np.int64)[ok], ev["count"].astype(np.int64)[ok]
    e = np.minimum(e, lens[ch])
    return of_intervals(zip(ch.tolist(), s.tolist(), e.tolist(), cnt.tolist()), len(lens))


def of_bed_rows(rows, names, lens):
    """{(sample, is_ctrl): Stats} from events.bed lines "chrom start end name", name = ..._<count>_<E|C>_<sample>; the lines are
    the reference's own -b output, so each IS an interval (its end printed as it was clamped; clamped again here: no change)."""
    idx = {n: i for i, n in enumerate(names)}
    per = {}
    for line in rows:
        c, s, e, nm = line.split("\t")
        _, cnt, kind, smp = nm.rsplit("_", 3)
        ci = idx[c]
        assert int(cnt) in VALID_COUNTS and int(s) < lens[ci]
        per.setdefault((int(smp), kind == "C"), []).append((ci, int(s), min(int(e), lens[ci]), int(cnt)))
    return {k: of_intervals(v, len(names)) for k, v in per.items()}


def add(results):
    """Stats of several contexts, added."""
    n, w = Counter(), Counter()
    for r in results:
        for L, a, b in r.lengths:
            n[L] += a
            w[L] += b
    cols = [[sum(x) for x in zip(*[r[k] for r in results])] for k in (3, 4, 5)]
    return Stats([(L, n[L], w[L]) for L in sorted(n)], sum(r.n_inverted for r in results), sum(r.w120_inverted for r in results), *cols)


def invariants(st):
    """The three sums the host checks after every pass."""
    return (sum(n for _, n, _ in st.lengths) + st.n_inverted == sum(st.cn) and sum(w for _, _, w in st.lengths) + st.w120_inverted == sum(st.cw120)
            and sum(w * L for L, _, w in st.lengths) == sum(st.cbases120))


def to_double(x):
    """An exact non-negative integer as the library makes it a double: its leading 64 bits, converted once, scaled."""
    bl = int(x).bit_length()
    if bl <= 64:
        return float(int(x))
    return math.ldexp(float(int(x) >> (bl - 64)), bl - 64)


def metrics(lengths, cuts=CUTS):
    """The figures as a dict: integers exact, doubles made as the library makes them (mean and sd None for an empty sample)."""
    N, W = sum(n for _, n, _ in lengths), sum(w for _, _, w in lengths)
    m = dict(n=N, w120=W, min=0, max=0, mode=0, mean=None, sd=None, share=[0.0] * (len(cuts) + 1))
    m.update({k: 0 for k, _ in QS})
    if not lengths:
        return m
    m["min"], m["max"] = lengths[0][0], lengths[-1][0]
    best = max(w for _, _, w in lengths)
    m["mode"] = min(L for L, _, w in lengths if w == best)
    swl, swl2 = sum(w * L for L, _, w in lengths), sum(w * L * L for L, _, w in lengths)
    m["mean"] = to_double(swl) / float(W)
    var = W * swl2 - swl * swl
    assert var >= 0
    m["sd"] = math.sqrt(to_double(var)) / float(W) if var else 0.0
    for k, q in QS:
        cum = 0
        for L, _, w in lengths:
            cum += w
            if 100 * cum >= q * W:
                m[k] = L
                break
    edges = [0] + list(cuts) + [None]
    for k in range(len(cuts) + 1):
        inside = sum(w for L, _, w in lengths if L >= edges[k] and (edges[k + 1] is None or L < edges[k + 1]))
        m["share"][k] = inside / W          # (true division of two integers: correctly rounded)
    return m


def label(rep, is_ctrl):
    return f"{'c' if is_ctrl else 't'}{rep}"


def w_text(w):
    """A 1/120 value as --counts prints one."""
    return str(w // 120) if w % 120 == 0 else "%.2f" % (w / 120.0)


def lengths_text(samples, cut_sites=False):
    """samples: [(rep, is_ctrl, Stats)] -> --lengths' table."""
    out = [LENGTHS_COMMENT_J if cut_sites else LENGTHS_COMMENT, LENGTHS_HEADER]
    for rep, ctrl, st in samples:
        W, cum = sum(w for _, _, w in st.lengths), 0
        for L, n, w in st.lengths:
            cum += w
            out.append("%s\t%d\t%d\t%s\t%.6f\n" % (label(rep, ctrl), L, n, w_text(w), cum / W))
        if st.n_inverted:
            out.append("%s\tinverted\t%d\t%s\tNA\n" % (label(rep, ctrl), st.n_inverted, w_text(st.w120_inverted)))
    return "".join(out)


def metrics_header(cuts=CUTS):
    cols = ["sample", "intervals", "weight", "mean", "sd", "min", "p5", "q25", "median", "q75", "p95", "max", "mode"]
    if not cuts:
        cols.append("all")
    for k in range(len(cuts) + 1 if cuts else 0):
        cols.append(f"lt{cuts[0]}" if k == 0 else f"ge{cuts[k - 1]}" if k == len(cuts) else f"ge{cuts[k - 1]}_lt{cuts[k]}")
    return "\t".join(cols) + "\n"


def metrics_text(samples, cuts=CUTS):
    out = [metrics_header(cuts)]
    for rep, ctrl, st in samples:
        m = metrics(st.lengths, cuts)
        f = [label(rep, ctrl), str(m["n"]), w_text(m["w120"])]
        f += ["NA" if m[k] is None else "%.6f" % m[k] for k in ("mean", "sd")]
        f += [str(m[k]) for k in ("min", "p5", "q25", "median", "q75", "p95", "max", "mode")]
        f += ["%.6f" % s for s in m["share"]]
        out.append("\t".join(f) + "\n")
    return "".join(out)


def chrom_text(names, lens, samples):
    out = [CHROM_COMMENT, "chrom\tlength" + "".join("\t{0}.intervals\t{0}.weight\t{0}.share\t{0}.mean_depth".format(label(r, c)) for r, c, _ in samples) + "\n"]
    for i, (nm, ln) in enumerate(zip(names, lens)):
        row = [nm, str(ln)]
        for _, _, st in samples:
            W = sum(st.cw120)
            row += [str(st.cn[i]), w_text(st.cw120[i]), "%.6f" % (st.cw120[i] / W if W else 0.0), "%.6f" % (st.cbases120[i] / (120 * ln) if ln else 0.0)]
        out.append("\t".join(row) + "\n")
    return "".join(out)
