"""A numpy reference for the genome bit vectors, GC content, the expected and observed GC tables, the percent classes, the
ratio and the two tables' text (include/genrich_amd.h, "the reference sequence, GC bias per sample and GC content per
interval"), by prefix sums over one byte per base.  Exact integers; the ratio repeats the library's one conversion per product."""
import math
from typing import NamedTuple

import numpy as np

VALID_COUNTS = (1, 2, 3, 4, 5, 6, 8, 10)
CLASSES = 101
MAX_WINDOW = 4096

_GC = np.zeros(256, dtype=bool)
_ACGT = np.zeros(256, dtype=bool)
for _c in b"GCgc":
    _GC[_c] = True
for _c in b"ACGTacgt":
    _ACGT[_c] = True


class Tables(NamedTuple):
    window: int
    F: list
    f_unclassed: int
    Nn: list
    Nw: list
    n_unclassed: int
    w_unclassed: int


def pack(seq, length):
    """(gc, acgt) bool arrays of `length` bases for the sequence bytes `seq` (None or shorter: the rest is unknown)."""
    gc, ac = np.zeros(length, dtype=bool), np.zeros(length, dtype=bool)
    if seq:
        b = np.frombuffer(bytes(seq), dtype=np.uint8)[:length]
        gc[:len(b)], ac[:len(b)] = _GC[b], _ACGT[b]
    return gc, ac


def genome(seqs, lens):
    return [pack(s, n) for s, n in zip(seqs, lens)]


def _prefix(bits, extra=0):
    return np.concatenate([[0], np.cumsum(np.concatenate([bits, np.zeros(extra, dtype=bool)]), dtype=np.int64)])


def content(gen, regions):
    """[(gc, acgt)] of (chrom, start, end) rows: end clamped to the length, end <= start or an unknown chromosome: 0."""
    pre = [(_prefix(g), _prefix(a)) for g, a in gen]
    out = []
    for c, s, e in regions:
        c, s, e = int(c), int(s), int(e)
        if c >= len(gen):
            out.append((0, 0))
            continue
        e = min(e, len(gen[c][0]))
        out.append((int(pre[c][0][e] - pre[c][0][s]), int(pre[c][1][e] - pre[c][1][s])) if s < e else (0, 0))
    return out


def _window_classes(gc, ac, W):
    """Per position of a chromosome: its window's class, -1 where not classed."""
    pg, pa = _prefix(gc, W), _prefix(ac, W)
    n = len(gc)
    a = pa[W:W + n] - pa[:n]
    g = pg[W:W + n] - pg[:n]
    return np.where(a == W, g, -1)


def expected(gen, W, take=None):
    """(F[W + 1], unclassed) over the positions of the chromosomes with take[c] (None: all)."""
    F = np.zeros(W + 1, dtype=np.int64)
    un = 0
    for c, (gc, ac) in enumerate(gen):
        if take is not None and not take[c]:
            continue
        k = _window_classes(gc, ac, W)
        F += np.bincount(k[k >= 0], minlength=W + 1)
        un += int((k < 0).sum())
    return [int(x) for x in F], un


def observed(gen, events, W, active=None):
    """(Nn, Nw, n_unclassed, w_unclassed) of the events a sample takes as intervals (gx_kept.h kept_interval): a count in
    VALID_COUNTS, a chromosome of the table that is active, a start below its length.  The window is the one at the start."""
    Nn, Nw = np.zeros(W + 1, dtype=np.int64), np.zeros(W + 1, dtype=np.int64)
    nu = wu = 0
    ch, st, cnt = (np.asarray(events[k], dtype=np.int64) for k in ("chrom", "start", "count"))
    ok = np.isin(cnt, VALID_COUNTS) & (ch < len(gen))
    for c, (gc, ac) in enumerate(gen):
        if active is not None and not active[c]:
            continue
        m = ok & (ch == c) & (st < len(gc))
        if not m.any():
            continue
        k = _window_classes(gc, ac, W)[st[m]]
        w = 120 // cnt[m]
        Nn += np.bincount(k[k >= 0], minlength=W + 1)
        Nw += np.bincount(k[k >= 0], weights=w[k >= 0], minlength=W + 1).astype(np.int64)
        nu += int((k < 0).sum())
        wu += int(w[k < 0].sum())
    return [int(x) for x in Nn], [int(x) for x in Nw], nu, wu


def tables(gen, events, W, active=None):
    F, fu = expected(gen, W, active)
    Nn, Nw, nu, wu = observed(gen, events, W, active)
    return Tables(W, F, fu, Nn, Nw, nu, wu)


def add(parts):
    parts = list(parts)
    W = parts[0].window
    s = lambda k: [sum(int(getattr(p, k)[g]) for p in parts) for g in range(W + 1)]
    t = lambda k: sum(int(getattr(p, k)) for p in parts)
    return Tables(W, s("F"), t("f_unclassed"), s("Nn"), s("Nw"), t("n_unclassed"), t("w_unclassed"))


def same(a, b):
    return (int(a.window) == int(b.window) and [int(x) for x in a.F] == [int(x) for x in b.F] and int(a.f_unclassed) == int(b.f_unclassed)
            and [int(x) for x in a.Nn] == [int(x) for x in b.Nn] and [int(x) for x in a.Nw] == [int(x) for x in b.Nw]
            and int(a.n_unclassed) == int(b.n_unclassed) and int(a.w_unclassed) == int(b.w_unclassed))


def gc_class(W, g):
    """The percent class of g in a window of W: round(100 g / W), halves up, in integers."""
    return (200 * g + W) // (2 * W)


def to_double(x):
    """A wide non-negative integer as the library converts one: its leading 64 bits, rounded once, scaled."""
    if x == 0:
        return 0.0
    shift = max(x.bit_length() - 64, 0)
    return math.ldexp(float(x >> shift), shift)


def fold(W, col):
    out = [0] * CLASSES
    for g in range(W + 1):
        out[gc_class(W, g)] += int(col[g])
    return out


def metrics(t):
    """The folded tables and the figures of gx_gc_metrics, as a dict."""
    W = t.window
    F, Nn, Nw = fold(W, t.F), fold(W, t.Nn), fold(W, t.Nw)
    sF, sW = sum(F), sum(Nw)
    ratio = [to_double(Nw[k] * sF) / to_double(F[k] * sW) if F[k] and sW else math.nan for k in range(CLASSES)]
    gF = sum(g * int(t.F[g]) for g in range(W + 1))
    gW = sum(g * int(t.Nw[g]) for g in range(W + 1))
    held = [k for k in range(CLASSES) if F[k] and sW and 100 * F[k] >= sF]
    lo = min(held, key=lambda k: (ratio[k], k)) if held else -1
    hi = max(held, key=lambda k: (ratio[k], -k)) if held else -1
    return dict(windows=sF, windows_unclassed=int(t.f_unclassed), intervals=sum(Nn), intervals_unclassed=int(t.n_unclassed), w120=sW,
                w120_unclassed=int(t.w_unclassed), cls_windows=F, cls_intervals=Nn, cls_w120=Nw, ratio=ratio,
                mean_gc_genome=to_double(gF) / to_double(sF * W) if sF else math.nan,
                mean_gc_sample=to_double(gW) / to_double(sW * W) if sW else math.nan,
                ratio_min=ratio[lo] if held else math.nan, ratio_max=ratio[hi] if held else math.nan, ratio_min_class=lo, ratio_max_class=hi)


def w120_text(w):
    return str(w // 120) if w % 120 == 0 else "%.2f" % (w / 120.0)


def _num(v):
    return "NA" if math.isnan(v) else "%.6f" % v


def bias_text(samples):
    """--gc-bias' table for [(rep, is_ctrl, Tables)]."""
    out = ["sample\tgc_percent\twindows\tintervals\tweight\tratio\n"]
    for rep, ctrl, t in samples:
        m = metrics(t)
        name = "%s%d" % ("c" if ctrl else "t", rep)
        out.append("# %s\tW=%d\twindows=%d\twindows_unclassed=%d\tintervals=%d\tintervals_unclassed=%d\n"
                   % (name, t.window, m["windows"], m["windows_unclassed"], m["intervals"], m["intervals_unclassed"]))
        for k in range(CLASSES):
            out.append("%s\t%d\t%d\t%d\t%s\t%s\n" % (name, k, m["cls_windows"][k], m["cls_intervals"][k], w120_text(m["cls_w120"][k]), _num(m["ratio"][k])))
    return "".join(out)


def peaks_text(names, regions, counts):
    """--gc-peaks' table for (chrom, start, end) rows and their [(gc, acgt)]."""
    out = ["chr\tstart\tend\tname\tlength\tacgt\tgc\tgc_fraction\n"]
    for i, ((c, s, e), (g, a)) in enumerate(zip(regions, counts)):
        out.append("%s\t%d\t%d\tpeak_%d\t%d\t%d\t%d\t%s\n" % (names[int(c)], s, e, i, int(e) - int(s), a, g, _num(g / a if a else math.nan)))
    return "".join(out)
