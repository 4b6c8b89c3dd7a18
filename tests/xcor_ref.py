"""The strand cross-correlation's reference, in numpy and Python integers (include/genrich_amd.h, gx_set_xcor).

Tags are (chromosome, position, strand) with strand 1 = plus, 0 = minus.  counts() makes one boolean array per chromosome and
strand and takes n11(d) by slicing: the positions x with plus[x] and minus[x + d], 0 <= x, x + d < len.  r(d), the figures and
the two texts follow the header's definitions: the numerator N n11 - nP nM and the radicand nP (N - nP) nM (N - nM) are Python
integers, each converted ONCE the way the library converts a big integer (its leading 64 bits, rounded by the conversion to a
double, scaled), then one math.sqrt and one division."""
import math
from typing import NamedTuple

import numpy as np


class Counts(NamedTuple):
    n_pos: int
    n_plus: int
    n_minus: int
    rejected: int
    lo: int
    hi: int
    n11: list


def counts(lens, tags, lo, hi, active=None):
    """Counts of `tags` (rows chrom, pos, strand; any integer array-like) over chromosomes of `lens`; active[c] False: the
    chromosome takes no part (its tags set nothing, its length is not in N).  A tag beyond the table, at or beyond its
    chromosome's length (active or not) or with a strand above 1 is rejected."""
    nc = len(lens)
    active = [True] * nc if active is None else [bool(a) for a in active]
    plus = [np.zeros(L, dtype=bool) for L in lens]
    minus = [np.zeros(L, dtype=bool) for L in lens]
    t = np.asarray(tags, dtype=np.int64).reshape(-1, 3)
    lens_a = np.asarray(list(lens) + [0], dtype=np.int64)
    c = t[:, 0]
    known = c < nc
    bad = ~known | (t[:, 1] >= lens_a[np.where(known, c, nc)]) | (t[:, 2] > 1)
    rejected = int(bad.sum())
    for ci in range(nc):
        if not active[ci]:
            continue
        sel = ~bad & (c == ci)
        plus[ci][t[sel & (t[:, 2] == 1), 1]] = True
        minus[ci][t[sel & (t[:, 2] == 0), 1]] = True
    N = sum(L for L, a in zip(lens, active) if a)
    nP = sum(int(p.sum()) for p in plus)
    nM = sum(int(m.sum()) for m in minus)
    n11 = []
    for d in range(lo, hi + 1):
        tot = 0
        for p, m in zip(plus, minus):
            L = len(p)
            if abs(d) >= L:
                continue
            tot += int(np.count_nonzero(p[:L - d] & m[d:])) if d >= 0 else int(np.count_nonzero(p[-d:] & m[:L + d]))
        n11.append(tot)
    return Counts(N, nP, nM, rejected, lo, hi, n11)


def sub_range(c, lo, hi):
    """The counts of a narrower range of shifts: n11(d) does not depend on the range."""
    assert c.lo <= lo <= hi <= c.hi
    return c._replace(lo=lo, hi=hi, n11=c.n11[lo - c.lo:hi - c.lo + 1])


def to_double(v):
    """A non-negative Python integer as the library converts one: the leading 64 bits, converted (round to nearest even), scaled."""
    if v == 0:
        return 0.0
    bits = v.bit_length()
    if bits <= 64:
        return float(v)
    return math.ldexp(float(v >> (bits - 64)), bits - 64)


def curve(c):
    """[r(d)] for lo .. hi; None where undefined (the radicand is 0)."""
    N, nP, nM = c.n_pos, c.n_plus, c.n_minus
    rad = nP * (N - nP) * nM * (N - nM)
    if rad == 0:
        return [None] * len(c.n11)
    den = math.sqrt(to_double(rad))
    out = []
    for n in c.n11:
        num = N * n - nP * nM
        out.append((to_double(num) if num >= 0 else -to_double(-num)) / den)
    return out


def metrics(c, read_len=0):
    """The figures as a dict; None where undefined ('NA')."""
    r = curve(c)
    ph = read_len - 1
    m = dict(fragment_length=None, frag_shift=None, r_frag=None, min_shift=None, r_min=None, phantom_shift=ph if read_len else None, r_phantom=None,
             nsc=None, rsc=None)
    if read_len and c.lo <= ph <= c.hi:
        m["r_phantom"] = r[ph - c.lo]
    if r[0] is None:
        return m
    for d in range(c.lo, c.hi + 1):
        v = r[d - c.lo]
        if m["r_min"] is None or v < m["r_min"]:
            m["r_min"], m["min_shift"] = v, d
        if d < 1 or (read_len and abs(d - ph) <= 10):
            continue
        if m["r_frag"] is None or v > m["r_frag"]:
            m["r_frag"], m["frag_shift"] = v, d
    if m["r_frag"] is not None:
        m["fragment_length"] = m["frag_shift"] + 1
        if m["r_min"] > 0:
            m["nsc"] = m["r_frag"] / m["r_min"]
        if m["r_phantom"] is not None and m["r_phantom"] - m["r_min"] > 0:
            m["rsc"] = (m["r_frag"] - m["r_min"]) / (m["r_phantom"] - m["r_min"])
    return m


def _f(v):
    return "NA" if v is None else "%.6f" % v


def _label(rep, ctrl):
    return ("c" if ctrl else "t") + str(rep)


def curve_text(samples):
    """--xcor's table; samples: [(rep, is_ctrl, Counts)]."""
    out = ["sample\tshift\tn11\tr\n"]
    for rep, ctrl, c in samples:
        lab = _label(rep, ctrl)
        out.append(f"# {lab}\tn_pos={c.n_pos}\tn_plus={c.n_plus}\tn_minus={c.n_minus}\trejected={c.rejected}\n")
        for d, n, r in zip(range(c.lo, c.hi + 1), c.n11, curve(c)):
            out.append(f"{lab}\t{d}\t{n}\t{_f(r)}\n")
    return "".join(out)


def metrics_text(samples, read_len=0):
    """--xcor-metrics' table."""
    out = ["sample\tn_pos\tn_plus\tn_minus\tfragment_length\tr_frag\tmin_shift\tr_min\tphantom_shift\tr_phantom\tNSC\tRSC\n"]
    for rep, ctrl, c in samples:
        m = metrics(c, read_len)
        i = lambda v: "NA" if v is None else str(v)
        out.append("\t".join([_label(rep, ctrl), str(c.n_pos), str(c.n_plus), str(c.n_minus), i(m["fragment_length"]), _f(m["r_frag"]), i(m["min_shift"]),
                              _f(m["r_min"]), i(m["phantom_shift"]), _f(m["r_phantom"]), _f(m["nsc"]), _f(m["rsc"])]) + "\n")
    return "".join(out)
