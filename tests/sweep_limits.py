"""The peak sweep's index space, rebuilt on the CPU, and inputs constructed to sit on its limits.

callPeaks on bit masks (genrich_amd/csrc/gx_stats.h, launched by run_sweep, gx_host_sweep.h) walks ONE index space: the
concatenated interval table ("tight": GX_NO_LOOSE, any control or replicate run, -q tight) or the tile stage's loose slots
("loose": slot(tile) = keys before it + its number; a tile has n + 1 slots, its intervals first, the others zero-length
fillers that are never significant -- gx_sbtile.h:17, :613).  sweep_census() gives every interval of the ORACLE's final table
its index in that space, rebuilds the significance / SKIP / chromosome-start bits, the runs, the candidates (run_is_head's rule)
and every candidate's float32 AUC terms -- and checks itself: with min_auc = min_len = 0 its candidates are the oracle's peaks.

The inputs are pileup PROFILES written by hand: a list of (length, pileup) segments per chromosome, turned into fragments
(first in, first out).  Every segment is one interval.  lambda is held at about 0.3 by the length of a chromosome that only
exists for that, so that pileups 0 and 1 are quiet (p = 0, 1.39) and 3 and more significant at -p 0.01 (2.74, 3.19, 3.55, ...).
Positions are moved with ballast: quiet single fragments on a chromosome before the stage (two intervals / two keys each; one
that ends at the chromosome's length: one), in the tight and in the loose space by different amounts -- assemble() adds ballast
until the marked interval has the index the case wants.  The cases that also run with -q multiply their significant pileups
(`boost`) and carry a wide, very high plateau on the lambda chromosome (`plateau`): only then has every level a q of its own.

Numpy and the oracle only: no GPU."""
from __future__ import annotations

import collections
import functools

import numpy as np

import backends as B
import ties as T

TB = 12
TILE = 1 << TB
SW_NT = 256             # gx_stats.h:1189
SW_ITEMS = 8            # gx_stats.h:1190  mask words per thread of the run pass
SW_CHUNK = SW_NT * SW_ITEMS   # gx_stats.h:1191  mask words per chunk (2048)
RC_CHUNK = SW_NT        # gx_stats.h:1194  runs / candidates per chunk of k_cands and k_peaks
RUN_NCH = 1024          # gx_stats.h:1680  chromosome starts runs_body<TABLE> keeps in LDS
PK_SHORT = 1024         # gx_stats.h:1296  i1 - i0 >= PK_SHORT: the candidate is walked by a wavefront (k_cand_hdr :1318)
LAMBDA = 0.3
PLATEAU_LEN, PLATEAU_V = 20_000, 200   # (p = 13.0: above p + log10(bases) of every level of a stage, 6.8 + 4.4 at the most)
QUIET, SIG = 1, 3       # the highest quiet pileup, the lowest significant one
GX_SKIP = np.float32(-1.0)


# ---- the index space -------------------------------------------------------------------------------------------------------------

def keys_per_tile(ev, lens):
    """keys of every tile as the tile stage counts them (a start key per fragment, an end key unless it ends at the length)"""
    lens = np.asarray(lens, dtype=np.int64)
    base = np.concatenate([[0], np.cumsum((lens + TILE - 1) >> TB)])
    c, s, e = ev["chrom"].astype(np.int64), ev["start"].astype(np.int64), ev["end"].astype(np.int64)
    has_end = e < lens[c]
    kt = np.concatenate([base[c] + (s >> TB), base[c[has_end]] + (e[has_end] >> TB)])
    return np.bincount(kt, minlength=base[-1]), base


def index_space(lens, ev, ends, space):
    """(index of every interval, per chromosome; size of the space).  ends[c]: the chromosome's interval ends, the closing one last."""
    if space == "tight":
        out, off = [], 0
        for e in ends:
            out.append(off + np.arange(len(e), dtype=np.int64))
            off += len(e)
        return out, off
    assert space == "loose"
    n, base = keys_per_tile(ev, lens)
    slot = np.concatenate([[0], np.cumsum(n)])[:-1] + np.arange(len(n))
    out = []
    for c, e in enumerate(ends):
        e = np.asarray(e, dtype=np.int64)
        if len(e) == 0:
            out.append(e)
            continue
        assert e[-1] == lens[c]
        t = np.where(e < lens[c], e >> TB, (lens[c] - 1) >> TB) + base[c]   # an interval is the tile's in which it ends
        rank = np.arange(len(e)) - np.searchsorted(t, t, side="left")
        assert (rank <= n[t]).all(), "a tile with more intervals than slots"
        out.append(slot[t] + rank)
    return out, int(n.sum()) + len(n)


Census = collections.namedtuple("Census", "space col N idx chrom start end pq sig skip brk runs cands terms words")


def sweep_census(o, case, space, par):
    """The sweep's view of the oracle's final table.  idx[c]: the intervals' indices; chrom / start / end / pq / sig / skip over
    the index space (fillers: chrom -1); brk: the indices that open a chromosome; runs: (first, last) index; cands: (first run,
    last run, i0, i1); terms[k]: candidate k's float32 products (e - s) * (pq - thr) in interval order; words: sig / skip / brk
    as 64-bit mask words."""
    lens = case["lens"]
    ev = case["replicates"][0]["treat"]
    nch = len(lens)
    got = [o.get_intervals(-1, c) for c in range(nch)]
    ends = [g[0].astype(np.int64) for g in got]
    col = "q" if par.qval_opt else "p"
    idx, N = index_space(lens, ev, ends, space)
    chrom = np.full(N, -1, dtype=np.int64)
    start, end = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    pq = np.zeros(N, dtype=np.float32)
    brk = []
    if space == "loose":
        n, base = keys_per_tile(ev, lens)
        slot = np.concatenate([[0], np.cumsum(n)])[:-1] + np.arange(len(n))
        brk = [int(slot[base[c]]) for c in range(nch)]          # tileSlot[first tile] (ChromStarts, gx_stats.h:1675)
    for c in range(nch):
        if len(ends[c]) == 0:
            continue
        i = idx[c]
        chrom[i], end[i], pq[i] = c, ends[c], got[c][1][col]
        start[i] = np.concatenate([[0], ends[c][:-1]])
        if space == "tight":
            brk.append(int(i[0]))
    thr = np.float32(par.thr)
    sig = (chrom >= 0) & (pq > thr)
    skip = (chrom >= 0) & (pq == GX_SKIP)
    isbrk = np.zeros(N, dtype=bool)
    isbrk[brk] = True
    # runs: adjacent significant indices, cut at a chromosome's first index
    prev = np.concatenate([[False], sig[:-1]])
    nxt = np.concatenate([sig[1:], [False]])
    nbrk = np.concatenate([isbrk[1:], [False]])
    rs = np.flatnonzero(sig & (~prev | isbrk))
    re = np.flatnonzero(sig & (~nxt | nbrk))
    assert len(rs) == len(re) and (rs <= re).all()
    runs = np.stack([rs, re], axis=1) if len(rs) else np.zeros((0, 2), dtype=np.int64)
    # candidates: run r links to run r - 1 on one chromosome, with no SKIP between, at a gap of 0 or at most max_gap
    heads = []
    for r in range(len(rs)):
        head = r == 0
        if not head:
            a, s = re[r - 1], rs[r]
            head = isbrk[s] or chrom[a] != chrom[s]
            if not head:
                gap = start[s] - end[a]
                assert gap >= 0
                head = (gap != 0 and gap > par.max_gap) or bool(skip[a + 1:s].any())
        if head:
            heads.append(r)
    cands = []
    for k, r0 in enumerate(heads):
        r1 = (heads[k + 1] if k + 1 < len(heads) else len(rs)) - 1
        cands.append((r0, r1, int(rs[r0]), int(re[r1])))
    terms = []
    for _, _, i0, i1 in cands:
        m = np.flatnonzero(sig[i0:i1 + 1]) + i0
        terms.append((end[m] - start[m]).astype(np.float32) * (pq[m] - thr))
    # the self-check: every candidate a peak at min_auc = min_len = 0
    if par.min_auc == 0.0 and par.min_len == 0:
        pk = o.get_peaks()
    else:
        o2 = B.Oracle(T.params(par, min_auc=0.0, min_len=0))
        B.run_case(o2, case)
        pk = o2.get_peaks()
        o2.close()
    mine = [(int(chrom[i0]), int(start[i0]), int(end[i1])) for _, _, i0, i1 in cands]
    theirs = [(int(p["chrom"]), int(p["start"]), int(p["end"])) for p in pk]
    assert mine == theirs, ("the census is wrong", len(mine), len(theirs), [x for x in zip(mine, theirs) if x[0] != x[1]][:3])

    def words(b):
        w = np.zeros(((N + 63) // 64) * 64, dtype=np.uint8)
        w[:N] = b
        return np.packbits(w.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1)
    return Census(space, col, N, idx, chrom, start, end, pq, sig, skip, isbrk, runs, cands, terms,
                  dict(sig=words(sig), skip=words(skip), brk=words(isbrk)))


def seq_sum(t):
    """float32 sum in order, as updatePeak adds (Genrich.c:950)"""
    a = np.float32(0.0)
    for x in np.asarray(t, dtype=np.float32):
        a = np.float32(a + x)
    return a


def pair_sum(t):
    t = np.asarray(t, dtype=np.float32)
    while len(t) > 1:
        if len(t) % 2:
            t = np.concatenate([t, np.zeros(1, dtype=np.float32)])
        t = (t[0::2] + t[1::2]).astype(np.float32)
    return np.float32(t[0]) if len(t) else np.float32(0.0)


def cand_len(cen, k):
    """a candidate's length in index units (fillers inside count)"""
    return cen.cands[k][3] - cen.cands[k][2] + 1


# ---- profiles -> fragments -------------------------------------------------------------------------------------------------------

def profile(chrom, segs):
    """[(length, pileup)] from base 0 -> (fragments, interval ends, chromosome length); every segment is one interval"""
    frags, open_, ends = [], collections.deque(), []
    x = h = 0
    prev = None
    for ln, v in segs:
        assert ln >= 1 and v != prev and v >= 0, (ln, v, prev)
        if v > h:
            open_.extend([x] * (v - h))
        for _ in range(h - v):
            frags.append((chrom, open_.popleft(), x))
        h = prev = v
        x += ln
        ends.append(x)
    frags += [(chrom, s, x) for s in open_]
    return frags, np.array(ends, dtype=np.int64), x


def rows(frags):
    a = np.zeros(len(frags), dtype=B.EVENT_DTYPE)
    if len(frags):
        f = np.asarray(frags, dtype=np.int64)
        a["chrom"], a["start"], a["end"], a["count"] = f[:, 0], f[:, 1], f[:, 2], 1
    return a


def quiet_chrom(b, clen=None, tail_sig=False):
    """a chromosome of exactly b intervals, all quiet: pairs of (a gap, a single fragment of 40 bases); an even b: the last
    fragment ends at the chromosome's length.
    tail_sig: the chromosome closes with a stair of single fragments that end at its length -- three or four start keys on
    distinct bases and no end key, the closing interval (pileup 3 or 4) significant; every key of the chromosome then lies on a
    base of its own and every such base ends an interval, so its last tile's slots are all taken: the closing interval is the
    slot before the next chromosome's first."""
    if tail_sig:
        assert b >= 5
        h = 3 if b % 2 == 0 else 4
        m = (b - h - 1) // 2
        return [(10, 0), (40, 1)] * m + [(10, 0)] + [(5, v) for v in range(1, h)] + [(30, h)]
    assert b >= 1
    m = b // 2
    L = -(-(50 * m + 60) // TILE) * TILE          # whole tiles: one interval more rarely moves the chromosomes behind it
    if b % 2:
        return [(10, 0), (40, 1)] * m + [(L - 50 * m, 0)]
    return [(10, 0), (40, 1)] * (m - 1) + [(L - 50 * (m - 1) - 40, 0), (40, 1)]


def run_of(k, lens=(3, 2, 4, 1, 5), levels=(3, 4, 3, 5), first=None):
    """k significant segments whose neighbours differ in pileup"""
    out = [(lens[i % len(lens)], levels[i % len(levels)]) for i in range(k)]
    if first is not None:
        out[0] = (out[0][0], first)
    return out


class Stage:
    """segments of the stage chromosome, with names for the segments a case is about"""

    def __init__(self):
        self.segs, self.marks = [], {}

    def add(self, segs, mark=None):
        if mark:
            self.marks[mark] = len(self.segs)
        segs = list(segs)
        if self.segs and segs and self.segs[-1][1] == segs[0][1]:   # two quiet stretches in a row: one interval
            assert segs[0][1] == 0
            self.segs[-1] = (self.segs[-1][0] + segs[0][0], 0)
            segs = segs[1:]
        self.segs += segs
        return self

    def quiet(self, g=50):
        return self.add([(g, 0)])

    @property
    def pos(self):
        return sum(s[0] for s in self.segs)

    def to_tile(self, off=10):
        """quiet up to `off` bases behind the next tile border"""
        g = (-self.pos) % TILE + off
        return self.quiet(g if g > 1 else g + TILE)


def assemble(space, stage, *, target=None, lam_first=False, empties=0, pre=True, tail_sig=False, bed=None, boost=1, plateau=False):
    """lens, events and the predicted indices of the stage's segments.  Chromosomes: [lam if lam_first] + pre (ballast) + `empties`
    chromosomes of 100 bases nobody touches + the stage + [lam unless lam_first].  target = (mark, modulus, residue): ballast on
    `pre` until the marked segment's index = residue mod modulus (modulus 0: = residue).  tail_sig: `pre` closes significant
    (quiet_chrom).  bed = (mark, k, offset, width): a -E region of `width` bases, `offset` bases into the (quiet) segment k behind
    the marked one; its SKIP interval is marked "skip".  plateau: the lam chromosome carries one interval of PLATEAU_LEN bases at a
    pileup far above the stage's (the cases that also run with -q: Benjamini-Hochberg's q = p - log10(genome) + log10(bases more
    significant) is capped by the q of the most significant value, whose own count is 1 -- without a wide value on top every
    significant level of the stage gets that one q, and a q read from the wrong interval would be the right number)."""
    # boost: the significant pileups times this (the cases that also run with -q: q = p - log10(genome) + log10(bases at least as
    # significant) is zero for every interval unless p is large); `levels` keeps the designed ones
    segs, marks = [(l, v if v <= QUIET else v * boost) for l, v in stage.segs], dict(stage.marks)
    levels = [v for _, v in stage.segs]
    bed_at = None
    if bed:
        g = marks[bed[0]] + bed[1]
        assert segs[g][1] == 0 and 0 < bed[2] and bed[2] + bed[3] < segs[g][0]
        x0 = sum(l for l, _ in segs[:g]) + bed[2]
        bed_at = (x0, x0 + bed[3])
        levels[g:g + 1] = [0, -1, 0]                      # the quiet interval is cut in three: quiet, SKIP, quiet
        marks = {k: v + 2 if v > g else v for k, v in marks.items()}
        marks["skip"] = g + 1

    def build(b, lam_len=None, lam_fill=0):
        top = [(50, 0), (PLATEAU_LEN, PLATEAU_V)] if plateau else []
        used = 50 * lam_fill + sum(l for l, _ in top)
        lam = ("lam", [(10, 0), (40, 1)] * lam_fill + top + [(lam_len - used, 0)] if lam_len else top + [(TILE, 0)])
        chroms = [lam] if lam_first else []
        if pre:
            chroms.append(("pre", quiet_chrom(b, TILE, tail_sig)))
        chroms += [("empty", [(100, 0)])] * empties
        chroms.append(("stage", segs))
        if not lam_first:
            chroms.append(lam)
        frags, ends, lens = [], [], []
        for c, (name, sg) in enumerate(chroms):
            f, e, l = profile(c, sg)
            if name == "stage" and bed_at:
                e = np.unique(np.concatenate([e, bed_at]))
            frags += f
            ends.append(e)
            lens.append(l)
        return [n for n, _ in chroms], frags, ends, lens

    def with_lambda(b):
        names, frags, ends, lens = build(b)
        f = np.asarray(frags, dtype=np.int64)
        frag = int((f[:, 2] - f[:, 1]).sum())
        others = sum(l for n, l in zip(names, lens) if n != "lam")
        fill = max(0, int(np.ceil((others + TILE - frag / LAMBDA) / 80.0)))   # (a fragment of 40 buys 133 bases and takes 50)
        if lam_first:   # (ahead of the stage its intervals count: as many for every amount of ballast)
            fill = held.setdefault("fill", fill)
        lam_len = int(round((frag + 40 * fill) / LAMBDA)) - others
        assert lam_len >= 50 * fill + 60 + (PLATEAU_LEN + 50 if plateau else 0), (lam_len, fill)
        return build(b, lam_len, fill)

    b = b_min = 5 if tail_sig else 1
    held = {}
    assert pre or target is None
    for _ in range(12):
        names, frags, ends, lens = with_lambda(b)
        ev = rows(frags)
        idx, N = index_space(lens, ev, ends, space)
        sc = names.index("stage")
        assert len(idx[sc]) == len(levels)
        if target is None:
            break
        mark, mod, res = target
        at = int(idx[sc][marks[mark]])
        d = res - at
        if mod:   # the nearest index of that residue, before or behind
            d = (d + mod // 2) % mod - mod // 2
            d += mod if b + d < b_min else 0
        if d == 0:
            break
        assert b + d >= b_min, "the stage alone is already behind the target"
        b += d   # (an interval more on `pre` is an index more -- tight -- or a key more -- loose --, but for a tile now and then)
    else:
        raise AssertionError("ballast did not converge")
    beds = None
    if bed_at:
        beds = [[] for _ in lens]
        beds[sc] = list(bed_at)
    return dict(space=space, names=names, lens=lens, ev=ev, stage=sc, idx=idx[sc], N=N, levels=np.array(levels), marks=marks,
                case=dict(lens=lens, beds=beds, replicates=[dict(save=None, treat=ev, ctrl=None)]))


def replay(cen, k, thr):
    """updatePeak (Genrich.c:943-970) over candidate k of the census: (float32 AUC, summit position relative to the start)"""
    _, _, i0, i1 = cen.cands[k]
    auc, best, pos, blen = np.float32(0.0), np.float32(-1.0), 0, 0
    origin = int(cen.start[i0])
    thr = np.float32(thr)
    for i in range(i0, i1 + 1):
        if not cen.sig[i]:
            continue
        s, e, v = int(cen.start[i]), int(cen.end[i]), cen.pq[i]
        auc = np.float32(auc + np.float32(np.float32(e - s) * np.float32(v - thr)))
        if v > best or (v == best and e - s > blen):
            if v > best:
                best = v
            pos, blen = (e + s) // 2 - origin, e - s
    return auc, pos


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
# name -> dict(space, lens, ev, case, idx (the stage's segments), levels, marks, par (make_params' arguments), also(census))

PAR = dict(pq=0.01, min_auc=0.0, min_len=0, max_gap=0)
WORD = 64
THREAD = SW_ITEMS * WORD          # indices per thread of the run pass
CHUNK = SW_CHUNK * WORD           # indices per chunk of the run pass (131,072)


def _case(a, also, **par):
    a["par"] = {**PAR, **par}
    a["thr"] = B.minus_log10f(a["par"]["pq"])
    a["also"] = also
    return a


def on_stage(cen, a):
    """the candidates that lie on the stage chromosome"""
    return [k for k, c in enumerate(cen.cands) if cen.chrom[c[2]] == a["stage"]]


def _run_of_index(cen, i):
    r = int(np.searchsorted(cen.runs[:, 0], i, side="right")) - 1
    assert r >= 0 and cen.runs[r, 0] <= i <= cen.runs[r, 1], ("no run holds index", i)
    return r


def case_run_border(space, modulus, residue, absolute=False):
    """a run of six significant intervals whose fourth sits at `residue` of `modulus`: residue 0 -- the run crosses the border
    (a word's, a thread's eight words', a chunk's 2048); residue 63 of 64 with a run that ENDS there is case_run_ends_bit63"""
    st = Stage().quiet(200).add(run_of(3)).add(run_of(3, first=5), "x").quiet(100).add(run_of(2)).quiet(60)
    a = assemble(space, st, target=("x", 0 if absolute else modulus, residue))

    def also(cen):
        i = int(a["idx"][a["marks"]["x"]])
        assert i % modulus == residue % modulus and (not absolute or i == residue) and cen.sig[i - 3:i + 3].all() and not cen.sig[i - 4] and not cen.sig[i + 3]
        r = _run_of_index(cen, i)
        assert tuple(cen.runs[r]) == (i - 3, i + 2)       # one run, open across the border
        w = i // WORD
        assert cen.words["sig"][w] & 1 and cen.words["sig"][w - 1] >> 63
    return _case(a, also)


def case_run_ends_bit63(space):
    st = Stage().quiet(200).add(run_of(4)).add(run_of(1, first=6), "x").quiet(100).add(run_of(2)).quiet(60)
    a = assemble(space, st, target=("x", WORD, WORD - 1))

    def also(cen):
        i = int(a["idx"][a["marks"]["x"]])
        assert i % WORD == WORD - 1 and cen.sig[i] and not cen.sig[i + 1]
        assert tuple(cen.runs[_run_of_index(cen, i)]) == (i - 4, i)
        assert not cen.words["sig"][i // WORD + 1] & 1
    return _case(a, also)


def case_chrom_start(space, modulus, absolute=False):
    """the stage's first interval at bit 0 of a word (of a chunk's first word), significant, and so is the closing interval of the
    chromosome before it: two runs, two peaks"""
    st = Stage().add(run_of(3)).quiet(100).add(run_of(2)).quiet(60)
    st.marks["x"] = 0
    a = assemble(space, st, target=("x", 0 if absolute else modulus, modulus if absolute else 0), tail_sig=True)

    def also(cen):
        i = int(a["idx"][0])
        assert i % modulus == 0 and i > 0 and cen.sig[i] and cen.sig[i - 1] and cen.brk[i]
        assert cen.chrom[i - 1] == a["stage"] - 1 and cen.chrom[i] == a["stage"]
        r = _run_of_index(cen, i)
        assert cen.runs[r, 0] == i and cen.runs[r - 1, 1] == i - 1          # cut between bit 63 and bit 0
        assert cen.words["brk"][i // WORD] & 1 and cen.words["sig"][i // WORD - 1] >> 63
    return _case(a, also)


def case_table_end(residue):
    """tight: the table ends with a run of three significant intervals, its last one (the stage's closing interval) at index
    N - 1 with N = residue mod 64: residue 1 -- a last word with one interval in it; residue 0 -- a table of exactly 64 k"""
    st = Stage().quiet(200).add(run_of(2)).quiet(100).add(run_of(3), "x")
    a = assemble("tight", st, target=("x", WORD, (residue - 3) % WORD), lam_first=True, boost=3, plateau=True)

    def also(cen):
        assert cen.N % WORD == residue and a["stage"] == len(a["lens"]) - 1
        assert cen.sig[cen.N - 3:].all() and not cen.sig[cen.N - 4] and tuple(cen.runs[-1]) == (cen.N - 3, cen.N - 1)
        assert cen.end[cen.N - 1] == a["lens"][-1]
        assert len(cen.words["sig"]) == (cen.N + 63) // 64
    return _case(a, also)


def case_index0(space):
    """a run of length 1 at index 0: the first chromosome's first interval, alone"""
    st = Stage().add(run_of(1)).quiet(100).add(run_of(2)).quiet(60)
    a = assemble(space, st, pre=False)

    def also(cen):
        assert a["stage"] == 0 and a["idx"][0] == 0 and cen.sig[0] and not cen.sig[1] and tuple(cen.runs[0]) == (0, 0)
        assert cen.cands[0][2:] == (0, 0) and cen.start[0] == 0
    return _case(a, also)


def case_many_chroms():
    """loose: more chromosomes than runs_body<TABLE> caches (RUN_NCH), the stage behind 1030 of them with a significant first slot,
    and the chromosome before it closing significant"""
    st = Stage().add(run_of(3)).quiet(100).add(run_of(2)).quiet(60)
    a = assemble("loose", st, empties=1030)

    def also(cen):
        i = int(a["idx"][0])
        assert a["stage"] > RUN_NCH and len(a["lens"]) > RUN_NCH and cen.sig[i] and cen.brk[i] and cen.runs[0, 0] == i
    return _case(a, also)


LINK_GAP = 10


def case_link(cut, n_before=255):
    """tight or loose alike (one tile border at most between two runs is avoided: every run in the quiet part of a tile): 255
    isolated runs, then run 255 and run 256 -- a chunk of k_cands apart -- at a gap of max_gap (linked) or max_gap + 1 (cut); at
    the end three linked runs, the last of them run R - 1"""
    st = Stage().quiet(100)
    for _ in range(n_before):
        st.add(run_of(2)).quiet(30)
    st.add(run_of(3), "a").quiet(LINK_GAP + (1 if cut else 0)).add(run_of(2), "b").quiet(30)
    for _ in range(5):
        st.add(run_of(2)).quiet(30)
    st.add(run_of(2), "t").quiet(LINK_GAP).add(run_of(1)).quiet(LINK_GAP - 1).add(run_of(4)).quiet(60)
    return st


def case_cand_border(space, cut):
    a = assemble(space, case_link(cut))

    def also(cen):
        R = len(cen.runs)
        assert R > RC_CHUNK
        ra, rb = _run_of_index(cen, int(a["idx"][a["marks"]["a"]])), _run_of_index(cen, int(a["idx"][a["marks"]["b"]]))
        assert (ra, rb) == (RC_CHUNK - 1, RC_CHUNK)                  # run 256 reads runEnd[255] of the chunk before
        firsts = [c[0] for c in cen.cands]
        assert (rb in firsts) == cut and ra in firsts
        assert cen.cands[-1][:2] == (R - 3, R - 1)                   # rLast = R - 1 for the last candidate
        assert len(cen.cands) == R - 2 - (0 if cut else 1)
    return _case(a, also, max_gap=LINK_GAP)


def case_exact_runs(space, R, **par):
    """exactly R isolated runs (R = H = 256: one full chunk of k_cands and of k_peaks; 257: a chunk of one)"""
    st = Stage().quiet(100)
    for k in range(R):
        st.add(run_of(2 + k % 3)).quiet(30)
    a = assemble(space, st)

    def also(cen):
        assert len(cen.runs) == R == len(cen.cands)
    return _case(a, also, **par)


N_MANY = 65 * RC_CHUNK + 1


def case_many_runs(space):
    """16,641 isolated runs at max_gap = 0: 66 chunks of runs, of candidates and of peaks -- more than a look-back window of 64"""
    st = Stage().quiet(100)
    for k in range(N_MANY):
        st.add([(2, 3)]).quiet(6)
    a = assemble(space, st)

    def also(cen):
        assert len(cen.runs) == len(cen.cands) == N_MANY and -(-N_MANY // RC_CHUNK) > 65
    return _case(a, also)


def case_plateau_tile_border(max_gap=0):
    """loose: a plateau that goes on over a tile border -- the tile's spare slots, zero-length fillers, lie between its two runs,
    which are 0 bases apart: linked at max_gap = 0, and the candidate's length counts the fillers.  max_gap = -1: every quiet
    interval ends a peak (Genrich.c:1032: end - peakEnd > maxGap), adjacent significant intervals still are one -- nothing but
    run_is_head's `gap != 0` keeps the plateau whole"""
    st = Stage().quiet(TILE - 40).add(run_of(30, lens=(3,)), "x").quiet(100).add(run_of(2)).quiet(60)
    a = assemble("loose", st, boost=3, plateau=True)

    def also(cen):
        i = int(a["idx"][a["marks"]["x"]])
        r = _run_of_index(cen, i)
        k = [c[0] for c in cen.cands].index(r)
        r0, r1, i0, i1 = cen.cands[k]
        assert r1 == r0 + 1 and i0 == i
        lo, hi = int(cen.runs[r0, 1]), int(cen.runs[r1, 0])
        assert hi > lo + 1 and (cen.chrom[lo + 1:hi] == -1).all()           # fillers between the two runs
        assert cen.start[hi] - cen.end[lo] == 0                             # gap == 0
        assert (cen.end[lo] >> TB) == 0 and (cen.end[hi] >> TB) == 1
        assert cand_len(cen, k) == 30 + (hi - lo - 1)
        assert len(on_stage(cen, a)) == 2
    return _case(a, also, max_gap=max_gap)


WALK_GROUPS = {"g16": (1, 15, 16, 17, 63, 64, 65), "g256": (255, 256, 257), "g1024": (1023, 1024, 1025),
               "g1280": (1279, 1280, 1281), "wave": (1, 17, 65, 1000, 1025, 5)}


def case_walk(space, group):
    """candidates of exactly these lengths in index units, each one run in a tile of its own (no fillers inside); `wave`: the first
    four share a wavefront of the short walk, a long one follows them"""
    lengths = WALK_GROUPS[group]
    st = Stage().quiet(100)
    for k, n in enumerate(lengths):
        st.to_tile()
        # (the highest pileup holds half of the significant bases: BH then gives every level a q of its own -- with a rare highest
        # level all of them share its q, and a q read from the wrong interval would be the right number)
        body = run_of(n, lens=(3, 2, 4, 1, 3), levels=(6, 5, 6, 4, 6, 3)[k % 2:] if n > 1 else (6,))
        if group == "wave" and n > 16:   # a long first interval: its product is the sum's largest term, added first (AUC_CASES)
            body[0] = (700, body[0][1])
        st.add(body, f"c{k}").quiet(50)
    a = assemble(space, st, boost=3, plateau=True)

    def also(cen):
        assert on_stage(cen, a) == list(range(len(lengths)))
        assert [cand_len(cen, k) for k in on_stage(cen, a)] == list(lengths)
        assert [c[1] - c[0] for c in cen.cands[:len(lengths)]] == [0] * len(lengths)
        for k, n in enumerate(lengths):
            assert cen.cands[k][2] == a["idx"][a["marks"][f"c{k}"]] and cen.sig[cen.cands[k][2]:cen.cands[k][3] + 1].all()
        if group == "wave":
            assert len({k // 4 for k in range(4)}) == 1 and cand_len(cen, 4) > PK_SHORT and cand_len(cen, 3) <= PK_SHORT
    return _case(a, also)


TOP = 7   # a pileup above every other of the summit cases


def case_summits(space):
    """candidate 0: the summit on its first interval, which opens the chromosome (peakStart = 0); 1 and 2 share a wavefront: 1 moves
    its summit in the step (intervals 16 .. 31) in which 2's row holds only quiet intervals inside its span; 3: the maximum twice in
    one row of 16, the later one longer; 4: the same across two steps; 5: the summit on the first interval, not at a chromosome's
    start; 6: a long candidate, the maximum twice in one step of 64, in two rows, the later one longer; 7: ... in two steps"""
    def body(n, tops):   # tops: {position: length}
        s = run_of(n, lens=(3, 2, 4), levels=(3, 4, 3, 5))
        for p, ln in tops.items():
            s[p] = (ln, TOP)
        return s
    st = Stage()
    st.add(body(5, {0: 4}), "c0").quiet(60)
    st.add(body(40, {2: 3, 20: 3}), "c1")
    st.segs[st.marks["c1"] + 20] = (3, TOP + 1)
    st.quiet(60)
    st.add(run_of(16), "c2").add([(1, 1 - i % 2) for i in range(16)]).add(run_of(4)).quiet(60)
    st.add(body(40, {3: 2, 9: 5}), "c3").quiet(60)
    st.add(body(40, {5: 2, 20: 5}), "c4").quiet(60)
    st.add(body(20, {0: 4}), "c5").quiet(60)
    st.to_tile()
    st.add(body(1100, {70: 2, 100: 5}), "c6").quiet(60)
    st.to_tile()
    st.add(body(1100, {70: 2, 200: 5}), "c7").quiet(60)
    a = assemble(space, st, pre=False, boost=3, plateau=True)
    want = {0: 0, 1: 20, 3: 9, 4: 20, 5: 0, 6: 100, 7: 200}   # candidate -> the interval (from i0) that holds the summit

    def also(cen):
        assert on_stage(cen, a) == list(range(8)) and cen.cands[0][2] == 0 and cen.start[0] == 0
        for k in range(8):
            assert cen.cands[k][2] == a["idx"][a["marks"][f"c{k}"]]
        r0, r1, i0, i1 = cen.cands[2]
        assert r1 == r0 + 1 and not cen.sig[i0 + 16:i0 + 32].any() and cen.sig[i0:i0 + 16].all() and (cen.chrom[i0:i1 + 1] >= 0).all()
        assert 1 // 4 == 2 // 4
        j0 = cen.cands[1][2]
        assert int(np.argmax(cen.pq[j0:j0 + 40])) == 20
        for k, j in want.items():
            i = cen.cands[k][2] + j
            s0 = int(cen.start[cen.cands[k][2]])
            assert replay(cen, k, cen_thr(cen, a))[1] == (int(cen.end[i]) + int(cen.start[i])) // 2 - s0, k
        for k, (p1, p2) in {3: (3, 9), 4: (5, 20), 6: (70, 100), 7: (70, 200)}.items():   # the `longer` branch: equal values, the later one longer
            i0 = cen.cands[k][2]
            seg = cen.pq[i0:cen.cands[k][3] + 1]
            assert seg[p1] == seg[p2] == seg.max() and (seg == seg.max()).sum() == 2
            assert cen.end[i0 + p2] - cen.start[i0 + p2] > cen.end[i0 + p1] - cen.start[i0 + p1]
        assert (3 // 16 == 9 // 16) and (5 // 16 != 20 // 16) and (70 // 64 == 100 // 64 and 70 // 16 != 100 // 16) and 70 // 64 != 200 // 64
        assert cand_len(cen, 6) > PK_SHORT and cand_len(cen, 7) > PK_SHORT
    return _case(a, also, max_gap=20)


def cen_thr(cen, a):
    return a["thr"]


def case_compact(space):
    """600 isolated runs; with min_len = 12: candidates 0 and 255 valid and 1 .. 254 not, all of 256 .. 511 not (a chunk of
    k_peaks with tot == 0), 512 .. 599 valid"""
    st = Stage().quiet(100)
    for k in range(600):
        long_ = k in (0, 255) or k >= 512
        st.add([(12, 3)] if long_ else [(2, 3), (1, 4)]).quiet(30)
    a = assemble(space, st)

    def also(cen):
        assert len(cen.cands) == 600
        ln = np.array([cen.end[c[3]] - cen.start[c[2]] for c in cen.cands])
        ok = ln >= 12
        assert ok[0] and ok[255] and not ok[1:255].any() and not ok[256:512].any() and ok[512:].all()
    return _case(a, also, min_len=12)


def case_skip(residue):
    """tight, -E: two runs 20 bases apart (max_gap 100 would link them) with a SKIP interval of two bases between them, on bit 63 or
    bit 0 of a word"""
    st = Stage().quiet(200).add(run_of(3), "a").quiet(20).add(run_of(3), "b").quiet(100).add(run_of(2), "c").quiet(30).add(run_of(2)).quiet(60)
    a = assemble("tight", st, target=("skip", WORD, residue), bed=("a", 3, 9, 2))

    def also(cen):
        i = int(a["idx"][a["marks"]["skip"]])
        assert i % WORD == residue and cen.skip[i] and cen.skip.sum() == 1
        ra, rb = _run_of_index(cen, i - 2), _run_of_index(cen, i + 2)
        assert rb == ra + 1 and cen.start[cen.runs[rb, 0]] - cen.end[cen.runs[ra, 1]] == 20
        firsts = [c[0] for c in cen.cands]
        assert ra in firsts and rb in firsts                  # split by the SKIP alone ...
        rc = _run_of_index(cen, int(a["idx"][a["marks"]["c"]]))
        assert rc + 1 not in firsts                           # ... while the two runs 30 apart behind them are linked
        assert int(cen.words["skip"][i // WORD]) >> (i % WORD) & 1
    return _case(a, also, max_gap=100)


def case_control():
    """tight (a control run sweeps the merged table): the thread-border run, with a control sample that is quiet wherever the
    treatment is (its fragments are the treatment's quiet ones)"""
    a = case_run_border("tight", THREAD, 0)
    ev = a["ev"]
    quiet = ev[ev["chrom"] != a["stage"]]
    assert len(quiet) > 10
    a["case"] = dict(a["case"], replicates=[dict(save=None, treat=ev, ctrl=quiet.copy())])
    return a


# name -> (builder, arguments, the paths it runs on).  A case runs where its limit is: in the space it was built for, on the paths
# whose kernels see it -- the run cases on both run passes of the loose slots (the overlapped launch's and k_runs<true>) and on
# k_runs<false>; the walks also with q from memory (eager), from the candidates' fill (lazy: k_q_fill_cands) and from the table by
# pileup (Q_LOOSE); the chunk borders also with one and two persistent workgroups.
L_RUN = ("loose-p", "loose-p-no-overlap")
GRIDS = ("loose-p-grid1", "loose-p-grid2")
CASES = {}
for _sp, _paths in (("loose", L_RUN), ("tight", ("tight-p",))):
    CASES[f"{_sp}:run-ends-bit63"] = (case_run_ends_bit63, (_sp,), _paths)
    CASES[f"{_sp}:run-across-word"] = (case_run_border, (_sp, WORD, 0), _paths)
    CASES[f"{_sp}:run-across-thread"] = (case_run_border, (_sp, THREAD, 0), _paths)
    CASES[f"{_sp}:run-across-chunk"] = (case_run_border, (_sp, CHUNK, CHUNK, True), _paths + (GRIDS if _sp == "loose" else ("tight-p-grid1",)))
    CASES[f"{_sp}:chrom-start-word"] = (case_chrom_start, (_sp, WORD), _paths)
    CASES[f"{_sp}:chrom-start-chunk"] = (case_chrom_start, (_sp, CHUNK, True), _paths + (GRIDS if _sp == "loose" else ("tight-p-grid1",)))
    CASES[f"{_sp}:index0"] = (case_index0, (_sp,), _paths)
    _one = _paths[:1]
    CASES[f"{_sp}:cand-link"] = (case_cand_border, (_sp, False), _one + (("loose-p-grid1",) if _sp == "loose" else ("tight-p-grid1",)))
    CASES[f"{_sp}:cand-cut"] = (case_cand_border, (_sp, True), _one)
    CASES[f"{_sp}:runs-256"] = (case_exact_runs, (_sp, 256), _one)
    CASES[f"{_sp}:runs-257"] = (case_exact_runs, (_sp, 257), _one)
    CASES[f"{_sp}:compact"] = (case_compact, (_sp,), _one)
    CASES[f"{_sp}:summits"] = (case_summits, (_sp,), _one + (("loose-q",) if _sp == "loose" else ("tight-q-eager",)))
    for _g in WALK_GROUPS:
        _q = ("loose-q",) if _sp == "loose" else ("tight-q-eager", "tight-q-lazy")
        CASES[f"{_sp}:walk-{_g}"] = (case_walk, (_sp, _g), _one + (_q if _g in ("g16", "g256", "wave") else ()))
CASES["loose:many-runs"] = (case_many_runs, ("loose",), ("loose-p",) + GRIDS)
CASES["tight:many-runs"] = (case_many_runs, ("tight",), ("tight-p", "tight-p-grid1"))
CASES["tight:zero-peaks"] = (case_exact_runs, ("tight", 256), ("tight-p",))
CASES["loose:zero-peaks"] = (case_exact_runs, ("loose", 256), ("loose-p",))
CASES["tight:last-word-single"] = (case_table_end, (1,), ("tight-p", "tight-q-lazy"))
CASES["tight:table-64k"] = (case_table_end, (0,), ("tight-p", "tight-q-lazy"))
CASES["loose:many-chroms"] = (case_many_chroms, (), L_RUN)
CASES["loose:plateau-tile-border"] = (case_plateau_tile_border, (), ("loose-p", "loose-q"))
CASES["loose:plateau-negative-gap"] = (case_plateau_tile_border, (-1,), ("loose-p",))
CASES["tight:skip-bit63"] = (case_skip, (WORD - 1,), ("bed",))
CASES["tight:skip-bit0"] = (case_skip, (0,), ("bed",))
CASES["tight:control"] = (case_control, (), ("ctrl",))
ZERO_PEAKS = dict(min_len=1_000_000)
AUC_CASES = [(f"{sp}:walk-wave", k) for sp in ("tight", "loose") for k in (2, 4)]   # a short candidate of 65 intervals, a long one of 1025


@functools.lru_cache(maxsize=None)
def built(name):
    fn, args, _ = CASES[name]
    a = fn(*args)
    if name.endswith("zero-peaks"):
        a["par"] = {**a["par"], **ZERO_PEAKS}
    return a


def q_threshold(a):
    """-q: a threshold between the q-values of the stage's quiet intervals and of its significant ones (q does not depend on it)"""
    par = B.make_params(**{**a["par"], "qval": True, "pq": 0.5})
    o = B.Oracle(par)
    B.run_case(o, a["case"])
    q = o.get_intervals(-1, a["stage"])[1]["q"]
    o.close()
    lv = a["levels"]
    lo, hi = float(q[(lv >= 0) & (lv <= QUIET)].max()), float(q[lv >= SIG].min())
    assert lo < hi, ("q does not separate the levels", lo, hi)
    return T.f32((lo + hi) / 2)


@functools.lru_cache(maxsize=None)
def reference(name, qval=False, **over):
    """(case, params, oracle, its scalars, census): computed once, shared by the oracle-only tests and the GPU tests, left unchanged"""
    a = built(name)
    par = B.make_params(**{**a["par"], **dict(over)})
    if qval:
        par = T.params(par, qval_opt=1, thr=q_threshold(a))
    o = B.Oracle(par)
    so = B.run_case(o, a["case"])
    cen = sweep_census(o, a["case"], a["space"], par)
    return a, par, o, so, cen


def check(name, qval=False):
    """the census of a case against what it was built for"""
    a, par, o, so, cen = reference(name, qval)
    assert cen.N == a["N"]
    idx, lv = a["idx"], a["levels"]
    assert (cen.chrom[idx] == a["stage"]).all()
    assert ((cen.sig[idx]) == (lv >= SIG)).all(), "the stage's significant intervals are not the designed ones"
    assert ((cen.skip[idx]) == (lv < 0)).all()
    if qval:   # every significant level a q of its own: a q taken from the wrong interval is then another number
        assert len({float(x) for x in cen.pq[idx][lv >= SIG]}) == len(set(lv[lv >= SIG].tolist())), "levels share a q"
    on_stage = cen.chrom[cen.runs[:, 0]] == a["stage"] if len(cen.runs) else np.zeros(0, dtype=bool)
    assert on_stage.sum() >= len(cen.runs) - 2          # (but the closing interval of the chromosome before the stage, and the plateau)
    a["also"](cen)
    if par.min_auc == 0.0 and par.min_len == 0:       # every candidate a peak: the float AUC in interval order, and the summit
        pk = o.get_peaks()
        for k in list(range(min(len(cen.cands), 40))) + list(range(max(0, len(cen.cands) - 8), len(cen.cands))):
            auc, pos = replay(cen, k, par.thr)
            assert auc.tobytes() == pk["auc"][k].tobytes() and pos == int(pk["summit"][k]), (name, k, auc, pk["auc"][k], pos, pk["summit"][k])
            assert seq_sum(cen.terms[k]).tobytes() == auc.tobytes()
    return cen
