"""Plain Python / numpy restatement of the motif definitions of include/genrich_amd.h (gx_set_genome_bases .. gx_format_motif_summary):
the sequence as codes, the scores of a count matrix, the threshold of a p-value by a dynamic program in Python integers and by
enumerating all 4^L L-mers, the scan of regions and of the genome, the two tables.  Everything is an exact integer except the
logarithm of the scores, the achieved p and the enrichment, which are computed by the same steps as the library's."""
import math
from fractions import Fraction

import numpy as np

SCALE = 128
MAX_WIDTH = 32
_CODE = np.full(256, -1, dtype=np.int8)
for _k, _ch in enumerate(b"ACGT"):
    _CODE[_ch] = _CODE[_ch | 0x20] = _k


def codes(seq, length):
    """int8[length]: 0 A, 1 C, 2 G, 3 T, -1 unknown (anything else, and everything never pushed)."""
    out = np.full(length, -1, dtype=np.int8)
    if seq is not None:
        out[:len(seq)] = _CODE[np.frombuffer(seq, dtype=np.uint8)]
    return out


def genome(seqs, lens):
    return [codes(s, n) for s, n in zip(seqs, lens)]


def letters(code, start, n):
    """What gx_get_sequence gives: upper-case ACGT, N for unknown and past the end."""
    out = np.full(n, ord("N"), dtype=np.uint8)
    part = code[start:start + n] if start < len(code) else code[:0]
    out[:len(part)] = np.frombuffer(b"ACGTN", dtype=np.uint8)[part]
    return out.tobytes()


MAX_MOTIFS = 4096


def read_jaspar(data):
    """[(id, name, counts[4][L])] of a JASPAR file in either form -- `>ID NAME` then four rows `A [ n n ... ]` .. `T [ ... ]`, or
    four bare rows in the order A C G T; any whitespace, CRLF, blank lines, no final newline.  ValueError("<id>: <reason>")."""
    out, seen = [], set()
    cur = None

    def close():
        if cur is None:
            return
        mid, name, rows = cur
        if len(rows) != 4:
            raise ValueError("%s: fewer than four rows" % mid)
        if len({len(r) for r in rows}) != 1:
            raise ValueError("%s: rows of unequal length" % mid)
        if not 1 <= len(rows[0]) <= MAX_WIDTH:
            raise ValueError("%s: the width must be 1 to 32" % mid)
        out.append((mid, name, rows))

    for raw in data.decode("latin-1").replace("\r", "").split("\n"):
        line = raw.strip()
        if not line:
            continue
        if line.startswith(">"):
            close()
            parts = line[1:].split(None, 1)
            if not parts:
                raise ValueError("?: a header without an ID")
            mid = parts[0]
            if mid in seen:
                raise ValueError("%s: a repeated ID" % mid)
            seen.add(mid)
            if len(seen) > MAX_MOTIFS:
                raise ValueError("%s: more than 4096 motifs" % mid)
            cur = (mid, parts[1].strip() if len(parts) > 1 else mid, [])
            continue
        if cur is None:
            raise ValueError("?: a row before the first header")
        mid, name, rows = cur
        if len(rows) == 4:
            raise ValueError("%s: more than four rows" % mid)
        body = line
        if body[0] in "ACGTacgt" and not body[0].isdigit():
            if body[0].upper() != "ACGT"[len(rows)]:
                raise ValueError("%s: rows out of the order A C G T" % mid)
            body = body[1:]
        toks = body.replace("[", " ").replace("]", " ").split()
        vals = []
        for t in toks:
            if not t.isdigit() or int(t) >= 1 << 31:
                raise ValueError("%s: a count that is not an integer from 0 to 2^31 - 1" % mid)
            vals.append(int(t))
        rows.append(vals)
    close()
    if not out:
        raise ValueError("no motif in the file")
    return out


def _round_half_away(v):
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def pssm(counts, pc=1.0):
    """scores[L][4] (A C G T) of counts[4][L]; ValueError where the library refuses."""
    L = len(counts[0])
    if not 1 <= L <= MAX_WIDTH:
        raise ValueError("width")
    if not (pc >= 0 and math.isfinite(pc)):
        raise ValueError("pseudocount")
    out = []
    for j in range(L):
        col = [int(counts[b][j]) for b in range(4)]
        if any(c < 0 or c >= 1 << 31 for c in col):
            raise ValueError("count")
        N = sum(col)
        row = []
        for c in col:
            num, den = float(c) + 0.25 * pc, float(N) + pc
            if not (den > 0 and num > 0):
                raise ValueError("minus infinity")
            s = _round_half_away(128.0 * math.log2((num / den) / 0.25))
            if not -32768 <= s <= 32767:
                raise ValueError("int16")
            row.append(s)
        out.append(row)
    return out


def score_range(scores):
    return sum(min(r) for r in scores), sum(max(r) for r in scores)


def _pick(n_ge_of, smin, smax, K):
    """The least integer t in [smin, smax + 1] with n_ge(t) <= K."""
    t = smax + 1
    for s in range(smax, smin - 1, -1):
        if n_ge_of(s) > K:
            break
        t = s
    return t


def n_ge(scores, t):
    """The L-mers whose score is >= t, by the dynamic program."""
    dist = {0: 1}
    for row in scores:
        nxt = {}
        for s, c in dist.items():
            for v in row:
                nxt[s + int(v)] = nxt.get(s + int(v), 0) + c
        dist = nxt
    return sum(c for s, c in dist.items() if s >= t)


def threshold(scores, p):
    """(t, smin, smax, n_ge(t), unreachable) by the dynamic program over the columns, in Python integers."""
    L = len(scores)
    K = int(Fraction(p) * 4 ** L)          # floor: p is a double, the product is exact
    dist = {0: 1}
    for row in scores:
        nxt = {}
        for s, c in dist.items():
            for v in row:
                nxt[s + int(v)] = nxt.get(s + int(v), 0) + c
        dist = nxt
    assert sum(dist.values()) == 4 ** L
    smin, smax = min(dist), max(dist)
    cum, acc = {}, 0
    for s in range(smax, smin - 1, -1):
        acc += dist.get(s, 0)
        cum[s] = acc
    t = _pick(lambda s: cum[s], smin, smax, K)
    return t, smin, smax, cum.get(t, 0), t > smax


def threshold_enumerated(scores, p):
    """The same by scoring every one of the 4^L L-mers (L <= 8)."""
    L = len(scores)
    assert L <= 8
    K = int(Fraction(p) * 4 ** L)
    tot = np.zeros(1, dtype=np.int64)
    for row in scores:
        tot = (tot[:, None] + np.asarray(row, dtype=np.int64)[None, :]).reshape(-1)
    assert tot.size == 4 ** L
    smin, smax = int(tot.min()), int(tot.max())
    t = _pick(lambda s: int((tot >= s).sum()), smin, smax, K)
    return t, smin, smax, int((tot >= t).sum()), t > smax


def p_achieved(n_ge, L):
    return math.ldexp(float(n_ge), -2 * L)


def scan(gen, regions, motifs, active=None):
    """(hits, counts): hits = sorted [(region, pos, score, motif, strand)], counts = [windows[m], hits_fwd[m], hits_rev[m]] of
    motifs = [(scores[L][4], t)] in regions = [(chrom, start, end)] of the genome `gen` (codes per chromosome); active[c] = 0: the
    chromosome has no words here (skipped, not owned) and scans nothing."""
    nM = len(motifs)
    counts = [[0] * nM for _ in range(3)]
    hits = []
    for r, (c, start, end) in enumerate(regions):
        if c >= len(gen) or (active is not None and not active[c]):
            continue
        e = min(end, len(gen[c]))
        if start >= e:
            continue
        code = gen[c][start:e].astype(np.int64)
        bad = np.concatenate([[0], np.cumsum(code < 0)])
        safe = np.where(code < 0, 0, code)
        for m, (scores, t) in enumerate(motifs):
            S = np.asarray(scores, dtype=np.int64)
            L = len(S)
            n = len(code) - L + 1
            if n <= 0:
                continue
            ok = (bad[L:L + n] - bad[:n]) == 0
            f, v = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
            for j in range(L):
                f += S[j][safe[j:j + n]]
                v += S[j][3 - safe[L - 1 - j:L - 1 - j + n]]
            counts[0][m] += int(ok.sum())
            for strand, sc in ((0, f), (1, v)):
                at = np.nonzero(ok & (sc >= t))[0]
                counts[1 + strand][m] += len(at)
                hits += [(r, int(x), int(sc[x]), m, strand) for x in at]
    hits.sort(key=lambda h: (h[0], h[1], h[3], h[4]))
    return hits, counts


def scan_genome(gen, motifs, active=None):
    """The counts over whole chromosomes (the genome pass)."""
    return scan(gen, [(c, 0, len(g)) for c, g in enumerate(gen)], motifs, active)[1]


def add_counts(a, b):
    return [[x + y for x, y in zip(ra, rb)] for ra, rb in zip(a, b)]


def hit_tuples(hits):
    """A MOTIF_HIT_DTYPE array as the tuples of scan()."""
    return [(int(h["region"]), int(h["pos"]), int(h["score"]), int(h["motif"]), int(h["strand"])) for h in hits]


def count_lists(cnt):
    return [[int(x) for x in row] for row in cnt]


def _p_text(p):
    return "NA" if p is None or (isinstance(p, float) and math.isnan(p)) else "%.3e" % p


def hits_text(names, peaks, summit_off, motifs, ids, mnames, pthr, hits):
    out = ["chr\tstart\tend\tmotif\tscore\tstrand\tname\tpeak\toffset_from_summit\tp_threshold\n"]
    for r, pos, score, m, strand in hits:
        c, start, end = peaks[r]
        L = len(motifs[m][0])
        at = start + pos
        out.append("%s\t%d\t%d\t%s\t%.4f\t%s\t%s\tpeak_%d\t%d\t%s\n" % (names[c], at, at + L, ids[m], score / 128.0, "-" if strand else "+", mnames[m], r,
                                                                         (2 * at + L) // 2 - (start + summit_off[r]), _p_text(pthr[m])))
    return "".join(out)


def _to_double(x):
    """The library's conversion of an exact product: the leading 64 bits, rounded once, scaled."""
    if x == 0:
        return 0.0
    sh = max(x.bit_length() - 64, 0)
    return math.ldexp(float(x >> sh), sh)


def summary_text(peaks, motifs, ids, mnames, pthr, hits, cp, cg):
    out = ["motif\tname\twidth\tthreshold\tp_threshold\tpeaks_scanned\tpeaks_with_hit\twindows_peaks\thits_peaks\twindows_genome\thits_genome\tenrichment\n"]
    for m, (scores, t) in enumerate(motifs):
        L = len(scores)
        scanned = sum(1 for c, s, e in peaks if e > s and e - s >= L)
        with_hit = len({h[0] for h in hits if h[3] == m})
        hp, hg, wp, wg = cp[1][m] + cp[2][m], cg[1][m] + cg[2][m], cp[0][m], cg[0][m]
        enr = "NA" if hg == 0 or wp == 0 else "%.6f" % (_to_double(hp * wg) / _to_double(hg * wp))
        out.append("%s\t%s\t%d\t%.4f\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % (ids[m], mnames[m], L, t / 128.0, _p_text(pthr[m]), scanned, with_hit, wp, hp, wg, hg, enr))
    return "".join(out)


# ---- the launch geometry (gx_motif_grid) -------------------------------------------------------------------------------------

WAVES, FLUSH_RUNS, GRID, MAX_GRID, MAX_STEP = 4, 1 << 25, 2048, 65535, 16


def runs_of_a_workgroup(units, step, grid):
    """The most runs of 64 positions one workgroup of `grid` walks per batch: its WAVES wavefronts take a unit of `step` runs each
    per round, rounds blockIdx, + grid, ..., and all add to the same 32-bit counters."""
    rounds = -(-units // WAVES)
    return -(-rounds // grid) * WAVES * step


def grid_of(units, step=4, grid=0):
    """What gx_motif_grid answers: the workgroups, or None when it refuses."""
    if not 1 <= step <= MAX_STEP or grid > MAX_GRID or units >= 1 << 32:
        return None
    if grid:
        return grid if runs_of_a_workgroup(units, step, grid) <= FLUSH_RUNS else None
    need = 1
    while runs_of_a_workgroup(units, step, need) > FLUSH_RUNS:
        need += 1
    return max(need, min(-(-units // WAVES), GRID), 1)
