"""Threshold ties: runs in which some value of the data is EXACTLY the threshold it is compared with.

callPeaks (Genrich.c:977-1069) decides with four comparisons, each with a direction:
  significance  pqval > minPQval (1015)             -- an interval with p (q) == thr is NOT significant
  end of a peak end[m] - peakEnd > maxGap (1032)     -- a gap == maxGap still links two runs
  AUC           auc >= minAUC (920)                   -- a peak with auc == minAUC is kept
  length        end - start >= minLen (921)           -- a peak with length == minLen is kept
Round thresholds never meet the data exactly, so a kernel with the wrong direction passes every other test.  The finders
here run the CPU oracle once, read a boundary value out of its result and return it with its neighbours (one float, or one
base, away).  Every tie is checked to be LIVE: the oracle's peaks (coordinates and summits) at the tie differ from the ones
one step away -- so a comparison that flips direction changes the result.

Only the oracle and the host build of the library's p-value routine (selftest_host, no GPU) are used: CPU only.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

import backends as B

GX_SKIP = np.float32(-1.0)   # GX_SKIPF / SKIP (Genrich.h): the value of an interval inside a -E region
GX_RISK_B = 2.0 ** -38       # gx_math.h


def f32(x) -> float:
    return float(np.float32(x))


def up(x) -> float:
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def down(x) -> float:
    return float(np.nextafter(np.float32(x), np.float32(-np.inf)))


def params(base: B.GxParams, **kw) -> B.GxParams:
    """A copy of `base` with some fields replaced (thr is set as a float directly, not through -log10f)."""
    d = {f: getattr(base, f) for f, _ in B.GxParams._fields_}
    d.update(kw)
    return B.GxParams(**d)


@dataclass
class Run:
    peaks: np.ndarray
    ends: list          # per chromosome: interval ends
    cols: list          # per chromosome: {"expt", "ctrl", "p", "q"}
    scal: list          # run_case's per-replicate (fragLen, lambda, factor)

    def key(self):
        """What a tie decides: which peaks there are and where their summits lie."""
        return [tuple(int(v) for v in r) for r in self.peaks[["chrom", "start", "end", "summit"]].tolist()]


def run_oracle(case, par) -> Run:
    o = B.Oracle(par)
    try:
        scal = B.run_case(o, case)
        ends, cols = [], []
        for c in range(len(case["lens"])):
            e, cl = o.get_intervals(-1, c)
            ends.append(e)
            cols.append(cl)
        return Run(o.get_peaks(), ends, cols, scal)
    finally:
        o.close()


@dataclass
class Tie:
    """One boundary: `param` set to `at` (the tie) and to `away` (one float / one base past it, on the side where the
    comparison flips).  runs[value] are the oracle's runs at each value tried."""
    kind: str
    param: str
    at: float
    away: float
    base: B.GxParams
    runs: dict = field(default_factory=dict)
    note: str = ""
    where: tuple = ()   # gap ties: (chrom, end of the first run, start of the second)
    tried: int = 0      # risky ties: how many genome lengths the search tried
    V: float = 0.0      # risky ties: the whole pileup whose p-value is the threshold

    def at_params(self):
        return params(self.base, **{self.param: self.at})

    def away_params(self):
        return params(self.base, **{self.param: self.away})

    def values(self):
        """the tie and its neighbours on both sides"""
        if self.param in ("thr", "min_auc"):
            return [down(self.at), self.at, up(self.at)]
        return [self.at - 1, self.at, self.at + 1]

    def live(self):
        return self.runs[self.at].key() != self.runs[self.away].key()


def _tie(case, kind, param, at, away, base, note=""):
    t = Tie(kind, param, at, away, base, note=note)
    for v in t.values():
        t.runs[v] = run_oracle(case, params(base, **{param: v}))
    if away not in t.runs:
        t.runs[away] = run_oracle(case, params(base, **{param: away}))
    return t


def _in_peaks(run, c):
    """mask of chromosome c's intervals that lie inside one of the run's peaks"""
    e = run.ends[c].astype(np.int64)
    s = np.concatenate([[0], e[:-1]])
    pk = run.peaks[run.peaks["chrom"] == c]
    m = np.zeros(len(e), dtype=bool)
    for p in pk:
        m |= (s >= int(p["start"])) & (e <= int(p["end"]))
    return m, e - s


def pq_ties(case, base, n_common=1, n_summit=1, max_tries=40):
    """p (or q, with base.qval_opt) ties: a float present in the run's final p (q) column inside a candidate peak, used as
    the threshold.  Kinds: `common` (the value with most bases inside the peaks) and `summit` (a peak's summit value, with
    min_auc 0).
    `away` = one float below: there the intervals with value == tie become significant."""
    col = "q" if base.qval_opt else "p"
    r0 = run_oracle(case, params(base, min_auc=0.0, min_len=0))
    assert len(r0.peaks), "the case must have candidate peaks"
    bp = {}
    for c in range(len(case["lens"])):
        m, ln = _in_peaks(r0, c)
        for v, l in zip(r0.cols[c][col][m], ln[m]):
            if v != GX_SKIP:
                bp[float(v)] = bp.get(float(v), 0) + int(l)
    common = [v for v, _ in sorted(bp.items(), key=lambda kv: -kv[1])]
    summits = sorted({float(v) for v in r0.peaks[col]}, key=lambda v: -bp.get(v, 0))
    out = []
    for kind, cands, want in (("common", common, n_common), ("summit", summits, n_summit)):
        got = 0
        for v in cands[:max_tries]:
            if got == want:
                break
            if any(t.at == v for t in out):
                continue
            # (a summit value is its peak's maximum: one float below it only the intervals holding it are significant, with an
            # AUC of a few ulps -- min_auc 0 keeps that peak)
            b = params(base, min_auc=0.0) if kind == "summit" else base
            t = _tie(case, f"{col}_{kind}", "thr", v, down(v), b, note=f"{bp.get(v, 0)} bp at {col} = {v!r}")
            if t.live():
                out.append(t)
                got += 1
        assert got == want, f"no live {col} tie of kind {kind} among {min(len(cands), max_tries)} candidates"
    return out


def auc_tie(case, base, pick="median"):
    """min_auc = a peak's exact AUC (kept: auc >= minAUC) and one float above (dropped); pick "max": the largest AUC."""
    r0 = run_oracle(case, params(base, min_auc=0.0))
    auc = np.sort(np.unique(r0.peaks["auc"]))
    assert len(auc) > 2
    a = float(auc[-1] if pick == "max" else auc[len(auc) // 2])
    t = _tie(case, "auc", "min_auc", a, up(a), base)
    assert t.live()
    return t, r0


def len_tie(case, base):
    """min_len = a peak's exact length (kept) and that + 1 (dropped)."""
    r0 = run_oracle(case, params(base, min_len=0))
    ln = np.sort(np.unique(r0.peaks["end"].astype(np.int64) - r0.peaks["start"]))
    assert len(ln) > 2
    L = int(ln[len(ln) // 2])
    t = _tie(case, "len", "min_len", L, L + 1, base)
    assert t.live()
    return t, r0


def sig_runs(run, c, par):
    """(first, last) interval index of each run of significant intervals on chromosome c, and the SKIP mask"""
    v = run.cols[c]["q" if par.qval_opt else "p"]
    sig = v > np.float32(par.thr)
    d = np.diff(np.concatenate([[0], sig.astype(np.int8), [0]]))
    return list(zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1) - 1)), v == GX_SKIP


def run_gaps(run, par, lo=1, hi=10_000):
    """[(chrom, gap, end of the first run, start of the second)] for consecutive significant runs with no SKIP between"""
    out = []
    for c in range(len(run.ends)):
        runs, skip = sig_runs(run, c, par)
        e = run.ends[c].astype(np.int64)
        for (a0, a1), (b0, b1) in zip(runs[:-1], runs[1:]):
            if skip[a1 + 1:b0].any():
                continue
            g = int(e[b0 - 1] - e[a1])
            if lo <= g <= hi:
                out.append((c, g, int(e[a1]), int(e[b0 - 1])))
    return out


def linked(run, c, a_end, b_start):
    """do the two runs lie in one peak?  (with min_auc = min_len = 0 every candidate is a peak)"""
    pk = run.peaks[run.peaks["chrom"] == c]
    return bool(((pk["start"] < a_end) & (pk["end"] > b_start)).any())


def gap_tie(case, base, lo=2, hi=2_000, raise_thr=True):
    """max_gap = the distance between two significant runs (linked: the gap is not > maxGap) and that - 1 (split).
    raise_thr: when no such pair is found at the given threshold (strong peaks are one run each), raise it to quantiles
    of the values inside the peaks until the runs break up."""
    b0 = params(base, min_auc=0.0, min_len=0)
    r0 = run_oracle(case, params(b0, max_gap=0))
    col = "q" if base.qval_opt else "p"
    thrs = [b0.thr]
    if raise_thr and len(r0.peaks):
        inside = np.concatenate([r0.cols[c][col][_in_peaks(r0, c)[0]] for c in range(len(r0.ends))])
        thrs += [float(np.float32(np.quantile(inside, qt))) for qt in (0.3, 0.5, 0.7, 0.85)]
    for thr in thrs:
        b1 = params(b0, thr=thr)
        r1 = run_oracle(case, params(b1, max_gap=0))
        gaps = sorted(run_gaps(r1, b1, lo, hi), key=lambda x: -x[1])
        for c, g, a_end, b_start in gaps[:: max(1, len(gaps) // 12)]:
            t = _tie(case, "gap", "max_gap", g, g - 1, b1, note=f"chrom {c}: [.., {a_end}) .. [{b_start}, ..)")
            if t.live() and linked(t.runs[g], c, a_end, b_start) and not linked(t.runs[g - 1], c, a_end, b_start):
                t.where = (c, a_end, b_start)
                return t
    raise AssertionError("no live gap tie")


def bed_gap_case(case, base, tie):
    """The gap tie's two runs with a one-base -E region in the middle of the gap between them: at max_gap >= gap they must
    split all the same (pqval == SKIP ends a peak, 1031).  Returns (case with the region, its runs at max_gap = gap and
    gap + 100)."""
    c, a_end, b_start = tie.where
    mid = (a_end + b_start) // 2
    beds = [list(b) for b in case.get("beds") or [[] for _ in case["lens"]]]
    assert not beds[c]
    beds[c] = [mid, mid + 1]
    bc = dict(case, beds=beds)
    g = int(tie.at)
    runs = {mg: run_oracle(bc, params(tie.base, max_gap=mg)) for mg in (g, g + 100)}
    return bc, runs


# ---- a p-value next to a float rounding boundary, at the threshold ------------------------------------------------

def _round_checked_np(d, margin):
    """gx_math.h round_checked on doubles (vectorised): True where the distance to the nearest float rounding boundary is
    below margin * GX_RISK_B of the value"""
    f = d.astype(np.float32)
    a = np.abs(d)
    fd = np.abs(f.astype(np.float64))
    err = np.abs(a - fd)
    b = np.abs(f).view(np.uint32)
    nb_up = (b + np.uint32(1)).view(np.float32).astype(np.float64)
    nb_dn = np.where(b > 0, (b - np.uint32(1)).view(np.float32).astype(np.float64), -1.401298464324817e-45)
    nb = np.where(a >= fd, nb_up, nb_dn)
    half = 0.5 * np.abs(nb - fd)
    return half - err < a * GX_RISK_B * margin


def risky_tie(case, base, l0=None, n_max=4000, margin=0.5):
    """No control, -p: search genome_len (-L; lambda = fragLen / genomeLen) until some whole pileup V present inside the
    candidate peaks has a host double p(V, lambda) within margin * GX_RISK_B * |p| of a float rounding midpoint (the device
    flags such an entry -- its double is < 0.2 RISK_B from the host's, gx_math.h -- and the host re-evaluates it after the
    tile stage has used the device's float: riskNearThr).  Then thr = that entry's float; the tie must be live.
    Returns (Tie, number of -L values tried)."""
    from genrich_amd.lib import selftest_host
    assert not base.qval_opt and all(r["ctrl"] is None for r in case["replicates"]) and len(case["replicates"]) == 1
    r0 = run_oracle(case, params(base, min_auc=0.0, min_len=0))
    frag = r0.scal[0][0]
    vs = set()
    for c in range(len(case["lens"])):
        m, _ = _in_peaks(r0, c)
        ex = r0.cols[c]["expt"][m]
        vs.update(float(v) for v in ex if v == np.floor(v) and 0 < v < 2000)
    vs = np.array(sorted(vs), dtype=np.float32)
    assert len(vs) > 10
    g0 = l0 or sum(case["lens"])
    tried = 0
    for k in range(n_max):
        L = g0 + 7 * k
        tried += 1
        lam = np.float32(frag / float(L))
        p, d = selftest_host(1, vs, np.full(len(vs), lam, dtype=np.float32))
        hit = np.flatnonzero(_round_checked_np(d, margin) & (p > 0))
        for i in hit:
            t = float(p[i])
            tie = _tie(case, "risky", "thr", t, down(t), params(base, genome_len=L),
                       note=f"-L {L}: lambda {float(lam)!r}, V = {float(vs[i])}, p double {float(d[i])!r}")
            if tie.live():
                tie.tried = tried
                tie.V = float(vs[i])
                return tie, tried
    raise AssertionError(f"no live risky p-value at the threshold within {n_max} genome lengths")


# ---- the threshold string of the command line (golden fixtures) ----------------------------------------------------

_libc = C.CDLL(None)
_libc.strtof.restype = C.c_float
_libc.strtof.argtypes = [C.c_char_p, C.c_void_p]


def strtof(s: str) -> float:
    return float(_libc.strtof(s.encode(), None))


def pq_string(t: float, span=256):
    """A decimal -p / -q argument s with -log10f(strtof(s)) == t exactly (getArgs, Genrich.c:5817), or None.  Searched over
    the floats around 10^-t; `%.9g` round-trips a float.  The Python route of the tests (float(s) rounded to a float) must
    land on the same float."""
    b0 = int(np.float32(10.0 ** -t).view(np.int32))
    for k in range(span):
        for sgn in (1, -1):
            x = np.array([b0 + sgn * k], dtype=np.int32).view(np.float32)[0]
            if B.minus_log10f(float(x)) == t:
                s = "%.9g" % float(x)
                if strtof(s) == float(x) and f32(float(s)) == float(x) and B.minus_log10f(float(s)) == t:
                    return s
    return None


# ---- the cases -------------------------------------------------------------------------------------------------------

def case_noctrl(seed=7, n=80_000, lens=(400_000, 90_000)):
    import synth
    lens = list(lens)
    ev = synth.make_fragments(lens, n, seed, peak_every=20_000, tower_every=150_000)
    return dict(lens=lens, replicates=[dict(save=None, treat=ev, ctrl=None)])


def case_ctrl(seed=21, lens=(300_000, 70_001)):
    import synth
    lens = list(lens)
    t = synth.make_fragments(lens, 70_000, seed, peak_every=20_000, tower_every=150_000)
    c = synth.make_fragments(lens, 50_000, seed + 1, uniform_only=True)
    return dict(lens=lens, replicates=[dict(save=None, treat=t, ctrl=c)])


# ---- summits: plateaus of equal value (updatePeak 958-966) ------------------------------------------------------------

def _stack(n, s, e):
    ev = np.zeros(n, dtype=B.EVENT_DTYPE)
    ev["start"], ev["end"], ev["count"] = s, e, 1
    return ev


SUMMIT_LEN = 60_000
N_BASE = 60
# (kind, base layer, plateau A, plateau B): A and B of one height on a base layer of N_BASE fragments
SUMMIT_PEAKS = [
    ("equal", (9_600, 10_800), (9_800, 10_000), (10_300, 10_500)),     # equal length: A stays the summit
    ("longer", (29_600, 30_900), (29_800, 30_000), (30_300, 30_550)),  # B longer: summitPos moves to B
]


def summit_events(n_plateau=60, q_pair=None, seed=3):
    """One chromosome: a light uniform background away from the peaks, and two peaks built from stacked identical fragments,
    each with two plateaus at its maximum (SUMMIT_PEAKS).  q_pair = (nA, nB): a third peak at 48,000 whose plateaus have
    different heights (so different p) -- summit_q_pair() picks them so that BH gives both the same q."""
    import synth
    L = [SUMMIT_LEN]
    bg = synth.make_fragments(L, 1_500, seed, uniform_only=True)
    keep = np.ones(len(bg), dtype=bool)
    for lo, hi in ((9_000, 11_400), (29_000, 31_500), (47_000, 50_000)):
        keep &= (bg["end"] <= lo) | (bg["start"] >= hi)
    parts = [bg[keep]]
    for _, base, a, b in SUMMIT_PEAKS:
        parts += [_stack(N_BASE, *base), _stack(n_plateau, *a), _stack(n_plateau, *b)]
    if q_pair:
        parts += [_stack(N_BASE, 47_600, 49_000), _stack(q_pair[0], 47_800, 48_000), _stack(q_pair[1], 48_050, 48_350)]
    return np.concatenate(parts)


def summit_case(q_pair=None):
    return dict(lens=[SUMMIT_LEN], replicates=[dict(save=None, treat=summit_events(q_pair=q_pair), ctrl=None)])


def summit_q_pair(pq=0.05, min_auc=20.0):
    """(nA, nB) with nA != nB such that the third peak's plateaus have different p but the same q, and that q is the peak's
    maximum: updatePeak then moves summitPos to the later, longer plateau B and keeps the FIRST plateau's p (958-966)."""
    par = B.make_params(pq=pq, qval=True, min_auc=min_auc)
    for na in range(300, 500, 10):
        for nb in (na + 1, na - 1, na + 2, na - 2):
            run = run_oracle(summit_case((na, nb)), par)
            e = run.ends[0].astype(np.int64)
            ia, ib = np.searchsorted(e, 48_000), np.searchsorted(e, 48_350)
            p, q = run.cols[0]["p"], run.cols[0]["q"]
            if p[ia] != p[ib] and q[ia] == q[ib] and q[ia] == q[max(0, ia - 5):ib + 5].max() and q[ia] > np.float32(par.thr):
                return na, nb
    raise AssertionError("no plateau heights with equal q and different p")
