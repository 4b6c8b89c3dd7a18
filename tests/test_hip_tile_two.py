"""sbt_tile_x2 (genrich_amd/csrc/gx_sbtile.h): two ordinary tiles per wavefront, on constructed PAIRS of tiles.

The plain first launch of k_sbtile hands a wavefront two adjacent tiles at once when both are active and both hold at most
GX_SBT_KR * 64 = 128 keys: the tiles b and b + 1 of a bin with b even (sbt_bin's order array).  Pairing is a function of the
data alone, restated here (pairs_of) and asserted for every case from the events (tile_census of test_hip_tile_limits.py), on a
machine without a GPU (test_pair_preconditions_on_the_oracle_alone): n and T of both tiles, that the pair forms or -- where
the case says so -- does not, and the intervals of both tiles from the oracle.  Library and oracle are compared by
assert_same_run: interval ends, pileups, p, q bit for bit, fragLen, lambda and the peaks as bytes.

The genome: five chromosomes, 27 tiles, bins of four (sb_shift = 2), so the pairs are the bin-relative (0, 1) and (2, 3):

  chromosome | length           | tiles (whole genome) | what it is for
  C0         | 3 tiles exactly  | 0 1 2                | its last tile closes at a tile multiple and is A of the pair (2, 3)
  C1         | 3 tiles + 1000   | 3 4 5 6              | tile 0 is B of (2, 3); tiles 1 | 2 are the interior pair (4, 5); its last tile -- no
             |                  |                      | tile multiple -- is A of (6, 7)
  C2         | 2 tiles + 700    | 7 8 9                | tile 0 is B of (6, 7); (8, 9) has a chromosome's last tile as B
  C3         | 2 tiles exactly  | 10 11                | quiet
  BG         | 60,000           | 12 .. 26             | the ordinary background of the existing modules; the last bin holds three tiles,
             |                  |                      | so tile 26 is always single (asserted)

Every fragment of a constructed tile lies inside it, except the one an odd key count needs and the partners of cancelling bases:
those reach into tiles that are not the pair's (`before` / `after`), so the two tiles' n and T are exactly what the case says.

That the cases see what they claim was checked once with scratch builds of the library, one value of sbt_tile_x2 broken each
(values stored into the tiles' own output slots only; no address, index or trip count), the default-path tests and the two -q
tests (36) run once on each:

  the break                                                      | tests that failed
  B's `before` (the pileup stored with an interval) one unit     | 36: every one -- the quiet neighbours pair too ("expt pileup bits", or the
    (1/120) too high                                             | library's own "Invalid pileup value")
  A's lastEnd taken from B (tileLastEnd, the fillers' ends)      | 5: carry-deep-A and carry-deep-B-ordinary-A (fragLen; an interval count), sig
                                                                 | with -p and both -q tests (the sweep walks A's fillers)
  B's running pileup taken from A before B's epilogue (the       | 1: last-as-B ("pileup of a chromosome does not return to 0 behind its last
    closing interval's value)                                    | base")
  B's fillers one short (`n - 1` handed to the epilogue)         | 3: sig with -p (summit, auc) and both -q tests
Not built: "step 2 of B skipped when A has one step" -- B's counters of the ranks 64 .. 127 would stay set in the wavefront's
scratch and put the following tiles' ranks, hence their output slots, out of bounds: a changed trip count, not a changed value.
The cases with a significant stretch over both tiles are what sees lastEnd and the fillers; an ordinary pair's neighbours are not
part of a peak, so nobody reads them there (as test_hip_tile_limits.py found for sbt_tile).
"""
import functools

import numpy as np
import pytest

import backends as B
from test_hip_merge_limits import MODES, TB, TILE, background
from test_hip_parity import assert_same_run, hip_backend
from test_hip_tile_limits import (FRAG_FAST_MAXV, FELL_BACK, FUSED, LOOSE, PAIRS, SBT_PEAK_KEYS, rows, run_oracle, sb_shift, stairs, tile_census,
                                  tile_counts)

X2_KEYS = 128           # gx_sbtile.h  SBT_X2_KEYS = GX_SBT_KR * 64: a paired tile's keys at most
STEP = 64               # touched bases per step
C0, C1, C2, C3, BGC = 0, 1, 2, 3, 4
LENS = [3 * TILE, 3 * TILE + 1000, 2 * TILE + 700, 2 * TILE, 60_000]
NT = [(l + TILE - 1) >> TB for l in LENS]
TILE_BASE = np.concatenate([[0], np.cumsum(NT)]).astype(np.int64)
N_TILES = int(TILE_BASE[-1])
SBS = sb_shift(N_TILES)
assert NT == [3, 4, 3, 2, 15] and SBS == 2 and N_TILES % 4 == 3   # bins of four tiles; the last bin holds three


def gt(chrom, tile):
    return int(TILE_BASE[chrom]) + tile


def pairs_of(n, active):
    """the pairs sbt_bin forms: the even tile of every two adjacent, even-aligned tiles (bins are multiples of four tiles, so
    even within the bin = even in the genome) that both exist, are active and hold at most X2_KEYS keys"""
    return {g for g in range(0, N_TILES - 1, 2) if active[g] and active[g + 1] and n[g] <= X2_KEYS and n[g + 1] <= X2_KEYS}


def calm(chrom, tile, rng, k=40):
    """a neighbour far from every limit: k stairs inside the tile (test_hip_tile_limits.quiet for this genome's lengths)"""
    lo, hi = tile * TILE + 300, min((tile + 1) * TILE, LENS[chrom]) - 300
    return stairs(chrom, rng.choice(np.arange(lo, hi), k, replace=False), spill=0, depth=8)


def fill(chrom, tile, n, T, seed, before=None, after=None, depth=16, base0=False):
    """n keys on exactly T offsets of the tile.  Every fragment lies inside the tile, except: the one an odd T needs and the one
    an odd number of further keys needs, which come from `before` (a position in an earlier tile) or go to `after`.  base0: one of
    the T touched bases is base 0 (a fragment from 0 to an end in use, or to a base of its own)."""
    if n == 0:
        return []
    assert n >= T >= 1
    rng = np.random.default_rng(1000 * T + seed)
    p0 = tile * TILE
    hi = min(p0 + TILE, LENS[chrom]) - 8
    P = np.sort(rng.choice(np.arange(p0 + 8, hi), T - (1 if base0 else 0), replace=False)).astype(np.int64)
    fr = []

    def outside(p, i=0):   # one key on p: a fragment to `after`, or from `before`
        return (chrom, int(p), int(after) + (i % 4), 1) if after is not None else (chrom, int(before) - (i % 4), int(p), 1)
    if len(P) % 2:
        odd = P[-1] if after is not None else P[0]
        fr.append(outside(odd))
        P = P[P != odd]
    fr += stairs(chrom, P, spill=0, depth=depth)
    inside = [f for f in fr if p0 <= f[1] and f[2] < p0 + TILE]
    if base0:
        assert p0 == 0
        ends = sorted(f[2] for f in inside)
        fr.append((chrom, 0, ends[-1] if ends else int(after), 1))   # base 0 and a key on an end in use
    have = sum(p0 <= f[1] < p0 + TILE for f in fr) + sum(p0 <= f[2] < p0 + TILE for f in fr)
    more = n - have
    assert more >= 0, (n, T, have)
    # (a further key goes on a start in use when it starts a fragment, on an end in use when it ends one: never a cancelling base)
    if inside:
        used = min(f[1] for f in inside) if after is not None else max(f[2] for f in inside)
    else:
        used = int(fr[0][1] if p0 <= fr[0][1] < p0 + TILE else fr[0][2])
    if more % 2 or not inside:
        k = more if not inside else 1
        fr += [outside(used, i) for i in range(k)]
        more -= k
    fr += [inside[i % len(inside)] for i in range(more // 2)]
    return fr


def cancelling(chrom, tile, ranks_of, T, seed, before, after, also_plain=True):
    """T touched bases of which those with the ranks `ranks_of` cancel (a fragment from `before` ends there and one of equal weight
    starts there and goes to `after`); the others are stairs inside the tile"""
    rng = np.random.default_rng(7000 + seed)
    p0 = tile * TILE
    P = np.sort(rng.choice(np.arange(p0 + 8, p0 + TILE - 8), T, replace=False)).astype(np.int64)
    cz = P[list(ranks_of)]
    plain = np.setdiff1d(P, cz)
    assert len(plain) % 2 == 0
    fr = stairs(chrom, plain, spill=0) if len(plain) else []
    for i, p in enumerate(cz):
        fr += [(chrom, int(before) - (i % 8), int(p), 1), (chrom, int(p), int(after) + (i % 8), 1)]
    return fr


# ---- the cases: name -> dict(frags, A, B, want=((nA, TA), (nB, TB)), pair, out=(outA, outB) or None, save, empty) ----------
IA, IB = (C1, 1), (C1, 2)                 # the interior pair: tiles 4 | 5 of the genome
I_BEFORE, I_AFTER = 600, 3 * TILE + 300   # ... and where its odd keys come from and go to: C1's first and last tile


def _case(frags, A, B, want, pair=True, out=None, save=None, empty=(), bare=(), also=None):
    """empty: tiles that must hold no key; bare: tiles that get no quiet filling either (they hold what the case put there)"""
    assert gt(*A) % 2 == 0 and gt(*B) == gt(*A) + 1 and (gt(*A) >> SBS) == (gt(*B) >> SBS)
    return dict(frags=frags, A=A, B=B, want=want, pair=pair, out=out, save=save, empty=set(empty), bare=set(bare) | set(empty), also=also)


def case_keys(nA, nB):
    """keys on few touched bases (32 each, or what the keys allow)"""
    TA, TB_ = min(32, nA), min(32, nB)
    fr = fill(*IA, nA, TA, 1, before=I_BEFORE) + fill(*IB, nB, TB_, 2, after=I_AFTER)
    return _case(fr, IA, IB, ((nA, TA), (nB, TB_)), pair=nA <= X2_KEYS and nB <= X2_KEYS)


def case_touched(TA, TB_):
    nA, nB = (TA + 1 if TA < X2_KEYS else TA), (TB_ + 1 if TB_ < X2_KEYS else TB_)
    if TA == 1:
        nA = 1
    if TB_ == 1:
        nB = 1
    fr = fill(*IA, nA, TA, 3, before=I_BEFORE) + fill(*IB, nB, TB_, 4, after=I_AFTER)
    return _case(fr, IA, IB, ((nA, TA), (nB, TB_)), out=(TA, TB_))


def case_cancel_all(mirror):
    """a tile all of whose touched bases cancel (T = 50, no interval: k_scan_iv fills its slots) beside an ordinary one"""
    X, Y = (IB, IA) if mirror else (IA, IB)
    fr = cancelling(*X, range(50), 50, 5, I_BEFORE, I_AFTER) + fill(*Y, 91, 90, 6, before=I_BEFORE + 40, after=None)
    w = {X: (100, 50), Y: (91, 90)}
    o = {X: 0, Y: 90}
    return _case(fr, IA, IB, (w[IA], w[IB]), out=(o[IA], o[IB]))


def case_cancel_last_step(mirror):
    """one tile's second step cancels altogether (ranks 64 and 65 of T = 66: `mask` is zero, lastEnd and outCount must stay) while
    the other tile emits in its second step; 300 fragments keep the pileup up behind the pair, so the next tile's first interval
    -- measured from the cancelling tile's lastEnd when that tile is B -- is part of a peak's area"""
    X, Y = (IB, IA) if mirror else (IA, IB)
    fr = cancelling(*X, (64, 65), 66, 7, I_BEFORE, I_AFTER) + fill(*Y, 101, 100, 8, before=I_BEFORE + 40)
    a0 = min(f[1] for f in fr if f[1] >= IA[1] * TILE)
    fr += [(C1, a0, I_AFTER + 200 + (i % 4), 1) for i in range(300)]   # (300 keys on a start in use: in A)
    w = {X: (68, 66), Y: (101, 100)}
    w[IA] = (w[IA][0] + 300, w[IA][1])
    o = {X: 64, Y: 100}
    # (A now holds more than 128 keys: the cancelling last step of a PAIRED tile is the next case's)
    return _case(fr, IA, IB, (w[IA], w[IB]), pair=False, out=(o[IA], o[IB]))


def case_cancel_last_step_paired(mirror):
    """... and with both tiles paired: the pileup behind the pair stays up by 20 fragments from the tile before"""
    X, Y = (IB, IA) if mirror else (IA, IB)
    fr = cancelling(*X, (64, 65), 66, 9, I_BEFORE, I_AFTER) + fill(*Y, 101, 100, 10, before=I_BEFORE + 40)
    fr += [(C1, I_BEFORE + 100 + (i % 4), I_AFTER + 200 + (i % 4), 1) for i in range(20)]   # (over the whole pair: no key in it)
    w = {X: (68, 66), Y: (101, 100)}
    o = {X: 64, Y: 100}
    return _case(fr, IA, IB, (w[IA], w[IB]), out=(o[IA], o[IB]))


def case_border(which, TB_=33):
    """A = a chromosome's last tile, with its closing interval (C0: the length is a tile multiple; C1: it is not), B = the next
    chromosome's first tile with a key on base 0.  Seven fragments end at A's chromosome's length (no end record): the closing
    interval's pileup."""
    (ca, ta), cb = ((C0, 2), C1) if which == "multiple" else ((C1, 3), C2)
    lo = ta * TILE
    fr = fill(ca, ta, 41, 40, 11, before=600)
    fr += [(ca, lo + 100 + 10 * i, LENS[ca], 1) for i in range(7)]
    nB = TB_ + 1
    fr += fill(cb, 0, nB, TB_, 12, after=TILE + 500, base0=True)

    def also(o, ev):
        e, cols = o.get_intervals(-1, ca)
        assert e[-1] == LENS[ca] and cols["expt"][-1] == np.float32(7)
        assert (ev["start"][ev["chrom"] == cb] == 0).sum() == 1
    return _case(fr, (ca, ta), (cb, 0), ((48, 47), (nB, TB_)), out=(47, TB_ - 1), also=also)


def case_last_as_b():
    """B = a chromosome's last tile (C2's), five fragments ending at the length"""
    A, Bt = (C2, 1), (C2, 2)
    fr = fill(*A, 61, 60, 13, before=700) + fill(*Bt, 31, 30, 14, before=900)
    fr += [(C2, 2 * TILE + 50 + 10 * i, LENS[C2], 1) for i in range(5)]
    return _case(fr, A, Bt, ((61, 60), (36, 35)), out=(60, 35))


def case_not_saved(which):
    """a chromosome switched off by `save` whose tile is A (C0's last) or B (C2's first) of an aligned pair: no pair, and the
    other tile is still right"""
    save = np.ones(len(LENS), dtype=np.uint8)
    if which == "A":
        save[C0] = 0
        b = case_border("multiple")
    else:
        save[C2] = 0
        b = case_border("other")
    b.update(save=save, pair=False, out=None, also=None)
    return b


DEEP_V, DEEP_DROP, DEEP_LEN = 2151, 110, 8001


def case_carry_deep(where, a_ordinary=False):
    """test_hip_tile_limits' carry-deep construction in a tile that can be paired (110 ends on its first touched base instead of
    300: at most 128 keys).  The tile is entered at a pileup of 2151 >= FRAG_FAST_MAXV and every `after` is below it, so only the
    initial value of bigM marks it deep; its first interval is 8001 bases long (8001 x 2151: odd and beyond 2^24), which needs
    the tiles between empty -- for the deep tile as B that is A: an active tile without keys.  a_ordinary: A holds stairs
    instead (entered and left above FRAG_FAST_MAXV itself; parity only)."""
    s0 = 300 if where == "B" else 60
    f = s0 + DEEP_LEN
    deep = IB if where == "B" else IA
    other = IA if where == "B" else IB
    p0 = deep[1] * TILE
    assert p0 <= f < p0 + TILE - 100
    fr = [(C1, s0, f if i < DEEP_DROP else 3 * TILE + 700 + (i % 4), 1) for i in range(DEEP_V)]
    fr += stairs(C1, [f + x for x in (10, 20, 30, 40, 50, 60)], spill=0, depth=3)   # (behind the drop: it is the tile's first touched base)
    empty = set()
    if where == "B" and not a_ordinary:
        wo = (0, 0)
        empty.add(IA)
    else:
        fr += fill(*other, 51, 50, 15, before=None, after=I_AFTER + 100) if where == "A" else fill(*other, 50, 50, 15, before=I_BEFORE)
        wo = (51, 50) if where == "A" else (50, 50)
    wd = (DEEP_DROP + 6, 7)

    def also(o, ev):
        assert DEEP_V * 120 >= FRAG_FAST_MAXV
        e, cols = o.get_intervals(-1, C1)
        idx = np.flatnonzero((e[:-1].astype(np.int64) >> TB) == deep[1])
        v = cols["expt"]
        assert e[idx[0]] == f and v[idx[0]] == DEEP_V and v[idx[1]] == DEEP_V - DEEP_DROP
        assert (v[idx[1]:idx[-1] + 1] * 120 < FRAG_FAST_MAXV).all()
        if not a_ordinary:
            assert e[idx[0] - 1] == s0 and float(np.float32(DEEP_LEN) * np.float32(DEEP_V)) != DEEP_LEN * DEEP_V
    w = {deep: wd, other: wo}
    return _case(fr, IA, IB, (w[IA], w[IB]), empty=empty, bare={(C1, 0)}, also=also)


def case_sig():
    """both tiles significant from A's first interval to B's last: 300 fragments lie over the whole pair (their keys in the tiles
    before and behind it), 60 more over the border between the two, stairs on them in both tiles -- the significance word that
    holds B's first slot also holds A's last intervals and fillers"""
    pa, pb = IA[1] * TILE, IB[1] * TILE
    fr = [(C1, pa + 3000 + i, pb + 1000 + i, 1) for i in range(60)]   # 60 keys in each tile
    fr += [(C1, I_BEFORE + (i % 4), I_AFTER + (i % 4), 1) for i in range(300)]   # (no key in the pair)
    rng = np.random.default_rng(21)
    fr += stairs(C1, rng.choice(np.arange(pa + 3100, pa + 4090), 50, replace=False), spill=0, depth=2)
    fr += stairs(C1, rng.choice(np.arange(pb + 8, pb + 990), 50, replace=False), spill=0, depth=2)

    def also(o, ev, mode="p"):
        e, cols = o.get_intervals(-1, C1)
        key, thr = ("q", np.float32(-np.log10(MODES["q"]["pq"]))) if mode == "q" else ("p", np.float32(-np.log10(MODES["p"]["pq"])))
        k = np.flatnonzero((e >= pa) & (e < pb + TILE))
        assert len(k) == 220 and (cols[key][k] > thr).all(), (mode, len(k), float(cols[key][k].min()))
    return _case(fr, IA, IB, ((110, 110), (110, 110)), out=(110, 110), also=also)


def case_order(nA, nB):
    """a peak tile (more than SBT_PEAK_KEYS keys: drawn first) or one of 129 .. 200 keys at A or B of an aligned position: both
    tiles single"""
    fr = fill(*IA, nA, 60, 16, before=I_BEFORE) + fill(*IB, nB, 60, 17, after=I_AFTER)
    return _case(fr, IA, IB, ((nA, 60), (nB, 60)), pair=False, out=(60, 60))


CASES = {
    "keys-128-128": (case_keys, (128, 128)), "keys-128-129": (case_keys, (128, 129)), "keys-129-128": (case_keys, (129, 128)),
    "keys-64-65": (case_keys, (64, 65)), "keys-65-64": (case_keys, (65, 64)), "keys-1-1": (case_keys, (1, 1)),
    "keys-0-128": (case_keys, (0, 128)), "keys-128-0": (case_keys, (128, 0)),
    "touched-64-64": (case_touched, (64, 64)), "touched-64-65": (case_touched, (64, 65)), "touched-65-64": (case_touched, (65, 64)),
    "touched-128-128": (case_touched, (128, 128)), "touched-1-128": (case_touched, (1, 128)), "touched-128-1": (case_touched, (128, 1)),
    "cancel-all-A": (case_cancel_all, (False,)), "cancel-all-B": (case_cancel_all, (True,)),
    "cancel-last-step-A": (case_cancel_last_step_paired, (False,)), "cancel-last-step-B": (case_cancel_last_step_paired, (True,)),
    "cancel-last-step-A-single": (case_cancel_last_step, (False,)),
    "border-multiple": (case_border, ("multiple",)), "border-other": (case_border, ("other",)),
    "border-base0-T64": (case_border, ("multiple", 64)), "border-base0-T65": (case_border, ("multiple", 65)),
    "last-as-B": (case_last_as_b, ()),
    "not-saved-A": (case_not_saved, ("A",)), "not-saved-B": (case_not_saved, ("B",)),
    "carry-deep-B": (case_carry_deep, ("B",)), "carry-deep-B-ordinary-A": (case_carry_deep, ("B", True)), "carry-deep-A": (case_carry_deep, ("A",)),
    "sig": (case_sig, ()),
    "order-peak-A": (case_order, (SBT_PEAK_KEYS + 1, 100)), "order-peak-B": (case_order, (100, SBT_PEAK_KEYS + 1)),
    "order-150-100": (case_order, (150, 100)), "order-100-150": (case_order, (100, 150)),
}


@functools.lru_cache(maxsize=None)
def _built(name):
    fn, args = CASES[name]
    b = fn(*args)
    rng = np.random.default_rng(len(name))
    own = {b["A"], b["B"]} | b["bare"]
    q = []
    for c in (C0, C1, C2, C3):
        for t in range(NT[c]):
            if (c, t) not in own:
                q += calm(c, t, rng)
    b["frags"] = list(b["frags"]) + q
    return b


@functools.lru_cache(maxsize=None)
def _oracle(name, mode="p"):
    """the reference of a case: computed once, shared by the oracle-only test and the GPU tests, left unchanged"""
    b = _built(name)
    bg = background(1700)
    bg["chrom"] = BGC
    ev = np.concatenate([rows(b["frags"]), bg])
    case = dict(lens=LENS, replicates=[dict(save=b["save"], treat=ev, ctrl=None)])
    params, o, so = run_oracle(case, mode)
    return b, ev, case, params, o, so


def check(name, mode="p"):
    b, ev, case, params, o, so = _oracle(name, mode)
    n, T = tile_census(ev, LENS)[:2]
    ga, gb = gt(*b["A"]), gt(*b["B"])
    got = ((int(n[ga]), int(T[ga])), (int(n[gb]), int(T[gb])))
    assert got == b["want"], (name, got, b["want"])
    active = np.repeat(np.ones(len(LENS), dtype=np.uint8) if b["save"] is None else b["save"], NT).astype(bool)
    formed = pairs_of(n, active)
    assert (ga in formed) == b["pair"], (name, got)
    assert N_TILES - 1 not in formed and (N_TILES - 1) % 2 == 0   # the last bin's third tile has no partner
    for c, t in b["empty"]:
        assert n[gt(c, t)] == 0
    if b["out"] is not None:
        for (c, t), want in zip((b["A"], b["B"]), b["out"]):
            assert int(tile_counts(o.get_intervals(-1, c)[0], LENS[c])[t]) == want, (name, c, t)
    if b["also"]:
        if name == "sig":
            b["also"](o, ev, mode)
        else:
            b["also"](o, ev)
    assert o.n_peaks > 0
    return got, sorted(formed)


@pytest.mark.parametrize("name", sorted(CASES))
def test_pair_preconditions_on_the_oracle_alone(name):
    print(name, check(name))


def test_the_significant_pair_is_significant_with_q_values_too():
    print(check("sig", "q"))


def test_the_cases_cover_the_pair_paths_limits():
    want = {k: _built(k)["want"] for k in CASES}
    ns = {w for k, w in want.items() if k.startswith("keys-")}
    assert {((128, 32), (128, 32)), ((128, 32), (129, 32)), ((129, 32), (128, 32)), ((1, 1), (1, 1)), ((0, 0), (128, 32))} <= ns
    ts = {(w[0][1], w[1][1]) for k, w in want.items() if k.startswith("touched-")}
    assert {(STEP, STEP), (STEP, STEP + 1), (STEP + 1, STEP), (X2_KEYS, X2_KEYS), (1, X2_KEYS), (X2_KEYS, 1)} <= ts
    assert not _built("keys-128-129")["pair"] and not _built("keys-129-128")["pair"] and _built("keys-128-128")["pair"]
    assert _built("cancel-all-A")["out"] == (0, 90) and _built("cancel-all-B")["out"] == (90, 0)
    for k in ("order-peak-A", "order-peak-B", "order-150-100", "order-100-150", "not-saved-A", "not-saved-B"):
        assert not _built(k)["pair"], k
    assert LENS[C0] % TILE == 0 and LENS[C1] % TILE != 0 and gt(C0, NT[C0] - 1) % 2 == 0 and gt(C1, NT[C1] - 1) % 2 == 0


# the instances: the default (k_sbtile<PAIRS>, pair path), one persistent workgroup for every bin, and -- for parity only -- the
# start / end key instance, which has no pair path
PATHS = {"default": {}, "one-workgroup": {"GX_SBT_GRID": "1"}, "start-end-keys": {"GX_NO_PAIRS": "1"}}


def _run(monkeypatch, name, path, mode="p", frac=False):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    check(name, mode)
    b, ev, case, params, o, so = _oracle(name, mode)
    h = hip_backend(params)
    if frac:
        h.expect_fractional(True)
    sh = B.run_case(h, case)
    flags = h.path_info()
    print(name, path, mode, "flags", flags)
    assert_same_run(o, h, so, sh, case)
    assert h.n_peaks == o.n_peaks > 0
    return flags


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["default", "one-workgroup"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_two_tiles_per_wavefront(monkeypatch, name, path):
    flags = _run(monkeypatch, name, path)
    assert flags & FUSED and flags & PAIRS and not flags & FELL_BACK, flags
    if name == "sig":
        assert flags & LOOSE, flags   # (-p on one replicate: the sweep walks the loose slots and reads the tile stage's bits)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_same_pairs_on_the_start_and_end_key_instance(monkeypatch, name):
    flags = _run(monkeypatch, name, "start-end-keys")
    assert flags & FUSED and not flags & PAIRS and not flags & FELL_BACK, flags


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["keys-128-128", "touched-64-65", "touched-128-128", "cancel-last-step-A", "border-other", "sig"])
def test_the_same_pairs_announced_as_weighted(monkeypatch, name):
    """the fractional instance (no pair path) on the same unit-weight events: parity only"""
    flags = _run(monkeypatch, name, "default", frac=True)
    assert flags & FUSED and flags & PAIRS and not flags & FELL_BACK, flags


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["default", "one-workgroup"])
def test_significance_bits_of_a_pair_with_q_values(monkeypatch, path):
    """-q: lambda comes with the p-values' table, the significance bits after the tile stage"""
    flags = _run(monkeypatch, "sig", path, mode="q")
    assert flags & FUSED and not flags & FELL_BACK, flags
