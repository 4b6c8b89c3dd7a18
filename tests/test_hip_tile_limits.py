"""The tile stage -- sbt_tile / sbt_heavy of genrich_amd/csrc/gx_sbtile.h, and on the general chain k_tile_fast
(gx_tile_fast.h) / k_tile_heavy -- at its per-tile limits, on constructed tiles.

A tile (4096 bp) is one wavefront's: its keys (start keys and end keys; `n`) mark an occupancy bitmap, every touched base (a
distinct offset with at least one key; `T`) gets a rank, the keys' weights are added by rank one ROUND of TR touched bases at
a time (later rounds relying on the unsigned wrap of `r -= r0; r < TR_CAP`), and a round is walked in STEPS of 64 touched
bases, each of which emits an interval where the net difference is not zero (`out`; never at base 0 of a chromosome) and hands
lastEnd / outCount / runBase to the next.  The first KR * 64 keys of a tile live in registers, the others are read from the
LDS list in every pass; past SBT_HEAVY keys the tile is the whole workgroup's (a counter per base).  Every case below builds ONE
tile by hand -- "stairs" (fragments with distinct starts and distinct ends), keys stacked on shared offsets, bases where a
fragment ends and one of equal weight starts ("cancelling": touched, but nothing ends there) -- next to quiet neighbours, and
every case ASSERTS n, T AND out OF ITS TILE: n and T from the events alone as the kernels count them (tile_census), out from the
oracle's interval ends (tile_counts) -- on a machine without a GPU (test_tile_preconditions_on_the_oracle_alone).  Oracle and
library are compared by assert_same_run: interval ends, pileups, p, q bit for bit, fragLen, lambda and the peaks as bytes.

What the suite reached before this module, counted with the events alone (tile_census over every tile of the inputs; n
"at a limit": 64 / 65, 128 / 129, 192 / 193, 200 / 201, 4096 / 4097; T: 64 / 65, 384 / 385, 448 / 449, 512 / 513, 896 / 897,
1024 / 1025, 4096):

  existing GPU test (its input)                                    | largest n | largest T | tiles exactly at a limit or one past it
  test_hip_paths _case(seed 11): 90,000 fragments, 136 tiles       |     3,128 |     1,292 | none
    (also test_hip_sbt_persistent _many_bins)                      |           |           |
  test_hip_paths _case(seed 5, 150,000 fragments)                  |     5,040 |     1,685 | none
  test_hip_paths ..._beyond_the_key_array[30000]                   |    20,689 |     4,070 | n = 129 (one tile)
    (also test_hip_sbt_persistent _pile_case)                      |           |           |
  test_hip_paths ..._beyond_the_key_array[58000]                   |    39,740 |     4,095 | n = 129 (one tile)
  test_hip_sbt_instances, plain: 430,000 fragments, dense launch   |    27,224 |     3,679 | none
  test_hip_parity::test_random_runs_against_oracle, 50 seeds,      |     6,292 |     1,986 | n = 64 (28 tiles), 65 (21), 128 (8), 129 (7),
    every sample of every run                                      |           |           | 192 (12), 193 (8), 200 (8), 201 (8); T = 64 (26),
                                                                   |           |           | 65 (20), 384 (3), 385 (1), 448 (3), 449 (1), 513 (1)
  (test_hip_fullsize: the same generator at 50 M fragments; not counted)

So later rounds, the keys beyond the registers and sbt_heavy HAD run, by the density of the generator, on tiles of thousands of
keys whose n and T nobody chose, and the fifty small random runs had met T = 448 / 449 and 384 / 385 in a handful of tiles
-- on whichever path that seed's run took, without any test saying so.  Never reached before: n = 4096 / 4097 (the step to
the whole workgroup), T = 512, 896 / 897, 1024 / 1025, a full tile (T = 4096: the most was 4,095), and nothing chosen: a step
or a round of cancelling bases, a tile all of whose touched bases cancel, base 0 on a step or a round border, a chosen residue
of a tile's first loose slot, a single that carries into a tile at 448 / 449, a tile entered at FRAG_FAST_MAXV.

That the cases see what they claim was checked once with scratch builds of the library, one line of gx_sbtile.h or
gx_tile_fast.h broken each (values inside a tile's own scratch and output slots only), the whole module as it stands (292 GPU
tests) run once on each:

  the break                                                     | tests that failed
  sbt_tile: put's bound `r < TR_CAP - 1` (a round's last rank   | 89: exactly the cases with T >= 448 on the fused paths -- touched-T448
    dropped)                                                    | and up (T447 passes), full, cancel-round*, base0-T448 / T449, long-* /
                                                                | cross-*, sig-*, their weighted twins; dense-T384 / T385 at TR = 384
                                                                | (T383 passes) and dense-cancel-round at both; none on the general chain
  sbt_tile: A2's loop over the keys beyond the registers one    | 211: every case on every fused path (wrong intervals, or the library's own
    stride late                                                 | "Invalid pileup value": the background's tiles hold more than 128 keys too)
  sbt_tile: lastEnd (and outCount) updated when `mask` is zero  | 8: cancel-last-step on default / start-end-keys / one-workgroup (the peak's
                                                                | area behind the tile), w-cancel-last-step, w-cancel-step, w-cancel-round,
                                                                | -round384, -round512 (fragLen's terms)
  sbt_tile: the base-0 compare dropped                          | 10: base0-T1 / T64 / T65 / T448 / T449 on default and start-end-keys
  sbt_tile: the fillers' `size = n`                             | 154: nearly every case wherever the sweep walks the loose slots (default,
                                                                | start-end-keys, one-workgroup, -q); none with -E regions or weights
  sbt_heavy: lastEnd from the first wavefront alone (*)         | 3: keys-n4097 on default, full-plus-one on default and one-workgroup (the
                                                                | area of the peak that crosses the tile's end)
  sbt_tile: bigM = 0 (the `carry >= FRAG_FAST_MAXV` start gone) | 2: carry-deep on default and start-end-keys (fragLen off by one unit)
  k_tile_fast: the same initial value gone                      | 1: carry-deep on the general chain (fragLen off by one unit)
  k_tile_fast: the start keys beyond the registers one stride   | 78: stream-nS129 on the general chain (nS128, nE128 / nE129 pass), and the
    late                                                        | 77 general-chain runs on the ordinary background (tiles of > 128 starts)
  k_tile_fast: the end keys beyond the registers likewise       | 77: the same 77 general-chain runs.  NOT stream-nE129 as it then stood: its
                                                                | extra ends lay on the tile's last touched base, where a missing key changes
                                                                | no interval; the case now stacks them on the lowest end (not run again)
  (*) "from the first thread" would be base 0 .. 3 of the tile for every tile and fail everything heavy at once; the first
  wavefront's maximum is the subtler wrong value -- right whenever the last breakpoint lies in the tile's first 256 bases.
An earlier state of the module was too weak against the lastEnd breaks -- a crowded tile, a full one and a cancelling last step
whose following interval was not significant, so nobody read the tile's last end --; those cases now keep the pileup up into the
next tile.
"""
import functools

import numpy as np
import pytest

import backends as B
from test_hip_merge_limits import MODES, TB, TILE, background, run_oracle, tile_counts
from test_hip_parity import assert_same_run, hip_backend

# ---- the kernels' limits, and where they are written -------------------------------------------------------------------
SBT_KR = 2              # gx_sbtile.h:243  GX_SBT_KR: keys per lane in registers (sbt_tile)
REG_KEYS = SBT_KR * 64  # gx_sbtile.h:262  `for (k = KR * 64 + lane; ..)`: keys 129 and up come from the LDS list in every pass
KEY_SLACK = 192         # gx_sbtile.h:124 / :252  the key array's slack: a tile's first 192 keys are read without a bounds check
SBT_PEAK_KEYS = 200     # gx_sbtile.h:64   more keys than this: the tile is drawn ahead of the ordinary ones (:1042)
SBT_TR = 448            # gx_sbtile.h:62   GX_SBT_TR: touched bases per round (:283 / :288)
SBT_TR_DENSE = 384      # gx_sbtile.h:81   ... in the dense launch's small instance
STEP = 64               # gx_sbtile.h:342  touched bases per step of a round
SBT_HEAVY = 4096        # gx_sbtile.h:65   more keys than this: the whole workgroup's tile (:952, :1074)
KEYCAP = 46_912         # gx_sbtile.h:124  sbt_keycap(448)
TF_TR_CAP = 512         # gx_tile_fast.h:37  TR_CAP of k_tile_fast (GX_NO_FUSED)
TF_REG_KEYS = 2 * 64    # gx_tile_fast.h:34  TF_KPL = 2: keys PER STREAM in registers (:90, :145-146, :201-202: `k < nS`, `k < nE`)
HEAVY_MIN = 4096        # gx_kernels.h:445   more records than this: k_tile_heavy (:617)
FRAG_FAST_MAXV = ((1 << 24) // (2 * TILE)) * 120   # gx_kernels.h:446, in 1/120 units: a pileup of 2048
UNIT_PAIR_MAXLEN, FRAC_PAIR_MAXLEN = 4095, 511     # gx_sort.h:882  `len - 1 < (1 << LENB) - 1`: LENB = 12, fractional 9
SBT_MAXSHIFT = 8        # gx_sort.h:573
# n or T of a tile that is "exactly at a limit or one past it"
AT = sorted({v + d for v in (STEP, REG_KEYS, KEY_SLACK, SBT_PEAK_KEYS, SBT_TR_DENSE, SBT_TR, TF_TR_CAP, 2 * SBT_TR, 2 * TF_TR_CAP, SBT_HEAVY)
             for d in (0, 1)})
FUSED, LOOSE, FELL_BACK, PAIRS, FRAC_PAIRS = 1, 2, 4, 16, 128   # gx_path_info bits (tests/test_hip_paths.py)
COUNTS = (1, 2, 3, 4, 5, 6, 8, 10)   # the eight weight classes of a fractional pair record (gx_sbtile.h:199 sbt_weight)

# Two stair chromosomes -- the first with a length that is a multiple of the tile (its closing interval ends beyond the last
# tile), the second not, and long enough to reach into a second super-bucket --, one with an ordinary background, one that
# nobody touches.
S0, S1, BG, NOBODY = 0, 1, 2, 3
LENS = [4 * TILE, 5 * TILE + 1000, 60_000, 5_000]
NT = [(l + TILE - 1) >> TB for l in LENS]
TILE_BASE = np.concatenate([[0], np.cumsum(NT)]).astype(np.int64)


def sb_shift(n_tiles):
    """tiles per super-bucket (log2) as the host plans them: gx_host_build.h:852-858"""
    lg = 0
    while (1 << lg) < n_tiles:
        lg += 1
    return min(SBT_MAXSHIFT, max(0, (lg - 1) // 2))


SBS = sb_shift(int(TILE_BASE[-1]))
assert SBS == 2 and TILE_BASE[S1] % (1 << SBS) == 0 and NT[S1] > (1 << SBS)   # S1's tile 3 | 4 is a super-bucket border


def tile_census(ev, lens=LENS):
    """Per tile of the whole genome (chromosome after chromosome), as the kernels count: n, the keys (a start key per fragment,
    an end key unless the fragment ends at the chromosome's length), T, the distinct offsets that hold one, and the keys by
    stream, nS start keys and nE end keys (k_tile_fast keeps 128 of EACH in registers)."""
    lens = np.asarray(lens, dtype=np.int64)
    base = np.concatenate([[0], np.cumsum((lens + TILE - 1) >> TB)])
    c = ev["chrom"].astype(np.int64)
    s, e = ev["start"].astype(np.int64), ev["end"].astype(np.int64)
    assert (s < e).all() and (e <= lens[c]).all()
    has_end = e < lens[c]
    kc = np.concatenate([c, c[has_end]])
    kp = np.concatenate([s, e[has_end]])
    kt = base[kc] + (kp >> TB)
    n = np.bincount(kt, minlength=base[-1])
    nS = np.bincount(kt[:len(c)], minlength=base[-1])
    uniq = np.unique(kt * TILE + (kp & (TILE - 1)))
    T = np.bincount(uniq >> TB, minlength=base[-1])
    return n, T, nS, n - nS


def gt(chrom, tile):
    return int(TILE_BASE[chrom]) + tile


def first_slot(ev, chrom, tile):
    """a tile's first loose slot: the keys before it plus its number (gx_sbtile.h:17, :1025)"""
    n = tile_census(ev)[0]
    return int(n[:gt(chrom, tile)].sum()) + gt(chrom, tile)


def rows(frags):
    return np.array([(int(c), int(s), int(e), int(k)) for c, s, e, k in frags], dtype=B.EVENT_DTYPE).reshape(-1)


def stairs(chrom, pos, spill, depth=16, counts=None):
    """Fragments whose starts and ends are exactly the distinct positions `pos`: sorted, in groups of 2 * depth -- the first
    half starts, the second half ends.  An odd one out starts a fragment that ends at `spill` (another tile).  counts: the
    fragments' counts cycle through them."""
    pos = np.sort(np.asarray(pos, dtype=np.int64))
    assert len(np.unique(pos)) == len(pos)
    out = []
    odd = None
    if len(pos) % 2:
        pos, odd = pos[:-1], int(pos[-1])
    for a in range(0, len(pos), 2 * depth):
        ch = pos[a:a + 2 * depth]
        m = len(ch) // 2
        out += [(chrom, int(s), int(e)) for s, e in zip(ch[:m], ch[m:])]
    if odd is not None:
        out.append((chrom, odd, int(spill)))
    cyc = counts or (1,)
    return [(c, s, e, cyc[i % len(cyc)]) for i, (c, s, e) in enumerate(out)]


def quiet(chrom, tiles, rng, k=40):
    """neighbours far from every limit: k stairs in each of the tiles"""
    fr = []
    for t in tiles:
        lo, hi = t * TILE + 300, min((t + 1) * TILE, LENS[chrom]) - 300
        fr += stairs(chrom, rng.choice(np.arange(lo, hi), k, replace=False), spill=0, depth=8)
    return fr


FORCED = (20, 531, 540, 1052)   # offsets 511 and 512 apart: a fractional pair record holds 9 bits of length, 512 is a single


def make_tile(chrom, tile, T, n=None, *, cancel=(), unequal=(), weights=False, seed=0, all_cancel=False, extra=(), spill_over=0, lens=LENS):
    """One tile with exactly T touched bases and n keys (default: T + 1, or what the cancelling bases need).  `cancel`: the ranks (among the tile's touched bases,
    in order) of bases where a fragment ends and one of equal weight starts; `unequal`: ranks where 60 come in and 40 go out
    (counts 2 and 3).  Their partners are the tile's lowest start and highest end (pair records) or, where the base lies
    outside those, positions in the neighbouring tiles.  weights: the eight counts cycle through the stairs, and two of them are
    511 and 512 bases long.  Keys beyond T are stacked on offsets in use: copies of stairs, one fragment into the next tile for an
    odd count.  Returns the fragments and what the tile must hold: (n, T, out)."""
    rng = np.random.default_rng(1000 * T + seed)
    p0 = tile * TILE
    counts = COUNTS if weights else None
    forced = [p0 + f for f in FORCED] if weights and not all_cancel and T >= 64 else []
    if T == TILE:
        P = np.arange(p0, p0 + TILE)
    else:
        pool = np.setdiff1d(np.arange(p0 + 8, p0 + TILE - 8), forced)
        P = np.sort(np.concatenate([rng.choice(pool, T - len(forced), replace=False), forced]).astype(np.int64))
    assert len(P) == T and P[0] > 0
    special = sorted(set(cancel) | set(unequal))
    assert all(0 <= r < T for r in special) and not set(cancel) & set(unequal)
    sp = P[special] if special else np.zeros(0, dtype=np.int64)
    assert not set(sp.tolist()) & set(forced)
    plain = np.setdiff1d(P, np.concatenate([sp, forced]).astype(np.int64))
    prev_pos, next_pos = p0 - 200, p0 + TILE + 40
    assert prev_pos > 0 and next_pos + 16 < lens[chrom]
    fr = stairs(chrom, plain, spill=next_pos + 2, counts=counts)
    if forced:
        fr += [(chrom, forced[0], forced[1], 2), (chrom, forced[2], forced[3], 3)]
        assert forced[1] - forced[0] == FRAC_PAIR_MAXLEN and forced[3] - forced[2] == FRAC_PAIR_MAXLEN + 1
    inside = [f for f in fr if f[1] >= p0 and f[2] < p0 + TILE]
    a0 = min((f[1] for f in fr if f[1] >= p0), default=None)
    b0 = max((f[2] for f in fr if f[2] < p0 + TILE), default=None)
    for i, r in enumerate(special):
        p = int(P[r])
        a = a0 if a0 is not None and a0 < p else prev_pos - (i % 8)
        b = b0 if b0 is not None and b0 > p else next_pos + 8 + (i % 8)
        cin = COUNTS[i % 8] if weights else 1
        cin, cout = (2, 3) if r in unequal else (cin, cin)
        fr += [(chrom, a, p, cin), (chrom, p, b, cout)]
    fr += list(extra)
    # fragments that start on the tile's lowest start and end in the next tile: the pileup stays up across the tile's end
    fr += [(chrom, a0, next_pos + 300 + (i % 4), 1) for i in range(spill_over)]
    have = sum(p0 <= f[1] < p0 + TILE for f in fr) + sum(p0 <= f[2] < p0 + TILE for f in fr)   # (no fragment ends at the chromosome's length)
    if n is None:   # just above T; with cancelling bases (two keys each, and their partners): what they take
        n = max(T + 1, have)
    more = n - have
    assert more >= 0, (n, have)
    if more % 2:   # one key on a start in use, its end in the next tile
        s = a0 if a0 is not None else int(P[0])
        fr.append((chrom, s, next_pos + 4, 1))
        more -= 1
    if more:
        assert inside, "no fragment inside the tile to copy"
        fr += [inside[i % len(inside)] for i in range(more // 2)]
    return fr, (n, T, T - len(cancel))


# ---- the cases: name -> (fragments of the stair chromosomes, chromosome, tile, (n, T, out), what else the oracle must show) ----

def _std(chrom, tile, fr, want, rng, also=None):
    """the constructed tile among quiet tiles on both stair chromosomes"""
    others = [(c, t) for c in (S0, S1) for t in range(NT[c]) if (c, t) != (chrom, tile) and t > 0]
    q = []
    for c, t in others:
        q += quiet(c, [t], rng)
    return dict(frags=fr + q, chrom=chrom, tile=tile, want=want, also=also)


def case_keys(n):
    """keys with few touched bases: n keys stacked on 32 offsets (64 for the thousands, where 300 fragments also reach into the
    next tile: its first interval is significant, so its length -- from the crowded tile's last end, which sbt_heavy and
    sbt_tile hand to the fillers and to tileLastEnd -- is part of a peak's area)"""
    T = 64 if n > 1000 else 32
    fr, want = make_tile(S0, 2, T, n, seed=n, spill_over=300 if n > 1000 else 0)
    return _std(S0, 2, fr, want, np.random.default_rng(n))


def case_touched(T, weights=False):
    fr, want = make_tile(S0, 2, T, weights=weights, seed=1)
    return _std(S0, 2, fr, want, np.random.default_rng(T))


def case_full(plus, weights=False):
    """every base of the tile a breakpoint: n = T = 4096 (10 rounds at 448, 8 at 512, the prefix counts at their largest);
    plus: one more key on an offset in use -- 4097 keys, the whole workgroup's tile with every base touched.  300 fragments lie
    over the whole tile (their keys in the tiles before and behind): the next tile's first interval is significant, so the tile's
    last end -- its last base, in sbt_heavy the last thread's -- is read by a peak's area."""
    p0 = 2 * TILE
    over = [(S0, p0 - 900 + (i % 4), p0 + TILE + 700 + (i % 4), 1) for i in range(300)]
    fr, want = make_tile(S0, 2, TILE, TILE + plus, weights=weights, seed=2, extra=over)
    return _std(S0, 2, fr, want, np.random.default_rng(7 + plus))


CANCEL_KINDS = {   # T, the cancelling ranks
    "lanes": (200, (63, 64, 127)),                         # lane 63 of a step, lane 0 and lane 63 of the next
    "step": (200, tuple(range(64, 128))),                  # a whole step: `mask` is zero, lastEnd must stay
    "round": (1000, tuple(range(SBT_TR, 2 * SBT_TR))),     # a whole round of 448
    "round384": (1000, tuple(range(SBT_TR_DENSE, 2 * SBT_TR_DENSE))),   # ... of the small instance
    "round512": (1100, tuple(range(TF_TR_CAP, 2 * TF_TR_CAP))),         # ... of k_tile_fast
    "last": (100, (98, 99)),                               # the tile's last touched bases: lastEnd and the fillers come from rank 97
    "last-step": (130, (128, 129)),                        # ... and they are a step of their own
    "first": (100, (0,)),
}


def case_cancel(kind, weights=False):
    T, ranks = CANCEL_KINDS[kind]
    # (last / last-step: 300 fragments keep the pileup up into the next tile, so that the length of its first interval -- measured
    # from this tile's lastEnd, which the fillers and tileLastEnd carry -- is part of a peak's area)
    fr, want = make_tile(S0, 2, T, cancel=ranks, weights=weights, seed=3, spill_over=300 if kind.startswith("last") else 0)
    return _std(S0, 2, fr, want, np.random.default_rng(11))


def case_cancel_all(weights=False):
    """every touched base of the tile cancels: out = 0 with T = 50 -- the tile has no interval, k_scan_iv fills its slots"""
    fr, want = make_tile(S0, 2, 50, 100, cancel=tuple(range(50)), weights=weights, seed=4, all_cancel=True)
    assert want == (100, 50, 0)
    return _std(S0, 2, fr, want, np.random.default_rng(12))


def case_unequal():
    """60 in and 40 out (counts 2 and 3) must emit, equal weights must not -- next to each other, on a step border"""
    fr, want = make_tile(S0, 2, 200, cancel=(62, 64, 100), unequal=(63, 65, 101), weights=True, seed=5)
    return _std(S0, 2, fr, want, np.random.default_rng(13))


def case_base0(T):
    """A fragment that starts at position 0 of the chromosome: base 0 is touched (rank 0) and never closes an interval.  Alone
    (T = 1: the tile has no interval at all), and with T on a step and a round border."""
    if T == 1:
        fr, want = [(S1, 0, TILE + 77, 1)], (1, 1, 0)
    else:
        p = np.random.default_rng(T).choice(np.arange(8, TILE - 8), T - 1 - (T % 2 == 0), replace=False)
        fr = stairs(S1, p, spill=TILE + 33)
        ends = sorted(f[2] for f in fr if f[2] < TILE)
        if T % 2:   # the fragment from base 0 ends on an end in use ...
            fr.append((S1, 0, ends[-1], 1))
        else:       # ... or on a base of its own
            q = next(x for x in range(TILE - 7, TILE) if x not in set(p.tolist()))
            fr.append((S1, 0, q, 1))
        nn = int(tile_census(rows(fr))[0][gt(S1, 0)])
        want = (nn, T, T - 1)
    rng = np.random.default_rng(20 + T)
    q = []
    for c, t in [(S0, 1), (S0, 2), (S0, 3), (S1, 1), (S1, 2), (S1, 3), (S1, 4), (S1, 5)]:
        q += quiet(c, [t], rng)
    return dict(frags=fr + q, chrom=S1, tile=0, want=want, also=None)


SEAM_OFFSETS = (0, 31, 32, 63, 64, 4095)


def case_seams():
    """touched bases at the bitmap words' and the wavefront's seams of a tile that is not its chromosome's first, and an end
    exactly at the next tile's first base"""
    p0 = 2 * TILE
    fr = stairs(S0, [p0 + o for o in SEAM_OFFSETS], spill=0, depth=3)
    fr.append((S0, p0 + 31, 3 * TILE, 1))   # ends at the next tile's first base

    def also(o, ev):
        e = o.get_intervals(-1, S0)[0].astype(np.int64)
        assert set(p0 + np.array(SEAM_OFFSETS)) <= set(e.tolist()) and 3 * TILE in set(e.tolist())
    return _std(S0, 2, fr, (7, 6, 6), np.random.default_rng(31), also)


def case_chrom_end():
    """fragments that end exactly at the chromosome's length (no end record), seven on the first stair chromosome, five on the
    second: the closing interval's pileup"""
    fr = [(S0, 3 * TILE + 100 + 10 * i, LENS[S0], 1) for i in range(7)] + [(S1, 5 * TILE + 100 + 10 * i, LENS[S1], 1) for i in range(5)]
    rng = np.random.default_rng(32)
    q = []
    for c, t in [(S0, 1), (S0, 2), (S1, 1), (S1, 2), (S1, 3), (S1, 4)]:
        q += quiet(c, [t], rng)

    def also(o, ev):
        for c, k in ((S0, 7), (S1, 5)):
            e, cols = o.get_intervals(-1, c)
            assert e[-1] == LENS[c] and cols["expt"][-1] == np.float32(k), (c, cols["expt"][-1])
        n, T = tile_census(ev)[:2]
        assert (n[gt(S1, 5)], T[gt(S1, 5)]) == (5, 5)
    return dict(frags=fr + q, chrom=S0, tile=3, want=(7, 7, 7), also=also)


def case_long(T, cross):
    """A single (8-byte record) carries into a tile at 448 / 449.  long: a fragment of more than 4095 bases; cross: one that
    crosses the super-bucket border (and one that passes over the whole tile before it)."""
    chrom, tile = (S1, 4) if cross else (S0, 2)
    p0 = tile * TILE
    if cross:
        extra = [(chrom, p0 - 100, p0 + 4050, 1), (chrom, p0 - 300, p0 + 4051, 1)]   # 4150 / 4351 bases, across the border
    else:
        extra = [(chrom, p0 - 5000, p0 + 4050, 1), (chrom, p0 - 4097, p0 + 4051, 1)]  # longer than 4095 within one super-bucket
    fr, _ = make_tile(chrom, tile, T - 2, T - 2, seed=6)
    assert not {p0 + 4050, p0 + 4051} & {x for f in fr for x in f[1:3]}
    fr += extra
    if cross:
        assert (gt(chrom, tile) >> SBS) == (gt(chrom, tile - 1) >> SBS) + 1
    else:
        assert all(f[2] - f[1] > UNIT_PAIR_MAXLEN for f in extra) and (gt(chrom, tile) >> SBS) == (gt(chrom, tile - 2) >> SBS)

    def also(o, ev):
        assert _carry_in(o, chrom, tile) == 2.0
    return _std(chrom, tile, fr, (T, T, T), np.random.default_rng(33 + T), also)


def _carry_in(o, chrom, tile):
    """the pileup on the tile's first base, from the oracle: that of the first interval that ends behind it"""
    e, cols = o.get_intervals(-1, chrom)
    return float(cols["expt"][int(np.searchsorted(e, tile * TILE, side="right"))])


def case_empty_between():
    """two constructed tiles with empty tiles between them, nothing handed on (second chromosome) and one fragment handed on
    through them (first chromosome)"""
    rng = np.random.default_rng(34)
    fr = quiet(S1, [1], rng) + quiet(S1, [4], rng) + quiet(S1, [5], rng, k=10)
    fr += quiet(S0, [3], rng) + [(S0, TILE - 50, 3 * TILE + 50, 1)]
    fr += quiet(S0, [0], rng, k=60) + [(S0, TILE - 60, 3 * TILE + 60, 1)]   # (tile 0 of the first chromosome, tiles 1 and 2 empty)

    def also(o, ev):
        n = tile_census(ev)[0]
        assert n[gt(S0, 1)] == n[gt(S0, 2)] == 0 and n[gt(S1, 2)] == n[gt(S1, 3)] == 0
        assert _carry_in(o, S0, 2) == 2.0 and _carry_in(o, S1, 3) == 0.0
        assert tile_counts(o.get_intervals(-1, S0)[0], LENS[S0])[1:3].sum() == 0
    nn, tt = (int(x[gt(S0, 0)]) for x in tile_census(rows(fr))[:2])
    return dict(frags=fr, chrom=S0, tile=0, want=(nn, tt, tt), also=also)


def case_carry(kind):
    """The tile under test is entered with a pileup of nine: from the tile before, and from the bin before."""
    chrom, tile = (S1, 4) if kind == "bin" else (S0, 2)
    p0 = tile * TILE
    k = 9
    over = [(chrom, p0 - 900 + (i % 4), p0 + TILE + 700 + (i % 4), 1) for i in range(k)]
    fr, want = make_tile(chrom, tile, 6, seed=8)

    def also(o, ev):
        assert _carry_in(o, chrom, tile) == float(k)
        n = tile_census(ev)[0]
        assert n[gt(chrom, tile)] == 7 and n[gt(chrom, tile - 1)] < SBT_HEAVY
    return _std(chrom, tile, fr + over, want, np.random.default_rng(35), also)


DEEP_V, DEEP_DROP, DEEP_LEN = 2151, 300, 8001


def case_carry_deep():
    """bigM from `carry` ALONE (gx_sbtile.h:275, gx_tile_fast.h:169).  The tile is entered at a pileup of 2151 >= FRAG_FAST_MAXV,
    and 300 of those fragments end on its first touched base, with no start before it: `after` is below FRAG_FAST_MAXV on every
    lane of every step, so nothing but the initial value of bigM marks the tile deep.  Its first interval -- pileup 2151 --
    starts 8001 bases earlier (the tile between is empty): shorter than two tiles, so no other correction looks at it, and
    8001 x 2151 is an odd number beyond 2^24, which the reference's float product rounds -- fragLen is the oracle's only if the
    tile is on the deep list.  The interval is significant and part of a peak."""
    p0, s0 = 2 * TILE, 300
    f = s0 + DEEP_LEN
    assert p0 <= f < p0 + 900 and DEEP_LEN < 2 * TILE
    fr = [(S0, s0, f if i < DEEP_DROP else 3 * TILE + 700 + (i % 4), 1) for i in range(DEEP_V)]
    fr += stairs(S0, [p0 + x for x in (1000, 1100, 1200, 2000, 2100, 2200)], spill=0, depth=3)
    rng = np.random.default_rng(38)
    for c, t in [(S0, 3), (S1, 1), (S1, 2), (S1, 3), (S1, 4), (S1, 5)]:
        fr += quiet(c, [t], rng)

    def also(o, ev):
        assert DEEP_V * 120 >= FRAG_FAST_MAXV and tile_census(ev)[0][gt(S0, 1)] == 0
        e, cols = o.get_intervals(-1, S0)
        idx = np.flatnonzero((e[:-1].astype(np.int64) >> TB) == 2)
        v = cols["expt"]
        assert e[idx[0]] == f and e[idx[0] - 1] == s0 and v[idx[0]] == DEEP_V          # the first interval: `before` = carry
        assert (v[idx[1]:idx[-1] + 2] * 120 < FRAG_FAST_MAXV).all() and v[idx[1]] == DEEP_V - DEEP_DROP   # every `after` of the tile
        prod = DEEP_LEN * DEEP_V
        assert prod >= 1 << 24 and float(np.float32(DEEP_LEN) * np.float32(DEEP_V)) != prod
        assert cols["p"][idx[0]] > 2.0
        pk = o.get_peaks()
        assert ((pk["chrom"] == S0) & (pk["start"] < f) & (pk["end"] >= f)).any()
    return dict(frags=fr, chrom=S0, tile=2, want=(DEEP_DROP + 6, 7, 7), also=also)


def case_stream(stream, k):
    """k_tile_fast's registers hold 128 keys of EACH stream: 64 touched bases (32 starts, 32 ends), and k - 32 more starts on the
    lowest start (their ends in the next tile) or k - 32 more ends on the LOWEST end (their starts in the tile before; on the
    tile's last touched base a wrong difference would change no interval: `before` is the scan minus the base's own difference).
    The background is thin and uniform here, so that no other tile of the input has a key beyond the registers either."""
    p0 = 2 * TILE
    fr = stairs(S0, np.random.default_rng(40 + k).choice(np.arange(p0 + 8, p0 + TILE - 8), 64, replace=False), spill=0)
    a0, b0 = min(f[1] for f in fr), min(f[2] for f in fr)
    if stream == "S":
        fr += [(S0, a0, p0 + TILE + 340 + (i % 4), 1) for i in range(k - 32)]
    else:
        fr += [(S0, p0 - 900 + (i % 4), b0, 1) for i in range(k - 32)]
    b = _std(S0, 2, fr, (32 + k, 64, 64), np.random.default_rng(41 + k))
    b["streams"] = (k, 32) if stream == "S" else (32, k)
    b["background"] = dict(n=500, uniform=True)

    def also(o, ev):
        _, _, nS, nE = tile_census(ev)
        g = gt(S0, 2)
        assert max(np.delete(nS, g).max(), np.delete(nE, g).max()) < TF_REG_KEYS
    b["also"] = also
    return b


def case_sig(residue):
    """The sweep's significance bits, written in loose-slot index space: a plateau of more than 128 consecutive significant
    intervals in a tile whose first loose slot is = residue mod 64 (fragments that start in the tile before and end in the tile
    behind pad the keys before the tile)."""
    p0 = 2 * TILE
    rng = np.random.default_rng(36)
    fr = [(S0, p0 + 50 + i, p0 + 3650 + i, 1) for i in range(400)]
    fr += stairs(S0, rng.choice(np.arange(p0 + 500, p0 + 3600), 300, replace=False), spill=0, depth=2)
    base = _std(S0, 2, fr, None, np.random.default_rng(37))
    pad = (residue - first_slot(np.concatenate([rows(base["frags"]), background(1700)]), S0, 2)) % 64
    base["frags"] += [(S0, TILE + 50 + (i % 2), 3 * TILE + 50 + (i % 2), 1) for i in range(pad)]
    base["want"] = (1100, 1100, 1100)

    def also(o, ev, mode="p"):
        assert first_slot(ev, S0, 2) % 64 == residue
        e, cols = o.get_intervals(-1, S0)
        idx = np.flatnonzero((e[:-1].astype(np.int64) >> TB) == 2)
        assert (MODES["q"]["pq"], MODES["p"]["pq"]) == (0.5, 0.01)
        key, thr = ("q", np.float32(-np.log10(0.5))) if mode == "q" else ("p", np.float32(2.0))   # (-q 0.5, -p 0.01)
        sig = cols[key][idx] > thr
        print("plateau", mode, float(cols[key][idx].min()), float(cols[key][idx].max()))
        run = best = 0
        for s in sig:
            run = run + 1 if s else 0
            best = max(best, run)
        assert best > 128, best
    base["also"] = also
    return base


CASES = {}
for _n in (64, 65, 127, 128, 129, 191, 192, 193, 200, 201, 4095, 4096, 4097):
    CASES[f"keys-n{_n}"] = (case_keys, (_n,))
T_VALUES = (1, 63, 64, 65, 383, 384, 385, 447, 448, 449, 511, 512, 513, 896, 897, 1024, 1025)
for _t in T_VALUES:
    CASES[f"touched-T{_t}"] = (case_touched, (_t,))
CASES["full"] = (case_full, (0,))
CASES["full-plus-one"] = (case_full, (1,))
for _k in CANCEL_KINDS:
    CASES[f"cancel-{_k}"] = (case_cancel, (_k,))
CASES["cancel-all"] = (case_cancel_all, ())
for _t in (1, 64, 65, 448, 449):
    CASES[f"base0-T{_t}"] = (case_base0, (_t,))
CASES["seams"] = (case_seams, ())
CASES["chrom-end"] = (case_chrom_end, ())
for _t in (448, 449):
    CASES[f"long-T{_t}"] = (case_long, (_t, False))
    CASES[f"cross-T{_t}"] = (case_long, (_t, True))
CASES["empty-between"] = (case_empty_between, ())
for _k in ("tile", "bin"):
    CASES[f"carry-{_k}"] = (case_carry, (_k,))
CASES["carry-deep"] = (case_carry_deep, ())
for _s in "SE":
    for _k in (TF_REG_KEYS, TF_REG_KEYS + 1):
        CASES[f"stream-n{_s}{_k}"] = (case_stream, (_s, _k))
for _r in (0, 1, 63):
    CASES[f"sig-r{_r}"] = (case_sig, (_r,))
# the weighted ones: the eight counts cycle through the stairs
W_CASES = {f"w-touched-T{_t}": (case_touched, (_t, True)) for _t in (447, 448, 449, 896, 897)}
W_CASES.update({f"w-cancel-{_k}": (case_cancel, (_k, True)) for _k in CANCEL_KINDS if _k != "first"})   # (rank 0 there: the 511-base fragment's start)
W_CASES["w-cancel-all"] = (case_cancel_all, (True,))
W_CASES["w-full"] = (case_full, (0, True))
W_CASES["w-unequal"] = (case_unequal, ())
ALL = {**CASES, **W_CASES}
T_AND_CANCEL = sorted(k for k in CASES if k.startswith(("touched-", "cancel-", "full")))


@functools.lru_cache(maxsize=None)
def _built(name):
    fn, args = ALL[name]
    return fn(*args)


@functools.lru_cache(maxsize=None)
def _oracle(name, mode="p", bed=False):
    """the reference of a case: computed once, shared by the oracle-only test and the GPU tests, left unchanged"""
    b = _built(name)
    ev = np.concatenate([rows(b["frags"]), background(1700, **b.get("background", {}))])
    case = dict(lens=LENS, beds=[[], [], [], [100, 200]] if bed else None, replicates=[dict(save=None, treat=ev, ctrl=None)])
    params, o, so = run_oracle(case, mode)
    return b, ev, case, params, o, so


def check(name, mode="p", bed=False):
    b, ev, case, params, o, so = _oracle(name, mode, bed)
    n, T, nS, nE = tile_census(ev)
    g = gt(b["chrom"], b["tile"])
    if "streams" in b:
        assert (int(nS[g]), int(nE[g])) == b["streams"], (name, nS[g], nE[g])
    out = int(tile_counts(o.get_intervals(-1, b["chrom"])[0], LENS[b["chrom"]])[b["tile"]])
    got = (int(n[g]), int(T[g]), out)
    assert got == b["want"], (name, got, b["want"])
    # the tile under test is the only one of the stair chromosomes at a limit or one past it
    for c in (S0, S1):
        for t in range(NT[c]):
            if (c, t) != (b["chrom"], b["tile"]):
                assert int(n[gt(c, t)]) not in AT and int(T[gt(c, t)]) not in AT and n[gt(c, t)] <= SBT_HEAVY, (name, c, t, n[gt(c, t)], T[gt(c, t)])
                assert not {int(nS[gt(c, t)]), int(nE[gt(c, t)])} & {TF_REG_KEYS, TF_REG_KEYS + 1}, (name, c, t)
    assert n[gt(NOBODY, 0)] == n[gt(NOBODY, 1)] == 0 and len(o.get_intervals(-1, NOBODY)[0]) == (3 if bed else 1)
    if b["also"]:
        if name.startswith("sig-"):
            b["also"](o, ev, mode)
        else:
            b["also"](o, ev)
    assert o.n_peaks > 0
    return got


@pytest.mark.parametrize("name", sorted(ALL))
def test_tile_preconditions_on_the_oracle_alone(name):
    print(name, check(name))


def test_the_cases_lie_exactly_at_and_one_past_every_limit():
    n_of = {_built(k)["want"][0] for k in CASES if k.startswith("keys-")}
    t_of = {_built(k)["want"][1] for k in CASES if k.startswith("touched-")}
    for lim in (STEP, REG_KEYS, KEY_SLACK, SBT_PEAK_KEYS, SBT_HEAVY, HEAVY_MIN):
        assert {lim, lim + 1} <= n_of, lim
    streams = [_built(k)["streams"] for k in CASES if k.startswith("stream-")]   # per stream: k_tile_fast's registers
    assert {TF_REG_KEYS, TF_REG_KEYS + 1} <= {a for a, _ in streams} and {TF_REG_KEYS, TF_REG_KEYS + 1} <= {b for _, b in streams}
    for lim in (STEP, SBT_TR_DENSE, SBT_TR, TF_TR_CAP, 2 * SBT_TR, 2 * TF_TR_CAP):
        assert {lim, lim + 1} <= t_of, lim
    assert _built("full")["want"] == (TILE, TILE, TILE) and _built("full-plus-one")["want"] == (SBT_HEAVY + 1, TILE, TILE)
    assert -(-TILE // SBT_TR) == 10 and -(-TILE // TF_TR_CAP) == 8
    for k, (T, ranks) in CANCEL_KINDS.items():
        assert _built(f"cancel-{k}")["want"][2] == T - len(ranks)
    assert _built("cancel-all")["want"][1:] == (50, 0)
    u = _built("w-unequal")["want"]
    assert u[1] - u[2] == 3   # three equal pairs do not emit, the three unequal ones do


# (switch, -E region on the chromosome nobody touches): the tile kernels' instances
PATHS = {"default": ({}, False),                          # k_sbtile<PAIRS>: pair records, fused
         "start-end-keys": ({"GX_NO_PAIRS": "1"}, False),  # k_sbtile<false, ..>: the start and end key instance (one wavefront whatever n)
         "general-chain": ({"GX_NO_FUSED": "1"}, False),   # k_tile_fast / k_tile_heavy
         "bed-instance": ({}, True),                       # k_sbtile<.., BED>: ordinary tiles of the -E instance
         "one-workgroup": ({"GX_SBT_GRID": "1"}, False)}   # one persistent workgroup takes every bin


def _run(monkeypatch, name, path, mode="p", frac=False):
    env, bed = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    check(name, mode, bed)
    b, ev, case, params, o, so = _oracle(name, mode, bed)
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
@pytest.mark.parametrize("path", ["default", "start-end-keys", "general-chain"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_tile_stage_at_its_limits(monkeypatch, name, path):
    flags = _run(monkeypatch, name, path)
    assert bool(flags & FUSED) == (path != "general-chain") and not flags & FELL_BACK, flags
    assert bool(flags & PAIRS) == (path == "default"), flags
    if name.startswith("sig-"):
        assert flags & LOOSE, flags   # (-p on one replicate: the sweep walks the loose slots and reads the tile stage's bits)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["bed-instance", "one-workgroup"])
@pytest.mark.parametrize("name", T_AND_CANCEL)
def test_tile_stage_in_the_bed_instance_and_with_one_workgroup(monkeypatch, name, path):
    flags = _run(monkeypatch, name, path)
    assert flags & FUSED and flags & PAIRS and not flags & FELL_BACK, flags
    # (without regions the sweep usually walks the loose slots; a table entry next to the threshold sends a run to the tight table --
    # riskNearThr, gx_host_build.h:690 --, so LOOSE is asserted where a case is about it: the sig-* cases)
    # gx_path_info has no bit for the instance of k_sbtile that ran (as in test_hip_sbt_instances.py): that the -E instance took these
    # tiles follows from the host's table alone (a run with regions launches <.., BED>, gx_host_build.h SBT_INSTANCES); what the flags
    # show of it is that lambda came late, so the loose slots are not swept
    assert not (flags & LOOSE and path == "bed-instance"), flags


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["default", "start-end-keys", "general-chain"])
@pytest.mark.parametrize("name", ["sig-r0", "sig-r1", "sig-r63"])
def test_significance_bits_with_q_values(monkeypatch, name, path):
    flags = _run(monkeypatch, name, path, mode="q")
    assert bool(flags & FUSED) == (path != "general-chain") and not flags & FELL_BACK, flags


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["default", "general-chain"])
@pytest.mark.parametrize("name", sorted(W_CASES))
def test_tile_stage_with_the_eight_weights(monkeypatch, name, path):
    """(Two paths: the start and end key instance cannot carry a weight -- fracOk, gx_host_build.h:160-165 --, so with GX_NO_PAIRS
    an announced fractional sample is planned on the general chain from the start and would only repeat the GX_NO_FUSED run.)"""
    flags = _run(monkeypatch, name, path, frac=True)
    if path == "default":
        assert flags & FUSED and flags & PAIRS and flags & FRAC_PAIRS and not flags & FELL_BACK, flags
    else:
        assert not flags & FUSED and not flags & FRAC_PAIRS and not flags & FELL_BACK, flags


# ---- TR = 384: the dense launch's small instance ------------------------------------------------------------------------
# A sample that is dense by the host's own rule (plan_build, gx_host_build.h:178-226; the arithmetic: test_hip_sbt_instances.py's
# docstring): 71 tiles, bins halved to 18 of four tiles, 422,208 < nEv <= 449,856 -- the average bin fits the key array in one
# round at TR = 384 and needs two at 448.  The generator's fragments are taken out of the constructed tile and its two
# neighbours, so the tile holds what the case put there and nothing else.
D_LENS = [200_000, 90_000]
D_TILE = 20
D_CASES = {"dense-T383": (SBT_TR_DENSE - 1, ()), "dense-T384": (SBT_TR_DENSE, ()), "dense-T385": (SBT_TR_DENSE + 1, ()),
           "dense-cancel-round": CANCEL_KINDS["round384"]}


@functools.lru_cache(maxsize=None)
def _dense_background():
    import synth
    ev = synth.make_fragments(D_LENS, 462_000, 63, peak_every=20_000, frac_tower=0.0)
    lo, hi = (D_TILE - 1) * TILE, (D_TILE + 2) * TILE
    near = (ev["chrom"] == 0) & (ev["end"] > lo) & (ev["start"] < hi)
    return ev[~near]


@functools.lru_cache(maxsize=None)
def _dense_oracle(name):
    T, ranks = D_CASES[name]
    fr, want = make_tile(0, D_TILE, T, cancel=ranks, seed=9, lens=D_LENS)
    ev = np.concatenate([rows(fr), _dense_background()])
    case = dict(lens=D_LENS, replicates=[dict(save=None, treat=ev, ctrl=None)])
    params, o, so = run_oracle(case, "p")
    return ev, want, case, params, o, so


def check_dense(name):
    from test_hip_sbt_instances import _check_sizing
    ev, want, case, params, o, so = _dense_oracle(name)
    assert 2 * len(ev) > 9 * (KEYCAP - KEYCAP // 10)   # bins of half the size: 18 of them (gx_host_build.h:179)
    _check_sizing(len(ev), 18)
    n, T = tile_census(ev, D_LENS)[:2]
    out = int(tile_counts(o.get_intervals(-1, 0)[0], D_LENS[0])[D_TILE])
    assert (int(n[D_TILE]), int(T[D_TILE]), out) == want, (n[D_TILE], T[D_TILE], out, want)
    assert T[D_TILE - 1] < 64 and T[D_TILE + 1] < 64
    assert o.n_peaks > 0
    return want


@pytest.mark.parametrize("name", sorted(D_CASES))
def test_dense_preconditions_on_the_oracle_alone(name):
    print(name, check_dense(name))


@pytest.mark.gpu
@pytest.mark.parametrize("tr", [SBT_TR_DENSE, SBT_TR])
@pytest.mark.parametrize("name", sorted(D_CASES))
def test_tile_stage_in_the_dense_launch(monkeypatch, name, tr):
    monkeypatch.setenv("GX_SBT_TR", str(tr))   # (read when the context is made)
    check_dense(name)
    ev, want, case, params, o, so = _dense_oracle(name)
    h = hip_backend(params)
    sh = B.run_case(h, case)
    flags = h.path_info()
    assert_same_run(o, h, so, sh, case)
    assert flags & FUSED and flags & PAIRS and not flags & FELL_BACK, flags
