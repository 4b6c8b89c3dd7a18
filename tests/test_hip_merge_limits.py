"""The control merge (savePval: k_merge2w / k_merge2) and the replicate merge (combinePval + multPval: k_mergeN_w<4>,
k_mergeN_w<8>, k_mergeN) of genrich_amd/csrc/gx_merge.h at their internal limits, on constructed tiles.

Every kernel works tile by tile (4096 bp) and changes its path past a threshold: the number of replicates picks the kernel
(combine_replicates, gx_host_stats.h), the intervals of one input in a tile decide whether its values are staged in LDS or
gathered from global memory (MNW_SCAP, M2W_CAP, MG_CAP), and the merged intervals of a tile are listed by rank one round at a
time (MNW_CAP, M2W_ROUND, MN_CAP), later rounds relying on an unsigned wrap of `rank = exU - r0`.  The cases below put a few
hundred hand-placed "stairs" (fragments with distinct starts and distinct ends: 2k breakpoints for k fragments) into chosen
tiles, and every case ASSERTS FROM THE ORACLE'S ARRAYS on which side of which limit it is -- so the preconditions hold (and are
run: test_*_preconditions_on_the_oracle_alone) on a machine without a GPU.  An interval belongs to the tile of its end
(`end >> 12`: `off = end - pos0` indexes the tile's bitmap), and the chromosome's closing interval (end == len) is handled
apart by lane / thread 0 and not counted (a1c in all five kernels; with len a multiple of 4096 its end lies beyond the last tile).
Oracle and library are compared by assert_same_run: interval ends, p, q bit for bit and the peaks as bytes, for every
replicate's array and for the combined one.

What the suite crossed before this module, counted with the oracle alone (the largest count of any tile; the synthetic streams
pile a third of their fragments onto a few peak centres, so their densest tiles are far denser than the average):

  existing GPU test                                        | intervals per input and tile  | merged per tile
  test_hip_parity::test_crowded_tile_takes_the_chunked_... | treatment 2,286, control 232  | 2,287
  test_hip_paths::test_control_merge_...[plain / bed]      | treatment 963, control 727    | 1,303
  test_hip_paths::test_control_merge_...[multimap]         | treatment 1,522, control 987  | 1,954
  test_hip_paths::test_control_merge_...[deep]             | treatment 831, control 727    | 1,182
  test_hip_parity::test_bh_table_grows_when_full           | treatment 1,343, control 1,140 | 1,819
  test_hip_parity::test_random_with_control_q              | treatment 1,041, control 834  | 1,440
  test_hip_parity::test_many_distinct_pvalues_... (3 replicates) | 1,510 per replicate     | 2,522
  test_hip_parity::test_random_three_replicates            | 1,377 per replicate           | 2,371
  test_hip_parity::test_random_runs_against_oracle (40 seeds) | 1,050 per replicate        | 1,795 (replicates), 1,487 (control)
  golden reps3 / reps3_p_missing / nopeaks_log             | 446 / 359 / 278 per replicate | 797 / 576 / 377
  (test_hip_fullsize::test_midsize_slice_against_oracle and the "deep" kinds without a control run no merge kernel)

So the unstaged gathers of k_mergeN_w<4> (MNW_SCAP) and of k_merge2w (M2W_CAP, either input) and several rounds of their rank
lists (MNW_CAP, M2W_ROUND) HAD run, by the density of the generator and without any test saying so.  Never crossed before:
  * every replicate count above three: k_mergeN_w<8>, all of k_mergeN (and MN_CAP with it), and the refusal of more than 32;
  * MG_CAP: k_merge2 only ran under GX_MERGE_WG in test_hip_ties, on tiles far below 1,024 intervals;
  * a count exactly at a limit or one past it (320 / 321, 384 / 385, 1024 / 1025, 256 / 257, 512 / 513);
  * a full tile: 4,096 merged intervals (the 16-bit prefix counts at their largest, 16 rounds); the most was 2,522;
  * a crowded tile in which one input alone is past its limit with the other one nearly empty, with the value behind the
    crowded input's last breakpoint in use and asserted to matter.

That the cases see what they claim was checked once with scratch builds of the library, one branch broken each: the unstaged
gather of k_mergeN_w reading idx + 1 failed staging-*-over / -lone, rounds-n2-u4096 and skip-* and nothing else; the same in
k_mergeN failed exactly the cases with nine replicates or more; a wrong staged tail value (sP[r][nR]) failed every case of
eight replicates or fewer; k_merge2w's nvA dropped failed the kinds above 384 on the three loose paths and none on tight
inputs; k_merge2's nvB dropped failed treat-1025 / ctrl-1025 / treat-full on the workgroup path alone; prefix counts that
stop at 4095 failed treat-full / ctrl-full alone; ranks that do not wrap in later rounds failed nearly everything.
"""
import functools

import numpy as np
import pytest

import backends as B
import synth
from test_hip_parity import assert_same_run, hip_backend

# ---- the kernels' limits (genrich_amd/csrc/gx_merge.h; the replicate counts: combine_replicates, gx_host_stats.h) ----
TB = 12                 # GX_TB
TILE = 1 << TB          # breakpoints a tile's bitmap holds
MNW_SMALL = 4           # k_mergeN_w<4> takes up to four replicates,
MNW_MAXREP = 8          # k_mergeN_w<8> up to eight,
MAX_REPS = 32           # k_mergeN up to 32 (its LDS: mergeN_lds_bytes(n)); beyond: GX_ERR_DF
MNW_SCAP = 320          # k_mergeN_w: intervals per replicate and tile whose p-values are staged in LDS
MNW_CAP = 256           # k_mergeN_w: merged intervals listed per round
MN_CAP = 512            # k_mergeN: merged intervals listed per round
M2W_CAP = 384           # k_merge2w: intervals per input and tile whose pileups are staged in LDS
M2W_ROUND = 256         # k_merge2w: merged intervals listed per round
MG_CAP = 1024           # k_merge2 (GX_MERGE_WG): intervals per input and tile staged in LDS
GX_ERR_DF = -9
GX_SKIP = np.float32(-1.0)
FUSED, FELL_BACK, MERGE_P = 1, 4, 1024   # gx_path_info bits (tests/test_hip_paths.py)

# two chromosomes of stairs -- one whose length is a multiple of the tile (its closing interval ends beyond the last tile's
# bitmap), one whose length is not --, one with an ordinary background (lambda, peaks), one that no replicate has
S0, S1, BG, NOBODY = 0, 1, 2, 3
LENS = [4 * TILE, 3 * TILE + 1000, 60_000, 5_000]
MODES = {"p": dict(pq=0.01, qval=False, min_auc=20.0), "q": dict(pq=0.5, qval=True, min_auc=5.0)}   # (peaks in every case, both ways)


def saw(chrom, pos, depth=16, count=1):
    """Fragments whose starts and ends are exactly the distinct positions `pos` (an odd count is made even by one more
    position in the chromosome's first tile): sorted, in groups of 2 * depth -- the first half starts, the second half ends --,
    so the pileup climbs to `depth` and comes down again and neighbouring intervals differ in p."""
    pos = np.asarray(pos, dtype=np.int64)
    assert len(np.unique(pos)) == len(pos) and pos.min() > 0
    if len(pos) % 2:
        pad = next(q for q in range(9, TILE, 2) if q not in set(pos.tolist()))
        pos = np.append(pos, pad)
    pos = np.sort(pos)
    rows = []
    for a in range(0, len(pos), 2 * depth):
        ch = pos[a:a + 2 * depth]
        m = len(ch) // 2
        rows += [(chrom, int(s), int(e), count) for s, e in zip(ch[:m], ch[m:])]
    return np.array(rows, dtype=B.EVENT_DTYPE)


def background(seed, n=1200, uniform=False):
    """an ordinary stream on the third chromosome, enriched enough for p and q to take hundreds of values and for peaks in -q"""
    ev = synth.make_fragments([LENS[BG]], n, seed, uniform_only=True) if uniform else \
        synth.make_fragments([LENS[BG]], n, seed, peak_every=8_000, tower_every=30_000, frac_peak=0.5, frac_tower=0.2)
    ev["chrom"] = BG
    return ev


def in_tile(chrom, tile, lo=0, hi=TILE):
    """the positions [lo, hi) of a tile that can be interval ends (not 0, not the chromosome's end or beyond)"""
    a = np.arange(tile * TILE + lo, min(tile * TILE + hi, LENS[chrom]))
    return a[a > 0]


def tile_counts(end, clen):
    """intervals per tile as the merge kernels count them: by the tile of the end, the closing interval left out"""
    n = (clen + TILE - 1) >> TB
    if len(end) == 0:
        return np.zeros(n, dtype=np.int64)
    assert end[-1] == clen
    return np.bincount(end[:-1].astype(np.int64) >> TB, minlength=n)


def ends_in(end, clen, tile):
    e = end[:-1].astype(np.int64)
    return e[(e >> TB) == tile]


def run_oracle(case, mode):
    params = B.make_params(**MODES[mode])
    o = B.Oracle(params)
    return params, o, B.run_case(o, case)


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


# =====================================================================================================================
# the replicate merge
# =====================================================================================================================

def _kernel_of(n):
    return "k_mergeN_w<4>" if n <= MNW_SMALL else "k_mergeN_w<8>" if n <= MNW_MAXREP else "k_mergeN" if n <= MAX_REPS else None


def _rep(treat_parts, save, ctrl=None):
    return dict(save=save, treat=np.concatenate(treat_parts), ctrl=ctrl)


def _control_for_a_replicate(seed):
    """a control of its own: uniform background, and a few stairs on the first stair chromosome"""
    rng = np.random.default_rng(seed)
    return np.concatenate([background(seed, 500, uniform=True), saw(S0, rng.choice(in_tile(S0, 1), 30, replace=False), depth=4)])


def build_count(n):
    """n replicates on one moderately crowded genome: ~60 breakpoints per replicate in one tile, stairs in both last tiles; the
    last replicate lacks the second stair chromosome, nobody has the fourth chromosome, and from five replicates on one has
    a control."""
    rng = np.random.default_rng(100 + n)
    reps = []
    for r in range(n):
        has_s1 = r != n - 1
        parts = [background(1000 + r),
                 saw(S0, np.concatenate([rng.choice(in_tile(S0, 1), 60, replace=False), rng.choice(in_tile(S0, 2), 30, replace=False),
                                         rng.choice(in_tile(S0, 3), 20, replace=False)]))]
        if has_s1:
            parts.append(saw(S1, np.concatenate([rng.choice(in_tile(S1, 1), 40, replace=False), rng.choice(in_tile(S1, 3), 20, replace=False)])))
        reps.append(_rep(parts, [True, has_s1, True, False], _control_for_a_replicate(2000 + r) if n >= 5 and r == 1 else None))
    case = dict(lens=LENS, replicates=reps)

    def check(o):
        assert len(case["replicates"]) == n and _kernel_of(n) == \
            {2: "k_mergeN_w<4>", 4: "k_mergeN_w<4>", 5: "k_mergeN_w<8>", 8: "k_mergeN_w<8>", 9: "k_mergeN", 16: "k_mergeN", 32: "k_mergeN"}[n]
        assert (n <= MNW_SMALL) == (n in (2, 4)) and (n <= MNW_MAXREP) == (n in (2, 4, 5, 8)) and n <= MAX_REPS
        for w in [-1] + list(range(n)):
            assert len(o.get_intervals(w, NOBODY)[0]) == 0          # `any == false` on its tiles
        assert len(o.get_intervals(n - 1, S1)[0]) == 0 and len(o.get_intervals(0, S1)[0]) > 0   # the `save` mask
        for c in (S0, S1):                                          # stairs in both last tiles, in every replicate that is there
            for r in range(n - (c == S1)):
                assert tile_counts(o.get_intervals(r, c)[0], LENS[c])[3] >= 20
        u = tile_counts(o.get_intervals(-1, S0)[0], LENS[S0])
        assert u[1] > 50 * min(n, 8)
        if n >= 16:
            assert u[1] > MN_CAP   # (the general kernel in more than one round, at its largest LDS for n = 32)
        return dict(union=u.tolist())

    return case, check


def build_staging(n, kind):
    """One replicate with exactly MNW_SCAP (`at`), MNW_SCAP + 1 (`over`) or 600 (`lone`) intervals in a tile, the others below 100
    -- in a tile that is not its chromosome's last and in one that is.  The others have breakpoints behind the crowded
    replicate's last one, so that its value behind that breakpoint (sP[r][nR], or the global read of the unstaged branch: the
    next tile's first interval, or the closing one) is used, and it differs from the value before."""
    K = dict(at=MNW_SCAP, over=MNW_SCAP + 1, lone=600)[kind]
    crowded = 1
    rng = np.random.default_rng(300 + n)
    reps = []
    for r in range(n):
        if r == crowded:
            s0 = in_tile(S0, 1)[100:100 + 3 * K:3]
            s1 = in_tile(S1, 3)[10:10 + K]
        else:
            s0 = np.concatenate([rng.choice(in_tile(S0, 1, 0, 2000), 20 + 5 * r, replace=False), rng.choice(in_tile(S0, 1, 2000), 20, replace=False)])
            s1 = np.concatenate([rng.choice(in_tile(S1, 3, 0, 650), 25, replace=False), rng.choice(in_tile(S1, 3, 650, 995), 15, replace=False)])
        s0 = np.concatenate([s0, rng.choice(in_tile(S0, 2, 40), 12, replace=False)])   # the next tile's first interval: its own value
        reps.append(_rep([background(1100 + r), saw(S0, s0), saw(S1, s1)], [True, True, True, False]))
    case = dict(lens=LENS, replicates=reps)

    def check(o):
        assert _kernel_of(n) == {3: "k_mergeN_w<4>", 6: "k_mergeN_w<8>"}[n]
        seen = {}
        for c, t in ((S0, 1), (S1, 3)):
            per = [int(tile_counts(o.get_intervals(r, c)[0], LENS[c])[t]) for r in range(n)]
            assert per[crowded] == K == max(per) and all(x < 100 for k, x in enumerate(per) if k != crowded), per
            assert (max(per) <= MNW_SCAP) == (kind == "at")          # staged exactly then
            e, cols = o.get_intervals(crowded, c)
            last = int(np.flatnonzero((e[:-1].astype(np.int64) >> TB) == t)[-1])
            union = ends_in(o.get_intervals(-1, c)[0], LENS[c], t)
            assert union.max() > e[last], "no merged interval lies behind the crowded replicate's last breakpoint"
            assert bits(cols["p"])[last + 1] != bits(cols["p"])[last], "the value behind the last breakpoint does not matter"
            assert (e[last + 1] == LENS[c]) == (t == 3)              # (the closing interval, in the last tile)
            seen[(c, t)] = per
        return seen

    return case, check


def build_rounds(n, U):
    """The union of the replicates' breakpoints in one tile is exactly U: 256 / 257 around one round of k_mergeN_w, 512 / 513 two
    rounds and the start of a third (and around MN_CAP for nine replicates), 4096 the whole bitmap (16 rounds / 8 rounds: a wrong
    wrap of `exU - r0` in a later round shows here)."""
    rng = np.random.default_rng(500 + U)
    pos = in_tile(S0, 2)[np.sort(rng.choice(TILE, U, replace=False))]
    reps = []
    for r in range(n):
        extra = np.concatenate([rng.choice(in_tile(S0, 3), 10, replace=False), rng.choice(in_tile(S0, 1), 10, replace=False)])
        reps.append(_rep([background(1200 + r), saw(S0, np.concatenate([pos[r::n], extra])),
                          saw(S1, rng.choice(in_tile(S1, 3), 10, replace=False))], [True, True, True, False]))
    case = dict(lens=LENS, replicates=reps)

    def check(o):
        assert _kernel_of(n) == {2: "k_mergeN_w<4>", 9: "k_mergeN"}[n]
        u = int(tile_counts(o.get_intervals(-1, S0)[0], LENS[S0])[2])
        assert u == U
        cap = MNW_CAP if n <= MNW_MAXREP else MN_CAP
        rounds = -(-u // cap)
        assert rounds == {(2, 256): 1, (2, 257): 2, (2, 512): 2, (2, 513): 3, (2, 4096): 16,
                          (9, 256): 1, (9, 257): 1, (9, 512): 1, (9, 513): 2, (9, 4096): 8}[(n, U)]
        per = max(int(tile_counts(o.get_intervals(r, S0)[0], LENS[S0])[2]) for r in range(n))
        if n == 2:
            assert (per <= MNW_SCAP) == (U <= 513)   # rounds on the staged branch, and (4096) on the unstaged one
        return dict(union=u, rounds=rounds, per=per)

    return case, check


SKIP_BEDS = [TILE + 600, TILE + 620, TILE + 900, TILE + 950, TILE + 1300, TILE + 1400, TILE + 2000, TILE + 2100]


def build_skip(n):
    """-E regions inside a crowded tile.  SKIP comes from the regions alone (saveLambda / savePileupCtrl write it for a
    replicate with and without a control alike, Genrich.c:1838-1877, 2122-2140), so the number of p-values that enter
    multPval (df / 2) changes between neighbouring merged intervals of one wavefront at the regions' edges, 0 <-> the replicates
    that have the chromosome; one replicate has a control, one lacks the chromosome."""
    rng = np.random.default_rng(700 + n)
    reps = []
    for r in range(n):
        has_s0 = r != 2
        parts = [background(1300 + r), saw(S1, rng.choice(in_tile(S1, 1), 30, replace=False))]
        if has_s0:
            parts.append(saw(S0, np.concatenate([rng.choice(in_tile(S0, 1, 300, 2600), 200, replace=False),
                                                 rng.choice(in_tile(S0, 3), 10, replace=False)])))
        reps.append(_rep(parts, [has_s0, True, True, False], _control_for_a_replicate(2300 + r) if r == 1 else None))
    case = dict(lens=LENS, beds=[SKIP_BEDS, [], [], []], replicates=reps)

    def check(o):
        e, cols = o.get_intervals(-1, S0)
        idx = np.flatnonzero((e[:-1].astype(np.int64) >> TB) == 1)
        skip = cols["p"][idx] == GX_SKIP
        assert skip.sum() == len(SKIP_BEDS) // 2 and len(idx) > MNW_CAP
        flips = np.flatnonzero(skip[1:] != skip[:-1])
        assert len(flips) == len(SKIP_BEDS) and len(set((flips // 64).tolist())) < len(flips)   # SKIP and not within 64 neighbours
        assert len(o.get_intervals(2, S0)[0]) == 0
        for r in (0, 1):   # every replicate that is there skips the same intervals
            er, cr = o.get_intervals(r, S0)
            assert (cr["p"] == GX_SKIP).sum() == len(SKIP_BEDS) // 2
        return dict(merged=len(idx), skip=int(skip.sum()))

    return case, check


REP_CASES = {}
for _n in (2, 4, 5, 8, 9, 16, 32):
    REP_CASES[f"count-n{_n}"] = (build_count, (_n,))
for _n in (3, 6):
    for _k in ("at", "over", "lone"):
        REP_CASES[f"staging-n{_n}-{_k}"] = (build_staging, (_n, _k))
for _n in (2, 9):
    for _u in (256, 257, 512, 513, 4096):
        REP_CASES[f"rounds-n{_n}-u{_u}"] = (build_rounds, (_n, _u))
for _n in (3, 6):
    REP_CASES[f"skip-n{_n}"] = (build_skip, (_n,))


@functools.lru_cache(maxsize=None)
def _rep_case(name):
    fn, args = REP_CASES[name]
    return fn(*args)


@functools.lru_cache(maxsize=None)
def _rep_oracle(name, mode):
    """the reference of a case: computed once, shared by the oracle-only test and the GPU test, left unchanged"""
    case, check = _rep_case(name)
    params, o, so = run_oracle(case, mode)
    return case, check, params, o, so


@pytest.mark.parametrize("name", sorted(REP_CASES))
def test_replicate_merge_preconditions_on_the_oracle_alone(name):
    case, check, params, o, so = _rep_oracle(name, "p")
    print(name, check(o))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["p", "q"])
@pytest.mark.parametrize("name", sorted(REP_CASES))
def test_replicate_merge_at_its_limits(name, mode):
    case, check, params, o, so = _rep_oracle(name, mode)
    check(o)
    h = hip_backend(params)
    sh = B.run_case(h, case)
    assert_same_run(o, h, so, sh, case)
    assert o.n_peaks > 0


def _three_replicates():
    return dict(lens=LENS, replicates=[_rep([background(1400 + r), saw(S0, in_tile(S0, 1)[50 + r:1500:7])], None) for r in range(3)])


def test_33_replicates_are_what_the_case_holds():
    assert MAX_REPS + 1 == 33 and _kernel_of(MAX_REPS + 1) is None and _kernel_of(MAX_REPS) == "k_mergeN"


@pytest.mark.gpu
def test_more_than_32_replicates_are_refused_and_the_context_lives_on():
    """33 replicates: the combination fails with GX_ERR_DF and says why (gx_last_error); after gx_reset the same context
    completes an ordinary three-replicate run with the oracle's bits."""
    params = B.make_params(**MODES["p"])
    h = hip_backend(params)
    one = _rep([background(1500, 300), saw(S0, in_tile(S0, 1)[50:450:4])], None)
    with pytest.raises(RuntimeError) as ei:
        B.run_case(h, dict(lens=LENS, replicates=[one] * (MAX_REPS + 1)))
    assert f"error {GX_ERR_DF}:" in str(ei.value) and "more than 32 replicates" in str(ei.value), str(ei.value)
    assert h.lib.gx_last_error(h.ctx).decode() == "more than 32 replicates are not supported"
    h.reset()
    case = _three_replicates()
    _, o, so = run_oracle(case, "p")
    sh = B.run_case(h, case)
    assert_same_run(o, h, so, sh, case)
    assert h.n_peaks > 0


# =====================================================================================================================
# the control merge
# =====================================================================================================================

def _pedestal():
    """ten control fragments over the whole first stair chromosome: every control stair on it changes max(factor * pileup, lambda)"""
    return np.array([(S0, 1 + i, LENS[S0] - 1 - i, 1) for i in range(10)], dtype=B.EVENT_DTYPE)


def _split(rng, tile, nA, nB, late):
    """nA + nB distinct positions of a tile at random, the last three of them given to input `late` (0 treatment, 1 control):
    merged intervals lie behind the other input's last breakpoint"""
    body = rng.permutation(in_tile(S0, tile, 20, 4000))
    tail = in_tile(S0, tile)[[4050, 4060, 4070]]
    a, b = (nA - 3, nB) if late == 0 else (nA, nB - 3)
    A, Bc = body[:a], body[a:a + b]
    return (np.concatenate([A, tail]), Bc) if late == 0 else (A, np.concatenate([Bc, tail]))


CTRL_KINDS = {   # (treatment, control) intervals of the crowded tiles
    "both-at-384": (M2W_CAP, M2W_CAP), "both-at-385": (M2W_CAP + 1, M2W_CAP + 1),
    "treat-over": (600, 50), "ctrl-over": (50, 600),
    "both-at-1024": (MG_CAP, MG_CAP), "treat-1025": (MG_CAP + 1, 30), "ctrl-1025": (30, MG_CAP + 1),
    "union-256": (128, 128), "union-257": (129, 128), "union-4096": (TILE // 2, TILE // 2),
    "treat-full": (TILE, 48), "ctrl-full": (48, TILE),   # one input alone fills the bitmap: the packed prefix counts reach 4096
    "fractional": (450, 450),
}


def build_ctrl(kind, bed=False):
    """One replicate with a control.  Two neighbouring tiles of the first stair chromosome (neither its last) hold the counts of
    the kind, the treatment's and the control's breakpoints shuffled among each other; in the first the control has the last
    breakpoints (the treatment's pileup behind ITS last one -- the next tile's first slot: nvA / tailElsewhere on the loose
    inputs -- is used), in the second the treatment has.  bed: a -E region on the fourth chromosome, where nothing else is --
    with any region the two samples are merged from their tight arrays (stash_or_pack, gx_host_build.h: LOOSE == false).  The control stands on ten fragments there, so each of its breakpoints
    changes max(factor * pileup, lambda); on the second stair chromosome it has breakpoints where the scaled pileup stays
    below lambda (bits of bmC, not of bmB): the merged count must not include them."""
    nA, nB = CTRL_KINDS[kind]
    rng = np.random.default_rng(900 + nA * 7 + nB)
    if kind == "union-4096":
        every = in_tile(S0, 2)
        assert len(every) == TILE
        A1, B1 = _split(rng, 1, 300, 300, late=1)
        A2, B2 = every[0::2], every[1::2]
    elif kind in ("treat-full", "ctrl-full"):
        A1, B1 = _split(rng, 1, 300, 300, late=1)
        A2, B2 = in_tile(S0, 2), in_tile(S0, 2)[100:100 + 60 * nB if kind == "treat-full" else 100 + 60 * nA:60]
        if kind == "ctrl-full":
            A2, B2 = B2, A2
    else:
        A1, B1 = _split(rng, 1, nA, nB, late=1)
        A2, B2 = _split(rng, 2, nA, nB, late=0)
    count = 1
    treat = [background(1600, 3000), saw(S0, np.concatenate([A1, A2, rng.choice(in_tile(S0, 3), 20, replace=False)])),
             saw(S1, np.concatenate([rng.choice(in_tile(S1, 1, 0, 2000), 20, replace=False), rng.choice(in_tile(S1, 3), 20, replace=False)]))]
    ctrl = [background(1601, 500, uniform=True), _pedestal(), saw(S0, np.concatenate([B1, B2, rng.choice(in_tile(S0, 3), 16, replace=False)])),
            saw(S1, rng.choice(in_tile(S1, 1, 2000), 40, replace=False), depth=1),
            saw(S1, rng.choice(in_tile(S1, 3), 16, replace=False), depth=1)]
    if kind == "fractional":   # every third stair fragment is one of two alignments of its read (weight 1/2; the other on the background)
        for part in (treat, ctrl):
            st = part[1] if part is treat else part[2]
            st["count"][::3] = 2
            twin = st[::3].copy()
            twin["chrom"] = BG
            twin["start"] = rng.integers(100, LENS[BG] - 5000, len(twin))
            twin["end"] = twin["start"] + 150
            part.append(twin)
    beds = [[], [], [], [100, 200]] if bed else None
    case = dict(lens=LENS, beds=beds, replicates=[dict(save=None, treat=np.concatenate(treat), ctrl=np.concatenate(ctrl))])

    def check(o):
        alone = {}
        for key in ("treat", "ctrl"):   # the two pileups' own run-length arrays: each sample as a replicate without a control
            _, oa, _ = run_oracle(dict(lens=LENS, beds=beds, replicates=[dict(save=None, treat=case["replicates"][0][key], ctrl=None)]), "p")
            alone[key] = [oa.get_intervals(-1, c) for c in (S0, S1)]
        cA, cB = (tile_counts(alone[k][S0][0], LENS[S0]) for k in ("treat", "ctrl"))
        merged = [o.get_intervals(-1, c) for c in (S0, S1)]
        cU = tile_counts(merged[S0][0], LENS[S0])
        seen = dict(treat=cA.tolist(), ctrl=cB.tolist(), merged=cU.tolist())
        if kind == "union-4096":
            assert (cA[2], cB[2], cU[2]) == (TILE // 2, TILE // 2, TILE) and min(cA[2], cB[2]) > MG_CAP
        elif kind in ("treat-full", "ctrl-full"):
            assert (cA[2], cB[2], cU[2]) == (nA, nB, TILE) and max(nA, nB) == TILE
        elif kind == "fractional":
            assert min(cA[1], cB[1], cA[2], cB[2]) > M2W_CAP
            ex = alone["treat"][S0][1]["expt"]
            assert (ex[(alone["treat"][S0][0] >> TB) == 1] % 1 != 0).any()   # fractional pileups: p by k_pairs_missed, not the table
        else:
            assert (cA[1], cB[1]) == (nA, nB) == (cA[2], cB[2]), seen
            assert cU[1] == nA + nB == cU[2]                         # (disjoint, and every control breakpoint counts there)
        if kind.startswith("union"):
            assert cU[2] == int(kind.split("-")[1])
        for t, early, ekey in ((1, "treat", "expt"), (2, "ctrl", "expt")):   # the value behind the earlier input's last breakpoint
            if kind in ("union-4096", "ctrl-full") and t == 2:
                early = "treat"   # (the last position of the tile is the control's)
            e, cols = alone[early][S0]
            last = int(np.flatnonzero((e[:-1].astype(np.int64) >> TB) == t)[-1])
            assert ends_in(merged[S0][0], LENS[S0], t).max() > e[last]
            assert cols[ekey][last + 1] != cols[ekey][last] and (int(e[last + 1]) >> TB) > t   # the next tile's first slot differs
        # control breakpoints below lambda are no breakpoints of the merge
        both = np.union1d(ends_in(alone["treat"][S1][0], LENS[S1], 1), ends_in(alone["ctrl"][S1][0], LENS[S1], 1))
        got = ends_in(merged[S1][0], LENS[S1], 1)
        assert len(ends_in(alone["ctrl"][S1][0], LENS[S1], 1)) >= 40 and len(got) < len(both)
        assert np.array_equal(got, ends_in(alone["treat"][S1][0], LENS[S1], 1))
        return seen

    return case, check


@functools.lru_cache(maxsize=None)
def _ctrl_oracle(kind, mode, bed=False):
    case, check = build_ctrl(kind, bed)
    params, o, so = run_oracle(case, mode)
    return case, check, params, o, so


@pytest.mark.parametrize("bed", [False, True])
@pytest.mark.parametrize("kind", sorted(CTRL_KINDS))
def test_control_merge_preconditions_on_the_oracle_alone(kind, bed):
    case, check, params, o, so = _ctrl_oracle(kind, "p", bed)
    print(kind, check(o))


def test_control_kinds_lie_on_both_sides_of_every_limit():
    for cap in (M2W_CAP, MG_CAP):
        sides = {(a <= cap, b <= cap) for a, b in CTRL_KINDS.values()}
        assert sides == {(True, True), (True, False), (False, True), (False, False)}, cap
        assert (cap, cap) in CTRL_KINDS.values() and any(a == cap + 1 for a, _ in CTRL_KINDS.values()) and any(b == cap + 1 for _, b in CTRL_KINDS.values())
    unions = {a + b for k, (a, b) in CTRL_KINDS.items() if k.startswith("union")}
    assert unions == {M2W_ROUND, M2W_ROUND + 1, TILE}


# (switch, -E region): the kernel instances of launch_merge2 (gx_host_stats.h)
CTRL_PATHS = {"default": (None, False),                 # k_merge2w<LOOSE, PV>
              "general-chain": ("GX_NO_FUSED", False),  # ... on loose slots that the general tile chain wrote, not k_sbtile
              "pileups-out": ("GX_NO_MERGE_P", False),  # k_merge2w<LOOSE, false>: both pileups left to k_pack_pairs
              "workgroup": ("GX_MERGE_WG", False),      # k_merge2<LOOSE, PV>, with MG_CAP of its own
              "tight-inputs": (None, True),             # k_merge2w<false, PV>: tight arrays, no tailElsewhere
              "tight-workgroup": ("GX_MERGE_WG", True)}  # k_merge2<false, PV>


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["p", "q"])
@pytest.mark.parametrize("path", sorted(CTRL_PATHS))
@pytest.mark.parametrize("kind", sorted(CTRL_KINDS))
def test_control_merge_at_its_limits(monkeypatch, kind, path, mode):
    """Every kind on the four combinations the switches select and, for both kernels, on tight inputs (GX_NO_FUSED alone
    leaves the samples in loose slots: the merge reads tight arrays only when the run has -E regions)."""
    switch, bed = CTRL_PATHS[path]
    if switch:
        monkeypatch.setenv(switch, "1")
    case, check, params, o, so = _ctrl_oracle(kind, mode, bed)
    check(o)
    h = hip_backend(params)
    sh = B.run_case(h, case)
    flags = h.path_info()
    if kind != "fractional":   # (fractional weights among unit ones: the sample may be built again on the general chain)
        assert bool(flags & FUSED) == (path != "general-chain") and not flags & FELL_BACK, flags
    assert bool(flags & MERGE_P) == (path != "pileups-out"), flags
    assert_same_run(o, h, so, sh, case)
    assert o.n_peaks > 0
