"""The tile walk under the three passes over a closed sample's pileup (gx_pileup.h has the rule; k_cov_bins, k_depth_hist and
k_profile each walk it) at the limits of its 64-lane step, on constructed tiles: a tile that ends exactly n intervals, for n around
the multiples of 64, with the first piece clipped at the tile's start and a tail behind its last breakpoint; the same on a
chromosome's last tile (no tail) and next to a one-base last tile; in all three forms the pileup can be in when the sample is
closed.  Exact equality with coverage_ref, depth_ref and profile_ref, as in the passes' own modules.

n of a tile [pos0, tEnd) = the positions e, pos0 < e <= tEnd, at which the per-base pileup changes (pile[e - 1] != pile[e]) or
the chromosome ends (e == len): the ends of the intervals the tile ends (test_the_rule_for_n_is_the_interval_ends')."""
import numpy as np
import pytest

import backends as B
import coverage_ref as CR
import depth_ref as DR
import profile_ref as PR
from test_hip_coverage import LENS, PARAMS, _check as _check_coverage, _run
from test_hip_depth import _check as _check_depth
from test_hip_profile import _check as _check_profile

pytestmark = pytest.mark.gpu

TILE = 4096
# (chromosome, the tile under test, a fragment under the whole tile, a fragment that adds ONE breakpoint to the tile)
PLACES = [
    (0, (4096, 8192), (100, 12_000), (8000, 9000)),   # tile 1 of 4: the pileup is non-zero across both borders; the one breakpoint's
                                                      # fragment ends in tile 2
    (1, (0, 4096), (0, 4096), (0, 30)),               # the only tile: TM_LAST, it ends the chromosome-closing interval (n >= 1; at
                                                      # n = 1 that one alone, non-zero; the case n = 0 leaves it empty), no tail
    (2, (0, 4096), (0, 4097), (4000, 4097)),          # next to a one-base last tile, which ends both long fragments
]
assert [LENS[c] for c, *_ in PLACES] == [3 * TILE + 17, TILE, TILE + 1]
# (n, the last breakpoint is the tile's end: the tail piece is empty)
CASES = [(0, False), (1, False), (63, False), (64, False), (65, False), (127, False), (128, False), (64, True)]
BED_ELSEWHERE = [[], [], [], [], [1000, 2000]]        # one -E region on chromosome 4: hasBed, the tiles under test undisturbed
# coverage bin sizes (W < 8: several passes of COV_CAP bins over the tile), each with a profile class (flank, bin)
CONFIGS = [(1, 4096, 8), (7, 1000, 4), (50, 4096, 8), (4096, 1000, 4)]
# flank 4096: 2500 -> a window that ends inside tile 1 of chromosome 0 (the early exit), 6144 -> one over tiles 0 to 2; flank 1000:
# 5500 -> a window inside tile 1, 2000 -> inside the tiles of chromosomes 1 and 2; 0 and 4096: windows cut by a chromosome's ends
ANCHORS = np.asarray([(c, p, s) for c, ps in ((0, (2500, 5500, 6144)), (1, (0, 2000)), (2, (0, 2000, 4096))) for p in ps for s in (1, -1)],
                     dtype=PR.ANCHOR_DTYPE)


def _n_of(pile, length, pos0, t_end):
    e = np.arange(pos0 + 1, min(t_end, length) + 1)
    nxt = np.append(pile, 0)
    return int(((e == length) | (nxt[e - 1] != nxt[e])).sum())


def _tile_events(place, n, at_end):
    """Fragments that put exactly n breakpoints into the place's tile (None where n cannot be: a last tile has n >= 1)."""
    chrom, (pos0, t_end), under, one = place
    closing = 1 if t_end == LENS[chrom] else 0        # the chromosome-closing interval's end
    frags = [under]
    if at_end:                                        # [t_end - 50, t_end): a breakpoint at its start and one at t_end (on a last
        frags.append((t_end - 50, t_end))             # tile: the closing one)
        left = n - 2
    else:
        left = n - closing
    if left < 0:
        return None
    if left % 2:
        frags.append(one)
    frags += [(pos0 + 100 + 60 * i, pos0 + 120 + 60 * i) for i in range(left // 2)]   # disjoint, two breakpoints each, below 4000
    ev = np.zeros(len(frags), dtype=B.EVENT_DTYPE)
    ev["chrom"], ev["count"] = chrom, 1
    ev["start"], ev["end"] = [f[0] for f in frags], [f[1] for f in frags]
    return ev


_SAMPLES = {}


def _sample(n, at_end):
    """The case's events on all three places, its n per place as the reference pileup has it, and the references (made once)."""
    if (n, at_end) not in _SAMPLES:
        parts = [_tile_events(p, n, at_end) for p in PLACES]
        ev = np.concatenate([p for p in parts if p is not None])
        ev = ev[np.random.default_rng(n).permutation(len(ev))]
        piles = {c: CR.pileup120(ev, c, LENS[c]) for c in range(len(LENS))}
        ns = [_n_of(piles[c], LENS[c], *tile) for c, tile, *_ in PLACES]
        assert ns == [n, max(n, 1), n], (n, at_end, ns)        # what was intended (chromosome 1 without events: the closing interval)
        if at_end:
            assert all(piles[c][t_end - 1] != np.append(piles[c], 0)[t_end] for c, (_, t_end), *_ in PLACES)
        assert piles[0][4095] and piles[0][4096] and piles[0][8191] and piles[0][8192] and piles[2][4096]   # clipped first piece, tailV != 0
        assert n == 0 or piles[1][4095]                                                                     # a non-zero closing interval
        cov = {W: CR.coverage(ev, LENS, W) for W, _, _ in CONFIGS}
        prof = {(F, Bn): PR.profile(ev, LENS, ANCHORS, F, Bn, piles=piles) for _, F, Bn in CONFIGS}
        assert all(x[0].any() for x in cov.values()) and all(x.any() for x in prof.values())
        _SAMPLES[n, at_end] = (ev, piles, cov, prof)
    return _SAMPLES[n, at_end]


def _depth(ev, piles, ctrl, beds):
    return DR.hist(ev, LENS, beds=beds, is_ctrl=ctrl, piles=piles)   # (BED_ELSEWHERE lies where no event is: the same piles)


def _ctx(W, F, Bn, beds=None):
    import genrich_amd
    h = genrich_amd.Genrich(B.make_params(**PARAMS))
    h.set_chroms(LENS, None, beds)
    h.set_coverage_bins(W)
    h.set_depth_hist(True)
    h.set_profile(ANCHORS, F, Bn, True)
    return h


@pytest.mark.parametrize("n,at_end", CASES)
def test_the_rule_for_n_is_the_interval_ends(n, at_end):
    """The ends of a no-control treatment's intervals, tile by tile, are the positions _n_of counts."""
    ev, piles, _, _ = _sample(n, at_end)
    h = _ctx(50, 4096, 8)
    _run(h, [(ev, None)])
    for c, (pos0, t_end), *_ in PLACES:
        ends, _ = h.get_intervals(-1, c)
        assert int(((ends > pos0) & (ends <= t_end)).sum()) == _n_of(piles[c], LENS[c], pos0, t_end), (c, ends)
    h.close()


@pytest.mark.parametrize("form", ["loose", "stashed", "tight"])
@pytest.mark.parametrize("n,at_end", CASES)
def test_the_walk_at_n(n, at_end, form):
    """loose: a treatment's slots; stashed: the same events as the control of a small treatment (its slots are stashed for the
    merge); tight: the arrays pack_pileup makes when the run has -E regions."""
    ev, piles, cov, prof = _sample(n, at_end)
    small, spiles, scov, sprof = _sample(1, False)
    beds = BED_ELSEWHERE if form == "tight" else None
    for W, F, Bn in CONFIGS:
        h = _ctx(W, F, Bn, beds)
        if form == "stashed":
            order, _ = _run(h, [(small, ev)])
            exp = [(scov[W], _depth(small, spiles, False, beds), sprof[F, Bn]), (cov[W], _depth(ev, piles, True, beds), prof[F, Bn])]
        else:
            order, _ = _run(h, [(ev, None)])
            exp = [(cov[W], _depth(ev, piles, False, beds), prof[F, Bn])]
        _check_coverage(h, order, [e[0] for e in exp])
        _check_depth(h, order, [e[1] for e in exp])
        _check_profile(h, order, [e[2] for e in exp])
        h.close()
