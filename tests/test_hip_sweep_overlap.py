"""The sweep's run pass beside the sample's closing scan (k_scan_iv_close_runs, gx_stats.h; spec_runs_wanted / run_sweep).

A treatment sample whose tile stage wrote the sweep's significance bits (lambda known early, -p, one rank) has its runs of
significant loose slots found in the very launch that scans the tiles and closes the sample: the scan's workgroups first, the
run pass's behind them, neither waiting for the other.  The run pass cannot read the chromosome-start mask -- the closing
workgroup writes it --, so it takes the chromosomes' first slots from tileSlot[first tile] (ChromStarts, k_runs<true>; the
sweep's own k_runs on the loose slots does the same).  gx_find_peaks takes that pass when the sweep turns out to be the one it
was launched for -- one replicate, no control, the loose slots accepted, the same capacity -- and drops it in every other case.

Every case is compared with the CPU oracle: the peak records as bytes, then the intervals (assert_same_run); gx_path_info's
bit 29 says whether the sweep took the speculative pass."""
import functools

import numpy as np
import pytest

import backends as B
import synth
from test_hip_parity import assert_same_run, hip_backend

pytestmark = pytest.mark.gpu

FUSED, LOOSE, FELL_BACK, PAIRS = 1, 2, 4, 16
OVERLAP = 536870912     # GX_PATH_SWEEP_OVERLAP
TB = 12                 # GX_TB
TILE = 1 << TB
SW_CHUNK = 256 * 8      # gx_stats.h: mask words per chunk of the run pass
STL_CHUNK = 256 * 8     # gx_kernels.h: tiles per chunk of the scan
PARAMS = dict(pq=0.01, min_auc=20.0)
THR = 2.0               # -log10(0.01)


def rows(frags):
    return np.array([(int(c), int(s), int(e), 1) for c, s, e in frags], dtype=B.EVENT_DTYPE).reshape(-1)


def _one(lens, ev, **kw):
    return dict(lens=list(lens), replicates=[dict(save=None, treat=ev, ctrl=None)], **kw)


def _oracle(case, **par):
    params = B.make_params(**{**PARAMS, **par})
    o = B.Oracle(params)
    return params, o, B.run_case(o, case)


def _hip(params, o, so, case, prepare=None):
    h = hip_backend(params)
    if prepare:
        prepare(h)
    sh = B.run_case(h, case)
    flags = h.path_info()
    assert h.get_peaks().tobytes() == o.get_peaks().tobytes()
    assert_same_run(o, h, so, sh, case)
    return h, flags


def keys_per_tile(ev, lens):
    """keys of every tile as the tile stage counts them: a start key per fragment, an end key unless it ends at the length"""
    lens = np.asarray(lens, dtype=np.int64)
    base = np.concatenate([[0], np.cumsum((lens + TILE - 1) >> TB)])
    c, s, e = ev["chrom"].astype(np.int64), ev["start"].astype(np.int64), ev["end"].astype(np.int64)
    has_end = e < lens[c]
    kt = np.concatenate([base[c] + (s >> TB), base[c[has_end]] + (e[has_end] >> TB)])
    return np.bincount(kt, minlength=base[-1]), base


# ---- 1: a full last tile: two significant slots of two chromosomes side by side ----------------------------------------------------

DEPTH = 24


@functools.lru_cache(maxsize=None)
def _full_tile():
    """Chromosome 0's last tile holds DEPTH start keys on distinct bases and nothing else: the fragments end at the chromosome's
    length (no end key).  DEPTH keys, DEPTH + 1 slots, DEPTH intervals and the closing one: the tile is exactly full, the closing
    interval (pileup DEPTH) lies in its last slot.  Chromosome 1 opens with DEPTH fragments from base 0: its first interval, in
    the very next slot, is as high."""
    lens = [2 * TILE + 1000, 2 * TILE, 2 * TILE + 5]
    fr = [(0, 2 * TILE + 100 + 7 * i, lens[0]) for i in range(DEPTH)]
    fr += [(1, 0, 300 + 5 * i) for i in range(DEPTH)]
    fr += [(1, TILE + 50 + 3 * i, TILE + 400 + 3 * i) for i in range(DEPTH)]          # (something in every chromosome's later tiles)
    fr += [(0, 500 + 11 * i, 700 + 11 * i) for i in range(DEPTH)]
    rng = np.random.default_rng(3)
    st = rng.integers(1, lens[2] - 200, size=150)
    fr += [(2, int(a), int(a) + 120) for a in st]
    case = _one(lens, rows(fr))
    return (case,) + _oracle(case)


def test_a_run_is_cut_between_a_full_last_tile_and_the_next_chromosomes_first_slot():
    case, params, o, so = _full_tile()
    ev, lens = case["replicates"][0]["treat"], case["lens"]
    n, base = keys_per_tile(ev, lens)
    e0, c0 = o.get_intervals(-1, 0)
    e1, c1 = o.get_intervals(-1, 1)
    last = int(base[1]) - 1
    # (an interval is the tile's in which it ends; the closing one ends at the length, inside the last tile)
    assert e0[-1] == lens[0] and int((e0.astype(np.int64) >> TB == 2).sum()) == n[last] + 1 == DEPTH + 1, "the tile is not exactly full"
    assert c0["p"][-1] > THR and c1["p"][0] > THR and e1[0] == 300, "the two neighbouring slots are not both significant"
    pk = o.get_peaks()
    assert (pk["chrom"] == 0).any() and ((pk["chrom"] == 1) & (pk["start"] == 0)).any()
    h, flags = _hip(params, o, so, case)
    assert flags & FUSED and flags & LOOSE and flags & OVERLAP, flags


# ---- 2: a run across a tile border, an empty tile, a chromosome without fragments, a skipped one ------------------------------------

@functools.lru_cache(maxsize=None)
def _border():
    lens = [3 * TILE - 7, 2 * TILE, 2 * TILE + 9, 2 * TILE + 1]
    fr = [(0, TILE - 200 + 3 * i, TILE + 200 + 5 * i) for i in range(30)]     # up before the border 0 | 1, down behind it; tile 2 stays empty
    fr += [(2, 1000 + i, 1500 + i) for i in range(30)]                         # on the skipped chromosome
    fr += [(3, 6000 + 2 * i, 6400 + 3 * i) for i in range(30)]
    rng = np.random.default_rng(5)
    fr += [(3, int(a), int(a) + 90) for a in rng.integers(1, lens[3] - 100, size=120)]
    case = _one(lens, rows(fr), skip=[0, 0, 1, 0])
    return (case,) + _oracle(case)


@pytest.mark.parametrize("overlap", [True, False])
def test_a_run_across_a_tile_border_beside_an_empty_tile_an_empty_and_a_skipped_chromosome(monkeypatch, overlap):
    if not overlap:
        monkeypatch.setenv("GX_NO_SWEEP_OVERLAP", "1")   # (the sweep's own k_runs<true>: the same table)
    case, params, o, so = _border()
    ev, lens = case["replicates"][0]["treat"], case["lens"]
    n, base = keys_per_tile(ev, lens)
    assert n[2] == 0 and n[int(base[1]):int(base[2])].sum() == 0   # chromosome 0's third tile and all of chromosome 1: no key
    pk = o.get_peaks()
    assert ((pk["chrom"] == 0) & (pk["start"] < TILE) & (pk["end"] > TILE)).any(), "no peak across the tile border"
    assert not (pk["chrom"] == 2).any() and (pk["chrom"] == 3).any()
    h, flags = _hip(params, o, so, case)
    assert flags & FUSED and flags & LOOSE and bool(flags & OVERLAP) == overlap, flags


# ---- 3 .. 6 share one ordinary input ------------------------------------------------------------------------------------------------

LENS = (300_000, 70_001, 5)


@functools.lru_cache(maxsize=None)
def _plain(qval=False):
    case = _one(LENS, synth.make_fragments(list(LENS[:2]), 30_000, 21, peak_every=20_000, tower_every=150_000))
    return (case,) + _oracle(case, **(dict(pq=0.5, qval=True, min_auc=5.0) if qval else {}))


def test_a_first_guess_that_overflows_runs_the_run_pass_again(monkeypatch):
    """GX_RUN_CAP_MIN = 4: the speculative pass and the first attempt count more runs than their arrays hold; the second attempt
    launches k_runs with arrays that fit.  The context remembers: after a reset the speculative pass fits and is taken."""
    monkeypatch.setenv("GX_RUN_CAP_MIN", "4")
    case, params, o, so = _plain()
    assert o.n_peaks > 16
    h, flags = _hip(params, o, so, case)
    assert flags & LOOSE and not flags & OVERLAP, flags
    h.reset()
    B.run_case(h, case)
    assert h.get_peaks().tobytes() == o.get_peaks().tobytes()
    assert h.path_info() & OVERLAP


def test_the_headline_path_takes_the_overlapped_launch():
    case, params, o, so = _plain()
    h, flags = _hip(params, o, so, case)
    assert flags & FUSED and flags & PAIRS and flags & LOOSE and flags & OVERLAP and not flags & FELL_BACK, flags


def test_the_sweep_twice_and_a_reset_between_two_runs():
    """The second gx_find_peaks on the same sample finds no speculative pass and launches k_runs; after a reset the same run takes
    the overlapped launch again.  Equal bytes every time."""
    case, params, o, so = _plain()
    want = o.get_peaks().tobytes()
    h = hip_backend(params)
    B.run_case(h, case)
    assert h.path_info() & OVERLAP and h.get_peaks().tobytes() == want
    h.find_peaks()
    assert h.path_info() & LOOSE and not h.path_info() & OVERLAP and h.get_peaks().tobytes() == want
    h.reset()
    sh = B.run_case(h, case)
    assert h.path_info() & OVERLAP and h.get_peaks().tobytes() == want
    assert_same_run(o, h, so, sh, case)


# ---- 4: whatever follows the sample, the speculative pass is dropped ----------------------------------------------------------------

def test_dropped_when_a_control_follows():
    lens = list(LENS[:2])
    t = _plain()[0]["replicates"][0]["treat"]
    c = synth.make_fragments(lens, 20_000, 22, uniform_only=True)
    case = dict(lens=lens, replicates=[dict(save=None, treat=t, ctrl=c)])
    params, o, so = _oracle(case)
    h, flags = _hip(params, o, so, case)
    assert flags & FUSED and not flags & (LOOSE | OVERLAP), flags


def test_dropped_with_three_replicates():
    lens = list(LENS[:2])
    t = _plain()[0]["replicates"][0]["treat"]
    case = dict(lens=lens, replicates=[dict(save=None, treat=t[k::3].copy(), ctrl=None) for k in range(3)])
    params, o, so = _oracle(case)
    h, flags = _hip(params, o, so, case)
    assert flags & FUSED and not flags & OVERLAP, flags


def test_not_launched_with_q_values():
    case, params, o, so = _plain(qval=True)
    h, flags = _hip(params, o, so, case)
    assert flags & FUSED and not flags & OVERLAP, flags


def test_not_launched_without_the_loose_slots(monkeypatch):
    monkeypatch.setenv("GX_NO_LOOSE", "1")
    case, params, o, so = _plain()
    h, flags = _hip(params, o, so, case)
    assert flags & FUSED and not flags & (LOOSE | OVERLAP), flags


def test_not_launched_when_fractional_weights_are_expected():
    case, params, o, so = _plain()
    h, flags = _hip(params, o, so, case, prepare=lambda h: h.expect_fractional(True))
    assert flags & FUSED and not flags & OVERLAP, flags


def test_dropped_when_the_sample_is_built_again_on_the_general_chain():
    """70,000 fragments inside one super-bucket: more pair records than k_sbtile's slots take.  The first build's launch has
    run the speculative pass over bits of a tile stage that gave up; the sample is built again, the sweep launches k_runs."""
    lens = [200_000]
    rng = np.random.default_rng(9)
    ev = synth.make_fragments(lens, 20_000, 2, peak_every=20_000, tower_every=150_000)
    pile = np.zeros(70_000, dtype=B.EVENT_DTYPE)
    pile["start"] = 66_000 + rng.integers(0, 12_000, size=len(pile))
    pile["end"] = pile["start"] + 100 + rng.integers(0, 200, size=len(pile))
    pile["count"] = 1
    case = _one(lens, np.concatenate([ev, pile]))
    params, o, so = _oracle(case)
    h, flags = _hip(params, o, so, case)
    assert flags & FELL_BACK and flags & LOOSE and not flags & OVERLAP, flags


# ---- 5: one workgroup per half ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _two_chunks():
    """9 Mbp = 2,198 tiles: two chunks of the scan; 70,000 fragments = 142,198 loose slots = 2,222 mask words: two chunks of the run pass"""
    lens = [6_000_000, 3_000_001]
    ev = synth.make_fragments(lens, 70_000, 13, peak_every=60_000, tower_every=2_000_000)
    n_tiles = sum((l + TILE - 1) >> TB for l in lens)
    assert n_tiles > STL_CHUNK and (2 * len(ev) + n_tiles + 16 + 63) // 64 > SW_CHUNK
    case = _one(lens, ev)
    return (case,) + _oracle(case)


@pytest.mark.parametrize("grid", [1, 2, 0])
def test_both_look_backs_finish_with_one_workgroup_per_half(monkeypatch, grid):
    """GX_SBT_GRID = 1, GX_SWEEP_GRID = 1: the fused launch is two workgroups, one walking every chunk of the scan (and closing
    the sample), one every chunk of the run pass -- each look-back finds its predecessors published by its own workgroup."""
    monkeypatch.setenv("GX_SBT_GRID", "1")
    if grid:
        monkeypatch.setenv("GX_SWEEP_GRID", str(grid))
    case, params, o, so = _two_chunks()
    h, flags = _hip(params, o, so, case)
    assert h.n_peaks > 0
    assert flags & FUSED and flags & LOOSE and flags & OVERLAP and not flags & FELL_BACK, flags
