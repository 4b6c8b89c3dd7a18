"""The persistent passes of the pair sort (gx_sort.h, round 8): a workgroup of k_sort_a takes the chunks b, b + grid, b + 2 grid ...
of 8,192 events of a piece and asks for the next chunk's first loads under the scatter of the one it holds; a workgroup of k_sort_b
walks the pages of its XCD class's coarse lists the same way.  GX_S2_GRID makes one workgroup (or two, three, seven) run many
chunks in a row on an input of a few chunks, so that everything a workgroup carries from one chunk to the next is exercised: the
LDS counts that must be back at zero, a last chunk that is not full, a prefetch with nothing to fetch, the slow events' replay
behind a later chunk, the early exit on a fractional weight, the sums posted once per workgroup -- and, on the host's side, page
tables sized for chunks that all fall into a few XCD classes.  Every run must give the CPU oracle's bits."""
import functools

import numpy as np
import pytest

import backends as B
import synth
from test_hip_parity import assert_same_run, hip_backend
from test_hip_paths import FELL_BACK, FRAC_PAIRS, FUSED, PAIRS

pytestmark = pytest.mark.gpu

CHUNK = 8_192        # gx_sort.h S2_CHUNK: events per chunk of k_sort_a, records per page of a coarse list
PACKED_USED = 512    # gx_path_info: a piece of 8-byte events was read in place (k_sort_a<.., PACKED>)
PARAMS = dict(pq=0.01, min_auc=20.0)


def _env(monkeypatch, grid, sbshift=None, **more):
    if sbshift is not None:
        monkeypatch.setenv("GX_SBSHIFT", str(sbshift))   # (sizes tables: read when the context is made)
    if grid:
        monkeypatch.setenv("GX_S2_GRID", str(grid))
    for k, v in more.items():
        monkeypatch.setenv(k, str(v))


def _one(lens, ev, **kw):
    return dict(lens=list(lens), replicates=[dict(save=None, treat=ev, ctrl=None)], **kw)


def _hip_run(o, so, case, prepare=None):
    h = hip_backend(B.make_params(**PARAMS))
    if prepare:
        prepare(h)
    sh = B.run_case(h, case)
    flags = h.path_info()
    assert_same_run(o, h, so, sh, case)
    return h, flags


def _oracle(case):
    o = B.Oracle(B.make_params(**PARAMS))
    return o, B.run_case(o, case)


def _same_tables(o, h, n_chrom, cols=("expt", "p")):
    assert h.get_peaks().tobytes() == o.get_peaks().tobytes()
    for c in range(n_chrom):
        eo, co = o.get_intervals(-1, c)
        eh, ch = h.get_intervals(-1, c)
        assert np.array_equal(eo, eh), c
        for k in cols:
            assert np.array_equal(co[k].view(np.uint32), ch[k].view(np.uint32)), (k, c)


# ---- 1: the edges of the chunk loop ------------------------------------------------------------------------------------------------

LENS = (400_000, 123_457, 16_384)


@functools.lru_cache(maxsize=None)
def _edge(n):
    case = _one(LENS, synth.make_fragments(list(LENS), n, 100 + n % 97, peak_every=20_000, tower_every=150_000))
    return (case,) + _oracle(case)


@pytest.mark.parametrize("grid", [1, 2, 0])
@pytest.mark.parametrize("n", [1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5])
def test_a_last_chunk_that_is_not_full_and_fewer_chunks_than_workgroups(monkeypatch, n, grid):
    """One event; a chunk short of one event, exactly one, one chunk and one event (the second chunk holds a single event: with
    grid 1 the prefetch's loads are all clamped to it, with grid 2 the second workgroup has nothing to fetch), three chunks and
    five events."""
    _env(monkeypatch, grid)
    case, o, so = _edge(n)
    h, flags = _hip_run(o, so, case)
    assert flags & FUSED and flags & PAIRS and not flags & FELL_BACK, flags


# ---- 2: many chunks per workgroup, coarse lists of several pages -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _many_chunks():
    """330,000 events = 41 chunks on 5 Mbp in bins of two tiles: 611 fine bins, ten coarse ones.  With one workgroup every chunk is
    of XCD class 0, and each of that class's ten coarse lists takes ~33,000 records: four pages and a fifth begun."""
    lens = [3_000_000, 1_500_000, 500_001]
    case = _one(lens, synth.make_fragments(lens, 330_000, 7, peak_every=40_000, tower_every=1_000_000))
    return (case,) + _oracle(case)


@pytest.mark.parametrize("grid", [1, 2, 3, 7, 0])
def test_a_workgroup_runs_many_chunks_and_the_coarse_lists_cross_pages(monkeypatch, grid):
    _env(monkeypatch, grid, sbshift=1)
    case, o, so = _many_chunks()
    h, flags = _hip_run(o, so, case)
    assert h.n_peaks > 0
    assert flags & FUSED and flags & PAIRS and not flags & FELL_BACK, flags


# ---- 3: slow events behind a workgroup's first chunk -------------------------------------------------------------------------------

def test_slow_events_in_the_second_and_third_chunk_of_one_workgroup(monkeypatch):
    """What does not leave as a pair record is replayed behind its chunk's scatter -- here from the chunks a workgroup takes after
    its first one (bins of two tiles: a bin border every 8,192 bases)."""
    _env(monkeypatch, 1, sbshift=1)
    lens = [400_000, 123_457, 50_000]
    ev = synth.make_fragments(lens[:2], 30_000, 41, peak_every=20_000, tower_every=150_000)

    def slow(shift):
        return np.array([(0, 8_100 + shift, 8_300 + shift, 1),                       # crosses a bin border
                         (0, 24_500 + shift, 24_700 + shift, 1),                     # ... another one (three bins on)
                         (0, 100_000 + shift, 100_000 + shift + 4_095, 1),           # 4,095 bases: no room in a pair record's length
                         (1, 60_000 + shift, 60_000 + shift + 9_000, 1),             # longer than a bin
                         (0, lens[0] - 150 - shift, lens[0], 1),                     # ends at the chromosome's length: no end record
                         (1, lens[1] - 99 - shift, lens[1], 1),
                         (2, 1_000 + shift, 1_200 + shift, 1),                       # on a skipped chromosome
                         (0, 250_000 + shift, 249_990 + shift, 1),                   # ends before it starts
                         (1, 5_000 + shift, 5_000 + shift, 1)],                      # empty
                        dtype=B.EVENT_DTYPE)

    a, b = slow(0), slow(37)
    ev[CHUNK + 700:CHUNK + 700 + len(a)] = a
    ev[2 * CHUNK + 5_000:2 * CHUNK + 5_000 + len(b)] = b
    ev[-len(a):] = slow(11)   # ... and in the last, partial chunk
    case = _one(lens, ev, skip=[0, 0, 1])
    o, so = _oracle(case)
    h, flags = _hip_run(o, so, case)
    assert flags & FUSED and flags & PAIRS and not flags & FELL_BACK, flags


# ---- 4: a fractional weight that first shows in the third chunk --------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _late_fraction():
    lens = [300_000, 70_001]
    unit = synth.make_fragments(lens, 30_000, 31, peak_every=20_000, tower_every=150_000)
    mm = synth.add_multimap(synth.make_fragments(lens, 4_000, 33, peak_every=20_000, tower_every=150_000), lens, 0.3, 32)
    at = 2 * CHUNK + 300
    case = _one(lens, np.concatenate([unit[:at], mm, unit[at:]]))
    assert (case["replicates"][0]["treat"]["count"][:2 * CHUNK] == 1).all()
    return (case,) + _oracle(case)


def test_a_fraction_in_the_third_chunk_sends_an_unhinted_sample_to_the_general_chain(monkeypatch):
    """The workgroup has scattered two chunks of unit-weight pair records when it meets the weight: ST_SB_FRAC goes up, the loop
    is left, the sample is built again on the general chain."""
    _env(monkeypatch, 1)
    case, o, so = _late_fraction()
    h, flags = _hip_run(o, so, case)
    assert flags & FELL_BACK, flags


@pytest.mark.parametrize("grid", [1, 3])
def test_a_fraction_in_the_third_chunk_of_a_hinted_context_rides_the_pair_records(monkeypatch, grid):
    _env(monkeypatch, grid)
    case, o, so = _late_fraction()
    h, flags = _hip_run(o, so, case, prepare=lambda h: h.expect_fractional(True))
    assert flags & FUSED and flags & FRAC_PAIRS and not flags & FELL_BACK, flags


# ---- 5: 8-byte events, an odd count ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid,frac", [(1, False), (3, False), (1, True), (3, True)])
def test_packed_events_of_an_odd_count(monkeypatch, grid, frac):
    """k_sort_a<.., PACKED> takes two events to a 16-byte load: with an odd count the last load of the last chunk -- and, with one
    workgroup, the prefetch before it -- is half events, half padding."""
    from genrich_amd.lib import pack_events
    _env(monkeypatch, grid)
    lens = [300_000, 70_001]
    ev = synth.make_fragments(lens, 3 * CHUNK + 2_222, 51, peak_every=20_000, tower_every=150_000)
    if frac:
        ev = synth.add_multimap(ev, lens, 0.3, 52)
    ev = ev[:len(ev) - 1 + len(ev) % 2].copy()   # an odd count
    p8, rest = pack_events(ev)
    assert len(rest) == 0 and len(p8) % 2 == 1 and len(p8) > 3 * CHUNK
    case = _one(lens, ev)
    o, so = _oracle(case)
    h = hip_backend(B.make_params(**PARAMS))
    if frac:
        h.expect_fractional(True)
    h.set_chroms(lens)
    h.sample_begin(0, None)
    h.push_events_packed(p8)
    h.sample_end()
    h.sample_no_control()
    h.pvalues()
    h.find_peaks()
    flags = h.path_info()
    assert flags & FUSED and flags & PAIRS and flags & PACKED_USED and not flags & FELL_BACK, flags
    assert bool(flags & FRAC_PAIRS) == frac, flags
    _same_tables(o, h, len(lens), cols=("p",) if frac else ("expt", "p"))


# ---- 6: one sample in three pieces -------------------------------------------------------------------------------------------------

def test_one_sample_in_three_pieces_of_unequal_sizes(monkeypatch):
    """Every piece is a launch of its own with its own grid (here two workgroups, classes 0 and 1); the classes' chunk counts add
    up over the pieces, and so must the page tables' rows."""
    _env(monkeypatch, 2, sbshift=1)
    lens = [400_000, 123_457]
    ev = synth.make_fragments(lens, 60_000, 61, peak_every=20_000, tower_every=150_000)
    case = _one(lens, ev)
    o, so = _oracle(case)
    h = hip_backend(B.make_params(**PARAMS))
    h.set_chroms(lens)
    h.sample_begin(0, None)
    cuts = [0, 9_001, 9_001 + 20_011, len(ev)]
    assert all((b - a) % CHUNK for a, b in zip(cuts[:-1], cuts[1:]))
    for a, b in zip(cuts[:-1], cuts[1:]):
        h.push_events(ev[a:b])
    frag, _, _ = h.sample_end()
    lam = h.sample_no_control()
    h.pvalues()
    h.find_peaks()
    flags = h.path_info()
    assert_same_run(o, h, so, [(frag, lam, None)], case)
    assert flags & FUSED and flags & PAIRS and not flags & FELL_BACK, flags


# ---- 7: the next sample starts clean -----------------------------------------------------------------------------------------------

def test_two_samples_in_a_row_and_treatment_with_control_on_one_context(monkeypatch):
    """One context, one workgroup: the same case twice with a reset between, then treatment and control (two sorts in one step).
    Cursors, page counts and the LDS counts of a workgroup must start at zero every time."""
    _env(monkeypatch, 1, sbshift=1)
    lens = [300_000, 70_001]
    params = B.make_params(pq=0.05, qval=True, min_auc=20.0)
    t = synth.make_fragments(lens, 40_000, 21, peak_every=20_000, tower_every=150_000)
    c = synth.make_fragments(lens, 30_000, 22, uniform_only=True)
    cases = [dict(lens=lens, replicates=[dict(save=None, treat=t, ctrl=None)]),
             dict(lens=lens, replicates=[dict(save=None, treat=t, ctrl=None)]),
             dict(lens=lens, replicates=[dict(save=None, treat=t, ctrl=c)])]
    h = hip_backend(params)
    oracles = {}
    for i, case in enumerate(cases):
        key = 0 if i < 2 else i
        if key not in oracles:
            o = B.Oracle(params)
            oracles[key] = (o, B.run_case(o, case))
        o, so = oracles[key]
        if i:
            h.reset()
        sh = B.run_case(h, case)
        flags = h.path_info()
        assert_same_run(o, h, so, sh, case)
        assert flags & FUSED and flags & PAIRS and not flags & FELL_BACK, (i, flags)


# ---- 8: the 128-key instance of the second pass ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _half_bins():
    """36 Mbp in half-size bins of one tile: 8,790 of them -- more than 4,096, so a coarse bin has 128 fine ones (two owner
    wavefronts in k_sort_b's scatter)."""
    lens = [20_000_000, 16_000_000]
    case = _one(lens, synth.make_fragments(lens, 200_000, 77, peak_every=200_000, tower_every=5_000_000))
    return (case,) + _oracle(case)


@pytest.mark.parametrize("grid", [1, 0])
def test_the_128_key_second_pass(monkeypatch, grid):
    _env(monkeypatch, grid, sbshift=1, GX_FORCE_HALF_BINS=1)
    case, o, so = _half_bins()
    h, flags = _hip_run(o, so, case)
    assert flags & FUSED and flags & PAIRS and not flags & FELL_BACK, flags
