"""The persistent first launch of k_sbtile (gx_sbtile.h, round 7): a workgroup draws its bins from a ticket counter and asks for
the next bin's list lengths, slot descriptors and records under the bin it is working on.  GX_SBT_GRID makes a few workgroups
(or one) run many bins in a row on a genome of a few dozen bins, so that everything a workgroup carries from one bin to the next
is exercised: an empty bin between occupied ones, a bin that leaves for the second launch, the overflow exit, a list that goes on
in a second page, the ticket word of the next sample.  Every run must give the CPU oracle's bits."""
import functools

import numpy as np
import pytest

import backends as B
import synth
from test_hip_parity import assert_same_run, hip_backend
from test_hip_paths import FELL_BACK, FRAC_PAIRS, FUSED, PAIRS, _bed_case, _case

pytestmark = pytest.mark.gpu


def _hip_run(monkeypatch, o, so, case, params, grid, sbshift=None, prepare=None):
    if sbshift is not None:
        monkeypatch.setenv("GX_SBSHIFT", str(sbshift))   # (sizes tables: read when the context is made)
    if grid:
        monkeypatch.setenv("GX_SBT_GRID", str(grid))
    h = hip_backend(params)
    if prepare:
        prepare(h)
    sh = B.run_case(h, case)
    flags = h.path_info()
    assert_same_run(o, h, so, sh, case)
    assert flags & FUSED and flags & PAIRS, flags
    return h, flags


# ---- 1: many bins per workgroup ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _many_bins():
    """136 tiles in bins of two: 68 bins.  Two stretches of chromosome 0 hold no fragment (five and three empty bins between
    occupied ones), the 5-base contig at the end is a bin without a record, chromosome 3 (4,097 bases) ends one base into a tile."""
    case = _case()
    ev = case["replicates"][0]["treat"]
    gap = (ev["chrom"] == 0) & (((ev["end"] > 122_880) & (ev["start"] < 163_840)) | ((ev["end"] > 303_104) & (ev["start"] < 327_680)))
    case["replicates"][0]["treat"] = ev[~gap].copy()
    params = B.make_params(pq=0.01, min_auc=50.0)
    o = B.Oracle(params)
    return case, params, o, B.run_case(o, case)


@pytest.mark.parametrize("grid", [1, 2, 3, 7, 0])
def test_a_workgroup_runs_many_bins_in_a_row(monkeypatch, grid):
    case, params, o, so = _many_bins()
    h, flags = _hip_run(monkeypatch, o, so, case, params, grid, sbshift=1)
    assert h.n_peaks > 0 and not flags & FELL_BACK


# ---- 2, 3: bins that leave early ---------------------------------------------------------------------------------------------------

def _pile_case(n_bg, n_pile):
    lens = [200_000]   # 49 tiles -> 4 tiles per super-bucket; the pile lies inside bin 4 of 13, background on both sides of it
    rng = np.random.default_rng(9)
    ev = synth.make_fragments(lens, n_bg, 2, peak_every=20_000, tower_every=150_000)
    pile = np.zeros(n_pile, dtype=B.EVENT_DTYPE)
    pile["start"] = 66_000 + rng.integers(0, 12_000, size=len(pile))
    pile["end"] = pile["start"] + 100 + rng.integers(0, 200, size=len(pile))
    pile["count"] = 1
    return dict(lens=lens, replicates=[dict(save=None, treat=np.concatenate([ev, pile]), ctrl=None)])


def test_a_bin_that_leaves_for_the_second_launch_between_ordinary_bins(monkeypatch):
    """30,000 fragments in one bin: more keys than the key array holds, so the one workgroup puts the bin on the second launch's
    list -- with the following bin's lengths already asked for -- and carries on."""
    case = _pile_case(4_000, 30_000)
    params = B.make_params(pq=0.01, min_auc=20.0)
    o = B.Oracle(params)
    h, flags = _hip_run(monkeypatch, o, B.run_case(o, case), case, params, 1)
    assert not flags & FELL_BACK, flags


def test_the_overflow_exit_of_a_persistent_workgroup(monkeypatch):
    """70,000 fragments in one bin: more pair records than the slots take.  The sample goes back to the general chain; the bits
    after the rebuild are the oracle's."""
    monkeypatch.setenv("GX_SBT_GRID", "1")
    case = _pile_case(20_000, 70_000)
    params = B.make_params(pq=0.01, min_auc=20.0)
    o = B.Oracle(params)
    so = B.run_case(o, case)
    h = hip_backend(params)
    sh = B.run_case(h, case)
    flags = h.path_info()
    assert_same_run(o, h, so, sh, case)
    assert flags & FELL_BACK and not flags & FUSED, flags


# ---- 4: a list that goes on in a second page -----------------------------------------------------------------------------------

def test_a_list_that_continues_into_a_second_page(monkeypatch):
    """One bin of 256 tiles (chromosome 0 and the head of chromosome 1) with 19,400 fragments, another bin behind it.  Which of a
    bin's eight lists a record joins is decided by where its event lies in the input: level 1 of the sort cuts the events into
    chunks of 8,192 and chunk c writes to list c mod 8.  So the events of chunks 0 and 8 lie on chromosome 0 -- 16,384 records in
    list 0 of bin 0, two pages of 8,192: the slots 32 .. 63 of that list find their page through the page table, which the
    workgroup reads one bin ahead -- and the chunks between them on a chromosome that is skipped (no record at all), but for 3,000
    on chromosome 1.  The lists' lengths themselves cannot be read back from the host side: the layout above is the sort's
    (gx_sort.h, S2_CHUNK and PgCfg<u32>), and the full-size test covers lists of several pages on real proportions."""
    lens = [1_000_000, 300_000, 100_000]
    skip = [0, 0, 1]

    def frags(length, n, seed, chrom):
        ev = synth.make_fragments([length], n, seed, peak_every=20_000, tower_every=400_000)
        ev["chrom"] = chrom
        return ev

    mid = np.concatenate([frags(100_000, 7 * 8_192 - 3_000, 72, 2), frags(300_000, 3_000, 73, 1)])
    np.random.default_rng(5).shuffle(mid)
    ev = np.concatenate([frags(1_000_000, 8_192, 71, 0), mid, frags(1_000_000, 8_192 + 3_000, 74, 0)])
    case = dict(lens=lens, skip=skip, replicates=[dict(save=None, treat=ev, ctrl=None)])
    params = B.make_params(pq=0.01, min_auc=20.0)
    o = B.Oracle(params)
    h, flags = _hip_run(monkeypatch, o, B.run_case(o, case), case, params, 1, sbshift=8)
    assert not flags & FELL_BACK, flags


# ---- 5: the ticket starts at zero every time -------------------------------------------------------------------------------------

def test_the_ticket_starts_at_zero_for_every_sample_of_a_context(monkeypatch):
    """One context, two workgroups: the same case twice with a reset between, then treatment and control (two tile stages in one
    step), then three replicates (-q throughout: a context has one set of parameters).  A ticket word that kept a count from the
    sample before would hand out no bin at all."""
    monkeypatch.setenv("GX_SBSHIFT", "1")
    monkeypatch.setenv("GX_SBT_GRID", "2")
    lens = [300_000, 70_001]
    params = B.make_params(pq=0.05, qval=True, min_auc=20.0)
    t = synth.make_fragments(lens, 70_000, 21, peak_every=20_000, tower_every=150_000)
    c = synth.make_fragments(lens, 50_000, 22, uniform_only=True)
    reps = [dict(save=None, treat=synth.make_fragments(lens, 40_000, 100 + r, peak_every=25_000, tower_every=110_000), ctrl=None)
            for r in range(3)]
    cases = [dict(lens=lens, replicates=[dict(save=None, treat=t, ctrl=None)]),
             dict(lens=lens, replicates=[dict(save=None, treat=t, ctrl=None)]),
             dict(lens=lens, replicates=[dict(save=None, treat=t, ctrl=c)]),
             dict(lens=lens, replicates=reps)]
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


# ---- 6: the other instances of the first launch ------------------------------------------------------------------------------------

def test_fractional_pair_records_with_one_persistent_workgroup(monkeypatch):
    lens = [300_000, 70_001]
    ev = synth.add_multimap(synth.make_fragments(lens, 60_000, 31, peak_every=20_000, tower_every=150_000), lens, 0.3, 32)
    case = dict(lens=lens, replicates=[dict(save=None, treat=ev, ctrl=None)])
    params = B.make_params(pq=0.01, min_auc=20.0)
    o = B.Oracle(params)
    h, flags = _hip_run(monkeypatch, o, B.run_case(o, case), case, params, 1, sbshift=1, prepare=lambda h: h.expect_fractional(True))
    assert flags & FRAC_PAIRS and not flags & FELL_BACK, flags


def test_excluded_regions_with_one_persistent_workgroup(monkeypatch):
    case = _bed_case()
    params = B.make_params(pq=0.01, min_auc=20.0)
    o = B.Oracle(params)
    h, flags = _hip_run(monkeypatch, o, B.run_case(o, case), case, params, 1, sbshift=1)
    assert h.n_peaks > 0 and not flags & FELL_BACK, flags
