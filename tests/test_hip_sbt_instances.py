"""Every instance of k_sbtile runs somewhere in the suite.  The host names the ten instances (PAIRS, BIG, FRAC, TRC, BED) once, in
a table (gx_host_build.h SBT_INSTANCES), and a launch looks its instance up there: one that is missing or mislabelled shows
only when a sample asks for it.  The first launch's instances and the second launch over the first one's list run in
  test_hip_sbt_persistent.py: test_a_workgroup_runs_many_bins_in_a_row, test_a_bin_that_leaves_for_the_second_launch_between_ordinary_bins,
      test_fractional_pair_records_with_one_persistent_workgroup, test_excluded_regions_with_one_persistent_workgroup,
  test_hip_paths.py: test_excluded_regions_on_the_fused_tile_stage_and_on_the_general_chain, the GX_NO_PAIRS cases,
  test_hip_tile_limits.py: constructed tiles at sbt_tile's and sbt_heavy's per-tile limits in the pair instance, the start / end
      key instance, the fractional one, the -E one (ordinary tiles), with one persistent workgroup, and -- four cases -- in the dense
      launch's two instances (test_tile_stage_in_the_dense_launch).
What is left is the DENSE launch -- a sample whose average bin holds more keys than the key array: one launch takes every bin
by rounds -- for plain data, -E regions and fractional pair records, each in the instance with the large scratch (TR = 448)
and the small one (TR = 384; GX_SBT_TR chooses, as the measurements do).

Sizing, by the host's own rule (plan_build).  lens = [200,000, 90,000]: 49 + 22 = 71 tiles of 4,096 bases, sbShift 3, 9 bins of
eight tiles.  The key array holds SBT_KEYCAP = 46,912 keys at TR = 448 and 49,984 at 384 (gx_sbtile.h sbt_keycap).
  * the fused stage is taken while nEv <= 9 x 64,000 = 576,000;
  * unit weights: bins of half the size once 2 nEv > 9 x (46,912 - 4,691), i.e. nEv > 189,994: 18 bins of four tiles;
    dense once 2 nEv > 18 x (46,912 - 2,932) = 791,640, i.e. nEv > 395,820 (with 9 bins the bound would be 197,910 -- beyond
    the 189,994 at which the bins are halved, so no smaller sample is dense);
  * fractional pair records keep the 9 bins: dense once 2 nEv > 9 x 43,980 = 395,820, i.e. nEv > 197,910.
The two instances differ in the rounds a bin takes, so the sample is the smallest round number at which the AVERAGE bin
(2 nEv / bins keys) fits the small scratch's key array in one round and needs two with the large scratch:
46,912 < 2 nEv / 18 <= 49,984 gives 422,208 < nEv <= 449,856: 430,000 fragments (47,778 keys per bin); with 9 bins
211,104 < nEv <= 224,928: 104,000 fragments of which a quarter become 2 .. 10 copies, about 219,000 events (the test
checks the window).  No towers (make_fragments' frac_tower = 0): no base nears the int16 limits, no bin outgrows the slots,
nothing goes back to the general chain."""
import functools

import pytest

import backends as B
import synth
from test_hip_parity import assert_same_run, hip_backend
from test_hip_paths import FELL_BACK, FRAC_PAIRS, FUSED, PAIRS

pytestmark = pytest.mark.gpu

LENS = [200_000, 90_000]
KEYCAP, KEYCAP_SMALL = 46_912, 49_984   # sbt_keycap(448), sbt_keycap(384)
# -E regions of the kinds of test_hip_paths._bed_case at this scale: touching position 0, one base, two edges in one tile,
# whole tiles and whole bins (40,000 .. 150,000: six bins of 16,384 bases), reaching a chromosome's end
BEDS = [[0, 900, 5_000, 5_001, 12_300, 12_390, 40_000, 150_000, 190_000, 190_070], [500, 600, 60_000, 64_123, 89_000, 90_000]]


def _check_sizing(n_ev, bins):
    assert n_ev <= 9 * 64_000                                  # the fused stage
    assert 2 * n_ev > bins * (KEYCAP - KEYCAP // 16)           # dense
    assert KEYCAP < 2 * n_ev // bins <= KEYCAP_SMALL           # one round of the average bin at 384, two at 448


@functools.lru_cache(maxsize=None)
def _dense(kind):
    params = B.make_params(pq=0.01, min_auc=20.0)
    if kind == "frac":
        # (a small replicate shows the context a fraction first: from then on there is no early lambda, as in a run on such data.
        # The test also announces the weights -- expect_fractional --, so that this replicate rides the pair records with a weight
        # class at once and is not sent back to the general chain, which would leave FELL_BACK set for the whole run)
        warm = synth.add_multimap(synth.make_fragments(LENS, 2_000, 5, frac_tower=0.0), LENS, 0.5, 6)
        ev = synth.add_multimap(synth.make_fragments(LENS, 104_000, 61, peak_every=20_000, frac_tower=0.0), LENS, 0.25, 62)
        _check_sizing(len(ev), 9)
        reps = [dict(save=None, treat=warm, ctrl=None), dict(save=None, treat=ev, ctrl=None)]
    else:
        ev = synth.make_fragments(LENS, 430_000, 63, peak_every=20_000, frac_tower=0.0)
        assert 2 * len(ev) > 9 * (KEYCAP - KEYCAP // 10)       # half-size bins: 18 of them
        _check_sizing(len(ev), 18)
        reps = [dict(save=None, treat=ev, ctrl=None)]
    case = dict(lens=LENS, replicates=reps)
    if kind == "bed":
        case["beds"] = BEDS
    o = B.Oracle(params)
    return case, params, o, B.run_case(o, case)


@pytest.mark.parametrize("tr", [384, 448])
@pytest.mark.parametrize("kind", ["plain", "bed", "frac"])
def test_the_dense_launch_of_every_kind_in_both_instances(monkeypatch, kind, tr):
    monkeypatch.setenv("GX_SBT_TR", str(tr))   # (read when the context is made)
    case, params, o, so = _dense(kind)
    h = hip_backend(params)
    if kind == "frac":
        h.expect_fractional(True)
    sh = B.run_case(h, case)
    flags = h.path_info()
    assert_same_run(o, h, so, sh, case)
    assert flags & FUSED and flags & PAIRS and not flags & FELL_BACK, flags
    assert bool(flags & FRAC_PAIRS) == (kind == "frac"), flags
    assert h.n_peaks > 0
