"""Profiles around anchor sites of every sample's pileup on the GPU (gx_set_profile / k_profile, genrich-amd --profile): exact
equality with the numpy definition (tests/profile_ref.py) of every sample, anchor and bin, for every class of flank and bin size,
on every tile-stage path, in every form the sample can be in when it is closed."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import backends as B
import coverage_ref as R
import golden_cases as G
import profile_ref as P
from genrich_amd.lib import GX_PATH_COVERAGE, GX_PATH_PROFILE
from test_hip_counts import Mem, _cli_inputs, _push
from test_hip_coverage import BEDS, LENS, ORDER, PARAMS, _events
from test_host_cli import _binary

pytestmark = pytest.mark.gpu

# (flank, bin): the default; one base per bin; two bins; one tile per bin; 1024 bins over six tiles; far larger than any chromosome
CLASSES = [(2000, 10), (64, 1), (50, 50), (4096, 4096), (10240, 20), (1 << 20, 1 << 11)]


def _anchors():
    """About 300 anchors, unsorted, on both strands, with duplicates: the chromosomes' ends and beyond, tile edges, the 37-base
    chromosome, the empty stretches of chromosome 4 and the events' clusters, one chromosome index behind the table."""
    rng = np.random.default_rng(11)
    rows = []
    for c, n in enumerate(LENS):
        for pos in (0, 1, n - 1, n, n + 5000):
            rows += [(c, pos, 1), (c, pos, -1)]
    for c in (0, 4):
        for pos in (4095, 4096, 4097, 8192):
            rows += [(c, pos, 1), (c, pos, -1)]
    rows += [(3, 18, 1), (3, 18, -1), (3, 36, 1), (2, 4090, -1), (1, 2048, 1)]
    for pos in (69_000, 70_000, 70_001, 73_728, 150_000, 151_552, 155_000):            # nothing starts near these on chromosome 4
        rows += [(4, pos, 1), (4, pos, -1)]
    for zone in (0, 30_000, 110_000, 190_000):                                         # the clusters
        rows += [(4, int(zone + p), int(s)) for p, s in zip(rng.integers(0, 10_000, 30), rng.choice([1, -1], 30))]
    for c in (0, 1, 2):
        rows += [(c, int(p), int(s)) for p, s in zip(rng.integers(0, LENS[c], 20), rng.choice([1, -1], 20))]
    rows += [(len(LENS), 100, 1), (1000, 0, -1)]                                       # behind the table
    rows += rows[5:25]                                                                 # duplicates
    a = np.asarray(rows, dtype=P.ANCHOR_DTYPE)
    return a[rng.permutation(len(a))]


ANCHORS = _anchors()
_PILES, _ROWS = {}, {}


def _expected(key, ev, F, Bn, skip=None, beds=None, save=None, owned=None, anchors=None):
    """profile_ref's matrix; the per-base pileups of a sample (`key` names it and its -E regions) and the rows of a class are
    computed once."""
    if key not in _PILES:
        _PILES[key] = {c: R.pileup120(ev, c, LENS[c], beds[c] if beds is not None else ()) for c in range(len(LENS))}
    if anchors is not None:
        return P.profile(ev, LENS, anchors, F, Bn, skip=skip, save=save, owned=owned, piles=_PILES[key])
    if (key, F, Bn) not in _ROWS:
        _ROWS[key, F, Bn] = P.profile(ev, LENS, ANCHORS, F, Bn, piles=_PILES[key])
    out = _ROWS[key, F, Bn].copy()
    for k, a in enumerate(ANCHORS):
        if not P.live_chrom(int(a["chrom"]), LENS, skip, save, owned):
            out[k] = 0
    return out


def _ctx(F, Bn, keep=True, skip=None, beds=None, owned=None, knobs=(), frac=False, params=None, anchors=None, cov=0):
    import genrich_amd
    h = genrich_amd.Genrich(B.make_params(**(params or PARAMS)))
    h.set_chroms(LENS, skip, beds)
    if owned is not None:
        h.set_owned(owned)
    for k, v in knobs:
        h.set_knob(k, v)
    if frac:
        h.expect_fractional(True)
    if cov:
        h.set_coverage_bins(cov)
    if F:
        h.set_profile(ANCHORS if anchors is None else anchors, F, Bn, keep)
    return h


def _run(h, reps, mode="host", saves=None, mem=None):
    """reps = [(treatment events, control events | None)]; -> the samples in gx_sample_end order as (rep, is_ctrl)."""
    mem = mem or Mem()
    order = []
    for r, (t, c) in enumerate(reps):
        h.sample_begin(0, saves[r] if saves else None)
        _push(h, t, mode, mem)
        h.sample_end()
        order.append((r, False))
        if c is not None:
            h.sample_begin(1, None)
            _push(h, c, mode, mem)
            h.sample_end()
            order.append((r, True))
        else:
            h.sample_no_control()
        h.pvalues()
    h.find_peaks()
    return order, mem


def _check(h, order, expected, keep=True):
    """expected[i] = the matrix of sample i: every anchor and bin, exactly; the aggregate = its column sums."""
    assert h.profile_samples() == len(order) == len(expected)
    for i, ((r, ctrl), exp) in enumerate(zip(order, expected)):
        got = h.profile(i)
        assert (got.rep, got.is_ctrl) == (r, ctrl)
        assert got.agg120.dtype == np.int64 and np.array_equal(got.agg120, exp.sum(axis=0)), (i, got.agg120, exp.sum(axis=0))
        if not keep:
            assert got.cell120 is None
            continue
        assert got.cell120.dtype == np.int64 and got.cell120.shape == exp.shape
        bad = np.argwhere(got.cell120 != exp)
        assert bad.size == 0, (i, bad[:8], [(int(got.cell120[a, j]), int(exp[a, j])) for a, j in bad[:8]])
        assert np.array_equal(got.agg120, got.cell120.sum(axis=0))


@pytest.fixture(scope="module")
def T0():
    return _events(1)


@pytest.fixture(scope="module")
def C0():
    return _events(2, n=20_000)


def test_the_anchor_set():
    assert 280 <= len(ANCHORS) <= 340 and {1, -1} == set(ANCHORS["strand"].tolist())
    assert len(np.unique(ANCHORS)) < len(ANCHORS) and (np.diff(ANCHORS["pos"].astype(np.int64)) < 0).any()
    assert (ANCHORS["chrom"] >= len(LENS)).any() and (ANCHORS["chrom"] == 3).any()


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("F,Bn", CLASSES)
def test_every_class_on_the_default_path(F, Bn, keep, T0):
    h = _ctx(F, Bn, keep)
    assert h.profile_layout() == (len(ANCHORS), 2 * F // Bn, F, Bn, keep)
    order, _ = _run(h, [(T0, None)])
    exp = _expected("T0", T0, F, Bn)
    assert exp.any() and not exp[ANCHORS["chrom"] >= len(LENS)].any()
    _check(h, order, [exp], keep)
    if not keep:
        assert h.lib.gx_get_profile(h.ctx, 0, None, None, None, np.zeros(2 * F // Bn, dtype=np.int64).ctypes.data, 0, 1) == ORDER
    assert h.path_info() & GX_PATH_PROFILE
    h.close()


@pytest.mark.parametrize("F,Bn", [(2000, 10), (4096, 4096)])
@pytest.mark.parametrize("knob", [("GX_NO_FUSED", 1), ("GX_NO_PAIRS", 1), ("GX_SBT_GRID", 1)])
def test_forced_tile_stage_paths(knob, F, Bn, T0, C0):
    h = _ctx(F, Bn, knobs=[knob])
    order, _ = _run(h, [(T0, C0)])
    _check(h, order, [_expected("T0", T0, F, Bn), _expected("C0", C0, F, Bn)])   # (the control: from its stashed loose slots)
    flags = h.path_info()
    assert not (knob[0] == "GX_NO_FUSED" and flags & 1) and not (knob[0] == "GX_NO_PAIRS" and flags & 16), flags   # (the path was forced)
    h.close()


@pytest.mark.parametrize("F,Bn", [(2000, 10), (64, 1)])
def test_a_pile_of_5000_fragments_in_one_tile(F, Bn, T0):
    tower = np.zeros(5000, dtype=B.EVENT_DTYPE)
    rng = np.random.default_rng(3)
    tower["chrom"] = 4
    tower["start"] = 2 * 4096 + 100 + rng.integers(0, 300, 5000)
    tower["end"] = tower["start"] + rng.integers(50, 900, 5000)
    tower["count"] = 1
    ev = np.concatenate([T0[:12_000], tower, T0[12_000:]])
    anchors = np.concatenate([ANCHORS, np.asarray([(4, 2 * 4096 + 300, 1), (4, 2 * 4096 + 420, -1)], dtype=P.ANCHOR_DTYPE)])
    h = _ctx(F, Bn, anchors=anchors)
    order, _ = _run(h, [(ev, None)])
    exp = _expected("tower", ev, F, Bn, anchors=anchors)
    assert exp[-2:].max() >= 120 * 2000 * Bn
    _check(h, order, [exp])
    h.close()


def test_fractional_weights():
    ev = _events(4, counts=(2, 3, 4, 5, 6, 8, 10))
    for F, Bn in ((2000, 10), (64, 1)):
        h = _ctx(F, Bn, frac=True)
        order, _ = _run(h, [(ev, None)])
        exp = _expected("frac", ev, F, Bn)
        assert (exp % 120 != 0).any()
        _check(h, order, [exp])
        h.close()


# anchors whose windows (F = 64 and F = 2000) straddle the edges of BEDS' regions, on top of the set
BED_ANCHORS = np.concatenate([ANCHORS, np.asarray(
    [(0, p, s) for p in (0, 90, 100, 110, 4990, 5000, 8190, 8192, 8200) for s in (1, -1)] +
    [(2, p, s) for p in (4085, 4090, 4096) for s in (1, -1)] +
    [(4, p, s) for p in (20_000, 20_010, 20_029, 20_030, 36_000, 44_990, 45_010, 198_990, 199_000, 199_999) for s in (1, -1)],
    dtype=P.ANCHOR_DTYPE)])


@pytest.mark.parametrize("F,Bn", [(2000, 10), (64, 1), (4096, 4096)])
def test_excluded_regions(F, Bn, T0, C0):
    h = _ctx(F, Bn, beds=BEDS, anchors=BED_ANCHORS)
    order, _ = _run(h, [(T0, C0)])
    et = _expected("T0bed", T0, F, Bn, beds=BEDS, anchors=BED_ANCHORS)
    ec = _expected("C0bed", C0, F, Bn, beds=BEDS, anchors=BED_ANCHORS)
    assert (et != _expected("T0", T0, F, Bn, anchors=BED_ANCHORS)).any()
    _check(h, order, [et, ec])
    h.close()
    h = _ctx(F, Bn, beds=BEDS, anchors=BED_ANCHORS)   # ... and without a control
    order, _ = _run(h, [(T0, None)])
    _check(h, order, [et])
    h.close()


def test_a_skipped_chromosome(T0):
    skip = [0, 0, 1, 0, 0]
    h = _ctx(2000, 10, skip=skip)
    order, _ = _run(h, [(T0, None)])
    exp = _expected("T0", T0, 2000, 10, skip=skip)
    assert not exp[ANCHORS["chrom"] == 2].any() and _expected("T0", T0, 2000, 10)[ANCHORS["chrom"] == 2].any()
    _check(h, order, [exp])
    h.close()


def test_a_save_mask_that_omits_a_chromosome_for_one_replicate(T0, C0):
    save = [1, 1, 0, 1, 1]
    h = _ctx(64, 1)
    order, _ = _run(h, [(T0, C0), (T0, None)], saves=[save, None])
    exp = [_expected("T0", T0, 64, 1, save=save), _expected("C0", C0, 64, 1, save=save), _expected("T0", T0, 64, 1)]
    on2 = ANCHORS["chrom"] == 2
    assert not exp[0][on2].any() and not exp[1][on2].any() and exp[2][on2].any()
    _check(h, order, exp)
    h.close()


def test_three_replicates_reuse_the_loose_slots(T0, C0):
    T1, T2 = _events(6), _events(7, n=30_000)
    h = _ctx(2000, 10)
    order, _ = _run(h, [(T0, C0), (T1, None), (T2, C0)])
    assert order == [(0, False), (0, True), (1, False), (2, False), (2, True)]
    _check(h, order, [_expected("T0", T0, 2000, 10), _expected("C0", C0, 2000, 10), _expected("T1", T1, 2000, 10),
                      _expected("T2", T2, 2000, 10), _expected("C0", C0, 2000, 10)])
    h.close()


@pytest.mark.parametrize("mode", ["packed_host", "packed_device", "device"])
def test_packed_and_device_pushes(mode, T0, C0):
    h = _ctx(2000, 10)
    order, mem = _run(h, [(T0, C0)], mode=mode)
    _check(h, order, [_expected("T0", T0, 2000, 10), _expected("C0", C0, 2000, 10)])
    h.close()
    mem.free()


@pytest.mark.parametrize("F,Bn", [(2000, 10), (1 << 20, 1 << 11)])
def test_two_contexts_with_complementary_chromosomes(F, Bn, T0, C0):
    owned = [1, 0, 1, 0, 0]
    other = [1 - x for x in owned]
    ha, hb, one = _ctx(F, Bn, owned=owned), _ctx(F, Bn, owned=other), _ctx(F, Bn)
    ev = [(T0, C0)]
    # (no collectives between them: each is a run of its own on its chromosomes, which is all the rows depend on)
    oa, _ = _run(ha, ev)
    ob, _ = _run(hb, ev)
    o1, _ = _run(one, ev)
    _check(ha, oa, [_expected("T0", T0, F, Bn, owned=owned), _expected("C0", C0, F, Bn, owned=owned)])
    _check(hb, ob, [_expected("T0", T0, F, Bn, owned=other), _expected("C0", C0, F, Bn, owned=other)])
    for i in range(2):
        a, b, c = ha.profile(i), hb.profile(i), one.profile(i)
        assert np.array_equal(a.cell120 + b.cell120, c.cell120) and np.array_equal(a.agg120 + b.agg120, c.agg120), i
        assert a.cell120.any() and b.cell120.any()
    for h in (ha, hb, one):
        h.close()


def test_profile_and_coverage_together(T0, C0):
    h = _ctx(2000, 10, cov=50)
    order, _ = _run(h, [(T0, C0)])
    _check(h, order, [_expected("T0", T0, 2000, 10), _expected("C0", C0, 2000, 10)])
    assert h.coverage_samples() == 2
    for i, key in enumerate(("T0", "C0")):
        for c in range(len(LENS)):
            assert np.array_equal(h.coverage(i, c).sum120, R.bin_sums(_PILES[key][c], 50)), (i, c)
    assert h.path_info() & GX_PATH_PROFILE and h.path_info() & GX_PATH_COVERAGE
    h.close()
    h = _ctx(64, 1, beds=BEDS, anchors=BED_ANCHORS, cov=4096)   # (-E regions: both read the tight arrays)
    order, _ = _run(h, [(T0, C0)])
    _check(h, order, [_expected("T0bed", T0, 64, 1, beds=BEDS, anchors=BED_ANCHORS),
                      _expected("C0bed", C0, 64, 1, beds=BEDS, anchors=BED_ANCHORS)])
    for i, key in enumerate(("T0bed", "C0bed")):
        for c in range(len(LENS)):
            assert np.array_equal(h.coverage(i, c).sum120, R.bin_sums(_PILES[key][c], 4096)), (i, c)
    h.close()


def test_reset_keeps_the_switch_and_a_second_run_equals_the_first(T0, C0):
    h = _ctx(2000, 10)
    order, _ = _run(h, [(T0, C0)])
    first = [h.profile(i) for i in range(2)]
    _check(h, order, [_expected("T0", T0, 2000, 10), _expected("C0", C0, 2000, 10)])
    h.reset()
    assert h.profile_samples() == 0 and not h.path_info() & GX_PATH_PROFILE
    assert h.lib.gx_get_profile(h.ctx, 0, None, None, None, None, 0, 0) == ORDER      # the results are gone ...
    assert h.profile_layout() == (len(ANCHORS), 400, 2000, 10, True)                  # ... the switch is not
    order, _ = _run(h, [(T0, C0)])
    assert h.profile_samples() == 2
    for i in range(2):
        again = h.profile(i)
        assert np.array_equal(again.cell120, first[i].cell120) and np.array_equal(again.agg120, first[i].agg120)
    h.close()


@pytest.mark.parametrize("with_ctrl", [False, True])
def test_the_switch_changes_nothing_else(with_ctrl, T0, C0):
    reps = [(T0, C0 if with_ctrl else None)]
    off, on = _ctx(0, 0), _ctx(2000, 10)
    _run(off, reps)
    _run(on, reps)
    assert off.get_peaks().tobytes() == on.get_peaks().tobytes()
    for c in range(len(LENS)):
        e0, c0 = off.get_intervals(-1, c)
        e1, c1 = on.get_intervals(-1, c)
        assert np.array_equal(e0, e1)
        for k in ("expt", "ctrl", "p"):
            assert np.array_equal(c0[k].view(np.uint32), c1[k].view(np.uint32)), k
    f0, f1 = off.path_info(), on.path_info()
    assert not f0 & GX_PATH_PROFILE and f1 == f0 | GX_PATH_PROFILE, (f0, f1)
    assert off.profile_samples() == 0 and off.profile_layout() == (0, 0, 0, 0, False)
    off.close()
    on.close()


def test_order_and_limit_errors(T0):
    import genrich_amd
    h = genrich_amd.Genrich(B.make_params(**PARAMS))
    lib, ctx = h.lib, h.ctx
    a = ANCHORS.copy()
    p, n = a.ctypes.data, len(a)
    assert lib.gx_set_profile(ctx, p, n, 2000, 10, 1) == ORDER             # before gx_set_chroms
    h.set_chroms(LENS)
    assert lib.gx_set_profile(ctx, p, n, 2000, 0, 1) == ORDER              # bin_size == 0
    assert lib.gx_set_profile(ctx, p, n, 0, 10, 1) == ORDER                # flank == 0
    assert lib.gx_set_profile(ctx, p, n, (1 << 20) + 1, (1 << 20) + 1, 1) == ORDER   # flank > 2^20
    assert lib.gx_set_profile(ctx, p, n, 2000, 7, 1) == ORDER              # flank % bin_size != 0
    assert lib.gx_set_profile(ctx, p, n, 2000, 2, 0) == ORDER              # nb = 2000 > 1024
    assert lib.gx_set_profile(ctx, p, n, 513, 1, 0) == ORDER               # nb = 1026
    bad = a.copy()
    bad["strand"][17] = 0
    assert lib.gx_set_profile(ctx, bad.ctypes.data, n, 2000, 10, 1) == ORDER   # a strand other than +1 / -1
    bad["strand"][17] = 2
    assert lib.gx_set_profile(ctx, bad.ctypes.data, n, 2000, 10, 0) == ORDER
    assert h.profile_layout() == (0, 0, 0, 0, False)                       # a refusal sets nothing
    many = np.zeros((1 << 16) + 1, dtype=P.ANCHOR_DTYPE)                    # 65537 x 1024 cells > 2^26
    many["strand"] = 1
    assert lib.gx_set_profile(ctx, many.ctypes.data, len(many), 10240, 20, 1) == ORDER
    assert lib.gx_set_profile(ctx, many.ctypes.data, len(many), 10240, 20, 0) == 0      # ... no cap without a matrix
    assert lib.gx_set_profile(ctx, many.ctypes.data, len(many) - 1, 10240, 20, 1) == 0  # 2^26 cells exactly
    assert lib.gx_set_profile(ctx, p, n, 1 << 20, 1 << 20, 1) == 0
    assert lib.gx_set_profile(ctx, None, 0, 0, 0, 0) == 0                  # off
    assert h.profile_layout() == (0, 0, 0, 0, False)
    assert lib.gx_set_profile(ctx, p, n, 2000, 10, 0) == 0
    a[:] = 0                                                               # the anchors were copied
    h.sample_begin(0, None)
    assert lib.gx_set_profile(ctx, p, n, 64, 1, 1) == ORDER                # a sample is open
    assert lib.gx_get_profile(ctx, 0, None, None, None, None, 0, 0) == ORDER
    h.push_events(T0)
    h.sample_end()
    assert lib.gx_set_profile(ctx, p, n, 64, 1, 1) == ORDER                # not idle
    assert lib.gx_get_profile(ctx, 0, None, None, None, None, 0, 0) == 0   # no gx_pvalues, no gx_find_peaks needed
    exp = _expected("T0", T0, 2000, 10)
    assert np.array_equal(h.profile(0).agg120, exp.sum(axis=0))
    buf = np.zeros((2, 400), dtype=np.int64)
    assert lib.gx_get_profile(ctx, 0, None, None, None, buf.ctypes.data, 0, 2) == ORDER   # rows, and no matrix was kept
    assert lib.gx_get_profile(ctx, 1, None, None, None, None, 0, 0) == ORDER              # no such sample
    assert lib.gx_get_profile(ctx, -1, None, None, None, None, 0, 0) == ORDER
    h.sample_begin(1, None)
    assert lib.gx_get_profile(ctx, 0, None, None, None, None, 0, 0) == ORDER              # a sample is open
    h.push_events(T0[:1000])
    h.sample_end()
    h.pvalues()
    h.find_peaks()
    assert lib.gx_set_profile(ctx, None, 0, 0, 0, 0) == ORDER              # until gx_reset
    h.reset()
    h.set_profile(ANCHORS, 2000, 10, True)
    _run(h, [(T0, None)])
    assert lib.gx_get_profile(ctx, 0, None, None, None, buf.ctypes.data, len(ANCHORS) - 1, 2) == ORDER   # rows beyond the anchors
    assert lib.gx_get_profile(ctx, 0, None, None, None, buf.ctypes.data, len(ANCHORS) + 1, 0) == ORDER
    assert lib.gx_get_profile(ctx, 0, None, None, None, buf.ctypes.data, len(ANCHORS) - 2, 2) == 0
    assert np.array_equal(buf, exp[-2:])
    assert np.array_equal(h.profile(0, rows=(7, 5)).cell120, exp[7:12])
    h.reset()
    assert lib.gx_set_profile(ctx, None, 0, 0, 0, 0) == 0
    h.close()


# ---- the command line -------------------------------------------------------------------------------------------------

def _bed_text(names, lens):
    """Anchors of a case: 3-, 4- and 6-column lines, strands +, - and ., the chromosomes' ends, one unknown chromosome."""
    lines = []
    for c, (nm, n) in enumerate(zip(names, lens)):
        if n < 40:
            continue
        m = n // 3
        lines += [f"{nm}\t{m}\t{m + 200}\tgene{c}a\t0\t+", f"{nm}\t{m}\t{m + 200}\tgene{c}b\t0\t-", f"{nm}\t{2 * m}\t{2 * m + 31}\tpeak{c}\t7\t.",
                  f"{nm}\t0\t50\tfirst{c}", f"{nm}\t{n - 10}\t{n}", f"{nm}\t{n - 1}\t{n + 3000}\tbeyond{c}\t1\t-\textra\tcolumns"]
    lines.insert(4, "chrUnknown\t100\t300\tnowhere\t0\t-")
    return "\n".join(lines) + "\n"


def _cli_expected(name, sample_names, F, Bn, at="tss"):
    """{file suffix: text}, the -v lines: from the case's events and the BED alone."""
    meta, case, _, names = G.load_case(name)
    bed = _bed_text(names, case["lens"])
    all_names, regions, row_names, strands, anchors = P.parse_bed(bed, names, at)
    counted = P.n_counted(anchors, case["lens"], case["skip"])
    files, lines, aggs = {}, [], []
    for r, rep in enumerate(case["replicates"]):
        for ctrl, ev in ((False, rep["treat"]), (True, rep["ctrl"])):
            if ev is None:
                continue
            cells = P.profile(ev, case["lens"], anchors, F, Bn, skip=case["skip"], beds=case["beds"], save=rep["save"])
            aggs.append(cells.sum(axis=0))
            files[f".{'c' if ctrl else 't'}{r}.matrix.tsv"] = P.rows_text(all_names, regions, row_names, strands, 0, cells, Bn)
            lines.append(P.enrichment_line(r, ctrl, aggs[-1], counted, Bn))
    assert counted == len(anchors) - 1 - sum(1 for a in anchors if a["chrom"] < len(names) and case["skip"][a["chrom"]])
    assert any(a.any() for a in aggs)
    files[".profile.tsv"] = P.profile_text(sample_names, aggs, counted, F, Bn)
    return bed, files, lines


@pytest.mark.parametrize("name", ["basic", "ctrl_q", "bedx"])
def test_cli_profile(name):
    meta, args, tmp, sample_names = _cli_inputs(name)
    out = os.path.join(tmp, "prof_out")
    bed, files, lines = _cli_expected(name, sample_names, 2000, 10)
    open(out + ".anchors.bed", "w").write(bed)
    res = subprocess.run([_binary(), "-v", "-o", out + ".narrowPeak", "--profile", out + ".anchors.bed", "--profile-out", out,
                          "--profile-matrix"] + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert len(files) >= 2
    for suffix, text in files.items():
        assert open(out + suffix).read() == text, suffix
    assert [l for l in res.stderr.splitlines() if l.startswith("  Profile, ")] == lines
    assert open(out + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")
    # without --profile-matrix: the table alone
    out2 = os.path.join(tmp, "prof2_out")
    res = subprocess.run([_binary(), "-o", out2 + ".narrowPeak", "--profile", out + ".anchors.bed", "--profile-out", out2] + args,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert open(out2 + ".profile.tsv").read() == files[".profile.tsv"]
    assert not [f for f in os.listdir(tmp) if f.startswith("prof2_out") and f.endswith(".matrix.tsv")]


def test_cli_gzip_two_contexts_X_and_center():
    name = "ctrl_q"
    meta, args, tmp, sample_names = _cli_inputs(name)
    bed, files, _ = _cli_expected(name, sample_names, 100, 5)
    bedfile = os.path.join(tmp, "profv.anchors.bed")
    open(bedfile, "w").write(bed)
    opts = ["--profile", bedfile, "--flank", "100", "--profile-bin", "5", "--profile-matrix"]
    out = os.path.join(tmp, "profz_out")
    res = subprocess.run([_binary(), "-z", "-o", out + ".narrowPeak", "--profile-out", out] + opts + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    for suffix, text in files.items():
        assert gzip.open(out + suffix + ".gz", "rb").read().decode() == text, suffix
    assert gzip.open(out + ".narrowPeak.gz", "rb").read() == G.read_gz(name, "out.narrowPeak")
    out2 = os.path.join(tmp, "prof2d_out")
    res = subprocess.run([_binary(), "--devices", "0,0", "-o", out2 + ".narrowPeak", "--profile-out", out2, "--coverage", out2] + opts + args,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    for suffix, text in files.items():
        assert open(out2 + suffix).read() == text, suffix
    assert open(out2 + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")
    out3 = os.path.join(tmp, "profx_out")
    res = subprocess.run([_binary(), "-X", "-f", out3 + ".log", "--profile-out", out3] + opts + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    for suffix, text in files.items():
        assert open(out3 + suffix).read() == text, suffix
    _, centred, lines = _cli_expected(name, sample_names, 100, 5, at="center")
    assert centred != files
    out4 = os.path.join(tmp, "profc_out")
    res = subprocess.run([_binary(), "-v", "-o", out4 + ".narrowPeak", "--profile-out", out4, "--profile-at", "center"] + opts + args,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    for suffix, text in centred.items():
        assert open(out4 + suffix).read() == text, suffix
    assert [l for l in res.stderr.splitlines() if l.startswith("  Profile, ")] == lines


def test_cli_refusals(tmp_path):
    meta, args, tmp, _ = _cli_inputs("basic")
    _, _, _, names = G.load_case("basic")
    bed = os.path.join(tmp, "refuse.anchors.bed")
    open(bed, "w").write(f"{names[0]}\t10\t20\tx\t0\t+\n")
    badbed = os.path.join(tmp, "refuse_bad.anchors.bed")
    open(badbed, "w").write(f"{names[0]}\t10\t20\tx\t0\t*\n")
    pre = str(tmp_path / "prof")
    both = ["--profile", bed, "--profile-out", pre]
    for extra, word in ((both + ["-P", "-f", os.path.join(tmp, "nonexistent.log")], "--profile"), (both + ["--events-only"], "--profile"),
                        (["--profile", bed], "--profile-out"), (["--profile-out", pre], "--profile"),
                        (["--flank", "100"], "--profile"), (["--profile-bin", "5"], "--profile"), (["--profile-at", "center"], "--profile"),
                        (["--profile-matrix"], "--profile"),
                        (both + ["--flank", "0"], "--flank"), (both + ["--flank", "1048577", "--profile-bin", "1048577"], "--flank"),
                        (both + ["--profile-bin", "0"], "--profile-bin"), (both + ["--profile-bin", "7"], "--profile-bin"),
                        (both + ["--profile-bin", "1"], "1024"), (both + ["--profile-at", "middle"], "--profile-at"),
                        (["--profile", badbed, "--profile-out", pre], "poorly formatted BED record")):
        res = subprocess.run([_binary(), "-o", str(tmp_path / "o.np")] + args + extra, capture_output=True, text=True)
        assert res.returncode == 1 and word in res.stderr, (extra, res.stderr)
        assert not list(tmp_path.iterdir()), extra
