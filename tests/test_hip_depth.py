"""The depth distribution of every sample's pileup on the GPU (gx_set_depth_hist / k_depth_hist, genrich-amd --depth): exact
equality of every integer with the numpy definition (tests/depth_ref.py), on every tile-stage path, in every form the sample can
be in when it is closed, across the class / list boundary and the list's rerun.  The shapes are tests/test_hip_coverage.py's."""
import ctypes
import gzip
import os
import subprocess

import numpy as np
import pytest

import backends as B
import depth_ref as R
import coverage_ref as CR
import golden_cases as G
from genrich_amd.lib import GX_PATH_COVERAGE, GX_PATH_DEPTH, depth_geometry, depth_group, depth_text
from test_hip_counts import _cli_inputs
from test_hip_coverage import LENS, PARAMS, _events, _run
from test_host_cli import _binary

pytestmark = pytest.mark.gpu

ORDER = -10
BOUND = R.DEPTH_BOUND
# -E regions as gx_set_chroms takes them (merged, sorted): one from base 0, one that covers exactly the second tile, one that ends at
# a tile edge, one inside a tile, one that reaches beyond the chromosome's end
BEDS = [[0, 100, 4096, 8192, 12_000, 12_288], [], [4090, 4097], [], [20_010, 20_030, 36_000, 45_000, 199_000, 300_000]]

_PILES = {}


def _expected(key, ev, rep=0, ctrl=False, skip=None, beds=None, save=None, owned=None):
    """depth_ref's histogram; the per-base pileups of a sample are computed once (`key` names the sample and its -E regions)."""
    if key not in _PILES:
        _PILES[key] = {c: CR.pileup120(ev, c, LENS[c], beds[c] if beds is not None else ()) for c in range(len(LENS))}
    return R.hist(ev, LENS, skip=skip, beds=beds, save=save, owned=owned, rep=rep, is_ctrl=ctrl, piles=_PILES[key])


def _ctx(on=True, skip=None, beds=None, owned=None, knobs=(), frac=False, params=None, W=0):
    import genrich_amd
    h = genrich_amd.Genrich(B.make_params(**(params or PARAMS)))
    h.set_chroms(LENS, skip, beds)
    if owned is not None:
        h.set_owned(owned)
    for k, v in knobs:
        h.set_knob(k, v)
    if frac:
        h.expect_fractional(True)
    if W:
        h.set_coverage_bins(W)
    if on:
        h.set_depth_hist(True)
    return h


def _check(h, order, expected):
    """expected[i] = the Hist of sample i: every integer, exactly."""
    assert h.depth_samples() == len(order) == len(expected)
    for i, ((r, ctrl), exp) in enumerate(zip(order, expected)):
        got = h.depth(i)
        assert (got.rep, got.is_ctrl) == (r, ctrl) == (exp.rep, exp.is_ctrl)
        assert got.bases.dtype == np.uint64
        assert R.same(got, exp) is None, (i, R.same(got, exp))


def _tower(T0, n, seed=3):
    """n staggered fragments in one tile of chromosome 4, in the middle of T0."""
    tower = np.zeros(n, dtype=B.EVENT_DTYPE)
    rng = np.random.default_rng(seed)
    tower["chrom"] = 4
    tower["start"] = 2 * 4096 + 100 + rng.integers(0, 300, n)
    tower["end"] = tower["start"] + rng.integers(50, 900, n)
    tower["count"] = 1
    return np.concatenate([T0[:12_000], tower, T0[12_000:]])


@pytest.fixture(scope="module")
def T0():
    return _events(1)


@pytest.fixture(scope="module")
def C0():
    return _events(2, n=20_000)


def test_the_default_path_treatment_and_control(T0, C0):
    h = _ctx()
    order, _ = _run(h, [(T0, C0)])
    et, ec = _expected("T0", T0), _expected("C0", C0, ctrl=True)
    assert et.total == sum(LENS) and et.excluded == 0 and et.zero > 37 and et.bases[1:5].all() and not et.rsum.any()
    assert et.min_v == 120 and et.max_v % 120 == 0 and et.max_v // 120 < BOUND and not et.deep
    _check(h, order, [et, ec])
    assert h.path_info() & GX_PATH_DEPTH
    assert h.depth_last() == (depth_geometry()[3], 0)
    h.close()


@pytest.mark.parametrize("knob", [("GX_NO_FUSED", 1), ("GX_NO_PAIRS", 1), ("GX_SBT_GRID", 1)])
def test_forced_tile_stage_paths(knob, T0, C0):
    h = _ctx(knobs=[knob])
    order, _ = _run(h, [(T0, C0)])
    _check(h, order, [_expected("T0", T0), _expected("C0", C0, ctrl=True)])
    flags = h.path_info()
    assert not (knob[0] == "GX_NO_FUSED" and flags & 1) and not (knob[0] == "GX_NO_PAIRS" and flags & 16), flags   # (the path was forced)
    h.close()


@pytest.mark.parametrize("n", [BOUND - 1, BOUND, BOUND + 1])
def test_a_pile_at_the_boundary_between_class_and_list(n, T0):
    """n identical fragments over 500 bases that nothing else covers: the bases at depth n are in class n (n < BOUND) or in the
    list with v = 120 n."""
    pile = np.zeros(n, dtype=B.EVENT_DTYPE)
    pile["chrom"], pile["start"], pile["end"], pile["count"] = 4, 60_000, 60_500, 1
    quiet = T0[~((T0["chrom"] == 4) & (T0["end"] > 60_000) & (T0["start"] < 60_500))]
    ev = np.concatenate([quiet[:9000], pile, quiet[9000:]])
    h = _ctx()
    order, _ = _run(h, [(ev, None)])
    exp = _expected(("pile", n), ev)
    if n < BOUND:
        assert not exp.deep and exp.bases[n] == 500 and exp.max_v == 120 * n
    else:
        assert exp.deep == [(120 * n, 500)] and exp.max_v == 120 * n
    _check(h, order, [exp])
    h.close()


@pytest.mark.parametrize("cap", [0, 4])
def test_a_staggered_pile_of_5000_in_one_tile(cap, T0):
    ev = _tower(T0, 5000)
    exp = _expected("tower", ev)
    assert len(exp.deep) > 100 and exp.bases[BOUND - 200:].any()     # many deep pieces with distinct v, and classes right below the bound
    h = _ctx(knobs=[("GX_DEPTH_LIST_CAP", cap)] if cap else [])
    order, _ = _run(h, [(ev, None)])
    _check(h, order, [exp])
    got_cap, reruns = h.depth_last()
    if cap:
        assert reruns == 1 and got_cap >= len(exp.deep) > cap          # exactly one rerun, with a list of the counted size
    else:
        assert reruns == 0 and got_cap == depth_geometry()[3]
    h.close()


def test_fractional_weights():
    ev = _events(4, counts=(1, 2, 3, 4, 5, 6, 8, 10))
    h = _ctx(frac=True)
    order, _ = _run(h, [(ev, None)])
    exp = _expected("frac", ev)
    assert exp.rsum[1:40].all() and exp.bases[0] and 0 < exp.min_v < 120 and (exp.rsq > exp.rsum).any()
    _check(h, order, [exp])
    h.close()


def test_fractional_weights_in_the_deep_list(T0):
    ev = _tower(T0, 5000)
    ev["count"][::7] = 3
    ev["count"][::11] = 8
    h = _ctx(frac=True)
    order, _ = _run(h, [(ev, None)])
    exp = _expected("fractower", ev)
    assert any(v % 120 for v, _ in exp.deep) and exp.rsq.any()
    _check(h, order, [exp])
    h.close()


def test_excluded_regions(T0, C0):
    h = _ctx(beds=BEDS)
    order, _ = _run(h, [(T0, C0)])
    et, ec = _expected("T0bed", T0, beds=BEDS), _expected("C0bed", C0, ctrl=True, beds=BEDS)
    assert et.excluded == 100 + 4096 + 288 + 7 + 20 + 9000 + 1000 and R.same(et, _expected("T0", T0)) is not None
    _check(h, order, [et, ec])
    h.close()
    h = _ctx(beds=BEDS)   # ... and without a control
    order, _ = _run(h, [(T0, None)])
    _check(h, order, [et])
    h.close()


def test_excluded_regions_and_coverage_bins_share_the_tight_arrays(T0, C0):
    h = _ctx(beds=BEDS, W=50)
    order, _ = _run(h, [(T0, C0)])
    _check(h, order, [_expected("T0bed", T0, beds=BEDS), _expected("C0bed", C0, ctrl=True, beds=BEDS)])
    for i, key, ev in ((0, "T0bed", T0), (1, "C0bed", C0)):
        for c in (0, 4):
            assert np.array_equal(h.coverage(i, c).sum120, CR.bin_sums(_PILES[key][c], 50)), (i, c)
    h.close()


def test_a_skipped_chromosome(T0):
    skip = [0, 0, 1, 0, 0]
    h = _ctx(skip=skip)
    order, _ = _run(h, [(T0, None)])
    exp = _expected("T0", T0, skip=skip)
    assert exp.total == sum(LENS) - LENS[2]
    _check(h, order, [exp])
    h.close()


def test_a_save_mask_that_omits_a_chromosome_for_one_replicate(T0, C0):
    save = [1, 1, 0, 1, 1]
    h = _ctx()
    order, _ = _run(h, [(T0, C0), (T0, None)], saves=[save, None])
    exp = [_expected("T0", T0, save=save), _expected("C0", C0, ctrl=True, save=save), _expected("T0", T0, rep=1)]
    assert exp[0].total == exp[2].total == sum(LENS) and exp[0].zero > exp[2].zero   # (the chromosome counts, at pileup 0)
    _check(h, order, exp)
    h.close()


def test_the_37_base_chromosome_with_no_events(T0):
    ev = T0[T0["chrom"] != 3]
    h = _ctx()
    order, _ = _run(h, [(ev, None)])
    exp = _expected("T0no3", ev)
    assert exp.total == sum(LENS) and exp.zero == _expected("T0", T0).zero + int((_PILES["T0"][3] > 0).sum())
    _check(h, order, [exp])
    h.close()


def test_three_replicates_reuse_the_loose_slots(T0, C0):
    T1, T2 = _events(6), _events(7, n=30_000)
    h = _ctx()
    order, _ = _run(h, [(T0, C0), (T1, None), (T2, C0)])
    assert order == [(0, False), (0, True), (1, False), (2, False), (2, True)]
    _check(h, order, [_expected("T0", T0), _expected("C0", C0, ctrl=True), _expected("T1", T1, rep=1), _expected("T2", T2, rep=2),
                      _expected("C0", C0, rep=2, ctrl=True)])
    h.close()


@pytest.mark.parametrize("mode", ["packed_host", "packed_device", "device"])
def test_packed_and_device_pushes(mode, T0, C0):
    h = _ctx()
    order, mem = _run(h, [(T0, C0)], mode=mode)
    _check(h, order, [_expected("T0", T0), _expected("C0", C0, ctrl=True)])
    h.close()
    mem.free()


def test_two_contexts_with_complementary_chromosomes(T0):
    ev = _tower(T0, 5000)
    owned = [1, 0, 1, 0, 0]
    other = [1 - x for x in owned]
    ha, hb, one = _ctx(owned=owned, beds=BEDS), _ctx(owned=other, beds=BEDS), _ctx(beds=BEDS)
    reps = [(ev, None)]
    # (no collectives between them: each is a run of its own on its chromosomes, which is all the distribution depends on)
    oa, _ = _run(ha, reps)
    ob, _ = _run(hb, reps)
    o1, _ = _run(one, reps)
    ea, eb = _expected("towerbed", ev, owned=owned, beds=BEDS), _expected("towerbed", ev, owned=other, beds=BEDS)
    _check(ha, oa, [ea])
    _check(hb, ob, [eb])
    whole = _expected("towerbed", ev, beds=BEDS)
    assert not ea.deep and eb.deep and R.same(R.add(ea, eb), whole) is None
    _check(one, o1, [whole])
    assert R.same(depth_group([ha, hb], 0), whole) is None and R.same(depth_group([one], 0), whole) is None
    assert depth_text([ha, hb]) == depth_text([one]) == (R.depth_text([whole]).encode(), R.metrics_text([whole]).encode())
    for h in (ha, hb, one):
        h.close()


@pytest.mark.parametrize("knobs", [[("GX_DEPTH_GRID", 1)], [("GX_DEPTH_GRID", 3), ("GX_DEPTH_PRIV", 1)], [("GX_DEPTH_PRIV", 1)]])
def test_every_geometry_gives_the_default_result(knobs, T0, C0):
    ev = _tower(T0, 5000)
    h = _ctx(knobs=knobs)
    order, _ = _run(h, [(ev, C0)])
    _check(h, order, [_expected("tower", ev), _expected("C0", C0, ctrl=True)])
    h.close()


def test_reset_keeps_the_switch_and_a_second_run_equals_the_first(T0, C0):
    h = _ctx()
    order, _ = _run(h, [(T0, C0)])
    _check(h, order, [_expected("T0", T0), _expected("C0", C0, ctrl=True)])
    h.reset()
    assert h.depth_samples() == 0 and not h.path_info() & GX_PATH_DEPTH
    assert h.lib.gx_get_depth(h.ctx, 0, None, None, None, None, None, None, 0, None) == ORDER     # the results are gone, the switch is not
    order, _ = _run(h, [(T0, C0)])
    _check(h, order, [_expected("T0", T0), _expected("C0", C0, ctrl=True)])
    h.close()


@pytest.mark.parametrize("with_ctrl", [False, True])
def test_the_switch_changes_nothing_else(with_ctrl, T0, C0):
    reps = [(T0, C0 if with_ctrl else None)]
    off, on = _ctx(on=False, W=50), _ctx(W=50)
    _run(off, reps)
    _run(on, reps)
    assert off.get_peaks().tobytes() == on.get_peaks().tobytes()
    for c in range(len(LENS)):
        e0, c0 = off.get_intervals(-1, c)
        e1, c1 = on.get_intervals(-1, c)
        assert np.array_equal(e0, e1)
        for k in ("expt", "ctrl", "p"):
            assert np.array_equal(c0[k].view(np.uint32), c1[k].view(np.uint32)), k
        for i in range(1 + with_ctrl):
            assert np.array_equal(off.coverage(i, c).sum120, on.coverage(i, c).sum120)
    f0, f1 = off.path_info(), on.path_info()
    assert f0 & GX_PATH_COVERAGE and not f0 & GX_PATH_DEPTH and f1 == f0 | GX_PATH_DEPTH, (f0, f1)
    assert off.depth_samples() == 0
    off.close()
    on.close()


def test_order_errors(T0):
    import genrich_amd
    h = genrich_amd.Genrich(B.make_params(**PARAMS))
    lib, ctx = h.lib, h.ctx
    none = (None,) * 6 + (0, None)
    assert lib.gx_set_depth_hist(ctx, 1) == ORDER                      # before gx_set_chroms
    h.set_chroms(LENS)
    assert lib.gx_set_depth_hist(ctx, 1) == 0
    assert lib.gx_set_depth_hist(ctx, 0) == 0
    assert lib.gx_set_depth_hist(ctx, 1) == 0
    h.sample_begin(0, None)
    assert lib.gx_set_depth_hist(ctx, 0) == ORDER                      # a sample is open
    assert lib.gx_get_depth(ctx, 0, *none) == ORDER
    h.push_events(T0)
    h.sample_end()
    assert lib.gx_set_depth_hist(ctx, 0) == ORDER                      # not idle
    assert lib.gx_get_depth(ctx, 0, *none) == 0                        # no gx_pvalues, no gx_find_peaks needed
    assert R.same(h.depth(0), _expected("T0", T0)) is None
    assert lib.gx_get_depth(ctx, 1, *none) == ORDER                    # no such sample
    assert lib.gx_get_depth(ctx, -1, *none) == ORDER
    assert lib.gx_get_depth(ctx, 0, None, None, None, None, None, None, 4, None) == ORDER   # cap without arrays
    h.sample_begin(1, None)
    assert lib.gx_get_depth(ctx, 0, *none) == ORDER                    # a sample is open
    h.push_events(T0[:1000])
    h.sample_end()
    h.pvalues()
    h.find_peaks()
    assert lib.gx_set_depth_hist(ctx, 0) == ORDER                      # until gx_reset
    arr = (ctypes.c_void_p * 1)(ctx)
    assert lib.gx_depth_group(arr, 0, 0, *none) == ORDER and lib.gx_depth_group(arr, 1, 2, *none) == ORDER
    assert lib.gx_write_depth_group(arr, 1, None, None) == ORDER
    h.reset()
    assert lib.gx_set_depth_hist(ctx, 0) == 0
    h.sample_begin(0, None)
    h.push_events(T0[:1000])
    h.sample_end()
    assert h.depth_samples() == 0 and not h.path_info() & GX_PATH_DEPTH    # off: nothing ran
    h.close()


# ---- the command line -------------------------------------------------------------------------------------------------

def _cli_expected(name, extra_beds=None):
    """(--depth's text, --depth-metrics', the -v lines): from the case's events alone."""
    meta, case, _, names = G.load_case(name)
    samples = []
    for r, rep in enumerate(case["replicates"]):
        for ctrl, ev in ((False, rep["treat"]), (True, rep["ctrl"])):
            if ev is None:
                continue
            beds = extra_beds if extra_beds is not None else case["beds"]
            samples.append(R.hist(ev, case["lens"], skip=case["skip"], beds=beds, save=rep["save"], rep=r, is_ctrl=ctrl))
    return R.depth_text(samples), R.metrics_text(samples), [R.verbose_line(h) for h in samples]


@pytest.mark.parametrize("name", ["basic", "ctrl_q", "bedx"])
def test_cli_depth(name):
    meta, args, tmp, _ = _cli_inputs(name)
    out = os.path.join(tmp, "depth_out")
    res = subprocess.run([_binary(), "-v", "-o", out + ".narrowPeak", "--depth", out + ".tsv", "--depth-metrics", out + ".metrics.tsv"] + args,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    text, metrics, lines = _cli_expected(name)
    assert len(text.splitlines()) > 3
    assert open(out + ".tsv").read() == text
    assert open(out + ".metrics.tsv").read() == metrics
    assert [l for l in res.stderr.splitlines() if l.startswith("  Depth, ")] == lines
    assert open(out + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")


def test_cli_gzip_two_contexts_X_and_each_option_alone():
    name = "ctrl_q"
    meta, args, tmp, _ = _cli_inputs(name)
    text, metrics, _ = _cli_expected(name)
    out = os.path.join(tmp, "depthz_out")
    res = subprocess.run([_binary(), "-X", "-z", "--devices", "0,0", "-f", out + ".log", "--depth", out + ".tsv", "--depth-metrics", out + ".m.tsv",
                          "--coverage", out] + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert gzip.open(out + ".tsv.gz", "rb").read().decode() == text
    assert gzip.open(out + ".m.tsv.gz", "rb").read().decode() == metrics
    out2 = os.path.join(tmp, "depth2_out")
    res = subprocess.run([_binary(), "-o", out2 + ".narrowPeak", "--depth-metrics", out2 + ".m.tsv"] + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert open(out2 + ".m.tsv").read() == metrics and not os.path.exists(out2 + ".tsv")
    assert open(out2 + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")
    out3 = os.path.join(tmp, "depth3_out")
    res = subprocess.run([_binary(), "-o", out3 + ".narrowPeak", "--depth", out3 + ".tsv"] + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert open(out3 + ".tsv").read() == text and not os.path.exists(out3 + ".m.tsv")


def test_cli_excluded_regions_that_overlap_nest_and_pass_the_end(tmp_path):
    """The -E file's lines as a user writes them: overlapping, nested, repeated, beyond the chromosome's end, a whole tile."""
    name = "basic"
    meta, args, tmp, _ = _cli_inputs(name)
    _, case, _, names = G.load_case(name)
    assert "-E" not in args and not any(len(b) for b in case["beds"])
    c = int(np.argmax(case["lens"]))
    L = int(case["lens"][c])
    assert L > 3 * 4096
    regions = [(10, 500), (300, 800), (400, 450), (300, 800), (4096, 8192), (5000, 6000), (L - 100, L + 5000)]
    bed = tmp_path / "x.bed"
    bed.write_text("".join(f"{names[c]}\t{a}\t{b}\n" for a, b in regions))
    beds = [[] for _ in case["lens"]]
    beds[c] = [x for ab in regions for x in ab]
    text, metrics, _ = _cli_expected(name, extra_beds=beds)
    out = str(tmp_path / "depth")
    res = subprocess.run([_binary(), "-o", out + ".narrowPeak", "-E", str(bed), "--depth", out + ".tsv", "--depth-metrics", out + ".m.tsv"] + args,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert metrics.splitlines()[1].split("\t")[2] == str(790 + 4096 + 100)
    assert open(out + ".tsv").read() == text
    assert open(out + ".m.tsv").read() == metrics
