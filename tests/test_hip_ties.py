"""GPU: every sweep path at exact threshold ties (tests/ties.py) against the oracle, bit for bit.

callPeaks' comparisons (Genrich.c:920-921, 1015, 1032) are restated on the device as derived thresholds -- the pileup from
which an interval is significant (lut_entry -> LooseCtl), the smallest significant p for lazy q (k_sig_from_p), q by pileup
(k_bh_small) -- and as literal compares (k_sig_mask, run_is_head, peak_finish).  Each test runs a tie the oracle shows to be
LIVE (one float or one base away its peaks change) at the tie and at both neighbours, so a compare of the wrong direction, or a
derived bound one off, fails here.  The path bits each test relies on are asserted."""
import functools

import numpy as np
import pytest

import backends as B
import synth
import ties as T
from test_hip_parity import assert_same_run, hip_backend

pytestmark = pytest.mark.gpu

FUSED, LOOSE, FELL_BACK, PAIRS, FRAC_PAIRS = 1, 2, 4, 16, 128
MERGE_P, PACK_HIST, LAZY_Q, LATE_LOOSE, Q_LOOSE = 1024, 2048, 8192, 16384, 32768

P = dict(pq=0.01, min_auc=20.0)
Q = dict(pq=0.05, qval=True, min_auc=20.0)


def _set(monkeypatch, knobs):
    for k in knobs:
        monkeypatch.setenv(k, "1")


def _parity(case, par, expect_fractional=False, runs=1):
    """the oracle and the library on one case; returns the library's path bits (of the last run on its context)"""
    o = B.Oracle(par)
    so = B.run_case(o, case)
    h = hip_backend(par)
    if expect_fractional:
        h.expect_fractional(True)
    for k in range(runs):
        if k:
            h.reset()
        sh = B.run_case(h, case)
        assert_same_run(o, h, so, sh, case)
    flags = h.path_info()
    h.close()
    o.close()
    return flags


def _run_tie(t, case, check_flags, **kw):
    assert t.live(), f"{t.kind}: not live ({t.note})"
    for v in t.values():
        flags = _parity(case, T.params(t.base, **{t.param: v}), **kw)
        check_flags(flags)
    return flags


# ---- the cases and their ties (oracle only: computed once per session) --------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(name):
    if name == "noctrl":
        return T.case_noctrl()
    if name == "ctrl":
        return T.case_ctrl()
    if name == "frac":
        lens = [300_000, 70_001]
        ev = synth.add_multimap(synth.make_fragments(lens, 60_000, 31, peak_every=20_000, tower_every=150_000), lens, 0.3, 32)
        return dict(lens=lens, replicates=[dict(save=None, treat=ev, ctrl=None)])
    if name == "reps3":
        lens = [150_000, 60_000]
        reps = []
        for r in range(3):
            tr = synth.make_fragments(lens, 25_000, 31 + r, peak_every=15_000, tower_every=70_000)
            ct = synth.make_fragments(lens, 20_000, 41 + r, uniform_only=True) if r != 1 else None
            reps.append(dict(save=None, treat=tr, ctrl=ct))
        return dict(lens=lens, replicates=reps)
    if name == "bed":
        c = T.case_noctrl(seed=41)
        return dict(c, beds=[[0, 9_000, 50_000, 50_001, 123_000, 123_900, 300_000, 320_000], [5_000, 6_000]])
    if name == "long":   # one candidate of > PK_SHORT = 1024 intervals (k_peak_walk: the AUC in DPP replay)
        rng = np.random.default_rng(11)
        lens = [500_000]
        bg = synth.make_fragments(lens, 4_000, seed=5)
        st = rng.integers(200_000, 230_000, 25_000).astype(np.uint32)
        big = np.zeros(len(st), dtype=B.EVENT_DTYPE)
        big["start"], big["end"], big["count"] = st, st + rng.integers(150, 400, len(st)).astype(np.uint32), 1
        return dict(lens=lens, replicates=[dict(save=None, treat=np.concatenate([bg, big]), ctrl=None)])
    raise KeyError(name)


def _base(kind):
    return B.make_params(**(Q if kind == "q" else P))


@functools.lru_cache(maxsize=None)
def _pq_ties(name, kind):
    return T.pq_ties(_case(name), _base(kind))


@functools.lru_cache(maxsize=None)
def _shape_ties(name, kind):
    """(AUC tie, length tie, gap tie) of a case"""
    case, base = _case(name), _base(kind)
    pick = "max" if name == "long" else "median"
    return T.auc_tie(case, base, pick=pick)[0], T.len_tie(case, base)[0], T.gap_tie(case, base)


# ---- the configurations --------------------------------------------------------------------------------------------

def _want(bits_on=0, bits_off=0):
    def check(flags):
        assert flags & bits_on == bits_on and not flags & bits_off, (flags, bits_on, bits_off)
    return check


CONFIGS = {
    # name: (case, p / q, knobs, bits on, bits off, shape ties too)
    "p_default": ("noctrl", "p", (), FUSED | LOOSE, FELL_BACK, True),
    "p_tight": ("noctrl", "p", ("GX_NO_LOOSE",), FUSED, LOOSE, True),
    "p_general": ("noctrl", "p", ("GX_NO_FUSED",), 0, FUSED, False),
    "q_loose": ("noctrl", "q", (), FUSED | LOOSE | Q_LOOSE, 0, True),
    "q_lazy": ("noctrl", "q", ("GX_NO_Q_LOOSE",), LAZY_Q, Q_LOOSE, False),
    "q_eager": ("noctrl", "q", ("GX_NO_Q_LOOSE", "GX_NO_LAZY_Q"), 0, Q_LOOSE | LAZY_Q, False),
    "q_no_pack_hist": ("noctrl", "q", ("GX_NO_Q_LOOSE", "GX_NO_PACK_HIST"), 0, Q_LOOSE | PACK_HIST, False),
    "ctrl_p": ("ctrl", "p", (), FUSED | MERGE_P, 0, True),
    "ctrl_q": ("ctrl", "q", (), FUSED | MERGE_P, 0, True),
    "ctrl_p_no_merge_p": ("ctrl", "p", ("GX_NO_MERGE_P",), FUSED, MERGE_P, False),
    "ctrl_q_no_merge_p": ("ctrl", "q", ("GX_NO_MERGE_P",), FUSED, MERGE_P, False),
    "ctrl_p_merge_wg": ("ctrl", "p", ("GX_MERGE_WG",), FUSED | MERGE_P, 0, False),
    "ctrl_q_merge_wg": ("ctrl", "q", ("GX_MERGE_WG",), FUSED | MERGE_P, 0, False),
    "reps3_p": ("reps3", "p", (), 0, 0, False),
    "reps3_q": ("reps3", "q", (), 0, 0, False),
    "bed_p": ("bed", "p", (), FUSED, 0, False),
    "long_p": ("long", "p", (), FUSED, 0, True),
}


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_pq_ties_on_every_sweep_path(monkeypatch, config):
    """thr = a p (q) present in the run -- a common value and a summit's --, and one float either side"""
    name, kind, knobs, on, off, _ = CONFIGS[config]
    _set(monkeypatch, knobs)
    for t in _pq_ties(name, kind):
        _run_tie(t, _case(name), _want(on, off))


@pytest.mark.parametrize("config", sorted(c for c in CONFIGS if CONFIGS[c][5]))
def test_auc_length_and_gap_ties(monkeypatch, config):
    """min_auc = a peak's float AUC (long_p: the DPP-replayed sum of the widest candidate), min_len = a peak's length,
    max_gap = the distance between two significant runs -- each with its neighbours"""
    name, kind, knobs, on, off, _ = CONFIGS[config]
    _set(monkeypatch, knobs)
    auc, ln, gap = _shape_ties(name, kind)
    for t in (auc, ln, gap):
        _run_tie(t, _case(name), _want(on, off))
    if name == "long":   # the AUC tie sits on the candidate of > 1024 intervals
        r = auc.runs[auc.at]
        e = r.ends[0]
        pk = r.peaks[r.peaks["auc"] == np.float32(auc.at)]
        assert len(pk) == 1 and np.searchsorted(e, pk["end"][0]) - np.searchsorted(e, pk["start"][0]) > 1024


def test_fractional_weights_at_a_p_tie():
    """multimapping weights: the hinted context's second run sweeps the loose slots with bits written late (k_loose_late)"""
    case = _case("frac")
    for t in _pq_ties("frac", "p"):
        _run_tie(t, case, _want(FUSED | FRAC_PAIRS | LATE_LOOSE | LOOSE, FELL_BACK), expect_fractional=True, runs=2)


def test_a_skip_between_two_runs_splits_them_at_any_max_gap():
    case = _case("noctrl")
    t = _shape_ties("noctrl", "p")[2]
    bc, runs = T.bed_gap_case(case, t.base, t)
    c, a_end, b_start = t.where
    for mg, r in runs.items():
        assert not T.linked(r, c, a_end, b_start) and T.linked(t.runs[t.at], c, a_end, b_start)
        _want(FUSED)(_parity(bc, T.params(t.base, max_gap=mg)))


def test_risky_table_entry_at_the_threshold():
    """thr = a p-value whose double lies next to a float rounding midpoint (the device flags it, the host re-evaluates it after
    the tile stage has compared the device's float): riskNearThr must send the sweep to the tight table when thr is that entry
    or the float below it, and the loose slots stay for a far threshold on the same data"""
    case = _case("noctrl")
    t, tried = T.risky_tie(case, _base("p"))
    print(f"risky tie after {tried} genome lengths: {t.note}")
    assert t.live()
    for v in t.values():
        flags = _parity(case, T.params(t.base, thr=v))
        assert flags & FUSED
        if v in (t.at, T.down(t.at)):
            assert not flags & LOOSE, (v, flags)
    far = T.params(t.base, thr=T.f32(2.0))
    assert _parity(case, far) & LOOSE


@pytest.mark.parametrize("knobs", [(), ("GX_NO_LOOSE",)])
@pytest.mark.parametrize("kind", ["p", "q"])
def test_summit_plateaus(monkeypatch, knobs, kind):
    """updatePeak (958-966): equal plateaus keep the first as the summit, a later longer one takes summitPos; with -q, equal q
    and different p keep the first plateau's p (the ties_summit fixtures pin the oracle to the reference)"""
    _set(monkeypatch, knobs)
    case = T.summit_case(T.summit_q_pair())
    flags = _parity(case, _base(kind))
    assert flags & FUSED and bool(flags & LOOSE) == (not knobs), flags
