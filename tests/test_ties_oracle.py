"""The tie finders of tests/ties.py on the CPU oracle: every tie they return is live (one float / one base away the peaks
change), and the oracle's keep / drop decisions at the tie follow callPeaks' comparisons (Genrich.c:920-921, 1015, 1032).
The GPU suite (tests/test_hip_ties.py) drives the same ties through every sweep path; the oracle's own direction at ties is
pinned to the reference by the ties_* golden fixtures (tests/test_oracle.py)."""
import numpy as np
import pytest

import backends as B
import ties as T


def _edges(run, col):
    """the p (q) values of each peak's first and last interval and of its summit interval"""
    out = []
    for pk in run.peaks:
        c = int(pk["chrom"])
        e = run.ends[c].astype(np.int64)
        i0 = np.searchsorted(e, int(pk["start"]), side="right")
        i1 = np.searchsorted(e, int(pk["end"]))
        v = run.cols[c][col]
        out += [float(v[i0]), float(v[i1])]
    return out


def _filtered(run, keep):
    return [k for k, ok in zip(run.key(), keep) if ok]


@pytest.mark.parametrize("qval,ctrl", [(False, False), (True, False), (False, True), (True, True)])
def test_pq_ties_are_live_and_strict(qval, ctrl):
    case = T.case_ctrl() if ctrl else T.case_noctrl()
    base = B.make_params(pq=0.05 if qval else 0.01, qval=qval, min_auc=20.0)
    col = "q" if qval else "p"
    ties = T.pq_ties(case, base)
    assert {t.kind for t in ties} == {f"{col}_common", f"{col}_summit"}
    for t in ties:
        assert t.live(), t.note
        at, away = t.runs[t.at], t.runs[t.away]
        # pqval > minPQval: at thr == value the intervals holding it are not significant, so no peak starts, ends or peaks on one
        assert all(v > np.float32(t.at) for v in _edges(at, col)), t.note
        assert np.float32(t.at) in [np.float32(v) for v in _edges(away, col)] or len(away.peaks) != len(at.peaks), t.note
        for r, thr in ((at, t.at), (away, t.away)):
            if qval:
                assert (r.peaks["q"] > np.float32(thr)).all()
            else:
                assert (r.peaks["p"] > np.float32(thr)).all()


@pytest.mark.parametrize("qval", [False, True])
def test_auc_and_length_ties_keep_the_equal_peak(qval):
    case = T.case_noctrl()
    base = B.make_params(pq=0.05 if qval else 0.01, qval=qval, min_auc=20.0, max_gap=100)
    t, r0 = T.auc_tie(case, base)
    for a in t.values():   # auc >= minAUC (920): the candidates of the unfiltered run whose AUC reaches a
        assert t.runs[a].key() == _filtered(r0, r0.peaks["auc"] >= np.float32(a)), a
    assert np.float32(t.at) in t.runs[t.at].peaks["auc"] and np.float32(t.at) not in t.runs[t.away].peaks["auc"]
    t, r0 = T.len_tie(case, T.params(base, min_auc=0.0))
    ln = r0.peaks["end"].astype(np.int64) - r0.peaks["start"]
    for L in t.values():   # end - start >= minLen (921)
        assert t.runs[L].key() == _filtered(r0, ln >= L), L
    assert t.live()


@pytest.mark.parametrize("qval", [False, True])
def test_gap_tie_links_at_max_gap_and_a_skip_splits(qval):
    case = T.case_noctrl()
    base = B.make_params(pq=0.05 if qval else 0.01, qval=qval, min_auc=20.0)
    t = T.gap_tie(case, base)
    c, a_end, b_start = t.where
    assert b_start - a_end == t.at
    # end[m] - peakEnd > maxGap (1032): a gap equal to maxGap links, one base more splits
    assert T.linked(t.runs[t.at], c, a_end, b_start) and T.linked(t.runs[t.at + 1], c, a_end, b_start)
    assert not T.linked(t.runs[t.at - 1], c, a_end, b_start)
    assert t.live()
    # a -E region between the two runs: SKIP ends the peak (1031) whatever maxGap says
    bc, runs = T.bed_gap_case(case, t.base, t)
    for mg, r in runs.items():
        assert not T.linked(r, c, a_end, b_start), mg
        assert r.key() != t.runs[t.at].key()


def test_risky_p_value_at_the_threshold():
    case = T.case_noctrl()
    t, tried = T.risky_tie(case, B.make_params(pq=0.01, min_auc=20.0))
    print(f"risky tie after {tried} genome lengths: {t.note}")
    assert 0 < tried <= 4000
    assert t.live(), t.note
    at = t.runs[t.at]
    assert all(v > np.float32(t.at) for v in _edges(at, "p"))


def test_summit_plateaus():
    """updatePeak (958-966): of two plateaus at a peak's maximum the first stays the summit unless the later one is longer;
    with -q, equal q and different p, summitPos moves to the later, longer plateau and the first one's p is kept."""
    qp = T.summit_q_pair()
    case = T.summit_case(qp)
    r = T.run_oracle(case, B.make_params(pq=0.01, min_auc=20.0))
    pk = {int(p["start"]): p for p in r.peaks}
    for kind, base, a, b in T.SUMMIT_PEAKS:
        want = (a if kind == "equal" else b)
        assert int(pk[base[0]]["summit"]) == (want[0] + want[1]) // 2 - base[0], kind
    r = T.run_oracle(case, B.make_params(pq=0.05, qval=True, min_auc=20.0))
    e = r.ends[0].astype(np.int64)
    ia, ib = np.searchsorted(e, 48_000), np.searchsorted(e, 48_350)
    (p3,) = [p for p in r.peaks if p["start"] <= 48_000 < p["end"]]
    assert p3["summit"] == (48_050 + 48_350) // 2 - p3["start"]
    assert p3["p"] == r.cols[0]["p"][ia] != r.cols[0]["p"][ib] and p3["q"] == r.cols[0]["q"][ib]


def test_pq_string_lands_on_the_tie():
    """the decimal -p / -q of the golden tie fixtures: -log10f(strtof(s)) is the float asked for (getArgs 5817)"""
    for t in (0.5, 1.3010299, 2.0, 4.177402973175049, 12.011187553405762):
        t = T.f32(t)
        s = T.pq_string(t)
        assert s is not None and B.minus_log10f(T.strtof(s)) == t, (t, s)
