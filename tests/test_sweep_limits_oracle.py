"""The proof, without a GPU, that the inputs of test_hip_sweep_limits.py are what it claims: every case of tests/sweep_limits.py
is built, the oracle runs it, sweep_census() rebuilds the sweep's index space from the oracle's table (and checks itself against
the oracle's peaks), and the case's `also` asserts the structural fact it exists for -- the bit, the word, the chunk, the run or
candidate number, the candidate's length in index units.  The AUC-order candidates and the ties are shown to be live."""
import numpy as np
import pytest

import sweep_limits as S
import ties as T


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_case_preconditions_on_the_oracle_alone(name):
    cen = S.check(name)
    print(name, "N", cen.N, "runs", len(cen.runs), "candidates", len(cen.cands))


@pytest.mark.parametrize("name", sorted(n for n in S.CASES if any("-q" in p for p in S.CASES[n][2])))
def test_case_preconditions_with_q_values(name):
    """the same structure when significance is decided on q: the threshold lies between the quiet and the significant levels"""
    cen = S.check(name, qval=True)
    print(name, "N", cen.N, "runs", len(cen.runs), "candidates", len(cen.cands))


def test_the_census_fails_when_it_is_wrong():
    """the self-check is live: a census that links two runs one base too far apart does not reproduce the oracle's peaks"""
    a, par, o, so, cen = S.reference("tight:cand-cut")
    S.sweep_census(o, a["case"], "tight", par)
    with pytest.raises(AssertionError, match="the census is wrong"):
        S.sweep_census(o, a["case"], "tight", T.params(par, max_gap=S.LINK_GAP + 1, min_auc=0.0, min_len=0))


@pytest.mark.parametrize("name,k", S.AUC_CASES)
def test_auc_order_candidates_are_live(name, k):
    """the candidate's float32 terms give another float summed in reverse or pairwise than in interval order, the in-order sum is
    the oracle's AUC, and min_auc = that sum keeps the peak while the next float up drops it"""
    a, par, o, so, cen = S.reference(name)
    t = cen.terms[k]
    seq = S.seq_sum(t)
    assert len(t) > 16 and seq.tobytes() == o.get_peaks()["auc"][k].tobytes()
    assert S.seq_sum(t[::-1]) != seq and S.pair_sum(t) != seq, (seq, S.seq_sum(t[::-1]), S.pair_sum(t))
    assert float(np.sum(t.astype(np.float64))) != float(seq)
    keys = {}
    for v in (T.down(seq), float(seq), T.up(seq)):
        _, _, o2, _, _ = S.reference(name, min_auc=v)
        keys[v] = [tuple(r) for r in o2.get_peaks()[["chrom", "start", "end"]].tolist()]
    c = cen.cands[k]
    me = (int(cen.chrom[c[2]]), int(cen.start[c[2]]), int(cen.end[c[3]]))
    assert me in keys[float(seq)] and me in keys[T.down(seq)] and me not in keys[T.up(seq)]


def test_the_walk_lengths_cover_every_step_and_batch_border():
    want = {1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1279, 1280, 1281}
    for sp in ("tight", "loose"):
        got = set()
        for g in S.WALK_GROUPS:
            cen = S.check(f"{sp}:walk-{g}")
            got |= {S.cand_len(cen, k) for k in range(len(cen.cands))}
        assert want <= got
    # 16 intervals a step and 4 steps a batch of the short walk, 64 and 256 of the long one and of k_q_fill_cands; PK_SHORT between them
    assert S.PK_SHORT == 1024 and {16, 64, 256, S.PK_SHORT, S.PK_SHORT + 256} <= want


def test_compaction_parameters_are_ties():
    """min_len = 12 sits exactly on the long candidates' length (kept: >=)"""
    a, par, o, so, cen = S.reference("tight:compact")
    ln = sorted({int(cen.end[c[3]] - cen.start[c[2]]) for c in cen.cands})
    assert ln == [3, 12] and par.min_len == 12
    assert o.n_peaks == 2 + 88 and S.reference("tight:zero-peaks")[2].n_peaks == 0 and len(S.reference("tight:zero-peaks")[4].runs) == 256
