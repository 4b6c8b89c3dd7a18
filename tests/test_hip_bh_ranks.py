"""Benjamini-Hochberg across ranks at its limits: the dense "bp at V" all-reduce with its side regions (k_bh_dense_fill /
k_bh_from_dense) and the range-partitioned exchange (gx_bhx.h, bh_range_exchange) with 2 .. 8 ranks in threads of this
process (tests/ranks.py) on inputs of a few dozen fragments: ranks with fewer distinct p-values than the 32 samples, with
one, with none; splitters that tie and owners that receive nothing; every rank holding the same values; ranks that own no
chromosome; side regions that fit and that overflow.  Every case first shows FROM THE ORACLE'S OUTPUT that its input has
the property it is about, then compares bits with the single-process oracle: every owned interval's end, p and q, the
scalars on every rank, the merged peaks -- and asserts which exchange ran (gx_path_info: 32 dense, 64 range)."""
import numpy as np
import pytest

import backends as B
import ranks as R
from genrich_amd import synth
from genrich_amd.dist import lpt_partition

pytestmark = pytest.mark.gpu

DENSE, RANGE = 32, 64
SAMPLES = 32              # BHX_SAMPLES (gx_bhx.h)
SIDE = 4096               # BHD_SIDE (gx_stats.h): values outside the table p(V) per rank
DEEP = 2185               # the first pileup outside the table: 2^18 / 120 = 2,184.5
QT_CHUNK = 2048           # entries per workgroup of k_qt_sums / k_qt_raw / k_qt_apply


# ---- inputs -------------------------------------------------------------------------------------------------------------

def _events(rows):
    ev = np.zeros(len(rows), dtype=B.EVENT_DTYPE)
    if rows:
        ev["chrom"], ev["start"], ev["end"] = np.asarray(rows, dtype=np.int64).T
    ev["count"] = 1
    return ev


def _tiny(n_chrom, seed, n_treat=6, n_ctrl=4, pile=(12, 6), empty=()):
    """Chromosomes of 60,000 .. 25,000 bp; on each a handful of background fragments of 100 .. 300 bp (6 treatment, 4 control)
    and a pile of 12 + 6 c treatment fragments within +-60 bp of its middle; none on the chromosomes of `empty`."""
    rng = np.random.default_rng(seed)
    lens = [int(x) // 1000 * 1000 for x in np.linspace(60_000, 25_000, n_chrom)] if n_chrom > 1 else [60_000]
    tr, ct = [], []
    for c, L in enumerate(lens):
        if c in empty:
            continue
        for rows, n in ((tr, n_treat), (ct, n_ctrl)):
            for _ in range(n):
                ln = int(rng.integers(100, 301))
                s = int(rng.integers(0, L - ln))
                rows.append((c, s, s + ln))
        for _ in range(pile[0] + pile[1] * c):
            ln = int(rng.integers(100, 301))
            s = L // 2 + int(rng.integers(-60, 61)) - ln // 2
            tr.append((c, s, s + ln))
    return lens, _events(tr), _events(ct)


def _staircase(chrom, first, n, end):
    """n fragments [first + i, end): pileups 1 .. n, each on one base pair, then n on the rest"""
    return _events([(chrom, first + i, end) for i in range(n)])


Q = dict(pq=0.05, qval=True, min_auc=1.0)


def _case(name):
    """-> dict(params, lens, reps, skip, beds, knobs, env)"""
    d = dict(params=B.make_params(**Q), skip=None, beds=None, knobs=None, env=None)
    if name == "tiny_ctrl":
        lens, tr, ct = _tiny(8, 1)
        d.update(lens=lens, reps=[(tr, ct)])
    elif name == "identical":
        _, tr, ct = _tiny(1, 2, n_treat=9, n_ctrl=3, pile=(18, 0))
        tr["start"] -= 5_000                                      # (the one chromosome of _tiny has 60,000 bp: its middle to 25,000)
        tr["end"] -= 5_000
        ct["start"] = np.minimum(ct["start"], 49_000)
        ct["end"] = ct["start"] + 300
        tr["start"], tr["end"] = np.clip(tr["start"], 0, 49_700), np.clip(tr["end"], 1, 50_000)
        n = 6

        def everywhere(ev):
            out = np.tile(ev, n)
            out["chrom"] = np.repeat(np.arange(n), len(ev))
            return out
        d.update(lens=[50_000] * n, reps=[(everywhere(tr), everywhere(ct))])
    elif name == "one_value":
        whole = _events([(c, 0, 3_000) for c in range(4)])
        d.update(lens=[3_000] * 4, reps=[(whole, whole.copy())])
    elif name == "empty_chrom":
        _, tr, ct = _tiny(3, 3, empty=(2,))
        d.update(lens=[60_000, 50_000, 40_000], reps=[(tr, ct)])
    elif name == "tiny_noctrl":
        lens, tr, _ = _tiny(8, 1)
        d.update(lens=lens, reps=[(tr, None)])
    elif name == "two_chroms_noctrl":
        lens, tr, _ = _tiny(8, 1)
        d.update(lens=lens[:2], reps=[(tr[tr["chrom"] < 2], None)])
    elif name == "excluded":
        lens, tr, _ = _tiny(8, 1)
        beds = [[0, 2_000, L // 2 + 100, L // 2 + 150] if c % 2 == 0 else [] for c, L in enumerate(lens)]
        d.update(lens=lens, reps=[(tr, None)], beds=beds)
    elif name == "no_dense":
        d = _case("tiny_noctrl")
        d["env"] = {"GX_NO_DENSE_BH": "1"}
    elif name in ("side", "side_overflow"):
        lens = [60_000, 40_000, 30_000]
        bg = synth.make_fragments(lens, 600, 4, peak_every=10_000, tower_every=10**9)
        n0 = 3_000 if name == "side" else 7_000
        tr = np.concatenate([bg, _staircase(0, 20_000, n0, 32_000), _staircase(1, 10_000, 2_600, 22_000)])
        d.update(lens=lens, reps=[(tr, None)])
    elif name == "fisher":
        reps = []
        for sd in (1, 5, 9):
            lens, tr, _ = _tiny(8, sd)
            reps.append((tr, None))
        d.update(lens=lens, reps=reps)
    else:
        raise KeyError(name)
    return d


_ORACLE = {}


@pytest.fixture(scope="module", autouse=True)
def _contexts_closed_at_the_end():
    yield
    R.close_pool()


def _oracle(name):
    """the case and its single-process result: computed once, shared by the worlds, left unchanged"""
    if name not in _ORACLE:
        d = _case(name)
        _ORACLE[name] = (d, R.run_oracle(d["params"], d["lens"], d["reps"], d["skip"], d["beds"]))
    return _ORACLE[name]


# ---- what the oracle's output says about an input -------------------------------------------------------------------------

def _bits(ora, chroms, col=1, deep_only=False):
    """the distinct p (col 1) or q (col 2) bits of the intervals of `chroms` that are not skipped (p = -1, -E)"""
    parts = []
    for c in chroms:
        p = ora.iv[c][1]
        keep = p != -1.0
        if deep_only:
            keep &= ora.expt[c] >= DEEP
        parts.append(ora.iv[c][col][keep].view(np.uint32))
    return np.unique(np.concatenate(parts)) if parts else np.zeros(0, dtype=np.uint32)


def _per_rank(ora, lens, world, owner=None, **kw):
    """[the distinct p bits rank r's table holds] for the partition run_ranks uses"""
    owner = lpt_partition(lens, world) if owner is None else owner
    return [_bits(ora, [c for c in range(len(lens)) if owner[c] == r], **kw) for r in range(world)]


def _ranges(per):
    """How many distinct values of the run each owner's range holds, by the library's own rule (k_bhx_samples, k_bhx_splitters,
    k_bhx_offsets): rank r's samples are its sorted values at (j + 1) D / 33 (0xFFFFFFFF when it has none), splitter k is the
    32 k-th of all samples in order, range o is [splitter o, splitter o + 1) and the last range takes the rest."""
    samples = []
    for keys in per:
        D = len(keys)
        samples += [int(keys[(j + 1) * D // (SAMPLES + 1)]) if D else 0xFFFFFFFF for j in range(SAMPLES)]
    samples.sort()
    values = np.unique(np.concatenate(per))
    cut = [0] + [int(np.searchsorted(values, samples[k * SAMPLES], side="left")) for k in range(1, len(per))] + [len(values)]
    return [cut[o + 1] - cut[o] for o in range(len(per))]


def _all(ora, col=1):
    return _bits(ora, sorted(ora.iv), col)


def _check(name, world, exchange):
    """The case on `world` ranks: the exchange that ran, on every rank, and everything against the oracle -> the ranks' results"""
    d, ora = _oracle(name)
    res = R.run_ranks(d["params"], d["lens"], d["reps"], world, skip=d["skip"], beds=d["beds"], knobs=d["knobs"], env=d["env"])
    for r in res:
        assert r.flags & (DENSE | RANGE) == exchange, (r.rank, r.flags & (DENSE | RANGE), exchange)
    R.assert_equals_oracle(res, ora, d["lens"])
    return res


# ---- the range-partitioned exchange ----------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 3, 5, 8])
def test_tiny_genome_with_a_control(world):
    """Ranks whose 32 samples repeat: fewer distinct values than samples."""
    d, ora = _oracle("tiny_ctrl")
    per = [len(x) for x in _per_rank(ora, d["lens"], world)]
    assert min(per) >= 2
    if world >= 5:
        assert min(per) < SAMPLES, per
    assert len(_all(ora, 2)) >= 5                                                # q is no constant
    assert set(ora.peaks["chrom"].tolist()) == set(range(len(d["lens"])))        # a peak on every chromosome
    _check("tiny_ctrl", world, RANGE)


@pytest.mark.parametrize("world", [2, 3, 6])
def test_every_rank_holds_the_same_values(world):
    """The owner's k_bh_insert merges `world` copies of every value."""
    d, ora = _oracle("identical")
    per = _per_rank(ora, d["lens"], world)
    assert all(np.array_equal(p, per[0]) for p in per) and len(per[0]) >= 10, [len(p) for p in per]
    assert len(_all(ora, 2)) >= 5
    assert set(ora.peaks["chrom"].tolist()) == set(range(len(d["lens"])))
    _check("identical", world, RANGE)


@pytest.mark.parametrize("world", [2, 4])
def test_one_value_per_rank(world):
    """One distinct p in the whole run: all samples are equal, all splitters tie, one owner receives everything and the
    others nothing (R = 0: a one-element sort of 0xFFFFFFFF, *Dptr = 0 in k_qt_sums / k_qt_raw / k_qt_apply, FLT_MAX as the
    range's minimum)."""
    d, ora = _oracle("one_value")
    assert len(_all(ora)) == 1
    per = _per_rank(ora, d["lens"], world)
    assert all(len(p) == 1 for p in per)
    assert _ranges(per) == [0] * (world - 1) + [1]
    _check("one_value", world, RANGE)


@pytest.mark.parametrize("world", [2, 3, 4])
def test_an_empty_chromosome_and_an_idle_rank(world):
    """No read on the third chromosome in either sample: at 3 ranks its owner's table holds one value; at 4 ranks rank 3 owns
    nothing (layout_tiles' dormant tile space) and sends 32 samples of 0xFFFFFFFF."""
    d, ora = _oracle("empty_chrom")
    assert len(ora.iv[2][0]) == 1 and ora.iv[2][0][0] == d["lens"][2]
    per = [len(x) for x in _per_rank(ora, d["lens"], world)]
    owner = lpt_partition(d["lens"], world)
    if world == 3:
        assert owner == [0, 1, 2] and per[2] == 1, (owner, per)
    if world == 4:
        assert owner == [0, 1, 2] and per[3] == 0, (owner, per)
        # the idle rank's samples of 0xFFFFFFFF make the top splitter one too: the top range is empty and its FLT_MAX is the
        # minimum that every range below takes over
        assert _ranges(_per_rank(ora, d["lens"], world))[3] == 0
    if world >= 3:
        assert _ranges(_per_rank(ora, d["lens"], world))[0] == 0      # ... and so is the bottom one: splitters that tie
    assert len(_all(ora, 2)) >= 3 and len(ora.peaks) >= 2
    res = _check("empty_chrom", world, RANGE)
    if world == 4:
        assert not res[3].owned.any() and len(res[3].peaks) == 0 and res[3].n_iv == 0


@pytest.mark.parametrize("world", [3, 8])
def test_excluded_regions_without_a_control(world):
    """-E makes the run take the range exchange also without a control (bedGiven); a skipped interval keeps q = -1."""
    d, ora = _oracle("excluded")
    skipped = sum(int((ora.iv[c][1] == -1.0).sum()) for c in ora.iv)
    assert skipped >= 8, skipped
    for c in ora.iv:
        assert (ora.iv[c][2][ora.iv[c][1] == -1.0] == -1.0).all()
    assert min(len(x) for x in _per_rank(ora, d["lens"], world)) < SAMPLES
    assert len(_all(ora, 2)) >= 5 and len(ora.peaks) >= len(d["lens"])
    _check("excluded", world, RANGE)


@pytest.mark.parametrize("world", [3, 8])
def test_fisher_combined_replicates(world):
    d, ora = _oracle("fisher")
    singles = []
    for tr, _ in d["reps"]:
        one = R.run_oracle(d["params"], d["lens"], [(tr, None)])
        singles.append(len(_all(one)))
    assert len(_all(ora)) > max(singles), (len(_all(ora)), singles)
    assert len(_all(ora, 2)) >= 5 and len(ora.peaks) >= 1
    _check("fisher", world, RANGE)


# ---- the dense all-reduce ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,world", [("tiny_noctrl", 8), ("two_chroms_noctrl", 3)])
def test_idle_ranks_without_a_control(name, world):
    """Ranks with a handful of values; with 3 ranks on two chromosomes one owns nothing."""
    d, ora = _oracle(name)
    per = [len(x) for x in _per_rank(ora, d["lens"], world)]
    assert min(per) < SAMPLES, per
    if name == "two_chroms_noctrl":
        assert per[2] == 0 and lpt_partition(d["lens"], world) == [0, 1]
    assert len(_all(ora, 2)) >= 5 and len(ora.peaks) >= len(d["lens"])
    res = _check(name, world, DENSE)
    if name == "two_chroms_noctrl":
        assert not res[2].owned.any() and len(res[2].peaks) == 0 and res[2].n_iv == 0


@pytest.mark.parametrize("world", [3, 8])
def test_no_dense_bh_gives_the_dense_runs_bits(world):
    """GX_NO_DENSE_BH: the same input through the range exchange, and NOT the dense one; the same q bits as the dense run."""
    d, ora = _oracle("no_dense")
    assert d["env"] == {"GX_NO_DENSE_BH": "1"}
    res = _check("no_dense", world, RANGE)
    dense = _check("tiny_noctrl", world, DENSE)
    for a, b in zip(res, dense):
        assert sorted(a.iv) == sorted(b.iv)
        for c in a.iv:
            assert np.array_equal(a.iv[c][2].view(np.uint32), b.iv[c][2].view(np.uint32)), (a.rank, c)


@pytest.mark.parametrize("world", [2, 3])
def test_side_regions(world):
    """Pileups beyond the table p(V) on two ranks: their values travel in the ranks' side regions of the dense buffer."""
    d, ora = _oracle("side")
    deep = [len(x) for x in _per_rank(ora, d["lens"], world, deep_only=True)]
    assert sum(n > 0 for n in deep) == 2 and 0 < max(deep) < SIDE, deep
    _check("side", world, DENSE)


@pytest.mark.parametrize("world", [2, 3])
def test_side_region_overflow(world):
    """One rank holds more values outside the table than its region takes: every rank sees it after the all-reduce, all go back
    to their own tables and take the range exchange -- whose owners' ranges span more than one chunk of QT_CHUNK entries, so
    that chunkSum and totals (k_qt_raw), chunkMin and mins (k_qt_apply) all count."""
    d, ora = _oracle("side_overflow")
    deep = [len(x) for x in _per_rank(ora, d["lens"], world, deep_only=True)]
    assert max(deep) > SIDE, deep
    assert len(_all(ora)) > 2 * QT_CHUNK, len(_all(ora))
    assert max(_ranges(_per_rank(ora, d["lens"], world))) > QT_CHUNK
    _check("side_overflow", world, RANGE)


# ---- a rank whose records are lost --------------------------------------------------------------------------------------------

def test_a_rank_whose_records_are_lost_fails_every_rank():
    """Rank 1 takes part in every exchange but its segment of the all-to-all buffer (the big payload: n > 4096 words) arrives
    as zeros.  Every rank must come back with an error -- not with q-values, not by the barrier's timeout.  What fails the run
    is the length check on the ranges' totals (computeQval 377-382, k_qt_raw): the owners' sums lack rank 1's base pairs on
    every rank alike.  k_bhx_answer's own missing-key check cannot be reached this way: an owner builds its table from the
    very records it answers, so a record that arrives damaged is still found."""
    lens, tr, ct = _tiny(8, 1, n_treat=2000, n_ctrl=1500, pile=(200, 50))
    params = B.make_params(**Q)
    ora = R.run_oracle(params, lens, [(tr, ct)])
    per = [len(x) for x in _per_rank(ora, lens, 3)]
    assert 2 * sum(per) + 1 > 4096 and 3 * SAMPLES <= 4096 and sum(per) // 2 + 1 <= 4096, per   # the records, and nothing else
    seen = []

    def wrap(rank, cb):
        def lossy(buf, n, user):
            if rank == 1 and n > 4096:
                np.ctypeslib.as_array(buf, shape=(n,))[:] = 0
                seen.append(n)
            return cb(buf, n, user)
        return lossy if rank == 1 else cb

    with pytest.raises(RuntimeError) as e:
        R.run_ranks(params, lens, [(tr, ct)], 3, wrap=wrap, timeout=20, fresh=True)
    assert seen == [2 * sum(per) + 1]
    errors = R.run_ranks.last_errors
    assert [r for r, _ in errors] == [0, 1, 2]
    for r, err in errors:
        assert "error -8" in str(err) and "does not match p-value length" in str(err), (r, str(err))
    assert "does not match p-value length" in str(e.value)   # (no rank was sent home by a broken barrier: each failed by its own check)
