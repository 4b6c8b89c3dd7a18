"""The sequence itself on the GPU and the motif scan (gx_set_genome_bases / gx_get_sequence / gx_set_motifs / gx_motif_scan_*)
against tests/motifs_ref.py, at the smallest shapes where the kernels can go wrong: chromosomes around the word (64) and the
directory block (512), regions that start and end around the word and the chromosome's end, motifs of width 1, 2, 31 and 32,
one motif, one LDS batch and one more, every step, a list that runs full.  Every comparison is == on integers."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import backends as B
import gcbias_ref as GR
import golden_cases as G
import motifs_ref as R
from genrich_amd import synth
from genrich_amd.lib import (GX_PATH_GC, GX_PATH_MOTIFS, MOTIF_HIT_DTYPE, REGION_DTYPE, format_motif_hits, format_motif_summary, motif_geometry,
                             motif_hits_text, motif_scan_genome_group, motif_summary_text, pack_motifs)
from ranks import ThreadAllreduce
from test_hip_counts import _cli_inputs
from test_hip_gcbias import LENS, _cli_genome, _cli_peaks, _events, _push_whole, _seqs, _whole, _write_fasta
from test_host_cli import _binary

pytestmark = pytest.mark.gpu

ORDER = -10
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motifs_small.jaspar")
LANES, GRID, POSITIONS, STEP, BATCH, LIST_MIN, FLUSH = motif_geometry()


def _ctx(lens=LENS, skip=None, owned=None, bases=True):
    import genrich_amd
    h = genrich_amd.Genrich(B.make_params(pq=0.01, min_auc=20.0))
    h.set_chroms(lens, skip)
    if owned is not None:
        h.set_owned(owned)
    h.set_genome(True)
    if bases:
        h.set_genome_bases(True)
    return h


def _regions(rows):
    return np.asarray(rows, dtype=np.uint32).reshape(-1, 3).view(REGION_DTYPE).reshape(-1)


def _random_scores(rng, L):
    return rng.integers(-900, 400, (L, 4)).tolist()


P_OF = {1: 0.25, 2: 0.0625, 3: 0.004}                                  # the p-value of a motif of 1, 2 and more columns


def _motifs(seed=17):
    """Widths 1, 2, 31, 32, a palindrome of 6, and 12 and 7 between them; thresholds that let a few windows in a thousand hit."""
    rng = np.random.default_rng(seed)
    half = _random_scores(rng, 3)
    pal = half + [row[::-1] for row in half[::-1]]              # s[j][b] = s[L - 1 - j][comp(b)]: both strands score alike
    tabs = [_random_scores(rng, L) for L in (1, 2, 31, 32)] + [pal, _random_scores(rng, 12), _random_scores(rng, 7)]
    out = []
    for s in tabs:
        t = R.threshold(s, P_OF[min(len(s), 3)])[0]
        out.append((s, t))
    return out


@pytest.fixture(scope="module")
def genome():
    seqs = _seqs(3)
    return seqs, R.genome(seqs, LENS)


@pytest.fixture(scope="module")
def motifs():
    return _motifs()


@pytest.fixture(scope="module")
def loaded(genome, motifs):
    h = _ctx()
    _push_whole(h, genome[0])
    h.set_motifs(motifs)
    yield h
    h.close()


def _border_regions():
    rows = []
    for c, n in enumerate(LENS):
        pts = sorted({0, 1, 63, 64, 65, max(n - 65, 0), max(n - 64, 0), max(n - 1, 0), n, n + 7})
        rows += [(c, s, e) for s in pts for e in pts if s <= e <= s + 600]      # (empty ones among them)
    for L in (1, 2, 6, 31, 32):                                        # shorter than, equal to and one longer than a motif
        rows += [(9, 700, 700 + L - 1), (9, 700, 700 + L), (9, 700, 700 + L + 1), (10, 200_003 - L, 200_003), (10, 200_003 - L + 1, 200_010)]
    rows += [(9, 900, 100), (10, 5, 2)]                                # inverted
    rows += [(10, 1000, 3000), (10, 2000, 4000), (10, 1000, 3000), (10, 1000, 3000)]   # overlapping and repeated
    rows += [(11, 0, 500), (1 << 31, 0, 500)]                          # outside the table
    return rows


def _same(got, want):
    hits, cnt = got
    assert R.count_lists(cnt) == want[1]
    assert R.hit_tuples(hits) == want[0]


# ---- the sequence -----------------------------------------------------------------------------------------------------------

def test_sequence_round_trip_in_one_push_and_in_shuffled_pieces(genome):
    seqs, gen = genome
    rng = np.random.default_rng(5)
    for split in (False, True):
        h = _ctx()
        assert h.get_sequence(10, 0, 70) == b"N" * 70                 # nothing pushed: every base unknown
        pieces = []
        for c, s in enumerate(seqs):
            cuts = [0, len(s)]
            if split and len(s) > 64:
                cuts = sorted(set(cuts + [64 * int(x) for x in rng.integers(1, (len(s) + 63) // 64, 6)]))
            pieces += [(c, a, s[a:b]) for a, b in zip(cuts, cuts[1:])]
        for i in rng.permutation(len(pieces)) if split else range(len(pieces)):
            h.push_sequence(*pieces[i])
        for c, n in enumerate(LENS):
            assert h.get_sequence(c, 0, n + 9) == R.letters(gen[c], 0, n + 9), c
        for start, n in ((1, 1), (63, 3), (64, 64), (199_999, 10), (200_003, 5), (300_000, 4), (5, 0)):
            assert h.get_sequence(10, start, n) == R.letters(gen[10], start, n), (start, n)
        assert set(R.letters(gen[10], 0, LENS[10])) == set(b"ACGTN") and h.path_info() & GX_PATH_GC
        h.close()


def test_the_third_vector_is_off_unless_asked_and_changes_no_gc_figure(genome):
    seqs, gen = genome
    ev = _events(20_000, 7)
    res = []
    for bases in (False, True):
        h = _ctx(bases=bases)
        _push_whole(h, seqs)
        g, a = h.gc_content(_whole(LENS))
        res.append((h.genome_info(), g.tolist(), a.tolist(), h.gc_bias_events(ev, 200)))
        lib, ctx = h.lib, h.ctx
        if not bases:
            out = C.create_string_buffer(8)
            assert lib.gx_get_sequence(ctx, 0, 0, 1, out) == ORDER and "gx_set_genome_bases" in lib.gx_last_error(ctx).decode()
            assert lib.gx_motif_scan_regions(ctx, None, 0, 0, 0, 0, 0, None, 0, None, None, None, None) == ORDER
            assert "gx_set_genome_bases" in lib.gx_last_error(ctx).decode()
            assert lib.gx_set_genome_bases(ctx, 1) == ORDER and "before the first base" in lib.gx_last_error(ctx).decode()   # after a push
        h.close()
    assert res[0][:3] == res[1][:3] and GR.same(res[0][3], res[1][3]) and res[0][0][0] == sum(LENS)
    h = _ctx(bases=False)
    h.set_genome(False)
    assert h.lib.gx_set_genome_bases(h.ctx, 1) == ORDER and "gx_set_genome(ctx, 1)" in h.lib.gx_last_error(h.ctx).decode()
    h.close()


def test_a_new_table_lays_the_third_vector_out_again_empty(genome):
    seqs, gen = genome
    h = _ctx(owned=[1] * 10 + [0])
    _push_whole(h, seqs)
    assert h.get_sequence(9, 0, 5000) == R.letters(gen[9], 0, 5000) and h.get_sequence(10, 0, 100) == b"N" * 100   # 10 is not owned
    h.set_owned([1] * 11)
    assert h.get_sequence(9, 0, 5000) == b"N" * 5000                   # laid out again, empty
    _push_whole(h, seqs)
    h.reset()                                                          # gx_reset keeps it
    assert h.get_sequence(10, 100_000, 3000) == R.letters(gen[10], 100_000, 3000)
    h.close()


# ---- regions against the reference --------------------------------------------------------------------------------------

def test_regions_at_every_border(genome, motifs, loaded):
    rows = _border_regions()
    want = R.scan(genome[1], rows, motifs)
    assert len(want[0]) > 100 and all(w > 0 for w in want[1][0]) and {h[4] for h in want[0]} == {0, 1}
    pal = [h for h in want[0] if h[3] == 4]
    assert pal and all((r, p, s, 4, 1 - st) in set(want[0]) for r, p, s, m, st in pal)     # a palindrome reports both strands
    _same(loaded.motif_scan_regions(_regions(rows)), want)
    assert loaded.path_info() & GX_PATH_MOTIFS
    _same(loaded.motif_scan_regions(_regions([])), ([], [[0] * len(motifs)] * 3))


def test_random_regions_in_every_geometry(genome, motifs, loaded):
    rng = np.random.default_rng(11)
    c = rng.integers(0, len(LENS), 400)
    ln = np.asarray(LENS)[c]
    a = rng.integers(0, 1 << 30, 400) % (ln + 9)
    b = np.minimum(a + rng.integers(0, 200, 400), ln + 9)
    rows = list(zip(c.tolist(), a.tolist(), b.tolist())) + [(10, 100_000, 110_000)]
    want = R.scan(genome[1], rows, motifs)
    assert 1000 < len(want[0]) < LIST_MIN                              # (the first list holds them: no rerun unless forced)
    reg = _regions(rows)
    for kw in [{}, {"grid": 1}, {"grid": 3}, {"batch_motifs": 2}, {"batch_motifs": 3}, {"batch_motifs": 7}, {"grid": 3, "batch_motifs": 1, "list_cap": 5}] + \
              [{"step_words": s} for s in range(1, 17)]:
        _same(loaded.motif_scan_regions(reg, **kw), want)
        reruns, batches = loaded.motif_last()
        assert batches == -(-len(motifs) // min(kw.get("batch_motifs", BATCH), len(motifs))), kw
        assert reruns == (1 if kw.get("list_cap") else 0), kw


def test_skipped_not_owned_and_unpushed_chromosomes_scan_nothing(genome, motifs):
    seqs, gen = genome
    skip, owned = [0] * 9 + [1, 0], [1] * 8 + [0, 1, 1]
    active = [int(o and not s) for s, o in zip(skip, owned)]
    seqs, gen = list(seqs), list(gen)
    seqs[7], gen[7] = None, R.codes(None, LENS[7])                     # a chromosome without sequence: nothing is known
    h = _ctx(skip=skip, owned=owned)
    _push_whole(h, seqs)
    h.set_motifs(motifs)
    rows = [(c, 0, n) for c, n in enumerate(LENS)] + [(9, 100, 900), (8, 0, 513), (7, 0, 512)]
    want = R.scan(gen, rows, motifs, active)
    assert {r for r, *_ in want[0]} <= {0, 1, 2, 3, 4, 5, 6, 10}
    _same(h.motif_scan_regions(_regions(rows)), want)
    _same((np.zeros(0, dtype=MOTIF_HIT_DTYPE), h.motif_scan_genome()), ([], R.scan_genome(gen, motifs, active)))
    h.close()


def test_one_unknown_base_at_the_first_the_last_and_a_middle_column(motifs):
    lens = [700, 130]
    rng = np.random.default_rng(13)
    clean = [bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)]) for n in lens]
    low = [(s, R.score_range(s)[0]) for s, t in motifs]                # at smin every scanned window hits on both strands
    h = _ctx(lens)
    h.set_motifs(low)
    for pos in (0, 63, 64, 300, lens[0] - 1):
        s = bytearray(clean[0])
        s[pos] = ord("N")
        gen = R.genome([bytes(s), clean[1]], lens)
        _push_whole(h, [bytes(s), clean[1]])
        rows = [(0, 0, lens[0]), (0, max(pos - 31, 0), pos + 32), (0, pos, pos + 40), (0, max(pos - 40, 0), pos + 1), (1, 0, 130)]
        want = R.scan(gen, rows, low)
        for m, (sc, t) in enumerate(low):                              # exactly the windows that cover it are lost
            L = len(sc)
            assert want[1][0][m] >= lens[0] - L + 1 - len(range(max(0, pos - L + 1), min(pos, lens[0] - L) + 1))
            assert want[1][1][m] == want[1][2][m] == want[1][0][m]
        _same(h.motif_scan_regions(_regions(rows)), want)
    h.close()


# ---- thresholds and the list ------------------------------------------------------------------------------------------------

def test_thresholds_at_smin_smax_and_beyond(genome, motifs):
    seqs, gen = genome
    h = _ctx()
    _push_whole(h, seqs)
    rows = [(10, 0, 20_000), (9, 0, 5000), (5, 0, 128), (0, 0, 1)]
    reg = _regions(rows)
    lo = [(s, R.score_range(s)[0]) for s, t in motifs]
    h.set_motifs(lo)
    want = R.scan(gen, rows, lo)
    assert len(want[0]) == 2 * sum(want[1][0]) > 300_000               # every scanned window, both strands
    for cap in (1, 1000):                                              # the list runs full: counted, then run once more
        _same(h.motif_scan_regions(reg, list_cap=cap), want)
        assert h.motif_last()[0] == 1
    _same(h.motif_scan_regions(reg, list_cap=len(want[0])), want)       # exactly enough
    assert h.motif_last()[0] == 0
    hi = [(s, R.score_range(s)[1]) for s, t in motifs]
    h.set_motifs(hi)
    want = R.scan(gen, rows, hi)
    assert not [x for x in want[0] if x[3] in (2, 3, 5)]               # (no window of 12 or more columns is the best L-mer)
    _same(h.motif_scan_regions(reg), want)
    over = [(s, R.score_range(s)[1] + 1) for s, t in motifs]
    h.set_motifs(over)
    got = h.motif_scan_regions(reg)
    assert len(got[0]) == 0 and R.count_lists(got[1]) == [want[1][0], [0] * len(motifs), [0] * len(motifs)]
    h.set_motifs(motifs[:1])                                           # one motif
    _same(h.motif_scan_regions(reg), R.scan(gen, rows, motifs[:1]))
    h.set_motifs([])                                                   # none: legal, nothing scanned
    got = h.motif_scan_regions(reg)
    assert len(got[0]) == 0 and got[1].shape == (3, 0)
    h.close()


def test_what_is_refused(genome, motifs, loaded):
    lib, ctx = loaded.lib, loaded.ctx
    err = lambda: lib.gx_last_error(ctx).decode()
    reg = _regions([(10, 0, 1000)])
    for args, msg in (((65_536, 0, 0, 0), "65535 workgroups"), ((0, 17, 0, 0), "1 to 16 words"), ((0, 0, 65, 0), "1 to 64 motifs"),
                      ((0, 0, 0, 1 << 31), "2^31 entries")):
        assert lib.gx_motif_scan_regions(ctx, reg.ctypes.data, 1, *args, None, 0, None, None, None, None) == ORDER and msg in err(), args
    n = C.c_size_t(0)
    assert lib.gx_motif_scan_peaks(ctx, C.byref(n)) == ORDER and "after gx_find_peaks" in err()
    assert lib.gx_get_motif_hits(ctx, None, 0) == ORDER
    h = _ctx()
    for width, msg in ((0, "1 <= L <= 32"), (33, "1 <= L <= 32")):
        rec, flat = pack_motifs([(np.zeros((1, 4), dtype=np.int16), 0)])
        rec["width"] = width
        big = np.zeros(4 * 40, dtype=np.int16)
        assert h.lib.gx_set_motifs(h.ctx, rec.ctypes.data, 1, big.ctypes.data) == ORDER and msg in h.lib.gx_last_error(h.ctx).decode()
    rec, flat = pack_motifs([(np.zeros((1, 4), dtype=np.int16), 0)] * 4097)
    assert h.lib.gx_set_motifs(h.ctx, rec.ctypes.data, 4097, flat.ctypes.data) == ORDER and "4096" in h.lib.gx_last_error(h.ctx).decode()
    h.set_motifs([(np.zeros((1, 4), dtype=np.int16), 0)] * 4096)       # the most a context takes
    h.close()


def test_many_motifs_go_through_lds_in_batches(genome):
    seqs, gen = genome
    rng = np.random.default_rng(23)
    many = []
    for k in range(130):                                               # two full batches of 64 and two more motifs
        s = _random_scores(rng, int(rng.integers(1, 33)))
        many.append((s, R.threshold(s, 0.01 if len(s) > 3 else 0.25)[0]))
    h = _ctx()
    _push_whole(h, seqs)
    h.set_motifs(many)
    rows = [(9, 0, 5000), (10, 150_000, 152_000)]
    _same(h.motif_scan_regions(_regions(rows)), R.scan(gen, rows, many))
    assert h.motif_last() == (0, 3)
    h.close()


# ---- the genome and the peaks -----------------------------------------------------------------------------------------------

def test_the_genome_pass_and_two_contexts_that_add_up(genome, motifs, loaded):
    seqs, gen = genome
    want = R.scan_genome(gen, motifs)
    assert R.count_lists(loaded.motif_scan_genome()) == want and sum(want[1]) > 1000
    hs = []
    for owned in ([1, 0] * 5 + [0], [0, 1] * 5 + [1]):
        h = _ctx(owned=owned)
        _push_whole(h, seqs)
        h.set_motifs(motifs)
        assert R.count_lists(h.motif_scan_genome()) == R.scan_genome(gen, motifs, owned)
        hs.append(h)
    assert R.count_lists(motif_scan_genome_group(hs)) == want
    assert R.add_counts(R.scan_genome(gen, motifs, [1, 0] * 5 + [0]), R.scan_genome(gen, motifs, [0, 1] * 5 + [1])) == want
    for h in hs:
        h.close()


RUN_LENS = [3_000_000, 2_000_000, 1_000_000]


def _run(seqs, motifs, ev, owned=None, coll=None):
    h = _ctx(RUN_LENS, owned=owned)
    if coll:
        h.set_collectives(*coll)
    _push_whole(h, seqs)
    h.set_motifs(motifs)
    h.sample_begin(0, None)
    h.push_events(ev)
    h.sample_end()
    h.sample_no_control()
    h.pvalues()
    h.find_peaks()
    return h


def test_the_peaks_of_a_run_and_the_two_tables(motifs):
    seqs = _seqs(29, RUN_LENS)
    gen = R.genome(seqs, RUN_LENS)
    ev = synth.make_fragments(RUN_LENS, 250_000, 40, peak_every=20_000, tower_every=3_000_000)
    h = _run(seqs, motifs, ev)
    assert h.n_peaks > 20 and not h.path_info() & GX_PATH_MOTIFS         # nothing of it before the first call
    pk = h.get_peaks()
    rows = list(zip(pk["chrom"].tolist(), pk["start"].tolist(), pk["end"].tolist()))
    want = R.scan(gen, rows, motifs)
    assert h.motif_scan_peaks() == len(want[0]) > 50
    assert R.hit_tuples(h.get_motif_hits()) == want[0] and R.count_lists(h.get_motif_counts()) == want[1]
    assert h.path_info() & GX_PATH_MOTIFS
    _same(h.motif_scan_regions(_regions(rows)), want)
    # the tables
    ids = ["M%d" % k for k in range(len(motifs))]
    names = ["name %d" % k for k in range(len(motifs))]
    chroms = ["chr%d" % (k + 1) for k in range(len(RUN_LENS))]
    pthr = [R.p_achieved(R.threshold(s, P_OF[min(len(s), 3)])[3], len(s)) for s, t in motifs]
    pthr[1] = float("nan")
    cg = R.scan_genome(gen, motifs)
    hits_want = R.hits_text(chroms, rows, pk["summit"].tolist(), motifs, ids, names, pthr, want[0])
    sum_want = R.summary_text(rows, motifs, ids, names, pthr, want[0], want[1], cg)
    assert format_motif_hits(chroms, _regions(rows), pk["summit"], motifs, ids, names, pthr, h.get_motif_hits()).decode() == hits_want
    assert format_motif_summary(_regions(rows), motifs, ids, names, pthr, h.get_motif_hits(), h.get_motif_counts(), h.motif_scan_genome()).decode() == sum_want
    assert motif_hits_text([h], chroms, motifs, ids, names, pthr).decode() == hits_want
    assert motif_summary_text([h], motifs, ids, names, pthr).decode() == sum_want
    assert "\tNA\t" in sum_want and sum_want.count("\n") == len(motifs) + 1
    # two contexts with the chromosomes between them: the same tables
    owns, coll = [[1, 0, 1], [0, 1, 0]], ThreadAllreduce(2)
    hs, errors = [None, None], []

    def rank(r):
        try:
            hs[r] = _run(seqs, motifs, ev, owned=owns[r], coll=(r, 2, coll.callback(r)))
        except BaseException as e:
            errors.append(e)
            coll.bar.abort()

    threads = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert 0 < hs[0].n_peaks < h.n_peaks and hs[0].n_peaks + hs[1].n_peaks == h.n_peaks
    assert motif_hits_text(hs, chroms, motifs, ids, names, pthr).decode() == hits_want
    assert motif_summary_text(hs, motifs, ids, names, pthr).decode() == sum_want
    h.reset()                                                          # the results go with the run
    assert h.lib.gx_get_motif_hits(h.ctx, None, 0) == ORDER and not h.path_info() & GX_PATH_MOTIFS
    for x in hs + [h]:
        x.close()


# ---- the command line ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ctrl_q", "bedx"])
def test_cli_motif_hits_and_summary_of_a_golden_fixture_on_one_and_two_contexts(name):
    case, names, seqs = _cli_genome(name)
    gen = R.genome(seqs, case["lens"])
    meta, args, tmp, _ = _cli_inputs(name)
    fa, out = os.path.join(tmp, "motif_genome.fa"), os.path.join(tmp, "motif_out")
    _write_fasta(fa, names, seqs)
    P = 0.01
    motifs, ids, mnames, pthr = [], [], [], []
    for mid, mname, counts in R.read_jaspar(open(GOLDEN, "rb").read()):
        s = R.pssm(counts, 1.0)
        t, smin, smax, n_ge, un = R.threshold(s, P)
        motifs.append((s, t))
        ids.append(mid)
        mnames.append(mname)
        pthr.append(float("nan") if un else R.p_achieved(n_ge, len(s)))
    assert any(p != p for p in pthr) and sum(p == p for p in pthr) >= 4         # (a motif that cannot hit stays in the run, with NA)
    rows = [l.split("\t") for l in G.read_gz(name, "out.narrowPeak").decode().splitlines()]
    peaks = [(names.index(r[0]), int(r[1]), int(r[2])) for r in rows]
    summit = [int(r[9]) for r in rows]
    active = [int(not k) for k in case["skip"]]
    took = [int(a and bool(v)) for a, v in zip(active, case["replicates"][-1]["save"])]
    hits, cp = R.scan(gen, peaks, motifs, active)
    cg = R.scan_genome(gen, motifs, took)
    assert len(hits) > 20 and sum(cg[1]) > len(hits)
    want_hits = R.hits_text(names, peaks, summit, motifs, ids, mnames, pthr, hits)
    want_sum = R.summary_text(peaks, motifs, ids, mnames, pthr, hits, cp, cg)
    for extra in ([], ["--devices", "0,0"]):
        res = subprocess.run([_binary(), "-v", "-o", out + ".narrowPeak", "--genome", fa, "--motifs", GOLDEN, "--motif-pvalue", str(P), "--motif-hits", out + ".hits",
                              "--motif-summary", out + ".summary", "--gc-peaks", out + ".gcpeaks"] + extra + args, capture_output=True, text=True)
        assert res.returncode == 0, (extra, res.stderr)
        assert open(out + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")
        assert open(out + ".hits").read() == want_hits, extra
        assert open(out + ".summary").read() == want_sum, extra
        assert open(out + ".gcpeaks").read() == _cli_peaks(name, names, GR.genome(seqs, case["lens"]))
        err = res.stderr.splitlines()
        assert any(l.startswith("Motifs " + GOLDEN + ": 6 matrices") for l in err) and sum(l.startswith("Warning! motif ") for l in err) == sum(p != p for p in pthr)
        assert any(l.startswith("Motif hits: %d in %d peaks" % (len(hits), len({h[0] for h in hits}))) for l in err), res.stderr
        assert any(l.startswith("  Motif summary: ") for l in err)
        for f in (".hits", ".summary"):
            os.remove(out + f)
    res = subprocess.run([_binary(), "-o", out + ".np2", "--genome", fa, "--gc-peaks", out + ".gcpeaks2"] + args, capture_output=True, text=True)
    assert res.returncode == 0 and open(out + ".np2", "rb").read() == G.read_gz(name, "out.narrowPeak")        # a run without motifs, as before
