"""The k-mer count on the GPU (gx_kmer_count_regions / gx_kmer_count_peaks / gx_kmer_count_genome, --kmers) against
tests/kmers_ref.py, at the smallest shapes where the kernel can go wrong: the chromosomes of the gcbias and motifs tests (around the
word, 64, and the directory block, 512), regions that start and end around the word and the chromosome's end and that are one
shorter than k, equal to k and one longer, k = 1, 2, 3 and 7 (LDS counters), 8 and 12 (global atomics), every geometry, flushes
forced, a homopolymer (one add per wavefront), unknown bases across a word's end.  Every comparison is == on integers or text."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import golden_cases as G
import kmers_ref as R
import motifs_ref as MR
from genrich_amd import synth
from genrich_amd.lib import GX_PATH_KMERS, format_kmers, kmer_count_genome_group, kmer_geometry, kmers_text
from test_hip_counts import _cli_inputs
from test_hip_gcbias import LENS, _cli_genome, _push_whole, _seqs, _write_fasta
from test_hip_motifs import RUN_LENS, _ctx, _regions, _run
from test_host_cli import _binary

pytestmark = pytest.mark.gpu

ORDER = -10
LANES, GRID, POSITIONS, STEP, FLUSH, MAX_K, LDS_MAX_K = kmer_geometry()
KS = (1, 2, 3, 7, 8, 12)


@pytest.fixture(scope="module")
def genome():
    seqs = _seqs(3)
    return seqs, MR.genome(seqs, LENS)


@pytest.fixture(scope="module")
def loaded(genome):
    h = _ctx()
    _push_whole(h, genome[0])
    yield h
    h.close()


def _border_rows():
    """The motifs test's rows at every border, with the short regions sized by k instead of by a motif's width."""
    rows = []
    for c, n in enumerate(LENS):
        pts = sorted({0, 1, 63, 64, 65, max(n - 65, 0), max(n - 64, 0), max(n - 1, 0), n, n + 7})
        rows += [(c, s, e) for s in pts for e in pts if s <= e <= s + 600]      # (empty ones among them)
    for k in KS:                                                       # one shorter than k, equal to k and one longer
        rows += [(9, 700, 700 + k - 1), (9, 700, 700 + k), (9, 700, 700 + k + 1), (10, 200_003 - k, 200_003), (10, 200_003 - k + 1, 200_010)]
    rows += [(9, 900, 100), (10, 5, 2)]                                # inverted
    rows += [(10, 1000, 3000), (10, 2000, 4000), (10, 1000, 3000), (10, 1000, 3000)]   # overlapping and repeated
    rows += [(11, 0, 500), (1 << 31, 0, 500)]                          # outside the table
    return rows


def _same(got, want):
    counts, windows = got
    assert windows == want[1] and int(counts.sum()) == windows
    assert np.array_equal(counts.astype(np.int64), want[0])


# ---- regions against the reference --------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_regions_at_every_border(genome, loaded, k):
    rows = _border_rows()
    want = R.count(genome[1], rows, k)
    assert want[1] > 1000 and (k > 3 or all(want[0] > 0))
    _same(loaded.kmer_count_regions(_regions(rows), k), want)
    assert loaded.kmer_last()[0] == (0 if k <= LDS_MAX_K else 1)       # both paths are taken: LDS up to 7, HBM from 8
    assert loaded.path_info() & GX_PATH_KMERS
    got = loaded.kmer_count_regions(_regions([]), k)
    assert got[1] == 0 and not got[0].any()
    for short in ([(9, 700, 700 + k - 1)], [(9, 900, 100)], [(11, 0, 500)]):                   # nothing to count: no window, no error
        got = loaded.kmer_count_regions(_regions(short), k)
        assert got[1] == 0 and not got[0].any()


def test_random_regions_in_every_geometry(genome, loaded):
    rng = np.random.default_rng(11)
    c = rng.integers(0, len(LENS), 400)
    ln = np.asarray(LENS)[c]
    a = rng.integers(0, 1 << 30, 400) % (ln + 9)
    b = np.minimum(a + rng.integers(0, 200, 400), ln + 9)
    rows = list(zip(c.tolist(), a.tolist(), b.tolist())) + [(10, 100_000, 140_000)]
    reg = _regions(rows)
    for k in (3, 7, 8):
        want = R.count(genome[1], rows, k)
        for kw in [{}, {"grid": 1}, {"grid": 3}, {"step_words": 1}, {"step_words": 16}, {"flush_runs": 1}, {"flush_runs": 3}, {"flush_runs": FLUSH},
                   {"grid": 1, "step_words": 1, "flush_runs": 1}, {"grid": 3, "step_words": 16, "flush_runs": 3}]:
            _same(loaded.kmer_count_regions(reg, k, **kw), want)
            path, flushes = loaded.kmer_last()
            assert path == (0 if k <= LDS_MAX_K else 1), (k, kw)
            if path == 0 and kw.get("flush_runs", FLUSH) < FLUSH and kw.get("grid"):           # few workgroups, many rounds each: flushes forced
                assert flushes > 0, (k, kw)
            if "flush_runs" not in kw or path == 1:
                assert flushes == 0, (k, kw)
        loaded.kmer_force_hbm(True)                                                            # the other path gives the same arrays
        _same(loaded.kmer_count_regions(reg, k), want)
        assert loaded.kmer_last() == (1, 0)
        loaded.kmer_force_hbm(False)


def test_what_is_refused(genome, loaded):
    lib, ctx = loaded.lib, loaded.ctx
    err = lambda: lib.gx_last_error(ctx).decode()
    reg = _regions([(10, 0, 1000)])
    w = C.c_uint64(0)
    for k, args, msg in ((0, (0, 0, 0), "1 <= k <= 12"), (13, (0, 0, 0), "1 <= k <= 12"), (-1, (0, 0, 0), "1 <= k <= 12"), (4, (65_536, 0, 0), "65535 workgroups"),
                         (4, (0, 17, 0), "1 to 16 words"), (4, (0, 0, (1 << 25) + 1), "1 to 2^25 runs")):
        assert lib.gx_kmer_count_regions(ctx, reg.ctypes.data, 1, k, *args, None, C.byref(w)) == ORDER and msg in err(), (k, args)
    assert lib.gx_kmer_count_peaks(ctx, 4, -1, None, None) == ORDER and "after gx_find_peaks" in err()
    assert lib.gx_get_kmer_counts(ctx, None, 0) == ORDER
    h = _ctx(bases=False)                                              # no bases
    for call in (lambda: h.lib.gx_kmer_count_regions(h.ctx, None, 0, 4, 0, 0, 0, None, None), lambda: h.lib.gx_kmer_count_peaks(h.ctx, 4, -1, None, None),
                 lambda: h.lib.gx_kmer_count_genome(h.ctx, 4, None, 0, None)):
        assert call() == ORDER and "gx_set_genome_bases" in h.lib.gx_last_error(h.ctx).decode()
    h.close()
    h = _ctx()                                                         # a sample open
    h.sample_begin(0, None)
    assert h.lib.gx_kmer_count_regions(h.ctx, None, 0, 4, 0, 0, 0, None, None) == ORDER and "a sample is open" in h.lib.gx_last_error(h.ctx).decode()
    assert h.lib.gx_kmer_count_genome(h.ctx, 4, None, 0, None) == ORDER and "a sample is open" in h.lib.gx_last_error(h.ctx).decode()
    h.close()


# ---- a constructed chromosome -------------------------------------------------------------------------------------------------

def test_a_homopolymer_a_repeat_and_unknown_bases_across_a_words_end():
    """4,096 A, then (AC)n, then a stretch of random bases; one N at offsets 62 .. 66 of a word in each of the three.  The runs
    inside the homopolymer hold one k-mer in every counted lane: one lane adds for the wavefront, and the counter must equal the
    closed form.  The unknown bases are more than k apart and from the ends: each removes exactly k windows."""
    rng = np.random.default_rng(31)
    clean = b"A" * 4096 + b"AC" * 1000 + bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 3000)])
    n = len(clean)
    at = [64 * w + 62 + i for i, w in enumerate((10, 20, 30, 40, 50))] + [4096 + 64 * w + 62 + i for i, w in enumerate((3, 8, 13, 18, 23))] + \
         [6144 + 64 * w + 62 + i for i, w in enumerate((3, 8, 13, 18, 23))]
    assert sorted(a % 64 for a in at) == [0, 0, 0, 1, 1, 1, 2, 2, 2, 62, 62, 62, 63, 63, 63]
    dirty = bytearray(clean)
    for a in at:
        dirty[a] = ord("N")
    h = _ctx([n])
    reg = _regions([(0, 0, n)])
    for k in (7, 8):
        poly_a, ac, ca = R.code_of("A" * k), R.code_of(("AC" * k)[:k]), R.code_of(("CA" * k)[:k])
        res = []
        for s in (clean, bytes(dirty)):
            h.push_sequence(0, 0, s)
            gen = MR.genome([s], [n])
            want = R.count(gen, [(0, 0, n)], k)
            for kw in ({}, {"grid": 1, "step_words": 1}, {"flush_runs": 1, "grid": 2}):
                _same(h.kmer_count_regions(reg, k, **kw), want)
            res.append(want)
        (c0, w0, _), (c1, w1, _) = res
        assert w0 == n - k + 1 and w0 - w1 == len(at) * k              # every N removes exactly k windows
        assert c0[poly_a] == 4097 - k + 1 and c1[poly_a] == 4097 - k + 1 - 5 * k               # the run is 4,096 A and the repeat's first
        assert c0[ac] + c0[ca] >= 2000 - k and c0[ac] + c0[ca] - (c1[ac] + c1[ca]) == 5 * k
    h.close()


def test_pushes_in_shuffled_pieces_of_64_bases_give_the_same_counts(genome):
    seqs, gen = genome
    rng = np.random.default_rng(5)
    h = _ctx()
    pieces = [(c, a, s[a:a + 64]) for c, s in enumerate(seqs) for a in range(0, len(s), 64) if c < 10] + [(10, 0, seqs[10])]
    for i in rng.permutation(len(pieces)):
        h.push_sequence(*pieces[i])
    rows = [(c, 0, n) for c, n in enumerate(LENS)] + [(9, 60, 70), (8, 500, 513)]
    for k in (3, 8):
        _same(h.kmer_count_regions(_regions(rows), k), R.count(gen, rows, k))
    h.close()


# ---- the genome and the peaks -----------------------------------------------------------------------------------------------

def test_the_genome_pass_with_a_skipped_chromosome_and_two_contexts_that_add_up(genome, loaded):
    seqs, gen = genome
    for k in (4, 9):
        want = R.count_genome(gen, k)
        _same(loaded.kmer_count_genome(k), want)
        skip = [0] * 9 + [1, 0]
        h = _ctx(skip=skip)
        _push_whole(h, seqs)
        _same(h.kmer_count_genome(k), R.count_genome(gen, k, [int(not s) for s in skip]))
        h.close()
        hs = []
        for owned in ([1, 0] * 5 + [0], [0, 1] * 5 + [1]):
            h = _ctx(owned=owned)
            _push_whole(h, seqs)
            _same(h.kmer_count_genome(k), R.count_genome(gen, k, owned))
            hs.append(h)
        _same(kmer_count_genome_group(hs, k), want)
        _same(kmer_count_genome_group([loaded], k), want)
        for h in hs:
            h.close()


def test_the_peaks_of_a_run_with_every_flank_and_the_table():
    seqs = _seqs(29, RUN_LENS)
    gen = MR.genome(seqs, RUN_LENS)
    ev = synth.make_fragments(RUN_LENS, 250_000, 40, peak_every=20_000, tower_every=3_000_000)
    h = _run(seqs, [], ev)
    assert h.n_peaks > 20 and not h.path_info() & GX_PATH_KMERS           # nothing of it before the first call
    assert h.lib.gx_get_kmer_counts(h.ctx, None, 0) == ORDER
    pk = h.get_peaks()
    peaks = list(zip(pk["chrom"].tolist(), pk["start"].tolist(), pk["end"].tolist()))
    longest = max(e - s for c, s, e in peaks)
    k = 6
    cg, wg = R.count_genome(gen, k)
    for flank in (-1, 0, 10, longest + 5):
        rows = R.flank_regions(peaks, pk["summit"].tolist(), flank)
        want = R.count(gen, rows, k)
        assert h.kmer_count_peaks(k, flank) == want[1:]
        _same((h.get_kmer_counts(), want[1]), want)
        assert h.path_info() & GX_PATH_KMERS
        if flank == 0:
            assert want[1:] == (0, 0)                                  # one base per peak: no window of 6
        if flank in (-1, longest + 5):
            assert want[1] == R.count(gen, peaks, k)[1] > 1000
        text = R.text(k, flank, want[2], want[1], wg, want[0], cg, 50)
        assert kmers_text([h], k, flank, 50).decode() == text
        assert format_kmers(k, flank, want[2], want[1], wg, h.get_kmer_counts(), h.kmer_count_genome(k)[0], 50).decode() == text
    for k_bad in (0, 13):
        assert h.lib.gx_kmer_count_peaks(h.ctx, k_bad, -1, None, None) == ORDER and "1 <= k <= 12" in h.lib.gx_last_error(h.ctx).decode()
    h.reset()                                                          # the results go with the run
    assert h.lib.gx_get_kmer_counts(h.ctx, None, 0) == ORDER and not h.path_info() & GX_PATH_KMERS
    h.close()


# ---- the command line ------------------------------------------------------------------------------------------------------

def test_cli_kmers_of_a_golden_fixture_on_one_and_two_contexts():
    name = "ctrl_q"
    case, names, seqs = _cli_genome(name)
    gen = MR.genome(seqs, case["lens"])
    meta, args, tmp, _ = _cli_inputs(name)
    fa, out = os.path.join(tmp, "kmer_genome.fa"), os.path.join(tmp, "kmer_out")
    _write_fasta(fa, names, seqs)
    K, FLANK = 6, 25
    rows = [l.split("\t") for l in G.read_gz(name, "out.narrowPeak").decode().splitlines()]
    peaks = [(names.index(r[0]), int(r[1]), int(r[2])) for r in rows]
    summit = [int(r[9]) for r in rows]
    active = [int(not s) for s in case["skip"]]
    took = [int(a and bool(v)) for a, v in zip(active, case["replicates"][-1]["save"])]
    cp, wp, n_reg = R.count(gen, R.flank_regions(peaks, summit, FLANK), K, active)
    cg, wg = R.count_genome(gen, K, took)
    assert wp > 100 and wg > wp
    want = R.text(K, FLANK, n_reg, wp, wg, cp, cg, 100)
    want_all = R.text(K, FLANK, n_reg, wp, wg, cp, cg, 0)
    assert want.count("\n") == 102 < want_all.count("\n")
    for extra in ([], ["--devices", "0,0"]):
        res = subprocess.run([_binary(), "-v", "-o", out + ".narrowPeak", "--genome", fa, "--kmers", out + ".kmers", "--kmer-k", str(K), "--kmer-flank", str(FLANK)] + extra + args,
                             capture_output=True, text=True)
        assert res.returncode == 0, (extra, res.stderr)
        assert open(out + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")
        assert open(out + ".kmers").read() == want, extra
        err = res.stderr.splitlines()
        assert any(l.startswith("K-mers (k = 6): %d windows in %d regions of the peaks, %d in the genome" % (wp, n_reg, wg)) for l in err), res.stderr
        assert sum(l.startswith("  K-mer ") for l in err) == 3 and any(l.startswith("  K-mers: the peaks in ") for l in err)
        os.remove(out + ".kmers")
    res = subprocess.run([_binary(), "-o", out + ".np2", "--genome", fa, "--kmers", out + ".all", "--kmer-k", str(K), "--kmer-flank", str(FLANK), "--kmer-top", "0",
                          "--gc-peaks", out + ".gcpeaks"] + args, capture_output=True, text=True)
    assert res.returncode == 0 and open(out + ".all").read() == want_all and open(out + ".np2", "rb").read() == G.read_gz(name, "out.narrowPeak")
