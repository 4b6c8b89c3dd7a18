"""The genome's bit vectors, GC content and GC bias on the GPU (gx_set_genome / gx_push_sequence / gx_gc_content / gx_gc_bias)
against tests/gcbias_ref.py, at the smallest shapes where the kernels can go wrong: chromosomes around the word (64), the tile
halo and the directory block (512), windows around the word and at both ends of their range, every launch geometry, every split
of the pushes.  Every comparison is == on integers; there is no tolerance anywhere."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import backends as B
import gcbias_ref as R
import golden_cases as G
from genrich_amd.lib import GC_MAX_WINDOW, GX_PATH_GC, REGION_DTYPE, gc_bias_group, gc_bias_text, pack_events
from test_hip_counts import _cli_inputs
from test_host_cli import _binary

pytestmark = pytest.mark.gpu

ORDER = -10
LENS = [1, 63, 64, 65, 127, 128, 511, 512, 513, 5000, 200_003]
WINDOWS = [1, 2, 63, 64, 65, 200, 4095, 4096]
ALPHABET = np.frombuffer(b"ACGTACGTACGTacgtacgtNnRYKMSWBDHVrykm", dtype=np.uint8)   # (a few unknown bases: long classed stretches exist)


def _seqs(seed, lens=LENS, unknown=0.001):
    """Random bases in both cases with a few N and IUPAC codes, rare enough that windows of 200 are mostly classed; 10,000 bases
    of the longest chromosome hold none, so that some window of 4096 is classed."""
    rng = np.random.default_rng(seed)
    out = []
    for n in lens:
        s = np.frombuffer(b"ACGTacgt", dtype=np.uint8)[rng.integers(0, 8, n)].copy()
        bad = rng.random(n) < unknown
        bad[100_000:110_000] = False
        s[bad] = ALPHABET[rng.integers(16, len(ALPHABET), int(bad.sum()))]
        out.append(bytes(s))
    return out


def _ctx(lens=LENS, skip=None, owned=None, genome=True):
    import genrich_amd
    h = genrich_amd.Genrich(B.make_params(pq=0.01, min_auc=20.0))
    h.set_chroms(lens, skip)
    if owned is not None:
        h.set_owned(owned)
    if genome:
        h.set_genome(True)
    return h


def _push_whole(h, seqs):
    for c, s in enumerate(seqs):
        if s is not None:
            h.push_sequence(c, 0, s)


def _whole(lens):
    reg = np.zeros(len(lens), dtype=REGION_DTYPE)
    reg["chrom"], reg["end"] = np.arange(len(lens)), lens
    return reg


def _pairs(a):
    return [(int(g), int(x)) for g, x in zip(*a)]


@pytest.fixture(scope="module")
def genome():
    seqs = _seqs(3)
    return seqs, R.genome(seqs, LENS)


@pytest.fixture(scope="module")
def loaded(genome):
    h = _ctx()
    _push_whole(h, genome[0])
    yield h
    h.close()


def _events(n, seed, lens=LENS, W=200):
    """n events a sample takes: starts anywhere, a third within W of either end of their chromosome; a tenth inverted; every
    weight class."""
    rng = np.random.default_rng(seed)
    ev = np.zeros(n, dtype=B.EVENT_DTYPE)
    ev["chrom"] = rng.integers(0, len(lens), n)
    ln = np.asarray(lens)[ev["chrom"]]
    where = rng.integers(0, 3, n)
    st = rng.integers(0, 1 << 30, n) % ln
    st = np.where(where == 1, rng.integers(0, W + 2, n) % ln, st)
    st = np.where(where == 2, np.maximum(ln - 1 - rng.integers(0, W + 2, n), 0), st)
    ev["start"] = st
    ev["end"] = st + rng.integers(0, 400, n)
    inv = rng.random(n) < 0.1
    ev["end"][inv] = np.maximum(st[inv].astype(np.int64) - 30, 0)
    ev["count"] = rng.choice(R.VALID_COUNTS, n)
    return ev


# ---- pack ------------------------------------------------------------------------------------------------------------------

def test_pack_in_one_push_and_in_shuffled_pieces(genome):
    seqs, gen = genome
    want = R.content(gen, [(c, 0, n) for c, n in enumerate(LENS)])
    total = (sum(LENS), sum(g for g, a in want), sum(a for g, a in want))
    assert 0 < total[1] < total[2] < total[0]
    rng = np.random.default_rng(5)
    for split in (False, True):
        h = _ctx()
        assert h.genome_info() == (0, 0, 0) and _pairs(h.gc_content(_whole(LENS))) == [(0, 0)] * len(LENS)
        pieces = []
        for c, s in enumerate(seqs):
            cuts = [0, len(s)]
            if split and len(s) > 64:
                cuts = sorted(set(cuts + [64 * int(x) for x in rng.integers(1, (len(s) + 63) // 64, 6)]))
            pieces += [(c, a, s[a:b]) for a, b in zip(cuts, cuts[1:])]
        assert (len(pieces) > 2 * len(LENS)) == split
        for i in rng.permutation(len(pieces)) if split else range(len(pieces)):
            h.push_sequence(*pieces[i])
        assert h.genome_info() == total and h.path_info() & GX_PATH_GC
        assert _pairs(h.gc_content(_whole(LENS))) == want
        for i in (0, len(pieces) // 2, len(pieces) - 1):      # the same stretch once more: nothing changes
            h.push_sequence(*pieces[i])
        assert h.genome_info() == total and _pairs(h.gc_content(_whole(LENS))) == want
        h.close()


def test_pushes_that_are_refused_and_chromosomes_that_take_nothing(genome):
    seqs, gen = genome
    h = _ctx(skip=[0] * 9 + [1, 0], owned=[1] * 8 + [0, 1, 1])
    lib, ctx = h.lib, h.ctx
    err = lambda: lib.gx_last_error(ctx).decode()
    s = seqs[10]
    for chrom, first, n, msg in ((10, 1, 64, "multiple of 64"), (10, 32, 32, "multiple of 64"), (10, 199_936, 128, "past the chromosome's length"),
                                 (10, 200_064, 0, "past the chromosome's length"), (4, 0, 128, "past the chromosome's length"),
                                 (10, 0, 100, "last push may end inside a word"), (11, 0, 1, "outside the table"), (-1, 0, 1, "outside the table")):
        assert lib.gx_push_sequence(ctx, chrom, first, s, n) == ORDER and msg in err(), (chrom, first, n, err())
    assert h.genome_info() == (0, 0, 0)
    _push_whole(h, seqs)                                          # 8 is not owned, 9 is skipped: no error, no bits
    want = R.content(gen, [(c, 0, n) for c, n in enumerate(LENS)])
    want[8] = want[9] = (0, 0)
    assert _pairs(h.gc_content(_whole(LENS))) == want
    h.push_sequence(10, 199_936, s[199_936:])                     # a last push that ends inside a word
    assert _pairs(h.gc_content(_whole(LENS))) == want
    h.set_chroms(LENS)                                            # a new table: the genome is laid out again, empty
    assert h.genome_info() == (0, 0, 0)
    h.set_genome(False)
    assert lib.gx_push_sequence(ctx, 0, 0, s, 1) == ORDER and lib.gx_genome_info(ctx, None, None, None) == ORDER
    n = C.c_int(0)
    assert lib.gx_gc_bias(ctx, 200, C.byref(n)) == ORDER and "gx_set_genome" in err()
    h.close()


# ---- content and the directory ---------------------------------------------------------------------------------------------

def test_content_at_every_border_and_at_random(genome, loaded):
    seqs, gen = genome
    rows = []
    for c, n in enumerate(LENS):
        pts = sorted({0, 1, 63, 64, 65, 511, 512, 513, max(n - 1, 0), n, n + 7})
        rows += [(c, s, e) for s in pts for e in pts if s <= e]
    rows += [(0, 5, 2), (10, 70_000, 3), (11, 0, 5), (1 << 31, 0, 5)]             # end before start; a chromosome outside the table
    rng = np.random.default_rng(9)
    c = rng.integers(0, len(LENS), 100_000)
    a, b = rng.integers(0, 1 << 30, 100_000) % (np.asarray(LENS)[c] + 9), rng.integers(0, 1 << 30, 100_000) % (np.asarray(LENS)[c] + 9)
    rows += list(zip(c.tolist(), np.minimum(a, b).tolist(), np.maximum(a, b).tolist()))
    reg = np.asarray(rows, dtype=np.uint32).view(REGION_DTYPE).reshape(-1)
    assert len(reg) > 100_000 and _pairs(loaded.gc_content(reg)) == R.content(gen, rows)
    assert _pairs(loaded.gc_content(reg[:0])) == []


# ---- expected --------------------------------------------------------------------------------------------------------------

NONE = np.zeros(0, dtype=B.EVENT_DTYPE)


@pytest.mark.parametrize("W", WINDOWS)
def test_expected_in_every_geometry(genome, loaded, W):
    """W above and below the word, the tile's halo and most chromosomes' lengths; one workgroup against the default grid; the
    smallest tile; a flush of the 32-bit counters before every tile."""
    F, un = R.expected(genome[1], W)
    assert sum(F) + un == sum(LENS) and sum(F) > 0 and un > 0
    for kw in ({}, {"grid_expected": 1}, {"tile_words": 64}, {"tile_words": 64, "flush_words": 64}, {"grid_expected": 3, "tile_words": 1024, "flush_words": 1024},
               {"grid_expected": 1, "tile_words": 128, "flush_words": 256}):
        got = loaded.gc_bias_events(NONE, W, **kw)
        assert ([int(x) for x in got.F], got.f_unclassed) == (F, un), (W, kw)
        assert not got.Nn.any() and not got.Nw.any() and got.n_unclassed == got.w_unclassed == 0


def test_one_unknown_base_leaves_unclassed_exactly_the_windows_that_cover_it():
    lens = [3000, 700]
    rng = np.random.default_rng(13)
    clean = [bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)]) for n in lens]
    h = _ctx(lens)
    for W in (1, 64, 200):
        for pos in (0, 63, 64, lens[0] - 1):
            s = bytearray(clean[0])
            s[pos] = ord("N")
            _push_whole(h, [bytes(s), clean[1]])
            got = h.gc_bias_events(NONE, W)
            covering = {x for x in range(max(0, pos - W + 1), pos + 1)} | {x for x in range(lens[0] - W + 1, lens[0])}
            assert got.f_unclassed == len(covering) + (W - 1) and int(got.F.sum()) == sum(lens) - got.f_unclassed, (W, pos)
            assert ([int(x) for x in got.F], got.f_unclassed) == R.expected(R.genome([bytes(s), clean[1]], lens), W)
    h.close()


def test_all_gc_next_to_all_at():
    lens = [1000, 1000, 130]
    seqs = [b"GC" * 500, b"AT" * 500, b"g" * 130]
    h = _ctx(lens)
    _push_whole(h, seqs)
    for W in (1, 65, 200):
        got = h.gc_bias_events(NONE, W)
        F = [int(x) for x in got.F]
        assert F[0] == 1000 - W + 1 and F[W] == (1000 - W + 1) + max(130 - W + 1, 0) and sum(F) == F[0] + (F[W] if W else 0)
        assert got.f_unclassed == sum(lens) - sum(F)
    h.close()


# ---- observed --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [65_535, 65_536, 65_537])
def test_observed_around_the_chunk_border_in_both_event_forms(genome, n):
    seqs, gen = genome
    seqs, gen = list(seqs), list(gen)
    seqs[6], gen[6] = None, R.pack(None, LENS[6])                  # a chromosome without sequence: its intervals are not classed
    h = _ctx()
    _push_whole(h, seqs)
    ev = _events(n, n)
    assert len(set(ev["count"].tolist())) == 8 and (ev["end"] < ev["start"]).sum() > n // 20 and (ev["chrom"] == 6).sum() > 100
    for W in (200, 1, 4096):
        want = R.tables(gen, ev, W)
        assert want.n_unclassed > 100 and sum(want.Nn) > {1: n // 2, 200: n // 10, 4096: 0}[W]
        for kw in ({}, {"grid_observed": 1}, {"grid_observed": 7}):
            assert R.same(h.gc_bias_events(ev, W, **kw), want), (W, kw)
    ev8, rest = pack_events(ev)
    assert len(ev8) > n // 2 and len(rest) > n // 20
    fits = ev[(ev["end"] >= ev["start"])]
    assert len(fits) == len(ev8)
    assert R.same(h.gc_bias_events(ev8, 200, packed=True), R.tables(gen, fits, 200))
    bad = _events(1000, 1)                                         # what a sample refuses is none of its intervals
    bad["count"][::3], bad["chrom"][1::3] = 7, len(LENS)
    bad["start"][2::3] = np.asarray(LENS)[bad["chrom"][2::3] % len(LENS)]
    bad["chrom"][2::3] %= len(LENS)
    assert R.same(h.gc_bias_events(bad, 65), R.tables(gen, bad, 65))
    lib, ctx = h.lib, h.ctx
    for W in (0, -1, GC_MAX_WINDOW + 1):
        assert lib.gx_gc_bias_events(ctx, ev.ctypes.data, 10, 0, W, 0, 0, 0, 0, None, None, None, None, None, None, 0) == ORDER
        assert "1 <= W <= 4096" in lib.gx_last_error(ctx).decode()
    for args, msg in (((0, 100, 0, 0), "multiple of 64"), ((0, 2048, 0, 0), "multiple of 64"), ((0, 128, 64, 0), "flush bound"), ((0, 0, 1 << 26, 0), "flush bound"),
                      ((65_536, 0, 0, 0), "65535 workgroups"), ((0, 0, 0, 65_536), "65535 workgroups")):
        assert lib.gx_gc_bias_events(ctx, ev.ctypes.data, 10, 0, 200, *args, None, None, None, None, None, None, 0) == ORDER
        assert msg in lib.gx_last_error(ctx).decode(), args
    h.close()


# ---- real samples ----------------------------------------------------------------------------------------------------------

# chromosome 2 is skipped (-e), 5 is outside the sample's save mask, 7 is not owned by the context
SKIP, SAVE, OWNED = [0, 0, 1] + [0] * 8, [1] * 5 + [0] + [1] * 5, [1] * 7 + [0] + [1] * 3
ACTIVE = [int(not s and v and o) for s, v, o in zip(SKIP, SAVE, OWNED)]


def _sample_events(n, seed, lens=LENS):
    """Events a sample can be built from: fragments of 40 .. 400 bases inside chromosomes 9 and 10 and a few on every other one."""
    rng = np.random.default_rng(seed)
    ev = np.zeros(n, dtype=B.EVENT_DTYPE)
    ev["chrom"] = np.where(rng.random(n) < 0.9, rng.choice([9, 10], n), rng.integers(0, len(lens), n))
    ln = np.asarray(lens)[ev["chrom"]]
    ev["start"] = rng.integers(0, 1 << 30, n) % ln
    ev["end"] = np.minimum(ev["start"] + rng.integers(40, 400, n), ln)
    ev["count"] = rng.choice([1, 1, 1, 2, 3], n)
    return ev


def _run(ev_t, ev_c, seqs, skip=SKIP, save=SAVE, owned=OWNED):
    h = _ctx(skip=skip, owned=owned)
    _push_whole(h, seqs)
    h.expect_fractional(True)
    h.set_count_in_peaks(True)
    h.sample_begin(0, save)
    h.push_events(ev_t)
    h.sample_end()
    if ev_c is not None:
        h.sample_begin(1, None)
        h.push_events(ev_c)
        h.sample_end()
    return h


def test_real_samples_under_the_masks_with_a_control(genome):
    seqs, gen = genome
    ev_t, ev_c = _sample_events(40_000, 51), _sample_events(30_000, 52)
    h = _run(ev_t, ev_c, seqs)
    assert h.gc_bias(200) == 2
    t, c = h.get_gc_bias(0), h.get_gc_bias(1)
    want_t, want_c = R.tables(gen, ev_t, 200, ACTIVE), R.tables(gen, ev_c, 200, ACTIVE)
    assert R.same(t, want_t) and (t.rep, t.is_ctrl) == (0, False)
    assert R.same(c, want_c) and (c.rep, c.is_ctrl) == (0, True)
    assert sum(want_t.Nn) > 20_000 and sum(want_t.F) + want_t.f_unclassed == sum(n for n, a in zip(LENS, ACTIVE) if a) and h.path_info() & GX_PATH_GC
    assert h.gc_bias(64) == 2 and R.same(h.get_gc_bias(1), R.tables(gen, ev_c, 64, ACTIVE))      # another window: the tables are made again
    assert gc_bias_text([h], 200).decode() == R.bias_text([(0, False, want_t), (0, True, want_c)])
    lib, ctx = h.lib, h.ctx
    n = C.c_int(0)
    assert lib.gx_gc_bias(ctx, 0, C.byref(n)) == ORDER and "1 <= W <= 4096" in lib.gx_last_error(ctx).decode()
    h.close()


def test_two_contexts_add_up_to_one(genome):
    seqs, gen = genome
    ev = _sample_events(40_000, 53)
    none = [0] * len(LENS)
    one = _run(ev, None, seqs, skip=none, save=None, owned=[1] * len(LENS))
    assert one.gc_bias(200) == 1
    whole = R.tables(gen, ev, 200)
    assert R.same(one.get_gc_bias(0), whole)
    hs = []
    for owned in ([1, 0] * 5 + [0], [0, 1] * 5 + [1]):
        h = _run(ev, None, seqs, skip=none, save=None, owned=owned)
        assert h.gc_bias(200) == 1 and R.same(h.get_gc_bias(0), R.tables(gen, ev, 200, owned))
        hs.append(h)
    got = gc_bias_group(hs, 0)
    assert R.same(got, whole) and R.same(got, R.add([h.get_gc_bias(0) for h in hs])) and (got.rep, got.is_ctrl) == (0, False)
    assert gc_bias_text(hs, 200) == gc_bias_text([one], 200)
    for h in hs + [one]:
        h.close()


def test_order_rules(genome):
    seqs, gen = genome
    h = _ctx(genome=False)
    lib, ctx = h.lib, h.ctx
    err = lambda: lib.gx_last_error(ctx).decode()
    n = C.c_int(0)
    assert lib.gx_gc_content(ctx, None, 0, None, None) == ORDER                                    # no genome
    h.set_genome(True)
    assert lib.gx_gc_bias(ctx, 200, C.byref(n)) == ORDER and "gx_set_count_in_peaks" in err()
    h.set_count_in_peaks(True)
    assert lib.gx_gc_bias(ctx, 200, C.byref(n)) == ORDER and "no closed sample" in err()
    h.sample_begin(0, None)
    assert lib.gx_gc_bias(ctx, 200, C.byref(n)) == ORDER and "a sample is open" in err()
    assert lib.gx_set_genome(ctx, 1) == ORDER and "a sample is open" in err()
    _push_whole(h, seqs)                                                                           # bases may come while a sample is open
    h.push_events(_sample_events(20_000, 54))
    h.sample_end()
    assert lib.gx_get_gc_bias(ctx, 0, None, None, None, None, None, None, None, None, None, 0) == ORDER     # no pass yet
    assert h.gc_bias(200) == 1 and R.same(h.get_gc_bias(0), R.tables(gen, _sample_events(20_000, 54), 200))
    assert lib.gx_get_gc_bias(ctx, 1, None, None, None, None, None, None, None, None, None, 0) == ORDER
    h.close()


# ---- the command line ------------------------------------------------------------------------------------------------------

# a control (-q); three replicates with a missing chromosome; ATAC -j (cut-site windows); -e; -r -y -s (fractional weights)
CLI = ["ctrl_q", "reps3_p_missing", "atac", "bedx", "dups_y"]


def _cli_genome(name, seed=7):
    meta, case, params, names = G.load_case(name)
    seqs = _seqs(seed, case["lens"], unknown=0.002)
    return case, names, seqs


def _write_fasta(path, names, seqs, width=60):
    """The sequences under their names (the first with a description), behind one that no header names."""
    with open(path, "wb") as f:
        f.write(b">chrUn_extra not in any header\nACGTNNNNACGT\nAC\n")
        for i, (n, s) in enumerate(zip(names, seqs)):
            if s is None:
                continue
            f.write(b">" + n.encode() + (b" the first one\n" if i == 0 else b"\n"))
            f.write(b"".join(s[k:k + width] + b"\n" for k in range(0, len(s), width)))


def _cli_samples(case, gen, W):
    out = []
    for r, rep in enumerate(case["replicates"]):
        active = [int(not k and bool(v)) for k, v in zip(case["skip"], rep["save"])]
        out.append((r, False, R.tables(gen, rep["treat"], W, active)))
        if rep["ctrl"] is not None:
            out.append((r, True, R.tables(gen, rep["ctrl"], W, active)))
    return out


def _cli_peaks(name, names, gen):
    rows = [l.split("\t") for l in G.read_gz(name, "out.narrowPeak").decode().splitlines()]
    regions = [(names.index(r[0]), int(r[1]), int(r[2])) for r in rows]
    return R.peaks_text(names, regions, R.content(gen, regions))


@pytest.mark.parametrize("name", CLI)
def test_cli_gc_bias_and_gc_peaks_of_the_golden_fixtures(name):
    case, names, seqs = _cli_genome(name)
    gen = R.genome(seqs, case["lens"])
    meta, args, tmp, _ = _cli_inputs(name)
    fa, out = os.path.join(tmp, "gc_genome.fa"), os.path.join(tmp, "gc_out")
    _write_fasta(fa, names, seqs)
    res = subprocess.run([_binary(), "-v", "-o", out + ".narrowPeak", "-b", out + ".bed", "--genome", fa, "--gc-bias", out + ".bias", "--gc-peaks", out + ".peaks"] + args,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert open(out + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak") and open(out + ".bed", "rb").read() == G.read_gz(name, "events.bed")
    samples = _cli_samples(case, gen, 200)
    assert open(out + ".bias").read() == R.bias_text(samples)
    assert open(out + ".peaks").read() == _cli_peaks(name, names, gen)
    assert sum(sum(t.Nn) for _, _, t in samples) > 1000
    lines = [l for l in res.stderr.splitlines() if l.startswith("  GC bias, ")]
    assert len(lines) == len(samples) and all("mean window GC 0." in l and "(genome 0." in l for l in lines), lines
    assert "Warning!" not in "".join(l for l in res.stderr.splitlines() if "is not in" in l)
    kept = [s for s, k in zip(seqs, case["skip"]) if not k]
    assert any(l.startswith("Genome " + fa + ": %d sequences, %d bases" % (len(kept), sum(len(s) for s in kept))) for l in res.stderr.splitlines()), res.stderr


def test_cli_window_gzip_no_peaks_and_two_contexts():
    name = "ctrl_q"
    case, names, seqs = _cli_genome(name)
    gen = R.genome(seqs, case["lens"])
    meta, args, tmp, _ = _cli_inputs(name)
    fa, out = os.path.join(tmp, "gc_genome2.fa"), os.path.join(tmp, "gc_out2")
    _write_fasta(fa, names, seqs, width=61)
    want = R.bias_text(_cli_samples(case, gen, 64))
    res = subprocess.run([_binary(), "-X", "-z", "-f", out + ".log", "--genome", fa, "--gc-bias", out + ".bias", "--gc-window", "64"] + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert gzip.open(out + ".bias.gz", "rb").read().decode() == want
    with open(fa, "rb") as f:                                      # the same FASTA gzip-compressed: through the input stream's inflaters
        gzip.open(fa + ".gz", "wb").write(f.read())
    for extra in (["--devices", "0,0"], ["--genome", fa + ".gz"]):   # chromosomes sharded over two contexts: each sequence to its owner
        res = subprocess.run([_binary(), "-o", out + ".np", "--genome", fa, "--gc-bias", out + ".bias2", "--gc-window", "64", "--gc-peaks", out + ".peaks2",
                              "--counts", out + ".counts"] + extra + args, capture_output=True, text=True)
        assert res.returncode == 0, (extra, res.stderr)
        assert open(out + ".bias2").read() == want and open(out + ".peaks2").read() == _cli_peaks(name, names, gen), extra
        assert open(out + ".np", "rb").read() == G.read_gz(name, "out.narrowPeak")


def test_cli_a_missing_chromosome_warns_and_a_wrong_length_ends_the_run():
    name = "ctrl_q"
    case, names, seqs = _cli_genome(name)
    meta, args, tmp, _ = _cli_inputs(name)
    fa, out = os.path.join(tmp, "gc_genome3.fa"), os.path.join(tmp, "gc_out3")
    _write_fasta(fa, names, [seqs[0], None])
    res = subprocess.run([_binary(), "-v", "-o", out + ".np", "--genome", fa, "--gc-bias", out + ".bias"] + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    warn = [l for l in res.stderr.splitlines() if l.startswith("Warning! ") and "is not in" in l]
    assert len(warn) == 1 and warn[0].startswith("Warning! chr2 is not in " + fa), res.stderr
    assert open(out + ".bias").read() == R.bias_text(_cli_samples(case, R.genome([seqs[0], None], case["lens"]), 200))
    quiet = subprocess.run([_binary(), "-o", out + ".np", "--genome", fa, "--gc-bias", out + ".bias"] + args, capture_output=True, text=True)
    assert quiet.returncode == 0 and "is not in" not in quiet.stderr
    for bad, said in ((seqs[1][:-5], "24995 bases"), (seqs[1] + b"ACGTA", "25005 bases"), (seqs[1][:64 * 300], "19200 bases"), (seqs[1] * 200, "bases or more")):
        _write_fasta(fa, names, [seqs[0], bad])
        res = subprocess.run([_binary(), "-o", out + ".np2", "--genome", fa, "--gc-bias", out + ".bias2"] + args, capture_output=True, text=True)
        assert res.returncode == 1 and "chr2" in res.stderr and said in res.stderr and "25000" in res.stderr, res.stderr
        assert not os.path.exists(out + ".bias2") and not os.path.exists(out + ".np2")
