"""CPU-only checks of the motif feature: the JASPAR reader on good and damaged files, the scores and the exact threshold
(gx_motif_pssm, gx_motif_threshold) against tests/motifs_ref.py -- the threshold by the dynamic program in Python integers and,
up to 8 columns, by enumerating all 4^L L-mers --, the two writers against the reference text, the reader and the host
routines once more in programs of their own under the sanitizers, and the command line's refusals."""
import math
import os
import subprocess

import numpy as np
import pytest

import motifs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "motifs_small.jaspar")
SAN = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def _clean(res):
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr


def _golden():
    return R.read_jaspar(open(GOLDEN, "rb").read())


# ---- the reference by hand ----------------------------------------------------------------------------------------------

def test_the_reference_by_hand():
    ms = _golden()
    assert [(i, n, len(c[0])) for i, n, c in ms] == [("T0001.1", "oneBase", 1), ("T0002.1", "ebox", 6), ("T0003.1", "palindrome", 6), ("T0004.1", "twelve", 12),
                                                    ("T0005.1", "wide32", 32), ("T0006.1", "T0006.1", 2)]
    assert ms[0][2] == [[10], [2], [30], [8]] and ms[3][2][2][:3] == [20, 5, 50]
    # one column, counts 10 2 30 8 of 50, pc 1: 128 log2(((c + .25) / 51) / .25), halves away from zero
    s = R.pssm(ms[0][2])
    assert s == [[round(128 * math.log2((c + 0.25) / 51 / 0.25)) for c in (10, 2, 30, 8)]] == [[-40, -320, 160, -80]]
    # (the LEAST integer that at most K L-mers reach: one above the next score down)
    assert R.threshold(s, 1.0)[:4] == (-320, -320, 160, 4) and R.threshold(s, 0.25)[:4] == (-39, -320, 160, 1) and R.threshold(s, 0.5)[:4] == (-79, -320, 160, 2)
    assert R.threshold(s, 0.2) == (161, -320, 160, 0, True)                      # fewer than one of four: it cannot hit
    # the scan: ACGTN, a motif of two columns that likes AC forward (GT is its reverse complement)
    gen = R.genome([b"ACGTNACgt"], [9])
    two = [[5, 0, 0, 0], [0, 5, 0, 0]]
    hits, cnt = R.scan(gen, [(0, 0, 9), (0, 5, 7), (0, 3, 6), (1, 0, 5)], [(two, 10)])
    assert cnt == [[3 + 3 + 1 + 0], [3], [2]] and hits == [(0, 0, 10, 0, 0), (0, 2, 10, 0, 1), (0, 5, 10, 0, 0), (0, 7, 10, 0, 1), (1, 0, 10, 0, 0)]
    assert R.letters(gen[0], 3, 8) == b"TNACGTNN"
    pal = R.pssm(ms[2][2])                                                       # ACATGT is its own reverse complement: both strands score alike
    assert all(pal[j][b] == pal[5 - j][3 - b] for j in range(6) for b in range(4))
    assert R.hits_text(["c"], [(0, 100, 200)], [30], [(two, 10)], ["I"], ["n"], [0.0625], [(0, 5, 10, 0, 1)]) == \
        "chr\tstart\tend\tmotif\tscore\tstrand\tname\tpeak\toffset_from_summit\tp_threshold\nc\t105\t107\tI\t0.0781\t-\tn\tpeak_0\t-24\t6.250e-02\n"


# ---- the scores and the threshold -------------------------------------------------------------------------------------------

def _matrices():
    rng = np.random.default_rng(41)
    out = [c for _, _, c in _golden()]
    for L in (1, 2, 3, 8, 13, 31, 32):
        out.append(rng.integers(0, 60, (4, L)).tolist())
    out.append([[7] * 9, [7] * 9, [7] * 9, [7] * 9])                             # every score 0: all 4^9 9-mers tie
    out.append([[1 << 30] * 4, [0] * 4, [5] * 4, [(1 << 31) - 1] * 4])           # the largest counts
    out.append([[3, 3, 0], [3, 0, 3], [0, 3, 3], [3, 3, 3]])                     # ties of many L-mers at one score
    return out


PVALUES = [1.0, 0.5, 0.25, 1e-2, 1e-4, 1e-9, 2.0 ** -64, 1e-30]


def test_pssm_and_threshold_against_the_reference():
    from genrich_amd.lib import motif_pssm, motif_threshold
    seen_unreachable = seen_big = 0
    for counts in _matrices():
        for pc in (1.0, 0.5, 4.0):
            want = R.pssm(counts, pc)
            s, lo, hi = motif_pssm(np.asarray(counts), pc)
            assert s.tolist() == want and (lo, hi) == R.score_range(want)
            L = len(want)
            for p in PVALUES + [4.0 ** -L, 4.0 ** -L * 0.99, 3 * 4.0 ** -L]:
                if not 0 < p <= 1:
                    continue
                t, smin, smax, n_ge, un = R.threshold(want, p)
                if L <= 8:
                    assert R.threshold_enumerated(want, p) == (t, smin, smax, n_ge, un), (counts, p)
                assert motif_threshold(s, p) == (t, smin, smax, R.p_achieved(n_ge, L), un), (counts, pc, p)
                assert n_ge <= p * 4 ** L and n_ge == R.n_ge(want, t)
                assert t == smin or R.n_ge(want, t - 1) > p * 4 ** L              # the LEAST such integer: one less lets too many in
                if p == 1.0:
                    assert t == smin and n_ge == 4 ** L                          # p = 1: every L-mer
                if p < 4.0 ** -L:
                    assert un and t == smax + 1 and n_ge == 0                    # fewer than one L-mer: unreachable
                seen_unreachable += un
                seen_big += n_ge >= 1 << 62
    assert seen_unreachable > 20 and seen_big > 3                                # (L = 32 at p = 1: 2^64 L-mers, beyond uint64)
    flat = R.pssm([[7] * 9] * 4)
    assert R.threshold(flat, 0.999) == (1, 0, 0, 0, True) and R.threshold(flat, 1.0)[:4] == (0, 0, 0, 4 ** 9)   # a tie cannot be split


def test_pssm_refusals():
    from genrich_amd.lib import motif_pssm
    for counts, pc, msg in (([[0], [1], [2], [3]], 0.0, "minus infinity"), ([[0], [0], [0], [0]], 0.0, "minus infinity"),
                            ([[1] * 33] * 4, 1.0, "1 <= L <= 32"), ([[1 << 31], [1], [1], [1]], 1.0, "count of 2.31"),
                            ([[1], [1], [1], [1]], -1.0, "pseudocount"), ([[1], [1], [1], [1]], float("nan"), "pseudocount"),
                            ([[0], [(1 << 31) - 1], [0], [0]], 1e-300, "int16")):
        with pytest.raises(ValueError, match=msg):
            motif_pssm(np.asarray(counts, dtype=np.uint32), pc)
        with pytest.raises(ValueError):
            R.pssm(counts, pc)
    s, lo, hi = motif_pssm(np.asarray([[0], [1], [2], [3]]), 1.0)                # the same counts with a pseudocount
    assert s.tolist() == R.pssm([[0], [1], [2], [3]], 1.0)


def test_the_geometry_and_the_constants():
    from genrich_amd.lib import GX_PATH_MOTIFS, MOTIF_DTYPE, MOTIF_HIT_DTYPE, MOTIF_MAX, MOTIF_MAX_WIDTH, MOTIF_SCALE, motif_geometry
    lanes, grid, positions, step, batch, list_cap, flush = motif_geometry()
    assert lanes == 256 and 1 <= grid <= 65535 and positions == 64 and 1 <= step <= 16 and 1 <= batch <= 64 and list_cap >= 1
    assert flush * positions < 1 << 32                                           # the 32-bit counters between two flushes
    assert batch * (4 * MOTIF_MAX_WIDTH * 4 + 8 + 12) <= 64 * 1024              # a batch's tables, records and counters fit the LDS
    assert (MOTIF_MAX_WIDTH, MOTIF_MAX, MOTIF_SCALE, GX_PATH_MOTIFS) == (R.MAX_WIDTH, R.MAX_MOTIFS, R.SCALE, 1 << 31)
    assert MOTIF_DTYPE.itemsize == 12 and MOTIF_HIT_DTYPE.itemsize == 16


def test_the_grid_keeps_a_workgroups_counters_below_2_32():
    """gx_motif_grid at the edge: a WORKGROUP's four wavefronts add to the same 32-bit LDS counters, at most 64 per run, so the
    grid that is accepted lets no workgroup walk more than 2^25 runs per batch; one workgroup fewer is refused."""
    from genrich_amd.lib import motif_geometry, motif_grid
    lanes, grid0, positions, step0, batch, list_cap, flush = motif_geometry()
    assert (lanes // 64, flush, grid0, step0) == (R.WAVES, R.FLUSH_RUNS, R.GRID, 4)
    hg38_twice = 2 * -(-(-(-3_088_286_401 // 64)) // 4)                           # units of the whole of hg38 listed twice, step 4
    cases = [(u, s) for s in (1, 2, 3, 4, 5, 16) for u in (0, 1, 4, 5, hg38_twice, (1 << 32) - 1)]
    for s in (1, 4, 16):                                                          # exactly what one, two and three workgroups may walk
        per_wg = R.FLUSH_RUNS // (s * R.WAVES) * R.WAVES
        cases += [(k * per_wg + d, s) for k in (1, 2, 3) for d in (-4, -1, 0, 1, 4, 5) if k * per_wg + d < 1 << 32]
    seen_refused = 0
    for units, step in cases:
        chosen = motif_grid(units, step, 0)
        assert chosen == R.grid_of(units, step, 0) and 1 <= chosen <= 65535, (units, step)
        assert R.runs_of_a_workgroup(units, step, chosen) * positions < 1 << 32, (units, step)
        need = 1
        while R.runs_of_a_workgroup(units, step, need) > R.FLUSH_RUNS:
            need += 1
        for g in {1, 2, 3, need - 1, need, need + 1, 2048, 65535} - {0}:
            got = motif_grid(units, step, g)
            assert got == R.grid_of(units, step, g) == (g if g >= need else None), (units, step, g)
            seen_refused += got is None
    assert seen_refused > 10
    assert motif_grid(hg38_twice, 4, 1) is None and motif_grid(hg38_twice, 0, 0) == 2048      # the review's case: one workgroup would wrap
    assert motif_grid(1 << 32, 4, 0) is None and motif_grid(10, 17, 0) is None and motif_grid(10, 4, 65536) is None and motif_grid(10, 0, 7) == 7


# ---- the writers ----------------------------------------------------------------------------------------------------------------

def _table_case(seed=3):
    """Peaks, motifs, hits and counts that agree with each other: a scan of a random genome by the reference."""
    rng = np.random.default_rng(seed)
    lens = [4000, 2500, 300]
    seqs = [bytes(np.frombuffer(b"ACGTacgtN", dtype=np.uint8)[rng.integers(0, 9, n)]) for n in lens]
    gen = R.genome(seqs, lens)
    golden = _golden()
    motifs, ids, names, pthr = [], [], [], []
    for (mid, name, counts), p in zip(golden, (0.25, 0.01, 0.01, 1e-3, 1e-4, 1e-9)):
        s = R.pssm(counts)
        t, smin, smax, n_ge, un = R.threshold(s, p)
        motifs.append((s, t))
        ids.append(mid)
        names.append(name.replace(" ", "_"))
        pthr.append(float("nan") if un else R.p_achieved(n_ge, len(s)))
    peaks = [(0, 100, 700), (0, 900, 905), (0, 3000, 4000), (1, 0, 2500), (2, 10, 300), (2, 20, 20)]
    summit = [300, 2, 0, 1234, 289, 0]
    hits, cp = R.scan(gen, peaks, motifs)
    cg = R.scan_genome(gen, motifs)
    return peaks, summit, motifs, ids, names, pthr, hits, cp, cg


def test_the_writers_against_the_reference():
    from genrich_amd.lib import MOTIF_HIT_DTYPE, REGION_DTYPE, format_motif_hits, format_motif_summary
    peaks, summit, motifs, ids, names, pthr, hits, cp, cg = _table_case()
    assert len(hits) > 100 and any(math.isnan(p) for p in pthr) and {h[4] for h in hits} == {0, 1}
    chroms = ["chrA", "chrB", "chrC"]
    reg = np.asarray(peaks, dtype=np.uint32).view(REGION_DTYPE).reshape(-1)
    h = np.zeros(len(hits), dtype=MOTIF_HIT_DTYPE)
    for k, f in enumerate(("region", "pos", "score", "motif", "strand")):
        h[f] = [x[k] for x in hits]
    text = format_motif_hits(chroms, reg, summit, motifs, ids, names, pthr, h).decode()
    assert text == R.hits_text(chroms, peaks, summit, motifs, ids, names, pthr, hits) and text.count("\n") == len(hits) + 1
    row = text.splitlines()[1].split("\t")
    assert len(row) == 10 and row[0] == "chrA" and int(row[2]) - int(row[1]) == len(motifs[ids.index(row[3])][0]) and row[5] in "+-" and row[7] == "peak_0"
    assert any(int(l.split("\t")[8]) < 0 for l in text.splitlines()[1:]) and any(int(l.split("\t")[8]) > 0 for l in text.splitlines()[1:])
    text = format_motif_summary(reg, motifs, ids, names, pthr, h, cp, cg).decode()
    assert text == R.summary_text(peaks, motifs, ids, names, pthr, hits, cp, cg)
    rows = [l.split("\t") for l in text.splitlines()[1:]]
    assert [r[0] for r in rows] == ids and rows[0][5] == "5" and rows[4][5] == "4" and "NA" in {r[4] for r in rows} and "NA" in {r[11] for r in rows}
    none = np.zeros(0, dtype=MOTIF_HIT_DTYPE)
    zero = [[0] * len(motifs)] * 3
    assert format_motif_summary(reg, motifs, ids, names, pthr, none, zero, zero).decode() == R.summary_text(peaks, motifs, ids, names, pthr, [], zero, zero)
    assert format_motif_hits(chroms, reg, summit, motifs, ids, names, pthr, none).decode().count("\n") == 1
    with pytest.raises(RuntimeError):                                            # a hit whose window leaves its peak
        bad = h[:1].copy()
        bad["region"], bad["pos"] = 1, 5
        format_motif_hits(chroms, reg, summit, motifs, ids, names, pthr, bad)


def test_format_standalone_under_sanitizers(tmp_path):
    """gx_emit.cpp's motif routines and writers in a program of its own (its own main, tests/motif_format_main.cpp), compiled with
    -fsanitize=address,undefined: any report makes the program fail (-fno-sanitize-recover, ASan aborts by default)."""
    exe = str(tmp_path / "motif_format")
    subprocess.check_call(SAN + [os.path.join(ROOT, "tests", "motif_format_main.cpp"), os.path.join(ROOT, "genrich_amd", "csrc", "gx_emit.cpp"), "-o", exe])
    lines, want = [], []
    for counts in _matrices() + [[[1] * 33] * 4, [[0], [1], [2], [3]]]:
        L = len(counts[0])
        for pc, p in ((1.0, 1e-4), (0.0, 1.0), (2.0, 4.0 ** -L), (1.0, 4.0 ** -L / 2)):
            lines.append("pssm %d %r %r" % (L, pc, p))
            lines += [" ".join(str(v) for v in row) for row in counts]
            try:
                s = R.pssm(counts, pc)
            except ValueError:
                want.append(None)
                continue
            t, smin, smax, n_ge, un = R.threshold(s, p)
            want.append(("scores " + " ".join(str(v) for row in s for v in row), (t, smin, smax, R.p_achieved(n_ge, L), int(un))))
    peaks, summit, motifs, ids, names, pthr, hits, cp, cg = _table_case()
    lines.append("tables %d %d %d" % (len(peaks), len(motifs), len(hits)))
    lines += ["%d %d %d %d" % (p + (s,)) for p, s in zip(peaks, summit)]
    lines += ["%s %s %d %d %r" % (i, n, len(m[0]), m[1], p) for i, n, m, p in zip(ids, names, motifs, pthr)]
    lines += ["%d %d %d %d %d" % x for x in hits]
    lines += [" ".join(str(v) for v in row) for row in cp + cg]
    chroms = ["chr0", "chr1", "chr2"]
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join(lines) + "\n")
    res = subprocess.run([exe, str(spec)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    _clean(res)
    parts = res.stdout.split("--\n")
    assert parts[-1] == "" and len(parts) == len(want) + 3
    refused = 0
    for got, w in zip(parts, want):
        if w is None:
            assert got.startswith("refused ") and len(got) > 12, got
            refused += 1
            continue
        a, b = got.splitlines()
        f = b.split()
        assert a == w[0] and f[0] == "threshold" and (int(f[1]), int(f[2]), int(f[3]), float(f[4]), int(f[5])) == w[1], (got, w)
    assert refused >= 8
    assert parts[-3] == R.hits_text(chroms, peaks, summit, motifs, ids, names, pthr, hits)
    assert parts[-2] == R.summary_text(peaks, motifs, ids, names, pthr, hits, cp, cg)


# ---- the reader -----------------------------------------------------------------------------------------------------------------

def _reader_text(motifs):
    return "".join("%s\t%s\t%d\t%s\n" % (i, n, len(c[0]), " ".join(str(v) for row in c for v in row)) for i, n, c in motifs)


def _good_files():
    data = open(GOLDEN, "rb").read()
    yield data
    yield data.replace(b"\n", b"\r\n")                                           # CRLF
    yield data[:-1]                                                              # no final newline
    yield b"\n\n" + data.replace(b"\n", b"\n\n") + b"\n"                          # blank lines
    yield data.replace(b" ", b"\t  ")                                             # any white space
    yield b">one\n1 2\n3 4\n5 6\n7 8"                                             # the raw form, no final newline
    yield b">x  a name with blanks \na[1]\nc[2]\ng[3]\nt[4]\n"                    # lower-case letters, brackets without blanks


def _bad_files():
    four = b"A [ 1 2 ]\nC [ 1 2 ]\nG [ 1 2 ]\nT [ 1 2 ]\n"
    yield b"", "no motif"
    yield b"\n \n", "no motif"
    yield b">m1\n" + four.replace(b"T [ 1 2 ]", b"T [ 1 2 3 ]"), "m1: rows of unequal length"
    yield b">m1\nA [ ]\nC [ ]\nG [ ]\nT [ ]\n", "m1: the width must be 1 to 32"
    yield b">m1\n" + b"".join(l + b" [ " + b"1 " * 33 + b"]\n" for l in (b"A", b"C", b"G", b"T")), "m1: the width must be 1 to 32"
    yield b">m1\n" + four.replace(b"G [ 1 2 ]", b"G [ 1 2.5 ]"), "m1: a count that is not an integer"
    yield b">m1\n" + four.replace(b"G [ 1 2 ]", b"G [ -1 2 ]"), "m1: a count that is not an integer"
    yield b">m1\n" + four.replace(b"G [ 1 2 ]", b"G [ 1 2147483648 ]"), "m1: a count that is not an integer"
    yield b">m1\n" + four.replace(b"G [ 1 2 ]", b"G [ 1 99999999999999999999999 ]"), "m1: a count that is not an integer"
    yield b">m1\n" + four + b">m2\n" + four + b">m1\n" + four, "m1: a repeated ID"
    yield b">m1\n" + four[:-10], "m1: fewer than four rows"
    yield b">m1\n" + four + b"1 2\n", "m1: more than four rows"
    yield b">m1\n" + four.replace(b"C [", b"G ["), "m1: rows out of the order A C G T"
    yield four, "a row before the first header"
    yield b">\n" + four, "a header without an ID"
    yield b"".join(b">m%d\n" % k + four for k in range(4097)), "m4096: more than 4096 motifs"


def test_the_reference_reader_on_good_and_damaged_files():
    want = _golden()
    for k, data in enumerate(_good_files()):
        got = R.read_jaspar(data)
        if k < 5:
            assert got == want, k
    assert R.read_jaspar(b">one\n1 2\n3 4\n5 6\n7 8") == [("one", "one", [[1, 2], [3, 4], [5, 6], [7, 8]])]
    assert R.read_jaspar(b">x  a name with blanks \na[1]\nc[2]\ng[3]\nt[4]\n") == [("x", "a name with blanks", [[1], [2], [3], [4]])]
    for data, msg in _bad_files():
        with pytest.raises(ValueError, match=msg.replace("[", r"\[")):
            R.read_jaspar(data)
    assert len(R.read_jaspar(b"".join(b">m%d\n1\n1\n1\n1\n" % k for k in range(4096)))) == 4096


def test_the_jaspar_reader_standalone_under_sanitizers(tmp_path):
    """genrich_amd/host/host_motifs.h behind a main of its own (tests/motif_reader_main.cpp): through the mapping and through the
    push parser in pieces of 1, 7 and 4096 bytes."""
    exe = str(tmp_path / "motif_reader")
    subprocess.check_call(SAN + [os.path.join(ROOT, "tests", "motif_reader_main.cpp"), "-o", exe])
    for i, data in enumerate(_good_files()):
        path = tmp_path / ("good%d.jaspar" % i)
        path.write_bytes(data)
        for piece in ([], ["1"], ["7"], ["4096"]):
            res = subprocess.run([exe, str(path)] + piece, capture_output=True, text=True)
            _clean(res)
            assert res.returncode == 0 and res.stdout == _reader_text(R.read_jaspar(data)), (i, piece, res.stderr)
    for i, (data, msg) in enumerate(_bad_files()):
        path = tmp_path / ("bad%d.jaspar" % i)
        path.write_bytes(data)
        for piece in ([], ["1"], ["4096"]):
            res = subprocess.run([exe, str(path)] + piece, capture_output=True, text=True)
            _clean(res)
            assert res.returncode == 1 and res.stdout == "" and msg in res.stderr, (i, piece, res.stderr)


# ---- the command line ---------------------------------------------------------------------------------------------------------

def test_cli_refusals_create_no_file(tmp_path):
    """Refused before any input is read: no GPU needed."""
    from genrich_amd import build

    binp = build.build_host()
    fa, sam, npk, hits, summ = (tmp_path / n for n in ("g.fa", "in.sam", "out.narrowPeak", "hits.tsv", "summary.tsv"))
    fa.write_text(">chr1\nACGT\n")
    sam.write_text("@HD\tVN:1.0\tSO:queryname\n@SQ\tSN:chr1\tLN:1000\n")
    base = [binp, "-t", str(sam), "-o", str(npk)]
    mo = ["--motifs", GOLDEN]
    for extra, msg in ((mo + ["--motif-hits", str(hits)], "--motifs needs the reference sequence (--genome FASTA)"),
                       (mo + ["--genome", str(fa)], "--motifs needs --motif-hits FILE or --motif-summary FILE"),
                       (["--genome", str(fa), "--motif-hits", str(hits)], "--motif-hits, --motif-summary, --motif-pvalue and --motif-pseudocount need --motifs FILE"),
                       (["--motif-pvalue", "0.01"], "--motif-hits, --motif-summary, --motif-pvalue and --motif-pseudocount need --motifs FILE"),
                       (mo + ["--genome", str(fa), "--motif-hits", str(hits), "-X"], "--motifs needs the peaks of this run on a device (not with -X, -P or --events-only)"),
                       (mo + ["--genome", str(fa), "--motif-summary", str(summ), "-P", "-f", str(tmp_path / "in.log")],
                        "--motifs needs the peaks of this run on a device (not with -X, -P or --events-only)"),
                       (mo + ["--genome", str(fa), "--motif-hits", str(hits), "--motif-pvalue", "0"], "--motif-pvalue takes a number in (0, 1]"),
                       (mo + ["--genome", str(fa), "--motif-hits", str(hits), "--motif-pvalue", "1.5"], "--motif-pvalue takes a number in (0, 1]"),
                       (mo + ["--genome", str(fa), "--motif-hits", str(hits), "--motif-pvalue", "1e-4x"], "--motif-pvalue takes a number in (0, 1]"),
                       (mo + ["--genome", str(fa), "--motif-hits", str(hits), "--motif-pseudocount", "-1"], "--motif-pseudocount takes a number >= 0"),
                       (["--genome", str(fa)], "--genome needs --gc-bias FILE or --gc-peaks FILE")):          # (the sentence from before the motifs)
        res = subprocess.run(base + extra, capture_output=True, text=True)
        assert res.returncode == 1 and msg in res.stderr, (extra, res.stderr)
    assert not hits.exists() and not summ.exists() and not npk.exists()


def test_cli_help_stays_and_help_motifs_names_the_options():
    from genrich_amd import build

    binp = build.build_host()
    res = subprocess.run([binp, "-h"], capture_output=True, text=True)
    assert res.returncode == 1 and res.stderr == open(os.path.join(ROOT, "tests", "host_usage.txt")).read()
    res = subprocess.run([binp, "--help-motifs"], capture_output=True, text=True)
    assert res.returncode == 1 and res.stdout == ""
    for opt in ("--motifs FILE", "--motif-hits FILE", "--motif-summary FILE", "--motif-pvalue P", "--motif-pseudocount X", "--genome FASTA"):
        assert opt in res.stderr, opt
