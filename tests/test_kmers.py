"""CPU-only checks of the k-mer feature: the reference by hand, gx_kmer_revcomp and the strand collapse for every k,
gx_kmer_stats and gx_format_kmers against tests/kmers_ref.py -- with a k-mer that is every window of the genome, k-mers the peaks
lack, ties in z, counts near 2^37 and --kmer-top 0, 1 and N --, the same host routines once more in a program of its own under the
sanitizers, the command line's refusals and --help-kmers, -h unchanged, the geometry and the constants."""
import os
import subprocess

import numpy as np
import pytest

import kmers_ref as R
import motifs_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


# ---- the reference by hand --------------------------------------------------------------------------------------------------

def test_the_reference_by_hand():
    gen = MR.genome([b"ACGTNACgt"], [9])
    # k = 2: the windows at 0 .. 7; those at 3 and 4 hold the N; the five counted are AC CG GT AC CG ... and GT at 7
    counts, windows, n_reg = R.count(gen, [(0, 0, 9)], 2)
    by_word = {R.word_of(2, c): v for c, v in enumerate(counts) if v}
    assert by_word == {"AC": 2, "CG": 2, "GT": 2} and windows == 6 and n_reg == 1
    # the issue's five: the region that ends before the last GT
    counts, windows, n_reg = R.count(gen, [(0, 0, 8)], 2)
    assert {R.word_of(2, c): v for c, v in enumerate(counts) if v} == {"AC": 2, "CG": 2, "GT": 1} and windows == 5
    # the collapse: GT is AC's reverse complement and AC < GT names the pair; CG is a palindrome and counts once
    assert R.revcomp(2, R.code_of("AC")) == R.code_of("GT") and R.revcomp(2, R.code_of("CG")) == R.code_of("CG")
    col = R.collapse(2, counts)
    assert {R.word_of(2, c): v for c, v in col.items() if v} == {"AC": 3, "CG": 2} and len(col) == 10      # 6 pairs and 4 palindromes
    assert R.code_of("A") == 0 and R.code_of("T") == 3 and R.code_of("AC") == 1 and R.code_of("CA") == 4 and R.code_of("TTT") == 63
    # regions: shorter than k counts nothing and is not a counted region; overlapping regions count twice; past the end clamps
    assert R.count(gen, [(0, 0, 1)], 2)[1:] == (0, 0) and not R.count(gen, [(0, 0, 1)], 2)[0].any()
    assert R.count(gen, [(0, 5, 9), (0, 5, 9), (0, 7, 30), (1, 0, 5), (0, 6, 2)], 2)[1:] == (3 + 3 + 1, 3)
    # the flank: the summit's base and N to either side, inside the peak
    assert R.flank_regions([(0, 100, 200), (1, 5, 9)], [0, 3], 10) == [(0, 100, 111), (1, 5, 9)]
    assert R.flank_regions([(0, 100, 200)], [50], 0) == [(0, 150, 151)] and R.flank_regions([(0, 100, 200)], [50], -1) == [(0, 100, 200)]
    # the figures: cp 3 of 5 windows against cg 30 of 1000: enrichment 20, z = (3 * 1000 - 30 * 5) / sqrt(5 * 30 * 970)
    cp, cg = [0] * 16, [0] * 16
    cp[R.code_of("AC")], cp[R.code_of("GT")], cp[R.code_of("CG")] = 2, 1, 2
    cg[R.code_of("AC")], cg[R.code_of("GT")], cg[R.code_of("CG")], cg[R.code_of("TT")] = 10, 20, 100, 870
    rows = R.stats(2, cp, 5, cg, 1000)
    assert [(R.word_of(2, r[0]), R.word_of(2, r[1]), r[2], r[3]) for r in rows] == [("AC", "GT", 3, 30), ("CG", "CG", 2, 100)]
    assert rows[0][4] == 20.0 and abs(rows[0][5] - 2850 / (5 * 30 * 970) ** 0.5) < 1e-12
    assert R.text(2, 25, 1, 5, 1000, cp, cg) == ("# k=2 flank=25 regions=1 windows_peaks=5 windows_genome=1000 kmers=2\n"
                                                  "kmer\trevcomp\tcount_peaks\tcount_genome\tenrichment\tz\n"
                                                  "AC\tGT\t3\t30\t20.000000\t7.4716\nCG\tCG\t2\t100\t4.000000\t2.2361\n")


# ---- the collapse -----------------------------------------------------------------------------------------------------------

def test_revcomp_and_the_collapse_for_every_k():
    from genrich_amd.lib import KMER_MAX_K, kmer_revcomp
    rng = np.random.default_rng(3)
    for k in range(1, KMER_MAX_K + 1):
        n = 4 ** k
        codes = list(range(n)) if k <= 6 else [0, 1, n - 1, n - 2] + rng.integers(0, n, 300).tolist()
        pal = 0
        for c in codes:
            rc = kmer_revcomp(k, c)
            assert rc == R.revcomp(k, c) and kmer_revcomp(k, rc) == c, (k, c)
            pal += rc == c
        assert kmer_revcomp(k, n) is None and kmer_revcomp(k, 0) == n - 1                   # AAA.. <-> TTT..
        if k <= 6:
            assert pal == (4 ** (k // 2) if k % 2 == 0 else 0)                               # palindromes only for even k
            assert len(R.collapse(k, [1] * n)) == (n + pal) // 2
    assert kmer_revcomp(0, 0) is None and kmer_revcomp(13, 0) is None


# ---- the figures and the table --------------------------------------------------------------------------------------------------

def _cases():
    """(k, flank, regions, cp, wp, cg, wg): random tables; one k-mer that is every window of the genome (z NA); k-mers the peaks
    lack (no row) and the genome lacks (enrichment and z NA); exact ties in z; counts near 2^37."""
    rng = np.random.default_rng(19)
    out = []
    for k in (1, 2, 3, 5, 8):
        n = 4 ** k
        cg = rng.integers(0, 5000, n)
        cp = np.minimum(rng.integers(0, 40, n) * (rng.random(n) < 0.7), cg)
        cp[:4] = 0                                                                            # cp == 0: no row
        out.append((k, -1, 17, cp.tolist(), int(cp.sum()), cg.tolist(), int(cg.sum())))
    # k = 2, ties: AA|TT and CC|GG have the same counts, so the same z and the same count_peaks: the code decides
    cp, cg = [0] * 16, [0] * 16
    for w, a, b in (("AA", 5, 100), ("TT", 2, 40), ("CC", 4, 70), ("GG", 3, 70), ("AT", 9, 500), ("CA", 1, 0), ("AC", 4, 300)):
        cp[R.code_of(w)], cg[R.code_of(w)] = a, b
    out.append((2, 0, 3, cp, sum(cp), cg, sum(cg)))
    # one k-mer is every window of the genome: cg == Wg, z NA, the enrichment stays
    cp, cg = [0] * 4, [0] * 4
    cp[0], cg[0] = 7, 1234
    out.append((1, 10, 1, cp, 7, cg, 1234))
    # counts near 2^37 (hg38 listed many times over): the products pass 2^64, the radicand 2^128
    big = 1 << 37
    cp, cg = [0] * 64, [0] * 64
    for i, w in enumerate(("AAA", "ACG", "CGT", "GGG", "TTT", "TAT", "ATA")):
        cp[R.code_of(w)] = big - 12345 * i
        cg[R.code_of(w)] = 3 * big + 977 * i * i
    cg[R.code_of("CCC")] = 5 * big
    out.append((3, -1, 1 << 20, cp, sum(cp), cg, sum(cg)))
    out.append((3, -1, 0, [0] * 64, 0, cg, sum(cg)))                                           # no peak at all: only the two header lines
    return out


def test_stats_and_the_table_against_the_reference():
    from genrich_amd.lib import format_kmers, kmer_stats
    seen_na_z = seen_na_enr = seen_tie = 0
    for k, flank, n_reg, cp, wp, cg, wg in _cases():
        want = R.stats(k, cp, wp, cg, wg)
        got = kmer_stats(k, cp, wp, cg, wg)
        assert [(int(r["code"]), int(r["revcomp"]), int(r["count_peaks"]), int(r["count_genome"])) for r in got] == [r[:4] for r in want]
        for r, w in zip(got, want):
            assert (None if np.isnan(r["enrichment"]) else float(r["enrichment"])) == w[4] and (None if np.isnan(r["z"]) else float(r["z"])) == w[5], (k, w)
        assert all(w[2] > 0 for w in want) and len(want) == sum(1 for v in R.collapse(k, cp).values() if v)
        seen_na_z += sum(w[5] is None and w[4] is not None for w in want)
        seen_na_enr += sum(w[4] is None for w in want)
        seen_tie += sum(a[5] is not None and a[5] == b[5] for a, b in zip(want, want[1:]))
        for top in (0, 1, 3, 100, 1 << 24):
            text = format_kmers(k, flank, n_reg, wp, wg, cp, cg, top).decode()
            assert text == R.text(k, flank, n_reg, wp, wg, cp, cg, top), (k, top)
            assert text.count("\n") == 2 + (min(top, len(want)) if top else len(want))
    assert seen_na_z >= 1 and seen_na_enr >= 1 and seen_tie >= 1
    # the ties' order: the same z and count_peaks, the smaller code first
    rows = R.stats(*[_cases()[5][i] for i in (0, 3, 4, 5, 6)])
    words = [R.word_of(2, r[0]) for r in rows]
    assert words.index("AA") + 1 == words.index("CC") and rows[words.index("AA")][5] == rows[words.index("CC")][5] and words[-1] == "CA"
    with pytest.raises(RuntimeError):                                                        # a canonical count above its windows
        kmer_stats(1, [5, 0, 0, 0], 4, [9, 0, 0, 0], 9)
    with pytest.raises(ValueError):
        kmer_stats(2, [0] * 4, 0, [0] * 4, 0)


def test_format_standalone_under_sanitizers(tmp_path):
    """gx_emit.cpp's k-mer routines in a program of its own (its own main, tests/kmer_format_main.cpp), compiled with
    -fsanitize=address,undefined: any report makes the program fail (-fno-sanitize-recover, ASan aborts by default)."""
    exe = str(tmp_path / "kmer_format")
    subprocess.check_call(SAN + [os.path.join(ROOT, "tests", "kmer_format_main.cpp"), os.path.join(ROOT, "genrich_amd", "csrc", "gx_emit.cpp"), "-o", exe])
    lines, want = [], []
    for k in (1, 2, 7, 12, 0, 13):
        n = 4 ** max(k, 1)
        codes = [0, 1, n // 3, n - 1, n]
        lines.append("revcomp %d %d %s" % (k, len(codes), " ".join(map(str, codes))))
        want.append(" ".join(str(R.revcomp(k, c) if 1 <= k <= 12 and c < n else 0xffffffff) for c in codes) + "\n")
    for k, flank, n_reg, cp, wp, cg, wg in _cases():
        for top in (0, 1, 5):
            sp, sg = [(c, v) for c, v in enumerate(cp) if v], [(c, v) for c, v in enumerate(cg) if v]
            lines.append("table %d %d %d %d %d %d %d %d" % (k, flank, n_reg, wp, wg, top, len(sp), len(sg)))
            lines += ["%d %d" % x for x in sp + sg]
            want.append(R.text(k, flank, n_reg, wp, wg, cp, cg, top))
    lines += ["table 1 -1 1 4 9 0 1 1", "0 5", "0 9"]                                       # refused: 5 counted in 4 windows
    want.append("refused -10\n")
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join(lines) + "\n")
    res = subprocess.run([exe, str(spec)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
    parts = res.stdout.split("--\n")
    assert parts[-1] == "" and parts[:-1] == want


# ---- the geometry and the constants -------------------------------------------------------------------------------------------

def test_the_geometry_and_the_constants():
    from genrich_amd.lib import GX_PATH_KMERS, KMER_LDS_MAX_K, KMER_MAX_K, KMER_ROW_DTYPE, kmer_geometry, motif_geometry
    lanes, grid, positions, step, flush, max_k, lds_max_k = kmer_geometry()
    assert (max_k, lds_max_k) == (KMER_MAX_K, KMER_LDS_MAX_K) == (R.MAX_K, R.LDS_MAX_K) == (12, 7) and GX_PATH_KMERS == 1 << 12
    assert (lanes, grid, positions, step, flush) == motif_geometry()[:4] + (motif_geometry()[6],)       # the motif scan's front end
    assert flush == 1 << 25 and flush * positions < 1 << 32                                   # the 32-bit counters between two flushes
    assert 4 * 4 ** lds_max_k <= 64 * 1024 < 4 * 4 ** (lds_max_k + 1)                        # the LDS path's counters fit 64 KiB, one k more does not
    assert 8 * 4 ** max_k == 128 << 20 and KMER_ROW_DTYPE.itemsize == 40
    import genrich_amd.lib as L
    bits = [v for n, v in vars(L).items() if n.startswith("GX_PATH_")]
    assert len(bits) == len(set(bits)) and all(v & (v - 1) == 0 for v in bits)               # bit 12 was the one unassigned


# ---- the command line ---------------------------------------------------------------------------------------------------------

def test_cli_refusals_create_no_file(tmp_path):
    """Refused before any input is read: no GPU needed."""
    from genrich_amd import build

    binp = build.build_host()
    fa, sam, npk, out = (tmp_path / n for n in ("g.fa", "in.sam", "out.narrowPeak", "kmers.tsv"))
    fa.write_text(">chr1\nACGT\n")
    sam.write_text("@HD\tVN:1.0\tSO:queryname\n@SQ\tSN:chr1\tLN:1000\n")
    base = [binp, "-t", str(sam), "-o", str(npk)]
    km = ["--kmers", str(out)]
    ge = ["--genome", str(fa)]
    for extra, msg in ((km, "--kmers needs the reference sequence (--genome FASTA)"),
                       (ge + ["--kmer-k", "6"], "--kmer-k, --kmer-flank and --kmer-top need --kmers FILE"),
                       (["--kmer-flank", "6"], "--kmer-k, --kmer-flank and --kmer-top need --kmers FILE"),
                       (["--kmer-top", "6"], "--kmer-k, --kmer-flank and --kmer-top need --kmers FILE"),
                       (km + ge + ["-X"], "--kmers needs the peaks of this run on a device (not with -X, -P or --events-only)"),
                       (km + ge + ["-P", "-f", str(tmp_path / "in.log")], "--kmers needs the peaks of this run on a device (not with -X, -P or --events-only)"),
                       (km + ge + ["--events-only"], "--kmers needs the peaks of this run on a device (not with -X, -P or --events-only)"),
                       (km + ge + ["--kmer-k", "0"], "--kmer-k takes an integer in [1, 12]"),
                       (km + ge + ["--kmer-k", "13"], "--kmer-k takes an integer in [1, 12]"),
                       (km + ge + ["--kmer-k", "8x"], "--kmer-k takes an integer in [1, 12]"),
                       (km + ge + ["--kmer-flank", "-1"], "--kmer-flank takes an integer in [0, 1000000000]"),
                       (km + ge + ["--kmer-top", "-3"], "--kmer-top takes an integer in [0, 16777216] (0: all)"),
                       (ge, "--genome needs --gc-bias FILE or --gc-peaks FILE")):             # (the sentence from before the k-mers)
        res = subprocess.run(base + extra, capture_output=True, text=True)
        assert res.returncode == 1 and msg in res.stderr, (extra, res.stderr)
    assert not out.exists() and not npk.exists()


def test_cli_help_stays_and_help_kmers_names_the_options():
    from genrich_amd import build

    binp = build.build_host()
    res = subprocess.run([binp, "-h"], capture_output=True, text=True)
    assert res.returncode == 1 and res.stderr == open(os.path.join(ROOT, "tests", "host_usage.txt")).read()
    res = subprocess.run([binp, "--help-kmers"], capture_output=True, text=True)
    assert res.returncode == 1 and res.stdout == ""
    for opt in ("--kmers FILE", "--kmer-k K", "--kmer-flank N", "--kmer-top N", "--genome FASTA", "p-value"):
        assert opt in res.stderr, opt
