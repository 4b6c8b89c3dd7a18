"""GC bias and GC content without a GPU: tests/gcbias_ref.py on hand-computed cases; the class fold at its exact ties;
gx_gc_metrics and the two writers through ctypes against the reference, byte for byte, `NA` rows included; the same writers as
a stand-alone program under AddressSanitizer / UBSan; the FASTA reader (genrich_amd/host/host_genome.h) as another, on files
written here.

What is compared how.  Every integer with ==.  A ratio is made of two exact integers, each converted once by the rule both
sides define alike (the leading 64 bits, rounded by the conversion, scaled), and one division: == against the reference, and
the texts byte for byte."""
import math
import os
import subprocess

import numpy as np
import pytest

import gcbias_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EV = np.dtype([("chrom", "<u4"), ("start", "<u4"), ("end", "<u4"), ("count", "<u4")])


def _ev(rows):
    ev = np.zeros(len(rows), dtype=EV)
    for i, r in enumerate(rows):
        ev[i] = r
    return ev


def test_the_reference_by_hand():
    #            0123456789
    gen = R.genome([b"ACGTNacgtR", b"GG", None], [10, 3, 4])
    gc, ac = gen[0]
    assert [int(x) for x in gc] == [0, 1, 1, 0, 0, 0, 1, 1, 0, 0] and [int(x) for x in ac] == [1, 1, 1, 1, 0, 1, 1, 1, 1, 0]
    assert [int(x) for x in gen[1][1]] == [1, 1, 0]                                   # a base never pushed is unknown
    assert R.content(gen, [(0, 0, 10), (0, 1, 3), (0, 3, 3), (0, 5, 2), (0, 8, 99), (1, 0, 3), (2, 0, 4), (3, 0, 1)]) == [
        (4, 8), (2, 2), (0, 0), (0, 0), (0, 1), (2, 2), (0, 0), (0, 0)]
    # W = 2 on chromosome 0: windows at 0..9: AC CG GT T? ?a ac cg gt t? ?-  -> classes 1 2 1 - - 1 2 1 - -
    F, un = R.expected(gen, 2, [1, 0, 0])
    assert F == [0, 4, 2] and un == 4
    F, un = R.expected(gen, 2)
    assert F == [0, 4, 3] and un == 4 + 2 + 4                                         # GG is classed 2; G? and the empty chromosome are not
    assert R.expected(gen, 1) == ([4, 6], 2 + 1 + 4)
    assert R.expected(gen, 11) == ([0] * 12, 17)                                      # wider than every chromosome
    ev = _ev([(0, 0, 5, 1), (0, 1, 1, 2), (0, 1, 0, 3), (0, 3, 9, 1), (0, 9, 12, 1), (1, 0, 2, 10), (1, 1, 3, 1), (2, 0, 1, 1),
              (0, 10, 12, 1), (0, 1, 2, 7), (3, 0, 1, 1), (1, 0, 2, 0)])              # the last four: no intervals of a sample
    t = R.tables(gen, ev, 2)
    assert (t.Nn, t.Nw, t.n_unclassed, t.w_unclassed) == ([0, 1, 3], [0, 120, 60 + 40 + 12], 4, 480)
    t = R.tables(gen, ev, 2, [1, 0, 1])
    assert (t.F, t.f_unclassed, t.Nn, t.Nw, t.n_unclassed, t.w_unclassed) == ([0, 4, 2], 8, [0, 1, 2], [0, 120, 100], 3, 360)


def test_the_class_fold_at_exact_ties():
    from genrich_amd.lib import gc_class
    assert (R.gc_class(200, 0), R.gc_class(200, 1), R.gc_class(200, 2), R.gc_class(200, 3), R.gc_class(200, 199), R.gc_class(200, 200)) == (0, 1, 1, 2, 100, 100)
    assert (R.gc_class(1, 0), R.gc_class(1, 1)) == (0, 100)
    assert (R.gc_class(4096, 0), R.gc_class(4096, 20), R.gc_class(4096, 21), R.gc_class(4096, 2048), R.gc_class(4096, 4075), R.gc_class(4096, 4076),
            R.gc_class(4096, 4096)) == (0, 0, 1, 50, 99, 100, 100)
    assert (R.gc_class(8, 1), R.gc_class(8, 3), R.gc_class(8, 5)) == (13, 38, 63)            # 12.5, 37.5, 62.5: halves up
    for W in (1, 2, 3, 7, 8, 63, 64, 65, 200, 1000, 4095, 4096):
        for g in range(W + 1):
            k = gc_class(W, g)
            assert k == R.gc_class(W, g) and 0 <= k <= 100 and abs(200 * g - 2 * W * k) <= W
    assert gc_class(0, 0) == gc_class(4097, 0) == gc_class(5, 6) == gc_class(5, -1) == -1


def _random_tables(rng, W, empty_classes=False, no_intervals=False, big=False):
    F = rng.integers(0, 1 << (40 if big else 20), W + 1)
    Nn = rng.integers(0, 1 << (30 if big else 12), W + 1)
    if empty_classes:
        F[rng.random(W + 1) < 0.5] = 0
        Nn[rng.random(W + 1) < 0.3] = 0
    if no_intervals:
        Nn[:] = 0
    cnt = rng.choice(R.VALID_COUNTS, W + 1)
    Nw = np.where(Nn > 0, (Nn - 1) * 120 + 120 // cnt, 0)
    return R.Tables(W, [int(x) for x in F], int(rng.integers(0, 1000)), [int(x) for x in Nn], [int(x) for x in Nw], int(rng.integers(0, 50)),
                    int(rng.integers(0, 50)) * 60)


def _cases():
    rng = np.random.default_rng(11)
    hand = R.tables(R.genome([b"ACGTNacgtR", b"GG", None], [10, 3, 4]), _ev([(0, 0, 5, 1), (0, 1, 1, 2), (0, 3, 9, 1), (1, 0, 2, 10)]), 2)
    return [[(0, False, hand)],
            [(0, False, _random_tables(rng, 200)), (0, True, _random_tables(rng, 200, empty_classes=True)), (1, False, _random_tables(rng, 200, no_intervals=True))],
            [(0, False, _random_tables(rng, 1, empty_classes=True))],
            [(3, False, _random_tables(rng, 4096, big=True)), (3, True, _random_tables(rng, 4096, empty_classes=True, big=True))],
            [(0, False, R.Tables(7, [0] * 8, 99, [0] * 8, [0] * 8, 0, 0))]]


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def test_metrics_against_the_reference():
    from genrich_amd.lib import GcBias, gc_metrics
    seen_na = seen_ratio = 0
    for samples in _cases():
        for rep, ctrl, t in samples:
            got, exp = gc_metrics(GcBias(*t)), R.metrics(t)
            for k in ("windows", "windows_unclassed", "intervals", "intervals_unclassed", "w120", "w120_unclassed", "ratio_min_class", "ratio_max_class"):
                assert int(got[k]) == exp[k], k
            for k in ("cls_windows", "cls_intervals", "cls_w120"):
                assert [int(x) for x in got[k]] == exp[k], k
            assert all(_same(float(g), e) for g, e in zip(got["ratio"], exp["ratio"]))
            for k in ("mean_gc_genome", "mean_gc_sample", "ratio_min", "ratio_max"):
                assert _same(float(got[k]), exp[k]), (k, got[k], exp[k])
            seen_na += sum(math.isnan(x) for x in exp["ratio"])
            seen_ratio += sum(not math.isnan(x) for x in exp["ratio"])
    assert seen_na > 100 and seen_ratio > 100
    m = R.metrics(_cases()[0][0][2])                                     # by hand: F = [0, 4, 3], Nw = [0, 120, 60 + 12] at W = 2
    assert m["cls_windows"][50] == 4 and m["cls_windows"][100] == 3 and m["ratio"][50] == (120 * 7) / (4 * 192) and m["ratio"][100] == (72 * 7) / (3 * 192)
    assert math.isnan(m["ratio"][0]) and m["mean_gc_genome"] == 10 / 14 and (m["ratio_min_class"], m["ratio_max_class"]) == (100, 50)


def _peak_case():
    names = ["chr%d" % i for i in range(10)]
    regions = [(0, 10, 20), (0, 100, 350), (3, 0, 1), (9, 5, 5), (2, 1000, 5096)]
    counts = [(5, 10), (0, 0), (1, 1), (0, 0), (1365, 4095)]
    return names, regions, counts


def test_the_writers_against_the_reference():
    from genrich_amd.lib import REGION_DTYPE, GcBias, format_gc_bias, format_gc_peaks
    for samples in _cases():
        text = format_gc_bias([GcBias(*t, rep, ctrl) for rep, ctrl, t in samples]).decode()
        assert text == R.bias_text(samples)
    assert "\tNA\n" in R.bias_text(_cases()[1]) and "# c0\tW=200\t" in R.bias_text(_cases()[1])
    names, regions, counts = _peak_case()
    reg = np.asarray(regions, dtype=np.uint32).view(REGION_DTYPE).reshape(-1)
    text = format_gc_peaks(names, reg, [g for g, a in counts], [a for g, a in counts]).decode()
    assert text == R.peaks_text(names, regions, counts)
    assert "chr0\t10\t20\tpeak_0\t10\t10\t5\t0.500000\n" in text and "chr0\t100\t350\tpeak_1\t250\t0\t0\tNA\n" in text
    with pytest.raises(RuntimeError):
        format_gc_peaks(names, reg[:1], [11], [10])


SAN = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def _clean(res):
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr


def test_format_standalone_under_sanitizers(tmp_path):
    """gx_emit.cpp's GC figures and writers in a program of its own (its own main, tests/gcbias_format_main.cpp), compiled with
    -fsanitize=address,undefined: any report makes the program fail (-fno-sanitize-recover, ASan aborts by default)."""
    exe = str(tmp_path / "gcbias_format")
    subprocess.check_call(SAN + [os.path.join(ROOT, "tests", "gcbias_format_main.cpp"), os.path.join(ROOT, "genrich_amd", "csrc", "gx_emit.cpp"), "-o", exe])
    lines, want = [], []
    for samples in _cases():
        lines.append("bias %d %d" % (len(samples), samples[0][2].window))
        for rep, ctrl, t in samples:
            lines.append("%d %d %d %d %d" % (rep, int(ctrl), t.f_unclassed, t.n_unclassed, t.w_unclassed))
            lines += [" ".join(str(int(x)) for x in col) for col in (t.F, t.Nn, t.Nw)]
        want.append(R.bias_text(samples))
    names, regions, counts = _peak_case()
    lines.append("peaks %d" % len(regions))
    lines += ["%d %d %d %d %d" % (r + c) for r, c in zip(regions, counts)]
    want.append(R.peaks_text(names, regions, counts))
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join(lines) + "\n")
    res = subprocess.run([exe, str(spec)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    _clean(res)
    parts = res.stdout.split("--\n")
    assert parts[-1] == "" and parts[:-1] == want


def _fasta_cases():
    """(file bytes, [(name, stripped bases)]) per case."""
    rng = np.random.default_rng(23)
    alphabet = np.frombuffer(b"ACGTacgtNnRYKMSWBDHVrykm", dtype=np.uint8)
    seq = lambda n: bytes(alphabet[rng.integers(0, len(alphabet), n)])
    wrap = lambda s, w, nl=b"\n": b"".join(s[i:i + w] + nl for i in range(0, len(s), w))
    out = []
    for w in (1, 60, 61):
        a, b = seq(1000), seq(123)
        out.append((b">a\n" + wrap(a, w) + b">b\n" + wrap(b, w), [("a", a), ("b", b)]))
    a, b = seq(300), seq(61)
    out.append((b">a\r\n" + wrap(a, 60, b"\r\n") + b">b\r\n" + wrap(b, 60, b"\r\n"), [("a", a), ("b", b)]))            # CRLF
    out.append((b"\n\n>a\n\n" + wrap(a, 50) + b"\n\n>b\n" + wrap(b, 7, b"\n\n"), [("a", a), ("b", b)]))                  # empty lines
    out.append((b">a\n" + wrap(a, 60) + b">b\n" + wrap(b, 60)[:-1], [("a", a), ("b", b)]))                             # no final newline
    low = bytes(np.frombuffer(b"acgtnryswkm", dtype=np.uint8)[rng.integers(0, 11, 500)])
    out.append((b">low\n" + wrap(low, 70), [("low", low)]))                                                            # lower case and IUPAC
    out.append((b">chr1 Homo sapiens chromosome 1\n" + wrap(a, 60) + b">chr2\tdesc\n" + wrap(b, 60), [("chr1", a), ("chr2", b)]))
    out.append((b">e1\n>x\n" + wrap(b, 60) + b">e2\n\n>e3", [("e1", b""), ("x", b), ("e2", b""), ("e3", b"")]))          # empty sequences
    s64, s65, s128 = seq(64), seq(65), seq(128)
    out.append((b">s64\n" + wrap(s64, 64) + b">s65\n" + wrap(s65, 64) + b">s128\n" + wrap(s128, 128), [("s64", s64), ("s65", s65), ("s128", s128)]))
    out.append((b">sp\nAC GT\tac\n", [("sp", b"ACGTac")]))                                                             # blanks inside a line
    return out


def _fnv(b):
    h = 1469598103934665603
    for c in b:
        h = ((h ^ c) * 1099511628211) & ((1 << 64) - 1)
    return h


def _reader_line(name, s):
    gc, ac = R.pack(s, len(s))
    return "%s %d %d %d %016x\n" % (name, len(s), int(gc.sum()), int(ac.sum()), _fnv(s))


def test_the_fasta_reader_standalone_under_sanitizers(tmp_path):
    """genrich_amd/host/host_genome.h behind a main of its own (tests/genome_reader_main.cpp): per sequence the length, gc, acgt and
    a checksum of the stripped bases, at a staging buffer of 64 bases (many calls per sequence) and of 1 MiB."""
    exe = str(tmp_path / "genome_reader")
    subprocess.check_call(SAN + [os.path.join(ROOT, "tests", "genome_reader_main.cpp"), "-o", exe])
    for i, (data, seqs) in enumerate(_fasta_cases()):
        path = tmp_path / ("case%d.fa" % i)
        path.write_bytes(data)
        for chunk in ("64", "1048576"):
            res = subprocess.run([exe, str(path), chunk], capture_output=True, text=True)
            assert res.returncode == 0, (i, chunk, res.returncode, res.stderr)
            _clean(res)
            assert res.stdout == "".join(_reader_line(n, s) for n, s in seqs), (i, chunk)
        res = subprocess.run([exe, str(path), "64", seqs[0][0]], capture_output=True, text=True)       # the first sequence skipped
        assert res.returncode == 0 and res.stdout == "".join(_reader_line(n, s) for n, s in seqs[1:]), (i, res.stderr)
        _clean(res)
    for name, data, msg in (("text.fa", b"ACGT\n>a\nAC\n", "text before the first '>' line"), ("z.fa.gz", b"\x1f\x8b\x08\x00rest", "is gzip-compressed")):
        (tmp_path / name).write_bytes(data)
        res = subprocess.run([exe, str(tmp_path / name), "64"], capture_output=True, text=True)
        assert res.returncode == 1 and msg in res.stderr, res.stderr
        _clean(res)
    res = subprocess.run([exe, str(tmp_path / "missing.fa"), "64"], capture_output=True, text=True)
    assert res.returncode == 1 and "cannot read" in res.stderr
    (tmp_path / "empty.fa").write_bytes(b"")
    res = subprocess.run([exe, str(tmp_path / "empty.fa"), "64"], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout == ""


def test_the_geometry_call():
    from genrich_amd.lib import GC_MAX_WINDOW, GC_MIN_TILE, GX_PATH_GC, gc_geometry
    lanes, grid, tile, min_tile, pad, block, flush = gc_geometry()
    assert lanes == 256 and 1 <= grid <= 65535 and tile % 64 == 0 and GC_MIN_TILE == min_tile == 64 <= tile <= 1024
    assert pad == GC_MAX_WINDOW // 64 + 1 and block == 512 and flush == 1 << 25 and flush * 64 < 1 << 32
    assert GX_PATH_GC == 1 << 30


# ---- the command line ------------------------------------------------------------------------------------------------------

def test_cli_refusals_create_no_file(tmp_path):
    """Refused before any input is read: no GPU needed."""
    from genrich_amd import build

    binp = build.build_host()
    sam, fa = tmp_path / "t.sam", tmp_path / "g.fa"
    sam.write_text("@SQ\tSN:chrA\tLN:1000\n")
    fa.write_text(">chrA\nACGT\n")
    bias, peaks, npk, ev = tmp_path / "gc.tsv", tmp_path / "gcp.tsv", tmp_path / "o.np", tmp_path / "ev.bed"
    base = [binp, "-o", str(npk), "-t", str(sam)]
    for extra, msg in ((["--gc-bias", str(bias)], "--gc-bias needs the reference sequence (--genome FASTA)"),
                       (["--gc-peaks", str(peaks)], "--gc-peaks needs the reference sequence (--genome FASTA)"),
                       (["--genome", str(fa), "--gc-window", "100", "--gc-peaks", str(peaks)], "--gc-window needs --gc-bias FILE"),
                       (["--genome", str(fa)], "--genome needs --gc-bias FILE or --gc-peaks FILE"),
                       (["--genome", str(fa), "--gc-bias", str(bias), "--events-only", "-b", str(ev)], "--gc-bias needs the intervals of this run (not with -P or --events-only)"),
                       (["--genome", str(fa), "--gc-bias", str(bias), "-P", "-f", str(tmp_path / "in.log")], "--gc-bias needs the intervals of this run (not with -P or --events-only)"),
                       (["--genome", str(fa), "--gc-peaks", str(peaks), "-X"], "--gc-peaks needs the peaks of this run on a device (not with -X, -P or --events-only)"),
                       (["--genome", str(fa), "--gc-peaks", str(peaks), "-P", "-f", str(tmp_path / "in.log")], "--gc-peaks needs the peaks of this run on a device")):
        res = subprocess.run(base + extra, capture_output=True, text=True)
        assert res.returncode == 1 and msg in res.stderr, (extra, res.stderr)
    for w in ("0", "4097", "-5", "200bp", "x", "", "1.5"):
        res = subprocess.run(base + ["--genome", str(fa), "--gc-bias", str(bias), "--gc-window", w], capture_output=True, text=True)
        assert res.returncode == 1 and "--gc-window takes an integer in [1, 4096]" in res.stderr, (w, res.stderr)
    assert not bias.exists() and not peaks.exists() and not npk.exists() and not ev.exists()


def test_cli_help_stays_and_help_gc_names_the_options():
    from genrich_amd import build

    binp = build.build_host()
    res = subprocess.run([binp, "-h"], capture_output=True, text=True)
    assert res.stderr == open(os.path.join(ROOT, "tests", "host_usage.txt")).read() and "--gc-bias" not in res.stderr
    res = subprocess.run([binp, "--help-gc"], capture_output=True, text=True)
    assert res.returncode == 1 and res.stdout == ""
    for word in ("--genome FASTA", "--gc-bias FILE [--gc-window W]", "--gc-peaks FILE", "(200; 1 .. 4096)", "NOT masked", "not with -P or --events-only", "Benjamini & Speed"):
        assert word in res.stderr, word
