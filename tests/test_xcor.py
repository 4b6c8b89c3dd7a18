"""The strand cross-correlation's reference, figures and text writers without a GPU: gx_xcor_metrics / gx_xcor_r through ctypes
against tests/xcor_ref.py and hand-computed cases; the two writers byte for byte, once more as a stand-alone program under
AddressSanitizer / UBSan; the geometry call; the command line's refusals.

What is compared how.  Every integer with ==.  r(d) is made of two exact integers, each converted once by the rule both sides
define alike (the leading 64 bits, rounded by the conversion, scaled), one square root and one division: == against the
reference, and the texts byte for byte.  NSC and RSC are one more division (and two subtractions) of those doubles: ==."""
import math
import os
import subprocess

import numpy as np
import pytest

import xcor_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tags(rows):
    return np.asarray(rows, dtype=np.int64).reshape(-1, 3)


def _pairs(chrom, xs, dist):
    """A plus tag at every x and a minus tag dist further."""
    return [(chrom, x, 1) for x in xs] + [(chrom, x + dist, 0) for x in xs]


def _same(a, b):
    return (a is None and math.isnan(b)) or a == b


def _check(c, read_len=0):
    """gx_xcor_r and gx_xcor_metrics against the reference; returns the library's record."""
    from genrich_amd.lib import xcor_metrics, xcor_r
    r, exp_r = xcor_r(c.n_pos, c.n_plus, c.n_minus, c.lo, c.hi, c.n11), R.curve(c)
    assert len(r) == len(exp_r) and all(_same(e, float(g)) for e, g in zip(exp_r, r))
    got, exp = xcor_metrics(c.n_pos, c.n_plus, c.n_minus, c.lo, c.hi, c.n11, read_len), R.metrics(c, read_len)
    assert bool(got["has_frag"]) == (exp["fragment_length"] is not None)
    if exp["fragment_length"] is not None:
        assert (int(got["frag_shift"]), int(got["fragment_length"])) == (exp["frag_shift"], exp["fragment_length"])
    if exp["r_min"] is not None:
        assert int(got["min_shift"]) == exp["min_shift"]
    assert bool(got["has_phantom"]) == (exp["r_phantom"] is not None or (read_len > 0 and c.lo <= read_len - 1 <= c.hi))
    for k in ("r_frag", "r_min", "r_phantom", "nsc", "rsc"):
        assert _same(exp[k], float(got[k])), (k, exp[k], got[k])
    return got


def test_the_reference_counts_by_hand():
    # chrA: plus at 2 and 5, minus at 4 and 5 and 9; chrB (length 3): plus at 2, minus at 0: its only pair is at d = -2
    c = R.counts([10, 3], _tags([(0, 2, 1), (0, 5, 1), (0, 5, 1), (0, 4, 0), (0, 5, 0), (0, 9, 0), (1, 2, 1), (1, 0, 0),
                                 (2, 0, 1), (0, 10, 0), (1, 3, 1), (0, 1, 2)]), -3, 7)
    assert (c.n_pos, c.n_plus, c.n_minus, c.rejected) == (13, 3, 4, 4)
    #      d:  -3 -2 -1  0  1  2  3  4  5  6  7
    assert c.n11 == [0, 1, 1, 1, 0, 1, 1, 1, 0, 0, 1]
    assert R.sub_range(c, 0, 2).n11 == [1, 0, 1]
    off = R.counts([10, 3], _tags([(0, 2, 1), (0, 4, 0), (1, 2, 1), (1, 0, 0)]), -3, 7, active=[True, False])
    assert (off.n_pos, off.n_plus, off.n_minus, sum(off.n11)) == (10, 1, 1, 1)


def test_a_single_planted_distance():
    c = R.counts([100_000], _tags(_pairs(0, range(1000, 90_000, 997), 180)), -100, 600)
    m = _check(c)
    n = len(range(1000, 90_000, 997))
    assert c.n11[180 + 100] == n == c.n_plus == c.n_minus
    assert (int(m["fragment_length"]), int(m["frag_shift"])) == (181, 180) and m["r_frag"] == 1.0
    assert m["r_min"] < 0 and math.isnan(m["nsc"]) and math.isnan(m["rsc"]) and not m["has_phantom"]


def test_a_tie_between_two_shifts_goes_to_the_smaller():
    xs = list(range(1000, 50_000, 1009))
    c = R.counts([100_000], _tags(_pairs(0, xs, 120) + [(0, x + 250, 0) for x in xs]), -100, 600)
    assert c.n11[220] == c.n11[350] == len(xs)
    m = _check(c)
    assert int(m["frag_shift"]) == 120 and int(m["fragment_length"]) == 121
    # ... and the least r, which nearly every shift shares, is reported at the smallest shift
    assert int(m["min_shift"]) == -100 and c.n11[0] == 0


def test_a_phantom_peak_higher_than_the_fragment_peak():
    xs = list(range(1000, 90_000, 1009))
    tags = _pairs(0, xs, 35) + [(0, x + 200, 0) for x in xs[::2]]
    c = R.counts([100_000], _tags(tags), -100, 600)
    without = _check(c)
    assert int(without["frag_shift"]) == 35 and not without["has_phantom"] and math.isnan(without["rsc"])      # nobody said it is a phantom
    m = _check(c, 36)
    assert int(m["frag_shift"]) == 200 and int(m["fragment_length"]) == 201 and m["has_phantom"] and int(m["phantom_shift"]) == 35
    assert m["r_phantom"] > m["r_frag"] > 0 and 0 < m["rsc"] < 1
    # the window of exclusion is |d - ph| <= 10: a peak 10 from the phantom is skipped, one 11 from it is not
    for dist, skipped in ((45, True), (46, False), (25, True), (24, False)):
        cc = R.counts([100_000], _tags(_pairs(0, xs, dist) + [(0, x + 300, 0) for x in xs[::2]]), -100, 600)
        assert int(_check(cc, 36)["frag_shift"]) == (300 if skipped else dist), dist


def test_no_tags_on_a_strand_and_every_base_tagged():
    full = [(0, x, s) for x in range(500) for s in (0, 1)]
    for tags in ([(0, 5, 0), (0, 9, 0)], [], full, [(0, x, 1) for x in range(500)] + [(0, 7, 0)]):
        c = R.counts([500], _tags(tags), -5, 20)
        m = _check(c, 4)
        assert not m["has_frag"] and all(math.isnan(m[k]) for k in ("r_frag", "r_min", "r_phantom", "nsc", "rsc"))
        assert m["has_phantom"] and int(m["phantom_shift"]) == 3
    assert R.counts([500], _tags(full), 0, 1).n11 == [500, 499]


def test_nsc_needs_a_positive_least_r_and_rsc_a_phantom_in_range():
    rng = np.random.default_rng(5)
    dense = [(0, int(x), 1) for x in np.nonzero(rng.random(20_000) < 0.3)[0]] + [(0, int(x), 0) for x in np.nonzero(rng.random(20_000) < 0.3)[0]]
    c = R.counts([20_000], _tags(dense), -50, 300)
    m = _check(c, 36)
    assert m["r_min"] < 0 and math.isnan(m["nsc"]) and m["has_frag"]
    # the first half of the chromosome tagged on both strands, the rest empty: n11(d) = 1000 - |d|, r(d) = 1 - 0.002 |d| > 0
    most = [(0, x, s) for x in range(1000) for s in (0, 1)]
    c = R.counts([2000], _tags(most), 1, 40)
    m = _check(c)
    assert m["r_min"] == 0.92 and int(m["min_shift"]) == 40 and m["r_frag"] == 0.998 and m["nsc"] == m["r_frag"] / m["r_min"] >= 1
    for read_len, inside in ((36, True), (41, True), (42, False), (1, False), (2, True)):
        m = _check(c, read_len)
        assert bool(m["has_phantom"]) == inside and (not inside) <= math.isnan(m["rsc"]), read_len
    # a range without a shift >= 1 has no fragment peak
    m = _check(R.counts([2000], _tags(most), -40, 0))
    assert not m["has_frag"] and m["r_min"] > 0 and math.isnan(m["nsc"])


def test_the_largest_counts_and_what_is_refused():
    from genrich_amd.lib import xcor_metrics
    N = (1 << 37) - 1
    c = R.Counts(N, N // 3, N // 5, 0, -4096, 4096, [(N // 15 + 7 * d) for d in range(8193)])
    _check(c, 101)
    for bad in (R.Counts(10, 11, 1, 0, 0, 1, [0, 0]), R.Counts(10, 3, 2, 0, 0, 1, [3, 0]), R.Counts(10, 3, 2, 0, 2, 1, []),
                R.Counts(10, 3, 2, 0, -4097, 0, [0] * 4098), R.Counts(10, 3, 2, 0, 0, 4097, [0] * 4098)):
        with pytest.raises(RuntimeError):
            xcor_metrics(bad.n_pos, bad.n_plus, bad.n_minus, bad.lo, bad.hi, bad.n11)
    with pytest.raises(RuntimeError):
        xcor_metrics(10, 3, 2, 0, 1, [0, 0], -1)


def test_random_cases_against_the_reference():
    rng = np.random.default_rng(7)
    for k in range(12):
        lens = [int(x) for x in rng.integers(1, 3000, int(rng.integers(1, 5)))]
        rows = []
        for ci, L in enumerate(lens):
            for s in (0, 1):
                rows += [(ci, int(x), s) for x in np.nonzero(rng.random(L) < rng.choice([0.02, 0.3, 0.9]))[0]]
        lo = int(rng.integers(-200, 50))
        c = R.counts(lens, _tags(rows), lo, lo + int(rng.integers(0, 400)))
        _check(c, int(rng.integers(0, 80)))


def test_the_geometry_call():
    from genrich_amd.lib import GX_PATH_XCOR, TAG_DTYPE, XCOR_MIN_TILE, xcor_geometry
    lanes, grid, tile, pad, flush = xcor_geometry()
    assert lanes == 256 and 1 <= grid <= 65535 and tile % 64 == 0 and XCOR_MIN_TILE == 64 <= tile <= 1024
    assert pad == 4096 // 64 + 1                      # a window shifted by 4096 bits ends at most 64 words and a word's rest further
    assert flush * 64 < 1 << 32 and flush >= tile     # 64 pairs per plus word at most: the 32-bit counters cannot wrap
    assert GX_PATH_XCOR == 1 << 27 and TAG_DTYPE.itemsize == 12


def _cases():
    """(label, read_len, [(rep, is_ctrl, Counts)]) with one range of shifts per case."""
    xs = list(range(1000, 90_000, 1009))
    planted = R.counts([100_000, 700], _tags(_pairs(0, xs, 35) + [(0, x + 200, 0) for x in xs[::2]] + [(1, 699, 1), (1, 700, 0), (5, 0, 1)]), -100, 600)
    empty = R.counts([100_000, 700], _tags([]), -100, 600)
    one_strand = R.counts([100_000, 700], _tags([(0, 5, 1)]), -100, 600)
    narrow = R.counts([300], _tags(_pairs(0, range(0, 200, 7), 3)), 0, 0)
    return [("planted", 36, [(0, False, planted)]), ("three", 0, [(0, False, empty), (0, True, planted), (1, False, one_strand)]),
            ("narrow", 2, [(2, True, narrow)]), ("outside", 900, [(0, False, planted)])]


def test_the_writers_against_the_reference():
    from genrich_amd.lib import Xcor, format_xcor, format_xcor_metrics
    for label, read_len, samples in _cases():
        xs = [Xcor(c.n_pos, c.n_plus, c.n_minus, c.rejected, c.lo, c.hi, c.n11, rep, ctrl) for rep, ctrl, c in samples]
        assert format_xcor(xs).decode() == R.curve_text(samples), label
        assert format_xcor_metrics(xs, read_len).decode() == R.metrics_text(samples, read_len), label
    text = R.metrics_text(_cases()[0][2], 36).splitlines()
    assert text[0].split("\t") == ["sample", "n_pos", "n_plus", "n_minus", "fragment_length", "r_frag", "min_shift", "r_min", "phantom_shift", "r_phantom",
                                   "NSC", "RSC"]
    assert text[1].split("\t")[:5] == ["t0", "100700", "90", "134", "201"] and text[1].split("\t")[8] == "35"
    three = R.metrics_text(_cases()[1][2]).splitlines()
    assert three[1] == "t0\t100700\t0\t0\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA"
    curve = R.curve_text(_cases()[0][2]).splitlines()
    assert curve[0] == "sample\tshift\tn11\tr" and curve[1] == "# t0\tn_pos=100700\tn_plus=90\tn_minus=134\trejected=2" and curve[2].startswith("t0\t-100\t0\t-")


def test_format_standalone_under_sanitizers(tmp_path):
    """gx_emit.cpp's figures and writers in a program of its own (its own main, tests/xcor_format_main.cpp), compiled with
    -fsanitize=address,undefined: any report makes the program fail (-fno-sanitize-recover, ASan aborts by default)."""
    exe = str(tmp_path / "xcor_format")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "xcor_format_main.cpp"),
                           os.path.join(ROOT, "genrich_amd", "csrc", "gx_emit.cpp"), "-o", exe])
    cases = _cases()
    lines = []
    for label, read_len, samples in cases:
        c0 = samples[0][2]
        lines.append(f"{len(samples)} {c0.lo} {c0.hi} {read_len}")
        for rep, ctrl, c in samples:
            lines.append(f"{rep} {int(ctrl)} {c.n_pos} {c.n_plus} {c.n_minus} {c.rejected}")
            lines.append(" ".join(str(v) for v in c.n11))
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join(lines) + "\n")
    res = subprocess.run([exe, str(spec)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
    parts = res.stdout.split("--\n")
    assert len(parts) == 2 * len(cases) + 1 and parts[-1] == ""
    for i, (label, read_len, samples) in enumerate(cases):
        assert parts[2 * i] == R.curve_text(samples), label
        assert parts[2 * i + 1] == R.metrics_text(samples, read_len), label


# ---- the command line ------------------------------------------------------------------------------------------------------------

def test_cli_refusals_create_no_file(tmp_path):
    """Refused before any input is read: no GPU needed."""
    from genrich_amd import build

    binp = build.build_host()
    sam = tmp_path / "t.sam"
    sam.write_text("@SQ\tSN:chrA\tLN:1000\n")
    out, met, npk, ev = tmp_path / "xc.tsv", tmp_path / "xcm.tsv", tmp_path / "o.np", tmp_path / "ev.bed"
    msg = "--xcor and --xcor-metrics need the alignments of this run (not with -P or --events-only)"
    for extra in (["-t", str(sam), "--xcor", str(out), "--events-only", "-b", str(ev)],
                  ["-t", str(sam), "--xcor-metrics", str(met), "--events-only", "-b", str(ev)],
                  ["-t", str(sam), "--xcor", str(out), "--xcor-metrics", str(met), "-P", "-f", str(tmp_path / "in.log")]):
        res = subprocess.run([binp, "-o", str(npk)] + extra, capture_output=True, text=True)
        assert res.returncode == 1 and msg in res.stderr, (extra, res.stderr)
        assert not out.exists() and not met.exists() and not npk.exists() and not ev.exists(), extra
    for extra in (["--xcor-shifts", "0,100"], ["--xcor-read-length", "36"], ["--xcor-unpaired"]):
        res = subprocess.run([binp, "-o", str(npk), "-t", str(sam)] + extra, capture_output=True, text=True)
        assert res.returncode == 1 and "need --xcor FILE or --xcor-metrics FILE" in res.stderr, (extra, res.stderr)
    for shifts in ("600,-100", "-4097,0", "0,4097", "5", "5,", ",5", "a,b", "1,2,3", "1.5,2", " 1,2", "1, 2", ""):
        res = subprocess.run([binp, "-o", str(npk), "-t", str(sam), "--xcor", str(out), "--xcor-shifts", shifts], capture_output=True, text=True)
        assert res.returncode == 1 and "--xcor-shifts takes two integers LO,HI with -4096 <= LO <= HI <= 4096" in res.stderr, (shifts, res.stderr)
    for rl in ("0", "-36", "36bp", "x", "", "1000001"):
        res = subprocess.run([binp, "-o", str(npk), "-t", str(sam), "--xcor", str(out), "--xcor-read-length", rl], capture_output=True, text=True)
        assert res.returncode == 1 and "--xcor-read-length takes a positive integer" in res.stderr, (rl, res.stderr)
    assert not out.exists() and not met.exists() and not npk.exists()


def test_cli_help_names_the_options():
    from genrich_amd import build

    res = subprocess.run([build.build_host(), "-h"], capture_output=True, text=True)
    assert "--xcor FILE [--xcor-metrics FILE] [--xcor-shifts LO,HI] [--xcor-read-length R] [--xcor-unpaired]" in res.stderr
    assert "-100,600" in res.stderr and "phantom peak" in res.stderr and "NSC" in res.stderr and "RSC" in res.stderr
