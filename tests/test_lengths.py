"""The interval lengths' reference, figures and text writers without a GPU: the two entry points of tests/lengths_ref.py against
each other on the golden fixtures; gx_lengths_metrics through ctypes against hand-computed cases and the reference; the writers
once more as a stand-alone program under AddressSanitizer / UBSan; the geometry call; the command line's refusals.

What is compared how.  Every integer with ==.  A share is ONE division of two exact integers below 2^53: the correctly rounded
double, ==.  mean and sd are made of the exact sums by the conversion both sides define alike (the leading 64 bits of the big
integer, converted once, scaled), one square root and one division: == against the reference, and the texts byte for byte; the
hand-computed values are exact in a double wherever they are compared with ==."""
import math
import os
import subprocess

import numpy as np
import pytest

import golden_cases as G
import lengths_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["ctrl_q", "dups_y", "atac", "unpaired_y", "dups_pairs", "bedx", "reps3_p_missing"]


def _check(lengths, cuts=R.CUTS):
    """gx_lengths_metrics against the reference; returns the library's record."""
    from genrich_amd.lib import lengths_metrics
    got, exp = lengths_metrics(lengths, cuts), R.metrics(lengths, cuts)
    for k in ("n", "w120", "min", "max", "mode", "p5", "q25", "median", "q75", "p95"):
        assert int(got[k]) == exp[k], (k, int(got[k]), exp[k])
    for k in ("mean", "sd"):
        assert (math.isnan(got[k]) and exp[k] is None) or got[k] == exp[k], (k, got[k], exp[k])
    assert int(got["n_shares"]) == len(cuts) + 1 and [float(x) for x in got["share"][:len(cuts) + 1]] == exp["share"]
    return got


@pytest.mark.parametrize("name", FIXTURES)
def test_the_two_entry_points_agree_on_the_fixtures(name):
    meta, case, params, names = G.load_case(name)
    lens = case["lens"]
    per = R.of_bed_rows(G.read_gz(name, "events.bed").decode().splitlines(), names, lens)
    seen = 0
    for r, rep in enumerate(case["replicates"]):
        for ctrl, ev in ((False, rep["treat"]), (True, rep["ctrl"])):
            if ev is None or not len(ev):
                assert (r, ctrl) not in per
                continue
            active = [not s for s in case["skip"]]
            st = R.of_events(ev, lens, active)
            assert st == per[(r, ctrl)] and R.invariants(st) and sum(st.cn) == len(ev)
            assert all(st.cn[c] == 0 for c in range(len(lens)) if case["skip"][c])
            seen += 1
    assert seen == len(per) >= 1
    if name == "atac":      # cut-site windows: nearly all of one length
        st = per[(0, False)]
        assert max(n for _, n, _ in st.lengths) > 0.9 * sum(n for _, n, _ in st.lengths)


def test_a_single_length():
    m = _check([(200, 7, 7 * 120)])
    assert (m["n"], m["w120"], m["min"], m["max"], m["mode"], m["p5"], m["median"], m["p95"]) == (7, 840, 200, 200, 200, 200, 200, 200)
    assert m["mean"] == 200.0 and m["sd"] == 0.0 and list(m["share"][:4]) == [0.0, 1.0, 0.0, 0.0]


def test_two_lengths_of_equal_weight_tie_to_the_smaller():
    m = _check([(100, 3, 360), (300, 6, 360)])        # 3 intervals at weight 1, 6 at weight 1/2
    assert (m["mode"], m["median"], m["q25"], m["q75"], m["p5"], m["p95"]) == (100, 100, 100, 300, 100, 300)
    assert m["mean"] == 200.0 and m["sd"] == 100.0 and m["n"] == 9
    assert list(m["share"][:4]) == [0.5, 0.0, 0.5, 0.0]      # 300 is not below the cut 300


def test_weights_of_all_eight_count_classes():
    lengths = [(50 + 10 * i, 2, 2 * (120 // c)) for i, c in enumerate(R.VALID_COUNTS)]
    W = 2 * sum(120 // c for c in R.VALID_COUNTS)
    assert W == 2 * (120 + 60 + 40 + 30 + 24 + 20 + 15 + 12)
    m = _check(lengths)
    assert m["w120"] == W and m["n"] == 16 and m["mode"] == 50
    # cumulative weight 240, 360, 440, 500, 548, 588, 618, 642: the median is the smallest L with 100 cum >= 50 W = 32100 -> 360 at L = 60
    assert m["median"] == 60 and m["q25"] == 50 and m["p5"] == 50 and m["q75"] == 80 and m["p95"] == 110
    assert m["mean"] == sum(w * L for L, _, w in lengths) / W


def test_a_cut_equal_to_an_occurring_length():
    lengths = [(149, 1, 120), (150, 1, 120), (299, 1, 120), (300, 1, 120), (500, 4, 480)]
    m = _check(lengths)
    assert list(m["share"][:4]) == [0.125, 0.25, 0.125, 0.5]
    m = _check(lengths, cuts=(150,))
    assert list(m["share"][:2]) == [0.125, 0.875]
    m = _check(lengths, cuts=())
    assert list(m["share"][:1]) == [1.0]


def test_the_largest_length_with_the_largest_weight():
    top, n = (1 << 32) - 1, 1 << 31
    m = _check([(top, n - 1, 120 * (n - 1))])
    # (sum w L has 70 bits: its leading 64 are converted, rounded to 53: 2^-53 of 2^32 after the division)
    assert abs(m["mean"] - float(top)) < 1e-3 and m["sd"] == 0.0 and m["max"] == top
    m = _check([(1, n >> 1, 120 * (n >> 1)), (top, n >> 1, 120 * (n >> 1))])
    assert m["mean"] == float(1 << 31) and abs(m["sd"] - float((1 << 31) - 1)) < 1e-3 and m["median"] == 1 and m["q75"] == top
    _check([(0, 5, 600), (top, n - 6, 12 * (n - 6))])


def test_an_empty_sample_and_what_is_refused():
    from genrich_amd.lib import lengths_metrics
    m = _check([])
    assert m["n"] == 0 and math.isnan(m["mean"]) and math.isnan(m["sd"]) and list(m["share"][:4]) == [0.0] * 4
    for bad in ([(5, 1, 120), (5, 1, 120)], [(5, 0, 0)], [(5, 1, 121)], [(5, 2, 1)], [(1 << 32, 1, 120)]):
        with pytest.raises(RuntimeError):
            lengths_metrics(bad)
    for cuts in ((300, 150), (0, 5), tuple(range(1, 10))):
        with pytest.raises(RuntimeError):
            lengths_metrics([(5, 1, 120)], cuts)


def test_random_cases_against_the_reference():
    rng = np.random.default_rng(7)
    for _ in range(20):
        k = int(rng.integers(1, 80))
        Ls = sorted(set(int(x) for x in rng.integers(0, 3000, k)))
        lengths = []
        for L in Ls:
            n = int(rng.integers(1, 10 ** 6))
            lengths.append((L, n, int(rng.integers(n, 120 * n + 1))))
        _check(lengths, tuple(sorted(set(int(x) for x in rng.integers(1, 3000, int(rng.integers(0, 9)))))))


def test_the_geometry_call():
    from genrich_amd.lib import GX_PATH_IVSTAT, interval_stats_geometry
    lanes, grid, bound, window, cap = interval_stats_geometry()
    assert lanes == 1024 and 1 <= grid <= 65535 and bound == 4096 and window == 512 and cap >= 1
    assert GX_PATH_IVSTAT == 1 << 26


def _cases():
    """(label, cut_sites, cuts, names, lens, [(rep, is_ctrl, Stats)])"""
    rng = np.random.default_rng(11)
    names, lens = ["chrA", "chrB", "chrEmpty"], [5000, 70_000, 0]
    rows = [(0, 10, 110, 1), (0, 10, 110, 2), (0, 4990, 5000, 3), (1, 100, 100, 1), (1, 500, 460, 4), (1, 0, 69_999, 10), (1, 7, 4103, 8)]
    mixed = R.of_intervals(rows, 3)
    empty = R.of_intervals([], 3)
    many = R.of_intervals([(int(rng.integers(0, 2)), 100, 100 + int(rng.integers(0, 900)), int(rng.choice(R.VALID_COUNTS))) for _ in range(3000)], 3)
    return [("mixed", False, R.CUTS, names, lens, [(0, False, mixed)]),
            ("empty_and_ctrl", False, R.CUTS, names, lens, [(0, False, empty), (0, True, mixed), (1, False, many)]),
            ("cut_sites", True, (100,), names, lens, [(2, False, many)]),
            ("no_cuts", False, (), names[:1], lens[:1], [(0, False, R.of_intervals(rows[:3], 1))])]


def test_format_standalone_under_sanitizers(tmp_path):
    """gx_emit.cpp's writers in a program of its own (its own main, tests/lengths_format_main.cpp), compiled with
    -fsanitize=address,undefined: any report makes the program fail (-fno-sanitize-recover, ASan aborts by default)."""
    exe = str(tmp_path / "lengths_format")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "lengths_format_main.cpp"),
                           os.path.join(ROOT, "genrich_amd", "csrc", "gx_emit.cpp"), "-o", exe])
    cases = _cases()
    lines = []
    for label, cut_sites, cuts, names, lens, samples in cases:
        lines.append(f"{len(samples)} {len(names)} {int(cut_sites)} {len(cuts)}")
        lines.append(" ".join(str(c) for c in cuts))
        lines += [f"{n} {ln}" for n, ln in zip(names, lens)]
        for rep, ctrl, st in samples:
            lines.append(f"{rep} {int(ctrl)} {len(st.lengths)} {st.n_inverted} {st.w120_inverted}")
            lines += [f"{L} {n} {w}" for L, n, w in st.lengths]
            lines += [f"{a} {b} {c}" for a, b, c in zip(st.cn, st.cw120, st.cbases120)]
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join(lines) + "\n")
    res = subprocess.run([exe, str(spec)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
    parts = res.stdout.split("--\n")
    assert len(parts) == 3 * len(cases) + 1 and parts[-1] == ""
    for i, (label, cut_sites, cuts, names, lens, samples) in enumerate(cases):
        assert parts[3 * i] == R.lengths_text(samples, cut_sites), label
        assert parts[3 * i + 1] == R.metrics_text(samples, cuts), label
        assert parts[3 * i + 2] == R.chrom_text(names, lens, samples), label
    mixed = parts[0].splitlines()
    assert mixed[0].startswith("# an interval is one of the sample's -b lines") and "-j" in mixed[0]
    assert "t0\t100\t2\t1.50\t" in parts[0] and "t0\tinverted\t1\t0.25\tNA\n" in parts[0] and "t0\t0\t1\t1\t" in parts[0]
    assert parts[6].startswith("# an interval is a cut-site window of -j")


# ---- the command line ------------------------------------------------------------------------------------------------------------

def test_cli_refusals_create_no_file(tmp_path):
    """Refused before any input is read: no GPU needed."""
    from genrich_amd import build

    binp = build.build_host()
    sam = tmp_path / "t.sam"
    sam.write_text("@SQ\tSN:chrA\tLN:1000\n")
    out, met, chs, npk, ev = tmp_path / "len.tsv", tmp_path / "lenm.tsv", tmp_path / "chr.tsv", tmp_path / "o.np", tmp_path / "ev.bed"
    msg = "--lengths, --lengths-metrics and --chrom-stats need the intervals of this run (not with -P or --events-only)"
    for extra in (["-t", str(sam), "--lengths", str(out), "--events-only", "-b", str(ev)],
                  ["-t", str(sam), "--lengths-metrics", str(met), "--events-only", "-b", str(ev)],
                  ["-t", str(sam), "--chrom-stats", str(chs), "--events-only", "-b", str(ev)],
                  ["-t", str(sam), "--lengths", str(out), "--chrom-stats", str(chs), "-P", "-f", str(tmp_path / "in.log")]):
        res = subprocess.run([binp, "-o", str(npk)] + extra, capture_output=True, text=True)
        assert res.returncode == 1 and msg in res.stderr, (extra, res.stderr)
        assert not out.exists() and not met.exists() and not chs.exists() and not npk.exists() and not ev.exists(), extra
    res = subprocess.run([binp, "-o", str(npk), "-t", str(sam), "--lengths", str(out), "--lengths-cuts", "100,200"], capture_output=True, text=True)
    assert res.returncode == 1 and "--lengths-cuts needs --lengths-metrics FILE" in res.stderr
    for cuts in ("300,150", "0,5", "1,2,3,4,5,6,7,8,9", "150,", "a", "150,,300", "-5"):
        res = subprocess.run([binp, "-o", str(npk), "-t", str(sam), "--lengths-metrics", str(met), "--lengths-cuts", cuts], capture_output=True, text=True)
        assert res.returncode == 1 and "--lengths-cuts takes at most 8 ascending positive integers" in res.stderr, (cuts, res.stderr)
    assert not out.exists() and not met.exists() and not npk.exists()


def test_cli_help_names_the_options():
    from genrich_amd import build

    res = subprocess.run([build.build_host(), "-h"], capture_output=True, text=True)
    assert "--lengths FILE [--lengths-metrics FILE] [--lengths-cuts A,B,...] [--chrom-stats FILE]" in res.stderr
    assert "cut-site windows" in res.stderr and "skipped with -e" in res.stderr
