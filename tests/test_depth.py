"""The depth distribution's reference, figures and text writers without a GPU: tests/depth_ref.py against a base-by-base brute
force; gx_depth_metrics and gx_format_depth* through ctypes against the reference; the writers once more as a stand-alone
program under AddressSanitizer / UBSan; the geometry call; the command line's refusals.

What is compared how.  Every integer (the classes, the list, B, covered, min, max, the percentiles) with ==.  covered_fraction and
the ge* figures are ONE division of two exact integers below 2^53: the correctly rounded double, ==.  mean and sd are made of the
exact sums by the conversion both sides define alike (the leading 64 bits of the big integer, converted once, scaled), one
square root (correctly rounded in IEEE arithmetic) and one division: ==, and the texts byte for byte."""
import math
import os
import subprocess

import numpy as np
import pytest

import backends as B
import depth_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hist(pairs, zero=0, excluded=0, rep=0, ctrl=False):
    """A histogram made up of (v, bases) pairs, `zero` bases at 0 and `excluded` bases inside -E regions."""
    bases, rsum, rsq = (np.zeros(R.DEPTH_BOUND, dtype=np.uint64) for _ in range(3))
    deep = []
    for v, n in sorted(pairs):
        d, r = divmod(v, 120)
        if d < R.DEPTH_BOUND:
            bases[d] += np.uint64(n)
            rsum[d] += np.uint64(r * n)
            rsq[d] += np.uint64(r * r * n)
        else:
            deep.append((v, n))
    covered = sum(n for _, n in pairs)
    vs = [v for v, _ in pairs]
    return R.Hist(rep, ctrl, covered + zero + excluded, excluded, zero, min(vs) if vs else 0, max(vs) if vs else 0, bases, rsum, rsq, deep)


def _cases():
    """(label, [Hist])"""
    rng = np.random.default_rng(31)
    out = [("no_bases", [_hist([]), _hist([], excluded=5000, rep=1)]),                       # B = 0, with and without a genome
           ("all_zero", [_hist([], zero=12_345)]),
           ("single_class", [_hist([(360, 500)]), _hist([(360, 500)], zero=1, excluded=7, ctrl=True)]),
           ("fractional", [_hist([(20, 10), (119, 3), (120, 40), (160, 7), (184, 9), (240, 5), (12 * 120 + 15, 2)], zero=100)]),
           ("class_zero_only", [_hist([(12, 4), (60, 4)])]),
           # one pileup of 3000 reads over 2^40 bases: v^2 bases = 1.4 * 10^23 > 2^64; and distinct v in one whole depth
           ("deep_beyond_64_bits", [_hist([(360_000, 1 << 40), (360_017, 3), (360_100, 2), (120 * 2048, 1), (120 * 2048 - 1, 1), (0x7fffffff, 2)],
                                          zero=1 << 30)]),
           # 100 bases, the cumulative counts 25, 50, 75, 95, 99, 100: every percentile lies exactly on a class boundary
           ("ties", [_hist([(120, 25), (240, 25), (360, 20), (480, 4), (600, 1)], zero=25),
                     _hist([(120, 24), (240, 26), (360, 20), (480, 4), (600, 1)], zero=25, rep=1),     # one base short of 50: the median moves up
                     _hist([(120 * 3000, 50)], zero=50, rep=2)])]                                     # the median at 0, q75 in the list
    for i in range(4):
        k = int(rng.integers(1, 60))
        vs = np.unique(np.concatenate([rng.integers(1, 120 * 40, k), rng.integers(120 * 2040, 120 * 2060, 6)]))
        out.append((f"random{i}", [_hist([(int(v), int(rng.integers(1, 10 ** 6))) for v in vs], zero=int(rng.integers(0, 10 ** 7)),
                                         excluded=int(rng.integers(0, 10 ** 5)), rep=i, ctrl=bool(i & 1))]))
    return out


@pytest.fixture(scope="module")
def cases():
    return _cases()


def test_reference_against_the_brute_force():
    rng = np.random.default_rng(5)
    lens = [300, 64, 1]
    n = 400
    ev = np.zeros(n, dtype=B.EVENT_DTYPE)
    ev["chrom"] = rng.choice(3, n, p=[0.7, 0.25, 0.05])
    ev["start"] = rng.integers(0, np.asarray(lens)[ev["chrom"]])
    ev["end"] = ev["start"] + rng.integers(0, 90, n)          # (empty intervals, ends beyond the length)
    ev["count"] = rng.choice([1, 2, 3, 4, 5, 6, 7, 8, 10], n)  # (7: not a valid count, dropped)
    pile = np.zeros(2100, dtype=B.EVENT_DTYPE)                 # ... and a pile across the class / list boundary
    pile["chrom"], pile["start"], pile["count"] = 0, 100 + np.arange(2100) % 3, 1
    pile["end"] = 130 - np.arange(2100) % 2
    ev = np.concatenate([ev, pile])
    for beds in (None, [[10, 20, 15, 40, 18, 19, 290, 400], [], [0, 1]], [[0, 100], [0, 10, 60, 64], []]):
        got, exp = R.hist(ev, lens, beds=beds), R.brute(ev, lens, beds)
        assert R.same(got, exp) is None, R.same(got, exp)
        assert exp.deep and exp.bases[1:].any() and exp.rsum.any()
        sv, sv2 = R.sums(exp)
        assert sv > 0 and sv2 >= sv
    assert R.hist(ev, lens, beds=[[0, 300], [0, 64], [0, 1]]).total == R.hist(ev, lens, beds=[[0, 300], [0, 64], [0, 1]]).excluded == 365
    # a skipped chromosome does not count; one the header does not list counts with pileup 0
    a, b = R.hist(ev, lens, skip=[0, 1, 0]), R.hist(ev, lens, save=[1, 0, 1])
    assert a.total == 301 and b.total == 365 and a.zero + 64 == b.zero and np.array_equal(a.bases, b.bases)


def test_metrics_through_ctypes_against_the_reference(cases):
    from genrich_amd.lib import Depth, depth_metrics
    for label, samples in cases:
        for h in samples:
            m, exp = depth_metrics(Depth(*h)), R.metrics(h)
            for k in ("bases", "excluded", "covered", "min_v", "max_v", "q25", "median", "q75", "p95", "p99"):
                assert int(m[k]) == exp[k], (label, k, int(m[k]), exp[k])
            for k in ("covered_fraction", "mean", "sd"):
                assert float(m[k]) == exp[k] or (math.isnan(float(m[k])) and math.isnan(exp[k])), (label, k, float(m[k]), exp[k])
            assert [float(x) for x in m["ge"]] == exp["ge"], (label, m["ge"], exp["ge"])
    by = dict(cases)
    m = depth_metrics(Depth(*by["ties"][0]))
    assert [int(m[k]) for k in ("q25", "median", "q75", "p95", "p99")] == [0, 1, 2, 3, 4] and float(m["mean"]) == 1.56
    m = depth_metrics(Depth(*by["ties"][1]))
    assert [int(m[k]) for k in ("q25", "median", "q75", "p95", "p99")] == [0, 2, 2, 3, 4]
    m = depth_metrics(Depth(*by["ties"][2]))
    assert [int(m[k]) for k in ("q25", "median", "q75", "p95", "p99")] == [0, 0, 3000, 3000, 3000] and float(m["sd"]) == 1500.0
    m = depth_metrics(Depth(*by["deep_beyond_64_bits"][0]))
    h = by["deep_beyond_64_bits"][0]
    assert R.sums(h)[1] > 1 << 64 and int(m["max_v"]) == 0x7fffffff and int(m["min_v"]) == 0
    m = depth_metrics(Depth(*by["single_class"][0]))
    assert (float(m["mean"]), float(m["sd"]), int(m["min_v"]), int(m["max_v"]), float(m["covered_fraction"])) == (3.0, 0.0, 360, 360, 1.0)
    assert [float(x) for x in m["ge"]] == [1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]


def test_format_through_ctypes_against_the_reference(cases):
    from genrich_amd.lib import Depth, format_depth, format_depth_metrics
    for label, samples in cases:
        ds = [Depth(*h) for h in samples]
        assert format_depth(ds).decode() == R.depth_text(samples), label
        assert format_depth_metrics(ds).decode() == R.metrics_text(samples), label
    by = dict(cases)
    assert format_depth([Depth(*h) for h in by["no_bases"]]).decode() == R.HEADER + "t0\t0\t0\t0\t0.000000\nt1\t0\t0\t0\t0.000000\n"
    row = format_depth_metrics([Depth(*by["no_bases"][1])]).decode().splitlines()[1].split("\t")
    assert row == ["t1", "0", "5000", "0", "0.000000", "NA", "NA", "0", "0", "0", "0", "0", "0", "0"] + ["0.000000"] * 7
    assert format_depth([Depth(*by["single_class"][1])]).decode() == R.HEADER + "c0\t0\t1\t501\t1.000000\nc0\t3\t500\t500\t0.998004\n"
    rows = format_depth([Depth(*by["deep_beyond_64_bits"][0])]).decode().splitlines()
    assert rows[-3].split("\t")[:3] == ["t0", "2048", "1"] and rows[-2].split("\t")[:3] == ["t0", "3000", str((1 << 40) + 5)]
    row = format_depth_metrics([Depth(*by["fractional"][0])]).decode().splitlines()[1].split("\t")
    assert row[7] == "0" and row[13] == "12.1250"
    row = format_depth_metrics([Depth(*by["class_zero_only"][0])]).decode().splitlines()[1].split("\t")
    assert row[7] == "0.1000" and row[13] == "0.5000" and row[14] == "0.000000"


def test_a_histogram_that_contradicts_itself_is_refused(cases):
    from genrich_amd.lib import Depth, depth_metrics, format_depth
    h = dict(cases)["fractional"][0]
    bad_rsum = h.rsum.copy()
    bad_rsum[1] = 120 * int(h.bases[1])
    for bad in (h._replace(zero=h.zero + 1), h._replace(excluded=h.total + 1), h._replace(rsum=bad_rsum), h._replace(min_v=0),
                h._replace(deep=[(120 * 2048 - 1, 1)], zero=h.zero - 1), h._replace(deep=[(300_000, 1), (300_000, 1)], zero=h.zero - 2)):
        with pytest.raises(RuntimeError):
            depth_metrics(Depth(*bad))
        with pytest.raises(RuntimeError):
            format_depth([Depth(*bad)])


def test_the_geometry_call():
    from genrich_amd.lib import DEPTH_BOUND, depth_geometry
    bound, lanes, grid, cap = depth_geometry()
    assert bound == DEPTH_BOUND == R.DEPTH_BOUND == 2048
    assert lanes % 64 == 0 and 64 <= lanes <= 1024 and 1 <= grid <= 65535 and cap >= 1


def test_format_standalone_under_sanitizers(cases, tmp_path):
    """gx_emit.cpp's writers in a program of its own (its own main, tests/depth_format_main.cpp), compiled with
    -fsanitize=address,undefined: any report makes the program fail (-fno-sanitize-recover, ASan aborts by default)."""
    exe = str(tmp_path / "depth_format")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "depth_format_main.cpp"),
                           os.path.join(ROOT, "genrich_amd", "csrc", "gx_emit.cpp"), "-o", exe])
    lines = []
    for label, samples in cases:
        lines.append(str(len(samples)))
        for h in samples:
            cls = [d for d in range(R.DEPTH_BOUND) if int(h.bases[d])]
            lines.append(f"{h.rep} {int(h.is_ctrl)} {h.total} {h.excluded} {h.zero} {h.min_v} {h.max_v} {len(cls)} {len(h.deep)}")
            lines += [f"{d} {int(h.bases[d])} {int(h.rsum[d])} {int(h.rsq[d])}" for d in cls]
            lines += [f"{v} {n}" for v, n in h.deep]
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join(lines) + "\n")
    res = subprocess.run([exe, str(spec)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
    parts = res.stdout.split("--\n")
    assert len(parts) == 2 * len(cases) + 1 and parts[-1] == ""
    for i, (label, samples) in enumerate(cases):
        assert parts[2 * i] == R.depth_text(samples), label
        assert parts[2 * i + 1] == R.metrics_text(samples), label


# ---- the command line ------------------------------------------------------------------------------------------------------------

def test_cli_refusals_create_no_file(tmp_path):
    """Refused before any input is read: no GPU needed."""
    from genrich_amd import build

    binp = build.build_host()
    sam = tmp_path / "t.sam"
    sam.write_text("@SQ\tSN:chrA\tLN:1000\n")
    out, met, npk, ev = tmp_path / "depth.tsv", tmp_path / "depthm.tsv", tmp_path / "o.np", tmp_path / "ev.bed"
    for extra in (["-t", str(sam), "--depth", str(out), "--events-only", "-b", str(ev)],
                  ["-t", str(sam), "--depth-metrics", str(met), "--events-only", "-b", str(ev)],
                  ["-t", str(sam), "--depth", str(out), "--depth-metrics", str(met), "-P", "-f", str(tmp_path / "in.log")]):
        res = subprocess.run([binp, "-o", str(npk)] + extra, capture_output=True, text=True)
        assert res.returncode == 1 and "--depth and --depth-metrics need the pileups of this run" in res.stderr, (extra, res.stderr)
        assert not out.exists() and not met.exists() and not npk.exists() and not ev.exists(), extra


def test_cli_help_names_the_options():
    from genrich_amd import build

    res = subprocess.run([build.build_host(), "-h"], capture_output=True, text=True)
    assert "--depth FILE [--depth-metrics FILE]" in res.stderr
