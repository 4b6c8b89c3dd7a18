"""The fingerprint's value classes, figures and text writers (gx_fp_class, gx_fingerprint_metrics, gx_format_fingerprint*) without
a GPU: through ctypes against tests/fingerprint_ref.py's integers and fractions, the writers once more as a stand-alone program
under AddressSanitizer / UBSan, and the command line's refusals."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import fingerprint_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1


# ---- the classes ---------------------------------------------------------------------------------------------------------------

def test_geometry():
    from genrich_amd.lib import FP_NC, FP_SUB_LOG, fp_geometry
    nc, sub_log, lanes, grid = fp_geometry()
    assert nc == 3776 == R.NC == FP_NC and sub_log == 6 == R.SUB_LOG == FP_SUB_LOG
    assert lanes % 64 == 0 and lanes >= 64 and grid >= 1


def test_classes_against_the_reference_at_every_edge():
    from genrich_amd.lib import fp_class, fp_class_hi, fp_class_lo
    rng = np.random.default_rng(3)
    xs = {0, U64}
    for k in range(R.NC):
        lo, hi = R.lo(k), R.hi(k)
        assert fp_class_lo(k) == lo and fp_class_hi(k) == hi, k
        xs.update(x for x in (lo - 1, lo, hi, hi + 1) if 0 <= x <= U64)
    xs.update(int(x) for x in rng.integers(0, 1 << 64, 10_000, dtype=np.uint64))
    xs.update(int(x) >> int(s) for x, s in zip(rng.integers(0, 1 << 64, 2000, dtype=np.uint64), rng.integers(0, 64, 2000)))   # every magnitude
    for x in xs:
        assert fp_class(x) == R.cls(x), x
    assert R.cls(U64) == R.NC - 1 and R.hi(R.NC - 1) == U64 and R.lo(0) == 0


def test_the_classes_are_monotone_and_tile_uint64():
    from genrich_amd.lib import fp_class, fp_class_hi, fp_class_lo
    for k in range(R.NC):
        assert fp_class(fp_class_lo(k)) == fp_class(fp_class_hi(k)) == k
        assert R.cls(R.lo(k)) == R.cls(R.hi(k)) == k
        if k + 1 < R.NC:
            assert fp_class_lo(k + 1) == fp_class_hi(k) + 1 and R.lo(k + 1) == R.hi(k) + 1
        if k >= 128:
            assert (R.hi(k) - R.lo(k) + 1) * 64 <= R.lo(k)          # a spread of less than 1 / 64
        else:
            assert R.lo(k) == R.hi(k) == k
    a = np.random.default_rng(4).integers(0, 1 << 64, 5000, dtype=np.uint64)
    assert [R.cls(int(x)) for x in a] == R.cls_array(a).tolist()     # the reference's own numpy form


# ---- the figures and the text ----------------------------------------------------------------------------------------------------

def _sparse(S, entries):
    """entries: {(sample, class): (count, sum)} -> (count, sum) as lists of NC ints per sample."""
    count, total = [[0] * R.NC for _ in range(S)], [[0] * R.NC for _ in range(S)]
    for (s, k), (c, t) in entries.items():
        count[s][k], total[s][k] = c, t
    return count, total


def _cases():
    """(label, names, (count, sum), ctrl_of)"""
    rng = np.random.default_rng(11)
    out = []
    out.append(("one_class", ["t0"], _sparse(1, {(0, 200): (7, 7 * R.lo(200))}), [-1]))
    out.append(("only_zeros", ["t0", "c0"], _sparse(2, {(0, 0): (1000, 0), (1, 0): (3, 0)}), [1, -1]))
    x = np.where(rng.random(5000) < 0.4, 0, rng.integers(0, 1 << 22, 5000))
    h = R.hist([x, x.copy()])
    out.append(("identical", ["t0", "c0"], h, [1, -1]))
    out.append(("disjoint", ["t0", "c0"], _sparse(2, {(0, 3): (10, 30), (0, 700): (5, 5 * R.hi(700)), (1, 4): (2, 8), (1, 699): (9, 9 * R.lo(699))}),
                [1, -1]))
    y = np.where(rng.random(3000) < 0.2, 0, rng.integers(0, 1 << 30, 3000))
    z = (rng.pareto(1.2, 4000) * 2000).astype(np.int64)
    out.append(("no_control", ["t0", "t1", "c1"], R.hist([y, z[:3000], z[1000:]]), [-1, 2, -1]))
    out.append(("ctrl_of_none", ["t0", "t1"], R.hist([y, z]), None))
    out.append(("near_2_64", ["t0", "c0"], _sparse(2, {(0, 5): (U64, U64), (0, 3775): (U64, U64 - 1), (0, 0): (U64 - 5, 0),
                                                        (1, 3000): (U64, U64), (1, 3001): (1, R.lo(3001))}), [1, -1]))
    out.append(("empty_sample", ["t0", "c0"], _sparse(2, {(1, 9): (4, 36)}), [1, -1]))     # n == 0: no row, every figure nan
    return out


@pytest.fixture(scope="module")
def cases():
    return _cases()


def _arrays(h):
    return np.array(h[0], dtype=np.uint64), np.array(h[1], dtype=np.uint64)


def test_the_reference_on_hand_made_cases(cases):
    by = {c[0]: c for c in cases}
    m = R.metrics(*by["one_class"][2], by["one_class"][3])[0]
    assert (m["zero_fraction"], m["auc"], m["gini"], m["elbow_bins"], m["elbow_gap"], m["jsd_control"]) == (0, Fraction(1, 2), 0, 1, 0, None)
    m = R.metrics(*by["only_zeros"][2], by["only_zeros"][3])
    assert m[0]["zero_fraction"] == 1 and m[0]["auc"] is None and m[0]["gini"] is None and m[0]["elbow_bins"] is None
    assert m[0]["jsd_control"] == 0.0 and m[1]["jsd_control"] is None
    assert R.metrics(*by["identical"][2], by["identical"][3])[0]["jsd_control"] == 0.0
    assert abs(R.metrics(*by["disjoint"][2], by["disjoint"][3])[0]["jsd_control"] - 1.0) < 1e-12
    m = R.metrics(*by["no_control"][2], by["no_control"][3])
    assert m[0]["jsd_control"] is None and 0 < m[1]["jsd_control"] < 1 and m[2]["jsd_control"] is None
    assert 0 < m[1]["gini"] < 1 and m[1]["elbow_gap"] > 0
    assert R.curve_text(by["only_zeros"][1], *by["only_zeros"][2]).splitlines()[1] == "t0\t0\t0\t1000\t0\t1.000000\tnan"
    # the Gini index by its textbook form over the values themselves, where no class holds two different values
    v = np.sort(np.random.default_rng(5).integers(0, 128, 400))
    g = R.metrics(*R.hist([v]))[0]["gini"]
    n, i = len(v), np.arange(1, len(v) + 1)
    mean_diff = Fraction(int((2 * i - n - 1).dot(v)) * 2, n * n)             # sum |x_i - x_j| / n^2
    assert g == mean_diff / (2 * Fraction(int(v.sum()), n))


def test_metrics_through_ctypes_against_the_reference(cases):
    from genrich_amd.lib import fingerprint_metrics
    for label, names, h, ctrl in cases:
        got = fingerprint_metrics(*_arrays(h), ctrl)
        for s, want in enumerate(R.metrics(*h, ctrl)):
            for f in R.FIGURES:
                if want[f] is None:
                    assert math.isnan(got[s][f]), (label, s, f)
                else:
                    assert abs(Fraction(float(got[s][f])) - Fraction(want[f])) <= Fraction(1, 10 ** 9), (label, s, f, got[s][f])
    c, t = _arrays(cases[0][2])
    for bad in ([0], [1], [5]):
        with pytest.raises(RuntimeError):
            fingerprint_metrics(c, t, bad)                      # its own control; no such sample


def test_format_through_ctypes_against_the_reference(cases):
    from genrich_amd.lib import format_fingerprint, format_fingerprint_metrics
    for label, names, h, ctrl in cases:
        assert R.check_curve(format_fingerprint(names, *_arrays(h)).decode(), names, *h) is None, label
        assert R.check_metrics(format_fingerprint_metrics(names, *_arrays(h), ctrl).decode(), names, *h, ctrl) is None, label
    by = {c[0]: c for c in cases}
    text = format_fingerprint_metrics(by["disjoint"][1], *_arrays(by["disjoint"][2]), by["disjoint"][3]).decode().splitlines()
    assert text[1].endswith("\t1.000000") and text[2].endswith("\tnan")
    text = format_fingerprint_metrics(by["identical"][1], *_arrays(by["identical"][2]), by["identical"][3]).decode().splitlines()
    assert text[1].endswith("\t0.000000")
    text = format_fingerprint_metrics(by["only_zeros"][1], *_arrays(by["only_zeros"][2]), by["only_zeros"][3]).decode().splitlines()
    assert text[1] == "t0\t1000\t1000\t0\t1.000000\tnan\tnan\tnan\tnan\t0.000000"
    text = format_fingerprint_metrics(by["near_2_64"][1], *_arrays(by["near_2_64"][2]), by["near_2_64"][3]).decode().splitlines()
    assert text[1].split("\t")[1:4] == [str(3 * U64 - 5), str(U64 - 5), str(2 * U64 - 1)]
    assert format_fingerprint(["a", "b"], *_arrays(by["empty_sample"][2])).decode().splitlines()[1:] == ["b\t9\t9\t4\t36\t1.000000\t1.000000"]


def test_the_check_itself_refuses_a_wrong_table(cases):
    label, names, h, ctrl = cases[2]
    good = R.curve_text(names, *h)
    assert R.check_curve(good, names, *h) is None
    lines = good.splitlines()
    f = lines[5].split("\t")
    for col, new in ((3, str(int(f[3]) + 1)), (5, f"{float(f[5]) + 2.1e-6:.6f}"), (6, "nan")):
        bad = lines[:5] + ["\t".join(f[:col] + [new] + f[col + 1:])] + lines[6:]
        assert R.check_curve("\n".join(bad) + "\n", names, *h) is not None, col
    assert R.check_curve("\n".join(lines[:-1]) + "\n", names, *h) is not None


def test_format_standalone_under_sanitizers(cases, tmp_path):
    """gx_emit.cpp's writers in a program of its own (its own main, tests/fingerprint_format_main.cpp), compiled with
    -fsanitize=address,undefined: any report makes the program fail (-fno-sanitize-recover, ASan aborts by default)."""
    exe = str(tmp_path / "fingerprint_format")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "fingerprint_format_main.cpp"),
                           os.path.join(ROOT, "genrich_amd", "csrc", "gx_emit.cpp"), "-o", exe])
    lines = []
    for label, names, (count, total), ctrl in cases:
        lines.append(str(len(names)))
        for s, name in enumerate(names):
            ks = [k for k in range(R.NC) if count[s][k]]
            lines.append(f"{name} {-1 if ctrl is None else ctrl[s]} {len(ks)}")
            lines += [f"{k} {count[s][k]} {total[s][k]}" for k in ks]
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join(lines) + "\n")
    res = subprocess.run([exe, str(spec)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
    parts = res.stdout.split("--\n")
    assert len(parts) == 2 * len(cases) + 1 and parts[-1] == ""
    for i, (label, names, h, ctrl) in enumerate(cases):
        assert R.check_curve(parts[2 * i], names, *h) is None, label
        assert R.check_metrics(parts[2 * i + 1], names, *h, ctrl) is None, label


# ---- the command line ------------------------------------------------------------------------------------------------------------

def test_cli_refusals_create_no_file(tmp_path):
    """Refused before any input is read: no GPU needed."""
    from genrich_amd import build

    binp = build.build_host()
    sam = tmp_path / "t.sam"
    sam.write_text("@SQ\tSN:chrA\tLN:1000\n")
    out, met, npk, ev = tmp_path / "fp.tsv", tmp_path / "fpm.tsv", tmp_path / "o.np", tmp_path / "ev.bed"
    t17 = ",".join([str(sam)] * 17)
    for extra, word in ((["-t", str(sam), "--fingerprint", str(out), "-P", "-f", str(tmp_path / "in.log")], "--fingerprint needs the pileups of this run"),
                        (["-t", str(sam), "--fingerprint", str(out), "--events-only", "-b", str(ev)], "--fingerprint needs the pileups of this run"),
                        (["-t", str(sam), "--fingerprint-metrics", str(met)], "--fingerprint-metrics needs --fingerprint FILE"),
                        (["-t", str(sam), "--fingerprint", str(out), "--bin-size", "0"], "--bin-size"),
                        (["-t", str(sam), "--fingerprint", str(out), "--coverage-scale", "2"], "--coverage"),
                        (["-t", ",".join([str(sam)] * 33), "--fingerprint", str(out), "--fingerprint-metrics", str(met)],
                         "--fingerprint takes at most 32 samples"),
                        (["-t", t17, "-c", ",".join([str(sam)] * 16), "--fingerprint", str(out)], "--fingerprint takes at most 32 samples")):
        res = subprocess.run([binp, "-o", str(npk)] + extra, capture_output=True, text=True)
        assert res.returncode == 1 and word in res.stderr, (extra, res.stderr)
        assert not out.exists() and not met.exists() and not npk.exists() and not ev.exists(), extra
    res = subprocess.run([binp, "-o", str(npk), "--fingerprint", str(out), "-t", t17, "-c", ",".join(["null"] * 16)], capture_output=True, text=True)
    assert "--fingerprint takes at most 32 samples" not in res.stderr   # 17 samples: the nulls are none
    res = subprocess.run([binp, "-o", str(npk), "--fingerprint", str(out), "--bin-size", "10", "-P", "-t", str(sam)], capture_output=True, text=True)
    assert "--bin-size and --coverage-scale need" not in res.stderr     # --bin-size is --fingerprint's too


def test_cli_help_names_the_options():
    from genrich_amd import build

    res = subprocess.run([build.build_host(), "-h"], capture_output=True, text=True)
    assert "--fingerprint FILE [--fingerprint-metrics FILE]" in res.stderr
