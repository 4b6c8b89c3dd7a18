"""Each sample's signal inside the peaks (gx_peak_signal, --peak-signal) without a GPU: tests/peaksig_ref.py's restatement
against its brute force, on random small cases and on the constructed cases the GPU tests use (tests/peaksig_cases.py);
gx_format_peak_signal through ctypes against peak_signal_text byte for byte; the writer once more as a stand-alone program
under AddressSanitizer / UBSan; the command line's refusals; the geometry call.  Everything is an exact integer: ==."""
import os
import subprocess

import numpy as np
import pytest

import backends as B
import peaksig_cases as K
import peaksig_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _geometry():
    from genrich_amd.lib import peak_signal_geometry
    return peak_signal_geometry()


def test_the_geometry_call_answers_without_a_device():
    lanes, grid, step, pad, most = _geometry()
    assert lanes % 64 == 0 and 64 <= lanes <= 1024 and 1 <= grid <= 65535
    assert pad == 4 and step == 64 * pad                      # one 16-byte load per lane, a wavefront per peak
    assert most == (1 << 31) // 120 - 1 and most * 120 < 1 << 31     # n >= 2^31 / 120 is refused; below it every depth fits 31 bits


def test_restatement_against_the_brute_force_on_random_cases():
    rng = np.random.default_rng(17)
    for trial in range(30):
        lens = [int(rng.integers(1, 400)) for _ in range(int(rng.integers(1, 4)))]
        n = int(rng.integers(0, 120))
        ev = np.zeros(n, dtype=B.EVENT_DTYPE)
        ev["chrom"] = rng.integers(0, len(lens) + 1, n)                      # (one beyond the table)
        ev["start"] = rng.integers(0, 420, n)                                # (starts at and beyond the length)
        span = rng.integers(0, 90, n)
        ev["end"] = np.where(rng.random(n) < 0.15, np.maximum(ev["start"].astype(np.int64) - span, 0), ev["start"].astype(np.int64) + span)
        ev["count"] = rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], n)
        peaks = []
        for c, ln in enumerate(lens):
            cuts = np.unique(rng.integers(0, ln + 1, int(rng.integers(0, 9))))
            peaks += [(c, int(a), int(b)) for a, b in zip(cuts[:-1:2], cuts[1::2])] if len(cuts) > 1 else []
        if trial % 3 == 0:                                                   # adjacent peaks, a whole chromosome
            peaks = [(0, 0, lens[0] // 2), (0, lens[0] // 2, lens[0])] if lens[0] > 1 else [(0, 0, 1)]
        so = [int(rng.integers(0, e - s)) for _, s, e in peaks]
        active = None if trial % 4 else [bool(c % 2 == 0) for c in range(len(lens))]
        got, exp = R.signal(ev, lens, peaks, so, active), R.brute(ev, lens, peaks, so, active)
        assert R.same(got, exp) is None, (trial, R.same(got, exp))


def test_restatement_against_the_brute_force_on_the_constructed_cases():
    step = _geometry()[2]
    for label, lens, peaks, so, ev in K.small_cases(step):
        got, exp = R.signal(ev, lens, peaks, so), R.brute(ev, lens, peaks, so)
        assert R.same(got, exp) is None, (label, R.same(got, exp))
    by = {c[0]: c for c in K.small_cases(step)}
    _, lens, peaks, so, ev = by["plateaus"]
    sig = R.signal(ev, lens, peaks, so)
    assert sig.summit.tolist() == [10, 3 * step - 1, step - 1, step - 1, 0, 2 * step - 1, 0]
    assert sig.max.tolist() == [240, 70, 24, 20, -15, 12, 0] and sig.covered.tolist() == [21, 3 * step, 1, 4, 0, 2, 0]
    assert sig.at_summit.tolist() == [240, 70, 24, 20, -15, -120, 0] and sig.area[4] == -15 * 3 * step
    _, lens, peaks, so, ev = by["edges"]
    sig = R.signal(ev, lens, peaks, so)
    assert sig.at_summit[4] >= 120 + 60 + 40 + 24 and (sig.covered[:5] > 0).all()   # the clamped intervals reach the last base
    assert {int(c) for c in ev["count"]} >= set(K.COUNTS)


def _text_cases():
    """(label, names, peaks, [Signal])"""
    a = np.array
    two = [(0, 10, 20), (1, 0, 7)]
    t0 = R.Signal(a([1200, 7]), a([240, 60]), a([3, 0]), a([10, 1]), a([120, 1]), 0, False)
    c0 = R.Signal(a([-15, 0]), a([0, -40]), a([0, 6]), a([0, 0]), a([-15, -7]), 0, True)
    t1 = R.Signal(a([2 ** 40 * 120 + 60, 119]), a([2 ** 31 - 1, 121]), a([9, 5]), a([10, 7]), a([-(2 ** 31), -120]), 1, False)
    empty = R.Signal(*(np.zeros(0, dtype=np.int64) for _ in range(5)), 0, False)
    return [("no_peaks", ["chrA"], [], [empty, empty._replace(rep=1, is_ctrl=True)]),
            ("no_samples", ["chrA", "chrB"], two, []),
            ("neither", ["chrA"], [], []),
            ("fractional_negative_control", ["chrA", "chr_B.1"], two, [t0, c0, t1])]


def test_format_through_ctypes_against_the_reference():
    from genrich_amd.lib import PeakSignal, format_peak_signal
    for label, names, peaks, samples in _text_cases():
        got = format_peak_signal(names, peaks, [PeakSignal(*s) for s in samples]).decode()
        assert got == R.peak_signal_text(names, peaks, samples), label
    by = {c[0]: c for c in _text_cases()}
    _, names, peaks, samples = by["fractional_negative_control"]
    lines = R.peak_signal_text(names, peaks, samples).splitlines()
    assert lines[0].split("\t")[4:9] == ["t0.max", "t0.summit", "t0.area", "t0.covered", "t0.at_summit"] and lines[0].split("\t")[9] == "c0.max"
    assert lines[1].split("\t")[:9] == ["chrA", "10", "20", "peak_0", "2", "3", "10", "10", "1"]
    assert lines[2].split("\t")[4:14] == ["0.50", "0", "0.06", "1", "0.01", "-0.33", "6", "0", "0", "-0.06"]
    assert lines[1].split("\t")[9:14] == ["0", "0", "-0.12", "0", "-0.12"]
    assert R.peak_signal_text(["chrA"], [], []) == "chr\tstart\tend\tname\n"


def test_format_standalone_under_sanitizers(tmp_path):
    """gx_emit.cpp's writer in a program of its own (its own main, tests/peak_signal_format_main.cpp), compiled with
    -fsanitize=address,undefined: any report makes the program fail (-fno-sanitize-recover, ASan aborts by default)."""
    exe = str(tmp_path / "peak_signal_format")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "peak_signal_format_main.cpp"),
                           os.path.join(ROOT, "genrich_amd", "csrc", "gx_emit.cpp"), "-o", exe])
    cases = _text_cases()
    lines = []
    for label, names, peaks, samples in cases:
        lines.append(f"{len(names)} {len(peaks)} {len(samples)}")
        lines += list(names)
        lines += [f"{c} {s} {e}" for c, s, e in peaks]
        for sm in samples:
            lines.append(f"{sm.rep} {int(sm.is_ctrl)}")
            lines += [f"{int(sm.area[k])} {int(sm.max[k])} {int(sm.summit[k])} {int(sm.covered[k])} {int(sm.at_summit[k])}" for k in range(len(peaks))]
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join(lines) + "\n")
    res = subprocess.run([exe, str(spec)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
    parts = res.stdout.split("--\n")
    assert len(parts) == len(cases) + 1 and parts[-1] == "chr\tstart\tend\tname\n"   # (the program's own last call: neither peaks nor samples)
    for part, (label, names, peaks, samples) in zip(parts, cases):
        assert part == R.peak_signal_text(names, peaks, samples), label


# ---- the command line ------------------------------------------------------------------------------------------------------------

def test_cli_refusals_create_no_file(tmp_path):
    """Refused before any input is read: no GPU needed."""
    from genrich_amd import build

    binp = build.build_host()
    sam = tmp_path / "t.sam"
    sam.write_text("@SQ\tSN:chrA\tLN:1000\n")
    out, npk, ev = tmp_path / "sig.tsv", tmp_path / "o.np", tmp_path / "ev.bed"
    for extra in (["-t", str(sam), "-o", str(npk), "-X", "-f", str(tmp_path / "x.log")],
                  ["-P", "-f", str(tmp_path / "in.log"), "-o", str(npk)],
                  ["-t", str(sam), "--events-only", "-b", str(ev)]):
        res = subprocess.run([binp, "--peak-signal", str(out)] + extra, capture_output=True, text=True)
        assert res.returncode == 1, (extra, res.stderr)
        assert "--peak-signal needs the peaks and the intervals of this run (not with -X, -P or --events-only)" in res.stderr, (extra, res.stderr)
        assert not out.exists() and not npk.exists() and not ev.exists(), extra


def test_cli_help_names_the_option():
    from genrich_amd import build

    res = subprocess.run([build.build_host(), "-h"], capture_output=True, text=True)
    assert "--peak-signal FILE" in res.stderr
