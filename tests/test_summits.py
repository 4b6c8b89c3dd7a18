"""The summits of the pooled treatment depth inside the peaks (gx_peak_summits, --summits) without a GPU: tests/summits_ref.py's
restatement over runs against its brute force, on random profiles and on the constructed cases the GPU tests use
(tests/summits_cases.py); the interior summits against scipy; gx_format_summits through ctypes against summits_text byte for
byte; the writer once more as a stand-alone program under AddressSanitizer / UBSan; the command line's refusals and help; the
geometry call.  Everything is an exact integer: ==."""
import os
import subprocess

import numpy as np
import pytest

import summits_cases as K
import summits_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _geometry():
    from genrich_amd.lib import peak_summits_geometry
    return peak_summits_geometry()


def test_the_geometry_call_answers_without_a_device():
    from genrich_amd.lib import peak_signal_geometry
    lanes, grid, step, runs, lmin, lper, most = _geometry()
    assert lanes % 64 == 0 and 64 <= lanes <= 1024 and 1 <= grid <= 65535
    assert step == peak_signal_geometry()[2] == 256                  # k_psig_reduce's loads: 4 bases per lane
    assert 64 <= runs and (lanes // 64) * runs * 12 <= 64 * 1024     # a workgroup's runs in LDS: well under a CU's 160 KiB
    assert lmin >= 1 and lper >= 1
    assert most == (1 << 31) // 120 - 1


def test_restatement_against_the_brute_force_on_random_profiles():
    rng = np.random.default_rng(23)
    for trial in range(400):
        L = int(rng.integers(1, 60))
        d = rng.integers(-2, 6, L) * 12 if trial % 2 else np.repeat(rng.integers(-1, 5, L), rng.integers(1, 4, L))[:L] * 20
        P, Rr = int(rng.choice([0, 10, 25, 50, 100])), int(rng.choice([0, 25, 50, 100]))
        assert R.of_depth(d, P, Rr) == R.brute_of_depth(d, P, Rr), (trial, d.tolist(), P, Rr)


def test_restatement_against_the_brute_force_on_the_constructed_cases():
    step = _geometry()[2]
    cases = K.constructed(step)
    for label, (lens, peaks, ev) in cases.items():
        for P, Rr in ((25, 50), (0, 0), (100, 100)):
            got, exp = R.summits([ev], lens, peaks, P, Rr), R.summits([ev], lens, peaks, P, Rr, of=R.brute_of_depth)
            assert R.same(got, exp) is None, (label, P, Rr, R.same(got, exp))
    u = K.UNIT
    lens, peaks, ev = cases["thresholds"]
    sm = R.summits([ev], lens, peaks)
    per = [[(int(r["pos"]), int(r["height"]), int(r["prominence"])) for r in sm[sm["peak"] == k]] for k in range(len(peaks))]
    assert per[0] == [(0, 8 * u, 8 * u), (2, 4 * u, u)]           # both rules hold with equality
    assert per[1] == [(0, 10 * u, 10 * u)] and per[2] == [(0, 9 * u, 9 * u)]   # one unit short of either
    assert per[3] == [(1, 4 * u, u), (3, 8 * u, 8 * u)]
    # 12 local maxima, 5 of them their peaks' highest; the other 7 have prominence 1 of height 4 or 5 -- P = 26 drops them all,
    # R = 51 too (none reaches 51 % of an 8, a 9 or a 10)
    assert [len(R.summits([ev], lens, peaks, p, r)) for p, r in ((25, 50), (26, 50), (25, 51), (0, 0), (100, 100), (100, 0), (0, 100))] == [
        10, 5, 5, 12, 5, 5, 5]
    lens, peaks, ev = cases["plateaus"]
    sm = R.summits([ev], lens, peaks)
    assert [(int(r["peak"]), int(r["pos"]), int(r["width"]), int(r["height"]), int(r["prominence"])) for r in sm] == [
        (0, 149, 300, 3 * u, 3 * u),                # the whole peak: the base is 0
        (1, 2, 6, 4 * u, 3 * u), (1, 106, 1, 3 * u, u),       # at the left edge: the right side alone; a small one over the 2s
        (2, 20, 1, 3 * u, u), (2, 124, 7, 4 * u, 3 * u),
        (3, 4, 3, 5 * u, 3 * u),
        (4, step - 1, 12, 4 * u, 3 * u), (4, step + 36, 2, 2 * u, u),
        (5, step + 2, 1, 5 * u, 3 * u),
        (6, 4, 5, 6 * u, 5 * u), (6, 11, 4, 6 * u, 5 * u),   # twins: an equal height does not end the other's walk
        (7, 13, 3, 5 * u, 4 * u)]                   # a staircase: one summit
    lens, peaks, ev = cases["negative"]
    sm = R.summits([ev], lens, peaks)
    assert [(int(r["peak"]), int(r["pos"]), int(r["height"]), int(r["prominence"])) for r in sm] == [
        (2, 1, 2 * u, 3 * u), (2, 3, u, 2 * u), (4, 1, u, u), (5, 2, 3 * u, 4 * u)]
    lens, peaks, ev = K.five()
    assert len(R.summits([ev], lens, peaks)) == 5
    lens, peaks, ev = K.limits(64, 1024)
    assert [int((R.summits([ev], lens, peaks)["peak"] == k).sum()) for k in range(8)] == [31, 32, 32, 500, 33, 512, 512, 1]   # (the fifth begins and ends high: 33 of its 65 runs)


def test_interior_summits_against_scipy():
    sig = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(29)
    for trial in range(300):
        L = int(rng.integers(3, 80))
        d = np.repeat(rng.integers(-2, 7, L), rng.integers(1, 4, L))[:L].astype(np.int64)
        idx, props = sig.find_peaks(d, plateau_size=1)
        prom = sig.peak_prominences(d, idx, wlen=None)[0]
        exp = {(int(i), int(r - l + 1), int(d[i]), int(p)) for i, l, r, p in zip(idx, props["left_edges"], props["right_edges"], prom) if d[i] > 0}
        got = {c for c in R.of_depth(d, 0, 0) if c[0] - (c[1] - 1) // 2 > 0 and c[0] - (c[1] - 1) // 2 + c[1] < L}
        assert got == exp, (trial, d.tolist())


def _text_cases():
    """(label, names, peaks, summits)"""
    def sm(rows):
        return np.array([(k, p, w, 0, h, pr) for k, p, w, h, pr in rows], dtype=R.SUMMIT_DTYPE) if rows else np.zeros(0, dtype=R.SUMMIT_DTYPE)
    two = [(0, 10, 40), (1, 0, 7), (1, 7, 9)]
    return [("none", ["chrA"], [], sm([])),
            ("peaks_without_summits", ["chrA", "chrB"], two, sm([])),
            ("fractional_and_large", ["chrA", "chr_B.1"], two,
             sm([(0, 0, 1, 120, 120), (0, 7, 4, 60, 7), (0, 29, 1, 2 ** 31 - 1, 2 ** 33), (2, 0, 2, 240, 1200)]))]


def test_format_through_ctypes_against_the_reference():
    from genrich_amd.lib import format_summits
    for label, names, peaks, sm in _text_cases():
        assert format_summits(names, peaks, sm).decode() == R.summits_text(names, peaks, sm), label
    _, names, peaks, sm = _text_cases()[2]
    lines = R.summits_text(names, peaks, sm).splitlines()
    assert lines[0] == R.HEADER and len(lines) == 5
    assert lines[1].split("\t") == ["chrA", "10", "11", "peak_0.1", "1", ".", "10", "11", "1", "10", "40"]
    assert lines[2].split("\t") == ["chrA", "17", "18", "peak_0.2", "0.50", ".", "16", "20", "0.06", "10", "40"]
    assert lines[3].split("\t")[3] == "peak_0.3" and lines[4].split("\t") == ["chr_B.1", "7", "8", "peak_2.1", "2", ".", "7", "9", "10", "7", "9"]
    with pytest.raises(RuntimeError):
        format_summits(names, peaks, sm[::-1])            # not ascending


def test_format_standalone_under_sanitizers(tmp_path):
    """gx_emit.cpp's writer in a program of its own (its own main, tests/summits_format_main.cpp), compiled with
    -fsanitize=address,undefined: any report makes the program fail (-fno-sanitize-recover, ASan aborts by default)."""
    exe = str(tmp_path / "summits_format")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "summits_format_main.cpp"),
                           os.path.join(ROOT, "genrich_amd", "csrc", "gx_emit.cpp"), "-o", exe])
    cases = _text_cases()
    lines = []
    for label, names, peaks, sm in cases:
        lines.append(f"{len(names)} {len(peaks)} {len(sm)}")
        lines += list(names)
        lines += [f"{c} {s} {e}" for c, s, e in peaks]
        lines += [f"{int(r['peak'])} {int(r['pos'])} {int(r['width'])} {int(r['height'])} {int(r['prominence'])}" for r in sm]
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join(lines) + "\n")
    res = subprocess.run([exe, str(spec)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
    parts = res.stdout.split("--\n")
    assert len(parts) == len(cases) + 1 and parts[-1] == R.HEADER + "\n"   # (the program's own last call: no summit)
    for part, (label, names, peaks, sm) in zip(parts, cases):
        assert part == R.summits_text(names, peaks, sm), label


# ---- the command line ------------------------------------------------------------------------------------------------------------

def test_cli_refusals_create_no_file(tmp_path):
    """Refused before any input is read: no GPU needed."""
    from genrich_amd import build

    binp = build.build_host()
    sam = tmp_path / "t.sam"
    sam.write_text("@SQ\tSN:chrA\tLN:1000\n")
    out, npk, ev = tmp_path / "summits.tsv", tmp_path / "o.np", tmp_path / "ev.bed"
    for extra in (["-t", str(sam), "-o", str(npk), "-X", "-f", str(tmp_path / "x.log")],
                  ["-P", "-f", str(tmp_path / "in.log"), "-o", str(npk)],
                  ["-t", str(sam), "--events-only", "-b", str(ev)]):
        res = subprocess.run([binp, "--summits", str(out)] + extra, capture_output=True, text=True)
        assert res.returncode == 1, (extra, res.stderr)
        assert "--summits needs the peaks and the intervals of this run (not with -X, -P or --events-only)" in res.stderr, (extra, res.stderr)
        assert not out.exists() and not npk.exists() and not ev.exists(), extra
    for extra, text in ((["--summits", str(out), "--summits-prominence", "101"], "--summits-prominence takes an integer in [0, 100]"),
                        (["--summits", str(out), "--summits-height", "-1"], "--summits-height takes an integer in [0, 100]"),
                        (["--summits", str(out), "--summits-height", "5x"], "--summits-height takes an integer in [0, 100]"),
                        (["--summits-prominence", "10"], "--summits-prominence and --summits-height need --summits FILE"),
                        (["--summits-height", "10"], "--summits-prominence and --summits-height need --summits FILE")):
        res = subprocess.run([binp, "-t", str(sam), "-o", str(npk)] + extra, capture_output=True, text=True)
        assert res.returncode == 1 and text in res.stderr, (extra, res.stderr)
        assert not out.exists() and not npk.exists(), extra


def test_cli_help_summits_names_the_options_and_h_is_unchanged():
    from genrich_amd import build

    binp = build.build_host()
    res = subprocess.run([binp, "--help-summits"], capture_output=True, text=True)
    assert res.returncode == 1 and res.stdout == ""
    for word in ("--summits FILE", "--summits-prominence PCT", "--summits-height PCT", "(25; 0 .. 100)", "(50;"):
        assert word in res.stderr, word
    h = subprocess.run([binp, "-h"], capture_output=True, text=True)
    assert h.returncode == res.returncode and "--summits" not in h.stderr
    assert h.stderr == open(os.path.join(ROOT, "tests", "host_usage.txt")).read()
