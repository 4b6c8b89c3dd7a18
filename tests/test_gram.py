"""The correlation matrix's text writer (gx_format_correlation) without a GPU: through ctypes against tests/gram_ref.py's exact
arithmetic, once more as a stand-alone program under AddressSanitizer / UBSan, and the command line's refusals."""
import os
import subprocess

import numpy as np
import pytest

import gram_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _names(S):
    return [f"t{i // 2}" if i % 2 == 0 else f"c{i // 2}" for i in range(S)]


def _cancellation_rows(seed):
    """2^20 values of 2^50 + noise, noise below 2^10: N g and s_i s_j agree in their first ~80 bits.  Two independent rows (r
    near 0) and one that follows the first (r near 0.7)."""
    rng = np.random.default_rng(seed)
    n = 1 << 20
    a, b = rng.integers(0, 1 << 10, n), rng.integers(0, 1 << 10, n)
    c = (a + rng.integers(0, 1 << 10, n)) // 2
    return [(1 << 50) + a, (1 << 50) + b, (1 << 50) + c]


CANCELLATION_SEEDS = (11, 12)


def _cases():
    """(label, rows, skip_zeros)"""
    rng = np.random.default_rng(7)
    out = []
    for S in (1, 2, 5, 32):
        base = rng.integers(0, 1 << 20, 200)
        rows = [np.where(rng.random(200) < 0.3, 0, base * rng.integers(1, 4) + rng.integers(0, 1 << 18, 200)) for _ in range(S)]
        out.append((f"random{S}", rows, False))
        out.append((f"random{S}_skip", rows, True))
    x = rng.integers(0, 1 << 30, 300)
    y = rng.integers(0, 1 << 30, 300)
    out.append(("identical", [x, x.copy()], False))
    out.append(("times_constant", [x, 12345 * x], False))
    out.append(("mirror", [x, x.max() - x], False))
    out.append(("constant_sample", [x, np.full(300, 777), y], False))
    out.append(("all_zero_sample", [x, np.zeros(300, dtype=np.int64), y], False))
    out.append(("one_bin", [x[:1], y[:1]], False))                                   # N < 2
    sparse = [np.concatenate([x[:1], np.zeros(9, dtype=np.int64)]), np.concatenate([y[:1], np.zeros(9, dtype=np.int64)])]
    out.append(("one_live_bin", sparse, False))                                      # N = 10: r = 1
    out.append(("one_live_bin_skip", sparse, True))                                  # N = 1: nan
    z = np.where(rng.random(300) < 0.8, 0, 1)                                        # four bins in five are 0 in both
    zx, zy = z * x, z * rng.integers(0, 1 << 30, 300)
    out.append(("mostly_zero", [zx, zy], False))
    out.append(("mostly_zero_skip", [zx, zy], True))
    big = [(1 << 51) - 1 - rng.integers(0, 1 << 40, 500), (1 << 51) - 1 - rng.integers(0, 1 << 40, 500)]   # sums near 2^111
    out.append(("near_the_bound", big, False))
    for seed in CANCELLATION_SEEDS:
        out.append((f"cancellation{seed}", _cancellation_rows(seed), False))
    return out


@pytest.fixture(scope="module")
def cases():
    """(label, names, (n, n_zero, sum, gram), skip_zeros, expected text): the sums are computed once."""
    out = []
    for label, rows, skip in _cases():
        g = R.gram(rows)
        names = _names(len(rows))
        out.append((label, names, g, skip, R.correlation_text(names, *g, skip)))
    return out


def _matrix(text):
    return [l.split("\t")[1:] for l in text.splitlines()[1:]]


def test_the_reference_on_hand_made_cases(cases):
    by = {c[0]: c for c in cases}
    assert _matrix(by["identical"][4]) == [["1.000000", "1.000000"]] * 2
    assert _matrix(by["times_constant"][4]) == [["1.000000", "1.000000"]] * 2
    assert _matrix(by["mirror"][4]) == [["1.000000", "-1.000000"], ["-1.000000", "1.000000"]]
    for label in ("constant_sample", "all_zero_sample"):
        m = _matrix(by[label][4])
        assert m[1] == ["nan", "1.000000", "nan"] and m[0][1] == m[2][1] == "nan" and m[0][2] not in ("nan", "1.000000")
    assert _matrix(by["one_bin"][4]) == [["1.000000", "nan"], ["nan", "1.000000"]]
    assert _matrix(by["one_live_bin"][4]) == [["1.000000", "1.000000"]] * 2
    assert _matrix(by["one_live_bin_skip"][4]) == [["1.000000", "nan"], ["nan", "1.000000"]]
    assert by["mostly_zero"][2][1] > 200 and _matrix(by["mostly_zero"][4]) != _matrix(by["mostly_zero_skip"][4])
    assert by["random5"][4].splitlines()[0] == "\tt0\tc0\tt1\tc1\tt2"
    # r by numpy's floats where floats are good enough
    rows = _cases()[4][1]
    want = np.corrcoef(np.asarray(rows, dtype=np.float64))
    got = np.asarray([[float(v) for v in row] for row in _matrix(by["random5"][4])])
    assert np.abs(want - got).max() < 1e-6


def test_the_cancellation_cases_are_what_they_claim(cases):
    """N g and s_i s_j agree in their leading ~80 bits (a double would be wrong from the first digit), and no value lies within
    1e-9 of a boundary of its %.6f text: the last bit of a sqrt cannot decide the comparison."""
    for label, names, g, skip, text in cases:
        if not label.startswith("cancellation"):
            continue
        n, nz, s, gr = g
        N, cov = R.differences(n, nz, s, gr)
        assert (N * gr[0][1]).bit_length() >= 140 and (N * gr[0][1]).bit_length() - abs(cov[0][1]).bit_length() >= 70
        assert R.min_boundary_distance(n, nz, s, gr) > 1e-9, label
        m = _matrix(text)
        assert abs(float(m[0][1])) < 0.01 and 0.6 < float(m[0][2]) < 0.8
        fl = float(N) * float(gr[0][1]) - float(s[0]) * float(s[1])     # the same step in doubles
        assert abs(fl - cov[0][1]) >= abs(cov[0][1])                     # (an error as large as the value)


def test_format_through_ctypes_against_the_reference(cases):
    from genrich_amd.lib import format_correlation
    for label, names, (n, nz, s, g), skip, text in cases:
        assert format_correlation(names, n, nz, s, g, skip).decode() == text, label
    with pytest.raises(RuntimeError):
        format_correlation(["a"], 1, 2, [1], [[1]], True)   # n_zero > n


def test_format_standalone_under_sanitizers(cases, tmp_path):
    """gx_emit.cpp's writer in a program of its own (its own main, tests/gram_format_main.cpp), compiled with
    -fsanitize=address,undefined: any report makes the program fail (-fno-sanitize-recover, ASan aborts by default)."""
    exe = str(tmp_path / "gram_format")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "gram_format_main.cpp"),
                           os.path.join(ROOT, "genrich_amd", "csrc", "gx_emit.cpp"), "-o", exe])
    w = lambda v: f"{v >> 64:x} {v & 0xFFFFFFFFFFFFFFFF:x}"
    lines = []
    for label, names, (n, nz, s, g), skip, text in cases:
        lines.append(f"{len(names)} {n} {nz} {int(skip)}")
        lines += [f"{nm} {w(v)}" for nm, v in zip(names, s)]
        lines += [w(v) for row in g for v in row]
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join(lines) + "\n")
    res = subprocess.run([exe, str(spec)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
    assert res.stdout == "".join(c[4] + "--\n" for c in cases)


def test_cli_refusals_create_no_file(tmp_path):
    """Refused before any input is read: no GPU needed."""
    from genrich_amd import build

    binp = build.build_host()
    sam = tmp_path / "t.sam"
    sam.write_text("@SQ\tSN:chrA\tLN:1000\n")
    out, npk, ev = tmp_path / "corr.tsv", tmp_path / "o.np", tmp_path / "ev.bed"
    for extra, word in ((["--correlation", str(out), "-P", "-f", str(tmp_path / "in.log")], "--correlation needs the pileups of this run"),
                        (["--correlation", str(out), "--events-only", "-b", str(ev)], "--correlation needs the pileups of this run"),
                        (["--corr-skip-zeros"], "--correlation"),
                        (["--correlation", str(out), "--bin-size", "0"], "--bin-size"),
                        (["--correlation", str(out), "--bin-size", "1048577"], "--bin-size"),
                        (["--correlation", str(out), "--coverage-scale", "2"], "--coverage"),
                        (["--bin-size", "10"], "--bin-size and --coverage-scale need --coverage PREFIX")):
        res = subprocess.run([binp, "-t", str(sam), "-o", str(npk)] + extra, capture_output=True, text=True)
        assert res.returncode == 1 and word in res.stderr, (extra, res.stderr)
        assert not out.exists() and not npk.exists() and not ev.exists(), extra


def test_cli_help_names_the_option():
    from genrich_amd import build

    res = subprocess.run([build.build_host(), "-h"], capture_output=True, text=True)
    assert "--correlation FILE [--corr-skip-zeros]" in res.stderr


def test_the_matrix_as_doubles_and_the_geometry(cases):
    from genrich_amd.lib import correlation_matrix, gram_geometry
    for label, names, (n, nz, s, g), skip, text in cases:
        r = correlation_matrix(n, nz, s, g, skip)
        want = [[float("nan") if v == "nan" else float(v) for v in row] for row in _matrix(text)]
        assert np.array_equal(np.isnan(r), np.isnan(want)), label
        assert np.nanmax(np.abs(r - np.asarray(want))) <= 5.0000001e-7, label
    tile, lanes, grid = gram_geometry()
    assert tile >= 2 and lanes % 64 == 0 and grid >= 1


def test_cli_refuses_more_than_32_samples_before_anything_is_written(tmp_path):
    from genrich_amd import build

    sam = tmp_path / "t.sam"
    sam.write_text("@SQ\tSN:chrA\tLN:1000\n")
    out, npk = tmp_path / "corr.tsv", tmp_path / "o.np"
    t17 = ",".join([str(sam)] * 17)
    for extra in (["-t", ",".join([str(sam)] * 33)], ["-t", t17, "-c", ",".join([str(sam)] * 16)]):
        res = subprocess.run([build.build_host(), "-o", str(npk), "--correlation", str(out)] + extra, capture_output=True, text=True)
        assert res.returncode == 1 and "--correlation takes at most 32 samples" in res.stderr, res.stderr
        assert not out.exists() and not npk.exists()
    res = subprocess.run([build.build_host(), "-o", str(npk), "--correlation", str(out), "-t", t17, "-c", ",".join(["null"] * 16)],
                         capture_output=True, text=True)
    assert "--correlation takes at most 32 samples" not in res.stderr   # 17 samples: the nulls are none
