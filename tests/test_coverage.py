"""The binned coverage's definition (tests/coverage_ref.py) and its text writer (gx_format_coverage), without a GPU: the numpy
reference against a brute-force loop, against the reference binary's own -k pileups of the golden fixtures, and the C writer
against the Python one -- through ctypes, and once more as a stand-alone program under AddressSanitizer / UBSan."""
import os
import subprocess

import numpy as np
import pytest

import backends as B
import coverage_ref as R
import golden_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_against_brute_force():
    rng = np.random.default_rng(5)
    lens = [3 * 4096 + 17, 37, 900]
    n = 200
    ev = np.zeros(n, dtype=B.EVENT_DTYPE)
    ev["chrom"] = rng.integers(0, len(lens), n)
    ln = np.asarray(lens)[ev["chrom"]]
    ev["start"] = rng.integers(0, ln + 3)                      # (a few at or beyond the length: left out)
    ev["end"] = ev["start"] + rng.integers(0, 700, n)         # (empty ones, and ends beyond the length: clamped)
    ev["count"] = rng.choice([1, 1, 1, 2, 3, 4, 5, 6, 8, 10, 7, 0], n)   # (7 and 0: no valid count, left out)
    assert (ev["start"] >= ln).any() and (ev["end"] > ln).any() and (~np.isin(ev["count"], R.VALID_COUNTS)).any()
    for W in (1, 7, 50, 4096, 5000):
        got, exp = R.coverage(ev, lens, W), R.coverage_brute(ev, lens, W)
        assert sorted(got) == sorted(exp) == [0, 1, 2]
        for c in got:
            assert got[c].dtype == np.int64 and np.array_equal(got[c], exp[c]), (W, c)
            assert len(got[c]) == -(-lens[c] // W)
    # -E bases count 0; a skipped or un-owned chromosome has no bins, one the header does not list has zero bins
    cov = R.coverage(ev, lens, 10, skip=[0, 1, 0], beds=[[0, 55, 4090, 4100], [], []], save=[1, 1, 0])
    assert sorted(cov) == [0, 2] and not cov[2].any()
    pile = R.pileup120(ev, 0, lens[0])
    pile[0:55] = 0
    pile[4090:4100] = 0
    assert np.array_equal(cov[0], R.bin_sums(pile, 10))


def _unit_single_cases():
    out = []
    for name in G.case_names():
        if G.read_gz(name, "out.pile") is None or G.read_gz(name, "events.bed") is None:
            continue
        meta, case, _, _ = G.load_case(name)
        if len(case["replicates"]) == 1 and (case["replicates"][0]["treat"]["count"] == 1).all():
            out.append(name)
    return out


def _pile_integral(name, names, lens):
    """Per-base treatment pileup (1/120 units) from the `experimental` column of the reference's -k file."""
    idx = {n: i for i, n in enumerate(names)}
    pile = {c: np.zeros(lens[c], dtype=np.int64) for c in range(len(lens))}
    for line in G.read_gz(name, "out.pile").decode().splitlines():
        if line.startswith("#") or line.startswith("chr\tstart"):
            continue
        f = line.split("\t")
        v = float(f[3])
        assert v == round(v)   # unit weights
        pile[idx[f[0]]][int(f[1]):int(f[2])] = int(round(v)) * 120
    return pile


@pytest.mark.parametrize("name", _unit_single_cases())
def test_definition_is_the_reference_binarys_pileup(name):
    meta, case, _, names = G.load_case(name)
    rep = case["replicates"][0]
    pile = _pile_integral(name, names, case["lens"])
    for W in (7, 50, 4096):
        cov = R.coverage(rep["treat"], case["lens"], W, skip=case["skip"], beds=case["beds"], save=rep["save"])
        for c, length in enumerate(case["lens"]):
            if case["skip"][c] or length == 0:
                assert c not in cov and not pile[c].any()
            else:
                assert np.array_equal(cov[c], R.bin_sums(pile[c], W)), (name, W, c)


def test_some_golden_case_ties_the_definition_to_the_reference():
    names = _unit_single_cases()
    assert "basic" in names and any("bedx" in n for n in names), names


# hand-made arrays: (name, len, W, sums, scale)
def _format_cases():
    return [
        ("zero", 1000, 50, [0] * 20, 1.0),                                   # all zero: one line
        ("lastmerges", 130, 50, [120 * 50 * 3, 120 * 50 * 3, 120 * 30 * 3], 1.0),   # a short last bin with its neighbour's mean
        ("lastnot", 130, 50, [120 * 50 * 3, 120 * 50 * 3, 120 * 30 * 3 + 1], 1.0),  # ... and one that differs by 1/120
        ("frac", 100, 10, [0, 40, 40, 1200, 1201, 7, 7, 7, 0, 0], 1.0),      # non-integer means
        ("scaled", 100, 10, [0, 1200, 1200, 2400, 40, 40, 0, 0, 0, 12], 0.1),    # scale != 1: no integer form
        ("scaled1e6", 64, 16, [120 * 16 * 5, 3, 3, 120 * 16], 1e6 / 12345678.0),
        ("single", 37, 4096, [120 * 37 * 2], 1.0),                           # one bin per chromosome
        ("single_frac", 37, 65536, [121], 1.0),
        ("one_base_bins", 5, 1, [120, 120, 0, 60, 60], 1.0),
        ("big", 3 * (1 << 20), 1 << 20, [(1 << 31) * (1 << 20) * 1, (1 << 31) * (1 << 20) * 1, (1 << 31) * 1000], 1.0),  # near 2^51
        ("negative", 40, 10, [-1200, -1200, -5, 0], 1.0),
    ]


def test_format_through_ctypes_against_the_python_writer():
    from genrich_amd.lib import format_coverage
    for name, length, W, sums, scale in _format_cases():
        got = format_coverage(name, length, W, np.asarray(sums, dtype=np.int64), scale).decode()
        assert got == R.format_chrom(name, length, W, sums, scale), name
        rows = [l.split("\t") for l in got.splitlines()]
        assert int(rows[0][1]) == 0 and int(rows[-1][2]) == length
        assert all(int(a[2]) == int(b[1]) for a, b in zip(rows, rows[1:]))   # the lines tile [0, len)
    assert format_coverage("zero", 1000, 50, np.zeros(20, dtype=np.int64)) == b"zero\t0\t1000\t0\n"
    assert format_coverage("lastmerges", 130, 50, np.asarray(_format_cases()[1][3])) == b"lastmerges\t0\t130\t3\n"
    assert format_coverage("f", 20, 10, np.asarray([40, 41])) == b"f\t0\t10\t0.0333\nf\t10\t20\t0.0342\n"
    with pytest.raises(RuntimeError):
        format_coverage("x", 10, 5, np.asarray([1]))   # n_bins != ceil(len / bin_size)


def test_format_standalone_under_sanitizers(tmp_path):
    """gx_emit.cpp's writer in a program of its own (its own main, tests/coverage_format_main.cpp), compiled with
    -fsanitize=address,undefined: any report makes the program fail (-fno-sanitize-recover, ASan aborts by default)."""
    exe = str(tmp_path / "coverage_format")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "coverage_format_main.cpp"),
                           os.path.join(ROOT, "genrich_amd", "csrc", "gx_emit.cpp"), "-o", exe])
    cases = _format_cases()
    spec = tmp_path / "spec.txt"
    spec.write_text("".join(f"{n} {ln} {W} {scale!r} {len(s)} {' '.join(str(x) for x in s)}\n" for n, ln, W, s, scale in cases))
    res = subprocess.run([exe, str(spec)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
    each, whole = res.stdout.split("--\n")
    assert each == "".join(R.format_chrom(n, ln, W, s, scale) for n, ln, W, s, scale in cases)
    assert whole == "".join(R.format_chrom(n, ln, W, s, cases[0][4]) for n, ln, W, s, _ in cases)
