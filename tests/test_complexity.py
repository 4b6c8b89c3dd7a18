"""Library complexity's figures and text writers (gx_complexity_metrics, gx_format_complexity*) without a GPU: through ctypes
against tests/complexity_ref.py's exact numbers, the writers once more as a stand-alone program under AddressSanitizer / UBSan,
and the command line's refusals.

Tolerances (derived, not tuned).  NRF, PBC1, PBC2 and the duplicate fraction are each ONE division of two exact integers below
2^53: the correctly rounded double, compared with ==.  A curve point is a sum of K non-negative terms h[m] (1 - p); p is a
product of m quotients of exact integers, so its relative error is at most 2 m ulp, and 1 - p >= n / N >= 0.05 turns that into
at most 20 * 2 m ulp of the term; the sum adds K ulp: (40 m_max + K) 2^-53 < 2 * 10^-11 for m_max = 4096, K = 100 even in double
(the library works in long double).  Asserted: 10^-10 relative.  The library size: on inputs with a duplicate fraction of at
least 1 % and N <= 10^7 the root's error is far below one observation (g'(X) ~ u^2 / 2 with u = N / X >= 0.02, g evaluated to
a few ulp of N); asserted: the reference's root, bracketed at 60 digits, lies within 1 of the integer given."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import complexity_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_hist(rng):
    """At most 100 classes, multiplicities at most 4096, N <= 10^7, a duplicate fraction of at least 1 %."""
    while True:
        K = int(rng.integers(1, 101))
        ms = np.sort(rng.choice(np.arange(1, 4097), size=K, replace=False))
        pairs = []
        budget = 10 ** 7
        for m in ms.tolist():
            top = min(budget // m, 20000 if m < 8 else 30)
            if top < 1:
                break
            k = int(rng.integers(1, top + 1))
            pairs.append((m, k))
            budget -= m * k
        N, D = sum(m * k for m, k in pairs), sum(k for _, k in pairs)
        if (N - D) * 100 >= N:
            return pairs


def _sample(pairs, rep=0, ctrl=False):
    return (rep, ctrl, sum(m * k for m, k in pairs), sum(k for _, k in pairs), pairs)


def _cases():
    """(label, [(rep, is_ctrl, N, D, pairs)])"""
    rng = np.random.default_rng(23)
    out = [("all_unique", [_sample([(1, 5000)])]),
           ("all_one_key", [_sample([(977, 1)])]),
           ("no_pairs_seen_twice", [_sample([(1, 900), (3, 40), (17, 2)])]),
           ("nothing", [_sample([]), _sample([(1, 3), (2, 1)], 0, True)]),
           ("one_heavy_key", [_sample([(1, 100_000), (4096, 1)])]),
           ("typical", [_sample([(1, 800_000), (2, 90_000), (3, 9000), (4, 1000), (5, 80), (9, 3)], 0),
                        _sample([(1, 500_000), (2, 7000), (3, 100)], 0, True),
                        _sample([(1, 10), (2, 10)], 1)])]
    for i in range(6):
        out.append((f"random{i}", [_sample(_random_hist(rng), i, bool(i & 1))]))
    return out


@pytest.fixture(scope="module")
def cases():
    return _cases()


def test_the_reference_on_hand_made_cases():
    N, D, pairs = R.histogram(["a", "b", "a", "c", "a", "b"])
    assert (N, D, pairs) == (6, 3, [(1, 1), (2, 1), (3, 1)])
    f = R.figures(N, D, pairs)
    assert (f["nrf"], f["pbc1"], f["pbc2"], f["dup_fraction"]) == (Fraction(1, 2), Fraction(1, 3), 1, Fraction(1, 2))
    assert f["curve"][-1] == D and R.curve_depth(6, 10) == 3
    # E_3 by the definition over all C(6, 3) = 20 draws of three of the six observations
    from itertools import combinations
    obs = ["a", "b", "a", "c", "a", "b"]
    want = Fraction(sum(len({obs[i] for i in c}) for c in combinations(range(6), 3)), 20)
    assert abs(f["curve"][9] - want) < Fraction(1, 1 << 200)
    lo, hi = f["library_size"]
    assert abs(3 / float(lo) - (1 - math.exp(-6 / float(lo)))) < 1e-12
    assert R.figures(5, 5, [(1, 5)])["library_size"] is None and R.figures(0, 0, [])["nrf"] is None
    ev = np.zeros(7, dtype=[("chrom", "<u4"), ("start", "<u4"), ("end", "<u4"), ("count", "<u4")])
    ev["chrom"] = [0, 0, 1, 0, 0, 2, 1]
    ev["start"] = [5, 5, 5, 99, 100, 1, 5]
    ev["end"] = [150, 120, 150, 50, 120, 9, 10]
    ev["count"] = [1, 2, 1, 1, 1, 1, 7]
    # chromosome 0: both ends clamp to 100 (one key, whatever the count); an interval that ends before it starts; start >= len;
    # an unknown chromosome; an invalid count
    assert R.of_events(ev, [100, 200]) == (4, 3, [(1, 2), (2, 1)])
    assert R.of_events(ev, [100, 200], active=[1, 0]) == (3, 2, [(1, 1), (2, 1)])


def test_geometry():
    from genrich_amd.lib import CPX_CURVE, GX_PATH_COMPLEXITY, complexity_geometry
    lanes, grid, bound, cap = complexity_geometry(0)
    assert lanes % 64 == 0 and grid >= 1 and bound >= 2 and cap >= 2 and CPX_CURVE == R.CURVE and GX_PATH_COMPLEXITY == 1 << 23
    for n in (1, 2, 3, 63, 64, 65, 65535, 65536, 65537, (1 << 31) - 1):
        cap = complexity_geometry(n)[3]
        assert cap & (cap - 1) == 0 and cap >= 2 * n and (cap // 2 < 2 * n or cap == 2), n
    assert complexity_geometry(1 << 31)[3] == 0


def test_metrics_through_ctypes_against_the_reference(cases):
    from genrich_amd.lib import complexity_metrics
    for label, samples in cases:
        for rep, ctrl, N, D, pairs in samples:
            got, want = complexity_metrics(N, D, pairs), R.figures(N, D, pairs)
            assert (int(got["h1"]), int(got["h2"])) == (want["h1"], want["h2"]), label
            for f in R.RATIOS:
                if want[f] is None:
                    assert math.isnan(got[f]), (label, f)
                else:
                    assert float(got[f]) == float(want[f]), (label, f, got[f])      # the correctly rounded double
            if want["library_size"] is None:
                assert math.isnan(got["library_size"]), label
            else:
                assert N <= 10 ** 7 and (N - D) * 100 >= N, label                  # where the bound above was derived
                lo, hi = want["library_size"]
                x = float(got["library_size"])
                assert x == int(x) and lo - 1 <= int(x) <= hi + 1, (label, x, lo)
            for k, E in enumerate(want["curve"]):
                assert abs(Fraction(float(got["curve"][k])) - E) <= E / 10 ** 10, (label, k, got["curve"][k], float(E))
            assert float(got["curve"][-1]) == D, label                              # E_N = D exactly
    for bad in ((3, 2, [(2, 1), (1, 1)]), (4, 2, [(1, 1), (2, 1)]), (3, 3, [(1, 1), (2, 1)]), (3, 2, [(0, 1), (3, 1)]), (3, 2, [(1, 1), (1, 1)])):
        with pytest.raises(RuntimeError):
            complexity_metrics(*bad)


def test_format_through_ctypes_against_the_reference(cases):
    from genrich_amd.lib import format_complexity, format_complexity_hist
    for label, samples in cases:
        assert R.check_metrics(format_complexity(samples).decode(), samples) is None, label
        assert format_complexity_hist(samples).decode() == R.hist_text(samples), label
    by = dict(cases)
    row = format_complexity(by["all_unique"]).decode().splitlines()[1].split("\t")
    assert row[:10] == ["t0", "5000", "5000", "5000", "0", "1.000000", "1.000000", "NA", "0.000000", "NA"]
    assert row[10:] == [f"{250 * k}.000" for k in range(1, 21)]
    rows = format_complexity(by["nothing"]).decode().splitlines()
    assert rows[1].split("\t") == ["t0", "0", "0", "0", "0", "NA", "NA", "NA", "NA", "NA"] + ["0.000"] * 20
    assert rows[2].split("\t")[:9] == ["c0", "5", "4", "3", "1", "0.800000", "0.750000", "3.000000", "0.200000"]
    row = format_complexity(by["all_one_key"]).decode().splitlines()[1].split("\t")
    assert row[:10] == ["t0", "977", "1", "0", "0", f"{1 / 977:.6f}", "0.000000", "NA", f"{976 / 977:.6f}", "1"] and row[10:] == ["1.000"] * 20
    assert format_complexity_hist(by["nothing"]).decode() == "sample\tmultiplicity\tkeys\nc0\t1\t3\nc0\t2\t1\n"


def test_the_check_itself_refuses_a_wrong_table(cases):
    label, samples = cases[5]
    from genrich_amd.lib import format_complexity
    good = format_complexity(samples).decode()
    assert R.check_metrics(good, samples) is None
    lines = good.splitlines()
    f = lines[1].split("\t")
    for col, new in ((1, str(int(f[1]) + 1)), (5, f"{float(f[5]) + 1e-6:.6f}"), (7, "NA"), (9, str(int(f[9]) + 3)), (12, f"{float(f[12]) + 0.002:.3f}")):
        bad = [lines[0], "\t".join(f[:col] + [new] + f[col + 1:])] + lines[2:]
        assert R.check_metrics("\n".join(bad) + "\n", samples) is not None, col
    assert R.check_metrics("\n".join(lines[:-1]) + "\n", samples) is not None


def test_format_standalone_under_sanitizers(cases, tmp_path):
    """gx_emit.cpp's writers in a program of its own (its own main, tests/complexity_format_main.cpp), compiled with
    -fsanitize=address,undefined: any report makes the program fail (-fno-sanitize-recover, ASan aborts by default)."""
    exe = str(tmp_path / "complexity_format")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "complexity_format_main.cpp"),
                           os.path.join(ROOT, "genrich_amd", "csrc", "gx_emit.cpp"), "-o", exe])
    lines = []
    for label, samples in cases:
        lines.append(str(len(samples)))
        for rep, ctrl, N, D, pairs in samples:
            lines.append(f"{rep} {int(ctrl)} {N} {D} {len(pairs)}")
            lines += [f"{m} {k}" for m, k in pairs]
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join(lines) + "\n")
    res = subprocess.run([exe, str(spec)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
    parts = res.stdout.split("--\n")
    assert len(parts) == 2 * len(cases) + 1 and parts[-1] == ""
    for i, (label, samples) in enumerate(cases):
        assert R.check_metrics(parts[2 * i], samples) is None, label
        assert parts[2 * i + 1] == R.hist_text(samples), label


# ---- the command line ------------------------------------------------------------------------------------------------------------

def test_cli_refusals_create_no_file(tmp_path):
    """Refused before any input is read: no GPU needed."""
    from genrich_amd import build

    binp = build.build_host()
    sam = tmp_path / "t.sam"
    sam.write_text("@SQ\tSN:chrA\tLN:1000\n")
    out, hist, npk, ev = tmp_path / "cpx.tsv", tmp_path / "cpxh.tsv", tmp_path / "o.np", tmp_path / "ev.bed"
    for extra, word in ((["-t", str(sam), "--complexity", str(out), "--events-only", "-b", str(ev)], "--complexity needs the intervals of this run"),
                        (["-t", str(sam), "--complexity", str(out), "--complexity-hist", str(hist), "-P", "-f", str(tmp_path / "in.log")],
                         "--complexity needs the intervals of this run"),
                        (["-t", str(sam), "--complexity-hist", str(hist)], "--complexity-hist needs --complexity FILE")):
        res = subprocess.run([binp, "-o", str(npk)] + extra, capture_output=True, text=True)
        assert res.returncode == 1 and word in res.stderr, (extra, res.stderr)
        assert not out.exists() and not hist.exists() and not npk.exists() and not ev.exists(), extra


def test_cli_help_names_the_options():
    from genrich_amd import build

    res = subprocess.run([build.build_host(), "-h"], capture_output=True, text=True)
    assert "--complexity FILE [--complexity-hist FILE]" in res.stderr
