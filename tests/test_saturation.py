"""The subsample's draw, the saturation table's overlap walk and its writer without a GPU (gx_subsample_draw,
gx_saturation_overlap, gx_format_saturation, gx_saturation_thresholds): through ctypes against tests/saturation_ref.py, the walk
and the writer once more as a stand-alone program under AddressSanitizer / UBSan, and the command line's refusals.

The kept share's bound: 10^6 draws kept with probability p = T / 2^32 ~ 0.1 are binomial with sd sqrt(p (1 - p) / 10^6) = 3 * 10^-4;
asserted: within 4 sd, 1.2 * 10^-3, of p."""
import os
import subprocess

import numpy as np
import pytest

import saturation_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPT = -3      # GX_ERR_EXPT


def _peaks(rows):
    from genrich_amd.lib import PEAK_DTYPE
    pk = np.zeros(len(rows), dtype=PEAK_DTYPE)
    for i, (c, s, e) in enumerate(rows):
        pk[i]["chrom"], pk[i]["start"], pk[i]["end"] = c, s, e
    return pk


def _random_list(rng, n_chrom=3):
    """A peak list in get_peaks() order: by chromosome, then start; disjoint, some abutting."""
    rows = []
    for c in range(n_chrom):
        pos = int(rng.integers(0, 50))
        for _ in range(int(rng.integers(0, 12))):
            start = pos + int(rng.choice([0, 0, 1, 5, 40]))         # (0: abuts the one before)
            end = start + int(rng.integers(1, 60))
            rows.append((c, start, end))
            pos = end
    return rows


HAND = [([], []),
        ([(0, 10, 20)], []),
        ([], [(0, 10, 20)]),
        ([(0, 10, 20)], [(0, 20, 30)]),                                   # abutting: no overlap
        ([(0, 10, 20), (0, 20, 30)], [(0, 0, 10), (0, 30, 40)]),          # ... on both sides
        ([(0, 10, 20)], [(0, 19, 21)]),                                   # one base
        ([(0, 0, 1000)], [(0, 10, 20), (0, 30, 40), (0, 999, 2000)]),     # one of the run's peaks spans several
        ([(0, 10, 20), (0, 30, 40), (0, 50, 60)], [(0, 0, 100)]),         # ... and the other way round
        ([(0, 10, 20), (1, 10, 20)], [(1, 10, 20), (2, 10, 20)]),         # different chromosomes
        ([(0, 10, 20), (2, 10, 20)], [(1, 0, 100)]),
        ([(0, 10, 20), (0, 25, 35), (1, 5, 9)], [(0, 15, 30), (1, 0, 6), (1, 8, 12)])]


@pytest.fixture(scope="module")
def lists():
    rng = np.random.default_rng(7)
    return HAND + [(_random_list(rng), _random_list(rng)) for _ in range(50)]


def test_the_reference_on_hand_made_cases():
    assert R.overlap(_peaks([(0, 10, 20)]), _peaks([(0, 20, 30)])) == (0, 0, 0)
    assert R.overlap(_peaks([(0, 0, 1000)]), _peaks([(0, 10, 20), (0, 30, 40), (0, 999, 2000)])) == (1, 3, 21)
    assert R.overlap(_peaks([(0, 10, 20), (1, 10, 20)]), _peaks([(1, 10, 20), (2, 10, 20)])) == (1, 1, 10)
    assert R.thresholds(3) == [1431655765, 2863311530, 1 << 32]
    assert R.draw(0, 0, 0) == int(R.draws(0, 0, [0])[0]) and 0 <= R.draw(5, 1, 9) < 1 << 32


def test_draw_through_ctypes_against_the_mirror():
    from genrich_amd.lib import load_library
    lib = load_library()
    rng = np.random.default_rng(3)
    n = 100_000
    seeds = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    samples = rng.integers(0, 32, n)
    index = rng.integers(0, 1 << 41, n, dtype=np.uint64)
    got = np.array([lib.gx_subsample_draw(int(s), int(k), int(i)) for s, k, i in zip(seeds, samples, index)], dtype=np.uint64)
    want = np.array([R.draw(s, k, i) for s, k, i in zip(seeds.tolist(), samples.tolist(), index.tolist())], dtype=np.uint64)
    assert np.array_equal(got, want)
    for seed in (0, (1 << 64) - 1):
        for k in (0, 31):
            idx = np.array([0, 1 << 40], dtype=np.uint64)
            vec = R.draws(seed, k, idx)
            for j, i in enumerate((0, 1 << 40)):
                assert lib.gx_subsample_draw(seed, k, i) == R.draw(seed, k, i) == int(vec[j]), (seed, k, i)
    # the vectorised mirror is the scalar one
    idx = np.arange(5000, dtype=np.uint64)
    assert np.array_equal(R.draws(12345, 3, idx), np.array([R.draw(12345, 3, i) for i in range(5000)], dtype=np.uint64))


def test_kept_share_nestedness_and_the_two_ends():
    from genrich_amd.lib import load_library
    lib = load_library()
    n = 1_000_000
    d = R.draws(1, 0, np.arange(n, dtype=np.uint64))
    assert all(lib.gx_subsample_draw(1, 0, i) == int(d[i]) for i in range(0, n, 997))
    T = (1 << 32) // 10
    share = float((d < np.uint64(T)).sum()) / n
    print("kept share at a tenth:", share)
    assert abs(share - 0.1) <= 1.2e-3
    t1, t2 = (3 << 32) // 10, (4 << 32) // 10
    k1, k2 = R.keep_mask(n, 1, 0, t1), R.keep_mask(n, 1, 0, t2)
    assert k1.sum() < k2.sum() and not (k1 & ~k2).any()                  # every event kept at 30 % is kept at 40 %
    assert not R.keep_mask(n, 1, 0, 0).any() and R.keep_mask(n, 1, 0, R.FULL).all()
    assert not np.array_equal(R.keep_mask(n, 1, 0, t1), R.keep_mask(n, 1, 1, t1))   # the sample matters
    assert not np.array_equal(R.keep_mask(n, 1, 0, t1), R.keep_mask(n, 2, 0, t1))   # ... and the seed


def test_thresholds_are_the_integer_formula():
    from genrich_amd.lib import saturation_thresholds
    for n in (1, 3, 10, 100):
        got = saturation_thresholds(n)
        assert got == [(j << 32) // n for j in range(1, n + 1)] == R.thresholds(n) and got[-1] == 1 << 32
    for n in (0, 101, -1):
        with pytest.raises(RuntimeError):
            saturation_thresholds(n)


def test_overlap_through_ctypes_against_brute_force(lists):
    from genrich_amd.lib import saturation_overlap
    seen = set()
    for full, sub in lists:
        f, s = _peaks(full), _peaks(sub)
        want = R.overlap(f, s)
        assert saturation_overlap(f, s) == want, (full, sub)
        a, b, c = saturation_overlap(s, f)                # the walk is symmetric
        assert (b, a, c) == want
        seen.add(want[0] > 0)
    assert seen == {False, True}
    assert saturation_overlap(_peaks(HAND[6][0]), _peaks(HAND[6][1])) == (1, 3, 21)
    assert saturation_overlap(_peaks(HAND[3][0]), _peaks(HAND[3][1])) == (0, 0, 0)


def _table():
    from genrich_amd.lib import SAT_POINT_DTYPE
    pts = np.zeros(3, dtype=SAT_POINT_DTYPE)
    pts["threshold"] = [1, (1 << 32) // 2, 1 << 32]
    pts["n_total"] = 1000
    pts["n_kept"] = [0, 497, 1000]
    pts["n_peaks"] = [0, 7, 12]
    pts["peak_bp"] = [0, 2100, 4800]
    pts["genome_len"] = [0, 5_000_000, 5_000_000]
    pts["status"] = [EXPT, 0, 0]
    return pts, [0, 6, 12], [0, 7, 12], [0, 2000, 4800]


GOLDEN = ("# run: 12 peaks, 4800 bp\n"
          "fraction\tthreshold\tkept\tpeaks\tpeak_bp\trecovered\trecovered_share\tin_run\tshared_bp\tstatus\n"
          "0.000000\t1\t0\t0\t0\t0\t0.000000\t0\t0\tno_fragments\n"
          "0.500000\t2147483648\t497\t7\t2100\t6\t0.500000\t7\t2000\tok\n"
          "1.000000\t4294967296\t1000\t12\t4800\t12\t1.000000\t12\t4800\tok\n")


def test_format_gives_the_golden_text():
    from genrich_amd.lib import format_saturation
    pts, rec, inr, bp = _table()
    assert format_saturation(pts, rec, inr, bp, 12, 4800).decode() == GOLDEN
    none = format_saturation(pts[:1], [0], [0], [0], 0, 0).decode().splitlines()
    assert none[0] == "# run: 0 peaks, 0 bp" and none[2].split("\t")[6] == "NA"
    with pytest.raises(RuntimeError):
        format_saturation(pts[:0], [], [], [], 0, 0)


def test_format_and_walk_standalone_under_sanitizers(lists, tmp_path):
    """gx_emit.cpp's walk and writer in a program of its own (its own main, tests/saturation_format_main.cpp), compiled with
    -fsanitize=address,undefined: any report makes the program fail (-fno-sanitize-recover, ASan aborts by default)."""
    exe = str(tmp_path / "saturation_format")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "saturation_format_main.cpp"),
                           os.path.join(ROOT, "genrich_amd", "csrc", "gx_emit.cpp"), "-o", exe])
    lines = []
    for full, sub in lists:
        lines.append(f"O {len(full)} {len(sub)}")
        lines += [f"{c} {s} {e}" for c, s, e in full + sub]
    pts, rec, inr, bp = _table()
    lines.append(f"F {len(pts)} 12 4800")
    for p, r, i, b in zip(pts, rec, inr, bp):
        lines.append(" ".join(str(int(p[k])) for k in ("threshold", "n_total", "n_kept", "n_peaks", "peak_bp", "genome_len", "status")) + f" {r} {i} {b}")
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join(lines) + "\n")
    res = subprocess.run([exe, str(spec)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
    out = res.stdout.splitlines(keepends=True)
    assert len(out) == len(lists) + GOLDEN.count("\n") + 1
    for line, (full, sub) in zip(out, lists):
        assert tuple(int(x) for x in line.split()) == R.overlap(_peaks(full), _peaks(sub)), (full, sub)
    assert "".join(out[len(lists):]) == GOLDEN + "--\n"


# ---- the command line ------------------------------------------------------------------------------------------------------------

def test_cli_refusals_create_no_file(tmp_path):
    """Refused before any input is read: no GPU needed."""
    from genrich_amd import build

    binp = build.build_host()
    sam = tmp_path / "t.sam"
    sam.write_text("@SQ\tSN:chrA\tLN:1000\n")
    out, npk, ev, log = tmp_path / "sat.tsv", tmp_path / "o.np", tmp_path / "ev.bed", tmp_path / "in.log"
    needs = "--saturation needs the peaks and the intervals of this run"
    for extra, word in ((["-t", str(sam), "--saturation", str(out), "-X"], needs),
                        (["-t", str(sam), "--saturation", str(out), "-P", "-f", str(log)], needs),
                        (["-t", str(sam), "--saturation", str(out), "--events-only", "-b", str(ev)], needs),
                        (["-t", str(sam), "--saturation", str(out), "--devices", "0,1"], "--saturation takes one device"),
                        (["-t", str(sam), "--saturation", str(out), "--devices", "0,0"], "--saturation takes one device"),
                        (["-t", str(sam), "--saturation", str(out), "--saturation-steps", "0"], "--saturation-steps must be in [1, 100]"),
                        (["-t", str(sam), "--saturation", str(out), "--saturation-steps", "101"], "--saturation-steps must be in [1, 100]"),
                        (["-t", str(sam), "--saturation-steps", "5"], "need --saturation FILE"),
                        (["-t", str(sam), "--saturation-seed", "5"], "need --saturation FILE"),
                        (["-t", str(sam), "--saturation", str(out), "--saturation-seed", "-1"], "--saturation-seed takes an integer"),
                        (["-t", str(sam), "--saturation", str(out), "--saturation-seed", "18446744073709551616"], "--saturation-seed takes an integer"),
                        (["-t", str(sam), "--saturation", str(out), "--saturation-seed", "7x"], "--saturation-seed takes an integer"),
                        (["-t", str(sam), "--saturation-controls"], "need --saturation FILE")):
        res = subprocess.run([binp, "-o", str(npk)] + extra, capture_output=True, text=True)
        assert res.returncode == 1 and word in res.stderr, (extra, res.stderr)
        assert not out.exists() and not npk.exists() and not ev.exists(), extra


def test_cli_help_names_the_options():
    from genrich_amd import build

    res = subprocess.run([build.build_host(), "-h"], capture_output=True, text=True)
    assert "--saturation FILE [--saturation-steps N] [--saturation-seed S] [--saturation-controls]" in res.stderr
