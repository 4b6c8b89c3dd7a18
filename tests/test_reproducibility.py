"""--reproducibility's support predicate, figures and writers without a GPU (gx_peaks_supported, gx_reproducibility_figures,
gx_format_reproducibility, gx_format_reproducibility_metrics, gx_format_narrowpeak): through ctypes against the brute force of
tests/reproducibility_ref.py, the golden text of both writers, everything once more as a stand-alone program under
AddressSanitizer / UBSan, and the command line's refusals and help."""
import os
import subprocess

import numpy as np
import pytest

import reproducibility_ref as R
from test_saturation import _peaks, _random_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPT = -3      # GX_ERR_EXPT

# (a, b, pct, hit of a): the edges of the predicate
EDGES = [([(0, 10, 20)], [(0, 20, 30)], 0, [0]),                                   # abutting: ov = 0, no support even at 0 %
         ([(0, 10, 20)], [(0, 0, 10)], 0, [0]),
         ([(0, 10, 20)], [(0, 19, 40)], 0, [1]),                                   # one base: touches
         ([(0, 10, 20)], [(0, 19, 40)], 1, [1]),                                   # ... 100 * 1 >= 1 * 10
         ([(0, 10, 20)], [(0, 19, 40)], 11, [0]),                                  # ... 100 * 1 < 11 * 10
         ([(0, 0, 200)], [(0, 199, 400)], 1, [0]),                                 # one base of 200 at 1 %: 100 < 200
         ([(0, 0, 100)], [(0, 50, 400)], 50, [1]),                                 # exactly half of the shorter
         ([(0, 0, 100)], [(0, 51, 400)], 50, [0]),                                 # ... one base less
         ([(0, 0, 101)], [(0, 51, 400)], 50, [0]),                                 # odd length: 50 of 101 is less than half
         ([(0, 0, 101)], [(0, 50, 400)], 50, [1]),
         ([(0, 0, 1000)], [(0, 100, 150)], 100, [1]),                              # containment: the shorter lies inside
         ([(0, 100, 150)], [(0, 0, 1000)], 100, [1]),
         ([(0, 0, 1000)], [(0, 960, 1010)], 100, [0]),                             # ... sticks out by ten bases
         ([(0, 0, 1000)], [(0, 960, 1010)], 80, [1]),
         ([(0, 10, 20), (1, 10, 20)], [(2, 10, 20)], 0, [0, 0]),                   # only a peak on another chromosome
         ([(1, 10, 20)], [(0, 10, 20), (2, 10, 20)], 0, [0]),
         ([], [], 50, []), ([], [(0, 1, 2)], 50, []), ([(0, 1, 2)], [], 50, [0]),  # empty lists
         ([(0, 0, 10_000)], [(0, 100 * k, 100 * k + 10) for k in range(90)], 100, [1]),          # one long peak over many short ones
         ([(0, 100 * k, 100 * k + 10) for k in range(90)], [(0, 0, 10_000)], 100, [1] * 90),
         ([(0, 0, 10_000), (0, 10_000, 10_050)], [(0, 100 * k, 100 * k + 10) for k in range(90)] + [(0, 9_990, 10_040)], 90, [1, 0]),
         ([(0, 0, 2_000_000_000)], [(0, 1_000_000_000, 3_000_000_000)], 50, [1]),  # 100 * ov beyond 32 bits
         ([(0, 0, 2_000_000_000)], [(0, 1_000_000_001, 3_000_000_000)], 50, [0])]


@pytest.fixture(scope="module")
def lists():
    rng = np.random.default_rng(11)
    return [(_random_list(rng), _random_list(rng)) for _ in range(60)]


def test_the_reference_on_hand_made_cases():
    for a, b, pct, want in EDGES:
        assert [int(x) for x in R.supported(_peaks(a), _peaks(b), pct)] == want, (a, b, pct)


def test_supported_through_ctypes_against_brute_force(lists):
    from genrich_amd.lib import peaks_supported
    for a, b, pct, want in EDGES:
        assert peaks_supported(_peaks(a), _peaks(b), pct).tolist() == want, (a, b, pct)
    seen = set()
    for a, b in lists:
        for pct in (0, 1, 25, 50, 75, 100):
            pa, pb = _peaks(a), _peaks(b)
            want = [int(x) for x in R.supported(pa, pb, pct)]
            assert peaks_supported(pa, pb, pct).tolist() == want, (a, b, pct)
            seen.update(want)
        hits = [int(peaks_supported(_peaks(a), _peaks(b), pct).sum()) for pct in (0, 50, 100)]
        assert hits[0] >= hits[1] >= hits[2]                    # a stricter overlap supports no more
    assert seen == {0, 1}
    for bad in (-1, 101):
        with pytest.raises(RuntimeError):
            peaks_supported(_peaks([(0, 1, 2)]), _peaks([(0, 1, 2)]), bad)


# ---- the figures ---------------------------------------------------------------------------------------------------------

def _grid(n, at=0, step=1000, width=100, chrom=0):
    """n peaks of `width` bases, one every `step`."""
    return [(chrom, at + step * k, at + step * k + width) for k in range(n)]


def _cases():
    """name -> (run, lists in the library's order)."""
    rng = np.random.default_rng(5)
    run = _grid(12)
    c = {}
    # one replicate: every ratio NA
    c["r1"] = (run, [run, _grid(9), _grid(10, at=20), _grid(11), _grid(8, at=50)])
    # two replicates, all well: Nt = 8, Np = 10, N_self = 7 / 6
    c["r2_pass"] = (run, [_grid(10), _grid(8, at=10), _grid(8), _grid(7, at=5), _grid(7, at=10), _grid(6, at=20), _grid(11), _grid(10, at=30)])
    # a zero minimum: the second replicate's halves share nothing with it
    c["r2_zero"] = (run, [_grid(10), _grid(8, at=10), _grid(8), _grid(7), _grid(3, at=500), _grid(3, at=600), _grid(11), _grid(10)])
    # ratios of exactly 2: Nt = 5, Np = 10; N_self = 8 / 4 -- not below 2, so both fail
    c["r2_exactly_two"] = (run, [_grid(10), _grid(5), _grid(8), _grid(9), _grid(5), _grid(4), _grid(10), _grid(11)])
    # ... and one base short of it: Np = 9 < 2 * 5 while N_self stays 8 / 4: borderline
    c["r2_borderline"] = (run, [_grid(10), _grid(5), _grid(8), _grid(9), _grid(5), _grid(4), _grid(9), _grid(11)])
    # three replicates: three pairs, the best one is (t1, t3); Np below Nt: the optimal set is the conservative one
    c["r3"] = (run, [_grid(11), _grid(4), _grid(9, at=40), _grid(9), _grid(9), _grid(4), _grid(3), _grid(8, at=40), _grid(7, at=40), _grid(8), _grid(6)])
    # a tie of Np and Nt goes to the conservative set, whose members differ from the pooled set's
    c["r2_tie"] = (run, [_grid(6), _grid(12), _grid(6), _grid(6), _grid(9), _grid(9), [run[k] for k in range(6, 12)], _grid(12)])
    # an empty run, and random lists on three chromosomes
    c["r2_empty_run"] = ([], [_grid(3), _grid(2), _grid(3), _grid(1), _grid(2), _grid(2), [], _grid(1)])
    for k in range(6):
        c[f"random{k}"] = (_random_list(rng), [_random_list(rng) for _ in range(3 * (1 + k % 3) + 2)])
    return c


def _library(run, lists, pct):
    from genrich_amd.lib import repro_calls, reproducibility_figures
    Rn = (len(lists) - 2) // 3
    calls = repro_calls(Rn, n_peaks=[len(l) for l in lists])
    return calls, reproducibility_figures(_peaks(run), calls, [_peaks(l) for l in lists], pct)


@pytest.mark.parametrize("name", sorted(_cases()))
def test_figures_through_ctypes_against_the_reference(name):
    from genrich_amd.lib import REPRO_VERDICTS, format_reproducibility_metrics
    run, lists = _cases()[name]
    for pct in (0, 50, 100):
        want = R.figures(_peaks(run), [_peaks(l) for l in lists], pct)
        _, got = _library(run, lists, pct)
        fig = got["fig"]
        assert got["nt_pair"].tolist() == want["nt_pair"] and got["n_self"].tolist() == want["n_self"], (name, pct)
        assert got["in_run"].tolist() == want["in_run"] and got["run_supported"].tolist() == want["run_supported"]
        assert (int(fig["np"]), int(fig["n_rep"])) == (want["np"], want["R"])
        if want["R"] > 1:
            assert (int(fig["nt"]), (int(fig["best_i"]), int(fig["best_j"]))) == (want["nt"], want["best"])
        else:
            assert (int(fig["best_i"]), int(fig["best_j"])) == (-1, -1)
        assert REPRO_VERDICTS[int(fig["verdict"])] == want["verdict"], (name, pct)
        for ratio, na in (("rescue", "rescue_na"), ("self_consistency", "self_na")):
            assert bool(fig[na]) == (want[ratio] is None)
            if want[ratio] is not None:
                assert float(fig[ratio]) == want[ratio]                  # one division of the same two integers
        assert got["conservative"].tolist() == [int(x) for x in want["conservative"]]
        assert got["optimal"].tolist() == [int(x) for x in want["optimal"]]
        assert (int(fig["n_conservative"]), int(fig["n_optimal"])) == (sum(want["conservative"]), sum(want["optimal"]))
        assert format_reproducibility_metrics(got).decode() == R.metrics_text(want)


def test_the_cases_are_what_their_names_say():
    c = _cases()
    f = {k: R.figures(_peaks(c[k][0]), [_peaks(l) for l in c[k][1]], 50) for k in c}
    assert f["r1"]["verdict"] == "NA" and f["r1"]["rescue"] is None and f["r1"]["self_consistency"] is None and f["r1"]["nt_pair"] == []
    assert (f["r2_pass"]["nt"], f["r2_pass"]["np"], f["r2_pass"]["n_self"], f["r2_pass"]["verdict"]) == (8, 10, [7, 6], "pass")
    assert f["r2_zero"]["n_self"][1] == 0 and f["r2_zero"]["verdict"] == "NA" and f["r2_zero"]["rescue"] is not None
    assert (f["r2_exactly_two"]["rescue"], f["r2_exactly_two"]["self_consistency"], f["r2_exactly_two"]["verdict"]) == (2.0, 2.0, "fail")
    assert f["r2_borderline"]["rescue"] == 1.8 and f["r2_borderline"]["self_consistency"] == 2.0 and f["r2_borderline"]["verdict"] == "borderline"
    assert len(f["r3"]["nt_pair"]) == 3 and f["r3"]["best"] == (0, 2) and f["r3"]["nt_pair"] == [4, 9, 4]
    assert f["r3"]["np"] < f["r3"]["nt"] and f["r3"]["optimal"] == f["r3"]["conservative"]
    assert f["r2_tie"]["np"] == f["r2_tie"]["nt"] == 6 and f["r2_tie"]["optimal"] == f["r2_tie"]["conservative"] == [True] * 6 + [False] * 6
    assert f["r2_pass"]["optimal"] != f["r2_pass"]["conservative"]          # Np > Nt: the pooled set


# ---- golden text ---------------------------------------------------------------------------------------------------------

def _golden_input():
    run, lists = _cases()["r2_pass"]
    n_events = [1000, 800, 497, 503, 391, 409, 888, 912]
    status = [0] * 8
    lists = list(lists)
    lists[5], n_events[5], status[5] = [], 0, EXPT              # a half with no fragment
    return run, lists, n_events, [100 * len(l) for l in lists], status


GOLDEN_CALLS = ("# run: 12 peaks, 1200 bp; overlap 50 %; seed 7\n"
                "call\trep\thalf\tintervals\tpeaks\tpeak_bp\tin_run\trun_supported\tstatus\n"
                "t1\t1\tNA\t1000\t10\t1000\t10\t10\tok\n"
                "t2\t2\tNA\t800\t8\t800\t8\t8\tok\n"
                "t1.pr1\t1\t1\t497\t8\t800\t8\t8\tok\n"
                "t1.pr2\t1\t2\t503\t7\t700\t7\t7\tok\n"
                "t2.pr1\t2\t1\t391\t7\t700\t7\t7\tok\n"
                "t2.pr2\t2\t2\t0\t0\t0\t0\t0\tno_fragments\n"
                "pooled.pr1\tNA\t1\t888\t11\t1100\t11\t11\tok\n"
                "pooled.pr2\tNA\t2\t912\t10\t1000\t10\t10\tok\n")
GOLDEN_METRICS = ("figure\tvalue\n"
                  "replicates\t2\n"
                  "Nt.t1.t2\t8\n"
                  "Nt\t8\n"
                  "Np\t10\n"
                  "N_self.t1\t7\n"
                  "N_self.t2\t0\n"
                  "rescue_ratio\t1.250000\n"
                  "self_consistency_ratio\tNA\n"
                  "verdict\tNA\n"
                  "conservative_peaks\t8\n"
                  "optimal_peaks\t10\n")
GOLDEN_R1 = ("figure\tvalue\nreplicates\t1\nNt\tNA\nNp\t8\nN_self.t1\t9\nrescue_ratio\tNA\nself_consistency_ratio\tNA\nverdict\tNA\n"
             "conservative_peaks\tNA\noptimal_peaks\t8\n")
GOLDEN_NARROWPEAK = "chrA\t10\t20\tpeak_7\t1000\t.\t30.000000\t2.000000\t-1\t15\nchrA\t40\t90\tpeak_8\t1000\t.\t100.000000\t3.000000\t1.500000\t60\n"


def test_writers_give_the_golden_text():
    from genrich_amd.lib import (PEAK_DTYPE, format_narrowpeak, format_reproducibility, format_reproducibility_metrics, repro_calls, repro_label,
                                 reproducibility_figures)
    run, lists, n_events, bp, status = _golden_input()
    calls = repro_calls(2, n_events=n_events, n_peaks=[len(l) for l in lists], peak_bp=bp, status=status)
    got = reproducibility_figures(_peaks(run), calls, [_peaks(l) for l in lists], 50)
    assert format_reproducibility(calls, got["in_run"], got["run_supported"], 12, 1200, 50, 7).decode() == GOLDEN_CALLS
    assert format_reproducibility_metrics(got).decode() == GOLDEN_METRICS
    assert [repro_label(c) for c in calls] == R.labels(2) == [l.split("\t")[0] for l in GOLDEN_CALLS.splitlines()[2:]]
    r1_run, r1_lists = _cases()["r1"]
    _, r1 = _library(r1_run, r1_lists, 50)
    assert format_reproducibility_metrics(r1).decode() == GOLDEN_R1
    two = np.zeros(2, dtype=PEAK_DTYPE)
    two[0] = (0, 10, 20, 15, 30.0, 2.0, -1.0)
    two[1] = (0, 40, 90, 60, 100.0, 3.0, 1.5)
    assert format_narrowpeak(two, ["chrA"], first_index=7).decode() == GOLDEN_NARROWPEAK
    assert format_narrowpeak(two[:0], ["chrA"]).decode() == ""


def test_everything_standalone_under_sanitizers(lists, tmp_path):
    """gx_emit.cpp's walk, figures and writers in a program of its own (its own main, tests/reproducibility_format_main.cpp),
    compiled with -fsanitize=address,undefined: any report makes the program fail (-fno-sanitize-recover, ASan aborts by default)."""
    exe = str(tmp_path / "reproducibility_format")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "reproducibility_format_main.cpp"),
                           os.path.join(ROOT, "genrich_amd", "csrc", "gx_emit.cpp"), "-o", exe])
    walks = [(a, b, pct) for a, b, pct, _ in EDGES] + [(a, b, pct) for a, b in lists[:20] for pct in (0, 50, 100)]
    lines = []
    for a, b, pct in walks:
        lines.append(f"S {len(a)} {len(b)} {pct}")
        lines += [f"{c} {s} {e}" for c, s, e in a + b]
    cases = _cases()
    groups = [(k, pct) for k in sorted(cases) for pct in (0, 50, 100)]
    run, glists, n_events, bp, status = _golden_input()
    for run_k, lists_k, pct, ev_k, bp_k, st_k, run_bp, seed in (
            [(cases[k][0], cases[k][1], pct, [0] * len(cases[k][1]), [0] * len(cases[k][1]), [0] * len(cases[k][1]), 0, 1) for k, pct in groups]
            + [(run, glists, 50, n_events, bp, status, 1200, 7)]):
        lines.append(f"G {len(run_k)} {(len(lists_k) - 2) // 3} {pct} {seed} {run_bp}")
        lines += [f"{c} {s} {e}" for c, s, e in run_k]
        for l, ne, b, st in zip(lists_k, ev_k, bp_k, st_k):
            lines.append(f"{ne} {len(l)} {b} {st}")
            lines += [f"{c} {s} {e}" for c, s, e in l]
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join(lines) + "\n")
    res = subprocess.run([exe, str(spec)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
    out = res.stdout.splitlines(keepends=True)
    for line, (a, b, pct) in zip(out, walks):
        assert line.strip() == "".join(str(int(x)) for x in R.supported(_peaks(a), _peaks(b), pct)), (a, b, pct)
    rest = "".join(out[len(walks):]).split("--\n")
    assert len(rest) == 2 * (len(groups) + 1) + 1
    for g, (k, pct) in enumerate(groups):
        want = R.figures(_peaks(cases[k][0]), [_peaks(l) for l in cases[k][1]], pct)
        bits = rest[2 * g + 2].splitlines()[:2]
        assert rest[2 * g + 1] == R.metrics_text(want), (k, pct)
        assert bits == ["".join(str(int(x)) for x in want[s]) for s in ("conservative", "optimal")], (k, pct)
    assert rest[-3].endswith(GOLDEN_CALLS) and rest[-2] == GOLDEN_METRICS
    assert rest[-1].endswith(GOLDEN_NARROWPEAK)


# ---- the command line ------------------------------------------------------------------------------------------------------------

def test_cli_refusals_create_no_file(tmp_path):
    """Refused before any input is read: no GPU needed."""
    from genrich_amd import build

    binp = build.build_host()
    sam = tmp_path / "t.sam"
    sam.write_text("@SQ\tSN:chrA\tLN:1000\n")
    out, met, npk, ev, log = tmp_path / "rep.tsv", tmp_path / "rep.metrics.tsv", tmp_path / "o.np", tmp_path / "ev.bed", tmp_path / "in.log"
    prefix = tmp_path / "pk"
    needs = "--reproducibility needs the peaks and the intervals of this run"
    sub = "need --reproducibility FILE or --reproducibility-metrics FILE"
    for extra, word in ((["-t", str(sam), "--reproducibility", str(out), "-X"], needs),
                        (["-t", str(sam), "--reproducibility-metrics", str(met), "-X"], needs),
                        (["-t", str(sam), "--reproducibility", str(out), "-P", "-f", str(log)], needs),
                        (["-t", str(sam), "--reproducibility", str(out), "--events-only", "-b", str(ev)], needs),
                        (["-t", str(sam), "--reproducibility", str(out), "--devices", "0,1"], "--reproducibility takes one device"),
                        (["-t", str(sam), "--reproducibility-metrics", str(met), "--devices", "0,0"], "--reproducibility takes one device"),
                        (["-t", str(sam), "--reproducibility-overlap", "50"], sub),
                        (["-t", str(sam), "--reproducibility-seed", "5"], sub),
                        (["-t", str(sam), "--reproducibility-peaks", str(prefix)], sub),
                        (["-t", str(sam), "--reproducibility", str(out), "--reproducibility-overlap", "101"], "--reproducibility-overlap takes an integer in [0, 100]"),
                        (["-t", str(sam), "--reproducibility", str(out), "--reproducibility-overlap", "-1"], "--reproducibility-overlap takes an integer"),
                        (["-t", str(sam), "--reproducibility", str(out), "--reproducibility-overlap", "50.5"], "--reproducibility-overlap takes an integer"),
                        (["-t", str(sam), "--reproducibility", str(out), "--reproducibility-seed", "-1"], "--reproducibility-seed takes an integer"),
                        (["-t", str(sam), "--reproducibility", str(out), "--reproducibility-seed", "18446744073709551616"],
                         "--reproducibility-seed takes an integer"),
                        (["-t", str(sam), "--reproducibility", str(out), "--reproducibility-seed", "7x"], "--reproducibility-seed takes an integer")):
        res = subprocess.run([binp, "-o", str(npk)] + extra, capture_output=True, text=True)
        assert res.returncode == 1 and word in res.stderr, (extra, res.stderr)
        assert len(res.stderr.strip().splitlines()) == 1, res.stderr                     # a one-line sentence
        assert sorted(p.name for p in tmp_path.iterdir()) == ["t.sam"], extra            # no file of any kind


def test_cli_help_names_the_options():
    from genrich_amd import build

    binp = build.build_host()
    res = subprocess.run([binp, "--help-reproducibility"], capture_output=True, text=True)
    usual = subprocess.run([binp, "-h"], capture_output=True, text=True)
    assert res.returncode == usual.returncode == 1 and res.stdout == usual.stdout == ""          # the same stream, the same status
    for word in ("--reproducibility FILE", "--reproducibility-metrics FILE", "--reproducibility-overlap PCT", "--reproducibility-seed S",
                 "--reproducibility-peaks PREFIX"):
        assert word in res.stderr, word
    assert "--reproducibility" not in usual.stderr
