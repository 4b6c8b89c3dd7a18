"""Counting each sample's intervals in the called peaks (gx_count_in_peaks, --counts): the numpy restatement the GPU tests
compare against, checked against the definition; the text format; the new entry points.  CPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import counts_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_case(rng, n_iv, n_chrom=3, clen=5000, n_peaks=12):
    pc, ps, pe = [], [], []
    for c in range(n_chrom):
        cuts = np.sort(rng.choice(np.arange(1, clen), size=2 * n_peaks, replace=False))
        for a, b in cuts.reshape(-1, 2):
            pc.append(c), ps.append(a), pe.append(b)
    pc, ps, pe = map(np.array, (pc, ps, pe))
    chrom = rng.integers(0, n_chrom, n_iv)
    s = rng.integers(0, clen, n_iv)
    e = np.minimum(clen, s + rng.integers(0, 900, n_iv))
    # the edges of the peaks themselves: s == pe and e == ps (no overlap), e == ps + 1 (overlap), spans over several peaks
    k = rng.integers(0, len(ps), n_iv // 4)
    s[: len(k)], e[: len(k)], chrom[: len(k)] = pe[k], pe[k] + 5, pc[k]
    k2 = rng.integers(0, len(ps), n_iv // 4)
    sl = slice(len(k), len(k) + len(k2))
    s[sl], e[sl], chrom[sl] = np.maximum(0, ps[k2] - 7), ps[k2] + rng.integers(0, 2, len(k2)), pc[k2]
    w = R.weights(rng.choice([1, 2, 3, 4, 5, 6, 8, 10], n_iv))
    return chrom, s, e, w, pc, ps, pe


@pytest.mark.parametrize("seed", range(6))
def test_restatement_matches_the_definition(seed):
    rng = np.random.default_rng(seed)
    args = _random_case(rng, 600)
    got = R.count_in_peaks(*args)
    exp = R.count_brute(*args)
    assert np.array_equal(got[0], exp[0]) and got[1:] == exp[1:]


def test_restatement_edges():
    pc, ps, pe = np.array([0, 0, 1]), np.array([100, 300, 100]), np.array([200, 400, 200])
    chrom = np.array([0, 0, 0, 0, 0, 1, 0])
    s = np.array([200, 50, 50, 150, 199, 150, 250])
    e = np.array([260, 100, 101, 350, 200, 160, 250])   # s == pe / e == ps: nothing; e == ps + 1: a hit; one spans two peaks
    w = R.weights([1, 1, 2, 1, 4, 1, 1])
    cnt, tot, inp = R.count_in_peaks(chrom, s, e, w, pc, ps, pe)
    assert cnt.tolist() == [60 + 120 + 30, 120, 120]
    assert tot == 120 * 5 + 60 + 30 and inp == 60 + 120 + 30 + 120
    assert (cnt, tot, inp)[1:] == R.count_brute(chrom, s, e, w, pc, ps, pe)[1:]


def test_restatement_without_peaks():
    cnt, tot, inp = R.count_in_peaks([0, 1], [5, 6], [9, 10], [120, 60], [], [], [])
    assert cnt.size == 0 and tot == 180 and inp == 0


def test_counts_text_format():
    txt = R.counts_text(["chrA", "chrB"], [(0, 10, 20), (1, 5, 7)], ["t0.sam", "c0.sam"], [[240, 130], [0, 40]])
    assert txt == ("chr\tstart\tend\tname\tt0.sam\tc0.sam\n"
                   "chrA\t10\t20\tpeak_0\t2\t0\n"
                   "chrB\t5\t7\tpeak_1\t1.08\t0.33\n")
    assert R.value_text(120 * 7) == "7" and R.value_text(30) == "0.25" and R.value_text(20) == "0.17"
    assert R.frip_line(1, True, 240, 60) == "  Intervals in peaks, control file #1: 0.50 of 2 (FRiP 0.250000)"
    assert R.frip_line(0, False, 0, 0) == "  Intervals in peaks, experimental file #0: 0 of 0 (FRiP 0.000000)"


def test_counting_entry_points_are_exported():
    import genrich_amd
    from genrich_amd import lib as L

    so = L.load_library()
    for name in ("gx_set_count_in_peaks", "gx_count_in_peaks", "gx_get_peak_counts", "gx_write_counts_group",
                 "gx_write_counts", "gx_write_counts_path"):
        assert hasattr(so, name), name
        assert name in L._SIGS, name
    hdr = open(os.path.join(ROOT, "include", "genrich_amd.h")).read()
    for name in ("gx_set_count_in_peaks", "gx_count_in_peaks", "gx_get_peak_counts", "gx_write_counts_group", "gx_write_counts"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
    assert re.search(r"#define GX_PATH_COUNTS 65536u", hdr)
    assert genrich_amd.GX_PATH_COUNTS == 65536
    for m in ("set_count_in_peaks", "count_in_peaks", "peak_counts", "write_counts"):
        assert callable(getattr(genrich_amd.Genrich, m)), m


def test_cli_refuses_counts_without_peak_calling(tmp_path):
    """--counts with -P or -X: exit 1 and no file (refused before any input is read, so no GPU is needed)."""
    import subprocess

    from genrich_amd import build

    binp = build.build_host()
    sam = tmp_path / "t.sam"
    sam.write_text("@SQ\tSN:chrA\tLN:1000\n")
    for extra in (["-X"], ["-P", "-f", str(tmp_path / "in.log")]):
        out = tmp_path / "c.tsv"
        res = subprocess.run([binp, "-t", str(sam), "-o", str(tmp_path / "o.np"), "--counts", str(out)] + extra,
                             capture_output=True, text=True)
        assert res.returncode == 1, res.stderr
        assert "--counts" in res.stderr
        assert not out.exists() and not (tmp_path / "o.np").exists()
