"""Counting each sample's intervals in a given region set (gx_count_in_regions, --count-regions): the numpy restatement the GPU
tests compare against, checked against the definition; the text format; the new entry points; the command line's refusals.
CPU only."""
import os
import re
import subprocess

import numpy as np
import pytest

import regions_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_case(rng, n_iv, n_chrom=3, clen=3000, n_reg=40):
    """Regions with ties, nesting and exact duplicates; intervals with empty and inverted ones and the regions' own edges."""
    rc = rng.integers(0, n_chrom + 1, n_reg)            # (one chromosome index beyond the intervals')
    rs = rng.integers(0, clen, n_reg) // 50 * 50        # (starts and ends on a coarse grid: many ties)
    re_ = rs + rng.choice([1, 50, 100, 700, 2 * clen], n_reg)
    k = rng.integers(0, n_reg, n_reg // 4)              # exact duplicates, and nested ones
    rc, rs, re_ = np.concatenate([rc, rc[k], rc[k]]), np.concatenate([rs, rs[k], rs[k] + 10]), np.concatenate([re_, re_[k], re_[k] + 15])
    re_ = np.maximum(re_, rs + 1)
    chrom = rng.integers(0, n_chrom, n_iv)
    s = rng.integers(0, clen, n_iv)
    e = np.minimum(clen, s + rng.integers(0, 400, n_iv))
    q = n_iv // 5
    k = rng.integers(0, len(rs), q)                     # s == end, e == start (no overlap) and one base more (overlap)
    s[:q], e[:q], chrom[:q] = re_[k] - rng.integers(0, 2, q), re_[k] + 5, np.minimum(rc[k], n_chrom - 1)
    k = rng.integers(0, len(rs), q)
    s[q:2 * q], e[q:2 * q], chrom[q:2 * q] = np.maximum(0, rs[k] - 7), rs[k] + rng.integers(0, 2, q), np.minimum(rc[k], n_chrom - 1)
    e[2 * q:2 * q + q // 2] = s[2 * q:2 * q + q // 2]   # empty
    inv = slice(2 * q + q // 2, 3 * q)                  # inverted
    e[inv] = np.maximum(0, s[inv] - rng.integers(1, 300, q - q // 2))
    w = R.weights(rng.choice([1, 2, 3, 4, 5, 6, 8, 10], n_iv))
    return chrom, s, e, w, rc, rs, re_


@pytest.mark.parametrize("seed", range(8))
def test_restatement_matches_the_definition(seed):
    rng = np.random.default_rng(seed)
    args = _random_case(rng, 500)
    chrom, s, e = args[:3]
    assert (e < s).any() and (e == s).any() and len(np.unique(args[5])) < len(args[5])
    got = R.count_in_regions(*args)
    exp = R.count_brute(*args)
    assert np.array_equal(got[0], exp[0]) and got[1:] == exp[1:]
    assert 0 < got[2] < got[1]


def test_restatement_edges():
    # regions: two that overlap, a duplicate, one nested, one on another chromosome, one on a chromosome without intervals
    rc = np.array([0, 0, 0, 0, 1, 2])
    rs = np.array([100, 150, 100, 120, 100, 0])
    re_ = np.array([200, 300, 200, 130, 200, 50])
    chrom = np.array([0, 0, 0, 0, 0, 0, 1, 0])
    s = np.array([200, 50, 50, 125, 299, 300, 150, 128])
    e = np.array([260, 100, 101, 125, 400, 310, 160, 122])
    # s == end of 0 / 2: only region 1; e == start: nothing; e == start + 1: regions 0 and 2; an empty interval inside 0, 2, 3;
    # the last base of region 1; s == end of 1: nothing; chromosome 1; an inverted interval that region 3 contains ([122, 128])
    w = R.weights([1, 1, 2, 1, 4, 1, 1, 3])
    cnt, tot, inr = R.count_in_regions(chrom, s, e, w, rc, rs, re_)
    assert cnt.tolist() == [60 + 120 + 40, 120 + 30, 60 + 120 + 40, 120 + 40, 120, 0]
    assert tot == 120 * 5 + 60 + 30 + 40 and inr == 120 + 60 + 120 + 30 + 120 + 40
    exp = R.count_brute(chrom, s, e, w, rc, rs, re_)
    assert np.array_equal(cnt, exp[0]) and (tot, inr) == exp[1:]


def test_restatement_without_regions():
    cnt, tot, inr = R.count_in_regions([0, 1], [5, 6], [9, 10], [120, 60], [], [], [])
    assert cnt.size == 0 and tot == 180 and inr == 0


def test_region_counts_text_format():
    txt = R.region_counts_text([("chrB", 5, 7, "promoter"), ("chrZ", 10, 20, None), ("chrA", 0, 9, None)], ["t0.sam", "c0.sam"],
                               [[240, 0, 130], [0, 0, 40]])
    assert txt == ("chr\tstart\tend\tname\tt0.sam\tc0.sam\n"
                   "chrB\t5\t7\tpromoter\t2\t0\n"
                   "chrZ\t10\t20\tregion_1\t0\t0\n"
                   "chrA\t0\t9\tregion_2\t1.08\t0.33\n")
    assert R.fraction_line(1, True, 240, 60) == "  Intervals in regions, control file #1: 0.50 of 2 (fraction 0.250000)"
    assert R.fraction_line(0, False, 0, 0) == "  Intervals in regions, experimental file #0: 0 of 0 (fraction 0.000000)"


def test_region_entry_points_are_exported():
    import genrich_amd
    from genrich_amd import lib as L

    so = L.load_library()
    names = ("gx_count_in_regions", "gx_get_region_counts", "gx_write_region_counts_group", "gx_write_region_counts",
             "gx_write_region_counts_path")
    hdr = open(os.path.join(ROOT, "include", "genrich_amd.h")).read()
    for name in names:
        assert hasattr(so, name), name
        assert name in L._SIGS, name
        assert re.search(r"\bint " + name + r"\(", hdr), name
    assert re.search(r"typedef struct \{ uint32_t chrom, start, end; \} gx_region;", hdr)
    assert re.search(r"#define GX_PATH_REGION_COUNTS 131072u", hdr)
    assert genrich_amd.GX_PATH_REGION_COUNTS == 131072
    assert genrich_amd.REGION_DTYPE.itemsize == 12 and genrich_amd.REGION_DTYPE.names == ("chrom", "start", "end")
    assert genrich_amd.RegionCounts._fields == ("count", "total", "in_regions", "rep", "is_ctrl")
    for m in ("count_in_regions", "region_counts", "write_region_counts"):
        assert callable(getattr(genrich_amd.Genrich, m)), m


def test_cli_refusals_create_no_file(tmp_path):
    """One option without the other, -P and --events-only: exit 1 and no file (refused before any input is read: no GPU needed)."""
    from genrich_amd import build

    binp = build.build_host()
    sam = tmp_path / "t.sam"
    sam.write_text("@SQ\tSN:chrA\tLN:1000\n")
    bed = tmp_path / "r.bed"
    bed.write_text("chrA\t10\t20\n")
    out, npk, ev = tmp_path / "rc.tsv", tmp_path / "o.np", tmp_path / "ev.bed"
    cases = [["--count-regions", str(bed)],
             ["--region-counts", str(out)],
             ["--count-regions", str(bed), "--region-counts", str(out), "-P", "-f", str(tmp_path / "in.log")],
             ["--count-regions", str(bed), "--region-counts", str(out), "--events-only", "-b", str(ev)]]
    for extra in cases:
        res = subprocess.run([binp, "-t", str(sam), "-o", str(npk)] + extra, capture_output=True, text=True)
        assert res.returncode == 1, (extra, res.stderr)
        assert "--count-regions" in res.stderr, (extra, res.stderr)
        assert not out.exists() and not npk.exists() and not ev.exists(), extra


def test_cli_help_names_the_options(tmp_path):
    from genrich_amd import build

    res = subprocess.run([build.build_host(), "-h"], capture_output=True, text=True)
    assert "--count-regions" in res.stderr and "--region-counts" in res.stderr
