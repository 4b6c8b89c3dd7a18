"""The profiles' definition (tests/profile_ref.py) and their text writers (gx_format_profile, gx_format_profile_rows), without a
GPU: the numpy reference against a base-by-base loop, and the C writers against the Python ones -- through ctypes, and once more
as a stand-alone program under AddressSanitizer / UBSan."""
import os
import subprocess

import numpy as np
import pytest

import backends as B
import coverage_ref as R
import profile_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [3 * 4096 + 17, 37, 900]


def _events():
    rng = np.random.default_rng(5)
    n = 200
    ev = np.zeros(n, dtype=B.EVENT_DTYPE)
    ev["chrom"] = rng.integers(0, len(LENS), n)
    ln = np.asarray(LENS)[ev["chrom"]]
    ev["start"] = rng.integers(0, ln + 3)
    ev["end"] = ev["start"] + rng.integers(0, 700, n)
    ev["count"] = rng.choice([1, 1, 1, 2, 3, 4, 5, 6, 8, 10], n)
    return ev


def test_reference_against_brute_force():
    ev = _events()
    for c, length in enumerate(LENS):
        pile = R.pileup120(ev, c, length)
        assert pile.any()
        pos = [0, 1, length // 2, length - 1, length, length + 5, length + 40]        # (at and beyond the length: legal)
        pos, strand = np.asarray(pos + pos), np.asarray([1] * len(pos) + [-1] * len(pos))
        for F, Bn in ((64, 1), (50, 50), (40, 10), (1000, 20), (16384, 4096)):        # (F larger than chromosomes 1 and 2, and than all)
            if F > 2000 and length > 2000:
                continue                                                              # (the loop is base by base)
            got, exp = P.rows_of(pile, pos, strand, F, Bn), P.rows_brute(pile, pos, strand, F, Bn)
            assert got.dtype == np.int64 and got.shape == (len(pos), 2 * F // Bn)
            assert np.array_equal(got, exp), (c, F, Bn)
            if F > length + 40:
                assert (got.sum(axis=1) == pile.sum()).all()                          # the window holds the whole chromosome
    # the anchor base is the first base, in reading direction, of bin nb / 2 -- on both strands
    pile = np.zeros(100, dtype=np.int64)
    pile[40] = 7
    for s in (1, -1):
        row = P.rows_of(pile, [40], [s], 10, 1)[0]
        assert row[10] == 7 and row.sum() == 7
    pile[41] = 3
    assert P.rows_of(pile, [40], [1], 10, 2)[0].tolist() == [0, 0, 0, 0, 0, 10, 0, 0, 0, 0]
    assert P.rows_of(pile, [40], [-1], 10, 2)[0].tolist() == [0, 0, 0, 0, 3, 7, 0, 0, 0, 0]


def test_rows_that_are_zero():
    ev = _events()
    anchors = np.asarray([(0, 100, 1), (1, 10, -1), (2, 500, 1), (3, 5, 1), (0, 100, -1)], dtype=P.ANCHOR_DTYPE)
    full = P.profile(ev, LENS, anchors, 40, 10)
    assert full[[0, 1, 2, 4]].any(axis=1).all() and not full[3].any()                 # chrom 3 lies behind the table
    for kw, dead in ((dict(skip=[0, 1, 0]), 1), (dict(owned=[1, 1, 0]), 2), (dict(save=[0, 1, 1]), 0)):
        got = P.profile(ev, LENS, anchors, 40, 10, **kw)
        for k, a in enumerate(anchors):
            assert np.array_equal(got[k], full[k] * (a["chrom"] != dead)), (kw, k)
    cut = P.profile(ev, LENS, anchors, 40, 10, beds=[[90, 110], [], []])             # -E bases count 0
    pile = R.pileup120(ev, 0, LENS[0])
    pile[90:110] = 0
    assert np.array_equal(cut[0], P.rows_of(pile, [100], [1], 40, 10)[0]) and not np.array_equal(cut[0], full[0])
    assert P.n_counted(anchors, LENS) == 4 and P.n_counted(anchors, LENS, skip=[1, 0, 0]) == 2


# hand-made tables: (flank, bin, counted, sample names, aggregates)
def _table_cases():
    return [
        (20, 10, 3, ["a.bam", "b.bam"], [[0, 3600, 3601, 120], [7, 0, 0, -240]]),
        (50, 50, 0, ["only"], [[5, 6]]),                                              # no anchor counted: zeros
        (4, 1, 1, [], []),                                                            # no sample: offsets alone
        (2000, 500, 20000, ["big"], [[(1 << 50) + 1, 1 << 40, 12345678901234, 0, 1, 2, 3, 1 << 55]]),
    ]


# (flank, bin, names, regions, row names, strands, first, cells of rows first ..)
def _row_cases():
    names = ["chr1", "chrM", "unknown"]
    regions = [(0, 100, 200), (1, 0, 1), (2, 5, 9), (0, 4096, 8192)]
    return [
        (20, 10, names, regions, ["tss_a", None, "x", None], [1, -1, 1, -1], 0,
         [[0, 1200, 2400, 1201], [40, 40, 40, 0], [0, 0, 0, 0], [-1200, -5, 120 * 10 * 1000000, 7]]),
        (20, 10, names, regions, None, [1, 1, -1, -1], 2, [[0, 0, 0, 0], [1, 2, 3, 4]]),   # rows 2 and 3: anchor_2, anchor_3
        (2, 1, names, regions, [None] * 4, [1] * 4, 1, [[120, 60, 40, 30]]),
    ]


def _anchors_of(regions, strands):
    a = np.zeros(len(regions), dtype=P.ANCHOR_DTYPE)
    for k, ((c, s, e), st) in enumerate(zip(regions, strands)):
        a[k] = (c, s, st)
    return a


def test_format_through_ctypes_against_the_python_writers():
    from genrich_amd.lib import REGION_DTYPE, format_profile, format_profile_rows
    for F, Bn, counted, names, aggs in _table_cases():
        got = format_profile(names, aggs, counted, F, Bn).decode()
        assert got == P.profile_text(names, aggs, counted, F, Bn), (F, Bn)
        assert len(got.splitlines()) == 1 + 2 * F // Bn
    assert format_profile(["s"], [[1200, 2400]], 2, 5, 5) == b"offset\ts\n-5\t1.000000\n0\t2.000000\n"
    for F, Bn, names, regions, row_names, strands, first, cells in _row_cases():
        got = format_profile_rows(names, np.asarray(regions, dtype=REGION_DTYPE), row_names, _anchors_of(regions, strands), first,
                                  np.asarray(cells, dtype=np.int64), Bn).decode()
        assert got == P.rows_text(names, regions, row_names, strands, first, cells, Bn), (F, Bn, first)
    assert format_profile_rows(["c"], np.asarray([(0, 3, 9)], dtype=REGION_DTYPE), None, _anchors_of([(0, 3, 9)], [-1]), 0,
                               np.asarray([[240, 121]], dtype=np.int64), 1) == b"c\t3\t9\tanchor_0\t-\t2\t1.0083\n"
    with pytest.raises(RuntimeError):
        format_profile(["s"], [[1, 2]], 1, 5, 0)   # bin_size == 0


def _spec(table, rows):
    F, Bn, counted, snames, aggs = table
    _, _, names, regions, row_names, strands, first, cells = rows
    nb = 2 * F // Bn
    out = [f"{F} {Bn} {counted} {len(snames)} {nb}"]
    out += [f"{n} {' '.join(str(x) for x in a)}" for n, a in zip(snames, aggs)]
    out.append(f"{len(names)} {' '.join(names)}")
    out.append(f"{len(regions)} {first} {len(cells)}")
    for k, ((c, s, e), st) in enumerate(zip(regions, strands)):
        rn = row_names[k] if row_names is not None and row_names[k] is not None else "*"
        out.append(f"{c} {s} {e} {rn} {st}")
    out += [" ".join(str(x) for x in row) for row in cells]
    return "\n".join(out) + "\n"


def test_format_standalone_under_sanitizers(tmp_path):
    """gx_emit.cpp's writers in a program of its own (its own main, tests/profile_format_main.cpp), compiled with
    -fsanitize=address,undefined: any report makes the program fail (-fno-sanitize-recover, ASan aborts by default)."""
    exe = str(tmp_path / "profile_format")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "profile_format_main.cpp"),
                           os.path.join(ROOT, "genrich_amd", "csrc", "gx_emit.cpp"), "-o", exe])
    # every table with a row case of its bin count (the rows' flank and bin size are the table's)
    eight = [[0, 120, 240, 360, 480, 600, 720, 121]]
    pairs = [(_table_cases()[0], _row_cases()[0]), (_table_cases()[0], _row_cases()[1]),
             (_table_cases()[1], (50, 50, ["c"], [(0, 1, 2)], None, [1], 0, [[6000, 1]])),
             (_table_cases()[2], (4, 1, ["c", "d"], [(1, 1, 2), (0, 7, 9)], ["n", None], [-1, 1], 1, eight)),
             (_table_cases()[3], (2000, 500, ["c"], [(0, 1, 2)], None, [-1], 0, [[x * 500 for x in eight[0]]]))]
    for k, (table, rows) in enumerate(pairs):
        F, Bn, counted, snames, aggs = table
        _, _, names, regions, row_names, strands, first, cells = rows
        assert all(len(r) == 2 * F // Bn for r in cells)
        spec = tmp_path / f"spec{k}.txt"
        spec.write_text(_spec(table, rows))
        res = subprocess.run([exe, str(spec)], capture_output=True, text=True)
        assert res.returncode == 0, (k, res.returncode, res.stderr)
        assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
        tab, mat = res.stdout.split("--\n")
        assert tab == P.profile_text(snames, aggs, counted, F, Bn), k
        assert mat == P.rows_text(names, regions, row_names, strands, first, cells, Bn), k


def test_enrichment_line():
    agg = [10] * 10 + [50] * 380 + [10] * 10
    agg[200] = 400
    assert P.enrichment(agg, 10) == 40.0                                              # ne = 10: 400 * 20 / 200
    assert P.enrichment([1, 9], 50) == 9 * 2 / 10                                     # nb = 2: ne = max(1, 0)
    assert P.enrichment([0, 5, 5, 0], 1) == 0.0                                       # an empty edge
    assert P.enrichment_line(1, True, agg, 7, 10) == "  Profile, control file #1: enrichment 40.000000 over 7 anchors"
