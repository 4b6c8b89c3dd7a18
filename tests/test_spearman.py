"""The rank correlation's host side without a GPU: tests/rank_ref.py (the definition) against scipy's spearmanr, the merge of the
contexts' value tables into rank tables (gx_rank_tables) through ctypes and once more as a stand-alone program under
AddressSanitizer / UBSan, the ctypes mirror, and the command line's refusals."""
import os
import subprocess

import numpy as np
import pytest

import rank_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tied_rows(seed, S=4, n=5000):
    """Rows with heavy ties and 60 % zeros: a few dozen distinct values, partly shared between the rows; some bins are 0 in all."""
    rng = np.random.default_rng(seed)
    base = rng.geometric(0.15, n)
    dead = rng.random(n) < 0.35                                   # 0 in every row
    rows = []
    for s in range(S):
        x = base * rng.integers(1, 3, n) + rng.geometric(0.3, n) * 120
        x[(rng.random(n) < 0.4) | dead] = 0
        rows.append(x.astype(np.uint64))
    return rows


# ---- 1. the definition is the one users know ---------------------------------------------------------------------------

@pytest.mark.parametrize("skip", [False, True])
def test_the_reference_against_scipy(skip):
    stats = pytest.importorskip("scipy.stats")
    rows = _tied_rows(3)
    keep, n_zero = K.kept(rows, skip)
    assert n_zero > 1000 and all(0.55 < float((r == 0).mean()) < 0.75 for r in rows) and all(len(np.unique(r)) < 500 for r in rows)
    want = stats.spearmanr(np.asarray(rows, dtype=np.float64)[:, keep].T).statistic
    got = K.rho(rows, skip)
    for i in range(len(rows)):
        for j in range(len(rows)):
            assert abs(float(got[i][j]) - want[i][j]) < 1e-9, (i, j)
    if skip:                                                     # taking the bins out changes rho (unlike a shift of all ranks)
        plain = K.rho(rows, False)
        assert abs(float(plain[0][1]) - float(got[0][1])) > 1e-3


def test_the_reference_by_hand():
    rows = [np.array([0, 5, 5, 0, 9, 0]), np.array([0, 1, 0, 0, 2, 3])]
    N, nz, R = K.rank_rows(rows)
    assert (N, nz) == (6, 2)
    assert R[0].tolist() == [4, 9, 9, 4, 12, 4]                 # ranks 1-3 -> 2, 4-5 -> 4.5, 6: doubled
    assert R[1].tolist() == [4, 8, 4, 4, 10, 12]
    N, nz, R = K.rank_rows(rows, skip_zeros=True)
    assert (N, nz) == (4, 2)
    assert R[0].tolist() == [0, 5, 5, 0, 8, 2] and R[1].tolist() == [0, 4, 2, 0, 6, 8]
    assert K.tables(rows, True)[0][0].tolist() == [0, 5, 9] and K.tables(rows, True)[0][1].tolist() == [2, 5, 8]
    assert K.spearman_text(["t0", "c0"], [rows[0], rows[0]]) == "\tt0\tc0\nt0\t1.000000\t1.000000\nc0\t1.000000\t1.000000\n"


# ---- 2. gx_rank_tables ----------------------------------------------------------------------------------------------------

def _split(rows, cuts):
    """The rows cut into contexts at the bin indices `cuts`."""
    edges = [0] + list(cuts) + [len(rows[0])]
    return [[r[a:b] for r in rows] for a, b in zip(edges[:-1], edges[1:])]


def _table_cases():
    """(label, contexts' rows, skip_zeros)"""
    rng = np.random.default_rng(11)
    rows = _tied_rows(5, S=3, n=3000)
    out = [("one_context", [rows], False), ("one_context_skip", [rows], True)]
    srt = [np.sort(r) for r in rows]                              # sorted rows: the contexts' values hardly overlap
    for label, rr in (("three_overlapping", rows), ("three_disjoint", srt)):
        out.append((label, _split(rr, (700, 1900)), False))
        out.append((label + "_skip", _split(rr, (700, 1900)), True))
    z = [rows[0], np.zeros(3000, dtype=np.uint64), rows[1]]
    out.append(("all_zero_sample", _split(z, (1000,)), False))
    out.append(("all_zero_sample_skip", _split(z, (1000,)), True))
    one = [np.where(rows[0] == 0, 0, 7).astype(np.uint64), np.where(rows[0] == 0, 0, rows[1] + 1).astype(np.uint64)]
    out.append(("zero_disappears_skip", [one], True))              # the rows are 0 at the same bins: value 0 leaves both tables
    out.append(("empty_tables", [[r[:0] for r in rows], [r[:0] for r in rows]], False))
    out.append(("an_empty_context", [[r[:0] for r in rows], rows], True))
    big = [rng.integers((1 << 51) - 50, 1 << 51, 400).astype(np.uint64), rng.integers(0, 3, 400).astype(np.uint64)]
    out.append(("values_up_to_the_domains_end", _split(big, (100, 200)), False))
    return out


@pytest.fixture(scope="module")
def table_cases():
    """(label, per-context tables, n_zero_to_drop, N, expected tables): computed once."""
    out = []
    for label, ctxs, skip in _table_cases():
        S = len(ctxs[0])
        whole = [np.concatenate([c[s] for c in ctxs]) for s in range(S)]
        keep, n_zero = K.kept(whole, skip)
        out.append((label, [[K.distinct(r) for r in c] for c in ctxs], n_zero if skip else 0, int(keep.sum()), K.tables(whole, skip)))
    return out


def test_rank_tables_through_ctypes_against_the_reference(table_cases):
    from genrich_amd.lib import rank_tables
    seen = set()
    for label, tabs, drop, N, exp in table_cases:
        gotN, got = rank_tables(tabs, drop)
        assert gotN == N, label
        for (v, r), (ev, er) in zip(got, exp):
            assert v.tolist() == ev.tolist() and r.tolist() == er.tolist(), label
            if len(v):
                assert int(r[-1]) <= 2 * N and int(r[0]) >= 1
        seen.add(label)
        if label == "zero_disappears_skip":
            assert drop > 0 and all(0 not in v.tolist() for v, _ in got)
        if label == "all_zero_sample":
            assert got[1][0].tolist() == [0] and got[1][1].tolist() == [N + 1]
        if label == "all_zero_sample_skip":
            assert got[1][0].tolist() == [0] and got[1][1].tolist() == [N + 1] and drop > 0
        if label == "empty_tables":
            assert N == 0 and all(len(v) == 0 for v, _ in got)
    assert len(seen) == len(table_cases)


def test_rank_tables_refusals():
    from genrich_amd.lib import rank_tables
    ok = ([0, 3, 5], [2, 1, 1])
    assert rank_tables([[ok]], 2)[0] == 2
    for tabs, drop in (([[([3, 3], [1, 1])]], 0),                 # not strictly ascending
                       ([[([5, 3], [1, 1])]], 0),
                       ([[([3, 5], [1, 0])]], 0),                 # a count of 0
                       ([[ok]], 3),                               # more to drop than zeros
                       ([[([3, 5], [1, 1])]], 1),                 # ... no zeros at all
                       ([[ok, ([1], [5])]], 0),                   # the samples differ in N
                       ([[([1], [1 << 41])]], 0),                 # N = 2^41
                       ([[([1], [1 << 40])], [([2], [1 << 40])]], 0),
                       ([[ok] * 33], 0)):                         # 33 samples
        with pytest.raises(RuntimeError):
            rank_tables(tabs, drop)
    assert rank_tables([[([1], [(1 << 41) - 1])]], 0)[1][0][1].tolist() == [1 << 41]   # the largest N: rank2 = N + 1


def test_rank_tables_standalone_under_sanitizers(table_cases, tmp_path):
    """gx_emit.cpp's merge in a program of its own (its own main, tests/rank_tables_main.cpp), compiled with
    -fsanitize=address,undefined: any report makes the program fail (-fno-sanitize-recover, ASan aborts by default)."""
    exe = str(tmp_path / "rank_tables")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "rank_tables_main.cpp"),
                           os.path.join(ROOT, "genrich_amd", "csrc", "gx_emit.cpp"), "-o", exe])
    lines, want = [], []
    for label, tabs, drop, N, exp in table_cases:
        lines.append(f"{len(tabs)} {len(tabs[0])} {drop}")
        for ctx in tabs:
            for v, c in ctx:
                lines.append(str(len(v)))
                lines += [f"{int(a)} {int(b)}" for a, b in zip(v, c)]
        want.append(f"0 {N}\n" + "".join(f"{len(v)}\n" + "".join(f"{int(a)} {int(b)}\n" for a, b in zip(v, r)) for v, r in exp) + "--\n")
    lines += ["1 1 5", "2", "0 4", "9 1"]                          # a refusal: more to drop than zeros
    want.append("-10 0\n--\n")
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join(lines) + "\n")
    res = subprocess.run([exe, str(spec)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
    assert res.stdout == "".join(want)


# ---- 3. the ctypes mirror ---------------------------------------------------------------------------------------------------

def test_the_mirror_and_the_geometry():
    import genrich_amd.lib as L
    assert L.GX_PATH_SPEARMAN == 1 << 22
    lanes, grid, cache, cap, limit = L.rank_geometry()
    assert lanes % 64 == 0 and grid >= 1 and cache >= 64 and cache & (cache - 1) == 0
    assert cap & (cap - 1) == 0 and 0 < limit < cap
    lib = L.load_library()
    for name in ("gx_coverage_distinct", "gx_rank_tables", "gx_coverage_rank_gram", "gx_coverage_spearman_group", "gx_write_spearman_group",
                 "gx_distinct_u64", "gx_rank_u64", "gx_rank_geometry", "gx_rank_last"):
        assert getattr(lib, name).argtypes is not None, name
    for name in ("coverage_distinct", "coverage_rank_gram", "distinct_u64", "rank_u64", "rank_last"):
        assert callable(getattr(L.Genrich, name)), name
    # no context: refused before anything is touched
    assert lib.gx_coverage_distinct(None, 0, None, None, 0, None) == -10
    assert lib.gx_distinct_u64(None, None, 0, 0, None, None, 0, None) == -10
    assert lib.gx_rank_u64(None, None, 1, 0, 0, 0, None, None) == -10
    assert lib.gx_coverage_rank_gram(None, None, 0, None, None, None, None, None, 0) == -10
    assert lib.gx_coverage_spearman_group(None, 1, 1, 0, None, None, None, None) == -10
    assert lib.gx_write_spearman_group(None, 1, 1, None, 0, None) == -10
    assert lib.gx_rank_last(None, None, None) == -10


# ---- 4. the command line -----------------------------------------------------------------------------------------------------

def test_cli_refusals_create_no_file(tmp_path):
    """Refused before any input is read: no GPU needed."""
    from genrich_amd import build

    binp = build.build_host()
    sam = tmp_path / "t.sam"
    sam.write_text("@SQ\tSN:chrA\tLN:1000\n")
    out, npk, ev = tmp_path / "rho.tsv", tmp_path / "o.np", tmp_path / "ev.bed"
    for extra, word in ((["--spearman", str(out), "-P", "-f", str(tmp_path / "in.log")], "--spearman needs the pileups of this run"),
                        (["--spearman", str(out), "--events-only", "-b", str(ev)], "--spearman needs the pileups of this run"),
                        (["--corr-skip-zeros"], "--corr-skip-zeros needs --correlation FILE or --spearman FILE"),
                        (["--spearman", str(out), "--bin-size", "0"], "--bin-size"),
                        (["--spearman", str(out), "--bin-size", "1048577"], "--bin-size"),
                        (["--spearman", str(out), "--coverage-scale", "2"], "--coverage")):
        res = subprocess.run([binp, "-t", str(sam), "-o", str(npk)] + extra, capture_output=True, text=True)
        assert res.returncode == 1 and word in res.stderr, (extra, res.stderr)
        assert not out.exists() and not npk.exists() and not ev.exists(), extra


def test_cli_refuses_more_than_32_samples_before_anything_is_written(tmp_path):
    from genrich_amd import build

    sam = tmp_path / "t.sam"
    sam.write_text("@SQ\tSN:chrA\tLN:1000\n")
    out, npk = tmp_path / "rho.tsv", tmp_path / "o.np"
    t17 = ",".join([str(sam)] * 17)
    for extra in (["-t", ",".join([str(sam)] * 33)], ["-t", t17, "-c", ",".join([str(sam)] * 16)]):
        res = subprocess.run([build.build_host(), "-o", str(npk), "--spearman", str(out)] + extra, capture_output=True, text=True)
        assert res.returncode == 1 and "--spearman takes at most 32 samples" in res.stderr, res.stderr
        assert not out.exists() and not npk.exists()
    res = subprocess.run([build.build_host(), "-o", str(npk), "--spearman", str(out), "-t", t17, "-c", ",".join(["null"] * 16)],
                         capture_output=True, text=True)
    assert "--spearman takes at most 32 samples" not in res.stderr   # 17 samples: the nulls are none


def test_cli_help_names_the_option():
    from genrich_amd import build

    res = subprocess.run([build.build_host(), "-h"], capture_output=True, text=True)
    assert "--spearman FILE [--corr-skip-zeros]" in res.stderr
