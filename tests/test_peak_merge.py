"""gx_peak_merge.h -- which peak is peak_N when several contexts own the chromosomes: the merge of their peak lists, a per-peak
column permuted into the merged order, and records that carry a peak index (summits, motif hits) renumbered and re-sorted.

The header is host-only, so it runs in a program of its own (tests/peak_merge_main.cpp, its own main) compiled with
-fsanitize=address,undefined: any report makes the program fail.  The reference is written here: the lists concatenated, then --
for more than one list -- Python's sorted with a (chrom, start) key, which is stable: equal keys keep the concatenation order.  One
list comes back as it went in, sorted or not.  Everything is an integer, compared with ==."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def _list(peaks, hits=(), summits=()):
    """One context: peaks (chrom, start, end, summit, value); hits (peak, pos, motif, strand, score) and summits (peak, pos) name a
    peak by its index in this list.  The scores tell the hits apart; no two hits of a case agree in (peak, pos, motif, strand)."""
    return (list(peaks), list(hits), list(summits))


def _cases():
    return [
        ("one list, in order", [_list([(0, 10, 20, 3, 100), (0, 50, 90, 7, 101), (2, 5, 9, 1, 102)],
                                      [(0, 2, 1, 0, 1), (0, 2, 1, 1, 2), (2, 0, 0, 0, 3)], [(0, 4), (1, 1), (1, 30), (2, 2)])]),
        # a single list is not re-sorted, and neither are its records
        ("one list, out of order", [_list([(2, 5, 9, 1, 100), (0, 50, 90, 7, 101), (0, 10, 20, 3, 102), (1, 0, 4, 0, 103)],
                                          [(3, 1, 0, 0, 1), (0, 2, 5, 1, 2), (0, 2, 1, 0, 3), (1, 9, 0, 0, 4)], [(2, 4), (0, 3), (0, 1)])]),
        ("two lists, chromosomes {0, 2} and {1}", [
            _list([(0, 10, 20, 3, 100), (0, 50, 90, 7, 101), (2, 5, 9, 1, 102), (2, 40, 60, 9, 103)],
                  [(0, 1, 0, 0, 1), (2, 3, 2, 1, 2), (3, 0, 0, 0, 3), (3, 5, 1, 0, 4)], [(0, 5), (1, 2), (1, 20), (3, 10)]),
            _list([(1, 0, 30, 4, 200), (1, 100, 140, 20, 201)], [(0, 7, 1, 1, 5), (1, 0, 0, 0, 6), (1, 0, 0, 1, 7)], [(0, 4), (1, 20), (1, 30)])]),
        ("three lists, the middle one empty", [
            _list([(1, 10, 20, 3, 100), (3, 0, 8, 2, 101)], [(1, 1, 0, 0, 1)], [(0, 3), (1, 2)]),
            _list([]),
            _list([(0, 7, 9, 1, 300), (2, 1, 2, 0, 301), (2, 3, 4, 0, 302)], [(2, 0, 0, 0, 2), (0, 1, 3, 1, 3)], [(1, 0), (2, 0)])]),
        ("all lists empty", [_list([]), _list([]), _list([])]),
        ("no list", []),
        # cannot happen in a run (a chromosome has one owner); the concatenation order decides
        ("two lists with the same (chrom, start)", [
            _list([(0, 5, 50, 1, 100), (1, 5, 20, 2, 101), (1, 9, 10, 0, 102)], [(1, 3, 0, 0, 1), (0, 3, 0, 0, 2)], [(1, 1), (2, 0)]),
            _list([(0, 5, 10, 3, 200), (1, 5, 30, 4, 201), (1, 5, 40, 5, 202)], [(1, 3, 0, 0, 3), (2, 3, 0, 0, 4), (0, 0, 0, 0, 5)], [(1, 2), (2, 3)])]),
        # hits of one peak at one position: (pos, motif, strand) decides, whichever list and place they came from
        ("position ties within a peak", [
            _list([(1, 0, 100, 50, 100)], [(0, 40, 2, 1, 1), (0, 40, 2, 0, 2), (0, 40, 0, 1, 3), (0, 7, 9, 0, 4), (0, 40, 1, 0, 5)], [(0, 40), (0, 7)]),
            _list([(0, 0, 100, 50, 200)], [(0, 40, 1, 1, 6), (0, 40, 0, 0, 7), (0, 40, 1, 0, 8), (0, 39, 7, 1, 9)], [(0, 41), (0, 39)])]),
    ]


def _want(lists):
    """The program's sections for one case."""
    cat = [(g, k, p) for g, l in enumerate(lists) for k, p in enumerate(l[0])]
    order = list(range(len(cat)))
    if len(lists) > 1:
        order = sorted(order, key=lambda j: (cat[j][2][0], cat[j][2][1]))
    rank = [0] * len(cat)
    for i, j in enumerate(order):
        rank[j] = i
    first = [0]
    for l in lists:
        first.append(first[-1] + len(l[0]))
    hits = [(rank[first[g] + h[0]],) + tuple(h[1:]) for g, l in enumerate(lists) for h in l[1]]
    sums = [(rank[first[g] + s[0]], s[1]) for g, l in enumerate(lists) for s in l[2]]
    if len(lists) > 1:
        hits = sorted(hits, key=lambda h: h[:4])
        sums = sorted(sums)
    return {"peaks": [tuple(cat[j][2][:4]) for j in order], "from": [(j,) for j in order], "rank": [(r,) for r in rank], "first": [(f,) for f in first],
            "column": [(cat[j][2][4],) for j in order], "hits": hits, "summits": sums}


def test_the_merge_standalone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "peak_merge")
    subprocess.check_call(SAN + [os.path.join(ROOT, "tests", "peak_merge_main.cpp"), "-o", exe])
    cases = _cases()
    lines = []
    for label, lists in cases:
        keys = [(g, h[:4]) for g, l in enumerate(lists) for h in l[1]] + [(g, s) for g, l in enumerate(lists) for s in l[2]]
        assert len(set(keys)) == len(keys), label   # (the test's own inputs: the order of the records is decided)
        lines.append("case %d" % len(lists))
        for peaks, hits, sums in lists:
            lines.append("list %d %d %d" % (len(peaks), len(hits), len(sums)))
            lines += [" ".join(str(v) for v in row) for row in peaks + hits + sums]
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
    parts = res.stdout.split("--\n")
    assert len(parts) == len(cases) + 1 and parts[-1] == ""
    heads = ("peaks", "from", "rank", "first", "column", "hits", "summits")
    for (label, lists), part in zip(cases, parts):
        got, at = {}, None
        for row in part.splitlines():
            if row in heads:
                at = got.setdefault(row, [])
            else:
                at.append(tuple(int(v) for v in row.split()))
        assert tuple(got) == heads, label
        want = _want(lists)
        for h in heads:
            assert got[h] == want[h], (label, h)
    # what the cases are there for, said once more in plain figures
    by = dict(cases)
    assert _want(by["one list, out of order"])["from"] == [(0,), (1,), (2,), (3,)]
    assert _want(by["two lists, chromosomes {0, 2} and {1}"])["from"] == [(0,), (1,), (4,), (5,), (2,), (3,)]
    assert _want(by["two lists with the same (chrom, start)"])["from"] == [(0,), (3,), (1,), (4,), (5,), (2,)]
    assert [h[4] for h in _want(by["position ties within a peak"])["hits"]] == [9, 7, 8, 6, 4, 3, 5, 2, 1]
