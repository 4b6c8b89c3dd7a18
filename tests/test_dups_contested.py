"""What the contested -r cases (tests/dups_cases.py; dups_contested_* under tests/golden/) hold, without a GPU: the reference's
rule walked over the records themselves names exactly the duplicates -- and the sets they matched -- of the reference's own -R
log, and on its way meets every situation the cases are made for.  (The command line runs on them in tests/test_host_cli.py:
the host's tables here, the device's on the GPU.)"""
import pytest

import dups_cases as D
import golden_cases as G
from test_host_cli import _cases

CASES = ["dups_contested_y", "dups_contested_x_bam", "dups_contested_pairs"]


def _walks(name):
    """[(alignment sets, {duplicate: matched set}, what the walk met)] of the case's treatment and control files."""
    case = _cases()[0][name]
    single = "-y" in case["args"] or "-x" in case["args"]
    out = []
    for which, off, prefix in (("t", 0, "t0_"), ("c", 1, "c0_")):
        names, lens, ev = case["reps"][0][which]
        recs = D.contested_records(names, lens, ev, case["mixed"]["seed"] + off, prefix)
        sets = D.alignment_sets(recs, case["mixed"]["bam"])
        out.append((sets,) + D.walk(sets, single))
    return out, single


def test_the_cases_are_there():
    assert set(CASES) <= set(G.case_names())
    args = {n: G.load_case(n)[0]["args"] for n in CASES}
    assert all("-r" in a and "-s" not in a for a in args.values())                 # secondary alignments survive without -s
    assert "-y" in args["dups_contested_y"] and "-x" in args["dups_contested_x_bam"]
    assert not {"-y", "-x", "-w"} & set(args["dups_contested_pairs"])
    assert _cases()[0]["dups_contested_x_bam"]["mixed"]["bam"]


@pytest.mark.parametrize("name", CASES)
def test_the_walk_names_the_duplicates_of_the_references_log(name):
    log = [l.split("\t") for l in G.read_gz(name, "out.dups").decode().splitlines() if not l.startswith("#")]
    want = {l[0]: l[2] for l in log}
    assert len(want) == len(log) > 300
    got = {}
    walks, single = _walks(name)
    for _, dup_of, _ in walks:
        got.update(dup_of)
    assert got == want
    kinds = {l[3] for l in log}
    assert kinds == ({"paired", "discordant", "single"} if single else {"paired"})


@pytest.mark.parametrize("name", CASES)
def test_the_walk_meets_what_the_cases_are_made_for(name):
    walks, single = _walks(name)
    for sets, dup_of, seen in walks:
        tables = ("pr", "dc", "sn") if single else ("pr",)
        n_sets = sum(len(sets[t]) for t in tables)
        assert 300 <= sum(len(sets[t]) for t in sets) <= 2000
        for t in tables:
            rows = sets[t]
            assert seen["multi_sets"][t] >= 50                                  # sets with several alignments, in every table
            assert 20 <= seen["multi_dup"][t] < seen["multi_sets"][t]           # ... duplicates (giving up all their keys) and kept
            assert seen["kept_after_a_multi_gave_up"][t] >= 5                   # a single set kept on a key a duplicate multi set held first
            kept = sum(1 for r in rows if r[0] not in dup_of)
            assert kept >= len(rows) // 4 and len(rows) - kept >= len(rows) // 4
        assert seen["single_before_multi"] >= 50 and seen["single_after_multi"] >= 50
        assert seen["same_key_twice"] >= 10                                     # two alignments of one set with one key
        assert seen["equal_quality"] >= n_sets * 9 // 10                        # the stable order decides nearly everywhere
        if single:
            assert seen["shapes"] == {(1, 1), (2, 1), (1, 2), (2, 2)}
            assert seen["sn_on_pair_end"] >= 30 and seen["sn_on_dc_end"] >= 5 and seen["sn_on_an_end_a_multi_sn_holds"] >= 30
            # a discordant template again with the mates swapped: one key (the unordered pair), met in both orders
            dc = {}
            for nm, _, keys, ends, shape in sets["dc"]:
                if shape == (1, 1):
                    dc.setdefault(keys[0], set()).add(tuple(ends))
            assert sum(1 for v in dc.values() if len(v) > 1) >= 5
