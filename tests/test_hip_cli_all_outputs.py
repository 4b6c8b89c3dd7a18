"""Every figure of the command line at once.  One run of genrich-amd -v with every figure option together; then every figure alone
must write the same bytes and print the same -v lines as it did in the combined run.  The combined run once more on two contexts
(--devices 0,0) and once more gzipped (-z) must write the same files.  This holds main's enable block, its count-in-peaks condition
and the order of its dispatch in place, which the per-figure tests exercise one at a time.

The input is the smallest on which every writer has something to say: two chromosomes of 20 kb and a third that no read touches,
two replicates of a few hundred paired fragments (the first with a control, the second with `null`), a handful of unpaired
alignments (-y) so that --xcor suggests an extension, one -E region, a BED of ten lines for --count-regions and --profile with
a line on a chromosome that no header names and lines on the minus strand, a FASTA of the three chromosomes (seeded random bases
with a short run of N) and three JASPAR motifs of width 6 to 8, loose enough (--motif-pvalue 0.01) to hit in the small peaks.

Three -v lines carry a wall-clock time (--genome's, and --motif-summary's two): the seconds are masked before lines are compared."""
import gzip
import os
import random
import re
import subprocess

import pytest

import synth

pytestmark = pytest.mark.gpu

NAMES, LENS = ["chrA", "chrB", "chrC"], [20_000, 21_000, 5_000]
BED = [("chrA", 900, 1400, "a1", "+"), ("chrA", 2800, 3300, "a2", "-"), ("chrB", 2900, 3100, "b1", "+"), ("chrZ", 10, 500, "z1", "+"),
       ("chrA", 8800, 9300, "a3", "-"), ("chrB", 10_900, 11_200, "b2", "."), ("chrA", 1000, 3000, "a4", "+"), ("chrC", 100, 900, "c1", "+"),
       ("chrB", 20_500, 21_000, "b3", "-"), ("chrA", 0, 300, "a5", "+")]

# figure -> (its options, the files it writes, the prefixes of its -v lines)
SAMPLES = ["t0", "c0", "t1"]
FIGURES = {
    "counts": (["--counts", "c.tsv"], ["c.tsv"], ["  Intervals in peaks,"]),
    "peak-signal": (["--peak-signal", "ps.tsv"], ["ps.tsv"], ["  Signal in peaks,"]),
    "count-regions": (["--count-regions", "sites.bed", "--region-counts", "rc.tsv"], ["rc.tsv"], ["  Intervals in regions,"]),
    "coverage": (["--coverage", "cov", "--bin-size", "100", "--coverage-scale", "2.5"], [f"cov.{s}.bedgraph" for s in SAMPLES], ["  Coverage,"]),
    "correlation": (["--correlation", "corr.tsv", "--bin-size", "100", "--corr-skip-zeros"], ["corr.tsv"], ["  Correlation:"]),
    "spearman": (["--spearman", "sp.tsv", "--bin-size", "100", "--corr-skip-zeros"], ["sp.tsv"], ["  Spearman:"]),
    "fingerprint": (["--fingerprint", "fp.tsv", "--fingerprint-metrics", "fm.tsv", "--bin-size", "100"], ["fp.tsv", "fm.tsv"], ["  Fingerprint "]),
    "complexity": (["--complexity", "cx.tsv", "--complexity-hist", "ch.tsv"], ["cx.tsv", "ch.tsv"], ["  Library complexity,"]),
    "lengths": (["--lengths", "len.tsv", "--lengths-metrics", "lm.tsv", "--lengths-cuts", "120,180,240", "--chrom-stats", "cs.tsv"],
                ["len.tsv", "lm.tsv", "cs.tsv"], ["  Interval lengths"]),
    "depth": (["--depth", "d.tsv", "--depth-metrics", "dm.tsv"], ["d.tsv", "dm.tsv"], ["  Depth,"]),
    "xcor": (["--xcor", "xc.tsv", "--xcor-metrics", "xm.tsv", "--xcor-shifts", "-50,400", "--xcor-read-length", "50"], ["xc.tsv", "xm.tsv"],
             ["  Strand cross-correlation,", "  suggested -x"]),
    "saturation": (["--saturation", "sat.tsv", "--saturation-steps", "4", "--saturation-seed", "3"], ["sat.tsv"], ["  Saturation"]),
    "summits": (["--summits", "sm.tsv", "--summits-prominence", "10", "--summits-height", "30"], ["sm.tsv"], ["  Summits in peaks:"]),
    "reproducibility": (["--reproducibility", "rp.tsv", "--reproducibility-metrics", "rm.tsv", "--reproducibility-overlap", "40", "--reproducibility-seed", "3",
                         "--reproducibility-peaks", "rpk"],
                        ["rp.tsv", "rm.tsv"] + [f"rpk.{c}.narrowPeak" for c in ("t1", "t1.pr1", "t1.pr2", "t2", "t2.pr1", "t2.pr2", "pooled.pr1", "pooled.pr2",
                                                                                "conservative", "optimal")], ["  Reproducibility"]),
    "gc-bias": (["--genome", "g.fa", "--gc-bias", "gc.tsv", "--gc-window", "150"], ["gc.tsv"], ["Genome ", "  GC bias,"]),
    "gc-peaks": (["--genome", "g.fa", "--gc-peaks", "gp.tsv"], ["gp.tsv"], ["Genome "]),
    "motifs": (["--genome", "g.fa", "--motifs", "m.jaspar", "--motif-hits", "mh.tsv", "--motif-summary", "ms.tsv", "--motif-pvalue", "0.01",
                "--motif-pseudocount", "0.5"], ["mh.tsv", "ms.tsv"], ["Genome ", "Motifs ", "Motif hits:", "  Motif "]),
    "profile": (["--profile", "sites.bed", "--profile-out", "prof", "--flank", "500", "--profile-bin", "20", "--profile-matrix"],
                ["prof.profile.tsv"] + [f"prof.{s}.matrix.tsv" for s in SAMPLES], ["  Profile,"]),
}
ONE_DEVICE = ["saturation", "reproducibility"]
PREFIXES = sorted({p for _, _, ps in FIGURES.values() for p in ps})
SECONDS = re.compile(r"\b\d+\.\d{3} s\b")
MOTIFS = [("M6", "six", "ACGTGA"), ("M7", "seven", "TTGACCA"), ("M8", "eight", "GGATCCAT")]      # (ID, NAME, consensus)
BASE = ["-v", "-y", "-p", "0.05", "-a", "20", "-t", "t0.sam,t1.sam", "-c", "c0.sam,null", "-E", "x.bed", "-o", "o.np"]
BASE_FILES = ["o.np"]
MORE = (["-f", "o.log", "-k", "o.pile", "-b", "o.bed"], ["o.log", "o.pile", "o.bed"])     # the combined runs write these as well


def _binary():
    from genrich_amd import build
    build.build()
    return build.HOST_BIN


def _inputs(d):
    two = LENS[:2]                                        # (the fragments are drawn on the first two chromosomes only)
    for name, n, seed, kw in (("t0", 400, 1, dict(frac_peak=0.5)), ("c0", 300, 2, dict(uniform_only=True)), ("t1", 350, 3, dict(frac_peak=0.5))):
        ev = synth.make_fragments(two, n, seed, peak_every=4000, tower_every=15_000, **kw)
        synth.write_sam_mixed(os.path.join(d, name + ".sam"), NAMES, LENS, ev, seed, name_prefix=name + "_", frac_single=0.04)
    with open(os.path.join(d, "x.bed"), "w") as f:
        f.write("chrA\t6000\t6400\n")
    with open(os.path.join(d, "sites.bed"), "w") as f:
        for c, s, e, nm, st in BED:
            f.write(f"{c}\t{s}\t{e}\t{nm}\t0\t{st}\n")
    rng = random.Random(7)
    with open(os.path.join(d, "g.fa"), "w") as f:
        for name, n in zip(NAMES, LENS):
            seq = "".join(rng.choice("ACGT") for _ in range(n))
            if name == "chrA":
                seq = seq[:3000] + "N" * 40 + seq[3040:]
            f.write(f">{name}\n" + "".join(seq[i:i + 60] + "\n" for i in range(0, n, 60)))
    with open(os.path.join(d, "m.jaspar"), "w") as f:
        for mid, name, cons in MOTIFS:          # 17 of 20 counts on the consensus base, one on each other
            f.write(f">{mid} {name}\n" + "".join(f"{b} [ " + " ".join("17" if c == b else "1" for c in cons) + " ]\n" for b in "ACGT"))
    return sorted(os.listdir(d))


def _run(tmp, tag, opts, files, gz=False):
    """One run in a directory of its own -> ({file: bytes}, stderr lines); exactly `files` (and nothing else) were written."""
    d = str(tmp / tag)
    os.makedirs(d)
    inputs = _inputs(d)
    res = subprocess.run([_binary()] + opts, cwd=d, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    made = sorted(set(os.listdir(d)) - set(inputs))
    assert made == sorted(f + (".gz" if gz else "") for f in files), (tag, made)
    read = (lambda p: gzip.open(p, "rb").read()) if gz else (lambda p: open(p, "rb").read())
    return {f: read(os.path.join(d, f + (".gz" if gz else ""))) for f in files}, SECONDS.sub("T s", res.stderr).splitlines()


def _figure_lines(lines, prefixes):
    return [l for l in lines if l.startswith(tuple(prefixes))]


@pytest.fixture(scope="module")
def combined(tmp_path_factory):
    opts = BASE + MORE[0] + [o for fo, _, _ in FIGURES.values() for o in fo]
    files = BASE_FILES + MORE[1] + [f for _, ff, _ in FIGURES.values() for f in ff]
    tmp = tmp_path_factory.mktemp("all")
    out, err = _run(tmp, "combined", opts, files)
    return dict(tmp=tmp, opts=opts, files=files, out=out, err=err)


def test_the_input_makes_every_writer_speak(combined):
    out, err = combined["out"], combined["err"]
    assert all(len(out[f]) > 0 for f in combined["files"])
    assert len(out["o.np"].splitlines()) >= 3                                   # peaks, on both chromosomes that have reads
    assert {l.split(b"\t")[0] for l in out["o.np"].splitlines()} == {b"chrA", b"chrB"}
    for name, (_, _, prefixes) in FIGURES.items():                              # every figure has -v lines, one per sample where it has them per sample
        for p in prefixes:
            n = len(_figure_lines(err, [p]))
            assert n >= 1, name
            if p.endswith(","):
                assert n == len(SAMPLES), (name, n)
    assert len(_figure_lines(err, ["  suggested -x"])) == 2                     # the two treatments: unpaired alignments, no extension chosen
    assert b"chrZ" in out["rc.tsv"] and b"chrZ" in out["prof.t0.matrix.tsv"]    # the chromosome that no header names keeps its rows
    assert "- control file #1 not provided -" in err


@pytest.mark.parametrize("name", list(FIGURES))
def test_a_figure_alone_is_the_figure_of_the_combined_run(combined, name):
    opts, files, prefixes = FIGURES[name]
    out, err = _run(combined["tmp"], name, BASE + opts, BASE_FILES + files)
    for f in BASE_FILES + files:
        assert out[f] == combined["out"][f], f
    assert _figure_lines(err, PREFIXES) == _figure_lines(combined["err"], prefixes)     # its lines, in order, and no other figure's
    rest = [l for l in combined["err"] if not l.startswith(tuple(PREFIXES))]
    assert [l for l in err if not l.startswith(tuple(PREFIXES))] == rest                # ... and around them the run's own


def test_two_contexts_write_the_same_files(combined):
    """(--saturation and --reproducibility take one device: every other figure)"""
    one_opts = [o for n in ONE_DEVICE for o in FIGURES[n][0]]
    one_files = [f for n in ONE_DEVICE for f in FIGURES[n][1]]
    opts = [o for o in combined["opts"] if o not in one_opts] + ["--devices", "0,0"]
    assert len(opts) == len(combined["opts"]) - len(one_opts) + 2
    files = [f for f in combined["files"] if f not in one_files]
    out, _ = _run(combined["tmp"], "two", opts, files)
    for f in files:
        assert out[f] == combined["out"][f], f


def test_gzipped_files_hold_the_same_bytes(combined):
    out, err = _run(combined["tmp"], "gz", combined["opts"] + ["-z"], combined["files"], gz=True)
    for f in combined["files"]:
        assert out[f] == combined["out"][f], f
    assert err == combined["err"]
