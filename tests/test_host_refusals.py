"""What the host program refuses before it reads or writes anything: every sentence of the validation block, the malformed
values of the nine strict integer options (two of them lists) and of the three doubles, which sentence wins when an argv breaks two
rules, the two refusals of --profile's BED that come just behind the block, -h's text and the line of GENRICH_THREADS_REPORT.
No GPU: every case ends before a device context is made.  Each case runs in an empty directory with relative file names and asserts
exit status 1, the exact stderr and that the directory is still empty afterwards."""
import gzip
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
USAGE = open(os.path.join(HERE, "host_usage.txt")).read()   # -h's text, recorded from the program before its sources were split

RUN = ["-t", "t.sam", "-o", "o.np"]                  # a whole run (the inputs do not exist: no case gets as far as opening them)
VIA = {"P": ["-P", "-f", "l.log", "-o", "o.np"],     # the three ways to a run without the figure's source
       "events": ["--events-only", "-t", "t.sam"],
       "X": ["-X", "-t", "t.sam"]}

# a figure's options, the sentence that refuses them without the intervals / pileups / alignments of the run (-P, --events-only) ...
NEEDS_RUN = [
    (["--count-regions", "r.bed", "--region-counts", "rc.tsv"], "--count-regions needs the intervals of this run (not with -P or --events-only)"),
    (["--coverage", "cov"], "--coverage needs the pileups of this run (not with -P or --events-only)"),
    (["--correlation", "corr.tsv"], "--correlation needs the pileups of this run (not with -P or --events-only)"),
    (["--spearman", "sp.tsv"], "--spearman needs the pileups of this run (not with -P or --events-only)"),
    (["--fingerprint", "fp.tsv"], "--fingerprint needs the pileups of this run (not with -P or --events-only)"),
    (["--complexity", "cx.tsv"], "--complexity needs the intervals of this run (not with -P or --events-only)"),
    (["--lengths", "len.tsv"], "--lengths, --lengths-metrics and --chrom-stats need the intervals of this run (not with -P or --events-only)"),
    (["--lengths-metrics", "lm.tsv"], "--lengths, --lengths-metrics and --chrom-stats need the intervals of this run (not with -P or --events-only)"),
    (["--chrom-stats", "cs.tsv"], "--lengths, --lengths-metrics and --chrom-stats need the intervals of this run (not with -P or --events-only)"),
    (["--xcor", "xc.tsv"], "--xcor and --xcor-metrics need the alignments of this run (not with -P or --events-only)"),
    (["--xcor-metrics", "xm.tsv"], "--xcor and --xcor-metrics need the alignments of this run (not with -P or --events-only)"),
    (["--depth", "d.tsv"], "--depth and --depth-metrics need the pileups of this run (not with -P or --events-only)"),
    (["--depth-metrics", "dm.tsv"], "--depth and --depth-metrics need the pileups of this run (not with -P or --events-only)"),
    (["--profile", "a.bed", "--profile-out", "prof"], "--profile needs the pileups of this run (not with -P or --events-only)"),
]
# ... and without its peaks as well (-X too)
NEEDS_PEAKS = [
    (["--counts", "c.tsv"], "--counts needs the peaks of this run (not with -P or -X)"),
    (["--peak-signal", "ps.tsv"], "--peak-signal needs the peaks and the intervals of this run (not with -X, -P or --events-only)"),
    (["--saturation", "sat.tsv"], "--saturation needs the peaks and the intervals of this run (not with -X, -P or --events-only)"),
    (["--summits", "sm.tsv"], "--summits needs the peaks and the intervals of this run (not with -X, -P or --events-only)"),
    (["--reproducibility", "rp.tsv"], "--reproducibility needs the peaks and the intervals of this run (not with -X, -P or --events-only)"),
    (["--reproducibility-metrics", "rm.tsv"], "--reproducibility needs the peaks and the intervals of this run (not with -X, -P or --events-only)"),
    (["--motifs", "m.jaspar", "--genome", "g.fa", "--motif-hits", "mh.tsv"], "--motifs needs the peaks of this run on a device (not with -X, -P or --events-only)"),
    (["--gc-peaks", "gp.tsv", "--genome", "g.fa"], "--gc-peaks needs the peaks of this run on a device (not with -X, -P or --events-only)"),
]
NEEDS_RUN.append((["--gc-bias", "gc.tsv", "--genome", "g.fa"], "--gc-bias needs the intervals of this run (not with -P or --events-only)"))

CASES = {}
for opts, msg in NEEDS_RUN + NEEDS_PEAKS:
    for via in ("P", "events") + (("X",) if (opts, msg) in NEEDS_PEAKS else ()):
        CASES[f"{opts[0]} via {via}"] = (VIA[via] + opts, msg)

REPRO_NEED = ("--reproducibility-overlap, --reproducibility-seed and --reproducibility-peaks need --reproducibility FILE or "
              "--reproducibility-metrics FILE")
MOTIF_NEED = "--motif-hits, --motif-summary, --motif-pvalue and --motif-pseudocount need --motifs FILE"
MANY = ",".join(f"t{i}.sam" for i in range(33))      # 33 samples
CASES.update({
    # the sentences that do not depend on the kind of run, in the order of the block
    "stray argument": (RUN + ["stray"], "stray: unknown command-line argument"),
    "regions without their output": (RUN + ["--count-regions", "r.bed"], "--count-regions BED and --region-counts FILE need each other"),
    "region output without regions": (RUN + ["--region-counts", "rc.tsv"], "--count-regions BED and --region-counts FILE need each other"),
    "skip-zeros alone": (RUN + ["--corr-skip-zeros"], "--corr-skip-zeros needs --correlation FILE or --spearman FILE"),
    "fingerprint metrics alone": (RUN + ["--fingerprint-metrics", "fm.tsv"], "--fingerprint-metrics needs --fingerprint FILE"),
    "complexity hist alone": (RUN + ["--complexity-hist", "ch.tsv"], "--complexity-hist needs --complexity FILE"),
    "lengths cuts alone": (RUN + ["--lengths", "len.tsv", "--lengths-cuts", "100,200"], "--lengths-cuts needs --lengths-metrics FILE"),
    "xcor shifts alone": (RUN + ["--xcor-shifts", "0,100"], "--xcor-shifts, --xcor-read-length and --xcor-unpaired need --xcor FILE or --xcor-metrics FILE"),
    "xcor read length alone": (RUN + ["--xcor-read-length", "36"], "--xcor-shifts, --xcor-read-length and --xcor-unpaired need --xcor FILE or --xcor-metrics FILE"),
    "xcor unpaired alone": (RUN + ["--xcor-unpaired"], "--xcor-shifts, --xcor-read-length and --xcor-unpaired need --xcor FILE or --xcor-metrics FILE"),
    "saturation steps alone": (RUN + ["--saturation-steps", "5"], "--saturation-steps, --saturation-seed and --saturation-controls need --saturation FILE"),
    "saturation seed alone": (RUN + ["--saturation-seed", "5"], "--saturation-steps, --saturation-seed and --saturation-controls need --saturation FILE"),
    "saturation controls alone": (RUN + ["--saturation-controls"], "--saturation-steps, --saturation-seed and --saturation-controls need --saturation FILE"),
    "saturation steps 0": (RUN + ["--saturation", "sat.tsv", "--saturation-steps", "0"], "--saturation-steps must be in [1, 100]"),
    "saturation steps 101": (RUN + ["--saturation", "sat.tsv", "--saturation-steps", "101"], "--saturation-steps must be in [1, 100]"),
    "saturation on two devices": (RUN + ["--saturation", "sat.tsv", "--devices", "0,1"], "--saturation takes one device (not with --devices of more than one)"),
    "33 samples, correlation": (["-t", MANY, "-o", "o.np", "--correlation", "corr.tsv"], "--correlation takes at most 32 samples"),
    "33 samples, spearman": (["-t", MANY, "-o", "o.np", "--spearman", "sp.tsv"], "--spearman takes at most 32 samples"),
    "33 samples, fingerprint": (["-t", MANY, "-o", "o.np", "--fingerprint", "fp.tsv"], "--fingerprint takes at most 32 samples"),
    "33 samples, 17 of them controls": (["-t", ",".join(f"t{i}.sam" for i in range(17)), "-c", ",".join(["null"] + [f"c{i}.sam" for i in range(16)]),
                                        "-o", "o.np", "--fingerprint", "fp.tsv"], "--fingerprint takes at most 32 samples"),
    "bin size alone": (RUN + ["--bin-size", "100"], "--bin-size and --coverage-scale need --coverage PREFIX"),
    "coverage scale without coverage": (RUN + ["--correlation", "corr.tsv", "--coverage-scale", "2"], "--bin-size and --coverage-scale need --coverage PREFIX"),
    "bin size 0": (RUN + ["--coverage", "cov", "--bin-size", "0"], "--bin-size must be in [1, 1048576]"),
    "bin size too large": (RUN + ["--spearman", "sp.tsv", "--bin-size", "1048577"], "--bin-size must be in [1, 1048576]"),
    "profile without its output": (RUN + ["--profile", "a.bed"], "--profile BED and --profile-out PREFIX need each other"),
    "profile output without its BED": (RUN + ["--profile-out", "prof"], "--profile BED and --profile-out PREFIX need each other"),
    "flank alone": (RUN + ["--flank", "100"], "--flank, --profile-bin, --profile-at and --profile-matrix need --profile BED"),
    "profile matrix alone": (RUN + ["--profile-matrix"], "--flank, --profile-bin, --profile-at and --profile-matrix need --profile BED"),
    "profile bin 0": (RUN + ["--profile", "a.bed", "--profile-out", "prof", "--profile-bin", "0"], "--profile: --profile-bin must be at least 1"),
    "flank 0": (RUN + ["--profile", "a.bed", "--profile-out", "prof", "--flank", "0"], "--profile: --flank must be in [1, 1048576]"),
    "flank no multiple": (RUN + ["--profile", "a.bed", "--profile-out", "prof", "--flank", "105"], "--profile: --flank must be a multiple of --profile-bin"),
    "too many profile bins": (RUN + ["--profile", "a.bed", "--profile-out", "prof", "--flank", "2000", "--profile-bin", "1"],
                              "--profile: at most 1024 bins (2 * flank / profile-bin)"),
    "profile-at": (RUN + ["--profile-at", "end"], "end: --profile-at takes tss or center"),
    "extension 0": (RUN + ["-w", "0"], "Extension length must be > 0"),
    "ATAC length 0": (RUN + ["-j", "-d", "0"], "ATAC-seq interval length must be > 0"),
    "negative peak length": (RUN + ["-l", "-1"], "Minimum peak length must be >= 0"),
    "negative AUC": (RUN + ["-a", "-1"], "Minimum AUC must be >= 0.0"),
    "negative score difference": (RUN + ["-s", "-1"], "Secondary alignment score threshold must be >= 0.0"),
    "p-value 0": (RUN + ["-p", "0"], "p-/q-value must be in (0,1]"),
    "q-value above 1": (RUN + ["-q", "1.5"], "p-/q-value must be in (0,1]"),
    "coverage scale, not a number": (RUN + ["--coverage-scale", "x"], "x: cannot convert to float"),
    "65 devices": (RUN + ["--devices", "0-64"], "at most 64 devices"),
    "summits prominence alone": (RUN + ["--summits-prominence", "30"], "--summits-prominence and --summits-height need --summits FILE"),
    "summits height alone": (RUN + ["--summits-height", "30"], "--summits-prominence and --summits-height need --summits FILE"),
    "reproducibility overlap alone": (RUN + ["--reproducibility-overlap", "30"], REPRO_NEED),
    "reproducibility seed alone": (RUN + ["--reproducibility-seed", "3"], REPRO_NEED),
    "reproducibility peaks alone": (RUN + ["--reproducibility-peaks", "rp"], REPRO_NEED),
    "reproducibility on two devices": (RUN + ["--reproducibility", "rp.tsv", "--devices", "0,1"], "--reproducibility takes one device (not with --devices of more than one)"),
    "reproducibility metrics on two devices": (RUN + ["--reproducibility-metrics", "rm.tsv", "--devices", "0,1"],
                                               "--reproducibility takes one device (not with --devices of more than one)"),
    "gc bias without genome": (RUN + ["--gc-bias", "gc.tsv"], "--gc-bias needs the reference sequence (--genome FASTA)"),
    "gc peaks without genome": (RUN + ["--gc-peaks", "gp.tsv"], "--gc-peaks needs the reference sequence (--genome FASTA)"),
    "gc window alone": (RUN + ["--gc-window", "100"], "--gc-window needs --gc-bias FILE"),
    "gc window with gc peaks only": (RUN + ["--gc-peaks", "gp.tsv", "--genome", "g.fa", "--gc-window", "100"], "--gc-window needs --gc-bias FILE"),
    "motifs without genome": (RUN + ["--motifs", "m.jaspar", "--motif-hits", "mh.tsv"], "--motifs needs the reference sequence (--genome FASTA)"),
    "motifs without either output": (RUN + ["--motifs", "m.jaspar", "--genome", "g.fa"], "--motifs needs --motif-hits FILE or --motif-summary FILE"),
    "motif hits alone": (RUN + ["--motif-hits", "mh.tsv"], MOTIF_NEED),
    "motif summary alone": (RUN + ["--motif-summary", "ms.tsv"], MOTIF_NEED),
    "motif pvalue alone": (RUN + ["--motif-pvalue", "0.001"], MOTIF_NEED),
    "motif pseudocount alone": (RUN + ["--motif-pseudocount", "2"], MOTIF_NEED),
    "genome alone": (RUN + ["--genome", "g.fa"], "--genome needs --gc-bias FILE or --gc-peaks FILE"),
    # two rules broken at once: the first of the block wins, and among the options' own values the first of the argv
    "counts with -P, and metrics without fingerprint": (VIA["P"] + ["--counts", "c.tsv", "--fingerprint-metrics", "fm.tsv"],
                                                        "--counts needs the peaks of this run (not with -P or -X)"),
    "metrics without fingerprint, and complexity with -P": (VIA["P"] + ["--complexity", "cx.tsv", "--fingerprint-metrics", "fm.tsv"],
                                                            "--fingerprint-metrics needs --fingerprint FILE"),
    "bin size 0 and coverage scale alone": (RUN + ["--bin-size", "0", "--coverage-scale", "2"], "--bin-size and --coverage-scale need --coverage PREFIX"),
    "33 samples, correlation and spearman": (["-t", MANY, "-o", "o.np", "--spearman", "sp.tsv", "--correlation", "corr.tsv"],
                                             "--correlation takes at most 32 samples"),
    "33 samples, spearman and fingerprint": (["-t", MANY, "-o", "o.np", "--fingerprint", "fp.tsv", "--spearman", "sp.tsv"], "--spearman takes at most 32 samples"),
    "33 samples and bin size 0": (["-t", MANY, "-o", "o.np", "--fingerprint", "fp.tsv", "--bin-size", "0"], "--fingerprint takes at most 32 samples"),
    "bin size 0 and profile without output": (RUN + ["--coverage", "cov", "--bin-size", "0", "--profile", "a.bed"], "--bin-size must be in [1, 1048576]"),
    "extension 0 and ATAC length 0": (RUN + ["-j", "-d", "0", "-w", "0"], "Extension length must be > 0"),
    "counts with -X and extension 0": (VIA["X"] + ["--counts", "c.tsv", "-w", "0"], "--counts needs the peaks of this run (not with -P or -X)"),
    "p-value 2 and negative peak length": (RUN + ["-p", "2", "-l", "-1"], "Minimum peak length must be >= 0"),
    "saturation steps 0 on two devices": (RUN + ["--saturation", "sat.tsv", "--devices", "0,1", "--saturation-steps", "0"], "--saturation-steps must be in [1, 100]"),
    "saturation with -X and steps 0": (VIA["X"] + ["--saturation", "sat.tsv", "--saturation-steps", "0"],
                                       "--saturation needs the peaks and the intervals of this run (not with -X, -P or --events-only)"),
    "complexity hist alone and lengths cuts alone": (RUN + ["--lengths-cuts", "1", "--complexity-hist", "ch.tsv"], "--complexity-hist needs --complexity FILE"),
    "two malformed values": (RUN + ["--xcor-read-length", "0", "--saturation-seed", "x"], "0: --xcor-read-length takes a positive integer (at most 1000000)"),
    "a malformed value and a stray argument": (RUN + ["stray", "--saturation-seed", "x"], "x: --saturation-seed takes an integer in [0, 2^64 - 1]"),
    "gc bias with -P and no genome": (VIA["P"] + ["--gc-bias", "gc.tsv"], "--gc-bias needs the reference sequence (--genome FASTA)"),
    "summits with -X and its height": (VIA["X"] + ["--summits", "sm.tsv", "--summits-height", "40"],
                                       "--summits needs the peaks and the intervals of this run (not with -X, -P or --events-only)"),
    "summits height alone and counts with -X": (VIA["X"] + ["--summits-height", "40", "--counts", "c.tsv"], "--counts needs the peaks of this run (not with -P or -X)"),
    "summits height alone and regions with -P": (VIA["P"] + ["--summits-height", "40", "--count-regions", "r.bed", "--region-counts", "rc.tsv"],
                                                 "--summits-prominence and --summits-height need --summits FILE"),
    "motifs with -P and no outputs": (VIA["P"] + ["--motifs", "m.jaspar", "--genome", "g.fa"], "--motifs needs --motif-hits FILE or --motif-summary FILE"),
    "motifs with -X and gc bias with -P's sentence behind it": (VIA["X"] + ["--motifs", "m.jaspar", "--genome", "g.fa", "--motif-summary", "ms.tsv", "--gc-peaks", "gp.tsv"],
                                                               "--motifs needs the peaks of this run on a device (not with -X, -P or --events-only)"),
    "genome alone with -P": (VIA["P"] + ["--genome", "g.fa"], "--genome needs --gc-bias FILE or --gc-peaks FILE"),
    "reproducibility with -X on two devices": (VIA["X"] + ["--reproducibility", "rp.tsv", "--devices", "0,1", "--reproducibility-seed", "2"],
                                               "--reproducibility needs the peaks and the intervals of this run (not with -X, -P or --events-only)"),
    "saturation and reproducibility on two devices": (RUN + ["--reproducibility", "rp.tsv", "--saturation", "sat.tsv", "--devices", "0,1"],
                                                      "--saturation takes one device (not with --devices of more than one)"),
    "stray argument and no files": (["stray"], "stray: unknown command-line argument"),
    # a sign where the range reaches below zero is no malformed value: the argv gets as far as the validation block
    "xcor shifts with signs": (RUN + ["--xcor-shifts", "-5,+10"], "--xcor-shifts, --xcor-read-length and --xcor-unpaired need --xcor FILE or --xcor-metrics FILE"),
})

# the strict integer options: empty, sign, trailing text, trailing blank, out of range, beyond 64 bits, leading blank (and for the
# lists, their own rules)
BIG = "99999999999999999999"    # (beyond 64 bits)
MALFORMED = {
    "--xcor-read-length": (": --xcor-read-length takes a positive integer (at most 1000000)", ["", "+36", "-36", "36x", "36 ", "0", "1000001", BIG, " 36", "x"]),
    "--saturation-seed": (": --saturation-seed takes an integer in [0, 2^64 - 1]", ["", "+1", "-1", "1x", "1 ", "18446744073709551616", BIG, " 1", "x"]),
    "--lengths-cuts": (": --lengths-cuts takes at most 8 ascending positive integers, A,B,...",
                       ["", "+150", "-150", "150x", "150,300x", "0", "4294967296", BIG, " 150", "150, 300", "150,", ",150", "150,,300",
                        "1,2,3,4,5,6,7,8,9", "300,150", "150,150"]),
    "--xcor-shifts": (": --xcor-shifts takes two integers LO,HI with -4096 <= LO <= HI <= 4096",
                      ["", "5", "5,", ",5", "5,6x", "5x,6", "5,6,7", "x", "-4097,0", "0,4097", BIG + ",5", "5," + BIG, " 5,6", "5, 6", "10,5", "- 5,6", "5,-+6"]),
}
PCT = ["", "+5", "-5", "5x", "5 ", "-1", "101", BIG, " 5", "x"]      # (an integer in [0, 100])
MALFORMED.update({
    "--reproducibility-overlap": (": --reproducibility-overlap takes an integer in [0, 100]", PCT),
    "--reproducibility-seed": (": --reproducibility-seed takes an integer in [0, 2^64 - 1]", ["", "+1", "-1", "1x", "1 ", "18446744073709551616", BIG, " 1", "x"]),
    "--summits-prominence": (": --summits-prominence takes an integer in [0, 100]", PCT),
    "--summits-height": (": --summits-height takes an integer in [0, 100]", PCT),
    "--gc-window": (": --gc-window takes an integer in [1, 4096]", ["", "+200", "-200", "200x", "200 ", "0", "4097", BIG, " 200", "x"]),
    # the three doubles: strtod's whole argument (a leading blank is strtod's to skip), and for the motifs' two their ranges
    "--coverage-scale": (": cannot convert to float", ["", "x", "1x", "1 "]),
    "--motif-pvalue": (": --motif-pvalue takes a number in (0, 1]", ["", "x", "1x", "1 ", "nan", "inf", "-inf", "0", "-0.5", "1.0000001", "1e400"]),
    "--motif-pseudocount": (": --motif-pseudocount takes a number >= 0", ["", "x", "1x", "1 ", "nan", "inf", "-1e-9", "-1", "1e400"]),
})
for opt, (tail, values) in MALFORMED.items():
    for v in values:
        CASES[f"{opt} {v!r}"] = (RUN + [opt, v], v + tail)
# ... and the ends of their ranges are no malformed values: the argv gets as far as the sentence that asks for the figure
ENDS = {
    "--xcor-read-length": (["1", "1000000"], "--xcor-shifts, --xcor-read-length and --xcor-unpaired need --xcor FILE or --xcor-metrics FILE"),
    "--saturation-seed": (["0", "18446744073709551615"], "--saturation-steps, --saturation-seed and --saturation-controls need --saturation FILE"),
    "--reproducibility-overlap": (["0", "100"], REPRO_NEED),
    "--reproducibility-seed": (["0", "18446744073709551615"], REPRO_NEED),
    "--summits-prominence": (["0", "100"], "--summits-prominence and --summits-height need --summits FILE"),
    "--summits-height": (["0", "100"], "--summits-prominence and --summits-height need --summits FILE"),
    "--gc-window": (["1", "4096"], "--gc-window needs --gc-bias FILE"),
    "--coverage-scale": (["nan", "inf", "-1", " 1", "1e400"], "--bin-size and --coverage-scale need --coverage PREFIX"),      # (any double)
    "--motif-pvalue": (["1", "1e-300", " 0.5"], MOTIF_NEED),
    "--motif-pseudocount": (["0", "1e300"], MOTIF_NEED),
}
for opt, (values, msg) in ENDS.items():
    for v in values:
        CASES[f"{opt} {v!r} is a value"] = (RUN + [opt, v], msg)


def _binary():
    from genrich_amd import build
    if not os.path.exists(build.LIB):       # (the program links the library; a tree that has it only needs the program)
        build.build()
    return build.build_host()


def _run(argv, cwd, env=None):
    res = subprocess.run([_binary()] + argv, cwd=cwd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert os.listdir(cwd) == [], (argv, os.listdir(cwd))     # refused: not one file was made, under any name
    assert res.returncode == 1 and res.stdout == "", (argv, res.returncode, res.stdout)
    return res.stderr


@pytest.mark.parametrize("name", list(CASES))
def test_refusal(name, tmp_path):
    argv, msg = CASES[name]
    assert _run(argv, tmp_path) == f"Error! {msg}\n"


PROFILE = RUN + ["--profile", "a.bed", "--profile-out", "prof"]


@pytest.mark.parametrize("lines, more, msg", [
    (0, [], "a.bed: --profile: no anchors"),
    (0, ["--profile-matrix", "--flank", "1048576", "--profile-bin", "2048"], "a.bed: --profile: no anchors"),
    ((1 << 16) + 1, ["--profile-matrix", "--flank", "1048576", "--profile-bin", "2048"], "--profile-matrix: more than 2^26 cells (BED lines times bins)"),
], ids=["no anchors", "no anchors, matrix", "2^26 cells and 1024 more"])
def test_the_refusals_of_the_anchors(lines, more, msg, tmp_path):
    """The two that come just behind the block, when --profile's BED has been read: the BED is the one file in the directory, and
    it is still the only one afterwards.  (A BED without a line is a gzip of nothing: an empty plain file cannot be opened.  2^16
    lines times 1024 bins are 2^26 cells, which are allowed: one line more)"""
    (tmp_path / "a.bed").write_bytes(gzip.compress(b"chr1\t0\t1\n" * lines, 1))
    res = subprocess.run([_binary()] + PROFILE + more, cwd=tmp_path, capture_output=True, text=True)
    assert os.listdir(tmp_path) == ["a.bed"]
    assert (res.returncode, res.stdout, res.stderr) == (1, "", f"Error! {msg}\n")


@pytest.mark.parametrize("argv", [[], ["-t", "t.sam"], ["-P", "-o", "o.np"], ["-o", "o.np"], ["-P", "-f", "l.log"],
                                  ["-t", "t.sam", "--counts", "c.tsv", "-P", "-w", "0"]], ids=" ".join)
def test_missing_files_print_the_usage(argv, tmp_path):
    """(the last one breaks two more rules: the files are asked for first)"""
    assert _run(argv, tmp_path) == "Error! Need input/output files\n" + USAGE


def test_help(tmp_path):
    assert _run(["-h"], tmp_path) == USAGE
    assert _run(["--help", "--counts", "c.tsv", "-P"], tmp_path) == USAGE
    assert _run(["--saturation-seed", "x", "-h"], tmp_path) == "Error! x: --saturation-seed takes an integer in [0, 2^64 - 1]\n"


THREADS_LINE = re.compile(r"\[threads\] inflate (\d+), decode (\d+), state (\d+); BAM: inflate (\d+), decode (\d+), state (\d+)\n")


@pytest.mark.parametrize("n", [1, 4, 16])
@pytest.mark.parametrize("how", ["--threads", "GENRICH_THREADS"])
def test_threads_report(n, how, tmp_path):
    """The split of --threads N depends on the host's cores: the line's format, and what the code states about the numbers."""
    argv, env = ["--events-only", "-t", "t.sam"], {"GENRICH_THREADS_REPORT": "1"}
    if how == "--threads":
        argv += ["--threads", str(n)]
    else:
        env["GENRICH_THREADS"] = str(n)
    err = _run(argv, tmp_path, env)
    tail = "Error! t.sam: cannot open file for reading\n"      # (the line comes after the validation block and before any input)
    assert err.endswith(tail)
    m = THREADS_LINE.fullmatch(err[:-len(tail)])
    assert m, err
    inf, dec, st, binf, bdec, bst = map(int, m.groups())
    if n == 1:      # one thread does it all, on any host
        assert (inf, dec, st, binf, bdec, bst) == (1,) * 6
        return
    assert inf >= 2 and binf >= 2                       # two inflaters keep the BGZF reader with its block checks
    assert st <= dec and bst <= bdec                    # never more state workers than decoders
    assert binf >= inf and bdec <= dec and bst <= st    # a BAM stream moves threads towards inflating, never away from it
    assert max(dec, st, bdec, bst, inf) <= n and binf <= 2 * n
    if (inf, dec, st) != (n, n, n):                     # a small host (fewer than 3 N + 2 cores): the pools share the budget
        assert (inf, dec, st) == (max(2, n // 4), max(2, n // 2), max(1, n // 2))
        assert (binf, bdec, bst) == (max(2, n // 2), max(2, n // 4), max(1, n // 4))
    else:
        assert (bdec, bst) == (n, n) and n <= binf


def test_a_report_does_not_change_a_refusal(tmp_path):
    """(and it stands between the block's last two sentences: behind -s's, in front of -p's)"""
    err = _run(["--threads", "4", "-t", "t.sam", "-o", "o.np", "-p", "0"], tmp_path, {"GENRICH_THREADS_REPORT": "1"})
    tail = "Error! p-/q-value must be in (0,1]\n"
    assert err.endswith(tail) and THREADS_LINE.fullmatch(err[:-len(tail)]), err
    assert _run(["--threads", "4", "-t", "t.sam", "-o", "o.np", "-p", "0", "-s", "-1"], tmp_path, {"GENRICH_THREADS_REPORT": "1"}) == (
        "Error! Secondary alignment score threshold must be >= 0.0\n")
