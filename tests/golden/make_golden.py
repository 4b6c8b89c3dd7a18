#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ by running the UNMODIFIED reference
(oracle/_ref/Genrich, built by oracle/Makefile from /root/reference) on small synthetic
SAM files.  Run in the build container only:  python tests/golden/make_golden.py

Per case the fixture holds DATA only:
  case.json          chromosome table, -e/-E, per-replicate `save` flags, parameters, the
                     scalars the reference printed under -v (lambda, factor, genome length,
                     peak count / bp)
  events.bed.gz      the reference's own -b output = the post-clamp event list
                     (chr start end name_count_[E|C]_sample; Genrich.c:2497-2508)
  out.narrowPeak.gz, out.log.gz (-f), out.pile.gz (-k)   the reference's outputs
The SAM inputs are regenerated from tests/synth.py and are not committed.
"""
import gzip
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "Genrich")


def merged_bed(regions, clen):
    """saveXBed's sort + clamp + merge (Genrich.c:1144-1206) for one chromosome."""
    iv = sorted([list(r) for r in regions if r[0] < clen], key=lambda r: r[0])
    out = []
    for s, e in iv:
        e = min(e, clen)
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return [c for r in out for c in r]


def multimap_reads(lens, n_reads, seed, hot=0.75):
    """Reads with 1..12 equally scored alignments (exercises counts 2,3,4,5,6,8,10 and the
    7 / 9 / >10 subsampling, Genrich.c:3145-3146)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = []
    for _ in range(n_reads):
        k = int(rng.integers(1, 13))
        for _a in range(k):
            c = int(rng.integers(0, len(lens)))
            fl = int(100 + rng.integers(0, 150))
            s = int(rng.integers(0, lens[c] - fl))
            # pull most of the alignments towards a few hot spots so peaks exist
            if rng.random() < hot:
                s = int(min(max(0, (s // 10000) * 10000 + 5000 + rng.integers(-60, 60)), lens[c] - fl))
            rows.append((c, s, s + fl, k))
    return np.array(rows, dtype=synth.EVENT_DTYPE)


def mf(lens, n, seed, peak_every=8000, tower_every=30000, **kw):
    """Strongly enriched stream so that the tiny genomes still yield peaks and q < 1."""
    if kw.get("uniform_only"):
        return synth.make_fragments(lens, n, seed, **kw)
    return synth.make_fragments(lens, n, seed, peak_every, tower_every, frac_peak=0.4,
                                frac_tower=0.3, **kw)


def int16_towers(lens, n_start, n_end, seed):
    """n_start fragments [1000, 1200), n_end fragments that all end at 5400 (starts spread over 50 bases) and some
    background, in random order."""
    rng = np.random.Generator(np.random.PCG64(seed))
    bg = mf(lens, 1500, seed + 1000)
    a = np.zeros(n_start, dtype=synth.EVENT_DTYPE)
    a["start"], a["end"], a["count"] = 1000, 1200, 1
    b = np.zeros(n_end, dtype=synth.EVENT_DTYPE)
    b["start"] = 5000 + 2 * rng.integers(0, 50, n_end)
    b["end"], b["count"] = 5400, 1
    ev = np.concatenate([bg, a, b])
    return ev[rng.permutation(len(ev))]


def int16_towers_frac(lens, n_start, n_end, seed):
    """As int16_towers, with a third of the tower reads multimapped (k = 2 .. 10 equally scored alignments, weight 1 / k):
    one alignment on the tower, the others elsewhere -- the int16 part of the reference's (cov, eighths, sixths, tenths)
    counters reaches its limits in between whole numbers.  Consecutive events with count = k are one read (write_sam)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    reads = [[(0, int(s), int(e), 1)] for _, s, e, _ in mf(lens, 1500, seed + 1000)]
    L = lens[0]

    def multi(first, k):
        out = [first + (k,)]
        for _ in range(k - 1):
            s = 10_000 + 1_000 * int(rng.integers(0, 40))
            out.append((0, s, s + 150 + 10 * int(rng.integers(0, 8)), k))
        perm = rng.permutation(k)
        return [out[j] for j in perm]

    for _ in range(n_start):
        k = int(rng.choice([1, 1, 1, 1, 2, 3, 4, 5, 6, 8, 10]))
        reads.append(multi((0, 1000, 1200), k) if k > 1 else [(0, 1000, 1200, 1)])
    for _ in range(n_end):
        k = int(rng.choice([1, 1, 1, 1, 2, 3, 4, 5, 6, 8, 10]))
        st = 5000 + 2 * int(rng.integers(0, 50))
        reads.append(multi((0, st, 5400), k) if k > 1 else [(0, st, 5400, 1)])
    order = rng.permutation(len(reads))
    rows = [a for i in order for a in reads[i]]
    return np.array(rows, dtype=synth.EVENT_DTYPE)


# CPU-only fixtures of tests/test_host_cli.py::test_cli_int16_decisions_more: the reference's -b list (hash + line count) and
# its read-by-read warnings.  Not `cases` (no case.json): the suites that walk every case leave them alone.
def int16_extra():
    L1 = [60_000]
    return {
        # a third of the piled-up reads multimapped
        "saturate16_frac": dict(ev=lambda: int16_towers_frac(L1, 100_000, 100_000, 71), mixed=None, args=["-a", "20"]),
        # ATAC cut sites (-j -d 40): two intervals per fragment, either of which can be the one that is dropped -- the
        # fragment's length towards the -x average is then the other one's; unpaired reads kept (-y)
        "saturate16_atac": dict(ev=lambda: int16_towers(L1, 47_600, 47_400, 81), mixed=dict(seed=6, bam=False),
                                args=["-j", "-d", "40", "-y", "-a", "20"]),
    }


def make_int16_extra(name):
    import hashlib
    spec = int16_extra()[name]
    L1 = [60_000]
    out_dir = os.path.join(HERE, name)
    os.makedirs(out_dir, exist_ok=True)
    tmp = os.path.join("/tmp/genrich_golden", name)
    shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(tmp)
    sam = os.path.join(tmp, "t0.sam")
    write_input(sam, ["chrA"], L1, spec["ev"](), spec["mixed"], 0, "t0_")
    res = subprocess.run([REF, "-t", sam, "-v", "-b", os.path.join(tmp, "events.bed"), "-o", os.path.join(tmp, "o.np")] + spec["args"],
                         capture_output=True, text=True)
    if res.returncode != 0:
        sys.exit(name + ": reference failed:\n" + res.stderr)
    bed = open(os.path.join(tmp, "events.bed"), "rb").read()
    with open(os.path.join(out_dir, "events.bed.sha256"), "w") as f:  # (megabytes of lines: their hash and count are kept)
        f.write(f"{hashlib.sha256(bed).hexdigest()} {bed.count(10)}\n")
    with gzip.GzipFile(os.path.join(out_dir, "out.int16.gz"), "wb", mtime=0) as g:
        g.write("".join(l + "\n" for l in res.stderr.splitlines() if "skipped due to" in l).encode())
    n = sum(1 for l in res.stderr.splitlines() if "skipped due to" in l)
    print(f"{name:18s} {n} alignments skipped by the reference")
    shutil.rmtree(tmp)


def cases():
    L1 = [60_000]
    yield dict(
        name="basic", names=["chrA"], args=[],
        reps=[dict(t=(["chrA"], L1, mf(L1, 3000, 11)), c=None)])

    L2 = [40_000, 25_000]
    N2 = ["chr1", "chr2"]
    yield dict(
        name="ctrl_q", names=N2, args=["-q", "0.3", "-a", "20"],
        reps=[dict(t=(N2, L2, mf(L2, 3000, 21)),
                   c=(N2, L2, mf(L2, 2500, 22, uniform_only=True)))])

    yield dict(
        name="multimap", names=N2, args=["-p", "0.05", "-a", "5", "-g", "50"],
        reps=[dict(t=(N2, L2, multimap_reads(L2, 1200, 31)),
                   c=(N2, L2, multimap_reads(L2, 600, 32, hot=0.0)))])

    yield dict(
        name="atac", names=N2, args=["-j", "-a", "50"],
        reps=[dict(t=(N2, L2, mf(L2, 2500, 41)), c=None)])

    yield dict(
        name="atac_odd", names=N2, args=["-j", "-d", "151", "-q", "0.5", "-a", "10", "-l", "40"],
        reps=[dict(t=(N2, L2, mf(L2, 2500, 42, min_len=30)),
                   c=(N2, L2, mf(L2, 2000, 43, uniform_only=True)))])

    yield dict(
        name="reps3", names=N2, args=["-q", "0.2", "-a", "30"],
        reps=[dict(t=(N2, L2, mf(L2, 2000, 51)),
                   c=(N2, L2, mf(L2, 2000, 52, uniform_only=True))),
              dict(t=(N2, L2, mf(L2, 2200, 53)), c="null"),
              dict(t=(N2, L2, mf(L2, 1800, 55)),
                   c=(N2, L2, mf(L2, 1500, 56, uniform_only=True)))])

    # three replicates, p-value mode, one replicate lacks chr2 (NULL padding, 1735-1750)
    yield dict(
        name="reps3_p_missing", names=N2, args=["-a", "100"],
        reps=[dict(t=(N2, L2, mf(L2, 2000, 61)), c=None),
              dict(t=(N2[:1], L2[:1], mf(L2[:1], 1500, 62)), c=None),
              dict(t=(N2, L2, mf(L2, 1800, 63)), c=None)])

    # five replicates (combinePval's union beyond four inputs), controls mixed file / null / file / null / file, one replicate
    # lacks chr2 -- fewer fragments per sample than reps3, so that the directory stays no larger
    yield dict(
        name="reps5_mixed", names=N2, args=["-q", "0.2", "-a", "20"],
        reps=[dict(t=(N2, L2, mf(L2, 800, 131)), c=(N2, L2, mf(L2, 700, 132, uniform_only=True))),
              dict(t=(N2, L2, mf(L2, 900, 133)), c="null"),
              dict(t=(N2, L2, mf(L2, 700, 134)), c=(N2, L2, mf(L2, 600, 135, uniform_only=True))),
              dict(t=(N2[:1], L2[:1], mf(L2[:1], 600, 136)), c="null"),
              dict(t=(N2, L2, mf(L2, 800, 137)), c=(N2, L2, mf(L2, 700, 138, uniform_only=True)))])

    # nine replicates without controls, p-value mode, one lacks chr2; a -E region on chr1: the intervals inside it are
    # skipped in every replicate, so the degrees of freedom of multPval vary along the chromosome
    yield dict(
        name="reps9", names=N2, args=["-p", "0.01", "-a", "20"], bed=[("chr1", 11_000, 17_500)],
        reps=[dict(t=((N2[:1], L2[:1], mf(L2[:1], 450, 141 + r)) if r == 6 else (N2, L2, mf(L2, 600 + 40 * r, 141 + r))), c=None)
              for r in range(9)])

    L3 = [30_000, 20_000, 8_000]
    N3 = ["chr1", "chr2", "chrX"]
    yield dict(
        name="bedx", names=N3, args=["-e", "chrX", "-a", "40", "-q", "0.2"],
        bed=[("chr1", 0, 1500), ("chr1", 9000, 9800), ("chr1", 9500, 11000),
             ("chr1", 29000, 31000), ("chr2", 5000, 5001), ("chr2", 19990, 20000),
             ("chr2", 25000, 26000)],
        reps=[dict(t=(N3, L3, mf(L3, 3000, 71)),
                   c=(N3, L3, mf(L3, 2500, 72, uniform_only=True)))])

    yield dict(
        name="bedx_noctrl", names=N3, args=["-a", "40"],
        bed=[("chr1", 0, 1500), ("chr1", 12000, 13000), ("chr2", 19000, 20000)],
        reps=[dict(t=(N3, L3, mf(L3, 3000, 73)), c=None)])

    # chrC appears only in the control header (save = false, Genrich.c:4244); chr2 has
    # treatment reads but no control reads
    NC = ["chr1", "chr2", "chrC"]
    LC = [30_000, 20_000, 10_000]
    ctrl = mf(LC, 2500, 82, uniform_only=True)
    ctrl = ctrl[ctrl["chrom"] != 1]
    yield dict(
        name="ctrl_only_chrom", names=NC, args=["-a", "40", "-L", "45000"],
        reps=[dict(t=(NC[:2], LC[:2], mf(LC[:2], 2500, 81)),
                   c=(NC, LC, ctrl))])

    # unpaired alignments: -y (as is), -w (fixed extension), -x (average fragment length), with a MAPQ
    # filter and assorted records the reader must skip; the same stream also as BAM input
    for nm, extra in (("unpaired_y", ["-y"]), ("unpaired_w", ["-w", "150", "-m", "10"]), ("unpaired_x", ["-x"]),
                      ("unpaired_bam_atac", ["-y", "-j", "-D", "-d", "80"])):
        yield dict(
            name=nm, names=N2, args=extra + ["-a", "20"], mixed=dict(seed=7, bam=nm.endswith("bam_atac")),
            reps=[dict(t=(N2, L2, mf(L2, 2500, 95)), c=(N2, L2, mf(L2, 2000, 96, uniform_only=True)))])

    # -r / -R: PCR-duplicate removal -- pairs only; with unpaired alignments kept (-y); BAM input with -x
    for nm, extra, isbam in (("dups_pairs", ["-r"], False), ("dups_y", ["-r", "-y", "-s", "1.5"], False),
                             ("dups_x_bam", ["-r", "-x"], True)):
        yield dict(
            name=nm, names=N2, args=extra + ["-a", "20"], mixed=dict(seed=21, bam=isbam, writer="dups"),
            reps=[dict(t=(N2, L2, mf(L2, 2500, 97)), c=(N2, L2, mf(L2, 2000, 98, uniform_only=True)))])

    # -r on contested sets (tests/dups_cases.py): secondary alignments of the primary's AS on proper pairs, singletons and
    # discordant pairs, on shared coordinates -- with unpaired alignments kept (-y), BAM input with -x, pairs only
    for nm, extra, isbam in (("dups_contested_y", ["-r", "-y"], False), ("dups_contested_x_bam", ["-r", "-x"], True),
                             ("dups_contested_pairs", ["-r"], False)):
        yield dict(
            name=nm, names=N2, args=extra + ["-a", "20"], mixed=dict(seed=41, bam=isbam, writer="contested"),
            reps=[dict(t=(N2, L2, mf(L2, 1200, 151)), c=(N2, L2, mf(L2, 900, 152, uniform_only=True)))])

    # valid but unusual records: SAM lines without optional fields (QUAL keeps its line feed), records
    # without SEQ (the BAM reader takes l_seq = 0 at face value), soft clips -- with -r, where qualities count
    # (the BAM case keeps to proper pairs: on an unpaired reverse read without SEQ the reference's own
    # arithmetic ends in "Invalid pileup value (< 0)")
    for nm, extra, isbam in (("quirks_sam", ["-r", "-y"], False), ("quirks_bam", ["-r"], True)):
        yield dict(
            name=nm, names=N2, args=extra + ["-a", "20"], mixed=dict(seed=33, bam=isbam, writer="dups", quirks=0.3),
            reps=[dict(t=(N2, L2, mf(L2, 2000, 101)), c=(N2, L2, mf(L2, 1500, 102, uniform_only=True)))])

    # saveInterval's int16 limits (Genrich.c:2558-2573): > 32,767 alignments that start on one base ("skipped due to
    # overflow"), > 32,768 that end on one ("underflow"), in shuffled order among ordinary reads; 30 % of them unpaired
    # and extended to the average fragment length at the end of the file (-x: the dropped pairs count as length 0).
    # The control piles 20,000 reads on the same bases: nothing of the treatment's state may be left.
    yield dict(
        name="saturate16", names=["chrA"], args=["-x", "-a", "20"], mixed=dict(seed=5, bam=False), int16=True,
        reps=[dict(t=(["chrA"], L1, int16_towers(L1, 47_600, 47_400, 61)),
                   c=(["chrA"], L1, int16_towers(L1, 20_000, 20_000, 62)))])

    # -X: no peak calling, just the -f log (logIntervals, Genrich.c:837)
    yield dict(
        name="nopeaks_log", names=N2, args=["-X", "-q", "0.05"],
        reps=[dict(t=(N2, L2, mf(L2, 1500, 91)), c=None),
              dict(t=(N2, L2, mf(L2, 1500, 92)), c=None)])

    # threshold ties (tests/ties.py): -p / -q at a value present in the run, -a at a peak's exact AUC, -l at a peak's exact
    # length, -g at the exact distance between two significant runs -- found here, with the oracle, and checked to be live on
    # the reference alone (tie_args)
    yield from tie_cases()


# -P re-calls on the -f log of a case (callPeaksLog, Genrich.c:1277-1488): new thresholds, new -e / -E
P_RUNS = {
    "ctrl_q": [dict(args=["-q", "0.4", "-a", "15"]), dict(args=["-p", "0.001", "-a", "10", "-g", "20", "-l", "50"])],
    "reps3": [dict(args=["-p", "0.01", "-a", "50"]), dict(args=["-q", "0.3", "-a", "5", "-e", "chr2"])],
    "bedx": [dict(args=["-q", "0.25", "-a", "30"], bed=[("chr1", 3000, 3400), ("chr1", 12000, 12345), ("chr2", 0, 777)])],
    "basic": [dict(args=["-a", "100", "-L", "1000"], bed=[("chrA", 12500, 12520)])],
    # ties_p / ties_q: -P re-calls at ties of the -f log's printed values (p_run_ties), added when the case is generated
    # (reps5_mixed / reps9 have none: test_cli_peaks_from_log's ids carry a running index over all cases' re-calls in name
    # order, and a re-call that sorts before ties_p would rename those that follow)
}
P_TIES = {"ties_p": ["-p"], "ties_q": ["-p", "-q"]}



# ---- threshold ties ----------------------------------------------------------------------------------------------------

def _ties():
    import ties
    return ties


def _ref_coords(args):
    """the reference's narrowPeak coordinates and summits (columns 1-3, 10) for one command line"""
    out = args[args.index("-o") + 1]
    res = subprocess.run([REF] + args, capture_output=True, text=True)
    if res.returncode != 0:
        sys.exit("reference failed:\n" + res.stderr)
    return [(l.split("\t")[0], l.split("\t")[1], l.split("\t")[2], l.split("\t")[9]) for l in open(out).read().splitlines()]


def _set(args, flag, value):
    a = list(args)
    a[a.index(flag) + 1] = value
    return a


def check_live_on_reference(args, flips, out):
    """each flip (flag, value one float / one base past the tie) must change the reference's peaks"""
    full = args + ["-o", out]
    base = _ref_coords(full)
    assert base, "the tie case has no peaks"
    for flag, v in flips:
        if _ref_coords(_set(full, flag, v)) == base:
            sys.exit(f"tie {flag} {args[args.index(flag) + 1]} is not live on the reference ({flag} {v} gives the same peaks)")


def design_ties(case, qval, lo_t=0.5):
    """(-p/-q string, min_auc, min_len, max_gap) for one case, every one a live tie on the oracle with the others fixed"""
    T = _ties()
    import backends as Bk
    base = Bk.make_params(pq=0.05 if qval else 0.01, qval=qval, min_auc=0.0, min_len=0, max_gap=100)
    r0 = T.run_oracle(case, base)
    col = "q" if qval else "p"
    bp = {}
    for c in range(len(case["lens"])):
        m, ln = T._in_peaks(r0, c)
        for v, l in zip(r0.cols[c][col][m], ln[m]):
            if v >= lo_t:
                bp[float(v)] = bp.get(float(v), 0) + int(l)
    for t in sorted(bp, key=lambda v: -bp[v])[:40]:
        s, s_dn = T.pq_string(t), T.pq_string(T.down(t))
        if s is None or s_dn is None:
            continue
        try:
            g = T.gap_tie(case, T.params(base, thr=t), lo=2, hi=1_000, raise_thr=False)
        except AssertionError:
            continue
        if g.base.thr != np.float32(t):
            continue
        gap = int(g.at)
        P = T.params(base, thr=t, max_gap=gap)
        r = T.run_oracle(case, P)
        if len(r.peaks) < 3:
            continue
        auc = np.sort(r.peaks["auc"])
        a = float(auc[len(auc) // 2])
        keep = r.peaks[r.peaks["auc"] >= np.float32(a)]
        L = int((keep["end"].astype(np.int64) - keep["start"]).min())
        P = T.params(P, min_auc=a, min_len=L)
        k0 = T.run_oracle(case, P).key()
        flips = dict(thr=T.down(t), min_auc=T.up(a), min_len=L + 1, max_gap=gap - 1)
        if all(T.run_oracle(case, T.params(P, **{f: v})).key() != k0 for f, v in flips.items()):
            return dict(pq=s, pq_away=s_dn, auc=a, len=L, gap=gap, t=t)
    sys.exit("no set of live ties found")


def tie_args(ev_t, ev_c, lens, qval):
    d = design_ties(dict(lens=lens, replicates=[dict(save=None, treat=ev_t, ctrl=ev_c)]), qval)
    args = ["-q" if qval else "-p", d["pq"], "-a", "%.9g" % d["auc"], "-l", str(d["len"]), "-g", str(d["gap"])]
    assert float(np.float32(float(args[3]))) == d["auc"]
    flips = [(args[0], d["pq_away"]), ("-a", "%.9g" % _ties().up(d["auc"])), ("-l", str(d["len"] + 1)), ("-g", str(d["gap"] - 1))]
    return args, flips


def tie_cases():
    T = _ties()
    N1, L1 = ["chrA"], [60_000]
    ev = mf(L1, 3000, 111)
    args, flips = tie_args(ev, None, L1, False)
    yield dict(name="ties_p", names=N1, args=args, flips=flips, reps=[dict(t=(N1, L1, ev), c=None)])
    L2, N2 = [32_000, 20_000], ["chr1", "chr2"]
    ev, ct = mf(L2, 4000, 121), mf(L2, 2000, 122, uniform_only=True)
    args, flips = tie_args(ev, ct, L2, True)
    yield dict(name="ties_q", names=N2, args=args, flips=flips, reps=[dict(t=(N2, L2, ev), c=(N2, L2, ct))])
    # summits (updatePeak 958-966): plateaus of one height, equal length / the later one longer; in -q mode two plateaus of
    # different p and equal q -- summitPos moves to the later, longer one, the p reported stays the first one's
    qp = T.summit_q_pair()
    ev = T.summit_events(q_pair=qp)
    yield dict(name="ties_summit", names=N1, args=["-a", "20"], reps=[dict(t=(N1, L1, ev), c=None)])
    yield dict(name="ties_summit_q", names=N1, args=["-q", "0.05", "-a", "20"], reps=[dict(t=(N1, L1, ev), c=None)])


def _log_rows(path):
    rows = []
    with open(path) as f:
        hdr = f.readline().rstrip("\n").split("\t")
        qcol = hdr.index("-log(q)") if "-log(q)" in hdr else None
        pcol = hdr.index("-log(p)")
        for line in f:
            x = line.rstrip("\n").split("\t")
            rows.append((x[0], int(x[1]), int(x[2]), x[pcol], x[qcol] if qcol is not None else None))
    return rows


def log_peaks(rows, col, thr, min_auc, min_len, max_gap):
    """callPeaksLog (Genrich.c:1277-1488) without -E / -e on parsed -f rows: (chrom, start, end, float AUC) of the peaks"""
    f = np.float32
    thr = f(thr)
    out = []
    state = dict(chrom=None, ps=-1, pe=-1, auc=f(0))

    def check():
        if state["ps"] != -1 and state["auc"] >= f(min_auc) and state["pe"] - state["ps"] >= min_len:
            out.append((state["chrom"], state["ps"], state["pe"], float(state["auc"])))
        state.update(ps=-1, pe=-1, auc=f(0))

    for chrom, s, e, ps, qs in rows:
        if chrom != state["chrom"]:
            check()
            state["chrom"] = chrom
        st = ps if col == "p" else qs
        if st == "NA":
            check()
            continue
        v = f(float(np.float32(float(st))))
        if v > thr:
            state["auc"] = f(state["auc"] + f(e - s) * f(v - thr))
            if state["ps"] == -1:
                state["ps"] = s
            state["pe"] = e
        elif e - state["pe"] > max_gap:
            check()
    check()
    return out


def p_run_ties(log_path, col, lo_t=0.5):
    """-P args at ties of the log's printed values: -p/-q at a printed value, -a at a peak's float AUC, -l at a peak's length,
    -g at a gap between significant runs; with their flips (checked on the reference by the caller)"""
    T = _ties()
    rows = _log_rows(log_path)
    vals = {}
    for chrom, s, e, ps, qs in rows:
        st = ps if col == "p" else qs
        if st not in ("NA", None) and float(st) >= lo_t:
            vals[st] = vals.get(st, 0) + e - s
    for st in sorted(vals, key=lambda v: -vals[v])[:60]:
        t = T.strtof(st)
        s, s_dn = T.pq_string(t), T.pq_string(T.down(t))
        if s is None or s_dn is None:
            continue
        # gaps between significant runs at thr = t
        gaps = []
        prev = None
        for chrom, a, e, ps, qs in rows:
            v = ps if col == "p" else qs
            sig = v != "NA" and np.float32(float(v)) > np.float32(t)
            if v == "NA":
                prev = None
            elif sig:
                if prev is not None and prev[0] == chrom and a - prev[1] > 1:
                    gaps.append(a - prev[1])
                prev = (chrom, e)
        for gap in sorted(set(g for g in gaps if g <= 1_000), reverse=True)[:8]:
            pk = log_peaks(rows, col, t, 0.0, 0, gap)
            if len(pk) < 3:
                continue
            L = sorted(e - a for _, a, e, _ in pk)[len(pk) // 2]
            keep = [x for x in pk if x[2] - x[1] >= L]
            coords = lambda *arg: [x[:3] for x in log_peaks(rows, col, *arg)]
            for a in sorted(x[3] for x in keep):   # (AUC: the float sum in interval order, as the reference adds it)
                pk = coords(t, a, L, gap)
                if pk not in (coords(T.down(t), a, L, gap), coords(t, T.up(a), L, gap), coords(t, a, L + 1, gap),
                              coords(t, a, L, gap - 1)):
                    return (["-" + col, s, "-a", "%.9g" % a, "-l", str(L), "-g", str(gap)],
                            [("-" + col, s_dn), ("-a", "%.9g" % T.up(a)), ("-l", str(L + 1)), ("-g", str(gap - 1))])
    sys.exit("no live -P ties")

def write_input(path, names, lens, ev, mixed, seed_off, prefix):
    """The synthetic SAM / BAM input of one sample, by the writer the case asks for."""
    if mixed and mixed.get("writer") == "dups":
        synth.write_sam_dups(path, names, lens, ev, mixed["seed"] + seed_off, name_prefix=prefix, bam=mixed["bam"],
                             quirks=mixed.get("quirks", 0.0))
    elif mixed and mixed.get("writer") == "contested":
        import dups_cases
        dups_cases.write_sam_contested(path, names, lens, ev, mixed["seed"] + seed_off, name_prefix=prefix, bam=mixed["bam"])
    elif mixed:
        synth.write_sam_mixed(path, names, lens, ev, mixed["seed"] + seed_off, name_prefix=prefix, bam=mixed["bam"])
    else:
        synth.write_sam(path, names, lens, ev, name_prefix=prefix)


def gz_copy(src, dst):
    with open(src, "rb") as f, gzip.GzipFile(dst, "wb", mtime=0) as g:
        shutil.copyfileobj(f, g)


def main():
    if not os.path.exists(REF):
        sys.exit("oracle/_ref/Genrich missing: run `make -C oracle` in the build container")
    for extra in int16_extra():
        if not sys.argv[1:] or extra in sys.argv[1:]:
            make_int16_extra(extra)
    for case in cases():
        if sys.argv[1:] and case["name"] not in sys.argv[1:]:
            continue  # (python make_golden.py <case> ...: only those)
        out_dir = os.path.join(HERE, case["name"])
        os.makedirs(out_dir, exist_ok=True)
        tmp = os.path.join("/tmp/genrich_golden", case["name"])
        shutil.rmtree(tmp, ignore_errors=True)
        os.makedirs(tmp)
        tfiles, cfiles = [], []
        chrom_order, chrom_len = [], {}
        saves = []

        def seen(names, lens):
            for n, l in zip(names, lens):
                if n not in chrom_len:
                    chrom_order.append(n)
                    chrom_len[n] = l

        for r, rep in enumerate(case["reps"]):
            names, lens, ev = rep["t"]
            mixed = case.get("mixed")
            ext = "bam" if mixed and mixed["bam"] else "sam"
            p = os.path.join(tmp, f"t{r}.{ext}")
            write_input(p, names, lens, ev, mixed, 0, f"t{r}_")
            tfiles.append(p)
            seen(names, lens)
            saves.append(list(names))
            if rep["c"] is None:
                cfiles.append(None)
            elif rep["c"] == "null":
                cfiles.append("null")
            else:
                names, lens, ev = rep["c"]
                p = os.path.join(tmp, f"c{r}.{ext}")
                write_input(p, names, lens, ev, mixed, 1, f"c{r}_")
                cfiles.append(p)
                seen(names, lens)
        args = [REF, "-t", ",".join(tfiles), "-v",
                "-f", os.path.join(tmp, "out.log"), "-k", os.path.join(tmp, "out.pile"),
                "-b", os.path.join(tmp, "events.bed")]
        if "-X" not in case["args"]:
            args += ["-o", os.path.join(tmp, "out.narrowPeak")]
        if any(c is not None for c in cfiles):
            args += ["-c", ",".join(c if c else "null" for c in cfiles)]
        if case.get("bed"):
            bp = os.path.join(tmp, "x.bed")
            with open(bp, "w") as f:
                for c, s, e in case["bed"]:
                    f.write(f"{c}\t{s}\t{e}\n")
            args += ["-E", bp]
        args += case["args"]
        if "-r" in case["args"]:
            args += ["-R", os.path.join(tmp, "out.dups")]
        res = subprocess.run(args, capture_output=True, text=True)
        if res.returncode != 0:
            sys.exit(f"{case['name']}: reference failed:\n{res.stderr}")
        err = res.stderr
        if case.get("flips"):   # every tie live on the reference alone: one float / one base away, other peaks
            ctl = ["-c", ",".join(c if c else "null" for c in cfiles)] if any(cfiles) else []
            check_live_on_reference(["-t", ",".join(tfiles)] + ctl + case["args"], case["flips"], os.path.join(tmp, "live.narrowPeak"))
        skip = []
        if "-e" in case["args"]:
            skip = case["args"][case["args"].index("-e") + 1].split(",")
        beds = {}
        for n in chrom_order:
            regs = [(s, e) for c, s, e in case.get("bed", []) if c == n]
            beds[n] = merged_bed(regs, chrom_len[n]) if n not in skip else []
        meta = dict(
            name=case["name"], args=case["args"],
            chroms=[dict(name=n, len=chrom_len[n], skip=n in skip, bed=beds[n]) for n in chrom_order],
            replicates=[dict(save=[n in s for n in chrom_order],
                             control=(None if c is None else ("null" if c == "null" else "file")),
                             expt_name=os.path.basename(t),
                             ctrl_name=(None if c is None else os.path.basename(c)))
                        for s, c, t in zip(saves, cfiles, tfiles)],
            ref_lambda=[float(v) for v in re.findall(r"Background pileup value: ([0-9.]+)", err)],
            ref_factor=[float(v) for v in re.findall(r"Scaling factor for control pileup: ([0-9.]+)", err)],
            ref_genome_len=[int(v) for v in re.findall(r"Genome length: (\d+)bp", err)],
            ref_peaks=[[int(a), int(b)] for a, b in re.findall(r"Peaks identified: (\d+) \((\d+)bp\)", err)],
            tmp_prefix=tmp + "/",
            ref_dups=[l.strip() for l in err.splitlines() if "aln sets:" in l or "duplicates:" in l],
        )
        with open(os.path.join(out_dir, "case.json"), "w") as f:
            json.dump(meta, f, indent=1)
        if case.get("int16"):  # the reference's read-by-read warnings, in order
            with gzip.GzipFile(os.path.join(out_dir, "out.int16.gz"), "wb", mtime=0) as g:
                g.write("".join(l + "\n" for l in err.splitlines() if "skipped due to" in l).encode())
        for fn in ("events.bed", "out.narrowPeak", "out.log", "out.pile", "out.dups"):
            src = os.path.join(tmp, fn)
            if os.path.exists(src):
                gz_copy(src, os.path.join(out_dir, fn + ".gz"))
        p_runs = list(P_RUNS.get(case["name"], []))
        for col in P_TIES.get(case["name"], []):   # -P at ties of the printed values, live on the reference
            pa, pflips = p_run_ties(os.path.join(tmp, "out.log"), col[1])
            check_live_on_reference(["-P", "-f", os.path.join(tmp, "out.log")] + pa, pflips, os.path.join(tmp, "live.P.narrowPeak"))
            p_runs.append(dict(args=pa))
        p_meta = []
        for k, pr in enumerate(p_runs):
            pargs = [REF, "-P", "-f", os.path.join(tmp, "out.log"), "-o", os.path.join(tmp, f"out.P{k}.narrowPeak")] + pr["args"]
            if pr.get("bed"):
                bp = os.path.join(tmp, f"xP{k}.bed")
                with open(bp, "w") as f:
                    for c, s_, e in pr["bed"]:
                        f.write(f"{c}\t{s_}\t{e}\n")
                pargs += ["-E", bp]
            r2 = subprocess.run(pargs, capture_output=True, text=True)
            if r2.returncode != 0:
                sys.exit(f"{case['name']}: reference -P failed:\n{r2.stderr}")
            gz_copy(os.path.join(tmp, f"out.P{k}.narrowPeak"), os.path.join(out_dir, f"out.P{k}.narrowPeak.gz"))
            p_meta.append(dict(args=pr["args"], bed=pr.get("bed", [])))
        meta["p_runs"] = p_meta
        with open(os.path.join(out_dir, "case.json"), "w") as f:
            json.dump(meta, f, indent=1)
        n_np = sum(1 for _ in open(os.path.join(tmp, "out.narrowPeak"))) if "-X" not in case["args"] else 0
        print(f"{case['name']:18s} peaks={n_np:4d} lambda={meta['ref_lambda']} factor={meta['ref_factor']}")
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
