"""The peak sweep -- callPeaks on bit masks, genrich_amd/csrc/gx_stats.h, launched by run_sweep (gx_host_sweep.h:31) -- at its word,
chunk, row and walk limits, on constructed inputs.

Every case is a pileup profile written by hand (tests/sweep_limits.py): its intervals' indices in the space the sweep walks -- the
concatenated table ("tight") or the tile stage's loose slots with their fillers ("loose") -- are computed from the oracle's table
by sweep_census(), which checks itself against the oracle's peaks, and the case ASSERTS the structural fact it exists for (the bit,
the word, the chunk, the run or candidate number, the length in index units) on a machine without a GPU
(tests/test_sweep_limits_oracle.py).  Here the library runs every case in the space it was built for, on the paths whose kernels see
its limit; the peaks are compared as bytes, intervals / p / q / fragLen / lambda through assert_same_run, the path bits are asserted.

The limits, and where they are written (gx_stats.h):
  run_bits :1244-1251, run_bits_brk :1254-1260   prevBit (:1246), nextBit (:1247), nextBrk (:1248) cross a 64-bit word
  runs_body :1695   SW_ITEMS = 8 words a thread (:1190), SW_CHUNK = 2048 words a chunk (:1191); ONE scan for starts and ends, the
                    ends' offset corrected by `ob -= sig0 & ~stb[0] & 1` (:1766) for a run open across a thread's first word;
                    <TABLE>: SW_CHUNK + 1 words of chromosome starts in LDS (:1703, :1720), cached up to RUN_NCH = 1024
                    chromosomes (:1680, :1706); the counts are the last chunk's (:1752-1757)
  k_cands :1835     RC_CHUNK = 256 runs a chunk (:1194); run_is_head (:1279-1293) reads runEnd[r - 1] (:1283), links at
                    `gap != 0 && gap > maxGap` (:1289) and looks for a SKIP bit between (:1291); *nCands from the last chunk (:1854)
  k_cand_hdr :1307  rLast = candRun[c + 1] - 1 or R - 1 (:1314); end[i0 - 1] unless atChromStart (:1316-1317); i1 - i0 >= PK_SHORT
                    = 1024 goes to the long list (:1318)
  peak_short_body :1424   16 intervals a step (:1452), AH = 4 steps a batch (:1430, :1446), four candidates a wavefront with the
                    wavefront's step count (:1441-1443), the AUC replayed through RowSeqSum<15> (:1475), rowSg / better / longer per
                    row under a wave-uniform ballot (:1482-1484)
  peak_walk_body :1515    64 intervals a step, 256 a batch (:1534); the AUC carried row to row through rdf(acc, 0 / 16 / 32 / 48)
                    (:1562-1566), the summit taken across rows (:1569-1575)
  k_q_fill_cands :562     one wavefront a candidate, 64 probes a step, 256 intervals a turn (:568)
  k_peaks :1864     256 candidates a chunk staged in LDS (:1871), nPeaks from the last chunk (:1895-1898), bp summed (:1889, :1918)
  lookback_gen :1630      a window of 64 predecessors (:1640), granules of another generation read as nothing (:1642)

What the suite reached before this module -- sweep_census over the inputs of the existing GPU tests, in the space each run takes
(R runs, C candidates; "x word / thread / chunk": runs open across such a border; lengths in index units):

  existing GPU test (its input)                         | space |       N |   R |   C | x word / thread / chunk | longest | at or next to a limit
  test_hip_parity random runs, 50 seeds (all together)  | 47 t, |  42,844 |  15 |  15 | 273 / 151 / 0           |     520 | lengths 1 (3 runs), 15, 64 (1 each); a run
                                                        | 3 l   | at most | at most   |                         |         | ending on bit 63: 2; N = 0 or 1 mod 64 with
                                                        |       |         |     |     |                         |         | a significant last interval: 2; SKIP on bit 63 / 0: 1
  test_hip_paths _case(seed 11, 90,000 fragments)       | loose | 179,587 |  37 |  33 | 36 / 24 / 0             |   1,859 | 4 links at gap 0 (max_gap 100)
  test_hip_paths _case(seed 5, 150,000 fragments)       | loose | 299,224 |  38 |  34 | 36 / 31 / 0             |   3,226 | length 256 (one candidate)
  test_hip_ties noctrl, -p and -q                       | loose | 159,681 |  31 |  29 | 31 / 23 / 0             |   1,803 | N = 1 mod 64, the last slot a filler
                                                        | tight | 102,074 |  29 |  29 | 29 / 22 / 0             |     451 |
  test_hip_ties ctrl                                    | tight | 123,047 |  22 |  21 | 21 / 14 / 0             |     468 | a chromosome starts on bit 0, quiet
  test_hip_ties long                                    | loose |  58,034 |  23 |  11 | 19 / 9 / 0              |  49,806 | 8 links at gap 0
  test_hip_ties bed                                     | tight |  95,380 |  29 |  29 | 29 / 25 / 0             |     445 | one SKIP interval on bit 63 or 0, not between two runs
  test_hip_sweep_overlap _full_tile                     | loose |     476 |   4 |   4 | 0 / 0 / 0               |      21 | a chromosome start with both neighbours
                                                        |       |         |     |     |                         |         | significant (asserted there; not on bit 0)
  test_hip_sweep_overlap _border (skipped chromosome)   | tight |     354 |   2 |   2 | 1 / 0 / 0               |      59 |
  test_hip_sweep_overlap _plain                         | loose |  59,740 |  23 |  21 | 23 / 18 / 0             |     894 |
  test_hip_sweep_overlap _two_chunks                    | loose | 142,008 | 179 | 156 | 161 / 62 / 1            |     316 | ONE run open across word 2047 | 2048, length 257
  test_hip_tile_limits case_sig (r0, r1, r63)           | loose |   3,813 |   7 |   4 | 4 / 1 / 0               |   1,015 | length 65; the plateau of > 128 slots it asserts
  (test_hip_fullsize: the same generator at 50 M fragments; not counted)

So runs across a word and a thread border, long candidates and links at gap 0 HAD run in every ordinary input, by density; one run of
_two_chunks happens to lie across the chunk border, and nobody said so.  Never reached: more than 256 runs -- k_cands, k_peaks and
their look-backs had only ever seen ONE chunk, so runEnd[r - 1] of another chunk, *nCands / nPeaks from a later chunk, a chunk of
k_peaks without a peak and a look-back past its 64-lane window did not exist; a chromosome start on bit 0 with both neighbours
significant; a run of length 1 at index 0; more than RUN_NCH chromosomes; a link that NEEDS `gap != 0` (every gap-0 link ran at
max_gap = 100); a SKIP on bit 63 / bit 0 between two runs within max_gap; the lengths 16, 17, 63, 255, 1023 - 1025, 1279 - 1281; a
summit decided by the `longer` branch across steps or rows by construction; an AUC whose order is shown to matter; k_q_fill_cands on
a candidate of more than 64 intervals whose q-values differ (with a rare highest pileup Benjamini-Hochberg gives every significant
level ONE q -- the first version of these cases had that, see below).  Nothing of the list was already pinned by a test that asserts
it but the significant chromosome start of _full_tile, which stays where it is; the cases here put it on bit 0 of a word and of a chunk.

That the cases see what they claim was checked once with scratch builds of the library, one line of gx_stats.h broken each -- only a
value that a kernel writes into its own output element (run_is_head's and nextBrk's verdicts move counts, consistently: starts and
ends stay paired) --, this module (87 GPU tests) run once on each:

  the break                                                       | tests that failed
  peak_short_body: RowSeqSum<15> -> <14> (:1475: a row's last     | 28: summits, walk-g16 / g256 / g1024 / wave on every path they run on (p, q
    product dropped)                                              | eager, q lazy, q on the loose slots), plateau-tile-border and -negative-gap,
                                                                  | the four AUC ties; walk-g1280 (long candidates only) passes
  peak_walk_body: rdf(acc, 16) -> rdf(acc, 0) (:1564: the third   | 17: summits, walk-g1024 / g1280 / wave on every path, the four AUC ties (the
    row starts from the first row's sum)                          | short candidate's too: its tie's runs hold the long candidate); g16 / g256 pass
  peak_short_body: `longer` never (:1483)                         | 14: summits (p, q eager, q loose), walk-g16 / g256 / g1024 / wave with -p (equal
                                                                  | pileups recur in every candidate), the short candidate's AUC ties (summit bytes)
  peak_walk_body: `mx == summitVal && ml > summitLen` never (:1576) | 4: summits on its four paths (candidates 6 and 7)
  run_is_head: `gap != 0 &&` dropped (:1289)                      | 1: plateau-negative-gap.  At max_gap >= 0 the term is redundant (0 > maxGap is
                                                                  | false): plateau-tile-border at max_gap = 0 passes, as it must
  run_bits: nextBrk = 0 (:1248; tight only)                       | 3: tight:chrom-start-word, tight:chrom-start-chunk on both grids (the runs merge
                                                                  | across the chromosome start); every loose case passes (run_bits_brk)
  k_peaks: `bp +=` dropped (:1889)                                | 85: every test with a peak (the two zero-peaks cases pass)
  k_q_fill_cands: the fourth step's q from the third's probe      | 2: tight:walk-g256 and tight:walk-wave on tight-q-lazy (candidates of more than 192
    (:589: `ge[k == 3 ? 2 : k]`)                                  | intervals).  NOT NOTICED by the first version of the cases: all their significant
                                                                  | intervals had one q; the cases that run with -q now carry a wide plateau of a high
                                                                  | pileup on another chromosome, which gives every level a q of its own (check()
                                                                  | asserts it).  Run again with the plateau at pileup 400: these 2 fail; the pileup
                                                                  | was then halved for the oracle's time, the q-values stay distinct
Not built, argued from the code: the `ob -=` correction (:1766) without which a thread whose first word opens inside a run writes
its ends one place too far -- an index, so no scratch build --: run-across-thread, run-across-chunk, run-across-word's neighbours
with bit 0 of a thread's first word significant would differ in every later runEnd; s_brk's `+ 1` word (:1703) -- chrom-start-chunk
on the loose slots reads exactly that word's bit 0 from the chunk before."""
import numpy as np
import pytest

import backends as B
import sweep_limits as S
import ties as T
from test_hip_parity import assert_same_run, hip_backend

pytestmark = pytest.mark.gpu

FUSED, LOOSE, FELL_BACK, PAIRS = 1, 2, 4, 16                   # gx_path_info bits (tests/test_hip_ties.py)
MERGE_P, LAZY_Q, Q_LOOSE, OVERLAP = 1024, 8192, 32768, 536870912

# path -> (switches, -q, bits that must be set, bits that must not)
PATHS = {
    "loose-p": ({}, False, FUSED | LOOSE | OVERLAP, FELL_BACK),                                   # runs_body<true> in k_scan_iv_close_runs
    "loose-p-no-overlap": ({"GX_NO_SWEEP_OVERLAP": 1}, False, FUSED | LOOSE, FELL_BACK | OVERLAP),  # the sweep's own k_runs<true>
    "loose-p-grid1": ({"GX_SWEEP_GRID": 1}, False, FUSED | LOOSE | OVERLAP, FELL_BACK),           # one persistent workgroup per look-back
    "loose-p-grid2": ({"GX_SWEEP_GRID": 2}, False, FUSED | LOOSE | OVERLAP, FELL_BACK),
    "loose-q": ({}, True, FUSED | LOOSE | Q_LOOSE, FELL_BACK | OVERLAP),                          # k_peak_both<false, true, true>
    "tight-p": ({"GX_NO_LOOSE": 1}, False, FUSED, LOOSE | OVERLAP),                               # k_sig_mask, k_runs<false>, k_peak_both<false, false>
    "tight-p-grid1": ({"GX_NO_LOOSE": 1, "GX_SWEEP_GRID": 1}, False, FUSED, LOOSE | OVERLAP),
    "tight-q-eager": ({"GX_NO_Q_LOOSE": 1, "GX_NO_LAZY_Q": 1}, True, FUSED, LOOSE | Q_LOOSE | LAZY_Q),   # k_peak_both<true, false>, q from memory
    "tight-q-lazy": ({"GX_NO_Q_LOOSE": 1}, True, FUSED | LAZY_Q, Q_LOOSE),                        # k_q_fill_cands writes the candidates' q
    "bed": ({}, False, FUSED, LOOSE | OVERLAP),                                                   # -E: SKIP intervals, the skip mask
    "ctrl": ({}, False, FUSED | MERGE_P, LOOSE | OVERLAP),                                        # k_runs<false> on the merged table
}
RUNS = [(n, p) for n in sorted(S.CASES) for p in S.CASES[n][2]]


def _library(monkeypatch, path, par, case):
    env, qval, on, off = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    h = hip_backend(par)
    sh = B.run_case(h, case)
    flags = h.path_info()
    assert flags & on == on and not flags & off, (path, flags, on, off)
    return h, sh


def _same(o, so, h, sh, case):
    assert h.get_peaks().tobytes() == o.get_peaks().tobytes()
    assert (h.n_peaks, h.peak_bp) == (o.n_peaks, o.peak_bp)
    assert_same_run(o, h, so, sh, case)


@pytest.mark.parametrize("name,path", RUNS)
def test_sweep_at_its_limits(monkeypatch, name, path):
    qval = PATHS[path][1]
    S.check(name, qval)                                   # the input is what the case claims (cached: the oracle ran once)
    a, par, o, so, cen = S.reference(name, qval)
    h, sh = _library(monkeypatch, path, par, a["case"])
    _same(o, so, h, sh, a["case"])
    assert (o.n_peaks == 0) == name.endswith("zero-peaks") and len(cen.runs) > 0
    h.close()


@pytest.mark.parametrize("name,k", S.AUC_CASES)
def test_auc_in_interval_order_at_its_own_tie(monkeypatch, name, k):
    """min_auc = the candidate's float32 AUC summed in interval order (kept), one float below (kept) and one above (dropped): the
    terms summed in any other order give another float (test_sweep_limits_oracle.py), which one of the three runs would show"""
    a, par, o, so, cen = S.reference(name)
    seq = S.seq_sum(cen.terms[k])
    assert seq.tobytes() == o.get_peaks()["auc"][k].tobytes()
    for v in (T.down(seq), float(seq), T.up(seq)):
        a, par2, o2, so2, _ = S.reference(name, min_auc=v)
        auc = o.get_peaks()["auc"]
        assert o2.n_peaks == int((auc >= np.float32(v)).sum()) and (seq in o2.get_peaks()["auc"]) == (v <= float(seq))
        h, sh = _library(monkeypatch, "tight-p" if name.startswith("tight") else "loose-p", par2, a["case"])
        _same(o2, so2, h, sh, a["case"])
        h.close()


@pytest.mark.parametrize("space", ["loose", "tight"])
def test_generation_tags_across_calls_on_one_context(monkeypatch, space):
    """One context: 66 chunks of runs, candidates and peaks (A), the sweep again, a reset, two chunks (B) and the sweep twice more,
    a reset, A again: the look-back granules of an earlier call -- more of them, with other counts -- must read as `nothing yet`"""
    A, Bn = f"{space}:many-runs", f"{space}:runs-257"
    a, par, oa, soa, _ = S.reference(A)
    b, parb, ob, sob, _ = S.reference(Bn)
    assert bytes(par) == bytes(parb)
    h, sh = _library(monkeypatch, "loose-p" if space == "loose" else "tight-p", par, a["case"])
    _same(oa, soa, h, sh, a["case"])
    h.find_peaks()
    assert h.get_peaks().tobytes() == oa.get_peaks().tobytes() and h.peak_bp == oa.peak_bp
    h.reset()
    sh = B.run_case(h, b["case"])
    _same(ob, sob, h, sh, b["case"])
    for _ in range(2):
        h.find_peaks()
        assert h.get_peaks().tobytes() == ob.get_peaks().tobytes() and h.peak_bp == ob.peak_bp
    h.reset()
    sh = B.run_case(h, a["case"])
    _same(oa, soa, h, sh, a["case"])
    h.close()
