"""ctypes binding of include/genrich_amd.h (the drop-in boundary of the hot path)."""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple, Optional

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libgenrich_amd.so")

EVENT_DTYPE = np.dtype([("chrom", "<u4"), ("start", "<u4"), ("end", "<u4"), ("count", "<u4")])
PEAK_DTYPE = np.dtype(
    [("chrom", "<u4"), ("start", "<u4"), ("end", "<u4"), ("summit", "<u4"),
     ("auc", "<f4"), ("p", "<f4"), ("q", "<f4")]
)
GX_IV_FINAL = -1
EVENT8_DTYPE = np.dtype([("start", "<u4"), ("lcc", "<u4")])   # gx_event8: lcc = [15:0] end - start, [18:16] count class, [31:19] chromosome
_COUNT_CLASS = np.full(11, 8, dtype=np.uint32)
_COUNT_CLASS[[1, 2, 3, 4, 5, 6, 8, 10]] = np.arange(8, dtype=np.uint32)


def pack_events(ev):
    """gx_event records -> (gx_event8 records of the ones that fit, the others as they are): include/genrich_amd.h, gx_event8_pack
    (the same rule, vectorised)."""
    ev = np.ascontiguousarray(ev)
    ln = ev["end"].astype(np.int64) - ev["start"].astype(np.int64)
    cnt = ev["count"]
    cls = np.where(cnt <= 10, _COUNT_CLASS[np.minimum(cnt, 10)], 8)
    fits = (ln >= 0) & (ln < 0xFFFF) & (cls < 8) & (ev["chrom"] < (1 << 13))
    out = np.empty(int(fits.sum()), dtype=EVENT8_DTYPE)
    sel = ev[fits]
    out["start"] = sel["start"]
    out["lcc"] = ln[fits].astype(np.uint32) | (cls[fits].astype(np.uint32) << 16) | (sel["chrom"].astype(np.uint32) << 19)
    return out, ev[~fits]

GX_PATH_COUNTS = 65536   # gx_path_info bit 16: the run kept its samples' intervals for counting


class PeakCounts(NamedTuple):
    """One sample's counts in the called peaks (gx_get_peak_counts), in 1/120 units: count[k] per peak, the weight of all its
    intervals (total) and of those that overlap a peak (in_peaks); FRiP = in_peaks / total."""
    count: np.ndarray
    total: int
    in_peaks: int
    rep: int
    is_ctrl: bool


GX_PATH_REGION_COUNTS = 131072   # gx_path_info bit 17: gx_count_in_regions has counted since the last reset
REGION_DTYPE = np.dtype([("chrom", "<u4"), ("start", "<u4"), ("end", "<u4")])   # gx_region
SUMMIT_DTYPE = np.dtype([("peak", "<u4"), ("pos", "<u4"), ("width", "<u4"), ("pad", "<u4"), ("height", "<i8"), ("prominence", "<i8")])   # gx_summit


class RegionCounts(NamedTuple):
    """One sample's counts in a given region set (gx_get_region_counts), in 1/120 units: count[k] per region in the caller's
    order, the weight of all its intervals (total) and of those that overlap at least one region (in_regions)."""
    count: np.ndarray
    total: int
    in_regions: int
    rep: int
    is_ctrl: bool


class PeakSignal(NamedTuple):
    """One sample's own depth inside the peaks (gx_get_peak_signal, gx_peak_signal_events), per peak: the area, the maximum
    and the depth at the run's summit base in 1/120 units (int64); the first base (from the peak's start) at which the
    maximum is reached and the bases with a depth above 0 (uint32)."""
    area: np.ndarray
    max: np.ndarray
    summit: np.ndarray
    covered: np.ndarray
    at_summit: np.ndarray
    rep: int
    is_ctrl: bool


GX_PATH_COVERAGE = 262144   # gx_path_info bit 18: the run summed its samples' pileups over bins (gx_set_coverage_bins)


class Coverage(NamedTuple):
    """One sample's binned coverage on one chromosome (gx_get_coverage): sum120[b] = the pileup summed over the bases of bin b,
    in 1/120 units."""
    sum120: np.ndarray
    rep: int
    is_ctrl: bool


GX_PATH_PROFILE = 524288    # gx_path_info bit 19: the run summed its samples' pileups around anchors (gx_set_profile)
ANCHOR_DTYPE = np.dtype([("chrom", "<u4"), ("pos", "<u4"), ("strand", "<i4")])   # gx_anchor


class Profile(NamedTuple):
    """One sample's profile around the anchors (gx_get_profile): agg120[j] = the pileup summed over bin j of every anchor, in
    1/120 units; cell120[a][j] the same per anchor, in the caller's anchor order (None when no matrix was kept or asked for)."""
    agg120: np.ndarray
    cell120: Optional[np.ndarray]
    rep: int
    is_ctrl: bool


GX_PATH_GRAM = 1048576     # gx_path_info bit 20: k_gram / k_gram_sum ran (gx_coverage_gram, gx_gram_u64)
U128_DTYPE = np.dtype([("lo", "<u8"), ("hi", "<u8")])   # gx_u128


def _join128(a):
    """gx_u128 records -> an object array of Python ints of the same shape."""
    out = np.empty(a.shape, dtype=object)
    for k in np.ndindex(a.shape):
        out[k] = int(a[k]["lo"]) | (int(a[k]["hi"]) << 64)
    return out


def _sums128(S):
    """Zeroed gx_u128 (sum [S], gram [S, S]) for the library to fill; one sample's room at least."""
    S = max(S, 1)
    return np.zeros(S, dtype=U128_DTYPE), np.zeros((S, S), dtype=U128_DTYPE)


def _u64_rows(rows):
    """(contiguous uint64 array, its address or None when it is empty): a hook's rows argument."""
    r = np.ascontiguousarray(rows, dtype=np.uint64)
    return r, (r.ctypes.data if r.size else None)


def _split128(values, shape):
    out = np.zeros(shape, dtype=U128_DTYPE)
    flat = out.reshape(-1)
    for k, v in enumerate(np.asarray(values, dtype=object).reshape(-1)):
        v = int(v)
        if not 0 <= v < 1 << 128:
            raise ValueError("not an unsigned 128-bit integer")
        flat[k] = (v & 0xFFFFFFFFFFFFFFFF, v >> 64)
    return out


GX_PATH_FINGERPRINT = 2097152   # gx_path_info bit 21: k_fp_hist ran (gx_coverage_fingerprint, gx_fp_u64)
FP_NC = 3776                    # GX_FP_NC: the fingerprint's value classes
FP_SUB_LOG = 6                  # GX_FP_SUB_LOG
FP_METRICS_DTYPE = np.dtype([(k, "<f8") for k in ("zero_fraction", "auc", "gini", "elbow_bins", "elbow_gap", "jsd_control")])   # gx_fp_metrics


GX_PATH_SPEARMAN = 4194304      # gx_path_info bit 22: k_rank ran (gx_coverage_rank_gram, gx_rank_u64)
GX_PATH_COMPLEXITY = 8388608    # gx_path_info bit 23: k_cpx_insert ran (gx_complexity, gx_complexity_events)
GX_PATH_IVSTAT = 67108864       # gx_path_info bit 26: k_ivstat ran (gx_interval_stats, gx_interval_stats_events)
GX_PATH_XCOR = 134217728        # gx_path_info bit 27: k_xc_set / k_xc_corr ran (gx_set_xcor with a sample closed, gx_push_tags, gx_xcor_tags)
GX_PATH_GC = 1073741824         # gx_path_info bit 30: a kernel of the genome / GC passes ran (gx_push_sequence, gx_gc_content, gx_gc_bias, gx_gc_bias_events)
GX_PATH_MOTIFS = 2147483648     # gx_path_info bit 31: k_motif_scan ran (gx_motif_scan_regions, gx_motif_scan_peaks, gx_motif_scan_genome)
GX_PATH_KMERS = 4096            # gx_path_info bit 12: k_kmer_count ran (gx_kmer_count_regions, gx_kmer_count_peaks, gx_kmer_count_genome)
KMER_MAX_K = 12                 # GX_KMER_MAX_K
KMER_LDS_MAX_K = 7              # GX_KMER_LDS_MAX_K
KMER_ROW_DTYPE = np.dtype([("code", "<u4"), ("revcomp", "<u4"), ("count_peaks", "<u8"), ("count_genome", "<u8"), ("enrichment", "<f8"), ("z", "<f8")])   # gx_kmer_row
MOTIF_MAX_WIDTH = 32            # GX_MOTIF_MAX_WIDTH
MOTIF_MAX = 4096                # GX_MOTIF_MAX
MOTIF_SCALE = 128               # GX_MOTIF_SCALE
MOTIF_DTYPE = np.dtype([("width", "<u4"), ("offset", "<u4"), ("threshold", "<i4")])   # gx_motif
MOTIF_HIT_DTYPE = np.dtype([("region", "<u4"), ("pos", "<u4"), ("score", "<i4"), ("motif", "<u2"), ("strand", "u1"), ("pad", "u1")])   # gx_motif_hit
GC_MAX_WINDOW = 4096            # GX_GC_MAX_WINDOW
GC_MIN_TILE = 64                # GX_GC_MIN_TILE
GC_CLASSES = 101                # GX_GC_CLASSES
GC_METRICS_DTYPE = np.dtype([(k, "<u8") for k in ("windows", "windows_unclassed", "intervals", "intervals_unclassed", "w120", "w120_unclassed")]
                            + [(k, "<u8", (GC_CLASSES,)) for k in ("cls_windows", "cls_intervals", "cls_w120")] + [("ratio", "<f8", (GC_CLASSES,))]
                            + [(k, "<f8") for k in ("mean_gc_genome", "mean_gc_sample", "ratio_min", "ratio_max")]
                            + [("ratio_min_class", "<i4"), ("ratio_max_class", "<i4")])   # gx_gc_metrics_t
TAG_DTYPE = np.dtype([("chrom", "<u4"), ("pos", "<u4"), ("strand", "<u4")])   # gx_tag; strand 1: +, 0: -
XCOR_MAX_SHIFT = 4096           # GX_XCOR_MAX_SHIFT
XCOR_MIN_TILE = 64              # GX_XCOR_MIN_TILE
XCOR_METRICS_DTYPE = np.dtype([(k, "<i4") for k in ("has_frag", "frag_shift", "fragment_length", "min_shift", "has_phantom", "phantom_shift", "_pad")]
                              + [("_pad2", "<i4")] + [(k, "<f8") for k in ("r_frag", "r_min", "r_phantom", "nsc", "rsc")])   # gx_xcor_metrics_t
LEN_MAX_CUTS = 8                # GX_LEN_MAX_CUTS: the most class borders gx_lengths_metrics takes
LEN_METRICS_DTYPE = np.dtype([(f, "<u8") for f in ("n", "w120", "min", "max", "mode", "p5", "q25", "median", "q75", "p95")]
                             + [("mean", "<f8"), ("sd", "<f8"), ("n_shares", "<i4"), ("_pad", "<i4"),
                                ("share", "<f8", (LEN_MAX_CUTS + 1,))])   # gx_len_metrics
CPX_CURVE = 20                  # GX_CPX_CURVE: the points of the complexity curve (5 % steps of the depth)
CPX_METRICS_DTYPE = np.dtype([("h1", "<u8"), ("h2", "<u8")] + [(k, "<f8") for k in ("nrf", "pbc1", "pbc2", "dup_fraction", "library_size")]
                             + [("curve", "<f8", (CPX_CURVE,))])   # gx_cpx_metrics


GX_PATH_SATURATION = 16777216   # gx_path_info bit 24: k_sub_write ran (gx_subsample_events, gx_subsample_kept, gx_saturation)
GX_SAT_CONTROLS = 1             # gx_saturation: the controls are subsampled at the point's threshold too
GX_ERR_EXPT = -3                # a point of gx_saturation whose subsample left no analyzable fragment
SAT_POINT_DTYPE = np.dtype([("threshold", "<u8"), ("n_total", "<u8"), ("n_kept", "<u8"), ("n_peaks", "<u8"), ("peak_bp", "<u8"),
                            ("genome_len", "<u8"), ("status", "<i4"), ("_pad", "<i4")])   # gx_sat_point
GX_PATH_SWEEP_OVERLAP = 536870912   # gx_path_info bit 29: the loose-slot sweep's run pass rode in the launch that closed the sample (k_scan_iv_close_runs): no k_runs launch
GX_PATH_SPLIT = 268435456       # gx_path_info bit 28: k_sub_split ran (gx_subsample_split_events, gx_subsample_split_kept, gx_reproducibility)
GX_REPRO_ALONE, GX_REPRO_SELF, GX_REPRO_POOLED = 0, 1, 2          # gx_repro_call.kind
REPRO_VERDICTS = ("pass", "borderline", "fail", "NA")              # GX_REPRO_PASS .. GX_REPRO_NA
REPRO_CALL_DTYPE = np.dtype([("kind", "<i4"), ("rep", "<i4"), ("half", "<i4"), ("status", "<i4"), ("n_events", "<u8"), ("n_peaks", "<u8"),
                             ("peak_bp", "<u8")])   # gx_repro_call
REPRO_FIGURES_DTYPE = np.dtype([(k, "<i4") for k in ("n_rep", "best_i", "best_j", "verdict", "rescue_na", "self_na", "optimal_is_pooled", "_pad")]
                               + [(k, "<u8") for k in ("nt", "np", "n_self_max", "n_self_min", "n_conservative", "n_optimal")]
                               + [("rescue", "<f8"), ("self_consistency", "<f8")])   # gx_repro_figures


GX_PATH_DEPTH = 33554432        # gx_path_info bit 25: k_depth_hist ran (gx_set_depth_hist)
DEPTH_BOUND = 2048              # GX_DEPTH_BOUND: whole depths below it are counted per class, the others listed with their exact pileup
DEPTH_GE = (1, 2, 5, 10, 20, 50, 100)
DEPTH_METRICS_DTYPE = np.dtype([(k, "<u8") for k in ("bases", "excluded", "covered", "min_v", "max_v", "q25", "median", "q75", "p95", "p99")]
                               + [(k, "<f8") for k in ("covered_fraction", "mean", "sd")] + [("ge", "<f8", (len(DEPTH_GE),))])   # gx_depth_metrics_t


class DepthHist(C.Structure):
    """gx_depth_hist: the scalars of one sample's depth distribution and pointers to its arrays."""
    _fields_ = [("rep", C.c_int32), ("is_ctrl", C.c_int32), ("total", C.c_uint64), ("excluded", C.c_uint64), ("zero", C.c_uint64),
                ("min_v", C.c_uint64), ("max_v", C.c_uint64), ("bases", C.c_void_p), ("rsum", C.c_void_p), ("rsq", C.c_void_p),
                ("deep_v", C.c_void_p), ("deep_bases", C.c_void_p), ("n_deep", C.c_size_t)]


class Depth(NamedTuple):
    """One sample's depth distribution (gx_get_depth): bases / rsum / rsq uint64[DEPTH_BOUND] per whole depth, deep = [(v, bases)]
    ascending with the exact pileup v (1/120 units) of the bases at DEPTH_BOUND or deeper."""
    rep: int
    is_ctrl: bool
    total: int
    excluded: int
    zero: int
    min_v: int
    max_v: int
    bases: np.ndarray
    rsum: np.ndarray
    rsq: np.ndarray
    deep: list


class Xcor(NamedTuple):
    """One sample's strand cross-correlation counts (gx_get_xcor): N bases, set bits per strand, refused tags, n11[d - lo]."""
    n_pos: int
    n_plus: int
    n_minus: int
    rejected: int
    lo: int
    hi: int
    n11: list
    rep: int = 0
    is_ctrl: bool = False


class GcBias(NamedTuple):
    """One sample's GC tables (gx_get_gc_bias): F / Nn / Nw uint64[W + 1] per window class, and what is not classed."""
    window: int
    F: np.ndarray
    f_unclassed: int
    Nn: np.ndarray
    Nw: np.ndarray
    n_unclassed: int
    w_unclassed: int
    rep: int = 0
    is_ctrl: bool = False


class IntervalStats(NamedTuple):
    """One sample's interval lengths and chromosome tallies (gx_get_interval_lengths, gx_get_chrom_stats): lengths = [(L, n, w120)]
    ascending, the inverted intervals, and cn / cw120 / cbases120 per chromosome of the table."""
    lengths: list
    n_inverted: int
    w120_inverted: int
    cn: list
    cw120: list
    cbases120: list
    rep: int = 0
    is_ctrl: bool = False


class Complexity(NamedTuple):
    """One sample's library complexity (gx_get_complexity): N observations, D distinct keys, pairs = [(m, h[m])] ascending."""
    n_obs: int
    n_distinct: int
    pairs: list
    rep: int
    is_ctrl: bool


class RankTable(C.Structure):
    """gx_rank_table (value ascending, count) and gx_rank_lut (value ascending, rank2): the same layout."""
    _fields_ = [("value", C.c_void_p), ("second", C.c_void_p), ("n", C.c_size_t)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_int64), C.c_size_t, C.c_void_p)


class GxParams(C.Structure):
    """gx_params: the peak-calling tail of runProgram's arguments (Genrich.c:5390-5395)."""
    _fields_ = [
        ("thr", C.c_float), ("qval_opt", C.c_int32), ("min_auc", C.c_float),
        ("min_len", C.c_int32), ("max_gap", C.c_int32), ("device", C.c_int32),
        ("genome_len", C.c_uint64),
    ]


_libm = C.CDLL("libm.so.6")
_libm.log10f.restype = C.c_float
_libm.log10f.argtypes = [C.c_float]


def minus_log10f(x: float) -> float:
    """getArgs: pqvalue = -log10f(pqvalue) (Genrich.c:5817), with the host's libm."""
    return float(-_libm.log10f(C.c_float(x)))


_lib = None

_SIGS = {
    "gx_create": [C.POINTER(C.c_void_p), C.POINTER(GxParams)],
    "gx_destroy": [C.c_void_p],
    "gx_reset": [C.c_void_p],
    "gx_set_chroms": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "gx_set_owned": [C.c_void_p, C.c_void_p],
    "gx_set_keep_pileups": [C.c_void_p, C.c_int],
    "gx_expect_fractional": [C.c_void_p, C.c_int],
    "gx_set_knob": [C.c_void_p, C.c_char_p, C.c_char_p],
    "gx_set_collectives": [C.c_void_p, C.c_int, C.c_int, ALLREDUCE_FN, C.c_void_p],
    "gx_rccl_unique_id": [C.c_void_p, C.c_size_t],
    "gx_set_rccl": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "gx_sample_begin": [C.c_void_p, C.c_int, C.c_void_p],
    "gx_push_events": [C.c_void_p, C.c_void_p, C.c_size_t],
    "gx_push_events_device": [C.c_void_p, C.c_void_p, C.c_size_t],
    "gx_push_events_pinned": [C.c_void_p, C.c_void_p, C.c_size_t],
    "gx_push_events_packed": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int],
    "gx_event8_pack": [C.c_void_p, C.c_void_p],
    "gx_sample_end": [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_float)],
    "gx_sample_no_control": [C.c_void_p, C.POINTER(C.c_float)],
    "gx_saturation_dropped": [C.c_void_p, C.POINTER(C.c_longlong)],
    "gx_window_net": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p],
    "gx_dups_first": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p],
    "gx_dups_geometry": [C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_void_p],
    "gx_pvalues": [C.c_void_p],
    "gx_find_peaks": [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    "gx_get_peaks": [C.c_void_p, C.c_void_p, C.c_size_t],
    "gx_peak_count": [C.c_void_p, C.POINTER(C.c_size_t)],
    "gx_write_narrowpeak_path": [C.c_void_p, C.c_void_p, C.c_char_p],
    "gx_write_narrowpeak_group": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "gx_write_pile_path": [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int],
    "gx_write_log_path": [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_char_p],
    "gx_total_intervals": [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)],
    "gx_interval_count": [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t)],
    "gx_get_intervals": [C.c_void_p, C.c_int, C.c_int, C.c_size_t] + [C.c_void_p] * 5,
    "gx_selftest": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
    "gx_selftest2": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)],
    "gx_selftest_host": [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
    "gx_path_info": [C.c_void_p, C.POINTER(C.c_uint)],
    "gx_set_count_in_peaks": [C.c_void_p, C.c_int],
    "gx_count_in_peaks": [C.c_void_p, C.POINTER(C.c_int)],
    "gx_get_peak_counts": [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_size_t,
                           C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "gx_count_in_regions": [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)],
    "gx_get_region_counts": [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_size_t,
                             C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "gx_write_region_counts_group": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p],
    "gx_write_region_counts": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p],
    "gx_write_region_counts_path": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_char_p],
    "gx_write_counts_group": [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "gx_write_counts": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "gx_write_counts_path": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_char_p],
    "gx_peak_signal": [C.c_void_p, C.POINTER(C.c_int)],
    "gx_get_peak_signal": [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)] + [C.c_void_p] * 5 + [C.c_size_t],
    "gx_peak_signal_events": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint] + [C.c_void_p] * 5,
    "gx_peak_signal_geometry": [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)],
    "gx_format_peak_signal": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int] + [C.c_void_p] * 7,
    "gx_write_peak_signal_group": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "gx_write_peak_signal": [C.c_void_p, C.c_void_p, C.c_void_p],
    "gx_peak_summits": [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t)],
    "gx_get_peak_summits": [C.c_void_p, C.c_void_p, C.c_size_t],
    "gx_peak_summits_events": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_size_t,
                               C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)],
    "gx_peak_summits_last": [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_uint)],
    "gx_peak_summits_geometry": [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                 C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)],
    "gx_format_summits": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t],
    "gx_write_summits_group": [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "gx_write_summits": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "gx_set_coverage_bins": [C.c_void_p, C.c_uint32],
    "gx_coverage_samples": [C.c_void_p, C.POINTER(C.c_int)],
    "gx_coverage_bin_count": [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)],
    "gx_coverage_layout": [C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
    "gx_get_coverage": [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_size_t],
    "gx_format_coverage": [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_double],
    "gx_write_coverage_group": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_void_p],
    "gx_write_coverage": [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_void_p],
    "gx_write_coverage_path": [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_char_p],
    "gx_set_profile": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_int],
    "gx_profile_samples": [C.c_void_p, C.POINTER(C.c_int)],
    "gx_profile_layout": [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                          C.POINTER(C.c_int)],
    "gx_get_profile": [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t],
    "gx_format_profile": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32],
    "gx_format_profile_rows": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32,
                               C.c_uint32, C.c_void_p],
    "gx_write_profile_group": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p],
    "gx_write_profile_rows_group": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "gx_coverage_gram": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_int],
    "gx_gram_u64": [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_uint, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p],
    "gx_format_correlation": [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int],
    "gx_write_correlation_group": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p],
    "gx_gram_geometry": [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "gx_correlation_matrix": [C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "gx_coverage_gram_group": [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p],
    "gx_coverage_fingerprint": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_int],
    "gx_fp_u64": [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_uint, C.c_void_p, C.c_void_p],
    "gx_fp_geometry": [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "gx_fingerprint_metrics": [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "gx_format_fingerprint": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "gx_format_fingerprint_metrics": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "gx_coverage_fingerprint_group": [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p],
    "gx_write_fingerprint_group": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "gx_coverage_distinct": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)],
    "gx_rank_tables": [C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint64)],
    "gx_coverage_rank_gram": [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p,
                              C.c_void_p, C.c_int],
    "gx_coverage_spearman_group": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p],
    "gx_write_spearman_group": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p],
    "gx_distinct_u64": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)],
    "gx_rank_u64": [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_uint, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)],
    "gx_rank_geometry": [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)],
    "gx_rank_last": [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int)],
    "gx_complexity": [C.c_void_p, C.POINTER(C.c_int)],
    "gx_get_complexity": [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p,
                          C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)],
    "gx_complexity_events": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p,
                             C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)],
    "gx_complexity_geometry": [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_size_t)],
    "gx_complexity_last": [C.c_void_p, C.POINTER(C.c_size_t)],
    "gx_complexity_group": [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                            C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)],
    "gx_set_xcor": [C.c_void_p, C.c_int, C.c_int],
    "gx_push_tags": [C.c_void_p, C.c_void_p, C.c_size_t],
    "gx_xcor_samples": [C.c_void_p, C.POINTER(C.c_int)],
    "gx_get_xcor": [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)] + [C.POINTER(C.c_uint64)] * 4 + [C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                                                                                  C.c_void_p, C.c_size_t],
    "gx_xcor_group": [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)] + [C.POINTER(C.c_uint64)] * 4
                     + [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_size_t],
    "gx_xcor_tags": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_uint, C.c_uint32] + [C.POINTER(C.c_uint64)] * 4
                    + [C.c_void_p, C.c_size_t],
    "gx_xcor_geometry": [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)],
    "gx_xcor_metrics": [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p],
    "gx_xcor_r": [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "gx_format_xcor": [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p],
    "gx_format_xcor_metrics": [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_void_p, C.c_int],
    "gx_write_xcor_group": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "gx_set_genome": [C.c_void_p, C.c_int],
    "gx_push_sequence": [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_size_t],
    "gx_genome_info": [C.c_void_p] + [C.POINTER(C.c_uint64)] * 3,
    "gx_gc_content": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p],
    "gx_gc_bias": [C.c_void_p, C.c_int, C.POINTER(C.c_int)],
    "gx_get_gc_bias": [C.c_void_p, C.c_int] + [C.POINTER(C.c_int)] * 3 + [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p,
                                                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_size_t],
    "gx_gc_bias_group": [C.c_void_p, C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 3 + [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p,
                                                                                    C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_size_t],
    "gx_gc_bias_events": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_uint, C.c_uint32, C.c_uint64, C.c_uint, C.c_void_p,
                          C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_size_t],
    "gx_gc_geometry": [C.POINTER(C.c_int), C.POINTER(C.c_int)] + [C.POINTER(C.c_uint32)] * 4 + [C.POINTER(C.c_uint64)],
    "gx_gc_class": [C.c_int, C.c_int],
    "gx_gc_metrics": [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p],
    "gx_format_gc_bias": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6,
    "gx_format_gc_peaks": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p],
    "gx_write_gc_bias_group": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "gx_write_gc_peaks_group": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "gx_set_genome_bases": [C.c_void_p, C.c_int],
    "gx_get_sequence": [C.c_void_p, C.c_int, C.c_uint64, C.c_size_t, C.c_void_p],
    "gx_set_motifs": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "gx_motif_scan_regions": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_uint32, C.c_uint32, C.c_size_t, C.c_void_p, C.c_size_t,
                              C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p, C.c_void_p],
    "gx_motif_scan_peaks": [C.c_void_p, C.POINTER(C.c_size_t)],
    "gx_get_motif_hits": [C.c_void_p, C.c_void_p, C.c_size_t],
    "gx_get_motif_counts": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
    "gx_motif_last": [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
    "gx_motif_scan_genome": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
    "gx_motif_scan_genome_group": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
    "gx_motif_geometry": [C.POINTER(C.c_int), C.POINTER(C.c_int)] + [C.POINTER(C.c_uint32)] * 3 + [C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)],
    "gx_motif_grid": [C.c_uint64, C.c_uint32, C.c_uint, C.POINTER(C.c_uint)],
    "gx_write_motifs_group": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p],
    "gx_motif_pssm": [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_char_p, C.c_size_t],
    "gx_motif_threshold": [C.c_void_p, C.c_int, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                           C.POINTER(C.c_double), C.POINTER(C.c_int)],
    "gx_format_motif_hits": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                             C.c_void_p, C.c_size_t],
    "gx_format_motif_summary": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
                                C.c_void_p, C.c_void_p],
    "gx_write_motif_hits_group": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "gx_write_motif_summary_group": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "gx_kmer_count_regions": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_uint, C.c_uint32, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)],
    "gx_kmer_count_peaks": [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    "gx_get_kmer_counts": [C.c_void_p, C.c_void_p, C.c_size_t],
    "gx_kmer_count_genome": [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)],
    "gx_kmer_count_genome_group": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)],
    "gx_kmer_last": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint32)],
    "gx_kmer_force_hbm": [C.c_void_p, C.c_int],
    "gx_kmer_geometry": [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int),
                         C.POINTER(C.c_int)],
    "gx_kmer_stats": [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)],
    "gx_format_kmers": [C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int],
    "gx_write_kmers_group": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "gx_interval_stats": [C.c_void_p, C.POINTER(C.c_int)],
    "gx_get_interval_lengths": [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    "gx_get_chrom_stats": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
    "gx_interval_stats_events": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                 C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
    "gx_interval_stats_geometry": [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)],
    "gx_interval_stats_last": [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int)],
    "gx_interval_stats_group": [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
    "gx_lengths_metrics": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p],
    "gx_format_lengths": [C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.c_int],
    "gx_format_lengths_metrics": [C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_int],
    "gx_format_chrom_stats": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5,
    "gx_write_interval_stats_group": [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "gx_complexity_metrics": [C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p],
    "gx_format_complexity": [C.c_void_p, C.c_int] + [C.c_void_p] * 7,
    "gx_format_complexity_hist": [C.c_void_p, C.c_int] + [C.c_void_p] * 5,
    "gx_write_complexity_group": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "gx_set_depth_hist": [C.c_void_p, C.c_int],
    "gx_depth_samples": [C.c_void_p, C.POINTER(C.c_int)],
    "gx_get_depth": [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_size_t, C.POINTER(C.c_size_t)],
    "gx_depth_group": [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_size_t, C.POINTER(C.c_size_t)],
    "gx_depth_geometry": [C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)],
    "gx_depth_last": [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int)],
    "gx_depth_metrics": [C.c_void_p, C.c_void_p],
    "gx_format_depth": [C.c_void_p, C.c_int, C.c_void_p],
    "gx_format_depth_metrics": [C.c_void_p, C.c_int, C.c_void_p],
    "gx_write_depth_group": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "gx_subsample_events": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint, C.c_void_p, C.c_size_t,
                            C.POINTER(C.c_size_t)],
    "gx_subsample_kept": [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)],
    "gx_subsample_geometry": [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint32)],
    "gx_saturation": [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_uint, C.c_void_p],
    "gx_get_saturation_peaks": [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t],
    "gx_saturation_thresholds": [C.c_int, C.c_void_p],
    "gx_saturation_overlap": [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    "gx_format_saturation": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64],
    "gx_write_saturation": [C.c_void_p, C.c_void_p],
    "gx_subsample_split_events": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint, C.c_void_p, C.c_size_t,
                                  C.POINTER(C.c_size_t)],
    "gx_subsample_split_kept": [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)],
    "gx_reproducibility": [C.c_void_p, C.c_uint64, C.c_uint, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)],
    "gx_get_reproducibility_peaks": [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t],
    "gx_peaks_supported": [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p],
    "gx_reproducibility_figures": [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p],
    "gx_reproducibility_label": [C.c_void_p, C.c_char_p, C.c_size_t],
    "gx_format_reproducibility": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64],
    "gx_format_reproducibility_metrics": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "gx_format_narrowpeak": [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p],
    "gx_write_reproducibility": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "gx_rccl_nranks": [C.c_void_p, C.POINTER(C.c_int)],
    "gx_set_phase_filter": [C.c_void_p, C.c_char_p],
    "gx_set_phase_timing": [C.c_void_p, C.c_int],
    "gx_phase_times": [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.POINTER(C.c_float))],
}


def load_library(path: str = os.environ.get("GENRICH_AMD_LIB", LIB_PATH)):
    """Load libgenrich_amd.so and declare every entry point of include/genrich_amd.h.
    Raises if the library or a symbol is missing -- there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = C.CDLL(path)
    for name, args in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.argtypes = args
        fn.restype = None if name == "gx_destroy" else C.c_int
    lib.gx_last_error.restype = C.c_char_p
    lib.gx_last_error.argtypes = [C.c_void_p]
    lib.gx_strerror.restype = C.c_char_p
    lib.gx_strerror.argtypes = [C.c_int]
    lib.gx_filter_saturation.restype = C.c_longlong
    lib.gx_filter_saturation.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    lib.gx_fp_class.restype, lib.gx_fp_class.argtypes = C.c_uint32, [C.c_uint64]
    lib.gx_subsample_draw.restype, lib.gx_subsample_draw.argtypes = C.c_uint32, [C.c_uint64, C.c_uint32, C.c_uint64]
    lib.gx_kmer_revcomp.restype, lib.gx_kmer_revcomp.argtypes = C.c_uint32, [C.c_int, C.c_uint32]
    lib.gx_fp_class_lo.restype, lib.gx_fp_class_lo.argtypes = C.c_uint64, [C.c_uint32]
    lib.gx_fp_class_hi.restype, lib.gx_fp_class_hi.argtypes = C.c_uint64, [C.c_uint32]
    _lib = lib
    return lib


def filter_saturation(events, lens):
    """keep flags (uint8) for `events` under the reference's int16 saturation rule (Genrich.c:2558-2573);
    host-only, needs no GPU."""
    import numpy as np
    lib = load_library()
    ev = np.ascontiguousarray(events)
    ln = np.ascontiguousarray(lens, dtype=np.uint32)
    keep = np.ones(len(ev), dtype=np.uint8)
    rc = lib.gx_filter_saturation(ev.ctypes.data, len(ev), len(ln), ln.ctypes.data, keep.ctypes.data)
    if rc < 0:
        raise RuntimeError(f"gx_filter_saturation: {rc}")
    return keep, int(rc)


def format_coverage(chrom_name, length, bin_size, sum120, scale=1.0) -> bytes:
    """--coverage's bedGraph lines of one chromosome's bins (gx_format_coverage); host-only, needs no GPU."""
    lib = load_library()
    libc = C.CDLL(None)
    libc.tmpfile.restype = C.c_void_p
    libc.fclose.argtypes = [C.c_void_p]
    libc.fflush.argtypes = [C.c_void_p]
    libc.fileno.argtypes = [C.c_void_p]
    a = np.ascontiguousarray(sum120, dtype=np.int64)
    f = libc.tmpfile()
    if not f:
        raise RuntimeError("tmpfile failed")
    try:
        rc = lib.gx_format_coverage(f, chrom_name.encode(), int(length), int(bin_size), a.ctypes.data if a.size else None, a.size,
                                    float(scale))
        if rc:
            raise RuntimeError(f"gx_format_coverage: {rc}")
        libc.fflush(f)
        fd = os.dup(libc.fileno(f))
    finally:
        libc.fclose(f)
    with os.fdopen(fd, "rb") as g:
        g.seek(0)
        return g.read()


def _to_tmpfile(call) -> bytes:
    """What call(FILE*) writes (a host-only writer of gx_emit.cpp); raises when it returns an error."""
    libc = C.CDLL(None)
    libc.tmpfile.restype = C.c_void_p
    libc.fclose.argtypes = [C.c_void_p]
    libc.fflush.argtypes = [C.c_void_p]
    libc.fileno.argtypes = [C.c_void_p]
    f = libc.tmpfile()
    if not f:
        raise RuntimeError("tmpfile failed")
    try:
        rc = call(f)
        if rc:
            raise RuntimeError(f"writer: {rc}")
        libc.fflush(f)
        fd = os.dup(libc.fileno(f))
    finally:
        libc.fclose(f)
    with os.fdopen(fd, "rb") as g:
        g.seek(0)
        return g.read()


def _c_names(names):
    arr = (C.c_char_p * max(len(names), 1))()
    for i, n in enumerate(names):
        arr[i] = None if n is None else n.encode()
    return arr


def format_profile(sample_names, agg120, n_anchors_counted, flank, bin_size) -> bytes:
    """--profile's aggregate table (gx_format_profile) of the samples' aggregates agg120[s]; host-only, needs no GPU."""
    lib = load_library()
    rows = [np.ascontiguousarray(a, dtype=np.int64) for a in agg120]
    n_bins = len(rows[0]) if rows else 2 * int(flank) // max(int(bin_size), 1)
    ptrs = (C.c_void_p * max(len(rows), 1))(*[r.ctypes.data for r in rows])
    names = _c_names(list(sample_names))
    return _to_tmpfile(lambda f: lib.gx_format_profile(f, len(rows), names, ptrs, int(n_anchors_counted), int(n_bins), int(flank),
                                                       int(bin_size)))


def format_profile_rows(names, regions, row_names, anchors, first, cell120, bin_size) -> bytes:
    """--profile-matrix's rows (gx_format_profile_rows): regions (REGION_DTYPE), row_names (None: anchor_N) and anchors
    (ANCHOR_DTYPE) are indexed by anchor, cell120 holds the rows first .. first + len(cell120) - 1; host-only."""
    lib = load_library()
    reg = np.ascontiguousarray(regions, dtype=REGION_DTYPE)
    anc = np.ascontiguousarray(anchors, dtype=ANCHOR_DTYPE)
    cells = np.ascontiguousarray(cell120, dtype=np.int64)
    n_rows, n_bins = cells.shape
    cn = _c_names(list(names))
    rn = _c_names(list(row_names)) if row_names is not None else None
    return _to_tmpfile(lambda f: lib.gx_format_profile_rows(f, cn, reg.ctypes.data, rn, anc.ctypes.data, int(first), n_rows, n_bins,
                                                            int(bin_size), cells.ctypes.data))


def gram_geometry():
    """(tile, lanes, grid) of k_gram as the library was built (gx_gram_geometry): the samples along a tile's edge, the lanes of a
    workgroup, the most workgroups along the bin axis by default."""
    lib = load_library()
    t, l, g = C.c_int(0), C.c_int(0), C.c_int(0)
    lib.gx_gram_geometry(C.byref(t), C.byref(l), C.byref(g))
    return t.value, l.value, g.value


def correlation_matrix(n, n_zero, sums, gram, skip_zeros=False):
    """The Pearson matrix as float64 [S, S] (gx_correlation_matrix), NaN where there is none; host-only."""
    lib = load_library()
    S = len(sums)
    s, g = _split128(sums, (S,)), _split128(gram, (S, S))
    r = np.zeros((S, S), dtype=np.float64)
    rc = lib.gx_correlation_matrix(S, int(n), int(n_zero), s.ctypes.data, g.ctypes.data, int(bool(skip_zeros)), r.ctypes.data)
    if rc:
        raise RuntimeError(f"gx_correlation_matrix: {rc}")
    return r


def format_correlation(sample_names, n, n_zero, sums, gram, skip_zeros=False) -> bytes:
    """--correlation's matrix (gx_format_correlation) from the exact sums: sums[S] and gram[S][S] as Python ints; host-only,
    needs no GPU."""
    lib = load_library()
    S = len(sample_names)
    s = _split128(sums, (S,))
    g = _split128(gram, (S, S))
    names = _c_names(list(sample_names))
    return _to_tmpfile(lambda f: lib.gx_format_correlation(f, S, names, int(n), int(n_zero), s.ctypes.data, g.ctypes.data,
                                                           int(bool(skip_zeros))))


def rank_geometry():
    """(lanes, grid, cache_entries, first_capacity, load_limit) of k_rank_distinct as the library was built (gx_rank_geometry):
    the lanes of a workgroup (two values each a step), the most workgroups by default, the entries of a workgroup's LDS cache,
    the table's first capacity and the distinct non-zero values it takes before it grows (half of any capacity)."""
    lib = load_library()
    l, g, c = C.c_int(0), C.c_int(0), C.c_int(0)
    cap, lim = C.c_size_t(0), C.c_size_t(0)
    lib.gx_rank_geometry(C.byref(l), C.byref(g), C.byref(c), C.byref(cap), C.byref(lim))
    return l.value, g.value, c.value, cap.value, lim.value


def _rank_structs(pairs):
    """[(first, second)] -> (a RankTable array, the arrays it points to)."""
    keep = []
    arr = (RankTable * max(len(pairs), 1))()
    for k, (a, b) in enumerate(pairs):
        a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
        if a.shape != b.shape or a.ndim != 1:
            raise ValueError("a table is two equally long vectors")
        keep += [a, b]
        arr[k] = RankTable(a.ctypes.data if a.size else None, b.ctypes.data if b.size else None, a.size)
    return arr, keep


def rank_tables(tables, n_zero_to_drop=0):
    """gx_rank_tables: tables[g][s] = (values ascending, counts) of context g's sample s -> (N, [(values, rank2) per sample]);
    host-only, needs no GPU.  Raises where the library refuses."""
    lib = load_library()
    G, S = len(tables), len(tables[0]) if tables else 0
    if any(len(t) != S for t in tables):
        raise ValueError("every context has one table per sample")
    arr, keep = _rank_structs([t for ctx in tables for t in ctx])
    n_out = np.zeros(max(S, 1), dtype=np.uintp)
    N = C.c_uint64(0)
    rc = lib.gx_rank_tables(G, S, C.addressof(arr), int(n_zero_to_drop), None, None, 0, n_out.ctypes.data, C.byref(N))
    if rc:
        raise RuntimeError(f"gx_rank_tables: {rc}")
    cap = int(n_out[:S].max()) if S else 0
    vals = [np.zeros(cap, dtype=np.uint64) for _ in range(S)]
    ranks = [np.zeros(cap, dtype=np.uint64) for _ in range(S)]
    pv = (C.c_void_p * max(S, 1))(*[v.ctypes.data for v in vals])
    pr = (C.c_void_p * max(S, 1))(*[r.ctypes.data for r in ranks])
    rc = lib.gx_rank_tables(G, S, C.addressof(arr), int(n_zero_to_drop), pv, pr, cap, n_out.ctypes.data, C.byref(N))
    if rc:
        raise RuntimeError(f"gx_rank_tables: {rc}")
    return N.value, [(vals[s][:int(n_out[s])], ranks[s][:int(n_out[s])]) for s in range(S)]


def coverage_spearman_group(ctxs, skip_zeros=False):
    """(N, sum, gram, n_distinct) of the rank rows over the contexts of a run (gx_coverage_spearman_group): Python ints, sum an
    object array [S], gram [S, S], n_distinct the entries of each sample's merged table."""
    lib = load_library()
    S = ctxs[0].coverage_samples()
    arr = (C.c_void_p * len(ctxs))(*[c.ctx for c in ctxs])
    s, g = _sums128(S)
    nd = np.zeros(max(S, 1), dtype=np.uint64)
    N = C.c_uint64(0)
    ctxs[0]._check(lib.gx_coverage_spearman_group(arr, len(ctxs), S, int(bool(skip_zeros)), C.byref(N), s.ctypes.data, g.ctypes.data,
                                                  nd.ctypes.data))
    return N.value, _join128(s[:S]), _join128(g[:S, :S]), [int(v) for v in nd[:S]]


def spearman_text(ctxs, sample_names, skip_zeros=False) -> bytes:
    """--spearman's matrix over the contexts of a run (gx_write_spearman_group)."""
    lib = load_library()
    arr = (C.c_void_p * len(ctxs))(*[c.ctx for c in ctxs])
    names = _c_names(list(sample_names))
    return _to_tmpfile(lambda f: lib.gx_write_spearman_group(arr, len(ctxs), len(sample_names), names, int(bool(skip_zeros)), f))


DUP_CONTESTED = 0x80000000      # gx_dups_first's owner word, bit 31: a multi-alignment set holds the key


def _dup_keys(keys):
    k = np.ascontiguousarray(keys, dtype=np.uint32)
    if k.ndim != 2 or k.shape[1] != 4:
        raise ValueError("keys: a uint32 array [n, 4]")
    return k


def dups_geometry(keys):
    """(capacity, home) of the -r table for these keys (uint32 [n, 4]) as the library was built (gx_dups_geometry): the slots
    gx_dups_first uses for n records and the slot at which each key's probe starts; host-only, needs no GPU."""
    k = _dup_keys(keys)
    cap = C.c_uint32(0)
    home = np.zeros(len(k), dtype=np.uint32)
    rc = load_library().gx_dups_geometry(k.ctypes.data if len(k) else None, len(k), C.byref(cap), home.ctypes.data if len(k) else None)
    if rc:
        raise RuntimeError(f"gx_dups_geometry: {rc}")
    return cap.value, home


def peak_signal_geometry():
    """(lanes of a workgroup of k_psig_reduce, its most workgroups, bases a wavefront covers per step, the multiple a peak's
    slots are padded to, the most events peak_signal_events takes) -- gx_peak_signal_geometry; needs no GPU."""
    lib = load_library()
    lanes, grid, step, pad, most = C.c_int(0), C.c_int(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    rc = lib.gx_peak_signal_geometry(C.byref(lanes), C.byref(grid), C.byref(step), C.byref(pad), C.byref(most))
    if rc:
        raise RuntimeError(f"gx_peak_signal_geometry: {rc}")
    return lanes.value, grid.value, step.value, pad.value, most.value


def _regions(regions):
    reg = np.asarray(regions)
    if reg.dtype != REGION_DTYPE:
        rows = np.asarray(regions, dtype=np.int64).reshape(-1, 3)
        reg = np.zeros(len(rows), dtype=REGION_DTYPE)
        reg["chrom"], reg["start"], reg["end"] = rows[:, 0], rows[:, 1], rows[:, 2]
    return np.ascontiguousarray(reg)


def format_peak_signal(names, peaks, samples) -> bytes:
    """--peak-signal's text (gx_format_peak_signal) of `samples` (PeakSignal each) in `peaks` (REGION_DTYPE, or rows of
    (chrom, start, end)); host-only, needs no GPU."""
    lib = load_library()
    reg = _regions(peaks)
    S = len(samples)
    cols = [[np.ascontiguousarray(getattr(x, f), dtype=t) for x in samples]
            for f, t in (("area", np.int64), ("max", np.int64), ("summit", np.uint32), ("covered", np.uint32), ("at_summit", np.int64))]
    ptrs = [(C.c_void_p * max(S, 1))(*[a.ctypes.data for a in col]) for col in cols]
    rep = (C.c_int * max(S, 1))(*[int(x.rep) for x in samples])
    ctrl = (C.c_int * max(S, 1))(*[int(x.is_ctrl) for x in samples])
    cn = _c_names(list(names))
    return _to_tmpfile(lambda f: lib.gx_format_peak_signal(f, cn, reg.ctypes.data if reg.size else None, reg.size, S, rep, ctrl, *ptrs))


def peak_summits_geometry():
    """(lanes of a workgroup of k_summits, its most workgroups, bases a wavefront covers per step, the runs of a peak a
    wavefront holds, the summit list's least first capacity, its entries per peak beyond that, the most events
    peak_summits_events takes) -- gx_peak_summits_geometry; needs no GPU."""
    lib = load_library()
    lanes, grid, step, runs, most = C.c_int(0), C.c_int(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    lmin, lper = C.c_uint64(0), C.c_uint32(0)
    rc = lib.gx_peak_summits_geometry(C.byref(lanes), C.byref(grid), C.byref(step), C.byref(runs), C.byref(lmin), C.byref(lper), C.byref(most))
    if rc:
        raise RuntimeError(f"gx_peak_summits_geometry: {rc}")
    return lanes.value, grid.value, step.value, runs.value, lmin.value, lper.value, most.value


def format_summits(names, peaks, summits) -> bytes:
    """--summits' text (gx_format_summits) of `summits` (SUMMIT_DTYPE, ascending in (peak, pos)) in `peaks` (REGION_DTYPE, or
    rows of (chrom, start, end)); host-only, needs no GPU."""
    lib = load_library()
    reg = _regions(peaks)
    sm = np.ascontiguousarray(summits, dtype=SUMMIT_DTYPE)
    cn = _c_names(list(names))
    return _to_tmpfile(lambda f: lib.gx_format_summits(f, cn, reg.ctypes.data if reg.size else None, reg.size, sm.ctypes.data if sm.size else None, sm.size))


def xcor_geometry():
    """(lanes, grid, tile_words, pad_words_for_4096, flush_words) of the cross-correlation pass as the library was built
    (gx_xcor_geometry): the lanes of a workgroup of k_xc_corr, its most workgroups with grid = 0, the default plus words per tile
    (the smallest a caller may ask for is XCOR_MIN_TILE), the zero words between chromosomes at the widest shifts, and the plus
    words a workgroup walks at most before its 32-bit counters are added to the 64-bit ones."""
    lib = load_library()
    lanes, grid, tile, pad, flush = C.c_int(0), C.c_int(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    lib.gx_xcor_geometry(C.byref(lanes), C.byref(grid), C.byref(tile), C.byref(pad), C.byref(flush))
    return lanes.value, grid.value, tile.value, pad.value, flush.value


def xcor_r(n_pos, n_plus, n_minus, lo, hi, n11):
    """r(d) for lo <= d <= hi as the library defines it (gx_xcor_r); NaN where undefined; host-only."""
    lib = load_library()
    a = np.ascontiguousarray(n11, dtype=np.uint64)
    out = np.zeros(max(a.size, 1), dtype=np.float64)
    rc = lib.gx_xcor_r(int(n_pos), int(n_plus), int(n_minus), int(lo), int(hi), a.ctypes.data if a.size == hi - lo + 1 else None, out.ctypes.data)
    if rc:
        raise RuntimeError(f"gx_xcor_r: {rc}")
    return out[:a.size]


def xcor_metrics(n_pos, n_plus, n_minus, lo, hi, n11, read_len=0):
    """gx_xcor_metrics as one XCOR_METRICS_DTYPE record; read_len 0: not given; host-only."""
    lib = load_library()
    a = np.ascontiguousarray(n11, dtype=np.uint64)
    out = np.zeros(1, dtype=XCOR_METRICS_DTYPE)
    rc = lib.gx_xcor_metrics(int(n_pos), int(n_plus), int(n_minus), int(lo), int(hi), a.ctypes.data if a.size == hi - lo + 1 else None, int(read_len),
                             out.ctypes.data)
    if rc:
        raise RuntimeError(f"gx_xcor_metrics: {rc}")
    return out[0]


def _xcor_cols(samples):
    """The writers' arrays from [Xcor]: (n, rep, ctrl, N, nP, nM, rejected, rows kept alive, row pointers)."""
    rep = np.ascontiguousarray([x.rep for x in samples], dtype=np.int32)
    ctrl = np.ascontiguousarray([int(x.is_ctrl) for x in samples], dtype=np.int32)
    cols = [np.ascontiguousarray([getattr(x, k) for x in samples], dtype=np.uint64) for k in ("n_pos", "n_plus", "n_minus", "rejected")]
    rows = [np.ascontiguousarray(x.n11, dtype=np.uint64) for x in samples]
    ptrs = (C.c_void_p * len(samples))(*[r.ctypes.data for r in rows])
    return rep, ctrl, cols, rows, ptrs


def format_xcor(samples) -> bytes:
    """--xcor's table for [Xcor] with one range of shifts (gx_format_xcor); host-only."""
    lib = load_library()
    rep, ctrl, cols, rows, ptrs = _xcor_cols(samples)
    return _to_tmpfile(lambda f: lib.gx_format_xcor(f, len(samples), rep.ctypes.data, ctrl.ctypes.data, *[c.ctypes.data for c in cols],
                                                    samples[0].lo, samples[0].hi, ptrs))


def format_xcor_metrics(samples, read_len=0) -> bytes:
    """--xcor-metrics' table for [Xcor] (gx_format_xcor_metrics); host-only."""
    lib = load_library()
    rep, ctrl, cols, rows, ptrs = _xcor_cols(samples)
    return _to_tmpfile(lambda f: lib.gx_format_xcor_metrics(f, len(samples), rep.ctypes.data, ctrl.ctypes.data, *[c.ctypes.data for c in cols[:3]],
                                                            samples[0].lo, samples[0].hi, ptrs, int(read_len)))


def _xcor_result(call, n_shifts):
    """An Xcor from call(rep, ctrl, N, nP, nM, rejected, lo, hi, n11, cap)."""
    rep, ctrl, lo, hi = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    N, nP, nM, rej = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    n11 = np.zeros(max(n_shifts, 1), dtype=np.uint64)
    call(C.byref(rep), C.byref(ctrl), C.byref(N), C.byref(nP), C.byref(nM), C.byref(rej), C.byref(lo), C.byref(hi), n11.ctypes.data, n_shifts)
    return Xcor(N.value, nP.value, nM.value, rej.value, lo.value, hi.value, [int(x) for x in n11[:hi.value - lo.value + 1]], rep.value, bool(ctrl.value))


def xcor_group(ctxs, sample):
    """Xcor of one sample added over the contexts of a run (gx_xcor_group)."""
    lib = load_library()
    arr = (C.c_void_p * len(ctxs))(*[c.ctx for c in ctxs])
    return _xcor_result(lambda *a: ctxs[0]._check(lib.gx_xcor_group(arr, len(ctxs), int(sample), *a)), 2 * XCOR_MAX_SHIFT + 1)


def xcor_text(ctxs, read_len=0):
    """(--xcor's table, --xcor-metrics') over the contexts of a run (gx_write_xcor_group)."""
    lib = load_library()
    arr = (C.c_void_p * len(ctxs))(*[c.ctx for c in ctxs])
    return (_to_tmpfile(lambda f: lib.gx_write_xcor_group(arr, len(ctxs), int(read_len), f, None)),
            _to_tmpfile(lambda f: lib.gx_write_xcor_group(arr, len(ctxs), int(read_len), None, f)))


def gc_geometry():
    """(lanes, grid, tile_words, min_tile_words, pad_words, block_bases, flush_words) of the GC passes as the library was built
    (gx_gc_geometry): the lanes of a workgroup of k_gc_expected, its most workgroups with grid = 0, its default and smallest words
    per tile, the zero words around a chromosome, the bases per directory block, and the words a workgroup walks at most before
    it adds its 32-bit counters to the 64-bit ones."""
    lib = load_library()
    lanes, grid, flush = C.c_int(0), C.c_int(0), C.c_uint64(0)
    t, mt, pad, blk = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    lib.gx_gc_geometry(C.byref(lanes), C.byref(grid), C.byref(t), C.byref(mt), C.byref(pad), C.byref(blk), C.byref(flush))
    return lanes.value, grid.value, t.value, mt.value, pad.value, blk.value, flush.value


def gc_class(window, g):
    """The percent class of g GC bases in a window of `window` (gx_gc_class; -1: out of range); host-only."""
    return int(load_library().gx_gc_class(int(window), int(g)))


def _gc_arrays(x):
    return [np.ascontiguousarray(a, dtype=np.uint64) for a in (x.F, x.Nn, x.Nw)]


def gc_metrics(x):
    """gx_gc_metrics of a GcBias as one GC_METRICS_DTYPE record; host-only."""
    lib = load_library()
    F, Nn, Nw = _gc_arrays(x)
    out = np.zeros(1, dtype=GC_METRICS_DTYPE)
    ok = F.size == Nn.size == Nw.size == int(x.window) + 1
    rc = lib.gx_gc_metrics(int(x.window), F.ctypes.data if ok else None, int(x.f_unclassed), Nn.ctypes.data, Nw.ctypes.data, int(x.n_unclassed),
                           int(x.w_unclassed), out.ctypes.data)
    if rc:
        raise RuntimeError(f"gx_gc_metrics: {rc}")
    return out[0]


def format_gc_bias(samples) -> bytes:
    """--gc-bias' table for [GcBias] of one window (gx_format_gc_bias); host-only."""
    lib = load_library()
    rep = np.ascontiguousarray([x.rep for x in samples], dtype=np.int32)
    ctrl = np.ascontiguousarray([int(x.is_ctrl) for x in samples], dtype=np.int32)
    rows = [_gc_arrays(x) for x in samples]
    ptrs = [(C.c_void_p * len(samples))(*[r[k].ctypes.data for r in rows]) for k in range(3)]
    sc = [np.ascontiguousarray([getattr(x, k) for x in samples], dtype=np.uint64) for k in ("f_unclassed", "n_unclassed", "w_unclassed")]
    return _to_tmpfile(lambda f: lib.gx_format_gc_bias(f, len(samples), rep.ctypes.data, ctrl.ctypes.data, int(samples[0].window), ptrs[0],
                                                       sc[0].ctypes.data, ptrs[1], ptrs[2], sc[1].ctypes.data, sc[2].ctypes.data))


def format_gc_peaks(names, regions, gc, acgt) -> bytes:
    """--gc-peaks' table for regions (REGION_DTYPE) with their counts (gx_format_gc_peaks); host-only."""
    lib = load_library()
    reg = np.ascontiguousarray(regions, dtype=REGION_DTYPE)
    g, a = np.ascontiguousarray(gc, dtype=np.uint64), np.ascontiguousarray(acgt, dtype=np.uint64)
    nm = (C.c_char_p * len(names))(*[n.encode() for n in names])
    return _to_tmpfile(lambda f: lib.gx_format_gc_peaks(f, nm, reg.ctypes.data, reg.size, g.ctypes.data, a.ctypes.data))


def _gc_result(call, window_cap=GC_MAX_WINDOW):
    """A GcBias from call(rep, ctrl, window, F, f_un, Nn, Nw, n_un, w_un, cap)."""
    rep, ctrl, w = C.c_int(0), C.c_int(0), C.c_int(0)
    fu, nu, wu = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    F, Nn, Nw = (np.zeros(window_cap + 1, dtype=np.uint64) for _ in range(3))
    call(C.byref(rep), C.byref(ctrl), C.byref(w), F.ctypes.data, C.byref(fu), Nn.ctypes.data, Nw.ctypes.data, C.byref(nu), C.byref(wu), window_cap + 1)
    k = w.value + 1
    return GcBias(w.value, F[:k].copy(), fu.value, Nn[:k].copy(), Nw[:k].copy(), nu.value, wu.value, rep.value, bool(ctrl.value))


def gc_bias_group(ctxs, sample):
    """GcBias of one sample added over the contexts of a run (gx_gc_bias_group)."""
    lib = load_library()
    arr = (C.c_void_p * len(ctxs))(*[c.ctx for c in ctxs])
    return _gc_result(lambda *a: ctxs[0]._check(lib.gx_gc_bias_group(arr, len(ctxs), int(sample), *a)))


def gc_bias_text(ctxs, window=200) -> bytes:
    """--gc-bias' table over the contexts of a run (gx_write_gc_bias_group)."""
    lib = load_library()
    arr = (C.c_void_p * len(ctxs))(*[c.ctx for c in ctxs])
    return _to_tmpfile(lambda f: ctxs[0]._check(lib.gx_write_gc_bias_group(arr, len(ctxs), int(window), f)))


def gc_peaks_text(ctxs, names) -> bytes:
    """--gc-peaks' table over the contexts of a run (gx_write_gc_peaks_group)."""
    lib = load_library()
    arr = (C.c_void_p * len(ctxs))(*[c.ctx for c in ctxs])
    nm = (C.c_char_p * len(names))(*[n.encode() for n in names])
    return _to_tmpfile(lambda f: ctxs[0]._check(lib.gx_write_gc_peaks_group(arr, len(ctxs), nm, f)))


def motif_geometry():
    """(lanes, grid, positions_per_step, step_words, batch_motifs, list_capacity, flush_runs) of the motif scan as the library was
    built (gx_motif_geometry): the lanes of a workgroup of k_motif_scan, its most workgroups with grid = 0, the positions a wavefront
    takes per step, the default runs of them per unit, the motifs per LDS batch, the first hit list's least capacity and the runs a
    workgroup walks at most per batch (its 32-bit counters)."""
    lib = load_library()
    lanes, grid = C.c_int(0), C.c_int(0)
    pos, step, batch = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    cap, flush = C.c_size_t(0), C.c_uint64(0)
    lib.gx_motif_geometry(C.byref(lanes), C.byref(grid), C.byref(pos), C.byref(step), C.byref(batch), C.byref(cap), C.byref(flush))
    return lanes.value, grid.value, pos.value, step.value, batch.value, cap.value, flush.value


def motif_grid(units, step_words=0, grid=0):
    """The workgroups a motif pass over `units` units of step_words runs takes (gx_motif_grid; host-only): the library's choice
    with grid = 0, else `grid` itself; None when the library refuses it (a workgroup would walk more than the flush bound, or a
    limit is broken)."""
    g = C.c_uint(0)
    rc = load_library().gx_motif_grid(int(units), int(step_words), int(grid), C.byref(g))
    return None if rc else g.value


def motif_pssm(counts, pseudocount=1.0):
    """(scores int16[L, 4] in column order A C G T, smin, smax) of a count matrix counts[4, L] (rows A C G T) in 1/128 bit against
    a uniform background (gx_motif_pssm); host-only.  ValueError with the library's sentence when it is refused."""
    lib = load_library()
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    if c.ndim != 2 or c.shape[0] != 4:
        raise ValueError("counts must be [4, L]")
    L = c.shape[1]
    s = np.zeros((max(L, 1), 4), dtype=np.int16)
    lo, hi = C.c_int32(0), C.c_int32(0)
    why = C.create_string_buffer(256)
    rc = lib.gx_motif_pssm(c.ctypes.data, L, float(pseudocount), s.ctypes.data, C.byref(lo), C.byref(hi), why, 256)
    if rc:
        raise ValueError(why.value.decode() or f"gx_motif_pssm: {rc}")
    return s[:L], lo.value, hi.value


def motif_threshold(scores, p):
    """(threshold, smin, smax, p_achieved, unreachable) of scores int16[L, 4] for the p-value p in (0, 1], counted exactly over all
    4^L L-mers (gx_motif_threshold); host-only."""
    lib = load_library()
    s = np.ascontiguousarray(scores, dtype=np.int16)
    t, lo, hi = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    pa, un = C.c_double(0.0), C.c_int(0)
    rc = lib.gx_motif_threshold(s.ctypes.data, s.shape[0], float(p), C.byref(t), C.byref(lo), C.byref(hi), C.byref(pa), C.byref(un))
    if rc:
        raise ValueError(f"gx_motif_threshold: {rc}")
    return t.value, lo.value, hi.value, pa.value, bool(un.value)


def pack_motifs(motifs):
    """(MOTIF_DTYPE records, int16 scores) for [(scores int16[L, 4], threshold)], as gx_set_motifs takes them."""
    rec = np.zeros(len(motifs), dtype=MOTIF_DTYPE)
    flat, at = [], 0
    for i, (s, t) in enumerate(motifs):
        s = np.ascontiguousarray(s, dtype=np.int16).reshape(-1, 4)
        rec[i] = (s.shape[0], at, int(t))
        flat.append(s.reshape(-1))
        at += s.size
    return rec, (np.concatenate(flat) if flat else np.zeros(0, dtype=np.int16))


def _motif_table_args(motifs, ids, motif_names, p_threshold):
    rec, _ = pack_motifs(motifs)
    p = np.ascontiguousarray(p_threshold, dtype=np.float64)
    return rec, _c_names(list(ids)), _c_names(list(motif_names)), p


def format_motif_hits(names, peaks, summit_off, motifs, ids, motif_names, p_threshold, hits) -> bytes:
    """--motif-hits' table (gx_format_motif_hits) of `hits` (MOTIF_HIT_DTYPE, sorted) in `peaks` (REGION_DTYPE) with their summits'
    offsets; motifs: [(scores, threshold)]; host-only."""
    lib = load_library()
    reg = np.ascontiguousarray(peaks, dtype=REGION_DTYPE)
    so = np.ascontiguousarray(summit_off, dtype=np.uint32)
    h = np.ascontiguousarray(hits, dtype=MOTIF_HIT_DTYPE)
    rec, ci, cn, p = _motif_table_args(motifs, ids, motif_names, p_threshold)
    nm = _c_names(names)
    return _to_tmpfile(lambda f: lib.gx_format_motif_hits(f, nm, reg.ctypes.data, so.ctypes.data, reg.size, rec.ctypes.data, ci, cn, p.ctypes.data, len(rec),
                                                          h.ctypes.data if h.size else None, h.size))


def format_motif_summary(peaks, motifs, ids, motif_names, p_threshold, hits, counts_peaks, counts_genome) -> bytes:
    """--motif-summary's table (gx_format_motif_summary); counts_*: uint64[3, motifs] windows, hits +, hits -; host-only."""
    lib = load_library()
    reg = np.ascontiguousarray(peaks, dtype=REGION_DTYPE)
    h = np.ascontiguousarray(hits, dtype=MOTIF_HIT_DTYPE)
    rec, ci, cn, p = _motif_table_args(motifs, ids, motif_names, p_threshold)
    cp, cg = np.ascontiguousarray(counts_peaks, dtype=np.uint64), np.ascontiguousarray(counts_genome, dtype=np.uint64)
    return _to_tmpfile(lambda f: lib.gx_format_motif_summary(f, reg.ctypes.data if reg.size else None, reg.size, rec.ctypes.data, ci, cn, p.ctypes.data, len(rec),
                                                             h.ctypes.data if h.size else None, h.size, cp.ctypes.data, cg.ctypes.data))


def motif_scan_genome_group(ctxs):
    """uint64[3, motifs] (windows, hits +, hits -) of the genome pass added over the contexts of a run (gx_motif_scan_genome_group)."""
    lib = load_library()
    arr = (C.c_void_p * len(ctxs))(*[c.ctx for c in ctxs])
    n = ctxs[0].n_motifs
    out = np.zeros((3, max(n, 1)), dtype=np.uint64)
    ctxs[0]._check(lib.gx_motif_scan_genome_group(arr, len(ctxs), out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, n))
    return out[:, :n]


def motif_hits_text(ctxs, names, motifs, ids, motif_names, p_threshold) -> bytes:
    """--motif-hits' table over the contexts of a run (gx_write_motif_hits_group)."""
    lib = load_library()
    arr = (C.c_void_p * len(ctxs))(*[c.ctx for c in ctxs])
    rec, ci, cn, p = _motif_table_args(motifs, ids, motif_names, p_threshold)
    nm = _c_names(names)
    return _to_tmpfile(lambda f: ctxs[0]._check(lib.gx_write_motif_hits_group(arr, len(ctxs), nm, rec.ctypes.data, ci, cn, p.ctypes.data, len(rec), f)))


def motif_summary_text(ctxs, motifs, ids, motif_names, p_threshold) -> bytes:
    """--motif-summary's table over the contexts of a run (gx_write_motif_summary_group)."""
    lib = load_library()
    arr = (C.c_void_p * len(ctxs))(*[c.ctx for c in ctxs])
    rec, ci, cn, p = _motif_table_args(motifs, ids, motif_names, p_threshold)
    return _to_tmpfile(lambda f: ctxs[0]._check(lib.gx_write_motif_summary_group(arr, len(ctxs), rec.ctypes.data, ci, cn, p.ctypes.data, len(rec), f)))


def kmer_geometry():
    """(lanes, grid, positions_per_step, step_words, flush_runs, max_k, lds_max_k) of the k-mer count as the library was built
    (gx_kmer_geometry); host-only."""
    lib = load_library()
    lanes, grid, mk, lk = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    pos, step, flush = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    lib.gx_kmer_geometry(C.byref(lanes), C.byref(grid), C.byref(pos), C.byref(step), C.byref(flush), C.byref(mk), C.byref(lk))
    return lanes.value, grid.value, pos.value, step.value, flush.value, mk.value, lk.value


def kmer_revcomp(k, code):
    """The code of the reverse complement of a k-mer's code (gx_kmer_revcomp); None where the library refuses; host-only."""
    r = load_library().gx_kmer_revcomp(int(k), int(code))
    return None if r == 0xffffffff else r


def _kmer_tables(k, counts_peaks, counts_genome):
    cp = np.ascontiguousarray(counts_peaks, dtype=np.uint64)
    cg = np.ascontiguousarray(counts_genome, dtype=np.uint64)
    if cp.size != 4 ** int(k) or cg.size != 4 ** int(k):
        raise ValueError("kmers: a table of 4^k counts")
    return cp, cg


def kmer_stats(k, counts_peaks, windows_peaks, counts_genome, windows_genome):
    """KMER_ROW_DTYPE rows, one per canonical k-mer counted in the peaks, sorted as --kmers prints them (gx_kmer_stats); host-only."""
    lib = load_library()
    cp, cg = _kmer_tables(k, counts_peaks, counts_genome)
    n = C.c_size_t(0)
    rc = lib.gx_kmer_stats(int(k), cp.ctypes.data, int(windows_peaks), cg.ctypes.data, int(windows_genome), None, 0, C.byref(n))
    if rc:
        raise RuntimeError(f"gx_kmer_stats: {rc}")
    rows = np.zeros(max(n.value, 1), dtype=KMER_ROW_DTYPE)
    rc = lib.gx_kmer_stats(int(k), cp.ctypes.data, int(windows_peaks), cg.ctypes.data, int(windows_genome), rows.ctypes.data, n.value, None)
    if rc:
        raise RuntimeError(f"gx_kmer_stats: {rc}")
    return rows[:n.value]


def format_kmers(k, flank, regions_counted, windows_peaks, windows_genome, counts_peaks, counts_genome, top=100) -> bytes:
    """--kmers' table (gx_format_kmers); host-only."""
    lib = load_library()
    cp, cg = _kmer_tables(k, counts_peaks, counts_genome)
    return _to_tmpfile(lambda f: lib.gx_format_kmers(f, int(k), int(flank), int(regions_counted), int(windows_peaks), int(windows_genome), cp.ctypes.data,
                                                     cg.ctypes.data, int(top)))


def kmer_count_genome_group(ctxs, k):
    """(counts uint64[4^k], windows) of the genome pass added over the contexts of a run (gx_kmer_count_genome_group)."""
    lib = load_library()
    arr = (C.c_void_p * len(ctxs))(*[c.ctx for c in ctxs])
    out = np.zeros(4 ** int(k), dtype=np.uint64)
    w = C.c_uint64(0)
    ctxs[0]._check(lib.gx_kmer_count_genome_group(arr, len(ctxs), int(k), out.ctypes.data, out.size, C.byref(w)))
    return out, w.value


def kmers_text(ctxs, k, flank=-1, top=100) -> bytes:
    """--kmers' table over the contexts of a run (gx_write_kmers_group)."""
    lib = load_library()
    arr = (C.c_void_p * len(ctxs))(*[c.ctx for c in ctxs])
    return _to_tmpfile(lambda f: ctxs[0]._check(lib.gx_write_kmers_group(arr, len(ctxs), int(k), int(flank), int(top), f, None)))


def interval_stats_geometry():
    """(lanes, grid, lds_bound, chrom_window, list_capacity) of the interval-length pass as the library was built
    (gx_interval_stats_geometry): the lanes of a workgroup of k_ivstat, its most workgroups with grid = 0, the length from which
    an interval goes to the list instead of an LDS counter, the chromosomes tallied in LDS, and the list's first capacity."""
    lib = load_library()
    lanes, grid, bound, win, cap = C.c_int(0), C.c_int(0), C.c_uint32(0), C.c_uint32(0), C.c_size_t(0)
    lib.gx_interval_stats_geometry(C.byref(lanes), C.byref(grid), C.byref(bound), C.byref(win), C.byref(cap))
    return lanes.value, grid.value, bound.value, win.value, cap.value


def _len_cols(lengths):
    return tuple(np.ascontiguousarray([t[k] for t in lengths], dtype=np.uint64) for k in range(3))


def lengths_metrics(lengths, cuts=(150, 300, 500)):
    """gx_lengths_metrics as one LEN_METRICS_DTYPE record; lengths: [(L, n, w120)] ascending; host-only."""
    lib = load_library()
    L, n, w = _len_cols(lengths)
    c = np.ascontiguousarray(list(cuts), dtype=np.uint64)
    out = np.zeros(1, dtype=LEN_METRICS_DTYPE)
    rc = lib.gx_lengths_metrics(L.ctypes.data if L.size else None, n.ctypes.data if L.size else None, w.ctypes.data if L.size else None, L.size,
                                c.ctypes.data if c.size else None, c.size, out.ctypes.data)
    if rc:
        raise RuntimeError(f"gx_lengths_metrics: {rc}")
    return out[0]


def _ivs_result(call, n_chrom):
    """An IntervalStats from call(rep, ctrl, length, n, w120, cap, n_classes, n_inv, w_inv, cn, cw, cb, chrom_cap), asked twice."""
    n = C.c_size_t(0)
    call(None, None, None, None, None, 0, C.byref(n), None, None, None, None, None, 0)
    L, k, w = (np.zeros(max(n.value, 1), dtype=np.uint64) for _ in range(3))
    cn, cw, cb = (np.zeros(max(n_chrom, 1), dtype=np.uint64) for _ in range(3))
    rep, ctrl, ni, wi = C.c_int(0), C.c_int(0), C.c_uint64(0), C.c_uint64(0)
    call(C.byref(rep), C.byref(ctrl), L.ctypes.data, k.ctypes.data, w.ctypes.data, n.value, C.byref(n), C.byref(ni), C.byref(wi), cn.ctypes.data,
         cw.ctypes.data, cb.ctypes.data, n_chrom)
    return IntervalStats([(int(a), int(b), int(c)) for a, b, c in zip(L[:n.value], k[:n.value], w[:n.value])], ni.value, wi.value,
                         [int(x) for x in cn[:n_chrom]], [int(x) for x in cw[:n_chrom]], [int(x) for x in cb[:n_chrom]], rep.value, bool(ctrl.value))


def interval_stats_group(ctxs, sample):
    """IntervalStats of one sample added over the contexts of a run (gx_interval_stats_group); every context has run interval_stats()."""
    lib = load_library()
    arr = (C.c_void_p * len(ctxs))(*[c.ctx for c in ctxs])
    return _ivs_result(lambda *a: ctxs[0]._check(lib.gx_interval_stats_group(arr, len(ctxs), int(sample), *a)), ctxs[0].n_chrom)


def interval_stats_text(ctxs, names, cut_sites=False, cuts=(150, 300, 500)):
    """(--lengths' table, --lengths-metrics', --chrom-stats') over the contexts of a run (gx_write_interval_stats_group)."""
    lib = load_library()
    arr = (C.c_void_p * len(ctxs))(*[c.ctx for c in ctxs])
    cn = _c_names(list(names))
    c = np.ascontiguousarray(list(cuts), dtype=np.uint64)
    out = []
    try:
        for k in range(3):
            files = [None, None, None]

            def one(f):
                files[k] = f
                return lib.gx_write_interval_stats_group(arr, len(ctxs), cn, len(names), int(bool(cut_sites)), c.ctypes.data if c.size else None,
                                                         c.size, *files)
            out.append(_to_tmpfile(one))
    except RuntimeError as e:
        raise RuntimeError(f"{e} [{'; '.join(lib.gx_last_error(x.ctx).decode() for x in ctxs)}]") from None
    return tuple(out)


def complexity_geometry(n=0):
    """(lanes, grid, lds_bound, least_capacity) of the complexity pass as the library was built (gx_complexity_geometry): the lanes
    of a workgroup of k_cpx_insert, its most workgroups with grid = 0, the multiplicity from which k_cpx_hist lists a key instead
    of counting it in LDS, and the least table capacity for a sample of n events."""
    lib = load_library()
    lanes, grid, bound, cap = C.c_int(0), C.c_int(0), C.c_uint32(0), C.c_size_t(0)
    lib.gx_complexity_geometry(C.byref(lanes), C.byref(grid), C.byref(bound), int(n), C.byref(cap))
    return lanes.value, grid.value, bound.value, cap.value


def _cpx_pairs(pairs):
    m = np.ascontiguousarray([p[0] for p in pairs], dtype=np.uint64)
    k = np.ascontiguousarray([p[1] for p in pairs], dtype=np.uint64)
    return m, k


def complexity_metrics(n_obs, n_distinct, pairs):
    """gx_complexity_metrics as one CPX_METRICS_DTYPE record; pairs: [(m, h[m])] ascending; host-only."""
    lib = load_library()
    m, k = _cpx_pairs(pairs)
    out = np.zeros(1, dtype=CPX_METRICS_DTYPE)
    rc = lib.gx_complexity_metrics(int(n_obs), int(n_distinct), m.ctypes.data if m.size else None, k.ctypes.data if k.size else None, m.size,
                                   out.ctypes.data)
    if rc:
        raise RuntimeError(f"gx_complexity_metrics: {rc}")
    return out[0]


def _cpx_samples(samples):
    """samples: [(rep, is_ctrl, N, D, pairs)] -> the arrays gx_format_complexity* take (and what keeps them alive)."""
    S = len(samples)
    rep = np.ascontiguousarray([s[0] for s in samples], dtype=np.int32)
    ctrl = np.ascontiguousarray([int(bool(s[1])) for s in samples], dtype=np.int32)
    N = np.ascontiguousarray([s[2] for s in samples], dtype=np.uint64)
    D = np.ascontiguousarray([s[3] for s in samples], dtype=np.uint64)
    cols = [_cpx_pairs(s[4]) for s in samples]
    pm = (C.c_void_p * max(S, 1))(*[c[0].ctypes.data if c[0].size else None for c in cols])
    pk = (C.c_void_p * max(S, 1))(*[c[1].ctypes.data if c[1].size else None for c in cols])
    npairs = (C.c_size_t * max(S, 1))(*[c[0].size for c in cols])
    return S, rep, ctrl, N, D, pm, pk, npairs, cols


def format_complexity(samples) -> bytes:
    """--complexity's table (gx_format_complexity); samples: [(rep, is_ctrl, N, D, pairs)]; host-only, needs no GPU."""
    lib = load_library()
    S, rep, ctrl, N, D, pm, pk, npairs, keep = _cpx_samples(samples)
    return _to_tmpfile(lambda f: lib.gx_format_complexity(f, S, rep.ctypes.data, ctrl.ctypes.data, N.ctypes.data, D.ctypes.data, pm, pk, npairs))


def format_complexity_hist(samples) -> bytes:
    """--complexity-hist's table (gx_format_complexity_hist); samples as for format_complexity."""
    lib = load_library()
    S, rep, ctrl, N, D, pm, pk, npairs, keep = _cpx_samples(samples)
    return _to_tmpfile(lambda f: lib.gx_format_complexity_hist(f, S, rep.ctypes.data, ctrl.ctypes.data, pm, pk, npairs))


def complexity_group(ctxs, sample):
    """Complexity of one sample added over the contexts of a run (gx_complexity_group); every context has run complexity()."""
    lib = load_library()
    arr = (C.c_void_p * len(ctxs))(*[c.ctx for c in ctxs])
    n = C.c_size_t(0)
    ctxs[0]._check(lib.gx_complexity_group(arr, len(ctxs), int(sample), None, None, None, None, None, None, 0, C.byref(n)))
    m, k = np.zeros(max(n.value, 1), dtype=np.uint64), np.zeros(max(n.value, 1), dtype=np.uint64)
    rep, ctrl, N, D = C.c_int(0), C.c_int(0), C.c_uint64(0), C.c_uint64(0)
    ctxs[0]._check(lib.gx_complexity_group(arr, len(ctxs), int(sample), C.byref(rep), C.byref(ctrl), C.byref(N), C.byref(D), m.ctypes.data,
                                           k.ctypes.data, n.value, C.byref(n)))
    return Complexity(N.value, D.value, [(int(a), int(b)) for a, b in zip(m[:n.value], k[:n.value])], rep.value, bool(ctrl.value))


def complexity_text(ctxs, with_hist=True):
    """(--complexity's table, --complexity-hist's) over the contexts of a run (gx_write_complexity_group)."""
    lib = load_library()
    arr = (C.c_void_p * len(ctxs))(*[c.ctx for c in ctxs])
    hist = []

    def both(f):
        if not with_hist:
            return lib.gx_write_complexity_group(arr, len(ctxs), f, None)
        hist.append(_to_tmpfile(lambda h: lib.gx_write_complexity_group(arr, len(ctxs), f, h)))
        return 0
    try:
        met = _to_tmpfile(both)
    except RuntimeError as e:
        raise RuntimeError(f"{e} [{'; '.join(lib.gx_last_error(c.ctx).decode() for c in ctxs)}]") from None
    return met, (hist[0] if hist else None)


def depth_geometry():
    """(bound, lanes, grid, list_capacity) of the depth pass as the library was built (gx_depth_geometry): the whole depth from which
    a piece is listed, the lanes of a workgroup of k_depth_hist, its most workgroups, the deep list's first capacity."""
    lib = load_library()
    bound, lanes, grid, cap = C.c_uint32(0), C.c_int(0), C.c_int(0), C.c_size_t(0)
    lib.gx_depth_geometry(C.byref(bound), C.byref(lanes), C.byref(grid), C.byref(cap))
    return bound.value, lanes.value, grid.value, cap.value


def _depth_fetch(call, check):
    """Both read-backs (gx_get_depth / gx_depth_group): the size of the deep list first, then everything."""
    n = C.c_size_t(0)
    check(call(None, None, None, None, None, None, 0, C.byref(n)))
    h = DepthHist()
    arr = [np.zeros(DEPTH_BOUND, dtype=np.uint64) for _ in range(3)] + [np.zeros(max(n.value, 1), dtype=np.uint64) for _ in range(2)]
    check(call(C.addressof(h), *[a.ctypes.data for a in arr], n.value, C.byref(n)))
    return Depth(h.rep, bool(h.is_ctrl), h.total, h.excluded, h.zero, h.min_v, h.max_v, arr[0], arr[1], arr[2],
                 [(int(v), int(b)) for v, b in zip(arr[3][:n.value], arr[4][:n.value])])


def _depth_structs(samples):
    """samples: [Depth] -> a gx_depth_hist array (and what keeps its arrays alive)."""
    hs = (DepthHist * max(len(samples), 1))()
    keep = []
    for h, d in zip(hs, samples):
        arr = [np.ascontiguousarray(a, dtype=np.uint64) for a in (d.bases, d.rsum, d.rsq, [p[0] for p in d.deep], [p[1] for p in d.deep])]
        keep.append(arr)
        h.rep, h.is_ctrl, h.total, h.excluded, h.zero, h.min_v, h.max_v = d.rep, int(bool(d.is_ctrl)), d.total, d.excluded, d.zero, d.min_v, d.max_v
        h.bases, h.rsum, h.rsq = (a.ctypes.data for a in arr[:3])
        h.deep_v, h.deep_bases = (a.ctypes.data if a.size else None for a in arr[3:])
        h.n_deep = len(d.deep)
    return hs, keep


def depth_metrics(sample):
    """gx_depth_metrics of one Depth as one DEPTH_METRICS_DTYPE record; host-only, needs no GPU."""
    lib = load_library()
    hs, keep = _depth_structs([sample])
    out = np.zeros(1, dtype=DEPTH_METRICS_DTYPE)
    rc = lib.gx_depth_metrics(C.addressof(hs), out.ctypes.data)
    if rc:
        raise RuntimeError(f"gx_depth_metrics: {rc}")
    return out[0]


def format_depth(samples) -> bytes:
    """--depth's table (gx_format_depth); samples: [Depth]; host-only, needs no GPU."""
    lib = load_library()
    hs, keep = _depth_structs(samples)
    return _to_tmpfile(lambda f: lib.gx_format_depth(f, len(samples), C.addressof(hs)))


def format_depth_metrics(samples) -> bytes:
    """--depth-metrics' table (gx_format_depth_metrics); samples: [Depth]; host-only, needs no GPU."""
    lib = load_library()
    hs, keep = _depth_structs(samples)
    return _to_tmpfile(lambda f: lib.gx_format_depth_metrics(f, len(samples), C.addressof(hs)))


def depth_group(ctxs, sample):
    """Depth of one sample added over the contexts of a run (gx_depth_group)."""
    lib = load_library()
    arr = (C.c_void_p * len(ctxs))(*[c.ctx for c in ctxs])
    return _depth_fetch(lambda *a: lib.gx_depth_group(arr, len(ctxs), int(sample), *a), ctxs[0]._check)


def depth_text(ctxs):
    """(--depth's table, --depth-metrics') over the contexts of a run (gx_write_depth_group)."""
    lib = load_library()
    arr = (C.c_void_p * len(ctxs))(*[c.ctx for c in ctxs])
    return (_to_tmpfile(lambda f: lib.gx_write_depth_group(arr, len(ctxs), f, None)),
            _to_tmpfile(lambda f: lib.gx_write_depth_group(arr, len(ctxs), None, f)))


def subsample_draw(seed, sample, index):
    """The 32-bit draw of event `index` of kept sample `sample` (gx_subsample_draw); host-only, needs no GPU."""
    return int(load_library().gx_subsample_draw(int(seed), int(sample), int(index)))


def subsample_geometry():
    """(lanes, grid, block_events) of the subsample pass as the library was built (gx_subsample_geometry)."""
    lanes, grid, block = C.c_int(0), C.c_int(0), C.c_uint32(0)
    load_library().gx_subsample_geometry(C.byref(lanes), C.byref(grid), C.byref(block))
    return lanes.value, grid.value, block.value


def saturation_thresholds(n_points):
    """--saturation's thresholds for n_points steps (gx_saturation_thresholds): [(j << 32) // n_points]; host-only."""
    out = np.zeros(max(int(n_points), 1), dtype=np.uint64)
    rc = load_library().gx_saturation_thresholds(int(n_points), out.ctypes.data)
    if rc:
        raise RuntimeError(f"gx_saturation_thresholds: {rc}")
    return [int(t) for t in out]


def saturation_overlap(full, sub):
    """(full_recovered, sub_in_full, shared_bp) of two peak lists in get_peaks() order (gx_saturation_overlap); host-only."""
    f, s = np.ascontiguousarray(full, dtype=PEAK_DTYPE), np.ascontiguousarray(sub, dtype=PEAK_DTYPE)
    a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = load_library().gx_saturation_overlap(f.ctypes.data if f.size else None, f.size, s.ctypes.data if s.size else None, s.size,
                                              C.byref(a), C.byref(b), C.byref(c))
    if rc:
        raise RuntimeError(f"gx_saturation_overlap: {rc}")
    return a.value, b.value, c.value


def format_saturation(points, full_recovered, sub_in_full, shared_bp, n_full, full_bp) -> bytes:
    """--saturation's table (gx_format_saturation); points: SAT_POINT_DTYPE records; host-only, needs no GPU."""
    lib = load_library()
    pts = np.ascontiguousarray(points, dtype=SAT_POINT_DTYPE)
    cols = [np.ascontiguousarray(c, dtype=np.uint64) for c in (full_recovered, sub_in_full, shared_bp)]
    return _to_tmpfile(lambda f: lib.gx_format_saturation(f, len(pts), pts.ctypes.data, cols[0].ctypes.data, cols[1].ctypes.data,
                                                          cols[2].ctypes.data, int(n_full), int(full_bp)))


def peaks_supported(a, b, pct):
    """hit[i] (uint8): peak a[i] is supported by a peak of b at `pct` percent of the shorter (gx_peaks_supported); two lists in
    get_peaks() order; host-only."""
    x, y = np.ascontiguousarray(a, dtype=PEAK_DTYPE), np.ascontiguousarray(b, dtype=PEAK_DTYPE)
    hit = np.zeros(max(x.size, 1), dtype=np.uint8)
    rc = load_library().gx_peaks_supported(x.ctypes.data if x.size else None, x.size, y.ctypes.data if y.size else None, y.size, int(pct),
                                           hit.ctypes.data if x.size else None)
    if rc:
        raise RuntimeError(f"gx_peaks_supported: {rc}")
    return hit[:x.size]


def repro_calls(n_rep, n_events=None, n_peaks=None, peak_bp=None, status=None):
    """gx_reproducibility's 3 R + 2 calls in its order, as REPRO_CALL_DTYPE records (the counts where given)."""
    R = int(n_rep)
    out = np.zeros(3 * R + 2, dtype=REPRO_CALL_DTYPE)
    for r in range(R):
        out[r] = (GX_REPRO_ALONE, r, -1, 0, 0, 0, 0)
        for h in range(2):
            out[R + 2 * r + h] = (GX_REPRO_SELF, r, h, 0, 0, 0, 0)
    for h in range(2):
        out[3 * R + h] = (GX_REPRO_POOLED, -1, h, 0, 0, 0, 0)
    for name, col in (("n_events", n_events), ("n_peaks", n_peaks), ("peak_bp", peak_bp), ("status", status)):
        if col is not None:
            out[name] = col
    return out


def reproducibility_figures(run, calls, lists, pct):
    """The figures of --reproducibility (gx_reproducibility_figures) from the run's peaks, the calls (REPRO_CALL_DTYPE, in
    gx_reproducibility's order) and their peak lists: a dict with the REPRO_FIGURES_DTYPE record `fig` and the arrays nt_pair,
    n_self, in_run, run_supported, conservative, optimal; host-only."""
    lib = load_library()
    run = np.ascontiguousarray(run, dtype=PEAK_DTYPE)
    calls = np.ascontiguousarray(calls, dtype=REPRO_CALL_DTYPE)
    R = (len(calls) - 2) // 3
    lists = [np.ascontiguousarray(l, dtype=PEAK_DTYPE) for l in lists]
    ptrs = (C.c_void_p * len(lists))(*[l.ctypes.data if l.size else None for l in lists])
    fig = np.zeros(1, dtype=REPRO_FIGURES_DTYPE)
    pair, n_self = np.zeros(max(R * (R - 1) // 2, 1), dtype=np.uint64), np.zeros(R, dtype=np.uint64)
    in_run, run_sup = np.zeros(len(calls), dtype=np.uint64), np.zeros(len(calls), dtype=np.uint64)
    cons, opt = np.zeros(max(run.size, 1), dtype=np.uint8), np.zeros(max(run.size, 1), dtype=np.uint8)
    rc = lib.gx_reproducibility_figures(run.ctypes.data if run.size else None, run.size, R, calls.ctypes.data, ptrs, int(pct), fig.ctypes.data,
                                        pair.ctypes.data, n_self.ctypes.data, in_run.ctypes.data, run_sup.ctypes.data, cons.ctypes.data,
                                        opt.ctypes.data)
    if rc:
        raise RuntimeError(f"gx_reproducibility_figures: {rc}")
    return dict(fig=fig[0], nt_pair=pair[:R * (R - 1) // 2], n_self=n_self, in_run=in_run, run_supported=run_sup,
                conservative=cons[:run.size], optimal=opt[:run.size])


def repro_label(call):
    """A call's label in the tables and file names (gx_reproducibility_label): t1, t1.pr2, pooled.pr1."""
    c = np.ascontiguousarray(np.asarray(call, dtype=REPRO_CALL_DTYPE).reshape(1))
    buf = C.create_string_buffer(64)
    load_library().gx_reproducibility_label(c.ctypes.data, buf, 64)
    return buf.value.decode()


def format_reproducibility(calls, in_run, run_supported, n_run, run_bp, pct, seed) -> bytes:
    """--reproducibility's call table (gx_format_reproducibility); host-only, needs no GPU."""
    lib = load_library()
    calls = np.ascontiguousarray(calls, dtype=REPRO_CALL_DTYPE)
    a, b = np.ascontiguousarray(in_run, dtype=np.uint64), np.ascontiguousarray(run_supported, dtype=np.uint64)
    return _to_tmpfile(lambda f: lib.gx_format_reproducibility(f, (len(calls) - 2) // 3, calls.ctypes.data, a.ctypes.data, b.ctypes.data,
                                                               int(n_run), int(run_bp), int(pct), int(seed)))


def format_reproducibility_metrics(figures) -> bytes:
    """--reproducibility-metrics' table (gx_format_reproducibility_metrics) of what reproducibility_figures() gave; host-only."""
    lib = load_library()
    fig = np.ascontiguousarray(np.asarray(figures["fig"], dtype=REPRO_FIGURES_DTYPE).reshape(1))
    pair = np.ascontiguousarray(np.append(figures["nt_pair"], 0), dtype=np.uint64)
    n_self = np.ascontiguousarray(figures["n_self"], dtype=np.uint64)
    return _to_tmpfile(lambda f: lib.gx_format_reproducibility_metrics(f, fig.ctypes.data, pair.ctypes.data, n_self.ctypes.data))


def format_narrowpeak(peaks, names, first_index=0) -> bytes:
    """-o's lines for a peak list (gx_format_narrowpeak); peak i is named peak_<first_index + i>; host-only."""
    lib = load_library()
    pk = np.ascontiguousarray(peaks, dtype=PEAK_DTYPE)
    arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
    return _to_tmpfile(lambda f: lib.gx_format_narrowpeak(pk.ctypes.data if pk.size else None, pk.size, arr, int(first_index), f))


def fp_geometry():
    """(n_classes, sub_log, lanes, grid) of k_fp_hist as the library was built (gx_fp_geometry): the value classes, log2 of the
    classes per octave, the lanes of a workgroup, the most workgroups of a launch by default."""
    lib = load_library()
    v = [C.c_int(0) for _ in range(4)]
    lib.gx_fp_geometry(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def fp_class(x):
    return int(load_library().gx_fp_class(int(x)))


def fp_class_lo(k):
    return int(load_library().gx_fp_class_lo(int(k)))


def fp_class_hi(k):
    return int(load_library().gx_fp_class_hi(int(k)))


def _fp_arrays(count, total):
    c = np.ascontiguousarray(count, dtype=np.uint64)
    t = np.ascontiguousarray(total, dtype=np.uint64)
    if c.ndim != 2 or c.shape[1] != FP_NC or t.shape != c.shape:
        raise ValueError("count and sum must be [S, FP_NC]")
    return c, t


def _fp_ctrl(ctrl_of, S):
    if ctrl_of is None:
        return None, None
    a = np.ascontiguousarray(ctrl_of, dtype=np.int32)
    if a.shape != (S,):
        raise ValueError("ctrl_of must have one entry per sample")
    return a, a.ctypes.data


def fingerprint_metrics(count, total, ctrl_of=None):
    """The figures of gx_fingerprint_metrics as a FP_METRICS_DTYPE array [S]; count / total: uint64 [S, FP_NC]; host-only."""
    lib = load_library()
    c, t = _fp_arrays(count, total)
    keep, cp = _fp_ctrl(ctrl_of, len(c))
    out = np.zeros(len(c), dtype=FP_METRICS_DTYPE)
    rc = lib.gx_fingerprint_metrics(len(c), c.ctypes.data, t.ctypes.data, cp, out.ctypes.data)
    if rc:
        raise RuntimeError(f"gx_fingerprint_metrics: {rc}")
    return out


def format_fingerprint(sample_names, count, total) -> bytes:
    """--fingerprint's curve table (gx_format_fingerprint); host-only, needs no GPU."""
    lib = load_library()
    c, t = _fp_arrays(count, total)
    names = _c_names(list(sample_names))
    return _to_tmpfile(lambda f: lib.gx_format_fingerprint(f, len(c), names, c.ctypes.data, t.ctypes.data))


def format_fingerprint_metrics(sample_names, count, total, ctrl_of=None) -> bytes:
    """--fingerprint-metrics' table (gx_format_fingerprint_metrics); host-only, needs no GPU."""
    lib = load_library()
    c, t = _fp_arrays(count, total)
    keep, cp = _fp_ctrl(ctrl_of, len(c))
    names = _c_names(list(sample_names))
    return _to_tmpfile(lambda f: lib.gx_format_fingerprint_metrics(f, len(c), names, c.ctypes.data, t.ctypes.data, cp))


def rccl_unique_id() -> bytes:
    lib = load_library()
    buf = C.create_string_buffer(128)
    rc = lib.gx_rccl_unique_id(buf, 128)
    if rc:
        raise RuntimeError(f"gx_rccl_unique_id: {rc}")
    return buf.raw


def selftest_host(what, a, b):
    """calcPval (what 1) / multPval's tail (what 3) by the host build of the library's routines: returns
    (float results, the doubles they were rounded from).  Needs no GPU."""
    import numpy as np
    lib = load_library()
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    out = np.zeros_like(a)
    dbl = np.zeros(a.size, dtype=np.float64)
    rc = lib.gx_selftest_host(int(what), a.ctypes.data, b.ctypes.data, out.ctypes.data, dbl.ctypes.data, a.size)
    if rc:
        raise RuntimeError(f"gx_selftest_host: {rc}")
    return out, dbl


class Genrich:
    """One run of the hot path on one GPU: the call order of runProgram (Genrich.c:5386-5607)."""

    def __init__(self, params: GxParams):
        self.lib = load_library()
        self.ctx = C.c_void_p()
        rc = self.lib.gx_create(C.byref(self.ctx), C.byref(params))
        if rc != 0:
            msg = self.lib.gx_last_error(self.ctx).decode() if self.ctx else ""
            raise RuntimeError(f"gx_create failed ({rc}): {self.lib.gx_strerror(rc).decode()} {msg}")
        self._keep = []
        self.n_peaks = 0

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(f"genrich_amd error {rc}: {self.lib.gx_strerror(rc).decode()} "
                               f"[{self.lib.gx_last_error(self.ctx).decode()}]")

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.gx_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_chroms(self, lens, skip=None, beds=None):
        n = len(lens)
        self.n_chrom = n
        lens_a = np.ascontiguousarray(lens, dtype=np.uint32)
        skip_a = np.ascontiguousarray(skip if skip is not None else np.zeros(n), dtype=np.uint8)
        bed_ptrs = (C.POINTER(C.c_uint32) * n)()
        bed_len = np.zeros(n, dtype=np.int32)
        keep = []
        if beds is not None:
            for i, b in enumerate(beds):
                arr = np.ascontiguousarray(b, dtype=np.uint32).ravel()
                keep.append(arr)
                bed_len[i] = arr.size
                bed_ptrs[i] = arr.ctypes.data_as(C.POINTER(C.c_uint32))
        self._keep.append((lens_a, skip_a, keep, bed_len, bed_ptrs))
        self._check(self.lib.gx_set_chroms(
            self.ctx, n, lens_a.ctypes.data, skip_a.ctypes.data,
            C.cast(bed_ptrs, C.c_void_p) if beds is not None else None,
            bed_len.ctypes.data if beds is not None else None))

    def reset(self):
        self._check(self.lib.gx_reset(self.ctx))
        self._n_treat = 0

    def expect_fractional(self, on=True):
        """Hint: the run may hold fractional weights (Genrich's -s): pair records with a weight class from the first sample on."""
        self._check(self.lib.gx_expect_fractional(self.ctx, int(bool(on))))

    def set_knob(self, name, value=1):
        """A test / measurement switch (GX_NO_LOOSE, ...) on the live context; the environment is read once, in gx_create."""
        self._check(self.lib.gx_set_knob(self.ctx, name.encode(), str(int(value)).encode()))

    def window_net(self, chrom, pos0, n):
        """The open sample's difference array on [pos0, pos0 + n) of a chromosome (1/120 units), from the events pushed so far."""
        out = np.zeros(n, dtype=np.int64)
        self._check(self.lib.gx_window_net(self.ctx, chrom, pos0, n, out.ctypes.data))
        return out

    def dups_first(self, keys, multi):
        """The raw owner words (uint32 [n]) of gx_dups_first for keys (uint32 [n, 4]) and multi (uint8 [n]): the index of the
        first record with record i's key, with DUP_CONTESTED set when a record with that key has multi != 0."""
        k = _dup_keys(keys)
        m = np.ascontiguousarray(multi, dtype=np.uint8)
        if m.shape != (len(k),):
            raise ValueError("multi: one flag per key")
        owner = np.zeros(len(k), dtype=np.uint32)
        self._check(self.lib.gx_dups_first(self.ctx, k.ctypes.data if len(k) else None, m.ctypes.data if len(k) else None, len(k),
                                           owner.ctypes.data if len(k) else None))
        return owner

    def set_keep_pileups(self, keep):
        """keep=False: the pileup floats of the p-value intervals (only the -f / -k emitters read them)
        are not materialised."""
        self._check(self.lib.gx_set_keep_pileups(self.ctx, int(bool(keep))))

    def set_owned(self, owned):
        a = np.ascontiguousarray(owned, dtype=np.uint8)
        self._check(self.lib.gx_set_owned(self.ctx, a.ctypes.data))

    def set_collectives(self, rank, world, allreduce):
        """Every exchange of the library through ONE host callback: an all-reduce (sum) of int64 words."""
        self._cb = ALLREDUCE_FN(allreduce)   # (kept alive with the object: the library calls it later)
        self._check(self.lib.gx_set_collectives(self.ctx, rank, world, self._cb, None))

    def set_rccl(self, rank, world, unique_id: bytes):
        """The library's own RCCL communicator (collective over all ranks); unique_id = rccl_unique_id()
        of one rank, handed to the others by the host program."""
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._check(self.lib.gx_set_rccl(self.ctx, int(rank), int(world), buf))

    def sample_begin(self, is_ctrl, save=None):
        sp = None
        if save is not None:
            sa = np.ascontiguousarray(save, dtype=np.uint8)
            self._keep.append(sa)
            sp = sa.ctypes.data
        self._check(self.lib.gx_sample_begin(self.ctx, int(is_ctrl), sp))
        if not is_ctrl:
            self._n_treat = getattr(self, "_n_treat", 0) + 1   # (reproducibility() sizes its output by it)

    def push_events(self, ev):
        ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
        self._check(self.lib.gx_push_events(self.ctx, ev.ctypes.data, len(ev)))

    def push_events_ptr(self, host_ptr, n, pinned=False):
        """gx_push_events on a raw host pointer; pinned=True: page-locked memory that stays untouched until
        sample_end (gx_push_events_pinned: uploaded in place)."""
        f = self.lib.gx_push_events_pinned if pinned else self.lib.gx_push_events
        self._check(f(self.ctx, C.c_void_p(host_ptr), int(n)))

    def push_events_device(self, dev_ptr: int, n: int):
        """Events already resident in HBM (e.g. a torch tensor's data_ptr())."""
        self._check(self.lib.gx_push_events_device(self.ctx, C.c_void_p(dev_ptr), n))

    def push_events_packed(self, ev8, where=0, n=None):
        """8-byte events (gx_event8: pack_events): a numpy array of EVENT8_DTYPE in host memory (where=0), or a raw pointer
        with n -- pinned host memory (where=1) or device memory (where=2)."""
        if isinstance(ev8, np.ndarray):
            ev8 = np.ascontiguousarray(ev8, dtype=EVENT8_DTYPE)
            self._check(self.lib.gx_push_events_packed(self.ctx, ev8.ctypes.data, len(ev8), 0))
        else:
            self._check(self.lib.gx_push_events_packed(self.ctx, C.c_void_p(int(ev8)), int(n), int(where)))

    def sample_end(self):
        frag, lam, fac = C.c_double(0), C.c_float(0), C.c_float(0)
        self._check(self.lib.gx_sample_end(self.ctx, C.byref(frag), C.byref(lam), C.byref(fac)))
        return frag.value, lam.value, fac.value

    def sample_no_control(self):
        lam = C.c_float(0)
        self._check(self.lib.gx_sample_no_control(self.ctx, C.byref(lam)))
        return lam.value

    def pvalues(self):
        self._check(self.lib.gx_pvalues(self.ctx))

    def find_peaks(self):
        n, g, bp = C.c_size_t(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.gx_find_peaks(self.ctx, C.byref(n), C.byref(g), C.byref(bp)))
        self.n_peaks, self.genome_len, self.peak_bp = n.value, g.value, bp.value
        return n.value, g.value, bp.value

    def get_peaks(self):
        out = np.zeros(self.n_peaks, dtype=PEAK_DTYPE)
        if self.n_peaks:
            self._check(self.lib.gx_get_peaks(self.ctx, out.ctypes.data, self.n_peaks))
        return out

    def get_intervals(self, which, chrom, piles=True):
        """(ends, {"expt", "ctrl", "p", "q"}) of one chromosome; piles=False leaves the pileup
        columns out (the only choice after set_keep_pileups(False))."""
        n = C.c_size_t(0)
        self._check(self.lib.gx_interval_count(self.ctx, int(which), int(chrom), C.byref(n)))
        n = n.value
        end = np.zeros(n, dtype=np.uint32)
        cols = {k: np.zeros(n, dtype=np.float32) for k in ("expt", "ctrl", "p", "q")}
        if n:
            self._check(self.lib.gx_get_intervals(
                self.ctx, int(which), int(chrom), n, end.ctypes.data,
                *[cols[k].ctypes.data if piles or k in ("p", "q") else None for k in ("expt", "ctrl", "p", "q")]))
        return end, cols

    # -- text emitters (gx_emit.cpp) ----------------------------------------------------
    def _names(self, names):
        arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
        self._keep.append(arr)
        return C.cast(arr, C.c_void_p)

    def write_narrowpeak(self, names, path):
        self._check(self.lib.gx_write_narrowpeak_path(self.ctx, self._names(names), path.encode()))

    def write_pile(self, rep, names, expt_name, ctrl_name, path, append=False):
        self._check(self.lib.gx_write_pile_path(
            self.ctx, rep, self._names(names), len(names), expt_name.encode(),
            ctrl_name.encode() if ctrl_name else None, path.encode(), int(append)))

    def write_log(self, n_rep, names, qval_opt, peaks_opt, thr, path):
        self._check(self.lib.gx_write_log_path(self.ctx, n_rep, self._names(names), len(names), int(qval_opt),
                                               int(peaks_opt), float(thr), path.encode()))

    def selftest(self, what, a, b=None):
        a = np.ascontiguousarray(a, dtype=np.float32)
        out = np.zeros_like(a)
        bp = None
        if b is not None:
            b = np.ascontiguousarray(b, dtype=np.float32)
            bp = b.ctypes.data
        self._check(self.lib.gx_selftest(self.ctx, int(what), a.ctypes.data, bp, out.ctypes.data, a.size))
        return out

    def selftest2(self, what, a, b):
        """selftest plus the doubles before rounding and the number of results the host re-evaluated."""
        a = np.ascontiguousarray(a, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        out = np.zeros_like(a)
        dbl = np.zeros(a.size, dtype=np.float64)
        nr = C.c_size_t(0)
        self._check(self.lib.gx_selftest2(self.ctx, int(what), a.ctypes.data, b.ctypes.data, out.ctypes.data,
                                          dbl.ctypes.data, a.size, C.byref(nr)))
        return out, dbl, nr.value

    def interval_total(self, which=GX_IV_FINAL):
        n = C.c_size_t(0)
        self._check(self.lib.gx_total_intervals(self.ctx, int(which), C.byref(n)))
        return n.value

    def path_info(self):
        """Which device path the last calls took: GX_PATH_* bits (1 fused tile stage, 2 loose-slot sweep, 4 fell back, 8 page tables grew,
        16 pair records, 32 dense BH all-reduce, 64 range BH exchange, 128 fractional pair records, 256 pileup floats written, 512 8-byte
        events read in place, 1024 the control merge scored its intervals, 2048 BH's histogram from the pileup sums, 8192 q looked up
        where it is read, 16384 the loose slots swept with bits written late, 32768 -q on the loose slots, 65536 intervals kept for counting, 131072 counted in a region set,
        262144 pileups summed over coverage bins, 524288 pileups summed around anchors, 1048576 the Gram kernels ran,
        2097152 the fingerprint kernel ran, 4194304 the rank kernel ran, 8388608 the complexity kernels ran, 16777216 the subsample kernels ran, 268435456 the split kernel ran, 33554432 the depth kernel ran, 67108864 the interval-length kernel ran, 134217728 the cross-correlation kernels ran,
        536870912 the sweep's run pass ran beside the sample's closing scan)."""
        f = C.c_uint(0)
        self._check(self.lib.gx_path_info(self.ctx, C.byref(f)))
        return f.value

    # -- counting in peaks (no Genrich counterpart; include/genrich_amd.h, gx_count_in_peaks) -------------------------
    def set_count_in_peaks(self, on=True):
        """Keep every sample's intervals for gx_count_in_peaks (only while idle: after creation / reset, before a sample).
        Device buffers pushed by pointer must then stay valid until the run's last count_in_peaks."""
        self._check(self.lib.gx_set_count_in_peaks(self.ctx, int(bool(on))))

    def count_in_peaks(self):
        """Count every kept sample's intervals in the peaks of the last find_peaks; returns the number of samples."""
        n = C.c_int(0)
        self._check(self.lib.gx_count_in_peaks(self.ctx, C.byref(n)))
        return n.value

    def peak_counts(self, sample):
        """PeakCounts(count int64[n_peaks], total, in_peaks, rep, is_ctrl) of one sample of the last count_in_peaks."""
        cnt = np.zeros(self.n_peaks, dtype=np.int64)
        rep, ctrl, tot, inp = C.c_int(0), C.c_int(0), C.c_int64(0), C.c_int64(0)
        self._check(self.lib.gx_get_peak_counts(self.ctx, int(sample), C.byref(rep), C.byref(ctrl), cnt.ctypes.data if cnt.size else None,
                                                cnt.size, C.byref(tot), C.byref(inp)))
        return PeakCounts(cnt, tot.value, inp.value, rep.value, bool(ctrl.value))

    def write_counts(self, names, sample_names, path):
        """--counts' text (gx_write_counts) of this context."""
        self._check(self.lib.gx_write_counts_path(self.ctx, self._names(names), len(sample_names), self._names(sample_names),
                                                  path.encode()))

    # -- each sample's signal inside the peaks (include/genrich_amd.h, gx_peak_signal) -----------------------------------
    def peak_signal(self):
        """Every kept sample's depth inside the peaks of the last find_peaks (gx_peak_signal); needs set_count_in_peaks(True).
        Returns the number of samples."""
        n = C.c_int(0)
        self._check(self.lib.gx_peak_signal(self.ctx, C.byref(n)))
        return n.value

    def peak_signal_of(self, sample):
        """PeakSignal of one sample of the last peak_signal()."""
        k = self.n_peaks
        a, m, t = (np.zeros(k, dtype=np.int64) for _ in range(3))
        s, c = (np.zeros(k, dtype=np.uint32) for _ in range(2))
        rep, ctrl = C.c_int(0), C.c_int(0)
        self._check(self.lib.gx_get_peak_signal(self.ctx, int(sample), C.byref(rep), C.byref(ctrl), *[x.ctypes.data if k else None for x in (a, m, s, c, t)], k))
        return PeakSignal(a, m, s, c, t, rep.value, bool(ctrl.value))

    def peak_signal_events(self, events, peaks, summit_off=None, grid=0):
        """PeakSignal of host events (EVENT_DTYPE) taken as one sample over this context's chromosome table, in the peaks given
        (REGION_DTYPE or rows of (chrom, start, end): sorted, disjoint), by the same kernels (gx_peak_signal_events);
        summit_off[k]: the base of peak k that at_summit reads (None: base 0); grid = 0: the library's geometry."""
        ev = np.ascontiguousarray(events, dtype=EVENT_DTYPE)
        reg = _regions(peaks)
        k = int(reg.size)
        so = None if summit_off is None else np.ascontiguousarray(summit_off, dtype=np.uint32)
        assert so is None or so.size == k
        a, m, t = (np.zeros(k, dtype=np.int64) for _ in range(3))
        s, c = (np.zeros(k, dtype=np.uint32) for _ in range(2))
        self._check(self.lib.gx_peak_signal_events(self.ctx, ev.ctypes.data if ev.size else None, ev.size, reg.ctypes.data if k else None, k,
                                                   so.ctypes.data if so is not None and k else None, int(grid),
                                                   *[x.ctypes.data if k else None for x in (a, m, s, c, t)]))
        return PeakSignal(a, m, s, c, t, 0, False)

    def peak_signal_text(self, names) -> bytes:
        """--peak-signal's text (gx_write_peak_signal) of this context; runs the pass."""
        cn = self._names(names)
        return _to_tmpfile(lambda f: self.lib.gx_write_peak_signal(self.ctx, cn, f))

    # -- the summits of the pooled treatment depth inside the peaks (include/genrich_amd.h, gx_peak_summits) ---------------
    def peak_summits(self, prominence_pct=25, height_pct=50):
        """The summits (SUMMIT_DTYPE, ascending in (peak, pos)) of the kept treatments' pooled depth inside the peaks of the
        last find_peaks (gx_peak_summits); needs set_count_in_peaks(True)."""
        n = C.c_size_t(0)
        self._check(self.lib.gx_peak_summits(self.ctx, int(prominence_pct), int(height_pct), C.byref(n)))
        out = np.zeros(n.value, dtype=SUMMIT_DTYPE)
        self._check(self.lib.gx_get_peak_summits(self.ctx, out.ctypes.data if n.value else None, n.value))
        return out

    def peak_summits_events(self, events, peaks, prominence_pct=25, height_pct=50, grid=0, run_cap=0, list_cap=0):
        """The summits of host events (EVENT_DTYPE) taken as one sample over this context's chromosome table, in the peaks
        given (REGION_DTYPE or rows of (chrom, start, end): sorted, disjoint), by the same kernels (gx_peak_summits_events);
        grid, run_cap, list_cap = 0: the library's."""
        ev = np.ascontiguousarray(events, dtype=EVENT_DTYPE)
        reg = _regions(peaks)
        k = int(reg.size)
        out = np.zeros(max(4096, 4 * k), dtype=SUMMIT_DTYPE)
        for _ in range(2):
            n = C.c_size_t(0)
            self._check(self.lib.gx_peak_summits_events(self.ctx, ev.ctypes.data if ev.size else None, ev.size, reg.ctypes.data if k else None, k,
                                                        int(prominence_pct), int(height_pct), int(grid), int(run_cap), int(list_cap),
                                                        out.ctypes.data, out.size, C.byref(n)))
            if n.value <= out.size:
                break
            out = np.zeros(n.value, dtype=SUMMIT_DTYPE)
        return out[:n.value].copy()

    def peak_summits_last(self):
        """(how often the last summit pass ran again for a full list, the peaks its second launch took) -- gx_peak_summits_last."""
        r, b = C.c_uint(0), C.c_uint(0)
        self._check(self.lib.gx_peak_summits_last(self.ctx, C.byref(r), C.byref(b)))
        return r.value, b.value

    def summits_text(self, names, prominence_pct=25, height_pct=50) -> bytes:
        """--summits' text (gx_write_summits) of this context; runs the pass."""
        cn = self._names(names)
        return _to_tmpfile(lambda f: self.lib.gx_write_summits(self.ctx, cn, int(prominence_pct), int(height_pct), f))

    # -- counting in a given region set (include/genrich_amd.h, gx_count_in_regions) ----------------------------------
    def count_in_regions(self, regions):
        """Count every sample closed so far in `regions` (REGION_DTYPE, or rows of (chrom, start, end)), which may overlap and
        come in any order; needs set_count_in_peaks(True), no peaks.  Returns the number of samples."""
        reg = np.asarray(regions)
        if reg.dtype != REGION_DTYPE:
            rows = np.asarray(regions, dtype=np.int64).reshape(-1, 3)
            reg = np.zeros(len(rows), dtype=REGION_DTYPE)
            reg["chrom"], reg["start"], reg["end"] = rows[:, 0], rows[:, 1], rows[:, 2]
        reg = np.ascontiguousarray(reg)
        n = C.c_int(0)
        self._check(self.lib.gx_count_in_regions(self.ctx, reg.ctypes.data if reg.size else None, reg.size, C.byref(n)))
        self._n_regions = int(reg.size)
        return n.value

    def region_counts(self, sample):
        """RegionCounts(count int64[n_regions], total, in_regions, rep, is_ctrl) of one sample of the last count_in_regions."""
        cnt = np.zeros(getattr(self, "_n_regions", 0), dtype=np.int64)
        rep, ctrl, tot, inr = C.c_int(0), C.c_int(0), C.c_int64(0), C.c_int64(0)
        self._check(self.lib.gx_get_region_counts(self.ctx, int(sample), C.byref(rep), C.byref(ctrl), cnt.ctypes.data if cnt.size else None,
                                                  cnt.size, C.byref(tot), C.byref(inr)))
        return RegionCounts(cnt, tot.value, inr.value, rep.value, bool(ctrl.value))

    def write_region_counts(self, names, regions, region_names, sample_names, path):
        """--region-counts' text (gx_write_region_counts) of this context; region_names: a list with None for region_N, or None."""
        reg = np.ascontiguousarray(np.asarray(regions, dtype=REGION_DTYPE))
        rn = None
        if region_names is not None:
            rn = (C.c_char_p * max(1, len(region_names)))(*[None if x is None else x.encode() for x in region_names])
        self._check(self.lib.gx_write_region_counts_path(self.ctx, self._names(names), reg.ctypes.data if reg.size else None, rn, reg.size,
                                                         len(sample_names), self._names(sample_names), path.encode()))

    # -- binned coverage tracks (include/genrich_amd.h, gx_set_coverage_bins) ------------------------------------------
    def set_coverage_bins(self, bin_size):
        """Sum every closed sample's pileup over bins of bin_size bases (0: off); only while idle, after set_chroms."""
        self._check(self.lib.gx_set_coverage_bins(self.ctx, int(bin_size)))

    def coverage_samples(self):
        n = C.c_int(0)
        self._check(self.lib.gx_coverage_samples(self.ctx, C.byref(n)))
        return n.value

    def coverage_bin_count(self, chrom):
        n = C.c_size_t(0)
        self._check(self.lib.gx_coverage_bin_count(self.ctx, int(chrom), C.byref(n)))
        return n.value

    def coverage(self, sample, chrom):
        """Coverage(sum120 int64[n_bins], rep, is_ctrl) of one closed sample on one chromosome."""
        out = np.zeros(self.coverage_bin_count(chrom), dtype=np.int64)
        rep, ctrl = C.c_int(0), C.c_int(0)
        self._check(self.lib.gx_get_coverage(self.ctx, int(sample), int(chrom), C.byref(rep), C.byref(ctrl),
                                             out.ctypes.data if out.size else None, out.size))
        return Coverage(out, rep.value, bool(ctrl.value))

    def write_coverage(self, sample, names, path, scale=1.0):
        """--coverage's bedGraph (gx_write_coverage) of one sample of this context."""
        self._check(self.lib.gx_write_coverage_path(self.ctx, int(sample), self._names(names), len(names), float(scale), path.encode()))

    # -- depth distribution of the samples' pileups (include/genrich_amd.h, gx_set_depth_hist) -------------------------------
    def set_depth_hist(self, on=True):
        """Take the per-base depth distribution of every closed sample's pileup; only while idle, after set_chroms."""
        self._check(self.lib.gx_set_depth_hist(self.ctx, int(bool(on))))

    def depth_samples(self):
        n = C.c_int(0)
        self._check(self.lib.gx_depth_samples(self.ctx, C.byref(n)))
        return n.value

    def depth(self, sample):
        """Depth of one closed sample of this context (gx_get_depth)."""
        return _depth_fetch(lambda *a: self.lib.gx_get_depth(self.ctx, int(sample), *a), self._check)

    def depth_last(self):
        """(list capacity, reruns) of the last depth pass of this context (gx_depth_last)."""
        c, r = C.c_size_t(0), C.c_int(0)
        self._check(self.lib.gx_depth_last(self.ctx, C.byref(c), C.byref(r)))
        return c.value, r.value

    # -- correlation of the samples' bins (include/genrich_amd.h, gx_coverage_gram) --------------------------------------
    def coverage_gram(self):
        """(n, n_zero, sum, gram) of the samples closed since the last reset: Python ints, sum an object array [S], gram [S, S]."""
        S = self.coverage_samples()
        s, g = _sums128(S)
        ns, n, nz = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.gx_coverage_gram(self.ctx, C.byref(ns), C.byref(n), C.byref(nz), s.ctypes.data, g.ctypes.data, max(S, 1)))
        return n.value, nz.value, _join128(s[:ns.value]), _join128(g[:ns.value, :ns.value])

    def gram_u64(self, rows, grid=0):
        """(n_zero, sum, gram) of the rows (uint64 [n_rows, n], every value < 2^51) by the same kernels (gx_gram_u64); grid = 0:
        the library's geometry, else that many workgroups along the bin axis."""
        r, ptr = _u64_rows(rows)
        n_rows, n = r.shape
        s, g = _sums128(n_rows)
        nz = C.c_uint64(0)
        self._check(self.lib.gx_gram_u64(self.ctx, ptr, n_rows, n, int(grid), C.byref(nz), s.ctypes.data,
                                         g.ctypes.data))
        return nz.value, _join128(s[:n_rows]), _join128(g[:n_rows, :n_rows])

    # -- library complexity of the samples' intervals (include/genrich_amd.h, gx_complexity) -----------------------------
    def complexity(self):
        """N, D and the duplication histogram of every sample closed so far (gx_complexity); needs set_count_in_peaks(True), no
        peaks.  Returns the number of samples."""
        n = C.c_int(0)
        self._check(self.lib.gx_complexity(self.ctx, C.byref(n)))
        return n.value

    def get_complexity(self, sample):
        """Complexity(n_obs, n_distinct, pairs, rep, is_ctrl) of one sample of the last complexity()."""
        n = C.c_size_t(0)
        self._check(self.lib.gx_get_complexity(self.ctx, int(sample), None, None, None, None, None, None, 0, C.byref(n)))
        m, k = np.zeros(max(n.value, 1), dtype=np.uint64), np.zeros(max(n.value, 1), dtype=np.uint64)
        rep, ctrl, N, D = C.c_int(0), C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.gx_get_complexity(self.ctx, int(sample), C.byref(rep), C.byref(ctrl), C.byref(N), C.byref(D), m.ctypes.data,
                                               k.ctypes.data, n.value, C.byref(n)))
        return Complexity(N.value, D.value, [(int(a), int(b)) for a, b in zip(m[:n.value], k[:n.value])], rep.value, bool(ctrl.value))

    def complexity_events(self, events, grid=0, cap_log=0):
        """(N, D, pairs) of host events (EVENT_DTYPE) taken as one sample over this context's chromosome table, by the same kernels
        (gx_complexity_events); grid = 0 / cap_log = 0: the library's geometry and capacity."""
        ev = np.ascontiguousarray(events, dtype=EVENT_DTYPE)
        N, D, n = C.c_uint64(0), C.c_uint64(0), C.c_size_t(0)
        cap = int(ev.size) + 1   # (at most one class per event)
        m, k = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
        self._check(self.lib.gx_complexity_events(self.ctx, ev.ctypes.data if ev.size else None, ev.size, int(grid), int(cap_log), C.byref(N),
                                                  C.byref(D), m.ctypes.data, k.ctypes.data, cap, C.byref(n)))
        return N.value, D.value, [(int(a), int(b)) for a, b in zip(m[:n.value], k[:n.value])]

    def complexity_last(self):
        """The table capacity the last complexity pass of this context used (gx_complexity_last; 0: none yet)."""
        c = C.c_size_t(0)
        self._check(self.lib.gx_complexity_last(self.ctx, C.byref(c)))
        return c.value

    # -- strand cross-correlation of the samples' 5' ends (include/genrich_amd.h, gx_set_xcor) ------------------------------
    def set_xcor(self, lo=-100, hi=600):
        """Keep two strand bit vectors per open sample and count, at sample_end, the tag pairs at every shift lo .. hi (gx_set_xcor);
        hi < lo: off.  Only while idle, after set_chroms."""
        self._check(self.lib.gx_set_xcor(self.ctx, int(lo), int(hi)))

    def push_tags(self, tags):
        """Tags (TAG_DTYPE) of the open sample, any order, any split (gx_push_tags)."""
        t = np.ascontiguousarray(tags, dtype=TAG_DTYPE)
        self._check(self.lib.gx_push_tags(self.ctx, t.ctypes.data if t.size else None, t.size))

    def xcor_samples(self):
        n = C.c_int(0)
        self._check(self.lib.gx_xcor_samples(self.ctx, C.byref(n)))
        return n.value

    def xcor(self, sample):
        """Xcor of one closed sample of this context (gx_get_xcor)."""
        return _xcor_result(lambda *a: self._check(self.lib.gx_get_xcor(self.ctx, int(sample), *a)), 2 * XCOR_MAX_SHIFT + 1)

    def xcor_tags(self, lens, tags, lo=-100, hi=600, grid=0, tile_words=0):
        """Xcor of host tags (TAG_DTYPE) over a chromosome table of their own, by the two kernels alone (gx_xcor_tags); grid = 0 /
        tile_words = 0: the library's geometry."""
        t = np.ascontiguousarray(tags, dtype=TAG_DTYPE)
        ln = np.ascontiguousarray(lens, dtype=np.uint32)
        n = max(int(hi) - int(lo) + 1, 1)
        n11 = np.zeros(n, dtype=np.uint64)
        N, nP, nM, rej = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.gx_xcor_tags(self.ctx, ln.ctypes.data, ln.size, t.ctypes.data if t.size else None, t.size, int(lo), int(hi), int(grid),
                                          int(tile_words), C.byref(N), C.byref(nP), C.byref(nM), C.byref(rej), n11.ctypes.data, n))
        return Xcor(N.value, nP.value, nM.value, rej.value, int(lo), int(hi), [int(x) for x in n11])

    # -- the reference sequence, GC bias and GC content (include/genrich_amd.h, gx_set_genome) ------------------------------
    def set_genome(self, on=True):
        """Allocate and clear the two bit vectors for this context's chromosome table, or free them (gx_set_genome)."""
        self._check(self.lib.gx_set_genome(self.ctx, int(bool(on))))

    def push_sequence(self, chrom, first_base, bases):
        """Plain sequence bytes of chromosome `chrom` from base `first_base` (a multiple of 64) on (gx_push_sequence)."""
        b = bytes(bases)
        self._check(self.lib.gx_push_sequence(self.ctx, int(chrom), int(first_base), b if b else None, len(b)))

    def genome_info(self):
        """(bases pushed, gc bits, acgt bits) of this context's genome (gx_genome_info)."""
        p, g, a = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.gx_genome_info(self.ctx, C.byref(p), C.byref(g), C.byref(a)))
        return p.value, g.value, a.value

    def gc_content(self, regions):
        """(gc, acgt) uint64 arrays for regions (REGION_DTYPE), by rank differences (gx_gc_content)."""
        reg = np.ascontiguousarray(regions, dtype=REGION_DTYPE)
        g, a = np.zeros(max(reg.size, 1), dtype=np.uint64), np.zeros(max(reg.size, 1), dtype=np.uint64)
        self._check(self.lib.gx_gc_content(self.ctx, reg.ctypes.data if reg.size else None, reg.size, g.ctypes.data, a.ctypes.data))
        return g[:reg.size], a[:reg.size]

    def gc_bias(self, window=200):
        """The GC tables of every sample closed so far (gx_gc_bias); needs set_genome() and set_count_in_peaks(True).  Returns the
        number of samples."""
        n = C.c_int(0)
        self._check(self.lib.gx_gc_bias(self.ctx, int(window), C.byref(n)))
        return n.value

    def get_gc_bias(self, sample):
        """GcBias of one sample of the last gc_bias() (gx_get_gc_bias)."""
        return _gc_result(lambda *a: self._check(self.lib.gx_get_gc_bias(self.ctx, int(sample), *a)))

    def gc_bias_events(self, events, window=200, packed=False, grid_expected=0, tile_words=0, flush_words=0, grid_observed=0):
        """GcBias of host events (EVENT_DTYPE; packed: EVENT8 records as pack_events gives them) taken as one sample over this
        context's genome, by the kernels alone (gx_gc_bias_events); 0: the library's geometry."""
        ev = np.ascontiguousarray(events)
        W = int(window)
        k = max(W, 0) + 1
        F, Nn, Nw = (np.zeros(k, dtype=np.uint64) for _ in range(3))
        fu, nu, wu = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.gx_gc_bias_events(self.ctx, ev.ctypes.data if ev.size else None, ev.size, int(bool(packed)), W, int(grid_expected),
                                               int(tile_words), int(flush_words), int(grid_observed), F.ctypes.data, C.byref(fu), Nn.ctypes.data,
                                               Nw.ctypes.data, C.byref(nu), C.byref(wu), k))
        return GcBias(W, F, fu.value, Nn, Nw, nu.value, wu.value)

    # -- the sequence itself and the motif scan (include/genrich_amd.h, gx_set_genome_bases) --------------------------------
    n_motifs = 0
    _n_motif_hits = 0

    def set_genome_bases(self, on=True):
        """The third bit vector: from now on push_sequence keeps the bases themselves (gx_set_genome_bases); after set_genome(),
        before the first push."""
        self._check(self.lib.gx_set_genome_bases(self.ctx, int(bool(on))))

    def get_sequence(self, chrom, start, n):
        """n letters of chromosome `chrom` from base `start` on: ACGT, N for unknown and past the end (gx_get_sequence)."""
        out = C.create_string_buffer(max(int(n), 1))
        self._check(self.lib.gx_get_sequence(self.ctx, int(chrom), int(start), int(n), out))
        return out.raw[:int(n)]

    def set_motifs(self, motifs):
        """The motifs to scan: [(scores int16[L, 4] in column order A C G T, threshold)] (gx_set_motifs); []: none."""
        rec, flat = pack_motifs(motifs)
        self._check(self.lib.gx_set_motifs(self.ctx, rec.ctypes.data if len(rec) else None, len(rec), flat.ctypes.data if len(rec) else None))
        self.n_motifs = len(rec)

    def _motif_counts(self):
        return np.zeros((3, max(self.n_motifs, 1)), dtype=np.uint64)

    def motif_scan_regions(self, regions, grid=0, step_words=0, batch_motifs=0, list_cap=0):
        """(hits MOTIF_HIT_DTYPE sorted by (region, pos, motif, strand), counts uint64[3, motifs]: windows, hits +, hits -) of the
        motifs in `regions` (REGION_DTYPE), by the kernel alone (gx_motif_scan_regions); 0: the library's geometry."""
        reg = np.ascontiguousarray(regions, dtype=REGION_DTYPE)
        cnt = self._motif_counts()
        n = C.c_size_t(0)
        args = (reg.ctypes.data if reg.size else None, reg.size, int(grid), int(step_words), int(batch_motifs), int(list_cap))
        hits = np.empty(1 << 18, dtype=MOTIF_HIT_DTYPE)
        for _ in range(2):   # (once more when there were more hits than the buffer held)
            self._check(self.lib.gx_motif_scan_regions(self.ctx, *args, hits.ctypes.data, hits.size, C.byref(n), cnt[0].ctypes.data, cnt[1].ctypes.data,
                                                       cnt[2].ctypes.data))
            if n.value <= hits.size:
                break
            hits = np.empty(n.value, dtype=MOTIF_HIT_DTYPE)
        return hits[:n.value].copy(), cnt[:, :self.n_motifs]

    def motif_scan_peaks(self):
        """Scan the peaks find_peaks left on this context (gx_motif_scan_peaks); returns the number of hits."""
        n = C.c_size_t(0)
        self._check(self.lib.gx_motif_scan_peaks(self.ctx, C.byref(n)))
        self._n_motif_hits = n.value
        return n.value

    def get_motif_hits(self):
        """The hits of the last motif_scan_peaks(), region = the peak's index (gx_get_motif_hits)."""
        hits = np.zeros(self._n_motif_hits, dtype=MOTIF_HIT_DTYPE)
        self._check(self.lib.gx_get_motif_hits(self.ctx, hits.ctypes.data if hits.size else None, hits.size))
        return hits

    def get_motif_counts(self):
        """uint64[3, motifs] (windows, hits +, hits -) of the last motif_scan_peaks() (gx_get_motif_counts)."""
        cnt = self._motif_counts()
        self._check(self.lib.gx_get_motif_counts(self.ctx, cnt[0].ctypes.data, cnt[1].ctypes.data, cnt[2].ctypes.data, self.n_motifs))
        return cnt[:, :self.n_motifs]

    def motif_last(self):
        """(reruns, batches) of the last motif scan (gx_motif_last)."""
        r, b = C.c_uint32(0), C.c_uint32(0)
        self._check(self.lib.gx_motif_last(self.ctx, C.byref(r), C.byref(b)))
        return r.value, b.value

    def motif_scan_genome(self):
        """uint64[3, motifs] of the count-only pass over every chromosome that takes part (gx_motif_scan_genome)."""
        cnt = self._motif_counts()
        self._check(self.lib.gx_motif_scan_genome(self.ctx, cnt[0].ctypes.data, cnt[1].ctypes.data, cnt[2].ctypes.data, self.n_motifs))
        return cnt[:, :self.n_motifs]

    # -- every k-mer counted (include/genrich_amd.h, gx_kmer_count_regions) --------------------------------------------------
    _kmer_k = 0

    def kmer_count_regions(self, regions, k, grid=0, step_words=0, flush_runs=0):
        """(counts uint64[4^k] in the public order, windows) of the k-mers of `regions` (REGION_DTYPE), by the kernel alone
        (gx_kmer_count_regions); 0: the library's geometry."""
        reg = np.ascontiguousarray(regions, dtype=REGION_DTYPE)
        out = np.zeros(4 ** int(k) if 1 <= int(k) <= KMER_MAX_K else 1, dtype=np.uint64)
        w = C.c_uint64(0)
        self._check(self.lib.gx_kmer_count_regions(self.ctx, reg.ctypes.data if reg.size else None, reg.size, int(k), int(grid), int(step_words),
                                                   int(flush_runs), out.ctypes.data, C.byref(w)))
        return out, w.value

    def kmer_count_peaks(self, k, flank=-1):
        """Count the k-mers of the peaks find_peaks left on this context (gx_kmer_count_peaks): (windows, regions counted)."""
        w, r = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.gx_kmer_count_peaks(self.ctx, int(k), int(flank), C.byref(w), C.byref(r)))
        self._kmer_k = int(k)
        return w.value, r.value

    def get_kmer_counts(self):
        """uint64[4^k] of the last kmer_count_peaks() (gx_get_kmer_counts)."""
        out = np.zeros(4 ** self._kmer_k, dtype=np.uint64)
        self._check(self.lib.gx_get_kmer_counts(self.ctx, out.ctypes.data, out.size))
        return out

    def kmer_count_genome(self, k):
        """(counts uint64[4^k], windows) over every chromosome that takes part (gx_kmer_count_genome)."""
        out = np.zeros(4 ** int(k) if 1 <= int(k) <= KMER_MAX_K else 1, dtype=np.uint64)
        w = C.c_uint64(0)
        self._check(self.lib.gx_kmer_count_genome(self.ctx, int(k), out.ctypes.data, out.size, C.byref(w)))
        return out, w.value

    def kmer_last(self):
        """(path: 0 LDS, 1 HBM; flushes before a workgroup's end) of the last k-mer pass (gx_kmer_last)."""
        p, f = C.c_int(0), C.c_uint32(0)
        self._check(self.lib.gx_kmer_last(self.ctx, C.byref(p), C.byref(f)))
        return p.value, f.value

    def kmer_force_hbm(self, on=True):
        """Every k takes the global-atomic path (gx_kmer_force_hbm): for measurements; no result changes."""
        self._check(self.lib.gx_kmer_force_hbm(self.ctx, 1 if on else 0))

    # -- lengths and chromosome tallies of the samples' intervals (include/genrich_amd.h, gx_interval_stats) --------------
    def interval_stats(self):
        """The lengths and the chromosome tallies of every sample closed so far (gx_interval_stats); needs set_count_in_peaks(True),
        no peaks.  Returns the number of samples."""
        n = C.c_int(0)
        self._check(self.lib.gx_interval_stats(self.ctx, C.byref(n)))
        return n.value

    def get_interval_stats(self, sample):
        """IntervalStats of one sample of the last interval_stats() (gx_get_interval_lengths + gx_get_chrom_stats)."""
        def call(rep, ctrl, L, n, w, cap, nc, ni, wi, cn, cw, cb, ccap):
            self._check(self.lib.gx_get_interval_lengths(self.ctx, int(sample), rep, ctrl, L, n, w, cap, nc, ni, wi))
            if ccap:
                self._check(self.lib.gx_get_chrom_stats(self.ctx, int(sample), cn, cw, cb, ccap))
        return _ivs_result(call, self.n_chrom)

    def interval_stats_events(self, events, grid=0, list_cap=0):
        """IntervalStats of host events (EVENT_DTYPE) taken as one sample over this context's chromosome table, by the same kernel
        (gx_interval_stats_events); grid = 0 / list_cap = 0: the library's geometry and first list capacity."""
        ev = np.ascontiguousarray(events, dtype=EVENT_DTYPE)
        cap = int(ev.size) + 1   # (at most one class per event)
        L, k, w = (np.zeros(cap, dtype=np.uint64) for _ in range(3))
        cn, cw, cb = (np.zeros(self.n_chrom, dtype=np.uint64) for _ in range(3))
        n, ni, wi = C.c_size_t(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.gx_interval_stats_events(self.ctx, ev.ctypes.data if ev.size else None, ev.size, int(grid), int(list_cap), L.ctypes.data,
                                                      k.ctypes.data, w.ctypes.data, cap, C.byref(n), C.byref(ni), C.byref(wi), cn.ctypes.data,
                                                      cw.ctypes.data, cb.ctypes.data, self.n_chrom))
        return IntervalStats([(int(a), int(b), int(c)) for a, b, c in zip(L[:n.value], k[:n.value], w[:n.value])], ni.value, wi.value,
                             [int(x) for x in cn], [int(x) for x in cw], [int(x) for x in cb])

    def interval_stats_last(self):
        """(list capacity, reruns) of the last interval-length pass of this context (gx_interval_stats_last)."""
        c, r = C.c_size_t(0), C.c_int(0)
        self._check(self.lib.gx_interval_stats_last(self.ctx, C.byref(c), C.byref(r)))
        return c.value, r.value

    # -- subsamples of the kept samples and the peak saturation curve (include/genrich_amd.h, gx_saturation) ----------------
    def subsample_events(self, events, seed, sample, threshold, grid=0, packed=False):
        """The events (EVENT_DTYPE; packed: EVENT8 records as pack_events gives them) kept at `threshold` as sample `sample`, by
        the subsample kernels (gx_subsample_events): always EVENT_DTYPE, in order."""
        ev = np.ascontiguousarray(events)
        out = np.zeros(max(int(ev.size), 1), dtype=EVENT_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.gx_subsample_events(self.ctx, ev.ctypes.data if ev.size else None, ev.size, int(bool(packed)), int(seed), int(sample),
                                                 int(threshold), int(grid), out.ctypes.data, ev.size, C.byref(n)))
        return out[:n.value]

    def subsample_kept(self, sample, seed, threshold):
        """Kept sample `sample`'s events kept at `threshold` (gx_subsample_kept), in kept order."""
        n = C.c_size_t(0)
        self._check(self.lib.gx_subsample_kept(self.ctx, int(sample), int(seed), int(threshold), None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=EVENT_DTYPE)
        self._check(self.lib.gx_subsample_kept(self.ctx, int(sample), int(seed), int(threshold), out.ctypes.data, n.value, C.byref(n)))
        return out[:n.value]

    def saturation(self, thresholds, seed=1, flags=0):
        """The peaks called once more per threshold on nested subsamples of the kept samples (gx_saturation), after find_peaks():
        SAT_POINT_DTYPE records, one per threshold."""
        thr = np.ascontiguousarray(thresholds, dtype=np.uint64)
        out = np.zeros(len(thr), dtype=SAT_POINT_DTYPE)
        self._check(self.lib.gx_saturation(self.ctx, thr.ctypes.data, len(thr), int(seed), int(flags), out.ctypes.data))
        self._sat_peaks = [int(p) for p in out["n_peaks"]]
        return out

    def saturation_peaks(self, point):
        """The peaks of one point of the last saturation() (gx_get_saturation_peaks), PEAK_DTYPE."""
        n = self._sat_peaks[point]
        out = np.zeros(n, dtype=PEAK_DTYPE)
        self._check(self.lib.gx_get_saturation_peaks(self.ctx, int(point), out.ctypes.data if n else None, n))
        return out

    def saturation_text(self) -> bytes:
        """--saturation's table of the last saturation() against this run's peaks (gx_write_saturation)."""
        return _to_tmpfile(lambda f: self.lib.gx_write_saturation(self.ctx, f))

    # -- both halves of a sample and the reproducibility calls (include/genrich_amd.h, gx_reproducibility) -----------------
    def subsample_split_events(self, events, seed, sample, threshold, grid=0, packed=False):
        """(out, n_a): the events as sample `sample` split at `threshold` by the split kernel (gx_subsample_split_events): half A
        in out[:n_a], half B behind it, both in order; always EVENT_DTYPE."""
        ev = np.ascontiguousarray(events)
        out = np.zeros(max(int(ev.size), 1), dtype=EVENT_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.gx_subsample_split_events(self.ctx, ev.ctypes.data if ev.size else None, ev.size, int(bool(packed)), int(seed),
                                                       int(sample), int(threshold), int(grid), out.ctypes.data, ev.size, C.byref(n)))
        return out[:ev.size], n.value

    def subsample_split_kept(self, sample, seed, threshold, n):
        """(out, n_a) of kept sample `sample` of `n` events (gx_subsample_split_kept)."""
        out = np.zeros(max(int(n), 1), dtype=EVENT_DTYPE)
        na = C.c_size_t(0)
        self._check(self.lib.gx_subsample_split_kept(self.ctx, int(sample), int(seed), int(threshold), out.ctypes.data, int(n), C.byref(na)))
        return out[:int(n)], na.value

    def reproducibility(self, seed=1, flags=0):
        """The peaks called once more on every replicate alone, on its two halves and on the two pools of halves
        (gx_reproducibility), after find_peaks(): REPRO_CALL_DTYPE records, 3 R + 2 of them."""
        n = C.c_size_t(0)
        cap = 3 * max(getattr(self, "_n_treat", 0), 1) + 2
        out = np.zeros(cap, dtype=REPRO_CALL_DTYPE)
        self._check(self.lib.gx_reproducibility(self.ctx, int(seed), int(flags), out.ctypes.data, cap, C.byref(n)))
        assert n.value <= cap, (n.value, cap)
        self._repro_peaks = [int(p) for p in out["n_peaks"][:n.value]]
        return out[:n.value]

    def reproducibility_peaks(self, call):
        """The peaks of one call of the last reproducibility() (gx_get_reproducibility_peaks), PEAK_DTYPE."""
        n = self._repro_peaks[call]
        out = np.zeros(n, dtype=PEAK_DTYPE)
        self._check(self.lib.gx_get_reproducibility_peaks(self.ctx, int(call), out.ctypes.data if n else None, n))
        return out

    def reproducibility_text(self, pct=50):
        """(calls, metrics): --reproducibility's two tables of the last reproducibility() against this run's peaks
        (gx_write_reproducibility)."""
        return (_to_tmpfile(lambda f: self.lib.gx_write_reproducibility(self.ctx, int(pct), f, None)),
                _to_tmpfile(lambda f: self.lib.gx_write_reproducibility(self.ctx, int(pct), None, f)))

    # -- fingerprint of the samples' bins (include/genrich_amd.h, gx_coverage_fingerprint) -------------------------------
    def coverage_fingerprint(self):
        """(n, count, sum) of the samples closed since the last reset: count and sum uint64 [S, FP_NC]."""
        S = max(self.coverage_samples(), 1)
        c, t = np.zeros((S, FP_NC), dtype=np.uint64), np.zeros((S, FP_NC), dtype=np.uint64)
        ns, n = C.c_int(0), C.c_uint64(0)
        self._check(self.lib.gx_coverage_fingerprint(self.ctx, C.byref(ns), C.byref(n), c.ctypes.data, t.ctypes.data, S))
        return n.value, c[:ns.value], t[:ns.value]

    def fp_u64(self, rows, grid=0):
        """(count, sum), uint64 [n_rows, FP_NC], of the rows (uint64 [n_rows, n]) by the same kernel (gx_fp_u64); grid = 0: the
        library's geometry, else that many workgroups along the bin axis."""
        r, ptr = _u64_rows(rows)
        n_rows, n = r.shape
        c, t = np.zeros((max(n_rows, 1), FP_NC), dtype=np.uint64), np.zeros((max(n_rows, 1), FP_NC), dtype=np.uint64)
        self._check(self.lib.gx_fp_u64(self.ctx, ptr, n_rows, n, int(grid), c.ctypes.data, t.ctypes.data))
        return c[:n_rows], t[:n_rows]

    # -- rank correlation of the samples' bins (include/genrich_amd.h, gx_coverage_distinct) -------------------------------
    def coverage_distinct(self, sample):
        """(values ascending, counts), uint64, of one closed sample's bins in this context (gx_coverage_distinct)."""
        n = C.c_size_t(0)
        self._check(self.lib.gx_coverage_distinct(self.ctx, int(sample), None, None, 0, C.byref(n)))
        v, c = np.zeros(n.value, dtype=np.uint64), np.zeros(n.value, dtype=np.uint64)
        if n.value:
            self._check(self.lib.gx_coverage_distinct(self.ctx, int(sample), v.ctypes.data, c.ctypes.data, n.value, C.byref(n)))
        return v, c

    def coverage_rank_gram(self, luts, skip_zeros=False):
        """(n, n_zero, sum, gram) of this context's rank rows by the samples' tables luts[s] = (values ascending, rank2)
        (gx_coverage_rank_gram): Python ints, sum an object array [S], gram [S, S]."""
        S = self.coverage_samples()
        arr, keep = _rank_structs(list(luts))
        s, g = _sums128(S)
        ns, n, nz = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        if len(luts) != S:
            raise ValueError("one table per sample")
        self._check(self.lib.gx_coverage_rank_gram(self.ctx, C.addressof(arr), int(bool(skip_zeros)), C.byref(ns), C.byref(n), C.byref(nz),
                                                   s.ctypes.data, g.ctypes.data, max(S, 1)))
        return n.value, nz.value, _join128(s[:ns.value]), _join128(g[:ns.value, :ns.value])

    def distinct_u64(self, row, grid=0):
        """(values ascending, counts) of the row (uint64 [n], every value < 2^51) by the same kernels (gx_distinct_u64); grid = 0:
        the library's geometry, else that many workgroups."""
        r, ptr = _u64_rows(row)
        n = C.c_size_t(0)
        v, c = np.zeros(max(r.size, 1), dtype=np.uint64), np.zeros(max(r.size, 1), dtype=np.uint64)
        self._check(self.lib.gx_distinct_u64(self.ctx, ptr, r.size, int(grid), v.ctypes.data, c.ctypes.data,
                                             v.size, C.byref(n)))
        return v[:n.value], c[:n.value]

    def rank_u64(self, rows, grid=0, skip_zeros=False):
        """(rank2 uint64 [n_rows, n], n_zero) of the rows (uint64 [n_rows, n], every value < 2^51) ranked as the samples of one
        context (gx_rank_u64); grid = 0: the library's geometry."""
        r, ptr = _u64_rows(rows)
        n_rows, n = r.shape
        out = np.zeros((n_rows, n), dtype=np.uint64)
        nz = C.c_uint64(0)
        self._check(self.lib.gx_rank_u64(self.ctx, ptr, n_rows, n, int(grid), int(bool(skip_zeros)),
                                         out.ctypes.data if out.size else None, C.byref(nz)))
        return out, nz.value

    def rank_last(self):
        """(capacity, n_grown) of this context's last k_rank_distinct pass (gx_rank_last); capacity 0: none yet."""
        cap, g = C.c_size_t(0), C.c_int(0)
        self._check(self.lib.gx_rank_last(self.ctx, C.byref(cap), C.byref(g)))
        return cap.value, g.value

    # -- profiles around anchors (include/genrich_amd.h, gx_set_profile) -------------------------------------------------
    def set_profile(self, anchors, flank, bin_size, keep_matrix=False):
        """Sum every closed sample's pileup over 2 * flank / bin_size bins around the anchors (ANCHOR_DTYPE; none: off); only
        while idle, after set_chroms."""
        a = np.ascontiguousarray(anchors, dtype=ANCHOR_DTYPE)
        self._check(self.lib.gx_set_profile(self.ctx, a.ctypes.data if a.size else None, a.size, int(flank), int(bin_size),
                                            int(bool(keep_matrix))))

    def profile_samples(self):
        n = C.c_int(0)
        self._check(self.lib.gx_profile_samples(self.ctx, C.byref(n)))
        return n.value

    def profile_layout(self):
        """(n_anchors, n_bins, flank, bin_size, has_matrix) as given to set_profile; zeros while off."""
        n, nb, f, b, m = C.c_size_t(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_int(0)
        self._check(self.lib.gx_profile_layout(self.ctx, C.byref(n), C.byref(nb), C.byref(f), C.byref(b), C.byref(m)))
        return n.value, nb.value, f.value, b.value, bool(m.value)

    def profile(self, sample, rows=None):
        """Profile(agg120 int64[n_bins], cell120 int64[n_rows, n_bins] | None, rep, is_ctrl) of one closed sample; rows = None:
        the whole matrix when one was kept, else (first_anchor, n_rows)."""
        n, nb, _, _, has = self.profile_layout()
        agg = np.zeros(nb, dtype=np.int64)
        if rows is None:
            rows = (0, n) if has else None
        cells = np.zeros((rows[1], nb), dtype=np.int64) if rows is not None else None
        rep, ctrl = C.c_int(0), C.c_int(0)
        self._check(self.lib.gx_get_profile(self.ctx, int(sample), C.byref(rep), C.byref(ctrl), agg.ctypes.data,
                                            cells.ctypes.data if cells is not None else None, rows[0] if rows else 0,
                                            rows[1] if rows else 0))
        return Profile(agg, cells, rep.value, bool(ctrl.value))

    def rccl_nranks(self):
        """Ranks of the library's own RCCL communicator as RCCL reports them (0: none)."""
        n = C.c_int(0)
        self._check(self.lib.gx_rccl_nranks(self.ctx, C.byref(n)))
        return n.value

    def set_phase_filter(self, name):
        """Time only the phase `name` (HIP events on the library's stream)."""
        self._check(self.lib.gx_set_phase_filter(self.ctx, name.encode()))

    def set_phase_timing(self, level):
        """0 none (default), 1 the tile stage only, 2 every phase (each event record costs the stream ~5 us)."""
        self._check(self.lib.gx_set_phase_timing(self.ctx, int(level)))

    def phase_times(self):
        names = C.c_char_p()
        ms = C.POINTER(C.c_float)()
        k = self.lib.gx_phase_times(self.ctx, C.byref(names), C.byref(ms))
        out = []
        # names are NUL-separated: walk the buffer
        addr = C.cast(names, C.c_void_p).value
        for i in range(k):
            s = C.string_at(addr)
            out.append((s.decode(), ms[i]))
            addr += len(s) + 1
        return out
