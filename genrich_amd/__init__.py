"""genrich_amd -- MI355X-native Genrich hot path (events -> pileup -> p -> q -> peaks).

The product is the C-ABI shared library `libgenrich_amd.so` (include/genrich_amd.h) built
from genrich_amd/csrc/*.hip; this package is the thin Python host mirror used by the tests
and bench.py.  It never falls back to a CPU implementation: loading fails loudly when the
HIP library is missing.
"""
from .lib import GxParams, Genrich, EVENT_DTYPE, PEAK_DTYPE, GX_PATH_COUNTS, PeakCounts, load_library, minus_log10f  # noqa: F401
from .lib import GX_PATH_REGION_COUNTS, REGION_DTYPE, RegionCounts  # noqa: F401
from .lib import GX_PATH_COVERAGE, Coverage, format_coverage  # noqa: F401
from .lib import GX_PATH_PROFILE, ANCHOR_DTYPE, Profile, format_profile, format_profile_rows  # noqa: F401
from .lib import GX_PATH_GRAM, U128_DTYPE, correlation_matrix, format_correlation, gram_geometry  # noqa: F401
from .lib import GX_PATH_FINGERPRINT, FP_NC, FP_METRICS_DTYPE, fp_geometry, fp_class, fp_class_lo, fp_class_hi  # noqa: F401
from .lib import fingerprint_metrics, format_fingerprint, format_fingerprint_metrics  # noqa: F401
from .lib import GX_PATH_IVSTAT, IntervalStats, interval_stats_geometry, interval_stats_group, interval_stats_text, lengths_metrics  # noqa: F401
from .lib import GX_PATH_XCOR, TAG_DTYPE, Xcor, xcor_geometry, xcor_group, xcor_metrics, xcor_r, xcor_text, format_xcor, format_xcor_metrics  # noqa: F401
