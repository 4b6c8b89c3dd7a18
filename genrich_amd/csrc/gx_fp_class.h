// gx_fp_class.h -- the value classes of the fingerprint (include/genrich_amd.h, gx_coverage_fingerprint), shared by the device
// (k_fp_hist), the host side of the library and the text writers.  A part of gx_math.h, kept in a file of its own only so that
// gx_emit.cpp, which is plain C++ and sees no HIP header, can include it too.
//
// With M = GX_FP_SUB_LOG = 6:   x < 2^M:  class(x) = x
//                               else      e = 63 - clz(x),  class(x) = (e - M) 2^M + (x >> (e - M))
// The mantissa x >> (e - M) lies in [2^M, 2^(M+1)), so the octave e starts at class (e - M + 1) 2^M, where the octave below
// ended: continuous and monotone.  Values below 2^(M+1) = 128 have a class of their own; above, an octave has 2^M = 64
// classes and a class's values differ by less than 1 / 64 relative.  GX_FP_NC = (64 - M + 1) 2^M = 3776 classes cover uint64.
// The inverse: k < 2^(M+1): lo = hi = k; else q = k / 2^M - 1, lo = (k - 2^M q) << q, hi = lo + 2^q - 1.
#pragma once
#include <stdint.h>

#ifndef GX_HD
#define GX_FP_HD_LOCAL
#define GX_HD
#endif

#define GX_FP_SUB_LOG 6
#define GX_FP_NC ((64 - GX_FP_SUB_LOG + 1) << GX_FP_SUB_LOG)

namespace gx {

GX_HD inline uint32_t fp_class(uint64_t x) {
  if (x < (1ull << GX_FP_SUB_LOG)) return (uint32_t)x;
  const int e = 63 - __builtin_clzll(x);
  return (uint32_t)(e - GX_FP_SUB_LOG) * (1u << GX_FP_SUB_LOG) + (uint32_t)(x >> (e - GX_FP_SUB_LOG));
}

// the smallest / largest value of class k < GX_FP_NC
GX_HD inline uint64_t fp_class_lo(uint32_t k) {
  if (k < (2u << GX_FP_SUB_LOG)) return k;
  const uint32_t q = (k >> GX_FP_SUB_LOG) - 1;
  return (uint64_t)(k - (q << GX_FP_SUB_LOG)) << q;
}
GX_HD inline uint64_t fp_class_hi(uint32_t k) {
  if (k < (2u << GX_FP_SUB_LOG)) return k;
  const uint32_t q = (k >> GX_FP_SUB_LOG) - 1;
  return fp_class_lo(k) + ((1ull << q) - 1);
}

}  // namespace gx

#ifdef GX_FP_HD_LOCAL
#undef GX_HD
#undef GX_FP_HD_LOCAL
#endif
