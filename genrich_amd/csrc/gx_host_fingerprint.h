// gx_host_fingerprint.h -- the host side of the samples' fingerprint histograms (gx_fingerprint.h): one fill and one launch
// over rows that are on the device already.  (a part of gx_api.hip's translation unit)
#pragma once
namespace {

// count[S][FP_NC] and sum[S][FP_NC] of the S device rows (16-byte aligned) of n values each; grid = 0: the library's geometry
int fp_pass(gx_ctx* ctx, const std::vector<const void*>& rows, u64 n, u32 grid, std::vector<uint64_t>& count, std::vector<uint64_t>& sum) {
  const u32 S = (u32)rows.size();
  count.assign((size_t)S * FP_NC, 0);
  sum.assign((size_t)S * FP_NC, 0);
  if (!n) return GX_OK;
  const u32 lanes = FP_NW * 64;
  // (a workgroup's step is two values a lane; with S rows the launch stays at FP_GRID workgroups: what is resident together)
  if (!grid) grid = (u32)std::min<u64>((n + 2 * lanes - 1) / (2 * lanes), std::max<u32>(FP_GRID / S, 1u));
  const size_t outBytes = (size_t)2 * S * FP_NC * 8;
  POOLED(ctx, ctx->fpOut, (size_t)2 * FP_MAX_S * FP_NC * 8);
  if (int rc = stat_upload_rows(ctx, rows)) return rc;
  hipStream_t s = ctx->stream;
  phase_begin(ctx, "fingerprint");
  HIPCHECK(hipMemsetAsync(ctx->fpOut.p, 0, outBytes, s));
  if (ctx->knob.fpAgg)
    hipLaunchKernelGGL(k_fp_hist<true>, dim3(grid, S), dim3(lanes), 0, s, ctx->statRows.as<const unsigned long long*>(), n,
                       ctx->fpOut.as<unsigned long long>());
  else
    hipLaunchKernelGGL(k_fp_hist<false>, dim3(grid, S), dim3(lanes), 0, s, ctx->statRows.as<const unsigned long long*>(), n,
                       ctx->fpOut.as<unsigned long long>());
  if (int rc__ = dbg_sync(ctx, "k_fp_hist")) return rc__;
  phase_end(ctx);
  HIPCHECK(hipGetLastError());
  ctx->fpUsed = true;
  HIPCHECK(hipMemcpyAsync(count.data(), ctx->fpOut.p, outBytes / 2, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(sum.data(), ctx->fpOut.as<char>() + outBytes / 2, outBytes / 2, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  return GX_OK;
}

}  // namespace
