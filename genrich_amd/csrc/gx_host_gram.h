// gx_host_gram.h -- the host side of the samples' Gram sums (gx_gram.h): the two launches over rows that are on the device
// already, the scatter of the tiles' results.  (a part of gx_api.hip's translation unit)
#pragma once
namespace {

// n_zero, sum[S], gram[S][S] (both halves) of the S device rows of n values each; grid = 0: the library's geometry
int gram_pass(gx_ctx* ctx, const std::vector<const void*>& rows, u64 n, u32 grid, u64* nZero, std::vector<gx_u128>& sum,
              std::vector<gx_u128>& gram) {
  const u32 S = (u32)rows.size();
  sum.assign(S, gx_u128{0, 0});
  gram.assign((size_t)S * S, gx_u128{0, 0});
  *nZero = 0;
  if (!n) return GX_OK;
  const u32 nT = (S + GRAM_T - 1) / GRAM_T, nY = nT * (nT + 1) / 2 + 1;
  const u32 lanes = GRAM_NW * 64;
  if (!grid) grid = (u32)std::min<u64>((n + lanes - 1) / lanes, GRAM_GRID);
  const size_t outWords = (size_t)nY * GRAM_ACCS * 2;
  POOLED(ctx, ctx->gramPartial, outWords * grid * 8);
  POOLED(ctx, ctx->gramOut, outWords * 8);
  if (int rc = stat_upload_rows(ctx, rows)) return rc;
  hipStream_t s = ctx->stream;
  phase_begin(ctx, "gram");
  hipLaunchKernelGGL(k_gram, dim3(grid, nY), dim3(lanes), 0, s, ctx->statRows.as<const unsigned long long*>(), S, n, nT,
                     ctx->gramPartial.as<unsigned long long>());
  if (int rc__ = dbg_sync(ctx, "k_gram")) return rc__;
  hipLaunchKernelGGL(k_gram_sum, dim3(nY), dim3(256), 0, s, ctx->gramPartial.as<unsigned long long>(), grid, ctx->gramOut.as<unsigned long long>());
  if (int rc__ = dbg_sync(ctx, "k_gram_sum")) return rc__;
  phase_end(ctx);
  HIPCHECK(hipGetLastError());
  ctx->gramUsed = true;
  std::vector<gx_u128> out((size_t)nY * GRAM_ACCS);
  HIPCHECK(hipMemcpyAsync(out.data(), ctx->gramOut.p, outWords * 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  u32 y = 0;
  for (u32 I = 0; I < nT; I++)
    for (u32 J = I; J < nT; J++, y++) {
      const gx_u128* t = out.data() + (size_t)y * GRAM_ACCS;
      for (u32 i = 0; i < (u32)GRAM_T; i++)
        for (u32 j = (I == J ? i : 0); j < (u32)GRAM_T; j++) {
          const u32 si = I * GRAM_T + i, sj = J * GRAM_T + j;
          if (si < S && sj < S) gram[(size_t)si * S + sj] = gram[(size_t)sj * S + si] = t[i * GRAM_T + j];
        }
      if (I == 0)
        for (u32 j = 0; j < (u32)GRAM_T; j++)
          if (J * GRAM_T + j < S) sum[J * GRAM_T + j] = t[GRAM_T * GRAM_T + j];
    }
  *nZero = out[(size_t)y * GRAM_ACCS + GRAM_ACCS - 1].lo;
  return GX_OK;
}

}  // namespace
