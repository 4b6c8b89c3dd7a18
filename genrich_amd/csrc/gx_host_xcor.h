// gx_host_xcor.h -- the host side of the strand cross-correlation (gx_xcor.h): the layout of the two bit vectors with their
// padding, the clearing at gx_sample_begin, the tags' way to the device (gx_push_tags), the pass at gx_sample_end with its
// read-back, the sum over contexts, and the kernels alone over given tags (gx_xcor_tags).  (a part of gx_api.hip's translation unit)
#pragma once
namespace {

constexpr size_t XC_PUSH = (size_t)1 << 20;   // tags per pinned staging buffer (12 MiB) and per k_xc_set launch of gx_push_tags

bool xc_chrom_laid_out(const gx_ctx* ctx, u32 c) { return !ctx->skip[c] && ctx->owned[c] && ctx->len[c] != 0; }

// the chromosomes' first words for a table of lengths (in[c]: the chromosome gets words at all), `pad` zero words before and
// after each; *words: the words of one vector
void xc_offsets(const uint32_t* len, const std::vector<uint8_t>& in, size_t n, u32 pad, std::vector<XcChrom>& tab, u64* words) {
  tab.assign(n, XcChrom{0, 0, 0});
  u64 at = pad;
  for (size_t c = 0; c < n; c++) {
    tab[c].len = len[c];
    if (!in[c]) continue;
    tab[c].off = at;
    at += ((u64)len[c] + 63) / 64 + pad;
  }
  *words = at;
}

// the limits of a setting, each with its sentence
int xc_check_range(gx_ctx* ctx, int lo, int hi, u64 bits) {
  if (lo < -XC_MAX_SHIFT || hi > XC_MAX_SHIFT || lo > hi) return refuse(ctx, "strand cross-correlation: the shifts must satisfy -4096 <= lo <= hi <= 4096");
  if (bits >= XC_MAX_BITS) return refuse(ctx, "strand cross-correlation: a genome of 2^37 bases or more");
  return GX_OK;
}

// the vectors for the context's table (after gx_set_xcor, and again when gx_set_chroms / gx_set_owned changed the table since)
int xc_layout(gx_ctx* ctx) {
  u64 bits = 0;
  std::vector<uint8_t> in(ctx->nChrom);
  for (u32 c = 0; c < ctx->nChrom; c++) {
    in[c] = xc_chrom_laid_out(ctx, c);
    if (in[c]) bits += ctx->len[c];
  }
  if (int rc = xc_check_range(ctx, ctx->xcLo, ctx->xcHi, bits)) return rc;
  xc_offsets(ctx->len.data(), in, ctx->nChrom, xc_pad_words(ctx->xcLo, ctx->xcHi), ctx->xcChrom, &ctx->xcWords);
  const size_t bytes = (size_t)(ctx->xcWords + XC_MAX_TILE) * 8;   // (a launch rounds the words up to whole tiles)
  if (ctx->xcPlus.ensure(bytes) != hipSuccess || ctx->xcMinus.ensure(bytes) != hipSuccess ||
      ctx->xcTab.ensure((size_t)ctx->nChrom * sizeof(XcChrom)) != hipSuccess ||
      ctx->xcOut.ensure((XCC_WORDS + (size_t)(2 * XC_MAX_SHIFT + 1)) * 8) != hipSuccess)
    return pool_failed(ctx);
  ctx->xcDirty = false;
  return GX_OK;
}

void drop_xcor(gx_ctx* ctx) {   // gx_reset: the results go, the setting and the buffers stay
  ctx->xc.clear();
  ctx->xcUsed = false;
}

// gx_sample_begin: which chromosomes take part in this sample, the two vectors and the counters cleared
int xc_begin(gx_ctx* ctx) {
  if (ctx->xcDirty)
    if (int rc = xc_layout(ctx)) return rc;
  hipStream_t s = ctx->stream;
  for (u32 c = 0; c < ctx->nChrom; c++) ctx->xcChrom[c].active = xc_chrom_laid_out(ctx, c) && ctx->save[c];
  HIPCHECK(hipMemcpyAsync(ctx->xcTab.p, ctx->xcChrom.data(), (size_t)ctx->nChrom * sizeof(XcChrom), hipMemcpyHostToDevice, s));
  const size_t bytes = (size_t)(ctx->xcWords + XC_MAX_TILE) * 8;
  HIPCHECK(hipMemsetAsync(ctx->xcPlus.p, 0, bytes, s));
  HIPCHECK(hipMemsetAsync(ctx->xcMinus.p, 0, bytes, s));
  HIPCHECK(hipMemsetAsync(ctx->xcOut.p, 0, (XCC_WORDS + (size_t)(ctx->xcHi - ctx->xcLo + 1)) * 8, s));
  HIPCHECK(hipStreamSynchronize(s));   // (the table's host copy is pageable and changes with the next sample)
  return GX_OK;
}

int xc_launch_set(gx_ctx* ctx, const XcTag* dTags, size_t n, const XcChrom* dTab, u32 nChrom, unsigned long long* plus,
                  unsigned long long* minus, unsigned long long* ctl) {
  for (size_t at = 0; at < n;) {   // (a launch of at most 2^30 tags: the grid stays below 2^31 workgroups)
    const size_t take = std::min(n - at, (size_t)1 << 30);
    hipLaunchKernelGGL(k_xc_set, dim3((unsigned)((take + XC_NT - 1) / XC_NT)), dim3(XC_NT), 0, ctx->stream, dTags + at, (u64)take, dTab, nChrom,
                       plus, minus, ctl);
    if (int rc__ = dbg_sync(ctx, "k_xc_set")) return rc__;
    HIPCHECK(hipGetLastError());
    at += take;
  }
  return GX_OK;
}

// gx_push_tags: through two pinned staging buffers to one device buffer and k_xc_set, all on the context's stream (the caller's
// memory is free on return)
int xc_push(gx_ctx* ctx, const gx_tag* tags, size_t n) {
  static_assert(sizeof(gx_tag) == sizeof(XcTag) && sizeof(gx_tag) == 12, "gx_tag is the kernel's record");
  hipStream_t s = ctx->stream;
  if (ctx->xcTags.ensure(XC_PUSH * sizeof(XcTag)) != hipSuccess) return pool_failed(ctx);
  while (n) {
    const size_t take = std::min(n, XC_PUSH);
    const int k = ctx->xcStageNext;
    ctx->xcStageNext ^= 1;
    HIPCHECK(ctx->xcStage[k].ensure(XC_PUSH * sizeof(XcTag)));
    if (!ctx->xcStageFree[k]) HIPCHECK(hipEventCreateWithFlags(&ctx->xcStageFree[k], hipEventDisableTiming));
    else HIPCHECK(hipEventSynchronize(ctx->xcStageFree[k]));   // its previous upload has left the buffer
    memcpy(ctx->xcStage[k].p, tags, take * sizeof(XcTag));
    HIPCHECK(hipMemcpyAsync(ctx->xcTags.p, ctx->xcStage[k].p, take * sizeof(XcTag), hipMemcpyHostToDevice, s));
    HIPCHECK(hipEventRecord(ctx->xcStageFree[k], s));
    if (int rc = xc_launch_set(ctx, ctx->xcTags.as<XcTag>(), take, ctx->xcTab.as<XcChrom>(), ctx->nChrom, ctx->xcPlus.as<unsigned long long>(),
                               ctx->xcMinus.as<unsigned long long>(), ctx->xcOut.as<unsigned long long>()))
      return rc;
    tags += take;
    n -= take;
  }
  ctx->xcUsed = true;
  return GX_OK;
}

// k_xc_corr over vectors of `words` words (allocated with XC_MAX_TILE words to spare); grid = 0 / tile = 0: the library's choices
int xc_launch_corr(gx_ctx* ctx, const unsigned long long* plus, const unsigned long long* minus, u64 words, int lo, int hi, unsigned grid, u32 tile,
                   unsigned long long* out) {
  if (tile == 0) tile = XC_TILE;
  if (tile < XC_MIN_TILE || tile > XC_MAX_TILE || tile % 64) return refuse(ctx, "strand cross-correlation: a tile must be a multiple of 64 words from 64 to 1024");
  if (grid > XC_MAX_GRID) return refuse(ctx, "strand cross-correlation: more than 65535 workgroups");
  const u64 nTiles = (words + tile - 1) / tile;
  if (grid == 0) grid = (unsigned)std::min<u64>(nTiles, XC_GRID);
  grid = std::max(1u, grid);
  const u32 pad = xc_pad_words(lo, hi);
  hipLaunchKernelGGL(k_xc_corr, dim3(grid), dim3(XC_NT), xc_lds_bytes(tile, pad, (u32)(hi - lo + 1)), ctx->stream, plus, minus, nTiles * tile, tile, lo,
                     hi, out);
  if (int rc__ = dbg_sync(ctx, "k_xc_corr")) return rc__;
  HIPCHECK(hipGetLastError());
  return GX_OK;
}

// the counters of one pass to the host
int xc_read(gx_ctx* ctx, const DevBuf& out, int lo, int hi, gx_ctx::XcResult& r) {
  const size_t nS = (size_t)(hi - lo + 1);
  std::vector<unsigned long long> h(XCC_WORDS + nS, 0);
  HIPCHECK(hipMemcpyAsync(h.data(), out.p, h.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  r.nP = h[XCC_NPLUS];
  r.nM = h[XCC_NMINUS];
  r.rejected = h[XCC_REJECTED];
  r.n11.assign(h.begin() + XCC_WORDS, h.end());
  for (uint64_t v : r.n11)
    if (v > r.nP || v > r.nM) {
      ctx->err = "strand cross-correlation: more pairs at a shift than tags on a strand (a lost or doubled contribution)";
      return GX_ERR_DEVICE;
    }
  return GX_OK;
}

// gx_sample_end, the cross-correlation on: the one pass over the sample's vectors
int xc_sample(gx_ctx* ctx, int isCtrl) {
  gx_ctx::XcResult r;
  r.rep = ctx->sample;
  r.ctrl = isCtrl != 0;
  for (u32 c = 0; c < ctx->nChrom; c++)
    if (ctx->xcChrom[c].active) r.N += ctx->len[c];
  phase_begin(ctx, isCtrl ? "c.xcor" : "t.xcor");
  if (int rc = xc_launch_corr(ctx, ctx->xcPlus.as<unsigned long long>(), ctx->xcMinus.as<unsigned long long>(), ctx->xcWords, ctx->xcLo, ctx->xcHi,
                              ctx->knob.xcorGrid > 0 ? (unsigned)ctx->knob.xcorGrid : 0u, ctx->knob.xcorTile > 0 ? (u32)ctx->knob.xcorTile : 0u,
                              ctx->xcOut.as<unsigned long long>()))
    return rc;
  phase_end(ctx);
  ctx->xcUsed = true;
  if (int rc = xc_read(ctx, ctx->xcOut, ctx->xcLo, ctx->xcHi, r)) return rc;
  ctx->xc.push_back(std::move(r));
  return GX_OK;
}

// gx_xcor_tags: the two kernels over tags in host memory and a table of its own, every chromosome taking part; buffers of its
// own (released on return), the context's setting and results untouched
int xc_tags(gx_ctx* ctx, const uint32_t* lens, int n_chrom, const gx_tag* tags, size_t n, int lo, int hi, unsigned grid, u32 tile,
            gx_ctx::XcResult& r) {
  u64 bits = 0;
  for (int c = 0; c < n_chrom; c++) bits += lens[c];
  if (int rc = xc_check_range(ctx, lo, hi, bits)) return rc;
  std::vector<XcChrom> tab;
  std::vector<uint8_t> in((size_t)n_chrom);
  for (int c = 0; c < n_chrom; c++) in[c] = lens[c] != 0;
  u64 words = 0;
  xc_offsets(lens, in, (size_t)n_chrom, xc_pad_words(lo, hi), tab, &words);
  for (int c = 0; c < n_chrom; c++) tab[c].active = in[c];
  r.N = bits;
  hipStream_t s = ctx->stream;
  DevBuf plus, minus, dTab, out, dTags;
  const size_t bytes = (size_t)(words + XC_MAX_TILE) * 8, outBytes = (XCC_WORDS + (size_t)(hi - lo + 1)) * 8;
  if (plus.ensure(bytes) != hipSuccess || minus.ensure(bytes) != hipSuccess || dTab.ensure(tab.size() * sizeof(XcChrom)) != hipSuccess ||
      out.ensure(outBytes) != hipSuccess || dTags.ensure(std::max<size_t>(n, 1) * sizeof(XcTag)) != hipSuccess)
    return pool_failed(ctx);
  HIPCHECK(hipMemcpy(dTab.p, tab.data(), tab.size() * sizeof(XcChrom), hipMemcpyHostToDevice));
  if (n) HIPCHECK(hipMemcpy(dTags.p, tags, n * sizeof(XcTag), hipMemcpyHostToDevice));
  HIPCHECK(hipMemsetAsync(plus.p, 0, bytes, s));
  HIPCHECK(hipMemsetAsync(minus.p, 0, bytes, s));
  HIPCHECK(hipMemsetAsync(out.p, 0, outBytes, s));
  phase_begin(ctx, "xcor.set");
  if (int rc = xc_launch_set(ctx, dTags.as<XcTag>(), n, dTab.as<XcChrom>(), (u32)n_chrom, plus.as<unsigned long long>(), minus.as<unsigned long long>(),
                             out.as<unsigned long long>()))
    return rc;
  phase_end(ctx);
  phase_begin(ctx, "xcor.corr");
  if (int rc = xc_launch_corr(ctx, plus.as<unsigned long long>(), minus.as<unsigned long long>(), words, lo, hi, grid, tile, out.as<unsigned long long>()))
    return rc;
  phase_end(ctx);
  ctx->xcUsed = true;
  if (int rc = xc_read(ctx, out, lo, hi, r)) return rc;   // (synchronises: the buffers may go)
  return GX_OK;
}

// b added to a (a chromosome lives on one context: everything adds)
void xc_add(gx_ctx::XcResult& a, const gx_ctx::XcResult& b) {
  a.N += b.N;
  a.nP += b.nP;
  a.nM += b.nM;
  a.rejected += b.rejected;
  if (a.n11.size() < b.n11.size()) a.n11.resize(b.n11.size(), 0);
  for (size_t k = 0; k < b.n11.size(); k++) a.n11[k] += b.n11[k];
}

int xc_give(const gx_ctx::XcResult& r, int rlo, int rhi, int* rep, int* is_ctrl, uint64_t* n_pos, uint64_t* n_plus, uint64_t* n_minus, uint64_t* rejected,
            int* lo, int* hi, uint64_t* n11, size_t cap) {
  if (cap && !n11) return GX_ERR_ORDER;
  if (rep) *rep = r.rep;
  if (is_ctrl) *is_ctrl = r.ctrl ? 1 : 0;
  if (n_pos) *n_pos = r.N;
  if (n_plus) *n_plus = r.nP;
  if (n_minus) *n_minus = r.nM;
  if (rejected) *rejected = r.rejected;
  if (lo) *lo = rlo;
  if (hi) *hi = rhi;
  const size_t n = std::min(cap, r.n11.size());
  if (n) std::copy(r.n11.begin(), r.n11.begin() + n, n11);
  return GX_OK;
}

}  // namespace
