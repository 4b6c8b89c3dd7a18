// gx_host_binstat.h -- what the statistics over the coverage bins share (gx_host_gram.h, gx_host_fingerprint.h, gx_host_rank.h):
// the closed samples' bins as device rows, the *_u64 hooks' domain and their staging copy, the table of row pointers, the
// 128-bit sums over contexts.  (a part of gx_api.hip's translation unit)
#pragma once
namespace {

constexpr size_t STAT_MAX_S = 32;   // the samples of a statistic
static_assert(STAT_MAX_S == GRAM_MAX_S && STAT_MAX_S == FP_MAX_S && STAT_MAX_S == RK_MAX_S, "the statistics share their row tables");
static_assert(GRAM_MAX_GRID == 65535 && FP_MAX_GRID == 65535 && RK_MAX_GRID == 65535, "the hooks share their grid limit");

// the closed samples' bins: S device rows (each the start of an allocation: aligned) of n values, over G bases
struct BinRows {
  std::vector<const void*> rows;
  u64 n = 0, G = 0;
};

// the order rules of every statistic over the bins, and the rows; `what`: the statistic, for the sentence about 32 samples
int stat_cov_rows(gx_ctx* ctx, const char* what, BinRows& b) {
  if (!ctx || !ctx->covW || ctx->cov.empty() || ctx->phase == 1 || ctx->phase == 3) return GX_ERR_ORDER;
  const size_t S = ctx->cov.size();
  if (S > STAT_MAX_S) {
    ctx->err = std::string("more than 32 samples for ") + what;
    return GX_ERR_ORDER;
  }
  if (ctx->covDirty)
    if (int rc = cov_layout(ctx)) return rc;
  b.n = ctx->covOff[ctx->nChrom];
  b.G = 0;   // (the lengths are u32, a table has fewer than 2^31 entries: no overflow)
  for (u32 c = 0; c < ctx->nChrom; c++)
    if (cov_has_bins(ctx, c)) b.G += ctx->len[c];
  b.rows.resize(S);
  for (size_t i = 0; i < S; i++) b.rows[i] = ctx->cov[i].bins.p;
  return GX_OK;
}

// an entry's arrays of cap samples a side take S samples
int stat_cap(gx_ctx* ctx, const char* entry, bool wanted, int cap, size_t S) {
  if (wanted && (cap < 0 || (size_t)cap < S)) return refuse(ctx, std::string(entry) + ": cap is smaller than the number of samples");
  return GX_OK;
}

// the *_u64 hooks' domain; `values`: every value below 2^51 too (the fingerprint's hook bounds the rows' totals instead)
int stat_u64_domain(gx_ctx* ctx, const char* entry, const uint64_t* rows, int n_rows, size_t n, unsigned grid, bool values) {
  if (!ctx) return GX_ERR_ORDER;
  const char* why = nullptr;
  if (n_rows < 1 || n_rows > (int)STAT_MAX_S) why = ": the number of rows is outside [1, 32]";
  else if (n > ((size_t)1 << 24)) why = ": more than 2^24 values a row";
  else if (n && !rows) why = ": no rows";
  else if (grid > 65535) why = ": a grid of more than 65535 workgroups";
  for (size_t k = 0; !why && values && k < (size_t)n_rows * n; k++)
    if (rows[k] >> 51) why = ": a value of 2^51 or more";
  return why ? refuse(ctx, std::string(entry) + why) : GX_OK;
}

// the caller's rows (host, row after row) on the device, 16 bytes apart at least: an odd n is padded by one value no lane reads
int stat_stage_rows(gx_ctx* ctx, const uint64_t* rows, int n_rows, size_t n, std::vector<const void*>& dev) {
  dev.assign((size_t)n_rows, nullptr);
  HIPCHECK(hipSetDevice(ctx->device));
  if (!n) return GX_OK;
  const size_t pitch = (n + 1) & ~(size_t)1;
  std::vector<uint64_t> staged((size_t)n_rows * pitch, 0);
  for (int r = 0; r < n_rows; r++) std::copy(rows + (size_t)r * n, rows + (size_t)(r + 1) * n, staged.begin() + (size_t)r * pitch);
  POOLED(ctx, ctx->statIn, staged.size() * 8);
  HIPCHECK(hipMemcpyAsync(ctx->statIn.p, staged.data(), staged.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHECK(hipStreamSynchronize(ctx->stream));   // (`staged` is this call's)
  for (int r = 0; r < n_rows; r++) dev[r] = ctx->statIn.as<uint64_t>() + (size_t)r * pitch;
  return GX_OK;
}

// the rows a kernel reads, and behind them the rows it writes, into ctx->statRows; the caller's vectors are free once the
// stream has been waited for: here, or with wait = false by a caller that queues more first
int stat_upload_rows(gx_ctx* ctx, const std::vector<const void*>& in, const std::vector<const void*>& out = {}, bool wait = true) {
  POOLED(ctx, ctx->statRows, 2 * STAT_MAX_S * sizeof(void*));
  HIPCHECK(hipMemcpyAsync(ctx->statRows.p, in.data(), in.size() * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
  if (!out.empty())
    HIPCHECK(hipMemcpyAsync(ctx->statRows.as<const void*>() + STAT_MAX_S, out.data(), out.size() * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
  if (wait) HIPCHECK(hipStreamSynchronize(ctx->stream));
  return GX_OK;
}

u128 join128(const gx_u128& x) { return ((u128)x.hi << 64) | x.lo; }
gx_u128 split128(u128 x) { return gx_u128{(uint64_t)x, (uint64_t)(x >> 64)}; }

// (sum[S], gram[S][S]) added over contexts with carries
struct Sums128 {
  size_t S;
  std::vector<u128> sum, gram;
  explicit Sums128(size_t S_) : S(S_), sum(S_, 0), gram(S_ * S_, 0) {}
  void add(const gx_u128* s, const gx_u128* g) {
    for (size_t k = 0; k < S; k++) sum[k] += join128(s[k]);
    for (size_t k = 0; k < S * S; k++) gram[k] += join128(g[k]);
  }
  void give(gx_u128* s, gx_u128* g) const {
    for (size_t k = 0; k < S; k++) s[k] = split128(sum[k]);
    for (size_t k = 0; k < S * S; k++) g[k] = split128(gram[k]);
  }
};

// a pass's dense sums to the caller: sum[S], and gram's rows cap entries apart; either may be absent
void stat_give_sums(const std::vector<gx_u128>& s1, const std::vector<gx_u128>& g1, gx_u128* sum, gx_u128* gram, size_t cap) {
  const size_t S = s1.size();
  if (sum) std::copy(s1.begin(), s1.end(), sum);
  if (gram)
    for (size_t i = 0; i < S; i++) std::copy(g1.begin() + i * S, g1.begin() + (i + 1) * S, gram + i * cap);
}

}  // namespace
