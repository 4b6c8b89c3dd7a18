// gx_host_rank.h -- the host side of the samples' rank rows (gx_rank.h): a row's distinct values through the table that grows,
// the count of the all-zero bins, the rank rows from the uploaded tables, the samples' rank tables over contexts.  (a part of
// gx_api.hip's translation unit)
#pragma once
namespace {

u32 rank_first_cap_log(const gx_ctx* ctx) {
  return ctx->knob.rankCapLog ? (u32)std::max(6, std::min(RK_CAP_LOG_MAX, ctx->knob.rankCapLog)) : (u32)RK_CAP_LOG;
}

// which k_rank runs: the table probed (true) or searched (false)
bool rank_lookup_probes(const gx_ctx* ctx) {
  return (ctx->knob.rankLookup ? ctx->knob.rankLookup : RK_LOOKUP) == 2;
}

int rank_read_ctl(gx_ctx* ctx, u32* ctl) {
  HIPCHECK(hipMemcpyAsync(ctl, ctx->rankCtl.p, RKC_WORDS * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  return GX_OK;
}

// the distinct values of one device row (16-byte aligned) of n values, ascending, and how often each occurs;
// grid = 0: the library's geometry
int rank_distinct_pass(gx_ctx* ctx, const void* row, u64 n, u32 grid, std::vector<uint64_t>& val, std::vector<uint64_t>& cnt) {
  val.clear();
  cnt.clear();
  if (!n) return GX_OK;
  HIPCHECK(hipSetDevice(ctx->device));
  const u32 lanes = RK_NW * 64;
  if (!grid) grid = (u32)std::min<u64>((n + 2 * lanes - 1) / (2 * lanes), RK_GRID);   // (a lane's load is two values; a row of more than
                                                                                     // 2 * RK_GRID * lanes values brings the second load of a step in)
  hipStream_t s = ctx->stream;
  u32 capLog = rank_first_cap_log(ctx), grown = 0;
  u32 ctl[RKC_WORDS];
  for (;;) {
    const size_t cap = (size_t)1 << capLog;
    POOLED(ctx, ctx->rankTab, cap * 12);
    POOLED(ctx, ctx->rankCtl, RKC_WORDS * 4);
    RankTab T;
    T.keys = ctx->rankTab.as<unsigned long long>();
    T.counts = reinterpret_cast<u32*>(T.keys + cap);
    T.mask = (u32)(cap - 1);
    T.limit = (u32)(cap / RK_LOAD_DIV);
    T.ctl = ctx->rankCtl.as<u32>();
    phase_begin(ctx, "rank_distinct");
    HIPCHECK(hipMemsetAsync(T.keys, 0xFF, cap * 8, s));
    HIPCHECK(hipMemsetAsync(T.counts, 0, cap * 4, s));
    HIPCHECK(hipMemsetAsync(T.ctl, 0, RKC_WORDS * 4, s));
    hipLaunchKernelGGL(k_rank_distinct, dim3(grid), dim3(lanes), 0, s, static_cast<const unsigned long long*>(row), n, T);
    if (int rc__ = dbg_sync(ctx, "k_rank_distinct")) return rc__;
    phase_end(ctx);
    HIPCHECK(hipGetLastError());
    if (int rc = rank_read_ctl(ctx, ctl)) return rc;
    if (!ctl[RKC_OVER]) {
      ctx->rankLastCapLog = capLog;
      ctx->rankLastGrown = grown;
      const u32 used = ctl[RKC_USED];
      const u64 zeros = (u64)ctl[RKC_ZEROS] | ((u64)ctl[RKC_ZEROS + 1] << 32);
      std::vector<uint64_t> v(used), c(used);
      if (used) {
        POOLED(ctx, ctx->rankPairs, (size_t)used * 16);
        unsigned long long* dv = ctx->rankPairs.as<unsigned long long>();
        phase_begin(ctx, "rank_compact");
        hipLaunchKernelGGL(k_rank_compact, dim3((u32)std::min<size_t>((cap + 255) / 256, RK_GRID)), dim3(256), 0, s, T, dv, dv + used);
        if (int rc__ = dbg_sync(ctx, "k_rank_compact")) return rc__;
        phase_end(ctx);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpyAsync(v.data(), dv, (size_t)used * 8, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipMemcpyAsync(c.data(), dv + used, (size_t)used * 8, hipMemcpyDeviceToHost, s));
        if (int rc = rank_read_ctl(ctx, ctl)) return rc;
        if (ctl[RKC_NOUT] != used) {
          ctx->err = "k_rank_compact: the table's slots do not add up";
          return GX_ERR_DEVICE;
        }
      }
      // (the slots come in the order of the races: nobody sees it)
      std::vector<u32> order(used);
      for (u32 i = 0; i < used; i++) order[i] = i;
      std::sort(order.begin(), order.end(), [&](u32 a, u32 b) { return v[a] < v[b]; });
      val.reserve((size_t)used + 1);
      cnt.reserve((size_t)used + 1);
      if (zeros) {
        val.push_back(0);
        cnt.push_back(zeros);
      }
      for (u32 i : order) {
        val.push_back(v[i]);
        cnt.push_back(c[i]);
      }
      return GX_OK;
    }
    if (capLog >= (u32)RK_CAP_LOG_MAX) {
      ctx->err = "more distinct values in a row than a table holds";
      return GX_ERR_ORDER;
    }
    capLog = std::min<u32>(capLog + RK_GROW_LOG, RK_CAP_LOG_MAX);
    grown++;
  }
}

// the row pointers for a kernel that counts into the control words, and those cleared
int rank_upload_rows(gx_ctx* ctx, const std::vector<const void*>& in, const std::vector<const void*>& out) {
  POOLED(ctx, ctx->rankCtl, RKC_WORDS * 4);
  if (int rc = stat_upload_rows(ctx, in, out, false)) return rc;
  HIPCHECK(hipMemsetAsync(ctx->rankCtl.p, 0, RKC_WORDS * 4, ctx->stream));
  HIPCHECK(hipStreamSynchronize(ctx->stream));   // (the vectors are the caller's)
  return GX_OK;
}

// the number of bins that are 0 in every one of the device rows
int rank_nzero_pass(gx_ctx* ctx, const std::vector<const void*>& rows, u64 n, u64* nZero) {
  *nZero = 0;
  if (!n) return GX_OK;
  HIPCHECK(hipSetDevice(ctx->device));
  if (int rc = rank_upload_rows(ctx, rows, {})) return rc;
  phase_begin(ctx, "rank_nzero");
  hipLaunchKernelGGL(k_rank_nzero, dim3((u32)std::min<u64>((n + 255) / 256, RK_GRID)), dim3(256), 0, ctx->stream,
                     ctx->statRows.as<const unsigned long long*>(), (u32)rows.size(), n, ctx->rankCtl.as<u32>());
  if (int rc__ = dbg_sync(ctx, "k_rank_nzero")) return rc__;
  phase_end(ctx);
  HIPCHECK(hipGetLastError());
  u32 ctl[RKC_WORDS];
  if (int rc = rank_read_ctl(ctx, ctl)) return rc;
  *nZero = (u64)ctl[RKC_NZERO] | ((u64)ctl[RKC_NZERO + 1] << 32);
  return GX_OK;
}

// the rank rows of the S device rows of n values each, by the samples' tables (value ascending, rank2); out: the S rows in
// ctx->rankOut (16-byte aligned, as k_gram reads bins); nZero: the bins that are 0 in every row.  grid = 0: the library's geometry
int rank_rows_pass(gx_ctx* ctx, const std::vector<const void*>& rows, u64 n, u32 grid, bool skip, const gx_rank_lut* lut,
                   std::vector<const void*>& out, u64* nZero) {
  const u32 S = (u32)rows.size();
  out.assign(S, nullptr);
  *nZero = 0;
  if (!n) return GX_OK;
  HIPCHECK(hipSetDevice(ctx->device));
  const size_t pitch = (size_t)((n + 1) & ~(u64)1);
  const bool probe = rank_lookup_probes(ctx);
  // binary search: the values of all samples, then their ranks; probe: per sample a power of two of (value, rank2) pairs, at
  // most half of them used, filled here as the kernel reads them (rk_lookup)
  std::vector<size_t> room(S, 0);
  size_t total = 0;
  for (u32 i = 0; i < S; i++) {
    room[i] = lut[i].n;
    if (probe && lut[i].n) {
      room[i] = 2;
      while (room[i] < 2 * lut[i].n) room[i] <<= 1;
    }
    total += room[i];
  }
  const size_t head = RK_MAX_S + 2;   // the offsets, in 8-byte words (even: the tables stay 16-byte aligned)
  POOLED(ctx, ctx->rankOut, (size_t)S * pitch * 8);
  POOLED(ctx, ctx->rankLut, (head + 2 * total) * 8);
  std::vector<uint64_t> staged(head + 2 * total, 0);
  if (probe) std::fill(staged.begin() + head, staged.end(), (uint64_t)RK_EMPTY);
  size_t at = 0;
  for (u32 i = 0; i < S; i++) {
    staged[i] = at;
    if (probe) {
      uint64_t* pairs = staged.data() + head + 2 * at;
      for (size_t k = 0; k < lut[i].n; k++) {
        size_t h = rk_hash(lut[i].value[k]) & (room[i] - 1);
        while (pairs[2 * h] != RK_EMPTY) h = (h + 1) & (room[i] - 1);
        pairs[2 * h] = lut[i].value[k];
        pairs[2 * h + 1] = lut[i].rank2[k];
      }
    } else if (lut[i].n) {
      std::copy(lut[i].value, lut[i].value + lut[i].n, staged.begin() + head + at);
      std::copy(lut[i].rank2, lut[i].rank2 + lut[i].n, staged.begin() + head + total + at);
    }
    at += room[i];
  }
  staged[S] = at;
  for (u32 i = 0; i < S; i++) out[i] = ctx->rankOut.as<uint64_t>() + (size_t)i * pitch;
  hipStream_t s = ctx->stream;
  HIPCHECK(hipMemcpyAsync(ctx->rankLut.p, staged.data(), staged.size() * 8, hipMemcpyHostToDevice, s));
  if (int rc = rank_upload_rows(ctx, rows, out)) return rc;   // (it waits for the stream: `staged` is this call's)
  if (!grid) grid = (u32)std::min<u64>((n + 255) / 256, RK_GRID);
  const unsigned long long* lutp = ctx->rankLut.as<unsigned long long>();
  phase_begin(ctx, "rank");
  hipLaunchKernelGGL(probe ? k_rank<true> : k_rank<false>, dim3(grid), dim3(256), 0, s, ctx->statRows.as<const unsigned long long*>(),
                     ctx->statRows.as<unsigned long long*>() + STAT_MAX_S, S, n, lutp + head, lutp + head + total,
                     reinterpret_cast<const u64*>(lutp), skip ? 1 : 0, ctx->rankCtl.as<u32>());
  if (int rc__ = dbg_sync(ctx, "k_rank")) return rc__;
  phase_end(ctx);
  HIPCHECK(hipGetLastError());
  ctx->rankUsed = true;
  u32 ctl[RKC_WORDS];
  if (int rc = rank_read_ctl(ctx, ctl)) return rc;
  if (ctl[RKC_MISSING]) {
    ctx->err = "a bin's value is missing from its sample's rank table";
    return GX_ERR_ORDER;
  }
  *nZero = (u64)ctl[RKC_NZERO] | ((u64)ctl[RKC_NZERO + 1] << 32);
  return GX_OK;
}

// the closed samples' bins as device rows (stat_cov_rows), within what a rank fits
int rank_cov_rows(gx_ctx* ctx, BinRows& b) {
  if (int rc = stat_cov_rows(ctx, "the rank correlation", b)) return rc;
  if (b.n > ((u64)1 << 30)) return refuse(ctx, "more than 2^30 bins in a context for the rank correlation");
  return GX_OK;
}

// the lookup tables a caller gives: ascending values below RK_EMPTY (the probed table's free slot), every rank2 in [1, 2^42)
bool rank_lut_ok(const gx_rank_lut* lut, size_t S) {
  for (size_t i = 0; i < S; i++) {
    if (lut[i].n && (!lut[i].value || !lut[i].rank2)) return false;
    for (size_t k = 0; k < lut[i].n; k++)
      if ((k && lut[i].value[k - 1] >= lut[i].value[k]) || lut[i].value[k] == RK_EMPTY || !lut[i].rank2[k] || lut[i].rank2[k] >> 42) return false;
  }
  return true;
}

// a pass's table to the caller: the number always, the pairs when cap says there is room (cap = 0: the number only)
int rank_give_table(gx_ctx* ctx, const char* who, const std::vector<uint64_t>& v, const std::vector<uint64_t>& c, uint64_t* value, uint64_t* count,
                    size_t cap, size_t* n_distinct) {
  if (n_distinct) *n_distinct = v.size();
  if (!cap) return GX_OK;
  if (cap < v.size()) {
    ctx->err = std::string(who) + ": cap is smaller than the number of distinct values";
    return GX_ERR_ORDER;
  }
  std::copy(v.begin(), v.end(), value);
  std::copy(c.begin(), c.end(), count);
  return GX_OK;
}

// the samples' rank tables over the rows of one or more contexts, and the storage behind them
struct RankGroup {
  gx_ctx* ctx;
  std::vector<const void*> rows;   // S device rows (16-byte aligned) of n values each
  u64 n;
};
struct RankTables {
  std::vector<std::vector<uint64_t>> value, rank2;   // per sample, what lut[] points to
  std::vector<gx_rank_lut> lut;
  std::vector<size_t> nDistinct;                     // the entries of each sample's table
  u64 nZero = 0, nRanked = 0;                        // the all-zero bins left out (skip), the bins ranked
};

// per group the count of the all-zero bins (skip) and a distinct pass per row, then gx_rank_tables over all groups; `why`: what
// every group's context says when the tables do not merge
int rank_make_tables(const std::vector<RankGroup>& groups, u32 grid, bool skip, const char* why, RankTables& t) {
  const size_t G = groups.size(), S = groups[0].rows.size();
  std::vector<std::vector<uint64_t>> v(G * S), c(G * S);
  std::vector<gx_rank_table> tabs(G * S);
  std::vector<size_t> room(S, 0);
  t.nZero = 0;
  for (size_t g = 0; g < G; g++) {
    const RankGroup& gr = groups[g];
    if (skip) {
      u64 nz = 0;
      if (int rc = rank_nzero_pass(gr.ctx, gr.rows, gr.n, &nz)) return rc;
      t.nZero += nz;
    }
    for (size_t i = 0; i < S; i++) {
      const size_t k = g * S + i;
      if (int rc = rank_distinct_pass(gr.ctx, gr.rows[i], gr.n, grid, v[k], c[k])) return rc;
      tabs[k] = gx_rank_table{v[k].data(), c[k].data(), v[k].size()};
      room[i] += v[k].size();
    }
  }
  const size_t most = *std::max_element(room.begin(), room.end());
  t.value.resize(S);
  t.rank2.resize(S);
  std::vector<uint64_t*> pv(S), pr(S);
  for (size_t i = 0; i < S; i++) {
    t.value[i].resize(most);
    t.rank2[i].resize(most);
    pv[i] = t.value[i].data();
    pr[i] = t.rank2[i].data();
  }
  t.nDistinct.assign(S, 0);
  uint64_t N = 0;
  if (int rc = gx_rank_tables((int)G, (int)S, tabs.data(), t.nZero, pv.data(), pr.data(), most, t.nDistinct.data(), &N)) {
    for (const RankGroup& gr : groups) gr.ctx->err = why;
    return rc;
  }
  t.nRanked = N;
  t.lut.resize(S);
  for (size_t i = 0; i < S; i++) t.lut[i] = gx_rank_lut{pv[i], pr[i], t.nDistinct[i]};
  return GX_OK;
}

}  // namespace
