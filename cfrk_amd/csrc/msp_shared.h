// msp_shared.h -- what the partitioned counting paths of both key widths share and that does not depend on the
// record format: the two one-workgroup helper kernels (exact layout of a level, sum of cursors), the numbering of
// the level-1 regions, and the host-side rules and steps of an add -- how many workgroups share a leaf, how much
// slack the leaf streams get, the index buffers, the exact level-1 layout after an overflow, the passes of a batch
// that does not fit.  Included by msp.hip (16-byte records, MspView) and msp2.hip (32-byte records, View2) inside
// their anonymous namespaces, like msp_runs.h (the exchange by runs).  The partition, leaf and dedupe kernels, and
// the retry loops that decide what to do about an overflow, stay in the two files.
#pragma once

// Level-1 region (and cursor) of bin `bin`, sub-region `xg`: sub-region major.  Global atomics
// execute at the memory side, one 64-byte request per touched 64 bytes: with the cursors of the
// 256 bins of one sub-region side by side, a workgroup's 256 reservations are 16 requests instead
// of 256.
__host__ __device__ __forceinline__ uint32_t l1_reg(uint32_t bin, uint32_t xg) { return xg * (uint32_t)B1 + bin; }

// bits of the minimizer hash, beyond the leaf id, that a record of a job with shared leaves carries at most
constexpr int SUB_BITS = 5;

// exact layout of a level from the demand the first attempt counted: base = exclusive prefix sum
// of the n cursors, cap = the cursors themselves (single workgroup, 1024 threads)
// (slack: room beyond the counted demand per region -- the chunked path runs P1 again, and which records its
//  first level PARKED last time depended on the order of atomics: a stream's demand may differ by a few)
__global__ __launch_bounds__(1024) void msp_layout_kernel(const uint32_t *__restrict__ cnt, uint32_t n,
                                                          uint64_t *__restrict__ base, uint32_t *__restrict__ cap, uint32_t slack = 0u) {
  __shared__ unsigned long long part[1024];
  const uint32_t per = (n + 1023u) / 1024u;
  const uint32_t tid = threadIdx.x;
  unsigned long long s = 0;
  for (uint32_t i = 0; i < per; ++i) { const uint32_t l = tid * per + i; if (l < n) s += (unsigned long long)cnt[l] + slack; }
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    unsigned long long run = 0;
    for (int i = 0; i < 1024; ++i) { const unsigned long long x = part[i]; part[i] = run; run += x; }
  }
  __syncthreads();
  unsigned long long run = part[tid];
  for (uint32_t i = 0; i < per; ++i) {
    const uint32_t l = tid * per + i;
    if (l < n) { const uint32_t c = cnt[l] + slack; base[l] = run; cap[l] = c; run += c; }
  }
}

// sum of n cursors (one workgroup): how many records the first chunk of a batch made.  out[1 .. SUM_CLASSES] are
// cleared for the class-sample kernel that follows (one word per class of leaf streams; the callers hand in 64 words)
constexpr int SUM_CLASSES = 4;
__global__ __launch_bounds__(1024) void msp_sum_kernel(const uint32_t *__restrict__ cnt, uint32_t n, uint64_t *out) {
  __shared__ unsigned long long tot;
  if (threadIdx.x == 0) tot = 0;
  __syncthreads();
  unsigned long long mine = 0;
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) mine += cnt[i];
  atomicAdd(&tot, mine);
  __syncthreads();
  if (threadIdx.x == 0) {
    out[0] = tot;
    for (int c = 1; c <= SUM_CLASSES; ++c) out[c] = 0;
  }
}

// Far more distinct k-mers expected per leaf (per_leaf: table slots announced) than the leaf tables hold
// (65536 x ~2500): records carry extra minimizer-hash bits and 2^sub_bits workgroups share a leaf (~2000 distinct
// k-mers each).
static uint32_t msp_sub_bits(const cfrk_ctx *ctx, uint64_t per_leaf) {
  uint32_t sub_bits = 0;
  while (sub_bits < (uint32_t)SUB_BITS && (per_leaf >> sub_bits) > 2048u) ++sub_bits;
  if (per_leaf <= 4096u) sub_bits = 0;
  if ((ctx->dbg_flags & CFRK_DEBUG_RECORD_SUBSETS) && sub_bits < 2u) sub_bits = 2u;
  return sub_bits;
}

// Room of a chunked batch's leaf streams over their share of the mean leaf, for windows of W k-mers: complete runs
// 1.45 x (measured on C3: with 1.3 x a few leaves' complete streams overflow and their records are parked --
// counted through the HBM table, +0.5 ms and a merge at finish; 1.4 x has none), truncated ones 1.6 x -- and more
// where a leaf holds few distinct runs, because its load scatters with their number (the copies of a run come and
// go together): lambda = distinct k-mers per leaf x 4 / (W + 1) -- 320 for C3, 64 for 20 M reads of a 20 Mb
// genome, whose heaviest complete stream is 2.0 x the mean one (5448 records parked at 1.45 x)
// (the table holds 2 .. 4 x the announced distinct k-mers: a third of it stands for the hint)
static void msp_leaf_slack(const cfrk_ctx *ctx, int W, double *fc_slack, double *ft_slack) {
  const double lambda = std::max(4.0, (double)ctx->g_cap / 3.0 / (double)NLEAF * 4.0 / (double)(W + 1));
  *fc_slack = std::min(4.0, std::max(1.45, 1.2 + 6.5 / std::sqrt(lambda)));
  *ft_slack = std::min(4.0, std::max(1.6, 1.3 + 6.5 / std::sqrt(lambda)));
}

// BUF_MSP_AUX: the leaf index (one entry per leaf, or per (leaf, sub-value) when leaves are shared: nseg entries),
// then the cursors of the nxg x B1 level-1 regions and of the ncnt2 leaf streams
template <class View>
static int msp_aux_buffers(cfrk_ctx *ctx, View &v, size_t nseg, int nxg, size_t ncnt2) {
  void *p;
  int rc;
  if ((rc = cfrk_pool_get(ctx, BUF_MSP_AUX, nseg * 8 + ((size_t)B1 * nxg + ncnt2 + nseg) * sizeof(uint32_t), &p))) return rc;
  v.leaf_off = (uint64_t *)p;
  v.cnt1 = (uint32_t *)(v.leaf_off + nseg); v.cnt2 = v.cnt1 + (size_t)B1 * nxg; v.leaf_n = v.cnt2 + ncnt2;
  return CFRK_OK;
}
// ... cleared before a pass: cnt1, cnt2 and -- first pass only -- the leaf index and the list cursor
template <class View>
static int msp_aux_clear(cfrk_ctx *ctx, const View &v, size_t nseg, int nxg, size_t ncnt2, bool first) {
  HIP_TRY(ctx, hipMemsetAsync(v.cnt1, 0, ((size_t)B1 * nxg + ncnt2 + (first ? nseg : 0)) * sizeof(uint32_t), ctx->stream));
  if (first) HIP_TRY(ctx, hipMemsetAsync(ctx->g_stats + ST_CURSOR, 0, sizeof(uint64_t), ctx->stream));
  return CFRK_OK;
}

// Exact level-1 layout after regions overflowed: the cursors counted on past the capacity, so cnt1 is the exact
// demand.  Regions back to back (rbase / rcap in BUF_MSP_LAYOUT1), the buffer grown when the batch holds more
// records than the density estimate allowed for (nreg x cap1), cnt1 and the ncnt2 cursors behind it cleared for
// the next attempt.  *maxbin: records of the heaviest bin.
template <class Rec>
static int msp_layout_level1(cfrk_ctx *ctx, uint32_t *cnt1, int nxg, size_t ncnt2, uint64_t cap1, Rec **rec1,
                             const uint64_t **rbase, const uint32_t **rcap, uint64_t *maxbin) {
  int rc;
  void *p;
  const size_t nreg = (size_t)B1 * nxg;
  if ((rc = cfrk_pool_get(ctx, BUF_MSP_LAYOUT1, nreg * (sizeof(uint64_t) + sizeof(uint32_t)), &p))) return rc;
  uint64_t *base = (uint64_t *)p;
  uint32_t *cap = (uint32_t *)(base + nreg);
  hipLaunchKernelGGL(msp_layout_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t *)cnt1, (uint32_t)nreg, base, cap, 0u);
  HIP_TRY(ctx, hipGetLastError());
  std::vector<uint32_t> c1(nreg);
  HIP_TRY(ctx, hipMemcpyAsync(c1.data(), cnt1, nreg * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t all = 0;
  *maxbin = 0;
  for (int b = 0; b < B1; ++b) {
    uint64_t sum = 0;
    for (int r = 0; r < nxg; ++r) sum += c1[l1_reg((uint32_t)b, (uint32_t)r)];
    *maxbin = std::max(*maxbin, sum);
    all += sum;
  }
  if (all > (uint64_t)nreg * cap1) {
    if ((rc = cfrk_pool_get(ctx, BUF_MSP_L1, (size_t)all * sizeof(Rec), &p))) return rc;
    *rec1 = (Rec *)p;
  }
  HIP_TRY(ctx, hipMemsetAsync(cnt1, 0, (nreg + ncnt2) * sizeof(uint32_t), ctx->stream));   // cnt1 and cnt2
  *rbase = base; *rcap = cap;
  return CFRK_OK;
}

// The tail of an add.  One pass: pass(slack, 0, 0, true) -- leaves are lumpy when the genome is small (few
// distinct runs per leaf, each repeated by every read over it), so with memory to spare (`widen`; have / need:
// bytes the pool holds / a pass needs, l2: bytes of the leaf streams) the streams get up to twice the room and an
// ordinary imbalance does not end in the spill path.  A batch whose records do not fit beside the caller's data is
// counted in `passes` passes over the WHOLE input, each emitting only the runs of 1/passes of the leaves (leaf id
// low bits): the partition kernel's front end runs again every pass, but every pass produces the FINAL counts of
// its leaves -- nothing to merge afterwards, and the result stays in per-leaf list form.
template <class Pass /* int(double slack, int sel_bits, uint32_t sel_val, bool first) */>
static int msp_for_each_pass(cfrk_ctx *ctx, int passes, bool widen, size_t have, size_t need, double l2, Pass pass) {
  if (passes == 1) {
    double slack = 1.0;
    size_t free_b = 0, total_b = 0;
    if (widen && hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
      size_t budget = have + free_b;
      if (ctx->mem_budget) budget = std::min(budget, ctx->mem_budget);
      const double room = 0.5 * (double)budget - (double)need;
      if (room > 0 && l2 > 0) slack = std::min(2.0, 1.0 + room / l2);
    }
    return pass(slack, 0, 0u, true);
  }
  int sel_bits = 0;
  while ((1 << sel_bits) < passes) ++sel_bits;
  for (int i = 0; i < passes; ++i) {
    const int rc = pass(1.0, sel_bits, (uint32_t)i, i == 0);
    // a refusal after the first pass must not reach the caller's fallback (it would count
    // the finished passes twice)
    if (i > 0 && (rc == CFRK_ERR_NOMEM || rc == CFRK_INTERNAL_FLOOD)) return cfrk_fail(ctx, CFRK_ERR_STATE, "out of device memory in pass %d of a multi-pass add", i);
    if (rc) return rc;
  }
  return CFRK_OK;
}
