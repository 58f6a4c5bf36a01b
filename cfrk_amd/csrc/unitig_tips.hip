// unitig_tips.hip -- the tip rule: which unitigs are short dead-end branches that hang off a better-supported path.  A
// pure function of the compacted graph: the unitigs' records (kc, n_kmers, circular), the link CSR as
// cfrk_global_unitig_links wrote it, and the job's strand rule.  No sequence, no index.  The contract is in
// include/cfrk_abi.h ("Unitig tips"); DESIGN 4.22 has the reasoning.
//
// The arrays are untrusted.  Passes, each a launch of its own on the context stream; every pass behind the check reads
// the error word first and does nothing when it is set, so that only checked rows are ever followed:
//   1 check     one lane per unitig: link_ptr[j] <= link_ptr[j + 1] inside [0, n_links] (0 at j = 0, n_links at the
//               end), a row of at most 16 links (4 when not canonical), targets below nS, no undefined flag bit (none
//               at all when not canonical).  Not canonical: a checked row counts its targets' in-degrees.
//   not canonical only, where in() cannot be read off a unitig's own row:
//   2 in-degree one lane per unitig: at most 4; hipCUB exclusive sum over the in-degrees, in place
//   3 in-rows   one lane per unitig: its links' sources into the targets' in-rows, a cursor per target (the order inside
//               an in-row does not matter: the rule only asks "is there one")
//   4 candidate one lane per unitig: not circular, n_kmers <= max_kmers, exactly one of left / right is 0 -> which
//   5 decide    one lane per unitig: a candidate's <= 8 attachments x their <= 8 siblings, BEATS in 128 bits
//   -- the one synchronisation: the error word and n_tips --
// In a canonical job the rows hold every link's mirror, so in(j,+) is the row's FROM_MINUS links mirrored, and the
// sources of in(v,-) are the targets of v's links that leave (v,+).
#include "staging.h"
#include "unitig_dev.h"

#include <hipcub/hipcub.hpp>

namespace {

constexpr unsigned long long UT_NONE = ~0ull;
enum { UTC_ERR = 0, UTC_TIPS, UTC_WORDS };
// error word = unitig << 8 | why, kept with an atomic minimum: the first offending unitig
enum { UTE_PTR = 1, UTE_ROW, UTE_TARGET, UTE_FLAGS, UTE_INDEG };
enum { UT_DEAD_RIGHT = 1, UT_DEAD_LEFT = 2 };         // a candidate's cand[] byte: which end has no link

struct UTWork {
  const cfrk_unitig *rec;
  const int64_t *ptr;
  const cfrk_unitig_link *links;
  uint64_t nS;
  int64_t n_links;
  uint32_t max_kmers, ratio_q8;
  unsigned long long *ctr;            // UTC_*
  uint8_t *cand;                      // [nS]
  unsigned long long *in_off;         // [nS + 1], not canonical: in-degrees, scanned into the in-rows' offsets
  uint32_t *in_cur;                   // [nS]: the fill pass's cursors
  uint32_t *in_src;                   // [n_links]: the in-rows
  uint8_t *tip;                       // [nS], the caller's
};

__device__ __forceinline__ void ut_fail(const UTWork &w, uint64_t j, int why) {
  atomicMin(&w.ctr[UTC_ERR], (unsigned long long)((j << 8) | (uint64_t)why));
}

// ---- 1 check ----------------------------------------------------------------------------------------------------
template <bool CANON>
__global__ __launch_bounds__(256) void ut_check_kernel(UTWork w) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = tid; j < w.nS; j += nthreads) {
    const int64_t a = w.ptr[j], b = w.ptr[j + 1];
    int why = 0;
    if ((j == 0 && a != 0) || (j + 1 == w.nS && b != w.n_links) || a < 0 || b < a || b > w.n_links) why = UTE_PTR;
    else if (b - a > (CANON ? 16 : 4)) why = UTE_ROW;
    else
      for (int64_t t = a; t < b; ++t) {
        const cfrk_unitig_link l = w.links[t];
        if (l.to >= w.nS) { why = UTE_TARGET; break; }
        if (l.flags & ~(CANON ? (uint32_t)(CFRK_LINK_FROM_MINUS | CFRK_LINK_TO_MINUS) : 0u)) { why = UTE_FLAGS; break; }
      }
    if (why) { ut_fail(w, j, why); continue; }
    if (!CANON)
      for (int64_t t = a; t < b; ++t) atomicAdd(&w.in_off[w.links[t].to], 1ull);
  }
}

// ---- 2, 3 the in-rows of a job that is not canonical ------------------------------------------------------------
__global__ __launch_bounds__(256) void ut_indeg_kernel(UTWork w) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = tid; j < w.nS; j += nthreads)
    if (w.in_off[j] > 4) ut_fail(w, j, UTE_INDEG);
}

__global__ __launch_bounds__(256) void ut_in_fill_kernel(UTWork w) {
  if (w.ctr[UTC_ERR] != UT_NONE) return;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = tid; j < w.nS; j += nthreads) {
    const int64_t a = w.ptr[j], b = w.ptr[j + 1];
    for (int64_t t = a; t < b; ++t) {
      const uint32_t v = w.links[t].to;
      const unsigned long long at = w.in_off[v] + atomicAdd(&w.in_cur[v], 1u);
      if (at < w.in_off[v + 1]) w.in_src[at] = (uint32_t)j;     // (always: the offsets are the scan of these very counts)
    }
  }
}

// ---- 4 candidates -----------------------------------------------------------------------------------------------
template <bool CANON>
__global__ __launch_bounds__(256) void ut_cand_kernel(UTWork w) {
  if (w.ctr[UTC_ERR] != UT_NONE) return;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = tid; j < w.nS; j += nthreads) {
    const int64_t a = w.ptr[j], b = w.ptr[j + 1];
    uint64_t left = 0, right = 0;
    if (CANON) {
      for (int64_t t = a; t < b; ++t) { if (w.links[t].flags & CFRK_LINK_FROM_MINUS) ++left; else ++right; }
    } else {
      right = (uint64_t)(b - a);
      left = w.in_off[j + 1] - w.in_off[j];
    }
    const cfrk_unitig r = w.rec[j];
    const bool c = !(r.flags & CFRK_UNITIG_CIRCULAR) && r.n_kmers <= w.max_kmers && ((left == 0) != (right == 0));
    w.cand[j] = c ? (uint8_t)(right == 0 ? UT_DEAD_RIGHT : UT_DEAD_LEFT) : (uint8_t)0;
  }
}

// ---- 5 decide ---------------------------------------------------------------------------------------------------
// sibling w beats candidate j: 256 kc_w n_j >= ratio_q8 kc_j n_w, and w is no candidate or ranks above j.  kc < 2^64,
// n < 2^32, ratio_q8 <= 2^16: every product stays below 2^113.
__device__ __forceinline__ bool ut_beats(const UTWork &w, uint32_t s, uint32_t j, const cfrk_unitig &rj) {
  const cfrk_unitig rs = w.rec[s];
  const u128 a = (u128)rs.kc * rj.n_kmers, b = (u128)rj.kc * rs.n_kmers;
  if ((a << 8) < b * w.ratio_q8) return false;
  return w.cand[s] == 0 || a > b || (a == b && s < j);
}

template <bool CANON>
__device__ __forceinline__ bool ut_is_tip(const UTWork &w, uint32_t j, int dead) {
  const cfrk_unitig rj = w.rec[j];
  const int64_t a = w.ptr[j], b = w.ptr[j + 1];
  if (CANON) {
    // dead right: the attachments are in(j,+), the mirrors (v,!ov) -> (j,+) of the row's links (j,-) -> (v,ov); the
    //   siblings are the targets of out(v,!ov).  dead left: the attachments are out(j,+), links (j,+) -> (v,ov); the
    //   siblings are the sources of in(v,ov), which are the targets of v's links that leave (v,!ov).
    // Either way: the links of row j that leave (j, dead right ? - : +), and at their target v the links that leave
    // (v,!ov).
    const uint32_t from = dead == UT_DEAD_RIGHT ? CFRK_LINK_FROM_MINUS : 0u;
    for (int64_t t = a; t < b; ++t) {
      const cfrk_unitig_link l = w.links[t];
      if ((l.flags & CFRK_LINK_FROM_MINUS) != from) continue;
      const uint32_t want = (l.flags & CFRK_LINK_TO_MINUS) ? 0u : CFRK_LINK_FROM_MINUS;
      const int64_t c = w.ptr[l.to], d = w.ptr[l.to + 1];
      for (int64_t x = c; x < d; ++x) {
        const cfrk_unitig_link m = w.links[x];
        if ((m.flags & CFRK_LINK_FROM_MINUS) == want && m.to != j && ut_beats(w, m.to, j, rj)) return true;
      }
    }
    return false;
  }
  if (dead == UT_DEAD_RIGHT) {                          // u -> j for every u of j's in-row; the siblings: u's targets
    for (unsigned long long t = w.in_off[j]; t < w.in_off[j + 1]; ++t) {
      const uint32_t u = w.in_src[t];
      for (int64_t x = w.ptr[u]; x < w.ptr[u + 1]; ++x) {
        const uint32_t s = w.links[x].to;
        if (s != j && ut_beats(w, s, j, rj)) return true;
      }
    }
    return false;
  }
  for (int64_t t = a; t < b; ++t) {                     // j -> v; the siblings: v's in-row
    const uint32_t v = w.links[t].to;
    for (unsigned long long x = w.in_off[v]; x < w.in_off[v + 1]; ++x) {
      const uint32_t s = w.in_src[x];
      if (s != j && ut_beats(w, s, j, rj)) return true;
    }
  }
  return false;
}

template <bool CANON>
__global__ __launch_bounds__(256) void ut_decide_kernel(UTWork w) {
  if (w.ctr[UTC_ERR] != UT_NONE) return;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  // (whole waves turn together: the ballot below counts a wave's tips)
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < w.nS; base += nthreads) {
    const uint64_t j = base + threadIdx.x;
    bool tip = false;
    if (j < w.nS) {
      const int dead = w.cand[j];
      tip = dead != 0 && ut_is_tip<CANON>(w, (uint32_t)j, dead);
      w.tip[j] = tip ? 1 : 0;
    }
    const unsigned long long m = __ballot(tip);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&w.ctr[UTC_TIPS], (unsigned long long)__popcll(m));
  }
}

}  // namespace

// The rule on device arrays; nS >= 1.  Synchronises once: CFRK_ERR_LAYOUT naming the unitig, or *n_tips.
int cfrk_unitig_tips_launch(cfrk_ctx *ctx, const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr,
                            const cfrk_unitig_link *d_links, int64_t n_links, uint32_t max_kmers, uint32_t ratio_q8,
                            uint8_t *d_tip, int64_t *n_tips) {
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  const uint64_t n = (uint64_t)nS, in_n = canon ? 0 : n;
  size_t scan_tmp = 0;
  if (!canon) HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_tmp, (unsigned long long *)nullptr, (size_t)(n + 1), ctx->stream));
  Carve c;
  const size_t o_ctr = c.part(UTC_WORDS * 8), o_cand = c.part(n), o_off = c.part(canon ? 0 : (in_n + 1) * 8), o_cur = c.part(in_n * 4),
               o_src = c.part(canon ? 0 : (size_t)n_links * 4), o_tmp = c.part(scan_tmp);
  void *base;
  if (const int rc = cfrk_pool_get(ctx, BUF_UNITIG_TIPS, c.end, &base)) return rc;
  UTWork w;
  w.rec = d_rec; w.ptr = d_link_ptr; w.links = d_links; w.nS = n; w.n_links = n_links;
  w.max_kmers = max_kmers; w.ratio_q8 = ratio_q8; w.tip = d_tip;
  w.ctr = carve_at<unsigned long long>(base, o_ctr);
  w.cand = carve_at<uint8_t>(base, o_cand);
  w.in_off = carve_at<unsigned long long>(base, o_off);
  w.in_cur = carve_at<uint32_t>(base, o_cur);
  w.in_src = carve_at<uint32_t>(base, o_src);
  HIP_TRY(ctx, hipMemsetAsync(w.ctr, 0xFF, 8, ctx->stream));                  // UTC_ERR: no unitig yet
  HIP_TRY(ctx, hipMemsetAsync(w.ctr + UTC_TIPS, 0, 8, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_tip, 0, n, ctx->stream));                     // every byte is written, whatever is refused
  const int grid = u_grid(ctx, n);
  if (canon) {
    hipLaunchKernelGGL(ut_check_kernel<true>, dim3(grid), dim3(256), 0, ctx->stream, w);
    hipLaunchKernelGGL(ut_cand_kernel<true>, dim3(grid), dim3(256), 0, ctx->stream, w);
    hipLaunchKernelGGL(ut_decide_kernel<true>, dim3(grid), dim3(256), 0, ctx->stream, w);
  } else {
    HIP_TRY(ctx, hipMemsetAsync(w.in_off, 0, (n + 1) * 8, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(w.in_cur, 0, n * 4, ctx->stream));
    hipLaunchKernelGGL(ut_check_kernel<false>, dim3(grid), dim3(256), 0, ctx->stream, w);
    hipLaunchKernelGGL(ut_indeg_kernel, dim3(grid), dim3(256), 0, ctx->stream, w);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(carve_at<void>(base, o_tmp), scan_tmp, w.in_off, (size_t)(n + 1), ctx->stream));
    hipLaunchKernelGGL(ut_in_fill_kernel, dim3(grid), dim3(256), 0, ctx->stream, w);
    hipLaunchKernelGGL(ut_cand_kernel<false>, dim3(grid), dim3(256), 0, ctx->stream, w);
    hipLaunchKernelGGL(ut_decide_kernel<false>, dim3(grid), dim3(256), 0, ctx->stream, w);
  }
  HIP_TRY(ctx, hipGetLastError());
  unsigned long long h[UTC_WORDS];
  HIP_TRY(ctx, hipMemcpyAsync(h, w.ctr, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (h[UTC_ERR] != UT_NONE) {
    const unsigned long long j = h[UTC_ERR] >> 8;
    const int why = (int)(h[UTC_ERR] & 255);
    const char *what = why == UTE_PTR      ? "has a link_ptr that does not ascend from 0 to n_links"
                       : why == UTE_ROW    ? "has a row of more links than an oriented end can have"
                       : why == UTE_TARGET ? "has a link to a unitig that is not in the list"
                       : why == UTE_FLAGS  ? "has a link with an undefined flag bit, or a strand flag in a job that is not canonical"
                                           : "is entered by more than 4 links";
    return cfrk_fail(ctx, CFRK_ERR_LAYOUT, "unitig %llu %s: not the links of a unitig list of this strand rule", j, what);
  }
  *n_tips = (int64_t)h[UTC_TIPS];
  return CFRK_OK;
}
