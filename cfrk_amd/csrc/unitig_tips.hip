// unitig_tips.hip -- the tip rule: which unitigs are short dead-end branches that hang off a better-supported path.  A
// pure function of the compacted graph: the unitigs' records (kc, n_kmers, circular), the link CSR as
// cfrk_global_unitig_links wrote it, and the job's strand rule.  No sequence, no index.  The contract is in
// include/cfrk_abi.h ("Unitig tips"); DESIGN 4.22 has the reasoning.
//
// The arrays are untrusted.  Passes, each a launch of its own on the context stream; every pass behind the check reads
// the error word first and does nothing when it is set, so that only checked rows are ever followed:
//   1-3 the check and, not canonical only, the in-rows: unitig_graph_dev.h, shared with the bubble rule
//   4 candidate one lane per unitig: not circular, n_kmers <= max_kmers, exactly one of left / right is 0 -> which
//   5 decide    one lane per unitig: a candidate's <= 8 attachments x their <= 8 siblings, BEATS in 128 bits
//   -- the one synchronisation: the error word and n_tips --
// In a canonical job the rows hold every link's mirror, so in(j,+) is the row's FROM_MINUS links mirrored, and the
// sources of in(v,-) are the targets of v's links that leave (v,+).
#include "unitig_graph_dev.h"

namespace {

enum { UTC_ERR = UGC_ERR, UTC_TIPS, UTC_WORDS };
enum { UT_DEAD_RIGHT = 1, UT_DEAD_LEFT = 2 };         // a candidate's cand[] byte: which end has no link

struct UTWork : UGraph {
  uint32_t max_kmers, ratio_q8;
  uint8_t *cand;                      // [nS]
  uint8_t *tip;                       // [nS], the caller's
};

// ---- 4 candidates -----------------------------------------------------------------------------------------------
template <bool CANON>
__global__ __launch_bounds__(256) void ut_cand_kernel(UTWork w) {
  if (w.ctr[UGC_ERR] != UG_NONE) return;
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
  if (w.ctr[UGC_ERR] != UG_NONE) return;
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
  if (const int rc = ug_scan_bytes(ctx, canon, n, &scan_tmp)) return rc;
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
  HIP_TRY(ctx, hipMemsetAsync(w.ctr + UTC_TIPS, 0, 8, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_tip, 0, n, ctx->stream));                     // every byte is written, whatever is refused
  const int grid = u_grid(ctx, n);
  if (const int rc = ug_check_launch(ctx, w, canon, grid, carve_at<void>(base, o_tmp), scan_tmp)) return rc;
  if (canon) {
    hipLaunchKernelGGL(ut_cand_kernel<true>, dim3(grid), dim3(256), 0, ctx->stream, w);
    hipLaunchKernelGGL(ut_decide_kernel<true>, dim3(grid), dim3(256), 0, ctx->stream, w);
  } else {
    hipLaunchKernelGGL(ut_cand_kernel<false>, dim3(grid), dim3(256), 0, ctx->stream, w);
    hipLaunchKernelGGL(ut_decide_kernel<false>, dim3(grid), dim3(256), 0, ctx->stream, w);
  }
  HIP_TRY(ctx, hipGetLastError());
  unsigned long long h[UTC_WORDS];
  HIP_TRY(ctx, hipMemcpyAsync(h, w.ctr, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (h[UTC_ERR] != UG_NONE) return ug_layout_error(ctx, h[UTC_ERR]);
  *n_tips = (int64_t)h[UTC_TIPS];
  return CFRK_OK;
}
