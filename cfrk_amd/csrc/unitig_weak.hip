// unitig_weak.hip -- the weak rule: which unitigs are erroneous connections (short, thin, linked at both ends, and at
// every one of those links beside a much better-covered way out of the same neighbour) and which are isolated
// low-coverage pieces (short, thin, no link at all).  A pure function of the compacted graph, like the tip rule: the
// unitigs' records, the link CSR as cfrk_global_unitig_links wrote it, and the job's strand rule.  No sequence, no
// index.  The contract is in include/cfrk_abi.h ("Weak unitigs"); DESIGN 4.27 has the reasoning.
//
// The arrays are untrusted.  Passes, each a launch of its own on the context stream; the pass behind the check reads the
// error word first and does nothing when it is set, so that only checked rows are ever followed:
//   1-3 the check and, not canonical only, the in-rows: unitig_graph_dev.h, shared with the tip rule
//   4 decide    one lane per unitig: its own row (<= 16 links) for left, right and SELF-FREE; no link at all: the
//               isolated test; a candidate: every link of the row is an attachment, and at its target the links on the
//               entering side are the siblings (<= 8 of them in a real link set): BEATS in 128 bits, "some sibling" inside
//               "every attachment", both loops leaving early.  No LDS, no scratch; the three counts are summed per wave over
//               the whole launch and added once
//   -- the one synchronisation: the error word and the three counts --
// In a canonical job the rows hold every link's mirror, so the left end of (j,+) is the right end of (j,-): a link
// (j,oj) -> (v,ov) of row j is an attachment of one end or the other, and the sources of in(v,ov) are the targets of
// v's links that leave (v,!ov).  One loop serves both ends.
#include "unitig_graph_dev.h"

namespace {

enum { UWC_ERR = UGC_ERR, UWC_CONN, UWC_ISO, UWC_CAND, UWC_WORDS };

struct UWWork : UGraph {
  uint32_t max_kmers, ratio_q8, iso_max_kmers, iso_mean_q8;
  uint8_t *weak;                      // [nS], the caller's
};

// sibling s beats j: 256 kc_s n_j >= ratio_q8 kc_j n_s, and s ranks above j.  kc < 2^64, n < 2^32, ratio_q8 <= 2^16:
// every product stays below 2^113.
__device__ __forceinline__ bool uw_beats(const UWWork &w, uint32_t s, uint32_t j, const cfrk_unitig &rj) {
  const cfrk_unitig rs = w.rec[s];
  const u128 a = (u128)rs.kc * rj.n_kmers, b = (u128)rj.kc * rs.n_kmers;
  if ((a << 8) < b * w.ratio_q8) return false;
  return a > b || (a == b && s < j);
}

// -> 0, CFRK_WEAK_CONNECTION or CFRK_WEAK_ISOLATED; cand: j is a candidate
template <bool CANON>
__device__ __forceinline__ int uw_decide(const UWWork &w, uint32_t j, bool &cand) {
  const cfrk_unitig rj = w.rec[j];
  if (rj.flags & CFRK_UNITIG_CIRCULAR) return 0;
  const int64_t a = w.ptr[j], b = w.ptr[j + 1];
  uint64_t left = 0, right = 0;
  bool self = false;
  for (int64_t t = a; t < b; ++t) {
    const cfrk_unitig_link l = w.links[t];
    if (l.to == j) self = true;
    if (CANON && (l.flags & CFRK_LINK_FROM_MINUS)) ++left; else ++right;
  }
  if (!CANON) {
    left = w.in_off[j + 1] - w.in_off[j];
    for (unsigned long long t = w.in_off[j]; t < w.in_off[j + 1]; ++t)
      if (w.in_src[t] == j) self = true;
  }
  if (left == 0 && right == 0)        // 256 kc < 2^72, iso_mean_q8 n < 2^64
    return rj.n_kmers <= w.iso_max_kmers && ((u128)rj.kc << 8) < (u128)((uint64_t)w.iso_mean_q8 * rj.n_kmers) ? CFRK_WEAK_ISOLATED : 0;
  if (rj.n_kmers > w.max_kmers || left == 0 || right == 0 || self) return 0;
  cand = true;
  if (CANON) {
    // a link (j,+) -> (v,ov) is an attachment of the right end, a link (j,-) -> (v,ov) the mirror of (v,!ov) -> (j,+), an
    // attachment of the left end, whose siblings, the targets of out(v,!ov), are as unitigs the sources of in(v,ov).
    // Either way: at the target v the links that leave (v,!ov).
    for (int64_t t = a; t < b; ++t) {
      const cfrk_unitig_link l = w.links[t];
      const uint32_t want = (l.flags & CFRK_LINK_TO_MINUS) ? 0u : CFRK_LINK_FROM_MINUS;
      const int64_t c = w.ptr[l.to], d = w.ptr[l.to + 1];             // (a checked target, a checked row)
      bool beaten = false;
      for (int64_t x = c; x < d && !beaten; ++x) {
        const cfrk_unitig_link m = w.links[x];
        beaten = (m.flags & CFRK_LINK_FROM_MINUS) == want && m.to != j && uw_beats(w, m.to, j, rj);
      }
      if (!beaten) return 0;
    }
    return CFRK_WEAK_CONNECTION;
  }
  for (int64_t t = a; t < b; ++t) {                     // j -> v; the siblings: v's in-row
    const uint32_t v = w.links[t].to;
    bool beaten = false;
    for (unsigned long long x = w.in_off[v]; x < w.in_off[v + 1] && !beaten; ++x) {
      const uint32_t s = w.in_src[x];
      beaten = s != j && uw_beats(w, s, j, rj);
    }
    if (!beaten) return 0;
  }
  for (unsigned long long t = w.in_off[j]; t < w.in_off[j + 1]; ++t) {          // u -> j; the siblings: u's targets
    const uint32_t u = w.in_src[t];
    bool beaten = false;
    for (int64_t x = w.ptr[u]; x < w.ptr[u + 1] && !beaten; ++x) {
      const uint32_t s = w.links[x].to;
      beaten = s != j && uw_beats(w, s, j, rj);
    }
    if (!beaten) return 0;
  }
  return CFRK_WEAK_CONNECTION;
}

template <bool CANON>
__global__ __launch_bounds__(256) void uw_decide_kernel(UWWork w) {
  if (w.ctr[UGC_ERR] != UG_NONE) return;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  uint32_t n_conn = 0, n_iso = 0, n_cand = 0;           // the wave's, over every turn of the loop (a lane does < 2^32 turns)
  // (whole waves turn together: the ballots below count a wave's finds)
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < w.nS; base += nthreads) {
    const uint64_t j = base + threadIdx.x;
    int kind = 0;
    bool cand = false;
    if (j < w.nS) {
      kind = uw_decide<CANON>(w, (uint32_t)j, cand);
      w.weak[j] = (uint8_t)kind;
    }
    n_conn += (uint32_t)__popcll(__ballot(kind == CFRK_WEAK_CONNECTION));
    n_iso += (uint32_t)__popcll(__ballot(kind == CFRK_WEAK_ISOLATED));
    n_cand += (uint32_t)__popcll(__ballot(cand));
  }
  if ((threadIdx.x & 63) == 0) {
    if (n_conn) atomicAdd(&w.ctr[UWC_CONN], (unsigned long long)n_conn);
    if (n_iso) atomicAdd(&w.ctr[UWC_ISO], (unsigned long long)n_iso);
    if (n_cand) atomicAdd(&w.ctr[UWC_CAND], (unsigned long long)n_cand);
  }
}

}  // namespace

// The rule on device arrays; 1 <= nS < 2^32.  Synchronises once: CFRK_ERR_LAYOUT naming the unitig, or *stats.
int cfrk_unitig_weak_launch(cfrk_ctx *ctx, const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr,
                            const cfrk_unitig_link *d_links, int64_t n_links, uint32_t max_kmers, uint32_t ratio_q8,
                            uint32_t iso_max_kmers, uint32_t iso_mean_q8, uint8_t *d_weak, cfrk_weak_stats *stats) {
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  const uint64_t n = (uint64_t)nS, in_n = canon ? 0 : n;
  size_t scan_tmp = 0;
  if (const int rc = ug_scan_bytes(ctx, canon, n, &scan_tmp)) return rc;
  Carve c;
  const size_t o_ctr = c.part(UWC_WORDS * 8), o_off = c.part(canon ? 0 : (in_n + 1) * 8), o_cur = c.part(in_n * 4),
               o_src = c.part(canon ? 0 : (size_t)n_links * 4), o_tmp = c.part(scan_tmp);
  void *base;
  if (const int rc = cfrk_pool_get(ctx, BUF_UNITIG_WEAK, c.end, &base)) return rc;
  UWWork w;
  w.rec = d_rec; w.ptr = d_link_ptr; w.links = d_links; w.nS = n; w.n_links = n_links;
  w.max_kmers = max_kmers; w.ratio_q8 = ratio_q8; w.iso_max_kmers = iso_max_kmers; w.iso_mean_q8 = iso_mean_q8; w.weak = d_weak;
  w.ctr = carve_at<unsigned long long>(base, o_ctr);
  w.in_off = carve_at<unsigned long long>(base, o_off);
  w.in_cur = carve_at<uint32_t>(base, o_cur);
  w.in_src = carve_at<uint32_t>(base, o_src);
  HIP_TRY(ctx, hipMemsetAsync(w.ctr + UWC_CONN, 0, (UWC_WORDS - UWC_CONN) * 8, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_weak, 0, n, ctx->stream));                    // every byte is written, whatever is refused
  const int grid = u_grid(ctx, n);
  if (const int rc = ug_check_launch(ctx, w, canon, grid, carve_at<void>(base, o_tmp), scan_tmp)) return rc;
  if (canon) hipLaunchKernelGGL(uw_decide_kernel<true>, dim3(grid), dim3(256), 0, ctx->stream, w);
  else hipLaunchKernelGGL(uw_decide_kernel<false>, dim3(grid), dim3(256), 0, ctx->stream, w);
  HIP_TRY(ctx, hipGetLastError());
  unsigned long long h[UWC_WORDS];
  HIP_TRY(ctx, hipMemcpyAsync(h, w.ctr, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (h[UWC_ERR] != UG_NONE) return ug_layout_error(ctx, h[UWC_ERR]);
  stats->connections = (int64_t)h[UWC_CONN];
  stats->isolated = (int64_t)h[UWC_ISO];
  stats->candidates = (int64_t)h[UWC_CAND];
  return CFRK_OK;
}
