// unitig_bubbles.hip -- the bubble rule: which unitigs are the weaker of two parallel single-unitig paths between the same
// two oriented unitigs (a substitution or a small indel in the middle of a read; with balanced coverage a heterozygous
// site).  A pure function of the compacted graph, like the tip rule: the unitigs' records, the link CSR as
// cfrk_global_unitig_links wrote it, and the job's strand rule.  No sequence, no index.  The contract is in
// include/cfrk_abi.h ("Unitig bubbles"); DESIGN 4.23 has the reasoning.
//
// The arrays are untrusted.  Passes, each a launch of its own on the context stream; every pass behind the check reads
// the error word first and does nothing when it is set, so that only checked rows are ever followed:
//   1-3 the check and, not canonical only, the in-rows: unitig_graph_dev.h, shared with the tip rule
//   4 arm       one lane per unitig: not circular, n_kmers <= max_kmers, |in(j,+)| = |out(j,+)| = 1, neither end on j
//               itself -> the arm byte and the record (src << 1 | o, dst << 1 | o)
//   5 decide    one lane per unitig: an arm's src has <= 16 links in its row; every target that is another arm, read in
//               the orientation the link enters it, with the same src and dst and a length within max_diff, that BEATS
//               the arm in 128 bits; the best-ranked of them is the partner
//   -- the one synchronisation: the error word and n_pop --
// In a canonical job the rows hold every link's mirror, so in(j,+) is the row's FROM_MINUS links mirrored; (s,-) is an
// arm iff (s,+) is, with src(s,-) = mirror(dst(s,+)) and dst(s,-) = mirror(src(s,+)): one record per unitig.
#include "unitig_graph_dev.h"

namespace {

enum { UBC_ERR = UGC_ERR, UBC_POP, UBC_WORDS };
constexpr uint32_t UB_NONE = 0xFFFFFFFFu;

struct UBArm { uint32_t src, dst; };  // oriented unitigs, u << 1 | o; 8 bytes

struct UBWork : UGraph {
  uint32_t max_kmers, max_diff, ratio_q8;
  uint8_t *arm;                       // [nS]
  UBArm *arec;                        // [nS], written for every unitig (both words UB_NONE when it is no arm)
  uint8_t *pop;                       // [nS], the caller's
  uint32_t *partner;                  // [nS], the caller's; may be NULL
};

// ---- 4 arms -----------------------------------------------------------------------------------------------------
template <bool CANON>
__global__ __launch_bounds__(256) void ub_arm_kernel(UBWork w) {
  if (w.ctr[UGC_ERR] != UG_NONE) return;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = tid; j < w.nS; j += nthreads) {
    const int64_t a = w.ptr[j], b = w.ptr[j + 1];
    uint32_t n_in = 0, n_out = 0, src = UB_NONE, dst = UB_NONE;
    uint32_t us = 0, ud = 0;          // the unitigs of src and dst
    if (CANON) {
      for (int64_t t = a; t < b; ++t) {
        const cfrk_unitig_link l = w.links[t];
        const uint32_t ov = (l.flags & CFRK_LINK_TO_MINUS) ? 1u : 0u;
        if (l.flags & CFRK_LINK_FROM_MINUS) { ++n_in; us = l.to; src = (l.to << 1) | (ov ^ 1u); }   // (j,-) -> (v,ov) mirrored
        else { ++n_out; ud = l.to; dst = (l.to << 1) | ov; }
      }
    } else {
      n_out = (uint32_t)(b - a);
      n_in = (uint32_t)(w.in_off[j + 1] - w.in_off[j]);
      if (n_out == 1) { ud = w.links[a].to; dst = ud << 1; }
      if (n_in == 1) { us = w.in_src[w.in_off[j]]; src = us << 1; }
    }
    const cfrk_unitig r = w.rec[j];
    const bool arm = !(r.flags & CFRK_UNITIG_CIRCULAR) && r.n_kmers <= w.max_kmers && n_in == 1 && n_out == 1 && us != (uint32_t)j &&
                     ud != (uint32_t)j;
    w.arm[j] = arm ? 1 : 0;
    UBArm rec;
    rec.src = arm ? src : UB_NONE;
    rec.dst = arm ? dst : UB_NONE;
    w.arec[j] = rec;
  }
}

// ---- 5 decide ---------------------------------------------------------------------------------------------------
// kc < 2^64, n < 2^32, ratio_q8 <= 2^16: every product stays below 2^113.
struct UBBest { uint32_t s, p; cfrk_unitig r; };

// arm (s,p), another unitig than j and a target of src(x): is it parallel to x = (j,+), does it beat it, is it the best so far?
__device__ __forceinline__ void ub_try(const UBWork &w, uint32_t j, const cfrk_unitig &rj, const UBArm &x, uint32_t s, uint32_t p,
                                       UBBest &best) {
  if (s == j || !w.arm[s]) return;
  const UBArm y = w.arec[s];
  const uint32_t ysrc = p ? (y.dst ^ 1u) : y.src, ydst = p ? (y.src ^ 1u) : y.dst;
  if (ysrc != x.src || ydst != x.dst) return;
  const cfrk_unitig rs = w.rec[s];
  const uint32_t diff = rs.n_kmers > rj.n_kmers ? rs.n_kmers - rj.n_kmers : rj.n_kmers - rs.n_kmers;
  if (diff > w.max_diff) return;
  const u128 a = (u128)rs.kc * rj.n_kmers, b = (u128)rj.kc * rs.n_kmers;
  if ((a << 8) < b * w.ratio_q8) return;
  if (!(a > b || (a == b && s < j))) return;            // s ranks above j
  if (best.s != UB_NONE) {
    if (best.s == s) { if (p < best.p) best.p = p; return; }                  // both orientations of one s: p = 0
    const u128 c = (u128)rs.kc * best.r.n_kmers, d = (u128)best.r.kc * rs.n_kmers;
    if (!(c > d || (c == d && s < best.s))) return;     // the best so far ranks above s
  }
  best.s = s; best.p = p; best.r = rs;
}

template <bool CANON>
__device__ __forceinline__ uint32_t ub_partner(const UBWork &w, uint32_t j) {
  const cfrk_unitig rj = w.rec[j];
  const UBArm x = w.arec[j];
  const uint32_t u = x.src >> 1;                        // (a checked target: below nS)
  const int64_t a = w.ptr[u], b = w.ptr[u + 1];         // (a checked row: at most 16 links)
  UBBest best;
  best.s = UB_NONE; best.p = 0; best.r = rj;
  for (int64_t t = a; t < b; ++t) {
    const cfrk_unitig_link l = w.links[t];
    if (CANON) {
      if (((l.flags & CFRK_LINK_FROM_MINUS) ? 1u : 0u) != (x.src & 1u)) continue;
      ub_try(w, j, rj, x, l.to, (l.flags & CFRK_LINK_TO_MINUS) ? 1u : 0u, best);
    } else {
      ub_try(w, j, rj, x, l.to, 0u, best);
    }
  }
  return best.s == UB_NONE ? UB_NONE : ((best.s << 1) | best.p);
}

template <bool CANON>
__global__ __launch_bounds__(256) void ub_decide_kernel(UBWork w) {
  if (w.ctr[UGC_ERR] != UG_NONE) return;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  // (whole waves turn together: the ballot below counts a wave's pops)
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < w.nS; base += nthreads) {
    const uint64_t j = base + threadIdx.x;
    bool pop = false;
    if (j < w.nS) {
      const uint32_t with = w.arm[j] ? ub_partner<CANON>(w, (uint32_t)j) : UB_NONE;
      pop = with != UB_NONE;
      w.pop[j] = pop ? 1 : 0;
      if (w.partner) w.partner[j] = with;
    }
    const unsigned long long m = __ballot(pop);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&w.ctr[UBC_POP], (unsigned long long)__popcll(m));
  }
}

}  // namespace

// The rule on device arrays; 1 <= nS < 2^31.  Synchronises once: CFRK_ERR_LAYOUT naming the unitig, or *n_pop.
int cfrk_unitig_bubbles_launch(cfrk_ctx *ctx, const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr,
                               const cfrk_unitig_link *d_links, int64_t n_links, uint32_t max_kmers, uint32_t max_diff,
                               uint32_t ratio_q8, uint8_t *d_pop, uint32_t *d_partner, int64_t *n_pop) {
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  const uint64_t n = (uint64_t)nS, in_n = canon ? 0 : n;
  size_t scan_tmp = 0;
  if (const int rc = ug_scan_bytes(ctx, canon, n, &scan_tmp)) return rc;
  Carve c;
  const size_t o_ctr = c.part(UBC_WORDS * 8), o_arm = c.part(n), o_arec = c.part(n * sizeof(UBArm)),
               o_off = c.part(canon ? 0 : (in_n + 1) * 8), o_cur = c.part(in_n * 4), o_src = c.part(canon ? 0 : (size_t)n_links * 4),
               o_tmp = c.part(scan_tmp);
  void *base;
  if (const int rc = cfrk_pool_get(ctx, BUF_UNITIG_BUBBLES, c.end, &base)) return rc;
  UBWork w;
  w.rec = d_rec; w.ptr = d_link_ptr; w.links = d_links; w.nS = n; w.n_links = n_links;
  w.max_kmers = max_kmers; w.max_diff = max_diff; w.ratio_q8 = ratio_q8; w.pop = d_pop; w.partner = d_partner;
  w.ctr = carve_at<unsigned long long>(base, o_ctr);
  w.arm = carve_at<uint8_t>(base, o_arm);
  w.arec = carve_at<UBArm>(base, o_arec);
  w.in_off = carve_at<unsigned long long>(base, o_off);
  w.in_cur = carve_at<uint32_t>(base, o_cur);
  w.in_src = carve_at<uint32_t>(base, o_src);
  HIP_TRY(ctx, hipMemsetAsync(w.ctr + UBC_POP, 0, 8, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_pop, 0, n, ctx->stream));                     // every byte is written, whatever is refused
  if (d_partner) HIP_TRY(ctx, hipMemsetAsync(d_partner, 0xFF, n * 4, ctx->stream));
  const int grid = u_grid(ctx, n);
  if (const int rc = ug_check_launch(ctx, w, canon, grid, carve_at<void>(base, o_tmp), scan_tmp)) return rc;
  if (canon) {
    hipLaunchKernelGGL(ub_arm_kernel<true>, dim3(grid), dim3(256), 0, ctx->stream, w);
    hipLaunchKernelGGL(ub_decide_kernel<true>, dim3(grid), dim3(256), 0, ctx->stream, w);
  } else {
    hipLaunchKernelGGL(ub_arm_kernel<false>, dim3(grid), dim3(256), 0, ctx->stream, w);
    hipLaunchKernelGGL(ub_decide_kernel<false>, dim3(grid), dim3(256), 0, ctx->stream, w);
  }
  HIP_TRY(ctx, hipGetLastError());
  unsigned long long h[UBC_WORDS];
  HIP_TRY(ctx, hipMemcpyAsync(h, w.ctr, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (h[UBC_ERR] != UG_NONE) return ug_layout_error(ctx, h[UBC_ERR]);
  *n_pop = (int64_t)h[UBC_POP];
  return CFRK_OK;
}
