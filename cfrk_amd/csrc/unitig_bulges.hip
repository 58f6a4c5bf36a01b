// unitig_bulges.hip -- the bulge rule: which arms run beside a CHAIN of better-supported unitigs between the same two
// oriented ends.  An error's arm is one unitig, but the true path beside it is cut by its neighbours' branch points, so the
// bubble rule (unitig_bubbles.hip), which compares single unitigs, rarely sees it.  A pure function of the compacted
// graph, like the tip and the bubble rule: the unitigs' records, the link CSR as cfrk_global_unitig_links wrote it, and
// the job's strand rule.  No sequence, no index.  The contract, with the order of the search, is in include/cfrk_abi.h
// ("Unitig bulges"); DESIGN 4.24 has the reasoning.
//
// The arrays are untrusted.  Passes, each a launch of its own on the context stream; every pass behind the check reads
// the error word first and does nothing when it is set, so that only checked rows are ever followed:
//   1-3 the check and, not canonical only, the in-rows: unitig_graph_dev.h, shared with the tip and the bubble rule
//   4 arm       one lane per unitig: the bubble rule's arm; an arm appends (j, src, dst) to a compact list
//   5 search    one lane per ARM of that list, so a wave is full of searches and not of non-arms: the depth-first search
//               from src, its stack in LDS ([depth][lane]: the path entry and the row cursor) -> pop, visits, the hops
//               into path_ptr; a popped arm appends itself to a second list
//   6 scan      hipCUB exclusive sum over path_ptr in place (only when paths are wanted)
//   -- the one synchronisation: the error word, the three counts and n_path --
//   7 fill      one lane per POPPED arm: the same search again (it is deterministic: it finds the same path), the path
//               into its row
// Every loop of the search is bounded by max_visits link examinations, max_hops <= 64 stack levels and the 16 links of a
// checked row.
#include "unitig_graph_dev.h"

namespace {

enum { UGB_ERR = UGC_ERR, UGB_ARMS, UGB_POP, UGB_UNDECIDED, UGB_WORDS };
constexpr int UGB_LANES = 64;         // one wave per workgroup: 64 x 64 x (4 + 1) bytes of stack = 20 KB of LDS

struct UGBArm { uint32_t j, src, dst; };  // src, dst: oriented unitigs, u << 1 | o

struct UGBWork : UGraph {
  uint32_t max_kmers, max_diff, max_hops, max_visits, ratio_q8;
  UGBArm *arms;                       // [nS]: the first ctr[UGB_ARMS] are written
  uint32_t *popped;                   // [nS]: indices into arms, the first ctr[UGB_POP] are written
  uint8_t *pop;                       // [nS], the caller's
  uint32_t *visits;                   // [nS], the caller's; may be NULL
  int64_t *path_ptr;                  // [nS + 1], the caller's; may be NULL
  uint32_t *path;                     // the caller's; the fill pass only
};

// ---- 4 arms -----------------------------------------------------------------------------------------------------
template <bool CANON>
__global__ __launch_bounds__(256) void ug_arm_list_kernel(UGBWork w) {
  if (w.ctr[UGC_ERR] != UG_NONE) return;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = tid; j < w.nS; j += nthreads) {
    const int64_t a = w.ptr[j], b = w.ptr[j + 1];
    uint32_t n_in = 0, n_out = 0, src = 0, dst = 0;
    if (CANON) {
      for (int64_t t = a; t < b; ++t) {
        const cfrk_unitig_link l = w.links[t];
        const uint32_t ov = (l.flags & CFRK_LINK_TO_MINUS) ? 1u : 0u;
        if (l.flags & CFRK_LINK_FROM_MINUS) { ++n_in; src = (l.to << 1) | (ov ^ 1u); }    // (j,-) -> (v,ov) mirrored
        else { ++n_out; dst = (l.to << 1) | ov; }
      }
    } else {
      n_out = (uint32_t)(b - a);
      n_in = (uint32_t)(w.in_off[j + 1] - w.in_off[j]);
      if (n_out == 1) dst = w.links[a].to << 1;
      if (n_in == 1) src = w.in_src[w.in_off[j]] << 1;
    }
    const cfrk_unitig r = w.rec[j];
    if ((r.flags & CFRK_UNITIG_CIRCULAR) || r.n_kmers > w.max_kmers || n_in != 1 || n_out != 1 || (src >> 1) == (uint32_t)j ||
        (dst >> 1) == (uint32_t)j)
      continue;
    UGBArm x;
    x.j = (uint32_t)j; x.src = src; x.dst = dst;
    w.arms[atomicAdd(&w.ctr[UGB_ARMS], 1ull)] = x;      // (one per unitig at most: below nS)
  }
}

// ---- 5, 7 the search --------------------------------------------------------------------------------------------
struct UGBFound { uint32_t hops, visits; bool found; };

// The search for arm x by the lane that owns column `lane` of the stack.  kc < 2^64, n < 2^32, ratio_q8 <= 2^16: every
// product stays below 2^113.  A path's length sum stays below 65 * 2^32.
template <bool CANON>
__device__ __forceinline__ UGBFound ugb_search(const UGBWork &w, const UGBArm &x, uint32_t (*s_path)[UGB_LANES], uint8_t (*s_cur)[UGB_LANES],
                                               int lane) {
  const cfrk_unitig rj = w.rec[x.j];
  const int64_t lo = (int64_t)rj.n_kmers - (int64_t)w.max_diff, hi = (int64_t)rj.n_kmers + (int64_t)w.max_diff;
  const uint32_t us = x.src >> 1, ut = x.dst >> 1;
  UGBFound f;
  f.hops = 0; f.visits = 0; f.found = false;
  uint32_t d = 0, cur = x.src, c = 0;                   // the depth, the oriented unitig whose row is walked, the cursor in it
  int64_t total = 0;
  int64_t a = w.ptr[us], b = w.ptr[us + 1];             // (a checked target's checked row: at most 16 links)
  for (;;) {
    if (a + c >= b) {                                   // this row is done: back to the one above, or the search is over
      if (d == 0) break;
      --d;
      total -= (int64_t)w.rec[s_path[d][lane] >> 1].n_kmers;
      c = s_cur[d][lane];
      cur = d ? s_path[d - 1][lane] : x.src;
      a = w.ptr[cur >> 1]; b = w.ptr[(cur >> 1) + 1];
      continue;
    }
    const cfrk_unitig_link l = w.links[a + c];
    ++c;
    if (CANON && ((l.flags & CFRK_LINK_FROM_MINUS) ? 1u : 0u) != (cur & 1u)) continue;   // not a link of out(cur)
    if (f.visits == w.max_visits) { f.visits = w.max_visits + 1; break; }                // undecided
    ++f.visits;
    const uint32_t y = (l.to << 1) | ((CANON && (l.flags & CFRK_LINK_TO_MINUS)) ? 1u : 0u);
    if (y == x.dst && d >= 1 && total >= lo) { f.found = true; f.hops = d; break; }
    if (l.to == x.j || l.to == us || l.to == ut || d >= w.max_hops) continue;
    const cfrk_unitig ry = w.rec[l.to];
    if (total + (int64_t)ry.n_kmers > hi) continue;
    const u128 p = (u128)ry.kc * rj.n_kmers, q = (u128)rj.kc * ry.n_kmers;
    if ((p << 8) < q * w.ratio_q8 || !(p > q || (p == q && l.to < x.j))) continue;       // not eligible
    bool on_path = false;
    for (uint32_t i = 0; i < d; ++i) on_path |= (s_path[i][lane] >> 1) == l.to;
    if (on_path) continue;
    s_path[d][lane] = y;                                // (d < max_hops <= 64)
    s_cur[d][lane] = (uint8_t)c;                        // (c <= 16)
    ++d;
    total += (int64_t)ry.n_kmers;
    cur = y; c = 0;
    a = w.ptr[l.to]; b = w.ptr[l.to + 1];
  }
  return f;
}

template <bool CANON>
__global__ __launch_bounds__(UGB_LANES) void ug_bulge_search_kernel(UGBWork w) {
  __shared__ uint32_t s_path[CFRK_BULGE_MAX_HOPS][UGB_LANES];
  __shared__ uint8_t s_cur[CFRK_BULGE_MAX_HOPS][UGB_LANES];
  if (w.ctr[UGC_ERR] != UG_NONE) return;
  const uint64_t n_arms = w.ctr[UGB_ARMS];
  const int lane = (int)threadIdx.x;
  // (whole waves turn together: the ballot below counts a wave's undecided arms)
  for (uint64_t base = (uint64_t)blockIdx.x * UGB_LANES; base < n_arms; base += (uint64_t)gridDim.x * UGB_LANES) {
    const uint64_t i = base + (uint64_t)lane;
    bool undecided = false;
    if (i < n_arms) {
      const UGBArm x = w.arms[i];
      const UGBFound f = ugb_search<CANON>(w, x, s_path, s_cur, lane);
      undecided = f.visits > w.max_visits;
      if (w.visits) w.visits[x.j] = f.visits;
      if (f.found) {
        w.pop[x.j] = 1;
        if (w.path_ptr) w.path_ptr[x.j] = (int64_t)f.hops;
        w.popped[atomicAdd(&w.ctr[UGB_POP], 1ull)] = (uint32_t)i;     // (one per arm at most: below nS)
      }
    }
    const unsigned long long m = __ballot(undecided);
    if (lane == 0 && m) atomicAdd(&w.ctr[UGB_UNDECIDED], (unsigned long long)__popcll(m));
  }
}

template <bool CANON>
__global__ __launch_bounds__(UGB_LANES) void ug_bulge_fill_kernel(UGBWork w) {
  __shared__ uint32_t s_path[CFRK_BULGE_MAX_HOPS][UGB_LANES];
  __shared__ uint8_t s_cur[CFRK_BULGE_MAX_HOPS][UGB_LANES];
  if (w.ctr[UGC_ERR] != UG_NONE) return;
  const uint64_t n_pop = w.ctr[UGB_POP];
  const int lane = (int)threadIdx.x;
  for (uint64_t i = (uint64_t)blockIdx.x * UGB_LANES + (uint64_t)lane; i < n_pop; i += (uint64_t)gridDim.x * UGB_LANES) {
    const UGBArm x = w.arms[w.popped[i]];
    const UGBFound f = ugb_search<CANON>(w, x, s_path, s_cur, lane);
    const int64_t at = w.path_ptr[x.j], end = w.path_ptr[x.j + 1];
    if (!f.found) continue;                             // (never: the search pass found it)
    for (uint32_t h = 0; h < f.hops && at + (int64_t)h < end; ++h) w.path[at + h] = s_path[h][lane];
  }
}

// the pool slot carved for nS unitigs: the same offsets for the search and for the fill pass behind it
int ugb_carve(cfrk_ctx *ctx, bool canon, uint64_t n, int64_t n_links, bool want_paths, UGBWork *w, void **scan_tmp, size_t *in_scan,
              size_t *path_scan) {
  *in_scan = *path_scan = 0;
  if (const int rc = ug_scan_bytes(ctx, canon, n, in_scan)) return rc;
  if (want_paths) HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, *path_scan, (int64_t *)nullptr, (size_t)(n + 1), ctx->stream));
  const uint64_t in_n = canon ? 0 : n;
  Carve c;
  const size_t o_ctr = c.part(UGB_WORDS * 8), o_arms = c.part(n * sizeof(UGBArm)), o_popped = c.part(n * 4),
               o_off = c.part(canon ? 0 : (in_n + 1) * 8), o_cur = c.part(in_n * 4), o_src = c.part(canon ? 0 : (size_t)n_links * 4),
               o_tmp = c.part(std::max(*in_scan, *path_scan));
  void *base;
  if (const int rc = cfrk_pool_get(ctx, BUF_UNITIG_BULGES, c.end, &base)) return rc;
  w->ctr = carve_at<unsigned long long>(base, o_ctr);
  w->arms = carve_at<UGBArm>(base, o_arms);
  w->popped = carve_at<uint32_t>(base, o_popped);
  w->in_off = carve_at<unsigned long long>(base, o_off);
  w->in_cur = carve_at<uint32_t>(base, o_cur);
  w->in_src = carve_at<uint32_t>(base, o_src);
  *scan_tmp = carve_at<void>(base, o_tmp);
  return CFRK_OK;
}

void ugb_fill_work(UGBWork *w, const cfrk_unitig *d_rec, uint64_t n, const int64_t *d_link_ptr, const cfrk_unitig_link *d_links, int64_t n_links,
                   const cfrk_bulge_params &p) {
  w->rec = d_rec; w->ptr = d_link_ptr; w->links = d_links; w->nS = n; w->n_links = n_links;
  w->max_kmers = p.max_kmers; w->max_diff = p.max_diff; w->max_hops = std::min<uint32_t>(p.max_hops, CFRK_BULGE_MAX_HOPS);
  w->max_visits = p.max_visits; w->ratio_q8 = p.ratio_q8;
}

// one wave per workgroup, 20 KB of LDS each: 8 workgroups share a CU's 160 KB
int ugb_grid(const cfrk_ctx *ctx, uint64_t items) {
  const uint64_t want = (items + UGB_LANES - 1) / UGB_LANES;
  return (int)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)ctx->num_cus * 8));
}

}  // namespace

// The rule on device arrays; 1 <= nS < 2^31.  Synchronises once: CFRK_ERR_LAYOUT naming the unitig, or the counts and,
// when d_path_ptr is given, *n_path = d_path_ptr[nS].
int cfrk_unitig_bulges_search(cfrk_ctx *ctx, const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr,
                              const cfrk_unitig_link *d_links, int64_t n_links, const cfrk_bulge_params &p, uint8_t *d_pop,
                              uint32_t *d_visits, int64_t *d_path_ptr, cfrk_bulge_stats *stats, int64_t *n_path) {
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  const uint64_t n = (uint64_t)nS;
  UGBWork w;
  void *scan_tmp;
  size_t in_scan, path_scan;
  if (const int rc = ugb_carve(ctx, canon, n, n_links, d_path_ptr != nullptr, &w, &scan_tmp, &in_scan, &path_scan)) return rc;
  ugb_fill_work(&w, d_rec, n, d_link_ptr, d_links, n_links, p);
  w.pop = d_pop; w.visits = d_visits; w.path_ptr = d_path_ptr; w.path = nullptr;
  HIP_TRY(ctx, hipMemsetAsync(w.ctr + UGB_ARMS, 0, (UGB_WORDS - UGB_ARMS) * 8, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_pop, 0, n, ctx->stream));                     // every byte is written, whatever is refused
  if (d_visits) HIP_TRY(ctx, hipMemsetAsync(d_visits, 0, n * 4, ctx->stream));
  if (d_path_ptr) HIP_TRY(ctx, hipMemsetAsync(d_path_ptr, 0, (n + 1) * 8, ctx->stream));
  const int grid = u_grid(ctx, n), sgrid = ugb_grid(ctx, n);
  if (const int rc = ug_check_launch(ctx, w, canon, grid, scan_tmp, in_scan)) return rc;
  if (canon) {
    hipLaunchKernelGGL(ug_arm_list_kernel<true>, dim3(grid), dim3(256), 0, ctx->stream, w);
    hipLaunchKernelGGL(ug_bulge_search_kernel<true>, dim3(sgrid), dim3(UGB_LANES), 0, ctx->stream, w);
  } else {
    hipLaunchKernelGGL(ug_arm_list_kernel<false>, dim3(grid), dim3(256), 0, ctx->stream, w);
    hipLaunchKernelGGL(ug_bulge_search_kernel<false>, dim3(sgrid), dim3(UGB_LANES), 0, ctx->stream, w);
  }
  HIP_TRY(ctx, hipGetLastError());
  unsigned long long h[UGB_WORDS];
  int64_t total = 0;
  if (d_path_ptr) {
    HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(scan_tmp, path_scan, d_path_ptr, (size_t)(n + 1), ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&total, d_path_ptr + n, 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipMemcpyAsync(h, w.ctr, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (h[UGB_ERR] != UG_NONE) return ug_layout_error(ctx, h[UGB_ERR]);
  stats->arms = (int64_t)h[UGB_ARMS];
  stats->popped = (int64_t)h[UGB_POP];
  stats->undecided = (int64_t)h[UGB_UNDECIDED];
  *n_path = total;
  return CFRK_OK;
}

// The fill pass behind a search of the same arguments that returned CFRK_OK with n_path > 0: the rows of d_path_ptr into
// d_path[n_path].  Returns with the kernel enqueued.
int cfrk_unitig_bulges_fill(cfrk_ctx *ctx, const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr,
                            const cfrk_unitig_link *d_links, int64_t n_links, const cfrk_bulge_params &p, int64_t n_popped,
                            const int64_t *d_path_ptr, uint32_t *d_path) {
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  UGBWork w;
  void *scan_tmp;
  size_t in_scan, path_scan;
  if (const int rc = ugb_carve(ctx, canon, (uint64_t)nS, n_links, true, &w, &scan_tmp, &in_scan, &path_scan)) return rc;
  ugb_fill_work(&w, d_rec, (uint64_t)nS, d_link_ptr, d_links, n_links, p);
  w.pop = nullptr; w.visits = nullptr; w.path_ptr = const_cast<int64_t *>(d_path_ptr); w.path = d_path;
  const int grid = ugb_grid(ctx, (uint64_t)n_popped);
  if (canon) hipLaunchKernelGGL(ug_bulge_fill_kernel<true>, dim3(grid), dim3(UGB_LANES), 0, ctx->stream, w);
  else hipLaunchKernelGGL(ug_bulge_fill_kernel<false>, dim3(grid), dim3(UGB_LANES), 0, ctx->stream, w);
  HIP_TRY(ctx, hipGetLastError());
  return CFRK_OK;
}
