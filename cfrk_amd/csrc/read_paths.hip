// read_paths.hip -- reads threaded through the unitig graph: the hits of a read (cfrk_global_read_hits) joined across
// links into paths, and the number of reads that walk every link.  A pure function of the hit CSR, the unitigs' n_kmers,
// the link CSR (or any sub-CSR of it) and the job's strand rule: no sequence, no index, no position map.  The contract is
// in include/cfrk_abi.h ("Read paths and link support"); DESIGN 4.26 has the reasoning.
//
// The arrays are untrusted.  The work is balanced by HITS: one lane per hit in every pass that touches hits, so a read of
// 10^5 hits costs what its hits cost; no lane's work grows with a read's hit count or a path's length (the only loops
// are the <= 16 links of a checked row and a binary search in hit_ptr, <= 64 steps).  Passes, each a launch of its own on
// the context stream; every pass behind the checks reads the error words first and does nothing when one is set:
//   1   the row check (not canonical: with the in-degrees it counts, without the in-rows): unitig_graph_dev.h
//   2   mark    one lane per read: hit_ptr[i] <= hit_ptr[i + 1] inside [0, n_hits], 0 at i = 0; flags the first hit of a
//               row that is not empty
//   3   hits    one lane per hit: unitig < nS, n_windows > 0, off + n_windows <= n_kmers.  A pass of its own in front
//               of the join, so that support[] is untouched whenever anything is refused
//   4   join    one lane per hit: unless flagged, (a)-(c) against hit h - 1 and the <= 16 links of its unitig for (d);
//               the start flag; the atomic add to support[r]; the four counters, summed per wave over the whole launch
//   5   scan    hipCUB exclusive sum over the start flags, in place: the number of the path a hit lies in
//   6   rows    one lane per read: path_ptr[i] = scan[hit_ptr[i]] (empty rows included)
//   -- the one synchronisation: the two error words, n_paths and the statistics --
//   7   events  one lane per hit: a start writes its path's first hit and read_off, an end its last hit and last window
//   8   finish  one lane per path: n_hits and n_windows from the two events, hit_first relative to the read's row
// support[] takes one plain no-return atomic add per step: adders spread over the links as the reads spread over the
// graph (DESIGN 4.26 has the measurement).
#include "unitig_graph_dev.h"

namespace {

enum { RPC_ERR = UGC_ERR, RPC_HIT_ERR, RPC_PATHS, RPC_STEPS, RPC_GAPS, RPC_UNLINKED, RPC_WORDS };
// hit error word = read << 8 | why, kept with an atomic minimum: the first offending read
enum { RPE_PTR = 1, RPE_UNITIG, RPE_EMPTY, RPE_PAST };

struct RPWork : UGraph {
  const int64_t *hit_ptr;
  const cfrk_read_hit *hits;
  uint64_t nR, n_hits;
  uint32_t *scan;                     // [n_hits + 1]: first-hit flags, start flags, then their exclusive sums
  int64_t *path_ptr;
  uint32_t *paths;                    // rows of cfrk_read_path as words: no alignment beyond 4 bytes is asked for
  uint64_t n_paths;
  uint32_t *support;
};

enum { RP_HIT_FIRST = 0, RP_N_HITS, RP_READ_OFF, RP_N_WINDOWS, RP_ROW_WORDS };

__device__ __forceinline__ bool rp_refused(const RPWork &w) {
  return w.ctr[RPC_ERR] != UG_NONE || w.ctr[RPC_HIT_ERR] != UG_NONE;
}

// the hits that lie in a row (hit_ptr is checked by then)
__device__ __forceinline__ uint64_t rp_total(const RPWork &w) { return w.nR ? (uint64_t)w.hit_ptr[w.nR] : 0; }

// the read whose row holds hit h: the last i with hit_ptr[i] <= h (hit_ptr ascending from 0: the mark pass refuses
// anything else); bounded by log2(nR) whatever hit_ptr holds
__device__ __forceinline__ uint64_t rp_read_of(const RPWork &w, uint64_t h) {
  uint64_t lo = 0, hi = w.nR;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    const int64_t p = w.hit_ptr[mid];
    if (p >= 0 && (uint64_t)p <= h) lo = mid + 1; else hi = mid;
  }
  return lo ? lo - 1 : 0;
}

// ---- 2 mark -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rp_mark_kernel(RPWork w) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  if (w.nR == 0 && tid == 0 && w.hit_ptr[0] != 0) atomicMin(&w.ctr[RPC_HIT_ERR], (unsigned long long)RPE_PTR);     // (no row: "read 0")
  for (uint64_t i = tid; i < w.nR; i += nthreads) {
    const int64_t a = w.hit_ptr[i], b = w.hit_ptr[i + 1];
    if ((i == 0 && a != 0) || a < 0 || b < a || (uint64_t)b > w.n_hits)
      atomicMin(&w.ctr[RPC_HIT_ERR], (unsigned long long)((i << 8) | RPE_PTR));
    else if (a < b) w.scan[a] = 1u;                     // (a < b <= n_hits)
  }
}

// ---- 3 hits -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rp_hits_kernel(RPWork w) {
  // hit_ptr is refused: no row to name.  Only what the mark pass wrote counts: this kernel stores the other reasons into
  // the same word, and a block that starts late must still look at its hits, or a later read could be the one named
  if ((w.ctr[RPC_HIT_ERR] & 255) == RPE_PTR) return;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t total = rp_total(w);
  for (uint64_t h = tid; h < total; h += nthreads) {
    const cfrk_read_hit x = w.hits[h];
    int why = 0;
    if (x.unitig >= w.nS) why = RPE_UNITIG;
    else if (x.n_windows == 0) why = RPE_EMPTY;
    else if ((uint64_t)(x.unitig_at >> 1) + x.n_windows > w.rec[x.unitig].n_kmers) why = RPE_PAST;
    if (why) atomicMin(&w.ctr[RPC_HIT_ERR], (unsigned long long)((rp_read_of(w, h) << 8) | (uint64_t)why));
  }
}

// ---- 4 join -----------------------------------------------------------------------------------------------------
// the link that joins checked hits p and c, window-adjacent in one read: its index in links[], -1 when there is none
__device__ __forceinline__ int64_t rp_step(const RPWork &w, const cfrk_read_hit &p, const cfrk_read_hit &c) {
  const uint32_t m = p.unitig_at & 1u, n = w.rec[p.unitig].n_kmers;
  const uint32_t pl = m ? (p.unitig_at >> 1) : (p.unitig_at >> 1) + p.n_windows - 1;
  if (pl != (m ? 0u : n - 1)) return -1;                // (b) does not leave at the end
  const uint32_t m2 = c.unitig_at & 1u, n2 = w.rec[c.unitig].n_kmers;
  const uint32_t pf = m2 ? (c.unitig_at >> 1) + c.n_windows - 1 : (c.unitig_at >> 1);
  if (pf != (m2 ? n2 - 1 : 0u)) return -1;              // (c) does not enter at the head
  const uint32_t want = (m ? (uint32_t)CFRK_LINK_FROM_MINUS : 0u) | (m2 ? (uint32_t)CFRK_LINK_TO_MINUS : 0u);
  const int64_t a = w.ptr[p.unitig], b = w.ptr[p.unitig + 1];     // (a checked row: at most 16 links)
  for (int64_t t = a; t < b; ++t) {
    const cfrk_unitig_link l = w.links[t];
    if (l.to == c.unitig && l.flags == want) return t;  // (d): the first such row
  }
  return -1;
}

__global__ __launch_bounds__(256) void rp_join_kernel(RPWork w) {
  if (rp_refused(w)) return;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t total = rp_total(w);
  unsigned long long n_start = 0, n_step = 0, n_gap = 0, n_unlinked = 0;      // this wave's events, every lane the same
  // (whole waves turn together: the ballots below count a wave's events)
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < total; base += nthreads) {
    const uint64_t h = base + threadIdx.x;
    bool start = false, step = false, gap = false, unlinked = false;
    if (h < total) {
      if (w.scan[h] != 0) start = true;                 // the first hit of its read (h > 0 for every other hit)
      else {
        const cfrk_read_hit p = w.hits[h - 1], c = w.hits[h];
        if ((uint64_t)p.read_off + p.n_windows != c.read_off) gap = true;       // (a)
        else {
          const int64_t r = rp_step(w, p, c);
          if (r < 0) unlinked = true;
          else {
            step = true;
            if (w.support) atomicAdd(&w.support[r], 1u);
          }
        }
        start = !step;
      }
      w.scan[h] = start ? 1u : 0u;
    }
    n_start += (unsigned)__popcll(__ballot(start));
    n_step += (unsigned)__popcll(__ballot(step));
    n_gap += (unsigned)__popcll(__ballot(gap));
    n_unlinked += (unsigned)__popcll(__ballot(unlinked));
  }
  // one add per wave and counter for the whole launch: an add per wave and turn is 5 * 10^6 adds to one word in the 1 %
  // case, and that word then bounds the kernel
  if ((threadIdx.x & 63) == 0) {
    if (n_start) atomicAdd(&w.ctr[RPC_PATHS], n_start);
    if (n_step) atomicAdd(&w.ctr[RPC_STEPS], n_step);
    if (n_gap) atomicAdd(&w.ctr[RPC_GAPS], n_gap);
    if (n_unlinked) atomicAdd(&w.ctr[RPC_UNLINKED], n_unlinked);
  }
}

// ---- 6 rows -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rp_rows_kernel(RPWork w) {
  if (rp_refused(w)) return;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = tid; i <= w.nR; i += nthreads) w.path_ptr[i] = (int64_t)w.scan[w.hit_ptr[i]];
}

// ---- 7 events ---------------------------------------------------------------------------------------------------
// scan[h] = the starts before h, scan[total] = n_paths.  Hit h starts path scan[h] iff scan[h + 1] != scan[h]; it ends
// path scan[h + 1] - 1 iff it is the last hit of all or h + 1 is a start.  The end's lane leaves the index behind the
// path's last hit and the window behind its last window for the finish pass.
__global__ __launch_bounds__(256) void rp_events_kernel(RPWork w) {
  if (rp_refused(w)) return;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t total = rp_total(w);
  for (uint64_t h = tid; h < total; h += nthreads) {
    const uint32_t s = w.scan[h], e = w.scan[h + 1];
    const bool ends = h + 1 == total || w.scan[h + 2] != e;       // (h + 2 <= total <= n_hits)
    if (s == e && !ends) continue;
    const cfrk_read_hit x = w.hits[h];
    if (s != e && s < w.n_paths) {
      uint32_t *row = w.paths + (uint64_t)s * RP_ROW_WORDS;
      row[RP_HIT_FIRST] = (uint32_t)h;
      row[RP_READ_OFF] = x.read_off;
    }
    if (ends && e != 0 && (uint64_t)e - 1 < w.n_paths) {
      uint32_t *row = w.paths + ((uint64_t)e - 1) * RP_ROW_WORDS;
      row[RP_N_HITS] = (uint32_t)(h + 1);
      row[RP_N_WINDOWS] = x.read_off + x.n_windows;
    }
  }
}

// ---- 8 finish ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rp_finish_kernel(RPWork w) {
  if (rp_refused(w)) return;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t p = tid; p < w.n_paths; p += nthreads) {
    uint32_t *row = w.paths + p * RP_ROW_WORDS;
    const uint32_t first = row[RP_HIT_FIRST];
    row[RP_HIT_FIRST] = (uint32_t)((uint64_t)first - (uint64_t)w.hit_ptr[rp_read_of(w, first)]);
    row[RP_N_HITS] -= first;
    row[RP_N_WINDOWS] -= row[RP_READ_OFF];             // (the windows of joined hits are contiguous by (a))
  }
}

struct RPPlan {
  size_t o_ctr, o_scan, o_off, o_tmp, bytes, scan_tmp;
};

int rp_plan(cfrk_ctx *ctx, bool canon, uint64_t nS, uint64_t n_hits, RPPlan *p) {
  p->scan_tmp = 0;
  HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, p->scan_tmp, (uint32_t *)nullptr, (size_t)(n_hits + 1), ctx->stream));
  Carve c;
  p->o_ctr = c.part(RPC_WORDS * 8);
  p->o_scan = c.part((size_t)(n_hits + 1) * 4);
  p->o_off = c.part(canon ? 0 : (size_t)(nS + 1) * 8);            // not canonical: the in-degrees the row check counts
  p->o_tmp = c.part(p->scan_tmp);
  p->bytes = c.end;
  return CFRK_OK;
}

void rp_work(RPWork *w, void *base, const RPPlan &p, const cfrk_read_paths_in &in) {
  w->rec = in.d_rec; w->ptr = in.d_link_ptr; w->links = in.d_links; w->nS = (uint64_t)in.nS; w->n_links = in.n_links;
  w->ctr = carve_at<unsigned long long>(base, p.o_ctr);
  w->in_off = carve_at<unsigned long long>(base, p.o_off);
  w->in_cur = nullptr; w->in_src = nullptr;
  w->hit_ptr = in.d_hit_ptr; w->hits = in.d_hits; w->nR = (uint64_t)in.nR; w->n_hits = (uint64_t)in.n_hits;
  w->scan = carve_at<uint32_t>(base, p.o_scan);
  w->path_ptr = nullptr; w->paths = nullptr; w->n_paths = 0; w->support = nullptr;
}

}  // namespace

// Passes 1-6 and the one synchronisation: d_path_ptr, *n_paths, *stats and (unless NULL) d_support complete, or
// CFRK_ERR_LAYOUT naming the unitig or the read, with d_path_ptr all 0 and d_support untouched.
int cfrk_read_paths_measure(cfrk_ctx *ctx, const cfrk_read_paths_in &in, int64_t *d_path_ptr, uint32_t *d_support,
                            int64_t *n_paths, cfrk_path_stats *stats) {
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  RPPlan p;
  if (const int rc = rp_plan(ctx, canon, (uint64_t)in.nS, (uint64_t)in.n_hits, &p)) return rc;
  void *base;
  if (const int rc = cfrk_pool_get(ctx, BUF_READ_PATHS, p.bytes, &base)) return rc;
  RPWork w;
  rp_work(&w, base, p, in);
  w.path_ptr = d_path_ptr; w.support = d_support;
  HIP_TRY(ctx, hipMemsetAsync(w.ctr + RPC_HIT_ERR, 0xFF, 8, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w.ctr + RPC_PATHS, 0, (RPC_WORDS - RPC_PATHS) * 8, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w.scan, 0, (size_t)(w.n_hits + 1) * 4, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_path_ptr, 0, (size_t)(w.nR + 1) * 8, ctx->stream));
  if (const int rc = ug_check_launch(ctx, w, canon, u_grid(ctx, w.nS), nullptr, 0, false)) return rc;     // (the in-rows are not read here)
  const int grid_r = u_grid(ctx, w.nR + 1), grid_h = u_grid(ctx, w.n_hits);
  hipLaunchKernelGGL(rp_mark_kernel, dim3(grid_r), dim3(256), 0, ctx->stream, w);
  hipLaunchKernelGGL(rp_hits_kernel, dim3(grid_h), dim3(256), 0, ctx->stream, w);
  hipLaunchKernelGGL(rp_join_kernel, dim3(grid_h), dim3(256), 0, ctx->stream, w);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(carve_at<void>(base, p.o_tmp), p.scan_tmp, w.scan, w.scan, (size_t)(w.n_hits + 1), ctx->stream));
  hipLaunchKernelGGL(rp_rows_kernel, dim3(grid_r), dim3(256), 0, ctx->stream, w);
  HIP_TRY(ctx, hipGetLastError());
  unsigned long long h[RPC_WORDS];
  HIP_TRY(ctx, hipMemcpyAsync(h, w.ctr, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (h[RPC_ERR] != UG_NONE) return ug_layout_error(ctx, h[RPC_ERR]);
  if (h[RPC_HIT_ERR] != UG_NONE) {
    const unsigned long long i = h[RPC_HIT_ERR] >> 8;
    const int why = (int)(h[RPC_HIT_ERR] & 255);
    const char *what = why == RPE_PTR      ? "has a hit_ptr that does not ascend from 0 inside [0, n_hits]"
                       : why == RPE_UNITIG ? "has a hit on a unitig that is not in the list"
                       : why == RPE_EMPTY  ? "has a hit of no windows"
                                           : "has a hit that runs past the end of its unitig";
    return cfrk_fail(ctx, CFRK_ERR_LAYOUT, "read %llu %s: not the hits of reads on this unitig list", i, what);
  }
  *n_paths = (int64_t)h[RPC_PATHS];
  stats->n_paths = h[RPC_PATHS]; stats->n_steps = h[RPC_STEPS]; stats->n_gaps = h[RPC_GAPS]; stats->n_unlinked = h[RPC_UNLINKED];
  return CFRK_OK;
}

// Passes 7 and 8 behind a measure call of the same arrays (its scan is still in the pool), left enqueued; n_paths >= 1.
int cfrk_read_paths_fill(cfrk_ctx *ctx, const cfrk_read_paths_in &in, cfrk_read_path *d_paths, int64_t n_paths) {
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  RPPlan p;
  if (const int rc = rp_plan(ctx, canon, (uint64_t)in.nS, (uint64_t)in.n_hits, &p)) return rc;
  void *base = ctx->pool[BUF_READ_PATHS].p;
  if (!base || ctx->pool[BUF_READ_PATHS].cap < p.bytes) return cfrk_fail(ctx, CFRK_ERR_STATE, "read paths: the fill pass without its measure pass");
  RPWork w;
  rp_work(&w, base, p, in);
  w.paths = (uint32_t *)d_paths; w.n_paths = (uint64_t)n_paths;
  hipLaunchKernelGGL(rp_events_kernel, dim3(u_grid(ctx, w.n_hits)), dim3(256), 0, ctx->stream, w);
  hipLaunchKernelGGL(rp_finish_kernel, dim3(u_grid(ctx, w.n_paths)), dim3(256), 0, ctx->stream, w);
  HIP_TRY(ctx, hipGetLastError());
  return CFRK_OK;
}
