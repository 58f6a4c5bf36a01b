// unitig_components.hip -- the connected components of the unitig graph, and the component every read goes with.  Pure
// functions of the unitigs' records, the link CSR, a drop byte per unitig, and (for the reads) the hit CSR: no sequence, no
// index, no counts.  The contracts are in include/cfrk_abi.h ("Unitig components", "Read components"); DESIGN 4.28 has the
// reasoning and the measurements.
//
// COMPONENTS.  The arrays are untrusted.  Passes, each a launch of its own on the context stream; every pass behind the
// check reads the error word first and does nothing when it is set, so that only checked rows are ever followed:
//   1 check    the shared row check (not canonical: with the in-degrees it counts, without the in-rows): unitig_graph_dev.h
//   2 init     parent[j] = j
//   3 hook     one lane per unitig walks its checked row (<= 16 links); for each link with both ends kept it unites them:
//              find both roots, hang the LARGER root under the SMALLER with a compare-and-swap on parent[larger]; a swap
//              that fails retries from the value it returned.  Finds halve their path as they go
//   4 flatten  one lane per unitig: parent[j] = root(j); flag[j] = (j == root(j) and kept)
//   5 scan     hipCUB exclusive sum over the flags, in place
//   6 label    comp[j] = scan[parent[j]], CFRK_COMP_NONE for a dropped unitig; the four statistics, summed per wave over
//              the whole launch and added once
//   -- the one synchronisation: the error word, n_comps and the statistics --
//   7 table    only when n_comps <= cap_comps: comps zeroed, then one lane per unitig adds its record and its kept links to
//              row comp[j], COMBINED WITHIN THE WAVE first: for each distinct comp value the wave holds (ballot, the first
//              lane's value, a sum over the equal lanes) one lane issues one atomic per field -- and holds the row back while the
//              next turns bring the same component again.  Left enqueued
//
// The union-find.  INVARIANT: parent[x] <= x at every instant: init writes x, a hook writes a smaller root into
// parent[larger root], halving writes an ancestor, which is smaller again, with an atomic minimum.  So
// parent[] only ever descends, an old value of parent[x] is still an ancestor of x, and the root a component ends with
// is its smallest unitig: that is where the numbering, and with it the determinism, comes from.
// VISIBILITY.  Inside the hook launch other workgroups, on other XCDs with L2s of their own, write parent[].  Every read
// of parent[] in the hook and flatten kernels is a relaxed atomic load at agent scope (uc_load), every write an agent-scope
// atomic: the compare-and-swap of the hook (uc_unite), the atomic minimum of the halving (uc_find), the relaxed store of
// the flatten.  No plain load or store of parent[] appears in those kernels.  A stale value could only name an older
// ancestor, which is still correct; with atomic loads nothing has to be argued over stale lines.  Across launches plain
// accesses are fine (init, label).
// TERMINATION.  A find descends strictly (it moves from x to parent[x] < x), so it takes at most x steps.  A swap fails
// only because another lane hooked that very root in the meantime; a root is hooked once, so at most nS - 1 hooks ever
// happen and a unite retries at most nS - 1 times in all.  No lane waits for another.
// No LDS; the wave sums go through cross-lane moves.  No scratch.
//
// READS.  Balanced by HITS, as read_paths.hip is; the only loop is the binary search in hit_ptr (<= 64 steps):
//   1 mark     one lane per read: hit_ptr[i] <= hit_ptr[i + 1] inside [0, n_hits], 0 at i = 0; best[i] = 0, flags[i] = 0
//   2 offer    one lane per hit: unitig < nS and n_windows > 0, or the read is refused; an eligible hit offers
//              (n_windows << 32) | (0xFFFFFFFF - index in row) to the atomic maximum of best[read] (most windows, then
//              the earliest; 0 = no offer, since n_windows > 0); one that is not ORs CFRK_READ_COMP_DROPPED
//   3 split    one lane per hit: an eligible hit whose component differs from the winner's ORs CFRK_READ_COMP_SPLIT
//   4 rows     one lane per read writes its row; the four statistics, summed per wave over the whole launch
//   -- the one synchronisation: the error word and the statistics --
#include "unitig_graph_dev.h"

namespace {

// ================================================================= components

enum { UCC_ERR = UGC_ERR, UCC_COMPS, UCC_UNITIGS, UCC_KMERS, UCC_LINKS, UCC_WORDS };

struct UCWork : UGraph {
  const uint8_t *drop;                // [nS] or NULL
  uint32_t *parent;                   // [nS]
  uint32_t *scan;                     // [nS]: the roots' flags, then their exclusive sums
  uint32_t *comp;                     // [nS], the caller's
  cfrk_unitig_component *comps;       // the caller's table
};

__device__ __forceinline__ bool uc_kept(const UCWork &w, uint64_t j) { return !w.drop || w.drop[j] == 0; }

__device__ __forceinline__ uint32_t uc_load(uint32_t *parent, uint32_t x) {
  return __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x as far as this lane can see, halving the path on the way: x's parent becomes its grandparent
__device__ __forceinline__ uint32_t uc_find(uint32_t *parent, uint32_t x) {
  uint32_t p = uc_load(parent, x);
  while (p != x) {                                      // (p < x: strictly down)
    const uint32_t g = uc_load(parent, p);
    if (g != p) __hip_atomic_fetch_min(&parent[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p; p = g;
  }
  return x;
}

__device__ __forceinline__ void uc_unite(uint32_t *parent, uint32_t a, uint32_t b) {
  a = uc_find(parent, a); b = uc_find(parent, b);
  while (a != b) {
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    uint32_t seen = hi;
    if (__hip_atomic_compare_exchange_strong(&parent[hi], &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    a = uc_find(parent, seen);                          // another lane hooked hi, under seen < hi
    b = uc_find(parent, lo);
  }
}

// ---- 2 init -----------------------------------------------------------------------------------------------------
// (parent[j] = j's smallest kept neighbour, which saves most hooks in a link set with mirrors, was measured and is slower
// on the real graph: the trees it starts the hook with are deeper than the ones the hook builds.  DESIGN 4.28)
__global__ __launch_bounds__(256) void uc_init_kernel(UCWork w) {
  if (w.ctr[UGC_ERR] != UG_NONE) return;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = tid; j < w.nS; j += nthreads) w.parent[j] = (uint32_t)j;
}

// ---- 3 hook -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void uc_hook_kernel(UCWork w) {
  if (w.ctr[UGC_ERR] != UG_NONE) return;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = tid; j < w.nS; j += nthreads) {
    if (!uc_kept(w, j)) continue;
    const int64_t a = w.ptr[j], b = w.ptr[j + 1];       // (a checked row: at most 16 links, targets below nS)
    for (int64_t t = a; t < b; ++t) {
      const uint32_t v = w.links[t].to;
      if (v != (uint32_t)j && uc_kept(w, v)) uc_unite(w.parent, (uint32_t)j, v);
    }
  }
}

// ---- 4 flatten --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void uc_flatten_kernel(UCWork w) {
  if (w.ctr[UGC_ERR] != UG_NONE) return;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = tid; j < w.nS; j += nthreads) {
    const uint32_t r = uc_find(w.parent, (uint32_t)j);  // (other lanes store roots meanwhile: ancestors still)
    __hip_atomic_store(&w.parent[j], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    w.scan[j] = (r == (uint32_t)j && uc_kept(w, j)) ? 1u : 0u;
  }
}

// the sum of x over the wave's 64 lanes, in every lane
__device__ __forceinline__ unsigned long long uc_wave_sum(unsigned long long x) {
  for (int d = 32; d; d >>= 1) x += __shfl_xor(x, d, 64);
  return x;
}

// the links of checked row j whose target is kept
__device__ __forceinline__ uint32_t uc_kept_links(const UCWork &w, uint64_t j) {
  uint32_t n = 0;
  for (int64_t t = w.ptr[j]; t < w.ptr[j + 1]; ++t) n += uc_kept(w, w.links[t].to) ? 1u : 0u;
  return n;
}

// ---- 6 label ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void uc_label_kernel(UCWork w) {
  if (w.ctr[UGC_ERR] != UG_NONE) return;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  unsigned long long n_comps = 0, n_unitigs = 0, n_kmers = 0, n_links = 0;      // this lane's, over every turn of the loop
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < w.nS; j += nthreads) {
    if (!uc_kept(w, j)) { w.comp[j] = CFRK_COMP_NONE; continue; }
    const uint32_t r = w.parent[j];
    w.comp[j] = w.scan[r];
    n_comps += r == (uint32_t)j;
    n_unitigs += 1;
    n_kmers += w.rec[j].n_kmers;
    n_links += uc_kept_links(w, j);
  }
  // one add per wave and counter for the whole launch (a contended word bounds its kernel)
  n_comps = uc_wave_sum(n_comps); n_unitigs = uc_wave_sum(n_unitigs); n_kmers = uc_wave_sum(n_kmers); n_links = uc_wave_sum(n_links);
  if ((threadIdx.x & 63) == 0) {
    if (n_comps) atomicAdd(&w.ctr[UCC_COMPS], n_comps);
    if (n_unitigs) atomicAdd(&w.ctr[UCC_UNITIGS], n_unitigs);
    if (n_kmers) atomicAdd(&w.ctr[UCC_KMERS], n_kmers);
    if (n_links) atomicAdd(&w.ctr[UCC_LINKS], n_links);
  }
}

// ---- 7 table ----------------------------------------------------------------------------------------------------
// comp[] holds numbers below n_comps <= cap_comps by now (label wrote them from the scan whose total n_comps is).  Whole
// waves turn together: the ballots below are a wave's.
__global__ __launch_bounds__(256) void uc_table_kernel(UCWork w) {
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  const unsigned lane = threadIdx.x & 63;
  // the wave's pending row, the same in every lane: a component met again in the next turn of either loop is added to it
  // in registers, and the row's atomics are issued when another component comes or the wave is done.  Where nearly every
  // unitig lies in one component that is four atomics per wave and launch, not per wave and turn
  uint32_t pc = CFRK_COMP_NONE, p_nu = 0;
  unsigned long long p_kc = 0, p_nk = 0, p_nl = 0;
  auto flush = [&]() {
    if (pc == CFRK_COMP_NONE || lane != 0) return;
    cfrk_unitig_component *row = &w.comps[pc];
    atomicAdd((unsigned long long *)&row->kc, p_kc); atomicAdd((unsigned long long *)&row->n_kmers, p_nk);
    if (p_nl) atomicAdd((unsigned long long *)&row->n_links, p_nl);
    atomicAdd(&row->n_unitigs, p_nu);
  };
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < w.nS; base += nthreads) {
    const uint64_t j = base + threadIdx.x;
    uint32_t c = CFRK_COMP_NONE;
    unsigned long long kc = 0, nk = 0, nl = 0;
    if (j < w.nS && (c = w.comp[j]) != CFRK_COMP_NONE) {
      const cfrk_unitig r = w.rec[j];
      kc = r.kc; nk = r.n_kmers; nl = uc_kept_links(w, j);
      if (w.parent[j] == (uint32_t)j) w.comps[c].first = (uint32_t)j;         // the root: the smallest member
    }
    unsigned long long todo = __ballot(c != CFRK_COMP_NONE);
    while (todo) {                                      // one turn per distinct component in the wave
      const int lead = __ffsll((long long)todo) - 1;
      const uint32_t cl = (uint32_t)__shfl((int)c, lead, 64);
      const bool mine = c == cl;
      const unsigned long long same = __ballot(mine);
      todo &= ~same;
      unsigned long long s_kc, s_nk, s_nl;
      if (same == (1ull << lead)) {                     // alone in its wave: nothing to sum
        s_kc = __shfl(kc, lead, 64); s_nk = __shfl(nk, lead, 64); s_nl = __shfl(nl, lead, 64);
      } else {
        s_kc = uc_wave_sum(mine ? kc : 0); s_nk = uc_wave_sum(mine ? nk : 0); s_nl = uc_wave_sum(mine ? nl : 0);
      }
      if (cl != pc) {
        flush();
        pc = cl; p_kc = p_nk = p_nl = 0; p_nu = 0;
      }
      p_kc += s_kc; p_nk += s_nk; p_nl += s_nl; p_nu += (uint32_t)__popcll(same);
    }
  }
  flush();
}

struct UCPlan {
  size_t o_ctr, o_parent, o_scan, o_off, o_tmp, bytes, scan_tmp;
};

int uc_plan(cfrk_ctx *ctx, bool canon, uint64_t n, UCPlan *p) {
  p->scan_tmp = 0;
  HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, p->scan_tmp, (uint32_t *)nullptr, (size_t)n, ctx->stream));
  Carve c;
  p->o_ctr = c.part(UCC_WORDS * 8);
  p->o_parent = c.part((size_t)n * 4);
  p->o_scan = c.part((size_t)n * 4);
  p->o_off = c.part(canon ? 0 : (size_t)(n + 1) * 8);             // not canonical: the in-degrees the row check counts
  p->o_tmp = c.part(p->scan_tmp);
  p->bytes = c.end;
  return CFRK_OK;
}

void uc_work(UCWork *w, void *base, const UCPlan &p, const cfrk_unitig_components_in &in) {
  w->rec = in.d_rec; w->ptr = in.d_link_ptr; w->links = in.d_links; w->nS = (uint64_t)in.nS; w->n_links = in.n_links;
  w->ctr = carve_at<unsigned long long>(base, p.o_ctr);
  w->in_off = carve_at<unsigned long long>(base, p.o_off);
  w->in_cur = nullptr; w->in_src = nullptr;
  w->drop = in.d_drop;
  w->parent = carve_at<uint32_t>(base, p.o_parent);
  w->scan = carve_at<uint32_t>(base, p.o_scan);
  w->comp = nullptr; w->comps = nullptr;
}

// ================================================================= reads

enum { RCC_ERR = 0, RCC_ASSIGNED, RCC_UNASSIGNED, RCC_SPLIT, RCC_DROPPED, RCC_WORDS };
// error word = read << 8 | why, kept with an atomic minimum: the first offending read
enum { RCE_PTR = 1, RCE_UNITIG, RCE_EMPTY };

struct RCWork {
  const int64_t *hit_ptr;
  const cfrk_read_hit *hits;
  uint64_t nR, n_hits, nS;
  const uint32_t *comp;
  unsigned long long *ctr;
  unsigned long long *best;           // [nR]: the largest offer
  uint32_t *flags;                    // [nR]
  uint32_t *out;                      // rows of cfrk_read_component as words
};

__device__ __forceinline__ uint64_t rc_total(const RCWork &w) { return w.nR ? (uint64_t)w.hit_ptr[w.nR] : 0; }

// the read whose row holds hit h: the last i with hit_ptr[i] <= h; bounded by log2(nR) whatever hit_ptr holds
__device__ __forceinline__ uint64_t rc_read_of(const RCWork &w, uint64_t h) {
  uint64_t lo = 0, hi = w.nR;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    const int64_t p = w.hit_ptr[mid];
    if (p >= 0 && (uint64_t)p <= h) lo = mid + 1; else hi = mid;
  }
  return lo ? lo - 1 : 0;
}

// ---- 1 mark -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rc_mark_kernel(RCWork w) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  if (w.nR == 0 && tid == 0 && w.hit_ptr[0] != 0) atomicMin(&w.ctr[RCC_ERR], (unsigned long long)RCE_PTR);       // (no row: "read 0")
  for (uint64_t i = tid; i < w.nR; i += nthreads) {
    const int64_t a = w.hit_ptr[i], b = w.hit_ptr[i + 1];
    if ((i == 0 && a != 0) || a < 0 || b < a || (uint64_t)b > w.n_hits)
      atomicMin(&w.ctr[RCC_ERR], (unsigned long long)((i << 8) | RCE_PTR));
    w.best[i] = 0;
    w.flags[i] = 0;
  }
}

// ---- 2 offer ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rc_offer_kernel(RCWork w) {
  // hit_ptr is refused: no row to name.  Only what the mark pass wrote counts: this kernel stores the other reasons into
  // the same word, and a block that starts late must still look at its hits, or a later read could be the one named
  if ((w.ctr[RCC_ERR] & 255) == RCE_PTR) return;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t total = rc_total(w);
  for (uint64_t h = tid; h < total; h += nthreads) {
    const cfrk_read_hit x = w.hits[h];
    const uint64_t i = rc_read_of(w, h);                // (total > 0: nR > 0, i < nR, hit_ptr[i] <= h)
    if (x.unitig >= w.nS || x.n_windows == 0) {
      atomicMin(&w.ctr[RCC_ERR], (unsigned long long)((i << 8) | (uint64_t)(x.unitig >= w.nS ? RCE_UNITIG : RCE_EMPTY)));
      continue;
    }
    if (w.comp[x.unitig] == CFRK_COMP_NONE) { atomicOr(&w.flags[i], (uint32_t)CFRK_READ_COMP_DROPPED); continue; }
    const uint32_t at = (uint32_t)(h - (uint64_t)w.hit_ptr[i]);               // (n_hits < 2^32)
    atomicMax(&w.best[i], ((unsigned long long)x.n_windows << 32) | (0xFFFFFFFFu - at));
  }
}

// ---- 3 split ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rc_split_kernel(RCWork w) {
  if (w.ctr[RCC_ERR] != UG_NONE) return;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t total = rc_total(w);
  for (uint64_t h = tid; h < total; h += nthreads) {
    const uint32_t c = w.comp[w.hits[h].unitig];
    if (c == CFRK_COMP_NONE) continue;
    const uint64_t i = rc_read_of(w, h);
    // (this hit offered, so best[i] is an offer of this row: the index is inside it)
    const uint64_t win = (uint64_t)w.hit_ptr[i] + (0xFFFFFFFFu - (uint32_t)w.best[i]);
    if (w.comp[w.hits[win].unitig] != c) atomicOr(&w.flags[i], (uint32_t)CFRK_READ_COMP_SPLIT);
  }
}

// ---- 4 rows -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rc_rows_kernel(RCWork w) {
  if (w.ctr[RCC_ERR] != UG_NONE) return;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  unsigned long long n_as = 0, n_un = 0, n_split = 0, n_drop = 0;   // this wave's, every lane the same
  // (whole waves turn together: the ballots below count a wave's reads)
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < w.nR; base += nthreads) {
    const uint64_t i = base + threadIdx.x;
    bool as = false, un = false;
    uint32_t f = 0;
    if (i < w.nR) {
      const unsigned long long best = w.best[i];
      f = w.flags[i];
      uint32_t *row = w.out + i * 4;
      if (best) {
        const uint32_t at = 0xFFFFFFFFu - (uint32_t)best;
        row[0] = w.comp[w.hits[(uint64_t)w.hit_ptr[i] + at].unitig]; row[1] = at; row[2] = (uint32_t)(best >> 32);
        as = true;
      } else {
        row[0] = 0xFFFFFFFFu; row[1] = 0xFFFFFFFFu; row[2] = 0;
        un = true;
      }
      row[3] = f;
    }
    n_as += (unsigned)__popcll(__ballot(as));
    n_un += (unsigned)__popcll(__ballot(un));
    n_split += (unsigned)__popcll(__ballot((f & CFRK_READ_COMP_SPLIT) != 0));
    n_drop += (unsigned)__popcll(__ballot((f & CFRK_READ_COMP_DROPPED) != 0));
  }
  if ((threadIdx.x & 63) == 0) {
    if (n_as) atomicAdd(&w.ctr[RCC_ASSIGNED], n_as);
    if (n_un) atomicAdd(&w.ctr[RCC_UNASSIGNED], n_un);
    if (n_split) atomicAdd(&w.ctr[RCC_SPLIT], n_split);
    if (n_drop) atomicAdd(&w.ctr[RCC_DROPPED], n_drop);
  }
}

}  // namespace

// Passes 1-6 and the one synchronisation: d_comp, *n_comps and *stats complete, or CFRK_ERR_LAYOUT naming the unitig with
// d_comp all CFRK_COMP_NONE.  1 <= nS < 2^32.
int cfrk_unitig_components_measure(cfrk_ctx *ctx, const cfrk_unitig_components_in &in, uint32_t *d_comp, int64_t *n_comps,
                                   cfrk_component_stats *stats) {
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  UCPlan p;
  if (const int rc = uc_plan(ctx, canon, (uint64_t)in.nS, &p)) return rc;
  void *base;
  if (const int rc = cfrk_pool_get(ctx, BUF_UNITIG_COMP, p.bytes, &base)) return rc;
  UCWork w;
  uc_work(&w, base, p, in);
  w.comp = d_comp;
  HIP_TRY(ctx, hipMemsetAsync(w.ctr + UCC_COMPS, 0, (UCC_WORDS - UCC_COMPS) * 8, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_comp, 0xFF, (size_t)w.nS * 4, ctx->stream));   // every word is written, whatever is refused
  const int grid = u_grid(ctx, w.nS);
  if (const int rc = ug_check_launch(ctx, w, canon, grid, nullptr, 0, false)) return rc;      // (the in-rows are not read here)
  hipLaunchKernelGGL(uc_init_kernel, dim3(grid), dim3(256), 0, ctx->stream, w);
  hipLaunchKernelGGL(uc_hook_kernel, dim3(grid), dim3(256), 0, ctx->stream, w);
  hipLaunchKernelGGL(uc_flatten_kernel, dim3(grid), dim3(256), 0, ctx->stream, w);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(carve_at<void>(base, p.o_tmp), p.scan_tmp, w.scan, w.scan, (size_t)w.nS, ctx->stream));
  hipLaunchKernelGGL(uc_label_kernel, dim3(grid), dim3(256), 0, ctx->stream, w);
  HIP_TRY(ctx, hipGetLastError());
  unsigned long long h[UCC_WORDS];
  HIP_TRY(ctx, hipMemcpyAsync(h, w.ctr, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (h[UCC_ERR] != UG_NONE) return ug_layout_error(ctx, h[UCC_ERR]);
  *n_comps = (int64_t)h[UCC_COMPS];
  stats->n_components = h[UCC_COMPS]; stats->n_unitigs = h[UCC_UNITIGS]; stats->n_kmers = h[UCC_KMERS]; stats->n_links = h[UCC_LINKS];
  return CFRK_OK;
}

// Pass 7 behind a measure call of the same arrays (its parent[] is still in the pool), left enqueued; d_comps has room for
// n_comps >= 1 rows.
int cfrk_unitig_components_fill(cfrk_ctx *ctx, const cfrk_unitig_components_in &in, const uint32_t *d_comp,
                                cfrk_unitig_component *d_comps, int64_t n_comps) {
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  UCPlan p;
  if (const int rc = uc_plan(ctx, canon, (uint64_t)in.nS, &p)) return rc;
  void *base = ctx->pool[BUF_UNITIG_COMP].p;
  if (!base || ctx->pool[BUF_UNITIG_COMP].cap < p.bytes) return cfrk_fail(ctx, CFRK_ERR_STATE, "unitig components: the table pass without its measure pass");
  UCWork w;
  uc_work(&w, base, p, in);
  w.comp = const_cast<uint32_t *>(d_comp); w.comps = d_comps;
  HIP_TRY(ctx, hipMemsetAsync(d_comps, 0, (size_t)n_comps * sizeof *d_comps, ctx->stream));
  hipLaunchKernelGGL(uc_table_kernel, dim3(u_grid(ctx, w.nS)), dim3(256), 0, ctx->stream, w);
  HIP_TRY(ctx, hipGetLastError());
  return CFRK_OK;
}

// The reads' rows on device arrays; synchronises once: CFRK_ERR_LAYOUT naming the read, or *stats.
int cfrk_read_components_launch(cfrk_ctx *ctx, const int64_t *d_hit_ptr, int64_t nR, const cfrk_read_hit *d_hits, int64_t n_hits,
                                const uint32_t *d_comp, int64_t nS, cfrk_read_component *d_out, cfrk_read_component_stats *stats) {
  Carve c;
  const size_t o_ctr = c.part(RCC_WORDS * 8), o_best = c.part((size_t)nR * 8), o_flags = c.part((size_t)nR * 4);
  void *base;
  if (const int rc = cfrk_pool_get(ctx, BUF_READ_COMP, c.end, &base)) return rc;
  RCWork w;
  w.hit_ptr = d_hit_ptr; w.hits = d_hits; w.nR = (uint64_t)nR; w.n_hits = (uint64_t)n_hits; w.nS = (uint64_t)nS; w.comp = d_comp;
  w.ctr = carve_at<unsigned long long>(base, o_ctr);
  w.best = carve_at<unsigned long long>(base, o_best);
  w.flags = carve_at<uint32_t>(base, o_flags);
  w.out = (uint32_t *)d_out;
  HIP_TRY(ctx, hipMemsetAsync(w.ctr, 0xFF, 8, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w.ctr + RCC_ASSIGNED, 0, (RCC_WORDS - RCC_ASSIGNED) * 8, ctx->stream));
  const int grid_r = u_grid(ctx, w.nR), grid_h = u_grid(ctx, w.n_hits);
  hipLaunchKernelGGL(rc_mark_kernel, dim3(grid_r), dim3(256), 0, ctx->stream, w);
  hipLaunchKernelGGL(rc_offer_kernel, dim3(grid_h), dim3(256), 0, ctx->stream, w);
  hipLaunchKernelGGL(rc_split_kernel, dim3(grid_h), dim3(256), 0, ctx->stream, w);
  hipLaunchKernelGGL(rc_rows_kernel, dim3(grid_r), dim3(256), 0, ctx->stream, w);
  HIP_TRY(ctx, hipGetLastError());
  unsigned long long h[RCC_WORDS];
  HIP_TRY(ctx, hipMemcpyAsync(h, w.ctr, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (h[RCC_ERR] != UG_NONE) {
    const unsigned long long i = h[RCC_ERR] >> 8;
    const int why = (int)(h[RCC_ERR] & 255);
    const char *what = why == RCE_PTR      ? "has a hit_ptr that does not ascend from 0 inside [0, n_hits]"
                       : why == RCE_UNITIG ? "has a hit on a unitig that is not in the list"
                                           : "has a hit of no windows";
    return cfrk_fail(ctx, CFRK_ERR_LAYOUT, "read %llu %s: not the hits of reads on this unitig list", i, what);
  }
  stats->n_assigned = h[RCC_ASSIGNED]; stats->n_unassigned = h[RCC_UNASSIGNED]; stats->n_split = h[RCC_SPLIT]; stats->n_dropped = h[RCC_DROPPED];
  return CFRK_OK;
}
