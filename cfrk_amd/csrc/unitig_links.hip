// unitig_links.hip -- the edges of the compacted de Bruijn graph: which oriented unitig follows which, as CSR rows over
// the unitig list cfrk_global_unitigs wrote.  The contract is in include/cfrk_abi.h ("Unitig links"); DESIGN 4.20 has the
// reasoning.
//
// Everything is answered from the lookup index of query.hip, which is not modified, and from the 2k end bases of every
// unitig: no lane walks a unitig.  Beside the index the call keeps one 64-bit TAG per index slot (k <= 12: the slot is
// the key): the unitig whose first or last k-mer is that node, and four end bits -- it is the first k-mer's node, that
// k-mer is the reverse complement of the stored key, and the same two for the last k-mer.  Every solid key lies in one
// unitig once, so a node is the end of at most one unitig; a single-node unitig sets all four bits.
//
// Passes, each a launch of its own on the context stream (a later one reads what an earlier one wrote):
//   1 tag     one lane per (unitig, end): the end k-mer from the codes, its node, the tag claimed with a compare-and-swap
//             (a second claim of a node is an inconsistent input, not a race to lose quietly)
//   2 count   one lane per oriented end (j,o): the tail k-mer, its <= 4 successors; a solid successor's tag says which
//             of (v,+), (v,-) begin with it: head(v,+) is v's first k-mer, head(v,-) the complement of its last
//   3 scan    hipCUB exclusive sum over the oriented ends' counts, in place; link_ptr[j] = the offset of (j,+)
//   -- the one synchronisation: the error word and n_links --
//   4 fill    pass 2 again, writing the rows at the scanned offsets: base order, + before -
// The first offending unitig and why go to the error word with an atomic minimum from passes 1 and 2.
//
// Work memory (BUF_UNITIG_LINKS): 8 bytes per index slot (tags), 8 bytes per oriented unitig (counts, then offsets), the
// scan's scratch and two words.
#include "staging.h"
#include "unitig_dev.h"

#include <hipcub/hipcub.hpp>

namespace {

constexpr unsigned long long UL_EMPTY = ~0ull;
enum { ULB_FIRST = 1, ULB_FIRST_RC = 2, ULB_LAST = 4, ULB_LAST_RC = 8 };      // tag = unitig << 4 | bits
enum { ULC_ERR = 0, ULC_TOTAL, ULC_WORDS };
// error word = missed << 40 | unitig << 8 | why, kept with an atomic minimum: the first unitig whose own ends are wrong
// (passes 1); only when there is none, the first with a missed successor (pass 2; `missed` = 1) -- a wrong end is often
// what makes a neighbour miss its successor
enum { ULE_RANGE = 1, ULE_CODE, ULE_ABSENT, ULE_CLAIMED, ULE_NO_HEAD };

struct ULWork {
  QIndex q;
  const int8_t *data; const int64_t *start; const int32_t *length;
  int64_t nN;
  uint64_t nS;
  USolid sol;                         // min_count and the graph mask
  unsigned long long *ctr;            // ULC_*
  unsigned long long *tag;            // [slots]
  int64_t *off;                       // [o nS + 1]: an oriented end's links, scanned into its first row
};

__device__ __forceinline__ void ul_fail(const ULWork &w, uint64_t j, int why) {
  atomicMin(&w.ctr[ULC_ERR], (unsigned long long)(((uint64_t)(why == ULE_NO_HEAD) << 40) | (j << 8) | (uint64_t)why));
}

// the first (end 0) or last (end 1) k-mer of unitig j as written; 0 or ULE_*.  Reads k codes inside [0, nN) or nothing.
__device__ __forceinline__ int ul_end_kmer(const ULWork &w, uint64_t j, int end, u128 &x) {
  const int k = w.q.k;
  const int64_t s = w.start[j], len = w.length[j];
  if (len < k || s < 0 || s > w.nN || len > w.nN - s) return ULE_RANGE;
  const int8_t *p = w.data + s + (end ? len - k : 0);
  uint32_t seen = 0;
  x = 0;
  for (int t = 0; t < k; ++t) {
    const uint32_t c = (uint8_t)p[t];
    seen |= c;
    x = (x << 2) | (u128)(c & 3u);
  }
  return seen > 3u ? ULE_CODE : 0;
}

// ---- 1 tag ------------------------------------------------------------------------------------------------------
template <int MODE, bool CANON, bool MASKED>
__device__ __forceinline__ void ul_tag_body(const ULWork &w) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = tid; i < 2 * w.nS; i += nthreads) {
    const uint64_t j = i >> 1;
    const int end = (int)(i & 1);
    u128 x;
    const int e = ul_end_kmer(w, j, end, x);
    if (e) { ul_fail(w, j, e); continue; }
    const bool single = w.length[j] == w.q.k;
    if (single && end) continue;                                  // (the other lane sets all four bits)
    int o; bool pal;
    const uint64_t slot = u_node<MODE, CANON>(w.q, x, o, pal);
    if (!u_solid<MODE, MASKED>(w.q, w.sol, slot)) { ul_fail(w, j, ULE_ABSENT); continue; }
    uint32_t bits = end ? ULB_LAST | (o ? ULB_LAST_RC : 0) : ULB_FIRST | (o ? ULB_FIRST_RC : 0);
    if (single) bits = ULB_FIRST | ULB_LAST | (o ? ULB_FIRST_RC | ULB_LAST_RC : 0);
    if (atomicCAS(&w.tag[slot], UL_EMPTY, (unsigned long long)((j << 4) | bits)) != UL_EMPTY) ul_fail(w, j, ULE_CLAIMED);
  }
}
U_SOLID_KERNELS(ul_tag, (ULWork w), (w))

// ---- 2 count, 4 fill --------------------------------------------------------------------------------------------
// the links out of oriented end i = o j + orientation: counted into off[i], or written from off[i] on
template <int MODE, bool CANON, bool MASKED, bool FILL>
__device__ __forceinline__ void ul_links(const ULWork &w, uint64_t i, cfrk_unitig_link *__restrict__ links) {
  const int k = w.q.k;
  const uint64_t j = CANON ? i >> 1 : i;
  const int minus = CANON ? (int)(i & 1) : 0;
  int64_t n = 0, at = 0, room = 0;
  if (FILL) { at = w.off[i]; room = w.off[i + 1] - at; }
  u128 t;
  if (ul_end_kmer(w, j, minus ? 0 : 1, t) == 0) {                 // tail(j,+): the last k-mer; tail(j,-): rc(the first)
    if (minus) t = u_rc(t, k);
    for (int b = 0; b < 4; ++b) {
      int oz; bool pal;
      const uint64_t slot = u_node<MODE, CANON>(w.q, u_succ_key(t, b, k), oz, pal);
      if (!u_solid<MODE, MASKED>(w.q, w.sol, slot)) continue;
      const unsigned long long tag = w.tag[slot];
      const uint32_t bits = tag == UL_EMPTY ? 0u : (uint32_t)tag & 15u;
      // head(v,+) = v's first k-mer: the stored key's orientation must be the successor's; head(v,-) = rc(v's last)
      const bool to_plus = (bits & ULB_FIRST) && (pal || ((bits & ULB_FIRST_RC) != 0) == (oz != 0));
      const bool to_minus = CANON && (bits & ULB_LAST) && (pal || ((bits & ULB_LAST_RC) != 0) != (oz != 0));
      if (!to_plus && !to_minus) { if (!FILL) ul_fail(w, j, ULE_NO_HEAD); continue; }
      if (FILL) {
        const uint32_t v = (uint32_t)(tag >> 4), from = minus ? CFRK_LINK_FROM_MINUS : 0u;
        if (to_plus && n < room) { cfrk_unitig_link r; r.to = v; r.flags = from; links[at + n] = r; }
        if (to_minus && n + (to_plus ? 1 : 0) < room) { cfrk_unitig_link r; r.to = v; r.flags = from | CFRK_LINK_TO_MINUS; links[at + n + (to_plus ? 1 : 0)] = r; }
      }
      n += (to_plus ? 1 : 0) + (to_minus ? 1 : 0);
    }
  }
  if (!FILL) w.off[i] = n;
}

template <int MODE, bool CANON, bool MASKED>
__device__ __forceinline__ void ul_count_body(const ULWork &w) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t items = (CANON ? 2 : 1) * w.nS;
  for (uint64_t i = tid; i < items; i += nthreads) ul_links<MODE, CANON, MASKED, false>(w, i, nullptr);
}
U_SOLID_KERNELS(ul_count, (ULWork w), (w))

template <int MODE, bool CANON, bool MASKED>
__device__ __forceinline__ void ul_fill_body(const ULWork &w, cfrk_unitig_link *__restrict__ links) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t items = (CANON ? 2 : 1) * w.nS;
  for (uint64_t i = tid; i < items; i += nthreads) ul_links<MODE, CANON, MASKED, true>(w, i, links);
}
U_SOLID_KERNELS(ul_fill, (ULWork w, cfrk_unitig_link *__restrict__ links), (w, links))

// ---- 3 the scanned offsets to the caller ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ul_ptr_kernel(ULWork w, int o, int64_t *__restrict__ link_ptr) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = tid; j <= w.nS; j += nthreads) {
    const int64_t v = w.off[(uint64_t)o * j];
    link_ptr[j] = v;
    if (j == w.nS) w.ctr[ULC_TOTAL] = (unsigned long long)v;
  }
}

// the parts of BUF_UNITIG_LINKS (the same carve in both steps); the bytes of its scan scratch in *scan_tmp
int ul_carve(cfrk_ctx *ctx, const QIndex &q, bool canon, uint64_t nS, bool get, ULWork *w, void **tmp, size_t *scan_tmp, uint64_t *slots) {
  const uint64_t M = q.k <= 12 ? 1ull << (2 * q.k) : q.mask + 1, items = (canon ? 2 : 1) * nS;
  *slots = M;
  if (M > (1ull << 31)) return cfrk_fail(ctx, CFRK_ERR_ARG, "an index of %llu slots is too large for the unitig links", (unsigned long long)M);
  *scan_tmp = 0;
  HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, *scan_tmp, (int64_t *)nullptr, (size_t)(items + 1), ctx->stream));
  Carve c;
  const size_t o_ctr = c.part(ULC_WORDS * 8), o_tag = c.part(M * 8), o_off = c.part((items + 1) * 8), o_tmp = c.part(*scan_tmp);
  void *base = ctx->pool[BUF_UNITIG_LINKS].p;
  if (get) { if (const int rc = cfrk_pool_get(ctx, BUF_UNITIG_LINKS, c.end, &base)) return rc; }
  else if (!base || ctx->pool[BUF_UNITIG_LINKS].cap < c.end) return cfrk_fail(ctx, CFRK_ERR_STATE, "unitig links: fill without measure");
  w->q = q;
  w->ctr = carve_at<unsigned long long>(base, o_ctr);
  w->tag = carve_at<unsigned long long>(base, o_tag);
  w->off = carve_at<int64_t>(base, o_off);
  *tmp = carve_at<void>(base, o_tmp);
  return CFRK_OK;
}

}  // namespace

int cfrk_unitig_links_measure(cfrk_ctx *ctx, uint32_t min_count, const int8_t *d_data, const int64_t *d_start,
                              const int32_t *d_length, int64_t nN, int64_t nS, int64_t *d_link_ptr, int64_t *n_links) {
  QIndex q;
  int rc = cfrk_query_index(ctx, &q);
  if (rc) return rc;
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  const int mode = q.k <= 12 ? 0 : q.k <= 32 ? 1 : 2;
  ULWork w;
  void *tmp;
  size_t scan_tmp;
  uint64_t M;
  if ((rc = ul_carve(ctx, q, canon, (uint64_t)nS, true, &w, &tmp, &scan_tmp, &M))) return rc;
  w.data = d_data; w.start = d_start; w.length = d_length; w.nN = nN; w.nS = (uint64_t)nS;
  w.sol = u_solid_rule(ctx, min_count);
  const uint64_t items = (canon ? 2 : 1) * w.nS;
  HIP_TRY(ctx, hipMemsetAsync(w.ctr, 0xFF, 8, ctx->stream));                  // ULC_ERR: no unitig yet
  HIP_TRY(ctx, hipMemsetAsync(w.ctr + ULC_TOTAL, 0, 8, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w.tag, 0xFF, M * 8, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w.off + items, 0, 8, ctx->stream));
  U_DISPATCH_SOLID(ul_tag, w.sol, u_grid(ctx, 2 * w.nS), w);
  U_DISPATCH_SOLID(ul_count, w.sol, u_grid(ctx, items), w);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(tmp, scan_tmp, w.off, (size_t)(items + 1), ctx->stream));
  hipLaunchKernelGGL(ul_ptr_kernel, dim3(u_grid(ctx, w.nS + 1)), dim3(256), 0, ctx->stream, w, canon ? 2 : 1, d_link_ptr);
  HIP_TRY(ctx, hipGetLastError());
  unsigned long long h[ULC_WORDS];
  HIP_TRY(ctx, hipMemcpyAsync(h, w.ctr, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (h[ULC_ERR] != UL_EMPTY) {
    const unsigned long long j = (h[ULC_ERR] >> 8) & 0xFFFFFFFFull;
    const int why = (int)(h[ULC_ERR] & 255);
    const char *what = why == ULE_RANGE     ? "is shorter than k or does not lie inside the data"
                       : why == ULE_CODE    ? "has an invalid code in an end k-mer"
                       : why == ULE_ABSENT  ? "has an end k-mer that is not a solid key of this job at this min_count"
                       : why == ULE_CLAIMED ? "has an end k-mer that another unitig end of the input has as well"
                                            : "has a tail with a solid successor that no unitig of the input begins with";
    return cfrk_fail(ctx, CFRK_ERR_LAYOUT, "unitig %llu %s: not the unitigs of this job at this min_count", j, what);
  }
  *n_links = (int64_t)h[ULC_TOTAL];
  return CFRK_OK;
}

int cfrk_unitig_links_fill(cfrk_ctx *ctx, uint32_t min_count, const int8_t *d_data, const int64_t *d_start,
                           const int32_t *d_length, int64_t nN, int64_t nS, cfrk_unitig_link *d_links) {
  QIndex q;
  int rc = cfrk_query_index(ctx, &q);
  if (rc) return rc;
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  const int mode = q.k <= 12 ? 0 : q.k <= 32 ? 1 : 2;
  ULWork w;
  void *tmp;
  size_t scan_tmp;
  uint64_t M;
  if ((rc = ul_carve(ctx, q, canon, (uint64_t)nS, false, &w, &tmp, &scan_tmp, &M))) return rc;
  w.data = d_data; w.start = d_start; w.length = d_length; w.nN = nN; w.nS = (uint64_t)nS;
  w.sol = u_solid_rule(ctx, min_count);
  U_DISPATCH_SOLID(ul_fill, w.sol, u_grid(ctx, (canon ? 2 : 1) * w.nS), w, d_links);
  HIP_TRY(ctx, hipGetLastError());
  return CFRK_OK;
}
