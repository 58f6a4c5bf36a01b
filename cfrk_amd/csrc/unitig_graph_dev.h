// unitig_graph_dev.h -- what the rules over the compacted graph share (unitig_tips.hip, unitig_bubbles.hip): the unitig
// records and the link CSR as untrusted arrays, the check that runs in front of every rule, and the in-rows of a job that
// is not canonical.  Every pass behind the check reads the error word first and does nothing when it is set, so that only
// checked rows are ever followed:
//   check     one lane per unitig: link_ptr[j] <= link_ptr[j + 1] inside [0, n_links] (0 at j = 0, n_links at the
//             end), a row of at most 16 links (4 when not canonical), targets below nS, no undefined flag bit (none
//             at all when not canonical).  Not canonical: a checked row counts its targets' in-degrees.
//   not canonical only, where in() cannot be read off a unitig's own row:
//   in-degree one lane per unitig: at most 4; hipCUB exclusive sum over the in-degrees, in place
//   in-rows   one lane per unitig: its links' sources into the targets' in-rows, a cursor per target (the order inside
//             an in-row does not matter: the rules only ask "is there one" or "which is the only one")
// Each file that includes this instantiates the kernels for itself; a rule's own work struct derives from UGraph.  The
// three kernels keep the names they had in unitig_tips.hip (ut_*), which the resource tests look for.
#pragma once

#include "staging.h"
#include "unitig_dev.h"

#include <hipcub/hipcub.hpp>

#ifdef __HIPCC__
namespace {

constexpr unsigned long long UG_NONE = ~0ull;
enum { UGC_ERR = 0 };                 // ctr[0] of every rule: the error word; the rule's own counters follow
// error word = unitig << 8 | why, kept with an atomic minimum: the first offending unitig
enum { UGE_PTR = 1, UGE_ROW, UGE_TARGET, UGE_FLAGS, UGE_INDEG };

struct UGraph {
  const cfrk_unitig *rec;
  const int64_t *ptr;
  const cfrk_unitig_link *links;
  uint64_t nS;
  int64_t n_links;
  unsigned long long *ctr;            // UGC_ERR, then the rule's own words
  unsigned long long *in_off;         // [nS + 1], not canonical: in-degrees, scanned into the in-rows' offsets
  uint32_t *in_cur;                   // [nS]: the fill pass's cursors
  uint32_t *in_src;                   // [n_links]: the in-rows
};

__device__ __forceinline__ void ug_fail(const UGraph &w, uint64_t j, int why) {
  atomicMin(&w.ctr[UGC_ERR], (unsigned long long)((j << 8) | (uint64_t)why));
}

// ---- check ------------------------------------------------------------------------------------------------------
template <bool CANON>
__global__ __launch_bounds__(256) void ut_check_kernel(UGraph w) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = tid; j < w.nS; j += nthreads) {
    const int64_t a = w.ptr[j], b = w.ptr[j + 1];
    int why = 0;
    if ((j == 0 && a != 0) || (j + 1 == w.nS && b != w.n_links) || a < 0 || b < a || b > w.n_links) why = UGE_PTR;
    else if (b - a > (CANON ? 16 : 4)) why = UGE_ROW;
    else
      for (int64_t t = a; t < b; ++t) {
        const cfrk_unitig_link l = w.links[t];
        if (l.to >= w.nS) { why = UGE_TARGET; break; }
        if (l.flags & ~(CANON ? (uint32_t)(CFRK_LINK_FROM_MINUS | CFRK_LINK_TO_MINUS) : 0u)) { why = UGE_FLAGS; break; }
      }
    if (why) { ug_fail(w, j, why); continue; }
    if (!CANON)
      for (int64_t t = a; t < b; ++t) atomicAdd(&w.in_off[w.links[t].to], 1ull);
  }
}

// ---- the in-rows of a job that is not canonical -----------------------------------------------------------------
__global__ __launch_bounds__(256) void ut_indeg_kernel(UGraph w) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = tid; j < w.nS; j += nthreads)
    if (w.in_off[j] > 4) ug_fail(w, j, UGE_INDEG);
}

__global__ __launch_bounds__(256) void ut_in_fill_kernel(UGraph w) {
  if (w.ctr[UGC_ERR] != UG_NONE) return;
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

// ---- host side --------------------------------------------------------------------------------------------------
// the scan's scratch for nS unitigs of a job that is not canonical (0 for a canonical one)
int ug_scan_bytes(cfrk_ctx *ctx, bool canon, uint64_t n, size_t *bytes) {
  *bytes = 0;
  if (!canon) HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, (unsigned long long *)nullptr, (size_t)(n + 1), ctx->stream));
  return CFRK_OK;
}

// the error word set to "no unitig yet", then the check; not canonical: the in-degrees, their scan and the in-rows.
// in_rows false: a caller that never reads in() gets the check and the in-degree refusal alone (in_off holds counts,
// in_cur, in_src and the scan's scratch are not touched)
int ug_check_launch(cfrk_ctx *ctx, const UGraph &g, bool canon, int grid, void *scan_tmp, size_t scan_bytes, bool in_rows = true) {
  HIP_TRY(ctx, hipMemsetAsync(g.ctr, 0xFF, 8, ctx->stream));
  if (canon) {
    hipLaunchKernelGGL(ut_check_kernel<true>, dim3(grid), dim3(256), 0, ctx->stream, g);
    return CFRK_OK;
  }
  HIP_TRY(ctx, hipMemsetAsync(g.in_off, 0, (g.nS + 1) * 8, ctx->stream));
  if (in_rows) HIP_TRY(ctx, hipMemsetAsync(g.in_cur, 0, g.nS * 4, ctx->stream));
  hipLaunchKernelGGL(ut_check_kernel<false>, dim3(grid), dim3(256), 0, ctx->stream, g);
  hipLaunchKernelGGL(ut_indeg_kernel, dim3(grid), dim3(256), 0, ctx->stream, g);
  HIP_TRY(ctx, hipGetLastError());
  if (!in_rows) return CFRK_OK;
  HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, g.in_off, (size_t)(g.nS + 1), ctx->stream));
  hipLaunchKernelGGL(ut_in_fill_kernel, dim3(grid), dim3(256), 0, ctx->stream, g);
  return CFRK_OK;
}

// CFRK_ERR_LAYOUT for a set error word
int ug_layout_error(cfrk_ctx *ctx, unsigned long long word) {
  const unsigned long long j = word >> 8;
  const int why = (int)(word & 255);
  const char *what = why == UGE_PTR      ? "has a link_ptr that does not ascend from 0 to n_links"
                     : why == UGE_ROW    ? "has a row of more links than an oriented end can have"
                     : why == UGE_TARGET ? "has a link to a unitig that is not in the list"
                     : why == UGE_FLAGS  ? "has a link with an undefined flag bit, or a strand flag in a job that is not canonical"
                                         : "is entered by more than 4 links";
  return cfrk_fail(ctx, CFRK_ERR_LAYOUT, "unitig %llu %s: not the links of a unitig list of this strand rule", j, what);
}

}  // namespace
#endif  // __HIPCC__
