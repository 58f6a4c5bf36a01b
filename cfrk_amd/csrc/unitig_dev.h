// unitig_dev.h -- what the graph kernels share (unitigs.hip, unitig_links.hip, unitig_locate.hip): k-mers as 128-bit numbers, the node
// (index slot and orientation) of an oriented k-mer, the grid size and the dispatch over the three index modes and
// the two strand rules.
#pragma once

#include "query_dev.h"

#include <algorithm>

#ifdef __HIPCC__
namespace {

typedef unsigned __int128 u128;

// ---- k-mers as 128-bit numbers (first base most significant) ---------------------------------------------------
__device__ __forceinline__ u128 u_make(uint64_t lo, uint64_t hi) { return ((u128)hi << 64) | lo; }
__device__ __forceinline__ u128 u_kmask(int k) { return k == 64 ? ~(u128)0 : ((((u128)1) << (2 * k)) - 1); }
__device__ __forceinline__ u128 u_rc(u128 x, int k) {
  const u128 r = ((u128)dev_revcomp64((uint64_t)x, 32) << 64) | dev_revcomp64((uint64_t)(x >> 64), 32);
  return r >> (128 - 2 * k);
}
__device__ __forceinline__ u128 u_succ_key(u128 x, int b, int k) { return ((x << 2) | (u128)(unsigned)b) & u_kmask(k); }
__device__ __forceinline__ u128 u_pred_key(u128 x, int b, int k) { return (x >> 2) | ((u128)(unsigned)b << (2 * (k - 1))); }

// ---- nodes ------------------------------------------------------------------------------------------------------
// the slot and the orientation of oriented k-mer z (in range); pal: z is its own reverse complement
template <int MODE, bool CANON>
__device__ __forceinline__ uint64_t u_node(const QIndex &q, u128 z, int &o, bool &pal) {
  o = 0; pal = false;
  if (CANON) {
    const u128 r = u_rc(z, q.k);
    pal = r == z;
    if (r < z) { z = r; o = 1; }
  }
  return q_slot_of<MODE>(q, (uint64_t)z, (uint64_t)(z >> 64));
}

int u_grid(const cfrk_ctx *ctx, uint64_t items) {
  const uint64_t want = (items + 255) / 256;
  return (int)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)ctx->num_cus * 16));
}

// KERNEL<MODE, CANON> on the context stream; `mode`, `canon` and `ctx` are the caller's
#define U_DISPATCH(KERNEL, grid, ...)                                                                                   \
  do {                                                                                                                  \
    if (mode == 0) { if (canon) hipLaunchKernelGGL((KERNEL<0, true>), dim3(grid), dim3(256), 0, ctx->stream, __VA_ARGS__);  \
                     else hipLaunchKernelGGL((KERNEL<0, false>), dim3(grid), dim3(256), 0, ctx->stream, __VA_ARGS__); }     \
    else if (mode == 1) { if (canon) hipLaunchKernelGGL((KERNEL<1, true>), dim3(grid), dim3(256), 0, ctx->stream, __VA_ARGS__); \
                          else hipLaunchKernelGGL((KERNEL<1, false>), dim3(grid), dim3(256), 0, ctx->stream, __VA_ARGS__); }    \
    else { if (canon) hipLaunchKernelGGL((KERNEL<2, true>), dim3(grid), dim3(256), 0, ctx->stream, __VA_ARGS__);            \
           else hipLaunchKernelGGL((KERNEL<2, false>), dim3(grid), dim3(256), 0, ctx->stream, __VA_ARGS__); }               \
  } while (0)

}  // namespace
#endif  // __HIPCC__
