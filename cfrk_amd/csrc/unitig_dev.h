// unitig_dev.h -- what the graph kernels share (unitigs.hip, unitig_links.hip, unitig_locate.hip, unitig_mask.hip): k-mers as
// 128-bit numbers, the node (index slot and orientation) of an oriented k-mer, the one test of solidity (count and graph
// mask), the grid size and the dispatch over the three index modes and the two strand rules.
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

// ---- solid keys -------------------------------------------------------------------------------------------------
// A slot holds a SOLID key iff its count is >= min_count (an empty slot counts 0, min_count >= 1) and the key is not
// masked.  The mask is one byte per index slot beside the index (BUF_UNITIG_MASK), NULL while no key is masked: the
// index itself, and with it every count-form walker, knows nothing of it.
struct USolid {
  uint32_t min_count;
  const uint8_t *mask;
};
// MASKED is a template parameter of the kernels, not a test of the pointer: without a mask they are the code they were
// (measured: DESIGN 4.22).
template <int MODE, bool MASKED>
__device__ __forceinline__ bool u_solid(const QIndex &q, const USolid &s, uint64_t slot) {
  if (slot == Q_NO_SLOT || q_slot_count<MODE>(q, slot) < s.min_count) return false;
  return !MASKED || s.mask[slot] == 0;
}

// the mask of the index as it is built now (after cfrk_query_index), NULL when there is none
const uint8_t *u_mask(const cfrk_ctx *ctx) {
  if (!ctx->q_valid || ctx->umask_epoch == 0 || ctx->umask_epoch != ctx->q_epoch) return nullptr;
  return static_cast<const uint8_t *>(ctx->pool[BUF_UNITIG_MASK].p);
}
USolid u_solid_rule(const cfrk_ctx *ctx, uint32_t min_count) {
  USolid s;
  s.min_count = min_count ? min_count : 1;
  s.mask = u_mask(ctx);
  return s;
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

// NAME_kernel<MODE, CANON> and NAME_masked_kernel<MODE, CANON> around NAME_body<MODE, CANON, MASKED>; the launch of the
// one the solidity rule asks for
#define U_SOLID_KERNELS(NAME, PARAMS, ARGS)                                                                             \
  template <int MODE, bool CANON> __global__ __launch_bounds__(256) void NAME##_kernel PARAMS { NAME##_body<MODE, CANON, false> ARGS; } \
  template <int MODE, bool CANON> __global__ __launch_bounds__(256) void NAME##_masked_kernel PARAMS { NAME##_body<MODE, CANON, true> ARGS; }
#define U_DISPATCH_SOLID(NAME, sol, grid, ...)                                                                          \
  do {                                                                                                                  \
    if ((sol).mask) U_DISPATCH(NAME##_masked_kernel, grid, __VA_ARGS__);                                                \
    else U_DISPATCH(NAME##_kernel, grid, __VA_ARGS__);                                                                  \
  } while (0)

}  // namespace
#endif  // __HIPCC__
