// unitig_mask.hip -- the graph mask: stored keys that are no longer part of the graph.  One byte per slot of the lookup
// index, beside the index (BUF_UNITIG_MASK), read by the one solidity test of unitig_dev.h and by nothing else: counts,
// digest, export and every count-form walker never see it.  The contract is in include/cfrk_abi.h ("Graph mask");
// DESIGN 4.22 has the reasoning.
//
// The mask belongs to one build of the index (ctx->umask_epoch == ctx->q_epoch), as the position map does: a rebuilt
// index has no mask.  Every change of the mask drops the position map (ctx->upos_epoch = 0), whose positions were those
// of another graph.
//
//   keys      one lane per key: range check, canonical form, slot, one plain byte store
//   unitigs   one workgroup per tile of UM_TILE window starts of the list's BYTES, 32 consecutive starts per thread, as
//             the claim pass of the position map: the read a window lies in from a binary search in start[], its drop
//             byte, the slot, one plain byte store.  No lane's work grows with a unitig's length.
//   count     one lane per slot, a wave's sum added by one lane
// Every store is the value 1 to a byte only this file writes: lanes that meet at a slot write the same thing.
#include "read_windows.h"
#include "staging.h"
#include "unitig_dev.h"

namespace {

constexpr int UM_TILE = 8192;                         // window starts per workgroup and turn
constexpr int UM_PER = UM_TILE / 256;                 // ... per thread

template <int MODE, bool CANON>
__global__ __launch_bounds__(256) void um_keys_kernel(QIndex q, const uint64_t *__restrict__ keys_lo,
                                                      const uint64_t *__restrict__ keys_hi, int64_t n, uint8_t *__restrict__ mask) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  const int k = q.k;
  for (int64_t i = tid; i < n; i += nthreads) {
    const uint64_t lo = keys_lo[i], hi = keys_hi ? keys_hi[i] : 0;
    bool in;                                            // no bits at or above 2k
    if (MODE < 2) in = hi == 0 && (k >= 32 || (lo >> (2 * k)) == 0);
    else in = k >= 64 || (hi >> (2 * k - 64)) == 0;
    if (!in) continue;
    int o; bool pal;
    const uint64_t slot = u_node<MODE, CANON>(q, u_make(lo, hi), o, pal);
    if (slot != Q_NO_SLOT) mask[slot] = 1;
  }
}

struct UMWork {
  QIndex q;
  const int8_t *data; const int64_t *start; const int32_t *length;
  int64_t nN;
  uint64_t nS;
  const uint8_t *drop;
  uint8_t *mask;
};

// the last read whose start is <= x, -1 when there is none (start[] ascending, as the struct-read layout has it; any
// other table only makes windows go unmasked: every index stays below nS)
__device__ __forceinline__ int64_t um_search(const UMWork &w, int64_t x) {
  uint64_t lo = 0, hi = w.nS;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (w.start[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return (int64_t)lo - 1;
}

// reads data[] only at offsets below nN, start[], length[] and drop[] only at indices below nS, whatever they hold
template <int MODE, bool CANON>
__global__ __launch_bounds__(256) void um_unitigs_kernel(UMWork w) {
  const int k = w.q.k;
  const int64_t nwin = w.nN - k + 1;                    // window starts whose k bytes lie below nN
  const int64_t ntiles = (nwin + UM_TILE - 1) / UM_TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t a = tile * UM_TILE + (int64_t)threadIdx.x * UM_PER;
    const int64_t b = a + UM_PER < nwin ? a + UM_PER : nwin;
    if (a >= b) continue;
    int64_t j = um_search(w, a);
    Roller<MODE == 2, CANON> R(k);
    for (int64_t p = a; p < b + k - 1; ++p) {           // p <= nwin + k - 2 = nN - 1
      R.push((int)w.data[p]);
      if (p < a + k - 1) continue;
      const int64_t ws = p - (k - 1);
      if ((uint64_t)(j + 1) < w.nS && w.start[j + 1] <= ws) j = um_search(w, ws);
      if (j < 0) continue;
      const int64_t s = w.start[j], len = w.length[j];
      if (s < 0 || s > ws || len < k || ws - s > len - k) continue;     // between two reads, or a read outside [0, nN)
      if (!R.valid() || w.drop[j] == 0) continue;
      const auto key = R.key();
      const uint64_t slot = q_slot_of<MODE>(w.q, (uint64_t)key, (uint64_t)(key >> (MODE == 2 ? 64 : 0)));
      if (slot != Q_NO_SLOT) w.mask[slot] = 1;
    }
  }
}

template <int MODE, bool CANON>
__global__ __launch_bounds__(256) void um_count_kernel(QIndex q, const uint8_t *__restrict__ mask, unsigned long long *__restrict__ out) {
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t M = q_nslots<MODE>(q);
  unsigned long long n = 0;
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < M; s += nthreads)
    if (mask[s] != 0 && q_slot_count<MODE>(q, s) != 0) ++n;
  n = group_sum_u64<64>(n);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(out, n);
}

// the index (built when it is not valid) and its mask, cleared when it was that of another build; the map is dropped
int um_open(cfrk_ctx *ctx, QIndex *q, uint8_t **mask) {
  int rc = cfrk_query_index(ctx, q);
  if (rc) return rc;
  const uint64_t M = q->k <= 12 ? 1ull << (2 * q->k) : q->mask + 1;
  void *p;
  if ((rc = cfrk_pool_get(ctx, BUF_UNITIG_MASK, M, &p))) return rc;
  if (ctx->umask_epoch != ctx->q_epoch) {
    ctx->umask_epoch = 0;
    HIP_TRY(ctx, hipMemsetAsync(p, 0, M, ctx->stream));
    ctx->umask_epoch = ctx->q_epoch;
  }
  ctx->upos_epoch = 0;
  *mask = static_cast<uint8_t *>(p);
  return CFRK_OK;
}

}  // namespace

int cfrk_mask_keys_launch(cfrk_ctx *ctx, const uint64_t *d_lo, const uint64_t *d_hi, int64_t n) {
  QIndex q;
  uint8_t *mask;
  int rc = um_open(ctx, &q, &mask);
  if (rc || n == 0) return rc;
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  const int mode = q.k <= 12 ? 0 : q.k <= 32 ? 1 : 2;
  U_DISPATCH(um_keys_kernel, u_grid(ctx, (uint64_t)n), q, d_lo, d_hi, n, mask);
  HIP_TRY(ctx, hipGetLastError());
  return CFRK_OK;
}

int cfrk_mask_unitigs_launch(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                             int64_t nS, const uint8_t *d_drop) {
  UMWork w;
  int rc = um_open(ctx, &w.q, &w.mask);
  if (rc || nS == 0 || nN < w.q.k) return rc;
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  const int mode = w.q.k <= 12 ? 0 : w.q.k <= 32 ? 1 : 2;
  w.data = d_data; w.start = d_start; w.length = d_length; w.nN = nN; w.nS = (uint64_t)nS; w.drop = d_drop;
  const int64_t ntiles = (nN - w.q.k + 1 + UM_TILE - 1) / UM_TILE;
  const int grid = (int)std::min<int64_t>(ntiles, (int64_t)ctx->num_cus * 16);
  U_DISPATCH(um_unitigs_kernel, grid, w);
  HIP_TRY(ctx, hipGetLastError());
  return CFRK_OK;
}

int cfrk_mask_clear_now(cfrk_ctx *ctx) {
  if (u_mask(ctx)) ctx->upos_epoch = 0;
  ctx->umask_epoch = 0;
  return CFRK_OK;
}

int cfrk_mask_count_now(cfrk_ctx *ctx, uint64_t *n_masked) {
  QIndex q;
  int rc = cfrk_query_index(ctx, &q);
  if (rc) return rc;
  *n_masked = 0;
  const uint8_t *mask = u_mask(ctx);
  if (!mask) return CFRK_OK;
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  const int mode = q.k <= 12 ? 0 : q.k <= 32 ? 1 : 2;
  void *p;
  if ((rc = cfrk_pool_get(ctx, BUF_UNITIG_MASK_AUX, 8, &p))) return rc;
  unsigned long long *d_n = static_cast<unsigned long long *>(p);
  HIP_TRY(ctx, hipMemsetAsync(d_n, 0, 8, ctx->stream));
  const uint64_t M = q.k <= 12 ? 1ull << (2 * q.k) : q.mask + 1;
  U_DISPATCH(um_count_kernel, u_grid(ctx, M), q, mask, d_n);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(n_masked, d_n, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CFRK_OK;
}
