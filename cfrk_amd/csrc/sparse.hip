// sparse.hip -- per-read SPARSE k-mer counts for gfx950: for every read its distinct k-mers in ascending order with
// their multiplicities, as CSR (row offsets, keys, counts).  1 <= k <= 32 (one-word keys), optional canonical k-mers.
// Semantics: the guarded ComputeFreq (what dense.hip does without CFRK_COMPAT), i.e. row i = the non-zero bins of the
// dense row i -- without the dense layout's nS * 4^k int32, which ends the dense form at k = 15 (and in practice at 8).
//
// Count pass, sparse_count_kernel<G, CANON>: G lanes of one wave own a read (the size classes and the three launches
// are lane_group.h's).  The read's codes are staged in LDS; every lane rolls its run of windows (read_windows.h's
// Roller); the keys go to LDS, an invalid window as the all-ones word.  The group sorts its keys in LDS with a bitonic
// network whose compare-exchanges all point upwards (so positions at and beyond n read as +infinity and a row needs no
// padding).  Invalid windows sort to the end: the first (windows - invalid) keys are the valid ones (an all-T 32-mer is
// the all-ones word too, but equal words are interchangeable).  Heads of runs of equal keys are flagged, a ballot gives
// every head its place, the run's end is found by bisection in LDS, and (key, count) are stored -- neighbouring heads
// to neighbouring addresses -- into a temporary slot of the context pool at the read's own offset start[i]: read i has
// at most length[i] windows and the reads' byte ranges are disjoint, so nN entries suffice and no sizes are needed
// beforehand.  No HBM atomics, no scratch.  The row's distinct count goes to row_ptr[i].
// Long reads: sparse_long_sort_kernel, one workgroup per read, writes the raw keys to the read's temporary range and
// sorts them there with the same network (the range stays in the L2), then sparse_runlength_kernel collapses the runs
// in place.  Exact for any length; a slow path, not the fast one.
// Scan: three small kernels turn the counts into offsets in place (reduce per block, scan of the block sums, apply).
// Compaction pass, sparse_compact_kernel: every row moves from its temporary place to row_ptr[i].
#include "common.h"
#include "lane_group.h"
#include "read_windows.h"

namespace {

constexpr int SP_PAD = 16;                             // keys between the groups' arrays: neighbouring groups half a bank row apart
constexpr int SP_STAGE_SLACK = 48;                     // k - 1 <= 31 bytes + skew <= 3 + dword round-up <= 3, kept a multiple of 8
constexpr int SP_BIG_ROW = 4096;                       // compaction: rows above this are copied by the whole workgroup
constexpr int SP_SCAN_ITEMS = 16;                      // scan: items per thread (256 threads: 4096 per block)

// first index in (idx, n) whose key differs from a[idx] (n when there is none); a is sorted
__device__ __forceinline__ int run_end(const uint64_t *a, int idx, int n, uint64_t key) {
  int lo = idx + 1, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] == key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

template <int G, bool CANON>
__device__ __forceinline__ void count_read(const int8_t *__restrict__ data, int64_t nN, int64_t i, int64_t st, int nwin,
                                           int k, uint64_t *keys, int32_t *stage_dw, int lane, int wave_lane,
                                           uint64_t *__restrict__ tmp_keys, uint32_t *__restrict__ tmp_cnt,
                                           int64_t *__restrict__ row_ptr) {
  const int skew = stage_read<G>(data, nN, st, nwin + k - 1, stage_dw, lane);
  wave_sync();
  const int8_t *stage = reinterpret_cast<const int8_t *>(stage_dw) + skew;
  const int per = (nwin + G - 1) / G;
  const int t0 = lane * per, t1 = min(t0 + per, nwin);
  int invalid = 0;
  if (t0 < t1) {
    Roller<false, CANON> R(k);
    for (int p = t0; p < t1 + k - 1; ++p) {
      R.push((int)stage[p]);
      if (p >= t0 + k - 1) {
        uint64_t key = R.key();
        if (!R.valid()) { key = ~0ull; ++invalid; }
        keys[p - (k - 1)] = key;
      }
    }
  }
  const int nvalid = nwin - group_sum<G>(invalid);
  wave_sync();
  sort_keys(keys, nwin, lane, G, WaveSync());
  // heads of runs -> (key, count), in order, to the read's temporary range
  const int gshift = wave_lane & ~(G - 1);
  int running = 0;
  for (int base = 0; base < nvalid; base += G) {
    const int idx = base + lane;
    const bool act = idx < nvalid;
    const uint64_t key = act ? keys[idx] : 0;
    const bool head = act && (idx == 0 || keys[idx - 1] != key);
    const int end = head ? run_end(keys, idx, nvalid, key) : 0;
    unsigned long long m = __ballot(head) >> gshift;
    if (G < 64) m &= (1ull << G) - 1;
    if (head) {
      const int pos = running + __popcll(m & ((1ull << lane) - 1));
      tmp_keys[st + pos] = key;
      tmp_cnt[st + pos] = (uint32_t)(end - idx);
    }
    running += __popcll(m);
  }
  if (lane == 0) row_ptr[i] = running;
  wave_sync();     // the group's LDS is reused by its next read
}

template <int G, bool CANON>
__global__ __launch_bounds__(G == 16 ? 256 : 64) void sparse_count_kernel(
    const int8_t *__restrict__ data, const int64_t *__restrict__ start, const int32_t *__restrict__ length, int64_t nN,
    int64_t nS, int k, uint64_t *__restrict__ tmp_keys, uint32_t *__restrict__ tmp_cnt, int64_t *__restrict__ row_ptr) {
  constexpr int RPB = (G == 16 ? 256 : 64) / G;
  constexpr int CAP = (G == 16) ? READ_CAP16 : READ_CAP64;
  __shared__ uint64_t s_keys[RPB][CAP + SP_PAD];
  __shared__ int32_t s_stage[RPB][(CAP + SP_STAGE_SLACK) / 4];
  const int grp = G == 16 ? threadIdx.x / G : 0, lane = threadIdx.x % G, wave_lane = threadIdx.x & 63;
  class_reads<G>(
      start, length, nN, nS, k,
      [&](int64_t i, int64_t st, int nwin) {
        count_read<G, CANON>(data, nN, i, st, nwin, k, s_keys[grp], s_stage[grp], lane, wave_lane, tmp_keys, tmp_cnt,
                             row_ptr);
      },
      [&](int64_t i) { if (lane == 0) row_ptr[i] = 0; });
}

// ---- long reads -----------------------------------------------------------------------------

constexpr int SP_LONG_NT = 1024;

// raw keys (invalid windows as the all-ones word) into the read's temporary range, sorted there.  row_ptr[i] receives
// the number of VALID windows (sparse_runlength_kernel turns it into the distinct count).
template <bool CANON>
__global__ __launch_bounds__(SP_LONG_NT) void sparse_long_sort_kernel(
    const int8_t *__restrict__ data, const int64_t *__restrict__ start, const int32_t *__restrict__ length, int64_t nN,
    int64_t nS, int k, uint64_t *tmp_keys, int64_t *__restrict__ row_ptr) {
  __shared__ int s_invalid;
  const int tid = threadIdx.x;
  // (the body ends on a barrier: s_invalid is reset by the next read)
  long_reads<SP_LONG_NT, true>(start, length, nN, nS, k, [&](int64_t i, int64_t st, int nwin) {
    uint64_t *seg = tmp_keys + st;                     // length[i] >= nwin entries
    if (tid == 0) s_invalid = 0;
    __syncthreads();
    int invalid = 0;
    for (int c0 = tid * 32; c0 < nwin; c0 += SP_LONG_NT * 32) {
      const int c1 = min(c0 + 32, nwin);
      Roller<false, CANON> R(k);
      for (int p = c0; p < c1 + k - 1; ++p) {          // st + p <= st + length[i] - 1
        R.push((int)data[st + p]);
        if (p >= c0 + k - 1) {
          uint64_t key = R.key();
          if (!R.valid()) { key = ~0ull; ++invalid; }
          seg[p - (k - 1)] = key;
        }
      }
    }
    if (invalid) atomicAdd(&s_invalid, invalid);
    __syncthreads();
    sort_keys(seg, nwin, tid, SP_LONG_NT, BlockSync());
    if (tid == 0) row_ptr[i] = nwin - s_invalid;
    __syncthreads();
  });
}

// runs of equal keys of every long read -> (key, count), in place at the front of the read's temporary range
__global__ __launch_bounds__(256) void sparse_runlength_kernel(
    const int64_t *__restrict__ start, const int32_t *__restrict__ length, int64_t nN, int64_t nS, int k,
    uint64_t *tmp_keys, uint32_t *tmp_cnt, int64_t *row_ptr) {
  __shared__ int s_wsum[4];
  const int tid = threadIdx.x, wl = tid & 63, wv = tid >> 6;
  // (the body ends on a barrier, also for a read without a tile)
  long_reads<256, true>(start, length, nN, nS, k, [&](int64_t i, int64_t st, int) {
    const int nvalid = (int)row_ptr[i];
    uint64_t *seg = tmp_keys + st;
    uint32_t *cseg = tmp_cnt + st;
    int running = 0;
    // a tile reads its keys (and its heads their runs' ends) before anything of it is written; what it writes lies
    // at or below the indices it read, so later tiles still find their keys (seg[tile - 1] can only have been
    // replaced by itself)
    for (int t0 = 0; t0 < nvalid; t0 += 256) {
      const int idx = t0 + tid;
      const bool act = idx < nvalid;
      const uint64_t key = act ? seg[idx] : 0;
      const bool head = act && (idx == 0 || seg[idx - 1] != key);
      const int end = head ? run_end(seg, idx, nvalid, key) : 0;
      const unsigned long long m = __ballot(head);
      if (wl == 0) s_wsum[wv] = __popcll(m);
      __syncthreads();
      int pos = running + __popcll(m & ((1ull << wl) - 1)), total = 0;
      for (int w = 0; w < 4; ++w) { if (w < wv) pos += s_wsum[w]; total += s_wsum[w]; }
      if (head) { seg[pos] = key; cseg[pos] = (uint32_t)(end - idx); }
      running += total;
      __syncthreads();
    }
    if (tid == 0) row_ptr[i] = running;
    __syncthreads();
  });
}

// ---- counts -> offsets ------------------------------------------------------------------------

// exclusive prefix of v over the 256 threads of the workgroup; total = their sum
__device__ __forceinline__ int64_t block_scan_excl(int64_t v, int64_t *s_w, int64_t &total) {
  const int wl = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int64_t inc = v;
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t u = __shfl_up(inc, o);
    if (wl >= o) inc += u;
  }
  if (wl == 63) s_w[wv] = inc;
  __syncthreads();
  int64_t pre = 0;
  total = 0;
  for (int w = 0; w < nw; ++w) { if (w < wv) pre += s_w[w]; total += s_w[w]; }
  __syncthreads();
  return pre + inc - v;
}

__global__ __launch_bounds__(256) void sparse_scan_reduce_kernel(const int64_t *__restrict__ x, int64_t n, int64_t *__restrict__ bsum) {
  __shared__ int64_t s_w[4];
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * SP_SCAN_ITEMS;
  int64_t v = 0;
  for (int j = 0; j < SP_SCAN_ITEMS; ++j) if (i0 + j < n) v += x[i0 + j];
  int64_t total;
  block_scan_excl(v, s_w, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: the block sums become block offsets; the grand total goes to *total_out (row_ptr[nS])
__global__ __launch_bounds__(256) void sparse_scan_sums_kernel(int64_t *bsum, int64_t nb, int64_t *total_out) {
  __shared__ int64_t s_w[4];
  int64_t carry = 0;
  for (int64_t c = 0; c < nb; c += 256) {
    const int64_t j = c + threadIdx.x;
    const int64_t v = (j < nb) ? bsum[j] : 0;
    int64_t total;
    const int64_t ex = block_scan_excl(v, s_w, total);
    if (j < nb) bsum[j] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) *total_out = carry;
}

__global__ __launch_bounds__(256) void sparse_scan_apply_kernel(int64_t *x, int64_t n, const int64_t *__restrict__ bsum) {
  __shared__ int64_t s_w[4];
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * SP_SCAN_ITEMS;
  int64_t item[SP_SCAN_ITEMS];
  int64_t v = 0;
#pragma unroll
  for (int j = 0; j < SP_SCAN_ITEMS; ++j) { item[j] = (i0 + j < n) ? x[i0 + j] : 0; v += item[j]; }
  int64_t total;
  int64_t at = bsum[blockIdx.x] + block_scan_excl(v, s_w, total);
#pragma unroll
  for (int j = 0; j < SP_SCAN_ITEMS; ++j) {
    if (i0 + j < n) x[i0 + j] = at;
    at += item[j];
  }
}

// ---- compaction ---------------------------------------------------------------------------------

// row i: temporary range at start[i] -> [row_ptr[i], row_ptr[i+1]).  16 lanes per row (neighbouring lanes move
// neighbouring entries: 128 contiguous bytes of keys per group and instruction); a row above SP_BIG_ROW entries is
// left to the whole workgroup.
__global__ __launch_bounds__(256) void sparse_compact_kernel(
    const int64_t *__restrict__ start, const int64_t *__restrict__ row_ptr, int64_t nS,
    const uint64_t *__restrict__ tmp_keys, const uint32_t *__restrict__ tmp_cnt, uint64_t *__restrict__ out_keys,
    uint32_t *__restrict__ out_cnt) {
  __shared__ int s_big[16];
  __shared__ int s_nbig;
  const int tid = threadIdx.x, grp = tid >> 4, lane = tid & 15;
  for (int64_t base = (int64_t)blockIdx.x * 16; base < nS; base += (int64_t)gridDim.x * 16) {
    if (tid == 0) s_nbig = 0;
    __syncthreads();
    const int64_t i = base + grp;
    if (i < nS) {
      const int64_t rp = row_ptr[i], n = row_ptr[i + 1] - rp;
      if (n > SP_BIG_ROW) {
        if (lane == 0) s_big[atomicAdd(&s_nbig, 1)] = grp;
      } else if (n > 0) {
        const int64_t st = start[i];
        for (int64_t j = lane; j < n; j += 16) {
          out_keys[rp + j] = tmp_keys[st + j];
          out_cnt[rp + j] = tmp_cnt[st + j];
        }
      }
    }
    __syncthreads();
    const int nbig = s_nbig;
    for (int q = 0; q < nbig; ++q) {
      const int64_t r = base + s_big[q];
      const int64_t rp = row_ptr[r], n = row_ptr[r + 1] - rp, st = start[r];
      for (int64_t j = tid; j < n; j += 256) {
        out_keys[rp + j] = tmp_keys[st + j];
        out_cnt[rp + j] = tmp_cnt[st + j];
      }
    }
    __syncthreads();
  }
}

}  // namespace

// Counts every read into the temporary slots and turns the per-read distinct counts into offsets: on return (kernels
// enqueued) d_row_ptr[0 .. nS] is the CSR row pointer, d_row_ptr[nS] = nnz.  nS >= 1.
int cfrk_sparse_count(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                      int64_t nS, int k, int flags, int64_t *d_row_ptr) {
  const bool canon = (flags & CFRK_CANONICAL) != 0;
  void *p_keys, *p_cnt, *p_aux;
  int rc;
  const int64_t scan_block = 256 * SP_SCAN_ITEMS;
  const int64_t nb = (nS + scan_block - 1) / scan_block;
  if ((rc = cfrk_pool_get(ctx, BUF_SPARSE_KEYS, (size_t)nN * 8, &p_keys))) return rc;
  if ((rc = cfrk_pool_get(ctx, BUF_SPARSE_CNT, (size_t)nN * 4, &p_cnt))) return rc;
  if ((rc = cfrk_pool_get(ctx, BUF_SPARSE_AUX, (size_t)nb * 8, &p_aux))) return rc;
  uint64_t *tk = (uint64_t *)p_keys;
  uint32_t *tc = (uint32_t *)p_cnt;
  int64_t *bsum = (int64_t *)p_aux;
  const int64_t cus = ctx->num_cus;                   // (the caps are this file's own, lower than class_grids')
  const unsigned g16 = reads_grid(nS, 16, cus * 8), g64 = reads_grid(nS, 64, cus * 8);
  const unsigned glong = reads_grid(nS, SP_LONG_NT, cus), grl = reads_grid(nS, 256, cus * 4);
#define CFRK_SPARSE_COUNT(G_, C_, GRID_)                                                                          \
  hipLaunchKernelGGL((sparse_count_kernel<G_, C_>), dim3(GRID_), dim3(G_ == 16 ? 256 : 64), 0, ctx->stream, d_data, \
                     d_start, d_length, nN, nS, k, tk, tc, d_row_ptr)
  if (canon) {
    CFRK_SPARSE_COUNT(16, true, g16);
    CFRK_SPARSE_COUNT(64, true, g64);
    hipLaunchKernelGGL((sparse_long_sort_kernel<true>), dim3(glong), dim3(SP_LONG_NT), 0, ctx->stream, d_data, d_start,
                       d_length, nN, nS, k, tk, d_row_ptr);
  } else {
    CFRK_SPARSE_COUNT(16, false, g16);
    CFRK_SPARSE_COUNT(64, false, g64);
    hipLaunchKernelGGL((sparse_long_sort_kernel<false>), dim3(glong), dim3(SP_LONG_NT), 0, ctx->stream, d_data, d_start,
                       d_length, nN, nS, k, tk, d_row_ptr);
  }
#undef CFRK_SPARSE_COUNT
  hipLaunchKernelGGL(sparse_runlength_kernel, dim3(grl), dim3(256), 0, ctx->stream, d_start, d_length, nN, nS, k, tk, tc,
                     d_row_ptr);
  hipLaunchKernelGGL(sparse_scan_reduce_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, (const int64_t *)d_row_ptr,
                     nS, bsum);
  hipLaunchKernelGGL(sparse_scan_sums_kernel, dim3(1), dim3(256), 0, ctx->stream, bsum, nb, d_row_ptr + nS);
  hipLaunchKernelGGL(sparse_scan_apply_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, d_row_ptr, nS,
                     (const int64_t *)bsum);
  HIP_TRY(ctx, hipGetLastError());
  return CFRK_OK;
}

// Moves the rows of the most recent cfrk_sparse_count (same d_start, d_row_ptr, nS) to d_keys / d_counts; enqueued.
int cfrk_sparse_compact(cfrk_ctx *ctx, const int64_t *d_start, const int64_t *d_row_ptr, int64_t nS, uint64_t *d_keys,
                        uint32_t *d_counts) {
  const unsigned grid = reads_grid(nS, 16, (int64_t)ctx->num_cus * 16);
  hipLaunchKernelGGL(sparse_compact_kernel, dim3(grid), dim3(256), 0, ctx->stream, d_start, d_row_ptr, nS,
                     (const uint64_t *)ctx->pool[BUF_SPARSE_KEYS].p, (const uint32_t *)ctx->pool[BUF_SPARSE_CNT].p, d_keys,
                     d_counts);
  HIP_TRY(ctx, hipGetLastError());
  return CFRK_OK;
}
