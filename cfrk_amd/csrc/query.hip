// query.hip -- point queries on a finished global result: how often does a k-mer occur?
//
// The result of any counting path resolves to one ResultSrc (cfrk_msp_resolve): the HBM table or a compact list.
// A query builds a read-only lookup index from it on the first call of a job (ctx->q_valid; every call that changes
// the result clears it) and answers from the index only, so digest, histogram and export read the same result
// afterwards.
//
// Index (pool slot BUF_QUERY_INDEX):
//   k <= 12: a dense uint32[4^k] array of counts (64 MiB at most).  Lookup = one load.
//   k  > 12: open addressing, 2^ceil(log2(2n)) slots (load <= 0.5, at least 1024), linear probing, AoS slots so that a
//            probe touches one line: 16 B {lo, count, pad} for k <= 32, 32 B {lo, hi, count, pad} for k > 32.  The slot
//            hash is the table's own.  An empty slot is count == 0 (result counts are >= 1), so no key is reserved:
//            the k = 32 all-T key, which the table keeps in its ST_ONES side word, is an ordinary entry here.
// The build is one lane per source entry: result keys are unique, so an insert claims a slot by a CAS of its count
// word 0 -> c and then stores the key words plainly; queries run in a later kernel on the same stream.
//
// Lookups: one lane per key, or, for reads, the packed front end of hash_count1_kernel (global_hash.hip) -- 2 KiB
// tiles per wave, 32 windows per lane -- with the first-slot loads of QB windows in flight before any is resolved,
// and the wave's 2048 answers staged in LDS so that they leave as coalesced 16-B stores.  k > 32 rolls byte-wise like
// hash_count2_kernel, its answers staged the same way.
#include "msp.h"
#include "query_dev.h"
#include "table.h"

#include <algorithm>

namespace {

constexpr int QROW = 33;              // a lane's 32 staged answers, rows padded by one word: conflict-free LDS access
constexpr int QSTAGE = 64 * QROW;     // one wave's staged answers (words)

// ---- index build -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void qidx_dense_kernel(ResultSrc r, uint32_t *__restrict__ dense, uint64_t nkeys) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (uint64_t i = tid; i < r.n; i += nthreads) {
    uint64_t lo, hi; uint32_t c;
    if (src_read(r, i, lo, hi, c) && lo < nkeys) dense[lo] = c;
  }
}

template <bool TWO>
__global__ __launch_bounds__(256) void qidx_hash_kernel(ResultSrc r, uint4 *__restrict__ slots, uint64_t mask, int shift) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (uint64_t i = tid; i < r.n; i += nthreads) {
    uint64_t lo, hi; uint32_t c;
    if (!src_read(r, i, lo, hi, c)) continue;
    uint64_t h = TWO ? q_slot2(lo, hi, shift) : q_slot1(lo, shift);
    for (uint64_t probe = 0; probe <= mask; ++probe) {
      uint4 *s = TWO ? &slots[2 * h] : &slots[h];
      uint32_t *cw = TWO ? &s[1].x : &s->z;
      if (atomicCAS(cw, 0u, c) == 0u) {
        uint64_t *kw = reinterpret_cast<uint64_t *>(s);
        kw[0] = lo;
        if (TWO) kw[1] = hi;
        break;
      }
      h = (h + 1) & mask;
    }
  }
}

// k = 32: the all-T key's count from the ST_ONES side word (a list may hold the key as an entry as well: added)
__global__ void qidx_ones_kernel(uint4 *__restrict__ slots, uint64_t mask, int shift, uint32_t ones) {
  uint64_t h = q_slot1(CFRK_EMPTY_KEY, shift);
  for (uint64_t probe = 0; probe <= mask; ++probe) {
    uint4 &s = slots[h];
    if (s.z == 0) {
      reinterpret_cast<uint64_t *>(&s)[0] = CFRK_EMPTY_KEY;
      s.z = ones;
      return;
    }
    if (q_lo(s) == CFRK_EMPTY_KEY) {
      s.z = s.z > CFRK_COUNT_MAX - ones ? CFRK_COUNT_MAX : s.z + ones;
      return;
    }
    h = (h + 1) & mask;
  }
}

// ---- lookups ---------------------------------------------------------------------------------------------------
// MODE 0: dense (k <= 12), 1: one-word hash (k <= 32), 2: two-word hash (k > 32): q_key, query_dev.h
template <int MODE, bool CANON>
__global__ __launch_bounds__(256) void query_keys_kernel(QIndex q, const uint64_t *__restrict__ keys_lo,
                                                         const uint64_t *__restrict__ keys_hi, int64_t n,
                                                         uint32_t *__restrict__ out) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = tid; i < n; i += nthreads) out[i] = q_key<MODE, CANON>(q, keys_lo[i], keys_hi ? keys_hi[i] : 0);
}

// a wave's 2048 staged answers (lane l's window j at st[l * QROW + j]) to out[base ..): chunk g = windows 4g .. 4g+3
__device__ __forceinline__ void q_flush(const uint32_t *st, uint32_t *__restrict__ out, int64_t base, int64_t nN,
                                        bool vec, int lane) {
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int g = r * 64 + lane;
    const int64_t p = base + 4 * g;
    if (p >= nN) break;
    const uint32_t *s = st + (g >> 3) * QROW + (g & 7) * 4;
    const uint4 v = make_uint4(s[0], s[1], s[2], s[3]);
    if (vec && p + 4 <= nN) {
      *reinterpret_cast<uint4 *>(out + p) = v;
    } else {
      out[p] = v.x;
      if (p + 1 < nN) out[p + 1] = v.y;
      if (p + 2 < nN) out[p + 2] = v.z;
      if (p + 3 < nN) out[p + 3] = v.w;
    }
  }
}

// k <= 32 (MODE 0 / 1).  The block's four waves take tiles t0 + wave: the loop's trip count is the block's, so the
// barriers around the LDS staging are reached by every wave.
template <int MODE, bool CANON>
__global__ __launch_bounds__(256) void query_reads1_kernel(const int8_t *__restrict__ data, int64_t nN, QIndex q,
                                                           uint32_t *__restrict__ out, bool vec) {
  __shared__ uint32_t stage[4 * QSTAGE];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t *st = stage + w * QSTAGE + lane * QROW;
  const int k = q.k;
  const uint4 *slots = static_cast<const uint4 *>(q.p);
  const uint32_t *dense = static_cast<const uint32_t *>(q.p);
  const int64_t ntiles = (nN + 2047) >> 11;
  for (int64_t t0 = (int64_t)blockIdx.x * 4; t0 < ntiles; t0 += (int64_t)gridDim.x * 4) {
    const int64_t tile = t0 + w;
    if (tile < ntiles) {
      const int64_t off = (tile << 11) + 32 * lane;
      uint32_t b0, b1, bad;
      dev_load_chunk32(data, off, nN, b0, b1, bad);
      uint32_t n0 = dev_lane_next(b0), n1 = dev_lane_next(b1), nbad = dev_lane_next(bad);
      if (lane == 63) dev_load_chunk32(data, off + 32, nN, n0, n1, nbad);
      const uint64_t hi = ((uint64_t)b0 << 32) | b1;
      const uint64_t lo = ((uint64_t)n0 << 32) | n1;
      const uint64_t M = ((uint64_t)bad << 32) | nbad;
      for (int b = 0; b < 32; b += QB) {
        uint64_t key[QB], h[QB];
        uint4 v[QB];
        uint32_t d[QB];
        bool ok[QB];
#pragma unroll
        for (int u = 0; u < QB; ++u) {                 // every first-slot load of the batch is issued here ...
          const int i = b + u;
          ok[u] = ((M << i) >> (64 - k)) == 0;
          key[u] = q_window<CANON>(hi, lo, i, k);
          if (MODE == 0) {
            d[u] = ok[u] ? dense[key[u]] : 0u;
          } else {
            h[u] = q_slot1(key[u], q.shift);
            v[u] = ok[u] ? slots[h[u]] : make_uint4(0, 0, 0, 0);
          }
        }
        uint32_t pend = 0;
#pragma unroll
        for (int u = 0; u < QB; ++u) {                 // ... before any is resolved
          uint32_t r = CFRK_QUERY_NONE;
          if (ok[u]) {
            if (MODE == 0) r = d[u];
            else if (v[u].z == 0) r = 0;
            else if (q_lo(v[u]) == key[u]) r = v[u].z;
            else pend |= 1u << u;
          }
          st[b + u] = r;
        }
        while (pend) {                                 // longer probes: from the second slot on
          const int u = __builtin_ctz(pend);
          pend &= pend - 1;
          const uint64_t kk = q_window<CANON>(hi, lo, b + u, k);
          st[b + u] = q_find1(slots, q.mask, (q_slot1(kk, q.shift) + 1) & q.mask, kk);
        }
      }
    }
    __syncthreads();
    if (tile < ntiles) q_flush(stage + w * QSTAGE, out, tile << 11, nN, vec, lane);
    __syncthreads();
  }
}

// k > 32: lane l of a tile's wave rolls over the bases of its 32 window starts (plus k - 1 of look-ahead)
template <bool CANON>
__global__ __launch_bounds__(256) void query_reads2_kernel(const int8_t *__restrict__ data, int64_t nN, QIndex q,
                                                           uint32_t *__restrict__ out, bool vec) {
  typedef unsigned __int128 u128;
  __shared__ uint32_t stage[4 * QSTAGE];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t *st = stage + w * QSTAGE + lane * QROW;
  const int k = q.k;
  const uint4 *slots = static_cast<const uint4 *>(q.p);
  const u128 mask = (k == 64) ? ~(u128)0 : ((((u128)1) << (2 * k)) - 1);
  const int64_t ntiles = (nN + 2047) >> 11;
  for (int64_t t0 = (int64_t)blockIdx.x * 4; t0 < ntiles; t0 += (int64_t)gridDim.x * 4) {
    const int64_t tile = t0 + w;
    if (tile < ntiles) {
      const int64_t s0 = (tile << 11) + 32 * lane;
      for (int j = 0; j < 32; ++j) st[j] = CFRK_QUERY_NONE;
      const int64_t end = min(s0 + 32 + k - 1, nN);
      u128 fwd = 0, rc = 0;
      int run = 0;
      for (int64_t p = s0; p < end; ++p) {
        const int c = (int)data[p];
        if (c < 0 || c > 3) { run = 0; continue; }
        fwd = ((fwd << 2) | (u128)(unsigned)c) & mask;
        rc = (rc >> 2) | ((u128)(unsigned)(3 - c) << (2 * (k - 1)));
        if (++run >= k) {
          const u128 key = (CANON && rc < fwd) ? rc : fwd;
          const uint64_t klo = (uint64_t)key, khi = (uint64_t)(key >> 64);
          st[p - k + 1 - s0] = q_find2(slots, q.mask, q_slot2(klo, khi, q.shift), klo, khi);
        }
      }
    }
    __syncthreads();
    if (tile < ntiles) q_flush(stage + w * QSTAGE, out, tile << 11, nN, vec, lane);
    __syncthreads();
  }
}

int q_grid(const cfrk_ctx *ctx, int64_t items_per_block, int64_t items) {
  const int64_t want = (items + items_per_block - 1) / items_per_block;
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)ctx->num_cus * 8));
}

}  // namespace

// the index of the job's current result, built when it is not valid
int cfrk_query_index(cfrk_ctx *ctx, QIndex *q) {
  const int k = ctx->g_k;
  const bool two = ctx->g_two;
  if (!ctx->q_valid) {
    ResultSrc r;
    bool use_list = false;
    int rc = cfrk_msp_resolve(ctx, &r, &use_list);
    if (rc) return rc;
    uint64_t st[ST_NWORDS];
    // (the digest's scan: distinct entries for the index size, the overflow flag; synchronises)
    if ((rc = cfrk_result_scan(ctx, use_list ? &r : nullptr, st))) return rc;
    if (st[ST_OVERFLOW]) return cfrk_fail(ctx, CFRK_ERR_TABLE_FULL, "table of %llu slots overflowed", (unsigned long long)ctx->g_cap);
    if (!use_list) {
      r.lo = ctx->g_keys_lo; r.hi = ctx->g_keys_hi; r.cnt = ctx->g_counts; r.n = ctx->g_cap;
      r.kind = two ? 1 : 0; r.stats = ctx->g_stats;
    }
    const uint64_t n = st[ST_DIG0];
    int lg = 0;
    size_t bytes;
    if (k <= 12) {
      bytes = (size_t)4 << (2 * k);
    } else {
      lg = 10;
      while (lg < 40 && (1ull << lg) < 2 * n) ++lg;
      bytes = ((size_t)1 << lg) * (two ? 32 : 16);
    }
    void *p;
    if ((rc = cfrk_pool_get(ctx, BUF_QUERY_INDEX, bytes, &p))) { (void)hipGetLastError(); return rc; }
    HIP_TRY(ctx, hipMemsetAsync(p, 0, bytes, ctx->stream));
    const int grid = q_grid(ctx, 256 * 4, (int64_t)r.n);
    const uint64_t mask = (1ull << lg) - 1;
    if (k <= 12) hipLaunchKernelGGL(qidx_dense_kernel, dim3(grid), dim3(256), 0, ctx->stream, r, (uint32_t *)p, 1ull << (2 * k));
    else if (two) hipLaunchKernelGGL(qidx_hash_kernel<true>, dim3(grid), dim3(256), 0, ctx->stream, r, (uint4 *)p, mask, 64 - lg);
    else hipLaunchKernelGGL(qidx_hash_kernel<false>, dim3(grid), dim3(256), 0, ctx->stream, r, (uint4 *)p, mask, 64 - lg);
    HIP_TRY(ctx, hipGetLastError());
    if (k == 32 && st[ST_ONES]) {
      const uint32_t ones = st[ST_ONES] > CFRK_COUNT_MAX ? CFRK_COUNT_MAX : (uint32_t)st[ST_ONES];
      hipLaunchKernelGGL(qidx_ones_kernel, dim3(1), dim3(1), 0, ctx->stream, (uint4 *)p, mask, 64 - lg, ones);
      HIP_TRY(ctx, hipGetLastError());
    }
    ctx->q_log2cap = lg;
    ctx->q_valid = true;
    ++ctx->q_epoch;      // (what is kept by slot beside an earlier build, the position map, is no longer this index's)
  }
  q->p = ctx->pool[BUF_QUERY_INDEX].p;
  q->mask = (1ull << ctx->q_log2cap) - 1;
  q->shift = 64 - ctx->q_log2cap;
  q->k = k;
  return CFRK_OK;
}

// Read-only: the geometry of the job's table and index and the slot hashes of one key, evaluated on the host by the
// functions the kernels call (q_slot1 / q_slot2 -> dev_mix64, compiled for both sides).
extern "C" int cfrk_debug_hash_info(const cfrk_ctx *ctx, uint64_t lo, uint64_t hi, uint64_t out[4]) {
  if (!out) return CFRK_ERR_ARG;
  out[0] = (ctx && ctx->g_active) ? (uint64_t)ctx->g_log2cap : 0;
  out[1] = (ctx && ctx->g_active && ctx->q_valid && ctx->g_k > 12) ? (uint64_t)ctx->q_log2cap : 0;
  out[2] = q_slot1(lo, 0);
  out[3] = q_slot2(lo, hi, 0);
  return CFRK_OK;
}

int cfrk_query_keys(cfrk_ctx *ctx, const uint64_t *d_lo, const uint64_t *d_hi, int64_t n, uint32_t *d_out) {
  QIndex q;
  int rc = cfrk_query_index(ctx, &q);
  if (rc || n == 0) return rc;
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  const int grid = q_grid(ctx, 256 * 4, n);
#define Q_KEYS(MODE)                                                                                                  \
  do {                                                                                                                \
    if (canon) hipLaunchKernelGGL((query_keys_kernel<MODE, true>), dim3(grid), dim3(256), 0, ctx->stream, q, d_lo, d_hi, n, d_out); \
    else hipLaunchKernelGGL((query_keys_kernel<MODE, false>), dim3(grid), dim3(256), 0, ctx->stream, q, d_lo, d_hi, n, d_out);     \
  } while (0)
  if (q.k <= 12) Q_KEYS(0);
  else if (q.k <= 32) Q_KEYS(1);
  else Q_KEYS(2);
#undef Q_KEYS
  HIP_TRY(ctx, hipGetLastError());
  return CFRK_OK;
}

int cfrk_query_reads(cfrk_ctx *ctx, const int8_t *d_data, int64_t nN, uint32_t *d_out) {
  QIndex q;
  int rc = cfrk_query_index(ctx, &q);
  if (rc || nN == 0) return rc;
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  const bool vec = ((uintptr_t)d_out & 15) == 0;
  const int grid = q_grid(ctx, 4 * 2048, nN);
  if (q.k <= 12) {
    if (canon) hipLaunchKernelGGL((query_reads1_kernel<0, true>), dim3(grid), dim3(256), 0, ctx->stream, d_data, nN, q, d_out, vec);
    else hipLaunchKernelGGL((query_reads1_kernel<0, false>), dim3(grid), dim3(256), 0, ctx->stream, d_data, nN, q, d_out, vec);
  } else if (q.k <= 32) {
    if (canon) hipLaunchKernelGGL((query_reads1_kernel<1, true>), dim3(grid), dim3(256), 0, ctx->stream, d_data, nN, q, d_out, vec);
    else hipLaunchKernelGGL((query_reads1_kernel<1, false>), dim3(grid), dim3(256), 0, ctx->stream, d_data, nN, q, d_out, vec);
  } else {
    if (canon) hipLaunchKernelGGL((query_reads2_kernel<true>), dim3(grid), dim3(256), 0, ctx->stream, d_data, nN, q, d_out, vec);
    else hipLaunchKernelGGL((query_reads2_kernel<false>), dim3(grid), dim3(256), 0, ctx->stream, d_data, nN, q, d_out, vec);
  }
  HIP_TRY(ctx, hipGetLastError());
  return CFRK_OK;
}
