// sketch.hip -- how many DISTINCT k-mers do these reads hold?  One streaming pass folds the hash of every valid window
// into a HyperLogLog sketch (format: include/cfrk_abi.h), so that a job can be sized before it is counted.
//
// Kernels: a persistent grid of 256-thread workgroups; each of the four waves takes 2048-base tiles.  k <= 32 forms
// its keys from packed chunks as query_reads1_kernel does (32 windows per lane), k > 32 rolls a 128-bit key byte-wise
// as query_reads2_kernel does.  Every window costs one hash and one LDS access:
//   the workgroup's 2^14 registers live in LDS as BYTES, four to a word (16 KiB).  A window reads its word and only
//   when its rank is larger than the byte there does it issue a compare-and-swap on the word (a loop: another bucket of
//   the word, or the same one, may have moved in between).  Registers only grow, so a stale read can only send a
//   window into the CAS needlessly, never past it wrongly.  After the first few thousand windows almost none raises
//   its register (a register of rank r is raised by a fraction 2^-r of its bucket's later keys), so the atomic is rare
//   and the layout is chosen for what is NOT rare: 16 KiB leave room for four workgroups on a CU beside whatever else
//   runs there, and zeroing and folding 4096 words per workgroup is a quarter of the work of 16384.  (One word per
//   register with ds atomic max is the alternative: 64 KiB, one or two workgroups per CU.  It is kept as a timing
//   variant of the ablation build only; the measured difference is in DESIGN.md.)
// At the end a workgroup folds its non-zero registers into a device array of words with atomicMax (again only where
// the word there is smaller), and a small kernel max-merges that array into the caller's bytes.  The number of valid
// windows is a wave reduction and one 64-bit atomic per workgroup.
#include "msp.h"
#include "query_dev.h"

#include <math.h>

#include <algorithm>

namespace {

constexpr int SK_M = CFRK_SKETCH_REGS;
constexpr int SK_LOG2M = CFRK_SKETCH_LOG2M;
constexpr int SK_RANK_MAX = 64 - SK_LOG2M + 1;
// BUF_SKETCH: [SK_M words: the workgroups' merged registers][one 64-bit window count, padded][SK_M bytes: the host form's registers]
constexpr size_t SK_OFF_WINDOWS = (size_t)SK_M * 4, SK_OFF_STAGE = SK_OFF_WINDOWS + 256, SK_BYTES = SK_OFF_STAGE + SK_M;
static_assert(SK_M == 1 << SK_LOG2M && SK_RANK_MAX < 256, "one byte per register");

// VAR 0: bytes packed four to a word, read first, CAS (the product).  Timing variants of the ablation build:
// VAR 1: one word per register, read first, atomicMax when larger; VAR 2: one word per register, atomicMax always.
template <int VAR> struct SkLds { static constexpr int WORDS = VAR == 0 ? SK_M / 4 : SK_M; };

template <int VAR>
__device__ __forceinline__ void sk_update(uint32_t *regs, uint64_t h) {
  const uint32_t bucket = (uint32_t)(h >> (64 - SK_LOG2M));
  const uint64_t w = h << SK_LOG2M;
  const uint32_t rank = w ? (uint32_t)__builtin_clzll(w) + 1u : (uint32_t)SK_RANK_MAX;
  if (VAR == 0) {
    uint32_t *wd = regs + (bucket >> 2);
    const int sh = (int)(bucket & 3u) * 8;
    uint32_t old = __atomic_load_n(wd, __ATOMIC_RELAXED);
    while (((old >> sh) & 0xFFu) < rank) {
      const uint32_t prev = atomicCAS(wd, old, (old & ~(0xFFu << sh)) | (rank << sh));
      if (prev == old) break;
      old = prev;
    }
  } else if (VAR == 1) {
    if (__atomic_load_n(regs + bucket, __ATOMIC_RELAXED) < rank) atomicMax(regs + bucket, rank);
  } else {
    atomicMax(regs + bucket, rank);
  }
}

template <int VAR>
__device__ __forceinline__ void sk_begin(uint32_t *regs) {
  for (int i = threadIdx.x; i < SkLds<VAR>::WORDS; i += blockDim.x) regs[i] = 0;
  __syncthreads();
}

__device__ __forceinline__ void sk_fold_one(uint32_t *__restrict__ acc, int j, uint32_t r) {
  if (r && __atomic_load_n(acc + j, __ATOMIC_RELAXED) < r) atomicMax(acc + j, r);
}

// the workgroup's registers into acc, its waves' window counts into *windows
template <int VAR>
__device__ __forceinline__ void sk_end(uint32_t *regs, uint32_t *wsum, uint32_t nwin, uint32_t *__restrict__ acc,
                                       unsigned long long *__restrict__ windows) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t tot = dev_wave_scan_incl(nwin);
  if (lane == 63) wsum[w] = tot;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long s = (unsigned long long)wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (s) atomicAdd(windows, s);
  }
  for (int i = threadIdx.x; i < SkLds<VAR>::WORDS; i += blockDim.x) {
    const uint32_t v = regs[i];
    if (VAR == 0) {
      if (v) {
        sk_fold_one(acc, 4 * i, v & 0xFFu);
        sk_fold_one(acc, 4 * i + 1, (v >> 8) & 0xFFu);
        sk_fold_one(acc, 4 * i + 2, (v >> 16) & 0xFFu);
        sk_fold_one(acc, 4 * i + 3, v >> 24);
      }
    } else {
      sk_fold_one(acc, i, v);
    }
  }
}

// k <= 32.  A wave's tiles are its own (no barrier inside the loop): tile = 4 * block + wave, then on by the grid.
template <bool CANON, int VAR>
__global__ __launch_bounds__(256) void sketch1_kernel(const int8_t *__restrict__ data, int64_t nN, int k,
                                                      uint32_t *__restrict__ acc, unsigned long long *__restrict__ windows) {
  __shared__ uint32_t regs[SkLds<VAR>::WORDS];
  __shared__ uint32_t wsum[4];
  sk_begin<VAR>(regs);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t ntiles = (nN + 2047) >> 11;
  uint32_t nwin = 0;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + w; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t off = (tile << 11) + 32 * lane;
    uint32_t b0, b1, bad;
    dev_load_chunk32(data, off, nN, b0, b1, bad);
    uint32_t n0 = dev_lane_next(b0), n1 = dev_lane_next(b1), nbad = dev_lane_next(bad);
    if (lane == 63) dev_load_chunk32(data, off + 32, nN, n0, n1, nbad);
    const uint64_t hi = ((uint64_t)b0 << 32) | b1;
    const uint64_t lo = ((uint64_t)n0 << 32) | n1;
    const uint64_t M = ((uint64_t)bad << 32) | nbad;
#pragma unroll 8
    for (int i = 0; i < 32; ++i) {
      if (((M << i) >> (64 - k)) != 0) continue;      // an invalid code or the end of the data inside the window
      sk_update<VAR>(regs, q_slot1(q_window<CANON>(hi, lo, i, k), 0));
      ++nwin;
    }
  }
  sk_end<VAR>(regs, wsum, nwin, acc, windows);
}

// k > 32: lane l of a tile's wave rolls over the bases of its 32 window starts (plus k - 1 of look-ahead)
template <bool CANON, int VAR>
__global__ __launch_bounds__(256) void sketch2_kernel(const int8_t *__restrict__ data, int64_t nN, int k,
                                                      uint32_t *__restrict__ acc, unsigned long long *__restrict__ windows) {
  typedef unsigned __int128 u128;
  __shared__ uint32_t regs[SkLds<VAR>::WORDS];
  __shared__ uint32_t wsum[4];
  sk_begin<VAR>(regs);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const u128 mask = (k == 64) ? ~(u128)0 : ((((u128)1) << (2 * k)) - 1);
  const int64_t ntiles = (nN + 2047) >> 11;
  uint32_t nwin = 0;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + w; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t s0 = (tile << 11) + 32 * lane;
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
        sk_update<VAR>(regs, q_slot2((uint64_t)key, (uint64_t)(key >> 64), 0));
        ++nwin;
      }
    }
  }
  sk_end<VAR>(regs, wsum, nwin, acc, windows);
}

// the call's registers (words) max-merged into the caller's bytes
__global__ __launch_bounds__(256) void sketch_merge_kernel(const uint32_t *__restrict__ acc, uint8_t *__restrict__ regs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= SK_M) return;
  const uint32_t r = acc[i];
  if (r > regs[i]) regs[i] = (uint8_t)r;
}

template <int VAR>
void sk_launch(cfrk_ctx *ctx, const int8_t *d_data, int64_t nN, int k, bool canon, uint32_t *acc, unsigned long long *windows) {
  const int64_t want = (((nN + 2047) >> 11) + 3) / 4;
  const int per_cu = VAR == 0 ? 4 : 2;               // (64 KiB of LDS per workgroup: two fit a CU)
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)ctx->num_cus * per_cu));
  if (k <= 32) {
    if (canon) hipLaunchKernelGGL((sketch1_kernel<true, VAR>), dim3(grid), dim3(256), 0, ctx->stream, d_data, nN, k, acc, windows);
    else hipLaunchKernelGGL((sketch1_kernel<false, VAR>), dim3(grid), dim3(256), 0, ctx->stream, d_data, nN, k, acc, windows);
  } else {
    if (canon) hipLaunchKernelGGL((sketch2_kernel<true, VAR>), dim3(grid), dim3(256), 0, ctx->stream, d_data, nN, k, acc, windows);
    else hipLaunchKernelGGL((sketch2_kernel<false, VAR>), dim3(grid), dim3(256), 0, ctx->stream, d_data, nN, k, acc, windows);
  }
}

double sk_estimate(const uint8_t *regs) {
  // sum of 2^-register over a histogram of the register values: every term is exact
  uint32_t hist[256] = {0};
  for (int i = 0; i < SK_M; ++i) ++hist[regs[i]];
  if (hist[0] == (uint32_t)SK_M) return 0.0;
  double sum = 0.0;
  for (int r = 255; r >= 0; --r)
    if (hist[r]) sum += ldexp((double)hist[r], -r);
  const double m = (double)SK_M;
  const double alpha = 0.7213 / (1.0 + 1.079 / m);
  double e = alpha * m * m / sum;
  if (e <= 2.5 * m && hist[0] > 0) e = m * log(m / (double)hist[0]);
  return e;
}

}  // namespace

int cfrk_sketch_stage(cfrk_ctx *ctx, uint8_t **d_stage) {
  void *p;
  const int rc = cfrk_pool_get(ctx, BUF_SKETCH, SK_BYTES, &p);
  if (rc) return rc;
  *d_stage = (uint8_t *)p + SK_OFF_STAGE;
  return CFRK_OK;
}

int cfrk_sketch_launch(cfrk_ctx *ctx, const int8_t *d_data, int64_t nN, int k, int flags, uint8_t *d_regs,
                       const uint64_t **d_windows) {
  void *p;
  int rc;
  if ((rc = cfrk_pool_get(ctx, BUF_SKETCH, SK_BYTES, &p))) return rc;
  uint32_t *acc = (uint32_t *)p;
  unsigned long long *windows = (unsigned long long *)((char *)p + SK_OFF_WINDOWS);
  HIP_TRY(ctx, hipMemsetAsync(p, 0, SK_OFF_WINDOWS + 8, ctx->stream));
  const bool canon = (flags & CFRK_CANONICAL) != 0;
#ifdef CFRK_ABLATIONS
  if (ctx->dbg_flags & CFRK_ABL_SK_ALWAYS) sk_launch<2>(ctx, d_data, nN, k, canon, acc, windows);
  else if (ctx->dbg_flags & CFRK_ABL_SK_WORDS) sk_launch<1>(ctx, d_data, nN, k, canon, acc, windows);
  else
#endif
  sk_launch<0>(ctx, d_data, nN, k, canon, acc, windows);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(sketch_merge_kernel, dim3(SK_M / 256), dim3(256), 0, ctx->stream, acc, d_regs);
  HIP_TRY(ctx, hipGetLastError());
  *d_windows = (const uint64_t *)windows;
  return CFRK_OK;
}

/* ------------------------------------------------------------------ the sketch on the host: no context, no device */

extern "C" int cfrk_sketch_estimate(const uint8_t *regs, double *distinct) {
  if (!regs || !distinct) return CFRK_ERR_ARG;
  *distinct = sk_estimate(regs);
  return CFRK_OK;
}

extern "C" int cfrk_sketch_merge(uint8_t *dst, const uint8_t *src) {
  if (!dst || !src) return CFRK_ERR_ARG;
  for (int i = 0; i < SK_M; ++i) dst[i] = std::max(dst[i], src[i]);
  return CFRK_OK;
}

extern "C" int cfrk_sketch_hint(const uint8_t *regs, uint64_t *hint) {
  if (!regs || !hint) return CFRK_ERR_ARG;
  // four standard errors of the estimator (1.04 / sqrt(m)) above the estimate
  const double want = ceil(sk_estimate(regs) * (1.0 + 4.0 * 1.04 / sqrt((double)SK_M)));
  const double lo = (double)(1ull << 20), hi = (double)(1ull << 31);
  *hint = (uint64_t)std::min(std::max(want, lo), hi);
  return CFRK_OK;
}
