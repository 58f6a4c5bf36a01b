// lane_group.h -- what the kernels that give every read to a group of lanes (or to a workgroup) share: the phase
// boundary of a wave, the sums over a group, the bitonic network that sorts a group's LDS array in place, and the
// window count of a read that may lie anywhere (sparse.hip, read_stats.hip, read_filter.hip).
#pragma once

#include "common.h"

#ifdef __HIPCC__
namespace {

// the lanes of one wave run in lock step and LDS is in order per wave: this only keeps the compiler from moving LDS
// accesses across a phase boundary
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
struct WaveSync { __device__ __forceinline__ void operator()() const { wave_sync(); } };
struct BlockSync { __device__ __forceinline__ void operator()() const { __syncthreads(); } };

template <int G>
__device__ __forceinline__ int group_sum(int v) {
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <class T>
__device__ __forceinline__ void cmp_exchange(T *a, int lo, int hi) {
  const T x = a[lo], y = a[hi];
  if (x > y) { a[lo] = y; a[hi] = x; }
}

// a[0 .. n) ascending, by nt cooperating threads (tid = 0 .. nt-1; all of them call with the same n).  Bitonic network
// in the form whose merges begin with a "flip" step: every compare-exchange puts the smaller key at the lower index,
// so with +infinity imagined at the indices >= n an exchange that reaches there never swaps and is skipped.
template <class T, class Sync>
__device__ __forceinline__ void sort_keys(T *a, int n, int tid, int nt, Sync sync) {
  if (n < 2) return;
  const int P = 1 << (32 - __clz(n - 1));
  const int half = P >> 1;
  for (int span = 2; span <= P; span <<= 1) {
    const int h = span >> 1;
    for (int t = tid; t < half; t += nt) {
      const int blk = (t & ~(h - 1)) << 1, off = t & (h - 1);
      const int hi = blk + span - 1 - off;
      if (hi < n) cmp_exchange(a, blk + off, hi);
    }
    sync();
    for (int j = h >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < half; t += nt) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        if (lo + j < n) cmp_exchange(a, lo, lo + j);
      }
      sync();
    }
  }
}

// windows of a read that can count: those that end inside it.  A read whose range does not lie in [0, nN) (the device
// form does not check the layout) has none, so nothing is ever read or written outside the buffers.
__device__ __forceinline__ int read_windows(int64_t st, int L, int64_t nN, int k) {
  return (st >= 0 && L >= k && st <= nN - (int64_t)L) ? L - k + 1 : 0;
}

// bytes [st, st + nbytes) of data into LDS as the aligned dwords that cover them, by the G lanes of a group (coalesced
// dword loads); a dword that is not wholly inside [data, data + nN) is assembled from guarded byte loads.  Returns the
// skew: the read's first byte is byte `skew` of stage_dw.  The caller puts a wave_sync() before the bytes are read.
template <int G>
__device__ __forceinline__ int stage_read(const int8_t *__restrict__ data, int64_t nN, int64_t st, int nbytes,
                                          int32_t *stage_dw, int lane) {
  const int skew = (int)((reinterpret_cast<uintptr_t>(data) + (uintptr_t)st) & 3u);
  const int ndw = (skew + nbytes + 3) >> 2;
  for (int d = lane; d < ndw; d += G) {
    const int64_t off = st - skew + 4 * (int64_t)d;
    int32_t w;
    if (off >= 0 && off + 4 <= nN) {
      w = *reinterpret_cast<const int32_t *>(data + off);
    } else {
      uint32_t u = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t g = off + j;
        const uint32_t c = (g >= 0 && g < nN) ? (uint32_t)(uint8_t)data[g] : 0xFFu;
        u |= c << (8 * j);
      }
      w = (int32_t)u;
    }
    stage_dw[d] = w;
  }
  return skew;
}

}  // namespace
#endif  // __HIPCC__
