// read_windows.h -- what the kernels that walk the windows of a read against the lookup index share (read_stats.hip,
// read_filter.hip): the rolling key of the last k bases, the lookup of one key in the index's form, and the sums,
// minimum and maximum over a group of lanes.
#pragma once

#include "common.h"
#include "query_dev.h"

#ifdef __HIPCC__
namespace {

template <bool TWO> struct RsKey { typedef uint64_t type; };
template <> struct RsKey<true> { typedef unsigned __int128 type; };

// rolling forward / reverse-complement key of the last k bases; run = valid bases in a row
template <bool TWO, bool CANON>
struct Roller {
  typedef typename RsKey<TWO>::type T;
  T fwd, rc, mask;
  int run, k, rcshift;
  __device__ __forceinline__ explicit Roller(int k_) : fwd(0), rc(0), run(0), k(k_), rcshift(2 * (k_ - 1)) {
    mask = (k_ == (TWO ? 64 : 32)) ? ~(T)0 : ((((T)1) << (2 * k_)) - 1);
  }
  __device__ __forceinline__ void push(int c) {
    if (c < 0 || c > 3) {
      run = 0;
    } else {
      fwd = ((fwd << 2) | (T)(unsigned)c) & mask;
      if (CANON) rc = (rc >> 2) | ((T)(unsigned)(3 - c) << rcshift);
      ++run;
    }
  }
  __device__ __forceinline__ bool valid() const { return run >= k; }
  __device__ __forceinline__ T key() const { return (CANON && rc < fwd) ? rc : fwd; }
};

template <int G>
__device__ __forceinline__ uint32_t group_sum_u32(uint32_t v) {
  for (int o = G / 2; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
  return v;
}
template <int G>
__device__ __forceinline__ uint64_t group_sum_u64(uint64_t v) {
  for (int o = G / 2; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o);
  return v;
}
template <int G>
__device__ __forceinline__ uint32_t group_min_u32(uint32_t v) {
  for (int o = G / 2; o > 0; o >>= 1) { const uint32_t u = (uint32_t)__shfl_xor((int)v, o); v = u < v ? u : v; }
  return v;
}
template <int G>
__device__ __forceinline__ uint32_t group_max_u32(uint32_t v) {
  for (int o = G / 2; o > 0; o >>= 1) { const uint32_t u = (uint32_t)__shfl_xor((int)v, o); v = u > v ? u : v; }
  return v;
}

// one key, already in the index's form (canonical when the job is)
template <int MODE, class T>
__device__ __forceinline__ uint32_t rs_lookup(const QIndex &q, T key) {
  const uint64_t lo = (uint64_t)key;
  if (MODE == 0) return static_cast<const uint32_t *>(q.p)[lo];
  if (MODE == 1) return q_find1(static_cast<const uint4 *>(q.p), q.mask, q_slot1(lo, q.shift), lo);
  const uint64_t hi = (uint64_t)(key >> (MODE == 2 ? 64 : 0));
  return q_find2(static_cast<const uint4 *>(q.p), q.mask, q_slot2(lo, hi, q.shift), lo, hi);
}

}  // namespace
#endif  // __HIPCC__
