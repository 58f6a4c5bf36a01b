// read_windows.h -- the windows of one read: the rolling key of the last k bases (sparse.hip and normalize.hip too, whose
// walkers look up in the live table and stand in normalize.hip), and what the kernels
// that look every window up in the index share (read_stats.hip, read_filter.hip): the lookup of one key in the
// index's form, the sums, minimum and maximum over a group of lanes, and the two walkers
//   staged_windows<G, MODE, CANON>   a lane group's read: staged in LDS, the windows split over the lanes, looked up
//                                    in batches whose first-slot loads are issued together
//   long_walk<NT, MODE, CANON>       a workgroup's long read: chunks of LONG_CHUNK windows per thread, rolled from
//                                    device memory, one lookup at a time
// Both call f(w, valid, count) for every window w in ascending order per lane / thread; count is the window's count
// in the index when valid (all k codes are bases), 0 otherwise.  Inlined into the kernel, as lane_group.h's walkers.
// A second form, chosen by the policy WinSlot in place of the default WinCount, calls f(w, valid, slot, minus): the
// window's SLOT in the index (Q_NO_SLOT when the key is absent or the window invalid) for a kernel that keeps an array
// of its own by slot (unitig_locate.hip), and whether the read spells the reverse complement of the stored key.
// MODE 0: dense index (k <= 12), 1: one-word hash (k <= 32), 2: two-word hash (k > 32).
#pragma once

#include "common.h"
#include "lane_group.h"
#include "query_dev.h"

#ifdef __HIPCC__
namespace {

constexpr int READ_STAGE_SLACK = 72;                   // k - 1 <= 63 bytes + skew <= 3 + dword round-up <= 3, a multiple of 8
                                                       // (sparse.hip, k <= 32, stages with a slack of its own)
constexpr int LONG_CHUNK = 32;                         // windows a thread of the long path rolls in a row

struct WinCount { static constexpr bool SLOT = false; };
struct WinSlot { static constexpr bool SLOT = true; };

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
  __device__ __forceinline__ bool minus() const { return CANON && rc < fwd; }      // key() is the reverse complement
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

// the same key's slot, Q_NO_SLOT when it is absent
template <int MODE, class T>
__device__ __forceinline__ uint64_t rs_lookup_slot(const QIndex &q, T key) {
  const uint64_t lo = (uint64_t)key;
  if (MODE == 0) return static_cast<const uint32_t *>(q.p)[lo] ? lo : Q_NO_SLOT;
  if (MODE == 1) return q_find1_slot(static_cast<const uint4 *>(q.p), q.mask, q_slot1(lo, q.shift), lo);
  const uint64_t hi = (uint64_t)(key >> (MODE == 2 ? 64 : 0));
  return q_find2_slot(static_cast<const uint4 *>(q.p), q.mask, q_slot2(lo, hi, q.shift), lo, hi);
}

// Read (nwin >= 1 windows from byte st on, inside [0, nN)) by the G lanes of a group.  stage_dw: the group's
// (READ_CAP + READ_STAGE_SLACK) / 4 dwords of LDS.  Lane l takes the windows [t0, t1) = its ceil(nwin / G), set before
// f is first called (so f may capture them by reference).  The caller puts a wave_sync() before its group's next read.
template <int G, int MODE, bool CANON, class P = WinCount, class F>
__device__ __forceinline__ void staged_windows(const int8_t *__restrict__ data, int64_t nN, int64_t st, int nwin,
                                               const QIndex &q, int32_t *stage_dw, int lane, int &t0, int &t1, F f) {
  constexpr bool TWO = MODE == 2;
  constexpr int B = TWO ? QB / 2 : QB;                 // (a two-word slot is two 16-byte loads)
  typedef typename RsKey<TWO>::type T;
  const int k = q.k;
  const uint4 *slots = static_cast<const uint4 *>(q.p);
  const uint32_t *dense = static_cast<const uint32_t *>(q.p);
  const int skew = stage_read<G>(data, nN, st, nwin + k - 1, stage_dw, lane);
  wave_sync();
  const int8_t *stage = reinterpret_cast<const int8_t *>(stage_dw) + skew;
  const int per = (nwin + G - 1) / G;
  t0 = lane * per;
  t1 = min(t0 + per, nwin);
  if (t0 >= t1) return;
  Roller<TWO, CANON> R(k);
  for (int p = t0; p < t0 + k - 1; ++p) R.push((int)stage[p]);
  for (int w0 = t0; w0 < t1; w0 += B) {
    T key[B];
    uint4 v[B], v2[B];
    uint32_t d[B];
    bool ok[B];
    bool om[B];                                        // (slot form only)
#pragma unroll
    for (int u = 0; u < B; ++u) {                      // every first-slot load of the batch is issued here ...
      const bool in = w0 + u < t1;
      if (in) R.push((int)stage[w0 + u + k - 1]);
      ok[u] = in && R.valid();
      key[u] = R.key();
      if constexpr (P::SLOT) om[u] = R.minus();
      if (MODE == 0) {
        d[u] = ok[u] ? dense[(uint64_t)key[u]] : 0u;
      } else if (MODE == 1) {
        v[u] = ok[u] ? slots[q_slot1((uint64_t)key[u], q.shift)] : make_uint4(0, 0, 0, 0);
      } else {
        const uint64_t h = q_slot2((uint64_t)key[u], (uint64_t)(key[u] >> (TWO ? 64 : 0)), q.shift);
        v[u] = ok[u] ? slots[2 * h] : make_uint4(0, 0, 0, 0);
        v2[u] = ok[u] ? slots[2 * h + 1] : make_uint4(0, 0, 0, 0);
      }
    }
#pragma unroll
    for (int u = 0; u < B; ++u) {                      // ... before any is resolved
      if (w0 + u >= t1) break;
      if constexpr (P::SLOT) {
        uint64_t r = Q_NO_SLOT;
        if (ok[u]) {
          const uint64_t lo = (uint64_t)key[u], hi = (uint64_t)(key[u] >> (TWO ? 64 : 0));
          if (MODE == 0) {
            if (d[u]) r = lo;
          } else if (MODE == 1) {
            const uint64_t h = q_slot1(lo, q.shift);
            if (v[u].z == 0) r = Q_NO_SLOT;
            else if (q_lo(v[u]) == lo) r = h;
            else r = q_find1_slot(slots, q.mask, (h + 1) & q.mask, lo);
          } else {
            const uint64_t h = q_slot2(lo, hi, q.shift);
            if (v2[u].x == 0) r = Q_NO_SLOT;
            else if (q_lo(v[u]) == lo && q_hi(v[u]) == hi) r = h;
            else r = q_find2_slot(slots, q.mask, (h + 1) & q.mask, lo, hi);
          }
        }
        f(w0 + u, ok[u], r, ok[u] && om[u]);
      } else if (ok[u]) {
        uint32_t r;
        const uint64_t lo = (uint64_t)key[u], hi = (uint64_t)(key[u] >> (TWO ? 64 : 0));
        if (MODE == 0) {
          r = d[u];
        } else if (MODE == 1) {
          if (v[u].z == 0) r = 0;
          else if (q_lo(v[u]) == lo) r = v[u].z;
          else r = q_find1(slots, q.mask, (q_slot1(lo, q.shift) + 1) & q.mask, lo);      // longer probes
        } else {
          if (v2[u].x == 0) r = 0;
          else if (q_lo(v[u]) == lo && q_hi(v[u]) == hi) r = v2[u].x;
          else r = q_find2(slots, q.mask, (q_slot2(lo, hi, q.shift) + 1) & q.mask, lo, hi);
        }
        f(w0 + u, true, r);
      } else {
        f(w0 + u, false, 0u);
      }
    }
  }
}

// the windows [c0, min(c0 + LONG_CHUNK, nwin)) of a read, rolled from its bytes in device memory (st + p <= st +
// length - 1); nothing when c0 >= nwin
template <int MODE, bool CANON, class P = WinCount, class F>
__device__ __forceinline__ void long_chunk(const int8_t *__restrict__ data, int64_t st, int nwin, const QIndex &q,
                                           int64_t c0, F f) {
  if (c0 >= nwin) return;
  const int k = q.k;
  const int64_t c1 = c0 + LONG_CHUNK < nwin ? c0 + LONG_CHUNK : (int64_t)nwin;
  Roller<MODE == 2, CANON> R(k);
  for (int64_t p = c0; p < c1 + k - 1; ++p) {
    R.push((int)data[st + p]);
    if (p >= c0 + k - 1) {
      if constexpr (P::SLOT) {
        if (R.valid()) f((int)(p - (k - 1)), true, rs_lookup_slot<MODE>(q, R.key()), R.minus());
        else f((int)(p - (k - 1)), false, Q_NO_SLOT, false);
      } else {
        if (R.valid()) f((int)(p - (k - 1)), true, rs_lookup<MODE>(q, R.key()));
        else f((int)(p - (k - 1)), false, 0u);
      }
    }
  }
}

// a long read by the NT threads of a workgroup, in rounds of NT chunks: chunk t of a round is thread t's.  (A kernel
// that has work of its own between the rounds walks them itself, with long_chunk.)
template <int NT, int MODE, bool CANON, class F>
__device__ __forceinline__ void long_walk(const int8_t *__restrict__ data, int64_t st, int nwin, const QIndex &q, int tid,
                                          F f) {
  for (int64_t c0 = (int64_t)tid * LONG_CHUNK; c0 < nwin; c0 += (int64_t)NT * LONG_CHUNK)
    long_chunk<MODE, CANON>(data, st, nwin, q, c0, f);
}

}  // namespace
#endif  // __HIPCC__
