// lane_group.h -- what the kernels that give every read to a group of lanes (or to a workgroup) share (sparse.hip,
// read_stats.hip, read_filter.hip, normalize.hip): the size classes of reads and their launch grids, the phase boundary of a wave,
// the sums over a group, the bitonic network that sorts a group's LDS array in place, the window count of a read that
// may lie anywhere, the staging of a read in LDS, and the two walkers over the reads of a batch:
//   class_reads<G>    the reads of a lane group's size class, one after the other by the group
//   long_reads<NT>    the reads above the fast path's capacity, one after the other by the whole workgroup
// Every read is handled by exactly one of three launches: G = 16 (0 .. READ_CAP16 windows, four reads per wave so that
// 150-base reads keep the lanes busy), G = 64 (up to READ_CAP64, one wave per workgroup) and a long-read kernel.  Each
// kernel sees the whole batch and skips the other classes' reads.  The walkers take the feature's part as a functor and
// are inlined into the kernel (no call survives); read_windows.h adds the walkers over the windows of one read.
#pragma once

#include "common.h"

#include <algorithm>

constexpr int READ_CAP16 = 256;                        // windows a 16-lane group takes
constexpr int READ_CAP64 = CFRK_SPARSE_FAST_WINDOWS;   // windows a 64-lane group takes (the fast path's capacity)
static_assert(CFRK_STATS_FAST_WINDOWS == READ_CAP64 && CFRK_SPANS_FAST_WINDOWS == READ_CAP64,
              "one pair of class limits: the three ABI constants name the same capacity");

// workgroups of a grid-stride launch over nS reads, `per` reads to a workgroup and turn, at most `cap`
inline unsigned reads_grid(int64_t nS, int per, int64_t cap) {
  return (unsigned)std::min<int64_t>((nS + per - 1) / per, cap);
}
// the grids of the three launches where the groups only look up (read_stats.hip, read_filter.hip); nt = threads of the
// long-read kernel.  Many more workgroups than fit at once: a CU takes a new one whenever one of those it holds ends.
struct ClassGrids { unsigned g16, g64, glong; };
inline ClassGrids class_grids(int64_t nS, int64_t cus, int nt) {
  return {reads_grid(nS, 16, cus * 64), reads_grid(nS, 64, cus * 64), reads_grid(nS, nt, cus * 4)};
}

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

// The reads of a lane group's size class.  Launched with 256 threads at G = 16 (16 groups, a read each per turn) and
// with 64 at G = 64.  body(i, st, nwin) is called by all G lanes of the group for read i of the class (nwin >= 1
// windows from byte st on, inside [0, nN)); empty(i) for a read without windows, which belongs to G = 16.  The kernel
// keeps its __shared__ arrays and hands its group's slice to its body: threadIdx.x / G at G = 16, the only one at
// G = 64.
template <int G, class Body, class Empty>
__device__ __forceinline__ void class_reads(const int64_t *__restrict__ start, const int32_t *__restrict__ length,
                                            int64_t nN, int64_t nS, int k, Body body, Empty empty) {
  static_assert(G == 16 || G == 64, "two lane-group widths");
  constexpr int RPB = (G == 16 ? 256 : 64) / G;
  const int grp = threadIdx.x / G, lane = threadIdx.x % G;
  if (G == 16) {
    for (int64_t i = (int64_t)blockIdx.x * RPB + grp; i < nS; i += (int64_t)gridDim.x * RPB) {
      const int64_t st = start[i];
      const int nwin = read_windows(st, length[i], nN, k);
      if (nwin > READ_CAP16) continue;
      if (nwin == 0) { empty(i); continue; }
      body(i, st, nwin);
    }
  } else {
    // the wave looks at 64 reads at a time and takes those of its size class one after the other
    for (int64_t base = (int64_t)blockIdx.x * 64; base < nS; base += (int64_t)gridDim.x * 64) {
      const int64_t mine = base + lane;
      int w = 0;
      if (mine < nS) w = read_windows(start[mine], length[mine], nN, k);
      unsigned long long todo = __ballot(w > READ_CAP16 && w <= READ_CAP64);
      while (todo) {
        const int b = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int64_t i = base + b;
        const int64_t st = start[i];
        body(i, st, read_windows(st, length[i], nN, k));
      }
    }
  }
}

// Every long read of the batch (more than READ_CAP64 windows), one after the other by the whole workgroup of NT
// threads: the workgroup looks at NT lengths at a time, lists the long reads among them in LDS and calls
// body(i, st, nwin) for each with all its threads.  The list is the template's, and so are the barriers around it:
//   (1) behind s_n = 0 and (2) behind the listing are here.
//   (3) the list must not be written again while a thread still reads it.  A body that uses LDS of its own between
//       reads ends on a barrier anyway, and that barrier is (3) as well: say ENDS_ON_BARRIER = true and none is added
//       (sparse_long_sort_kernel, sparse_runlength_kernel, read_stats_long_kernel).  A body that does not end on one
//       says false, and (3) is put once behind the block's last read (read_spans_long_kernel, whose rounds alternate
//       between two LDS sets and need no barrier between reads).
// Without a long read in the block nobody reads the list, and s_n is overwritten by the value it holds.
template <int NT, bool ENDS_ON_BARRIER, class Body>
__device__ __forceinline__ void long_reads(const int64_t *__restrict__ start, const int32_t *__restrict__ length,
                                           int64_t nN, int64_t nS, int k, Body body) {
  __shared__ int s_list[NT];
  __shared__ int s_n;
  const int tid = threadIdx.x;
  for (int64_t base = (int64_t)blockIdx.x * NT; base < nS; base += (int64_t)gridDim.x * NT) {
    if (tid == 0) s_n = 0;
    __syncthreads();                                    // (1)
    if (base + tid < nS && read_windows(start[base + tid], length[base + tid], nN, k) > READ_CAP64)
      s_list[atomicAdd(&s_n, 1)] = tid;
    __syncthreads();                                    // (2)
    const int nl = s_n;
    for (int j = 0; j < nl; ++j) {
      const int64_t i = base + s_list[j];
      const int64_t st = start[i];
      body(i, st, read_windows(st, length[i], nN, k));
    }
    if (!ENDS_ON_BARRIER) __syncthreads();              // (3)
  }
}

}  // namespace
#endif  // __HIPCC__
