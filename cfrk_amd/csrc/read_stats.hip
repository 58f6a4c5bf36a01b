// read_stats.hip -- per-read abundance statistics against a finished global result: for every read the number of its
// valid windows, how many of their k-mers are present / below a threshold, and min, lower median, max and sum of
// their counts (cfrk_read_stats, 32 bytes per read).  The index and its probes are query.hip's (query_dev.h); the
// three launches by size class and the walk over a read's windows are lane_group.h's and read_windows.h's.  Nothing
// per window goes to HBM.
//
// Fast path, read_stats_kernel<G, MODE, CANON>: windows, present, below, min, max and sum are kept per lane and reduced
// across the group with shuffles.  The median is exact and needs no sort: every window's count is parked in LDS (slot j
// of lane l at j * G + l, so a lane reads back only what it wrote, without bank conflicts; an invalid window as
// 0xFFFFFFFF, above every count), and the group bisects on the VALUE between min and max -- a radix select of one bit
// per step, whose histogram is a count per lane and a sum across the group: ceil(log2(max - min + 1)) steps, none when
// all counts are equal.  (A bitonic sort of the counts in LDS, the network of lane_group.h, was built first and
// measured: DESIGN.md 4.9.)  One lane stores the row as two 16-byte stores.  No scratch, no HBM atomics.
// Long reads, read_stats_long_kernel: one workgroup per read, a pass for the reductions and four 8-bit radix-select
// passes for the median (LDS histogram of 256 bins), each of which looks the windows up again -- no buffer, exact for
// any length, slow.
#include "common.h"
#include "lane_group.h"
#include "query_dev.h"
#include "read_windows.h"

namespace {

constexpr int RS_LONG_NT = 256;
constexpr uint32_t RS_INVALID = 0xFFFFFFFFu;           // an invalid window in the count array: sorts behind every count

// what a lane (or a thread of the long path) has seen of its read
struct Acc {
  uint32_t windows, present, below, mn, mx;
  uint64_t sum;
  __device__ __forceinline__ Acc() : windows(0), present(0), below(0), mn(0xFFFFFFFFu), mx(0), sum(0) {}
  __device__ __forceinline__ void add(uint32_t c, uint32_t threshold) {
    ++windows;
    present += c != 0;
    below += c < threshold;
    mn = c < mn ? c : mn;
    mx = c > mx ? c : mx;
    sum += c;
  }
};

__device__ __forceinline__ void store_row(cfrk_read_stats *__restrict__ out, int64_t i, bool vec, uint32_t windows,
                                          uint32_t present, uint32_t below, uint32_t mn, uint32_t med, uint32_t mx,
                                          uint64_t sum) {
  if (vec) {
    uint4 *p = reinterpret_cast<uint4 *>(out + i);
    p[0] = make_uint4(windows, present, below, mn);
    p[1] = make_uint4(med, mx, (uint32_t)sum, (uint32_t)(sum >> 32));
  } else {
    cfrk_read_stats &r = out[i];
    r.windows = windows; r.present = present; r.below = below;
    r.min = mn; r.median = med; r.max = mx; r.sum = sum;
  }
}

// read i (nwin >= 1 windows from byte st on, inside [0, nN)) by the G lanes of a group
template <int G, int MODE, bool CANON>
__device__ __forceinline__ void stats_read(const int8_t *__restrict__ data, int64_t nN, int64_t i, int64_t st, int nwin,
                                           const QIndex &q, uint32_t threshold, uint32_t *cnt, int32_t *stage_dw,
                                           int lane, cfrk_read_stats *__restrict__ out, bool vec) {
  Acc acc;
  int t0, t1;
  staged_windows<G, MODE, CANON>(data, nN, st, nwin, q, stage_dw, lane, t0, t1, [&](int w, bool valid, uint32_t c) {
    if (valid) acc.add(c, threshold);
    cnt[(w - t0) * G + lane] = valid ? c : RS_INVALID;   // (slot j of lane l at j * G + l: conflict-free, read by l only)
  });
  const uint32_t windows = group_sum_u32<G>(acc.windows);
  const uint32_t present = group_sum_u32<G>(acc.present), below = group_sum_u32<G>(acc.below);
  const uint32_t mn = group_min_u32<G>(acc.mn), mx = group_max_u32<G>(acc.mx);
  const uint64_t sum = group_sum_u64<G>(acc.sum);
  // the lower median = the smallest v with (counts <= v) > rank: bisection on v between min and max, every step a
  // count over the lane's own slots and a sum across the group (an invalid window's 0xFFFFFFFF is above every v)
  const uint32_t rank = windows ? (windows - 1) >> 1 : 0;
  uint32_t lo = mn, hi = windows ? mx : mn;            // (the group's lanes agree on both: the loop is uniform in it)
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    uint32_t c = 0;
    for (int j = 0; j < t1 - t0; ++j) c += cnt[j * G + lane] <= mid;
    c = group_sum_u32<G>(c);
    if (c > rank) hi = mid; else lo = mid + 1;
  }
  const uint32_t med = lo;
  if (lane == 0) {
    if (windows) store_row(out, i, vec, windows, present, below, mn, med, mx, sum);
    else store_row(out, i, vec, 0, 0, 0, 0, 0, 0, 0);
  }
  wave_sync();     // the group's LDS is reused by its next read
}

template <int G, int MODE, bool CANON>
__global__ __launch_bounds__(G == 16 ? 256 : 64) void read_stats_kernel(
    const int8_t *__restrict__ data, const int64_t *__restrict__ start, const int32_t *__restrict__ length, int64_t nN,
    int64_t nS, QIndex q, uint32_t threshold, cfrk_read_stats *__restrict__ out, bool vec) {
  constexpr int RPB = (G == 16 ? 256 : 64) / G;
  constexpr int CAP = (G == 16) ? READ_CAP16 : READ_CAP64;
  __shared__ uint32_t s_cnt[RPB][CAP + G];           // ceil(nwin / G) * G slots
  __shared__ int32_t s_stage[RPB][(CAP + READ_STAGE_SLACK) / 4];
  const int grp = G == 16 ? threadIdx.x / G : 0, lane = threadIdx.x % G;
  class_reads<G>(
      start, length, nN, nS, q.k,
      [&](int64_t i, int64_t st, int nwin) {
        stats_read<G, MODE, CANON>(data, nN, i, st, nwin, q, threshold, s_cnt[grp], s_stage[grp], lane, out, vec);
      },
      [&](int64_t i) { if (lane == 0) store_row(out, i, vec, 0, 0, 0, 0, 0, 0, 0); });
}

// ---- long reads -----------------------------------------------------------------------------

template <int MODE, bool CANON>
__global__ __launch_bounds__(RS_LONG_NT) void read_stats_long_kernel(
    const int8_t *__restrict__ data, const int64_t *__restrict__ start, const int32_t *__restrict__ length, int64_t nN,
    int64_t nS, QIndex q, uint32_t threshold, cfrk_read_stats *__restrict__ out, bool vec) {
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_windows, s_present, s_below, s_mn, s_mx, s_prefix, s_rank;
  __shared__ unsigned long long s_sum;
  const int tid = threadIdx.x;
  // (the body ends on a barrier: the sums are reset by the next read)
  long_reads<RS_LONG_NT, true>(start, length, nN, nS, q.k, [&](int64_t i, int64_t st, int nwin) {
    if (tid == 0) {
      s_windows = 0; s_present = 0; s_below = 0; s_mn = 0xFFFFFFFFu; s_mx = 0; s_sum = 0;
    }
    __syncthreads();
    Acc acc;
    long_walk<RS_LONG_NT, MODE, CANON>(data, st, nwin, q, tid, [&](int, bool valid, uint32_t c) {
      if (valid) acc.add(c, threshold);
    });
    if (acc.windows) {
      atomicAdd(&s_windows, acc.windows);
      atomicAdd(&s_present, acc.present);
      atomicAdd(&s_below, acc.below);
      atomicMin(&s_mn, acc.mn);
      atomicMax(&s_mx, acc.mx);
      atomicAdd(&s_sum, (unsigned long long)acc.sum);
    }
    __syncthreads();
    const uint32_t windows = s_windows, mn = s_mn, mx = s_mx;
    uint32_t med = mn;
    if (windows && mn != mx) {
      // radix select, most significant byte first: the element of rank `rank` among the counts whose bytes above
      // the current one equal `prefix`
      uint32_t prefix = 0, rank = (windows - 1) >> 1;
      // (one copy of the pass in every index mode, as before the walk was shared: with the wider functor the compiler
      // peels the first pass and doubles the hash modes' kernels)
#pragma nounroll
      for (int d = 3; d >= 0; --d) {
        s_hist[tid] = 0;                               // (RS_LONG_NT == 256 bins)
        __syncthreads();
        uint32_t bin = 0, n = 0;                       // equal neighbours are added together
        long_walk<RS_LONG_NT, MODE, CANON>(data, st, nwin, q, tid, [&](int, bool valid, uint32_t c) {
          if (!valid || (d < 3 && (c >> (8 * (d + 1))) != prefix)) return;
          const uint32_t b = (c >> (8 * d)) & 255u;
          if (b != bin && n) { atomicAdd(&s_hist[bin], n); n = 0; }
          bin = b;
          ++n;
        });
        if (n) atomicAdd(&s_hist[bin], n);
        __syncthreads();
        if (tid == 0) {
          uint32_t before = 0;
          int b = 0;
          while (b < 255 && before + s_hist[b] <= rank) before += s_hist[b++];
          s_prefix = (prefix << 8) | (uint32_t)b;
          s_rank = rank - before;
        }
        __syncthreads();
        prefix = s_prefix;
        rank = s_rank;
      }
      med = prefix;
    }
    if (tid == 0) {
      if (windows) store_row(out, i, vec, windows, s_present, s_below, mn, med, mx, (uint64_t)s_sum);
      else store_row(out, i, vec, 0, 0, 0, 0, 0, 0, 0);
    }
    __syncthreads();
  });
}

template <int MODE, bool CANON>
void launch_all(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                int64_t nS, const QIndex &q, uint32_t threshold, cfrk_read_stats *d_out, bool vec) {
  const ClassGrids g = class_grids(nS, ctx->num_cus, RS_LONG_NT);       // (at G = 16 a CU holds seven workgroups, by LDS)
  hipLaunchKernelGGL((read_stats_kernel<16, MODE, CANON>), dim3(g.g16), dim3(256), 0, ctx->stream, d_data, d_start,
                     d_length, nN, nS, q, threshold, d_out, vec);
  hipLaunchKernelGGL((read_stats_kernel<64, MODE, CANON>), dim3(g.g64), dim3(64), 0, ctx->stream, d_data, d_start,
                     d_length, nN, nS, q, threshold, d_out, vec);
  hipLaunchKernelGGL((read_stats_long_kernel<MODE, CANON>), dim3(g.glong), dim3(RS_LONG_NT), 0, ctx->stream, d_data,
                     d_start, d_length, nN, nS, q, threshold, d_out, vec);
}

}  // namespace

// Statistics of every read against the job's index (built, synchronising, when it is not valid); the three kernels --
// one per size class of reads -- are left enqueued.  Arguments are checked by the callers (abi.hip).  nS >= 1.
int cfrk_read_stats_launch(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                           int64_t nN, int64_t nS, uint32_t threshold, cfrk_read_stats *d_out) {
  QIndex q;
  int rc = cfrk_query_index(ctx, &q);
  if (rc) return rc;
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  const bool vec = ((uintptr_t)d_out & 15) == 0;
#define RS_LAUNCH(MODE)                                                                                          \
  do {                                                                                                           \
    if (canon) launch_all<MODE, true>(ctx, d_data, d_start, d_length, nN, nS, q, threshold, d_out, vec);         \
    else launch_all<MODE, false>(ctx, d_data, d_start, d_length, nN, nS, q, threshold, d_out, vec);              \
  } while (0)
  if (q.k <= 12) RS_LAUNCH(0);
  else if (q.k <= 32) RS_LAUNCH(1);
  else RS_LAUNCH(2);
#undef RS_LAUNCH
  HIP_TRY(ctx, hipGetLastError());
  return CFRK_OK;
}
