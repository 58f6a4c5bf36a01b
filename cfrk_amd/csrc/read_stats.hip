// read_stats.hip -- per-read abundance statistics against a finished global result: for every read the number of its
// valid windows, how many of their k-mers are present / below a threshold, and min, lower median, max and sum of
// their counts (cfrk_read_stats, 32 bytes per read).  The lookups are query.hip's (query_dev.h: same index, same
// probes); the front end is sparse.hip's (lane_group.h: a group of lanes per read, the read staged in LDS).  Nothing
// per window goes to HBM.
//
// Fast path, read_stats_kernel<G, MODE, CANON>: G lanes of one wave own a read (G = 16: up to 256 windows, four reads
// per wave; G = 64: up to CFRK_STATS_FAST_WINDOWS).  The read's codes are staged in LDS with coalesced dword loads;
// every lane rolls its run of windows (forward key and, when canonical, the reverse complement: one word for
// k <= 32, unsigned __int128 above) and looks them up in batches: the first-slot loads of a batch are all issued
// before any is resolved (the QB pattern of query_reads1_kernel).  windows, present, below, min, max and sum are kept
// per lane and reduced across the group with shuffles.  The median is exact and needs no sort: every window's count
// is parked in LDS (slot j of lane l at j * G + l, so a lane reads back only what it wrote, without bank conflicts; an
// invalid window as 0xFFFFFFFF, above every count), and the group bisects on the VALUE between min and max -- a radix
// select of one bit per step, whose histogram is a count per lane and a sum across the group: ceil(log2(max - min + 1))
// steps, none when all counts are equal.  (A bitonic sort of the counts in LDS, the network of lane_group.h, was built
// first and measured: DESIGN.md 4.9.)  One lane stores the row as two 16-byte stores.  No scratch, no HBM atomics.
// Every read is handled by exactly one of three launches, by its size class (as cfrk_sparse_count does): G = 16,
// G = 64, and for reads above the fast path's capacity read_stats_long_kernel: one workgroup per read, a pass for
// the reductions and four 8-bit radix-select passes for the median (LDS histogram of 256 bins), each of which looks
// the windows up again -- no buffer, exact for any length, slow.
// MODE 0: dense index (k <= 12), 1: one-word hash (k <= 32), 2: two-word hash (k > 32).
#include "common.h"
#include "lane_group.h"
#include "query_dev.h"
#include "read_windows.h"

#include <algorithm>

namespace {

constexpr int RS_CAP16 = 256;                          // windows a 16-lane group holds
constexpr int RS_CAP64 = CFRK_STATS_FAST_WINDOWS;      // windows a 64-lane group holds (the fast path's capacity)
constexpr int RS_STAGE_SLACK = 72;                     // k - 1 <= 63 bytes + skew <= 3 + dword round-up <= 3, a multiple of 8
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
  const int t0 = lane * per, t1 = min(t0 + per, nwin);
  Acc acc;
  if (t0 < t1) {
    Roller<TWO, CANON> R(k);
    for (int p = t0; p < t0 + k - 1; ++p) R.push((int)stage[p]);
    for (int w0 = t0; w0 < t1; w0 += B) {
      T key[B];
      uint4 v[B], v2[B];
      uint32_t d[B];
      bool ok[B];
#pragma unroll
      for (int u = 0; u < B; ++u) {                    // every first-slot load of the batch is issued here ...
        const bool in = w0 + u < t1;
        if (in) R.push((int)stage[w0 + u + k - 1]);
        ok[u] = in && R.valid();
        key[u] = R.key();
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
      for (int u = 0; u < B; ++u) {                    // ... before any is resolved
        if (w0 + u >= t1) break;
        uint32_t r = RS_INVALID;
        if (ok[u]) {
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
          acc.add(r, threshold);
        }
        cnt[(w0 + u - t0) * G + lane] = r;   // (slot j of lane l at j * G + l: conflict-free, read back by l only)
      }
    }
  }
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

// G = 16: reads of 0 .. RS_CAP16 windows (a read without windows gets its zero row here); G = 64: RS_CAP16 + 1 .. RS_CAP64
template <int G, int MODE, bool CANON>
__global__ __launch_bounds__(G == 16 ? 256 : 64) void read_stats_kernel(
    const int8_t *__restrict__ data, const int64_t *__restrict__ start, const int32_t *__restrict__ length, int64_t nN,
    int64_t nS, QIndex q, uint32_t threshold, cfrk_read_stats *__restrict__ out, bool vec) {
  constexpr int NT = (G == 16) ? 256 : 64;
  constexpr int RPB = NT / G;
  constexpr int CAP = (G == 16) ? RS_CAP16 : RS_CAP64;
  __shared__ uint32_t s_cnt[RPB][CAP + G];           // ceil(nwin / G) * G slots
  __shared__ int32_t s_stage[RPB][(CAP + RS_STAGE_SLACK) / 4];
  const int grp = threadIdx.x / G, lane = threadIdx.x % G;
  const int k = q.k;
  if (G == 16) {
    for (int64_t i = (int64_t)blockIdx.x * RPB + grp; i < nS; i += (int64_t)gridDim.x * RPB) {
      const int64_t st = start[i];
      const int nwin = read_windows(st, length[i], nN, k);
      if (nwin > RS_CAP16) continue;
      if (nwin == 0) { if (lane == 0) store_row(out, i, vec, 0, 0, 0, 0, 0, 0, 0); continue; }
      stats_read<G, MODE, CANON>(data, nN, i, st, nwin, q, threshold, s_cnt[grp], s_stage[grp], lane, out, vec);
    }
  } else {
    // the wave looks at 64 reads at a time and takes those of its size class one after the other
    for (int64_t base = (int64_t)blockIdx.x * 64; base < nS; base += (int64_t)gridDim.x * 64) {
      const int64_t mine = base + lane;
      int w = 0;
      if (mine < nS) w = read_windows(start[mine], length[mine], nN, k);
      unsigned long long todo = __ballot(w > RS_CAP16 && w <= RS_CAP64);
      while (todo) {
        const int b = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int64_t i = base + b;
        const int64_t st = start[i];
        const int nwin = read_windows(st, length[i], nN, k);
        stats_read<G, MODE, CANON>(data, nN, i, st, nwin, q, threshold, s_cnt[0], s_stage[0], lane, out, vec);
      }
    }
  }
}

// ---- long reads -----------------------------------------------------------------------------

// the counts of the read's valid windows, every thread a share of them (chunks of 32 windows, rolled from the read's
// bytes in device memory: st + p <= st + length - 1): f(count)
template <int MODE, bool CANON, class F>
__device__ __forceinline__ void long_walk(const int8_t *__restrict__ data, int64_t st, int nwin, const QIndex &q, int tid,
                                          F f) {
  const int k = q.k;
  for (int64_t c0 = (int64_t)tid * 32; c0 < nwin; c0 += (int64_t)RS_LONG_NT * 32) {
    const int64_t c1 = c0 + 32 < nwin ? c0 + 32 : (int64_t)nwin;
    Roller<MODE == 2, CANON> R(k);
    for (int64_t p = c0; p < c1 + k - 1; ++p) {
      R.push((int)data[st + p]);
      if (p >= c0 + k - 1 && R.valid()) f(rs_lookup<MODE>(q, R.key()));
    }
  }
}

// every workgroup looks at RS_LONG_NT reads at a time, lists the long ones in LDS and takes them one after the other
template <int MODE, bool CANON>
__global__ __launch_bounds__(RS_LONG_NT) void read_stats_long_kernel(
    const int8_t *__restrict__ data, const int64_t *__restrict__ start, const int32_t *__restrict__ length, int64_t nN,
    int64_t nS, QIndex q, uint32_t threshold, cfrk_read_stats *__restrict__ out, bool vec) {
  __shared__ int s_list[RS_LONG_NT];
  __shared__ int s_n;
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_windows, s_present, s_below, s_mn, s_mx, s_prefix, s_rank;
  __shared__ unsigned long long s_sum;
  const int tid = threadIdx.x;
  const int k = q.k;
  for (int64_t base = (int64_t)blockIdx.x * RS_LONG_NT; base < nS; base += (int64_t)gridDim.x * RS_LONG_NT) {
    if (tid == 0) s_n = 0;
    __syncthreads();
    if (base + tid < nS && read_windows(start[base + tid], length[base + tid], nN, k) > RS_CAP64)
      s_list[atomicAdd(&s_n, 1)] = tid;
    __syncthreads();
    const int nl = s_n;
    for (int j = 0; j < nl; ++j) {
      const int64_t i = base + s_list[j];
      const int64_t st = start[i];
      const int nwin = read_windows(st, length[i], nN, k);
      if (tid == 0) {
        s_windows = 0; s_present = 0; s_below = 0; s_mn = 0xFFFFFFFFu; s_mx = 0; s_sum = 0;
      }
      __syncthreads();
      Acc acc;
      long_walk<MODE, CANON>(data, st, nwin, q, tid, [&](uint32_t c) { acc.add(c, threshold); });
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
        for (int d = 3; d >= 0; --d) {
          s_hist[tid] = 0;                             // (RS_LONG_NT == 256 bins)
          __syncthreads();
          uint32_t bin = 0, n = 0;                     // equal neighbours are added together
          long_walk<MODE, CANON>(data, st, nwin, q, tid, [&](uint32_t c) {
            if (d < 3 && (c >> (8 * (d + 1))) != prefix) return;
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
    }
  }
}

template <int MODE, bool CANON>
void launch_all(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                int64_t nS, const QIndex &q, uint32_t threshold, cfrk_read_stats *d_out, bool vec) {
  const int64_t cus = ctx->num_cus;
  // (many more workgroups than fit at once: a CU takes a new one whenever one of its seven -- LDS -- ends)
  const unsigned g16 = (unsigned)std::min<int64_t>((nS + 15) / 16, cus * 64);
  const unsigned g64 = (unsigned)std::min<int64_t>((nS + 63) / 64, cus * 64);
  const unsigned glong = (unsigned)std::min<int64_t>((nS + RS_LONG_NT - 1) / RS_LONG_NT, cus * 4);
  hipLaunchKernelGGL((read_stats_kernel<16, MODE, CANON>), dim3(g16), dim3(256), 0, ctx->stream, d_data, d_start,
                     d_length, nN, nS, q, threshold, d_out, vec);
  hipLaunchKernelGGL((read_stats_kernel<64, MODE, CANON>), dim3(g64), dim3(64), 0, ctx->stream, d_data, d_start,
                     d_length, nN, nS, q, threshold, d_out, vec);
  hipLaunchKernelGGL((read_stats_long_kernel<MODE, CANON>), dim3(glong), dim3(RS_LONG_NT), 0, ctx->stream, d_data,
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
