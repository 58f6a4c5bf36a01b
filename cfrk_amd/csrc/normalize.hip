// normalize.hip -- digital normalisation (normalize-by-median) against the LIVE HBM table: the reads of a call are
// taken in rounds of batch_reads; every read of a round is judged against the table as it stands at the round's
// beginning (kept iff it has a valid window and the lower median of its windows' counts is below the cutoff), then every
// valid window of every kept read of the round is added to the table.  Two phases per round, three launches each -- one
// per size class of reads (lane_group.h) -- all enqueued on the context stream without a host synchronisation between
// rounds: the stream orders judge(r) < insert(r) < judge(r + 1), so a judge kernel never runs beside a writer and reads
// the table with plain loads (table.h: table_find1 / table_find2), and the inserts are commutative saturating adds
// (table_add1 / table_add2).  Keep bytes and counts are therefore independent of scheduling.
// A paired call (interleaved mates 2j, 2j + 1) puts ONE more launch between the two phases of a round: the join of
// pairs.hip rewrites the round's keep bytes in place so that both mates of a pair carry the same byte, and counts the
// kept pairs.  It is a launch of its own and not part of the insert kernels because the two mates of a pair may belong
// to different size classes, hence to different launches; the kernels of this file are the same in both kinds of call.
//
// The judge needs no median select: with W valid windows the lower median is element (W - 1) / 2 of the sorted counts,
// which is below the cutoff iff more than (W - 1) / 2 counts are -- one count per lane and one sum across the group.
//
// Fast path, normalize_judge_kernel<G, TWO, CANON> / normalize_insert_kernel<G, TWO, CANON>: the read is staged in LDS
// by its lane group, the windows are split over the lanes and rolled from LDS.  The judge computes the keys of a batch
// of NB windows per lane and issues their first-slot loads together before resolving any.  The table is SoA: the key
// word(s) and the count word of a slot are separate loads; the count is loaded SPECULATIVELY with the key -- a judged
// window mostly hits (the reads of a covered locus are what the call is there to drop), so waiting for the key first
// would put a second dependent HBM round trip on almost every window, while the speculative load costs one extra
// 4-byte request on the windows that miss.  Longer probes resolve one after the other.
// Long reads (more than READ_CAP64 windows): a workgroup per read, chunks of LONG_CHUNK windows per thread rolled from
// device memory, one lookup or add at a time.
#include "common.h"
#include "lane_group.h"
#include "msp.h"
#include "read_windows.h"
#include "table.h"

namespace {

constexpr int NORM_LONG_NT = 256;
constexpr int NB = 8;                                  // windows per lane whose first-slot loads are in flight together

template <bool TWO, class T>
__device__ __forceinline__ uint64_t key_hi(T key) {
  if constexpr (TWO) return (uint64_t)(key >> 64);
  else return 0;
}
template <bool TWO, class T>
__device__ __forceinline__ uint64_t key_slot(const TableView &t, T key) {
  return (TWO ? dev_mix64((uint64_t)key ^ dev_mix64(key_hi<TWO>(key))) : dev_mix64((uint64_t)key)) >> t.shift;
}
template <bool TWO, class T>
__device__ __forceinline__ uint32_t key_find(const TableView &t, T key, uint32_t limit) {
  return TWO ? table_find2(t, (uint64_t)key, key_hi<TWO>(key), limit) : table_find1(t, (uint64_t)key, limit);
}
template <bool TWO, class T>
__device__ __forceinline__ void key_add(const TableView &t, T key, uint32_t limit) {
  if (TWO) table_add2(t, (uint64_t)key, key_hi<TWO>(key), 1u, limit);
  else table_add1(t, (uint64_t)key, 1u, limit);
}

// what a lane (or a thread of the long path) has seen of its read
struct Tally {
  uint32_t windows = 0, below = 0;
  __device__ __forceinline__ void add(uint32_t c, uint32_t cutoff) { ++windows; below += c < cutoff; }
};
__device__ __forceinline__ bool kept_by(uint32_t windows, uint32_t below) {
  return windows != 0 && below > ((windows - 1) >> 1);
}

// Read (nwin >= 1 windows from byte st on, inside [0, nN)) judged by the G lanes of a group; stage_dw as
// read_windows.h's staged_windows.  The same verdict in every lane of the group.
template <int G, bool TWO, bool CANON>
__device__ __forceinline__ bool judge_read(const int8_t *__restrict__ data, int64_t nN, int64_t st, int nwin, int k,
                                           const TableView &t, uint32_t limit, uint32_t cutoff, int32_t *stage_dw,
                                           int lane) {
  constexpr int B = TWO ? NB / 2 : NB;                 // (a two-word slot is three loads)
  typedef typename RsKey<TWO>::type T;
  const int skew = stage_read<G>(data, nN, st, nwin + k - 1, stage_dw, lane);
  wave_sync();
  const int8_t *stage = reinterpret_cast<const int8_t *>(stage_dw) + skew;
  const int per = (nwin + G - 1) / G;
  const int t0 = lane * per, t1 = min(t0 + per, nwin);
  Tally acc;
  if (t0 < t1) {
    Roller<TWO, CANON> R(k);
    for (int p = t0; p < t0 + k - 1; ++p) R.push((int)stage[p]);
    for (int w0 = t0; w0 < t1; w0 += B) {
      T key[B];
      uint64_t h[B], klo[B], khi[B];
      uint32_t c[B];
      bool ok[B];
#pragma unroll
      for (int u = 0; u < B; ++u) {                    // every first-slot load of the batch is issued here ...
        if (w0 + u < t1) R.push((int)stage[w0 + u + k - 1]);
        ok[u] = w0 + u < t1 && R.valid();
        key[u] = R.key();
        h[u] = key_slot<TWO>(t, key[u]);
        const bool ld = ok[u] && (TWO || (uint64_t)key[u] != CFRK_EMPTY_KEY);
        klo[u] = ld ? t.lo[h[u]] : CFRK_EMPTY_KEY;
        c[u] = ld ? t.cnt[h[u]] : 0u;
        if (TWO) khi[u] = ld ? t.hi[h[u]] : 0;
      }
#pragma unroll
      for (int u = 0; u < B; ++u) {                    // ... before any is resolved
        if (!ok[u]) continue;
        const uint64_t lo = (uint64_t)key[u], hi = key_hi<TWO>(key[u]);
        uint32_t r;
        if (TWO) {
          if (c[u] == 0) r = 0;
          else if (klo[u] == lo && khi[u] == hi) r = c[u];
          else r = table_find2_from(t, (h[u] + 1) & t.mask, lo, hi, limit - 1);          // longer probes
        } else {
          if (lo == CFRK_EMPTY_KEY) r = sat_ones(t.stats[ST_ONES]);
          else if (klo[u] == CFRK_EMPTY_KEY) r = 0;
          else if (klo[u] == lo) r = c[u];
          else r = table_find1_from(t, (h[u] + 1) & t.mask, lo, limit - 1);
        }
        acc.add(r, cutoff);
      }
    }
  }
  const uint32_t windows = group_sum_u32<G>(acc.windows), below = group_sum_u32<G>(acc.below);
  wave_sync();     // the group's LDS is reused by its next read
  return kept_by(windows, below);
}

// every valid window of the read added to the table by the G lanes of a group
template <int G, bool TWO, bool CANON>
__device__ __forceinline__ void insert_read(const int8_t *__restrict__ data, int64_t nN, int64_t st, int nwin, int k,
                                            const TableView &t, uint32_t limit, int32_t *stage_dw, int lane) {
  const int skew = stage_read<G>(data, nN, st, nwin + k - 1, stage_dw, lane);
  wave_sync();
  const int8_t *stage = reinterpret_cast<const int8_t *>(stage_dw) + skew;
  const int per = (nwin + G - 1) / G;
  const int t0 = lane * per, t1 = min(t0 + per, nwin);
  if (t0 < t1) {
    Roller<TWO, CANON> R(k);
    for (int p = t0; p < t0 + k - 1; ++p) R.push((int)stage[p]);
    for (int w = t0; w < t1; ++w) {
      R.push((int)stage[w + k - 1]);
      if (R.valid()) key_add<TWO>(t, R.key(), limit);
    }
  }
  wave_sync();     // the group's LDS is reused by its next read
}

// the kept reads a thread has counted, added to the call's counter once per wave
__device__ __forceinline__ void flush_kept(uint32_t kept, unsigned long long *n_kept) {
  kept = group_sum_u32<64>(kept);
  if ((threadIdx.x & 63) == 0 && kept) atomicAdd(n_kept, (unsigned long long)kept);
}

template <int G, bool TWO, bool CANON>
__global__ __launch_bounds__(G == 16 ? 256 : 64) void normalize_judge_kernel(
    const int8_t *__restrict__ data, const int64_t *__restrict__ start, const int32_t *__restrict__ length, int64_t nN,
    int64_t nS, int k, TableView t, uint32_t cutoff, uint8_t *__restrict__ keep, unsigned long long *n_kept) {
  constexpr int RPB = (G == 16 ? 256 : 64) / G;
  constexpr int CAP = (G == 16) ? READ_CAP16 : READ_CAP64;
  __shared__ int32_t s_stage[RPB][(CAP + READ_STAGE_SLACK) / 4];
  const int grp = G == 16 ? threadIdx.x / G : 0, lane = threadIdx.x % G;
  const uint32_t limit = table_probe_limit(t);
  uint32_t kept = 0;
  class_reads<G>(
      start, length, nN, nS, k,
      [&](int64_t i, int64_t st, int nwin) {
        const bool yes = judge_read<G, TWO, CANON>(data, nN, st, nwin, k, t, limit, cutoff, s_stage[grp], lane);
        if (lane == 0) { keep[i] = yes; kept += yes; }
      },
      [&](int64_t i) { if (lane == 0) keep[i] = 0; });
  flush_kept(kept, n_kept);
}

template <int G, bool TWO, bool CANON>
__global__ __launch_bounds__(G == 16 ? 256 : 64) void normalize_insert_kernel(
    const int8_t *__restrict__ data, const int64_t *__restrict__ start, const int32_t *__restrict__ length, int64_t nN,
    int64_t nS, int k, TableView t, const uint8_t *__restrict__ keep) {
  constexpr int RPB = (G == 16 ? 256 : 64) / G;
  constexpr int CAP = (G == 16) ? READ_CAP16 : READ_CAP64;
  __shared__ int32_t s_stage[RPB][(CAP + READ_STAGE_SLACK) / 4];
  const int grp = G == 16 ? threadIdx.x / G : 0, lane = threadIdx.x % G;
  const uint32_t limit = table_probe_limit(t);
  class_reads<G>(
      start, length, nN, nS, k,
      [&](int64_t i, int64_t st, int nwin) {
        if (keep[i]) insert_read<G, TWO, CANON>(data, nN, st, nwin, k, t, limit, s_stage[grp], lane);
      },
      [](int64_t) {});
}

// ---- long reads -----------------------------------------------------------------------------

// the keys of the valid windows among [c0, min(c0 + LONG_CHUNK, nwin)) of a read, rolled from its bytes in device
// memory (st + p <= st + length - 1); nothing when c0 >= nwin
template <bool TWO, bool CANON, class F>
__device__ __forceinline__ void long_keys(const int8_t *__restrict__ data, int64_t st, int nwin, int k, int64_t c0, F f) {
  if (c0 >= nwin) return;
  const int64_t c1 = c0 + LONG_CHUNK < nwin ? c0 + LONG_CHUNK : (int64_t)nwin;
  Roller<TWO, CANON> R(k);
  for (int64_t p = c0; p < c1 + k - 1; ++p) {
    R.push((int)data[st + p]);
    if (p >= c0 + k - 1 && R.valid()) f(R.key());
  }
}

template <bool TWO, bool CANON>
__global__ __launch_bounds__(NORM_LONG_NT) void normalize_judge_long_kernel(
    const int8_t *__restrict__ data, const int64_t *__restrict__ start, const int32_t *__restrict__ length, int64_t nN,
    int64_t nS, int k, TableView t, uint32_t cutoff, uint8_t *__restrict__ keep, unsigned long long *n_kept) {
  __shared__ uint32_t s_windows, s_below;
  const int tid = threadIdx.x;
  const uint32_t limit = table_probe_limit(t);
  uint32_t kept = 0;
  // (the body ends on a barrier: the sums are reset by the next read)
  long_reads<NORM_LONG_NT, true>(start, length, nN, nS, k, [&](int64_t i, int64_t st, int nwin) {
    if (tid == 0) { s_windows = 0; s_below = 0; }
    __syncthreads();
    Tally acc;
    for (int64_t c0 = (int64_t)tid * LONG_CHUNK; c0 < nwin; c0 += (int64_t)NORM_LONG_NT * LONG_CHUNK)
      long_keys<TWO, CANON>(data, st, nwin, k, c0, [&](typename RsKey<TWO>::type key) {
        acc.add(key_find<TWO>(t, key, limit), cutoff);
      });
    if (acc.windows) { atomicAdd(&s_windows, acc.windows); atomicAdd(&s_below, acc.below); }
    __syncthreads();
    if (tid == 0) {
      const bool yes = kept_by(s_windows, s_below);
      keep[i] = yes;
      kept += yes;
    }
    __syncthreads();
  });
  flush_kept(kept, n_kept);
}

template <bool TWO, bool CANON>
__global__ __launch_bounds__(NORM_LONG_NT) void normalize_insert_long_kernel(
    const int8_t *__restrict__ data, const int64_t *__restrict__ start, const int32_t *__restrict__ length, int64_t nN,
    int64_t nS, int k, TableView t, const uint8_t *__restrict__ keep) {
  const int tid = threadIdx.x;
  const uint32_t limit = table_probe_limit(t);
  // (no LDS of its own between reads: the walker puts its barrier (3) behind the block's last read)
  long_reads<NORM_LONG_NT, false>(start, length, nN, nS, k, [&](int64_t i, int64_t st, int nwin) {
    if (!keep[i]) return;
    for (int64_t c0 = (int64_t)tid * LONG_CHUNK; c0 < nwin; c0 += (int64_t)NORM_LONG_NT * LONG_CHUNK)
      long_keys<TWO, CANON>(data, st, nwin, k, c0, [&](typename RsKey<TWO>::type key) { key_add<TWO>(t, key, limit); });
  });
}

// the launches of one round: reads [0, nS) of the arrays as they are passed; judge, then (paired calls: the join of
// pairs.hip between the two) insert
template <bool TWO, bool CANON>
void launch_judge(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                  int64_t nS, const TableView &t, uint32_t cutoff, uint8_t *d_keep, unsigned long long *d_kept) {
  const ClassGrids g = class_grids(nS, ctx->num_cus, NORM_LONG_NT);
  const int k = ctx->g_k;
  hipLaunchKernelGGL((normalize_judge_kernel<16, TWO, CANON>), dim3(g.g16), dim3(256), 0, ctx->stream, d_data, d_start,
                     d_length, nN, nS, k, t, cutoff, d_keep, d_kept);
  hipLaunchKernelGGL((normalize_judge_kernel<64, TWO, CANON>), dim3(g.g64), dim3(64), 0, ctx->stream, d_data, d_start,
                     d_length, nN, nS, k, t, cutoff, d_keep, d_kept);
  hipLaunchKernelGGL((normalize_judge_long_kernel<TWO, CANON>), dim3(g.glong), dim3(NORM_LONG_NT), 0, ctx->stream, d_data,
                     d_start, d_length, nN, nS, k, t, cutoff, d_keep, d_kept);
}
template <bool TWO, bool CANON>
void launch_insert(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                   int64_t nS, const TableView &t, const uint8_t *d_keep) {
  const ClassGrids g = class_grids(nS, ctx->num_cus, NORM_LONG_NT);
  const int k = ctx->g_k;
  hipLaunchKernelGGL((normalize_insert_kernel<16, TWO, CANON>), dim3(g.g16), dim3(256), 0, ctx->stream, d_data, d_start,
                     d_length, nN, nS, k, t, d_keep);
  hipLaunchKernelGGL((normalize_insert_kernel<64, TWO, CANON>), dim3(g.g64), dim3(64), 0, ctx->stream, d_data, d_start,
                     d_length, nN, nS, k, t, d_keep);
  hipLaunchKernelGGL((normalize_insert_long_kernel<TWO, CANON>), dim3(g.glong), dim3(NORM_LONG_NT), 0, ctx->stream, d_data,
                     d_start, d_length, nN, nS, k, t, d_keep);
}

// every round of a call; d_pairs NULL: reads on their own (the judge counts the kept reads into *d_kept); else interleaved
// pairs, `mode` applied to the round's keep bytes in place by the join, which adds its four counts to d_pairs[0 .. 4)
template <bool TWO, bool CANON>
int launch_rounds(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN, int64_t nS,
                  uint32_t cutoff, int64_t batch_reads, int mode, uint8_t *d_keep, unsigned long long *d_kept,
                  unsigned long long *d_pairs) {
  const TableView t = cfrk_table_view(ctx);
  for (int64_t off = 0; off < nS;) {
    const int64_t nb = nS - off < batch_reads ? nS - off : batch_reads;
    launch_judge<TWO, CANON>(ctx, d_data, d_start + off, d_length + off, nN, nb, t, cutoff, d_keep + off, d_kept);
    if (d_pairs) {
      HIP_TRY(ctx, hipGetLastError());
      if (const int rc = cfrk_pair_join_launch(ctx, nb / 2, 2, mode, 0, d_keep + off, d_keep + off + 1, nullptr, nullptr, nullptr,
                                               nullptr, d_keep + off, d_keep + off + 1, nullptr, nullptr, d_pairs)) return rc;
    }
    launch_insert<TWO, CANON>(ctx, d_data, d_start + off, d_length + off, nN, nb, t, d_keep + off);
    HIP_TRY(ctx, hipGetLastError());
    off += nb;
  }
  return CFRK_OK;
}

int launch_call(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN, int64_t nS,
                uint32_t cutoff, int64_t batch_reads, int mode, uint8_t *d_keep, unsigned long long *d_kept,
                unsigned long long *d_pairs) {
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  if (ctx->g_two) {
    if (canon) return launch_rounds<true, true>(ctx, d_data, d_start, d_length, nN, nS, cutoff, batch_reads, mode, d_keep, d_kept, d_pairs);
    return launch_rounds<true, false>(ctx, d_data, d_start, d_length, nN, nS, cutoff, batch_reads, mode, d_keep, d_kept, d_pairs);
  }
  if (canon) return launch_rounds<false, true>(ctx, d_data, d_start, d_length, nN, nS, cutoff, batch_reads, mode, d_keep, d_kept, d_pairs);
  return launch_rounds<false, false>(ctx, d_data, d_start, d_length, nN, nS, cutoff, batch_reads, mode, d_keep, d_kept, d_pairs);
}

}  // namespace

// Every round of the call enqueued on the context stream: judge into d_keep (every byte written), insert the kept
// reads, the number of kept reads added to *d_kept (zeroed by the caller).  The result must live in the HBM table
// (abi.hip flushes a pending list first).  A round addresses its reads by offsetting start / length / keep.  No host
// synchronisation.  Arguments are checked by the callers (abi.hip).  nS >= 1, batch_reads >= 1.
int cfrk_normalize_launch(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                          int64_t nS, uint32_t cutoff, int64_t batch_reads, uint8_t *d_keep, unsigned long long *d_kept) {
  return launch_call(ctx, d_data, d_start, d_length, nN, nS, cutoff, batch_reads, 0, d_keep, d_kept, nullptr);
}

// The same for interleaved pairs: judge (the kernels' own count of kept reads goes to *d_scratch, which nobody reads),
// join, insert per round; the join's counts are added to d_pairs[0 .. 4) (zeroed by the caller), the kept reads of the
// call are twice its kept pairs.  nS >= 2, nS and batch_reads even: a round holds whole pairs.
int cfrk_normalize_pairs_launch(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                                int64_t nS, uint32_t cutoff, int64_t batch_reads, int mode, uint8_t *d_keep,
                                unsigned long long *d_scratch, unsigned long long *d_pairs) {
  return launch_call(ctx, d_data, d_start, d_length, nN, nS, cutoff, batch_reads, mode, d_keep, d_scratch, d_pairs);
}
