// read_filter.hip -- act on a finished global result per read: the SOLID SPAN of every read (cfrk_read_span: the
// bases that a run of windows whose counts lie in [min_count, max_count] covers), and the SELECT that compacts the kept,
// trimmed reads into new struct-read buffers.  The trimmed read set stays on the device from text to second count.
//
// Spans.  The three launches by size class and the walk over a read's windows are lane_group.h's and
// read_windows.h's; what is the filter's is the reduction, the "longest run of ones" monoid: a
// stretch of windows is summarised as {first window, windows, solid windows at its beginning, solid windows at its
// end, longest solid run inside and where it begins}; two neighbouring stretches combine into their union (runs_join:
// the run across the seam is a.suf + b.pre), associatively, so the lanes' stretches are combined in lane order by a
// shuffle tree and the long path's waves through LDS.  CFRK_SPAN_PREFIX reads `pre` of the whole read, CFRK_SPAN_LONGEST
// `best` / `at`; ties keep the earlier run because a later candidate replaces only when it is strictly longer.
// Nothing per window goes to HBM: no scratch, no atomics, one 8-byte store per read.
//
// Select.  A memory-bound compaction in the shape of ingest.hip; launches on the context stream, no workgroup waits
// for another one:
//   sel_reduce_kernel  one workgroup per tile of CFRK_SELECT_TILE_READS reads: kept reads and their output bytes
//   sel_scan_kernel    ONE workgroup walks the tile aggregates in blocks of CFRK_SELECT_SCAN_TILES: exclusive sums, totals
//   -- the host reads the totals back (the call's one synchronisation) and checks the capacities --
//   sel_index_kernel   per read again: start_out / length_out / index_out and the kept reads' source offsets
//   sel_copy_kernel    one workgroup per tile of CFRK_SELECT_TILE_BYTES of data_out: the reads that intersect the tile
//                      are found by a search in start_out; their source bytes are loaded as the aligned dwords that cover
//                      them and written into LDS at the alignment they have in data_out (the mutual misalignment of
//                      source and destination is taken up by LDS byte writes), then stored as whole 16-byte blocks;
//                      only the up to 15 bytes at a tile end that share a block with the neighbour go out as bytes.
//                      The work is balanced by output bytes: a long read is spread over its tiles, and inside a tile
//                      the reads go to lane groups of 16, 64 or all 256 threads by the tile's mean read size.
// All offsets are 64-bit.
#include "common.h"
#include "lane_group.h"
#include "query_dev.h"
#include "read_windows.h"

namespace {

// ---- spans ------------------------------------------------------------------------------------

constexpr int SP_LONG_NT = 256;

// a stretch of windows [first, first + len) of one read
struct Runs {
  int first, len;
  int pre, suf;      // solid windows at its beginning (== len: all solid) / at its end
  int best, at;      // the longest solid run inside, the earliest one: its windows and its first window
};

__device__ __forceinline__ Runs runs_none(int first) { Runs r; r.first = first; r.len = r.pre = r.suf = r.best = r.at = 0; return r; }

// window w = r.first + r.len joins the stretch
__device__ __forceinline__ void runs_push(Runs &r, int w, bool solid) {
  if (solid) {
    if (r.pre == r.len) ++r.pre;
    ++r.suf;
    if (r.suf > r.best) { r.best = r.suf; r.at = w - r.suf + 1; }
  } else {
    r.suf = 0;
  }
  ++r.len;
}

// a, then b behind it
__device__ __forceinline__ Runs runs_join(const Runs &a, const Runs &b) {
  if (b.len == 0) return a;
  if (a.len == 0) return b;
  Runs r;
  r.first = a.first;
  r.len = a.len + b.len;
  r.pre = a.pre == a.len ? a.len + b.pre : a.pre;
  r.suf = b.suf == b.len ? b.len + a.suf : b.suf;
  r.best = a.best; r.at = a.at;
  const int mid = a.suf + b.pre;                       // the run across the seam
  if (mid > r.best) { r.best = mid; r.at = b.first - a.suf; }
  if (b.best > r.best) { r.best = b.best; r.at = b.at; }
  return r;
}

// the stretches of the G lanes of a group joined in lane order; the result is lane 0's
template <int G>
__device__ __forceinline__ Runs group_runs(Runs r) {
  for (int o = 1; o < G; o <<= 1) {                    // (a lane that is a multiple of 2o joins [l, l+o) and [l+o, l+2o))
    Runs b;
    b.first = __shfl_down(r.first, o, G); b.len = __shfl_down(r.len, o, G);
    b.pre = __shfl_down(r.pre, o, G); b.suf = __shfl_down(r.suf, o, G);
    b.best = __shfl_down(r.best, o, G); b.at = __shfl_down(r.at, o, G);
    r = runs_join(r, b);
  }
  return r;
}

__device__ __forceinline__ void store_span(cfrk_read_span *__restrict__ out, int64_t i, const Runs &r, int mode, int k) {
  const int n = mode == CFRK_SPAN_PREFIX ? r.pre : r.best;
  cfrk_read_span s;
  s.offset = n ? (mode == CFRK_SPAN_PREFIX ? 0 : r.at) : 0;
  s.length = n ? n + k - 1 : 0;
  out[i] = s;
}

// read i (nwin >= 1 windows from byte st on, inside [0, nN)) by the G lanes of a group
template <int G, int MODE, bool CANON>
__device__ __forceinline__ void spans_read(const int8_t *__restrict__ data, int64_t nN, int64_t i, int64_t st, int nwin,
                                           const QIndex &q, uint32_t mn, uint32_t mx, int mode, int32_t *stage_dw,
                                           int lane, cfrk_read_span *__restrict__ out) {
  Runs acc = runs_none(0);
  int t0, t1;
  staged_windows<G, MODE, CANON>(data, nN, st, nwin, q, stage_dw, lane, t0, t1, [&](int w, bool valid, uint32_t c) {
    runs_push(acc, w, valid && c >= mn && c <= mx);
  });
  acc.first = t0;                                     // (runs_push leaves it alone)
  const Runs all = group_runs<G>(acc);
  if (lane == 0) store_span(out, i, all, mode, q.k);
  wave_sync();     // the group's LDS is reused by its next read
}

template <int G, int MODE, bool CANON>
__global__ __launch_bounds__(G == 16 ? 256 : 64) void read_spans_kernel(
    const int8_t *__restrict__ data, const int64_t *__restrict__ start, const int32_t *__restrict__ length, int64_t nN,
    int64_t nS, QIndex q, uint32_t mn, uint32_t mx, int mode, cfrk_read_span *__restrict__ out) {
  constexpr int RPB = (G == 16 ? 256 : 64) / G;
  constexpr int CAP = (G == 16) ? READ_CAP16 : READ_CAP64;
  __shared__ int32_t s_stage[RPB][(CAP + READ_STAGE_SLACK) / 4];
  const int grp = G == 16 ? threadIdx.x / G : 0, lane = threadIdx.x % G;
  class_reads<G>(
      start, length, nN, nS, q.k,
      [&](int64_t i, int64_t st, int nwin) {
        spans_read<G, MODE, CANON>(data, nN, i, st, nwin, q, mn, mx, mode, s_stage[grp], lane, out);
      },
      [&](int64_t i) { if (lane == 0) store_span(out, i, runs_none(0), mode, q.k); });
}

// long reads.  A read is walked in rounds of SP_LONG_NT chunks, chunk t of a round by thread t; the round's stretches
// are joined in thread order -- a shuffle tree per wave, the waves' results through LDS -- and appended to what came
// before.
template <int MODE, bool CANON>
__global__ __launch_bounds__(SP_LONG_NT) void read_spans_long_kernel(
    const int8_t *__restrict__ data, const int64_t *__restrict__ start, const int32_t *__restrict__ length, int64_t nN,
    int64_t nS, QIndex q, uint32_t mn, uint32_t mx, int mode, cfrk_read_span *__restrict__ out) {
  constexpr int NW = SP_LONG_NT / 64;
  __shared__ Runs s_runs[2][NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned round = 0;                                   // (never reset: the two sets of s_runs alternate across reads too)
  // (the body does not end on a barrier: a round's barrier stands between its writes and its reads only)
  long_reads<SP_LONG_NT, false>(start, length, nN, nS, q.k, [&](int64_t i, int64_t st, int nwin) {
    Runs all = runs_none(0);
    for (int64_t r0 = 0; r0 < nwin; r0 += (int64_t)SP_LONG_NT * LONG_CHUNK, ++round) {
      const int64_t c0 = r0 + (int64_t)tid * LONG_CHUNK;
      Runs acc = runs_none((int)(c0 < nwin ? c0 : 0));
      long_chunk<MODE, CANON>(data, st, nwin, q, c0, [&](int w, bool valid, uint32_t c) {
        runs_push(acc, w, valid && c >= mn && c <= mx);
      });
      const Runs wv = group_runs<64>(acc);
      Runs *buf = s_runs[round & 1u];
      if (lane == 0) buf[wave] = wv;
      __syncthreads();
#pragma unroll
      for (int w = 0; w < NW; ++w) all = runs_join(all, buf[w]);   // (every thread: the same sums, no second barrier)
    }
    if (tid == 0) store_span(out, i, all, mode, q.k);
  });
}

template <int MODE, bool CANON>
void spans_launch_all(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                      int64_t nS, const QIndex &q, uint32_t mn, uint32_t mx, int mode, cfrk_read_span *d_out) {
  const ClassGrids g = class_grids(nS, ctx->num_cus, SP_LONG_NT);
  hipLaunchKernelGGL((read_spans_kernel<16, MODE, CANON>), dim3(g.g16), dim3(256), 0, ctx->stream, d_data, d_start,
                     d_length, nN, nS, q, mn, mx, mode, d_out);
  hipLaunchKernelGGL((read_spans_kernel<64, MODE, CANON>), dim3(g.g64), dim3(64), 0, ctx->stream, d_data, d_start,
                     d_length, nN, nS, q, mn, mx, mode, d_out);
  hipLaunchKernelGGL((read_spans_long_kernel<MODE, CANON>), dim3(g.glong), dim3(SP_LONG_NT), 0, ctx->stream, d_data,
                     d_start, d_length, nN, nS, q, mn, mx, mode, d_out);
}

// ---- select -----------------------------------------------------------------------------------

constexpr int SEL_THREADS = 256;
constexpr int SEL_TILE = CFRK_SELECT_TILE_BYTES;
constexpr int SEL_SCAN = CFRK_SELECT_SCAN_TILES;
static_assert(CFRK_SELECT_TILE_READS == SEL_THREADS, "a tile of reads is one read per thread");
static_assert(SEL_TILE % 16 == 0 && SEL_TILE + 16 <= 65536, "a tile of data_out and its skew fit LDS");
static_assert(SEL_SCAN % 64 == 0 && SEL_SCAN <= 1024 && (int64_t)SEL_SCAN * CFRK_SELECT_TILE_READS < ((int64_t)1 << 31), "the block's read counts are 32-bit");

enum { SW_READS = 0, SW_BYTES, SW_NWORDS = 8 };       // device words of a select (uint64 each), in front of the aggregates
constexpr size_t SEL_WORDS_BYTES = 64;

struct SelIn {
  const int64_t *start; const int32_t *length; const cfrk_read_span *span; const uint8_t *keep;
  int64_t nN, nS;
  int32_t min_len;
};

// is read i kept?  src = offset in data of the first kept byte, len = kept bytes.  Every term is range-checked before
// it is used: a read that does not lie inside [0, nN) or a span that does not lie inside its read is dropped.
__device__ __forceinline__ bool sel_read(const SelIn &a, int64_t i, int64_t &src, int32_t &len) {
  if (a.keep && !a.keep[i]) return false;
  const int64_t st = a.start[i];
  const int32_t L = a.length[i];
  if (st < 0 || L < 0 || st > a.nN - (int64_t)L) return false;
  int32_t off = 0, n = L;
  if (a.span) {
    const cfrk_read_span s = a.span[i];
    off = s.offset; n = s.length;
    if (off < 0 || n < 0 || (int64_t)off + (int64_t)n > (int64_t)L) return false;
  }
  if (n < a.min_len) return false;
  src = st + off;
  len = n;
  return true;
}

__device__ __forceinline__ uint64_t sel_wave_scan_incl_u64(uint64_t x, int lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t y = (uint64_t)__shfl_up((unsigned long long)x, o);
    if (lane >= o) x += y;
  }
  return x;
}

__global__ __launch_bounds__(SEL_THREADS) void sel_reduce_kernel(SelIn a, ulonglong2 *__restrict__ agg) {
  __shared__ uint32_t sc[SEL_THREADS / 64];
  __shared__ unsigned long long sb[SEL_THREADS / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
  int64_t src = 0; int32_t len = 0;
  const bool kept = i < a.nS && sel_read(a, i, src, len);
  const uint32_t c = group_sum_u32<64>(kept ? 1u : 0u);
  const uint64_t b = group_sum_u64<64>(kept ? (uint64_t)len + 1u : 0u);
  if (lane == 0) { sc[w] = c; sb[w] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t tc = 0, tb = 0;
    for (int j = 0; j < SEL_THREADS / 64; ++j) { tc += sc[j]; tb += sb[j]; }
    agg[blockIdx.x] = make_ulonglong2(tc, tb);
  }
}

// one workgroup of SEL_SCAN threads: tile t of a block is thread t's
__global__ __launch_bounds__(SEL_SCAN) void sel_scan_kernel(const ulonglong2 *__restrict__ agg, int64_t ntiles, uint64_t *__restrict__ words,
                                                            ulonglong2 *__restrict__ pre) {
  constexpr int NW = SEL_SCAN / 64;
  __shared__ uint32_t sc[NW];
  __shared__ unsigned long long sb[NW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t base_c = 0, base_b = 0;
  for (int64_t b0 = 0; b0 < ntiles; b0 += SEL_SCAN) {
    const int64_t t = b0 + threadIdx.x;
    const ulonglong2 a = t < ntiles ? agg[t] : make_ulonglong2(0, 0);
    const uint32_t c = (uint32_t)a.x;
    const uint32_t ic = dev_wave_scan_incl(c);
    const uint64_t ib = sel_wave_scan_incl_u64(a.y, lane);
    if (lane == 63) { sc[w] = ic; sb[w] = ib; }
    __syncthreads();
    uint64_t pc = 0, pb = 0, tc = 0, tb = 0;
    for (int j = 0; j < NW; ++j) {
      if (j < w) { pc += sc[j]; pb += sb[j]; }
      tc += sc[j]; tb += sb[j];
    }
    if (t < ntiles) pre[t] = make_ulonglong2(base_c + pc + ic - c, base_b + pb + ib - a.y);
    base_c += tc; base_b += tb;
    __syncthreads();       // (sc / sb are written again by the next block)
  }
  if (threadIdx.x == 0) { words[SW_READS] = base_c; words[SW_BYTES] = base_b; }
}

__global__ __launch_bounds__(SEL_THREADS) void sel_index_kernel(SelIn a, const ulonglong2 *__restrict__ pre, int64_t *__restrict__ start_out,
                                                                int32_t *__restrict__ length_out, int64_t *__restrict__ index_out,
                                                                int64_t *__restrict__ src_off) {
  __shared__ uint32_t sc[SEL_THREADS / 64];
  __shared__ unsigned long long sb[SEL_THREADS / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
  int64_t src = 0; int32_t len = 0;
  const bool kept = i < a.nS && sel_read(a, i, src, len);
  const uint32_t c = kept ? 1u : 0u;
  const uint64_t b = kept ? (uint64_t)len + 1u : 0u;
  const uint32_t ic = dev_wave_scan_incl(c);
  const uint64_t ib = sel_wave_scan_incl_u64(b, lane);
  if (lane == 63) { sc[w] = ic; sb[w] = ib; }
  __syncthreads();
  uint64_t pc = 0, pb = 0;
  for (int j = 0; j < w; ++j) { pc += sc[j]; pb += sb[j]; }
  if (!kept) return;
  const ulonglong2 p = pre[blockIdx.x];
  const int64_t j = (int64_t)(p.x + pc + ic - c);
  start_out[j] = (int64_t)(p.y + pb + ib - b);
  length_out[j] = len;
  if (index_out) index_out[j] = i;
  src_off[j] = src;
}

// reads [j0, j1) into the tile's stage, read by read by groups of G threads.  stage byte off0 + x is byte T0 + x of data_out.
template <int G>
__device__ __forceinline__ void sel_gather(const int8_t *__restrict__ data, int64_t nN, const int64_t *__restrict__ start_out,
                                           const int32_t *__restrict__ length_out, const int64_t *__restrict__ src_off, int64_t j0,
                                           int64_t j1, int64_t T0, int64_t T1, uint8_t *stage, uint32_t off0) {
  const int grp = threadIdx.x / G, lane = threadIdx.x % G;
  for (int64_t j = j0 + grp; j < j1; j += SEL_THREADS / G) {
    const int64_t s = start_out[j], e = s + (int64_t)length_out[j];      // e: the terminator's place
    const int64_t a = s > T0 ? s : T0, b = e < T1 ? e : T1;
    if (a < b) {
      const int64_t sa = src_off[j] + (a - s);
      const int n = (int)(b - a);
      const int skew = (int)((reinterpret_cast<uintptr_t>(data) + (uintptr_t)sa) & 3u);
      const int ndw = (skew + n + 3) >> 2;
      uint8_t *dst = stage + off0 + (uint32_t)(a - T0);
      for (int d = lane; d < ndw; d += G) {
        const int64_t off = sa - skew + 4 * (int64_t)d;
        uint32_t w;
        if (off >= 0 && off + 4 <= nN) {
          w = *reinterpret_cast<const uint32_t *>(data + off);
        } else {
          w = 0;
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            const int64_t g = off + x;
            if (g >= 0 && g < nN) w |= (uint32_t)(uint8_t)data[g] << (8 * x);
          }
        }
        const int p = 4 * d - skew;
        if (p >= 0 && p + 4 <= n && ((uint32_t)(dst + p - stage) & 3u) == 0) {
          *reinterpret_cast<uint32_t *>(dst + p) = w;
        } else {
#pragma unroll
          for (int x = 0; x < 4; ++x)
            if (p + x >= 0 && p + x < n) dst[p + x] = (uint8_t)(w >> (8 * x));
        }
      }
    }
    if (lane == 0 && e >= T0 && e < T1) stage[off0 + (uint32_t)(e - T0)] = 0xFFu;
  }
}

__global__ __launch_bounds__(SEL_THREADS) void sel_copy_kernel(const int8_t *__restrict__ data, int64_t nN, const int64_t *__restrict__ start_out,
                                                               const int32_t *__restrict__ length_out, const int64_t *__restrict__ src_off,
                                                               int64_t nS_out, int64_t nN_out, int8_t *__restrict__ data_out) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[SEL_TILE + 16];
  const int64_t T0 = (int64_t)blockIdx.x * SEL_TILE;
  const int64_t T1 = T0 + SEL_TILE < nN_out ? T0 + SEL_TILE : nN_out;
  // the read that holds byte T0: the last one with start_out <= T0 (start_out[0] = 0, strictly ascending, and the reads
  // with their terminators cover data_out without gaps)
  int64_t lo = 0, hi = nS_out;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (start_out[mid] <= T0) lo = mid + 1; else hi = mid;
  }
  const int64_t j0 = lo - 1;
  // the first read that begins at or behind T1: every read takes a byte, so it is at most T1 - T0 reads on
  hi = j0 + 1 + (T1 - T0) < nS_out ? j0 + 1 + (T1 - T0) : nS_out;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (start_out[mid] < T1) lo = mid + 1; else hi = mid;
  }
  const int64_t j1 = lo, nreads = j1 - j0;
  const uint32_t off0 = (uint32_t)(reinterpret_cast<uintptr_t>(data_out + T0) & 15u);
  if (nreads * 1024 <= SEL_TILE) sel_gather<SEL_THREADS>(data, nN, start_out, length_out, src_off, j0, j1, T0, T1, stage, off0);
  else if (nreads * 256 <= SEL_TILE) sel_gather<64>(data, nN, start_out, length_out, src_off, j0, j1, T0, T1, stage, off0);
  else sel_gather<16>(data, nN, start_out, length_out, src_off, j0, j1, T0, T1, stage, off0);
  __syncthreads();
  // LDS -> data_out: whole aligned 16-byte blocks, bytes at the two ends (the neighbours' bytes share those blocks)
  int8_t *g0 = data_out + T0 - off0;
  const uint32_t end = off0 + (uint32_t)(T1 - T0);
  for (uint32_t b = threadIdx.x * 16; b < end; b += SEL_THREADS * 16) {
    if (b >= off0 && b + 16 <= end) {
      *reinterpret_cast<uint4 *>(g0 + b) = *reinterpret_cast<const uint4 *>(stage + b);
    } else {
      for (uint32_t x = b; x < b + 16; ++x)
        if (x >= off0 && x < end) g0[x] = (int8_t)stage[x];
    }
  }
}

struct SelPlan { uint64_t *words; ulonglong2 *agg, *pre; int64_t ntiles; };

int sel_plan(cfrk_ctx *ctx, int64_t nS, SelPlan *pl) {
  pl->ntiles = (nS + SEL_THREADS - 1) / SEL_THREADS;
  void *p;
  const int rc = cfrk_pool_get(ctx, BUF_SELECT, SEL_WORDS_BYTES + (size_t)pl->ntiles * 32, &p);
  if (rc) return rc;
  pl->words = (uint64_t *)p;
  pl->agg = (ulonglong2 *)((char *)p + SEL_WORDS_BYTES);
  pl->pre = pl->agg + pl->ntiles;
  return CFRK_OK;
}

}  // namespace

// One span per read against the job's index (built, synchronising, when it is not valid); the three kernels -- one per
// size class of reads -- are left enqueued.  Arguments are checked by the callers (abi.hip).  nS >= 1.
int cfrk_read_spans_launch(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                           int64_t nN, int64_t nS, uint32_t min_count, uint32_t max_count, int mode, cfrk_read_span *d_out) {
  QIndex q;
  int rc = cfrk_query_index(ctx, &q);
  if (rc) return rc;
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
#define SP_LAUNCH(MODE)                                                                                                  \
  do {                                                                                                                   \
    if (canon) spans_launch_all<MODE, true>(ctx, d_data, d_start, d_length, nN, nS, q, min_count, max_count, mode, d_out);  \
    else spans_launch_all<MODE, false>(ctx, d_data, d_start, d_length, nN, nS, q, min_count, max_count, mode, d_out);       \
  } while (0)
  if (q.k <= 12) SP_LAUNCH(0);
  else if (q.k <= 32) SP_LAUNCH(1);
  else SP_LAUNCH(2);
#undef SP_LAUNCH
  HIP_TRY(ctx, hipGetLastError());
  return CFRK_OK;
}

// reduce + scan, the totals read back (synchronises).  nS >= 1.
int cfrk_select_measure(cfrk_ctx *ctx, const int64_t *d_start, const int32_t *d_length, int64_t nN, int64_t nS,
                        const cfrk_read_span *d_span, const uint8_t *d_keep, int32_t min_len, int64_t *nN_out, int64_t *nS_out) {
  SelPlan pl;
  int rc = sel_plan(ctx, nS, &pl);
  if (rc) return rc;
  const SelIn in = {d_start, d_length, d_span, d_keep, nN, nS, min_len};
  hipLaunchKernelGGL(sel_reduce_kernel, dim3((unsigned)pl.ntiles), dim3(SEL_THREADS), 0, ctx->stream, in, pl.agg);
  hipLaunchKernelGGL(sel_scan_kernel, dim3(1), dim3(SEL_SCAN), 0, ctx->stream, pl.agg, pl.ntiles, pl.words, pl.pre);
  HIP_TRY(ctx, hipGetLastError());
  uint64_t wd[2];
  HIP_TRY(ctx, hipMemcpyAsync(wd, pl.words, sizeof wd, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *nS_out = (int64_t)wd[SW_READS];
  *nN_out = (int64_t)wd[SW_BYTES];
  return CFRK_OK;
}

// the index pass and the copy, left enqueued, after cfrk_select_measure with the same arguments.  nS_out >= 1.
int cfrk_select_emit(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                     int64_t nS, const cfrk_read_span *d_span, const uint8_t *d_keep, int32_t min_len, int8_t *d_data_out,
                     int64_t *d_start_out, int32_t *d_length_out, int64_t *d_index_out, int64_t nN_out, int64_t nS_out) {
  SelPlan pl;
  int rc = sel_plan(ctx, nS, &pl);                     // (the slot holds it already: the pointers of the measure step)
  if (rc) return rc;
  void *p_src;
  if ((rc = cfrk_pool_get(ctx, BUF_SELECT_SRC, (size_t)nS_out * 8, &p_src))) return rc;
  const SelIn in = {d_start, d_length, d_span, d_keep, nN, nS, min_len};
  hipLaunchKernelGGL(sel_index_kernel, dim3((unsigned)pl.ntiles), dim3(SEL_THREADS), 0, ctx->stream, in, pl.pre, d_start_out,
                     d_length_out, d_index_out, (int64_t *)p_src);
  const int64_t ctiles = (nN_out + SEL_TILE - 1) / SEL_TILE;
  hipLaunchKernelGGL(sel_copy_kernel, dim3((unsigned)ctiles), dim3(SEL_THREADS), 0, ctx->stream, d_data, nN, d_start_out,
                     d_length_out, (const int64_t *)p_src, nS_out, nN_out, d_data_out);
  HIP_TRY(ctx, hipGetLastError());
  return CFRK_OK;
}
