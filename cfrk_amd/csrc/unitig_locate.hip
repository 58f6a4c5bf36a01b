// unitig_locate.hip -- where the k-mers of a job lie on its unitigs: the position map (one cfrk_unitig_pos per slot of
// the lookup index), point lookups in it, and the hits of reads (maximal colinear stretches of windows) as CSR rows.
// The contract is in include/cfrk_abi.h ("Unitig positions and read hits"); DESIGN 4.21 has the reasoning.
//
// Map build (cfrk_unitig_index_build), every pass a launch of its own on the context stream:
//   1 check   one lane per unitig: length >= k, the range inside [0, nN), behind its predecessor
//   2 claim   one workgroup per tile of UP_TILE window starts of the unitig BYTES, 32 consecutive starts per thread
//             (plus k - 1 bytes of look-ahead), rolled with Roller; the unitig a window lies in comes from a binary
//             search in start[], repeated only when a start is crossed.  A window inside a unitig canonicalises,
//             finds its slot and claims pos[slot] with a compare-and-swap.  The work is balanced by bases: no lane's
//             work grows with a unitig's length.
//   3 cover   one lane per index slot: a solid key without a position is a key no unitig of the input holds
//   -- the one synchronisation: the error word --
// The claim pass reads data[] only at offsets below nN, start[] and length[] only at indices below nS, whatever they
// hold; its loops are bounded by the tile and by log2(nS).
//
// Hits (cfrk_read_hits_count / _fill): three launches per pass over the size classes of lane_group.h.  A read's window
// positions go to LDS (the slot form of the walkers of read_windows.h: the functor gets the window's SLOT and loads
// pos[slot]); then every lane walks its own stretch of windows once more in LDS.  At window w its owner sees, from
// pos(w - 1) and pos(w), whether a hit STARTS at w and whether one ENDS at w - 1.  The number of starts before w is the
// row of both events (an exclusive prefix over the lanes), so no lane has to find its partner: the start's lane writes
// unitig, position and read_off of its row, the end's lane the last window, and a pass over the rows (rh_finish_kernel)
// turns the pair into n_windows and the smaller offset.  The count pass writes per-read counts into hit_ptr, hipCUB's
// exclusive sum scans them in place, and after the one synchronisation the fill pass repeats the lookups.  Long reads
// go round by round (RH_LONG_NT chunks of LONG_CHUNK windows) with the last position and the running row carried.
#include "lane_group.h"
#include "read_windows.h"
#include "staging.h"
#include "unitig_dev.h"

#include <hipcub/hipcub.hpp>

namespace {

constexpr unsigned long long UP_NONE = ~0ull;         // cfrk_unitig_pos as one word: at << 32 | unitig
constexpr int UP_TILE = 8192;                         // window starts per workgroup and turn
constexpr int UP_PER = UP_TILE / 256;                 // ... per thread
enum { UPC_ERR = 0, UPC_MISSING, UPC_WORDS };
// error word = unitig << 8 | why, kept with an atomic minimum: the first offending unitig
enum { UPE_RANGE = 1, UPE_CODE, UPE_ABSENT, UPE_CLAIMED };

struct UPWork {
  QIndex q;
  const int8_t *data; const int64_t *start; const int32_t *length;
  int64_t nN;
  uint64_t nS;
  USolid sol;                         // min_count and the graph mask
  unsigned long long *ctr;            // UPC_*
  unsigned long long *pos;            // [slots]
};

__device__ __forceinline__ void up_fail(const UPWork &w, uint64_t j, int why) {
  atomicMin(&w.ctr[UPC_ERR], (unsigned long long)((j << 8) | (uint64_t)why));
}

// ---- 1 check ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void up_check_kernel(UPWork w) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = tid; j < w.nS; j += nthreads) {
    const int64_t s = w.start[j], len = w.length[j];
    bool bad = len < w.q.k || s < 0 || s > w.nN || len > w.nN - s;
    if (!bad && j) {                                    // (the predecessor's own range is its own lane's to refuse)
      const int64_t ps = w.start[j - 1], pl = w.length[j - 1];
      if (ps >= 0 && ps <= w.nN && pl >= 0 && pl <= w.nN - ps && s < ps + pl) bad = true;
      if (ps > s) bad = true;
    }
    if (bad) up_fail(w, j, UPE_RANGE);
  }
}

// ---- 2 claim ----------------------------------------------------------------------------------------------------
// the last unitig whose start is <= x, -1 when there is none (start[] ascending: the check pass refuses anything else)
__device__ __forceinline__ int64_t up_search(const UPWork &w, int64_t x) {
  uint64_t lo = 0, hi = w.nS;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (w.start[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return (int64_t)lo - 1;
}

template <int MODE, bool CANON, bool MASKED>
__device__ __forceinline__ void up_claim_body(const UPWork &w) {
  const int k = w.q.k;
  const int64_t nwin = w.nN - k + 1;                    // window starts whose k bytes lie below nN
  const int64_t ntiles = (nwin + UP_TILE - 1) / UP_TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t a = tile * UP_TILE + (int64_t)threadIdx.x * UP_PER;
    const int64_t b = a + UP_PER < nwin ? a + UP_PER : nwin;
    if (a >= b) continue;
    int64_t j = up_search(w, a);
    Roller<MODE == 2, CANON> R(k);
    for (int64_t p = a; p < b + k - 1; ++p) {           // p <= nwin + k - 2 = nN - 1
      R.push((int)w.data[p]);
      if (p < a + k - 1) continue;
      const int64_t ws = p - (k - 1);
      if ((uint64_t)(j + 1) < w.nS && w.start[j + 1] <= ws) j = up_search(w, ws);
      if (j < 0) continue;
      const int64_t s = w.start[j], len = w.length[j];
      if (s < 0 || s > ws || len < k || ws - s > len - k) continue;     // between two unitigs
      if (!R.valid()) { up_fail(w, (uint64_t)j, UPE_CODE); continue; }
      const auto key = R.key();
      const uint64_t slot = q_slot_of<MODE>(w.q, (uint64_t)key, (uint64_t)(key >> (MODE == 2 ? 64 : 0)));
      if (!u_solid<MODE, MASKED>(w.q, w.sol, slot)) { up_fail(w, (uint64_t)j, UPE_ABSENT); continue; }
      const unsigned long long at = ((unsigned long long)(ws - s) << 1) | (R.minus() ? 1ull : 0ull);
      const unsigned long long old = atomicCAS(&w.pos[slot], UP_NONE, (at << 32) | (unsigned long long)j);
      // (named is the later of the two claimants: the one that comes second in the list)
      if (old != UP_NONE) up_fail(w, max((uint64_t)j, (uint64_t)(old & 0xFFFFFFFFull)), UPE_CLAIMED);
    }
  }
}
U_SOLID_KERNELS(up_claim, (UPWork w), (w))

// ---- 3 cover ----------------------------------------------------------------------------------------------------
template <int MODE, bool CANON, bool MASKED>
__device__ __forceinline__ void up_cover_body(const UPWork &w) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t M = q_nslots<MODE>(w.q);
  for (uint64_t s = tid; s < M; s += nthreads) {
    if (u_solid<MODE, MASKED>(w.q, w.sol, s) && w.pos[s] == UP_NONE) w.ctr[UPC_MISSING] = 1;      // (a masked key is not one)
  }
}
U_SOLID_KERNELS(up_cover, (UPWork w), (w))

// ---- locate -----------------------------------------------------------------------------------------------------
// the position of oriented k-mer z (in range) exactly as given
template <int MODE, bool CANON>
__device__ __forceinline__ unsigned long long up_locate(const QIndex &q, const unsigned long long *__restrict__ pos, u128 z) {
  int o; bool pal;
  const uint64_t slot = u_node<MODE, CANON>(q, z, o, pal);
  if (slot == Q_NO_SLOT) return UP_NONE;
  const unsigned long long v = pos[slot];
  return v == UP_NONE ? v : v ^ ((unsigned long long)o << 32);
}

template <int MODE, bool CANON>
__global__ __launch_bounds__(256) void up_locate_kernel(QIndex q, const unsigned long long *__restrict__ pos,
                                                        const uint64_t *__restrict__ keys_lo, const uint64_t *__restrict__ keys_hi,
                                                        int64_t n, cfrk_unitig_pos *__restrict__ out) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  const int k = q.k;
  for (int64_t i = tid; i < n; i += nthreads) {
    const uint64_t lo = keys_lo[i], hi = keys_hi ? keys_hi[i] : 0;
    bool in;                                            // no bits at or above 2k
    if (MODE < 2) in = hi == 0 && (k >= 32 || (lo >> (2 * k)) == 0);
    else in = k >= 64 || (hi >> (2 * k - 64)) == 0;
    const unsigned long long v = in ? up_locate<MODE, CANON>(q, pos, u_make(lo, hi)) : UP_NONE;
    out[i].unitig = (uint32_t)v;                        // (two words: out need not lie on an 8-byte boundary)
    out[i].at = (uint32_t)(v >> 32);
  }
}

// ---- hits -------------------------------------------------------------------------------------------------------
constexpr int RH_LONG_NT = 128;                       // threads of the long-read kernel: a round's positions are 32 KiB of LDS

struct RHWork {
  QIndex q;
  const unsigned long long *pos;      // the map
  const int8_t *data; const int64_t *start; const int32_t *length;
  int64_t nN, nS;
  int64_t *hit_ptr;                   // [nS + 1]: counts (count pass), then their exclusive sums
  cfrk_read_hit *hits;
};

// the position of a window from its slot and the orientation the read spells it in
__device__ __forceinline__ unsigned long long rh_pos(const RHWork &w, bool valid, uint64_t slot, bool minus) {
  if (!valid || slot == Q_NO_SLOT) return UP_NONE;
  const unsigned long long v = w.pos[slot];
  return v == UP_NONE ? v : v ^ ((unsigned long long)(minus ? 1 : 0) << 32);
}

// a, then b one window later: both located, same unitig, same strand, one step along the strand (no wrap-around)
__device__ __forceinline__ bool rh_colinear(unsigned long long a, unsigned long long b) {
  if (a == UP_NONE || b == UP_NONE) return false;
  if (((a ^ b) & 0x1FFFFFFFFull) != 0) return false;    // unitig and minus
  const uint32_t pa = (uint32_t)(a >> 33), pb = (uint32_t)(b >> 33);
  return ((a >> 32) & 1) ? (pa != 0 && pb == pa - 1) : pb == pa + 1;
}

// Windows [t0, t1) of a read whose positions lie in s_pos[w - w0]; prev = pos(t0 - 1) (UP_NONE at the read's
// beginning).  Returns the hits that start in the stretch.  FILL: `row` is the number of starts before t0; the events
// go to the read's rows [base, base + room).  last: the stretch ends the read, so a hit open at its end ends there.
template <bool FILL>
__device__ __forceinline__ int rh_events(const unsigned long long *s_pos, int64_t w0, int64_t t0, int64_t t1,
                                         unsigned long long prev, bool last, int64_t row, cfrk_read_hit *__restrict__ hits,
                                         int64_t base, int64_t room) {
  int n = 0;
  for (int64_t w = t0; w < t1; ++w) {
    const unsigned long long cur = s_pos[w - w0];
    const bool col = rh_colinear(prev, cur);
    if (FILL && prev != UP_NONE && !col) {              // a hit ends at w - 1: the row of the latest start
      const int64_t r = row + n - 1;
      if (r >= 0 && r < room) hits[base + r].n_windows = (uint32_t)(w - 1);
    }
    if (cur != UP_NONE && !col) {
      if (FILL) {
        const int64_t r = row + n;
        if (r < room) {
          hits[base + r].unitig = (uint32_t)cur;
          hits[base + r].unitig_at = (uint32_t)(cur >> 32);
          hits[base + r].read_off = (uint32_t)w;
        }
      }
      ++n;
    }
    prev = cur;
  }
  if (FILL && last && t0 < t1 && prev != UP_NONE) {
    const int64_t r = row + n - 1;
    if (r >= 0 && r < room) hits[base + r].n_windows = (uint32_t)(t1 - 1);
  }
  return n;
}

// read i (nwin >= 1 windows from byte st on, inside [0, nN)) by the G lanes of a group
template <int G, int MODE, bool CANON, bool FILL>
__device__ __forceinline__ void rh_read(const RHWork &w, int64_t i, int64_t st, int nwin, int32_t *stage_dw,
                                        unsigned long long *s_pos, int lane) {
  int t0, t1;
  staged_windows<G, MODE, CANON, WinSlot>(w.data, w.nN, st, nwin, w.q, stage_dw, lane, t0, t1,
                                          [&](int win, bool valid, uint64_t slot, bool minus) {
                                            s_pos[win] = rh_pos(w, valid, slot, minus);
                                          });
  wave_sync();
  const unsigned long long prev = (t0 < t1 && t0 > 0) ? s_pos[t0 - 1] : UP_NONE;
  const int c = rh_events<false>(s_pos, 0, t0, t1, prev, false, 0, nullptr, 0, 0);
  int incl = c;
  for (int o = 1; o < G; o <<= 1) { const int t = __shfl_up(incl, o, G); if (lane >= o) incl += t; }
  if (!FILL) {
    if (lane == G - 1) w.hit_ptr[i] = incl;
  } else {
    const int64_t base = w.hit_ptr[i], room = w.hit_ptr[i + 1] - base;
    rh_events<true>(s_pos, 0, t0, t1, prev, t1 == nwin, incl - c, w.hits, base, room);
  }
  wave_sync();     // the group's LDS is reused by its next read
}

template <int G, int MODE, bool CANON, bool FILL>
__global__ __launch_bounds__(G == 16 ? 256 : 64) void read_hits_kernel(RHWork w) {
  constexpr int RPB = (G == 16 ? 256 : 64) / G;
  constexpr int CAP = (G == 16) ? READ_CAP16 : READ_CAP64;
  __shared__ int32_t s_stage[RPB][(CAP + READ_STAGE_SLACK) / 4];
  __shared__ unsigned long long s_pos[RPB][CAP];
  const int grp = G == 16 ? threadIdx.x / G : 0, lane = threadIdx.x % G;
  class_reads<G>(
      w.start, w.length, w.nN, w.nS, w.q.k,
      [&](int64_t i, int64_t st, int nwin) { rh_read<G, MODE, CANON, FILL>(w, i, st, nwin, s_stage[grp], s_pos[grp], lane); },
      [&](int64_t i) { if (!FILL && lane == 0) w.hit_ptr[i] = 0; });
}

// long reads: rounds of RH_LONG_NT chunks, chunk t of a round by thread t; the last position of a round and the hits
// begun so far are carried into the next
template <int MODE, bool CANON, bool FILL>
__global__ __launch_bounds__(RH_LONG_NT) void read_hits_long_kernel(RHWork w) {
  constexpr int NW = RH_LONG_NT / 64;
  constexpr int ROUND = RH_LONG_NT * LONG_CHUNK;
  __shared__ unsigned long long s_pos[ROUND];
  __shared__ int s_wave[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // (every round ends on a barrier, and a long read has at least one round)
  long_reads<RH_LONG_NT, true>(w.start, w.length, w.nN, w.nS, w.q.k, [&](int64_t i, int64_t st, int nwin) {
    unsigned long long carry = UP_NONE;
    int64_t rows = 0, base = 0, room = 0;
    if (FILL) { base = w.hit_ptr[i]; room = w.hit_ptr[i + 1] - base; }
    for (int64_t r0 = 0; r0 < nwin; r0 += ROUND) {
      const int64_t c0 = r0 + (int64_t)tid * LONG_CHUNK;
      long_chunk<MODE, CANON, WinSlot>(w.data, st, nwin, w.q, c0, [&](int win, bool valid, uint64_t slot, bool minus) {
        s_pos[win - r0] = rh_pos(w, valid, slot, minus);
      });
      __syncthreads();
      const int64_t c1 = c0 + LONG_CHUNK < nwin ? c0 + LONG_CHUNK : (int64_t)nwin;      // (c0 >= nwin: no window)
      const unsigned long long prev = c0 > r0 ? (c0 <= nwin ? s_pos[c0 - r0 - 1] : UP_NONE) : carry;
      const int c = rh_events<false>(s_pos, r0, c0, c1, prev, false, 0, nullptr, 0, 0);
      const int incl = (int)dev_wave_scan_incl((uint32_t)c);
      if (lane == 63) s_wave[wave] = incl;
      __syncthreads();
      int before = incl - c, total = 0;
#pragma unroll
      for (int v = 0; v < NW; ++v) { if (v < wave) before += s_wave[v]; total += s_wave[v]; }
      if (FILL) rh_events<true>(s_pos, r0, c0, c1, prev, c1 == nwin, rows + before, w.hits, base, room);
      const int64_t r1 = r0 + ROUND < nwin ? r0 + ROUND : (int64_t)nwin;
      carry = s_pos[r1 - r0 - 1];
      rows += total;
      __syncthreads();
    }
    if (!FILL && tid == 0) w.hit_ptr[i] = rows;
  });
}

// the rows as the fill pass left them (unitig_at = the first window's position, n_windows = the last window) into
// their final form: n_windows, and the smaller of the two end positions
__global__ __launch_bounds__(256) void rh_finish_kernel(cfrk_read_hit *__restrict__ hits, int64_t n) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = tid; i < n; i += nthreads) {
    const uint32_t a = hits[i].read_off, b = hits[i].n_windows, at = hits[i].unitig_at;
    const uint32_t m = b - a + 1;
    hits[i].n_windows = m;
    if (at & 1u) hits[i].unitig_at = (((at >> 1) - (m - 1)) << 1) | 1u;
  }
}

template <int MODE, bool CANON, bool FILL>
void rh_launch_all(cfrk_ctx *ctx, const RHWork &w) {
  const ClassGrids g = class_grids(w.nS, ctx->num_cus, RH_LONG_NT);
  hipLaunchKernelGGL((read_hits_kernel<16, MODE, CANON, FILL>), dim3(g.g16), dim3(256), 0, ctx->stream, w);
  hipLaunchKernelGGL((read_hits_kernel<64, MODE, CANON, FILL>), dim3(g.g64), dim3(64), 0, ctx->stream, w);
  hipLaunchKernelGGL((read_hits_long_kernel<MODE, CANON, FILL>), dim3(g.glong), dim3(RH_LONG_NT), 0, ctx->stream, w);
}

template <bool FILL>
void rh_launch(cfrk_ctx *ctx, const RHWork &w, bool canon) {
  const int mode = w.q.k <= 12 ? 0 : w.q.k <= 32 ? 1 : 2;
  if (mode == 0) { if (canon) rh_launch_all<0, true, FILL>(ctx, w); else rh_launch_all<0, false, FILL>(ctx, w); }
  else if (mode == 1) { if (canon) rh_launch_all<1, true, FILL>(ctx, w); else rh_launch_all<1, false, FILL>(ctx, w); }
  else { if (canon) rh_launch_all<2, true, FILL>(ctx, w); else rh_launch_all<2, false, FILL>(ctx, w); }
}

// the index and the map of the job, CFRK_ERR_STATE when the map is not the index's
int up_map(cfrk_ctx *ctx, const char *what, QIndex *q, const unsigned long long **pos) {
  if (!ctx->q_valid || ctx->upos_epoch == 0 || ctx->upos_epoch != ctx->q_epoch || !ctx->pool[BUF_UNITIG_POS].p)
    return cfrk_fail(ctx, CFRK_ERR_STATE, "%s without a position map: cfrk_global_unitig_index comes first, and again after the result changed", what);
  if (const int rc = cfrk_query_index(ctx, q)) return rc;
  *pos = carve_at<unsigned long long>(ctx->pool[BUF_UNITIG_POS].p, 256);
  return CFRK_OK;
}

}  // namespace

int cfrk_unitig_index_build(cfrk_ctx *ctx, uint32_t min_count, const int8_t *d_data, const int64_t *d_start,
                            const int32_t *d_length, int64_t nN, int64_t nS) {
  ctx->upos_epoch = 0;
  UPWork w;
  int rc = cfrk_query_index(ctx, &w.q);
  if (rc) return rc;
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  const int mode = w.q.k <= 12 ? 0 : w.q.k <= 32 ? 1 : 2;
  const uint64_t M = w.q.k <= 12 ? 1ull << (2 * w.q.k) : w.q.mask + 1;
  if (M > (1ull << 31)) return cfrk_fail(ctx, CFRK_ERR_ARG, "an index of %llu slots is too large for the position map", (unsigned long long)M);
  void *base;
  if ((rc = cfrk_pool_get(ctx, BUF_UNITIG_POS, 256 + M * 8, &base))) return rc;
  w.ctr = carve_at<unsigned long long>(base, 0);
  w.pos = carve_at<unsigned long long>(base, 256);
  w.data = d_data; w.start = d_start; w.length = d_length; w.nN = nN; w.nS = (uint64_t)nS;
  w.sol = u_solid_rule(ctx, min_count);
  HIP_TRY(ctx, hipMemsetAsync(w.ctr, 0xFF, 8, ctx->stream));                  // UPC_ERR: no unitig yet
  HIP_TRY(ctx, hipMemsetAsync(w.ctr + UPC_MISSING, 0, 8, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w.pos, 0xFF, M * 8, ctx->stream));
  if (nS > 0) {
    hipLaunchKernelGGL(up_check_kernel, dim3(u_grid(ctx, w.nS)), dim3(256), 0, ctx->stream, w);
    if (nN >= w.q.k) {
      const int64_t ntiles = (nN - w.q.k + 1 + UP_TILE - 1) / UP_TILE;
      const int grid = (int)std::min<int64_t>(ntiles, (int64_t)ctx->num_cus * 16);
      U_DISPATCH_SOLID(up_claim, w.sol, grid, w);
    }
  }
  U_DISPATCH_SOLID(up_cover, w.sol, u_grid(ctx, M), w);
  HIP_TRY(ctx, hipGetLastError());
  unsigned long long h[UPC_WORDS];
  HIP_TRY(ctx, hipMemcpyAsync(h, w.ctr, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (h[UPC_ERR] != UP_NONE) {
    const unsigned long long j = h[UPC_ERR] >> 8;
    const int why = (int)(h[UPC_ERR] & 255);
    const char *what = why == UPE_RANGE    ? "is shorter than k, does not lie inside the data or does not lie behind its predecessor"
                       : why == UPE_CODE   ? "has an invalid code"
                       : why == UPE_ABSENT ? "has a k-mer that is not a solid key of this job at this min_count"
                                           : "has a k-mer that an earlier k-mer of the input has as well";
    return cfrk_fail(ctx, CFRK_ERR_LAYOUT, "unitig %llu %s: not the unitigs of this job at this min_count", j, what);
  }
  if (h[UPC_MISSING])
    return cfrk_fail(ctx, CFRK_ERR_LAYOUT, "a solid key of this job lies in none of the unitigs: not the unitigs of this job at this min_count");
  ctx->upos_epoch = ctx->q_epoch;
  return CFRK_OK;
}

int cfrk_unitig_locate_launch(cfrk_ctx *ctx, const uint64_t *d_lo, const uint64_t *d_hi, int64_t n, cfrk_unitig_pos *d_out) {
  QIndex q;
  const unsigned long long *pos;
  int rc = up_map(ctx, "locate", &q, &pos);
  if (rc || n == 0) return rc;
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  const int mode = q.k <= 12 ? 0 : q.k <= 32 ? 1 : 2;
  U_DISPATCH(up_locate_kernel, u_grid(ctx, (uint64_t)n), q, pos, d_lo, d_hi, n, d_out);
  HIP_TRY(ctx, hipGetLastError());
  return CFRK_OK;
}

int cfrk_read_hits_count(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                         int64_t nS, int64_t *d_hit_ptr, int64_t *n_hits) {
  RHWork w;
  int rc = up_map(ctx, "read hits", &w.q, &w.pos);
  if (rc) return rc;
  size_t scan_tmp = 0;
  HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_tmp, (int64_t *)nullptr, (size_t)(nS + 1), ctx->stream));
  void *tmp;
  if ((rc = cfrk_pool_get(ctx, BUF_READ_HITS, scan_tmp + 8, &tmp))) return rc;
  w.data = d_data; w.start = d_start; w.length = d_length; w.nN = nN; w.nS = nS;
  w.hit_ptr = d_hit_ptr; w.hits = nullptr;
  HIP_TRY(ctx, hipMemsetAsync(d_hit_ptr + nS, 0, 8, ctx->stream));
  if (nS > 0) rh_launch<false>(ctx, w, (ctx->g_flags & CFRK_CANONICAL) != 0);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(tmp, scan_tmp, d_hit_ptr, (size_t)(nS + 1), ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(n_hits, d_hit_ptr + nS, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CFRK_OK;
}

int cfrk_read_hits_fill(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                        int64_t nS, int64_t *d_hit_ptr, cfrk_read_hit *d_hits, int64_t n_hits) {
  RHWork w;
  int rc = up_map(ctx, "read hits", &w.q, &w.pos);
  if (rc) return rc;
  w.data = d_data; w.start = d_start; w.length = d_length; w.nN = nN; w.nS = nS;
  w.hit_ptr = d_hit_ptr; w.hits = d_hits;
  rh_launch<true>(ctx, w, (ctx->g_flags & CFRK_CANONICAL) != 0);
  hipLaunchKernelGGL(rh_finish_kernel, dim3(u_grid(ctx, (uint64_t)n_hits)), dim3(256), 0, ctx->stream, d_hits, n_hits);
  HIP_TRY(ctx, hipGetLastError());
  return CFRK_OK;
}
