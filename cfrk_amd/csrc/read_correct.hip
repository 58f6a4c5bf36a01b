// read_correct.hip -- spectral correction of substitution errors against a finished global result
// (cfrk_global_correct_reads): the rule of include/cfrk_abi.h.  data_out is a copy of data (one device-to-device copy,
// enqueued by the caller in abi.hip) into which these kernels store single bytes, one per corrected weak run; every run
// is judged against the ORIGINAL read in `data`, which the kernels only read, so neither the order of the runs nor the
// order of the reads matters.
//
// The three launches by size class and the walk over a read's windows are lane_group.h's and read_windows.h's.  What
// is this file's:
//   classes     every window of a read is weak (valid, count < min_count), invalid, or solid (neither): one bit per
//               window in two words of its lane (a lane's stretch is at most 32 windows).
//   early exit  a read without a weak window ends behind the group sum over "my word has a weak bit": what a span
//               costs, nothing in LDS but the staged read.
//   bitmaps     otherwise the lanes OR their words into two bitmaps of the group in LDS (a stretch lies in one dword or
//               two; neighbouring stretches share dwords).  A thread of the long path owns a whole dword
//               (LONG_CHUNK == 32).
//   runs        every lane looks for the run starts of its own stretch, reads at most k + 1 bits ahead for the run's
//               end and classifies it by the table of the rule: left alone, or a candidate {a, n, p}.
//   verdicts    candidates x 3 bases are dealt round-robin to the lanes; an item rolls the windows a .. b of the read
//               with c[p] replaced and looks them up CR_B at a time, until one is below min_count.  A base that passes sets its
//               bit in the candidate's word (LDS OR); one lane per candidate stores the byte when exactly one bit is set.
// The long path walks a read in rounds of CR_LONG_NT * LONG_CHUNK windows.  The bitmaps are a ring of four rounds; the
// run starts of a round are handled once the k + 1 windows behind them are known, that is up to k + 1 windows before
// the round's end (the rest with the next round), each by the thread that finds it, with the read's bases taken from
// device memory.  One barrier per round: the dwords a round writes are three rounds away from those a late thread
// still reads.
// Temporary memory: none outside LDS.  No workgroup waits for another; no scratch.
#include "common.h"
#include "lane_group.h"
#include "query_dev.h"
#include "read_windows.h"

namespace {

constexpr int CR_LONG_NT = 256;
constexpr int CR_ROUND = CR_LONG_NT * LONG_CHUNK;      // windows of a round of the long path
constexpr int CR_RING_DW = 4 * CR_ROUND / 32;          // dwords of a bitmap of the long path's ring
static_assert(LONG_CHUNK == 32, "a thread of the long path owns one dword of each bitmap");
static_assert((CR_RING_DW & (CR_RING_DW - 1)) == 0 && CR_ROUND > 2 * 66, "the ring wraps by a mask and holds k + 2 windows of look-back");

// a candidate in LDS: a | n << 12 | tail << 19, and from bit 24 on the bases that passed
constexpr int CR_PASS_SHIFT = 24;
static_assert(READ_CAP64 + 64 <= (1 << 12), "a window index takes 12 bits of a candidate");
__device__ __forceinline__ uint32_t cand_pack(int a, int n, bool tail) { return (uint32_t)a | ((uint32_t)n << 12) | (tail ? 1u << 19 : 0u); }

// What becomes of the weak run that begins at window a, by the table of the rule: false = left alone; true = attempted,
// n windows with the position p in all of them.  weak(w) / invalid(w) answer for the windows a - 1 .. a + k + 1 that
// exist (0 <= w < nwin).
template <class Weak, class Invalid>
__device__ __forceinline__ bool run_attempted(int a, int nwin, int k, Weak weak, Invalid invalid, int &n, int &p) {
  n = 1;
  while (n <= k && a + n < nwin && weak(a + n)) ++n;   // (n == k + 1: longer than k, however long)
  if (n > k) return false;
  const int e = a + n;                                  // the window behind the run
  const bool left_none = a == 0, right_none = e == nwin;
  if (left_none && right_none) return false;
  if ((!left_none && invalid(a - 1)) || (!right_none && invalid(e))) return false;
  if (!left_none && !right_none && n != k) return false;
  p = right_none ? a + k - 1 : e - 1;
  return true;
}

// does base x at position p make every window a .. a + n - 1 solid?  code(pos) is the read's base at pos.  The windows
// are looked up CR_B at a time, their first-slot loads issued together as staged_windows does; the answer falls at the
// first window below mn (a wrong base usually fails in its first batch).
constexpr int CR_B = 4;
template <int MODE, bool CANON, class Code>
__device__ __forceinline__ bool base_passes(const QIndex &q, uint32_t mn, int a, int n, int p, int x, Code code) {
  constexpr bool TWO = MODE == 2;
  typedef typename RsKey<TWO>::type T;
  const int k = q.k;
  const uint4 *slots = static_cast<const uint4 *>(q.p);
  const uint32_t *dense = static_cast<const uint32_t *>(q.p);
  Roller<TWO, CANON> R(k);
  for (int pos = a; pos < a + k - 1; ++pos) R.push(pos == p ? x : code(pos));
  for (int w0 = a; w0 < a + n; w0 += CR_B) {
    T key[CR_B];
    uint4 v[CR_B], v2[CR_B];
    uint32_t d[CR_B];
#pragma unroll
    for (int u = 0; u < CR_B; ++u) {
      const bool in = w0 + u < a + n;
      const int pos = w0 + u + k - 1;
      if (in) R.push(pos == p ? x : code(pos));
      key[u] = R.key();
      if (MODE == 0) {
        d[u] = in ? dense[(uint64_t)key[u]] : 0u;
      } else if (MODE == 1) {
        v[u] = in ? slots[q_slot1((uint64_t)key[u], q.shift)] : make_uint4(0, 0, 0, 0);
      } else {
        const uint64_t h = q_slot2((uint64_t)key[u], (uint64_t)(key[u] >> (TWO ? 64 : 0)), q.shift);
        v[u] = in ? slots[2 * h] : make_uint4(0, 0, 0, 0);
        v2[u] = in ? slots[2 * h + 1] : make_uint4(0, 0, 0, 0);
      }
    }
#pragma unroll
    for (int u = 0; u < CR_B; ++u) {
      if (w0 + u >= a + n) break;
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
      if (r < mn) return false;
    }
  }
  return true;
}

__device__ __forceinline__ void store_fix(cfrk_read_fix *__restrict__ fix, int64_t i, uint32_t fixed, uint32_t left) {
  if (!fix) return;
  cfrk_read_fix r;
  r.fixed = fixed; r.left = left;
  fix[i] = r;
}

// read i (nwin >= 1 windows from byte st on, inside [0, nN)) by the G lanes of a group.  s_wk / s_iv: the group's
// bitmaps (CAP / 32 dwords each), s_cand: its CAP / 2 candidates, s_nc: their number.
template <int G, int MODE, bool CANON>
__device__ __forceinline__ void correct_read(const int8_t *__restrict__ data, int64_t nN, int64_t i, int64_t st, int nwin,
                                             const QIndex &q, uint32_t mn, int32_t *stage_dw, uint32_t *s_wk, uint32_t *s_iv,
                                             uint32_t *s_cand, uint32_t *s_nc, int lane, int8_t *__restrict__ data_out,
                                             cfrk_read_fix *__restrict__ fix) {
  static_assert((G == 16 ? READ_CAP16 : READ_CAP64) / G <= 32, "a lane's stretch of windows fits the bits of a word");
  const int k = q.k;
  // bit j: window t0 + j of the lane's stretch is weak, bit 32 + j: it is invalid.  (One word and a selected shift: as two
  // words that a branch chooses between, the compiler puts the pair into scratch and indexes it.)
  uint64_t cls = 0;
  int t0, t1;
  staged_windows<G, MODE, CANON>(data, nN, st, nwin, q, stage_dw, lane, t0, t1, [&](int w, bool valid, uint32_t c) {
    cls |= (uint64_t)(!valid || c < mn ? 1u : 0u) << ((valid ? 0 : 32) + (w - t0));
  });
  const uint32_t wk = (uint32_t)cls, iv = (uint32_t)(cls >> 32);
  if (group_sum<G>(wk != 0 ? 1 : 0) == 0) {             // the common case: no LDS beyond the staging
    if (lane == 0) store_fix(fix, i, 0, 0);
    wave_sync();   // the group's LDS is reused by its next read
    return;
  }
  // the lanes' words into the group's bitmaps: a stretch lies in one dword or two
  for (int d = lane; d < (nwin + 31) >> 5; d += G) { s_wk[d] = 0; s_iv[d] = 0; }
  if (lane == 0) *s_nc = 0;
  wave_sync();
  if (wk | iv) {
    const int sh = t0 & 31, d = t0 >> 5;
    if (wk << sh) atomicOr(&s_wk[d], wk << sh);
    if (iv << sh) atomicOr(&s_iv[d], iv << sh);
    if (sh) {
      if (wk >> (32 - sh)) atomicOr(&s_wk[d + 1], wk >> (32 - sh));
      if (iv >> (32 - sh)) atomicOr(&s_iv[d + 1], iv >> (32 - sh));
    }
  }
  wave_sync();
  const int skew = (int)((reinterpret_cast<uintptr_t>(data) + (uintptr_t)st) & 3u);
  const int8_t *stage = reinterpret_cast<const int8_t *>(stage_dw) + skew;
  auto weak = [&](int w) { return ((s_wk[w >> 5] >> (w & 31)) & 1u) != 0; };
  auto invalid = [&](int w) { return ((s_iv[w >> 5] >> (w & 31)) & 1u) != 0; };
  uint32_t fixed = 0, left = 0;
  if (wk) {
    for (int a = t0; a < t1; ++a) {
      if (!weak(a) || (a > 0 && weak(a - 1))) continue;
      int n, p;
      if (run_attempted(a, nwin, k, weak, invalid, n, p)) s_cand[atomicAdd(s_nc, 1u)] = cand_pack(a, n, p != a + n - 1);
      else ++left;
    }
  }
  wave_sync();
  const int nc = (int)*s_nc;
  for (int it = lane; it < 3 * nc; it += G) {
    const int c = it / 3;
    const uint32_t cw = s_cand[c];
    const int a = (int)(cw & 0xFFFu), n = (int)((cw >> 12) & 0x7Fu);
    const int p = ((cw >> 19) & 1u) ? a + k - 1 : a + n - 1;
    const int x = ((int)stage[p] + 1 + it % 3) & 3;
    if (base_passes<MODE, CANON>(q, mn, a, n, p, x, [&](int pos) { return (int)stage[pos]; }))
      atomicOr(&s_cand[c], 1u << (CR_PASS_SHIFT + x));
  }
  wave_sync();
  for (int c = lane; c < nc; c += G) {
    const uint32_t cw = s_cand[c];
    const uint32_t pass = cw >> CR_PASS_SHIFT;
    if (__popc(pass) == 1) {
      const int a = (int)(cw & 0xFFFu), n = (int)((cw >> 12) & 0x7Fu);
      const int p = ((cw >> 19) & 1u) ? a + k - 1 : a + n - 1;
      data_out[st + p] = (int8_t)(__ffs((int)pass) - 1);
      ++fixed;
    } else {
      ++left;
    }
  }
  fixed = group_sum_u32<G>(fixed);
  left = group_sum_u32<G>(left);
  if (lane == 0) store_fix(fix, i, fixed, left);
  wave_sync();     // the group's LDS is reused by its next read
}

template <int G, int MODE, bool CANON>
__global__ __launch_bounds__(G == 16 ? 256 : 64) void read_correct_kernel(
    const int8_t *__restrict__ data, const int64_t *__restrict__ start, const int32_t *__restrict__ length, int64_t nN,
    int64_t nS, QIndex q, uint32_t mn, int8_t *__restrict__ data_out, cfrk_read_fix *__restrict__ fix) {
  constexpr int RPB = (G == 16 ? 256 : 64) / G;
  constexpr int CAP = (G == 16) ? READ_CAP16 : READ_CAP64;
  __shared__ int32_t s_stage[RPB][(CAP + READ_STAGE_SLACK) / 4];
  __shared__ uint32_t s_wk[RPB][CAP / 32], s_iv[RPB][CAP / 32];
  __shared__ uint32_t s_cand[RPB][CAP / 2];
  __shared__ uint32_t s_nc[RPB];
  const int grp = G == 16 ? threadIdx.x / G : 0, lane = threadIdx.x % G;
  class_reads<G>(
      start, length, nN, nS, q.k,
      [&](int64_t i, int64_t st, int nwin) {
        correct_read<G, MODE, CANON>(data, nN, i, st, nwin, q, mn, s_stage[grp], s_wk[grp], s_iv[grp], s_cand[grp],
                                     &s_nc[grp], lane, data_out, fix);
      },
      [&](int64_t i) { if (lane == 0) store_fix(fix, i, 0, 0); });
}

// long reads
template <int MODE, bool CANON>
__global__ __launch_bounds__(CR_LONG_NT) void read_correct_long_kernel(
    const int8_t *__restrict__ data, const int64_t *__restrict__ start, const int32_t *__restrict__ length, int64_t nN,
    int64_t nS, QIndex q, uint32_t mn, int8_t *__restrict__ data_out, cfrk_read_fix *__restrict__ fix) {
  constexpr int NW = CR_LONG_NT / 64;
  __shared__ uint32_t s_wk[CR_RING_DW], s_iv[CR_RING_DW];
  __shared__ uint32_t s_sum[NW][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = q.k;
  auto weak = [&](int w) { return ((s_wk[(w >> 5) & (CR_RING_DW - 1)] >> (w & 31)) & 1u) != 0; };
  auto invalid = [&](int w) { return ((s_iv[(w >> 5) & (CR_RING_DW - 1)] >> (w & 31)) & 1u) != 0; };
  // (the body ends on a barrier: the ring and the sums are written again by the next read)
  long_reads<CR_LONG_NT, true>(start, length, nN, nS, k, [&](int64_t i, int64_t st, int nwin) {
    uint32_t fixed = 0, left = 0;
    int done = 0;                                       // the run starts below it are handled
    for (int64_t r0 = 0; r0 < nwin; r0 += CR_ROUND) {
      const int64_t c0 = r0 + (int64_t)tid * LONG_CHUNK;
      uint32_t wk = 0, iv = 0;
      long_chunk<MODE, CANON>(data, st, nwin, q, c0, [&](int w, bool valid, uint32_t c) {
        const uint32_t bit = 1u << (w & 31);                   // (selects, not branches: two words the compiler keeps in registers)
        iv |= valid ? 0u : bit;
        wk |= valid && c < mn ? bit : 0u;
      });
      const int slot = (int)((c0 >> 5) & (CR_RING_DW - 1));
      s_wk[slot] = wk;
      s_iv[slot] = iv;
      __syncthreads();
      const int64_t e = r0 + CR_ROUND < nwin ? r0 + CR_ROUND : (int64_t)nwin;   // the windows below it are known
      const int lim = e == nwin ? nwin : (int)e - (k + 1);
      for (int a = done + tid; a < lim; a += CR_LONG_NT) {
        if (!weak(a) || (a > 0 && weak(a - 1))) continue;
        int n, p;
        uint32_t pass = 0;
        if (run_attempted(a, nwin, k, weak, invalid, n, p)) {
          const int orig = (int)data[st + p];
          for (int j = 1; j <= 3; ++j) {
            const int x = (orig + j) & 3;
            if (base_passes<MODE, CANON>(q, mn, a, n, p, x, [&](int pos) { return (int)data[st + pos]; })) pass |= 1u << x;
          }
        }
        const uint32_t ok = __popc(pass) == 1 ? 1u : 0u;      // (sums, not branches: two counters the compiler keeps in registers)
        if (ok) data_out[st + p] = (int8_t)(__ffs((int)pass) - 1);
        fixed += ok;
        left += 1u - ok;
      }
      done = lim;
    }
    fixed = group_sum_u32<64>(fixed);
    left = group_sum_u32<64>(left);
    if (lane == 0) { s_sum[wave][0] = fixed; s_sum[wave][1] = left; }
    __syncthreads();
    if (tid == 0) {
      uint32_t f = 0, l = 0;
      for (int w = 0; w < NW; ++w) { f += s_sum[w][0]; l += s_sum[w][1]; }
      store_fix(fix, i, f, l);
    }
    __syncthreads();
  });
}

template <int MODE, bool CANON>
void correct_launch_all(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                        int64_t nS, const QIndex &q, uint32_t mn, int8_t *d_data_out, cfrk_read_fix *d_fix) {
  const ClassGrids g = class_grids(nS, ctx->num_cus, CR_LONG_NT);
  hipLaunchKernelGGL((read_correct_kernel<16, MODE, CANON>), dim3(g.g16), dim3(256), 0, ctx->stream, d_data, d_start,
                     d_length, nN, nS, q, mn, d_data_out, d_fix);
  hipLaunchKernelGGL((read_correct_kernel<64, MODE, CANON>), dim3(g.g64), dim3(64), 0, ctx->stream, d_data, d_start,
                     d_length, nN, nS, q, mn, d_data_out, d_fix);
  hipLaunchKernelGGL((read_correct_long_kernel<MODE, CANON>), dim3(g.glong), dim3(CR_LONG_NT), 0, ctx->stream, d_data,
                     d_start, d_length, nN, nS, q, mn, d_data_out, d_fix);
}

}  // namespace

// The corrected bases of every read into d_data_out (which holds a copy of d_data already, or will by stream order) and
// one cfrk_read_fix per read (d_fix may be NULL), against the job's index (built, synchronising, when it is not valid);
// the three kernels -- one per size class of reads -- are left enqueued.  Arguments are checked by the callers
// (abi.hip).  nS >= 1.
int cfrk_read_correct_launch(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                             int64_t nN, int64_t nS, uint32_t min_count, int8_t *d_data_out, cfrk_read_fix *d_fix) {
  QIndex q;
  int rc = cfrk_query_index(ctx, &q);
  if (rc) return rc;
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
#define CR_LAUNCH(MODE)                                                                                          \
  do {                                                                                                           \
    if (canon) correct_launch_all<MODE, true>(ctx, d_data, d_start, d_length, nN, nS, q, min_count, d_data_out, d_fix);   \
    else correct_launch_all<MODE, false>(ctx, d_data, d_start, d_length, nN, nS, q, min_count, d_data_out, d_fix);        \
  } while (0)
  if (q.k <= 12) CR_LAUNCH(0);
  else if (q.k <= 32) CR_LAUNCH(1);
  else CR_LAUNCH(2);
#undef CR_LAUNCH
  HIP_TRY(ctx, hipGetLastError());
  return CFRK_OK;
}
