// pairs.hip -- paired-end reads (cfrk_abi.h, the pairs section): the JOIN of the two mates' keep decisions and the
// CHECK that the two mates of every pair carry the same name.  Both address mate A of pair j as element j * stride of
// the *_a arrays and mate B as element j * stride of the *_b arrays: interleaved reads are (a, a + 1, 2), split reads
// are (a, b, 1).
//
// Join: one launch, one thread per pair and turn (grid-stride behind PAIR_GRID_WGS_PER_CU workgroups per CU).  A thread
// reads everything of BOTH mates before it writes anything, and no thread reads another pair's elements, so the outputs
// may be the keep inputs.  The four counts are kept in registers over a thread's turns, summed over the wave, then over
// the workgroup in LDS, and added once per workgroup: added once per wave from 8 workgroups per CU, a join of 131 072
// pairs took 32 us, its 2 048 waves' adds queueing on one cache line, for a kernel that moves 512 KB.
// normalize.hip puts this launch between the judge and the insert kernels of a paired round.
//
// Name check, two launches over all pairs, each taking the pairs of its class:
//   pair_names_kernel        both names of at most CFRK_PAIR_NAME_FAST = 16 x 16 bytes: a group of 16 lanes per pair (four
//                            pairs per wave and turn), lane l looks at bytes [16 l, 16 l + 16) of both names -- at most 32
//                            byte loads per lane and pair whatever the names hold.  Pairs whose header range does not lie
//                            inside its text are judged (bad) here as well, without a load from the text.
//   pair_names_long_kernel   a longer name: the workgroup lists the long pairs among PN_LONG_NT pairs in LDS (the walker of
//                            lane_group.h's long_reads) and takes them one after the other, thread t looking at the
//                            16-byte pieces t, t + PN_LONG_NT, ..  A 20 KB name is 80 bytes per thread instead of a wave
//                            that waits for one lane's 20 000 turns.
// What a lane reports of its piece: the first space or tab of A, the first of B, and the first index at which the two
// names differ (inside both).  The minima over the group give the identifiers' ends eA and eB and the first mismatch m;
// with e = eA = eB and d = 2 where A[e-2, e) is "/1" and B[e-2, e) is "/2", else 0, the pair is good iff e - d > 0 and
// m >= e - d.  (Identifiers of different lengths are never equal: the two suffixes are dropped together or not at all.)
// Byte loads: the two names of a pair are not aligned to each other and a header is some tens of bytes.
#include "common.h"
#include "lane_group.h"
#include "read_windows.h"
#include "staging.h"

#include <vector>

namespace {

constexpr int PAIR_NT = 256;
constexpr int PAIR_GRID_WGS_PER_CU = 1;
constexpr int PN_PIECE = 16;
constexpr int PN_LONG_NT = 256;
static_assert(CFRK_PAIR_NAME_FAST == 16 * PN_PIECE, "a 16-lane group holds the fast class in one piece per lane");
static_assert(sizeof(cfrk_pair_counts) == 32, "cfrk_pair_counts is 32 bytes without padding");

enum { PW_PAIRS = 0, PW_ORPHAN_A, PW_ORPHAN_B, PW_DROPPED, PW_FIRST_BAD, PW_N_BAD, PW_NWORDS = 8 };

// ---- join -------------------------------------------------------------------------------------

struct PairSide { const uint8_t *keep; const cfrk_read_span *span; const int32_t *length; };
struct PairIn { PairSide a, b; int64_t n_pairs; int stride; int mode; int32_t min_len; };

// the survive rule of cfrk_abi.h for element i of a side
__device__ __forceinline__ bool pair_survives(const PairSide &s, int64_t i, int32_t min_len) {
  if (s.keep && !s.keep[i]) return false;
  if (s.span) {
    const cfrk_read_span sp = s.span[i];
    if (sp.offset < 0 || sp.length < 0 || (int64_t)sp.offset + (int64_t)sp.length > (int64_t)s.length[i]) return false;
    return sp.length >= min_len;
  }
  return !s.length || s.length[i] >= min_len;
}

// (no __restrict__: pair_a / pair_b may be the keep arrays of `in`)
__global__ __launch_bounds__(PAIR_NT) void pair_join_kernel(PairIn in, uint8_t *pair_a, uint8_t *pair_b, uint8_t *orphan_a,
                                                            uint8_t *orphan_b, unsigned long long *counts) {
  __shared__ uint32_t s_counts[4];
  if (threadIdx.x < 4) s_counts[threadIdx.x] = 0;
  __syncthreads();
  uint32_t n_pair = 0, n_oa = 0, n_ob = 0, n_drop = 0;
  for (int64_t j = (int64_t)blockIdx.x * PAIR_NT + threadIdx.x; j < in.n_pairs; j += (int64_t)gridDim.x * PAIR_NT) {
    const int64_t i = j * in.stride;
    const bool sa = pair_survives(in.a, i, in.min_len), sb = pair_survives(in.b, i, in.min_len);   // both mates read ...
    const bool either = in.mode == CFRK_PAIR_EITHER;
    const bool pair = either ? (sa || sb) : (sa && sb);
    const bool oa = !either && sa && !sb, ob = !either && sb && !sa;
    pair_a[i] = pair;                                                                             // ... before either is written
    pair_b[i] = pair;
    if (orphan_a) orphan_a[i] = oa;
    if (orphan_b) orphan_b[i] = ob;
    n_pair += pair; n_oa += oa; n_ob += ob; n_drop += !(pair || oa || ob);
  }
  n_pair = group_sum_u32<64>(n_pair);
  n_oa = group_sum_u32<64>(n_oa);
  n_ob = group_sum_u32<64>(n_ob);
  n_drop = group_sum_u32<64>(n_drop);
  if ((threadIdx.x & 63) == 0) {
    if (n_pair) atomicAdd(&s_counts[PW_PAIRS], n_pair);
    if (n_oa) atomicAdd(&s_counts[PW_ORPHAN_A], n_oa);
    if (n_ob) atomicAdd(&s_counts[PW_ORPHAN_B], n_ob);
    if (n_drop) atomicAdd(&s_counts[PW_DROPPED], n_drop);
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_counts[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)s_counts[threadIdx.x]);
}

// ---- name check -------------------------------------------------------------------------------

struct NameIn {
  const uint8_t *text_a, *text_b;
  const cfrk_text_record *rec_a, *rec_b;
  int64_t nbytes_a, nbytes_b, n_pairs;
  int stride;
};

// a name: n bytes from text[off ..); ok = the header range lies inside the text (nothing is loaded otherwise)
struct Name { const uint8_t *p; int32_t n; bool ok; };
__device__ __forceinline__ Name pn_name(const uint8_t *text, int64_t nbytes, const cfrk_text_record &r) {
  const bool ok = r.head_off >= 0 && r.head_len >= 0 && r.head_off <= nbytes && (int64_t)r.head_len <= nbytes - r.head_off;
  Name m;
  m.ok = ok;
  m.n = ok && r.head_len > 0 ? r.head_len - 1 : 0;
  m.p = text + (ok ? r.head_off + 1 : 0);     // (never dereferenced when n == 0)
  return m;
}
__device__ __forceinline__ bool pn_is_long(const Name &a, const Name &b) {
  return a.ok && b.ok && (a.n > CFRK_PAIR_NAME_FAST || b.n > CFRK_PAIR_NAME_FAST);
}

constexpr uint32_t PN_NONE = 0x7FFFFFFFu;      // (a name has at most 2^31 - 2 bytes)
struct Piece {
  uint32_t first_a = PN_NONE, first_b = PN_NONE, mism = PN_NONE;
  // bytes [i0, i0 + PN_PIECE) of both names
  __device__ __forceinline__ void look(const Name &a, const Name &b, int64_t i0) {
#pragma unroll
    for (int u = 0; u < PN_PIECE; ++u) {
      const int64_t i = i0 + u;
      const bool ia = i < a.n, ib = i < b.n;
      const int ca = ia ? (int)a.p[i] : -1, cb = ib ? (int)b.p[i] : -1;
      if ((ca == ' ' || ca == '\t') && first_a == PN_NONE) first_a = (uint32_t)i;
      if ((cb == ' ' || cb == '\t') && first_b == PN_NONE) first_b = (uint32_t)i;
      if (ia && ib && ca != cb && mism == PN_NONE) mism = (uint32_t)i;
    }
  }
};

// the verdict from the minima over all pieces
__device__ __forceinline__ bool pn_good(const Name &a, const Name &b, uint32_t first_a, uint32_t first_b, uint32_t mism) {
  const uint32_t ea = min(first_a, (uint32_t)a.n), eb = min(first_b, (uint32_t)b.n);
  if (ea != eb) return false;
  uint32_t e = ea;
  if (e >= 2 && a.p[e - 2] == '/' && a.p[e - 1] == '1' && b.p[e - 2] == '/' && b.p[e - 1] == '2') e -= 2;
  return e > 0 && mism >= e;
}

__device__ __forceinline__ uint32_t group16_min(uint32_t v) {
  for (int o = 8; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}

// the bad pairs a wave has seen, to the two result words: once per wave
__device__ __forceinline__ void pn_flush(uint32_t bad, unsigned long long first, unsigned long long *words) {
  bad = group_sum_u32<64>(bad);
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long x = __shfl_xor(first, o);
    first = x < first ? x : first;
  }
  if ((threadIdx.x & 63) == 0 && bad) {
    atomicAdd(words + PW_N_BAD, (unsigned long long)bad);
    atomicMin(words + PW_FIRST_BAD, first);
  }
}

__global__ __launch_bounds__(256) void pair_names_kernel(NameIn in, unsigned long long *words) {
  const int grp = threadIdx.x / 16, lane = threadIdx.x % 16;
  uint32_t bad = 0;
  unsigned long long first = ~0ull;
  for (int64_t j = (int64_t)blockIdx.x * 16 + grp; j < in.n_pairs; j += (int64_t)gridDim.x * 16) {
    const Name a = pn_name(in.text_a, in.nbytes_a, in.rec_a[j * in.stride]);
    const Name b = pn_name(in.text_b, in.nbytes_b, in.rec_b[j * in.stride]);
    if (pn_is_long(a, b)) continue;                                    // (the whole group agrees)
    bool good = false;
    if (a.ok && b.ok) {
      Piece pc;
      pc.look(a, b, (int64_t)lane * PN_PIECE);
      good = pn_good(a, b, group16_min(pc.first_a), group16_min(pc.first_b), group16_min(pc.mism));
    }
    if (lane == 0 && !good) { ++bad; if ((unsigned long long)j < first) first = (unsigned long long)j; }
  }
  pn_flush(bad, first, words);
}

__global__ __launch_bounds__(PN_LONG_NT) void pair_names_long_kernel(NameIn in, unsigned long long *words) {
  __shared__ int s_list[PN_LONG_NT];
  __shared__ int s_n;
  __shared__ uint32_t s_min[3];
  const int tid = threadIdx.x;
  uint32_t bad = 0;
  unsigned long long first = ~0ull;
  for (int64_t base = (int64_t)blockIdx.x * PN_LONG_NT; base < in.n_pairs; base += (int64_t)gridDim.x * PN_LONG_NT) {
    if (tid == 0) s_n = 0;
    __syncthreads();
    if (base + tid < in.n_pairs) {
      const int64_t i = (base + tid) * in.stride;
      if (pn_is_long(pn_name(in.text_a, in.nbytes_a, in.rec_a[i]), pn_name(in.text_b, in.nbytes_b, in.rec_b[i])))
        s_list[atomicAdd(&s_n, 1)] = tid;
    }
    __syncthreads();
    const int nl = s_n;
    for (int q = 0; q < nl; ++q) {
      const int64_t j = base + s_list[q];
      const Name a = pn_name(in.text_a, in.nbytes_a, in.rec_a[j * in.stride]);
      const Name b = pn_name(in.text_b, in.nbytes_b, in.rec_b[j * in.stride]);
      if (tid < 3) s_min[tid] = PN_NONE;
      __syncthreads();
      Piece pc;
      const int64_t nmax = a.n > b.n ? a.n : b.n;
      for (int64_t i0 = (int64_t)tid * PN_PIECE; i0 < nmax; i0 += (int64_t)PN_LONG_NT * PN_PIECE) pc.look(a, b, i0);
      if (pc.first_a != PN_NONE) atomicMin(&s_min[0], pc.first_a);
      if (pc.first_b != PN_NONE) atomicMin(&s_min[1], pc.first_b);
      if (pc.mism != PN_NONE) atomicMin(&s_min[2], pc.mism);
      __syncthreads();
      if (tid == 0 && !pn_good(a, b, s_min[0], s_min[1], s_min[2])) {
        ++bad;
        if ((unsigned long long)j < first) first = (unsigned long long)j;
      }
      __syncthreads();                                                  // (the minima are reset for the next pair)
    }
    // (the list is written again only behind the barrier that follows s_n = 0, and every thread has left the loop above
    // through its last barrier or never entered it)
  }
  pn_flush(bad, first, words);
}

// ---- host side ----------------------------------------------------------------------------------

int pair_words(cfrk_ctx *ctx, unsigned long long **words) {
  void *p;
  if (const int rc = cfrk_pool_get(ctx, BUF_PAIRS, PW_NWORDS * sizeof(unsigned long long), &p)) return rc;
  *words = (unsigned long long *)p;
  return CFRK_OK;
}

int join_check(cfrk_ctx *ctx, int64_t n_pairs, int stride, int mode, int32_t min_len, const void *span_a, const void *span_b,
               const void *length_a, const void *length_b, const void *pair_a, const void *pair_b) {
  if (!ctx) return CFRK_ERR_ARG;
  if (n_pairs < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative n_pairs");
  if (min_len < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "min_len %d is negative", (int)min_len);
  if (stride != 1 && stride != 2) return cfrk_fail(ctx, CFRK_ERR_ARG, "stride %d: 1 (split) or 2 (interleaved)", stride);
  if (mode != CFRK_PAIR_BOTH && mode != CFRK_PAIR_EITHER) return cfrk_fail(ctx, CFRK_ERR_ARG, "mode %d: CFRK_PAIR_BOTH or CFRK_PAIR_EITHER", mode);
  if ((!length_a && (span_a || min_len > 0)) || (!length_b && (span_b || min_len > 0)))
    return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL length with a span or with min_len > 0");
  if (n_pairs > 0 && (!pair_a || !pair_b)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL output");
  return CFRK_OK;
}

// the device words down to a counts row; synchronises
int join_counts(cfrk_ctx *ctx, const unsigned long long *words, cfrk_pair_counts *counts) {
  unsigned long long w[4];
  HIP_TRY(ctx, hipMemcpyAsync(w, words, sizeof w, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *counts = {(int64_t)w[PW_PAIRS], (int64_t)w[PW_ORPHAN_A], (int64_t)w[PW_ORPHAN_B], (int64_t)w[PW_DROPPED]};
  return CFRK_OK;
}

int names_check(cfrk_ctx *ctx, int64_t n_pairs, int stride, const void *text_a, uint64_t nbytes_a, const void *rec_a, const void *text_b,
                uint64_t nbytes_b, const void *rec_b, int64_t *first_bad, int64_t *n_bad) {
  if (!ctx) return CFRK_ERR_ARG;
  if (n_pairs < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative n_pairs");
  if (stride != 1 && stride != 2) return cfrk_fail(ctx, CFRK_ERR_ARG, "stride %d: 1 (split) or 2 (interleaved)", stride);
  if (!first_bad || !n_bad) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL output");
  if (n_pairs > 0 && (!rec_a || !rec_b)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL records");
  if ((nbytes_a > 0 && !text_a) || (nbytes_b > 0 && !text_b)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL text");
  if (nbytes_a > ((uint64_t)1 << 62) || nbytes_b > ((uint64_t)1 << 62)) return cfrk_fail(ctx, CFRK_ERR_ARG, "nbytes");
  *first_bad = -1;
  *n_bad = 0;
  return CFRK_OK;
}

// both launches and the two results; synchronises.  n_pairs >= 1.
int names_core(cfrk_ctx *ctx, const NameIn &in, int64_t *first_bad, int64_t *n_bad) {
  unsigned long long *words;
  if (const int rc = pair_words(ctx, &words)) return rc;
  HIP_TRY(ctx, hipMemsetAsync(words + PW_FIRST_BAD, 0xFF, sizeof *words, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(words + PW_N_BAD, 0, sizeof *words, ctx->stream));
  hipLaunchKernelGGL(pair_names_kernel, dim3(reads_grid(in.n_pairs, 16, (int64_t)ctx->num_cus * 64)), dim3(256), 0, ctx->stream, in, words);
  hipLaunchKernelGGL(pair_names_long_kernel, dim3(reads_grid(in.n_pairs, PN_LONG_NT, (int64_t)ctx->num_cus * 4)), dim3(PN_LONG_NT), 0,
                     ctx->stream, in, words);
  HIP_TRY(ctx, hipGetLastError());
  unsigned long long w[2];
  HIP_TRY(ctx, hipMemcpyAsync(w, words + PW_FIRST_BAD, sizeof w, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *n_bad = (int64_t)w[1];
  *first_bad = w[1] ? (int64_t)w[0] : -1;
  return CFRK_OK;
}

}  // namespace

// The join of n_pairs >= 1 pairs enqueued on the context stream, its four counts ADDED to d_counts[0 .. 4) (pairs kept,
// orphans A, orphans B, pairs dropped).  Arguments are checked by the callers.
int cfrk_pair_join_launch(cfrk_ctx *ctx, int64_t n_pairs, int stride, int mode, int32_t min_len, const uint8_t *d_keep_a,
                          const uint8_t *d_keep_b, const cfrk_read_span *d_span_a, const cfrk_read_span *d_span_b,
                          const int32_t *d_length_a, const int32_t *d_length_b, uint8_t *d_pair_a, uint8_t *d_pair_b,
                          uint8_t *d_orphan_a, uint8_t *d_orphan_b, unsigned long long *d_counts) {
  const PairIn in = {{d_keep_a, d_span_a, d_length_a}, {d_keep_b, d_span_b, d_length_b}, n_pairs, stride, mode, min_len};
  hipLaunchKernelGGL(pair_join_kernel, dim3(reads_grid(n_pairs, PAIR_NT, (int64_t)ctx->num_cus * PAIR_GRID_WGS_PER_CU)), dim3(PAIR_NT), 0,
                     ctx->stream, in, d_pair_a, d_pair_b, d_orphan_a, d_orphan_b, d_counts);
  HIP_TRY(ctx, hipGetLastError());
  return CFRK_OK;
}

extern "C" int cfrk_reads_pair_keep_device(cfrk_ctx *ctx, int64_t n_pairs, int stride, int mode, int32_t min_len, const uint8_t *d_keep_a,
                                           const uint8_t *d_keep_b, const cfrk_read_span *d_span_a, const cfrk_read_span *d_span_b,
                                           const int32_t *d_length_a, const int32_t *d_length_b, uint8_t *d_pair_a, uint8_t *d_pair_b,
                                           uint8_t *d_orphan_a, uint8_t *d_orphan_b, cfrk_pair_counts *counts) {
  int rc = join_check(ctx, n_pairs, stride, mode, min_len, d_span_a, d_span_b, d_length_a, d_length_b, d_pair_a, d_pair_b);
  if (rc) return rc;
  if (counts) *counts = {0, 0, 0, 0};
  if (n_pairs == 0) return CFRK_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  unsigned long long *words;
  if ((rc = pair_words(ctx, &words))) return rc;
  HIP_TRY(ctx, hipMemsetAsync(words, 0, 4 * sizeof *words, ctx->stream));
  if ((rc = cfrk_pair_join_launch(ctx, n_pairs, stride, mode, min_len, d_keep_a, d_keep_b, d_span_a, d_span_b, d_length_a, d_length_b,
                                  d_pair_a, d_pair_b, d_orphan_a, d_orphan_b, words))) return rc;
  return counts ? join_counts(ctx, words, counts) : CFRK_OK;
}

extern "C" int cfrk_reads_pair_keep(cfrk_ctx *ctx, int64_t n_pairs, int stride, int mode, int32_t min_len, const uint8_t *keep_a,
                                    const uint8_t *keep_b, const cfrk_read_span *span_a, const cfrk_read_span *span_b,
                                    const int32_t *length_a, const int32_t *length_b, uint8_t *pair_a, uint8_t *pair_b, uint8_t *orphan_a,
                                    uint8_t *orphan_b, cfrk_pair_counts *counts) {
  int rc = join_check(ctx, n_pairs, stride, mode, min_len, span_a, span_b, length_a, length_b, pair_a, pair_b);
  if (rc) return rc;
  if (counts) *counts = {0, 0, 0, 0};
  if (n_pairs == 0) return CFRK_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // the addressed elements gathered side by side (the device runs the split layout whatever the caller's is):
  // [keep a | keep b | span a | span b | length a | length b] in, [pair a | pair b | orphan a | orphan b] out
  const size_t n = (size_t)n_pairs;
  const size_t in_bytes[6] = {keep_a ? n : 0, keep_b ? n : 0, span_a ? n * 8 : 0, span_b ? n * 8 : 0, length_a ? n * 4 : 0, length_b ? n * 4 : 0};
  const void *src[6] = {keep_a, keep_b, span_a, span_b, length_a, length_b};
  const size_t elem[6] = {1, 1, 8, 8, 4, 4};
  Carve c;
  size_t off[10];
  for (int q = 0; q < 6; ++q) off[q] = c.part(in_bytes[q]);
  const size_t in_end = c.end;
  for (int q = 6; q < 10; ++q) off[q] = c.part(n);
  std::vector<uint8_t> h;
  try { h.resize(c.end); } catch (...) { return cfrk_fail(ctx, CFRK_ERR_NOMEM, "%zu bytes of host memory", c.end); }
  for (int q = 0; q < 6; ++q)
    if (src[q])
      for (size_t j = 0; j < n; ++j) memcpy(&h[off[q] + j * elem[q]], (const char *)src[q] + j * (size_t)stride * elem[q], elem[q]);
  void *p;
  unsigned long long *words;
  if ((rc = cfrk_pool_get(ctx, BUF_PAIRS_IN, c.end, &p)) || (rc = pair_words(ctx, &words))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(p, h.data(), in_end, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(words, 0, 4 * sizeof *words, ctx->stream));
  auto dev = [&](int q) { return q < 6 && !src[q] ? nullptr : (char *)p + off[q]; };
  if ((rc = cfrk_pair_join_launch(ctx, n_pairs, 1, mode, min_len, (const uint8_t *)dev(0), (const uint8_t *)dev(1), (const cfrk_read_span *)dev(2),
                                  (const cfrk_read_span *)dev(3), (const int32_t *)dev(4), (const int32_t *)dev(5), (uint8_t *)dev(6),
                                  (uint8_t *)dev(7), orphan_a ? (uint8_t *)dev(8) : nullptr, orphan_b ? (uint8_t *)dev(9) : nullptr, words)))
    return stage_drain(ctx, rc);
  HIP_TRY(ctx, hipMemcpyAsync(&h[off[6]], dev(6), c.end - off[6], hipMemcpyDeviceToHost, ctx->stream));
  cfrk_pair_counts row;
  if ((rc = join_counts(ctx, words, &row))) return rc;                  // (synchronises: the bytes are down as well)
  if (counts) *counts = row;
  uint8_t *dst[4] = {pair_a, pair_b, orphan_a, orphan_b};
  for (int q = 0; q < 4; ++q)
    if (dst[q])
      for (size_t j = 0; j < n; ++j) dst[q][j * (size_t)stride] = h[off[6 + q] + j];
  return CFRK_OK;
}

extern "C" int cfrk_text_pair_check_device(cfrk_ctx *ctx, int64_t n_pairs, int stride, const uint8_t *d_text_a, uint64_t nbytes_a,
                                           const cfrk_text_record *d_rec_a, const uint8_t *d_text_b, uint64_t nbytes_b,
                                           const cfrk_text_record *d_rec_b, int64_t *first_bad, int64_t *n_bad) {
  const int rc = names_check(ctx, n_pairs, stride, d_text_a, nbytes_a, d_rec_a, d_text_b, nbytes_b, d_rec_b, first_bad, n_bad);
  if (rc || n_pairs == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const NameIn in = {d_text_a, d_text_b, d_rec_a, d_rec_b, (int64_t)nbytes_a, (int64_t)nbytes_b, n_pairs, stride};
  return names_core(ctx, in, first_bad, n_bad);
}

extern "C" int cfrk_text_pair_check(cfrk_ctx *ctx, int64_t n_pairs, int stride, const char *text_a, uint64_t nbytes_a,
                                    const cfrk_text_record *rec_a, const char *text_b, uint64_t nbytes_b, const cfrk_text_record *rec_b,
                                    int64_t *first_bad, int64_t *n_bad) {
  int rc = names_check(ctx, n_pairs, stride, text_a, nbytes_a, rec_a, text_b, nbytes_b, rec_b, first_bad, n_bad);
  if (rc || n_pairs == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // the addressed records gathered side by side, the texts behind them (one copy when both mates live in one text)
  const size_t n = (size_t)n_pairs;
  const bool one_text = text_a == text_b && nbytes_a == nbytes_b;
  std::vector<cfrk_text_record> h;
  try { h.resize(2 * n); } catch (...) { return cfrk_fail(ctx, CFRK_ERR_NOMEM, "%zu records of host memory", 2 * n); }
  for (size_t j = 0; j < n; ++j) { h[j] = rec_a[j * (size_t)stride]; h[n + j] = rec_b[j * (size_t)stride]; }
  Carve c;
  const size_t o_rec = c.part(2 * n * sizeof(cfrk_text_record));
  const size_t o_ta = c.part((size_t)nbytes_a), o_tb = one_text ? o_ta : c.part((size_t)nbytes_b);
  void *p;
  if ((rc = cfrk_pool_get(ctx, BUF_PAIRS_IN, c.end, &p))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync((char *)p + o_rec, h.data(), 2 * n * sizeof(cfrk_text_record), hipMemcpyHostToDevice, ctx->stream));
  if (nbytes_a) HIP_TRY(ctx, hipMemcpyAsync((char *)p + o_ta, text_a, (size_t)nbytes_a, hipMemcpyHostToDevice, ctx->stream));
  if (nbytes_b && !one_text) HIP_TRY(ctx, hipMemcpyAsync((char *)p + o_tb, text_b, (size_t)nbytes_b, hipMemcpyHostToDevice, ctx->stream));
  const cfrk_text_record *d_rec = carve_at<cfrk_text_record>(p, o_rec);
  const NameIn in = {carve_at<uint8_t>(p, o_ta), carve_at<uint8_t>(p, o_tb), d_rec, d_rec + n, (int64_t)nbytes_a, (int64_t)nbytes_b, n_pairs, 1};
  return stage_drain(ctx, names_core(ctx, in, first_bad, n_bad));
}
