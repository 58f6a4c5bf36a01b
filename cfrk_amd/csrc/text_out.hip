// text_out.hip -- text back out of the device: the RECORD INDEX of a text (where each record's header line and quality
// line lie, cfrk_text_record) and the EMITTER that writes the kept, trimmed reads as FASTA or FASTQ text with their
// original names and the matching slice of their quality line.  The definitions are in cfrk_abi.h.
//
// Index.  The shape of the parsers (ingest.hip, ingest_fastq.hip), with another carry.  A line is closed by its '\n' or
// by the text's end, and the thread on that byte writes the line's fields: it needs the line's START and its NUMBER.
// Both are prefix quantities of the newlines in front of it:
//   the start   = the position behind the last '\n' before the closing byte (0 when there is none): a running MAXIMUM
//   the number  = FASTQ: the '\n' before it (line 4r is record r's header, line 4r + 3 its quality line);
//                 FASTA: the header lines that begin before it, minus one -- a header line begins behind a '\n' that is
//                 followed by '>' (or at byte 0), so the count is kept with those newlines: a running SUM
// and, for FASTA, whether the line being closed is a header: one bit that travels with the start (the maximum is taken
// over start << 1 | bit).  A line may have begun any number of tiles before its end, so nothing looks back or ahead for
// these: the scan carries all three across the tiles, and inside a tile they are scanned across lanes, waves and
// iterations.  The only bytes a thread reads beside its own 16 are the one behind them (is the line that a lane's
// last '\n' opens a header?) and the one in front of a closing byte (a '\r' to drop).
//   tx_reduce_kernel   one workgroup per tile of CFRK_TEXT_TILE_BYTES: the counted newlines, the last line start
//   tx_scan_kernel     ONE workgroup walks the tile aggregates in blocks of CFRK_TEXT_SCAN_TILES: exclusive count and
//                      carried line start per tile, the totals
//   -- the host reads the totals back (the call's one synchronisation) and checks the capacity --
//   tx_scatter_kernel  re-reads the text; the closing threads write head_off / head_len or qual_off / qual_len
//
// Emitter.  The shape of the select (read_filter.hip): a per-read measure pass reduced per tile of reads, a
// one-workgroup scan, a pass that writes each kept read's output offset and input index, and the copy.  The copy is
// balanced by OUTPUT bytes: one workgroup takes CFRK_EMIT_TILE_BYTES of d_out, finds the reads that meet its tile by a
// search in the output offsets, and gathers each read's pieces -- marker, name, '\n', bases, ("\n+\n", qualities,) '\n' --
// clipped to the tile: the source bytes are loaded as the aligned dwords that cover them (codes are translated to
// letters a dword at a time) and written into LDS at the alignment they have in d_out, then stored as whole 16-byte
// blocks.  A read of 10^6 bases or a 20 KB name is spread over its tiles like any other bytes; inside a tile the reads go
// to lane groups of 16, 64 or all 256 threads by the tile's mean read size.  All offsets are 64-bit.
#include "common.h"
#include "ingest_bytes.h"
#include "staging.h"

namespace {

// ---- index ------------------------------------------------------------------------------------

constexpr int TX_THREADS = 256;
constexpr int TX_WAVES = TX_THREADS / 64;
constexpr int TX_ITER_BYTES = TX_THREADS * 16;
constexpr int TX_TILE = CFRK_TEXT_TILE_BYTES;
constexpr int TX_ITERS = TX_TILE / TX_ITER_BYTES;
constexpr int TX_SCAN = CFRK_TEXT_SCAN_TILES;
static_assert(TX_TILE % TX_ITER_BYTES == 0 && TX_TILE <= 32768, "a tile is whole iterations; a line start inside it and its bit take 16 bits");
static_assert(TX_SCAN % 64 == 0 && TX_SCAN <= 1024 && (int64_t)TX_SCAN * TX_TILE < ((int64_t)1 << 31), "the block sums are 32-bit");
static_assert(sizeof(cfrk_text_record) == 24, "cfrk_text_record is 24 bytes without padding");

enum { TW_COUNT = 0, TW_OPEN_END, TW_LONG_REC, TW_NWORDS = 8 };      // device words of an index (uint64 each), in front of the aggregates
constexpr size_t TX_WORDS_BYTES = TW_NWORDS * 8;

struct TxLane {
  uint32_t nl;        // '\n' among the lane's bytes inside the text
  uint32_t hdr;       // ... that are followed by a '>' inside the text: a header line begins behind them
};

__device__ __forceinline__ void tx_lane(const uint8_t *__restrict__ text, uint64_t p0, uint64_t n, TxLane &L) {
  uint32_t valid;
  const uint4 v = fa_load(text, p0, n, valid);
  L.nl = fa_eq16(v, 0x0A0A0A0Au) & valid;
  uint32_t gt = (fa_eq16(v, 0x3E3E3E3Eu) & valid) >> 1;
  if ((L.nl >> 15) && p0 + 16 < n) gt |= (uint32_t)(text[p0 + 16] == '>') << 15;
  L.hdr = L.nl & gt;
}

// the lane's last line start, relative to the tile, with its header bit: (offset behind its last '\n') << 1 | bit, 0: none
__device__ __forceinline__ uint32_t tx_last_start(const TxLane &L, uint32_t off) {
  if (!L.nl) return 0u;
  const uint32_t b = 31u - (uint32_t)__clz(L.nl);
  return ((off + b + 1u) << 1) | ((L.hdr >> b) & 1u);
}

// inclusive prefix maximum over the 64 lanes of a wave: dev_wave_scan_incl's six DPP steps with max (0 is the identity)
__device__ __forceinline__ uint32_t tx_wave_max_incl(uint32_t x) {
  x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false));
  x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false));
  x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false));
  x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false));
  x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false));
  x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false));
  return x;
}

__device__ __forceinline__ uint64_t tx_wave_scan_incl_u64(uint64_t x, int lane, bool take_max) {
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t y = (uint64_t)__shfl_up((unsigned long long)x, o);
    if (lane >= o) x = take_max ? (y > x ? y : x) : x + y;
  }
  return x;
}

// tile aggregate: x = counted newlines (FASTQ: all, FASTA: those that open a header line), y = the tile's last line start
template <bool FASTQ>
__global__ __launch_bounds__(TX_THREADS) void tx_reduce_kernel(const uint8_t *__restrict__ text, uint64_t n, uint2 *__restrict__ agg) {
  __shared__ uint32_t sc[TX_WAVES], sm[TX_WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t tile = blockIdx.x, base = tile * (uint64_t)TX_TILE;
  uint32_t cnt = 0, last = 0;
  for (int it = 0; it < TX_ITERS; ++it) {
    const uint32_t off = (uint32_t)(it * TX_ITER_BYTES + threadIdx.x * 16);
    if (base + off >= n) break;
    TxLane L;
    tx_lane(text, base + off, n, L);
    cnt += (uint32_t)__popc(FASTQ ? L.nl : L.hdr);
    last = max(last, tx_last_start(L, off));
  }
  const uint32_t ic = dev_wave_scan_incl(cnt), im = tx_wave_max_incl(last);
  if (lane == 63) { sc[w] = ic; sm[w] = im; }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tc = 0, tm = 0;
    for (int j = 0; j < TX_WAVES; ++j) { tc += sc[j]; tm = max(tm, sm[j]); }
    agg[tile] = make_uint2(tc, tm);
  }
}

// one workgroup of TX_SCAN threads: tile t of a block is thread t's.  pre[t] = {count in front of the tile (FASTA: the
// header at byte 0 included), the line that is open at its beginning as start << 1 | header bit}
template <bool FASTQ>
__global__ __launch_bounds__(TX_SCAN) void tx_scan_kernel(const uint8_t *__restrict__ text, uint64_t n, const uint2 *__restrict__ agg, uint64_t ntiles,
                                                          uint64_t *__restrict__ words, ulonglong2 *__restrict__ pre) {
  constexpr int NW = TX_SCAN / 64;
  __shared__ uint32_t sc[NW];
  __shared__ unsigned long long sm[NW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t first_hdr = (n > 0 && text[0] == '>') ? 1u : 0u;       // the line at byte 0 is opened by no newline
  uint64_t base_c = FASTQ ? 0u : first_hdr, base_m = first_hdr;
  for (uint64_t b0 = 0; b0 < ntiles; b0 += TX_SCAN) {
    const uint64_t t = b0 + threadIdx.x;
    const uint2 a = t < ntiles ? agg[t] : make_uint2(0u, 0u);
    const uint64_t m = a.y ? (((t * (uint64_t)TX_TILE + (a.y >> 1)) << 1) | (a.y & 1u)) : 0u;
    const uint32_t ic = dev_wave_scan_incl(a.x);
    const uint64_t im = tx_wave_scan_incl_u64(m, lane, true);
    const uint64_t em = (uint64_t)__shfl_up((unsigned long long)im, 1);
    if (lane == 63) { sc[w] = ic; sm[w] = im; }
    __syncthreads();
    uint64_t pc = 0, tc = 0, pm = 0, tm = 0;
    for (int j = 0; j < NW; ++j) {
      if (j < w) { pc += sc[j]; pm = sm[j] > pm ? sm[j] : pm; }
      tc += sc[j]; tm = sm[j] > tm ? sm[j] : tm;
    }
    if (lane > 0 && em > pm) pm = em;
    if (t < ntiles) pre[t] = make_ulonglong2(base_c + pc + ic - a.x, pm > base_m ? pm : base_m);
    base_c += tc;
    if (tm > base_m) base_m = tm;
    __syncthreads();       // (sc / sm are written again by the next block)
  }
  if (threadIdx.x == 0) {
    words[TW_COUNT] = base_c;
    words[TW_OPEN_END] = (n > 0 && text[n - 1] != '\n') ? 1u : 0u;
  }
}

// the line that ends at c (its '\n', or n) began at s and is line / header number `num` (see the file comment)
template <bool FASTQ>
__device__ __forceinline__ void tx_close(const uint8_t *__restrict__ text, uint64_t s, bool is_hdr, uint64_t c, uint64_t num, uint64_t nS,
                                         cfrk_text_record *__restrict__ rec, uint64_t *__restrict__ words) {
  uint64_t r;
  bool qual = false;
  if (FASTQ) {
    const uint32_t kind = (uint32_t)num & 3u;
    if (kind != 0u && kind != 3u) return;
    qual = kind == 3u;
    r = num >> 2;
  } else {
    if (!is_hdr || num == 0) return;
    r = num - 1;
  }
  if (r >= nS) return;                                  // (FASTQ: the lines of an incomplete last record)
  uint64_t len = c - s;
  if (len > 0 && text[c - 1] == '\r') --len;
  if (len > 0x7FFFFFFFull) {
    atomicMin((unsigned long long *)&words[TW_LONG_REC], (unsigned long long)r);
    len = 0x7FFFFFFFull;
  }
  if (qual) {
    rec[r].qual_off = (int64_t)s;
    rec[r].qual_len = (int32_t)len;
  } else {
    rec[r].head_off = (int64_t)s;
    rec[r].head_len = (int32_t)len;
    if (!FASTQ) { rec[r].qual_off = -1; rec[r].qual_len = 0; }
  }
}

template <bool FASTQ>
__global__ __launch_bounds__(TX_THREADS) void tx_scatter_kernel(const uint8_t *__restrict__ text, uint64_t n, const ulonglong2 *__restrict__ pre,
                                                                uint64_t *__restrict__ words, cfrk_text_record *__restrict__ rec, uint64_t nS) {
  __shared__ uint32_t sc[2][TX_WAVES], sm[2][TX_WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t tile = blockIdx.x, base = tile * (uint64_t)TX_TILE;
  const ulonglong2 p = pre[tile];
  uint64_t cbase = p.x;
  const uint64_t open = p.y;
  uint32_t run = 0;                                     // the last line start of the iterations before this one
  for (int it = 0; it < TX_ITERS; ++it) {
    const uint32_t off = (uint32_t)(it * TX_ITER_BYTES + threadIdx.x * 16);
    if (base + (uint64_t)it * TX_ITER_BYTES >= n) break;
    const uint64_t p0 = base + off;
    TxLane L;
    tx_lane(text, p0, n, L);
    const uint32_t cm = FASTQ ? L.nl : L.hdr;
    const uint32_t mine = (uint32_t)__popc(cm);
    const uint32_t ic = dev_wave_scan_incl(mine), im = tx_wave_max_incl(tx_last_start(L, off));
    uint32_t before = dev_lane_prev(im);                // (lane 0 reads 0)
    if (lane == 63) { sc[it & 1][w] = ic; sm[it & 1][w] = im; }
    __syncthreads();       // (one barrier per iteration: the two sets alternate)
    uint32_t excl = ic - mine, total = 0, all = 0;
#pragma unroll
    for (int j = 0; j < TX_WAVES; ++j) {
      const uint32_t c = sc[it & 1][j], m = sm[it & 1][j];
      if (j < w) { excl += c; before = max(before, m); }
      total += c; all = max(all, m);
    }
    before = max(before, run);
    // the closing bytes among the lane's: its newlines, and the text's last byte when that is none
    uint32_t closing = L.nl;
    const bool at_end = p0 < n && n - p0 <= 16 && !((L.nl >> (int)(n - p0 - 1)) & 1u);
    if (at_end) closing |= 1u << (int)(n - p0);         // (bit 16 when the last byte is the lane's sixteenth)
    for (uint32_t m = closing; m; m &= m - 1u) {
      const uint32_t low = (m & (0u - m)) - 1u;
      const uint32_t below = L.nl & low;
      uint64_t s;
      bool is_hdr;
      if (below) {
        const uint32_t b = 31u - (uint32_t)__clz(below);
        s = p0 + b + 1u; is_hdr = (L.hdr >> b) & 1u;
      } else if (before) {
        s = base + (before >> 1); is_hdr = before & 1u;
      } else {
        s = open >> 1; is_hdr = open & 1u;
      }
      tx_close<FASTQ>(text, s, is_hdr, p0 + (uint32_t)__popc(low), cbase + excl + (uint32_t)__popc(cm & low), nS, rec, words);
    }
    run = max(run, all);
    cbase += total;
  }
}

struct TxPlan { uint64_t *words; uint2 *agg; ulonglong2 *pre; uint64_t ntiles; };

int tx_plan(cfrk_ctx *ctx, uint64_t nbytes, TxPlan *pl) {
  pl->ntiles = (nbytes + TX_TILE - 1) / TX_TILE;
  void *p;
  const int rc = cfrk_pool_get(ctx, BUF_TEXT_INDEX, TX_WORDS_BYTES + (size_t)pl->ntiles * 24, &p);
  if (rc) return rc;
  pl->words = (uint64_t *)p;
  pl->pre = (ulonglong2 *)((char *)p + TX_WORDS_BYTES);
  pl->agg = (uint2 *)(pl->pre + pl->ntiles);
  return CFRK_OK;
}

// reduce + scan, the number of records read back (synchronises).  nbytes >= 1.
int tx_measure(cfrk_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, int format, const TxPlan &pl, int64_t *nS) {
  HIP_TRY(ctx, hipMemsetAsync(pl.words, 0xFF, TX_WORDS_BYTES, ctx->stream));
  if (format == CFRK_TEXT_FASTQ) {
    hipLaunchKernelGGL(tx_reduce_kernel<true>, dim3((unsigned)pl.ntiles), dim3(TX_THREADS), 0, ctx->stream, d_text, nbytes, pl.agg);
    hipLaunchKernelGGL(tx_scan_kernel<true>, dim3(1), dim3(TX_SCAN), 0, ctx->stream, d_text, nbytes, pl.agg, pl.ntiles, pl.words, pl.pre);
  } else {
    hipLaunchKernelGGL(tx_reduce_kernel<false>, dim3((unsigned)pl.ntiles), dim3(TX_THREADS), 0, ctx->stream, d_text, nbytes, pl.agg);
    hipLaunchKernelGGL(tx_scan_kernel<false>, dim3(1), dim3(TX_SCAN), 0, ctx->stream, d_text, nbytes, pl.agg, pl.ntiles, pl.words, pl.pre);
  }
  HIP_TRY(ctx, hipGetLastError());
  uint64_t wd[2];
  HIP_TRY(ctx, hipMemcpyAsync(wd, pl.words, sizeof wd, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *nS = (int64_t)(format == CFRK_TEXT_FASTQ ? (wd[TW_COUNT] + wd[TW_OPEN_END]) >> 2 : wd[TW_COUNT]);
  return CFRK_OK;
}

// the scatter, left enqueued; only a text that can hold an over-long line is waited for
int tx_scatter(cfrk_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, int format, const TxPlan &pl, cfrk_text_record *d_rec, int64_t nS) {
  if (format == CFRK_TEXT_FASTQ)
    hipLaunchKernelGGL(tx_scatter_kernel<true>, dim3((unsigned)pl.ntiles), dim3(TX_THREADS), 0, ctx->stream, d_text, nbytes, pl.pre, pl.words, d_rec, (uint64_t)nS);
  else
    hipLaunchKernelGGL(tx_scatter_kernel<false>, dim3((unsigned)pl.ntiles), dim3(TX_THREADS), 0, ctx->stream, d_text, nbytes, pl.pre, pl.words, d_rec, (uint64_t)nS);
  HIP_TRY(ctx, hipGetLastError());
  if (nbytes <= 0x7FFFFFFFull) return CFRK_OK;
  uint64_t bad;
  HIP_TRY(ctx, hipMemcpyAsync(&bad, pl.words + TW_LONG_REC, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (bad != ~0ull) return cfrk_fail(ctx, CFRK_ERR_LAYOUT, "text index: record %llu has a line of more than 2^31 - 1 bytes", (unsigned long long)bad);
  return CFRK_OK;
}

int tx_check(cfrk_ctx *ctx, const void *text, uint64_t nbytes, int format, const void *rec, uint64_t cap_reads, int64_t *nS_out) {
  if (!ctx) return CFRK_ERR_ARG;
  if (format != CFRK_TEXT_FASTA && format != CFRK_TEXT_FASTQ) return cfrk_fail(ctx, CFRK_ERR_ARG, "format %d: CFRK_TEXT_FASTA or CFRK_TEXT_FASTQ", format);
  if (!nS_out) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL size output");
  if (nbytes > 0 && !text) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL text");
  if (cap_reads > 0 && !rec) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL array with a capacity above 0");
  if (nbytes > ((uint64_t)1 << 62)) return cfrk_fail(ctx, CFRK_ERR_ARG, "nbytes");
  *nS_out = 0;
  return CFRK_OK;
}

int tx_fit(cfrk_ctx *ctx, int64_t nS, uint64_t cap_reads, int64_t *nS_out) {
  *nS_out = nS;
  if ((uint64_t)nS > cap_reads)
    return cfrk_fail(ctx, CFRK_ERR_SMALL_BUF, "text index: %lld records, room for %llu", (long long)nS, (unsigned long long)cap_reads);
  return CFRK_OK;
}

// ---- emitter ----------------------------------------------------------------------------------

constexpr int EM_THREADS = 256;
constexpr int EM_TILE = CFRK_EMIT_TILE_BYTES;
constexpr int EM_SCAN = CFRK_SELECT_SCAN_TILES;
static_assert(CFRK_SELECT_TILE_READS == EM_THREADS, "a tile of reads is one read per thread");
static_assert(EM_TILE % 16 == 0 && EM_TILE + 16 <= 65536, "a tile of d_out and its skew fit LDS");
static_assert(EM_SCAN % 64 == 0 && EM_SCAN <= 1024 && (int64_t)EM_SCAN * EM_THREADS < ((int64_t)1 << 31), "the block's read counts are 32-bit");

enum { EW_READS = 0, EW_BYTES, EW_NWORDS = 8 };
constexpr size_t EM_WORDS_BYTES = EW_NWORDS * 8;

struct EmIn {
  const int64_t *start; const int32_t *length; const cfrk_read_span *span; const uint8_t *keep; const cfrk_text_record *rec;
  int64_t nN, nS, nbytes;
  int32_t min_len;
  int fastq;
};

// what a kept read contributes: n codes from data[src ..], name_len bytes from text[name_off ..], n bytes from text[qsrc ..]
struct EmRead { int64_t src, name_off, qsrc; int32_t n, name_len; };

// does [off, off + len) lie inside [0, nbytes]?
__host__ __device__ __forceinline__ bool em_range_ok(int64_t off, int32_t len, int64_t nbytes) {
  return off >= 0 && len >= 0 && off <= nbytes && (int64_t)len <= nbytes - off;
}
// the record rule of cfrk_abi.h: 0 = fine, 1 = a range outside the text, 2 = FASTQ output without a matching quality line
__host__ __device__ __forceinline__ int em_record_fault(const cfrk_text_record &t, int32_t L, int64_t nbytes, int fastq) {
  const bool no_qual = t.qual_off == -1 && t.qual_len == 0;
  if (!em_range_ok(t.head_off, t.head_len, nbytes) || !(no_qual || em_range_ok(t.qual_off, t.qual_len, nbytes))) return 1;
  if (fastq && (no_qual || t.qual_len != L)) return 2;
  return 0;
}

// is read i kept?  Every term is range-checked before it is used (the select's rule, then the record's)
__device__ __forceinline__ bool em_read(const EmIn &a, int64_t i, EmRead &r) {
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
  const cfrk_text_record t = a.rec[i];
  if (em_record_fault(t, L, a.nbytes, a.fastq)) return false;
  r.src = st + off;
  r.n = n;
  r.name_off = t.head_off + 1;
  r.name_len = t.head_len > 0 ? t.head_len - 1 : 0;
  r.qsrc = t.qual_off + off;
  return true;
}
__device__ __forceinline__ uint64_t em_bytes(const EmRead &r, int fastq) {
  return fastq ? (uint64_t)r.name_len + 2u * (uint64_t)r.n + 6u : (uint64_t)r.name_len + (uint64_t)r.n + 3u;
}

__global__ __launch_bounds__(EM_THREADS) void em_reduce_kernel(EmIn a, ulonglong2 *__restrict__ agg) {
  __shared__ uint32_t sc[EM_THREADS / 64];
  __shared__ unsigned long long sb[EM_THREADS / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * EM_THREADS + threadIdx.x;
  EmRead r;
  const bool kept = i < a.nS && em_read(a, i, r);
  const uint32_t ic = dev_wave_scan_incl(kept ? 1u : 0u);
  const uint64_t ib = tx_wave_scan_incl_u64(kept ? em_bytes(r, a.fastq) : 0u, lane, false);
  if (lane == 63) { sc[w] = ic; sb[w] = ib; }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t tc = 0, tb = 0;
    for (int j = 0; j < EM_THREADS / 64; ++j) { tc += sc[j]; tb += sb[j]; }
    agg[blockIdx.x] = make_ulonglong2(tc, tb);
  }
}

// one workgroup of EM_SCAN threads: tile t of a block is thread t's
__global__ __launch_bounds__(EM_SCAN) void em_scan_kernel(const ulonglong2 *__restrict__ agg, int64_t ntiles, uint64_t *__restrict__ words,
                                                          ulonglong2 *__restrict__ pre) {
  constexpr int NW = EM_SCAN / 64;
  __shared__ uint32_t sc[NW];
  __shared__ unsigned long long sb[NW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t base_c = 0, base_b = 0;
  for (int64_t b0 = 0; b0 < ntiles; b0 += EM_SCAN) {
    const int64_t t = b0 + threadIdx.x;
    const ulonglong2 a = t < ntiles ? agg[t] : make_ulonglong2(0, 0);
    const uint32_t c = (uint32_t)a.x;
    const uint32_t ic = dev_wave_scan_incl(c);
    const uint64_t ib = tx_wave_scan_incl_u64(a.y, lane, false);
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
  if (threadIdx.x == 0) { words[EW_READS] = base_c; words[EW_BYTES] = base_b; }
}

// per read again: kept read j begins at byte out_off[j] of the output and is input read src_idx[j]
__global__ __launch_bounds__(EM_THREADS) void em_index_kernel(EmIn a, const ulonglong2 *__restrict__ pre, int64_t *__restrict__ out_off,
                                                              int64_t *__restrict__ src_idx) {
  __shared__ uint32_t sc[EM_THREADS / 64];
  __shared__ unsigned long long sb[EM_THREADS / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * EM_THREADS + threadIdx.x;
  EmRead r;
  const bool kept = i < a.nS && em_read(a, i, r);
  const uint32_t c = kept ? 1u : 0u;
  const uint64_t b = kept ? em_bytes(r, a.fastq) : 0u;
  const uint32_t ic = dev_wave_scan_incl(c);
  const uint64_t ib = tx_wave_scan_incl_u64(b, lane, false);
  if (lane == 63) { sc[w] = ic; sb[w] = ib; }
  __syncthreads();
  uint64_t pc = 0, pb = 0;
  for (int j = 0; j < w; ++j) { pc += sc[j]; pb += sb[j]; }
  if (!kept) return;
  const ulonglong2 p = pre[blockIdx.x];
  const int64_t j = (int64_t)(p.x + pc + ic - c);
  out_off[j] = (int64_t)(p.y + pb + ib - b);
  src_idx[j] = i;
}

// four codes -> four letters: 0 1 2 3 -> A C G T, anything else -> N
__device__ __forceinline__ uint32_t em_letters4(uint32_t w) {
  uint32_t out = 0;
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const uint32_t c = (w >> (8 * x)) & 0xFFu;
    out |= (c < 4u ? (0x54474341u >> (8 * c)) & 0xFFu : (uint32_t)'N') << (8 * x);
  }
  return out;
}

// The part of a piece that meets the tile, into the stage: the piece is n bytes of src[sa ..] (src holds `limit` bytes)
// and lies at [pos, pos + n) of the output; stage byte off0 + x is byte T0 + x of the output.  By the G lanes of a group.
template <int G, bool LETTERS>
__device__ __forceinline__ void em_piece(const uint8_t *__restrict__ src, int64_t limit, int64_t sa, int64_t pos, int64_t n, int64_t T0, int64_t T1,
                                         uint8_t *stage, uint32_t off0, int lane) {
  const int64_t a = pos > T0 ? pos : T0, b = pos + n < T1 ? pos + n : T1;
  if (a >= b) return;
  sa += a - pos;
  const int cnt = (int)(b - a);
  const int skew = (int)((reinterpret_cast<uintptr_t>(src) + (uintptr_t)sa) & 3u);
  const int ndw = (skew + cnt + 3) >> 2;
  uint8_t *dst = stage + off0 + (uint32_t)(a - T0);
  for (int d = lane; d < ndw; d += G) {
    const int64_t off = sa - skew + 4 * (int64_t)d;
    uint32_t w;
    if (off >= 0 && off + 4 <= limit) {
      w = *reinterpret_cast<const uint32_t *>(src + off);
    } else {
      w = 0;
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int64_t g = off + x;
        if (g >= 0 && g < limit) w |= (uint32_t)src[g] << (8 * x);
      }
    }
    if (LETTERS) w = em_letters4(w);
    const int p = 4 * d - skew;
    if (p >= 0 && p + 4 <= cnt && ((uint32_t)(dst + p - stage) & 3u) == 0) {
      *reinterpret_cast<uint32_t *>(dst + p) = w;
    } else {
#pragma unroll
      for (int x = 0; x < 4; ++x)
        if (p + x >= 0 && p + x < cnt) dst[p + x] = (uint8_t)(w >> (8 * x));
    }
  }
}

__device__ __forceinline__ void em_literal(int64_t pos, uint8_t ch, int64_t T0, int64_t T1, uint8_t *stage, uint32_t off0) {
  if (pos >= T0 && pos < T1) stage[off0 + (uint32_t)(pos - T0)] = ch;
}

// kept reads [j0, j1) into the tile's stage, read by read by groups of G threads
template <int G>
__device__ __forceinline__ void em_gather(const EmIn &a, const uint8_t *__restrict__ data, const uint8_t *__restrict__ text,
                                          const int64_t *__restrict__ out_off, const int64_t *__restrict__ src_idx, int64_t j0, int64_t j1,
                                          int64_t T0, int64_t T1, uint8_t *stage, uint32_t off0) {
  const int grp = threadIdx.x / G, lane = threadIdx.x % G;
  for (int64_t j = j0 + grp; j < j1; j += EM_THREADS / G) {
    const int64_t i = src_idx[j];
    EmRead r;
    if (i < 0 || i >= a.nS || !em_read(a, i, r)) continue;      // (the passes before this one kept it: never taken)
    int64_t pos = out_off[j];
    const int64_t name_at = pos + 1, bases_at = name_at + r.name_len + 1, behind = bases_at + r.n;
    if (lane == 0) {
      em_literal(pos, a.fastq ? '@' : '>', T0, T1, stage, off0);
      em_literal(bases_at - 1, '\n', T0, T1, stage, off0);
      em_literal(behind, '\n', T0, T1, stage, off0);
    }
    em_piece<G, false>(text, a.nbytes, r.name_off, name_at, r.name_len, T0, T1, stage, off0, lane);
    em_piece<G, true>(data, a.nN, r.src, bases_at, r.n, T0, T1, stage, off0, lane);
    if (a.fastq) {
      if (lane == G - 1) {
        em_literal(behind + 1, '+', T0, T1, stage, off0);
        em_literal(behind + 2, '\n', T0, T1, stage, off0);
        em_literal(behind + 3 + r.n, '\n', T0, T1, stage, off0);
      }
      em_piece<G, false>(text, a.nbytes, r.qsrc, behind + 3, r.n, T0, T1, stage, off0, lane);
    }
  }
}

__global__ __launch_bounds__(EM_THREADS) void em_copy_kernel(EmIn a, const int8_t *__restrict__ data, const uint8_t *__restrict__ text,
                                                             const int64_t *__restrict__ out_off, const int64_t *__restrict__ src_idx,
                                                             int64_t nS_out, int64_t nbytes_out, uint8_t *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[EM_TILE + 16];
  const int64_t T0 = (int64_t)blockIdx.x * EM_TILE;
  const int64_t T1 = T0 + EM_TILE < nbytes_out ? T0 + EM_TILE : nbytes_out;
  // the read that holds byte T0: the last one with out_off <= T0 (out_off[0] = 0, strictly ascending, and the reads
  // cover the output without gaps); then the first read that begins at or behind T1
  int64_t lo = 0, hi = nS_out;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (out_off[mid] <= T0) lo = mid + 1; else hi = mid;
  }
  const int64_t j0 = lo - 1;
  hi = j0 + 1 + (T1 - T0) < nS_out ? j0 + 1 + (T1 - T0) : nS_out;      // (every read takes at least three bytes)
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (out_off[mid] < T1) lo = mid + 1; else hi = mid;
  }
  const int64_t j1 = lo, nreads = j1 - j0;
  const uint32_t off0 = (uint32_t)(reinterpret_cast<uintptr_t>(out + T0) & 15u);
  const uint8_t *codes = reinterpret_cast<const uint8_t *>(data);
  if (j0 >= 0) {
    if (nreads * 2048 <= EM_TILE) em_gather<EM_THREADS>(a, codes, text, out_off, src_idx, j0, j1, T0, T1, stage, off0);
    else if (nreads * 512 <= EM_TILE) em_gather<64>(a, codes, text, out_off, src_idx, j0, j1, T0, T1, stage, off0);
    else em_gather<16>(a, codes, text, out_off, src_idx, j0, j1, T0, T1, stage, off0);
  }
  __syncthreads();
  // LDS -> out: whole aligned 16-byte blocks, bytes at the two ends (the neighbours' bytes share those blocks)
  uint8_t *g0 = out + T0 - off0;
  const uint32_t end = off0 + (uint32_t)(T1 - T0);
  for (uint32_t b = threadIdx.x * 16; b < end; b += EM_THREADS * 16) {
    if (b >= off0 && b + 16 <= end) {
      *reinterpret_cast<uint4 *>(g0 + b) = *reinterpret_cast<const uint4 *>(stage + b);
    } else {
      for (uint32_t x = b; x < b + 16; ++x)
        if (x >= off0 && x < end) g0[x] = stage[x];
    }
  }
}

struct EmPlan { uint64_t *words; ulonglong2 *agg, *pre; int64_t ntiles; };

int em_plan(cfrk_ctx *ctx, int64_t nS, EmPlan *pl) {
  pl->ntiles = (nS + EM_THREADS - 1) / EM_THREADS;
  void *p;
  const int rc = cfrk_pool_get(ctx, BUF_EMIT, EM_WORDS_BYTES + (size_t)pl->ntiles * 32, &p);
  if (rc) return rc;
  pl->words = (uint64_t *)p;
  pl->agg = (ulonglong2 *)((char *)p + EM_WORDS_BYTES);
  pl->pre = pl->agg + pl->ntiles;
  return CFRK_OK;
}

// reduce + scan, the totals read back (synchronises).  nS >= 1.
int em_measure(cfrk_ctx *ctx, const EmIn &in, const EmPlan &pl, uint64_t *nbytes_out, int64_t *nS_out) {
  hipLaunchKernelGGL(em_reduce_kernel, dim3((unsigned)pl.ntiles), dim3(EM_THREADS), 0, ctx->stream, in, pl.agg);
  hipLaunchKernelGGL(em_scan_kernel, dim3(1), dim3(EM_SCAN), 0, ctx->stream, pl.agg, pl.ntiles, pl.words, pl.pre);
  HIP_TRY(ctx, hipGetLastError());
  uint64_t wd[2];
  HIP_TRY(ctx, hipMemcpyAsync(wd, pl.words, sizeof wd, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *nS_out = (int64_t)wd[EW_READS];
  *nbytes_out = wd[EW_BYTES];
  return CFRK_OK;
}

// the index pass and the copy, left enqueued.  nS_out >= 1.
int em_write(cfrk_ctx *ctx, const EmIn &in, const EmPlan &pl, const int8_t *d_data, const uint8_t *d_text, uint8_t *d_out, uint64_t nbytes_out,
             int64_t nS_out) {
  void *p;
  if (const int rc = cfrk_pool_get(ctx, BUF_EMIT_OFF, (size_t)nS_out * 16, &p)) return rc;
  int64_t *out_off = (int64_t *)p, *src_idx = out_off + nS_out;
  hipLaunchKernelGGL(em_index_kernel, dim3((unsigned)pl.ntiles), dim3(EM_THREADS), 0, ctx->stream, in, pl.pre, out_off, src_idx);
  const uint64_t ctiles = (nbytes_out + EM_TILE - 1) / EM_TILE;
  hipLaunchKernelGGL(em_copy_kernel, dim3((unsigned)ctiles), dim3(EM_THREADS), 0, ctx->stream, in, d_data, d_text, (const int64_t *)out_off,
                     (const int64_t *)src_idx, nS_out, (int64_t)nbytes_out, d_out);
  HIP_TRY(ctx, hipGetLastError());
  return CFRK_OK;
}

int em_check(cfrk_ctx *ctx, const void *data, const void *start, const void *length, int64_t nN, int64_t nS, int32_t min_len, const void *text,
             uint64_t nbytes, const void *rec, int out_format, const void *out, uint64_t cap_out, uint64_t *nbytes_out, int64_t *nS_out) {
  if (!ctx) return CFRK_ERR_ARG;
  if (nN < 0 || nS < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (min_len < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "min_len %d is negative", (int)min_len);
  if (out_format != CFRK_TEXT_FASTA && out_format != CFRK_TEXT_FASTQ)
    return cfrk_fail(ctx, CFRK_ERR_ARG, "out_format %d: CFRK_TEXT_FASTA or CFRK_TEXT_FASTQ", out_format);
  if (!nbytes_out || !nS_out) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL size output");
  if ((nS > 0 && (!start || !length || !rec)) || (nN > 0 && !data) || (nbytes > 0 && !text)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  if (cap_out > 0 && !out) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL array with a capacity above 0");
  if (nbytes > ((uint64_t)1 << 62)) return cfrk_fail(ctx, CFRK_ERR_ARG, "nbytes");
  *nbytes_out = 0;
  *nS_out = 0;
  return CFRK_OK;
}

int em_fit(cfrk_ctx *ctx, uint64_t nb, int64_t ns, uint64_t cap_out, uint64_t *nbytes_out, int64_t *nS_out) {
  *nbytes_out = nb; *nS_out = ns;
  if (nb > cap_out)
    return cfrk_fail(ctx, CFRK_ERR_SMALL_BUF, "emit: %llu bytes of text, room for %llu", (unsigned long long)nb, (unsigned long long)cap_out);
  return CFRK_OK;
}

}  // namespace

extern "C" int cfrk_text_index_device(cfrk_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, int format, cfrk_text_record *d_rec,
                                      uint64_t cap_reads, int64_t *nS_out) {
  int rc = tx_check(ctx, d_text, nbytes, format, d_rec, cap_reads, nS_out);
  if (rc || nbytes == 0) return rc;
  if (((uintptr_t)d_text & 15) != 0) return cfrk_fail(ctx, CFRK_ERR_ALIGN, "d_text %p", (const void *)d_text);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  TxPlan pl;
  int64_t nS = 0;
  if ((rc = tx_plan(ctx, nbytes, &pl)) || (rc = tx_measure(ctx, d_text, nbytes, format, pl, &nS)) || (rc = tx_fit(ctx, nS, cap_reads, nS_out)) || nS == 0)
    return rc;
  return tx_scatter(ctx, d_text, nbytes, format, pl, d_rec, nS);
}

extern "C" int cfrk_text_index(cfrk_ctx *ctx, const char *text, uint64_t nbytes, int format, cfrk_text_record *rec, uint64_t cap_reads,
                               int64_t *nS_out) {
  int rc = tx_check(ctx, text, nbytes, format, rec, cap_reads, nS_out);
  if (rc || nbytes == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  TxPlan pl;
  void *d_text, *d_rec;
  int64_t nS = 0;
  if ((rc = tx_plan(ctx, nbytes, &pl)) || (rc = cfrk_pool_get(ctx, BUF_TEXT_IN, (size_t)nbytes + 16, &d_text))) return rc;   // (every slot before the copy)
  HIP_TRY(ctx, hipMemcpyAsync(d_text, text, (size_t)nbytes, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = tx_measure(ctx, (const uint8_t *)d_text, nbytes, format, pl, &nS)) || (rc = tx_fit(ctx, nS, cap_reads, nS_out)) || nS == 0)
    return stage_drain(ctx, rc);
  if ((rc = cfrk_pool_get(ctx, BUF_TEXT_OUT, (size_t)nS * sizeof(cfrk_text_record), &d_rec))) return rc;
  if ((rc = tx_scatter(ctx, (const uint8_t *)d_text, nbytes, format, pl, (cfrk_text_record *)d_rec, nS))) return stage_drain(ctx, rc);
  return cfrk_memcpy_d2h(ctx, rec, d_rec, (size_t)nS * sizeof(cfrk_text_record));
}

extern "C" int cfrk_reads_emit_text_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                                           int64_t nS, const cfrk_read_span *d_span, const uint8_t *d_keep, int32_t min_len,
                                           const uint8_t *d_text, uint64_t nbytes, const cfrk_text_record *d_rec, int out_format,
                                           uint8_t *d_out, uint64_t cap_out, uint64_t *nbytes_out, int64_t *nS_out) {
  int rc = em_check(ctx, d_data, d_start, d_length, nN, nS, min_len, d_text, nbytes, d_rec, out_format, d_out, cap_out, nbytes_out, nS_out);
  if (rc || nS == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const EmIn in = {d_start, d_length, d_span, d_keep, d_rec, nN, nS, (int64_t)nbytes, min_len, out_format == CFRK_TEXT_FASTQ};
  EmPlan pl;
  uint64_t nb = 0;
  int64_t ns = 0;
  if ((rc = em_plan(ctx, nS, &pl)) || (rc = em_measure(ctx, in, pl, &nb, &ns)) || (rc = em_fit(ctx, nb, ns, cap_out, nbytes_out, nS_out)) || ns == 0)
    return rc;
  return em_write(ctx, in, pl, d_data, d_text, d_out, nb, ns);
}

extern "C" int cfrk_reads_emit_text(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length, int64_t nN, int64_t nS,
                                    const cfrk_read_span *span, const uint8_t *keep, int32_t min_len, const char *text, uint64_t nbytes,
                                    const cfrk_text_record *rec, int out_format, char *out, uint64_t cap_out, uint64_t *nbytes_out,
                                    int64_t *nS_out) {
  int rc = em_check(ctx, data, start, length, nN, nS, min_len, text, nbytes, rec, out_format, out, cap_out, nbytes_out, nS_out);
  if (rc || nS == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int fastq = out_format == CFRK_TEXT_FASTQ;
  StagePart x[4] = {{span, span ? (size_t)nS * sizeof(cfrk_read_span) : 0, nullptr},
                    {keep, keep ? (size_t)nS : 0, nullptr},
                    {rec, (size_t)nS * sizeof(cfrk_text_record), nullptr},
                    {text, (size_t)nbytes, nullptr}};
  StagedReads d;
  if ((rc = stage_reads(ctx, BUF_EMIT_IN, data, start, length, nN, nS, STAGE_TABLE, x, 4, &d))) return rc;
  // (the layout holds: every length[i] is in range)
  for (int64_t i = 0; i < nS; ++i) {
    const char *why = nullptr;
    if (span && (span[i].offset < 0 || span[i].length < 0 || (int64_t)span[i].offset + (int64_t)span[i].length > (int64_t)length[i]))
      why = "its span does not lie inside its bases";
    else if (const int f = em_record_fault(rec[i], length[i], (int64_t)nbytes, fastq))
      why = f == 1 ? "its record's header or quality range does not lie inside the text" : "FASTQ output needs a quality line as long as the read";
    if (why) {
      cfrk_fail(ctx, CFRK_ERR_LAYOUT, "read %lld: %s", (long long)i, why);
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // (the copies read the caller's buffers)
      return CFRK_ERR_LAYOUT;
    }
  }
  const EmIn in = {d.start, d.length, (const cfrk_read_span *)x[0].dev, (const uint8_t *)x[1].dev, (const cfrk_text_record *)x[2].dev,
                   nN, nS, (int64_t)nbytes, min_len, fastq};
  EmPlan pl;
  uint64_t nb = 0;
  int64_t ns = 0;
  if ((rc = em_plan(ctx, nS, &pl)) || (rc = em_measure(ctx, in, pl, &nb, &ns)) || (rc = em_fit(ctx, nb, ns, cap_out, nbytes_out, nS_out)) || ns == 0)
    return stage_drain(ctx, rc);
  void *d_out;
  if ((rc = cfrk_pool_get(ctx, BUF_EMIT_OUT, (size_t)nb + 16, &d_out))) return stage_drain(ctx, rc);
  if ((rc = em_write(ctx, in, pl, d.data, (const uint8_t *)x[3].dev, (uint8_t *)d_out, nb, ns))) return stage_drain(ctx, rc);
  return cfrk_memcpy_d2h(ctx, out, d_out, (size_t)nb);
}
