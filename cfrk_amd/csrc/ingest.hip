// ingest.hip -- FASTA text in device memory -> the struct-read layout (data / start / length), byte for byte what
// cfrk_host_parse_fasta (cfrk_amd/host/cfrk_host.cpp) produces.  A memory-bound compaction: classify, scan, scatter.
//
// Every byte of the text either EMITS one byte of `data` or nothing, and the emitted bytes appear in text order without
// gaps, so a byte's place in `data` is the number of emitting bytes before it:
//   a byte of a sequence line emits its code when it is KEPT: always in compat mode (newlines encode as -1), in native
//     mode unless it belongs to the line's trailing run of '\n' / '\r';
//   in native mode the '>' of a header line emits the -1 that terminates the record before it (its code is -1 anyway);
//     the '>' at offset 0 has no record before it and emits nothing.  The last terminator is written by the length pass.
//   start[r] = emitting bytes before the '>' of record r (+ 1 in native mode for r > 0: behind that terminator).
// Whether a byte lies on a header line is a carry along the text: state = (seen a line start, the last line start is a
// header), combine(a, b) = b.seen ? b : a -- associative, so it is scanned like a sum.  A tile that does not know its
// carry yet counts its kept bytes before its first line start apart (they are emitted only when the carry says
// "sequence line").
//
// Launches, all on the context stream, no workgroup ever waits for another one:
//   fa_reduce_kernel  one workgroup per tile of CFRK_FASTA_TILE_BYTES: emit counts (before / after the first line
//                     start), header line starts, the tile's carry, where its first line start is
//   fa_scan_kernel    ONE workgroup walks the tile aggregates in blocks of CFRK_FASTA_SCAN_TILES: carry in, exclusive
//                     emit and header counts per tile, the totals (aggregate + scan: 32 bytes per tile, 2 MB per GB of text)
//   -- the host reads the totals and the error words back (the call's one synchronisation) and checks the capacities --
//   fa_scatter_kernel re-reads the text, compacts the codes of 4096 bytes through LDS and writes them with 16-byte
//                     stores; the thread on a record's '>' writes start[r]
//   fa_length_kernel  length[r] = next start (or nN) - start[r] - 1, the record's terminator, the over-long check
// The trailing-'\r' rule of native mode looks ahead from a '\r' at the end of a lane's 16 bytes to the first byte that
// is not '\r', through global memory and across tiles.  The look ahead is bounded: a sequence line that holds more than
// CFRK_FASTA_MAX_CR_RUN carriage returns in a row is refused, exactly (the lane in which a run begins adds its own
// '\r's to those it finds ahead, so the bound does not depend on how the run lies in the 16-byte pieces).  A run in a
// header line is never refused; where the reduce pass does not know yet whether it is in one (no line start in the
// tile before the run), the tile aggregate carries the run's offset and the scan, which knows the carry, decides.
#include "common.h"
#include "ingest_bytes.h"
#include "staging.h"

#include <algorithm>

namespace {

constexpr int FA_THREADS = 256;
constexpr int FA_ITER_BYTES = FA_THREADS * 16;
constexpr int FA_TILE = CFRK_FASTA_TILE_BYTES;
constexpr int FA_ITERS = FA_TILE / FA_ITER_BYTES;
constexpr int FA_SCAN = CFRK_FASTA_SCAN_TILES;
static_assert(FA_TILE % FA_ITER_BYTES == 0 && FA_TILE < 65535 && CFRK_FASTA_MAX_CR_RUN > 16, "a tile is whole iterations; offsets inside it take 20 bits");
static_assert(FA_SCAN % 64 == 0 && FA_SCAN <= 1024 && (int64_t)FA_SCAN * FA_TILE < ((int64_t)1 << 31), "the block sums are 32-bit");

// device words of a parse (uint64 each), in front of the tile aggregates
enum { FW_EMIT = 0, FW_NHDR, FW_FLAGS, FW_OFF_EMPTY, FW_OFF_CR, FW_REC_LONG, FW_NWORDS = 8 };
enum { FE_NO_HEADER = 1, FE_EMPTY = 2, FE_CR_RUN = 4, FE_LONG = 8 };
// tile aggregate: x = emits before the first line start (kept bytes, if the carry is a sequence line) | (1 + offset of
// an over-long '\r' run in that part, 0: none) << 16, y = emits from it on, z = header line starts, w = flags | offset of the first line start << 8
enum { FT_HAS = 1, FT_LAST_HDR = 2, FT_FIRST_HDR = 4 };
constexpr uint64_t FA_CARRY_BIT = 1ull << 63;

// carry state: bit 0 = a line start was seen, bit 1 = the last one is a header
__device__ __forceinline__ uint32_t fa_fold(uint32_t a, uint32_t b) { return (b & 1u) ? b : a; }

// native mode, a '\r' in a lane's last byte: is the first byte at or behind q that is not '\r' a '\n' (or the end)?
// over: more than max_cr carriage returns lie at q and behind it (the answer is then of no use: the text is refused)
__device__ __forceinline__ uint32_t fa_look_ahead(const uint8_t *__restrict__ text, uint64_t q, uint64_t n, uint32_t max_cr, bool &over) {
  over = false;
  for (uint32_t seen = 0; q < n; ++q, ++seen) {
    const uint8_t c = text[q];
    if (c == '\n') return 1u;
    if (c != '\r') return 0u;
    if (seen >= max_cr) { over = true; return 0u; }
  }
  return 1u;
}

struct FaLane {
  uint4 v;            // the text bytes
  uint32_t valid;     // bytes inside the text
  uint32_t S, Hd;     // line starts, header line starts
  uint32_t emit;      // bytes that emit (undefined positions counted as sequence lines)
  uint32_t undef;     // positions whose line start lies before everything this workgroup has seen
  uint32_t empty;     // header line starts that follow a header line (compat: an empty record)
  uint32_t wsum;      // the wave's carry summary
};

// Classify a lane's 16 bytes.  `carry` = state in front of the workgroup's 4096 bytes; ws = 4 words of LDS for the
// waves' summaries (the caller alternates two sets and places the barrier: see fa_finish).
__device__ __forceinline__ void fa_classify(const uint8_t *__restrict__ text, uint64_t p0, uint64_t n, FaLane &L, uint32_t *ws) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  L.v = fa_load(text, p0, n, L.valid);
  const uint32_t nl = fa_eq16(L.v, 0x0A0A0A0Au) & L.valid;
  uint32_t prev = dev_lane_prev(nl >> 15);
  if (lane == 0) prev = (p0 == 0) ? 1u : (p0 <= n ? (uint32_t)(text[p0 - 1] == '\n') : 0u);
  L.S = ((nl << 1) | prev) & L.valid;
  L.Hd = L.S & fa_eq16(L.v, 0x3E3E3E3Eu);
  const bool has = L.S != 0;
  const bool lasth = has && ((L.Hd >> (31 - __clz(L.S))) & 1u);
  const unsigned long long hm = __ballot(has), lm = __ballot(lasth);
  L.wsum = hm ? (1u | ((uint32_t)((lm >> (63 - __clzll(hm))) & 1ull) << 1)) : 0u;
  if (lane == 0) ws[w] = L.wsum;
}

// after the barrier behind fa_classify: the rest of the masks.  Returns the carry behind the workgroup's 4096 bytes.
// words / pre_cr: where the reduce pass reports a run of carriage returns that is too long (the error words; an LDS
// word that takes the smallest tile offset of such a run at a position whose line start the tile has not seen);
// both NULL in the scatter pass, which runs only on texts the reduce pass and the scan have accepted.
template <bool COMPAT>
__device__ __forceinline__ uint32_t fa_finish(const uint8_t *__restrict__ text, uint64_t p0, uint64_t n, FaLane &L, const uint32_t *ws,
                                              uint32_t carry, uint64_t *__restrict__ words, uint32_t *pre_cr, uint32_t tile_off) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t win = carry, wout = carry;
#pragma unroll
  for (int i = 0; i < FA_THREADS / 64; ++i) {
    const uint32_t s = ws[i];
    if (i < w) win = fa_fold(win, s);
    wout = fa_fold(wout, s);
  }
  // the lane's carry: the nearest lane below it in the wave that holds a line start, else the wave's
  const bool has = L.S != 0;
  const bool lasth = has && ((L.Hd >> (31 - __clz(L.S))) & 1u);
  const unsigned long long hm = __ballot(has), lm = __ballot(lasth);
  const unsigned long long below = hm & ((1ull << lane) - 1ull);
  uint32_t cin = win;
  if (below) cin = 1u | ((uint32_t)((lm >> (63 - __clzll(below))) & 1ull) << 1);
  const uint32_t cdef = cin & 1u, chdr = (cin >> 1) & cdef;
  // "on a header line" per byte: every line start's kind copied forward to the next line start
  uint32_t K = L.S, V = L.Hd;
  V |= (V << 1) & ~K; K |= K << 1;
  V |= (V << 2) & ~K; K |= K << 2;
  V |= (V << 4) & ~K; K |= K << 4;
  V |= (V << 8) & ~K; K |= K << 8;
  K &= 0xFFFFu; V &= 0xFFFFu;
  const uint32_t F = V | (~K & (chdr ? 0xFFFFu : 0u));
  L.undef = ~K & (cdef ? 0u : 0xFFFFu) & 0xFFFFu;
  L.empty = L.Hd & ((F << 1) | chdr);
  uint32_t kept = L.valid & ~F;
  if (!COMPAT) {
    const uint32_t nl = fa_eq16(L.v, 0x0A0A0A0Au) & L.valid, cr = fa_eq16(L.v, 0x0D0D0D0Du) & L.valid;
    uint32_t D = nl;
    if (p0 < n && n - p0 < 16) D |= 1u << (int)(n - p0);           // the end of the text ends a line as well
    uint32_t prev_cr = dev_lane_prev(cr >> 15);
    if ((cr & kept) >> 15) {
      // t = the '\r's that end the lane's bytes; the run begins in this lane unless all 16 are '\r' and so is the byte before
      const uint32_t t = (uint32_t)__clz((int)~(cr << 16));
      if (lane == 0 && t == 16) prev_cr = (p0 > 0) ? (uint32_t)(text[p0 - 1] == '\r') : 0u;
      const bool begins = t < 16 || !prev_cr;
      bool over;
      D |= fa_look_ahead(text, p0 + 16, n, begins ? (uint32_t)CFRK_FASTA_MAX_CR_RUN - t : (uint32_t)CFRK_FASTA_MAX_CR_RUN, over) << 16;
      if (over && begins && words) {
        if ((L.undef >> 15) & 1u) {
          atomicMin(pre_cr, tile_off + 16u - t);
        } else {
          atomicOr((unsigned long long *)&words[FW_FLAGS], (unsigned long long)FE_CR_RUN);
          atomicMin((unsigned long long *)&words[FW_OFF_CR], (unsigned long long)(p0 + 16 - t));
        }
      }
    }
    for (;;) {
      const uint32_t nd = D | (cr & (D >> 1));
      if (nd == D) break;
      D = nd;
    }
    kept &= ~D;
    L.emit = kept | (p0 == 0 ? L.Hd & ~1u : L.Hd);
  } else {
    L.emit = kept;
  }
  return wout;
}

template <bool COMPAT>
__global__ __launch_bounds__(FA_THREADS) void fa_reduce_kernel(const uint8_t *__restrict__ text, uint64_t n, uint64_t *__restrict__ words,
                                                               uint4 *__restrict__ agg) {
  __shared__ uint32_t ws[2][FA_THREADS / 64];
  __shared__ uint32_t red[5];      // emits before / from the first line start, headers, min(first line start << 1 | header),
                                   // min offset of an over-long '\r' run in front of the first line start
  const uint64_t tile = blockIdx.x, base = tile * (uint64_t)FA_TILE;
  if (threadIdx.x < 3) red[threadIdx.x] = 0;
  if (threadIdx.x == 3) red[3] = red[4] = 0xFFFFFFFFu;
  if (tile == 0 && threadIdx.x == 0 && text[0] != '>') atomicOr((unsigned long long *)&words[FW_FLAGS], (unsigned long long)FE_NO_HEADER);
  uint32_t carry = 0, e_pre = 0, e_rest = 0, nh = 0, first = 0xFFFFFFFFu;
  for (int it = 0; it < FA_ITERS; ++it) {
    const uint64_t p0 = base + (uint64_t)it * FA_ITER_BYTES + (uint64_t)threadIdx.x * 16;
    if (base + (uint64_t)it * FA_ITER_BYTES >= n) break;
    FaLane L;
    fa_classify(text, p0, n, L, ws[it & 1]);
    __syncthreads();
    carry = fa_finish<COMPAT>(text, p0, n, L, ws[it & 1], carry, words, &red[4], (uint32_t)(it * FA_ITER_BYTES + threadIdx.x * 16));
    e_pre += __popc(L.emit & L.undef);
    e_rest += __popc(L.emit & ~L.undef);
    nh += __popc(L.Hd);
    if (L.S && first == 0xFFFFFFFFu) {
      const int j = __ffs(L.S) - 1;
      first = ((uint32_t)(it * FA_ITER_BYTES + threadIdx.x * 16 + j) << 1) | ((L.Hd >> j) & 1u);
    }
    if (COMPAT && L.empty) {
      atomicOr((unsigned long long *)&words[FW_FLAGS], (unsigned long long)FE_EMPTY);
      atomicMin((unsigned long long *)&words[FW_OFF_EMPTY], (unsigned long long)(p0 + (uint64_t)(__ffs(L.empty) - 1)));
    }
  }
  // the tile's sums: a wave scan each, then one LDS atomic per wave
  const uint32_t s0 = dev_wave_scan_incl(e_pre), s1 = dev_wave_scan_incl(e_rest), s2 = dev_wave_scan_incl(nh);
  if ((threadIdx.x & 63) == 63) {
    if (s0) atomicAdd(&red[0], s0);
    if (s1) atomicAdd(&red[1], s1);
    if (s2) atomicAdd(&red[2], s2);
  }
  if (first != 0xFFFFFFFFu) atomicMin(&red[3], first);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t fl = 0;
    if (carry & 1u) fl = FT_HAS | ((carry & 2u) ? FT_LAST_HDR : 0u) | ((red[3] & 1u) ? FT_FIRST_HDR : 0u) | ((red[3] >> 1) << 8);
    agg[tile] = make_uint4(red[0] | ((red[4] == 0xFFFFFFFFu ? 0u : red[4] + 1u) << 16), red[1], red[2], fl);
  }
}

// one workgroup of FA_SCAN threads: tile t of a block is thread t's
template <bool COMPAT>
__global__ __launch_bounds__(FA_SCAN) void fa_scan_kernel(const uint4 *__restrict__ agg, uint64_t ntiles, uint64_t n, uint64_t *__restrict__ words,
                                                          ulonglong2 *__restrict__ out) {
  constexpr int NW = FA_SCAN / 64;
  __shared__ uint32_t ws[NW], se[NW], sh[NW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t carry = 0;
  uint64_t base_e = 0, base_h = 0;
  for (uint64_t b0 = 0; b0 < ntiles; b0 += FA_SCAN) {
    const uint64_t t = b0 + threadIdx.x;
    const uint4 a = t < ntiles ? agg[t] : make_uint4(0, 0, 0, 0);
    const bool has = a.w & FT_HAS, lasth = has && (a.w & FT_LAST_HDR);
    const unsigned long long hm = __ballot(has), lm = __ballot(lasth);
    if (lane == 0) ws[w] = hm ? (1u | ((uint32_t)((lm >> (63 - __clzll(hm))) & 1ull) << 1)) : 0u;
    __syncthreads();
    uint32_t win = carry, wout = carry;
    for (int i = 0; i < NW; ++i) {
      const uint32_t s = ws[i];
      if (i < w) win = fa_fold(win, s);
      wout = fa_fold(wout, s);
    }
    const unsigned long long below = hm & ((1ull << lane) - 1ull);
    uint32_t cin = win;
    if (below) cin = 1u | ((uint32_t)((lm >> (63 - __clzll(below))) & 1ull) << 1);
    const uint32_t chdr = (cin & 1u) & (cin >> 1);
    carry = wout;
    if (COMPAT && has && chdr && (a.w & FT_FIRST_HDR)) {
      atomicOr((unsigned long long *)&words[FW_FLAGS], (unsigned long long)FE_EMPTY);
      atomicMin((unsigned long long *)&words[FW_OFF_EMPTY], (unsigned long long)(t * (uint64_t)FA_TILE + (a.w >> 8)));
    }
    if (!COMPAT && !chdr && (a.x >> 16)) {               // an over-long '\r' run in front of the tile's first line start: a sequence line
      atomicOr((unsigned long long *)&words[FW_FLAGS], (unsigned long long)FE_CR_RUN);
      atomicMin((unsigned long long *)&words[FW_OFF_CR], (unsigned long long)(t * (uint64_t)FA_TILE + (a.x >> 16) - 1u));
    }
    const uint32_t e = a.y + (chdr ? 0u : (a.x & 0xFFFFu)), h = a.z;
    const uint32_t ie = dev_wave_scan_incl(e), ih = dev_wave_scan_incl(h);
    if (lane == 63) { se[w] = ie; sh[w] = ih; }
    __syncthreads();
    uint32_t pe = 0, ph = 0, te = 0, th = 0;
    for (int i = 0; i < NW; ++i) {
      if (i < w) { pe += se[i]; ph += sh[i]; }
      te += se[i]; th += sh[i];
    }
    if (t < ntiles) out[t] = make_ulonglong2(base_e + pe + ie - e, (base_h + ph + ih - h) | (chdr ? FA_CARRY_BIT : 0ull));
    base_e += te; base_h += th;
    __syncthreads();       // (ws / se / sh are written again by the next block)
  }
  if (threadIdx.x == 0) {
    words[FW_EMIT] = base_e;
    words[FW_NHDR] = base_h;
    if (COMPAT && n > 0 && (carry & 3u) == 3u) {       // the text ends on a header line
      atomicOr((unsigned long long *)&words[FW_FLAGS], (unsigned long long)FE_EMPTY);
      atomicMin((unsigned long long *)&words[FW_OFF_EMPTY], (unsigned long long)n);
    }
  }
}

template <bool COMPAT>
__global__ __launch_bounds__(FA_THREADS) void fa_scatter_kernel(const uint8_t *__restrict__ text, uint64_t n, const ulonglong2 *__restrict__ pre,
                                                                uint64_t *__restrict__ words, int8_t *__restrict__ data, int64_t *__restrict__ start) {
  __shared__ uint32_t ws[2][FA_THREADS / 64];
  __shared__ uint32_t wsum[FA_THREADS / 64];
  __shared__ __attribute__((aligned(16))) uint8_t stage[FA_ITER_BYTES + 16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t tile = blockIdx.x, base = tile * (uint64_t)FA_TILE;
  const ulonglong2 pr = pre[tile];
  uint64_t ebase = pr.x, hbase = pr.y & ~FA_CARRY_BIT;
  uint32_t carry = 1u | ((pr.y & FA_CARRY_BIT) ? 2u : 0u);
  for (int it = 0; it < FA_ITERS; ++it) {
    const uint64_t p0 = base + (uint64_t)it * FA_ITER_BYTES + (uint64_t)threadIdx.x * 16;
    if (base + (uint64_t)it * FA_ITER_BYTES >= n) break;
    FaLane L;
    fa_classify(text, p0, n, L, ws[it & 1]);
    __syncthreads();
    carry = fa_finish<COMPAT>(text, p0, n, L, ws[it & 1], carry, nullptr, nullptr, 0u);
    // exclusive emit / header counts of the lane inside these 4096 bytes (<= 4096 and <= 2048: 16 bits each)
    const uint32_t mine = (uint32_t)__popc(L.emit) | ((uint32_t)__popc(L.Hd) << 16);
    const uint32_t incl = dev_wave_scan_incl(mine);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint32_t excl = incl - mine, total = 0;
#pragma unroll
    for (int i = 0; i < FA_THREADS / 64; ++i) {
      const uint32_t s = wsum[i];
      if (i < w) excl += s;
      total += s;
    }
    const uint32_t le = excl & 0xFFFFu, lh = excl >> 16, te = total & 0xFFFFu, th = total >> 16;
    // the codes into LDS at the alignment they have in `data`
    const uint32_t off0 = (uint32_t)((uintptr_t)(data + ebase) & 15u);
    const uint32_t c0 = fa_code4(L.v.x), c1 = fa_code4(L.v.y), c2 = fa_code4(L.v.z), c3 = fa_code4(L.v.w);
    uint8_t *dst = stage + off0 + le;
    if (L.emit == 0xFFFFu) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uint32_t cw = j < 4 ? c0 : j < 8 ? c1 : j < 12 ? c2 : c3;
        dst[j] = (uint8_t)(cw >> (8 * (j & 3)));
      }
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uint32_t cw = j < 4 ? c0 : j < 8 ? c1 : j < 12 ? c2 : c3;
        if ((L.emit >> j) & 1u) dst[__popc(L.emit & ((1u << j) - 1u))] = (uint8_t)(cw >> (8 * (j & 3)));
      }
    }
    for (uint32_t hmask = L.Hd; hmask; hmask &= hmask - 1u) {
      const int j = __ffs(hmask) - 1;
      const uint32_t lowbits = (1u << j) - 1u;
      const uint64_t r = hbase + lh + (uint32_t)__popc(L.Hd & lowbits);
      start[r] = (int64_t)(ebase + le + (uint32_t)__popc(L.emit & lowbits) + ((!COMPAT && p0 + (uint64_t)j > 0) ? 1u : 0u));
    }
    __syncthreads();
    // LDS -> data: whole aligned 16-byte blocks, bytes at the two ends (the neighbours' bytes share those blocks)
    int8_t *g0 = data + ebase - off0;
    const uint32_t end = off0 + te;
    for (uint32_t b = threadIdx.x * 16; b < end; b += FA_THREADS * 16) {
      if (b >= off0 && b + 16 <= end) {
        *reinterpret_cast<uint4 *>(g0 + b) = *reinterpret_cast<const uint4 *>(stage + b);
      } else {
        for (uint32_t i = b; i < b + 16; ++i)
          if (i >= off0 && i < end) g0[i] = (int8_t)stage[i];
      }
    }
    ebase += te; hbase += th;
    // (no barrier here: the next stage[] writes come behind two more barriers, wsum's behind one)
  }
}

template <bool COMPAT>
__global__ __launch_bounds__(256) void fa_length_kernel(const int64_t *__restrict__ start, int64_t nN, int64_t nS, int8_t *__restrict__ data,
                                                        int32_t *__restrict__ length, uint64_t *__restrict__ words) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nS) return;
  const int64_t s = start[r], e = (r + 1 < nS) ? start[r + 1] : nN;
  int64_t len = e - s - 1;
  if (len > 0x7FFFFFFFll) {
    atomicOr((unsigned long long *)&words[FW_FLAGS], (unsigned long long)FE_LONG);
    atomicMin((unsigned long long *)&words[FW_REC_LONG], (unsigned long long)r);
    len = 0x7FFFFFFFll;
  }
  if (len < 0) len = 0;        // (an empty compat record: refused before this kernel is launched)
  length[r] = (int32_t)len;
  if (e - 1 >= 0 && e - 1 < nN) data[e - 1] = (int8_t)-1;   // the terminator: in compat mode the record's last contributed byte
}

constexpr size_t FA_WORDS_BYTES = 64;
size_t fa_pool_bytes(uint64_t ntiles) { return FA_WORDS_BYTES + (size_t)ntiles * 32; }

struct FaPlan { uint64_t *words; uint4 *agg; ulonglong2 *pre; uint64_t ntiles; };

int fa_plan(cfrk_ctx *ctx, uint64_t nbytes, FaPlan *pl) {
  pl->ntiles = (nbytes + FA_TILE - 1) / FA_TILE;
  void *p;
  const int rc = cfrk_pool_get(ctx, BUF_FASTA, fa_pool_bytes(pl->ntiles), &p);
  if (rc) return rc;
  pl->words = (uint64_t *)p;
  pl->agg = (uint4 *)((char *)p + FA_WORDS_BYTES);
  pl->pre = (ulonglong2 *)((char *)p + FA_WORDS_BYTES + (size_t)pl->ntiles * 16);
  return CFRK_OK;
}

// reduce + scan, the totals and the error words read back (synchronises).  nbytes >= 1.
int fa_measure(cfrk_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, bool compat, const FaPlan &pl, int64_t *nN, int64_t *nS) {
  HIP_TRY(ctx, hipMemsetAsync(pl.words, 0, FW_OFF_EMPTY * 8, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(pl.words + FW_OFF_EMPTY, 0xFF, (FW_NWORDS - FW_OFF_EMPTY) * 8, ctx->stream));
  if (compat) {
    hipLaunchKernelGGL(fa_reduce_kernel<true>, dim3((unsigned)pl.ntiles), dim3(FA_THREADS), 0, ctx->stream, d_text, nbytes, pl.words, pl.agg);
    hipLaunchKernelGGL(fa_scan_kernel<true>, dim3(1), dim3(FA_SCAN), 0, ctx->stream, pl.agg, pl.ntiles, nbytes, pl.words, pl.pre);
  } else {
    hipLaunchKernelGGL(fa_reduce_kernel<false>, dim3((unsigned)pl.ntiles), dim3(FA_THREADS), 0, ctx->stream, d_text, nbytes, pl.words, pl.agg);
    hipLaunchKernelGGL(fa_scan_kernel<false>, dim3(1), dim3(FA_SCAN), 0, ctx->stream, pl.agg, pl.ntiles, nbytes, pl.words, pl.pre);
  }
  HIP_TRY(ctx, hipGetLastError());
  uint64_t wd[FW_NWORDS];
  HIP_TRY(ctx, hipMemcpyAsync(wd, pl.words, sizeof wd, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  // (the `cfrk` command recognises this cause by the words "before the first header": cfrk_cli.cpp, DeviceText::load;
  //  tests/test_gpu_ingest.py pins them)
  if (wd[FW_FLAGS] & FE_NO_HEADER)
    return cfrk_fail(ctx, CFRK_ERR_LAYOUT, "FASTA: a sequence line before the first header (byte offset 0)");
  if (wd[FW_FLAGS] & FE_CR_RUN)
    return cfrk_fail(ctx, CFRK_ERR_LAYOUT, "FASTA: more than %d carriage returns in a row in a sequence line, from byte offset %llu", CFRK_FASTA_MAX_CR_RUN,
                     (unsigned long long)wd[FW_OFF_CR]);
  if (wd[FW_FLAGS] & FE_EMPTY)
    return cfrk_fail(ctx, CFRK_ERR_LAYOUT, "FASTA: a header without a sequence line (the record ends at byte offset %llu)",
                     (unsigned long long)wd[FW_OFF_EMPTY]);
  *nS = (int64_t)wd[FW_NHDR];
  *nN = compat ? (int64_t)wd[FW_EMIT] : (*nS ? (int64_t)wd[FW_EMIT] + 1 : 0);
  return CFRK_OK;
}

// scatter + lengths, left enqueued -- unless a record could be over-long (text of 2^31 bytes or more): then the error
// word of the length pass is read back
int fa_emit(cfrk_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, bool compat, const FaPlan &pl, int8_t *d_data, int64_t *d_start,
            int32_t *d_length, int64_t nN, int64_t nS) {
  const unsigned lgrid = (unsigned)((nS + 255) / 256);
  if (compat) {
    hipLaunchKernelGGL(fa_scatter_kernel<true>, dim3((unsigned)pl.ntiles), dim3(FA_THREADS), 0, ctx->stream, d_text, nbytes, pl.pre, pl.words, d_data, d_start);
    hipLaunchKernelGGL(fa_length_kernel<true>, dim3(lgrid), dim3(256), 0, ctx->stream, d_start, nN, nS, d_data, d_length, pl.words);
  } else {
    hipLaunchKernelGGL(fa_scatter_kernel<false>, dim3((unsigned)pl.ntiles), dim3(FA_THREADS), 0, ctx->stream, d_text, nbytes, pl.pre, pl.words, d_data, d_start);
    hipLaunchKernelGGL(fa_length_kernel<false>, dim3(lgrid), dim3(256), 0, ctx->stream, d_start, nN, nS, d_data, d_length, pl.words);
  }
  HIP_TRY(ctx, hipGetLastError());
  if (nbytes > 0x7FFFFFFFull) {
    uint64_t wd[FW_NWORDS];
    HIP_TRY(ctx, hipMemcpyAsync(wd, pl.words, sizeof wd, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (wd[FW_FLAGS] & FE_LONG)
      return cfrk_fail(ctx, CFRK_ERR_LAYOUT, "FASTA: record %llu is longer than 2^31 - 1 bases", (unsigned long long)wd[FW_REC_LONG]);
  }
  return CFRK_OK;
}

// measure, refuse or place the outputs, emit: what both forms run on device text (the callers plan)
int fa_core(cfrk_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, int flags, const FaPlan &pl, ReadsOut *o, int64_t *nN_out, int64_t *nS_out) {
  const bool compat = (flags & CFRK_COMPAT) != 0;
  int64_t nN = 0, nS = 0;
  int rc = fa_measure(ctx, d_text, nbytes, compat, pl, &nN, &nS);
  if (rc || (rc = reads_out_fit(ctx, "FASTA", *o, nN, nS, nN_out, nS_out)) || (rc = reads_out_carve(ctx, o, nN, nS))) return rc;
  return fa_emit(ctx, d_text, nbytes, compat, pl, o->data, o->start, o->length, nN, nS);
}

int fa_check(cfrk_ctx *ctx, const void *text, uint64_t nbytes, int flags, const void *data, uint64_t cap_data, const void *start,
             const void *length, uint64_t cap_reads, int64_t *nN_out, int64_t *nS_out) {
  if (!ctx) return CFRK_ERR_ARG;
  if (flags & ~CFRK_COMPAT) return cfrk_fail(ctx, CFRK_ERR_ARG, "flags 0x%x: the FASTA parser takes CFRK_COMPAT only", flags);
  return parse_check(ctx, text, nbytes, data, cap_data, start, length, cap_reads, nN_out, nS_out);
}

}  // namespace

extern "C" int cfrk_fasta_parse_device(cfrk_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, int flags, int8_t *d_data, uint64_t cap_data,
                                       int64_t *d_start, int32_t *d_length, uint64_t cap_reads, int64_t *nN_out, int64_t *nS_out) {
  int rc = fa_check(ctx, d_text, nbytes, flags, d_data, cap_data, d_start, d_length, cap_reads, nN_out, nS_out);
  if (rc || nbytes == 0) return rc;
  if (((uintptr_t)d_text & 15) != 0) return cfrk_fail(ctx, CFRK_ERR_ALIGN, "d_text %p", (const void *)d_text);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  FaPlan pl;
  if ((rc = fa_plan(ctx, nbytes, &pl))) return rc;
  ReadsOut o = {d_data, d_start, d_length, nullptr, cap_data, cap_reads, -1, false};
  return fa_core(ctx, d_text, nbytes, flags, pl, &o, nN_out, nS_out);
}

extern "C" int cfrk_fasta_parse(cfrk_ctx *ctx, const char *text, uint64_t nbytes, int flags, int8_t *data, uint64_t cap_data, int64_t *start,
                                int32_t *length, uint64_t cap_reads, int64_t *nN_out, int64_t *nS_out) {
  int rc = fa_check(ctx, text, nbytes, flags, data, cap_data, start, length, cap_reads, nN_out, nS_out);
  if (rc || nbytes == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  FaPlan pl;
  void *d_text;
  if ((rc = fa_plan(ctx, nbytes, &pl)) || (rc = cfrk_pool_get(ctx, BUF_FASTA_IN, (size_t)nbytes + 16, &d_text))) return rc;   // (every slot before the copy)
  HIP_TRY(ctx, hipMemcpyAsync(d_text, text, (size_t)nbytes, hipMemcpyHostToDevice, ctx->stream));
  ReadsOut o = {nullptr, nullptr, nullptr, nullptr, cap_data, cap_reads, BUF_FASTA_OUT, false};
  if ((rc = fa_core(ctx, (const uint8_t *)d_text, nbytes, flags, pl, &o, nN_out, nS_out))) return stage_drain(ctx, rc);
  return download_reads(ctx, o, data, start, length, nullptr, *nN_out, *nS_out);
}
