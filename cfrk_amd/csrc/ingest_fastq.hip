// ingest_fastq.hip -- strict four-line FASTQ text in device memory -> the struct-read layout (data / start / length),
// byte for byte what cfrk_host_parse_fastq (cfrk_amd/host/cfrk_host.cpp) produces; the grammar is in cfrk_abi.h.
// The same memory-bound compaction as ingest.hip (classify, scan, scatter through LDS), with another carry.
//
// A byte's line is the number of '\n' in front of it, its CLASS that number mod 4: 0 the '@' line, 1 the sequence line,
// 2 the '+' line, 3 the quality line.  A byte is KEPT unless it is a '\n', a '\r' directly in front of a '\n' or a '\r'
// that ends the text.  Every byte of the text EMITS one byte of `data` or nothing, in text order without gaps:
//   a kept byte of a class-1 line emits its code; the '\n' that ends a class-1 line emits the record's terminator (its
//   code is -1 anyway; in a text of whole records every sequence line has its '\n': two more lines follow it).
// So a byte's place in `data` is the number of emitting bytes before it, and start[r] is that number at the '\n' that
// ends record r's '@' line.  A tile does not know its phase (newlines before it, mod 4) in the reduce pass: it counts
// its kept bytes per LOCAL class (newlines before the byte inside the tile, mod 4) and notes, per local class, the first
// line start that is not '@' and the first that is not '+'; the scan, which carries the phase, picks the local classes
// that are the sequence / quality / '@' / '+' lines of that tile.  The newlines of a local class follow from the tile's
// newline count alone (newline j of the tile ends a line of local class j mod 4).
//
// Launches, all on the context stream, no workgroup ever waits for another one:
//   fq_reduce_kernel  one workgroup per tile of CFRK_FASTQ_TILE_BYTES: kept bytes per local class, newlines, the first
//                     line start per local class that is not '@' / not '+'
//   fq_scan_kernel    ONE workgroup walks the tile aggregates in blocks of CFRK_FASTQ_SCAN_TILES: exclusive newline,
//                     emit and kept-quality counts per tile, the totals, the earliest structural fault
//   -- the host reads the totals and the error words back (first synchronisation), checks structure and capacities;
//      on a structural fault fq_line_kernel counts the newlines in front of the faulty line start for the message --
//   fq_scatter_kernel re-reads the text, compacts the codes of 4096 bytes through LDS and writes them with 16-byte
//                     stores; the thread on the '\n' of an '@' line writes start[r]; the thread on an '@' line's first
//                     byte compares the sequence and quality bytes kept so far (the length check)
//   fq_mask_kernel    (min_qual > 0) the same walk with the quality class in place of the sequence class: the quality
//                     byte of record r with Eq kept quality bytes before it belongs to data[Eq + r]; a byte store of -1
//                     where the quality is low
//   fq_length_kernel  length[r] = next start (or nN) - start[r] - 1, the over-long check
//   -- the host reads the error words back (second synchronisation): the length check's verdict --
#include "common.h"
#include "ingest_bytes.h"
#include "staging.h"

#include <algorithm>

namespace {

constexpr int FQ_THREADS = 256;
constexpr int FQ_WAVES = FQ_THREADS / 64;
constexpr int FQ_ITER_BYTES = FQ_THREADS * 16;
constexpr int FQ_TILE = CFRK_FASTQ_TILE_BYTES;
constexpr int FQ_ITERS = FQ_TILE / FQ_ITER_BYTES;
constexpr int FQ_SCAN = CFRK_FASTQ_SCAN_TILES;
static_assert(FQ_TILE % FQ_ITER_BYTES == 0 && FQ_TILE < 65535, "a tile is whole iterations; counts and offsets inside it take 16 bits");
static_assert(FQ_SCAN % 64 == 0 && FQ_SCAN <= 1024 && (int64_t)FQ_SCAN * FQ_TILE * 2 < ((int64_t)1 << 31), "the block sums are 32-bit");
static_assert(CFRK_FASTQ_QUAL_BASE + CFRK_FASTQ_MAX_QUAL <= 126, "fq_lt16 compares seven bits");

// device words of a parse (uint64 each), in front of the tile aggregates: the first FQ_W_ONES start as 0, the rest as ~0
enum { FQ_W_EMIT = 0, FQ_W_QKEPT, FQ_W_NL, FQ_W_OPEN_END, FQ_W_LONG, FQ_W_LINE, FQ_W_ONES = 8,
       FQ_W_BAD_OFF = 8, FQ_W_REC_DIFF, FQ_W_REC_LONG, FQ_NWORDS = 16 };
constexpr uint32_t FQ_NONE = 0xFFFFu;

// tile aggregate, two uint4:  a.x = K0 | K1 << 16, a.y = K2 | K3 << 16 (kept bytes per local class), a.z = newlines;
// b.x / b.y = first line start of local class 0 | 1 << 16, 2 | 3 << 16 that is not '@', b.z / b.w = that is not '+' (FQ_NONE: none)
__device__ __forceinline__ uint32_t fq_half(uint32_t lo, uint32_t hi, uint32_t c) { return (((c & 2u) ? hi : lo) >> ((c & 1u) * 16)) & 0xFFFFu; }
// newlines of local class c among the nl newlines of a tile
__device__ __forceinline__ uint32_t fq_class_newlines(uint32_t nl, uint32_t c) { return nl > c ? (nl - c + 3u) >> 2 : 0u; }

struct FqLane {
  uint4 v;             // the text bytes
  uint32_t valid;      // bytes inside the text
  uint32_t nl;         // '\n'
  uint32_t kept;       // neither '\n' nor a dropped '\r'
  uint32_t c0, c1;     // the two bits of each byte's class
  uint32_t excl_nl;    // newlines of this iteration's 4096 bytes in front of the lane
  uint32_t total_nl;   // newlines of this iteration's 4096 bytes
};

__device__ __forceinline__ uint32_t fq_prefix_xor16(uint32_t x) {
  x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8;
  return x & 0xFFFFu;
}

// load and classify a lane's 16 bytes; ws = FQ_WAVES words of LDS for the waves' newline counts.  Holds one barrier.
// phase = newlines in front of these 4096 bytes (mod 4 is all that matters).
__device__ __forceinline__ void fq_lane(const uint8_t *__restrict__ text, uint64_t p0, uint64_t n, uint32_t phase, FqLane &L, uint32_t *ws) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  L.v = fa_load(text, p0, n, L.valid);
  L.nl = fa_eq16(L.v, 0x0A0A0A0Au) & L.valid;
  const uint32_t cr = fa_eq16(L.v, 0x0D0D0D0Du) & L.valid;
  uint32_t drop = L.nl >> 1;                                       // a '\r' directly in front of a '\n' ...
  if (p0 < n && n - p0 <= 16) drop |= 1u << (int)(n - p0 - 1);     // ... or as the text's last byte
  if ((cr >> 15) && p0 + 16 < n) drop |= (uint32_t)(text[p0 + 16] == '\n') << 15;
  L.kept = L.valid & ~L.nl & ~(cr & drop);
  const uint32_t cnt = (uint32_t)__popc(L.nl);
  const uint32_t incl = dev_wave_scan_incl(cnt);
  if (lane == 63) ws[w] = incl;
  __syncthreads();
  uint32_t excl = incl - cnt, total = 0;
#pragma unroll
  for (int i = 0; i < FQ_WAVES; ++i) {
    const uint32_t s = ws[i];
    if (i < w) excl += s;
    total += s;
  }
  L.excl_nl = excl; L.total_nl = total;
  // newlines in front of each byte, mod 4: bit 0 is the parity of the newlines before it, bit 1 flips wherever that
  // count becomes even; then the lane's own phase is added (two-bit add)
  const uint32_t cin = (phase + excl) & 3u;
  const uint32_t x = (L.nl << 1) & 0xFFFFu;
  const uint32_t b0 = fq_prefix_xor16(x);
  const uint32_t b1 = fq_prefix_xor16(x & ~b0);
  const uint32_t m0 = (cin & 1u) ? 0xFFFFu : 0u, m1 = (cin & 2u) ? 0xFFFFu : 0u;
  L.c0 = b0 ^ m0;
  L.c1 = (b1 ^ m1 ^ (b0 & m0)) & 0xFFFFu;
}
__device__ __forceinline__ uint32_t fq_class_mask(const FqLane &L, uint32_t c) {
  return ((c & 1u) ? L.c0 : ~L.c0) & ((c & 2u) ? L.c1 : ~L.c1) & 0xFFFFu;
}
// line starts among the lane's bytes (inside the text: a trailing '\n' opens no line)
__device__ __forceinline__ uint32_t fq_line_starts(const uint8_t *__restrict__ text, uint64_t p0, uint64_t n, const FqLane &L) {
  uint32_t prev = dev_lane_prev(L.nl >> 15);
  if ((threadIdx.x & 63) == 0) prev = (p0 == 0) ? 1u : (p0 < n ? (uint32_t)(text[p0 - 1] == '\n') : 0u);
  return ((L.nl << 1) | prev) & L.valid;
}

__global__ __launch_bounds__(FQ_THREADS) void fq_reduce_kernel(const uint8_t *__restrict__ text, uint64_t n, uint4 *__restrict__ agg) {
  __shared__ uint32_t ws[2][FQ_WAVES];
  __shared__ uint32_t red[12];       // kept bytes per local class; first line start per local class that is not '@' (4..7), not '+' (8..11)
  const uint64_t tile = blockIdx.x, base = tile * (uint64_t)FQ_TILE;
  if (threadIdx.x < 4) red[threadIdx.x] = 0;
  else if (threadIdx.x < 12) red[threadIdx.x] = FQ_NONE;
  uint32_t run_nl = 0, k0 = 0, k1 = 0, k2 = 0, k3 = 0;
  for (int it = 0; it < FQ_ITERS; ++it) {
    if (base + (uint64_t)it * FQ_ITER_BYTES >= n) break;
    const uint32_t off = (uint32_t)(it * FQ_ITER_BYTES + threadIdx.x * 16);
    const uint64_t p0 = base + off;
    FqLane L;
    fq_lane(text, p0, n, run_nl, L, ws[it & 1]);       // (behind its barrier red[] is initialised as well)
    const uint32_t is0 = fq_class_mask(L, 0), is1 = fq_class_mask(L, 1), is2 = fq_class_mask(L, 2), is3 = fq_class_mask(L, 3);
    k0 += __popc(L.kept & is0); k1 += __popc(L.kept & is1); k2 += __popc(L.kept & is2); k3 += __popc(L.kept & is3);
    const uint32_t S = fq_line_starts(text, p0, n, L);
    if (S) {
      const uint32_t not_at = S & ~fa_eq16(L.v, 0x40404040u), not_plus = S & ~fa_eq16(L.v, 0x2B2B2B2Bu);
#pragma unroll
      for (uint32_t c = 0; c < 4; ++c) {
        const uint32_t isc = c == 0 ? is0 : c == 1 ? is1 : c == 2 ? is2 : is3;
        if (not_at & isc) atomicMin(&red[4 + c], off + (uint32_t)__ffs(not_at & isc) - 1u);
        if (not_plus & isc) atomicMin(&red[8 + c], off + (uint32_t)__ffs(not_plus & isc) - 1u);
      }
    }
    run_nl += L.total_nl;
  }
  const uint32_t s0 = dev_wave_scan_incl(k0), s1 = dev_wave_scan_incl(k1), s2 = dev_wave_scan_incl(k2), s3 = dev_wave_scan_incl(k3);
  if ((threadIdx.x & 63) == 63) {
    if (s0) atomicAdd(&red[0], s0);
    if (s1) atomicAdd(&red[1], s1);
    if (s2) atomicAdd(&red[2], s2);
    if (s3) atomicAdd(&red[3], s3);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    agg[2 * tile] = make_uint4(red[0] | (red[1] << 16), red[2] | (red[3] << 16), run_nl, 0u);
    agg[2 * tile + 1] = make_uint4(red[4] | (red[5] << 16), red[6] | (red[7] << 16), red[8] | (red[9] << 16), red[10] | (red[11] << 16));
  }
}

// one workgroup of FQ_SCAN threads: tile t of a block is thread t's.  pre[3 t ..] = exclusive emit, kept-quality and newline counts
__global__ __launch_bounds__(FQ_SCAN) void fq_scan_kernel(const uint8_t *__restrict__ text, uint64_t n, const uint4 *__restrict__ agg, uint64_t ntiles,
                                                          uint64_t *__restrict__ words, uint64_t *__restrict__ pre) {
  constexpr int NW = FQ_SCAN / 64;
  __shared__ uint32_t sn[NW], se[NW], sq[NW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t base_n = 0, base_e = 0, base_q = 0;
  for (uint64_t b0 = 0; b0 < ntiles; b0 += FQ_SCAN) {
    const uint64_t t = b0 + threadIdx.x;
    const bool in = t < ntiles;
    const uint4 a = in ? agg[2 * t] : make_uint4(0, 0, 0, 0);
    const uint4 b = in ? agg[2 * t + 1] : make_uint4(~0u, ~0u, ~0u, ~0u);
    const uint32_t nl = a.z;
    const uint32_t in_n = dev_wave_scan_incl(nl);
    if (lane == 63) sn[w] = in_n;
    __syncthreads();
    uint32_t pn = 0, tn = 0;
    for (int i = 0; i < NW; ++i) {
      if (i < w) pn += sn[i];
      tn += sn[i];
    }
    const uint64_t nl_before = base_n + pn + in_n - nl;
    const uint32_t phase = (uint32_t)nl_before & 3u;
    // local class c is the class (c + phase) mod 4 of the text
    const uint32_t l_at = (0u - phase) & 3u, l_seq = (1u - phase) & 3u, l_plus = (2u - phase) & 3u, l_qual = (3u - phase) & 3u;
    const uint32_t bad = min(fq_half(b.x, b.y, l_at), fq_half(b.z, b.w, l_plus));
    if (bad != FQ_NONE) atomicMin((unsigned long long *)&words[FQ_W_BAD_OFF], (unsigned long long)(t * (uint64_t)FQ_TILE + bad));
    const uint32_t e = fq_half(a.x, a.y, l_seq) + fq_class_newlines(nl, l_seq), q = fq_half(a.x, a.y, l_qual);
    const uint32_t ie = dev_wave_scan_incl(e), iq = dev_wave_scan_incl(q);
    if (lane == 63) { se[w] = ie; sq[w] = iq; }
    __syncthreads();
    uint32_t pe = 0, pq = 0, te = 0, tq = 0;
    for (int i = 0; i < NW; ++i) {
      if (i < w) { pe += se[i]; pq += sq[i]; }
      te += se[i]; tq += sq[i];
    }
    if (in) {
      pre[3 * t] = base_e + pe + ie - e;
      pre[3 * t + 1] = base_q + pq + iq - q;
      pre[3 * t + 2] = nl_before;
    }
    base_n += tn; base_e += te; base_q += tq;
    __syncthreads();       // (sn / se / sq are written again by the next block)
  }
  if (threadIdx.x == 0) {
    words[FQ_W_EMIT] = base_e;
    words[FQ_W_QKEPT] = base_q;
    words[FQ_W_NL] = base_n;
    words[FQ_W_OPEN_END] = (n > 0 && text[n - 1] != '\n') ? 1u : 0u;
  }
}

// the newlines in front of byte `off` = those in front of its tile + those of the tile in front of it: the line number of a faulty line start
__global__ __launch_bounds__(FQ_THREADS) void fq_line_kernel(const uint8_t *__restrict__ text, uint64_t off, const uint64_t *__restrict__ pre,
                                                             uint64_t *__restrict__ words) {
  const uint64_t tile = off / FQ_TILE, base = tile * (uint64_t)FQ_TILE;
  uint32_t c = 0;
  for (uint64_t p = base + threadIdx.x; p < off; p += FQ_THREADS) c += (uint32_t)(text[p] == '\n');
  const uint32_t s = dev_wave_scan_incl(c);
  if ((threadIdx.x & 63) == 63 && s) atomicAdd((unsigned long long *)&words[FQ_W_LINE], (unsigned long long)s);
  if (threadIdx.x == 0) atomicAdd((unsigned long long *)&words[FQ_W_LINE], (unsigned long long)pre[3 * tile + 2]);
}

__global__ __launch_bounds__(FQ_THREADS) void fq_scatter_kernel(const uint8_t *__restrict__ text, uint64_t n, const uint64_t *__restrict__ pre,
                                                                uint64_t *__restrict__ words, int8_t *__restrict__ data, int64_t *__restrict__ start,
                                                                uint64_t nN, uint64_t nS) {
  __shared__ uint32_t wn[FQ_WAVES];
  __shared__ uint32_t wsum[FQ_WAVES];
  __shared__ __attribute__((aligned(16))) uint8_t stage[FQ_ITER_BYTES + 16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t tile = blockIdx.x, base = tile * (uint64_t)FQ_TILE;
  uint64_t ebase = pre[3 * tile], qbase = pre[3 * tile + 1], nbase = pre[3 * tile + 2];
  for (int it = 0; it < FQ_ITERS; ++it) {
    if (base + (uint64_t)it * FQ_ITER_BYTES >= n) break;
    const uint64_t p0 = base + (uint64_t)it * FQ_ITER_BYTES + (uint64_t)threadIdx.x * 16;
    FqLane L;
    fq_lane(text, p0, n, (uint32_t)nbase & 3u, L, wn);
    const uint32_t is0 = fq_class_mask(L, 0);
    const uint32_t emit = (L.kept | L.nl) & fq_class_mask(L, 1), qk = L.kept & fq_class_mask(L, 3);
    // exclusive emit / kept-quality counts of the lane inside these 4096 bytes (<= 4096 each: 16 bits)
    const uint32_t mine = (uint32_t)__popc(emit) | ((uint32_t)__popc(qk) << 16);
    const uint32_t incl = dev_wave_scan_incl(mine);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint32_t excl = incl - mine, total = 0;
#pragma unroll
    for (int i = 0; i < FQ_WAVES; ++i) {
      const uint32_t s = wsum[i];
      if (i < w) excl += s;
      total += s;
    }
    const uint32_t le = excl & 0xFFFFu, lq = excl >> 16, te = total & 0xFFFFu, tq = total >> 16;
    // the codes into LDS at the alignment they have in `data`
    const uint32_t off0 = (uint32_t)((uintptr_t)(data + ebase) & 15u);
    const uint32_t c0 = fa_code4(L.v.x), c1 = fa_code4(L.v.y), c2 = fa_code4(L.v.z), c3 = fa_code4(L.v.w);
    uint8_t *dst = stage + off0 + le;
    if (emit == 0xFFFFu) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uint32_t cw = j < 4 ? c0 : j < 8 ? c1 : j < 12 ? c2 : c3;
        dst[j] = (uint8_t)(cw >> (8 * (j & 3)));
      }
    } else if (emit) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uint32_t cw = j < 4 ? c0 : j < 8 ? c1 : j < 12 ? c2 : c3;
        if ((emit >> j) & 1u) dst[__popc(emit & ((1u << j) - 1u))] = (uint8_t)(cw >> (8 * (j & 3)));
      }
    }
    // the '\n' of an '@' line: the record's codes begin behind the bytes emitted so far
    for (uint32_t m = L.nl & is0; m; m &= m - 1u) {
      const uint32_t low = (m & (0u - m)) - 1u;
      const uint64_t r = (nbase + L.excl_nl + (uint32_t)__popc(L.nl & low)) >> 2;
      if (r < nS) start[r] = (int64_t)(ebase + le + (uint32_t)__popc(emit & low));
    }
    // the first byte of an '@' line: r whole records lie in front of it, their sequence and quality lines kept the
    // same number of bytes each if and only if the two running counts agree here (the emits count r terminators)
    for (uint32_t m = fq_line_starts(text, p0, n, L) & is0; m; m &= m - 1u) {
      const uint32_t low = (m & (0u - m)) - 1u;
      const uint64_t r = (nbase + L.excl_nl + (uint32_t)__popc(L.nl & low)) >> 2;
      const uint64_t eb = ebase + le + (uint32_t)__popc(emit & low), qb = qbase + lq + (uint32_t)__popc(qk & low);
      if (r > 0 && eb - r != qb) atomicMin((unsigned long long *)&words[FQ_W_REC_DIFF], (unsigned long long)(r - 1));
    }
    __syncthreads();
    // LDS -> data: whole aligned 16-byte blocks, bytes at the two ends (the neighbours' bytes share those blocks);
    // never past nN (in a text of whole records the counts add up to it)
    const uint64_t room = ebase < nN ? nN - ebase : 0;
    int8_t *g0 = data + ebase - off0;
    const uint32_t end = off0 + (room < te ? (uint32_t)room : te);
    for (uint32_t b = threadIdx.x * 16; b < end; b += FQ_THREADS * 16) {
      if (b >= off0 && b + 16 <= end) {
        *reinterpret_cast<uint4 *>(g0 + b) = *reinterpret_cast<const uint4 *>(stage + b);
      } else {
        for (uint32_t i = b; i < b + 16; ++i)
          if (i >= off0 && i < end) g0[i] = (int8_t)stage[i];
      }
    }
    ebase += te; qbase += tq; nbase += L.total_nl;
    // (no barrier here: the next stage[] writes come behind two more barriers, wn's behind this one, wsum's behind one more)
  }
}

// 16 bytes -> 16 bits: byte < t, for 2 <= t <= 127 (a byte of 128 or more is not below)
__device__ __forceinline__ uint32_t fq_lt4(uint32_t w, uint32_t add) {      // add = (128 - t) in every byte
  const uint32_t f = ~((w & 0x7F7F7F7Fu) + add) & ~w & 0x80808080u;
  return ((f >> 7) * 0x01020408u) >> 24;
}
__device__ __forceinline__ uint32_t fq_lt16(uint4 v, uint32_t t) {
  const uint32_t add = (128u - t) * 0x01010101u;
  return fq_lt4(v.x, add) | (fq_lt4(v.y, add) << 4) | (fq_lt4(v.z, add) << 8) | (fq_lt4(v.w, add) << 12);
}

__global__ __launch_bounds__(FQ_THREADS) void fq_mask_kernel(const uint8_t *__restrict__ text, uint64_t n, const uint64_t *__restrict__ pre,
                                                             uint32_t threshold, int8_t *__restrict__ data, uint64_t nN) {
  __shared__ uint32_t wn[FQ_WAVES];
  __shared__ uint32_t wsum[FQ_WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t tile = blockIdx.x, base = tile * (uint64_t)FQ_TILE;
  uint64_t qbase = pre[3 * tile + 1], nbase = pre[3 * tile + 2];
  for (int it = 0; it < FQ_ITERS; ++it) {
    if (base + (uint64_t)it * FQ_ITER_BYTES >= n) break;
    const uint64_t p0 = base + (uint64_t)it * FQ_ITER_BYTES + (uint64_t)threadIdx.x * 16;
    FqLane L;
    fq_lane(text, p0, n, (uint32_t)nbase & 3u, L, wn);
    const uint32_t qk = L.kept & fq_class_mask(L, 3);
    const uint32_t mine = (uint32_t)__popc(qk);
    const uint32_t incl = dev_wave_scan_incl(mine);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint32_t excl = incl - mine, total = 0;
#pragma unroll
    for (int i = 0; i < FQ_WAVES; ++i) {
      const uint32_t s = wsum[i];
      if (i < w) excl += s;
      total += s;
    }
    // a byte of quality line 4 r + 3 has 4 r + 3 newlines in front of it
    for (uint32_t m = qk & fq_lt16(L.v, threshold); m; m &= m - 1u) {
      const uint32_t low = (m & (0u - m)) - 1u;
      const uint64_t r = (nbase + L.excl_nl + (uint32_t)__popc(L.nl & low)) >> 2;
      const uint64_t i = qbase + excl + (uint32_t)__popc(qk & low) + r;
      if (i < nN) data[i] = (int8_t)-1;
    }
    qbase += total; nbase += L.total_nl;
    // (wn is written again behind the barrier above, wsum behind the next one)
  }
}

__global__ __launch_bounds__(256) void fq_length_kernel(const int64_t *__restrict__ start, int64_t nN, int64_t nS, int32_t *__restrict__ length,
                                                        uint64_t *__restrict__ words) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nS) return;
  const int64_t s = start[r], e = (r + 1 < nS) ? start[r + 1] : nN;
  int64_t len = e - s - 1;
  if (len > 0x7FFFFFFFll) {
    atomicOr((unsigned long long *)&words[FQ_W_LONG], 1ull);
    atomicMin((unsigned long long *)&words[FQ_W_REC_LONG], (unsigned long long)r);
    len = 0x7FFFFFFFll;
  }
  if (len < 0) len = 0;
  length[r] = (int32_t)len;
}

constexpr size_t FQ_WORDS_BYTES = FQ_NWORDS * 8;
constexpr size_t FQ_TILE_POOL_BYTES = 32 + 24;

struct FqPlan { uint64_t *words; uint4 *agg; uint64_t *pre; uint64_t ntiles; };

int fq_plan(cfrk_ctx *ctx, uint64_t nbytes, FqPlan *pl) {
  pl->ntiles = (nbytes + FQ_TILE - 1) / FQ_TILE;
  void *p;
  const int rc = cfrk_pool_get(ctx, BUF_FASTA, FQ_WORDS_BYTES + (size_t)pl->ntiles * FQ_TILE_POOL_BYTES, &p);
  if (rc) return rc;
  pl->words = (uint64_t *)p;
  pl->agg = (uint4 *)((char *)p + FQ_WORDS_BYTES);
  pl->pre = (uint64_t *)((char *)p + FQ_WORDS_BYTES + (size_t)pl->ntiles * 32);
  return CFRK_OK;
}

struct FqSizes { int64_t nN, nS; uint64_t qkept; };

// reduce + scan, the totals and the structural verdict read back (synchronises).  nbytes >= 1.
int fq_measure(cfrk_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, const FqPlan &pl, FqSizes *sz) {
  HIP_TRY(ctx, hipMemsetAsync(pl.words, 0, FQ_W_ONES * 8, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(pl.words + FQ_W_ONES, 0xFF, (FQ_NWORDS - FQ_W_ONES) * 8, ctx->stream));
  hipLaunchKernelGGL(fq_reduce_kernel, dim3((unsigned)pl.ntiles), dim3(FQ_THREADS), 0, ctx->stream, d_text, nbytes, pl.agg);
  hipLaunchKernelGGL(fq_scan_kernel, dim3(1), dim3(FQ_SCAN), 0, ctx->stream, d_text, nbytes, pl.agg, pl.ntiles, pl.words, pl.pre);
  HIP_TRY(ctx, hipGetLastError());
  uint64_t wd[FQ_NWORDS];
  HIP_TRY(ctx, hipMemcpyAsync(wd, pl.words, sizeof wd, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  // (the `cfrk` command and the tests recognise the causes by these words; the host parser's message, cfrk_host_fastq_message, uses the same)
  if (wd[FQ_W_BAD_OFF] != ~0ull) {
    const uint64_t off = wd[FQ_W_BAD_OFF];
    if (off >= nbytes) return cfrk_fail(ctx, CFRK_ERR_HIP, "FASTQ: fault offset %llu outside the text", (unsigned long long)off);
    hipLaunchKernelGGL(fq_line_kernel, dim3(1), dim3(FQ_THREADS), 0, ctx->stream, d_text, off, pl.pre, pl.words);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(wd, pl.words, sizeof wd, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return cfrk_fail(ctx, CFRK_ERR_LAYOUT, "FASTQ: line %llu does not begin with '%c' (byte offset %llu)", (unsigned long long)wd[FQ_W_LINE],
                     (wd[FQ_W_LINE] & 3) == 0 ? '@' : '+', (unsigned long long)off);
  }
  const uint64_t lines = wd[FQ_W_NL] + wd[FQ_W_OPEN_END];
  if (lines & 3) return cfrk_fail(ctx, CFRK_ERR_LAYOUT, "FASTQ: %llu lines, not a multiple of four", (unsigned long long)lines);
  sz->nS = (int64_t)(lines >> 2);
  sz->nN = (int64_t)wd[FQ_W_EMIT];
  sz->qkept = wd[FQ_W_QKEPT];
  return CFRK_OK;
}

// scatter, mask, lengths; the verdict of the length check read back (synchronises)
int fq_emit(cfrk_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, int min_qual, const FqPlan &pl, int8_t *d_data, int64_t *d_start,
            int32_t *d_length, const FqSizes &sz) {
  hipLaunchKernelGGL(fq_scatter_kernel, dim3((unsigned)pl.ntiles), dim3(FQ_THREADS), 0, ctx->stream, d_text, nbytes, pl.pre, pl.words, d_data,
                     d_start, (uint64_t)sz.nN, (uint64_t)sz.nS);
  if (min_qual > 0)
    hipLaunchKernelGGL(fq_mask_kernel, dim3((unsigned)pl.ntiles), dim3(FQ_THREADS), 0, ctx->stream, d_text, nbytes, pl.pre,
                       (uint32_t)(CFRK_FASTQ_QUAL_BASE + min_qual), d_data, (uint64_t)sz.nN);
  hipLaunchKernelGGL(fq_length_kernel, dim3((unsigned)((sz.nS + 255) / 256)), dim3(256), 0, ctx->stream, d_start, sz.nN, sz.nS, d_length, pl.words);
  HIP_TRY(ctx, hipGetLastError());
  uint64_t wd[FQ_NWORDS];
  HIP_TRY(ctx, hipMemcpyAsync(wd, pl.words, sizeof wd, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t diff = wd[FQ_W_REC_DIFF];
  if (diff == ~0ull && (uint64_t)(sz.nN - sz.nS) != sz.qkept) diff = (uint64_t)sz.nS - 1;      // the end of the text closes the last record
  if (diff != ~0ull)
    return cfrk_fail(ctx, CFRK_ERR_LAYOUT, "FASTQ: record %llu has sequence and quality lines of different lengths", (unsigned long long)diff);
  if (wd[FQ_W_LONG])
    return cfrk_fail(ctx, CFRK_ERR_LAYOUT, "FASTQ: record %llu is longer than 2^31 - 1 bases", (unsigned long long)wd[FQ_W_REC_LONG]);
  return CFRK_OK;
}

// measure, refuse or place the outputs, emit: what both forms run on device text
int fq_core(cfrk_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, int min_qual, const FqPlan &pl, ReadsOut *o, int64_t *nN_out, int64_t *nS_out) {
  FqSizes sz;
  int rc = fq_measure(ctx, d_text, nbytes, pl, &sz);
  if (rc || (rc = reads_out_fit(ctx, "FASTQ", *o, sz.nN, sz.nS, nN_out, nS_out)) || (rc = reads_out_carve(ctx, o, sz.nN, sz.nS))) return rc;
  return fq_emit(ctx, d_text, nbytes, min_qual, pl, o->data, o->start, o->length, sz);
}

int fq_check(cfrk_ctx *ctx, const void *text, uint64_t nbytes, int min_qual, const void *data, uint64_t cap_data, const void *start,
             const void *length, uint64_t cap_reads, int64_t *nN_out, int64_t *nS_out) {
  if (!ctx) return CFRK_ERR_ARG;
  if (min_qual < 0 || min_qual > CFRK_FASTQ_MAX_QUAL) return cfrk_fail(ctx, CFRK_ERR_ARG, "min_qual %d: 0 .. %d", min_qual, CFRK_FASTQ_MAX_QUAL);
  return parse_check(ctx, text, nbytes, data, cap_data, start, length, cap_reads, nN_out, nS_out);
}

}  // namespace

extern "C" int cfrk_fastq_parse_device(cfrk_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, int min_qual, int8_t *d_data, uint64_t cap_data,
                                       int64_t *d_start, int32_t *d_length, uint64_t cap_reads, int64_t *nN_out, int64_t *nS_out) {
  int rc = fq_check(ctx, d_text, nbytes, min_qual, d_data, cap_data, d_start, d_length, cap_reads, nN_out, nS_out);
  if (rc || nbytes == 0) return rc;
  if (((uintptr_t)d_text & 15) != 0) return cfrk_fail(ctx, CFRK_ERR_ALIGN, "d_text %p", (const void *)d_text);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  FqPlan pl;
  if ((rc = fq_plan(ctx, nbytes, &pl))) return rc;
  ReadsOut o = {d_data, d_start, d_length, nullptr, cap_data, cap_reads, -1, false};
  return fq_core(ctx, d_text, nbytes, min_qual, pl, &o, nN_out, nS_out);
}

extern "C" int cfrk_fastq_parse(cfrk_ctx *ctx, const char *text, uint64_t nbytes, int min_qual, int8_t *data, uint64_t cap_data, int64_t *start,
                                int32_t *length, uint64_t cap_reads, int64_t *nN_out, int64_t *nS_out) {
  int rc = fq_check(ctx, text, nbytes, min_qual, data, cap_data, start, length, cap_reads, nN_out, nS_out);
  if (rc || nbytes == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  FqPlan pl;
  void *d_text;
  if ((rc = fq_plan(ctx, nbytes, &pl)) || (rc = cfrk_pool_get(ctx, BUF_FASTA_IN, (size_t)nbytes + 16, &d_text))) return rc;   // (every slot before the copy)
  HIP_TRY(ctx, hipMemcpyAsync(d_text, text, (size_t)nbytes, hipMemcpyHostToDevice, ctx->stream));
  ReadsOut o = {nullptr, nullptr, nullptr, nullptr, cap_data, cap_reads, BUF_FASTA_OUT, false};
  if ((rc = fq_core(ctx, (const uint8_t *)d_text, nbytes, min_qual, pl, &o, nN_out, nS_out))) return stage_drain(ctx, rc);
  return download_reads(ctx, o, data, start, length, nullptr, *nN_out, *nS_out);
}
