// msp.hip -- minimizer-partitioned global k-mer counting for gfx950 (16 <= k <= 32).
//
// Why: one HBM atomic per k-mer occurrence (global_hash.hip) runs at the chip's scattered-atomic
// rate (~2e10/s), two orders of magnitude under what HBM bandwidth allows.  Here HBM only sees
// streams, and every occurrence is counted with LDS atomics:
//
//   P1  msp_p1b_kernel read the flat code buffer once (2 x dwordx4 per lane, 2-bit packing in
//                      registers), compute for every k-mer the minimum hash over its W = k-m+1
//                      canonical m-mers (its minimizer), cut the k-mers into runs that share one
//                      minimizer occurrence ("super-k-mers"; content-defined, they may cross into
//                      the next lane's chunk), and append each run as one 16-B record
//                      {48 bases, leaf id, closed-end flags, n} to level-1 bin = leaf >> 8.  A
//                      workgroup stages its records in LDS, reserves space with ONE global
//                      atomic per non-empty bin per 15.6 KB of input, then copies out in bin
//                      order (coalesced).  Emission is wave-balanced: lane i builds the wave's
//                      i-th record.
//   P2  msp_p2_kernel  stream every level-1 region, split it 512 ways: leaf low byte x
//                      {truncated run, complete run} (LDS counting sort of 4096-record tiles,
//                      one global atomic per stream per tile, coalesced copy-out).
//   P3  msp_p3_kernel  one workgroup per leaf (65536 leaves), everything in LDS: complete runs
//                      are counted per RECORD in a record table (at depth most are identical),
//                      then every distinct record is expanded once with its multiplicity, and
//                      truncated runs with weight 1, into a bucketized k-mer table
//                      (ds_cmpst_b64 to claim, ds_add_u32 to count); the occupied slots are
//                      compacted to the output list with one cursor atomic per workgroup.
//                      Leaves with more distinct runs than the record table holds (and every
//                      leaf for k < 28) deduplicate in a table over the whole LDS pool first
//                      and list the distinct runs at the head of their own stream.
//   multi-GPU          leaves are disjoint in key space on every rank, so lists are exchanged
//                      and added per leaf, again in LDS (msp_gather_kernel, msp_merge_kernel).
//
// All occurrences of a k-mer share its minimizer, hence its leaf, so leaves are disjoint in key
// space and the output list is the final result.  Anything that does not fit (bin capacity, LDS
// table) is counted with table_add1() into the global HBM table instead ("64-bit HBM atomics
// only on spill") and ST_SPILLED is raised; the host then folds the list into the table.
//
// msp_shared.h holds what this file shares with msp2.hip (33 <= k <= 64) and that does not depend on the record
// format -- the layout and sum kernels, the sizing rules, the index buffers, the exact level-1 layout, the passes
// of a batch that does not fit -- and msp_runs.h the exchange by runs, host side included.
//
// Semantics are those of global_hash.hip (the guarded ComputeFreq of
// /root/reference/src/kmer_kernel.cu:52-70 summed over reads).
#include "msp.h"
#include "table.h"
#include "msp_dev.h"

#include <algorithm>
#include <cmath>
#include <new>
#include <type_traits>
#include <vector>

namespace {
#include "msp_shared.h"
#include "msp_runs.h"

constexpr int P1_THREADS = 512;

constexpr int P2_THREADS = 512, P2_PER = 8;   // (4096-record tiles: two 75 KB workgroups per CU; 8192 and 2560 measured slower, profiles/r05/p2_tile_size_*)
constexpr int P2_GROUP = 4;                      // consecutive tiles per workgroup (next tile prefetched)

constexpr int P3_THREADS = 1024;
constexpr int TS_LOG = 12, TS = 1 << TS_LOG;   // LDS table slots per leaf

// count every k-mer of a record straight into the global HBM table
// (the table view by value: a reference makes every thread of the calling kernel store the view
// to scratch memory at kernel entry -- 48 bytes per thread that reach HBM)
__device__ __noinline__ void spill_record(uint4 rec, int k, bool canon, TableView t, uint32_t weight = 1u) {
  t.stats[ST_SPILLED] = 1;
  dev_count_event(&t.stats[ST_AUX0]);
  const int nk = (int)(rec.w & 63u) + 1;
  const uint64_t hi = ((uint64_t)rec.x << 32) | rec.y;
  const uint64_t lo = (uint64_t)rec.z << 32;
  for (int j = 0; j < nk; ++j) {
    const uint64_t x = j ? ((hi << (2 * j)) | (lo >> (64 - 2 * j))) : hi;
    uint64_t key = x >> (64 - 2 * k);
    if (canon) {
      const uint64_t rc = dev_revcomp64(key, k);
      key = rc < key ? rc : key;
    }
    table_add1(t, key, weight);
  }
}

// Wave layout: 64 lanes load 64 consecutive 32-byte chunks; lane 0 and lanes 62, 63 are halo
// lanes (they compute, never emit), lanes 1..61 own their chunk's 32 window starts.  A run is
// emitted by the lane that owns its FIRST k-mer and may extend up to W-1 positions into the next
// lane's chunk, so run boundaries depend on the sequence only -- not on where a read happens to
// sit in the buffer -- and every read covering a locus emits the same record.
constexpr int P1_OWN = 61;                       // owner lanes per wave
constexpr int P1_WAVES = P1_THREADS / 64;

// level-1 bin of a record: the leaf id's high byte (header bits 16..23; the top byte may hold sub-value bits)
template <bool SUB>
__device__ __forceinline__ uint32_t bin_of(uint32_t w) { return SUB ? ((w >> 16) & (uint32_t)(B1 - 1)) : (w >> 16); }

// write record `rec` as entry `dst` of level-1 region `reg`; a full region parks a few records and
// beyond that raises ST_L1OVF (the cursors keep counting: the host redoes P1 with exact sizes)
// (EX = false: compiled for the fixed-stride layout only -- the fused pipeline kernel, which never
// runs on an exact layout, sheds the code and the scalar registers of that case)
template <bool EX>
__device__ __forceinline__ void l1_put(const MspView &v, uint32_t reg, uint32_t dst, uint4 rec, int k, bool canon,
                                       const TableView &t) {
  const bool exact1 = EX && v.exact1;
  const uint64_t cap = exact1 ? (uint64_t)v.rcap[reg] : v.cap1;
  const uint64_t at = exact1 ? v.rbase[reg] : (uint64_t)reg * v.cap1;
  if (dst < cap) {
    v.rec1[at + dst] = rec;
  } else if (exact1) {
    spill_record(rec, k, canon, t);                      // cannot happen: cap is the exact count
  } else if (*(volatile uint64_t *)&v.stats[ST_L1OVF] == 0) {
    const unsigned long long o = atomicAdd((unsigned long long *)&v.stats[ST_OVFN1], 1ull);
    if (o < v.ovf1_cap) v.ovf1[o] = rec;
    else v.stats[ST_L1OVF] = 1;
  }
}

// ---------------------------------------------------------------------------------------- P1
// Emission is wave-balanced.  Building a lane's records in a loop over ITS runs (first version)
// costs the wave max-over-lanes trips (5..6 at W = 18 for 2.8 runs per lane on average, 18 at
// W = 4) of a ~75-instruction body.  Here a lane only lists its run starts (position descriptors,
// a few instructions per trip); everything a record is made of is staged per wave in LDS -- the
// wave's 2-bit base string, run terminators, validity, the leaf id of every position -- and then
// lane i builds the wave's i-th record: ceil(runs / 64) trips with all lanes busy.  Records stay
// in registers until the workgroup's bin histogram is scanned and go to LDS directly in bin order
// (rank from the histogram atomic), so the staging area and the sorted records share one
// allocation.  Runs per wave grow as 2/(W+1): the trips held in registers are a template
// parameter (4 for W >= 16 ... 12 for W = 4), and so are registers and workgroups per CU.
// P1B_TR = balanced trips held in registers (64 runs per wave each)
// LDS of one P1 workgroup: per-wave staging (later the bin-sorted records), histogram, offsets
// SUB: a job with far more distinct k-mers than the leaf tables hold (capacity hint > ~2.7e8) also stages
// five bits of every position's minimizer hash that the leaf id does not use and writes them to the top
// byte of the record's header word: the leaf kernel then splits an overfull leaf by RECORD, not by key,
// so that every record is expanded once (msp2.hip does the same; SUB_BITS: msp_shared.h).  2 KB more staging per
// wave: two workgroups per CU instead of three.
#define P1_MARK(text) asm volatile("; " text)
// the same for the parts of the leaf kernel's scan of the complete stream (p3_body, phase 1a; tools/p3_isa_account.py)
// ... and of its phase 2
#define P3_MARK(text) asm volatile("; " text)
template <int P1B_TR, bool SUB = false>
struct P1Lds {
  static constexpr int STAGE = 4096 + 3 * 512 + P1B_TR * 128 + (SUB ? 2048 : 0);     // bytes of staging per wave
  static constexpr int ARENA = P1_WAVES * STAGE;
  static constexpr int BYTES = ARENA + 2 * B1 * 4 + 32;
};

// Workgroup-level body of the partition kernel: tile `tile` of the input, appended to sub-region
// `subreg` of every level-1 bin.
// (One tile per workgroup, not a persistent loop: a looping workgroup waits at the top of every
// tile for its input loads -- and, vmcnt being one in-order counter, for the previous tile's
// stores before them; measured 16-28 % slower, profiles/r03/persistent_p1_is_slower.txt.)
template <int W, int P1B_TR, bool EX, bool SUB>
__device__ __forceinline__ void p1_tile(uint4 *pool, const int8_t *__restrict__ data, int64_t nN, int k, int m, int canon,
                                        int64_t tile, uint32_t subreg, const MspView &v, const TableView &t) {
  constexpr int NH = 32 + W - 1;
  constexpr int P1B_STAGE = P1Lds<P1B_TR, SUB>::STAGE;
  // sorted records share the staging bytes; the last 2.5 KB hold the copy-out table (dabs, plim)
  constexpr int P1B_TAIL = B1 * 10;
  constexpr int P1B_RCAP = (P1_WAVES * P1B_STAGE - P1B_TAIL) / 16;
  uint4 *const arena = pool;                     // per-wave staging, later the bin-sorted records (P1B_RCAP of them)
  uint32_t *const hist = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(pool) + P1Lds<P1B_TR, SUB>::ARENA);
  uint32_t *const loff = hist + B1;
  uint32_t *const wtot = loff + B1;              // 4 words
  uint32_t *const nrec_p = wtot + 4;
  uint32_t *const gbase = hist;                  // the global bases take the histogram's place once it is scanned
  // copy-out fast path, worked out once per bin and tile by the thread that reserved the segment:
  // arena position p of bin b goes to record dabs[b] + p of the level-1 buffer while p < plim[b]
  // (at the end of the arena: the staging area is dead by then and three workgroups keep fitting a CU's LDS)
  unsigned long long *const dabs = reinterpret_cast<unsigned long long *>(reinterpret_cast<uint8_t *>(arena) + P1B_RCAP * 16);
  uint16_t *const plim = reinterpret_cast<uint16_t *>(dabs + B1);
  static_assert((P1_WAVES * P1B_STAGE - P1B_TAIL) % 16 == 0, "the table starts on a record boundary");

  const int nkmax = min(48 - k + 1, 32);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint8_t *const stage = reinterpret_cast<uint8_t *>(arena) + wave * P1B_STAGE;
  // (the base string first: the four dwords of a record's bases are read with small immediate offsets from one
  // address; terminators and validity side by side: one 16-byte read per record)
  uint32_t *const s_str = reinterpret_cast<uint32_t *>(stage);                // 128 dwords of bases
  uint4 *const s_EW = reinterpret_cast<uint4 *>(stage + 512);                 // per lane {E low, E high, W low, W high}:
                                                                              // run terminators, validity of position p-1
  uint16_t *const s_leaf = reinterpret_cast<uint16_t *>(stage + 1536);        // [64 lanes][32 positions]
  uint16_t *const s_dsc = reinterpret_cast<uint16_t *>(stage + 4096 + 1536);  // (lane << 5) | position
  uint8_t *const s_sub = stage + 4096 + 1536 + P1B_TR * 128;                  // [64 lanes][32 positions] (SUB only)
  if (tid < B1) hist[tid] = 0;
  lds_barrier();

  // (P1_PHASE_* / P1_COLD: assembly comments, no instructions; tools/p1_isa_account.py counts between them)
  P1_MARK("P1_PHASE_A");
  // ---- A: this lane's chunk, packed 2 bits per base; neighbours' chunks by shuffle ----
  const int64_t wave_g = tile * P1_WAVES + wave;
  const int64_t chunk = wave_g * P1_OWN + lane - 1;
  const int64_t off = chunk * 32;
  uint32_t b0 = 0, b1 = 0, bad = 0xFFFFFFFFu;
  if (chunk >= 0) {
    if (off + 32 > nN) P1_MARK("P1_COLD byte-wise tail chunk");
    dev_load_chunk32(data, off, nN, b0, b1, bad);
  }
  const uint32_t n0 = dev_lane_next(b0), n1 = dev_lane_next(b1);
  const uint32_t nbad = dev_lane_next(bad), nnbad = dev_lane_next(dev_lane_next(bad));
  const uint64_t hi = ((uint64_t)b0 << 32) | b1;
  const uint64_t mid = ((uint64_t)n0 << 32) | n1;
  // invalid bases smeared over the k - 1 positions before them, by doubling, on the three words there are
  // (every shift is between 1 and 16: one v_alignbit and one v_or per word and step)
  uint32_t Q0 = bad, Q1 = nbad, Q2 = nnbad;
  {
    int w = 1;
#pragma unroll
    for (int st = 0; st < 5; ++st) {
      if (2 * w <= k) {
        Q0 |= __builtin_amdgcn_alignbit(Q0, Q1, 32 - w);
        Q1 |= __builtin_amdgcn_alignbit(Q1, Q2, 32 - w);
        Q2 |= Q2 << w;
        w *= 2;
      }
    }
    if (k > w) {
      Q0 |= __builtin_amdgcn_alignbit(Q0, Q1, 32 - (k - w));
      Q1 |= __builtin_amdgcn_alignbit(Q1, Q2, 32 - (k - w));
    }
  }
  const uint64_t Vx = ~(((uint64_t)Q0 << 32) | Q1);
  const uint32_t V = (uint32_t)(Vx >> 32);
  const uint32_t prevV = dev_lane_prev(V) & 1u;

  uint32_t H[NH];
  const uint64_t Cx = msp_minimizers<W>(hi, mid, chunk, m, H);
  const uint64_t E = Cx | ~Vx | (1ull << (63 - NH));
  const uint32_t Vprev = (V >> 1) | (prevV << 31);
  uint32_t S = V & ((uint32_t)(Cx >> 32) | ~Vprev);
  const bool owner = lane >= 1 && lane <= P1_OWN && off < nN;
  if (!owner) S = 0;

  // ---- B1: stage what records are made of; list the run starts ----
  P1_MARK("P1_PHASE_B1");
  {
    const LeafPack LP = leaf_pack(H);
    uint4 *lp = reinterpret_cast<uint4 *>(s_leaf + lane * 32);
    lp[0] = make_uint4(LP.w[0], LP.w[1], LP.w[2], LP.w[3]);
    lp[1] = make_uint4(LP.w[4], LP.w[5], LP.w[6], LP.w[7]);
    lp[2] = make_uint4(LP.w[8], LP.w[9], LP.w[10], LP.w[11]);
    lp[3] = make_uint4(LP.w[12], LP.w[13], LP.w[14], LP.w[15]);
    reinterpret_cast<uint2 *>(s_str)[lane] = make_uint2(b0, b1);
    s_EW[lane] = make_uint4((uint32_t)E, (uint32_t)(E >> 32), ((uint32_t)Vx >> 1) | (V << 31), Vprev);
    if (SUB) {
      // bits 24..27 and 7 of the packed minimum: hash bits, equal for every occurrence of a k-mer, that
      // neither the leaf id (bits 8..23) nor the position tag (bits 0..4) uses; bit 7 -- the uniform one -- lowest
      uint32_t sw[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        uint32_t x = 0;
#pragma unroll
        for (int j = 3; j >= 0; --j) {
          const uint32_t h = H[4 * i + j];
          x = (x << 8) | (((h >> 24) & 15u) << 1) | ((h >> 7) & 1u);
        }
        sw[i] = x;
      }
      uint4 *sp = reinterpret_cast<uint4 *>(s_sub + lane * 32);
      sp[0] = make_uint4(sw[0], sw[1], sw[2], sw[3]);
      sp[1] = make_uint4(sw[4], sw[5], sw[6], sw[7]);
    }
  }
  if (v.dbg & CFRK_ABL_P1_NO_EMIT) {             // timing ablation: keep the front end alive, emit nothing
    if (S == 0x12345678u && (uint32_t)E == 0x9ABCDEFu) v.stats[ST_AUX0] = 1;
    return;
  }
  uint32_t cnt_w;
  uint32_t S2 = 0;                               // run starts beyond the balanced phase's capacity
  // (CFRK_DEBUG_SMALL_WAVE_CAP: one trip's worth, so that tests reach the direct-append path)
  const uint32_t wcap = (v.dbg & CFRK_DEBUG_SMALL_WAVE_CAP) ? 64u : (uint32_t)(P1B_TR * 64);
  {
    const uint32_t mine = (uint32_t)__popc(S);
    const uint32_t incl = dev_wave_scan_incl(mine);
    cnt_w = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    uint32_t widx = incl - mine;
    const uint32_t tag = (uint32_t)lane << 5;
    if (incl <= wcap) {                          // all of this lane's runs fit: nothing to test per run
      uint16_t *dp = s_dsc + widx - 1;           // (pre-increment: the address register is updated in place)
      while (S) {
        const int a = __clz(S);
        S &= ~(0x80000000u >> a);
        *++dp = (uint16_t)(tag | (uint32_t)a);
      }
    } else {
      P1_MARK("P1_COLD wave over capacity");
      while (S) {
        const int a = __clz(S);
        const uint32_t bit = 0x80000000u >> a;
        S &= ~bit;
        if (widx < wcap) s_dsc[widx] = (uint16_t)(tag | (uint32_t)a);
        else S2 |= bit;
        ++widx;
      }
    }
  }
  lds_wave_sync();                               // the wave's staging is written: lanes read each other's

  // record of the run that starts at position d & 31 of lane d >> 5 (d is also the index of its leaf id)
  // (32-bit work where the ranges allow: a <= 31 and n <= 32, so the terminators that decide n are one
  // 32-bit window of E from the run start, and alignbit / shifts take the low five bits of ~d = 31 - a)
  const uint32_t nkm1 = (uint32_t)(nkmax - 1);
  const int zc = 2 * (48 - k);                   // cleared tail bits of a run of one k-mer
  auto build = [&](uint32_t d) {
    const uint4 ew = s_EW[d >> 5];
    const uint32_t leaf = s_leaf[d];
    // 96 bits of the wave's base string from bit 2d - 2: dwords idx0..idx0+3, funnel-shifted by
    // 30 - ((2d - 2) & 31) = -2d (mod 32)
    const uint32_t idx0 = (d - 1u) >> 4, sh = 0u - 2u * d;
    const uint32_t D0 = s_str[idx0], D1 = s_str[idx0 + 1], D2 = s_str[idx0 + 2], D3 = s_str[idx0 + 3];
    const uint32_t a = d & 31u, na = ~d;
    // terminators of positions a+1 .. a+32, the first in the top bit (none set: clz = 32, the min catches it)
    const uint32_t e32 = __builtin_amdgcn_alignbit(ew.y, ew.x, na);
    const uint32_t nm1 = min((uint32_t)__clz(e32), nkm1);        // n - 1
    // An end of the run is "closed" when it is a minimizer change between valid k-mers (header
    // bit 6: left end, bit 7: right end) and open when the read or an invalid base cut it.  Both
    // closed = a complete run: every read covering this locus emits the same record.  One end
    // open = a prefix (suffix) of the complete run of its locus, with which it shares its first
    // (last) k-mer.
    // left: bit 63 - a of W; right: bit 62 - a - n, brought to the top
    const uint32_t lf = (ew.w >> (na & 31u)) & 1u;
    const uint64_t Ws = ((uint64_t)ew.w << 32) | ew.z;
    const uint32_t rf = (uint32_t)((Ws << (a + nm1 + 2u)) >> 63);
    uint4 rec;
    rec.x = __builtin_amdgcn_alignbit(D0, D1, sh);
    // bases after the run's last k-mer are cleared: equal runs -> byte-identical records
    const int z = zc - 2 * (int)nm1;             // 2 * (48 - (n + k - 1)), < 64 for k >= 17
    uint64_t r12 = ((uint64_t)__builtin_amdgcn_alignbit(D1, D2, sh) << 32) | __builtin_amdgcn_alignbit(D2, D3, sh);
    r12 = (W < 8 && z >= 64) ? 0ull : (r12 & (~0ull << z));
    rec.y = (uint32_t)(r12 >> 32);
    rec.z = (uint32_t)r12;
    rec.w = (leaf << 8) | (rf << 7) | (lf << 6) | nm1;
    if (SUB) rec.w |= (uint32_t)s_sub[d] << 24;
    return rec;
  };

  // more runs in this wave than the balanced phase holds (pathological input): append directly
  while (S2) {
    P1_MARK("P1_COLD direct append");
    const int a = __clz(S2);
    S2 &= ~(0x80000000u >> a);
    const uint4 rec = build(((uint32_t)lane << 5) | (uint32_t)a);
    if (((rec.w >> 8) & v.sel_mask) != v.sel_val) continue;    // not a leaf of this pass
    const uint32_t reg = l1_reg(bin_of<SUB>(rec.w), subreg);
    const uint32_t dst = atomicAdd(&v.cnt1[reg], 1u);
    l1_put<EX>(v, reg, dst, rec, k, canon != 0, t);
  }

  // ---- B2: lane i builds the wave's i-th record ----
  P1_MARK("P1_PHASE_B2");
  uint4 rc[P1B_TR];
  uint32_t rk[P1B_TR];                           // rank inside the record's bin; ~0: no record
  cnt_w = min(cnt_w, wcap);
  // (rc[tr] is only ever read where rk[tr] says there is a record: no filler values to move around;
  // the leaf selection of a multi-pass batch is tested per record only in such a batch)
  auto emit = [&](auto sel) {
    if (decltype(sel)::value) P1_MARK("P1_COLD multi-pass selection");
#pragma unroll
    for (int tr = 0; tr < P1B_TR; ++tr) {
      rk[tr] = 0xFFFFFFFFu;
      const uint32_t i = (uint32_t)(tr * 64 + lane);
      if (i < cnt_w) {
        rc[tr] = build(s_dsc[i]);
        if (!decltype(sel)::value || ((rc[tr].w >> 8) & v.sel_mask) == v.sel_val)
          rk[tr] = atomicAdd(&hist[bin_of<SUB>(rc[tr].w)], 1u);
      }
    }
  };
  if (v.sel_mask == 0 && v.sel_val == 0) emit(std::false_type{});     // every leaf: all one-pass jobs
  else emit(std::true_type{});
  lds_barrier();

  // ---- C: one global reservation per non-empty bin; bin offsets ----
  P1_MARK("P1_PHASE_C");
  uint32_t my_base = 0;
  if (tid < B1) {
    const uint32_t c = hist[tid];
    if (c) my_base = atomicAdd(&v.cnt1[l1_reg(tid, subreg)], c);
  }
  block_scan<B1, true>(hist, loff, wtot);              // ends with a barrier: the staging area is dead
  if (tid == B1 - 1) *nrec_p = loff[tid] + hist[tid];   // (before this thread overwrites hist[tid] below)
#pragma unroll
  for (int tr = 0; tr < P1B_TR; ++tr) {
    if (rk[tr] != 0xFFFFFFFFu) {
      const uint32_t pos = loff[bin_of<SUB>(rc[tr].w)] + rk[tr];
      if (pos < (uint32_t)P1B_RCAP) arena[pos] = rc[tr];
    }
  }
  if (tid < B1) {
    gbase[tid] = my_base;
    const uint32_t reg = l1_reg(tid, subreg);
    const bool exact1 = EX && v.exact1;
    const uint64_t cap = exact1 ? (uint64_t)v.rcap[reg] : v.cap1;
    const uint64_t at = exact1 ? v.rbase[reg] : (uint64_t)reg * v.cap1;
    const uint32_t lo = loff[tid];
    dabs[tid] = at + my_base - lo;
    const uint64_t room = cap > (uint64_t)my_base ? cap - my_base : 0;       // records of this segment that fit the region
    plim[tid] = (uint16_t)min((uint64_t)lo + room, (uint64_t)0xFFFFu);
    static_assert(P1B_RCAP <= 0xFFFF, "arena positions fit 16 bits");
  }
  lds_barrier();

  // ---- D: copy out in bin order ----
  P1_MARK("P1_PHASE_D");
  const uint32_t nrec_s = *nrec_p;
  const uint32_t nrec = min(nrec_s, (uint32_t)P1B_RCAP);
  for (uint32_t p = tid; p < nrec; p += P1_THREADS) {
    const uint4 rec = arena[p];
    const uint32_t b = bin_of<SUB>(rec.w);
    if (p < (uint32_t)plim[b]) {
      v.rec1[dabs[b] + p] = rec;
    } else {                                     // region full: park / flag
      P1_MARK("P1_COLD region full");
      l1_put<EX>(v, l1_reg(b, subreg), gbase[b] + (p - loff[b]), rec, k, canon != 0, t);
    }
  }
  if (nrec_s > (uint32_t)P1B_RCAP) {             // records beyond the LDS arena go to their reserved places
    P1_MARK("P1_COLD arena overflow");
#pragma unroll
    for (int tr = 0; tr < P1B_TR; ++tr) {
      if (rk[tr] != 0xFFFFFFFFu) {
        const uint32_t b = bin_of<SUB>(rc[tr].w);
        if (loff[b] + rk[tr] >= (uint32_t)P1B_RCAP)
          l1_put<EX>(v, l1_reg(b, subreg), gbase[b] + rk[tr], rc[tr], k, canon != 0, t);
      }
    }
  }
}

template <int W, int P1B_TR, bool SUB>
__global__ __launch_bounds__(P1_THREADS, ((P1B_TR <= 6 && !SUB) ? 6 : 4)) void msp_p1b_kernel(const int8_t *__restrict__ data,
                                                             int64_t nN, int k, int m, int canon,
                                                             int64_t tile0, MspView v, TableView t) {
  __shared__ uint4 pool[P1Lds<P1B_TR, SUB>::BYTES / 16];
  const int64_t tile = tile0 + blockIdx.x;
  p1_tile<W, P1B_TR, true, SUB>(pool, data, nN, k, m, canon, tile, (uint32_t)tile & (v.nxg - 1), v, t);
}

// ---------------------------------------------------------------------------------------- P2
// sub-bin of a record inside its level-1 bin: leaf low byte x {truncated run, complete run}.
// Complete runs get a stream of their own so that P3 can count them per RECORD with every lane
// busy, instead of k-mer by k-mer.
// PERSISTENT grid of nwg workgroups (a multiple of 8).  Workgroup w belongs to XCD group w % 8 and
// that group walks ITS bins (b1 = group, group + 8, ...) one after the other: the group's work items
// -- P2_GROUP consecutive tiles of one bin -- are numbered bin after bin from the records the bins
// really hold (no empty items), and workgroup j of the group takes items j, j + nwg/8, ...  At any
// moment the workgroups of one XCD append to the leaf streams of one or two level-1 bins: a leaf
// stream is only ever written from one XCD and its frontier sectors merge in L2 (P2: 11.6 -> 10.0 ms).
// Two streams per leaf: truncated runs (class 0) and complete runs (class 1).  The leaf kernel
// sorts records by length itself, so finer classes would only shorten P2's write segments.
constexpr int NCLS = 2;
static_assert(NCLS <= SUM_CLASSES, "msp_sum_kernel clears a word per class");
constexpr int NSUB = NCLS * B2;                           // 512 sub-bins of a level-1 bin
__device__ __forceinline__ uint32_t sub_of(uint32_t w) { return (((w >> 8) & (B2 - 1)) << 1) | ((((w >> 6) & 3u) == 3u) ? 1u : 0u); }

// LDS of one P2 workgroup with tiles of P2_THREADS * PER records (byte offsets into its pool)
template <int PER>
struct P2Lds {
  static constexpr int TILE = P2_THREADS * PER;
  static constexpr int DABS = TILE * 16;                   // u64[NSUB]
  static constexpr int HIST = DABS + NSUB * 8;             // u32[NSUB]
  static constexpr int LOFF = HIST + NSUB * 4;             // u32[NSUB]
  static constexpr int PLIM = LOFF + NSUB * 4;             // u16[NSUB]
  static constexpr int WTOT = PLIM + NSUB * 2;             // u32[P2_THREADS / 64]
  static constexpr int RPRE = WTOT + (P2_THREADS / 64) * 4;   // u32[NXG + 1]
  static constexpr int GPRE = RPRE + (NXG + 1) * 4;        // u32[B1 / NXCD + 1] (persistent form only)
  static constexpr int BYTES = (GPRE + (B1 / NXCD + 1) * 4 + 15) / 16 * 16;
};

// One work item of the second-level kernel: the tiles [grp * NGRP, (grp + 1) * NGRP) of level-1 bin
// b1 (all of it that exists; nothing if the bin holds fewer records).
// PER = records per thread and tile: 8 stand-alone (two workgroups of 75 KB per CU), 5 in the fused
// kernel (the LDS of a P1 workgroup, 80 VGPRs); NGRP = consecutive tiles per item.
template <int PER, bool EX, bool PF, int NGRP>
__device__ __forceinline__ void p2_item(uint4 *pool, uint32_t b1, uint32_t grp, int k, int canon, const MspView &v, const TableView &t) {
  constexpr int TILE = P2_THREADS * PER;
  static_assert(TILE <= 0xFFFF, "tile positions fit 16 bits");
  uint4 *const sorted = pool;
  uint8_t *const pb = reinterpret_cast<uint8_t *>(pool);
  // copy-out fast path, once per stream and tile: sorted position p of sub-bin sb goes to record
  // dabs[sb] + p of the leaf buffer while p < plim[sb]
  unsigned long long *const dabs = reinterpret_cast<unsigned long long *>(pb + P2Lds<PER>::DABS);
  uint32_t *const hist = reinterpret_cast<uint32_t *>(pb + P2Lds<PER>::HIST);   // hist doubles as the fill cursor
  uint32_t *const loff = reinterpret_cast<uint32_t *>(pb + P2Lds<PER>::LOFF);
  uint16_t *const plim = reinterpret_cast<uint16_t *>(pb + P2Lds<PER>::PLIM);
  uint32_t *const wtot = reinterpret_cast<uint32_t *>(pb + P2Lds<PER>::WTOT);
  uint32_t *const rpre = reinterpret_cast<uint32_t *>(pb + P2Lds<PER>::RPRE);   // exclusive prefix of the bin's sub-region sizes
  static_assert(NSUB <= P2_THREADS && NSUB % 64 == 0, "the scan below gives one thread per sub-bin");
  static_assert(NXG <= 64, "one wave scans the sub-region sizes");
  const int tid = threadIdx.x;
  const bool exact1 = EX && v.exact1, exact2 = EX && v.exact;
  // The bin's sub-regions are read as ONE stream (region after region): tiles are full except the
  // bin's last one, however many cursors P1 spreads its appends over.
  if (tid < 64) {
    const uint32_t c = ((uint32_t)tid < v.nxg) ? (uint32_t)min((uint64_t)v.cnt1[l1_reg(b1, tid)],
                                                               exact1 ? (uint64_t)v.rcap[l1_reg(b1, tid)] : v.cap1) : 0u;
    const uint32_t incl = dev_wave_scan_incl(c);
    if ((uint32_t)tid < v.nxg) rpre[tid] = incl - c;
    if (tid == 63) rpre[v.nxg] = incl;
  }
  lds_barrier();
  const uint64_t n = rpre[v.nxg];
  // a workgroup takes NGRP consecutive tiles and asks for the next tile's records before it
  // sorts and writes the current one: the load latency hides under the LDS work
  const uint64_t g0r = (uint64_t)grp * NGRP * TILE;
  if (g0r >= n) return;
  // record `idx` of the bin's stream lies in the sub-region `sr` with rpre[sr] <= idx < rpre[sr + 1]: one
  // binary search for a thread's first record, then the cursor only moves forward (a thread's
  // indices grow from fetch to fetch)
  uint32_t sr = 0;
  {
    uint32_t hi = v.nxg;                         // invariant: rpre[sr] <= idx < rpre[hi]
    const uint64_t idx = g0r + tid;
    while (hi - sr > 1) {
      const uint32_t mid = (sr + hi) >> 1;
      if (rpre[mid] <= idx) sr = mid; else hi = mid;
    }
  }
  auto fetch = [&](uint64_t idx) {
    while (sr + 1 < v.nxg && rpre[sr + 1] <= idx) ++sr;
    if (exact1) return v.rec1[v.rbase[l1_reg(b1, sr)] + (idx - rpre[sr])];
    return v.rec1[(uint64_t)l1_reg(b1, sr) * v.cap1 + (idx - rpre[sr])];
  };
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  // PF: the next tile's records are asked for before the current tile is sorted and written (PER
  // more uint4 registers).  The fused kernel's copy of this role goes without: it has 80 VGPRs,
  // and while it waits for its loads the partitioning workgroups of its CU keep the vector pipe busy.
  uint4 nx[PF ? PER : 1];
  if (PF) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const uint64_t idx = g0r + (uint64_t)i * P2_THREADS + tid;
      nx[PF ? i : 0] = zero4;
      if (idx < n) nx[PF ? i : 0] = fetch(idx);
    }
  }
  for (int tt = 0; tt < NGRP; ++tt) {
    const uint64_t r0 = g0r + (uint64_t)tt * TILE;
    if (r0 >= n) break;
    const uint32_t nt = (uint32_t)min((uint64_t)TILE, n - r0);
    uint4 r[PER];
    if (PF) {
#pragma unroll
      for (int i = 0; i < PER; ++i) r[i] = nx[PF ? i : 0];
      if (tt + 1 < NGRP) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
          const uint64_t idx = r0 + TILE + (uint64_t)i * P2_THREADS + tid;
          nx[PF ? i : 0] = zero4;
          if (idx < n) nx[PF ? i : 0] = fetch(idx);
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        const uint64_t idx = r0 + (uint64_t)i * P2_THREADS + tid;
        r[i] = zero4;
        if (idx < n) r[i] = fetch(idx);
      }
    }
    if (tid < NSUB) hist[tid] = 0;
    lds_barrier();
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const uint32_t idx = (uint32_t)i * P2_THREADS + tid;
      if (idx < nt) atomicAdd(&hist[sub_of(r[i].w)], 1u);
    }
    lds_barrier();
    uint32_t g0 = 0;
    {
      // per-stream reservation + exclusive scan of the sub-bin sizes (one per thread, tid < NSUB)
      const int lane = tid & 63, wave = tid >> 6;
      const bool mine = tid < NSUB;
      const uint32_t x0 = mine ? hist[tid] : 0u;
      // returning atomic: issued here, consumed after the sort (its latency flies under it)
      if (x0 && !(v.dbg & CFRK_ABL_P2_NO_ATOMIC)) g0 = atomicAdd(&v.cnt2[b1 * NSUB + tid], x0);
      const uint32_t incl = dev_wave_scan_incl(x0);
      if (lane == 63) wtot[wave] = incl;
      lds_barrier();
      uint32_t bs = 0;
      for (int w = 0; w < wave; ++w) bs += wtot[w];
      if (mine) {
        loff[tid] = bs + incl - x0;
        hist[tid] = 0;                                     // from here on: fill cursor
      }
      lds_barrier();
    }
    // counting sort of the tile by sub-bin, in LDS
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const uint32_t idx = (uint32_t)i * P2_THREADS + tid;
      if (idx < nt) {
        const uint32_t sb = sub_of(r[i].w);
        sorted[loff[sb] + atomicAdd(&hist[sb], 1u)] = r[i];
      }
    }
    if (tid < NSUB) {
      const uint64_t leaf = ((uint64_t)b1 * NSUB + tid) >> 1;
      const uint32_t cls = tid & 1u;
      uint64_t cap = cls ? v.cap2c : v.cap2t;
      uint64_t at = (leaf >> v.sel_bits) * (v.cap2c + v.cap2t) + (cls ? 0 : v.cap2c);
      if (exact2) { cap = v.lcap[b1 * NSUB + tid]; at = v.lbase[b1 * NSUB + tid]; }
      const uint32_t lo = loff[tid];
      dabs[tid] = at + g0 - lo;
      const uint64_t room = cap > (uint64_t)g0 ? cap - g0 : 0;
      plim[tid] = (uint16_t)min((uint64_t)lo + room, (uint64_t)0xFFFFu);
    }
    lds_barrier();
    // copy out: consecutive lanes -> consecutive records of the same stream
    for (uint32_t p = tid; p < nt; p += P2_THREADS) {
      const uint4 rec = sorted[p];
      const uint32_t sb = sub_of(rec.w);
      if (v.dbg & CFRK_ABL_P2_LINEAR_OUT) {                // timing ablation: the tile goes out as it lies in LDS, bin after bin
        v.rec2[(uint64_t)b1 * (NSUB / 2) * (v.cap2c + v.cap2t) + r0 + p] = rec;
        continue;
      }
      if (p < (uint32_t)plim[sb]) { v.rec2[dabs[sb] + p] = rec; continue; }
      // the stream is full: park the record or raise the flag (below)
      const uint64_t leaf = ((uint64_t)b1 * NSUB + sb) >> 1;
      const uint32_t cls = sb & 1u;
      uint64_t cap = cls ? v.cap2c : v.cap2t;
      uint64_t at = (leaf >> v.sel_bits) * (v.cap2c + v.cap2t) + (cls ? 0 : v.cap2c);
      if (exact2) { cap = v.lcap[b1 * NSUB + sb]; at = v.lbase[b1 * NSUB + sb]; }
      const uint64_t dst = dabs[sb] + p - at;              // = the stream's reserved base + rank inside the segment
      // a stream position beyond 2^31: a single-key flood is on its way to wrapping the 32-bit cursor -- the host counts
      // the add through the HBM table instead (checked HERE, on the full-stream path only: a flood fills its stream first)
      if (dst >= 0x80000000ull) v.stats[ST_CWRAP] = 1;
      if (dst < cap) v.rec2[at + dst] = rec;
      else if (exact2) spill_record(rec, k, canon != 0, t);      // cannot happen: cap is the exact count
      else {
        // too small by a little: park the record (the host counts the parked ones through the
        // HBM table); by a lot: the cursors keep counting and the host redoes P2 with exact sizes
        // (once the flag is up nobody takes a number any more: 10^7 atomics on one word are slow)
        if (*(volatile uint64_t *)&v.stats[ST_L2OVF] == 0) {
          const unsigned long long o = atomicAdd((unsigned long long *)&v.stats[ST_OVFN], 1ull);
          if (o < v.ovf_cap) v.ovf[o] = rec;
          else v.stats[ST_L2OVF] = 1;
        }
      }
    }
    lds_barrier();                                       // sorted/loff/dabs are reused by the next tile
  }
}

// PERSISTENT form (stand-alone kernel): nwg workgroups (a multiple of 8); workgroup w belongs to XCD
// group w % 8 and that group walks ITS bins one after the other -- the group's items are numbered
// bin after bin from the records the bins really hold (no empty items), and workgroup j of the group
// takes items j, j + nwg/8, ...
template <int PER, bool EX, bool PF>
__device__ __forceinline__ void p2_role(uint4 *pool, uint32_t wg, uint32_t nwg, int k, int canon, const MspView &v, const TableView &t) {
  constexpr int TILE = P2_THREADS * PER;
  uint32_t *const gpre = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(pool) + P2Lds<PER>::GPRE);   // exclusive prefix of the group's items per bin
  constexpr int BPG = B1 / NXCD;                 // bins per XCD group
  static_assert(P2_THREADS == BPG * 16, "sixteen threads add up a bin's sub-regions");
  const int tid = threadIdx.x;
  const bool exact1 = EX && v.exact1;
  const uint32_t xg = wg & (NXCD - 1), j0 = wg / NXCD, nj = nwg / NXCD;
  // items per bin of this group: sixteen threads per bin add the sub-region sizes
  {
    const uint32_t i = (uint32_t)tid >> 4, part = (uint32_t)tid & 15u, b = xg + NXCD * i;
    uint32_t sum = 0;
    for (uint32_t sr = part; sr < v.nxg; sr += 16u) {
      const uint32_t reg = l1_reg(b, sr);
      sum += (uint32_t)min((uint64_t)v.cnt1[reg], exact1 ? (uint64_t)v.rcap[reg] : v.cap1);
    }
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) sum += __shfl_xor(sum, d);
    if (part == 0) gpre[i + 1] = (sum + (uint32_t)(TILE * P2_GROUP) - 1u) / (uint32_t)(TILE * P2_GROUP);
    if (tid == 0) gpre[0] = 0;
    lds_barrier();
    if (tid == 0) for (int q = 1; q <= BPG; ++q) gpre[q] += gpre[q - 1];
    lds_barrier();
  }
  const uint32_t nitems = gpre[BPG];
  uint32_t bi = 0;                               // bin of the current item (items grow: the cursor only moves forward)
  for (uint32_t item = j0; item < nitems; item += nj) {
    while (gpre[bi + 1] <= item) ++bi;
    p2_item<PER, EX, PF, P2_GROUP>(pool, xg + NXCD * bi, item - gpre[bi], k, canon, v, t);
  }
}

__global__ __launch_bounds__(P2_THREADS, 4) void msp_p2_kernel(int k, int canon, MspView v, TableView t) {
  __shared__ uint4 pool[(P2Lds<P2_PER>::BYTES + 15) / 16];
  p2_role<P2_PER, true, true>(pool, blockIdx.x, gridDim.x, k, canon, v, t);
}

// ---------------------------------------------------------------------------------------- P3
// rare path, kept out of line so that the hot loop stays small
__device__ __noinline__ void spill_kmer(TableView t, uint64_t key, uint32_t add) {
  if (key == CFRK_EMPTY_KEY) {   // k = 32, all T, forward strand
    atomicAdd((unsigned long long *)&t.stats[ST_ONES], (unsigned long long)add);
    return;
  }
  t.stats[ST_SPILLED] = 1;
  dev_count_event(&t.stats[ST_AUX1]);
  table_add1(t, key, add);
}

// The leaf's k-mer table is TS/2 buckets of two keys (one ds_read_b128 fetches a bucket), linear
// probing over buckets.
constexpr int NBUCKET = TS / 2;
__device__ __forceinline__ uint32_t lds_bucket(uint64_t key) {
  return (((uint32_t)key ^ (uint32_t)(key >> 32)) * 0x9E3779B1u) >> (32 - (TS_LOG - 1));
}

// Every instruction, vector or scalar, costs an issue slot, and a wave runs a probe loop for as
// long as its slowest lane: the step below is written for instruction count (one CAS-or-match
// decision per bucket, no per-lane probe counter), and callers feed waves with records of equal
// length.
constexpr int KT_TRIPS = 64;
constexpr int KT_TRIPS_SPLIT = 16;          // (buckets of two slots)

// One bucket attempt for one key per lane: count on a match, claim an empty slot, else move on.
// The lane's state is its bucket index b with KT_DONE or-ed in once the key is counted (or the
// lane had none): written to keep lane masks out of loop-carried values and control-flow merges
// (each costs the compiler three scalar instructions) -- the only branch is the rare claim, its
// outcome lands in a VGPR, and lanes with nothing to count add 0.
// SAT: the count saturates at CFRK_COUNT_MAX (table.h: sat_add) -- the merge of lists whose counts nothing bounds;
// the leaf kernel's own counts cannot overflow (HUGE_LEAF)
constexpr uint32_t KT_DONE = 0x80000000u;
// Path counters of the leaf kernel, in an ABLATION BUILD only and there only with CFRK_ABL_P3_PATHS set (msp.h; read by
// cfrk_debug_p3_paths, tools/p3_paths.py): how often the expansion of the distinct complete runs takes which way.  The
// product build has none of it, and the timing ablations run without it (the counters are global atomics).
enum { P3C_LEAVES_1 = 0, P3C_LEAVES_2, P3C_LEAVES_3,   // leaves whose record table is listed, by the lanes per run 1024 threads gave before every leaf took three
       P3C_CEXP_WAVES, P3C_CEXP_SLOW,                  // wave-calls of the complete runs' expansion with notes / those that leave the one-walk path
       P3C_KT_CLAIMED, P3C_KT_MATCHED,                 // k-mer table: keys of that expansion that claimed an empty slot / found their key
       P3C_RT_ENTRIES, P3C_RT_TWINNED, P3C_RT_PALIN,   // record-table entries / whose reverse complement is an entry too / that are their own
       P3C_N };
#ifdef CFRK_ABLATIONS
__device__ unsigned long long p3_paths[P3C_N];
#define P3_COUNT(i, n) atomicAdd(&p3_paths[i], (unsigned long long)(n))
#else
#define P3_COUNT(i, n) ((void)0)
#endif
template <bool SAT = false, bool PATHS = false>
__device__ __forceinline__ void kt_try(unsigned long long *keys, uint32_t *cnts, uint64_t key, uint32_t &b,
                                       uint32_t add) {
  const bool p = (int32_t)b >= 0;
  const uint32_t bb = b & (NBUCKET - 1);
  const ulonglong2 q = reinterpret_cast<const ulonglong2 *>(keys)[bb];
  const bool m0 = q.x == key, m1 = q.y == key;
  const bool e0 = q.x == CFRK_EMPTY_KEY, e1 = q.y == CFRK_EMPTY_KEY;
  const bool hit = m0 || m1;
  const uint32_t s = 2 * bb + ((m0 || (!m1 && e0)) ? 0u : 1u);  // matching slot, else first empty, else any
  uint32_t won = 0u;
  if (p && !hit && (e0 || e1)) {
    const unsigned long long old = atomicCAS(&keys[s], (unsigned long long)CFRK_EMPTY_KEY, (unsigned long long)key);
    won = (old == CFRK_EMPTY_KEY || old == key) ? 1u : 0u;      // lost to another key: same bucket again
  }
  const bool ok = hit || won != 0u;
#ifdef CFRK_ABLATIONS
  if (PATHS) {
    const unsigned long long mh = __ballot(p && hit), mw = __ballot(p && !hit && won != 0u);
    if ((threadIdx.x & 63) == 0) {
      if (mh) P3_COUNT(P3C_KT_MATCHED, __popcll(mh));
      if (mw) P3_COUNT(P3C_KT_CLAIMED, __popcll(mw));
    }
  }
#endif
  if (SAT) {
    if (p && ok) {
      const uint32_t old = atomicAdd(&cnts[s], add);
      if (old > CFRK_COUNT_MAX - add) atomicExch(&cnts[s], CFRK_COUNT_MAX);
    }
  } else atomicAdd(&cnts[s], (p && ok) ? add : 0u);
  const bool full = !(hit || e0 || e1);
  const uint32_t nb = full ? ((bb + 1) & (NBUCKET - 1)) : bb;
  b = (p && !ok) ? nb : (b | KT_DONE);
}

// count one key per lane (valid lanes) `add` times, saturating; every lane of the wave must call
__device__ __forceinline__ void kt_count(unsigned long long *keys, uint32_t *cnts, uint64_t key, uint32_t add,
                                         bool valid, const TableView &t) {
  uint32_t b = lds_bucket(key) | (valid ? 0u : KT_DONE);
  add = min(add, CFRK_COUNT_MAX);
  for (int it = 0; it < KT_TRIPS && __ballot((int32_t)b >= 0); ++it) kt_try<true>(keys, cnts, key, b, add);
  if ((int32_t)b >= 0) spill_kmer(t, key, add);
}

// Subset of a leaf's key space (a leaf with more distinct k-mers than its LDS table holds is
// counted in several passes, each over the keys whose selector bits equal `val`): the selector
// comes from the same product as the bucket index, but from bits the bucket does not use.
struct KeySubset { uint32_t mask, val; };
__device__ __forceinline__ bool in_subset(uint64_t key, KeySubset ss) {
  return (((((uint32_t)key ^ (uint32_t)(key >> 32)) * 0x9E3779B1u) >> 8) & ss.mask) == ss.val;
}

// expand one record per lane (valid lanes), two k-mers per step; every lane of the wave must call.
// Only keys of subset `ss` are counted.  A key that finds no room is counted in the HBM table when
// ovf == nullptr; otherwise *ovf (an LDS flag) is raised and the caller redoes the subset in
// halves -- and waves that see the flag up stop working on a pass that is lost anyway.
// PATHS (an ablation build's caller with CFRK_ABL_P3_PATHS set, for the complete runs' expansion): count the paths taken.
template <bool CANON, bool PATHS = false>
__device__ __forceinline__ void count_record_v2(unsigned long long *keys, uint32_t *cnts, uint4 rec, uint32_t add,
                                                bool valid, int k, uint64_t kmask, int rcsh,
                                                const TableView &t, KeySubset ss = KeySubset{0u, 0u},
                                                uint32_t *ovf = nullptr, int part = 0, int parts = 1,
                                                const uint8_t *tb = nullptr, uint32_t tb_n = 0u,
                                                const uint8_t *tb2 = nullptr, uint32_t tb2_n = 0u) {
  // tb[0 .. tb_n): lengths (in k-mers) of the truncated runs that are prefixes of this record: k-mer J
  // of the record is counted once more for every one of them that is longer than J
  // tb2[0 .. tb2_n) (canonical, with tb): the same lengths noted with the record's STRAND TWIN, whose k-mers are this
  // record's in reverse order: k-mer J of n is counted once more for every one of them with t >= n - J
  if (ovf && *(volatile uint32_t *)ovf) return;
  P3_MARK("P3_PART_XSETUP");
  // a record may be shared by `parts` lanes (1 .. 6), each expanding a contiguous share of its k-mers
  const int nall = valid ? (int)(rec.w & 63u) + 1 : 0;
  // (ceil(nall / parts), nall <= 64, by a multiply: `parts` is uniform and the reciprocal a scalar)
  const int per = (parts <= 3) ? ((parts == 1) ? nall : (parts == 2) ? ((nall + 1) >> 1) : ((nall + 2) / 3))
                               : (int)(((uint32_t)(nall + parts - 1) * (65536u / (uint32_t)parts + 1u)) >> 16);
  const int j0 = part * per;
  const int nk = max(min(nall, j0 + per) - j0, 0);
  uint64_t hi = ((uint64_t)rec.x << 32) | rec.y;
  uint64_t lo = (uint64_t)rec.z << 32;
  if (parts != 1 && j0) {                          // start at k-mer j0: 1 <= j0 <= 31
    hi = (hi << (2 * j0)) | (lo >> (64 - 2 * j0));
    lo <<= 2 * j0;
  }
  uint64_t fwd = hi >> (64 - 2 * k);
  uint64_t rc = CANON ? dev_revcomp64(fwd, k) : 0;
  uint64_t T = (k == 32) ? lo : ((hi << (2 * k)) | (lo >> (64 - 2 * k)));
  // (canonical counting) the lists are walked ONCE when every lane of the wave has at most 8 k-mers
  // to expand and at most 127 noted runs: a lane counts its list's entries by d = clamp(length - j0,
  // 0, 8) in nine 7-bit fields of one 64-bit register; k-mer j0 + q is counted once more for every
  // entry with d > q, i.e. the fields' suffix sums, kept as eight bytes (msp2.hip: count_record2).
  // The forward-strand instantiation keeps the loop per k-mer pair: it is out of registers.
  unsigned long long exq = 0ull;
  const bool tb_fast = CANON && tb && !__ballot(valid && (nk > 8 || tb_n > 127u));
  if (tb) {
    P3_MARK("P3_PART_XWALK");
#ifdef CFRK_ABLATIONS
    if (PATHS && (threadIdx.x & 63) == 0) { P3_COUNT(P3C_CEXP_WAVES, 1); if (!tb_fast) P3_COUNT(P3C_CEXP_SLOW, 1); }
#endif
  }
  if (tb_fast) exq = noted_counts8(tb, tb_n, j0);
  for (int j = 0; __ballot(j < nk); j += 2) {
    P3_MARK("P3_PART_XSTEP");
    uint32_t add0 = add, add1 = add;
    if (tb_fast) {
      add0 += (uint32_t)(exq >> (8 * (j & 7))) & 255u;
      add1 += (uint32_t)(exq >> (8 * ((j + 1) & 7))) & 255u;
    } else if (tb) {
      const uint32_t J = (uint32_t)(j0 + j);
      for (uint32_t e = 0; __ballot(e < tb_n); ++e) {       // (as many steps as the wave's longest list)
        const uint32_t tv = (e < tb_n) ? (uint32_t)tb[e] : 0u;
        add0 += (tv > J) ? 1u : 0u;
        add1 += (tv > J + 1u) ? 1u : 0u;
      }
    }
    const uint64_t key0 = (CANON && rc < fwd) ? rc : fwd;
    uint32_t nb = (uint32_t)(T >> 62);
    T <<= 2;
    fwd = ((fwd << 2) | nb) & kmask;
    if (CANON) rc = (rc >> 2) | ((uint64_t)(3u - nb) << rcsh);
    const uint64_t key1 = (CANON && rc < fwd) ? rc : fwd;
    nb = (uint32_t)(T >> 62);
    T <<= 2;
    fwd = ((fwd << 2) | nb) & kmask;
    if (CANON) rc = (rc >> 2) | ((uint64_t)(3u - nb) << rcsh);
    bool p0 = j < nk && in_subset(key0, ss), p1 = j + 1 < nk && in_subset(key1, ss);
    if (!CANON && k == 32) {
      // forward-strand all-T 32-mer collides with the EMPTY marker: side counter
      if (p0 && key0 == CFRK_EMPTY_KEY) { spill_kmer(t, key0, add0); p0 = false; }
      if (p1 && key1 == CFRK_EMPTY_KEY) { spill_kmer(t, key1, add1); p1 = false; }
    }
    uint32_t b0 = lds_bucket(key0) | (p0 ? 0u : KT_DONE), b1 = lds_bucket(key1) | (p1 ? 0u : KT_DONE);
    // (a pass that may still be split gives up early: probing a nearly full table is the slow way
    //  to find out that it is full)
    // (... but not the pass over the WHOLE leaf: an unlucky cluster in a table that is a third full must not
    //  split a leaf that fits -- a split leaf has two segments in the result list and no entry in the leaf
    //  index, which the export by leaf needs: at C3's size a handful of the 65 536 leaves were split)
    const int trips = ovf ? (ss.mask == 0u ? KT_TRIPS : KT_TRIPS_SPLIT) : KT_TRIPS;
    for (int it = 0; it < trips && __ballot((int32_t)(b0 & b1) >= 0); ++it) {
      kt_try<false, PATHS>(keys, cnts, key0, b0, add0);
      kt_try<false, PATHS>(keys, cnts, key1, b1, add1);
    }
    if (ovf) {
      if ((int32_t)(b0 & b1) >= 0) *ovf = 1u;
    } else {
      if ((int32_t)b0 >= 0) spill_kmer(t, key0, add0);
      if ((int32_t)b1 >= 0) spill_kmer(t, key1, add1);
    }
  }
}

// Record table: at high coverage most complete super-k-mer records of a leaf are byte-identical
// (the same genome locus seen by many reads).  Entries are {R0,R1,R2,meta},
// meta = count << 6 | (n-1); meta == RT_EMPTY empty, RT_LOCK while the claiming lane writes the
// bases.
constexpr int RT_LOG = 10, RT = 1 << RT_LOG;
constexpr int TL_PER = 4, TL_CAP = TL_PER * 1024;     // length-sorted list of truncated runs (indices)
constexpr int FL_CAP = 1024;                          // truncated runs without a complete twin, when the others are anchored
static_assert(TL_CAP <= (1 << 14), "list positions are 14 bits");
static_assert(RT == P3_THREADS, "phase 2 lists the record table with one slot per thread");
constexpr uint32_t RT_LOCK = 0xFFFFFFFFu;

// (rotations decorrelate the three base words, one multiply spreads them into the top bits: the
// bases of a record are sequence, already close to uniform)
__device__ __forceinline__ uint32_t rtab_slot(uint4 rec, int log_slots = RT_LOG) {
  const uint32_t t = rec.x ^ __builtin_amdgcn_alignbit(rec.y, rec.y, 11) ^ __builtin_amdgcn_alignbit(rec.z, rec.z, 21) ^
                     ((rec.w & 63u) << 26);
  return (t * 0x9E3779B1u) >> (32 - log_slots);
}

// Every instruction -- vector or scalar -- costs an issue slot here, so the probe step is written
// for instruction count: identity is one OR-reduction of XORs (EMPTY and LOCK carry low header
// bits no record has, so they never compare equal), and the loop is bounded by a wave-uniform
// trip counter instead of per-lane probe counts.
constexpr uint32_t RT_EMPTY = 62u;                 // n-1 = 62 does not occur (n <= 32)
constexpr int RT_TRIPS = 96;

__device__ __forceinline__ uint32_t rtab_diff(uint4 e, uint4 rec) {
  return (e.x ^ rec.x) | (e.y ^ rec.y) | (e.z ^ rec.z) | ((e.w ^ rec.w) & 63u);
}

// The record table of the ordinary path is keyed by the record's FIRST k-mer: a truncated run that
// is a prefix of a complete run shares it, so it finds its complete twin by probing from the same
// slot (a suffix is a prefix of the other strand's twin after a reverse complement).
__device__ __forceinline__ uint32_t rtab_prod_k(uint4 rec, int k) {
  const uint32_t y = (k >= 32) ? rec.y : (rec.y & ~(0xFFFFFFFFu >> (2 * k - 32)));   // 16 <= k: the top 2k-32 bits of y
  const uint32_t t = rec.x ^ __builtin_amdgcn_alignbit(y, y, 11);
  return t * 0x9E3779B1u;
}
__device__ __forceinline__ uint32_t rtab_slot_k(uint4 rec, int k, int log_slots) {
  return rtab_prod_k(rec, k) >> (32 - log_slots);
}
// do the first `len` bases (32 <= 2*len <= 96 bits) of two records agree?
__device__ __forceinline__ bool rec_prefix_equal(uint4 e, uint4 r, int len) {
  const int rb = 2 * len - 32;                     // bits beyond the first word: 0 .. 64
  const uint32_t my = (rb >= 32) ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> rb);
  const uint32_t mz = (rb <= 32) ? 0u : ((rb >= 64) ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> (rb - 32)));
  return ((e.x ^ r.x) | ((e.y ^ r.y) & my) | ((e.z ^ r.z) & mz)) == 0u;
}
// reverse complement of a record's run (len bases, 16 <= len <= 48); header word unchanged
__device__ __forceinline__ uint4 revcomp_record(uint4 rec, int len) {
  auto rcw = [](uint32_t x) {                      // reverse the 16 bases of a word and complement them
    x = __brev(x);
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    return ~x;
  };
  // the 48-base field reversed: the reverse complement preceded by 48 - len complemented pad bases
  const uint64_t A = ((uint64_t)rcw(rec.z) << 32) | rcw(rec.y);
  const uint64_t B = (uint64_t)rcw(rec.x) << 32;
  const int s = 2 * (48 - len);                    // 0 .. 64: shift the pad out at the top
  uint64_t hi, lo;
  if (s == 0) { hi = A; lo = B; }
  else if (s < 64) { hi = (A << s) | (B >> (64 - s)); lo = B << s; }
  else { hi = B; lo = 0; }
  uint4 out = rec;
  out.x = (uint32_t)(hi >> 32); out.y = (uint32_t)hi; out.z = (uint32_t)(lo >> 32);
  return out;
}

// insert-or-count one record per lane; the lane's state is its slot h with RT_DONE or-ed in once
// the record is placed (lanes without a record start that way).  On return lanes still without
// RT_DONE found no place.
constexpr uint32_t RT_DONE = 0x80000000u;
// inc = the record's weight << 6: 1 << 6 for a record straight from a read, its multiplicity when
// the stream already holds deduplicated runs (the owner side of the multi-GPU exchange)
__device__ __forceinline__ void rtab_insert_loop(uint4 *rtab, uint4 rec, uint32_t &h, uint32_t mask = RT - 1,
                                                 int trips = RT_TRIPS, uint32_t inc = 1u << 6) {
  uint32_t *rmeta = reinterpret_cast<uint32_t *>(rtab);
  const uint32_t nm1 = rec.w & 63u;
  for (int it = 0; it < trips && __ballot((int32_t)h >= 0); ++it) {
    const bool p = (int32_t)h >= 0;
    const uint32_t hh = h & mask;
    const uint4 e = rtab[hh];
    const bool match = rtab_diff(e, rec) == 0u;
    const bool empty = e.w == RT_EMPTY;
    uint32_t won = 0u;
    if (p && empty) {
      if (atomicCAS(&rmeta[4 * hh + 3], RT_EMPTY, RT_LOCK) == RT_EMPTY) {
        rmeta[4 * hh + 0] = rec.x; rmeta[4 * hh + 1] = rec.y; rmeta[4 * hh + 2] = rec.z;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        atomicExch(&rmeta[4 * hh + 3], inc | nm1);
        won = 1u;
      }
    }
    atomicAdd(&rmeta[4 * hh + 3], (p && match) ? inc : 0u);
    // an empty slot lost to another lane, or a locked one, is read again; a slot holding another
    // record sends the lane on
    const bool stay = match || empty || e.w == RT_LOCK;
    const uint32_t nh = stay ? hh : ((hh + 1) & mask);
    h = (p && !match && won == 0u) ? nh : (h | RT_DONE);
  }
}

// Second chance for a leaf whose complete runs do not fit the record table (a small k has short
// windows, hence ~2/(W+1) distinct runs per locus and strand: ~600 per leaf at k = 21 where k = 31
// has ~300, and heavy leaves several times that).  Before phase 2 the k-mer table is still empty,
// so the whole LDS pool (k-mer table + record table, 64 KB) serves as one 4096-slot record table;
// the distinct runs with their multiplicities then overwrite the head of the leaf's complete-run
// stream in HBM -- this workgroup is its only reader and has read all of it -- and phase 2 expands
// them from there.  Returns the number of distinct runs, or ~0 if even that table is too small
// (the leaf is then counted k-mer by k-mer from its streams).  Out of line: a rare path that would
// otherwise cost the hot path registers.
constexpr int BT_LOG = 12, BT = 1 << BT_LOG, BT_TRIPS = 192;
constexpr int BT_MIN_RUNS = 2 * BT;
// occupied slots of the pool-wide record table -> head of the stream; returns their number
__device__ __noinline__ uint32_t p3_compact(uint4 *pool, uint4 *stream, uint32_t *wsum) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t *meta = reinterpret_cast<const uint32_t *>(pool);
  // a thread owns BT / P3_THREADS consecutive slots (two passes over LDS: an array of entries
  // would live in scratch memory)
  constexpr int PER = BT / P3_THREADS;
  uint32_t mine = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) mine += (meta[4 * (PER * tid + i) + 3] != RT_EMPTY) ? 1u : 0u;
  uint32_t incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(incl, d);
    if (lane >= d) incl += y;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint32_t base = 0, total = 0;
  for (int w = 0; w < P3_THREADS / 64; ++w) {
    const uint32_t x = wsum[w];
    base += (w < wave) ? x : 0u;
    total += x;
  }
  uint32_t at = base + incl - mine;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const uint4 e = pool[PER * tid + i];
    if (e.w != RT_EMPTY) stream[at++] = e;
  }
  // the list is read back by the waves of this workgroup only: workgroup scope (one CU, whose
  // vector cache its own stores keep current) -- an agent-scope release would write back the L2
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  return total;
}
// occupied slots of the ordinary record table (one per thread) -> head of the stream; returns their number
__device__ __noinline__ uint32_t p3_dump_rtab(const uint4 *rtab, uint4 *stream, uint32_t *wsum) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint4 e = rtab[tid];
  const bool occ = e.w != RT_EMPTY;
  const unsigned long long m = __ballot(occ);
  if (lane == 0) wsum[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t base = 0, total = 0;
  for (int w = 0; w < P3_THREADS / 64; ++w) {
    const uint32_t x = wsum[w];
    base += (w < wave) ? x : 0u;
    total += x;
  }
  if (occ) stream[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = e;
  return total;
}

__device__ __noinline__ uint32_t p3_big_dedupe(uint4 *pool, uint4 *stream, uint64_t n1, uint32_t *wsum, uint32_t *fail, bool weighted) {
  const int tid = threadIdx.x;
  __syncthreads();                               // every thread has read *fail (that is why we are here)
  for (int s = tid; s < BT; s += P3_THREADS) pool[s] = make_uint4(0u, 0u, 0u, RT_EMPTY);
  if (tid == 0) *fail = 0u;
  __syncthreads();
  for (uint64_t r = tid; r < ((n1 + 63) & ~63ull); r += P3_THREADS) {
    const bool valid = r < n1;
    uint4 rec = make_uint4(0u, 0u, 0u, 0u);
    if (valid) rec = stream[r];
    uint32_t h = valid ? rtab_slot(rec, BT_LOG) : RT_DONE;
    rtab_insert_loop(pool, rec, h, BT - 1, BT_TRIPS, weighted ? ((rec.w >> 6) << 6) : (1u << 6));
    if ((int32_t)h >= 0) *fail = 1u;
  }
  __syncthreads();
  if (*fail) return 0xFFFFFFFFu;
  return p3_compact(pool, stream, wsum);
}

// HUGE LEAF: 2^25 records or more in one leaf (half a gigabyte: a single-key flood -- a homopolymer, one amplicon
// sequenced 10^8 times).  The record table keeps a run's multiplicity in 26 bits and the LDS k-mer counts are 32-bit:
// below this size neither can overflow (2^25 records x 32 k-mers < 2^31); at or above it the leaf is not counted in
// LDS at all but k-mer by k-mer in the HBM table, whose adds SATURATE (table.h: sat_add).  Slow and exact.
// (A sender of the runs exchange does not deduplicate a leaf of 2^19 complete runs or more, so that the multiplicities
// an owner adds up for one run stay below 64 ranks x 2^19 + 2^25 = 2^26.)
constexpr uint64_t HUGE_LEAF = 1ull << 25;
constexpr uint64_t HUGE_LEAF_SENDER = 1ull << 19;
// (a kernel of its own, launched behind the leaf kernel: every thread looks at ONE leaf's sizes and normally finds
//  nothing -- a few microseconds; inside the leaf kernel the same loop cost the canonical instantiation four more
//  spilled dwords)
__global__ __launch_bounds__(256) void msp_huge_leaves_kernel(int k, int canon, int weighted, uint32_t nl /* leaves of this pass / owner */, MspView v, TableView t) {
  __shared__ uint32_t nhuge, huge[256];
  if (threadIdx.x == 0) nhuge = 0;
  __syncthreads();
  const uint32_t i0 = blockIdx.x * 256u + threadIdx.x;
  if (i0 < nl) {
    const uint32_t leaf = (i0 << v.sel_bits) | v.sel_val;
    const uint64_t nt = min((uint64_t)v.cnt2[NCLS * leaf + 0], v.exact ? (uint64_t)v.lcap[NCLS * leaf + 0] : v.cap2t);
    const uint64_t n1 = min((uint64_t)v.cnt2[NCLS * leaf + 1], v.exact ? (uint64_t)v.lcap[NCLS * leaf + 1] : v.cap2c);
    if (nt + n1 >= HUGE_LEAF) huge[atomicAdd(&nhuge, 1u)] = i0;
  }
  __syncthreads();
  for (uint32_t q = 0; q < nhuge; ++q) {
    const uint32_t i = huge[q], leaf = (i << v.sel_bits) | v.sel_val;
    const uint64_t nt = min((uint64_t)v.cnt2[NCLS * leaf + 0], v.exact ? (uint64_t)v.lcap[NCLS * leaf + 0] : v.cap2t);
    const uint64_t n1 = min((uint64_t)v.cnt2[NCLS * leaf + 1], v.exact ? (uint64_t)v.lcap[NCLS * leaf + 1] : v.cap2c);
    const uint4 *c1 = v.exact ? v.rec2 + v.lbase[NCLS * leaf + 1] : v.rec2 + (uint64_t)i * (v.cap2c + v.cap2t);
    const uint4 *c0 = v.exact ? v.rec2 + v.lbase[NCLS * leaf + 0] : c1 + v.cap2c;
    for (uint64_t j = threadIdx.x; j < n1 + nt; j += 256) {
      const uint4 rec = (j < n1) ? c1[j] : c0[j - n1];
      spill_record(rec, k, canon != 0, t, (weighted && j < n1) ? (rec.w >> 6) : 1u);
    }
  }
}

// mode: P3_WEIGHTED = the complete stream holds DISTINCT runs, header word = multiplicity << 6 | n-1
// (what msp_dedupe_export_kernel leaves behind; from several ranks): an owner counting the runs it received.
// SHARED: 2^sub_bits workgroups per leaf, each taking the records whose sub-value -- the extra
// minimizer-hash bits in the header's top byte, written by msp_p1b_kernel<.., true> -- names it.  Every
// occurrence of a k-mer has the same minimizer, so the workgroups' key sets are disjoint and every record
// is expanded once, where key-subset passes expand every record in every pass (the c5 shape at k = 31:
// 15 000 distinct k-mers per leaf).  The workgroups of a leaf run next to each other on one XCD, whose L2
// serves all but the first read of the leaf's streams (msp2.hip: msp2_p3_kernel<.., true>).
// P3_EXPORT = stop after the deduplication and leave the leaf's distinct complete runs at the head of its
// stream (leaf_n = their number).  The host no longer asks for it (msp_dedupe_export_kernel does that job
// with eight workgroups per CU), but the compiler allocates the hot loops' registers better with the
// branch in place: without it the canonical kernel spills six dwords instead of two and P3 takes 7.10
// instead of 6.80 ms on C3.
constexpr uint32_t P3_EXPORT = 1u, P3_WEIGHTED = 2u;
// LISTS (round 5, the owner side of the PIPELINED runs exchange): the leaf's runs are not two streams in rec2 but the
// N lists its ranks sent, read IN PLACE from the receive buffer -- rank r's segment of this group starts with a header
// (row 0: {rows used, leaves, first local leaf, magic}, then one uint4 {row offset, distinct, truncated, noted} per local
// leaf), and a leaf's rows are [distinct complete runs, header = multiplicity << 6 | n-1][truncated runs][notes, eight per
// row].  A note is turned back into the run it stands for (the first n k-mers of its twin) where it is read.  No layout
// kernels, no scatter pass, no host synchronisation before the leaf kernel.  An instantiation of its own
// (msp_p3_lists_kernel): the one-GPU kernel's code and registers are what they were.
template <bool CANON, bool SHARED, bool LISTS>
__device__ __forceinline__ void p3_body(int k, uint32_t mode, const MspView &v, const TableView &t, const P3ListsT<LISTS> &lx) {
  // k-mer table (keys, counts) and record table in one allocation: p3_big_dedupe uses all of it
  __shared__ uint4 pool[BT];
  static_assert(BT * 16 == TS * 12 + RT * 16, "the pool is exactly the k-mer table plus the record table");
  unsigned long long *const keys = reinterpret_cast<unsigned long long *>(pool);
  uint32_t *const cnts = reinterpret_cast<uint32_t *>(pool + TS / 2);
  uint4 *const rtab = pool + TS / 2 + TS / 4;
  __shared__ uint16_t occ_list[RT];
  // truncated runs: either a length-sorted list of stream positions (tlist), or -- with the record
  // table resident -- their lengths grouped by the complete twin they are a prefix of (th: per
  // record-table slot the group's start, tbytes: the lengths) plus the few without a twin (flist)
  __shared__ uint32_t tmem[RT + 1 + TL_CAP / 4 + 2];
  uint16_t *const tlist = reinterpret_cast<uint16_t *>(tmem);
  uint32_t *const th = tmem;
  uint8_t *const tbytes = reinterpret_cast<uint8_t *>(tmem + RT + 1);
  static_assert(sizeof(uint16_t) * TL_CAP <= sizeof(uint32_t) * (RT + 1 + TL_CAP / 4), "tlist fits the same memory");
  __shared__ uint16_t flist[FL_CAP];
  __shared__ uint32_t nfb, nfl;
  __shared__ uint32_t nhist[32], thist[32];
  __shared__ uint32_t wsum[P3_THREADS / 64];
  __shared__ uint32_t nocc;
  __shared__ uint32_t wg_total;
  __shared__ unsigned long long wg_base;
  __shared__ uint32_t rt_fail;                   // the record table ran out of room: second chance, then count from the streams
  __shared__ uint32_t kovf;                      // the k-mer table ran out of room in this pass
  __shared__ uint32_t stk[40];                   // key subsets still to count: bits << 16 | value
  __shared__ int sp;
  __shared__ uint32_t leaf_total, nseg;
  const int tid = threadIdx.x, lane = tid & 63;
  // (the grid holds the leaves of this pass only: were the others launched and left at once, the
  //  pass's leaves -- equal low bits -- would all sit on 8 / 2^sel_bits of the 8 XCDs)
  // (shared leaves: workgroup b goes to XCD b % 8 -- eight leaves side by side, a leaf's workgroups one after the other)
  const uint32_t sub_bits = SHARED ? v.sub_bits : 0u, smask = (1u << sub_bits) - 1u;
  const uint32_t vq = blockIdx.x >> 3, rsel = vq & smask;
  const uint32_t leaf = ((SHARED ? (((vq >> sub_bits) << 3) | (blockIdx.x & 7u)) : blockIdx.x) << v.sel_bits) | v.sel_val;
  auto mine = [&](uint32_t w) { return !SHARED || ((w >> 24) & smask) == rsel; };
  // LISTS: rank r's lists of this leaf -- l_base[r] = its first row, complete runs [l_cpre[r], l_cpre[r+1]) of the leaf's
  // complete "stream", truncated runs + notes [l_tpre[r], l_tpre[r+1]) of its truncated one (l_nu[r] records, then the notes)
  __shared__ uint32_t l_cpre[LISTS ? 65 : 1], l_tpre[LISTS ? 65 : 1], l_nu[LISTS ? 64 : 1];
  __shared__ const uint4 *l_base[LISTS ? 64 : 1];
  uint64_t nt_ = 0, n1_ = 0;
  if constexpr (LISTS) {
    if (tid < 64) {
      const int r = tid;
      uint32_t nd = 0, nu = 0, na = 0;
      const uint4 *base = nullptr;
      if (r < lx.parts) {
        const uint4 *hdr = lx.packed + lx.rr.rstart[r];
        const uint64_t rows = lx.rr.rows[r], hrows = 1ull + lx.lcount;
        bool ok = rows >= hrows;
        if (ok) { const uint4 h0 = hdr[0]; ok = h0.y == lx.lcount && h0.z == lx.ll0 && h0.w == RUNS2_MAGIC; }
        if (ok) {
          const uint4 e = hdr[1u + blockIdx.x];
          const uint64_t tot = (uint64_t)e.y + e.z + (e.w + (uint32_t)NOTES_PER_ROW - 1u) / (uint32_t)NOTES_PER_ROW;
          // (a segment that does not add up, or notes without a run they could point at, is not followed)
          if ((uint64_t)e.x + tot <= rows - hrows && (e.w == 0u || e.y != 0u)) { nd = e.y; nu = e.z; na = e.w; base = hdr + hrows + e.x; }
          else if (tot) ok = false;
        }
        if (!ok) v.stats[ST_OVERFLOW] = 1;                 // (reported by finish / digest: the result would be incomplete)
      }
      const uint32_t ci = dev_wave_scan_incl(nd), ti = dev_wave_scan_incl(nu + na);
      l_cpre[r] = ci - nd; l_tpre[r] = ti - (nu + na); l_nu[r] = nu; l_base[r] = base;
      if (r == 63) { l_cpre[64] = ci; l_tpre[64] = ti; }
    }
    __syncthreads();
    n1_ = l_cpre[64]; nt_ = l_tpre[64];
  } else {
    nt_ = min((uint64_t)v.cnt2[NCLS * leaf + 0], v.exact ? (uint64_t)v.lcap[NCLS * leaf + 0] : v.cap2t);  // truncated runs
    n1_ = min((uint64_t)v.cnt2[NCLS * leaf + 1], v.exact ? (uint64_t)v.lcap[NCLS * leaf + 1] : v.cap2c);  // complete runs
  }
  const uint64_t nt = nt_, n1 = n1_;
  const uint4 *leaf_rec = LISTS ? nullptr : (v.exact ? v.rec2 + v.lbase[NCLS * leaf + 1] : v.rec2 + (uint64_t)(leaf >> v.sel_bits) * (v.cap2c + v.cap2t));
  // record i of the leaf's complete runs / of its truncated runs, wherever they lie
  auto l_find = [&](const uint32_t *pre, uint32_t i) {        // rank r with pre[r] <= i < pre[r + 1] (LISTS)
    uint32_t lo = 0, hi = 64;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (pre[mid] <= i) lo = mid; else hi = mid; }
    return lo;
  };
  auto ld_c = [&](uint64_t i) -> uint4 {
    if constexpr (LISTS) { const uint32_t r = l_find(l_cpre, (uint32_t)i); return l_base[r][(uint32_t)i - l_cpre[r]]; }
    else return leaf_rec[i];
  };
  if constexpr (!LISTS) {
    if (nt + n1 - 1ull >= HUGE_LEAF - 1ull) return;     // nothing to count -- or a HUGE leaf: msp_huge_leaves_kernel counts it
  }
  // Short windows (k < 28) mean more distinct runs per leaf than the record table holds (~600 at
  // k = 21, heavy leaves several times that): the complete runs are then deduplicated in a table
  // over the whole pool right away and listed in the stream (see p3_big_dedupe / p3_compact).
  // Both uses of the pool-wide table need duplicates to pay for the extra pass: a leaf with
  // fewer than BT_MIN_RUNS complete runs cannot hold many copies of more than ~10^3 distinct ones
  // (low coverage of a large genome: the stream path is the better fallback there).
  // (a shared leaf never rewrites its stream: the other workgroups are reading it)
  const bool big_first = !SHARED && !LISTS && k < 28 && n1 >= (uint64_t)BT_MIN_RUNS;   // (lists are read in place: nothing to rewrite)
  uint4 *const tab = big_first ? pool : rtab;
  const int tab_log = big_first ? BT_LOG : RT_LOG;
  const uint32_t tab_mask = (1u << tab_log) - 1u;
  const int tab_trips = big_first ? BT_TRIPS : RT_TRIPS;
  if (!SHARED && (mode & P3_EXPORT) && n1 == 0) return;      // nothing to deduplicate: the truncated runs leave as they are
  // DISPLACED-RUN CACHE.  At load 0.3 a sixth of the distinct runs do not sit in their home slot of the
  // record table, and every copy of such a run (~50 each at C3's depth) took the slow path: compaction
  // across the wave plus the probe loop -- there is such a record in nearly every wave-step.  While the
  // stream is scanned the k-mer table's memory is idle: it holds a direct-mapped cache of DC entries
  // (same entry format; its slot: other bits of the slot hash's product, dc_slot below) in which a displaced run is installed by the probe loop that placed or
  // found it.  A record that misses its home slot looks there next (one more LDS read) and counts in the
  // cache entry; after the scan the cache's counts are added to the table's entries and the memory
  // becomes the k-mer table.  Only first sightings and cache conflicts still take the slow path.
  constexpr int DC = TS / 2 + TS / 4;            // uint4 entries in the k-mer table's memory (3072)
  const bool use_cache = !big_first;
  uint4 *const dcache = pool;
  if (big_first) {
    for (int s = tid; s < BT; s += P3_THREADS) pool[s] = make_uint4(0u, 0u, 0u, RT_EMPTY);
  } else {
    for (int s = tid; s < DC; s += P3_THREADS) dcache[s] = make_uint4(0u, 0u, 0u, RT_EMPTY);
    for (int s = tid; s < RT; s += P3_THREADS) rtab[s] = make_uint4(0u, 0u, 0u, RT_EMPTY);
  }
  if (tid == 0) { wg_total = 0; nocc = 0; rt_fail = 0; kovf = 0; sp = 0; leaf_total = 0; nseg = 0; nfb = 0; nfl = 0; }
  if (tid < 32) { nhist[tid] = 0; thist[tid] = 0; }
  for (int s = tid; s < RT + 1; s += P3_THREADS) th[s] = 0;
  __syncthreads();

  const uint64_t kmask = (k == 32) ? ~0ull : ((1ull << (2 * k)) - 1ull);
  const int rcsh = 2 * k - 2;
  // truncated runs that go through the length-sorted list: as many as fit
  const uint4 *trunc = LISTS ? nullptr : (v.exact ? v.rec2 + v.lbase[NCLS * leaf + 0] : leaf_rec + v.cap2c);
  const uint32_t tl = (uint32_t)min(nt, (uint64_t)TL_CAP);
  auto ld_t = [&](uint64_t i) -> uint4 {
    if constexpr (LISTS) {
      const uint32_t r = l_find(l_tpre, (uint32_t)i), j = (uint32_t)i - l_tpre[r];
      const uint4 *b = l_base[r];
      const uint32_t nd_r = l_cpre[r + 1] - l_cpre[r], nu_r = l_nu[r];
      if (j < nu_r) return b[nd_r + j];
      // a note: the first n k-mers of its twin, closed on the left only (msp_runs_scatter_kernel did this in a pass of its own)
      const uint32_t note = reinterpret_cast<const uint16_t *>(b + nd_r + nu_r)[j - nu_r];
      const uint4 twin = b[min(note >> 5, nd_r - 1u)];                    // a position outside the list is not followed
      const uint32_t nm1 = min(note & 31u, twin.w & 31u);
      const int rb = 2 * ((int)nm1 + k) - 32;                           // bits of the run beyond the first word: 0 .. 64
      const uint32_t my = (rb >= 32) ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> rb);
      const uint32_t mz = (rb <= 32) ? 0u : ((rb >= 64) ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> (rb - 32)));
      return make_uint4(twin.x, twin.y & my, twin.z & mz, 64u | nm1);
    } else return trunc[i];
  };
  if constexpr (LISTS) {
    if (nt + n1 == 0) return;
    if (nt + n1 >= HUGE_LEAF) {                        // (see HUGE_LEAF: counted in the HBM table, whose adds saturate)
      for (uint64_t i = tid; i < n1 + nt; i += P3_THREADS) {
        const uint4 rec = (i < n1) ? ld_c(i) : ld_t(i - n1);
        spill_record(rec, k, CANON, t, (i < n1) ? (rec.w >> 6) : 1u);
      }
      return;
    }
  }

  // ---- phase 1a: complete runs, one record-table update per record.  Most records find their
  //      twin in the home slot: that case is one LDS read + one LDS add with every lane busy.
  //      The rest (first sightings, displaced entries) are compacted into a wave-private
  //      leftover set, 64 lanes wide, and only a full set runs the probe loop -- the loop's trip
  //      count is the longest chain among its lanes, so it must not run for a handful of them.
  {
    const uint4 *src = leaf_rec;
    const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
    const uint64_t n1a = n1;
    uint32_t *rmeta = reinterpret_cast<uint32_t *>(tab);
    uint4 L = zero4;                 // leftover records, lanes [0, c)
    uint32_t Lh = 0;
    int c = 0;                       // wave-uniform
    const bool weighted = !SHARED && (mode & P3_WEIGHTED) != 0u;   // (an owner's leaves are never shared)
    // the cache slot comes from the product the home slot is the top bits of (p = rtab_prod_k): the RT_LOG + 2 bits
    // below them, scaled to the DC = 3/4 * 4096 entries -- three full-rate instructions, where a hash of its own over
    // the whole record was nine with two multiplies.  Runs with one first k-mer share a cache slot (the compare is
    // exact; the second comer takes the slow path as any conflict does).
    static_assert(DC == 3 << RT_LOG, "dc_slot scales RT_LOG + 2 bits by 3/4");
    auto dc_slot = [&](uint32_t p) { return (((p >> (30 - 2 * RT_LOG)) & (4u * RT - 1u)) * 3u) >> 2; };
    // FAST: the scan of the headline case (below) -- table, mask, trips and increment are constants there
    auto drain = [&](auto fast_, int cnt) {
      constexpr bool FAST = decltype(fast_)::value;
      P3_MARK("P3_PART_DRAIN");
      uint32_t h = Lh | ((lane < cnt) ? 0u : RT_DONE);
      if (FAST) rtab_insert_loop(rtab, L, h);
      else rtab_insert_loop(tab, L, h, tab_mask, tab_trips, weighted ? ((L.w >> 6) << 6) : (1u << 6));
      // no room in the record table: a leaf with more distinct runs than it holds (low coverage
      // of a large genome).  Dedupe is pointless there: the whole leaf is counted from its streams.
      if ((int32_t)h >= 0) rt_fail = 1u;
      // a record that ended up away from its home slot goes into the cache (count 0: what the table's entry
      // holds stays there), so that its next copies find it with one look instead of coming through here
      if ((FAST || use_cache) && lane < cnt && (int32_t)h < 0 && ((h ^ Lh) & (FAST ? (uint32_t)(RT - 1) : tab_mask)) != 0u) {
        uint32_t *dmeta = reinterpret_cast<uint32_t *>(dcache);
        const uint32_t cs = dc_slot(rtab_prod_k(L, k));
        if (atomicCAS(&dmeta[4 * cs + 3], RT_EMPTY, RT_LOCK) == RT_EMPTY) {
          dmeta[4 * cs + 0] = L.x; dmeta[4 * cs + 1] = L.y; dmeta[4 * cs + 2] = L.z;
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
          atomicExch(&dmeta[4 * cs + 3], L.w & 63u);
        }
      }
    };
    // the lanes of `mask` (= __ballot(left)) hand their record and home slot to the wave's leftover set
    auto leftover = [&](auto fast_, const uint4 rec, uint32_t h, bool left, unsigned long long mask) {
      P3_MARK("P3_PART_APPEND");
      const int n = __popcll(mask);
      if (c + n > 64) { drain(fast_, c); c = 0; }
      uint32_t set[5] = {L.x, L.y, L.z, L.w, Lh};
      const uint32_t mine_[5] = {rec.x, rec.y, rec.z, rec.w, h};
      wave_append<5>(set, mine_, left, mask, c, n);
      L = make_uint4(set[0], set[1], set[2], set[3]); Lh = set[4];
      c = __builtin_amdgcn_readfirstlane(c + n);             // (uniform: the compiler keeps it in a scalar register)
    };
    auto home = [&](const uint4 rec, bool valid) {
      P3_MARK("P3_PART_HOME");
      const uint32_t p = rtab_prod_k(rec, k);
      const uint32_t h = big_first ? rtab_slot(rec, tab_log) : (p >> (32 - RT_LOG));
      const uint4 e = tab[h];
      const bool match = valid && rtab_diff(e, rec) == 0u;
      if (match) atomicAdd(&rmeta[4 * h + 3], weighted ? ((rec.w >> 6) << 6) : (1u << 6));
      bool left = valid && !match;
      if (use_cache && __ballot(left)) {
        P3_MARK("P3_PART_CACHE");
        uint32_t *dmeta = reinterpret_cast<uint32_t *>(dcache);
        const uint32_t cs = dc_slot(p);
        const uint4 ce = dcache[cs];
        const bool chit = left && rtab_diff(ce, rec) == 0u;
        if (chit) atomicAdd(&dmeta[4 * cs + 3], weighted ? ((rec.w >> 6) << 6) : (1u << 6));
        left = left && !chit;
      }
      const unsigned long long mask = __ballot(left);
      if (mask == 0ull) return;
      leftover(std::false_type{}, rec, h, left, mask);
    };
    // THE CASE THE HEADLINE WORKLOAD RUNS -- reads counted on one GPU at k >= 28, or a leaf too small for the pool-wide
    // table: multiplicity 1, the 1024-slot table, cache on -- has a scan of its own.  Table, mask and increment are
    // constants; the cache entry is read NEXT TO the table's entry (at load 0.3 some lane of the wave needs it in nearly
    // every step: the look is no longer a second round trip behind a ballot), and the one lane-wise add goes to
    // whichever of the two matched.  FULL: every lane holds a record (the main loop; the tail is peeled).
    [[maybe_unused]] auto home_fast = [&](auto full_, const uint4 rec, bool valid) {
      constexpr bool FULL = decltype(full_)::value;
      constexpr uint32_t RT_W0 = 4u * (uint32_t)DC;            // the record table's first word in the pool
      uint32_t *const pmeta = reinterpret_cast<uint32_t *>(pool);
      P3_MARK("P3_PART_HOME");
      const uint32_t p = rtab_prod_k(rec, k);
      const uint32_t h = p >> (32 - RT_LOG), cs = dc_slot(p);
      const uint4 e = rtab[h];
      const uint4 ce = dcache[cs];
      const uint32_t d0 = rtab_diff(e, rec);
      P3_MARK("P3_PART_CACHE");
      const uint32_t d1 = rtab_diff(ce, rec);
      // no branch around the add: a lane without a hit adds 0 (as rtab_insert_loop does) -- exec-mask bookkeeping is
      // scalar issue slots in every step, the add of 0 costs nothing the other lanes' add does not pay already
      const bool match = d0 == 0u, hit = min(d0, d1) == 0u;   // (never both: a run is cached because it is NOT in its home slot)
      const bool take = FULL ? hit : (valid && hit);
      atomicAdd(&pmeta[match ? (RT_W0 + 4u * h + 3u) : (4u * cs + 3u)], take ? (1u << 6) : 0u);
      const bool left = FULL ? !hit : (valid && !hit);
      const unsigned long long mask = __ballot(left);
      if (mask == 0ull) return;
      leftover(std::true_type{}, rec, h, left, mask);
    };
    bool fast = false;
    if constexpr (!SHARED && !LISTS) fast = !weighted && !big_first && !(v.dbg & CFRK_ABL_P3_NO_RTAB);
    if (fast) {
      if constexpr (!SHARED && !LISTS) {
        const uint32_t n32 = (uint32_t)n1a;                    // (< HUGE_LEAF)
        uint32_t wb = __builtin_amdgcn_readfirstlane((uint32_t)(tid - lane));   // the wave's first record: a scalar
        P3_MARK("P3_PART_LOAD");
        // (measured and not kept, round 27: the loop one trip ahead of its loads -- 0.05 ms of P3's 6.3 in each of three
        //  rounds, under the bar of three standard deviations -- and the first trip's records asked for at the kernel's
        //  entry, in front of the clear of the tables: 0.06 ms on its own, nothing beside the truncated records' early
        //  loads below.  Sixteen waves per workgroup and two workgroups per CU already hide a record's way from HBM.)
        for (; wb + (uint32_t)P3_THREADS + 64u <= n32; wb += 2u * P3_THREADS) {
          const uint4 rec0 = src[wb + lane], rec1 = src[wb + P3_THREADS + lane];
          home_fast(std::true_type{}, rec0, true);
          home_fast(std::true_type{}, rec1, true);
          P3_MARK("P3_PART_LOAD");
        }
        // the tail: at most two wave-steps, the only ones with lanes past the end
#pragma unroll 1
        for (int u = 0; u < 2 && wb < n32; ++u, wb += P3_THREADS) {
          const bool vv = wb + lane < n32;
          uint4 rec = zero4;
          if (vv) rec = src[wb + lane];
          home_fast(std::false_type{}, rec, vv);
          P3_MARK("P3_PART_LOAD");
        }
        if (c) drain(std::true_type{}, c);
        c = 0;
      }
    } else if (!SHARED) {
      P3_MARK("P3_PART_LOAD");
      for (uint64_t r = tid; r < ((n1a + 63) & ~63ull) && !(v.dbg & CFRK_ABL_P3_NO_RTAB); r += 2ull * P3_THREADS) {
        const uint64_t r1 = r + P3_THREADS;
        const bool v0 = r < n1a, v1 = r1 < n1a;
        uint4 rec0 = zero4, rec1 = zero4;
        if (v0) rec0 = LISTS ? ld_c(r) : src[r];
        if (v1) rec1 = LISTS ? ld_c(r1) : src[r1];
        home(rec0, v0);
        home(rec1, v1);
        P3_MARK("P3_PART_LOAD");
      }
    } else {
      // a shared leaf: most records read here are another workgroup's.  The one lane in 2^sub_bits that
      // holds a record of this workgroup is gathered into full sets of 64 before the table look-up:
      // home() costs the wave ~100 instructions however few lanes take part (msp2.hip)
      uint4 Cr = zero4;
      int cc = 0;                        // wave-uniform
      auto cfeed = [&](const uint4 rec, bool keep) {
        const unsigned long long mask = __ballot(keep);
        if (mask == 0ull) return;
        const int n = __popcll(mask);
        if (cc + n > 64) { home(Cr, lane < cc); cc = 0; }
        uint32_t set[4] = {Cr.x, Cr.y, Cr.z, Cr.w};
        const uint32_t mine_[4] = {rec.x, rec.y, rec.z, rec.w};
        wave_append<4>(set, mine_, keep, mask, cc, n);
        Cr = make_uint4(set[0], set[1], set[2], set[3]);
        cc += n;
      };
      P3_MARK("P3_PART_LOAD");
      for (uint64_t r = tid; r < ((n1a + 63) & ~63ull); r += 2ull * P3_THREADS) {
        const uint64_t r1 = r + P3_THREADS;
        const bool v0 = r < n1a, v1 = r1 < n1a;
        uint4 rec0 = zero4, rec1 = zero4;
        if (v0) rec0 = src[r];
        if (v1) rec1 = src[r1];
        cfeed(rec0, v0 && mine(rec0.w));
        if (r1 < ((n1a + 63) & ~63ull)) cfeed(rec1, v1 && mine(rec1.w));       // (wave-uniform)
        P3_MARK("P3_PART_LOAD");
      }
      if (cc) home(Cr, lane < cc);
    }
    if (c) drain(std::false_type{}, c);
    if ((v.dbg & CFRK_DEBUG_FORCE_RT_OVERFLOW) && !big_first) rt_fail = 1u;
  }
  // The first TL_CAP truncated records, TL_PER per thread, are asked for HERE: their addresses were known at entry, and
  // the cache merge, the clear of the k-mer table and their three barriers need nothing of them -- the HBM round trip
  // (~1.5 us per leaf, two leaves per CU) runs under that work instead of behind it.  All of a thread's records in
  // one go and WITHOUT A BRANCH around them (behind one the compiler copies the records into other registers at once,
  // and waits for them to do so): lanes past the end load the last record again; a leaf without truncated runs, an
  // exporting leaf, which never looks at them, and a leaf of the pool-wide table load one record that is surely there.
  // The one-GPU counting kernels only: the shared and the lists forms keep their registers as they were.
  constexpr bool TREC_EARLY = !SHARED && !LISTS;
  uint4 trec[TL_PER];
  auto load_trec = [&](bool early) {
    if constexpr (TREC_EARLY) {
      const uint4 *tb = tl ? trunc : v.rec2;
      // (big_first: the pool-wide table's path asks again behind its own code -- one record here, not four per thread)
      const uint32_t lim = (tl && !(mode & P3_EXPORT) && !(early && big_first)) ? tl - 1u : 0u;
#pragma unroll
      for (int i = 0; i < TL_PER; ++i) trec[i] = tb[min((uint32_t)(i * P3_THREADS + tid), lim)];
    } else {
#pragma unroll
      for (int i = 0; i < TL_PER; ++i) trec[i] = make_uint4(0u, 0u, 0u, 0u);
      if (tl) {                                      // (uniform)
#pragma unroll
        for (int i = 0; i < TL_PER; ++i) trec[i] = ld_t(min((uint32_t)(i * P3_THREADS + tid), tl - 1u));
      }
    }
  };
  if constexpr (TREC_EARLY) load_trec(true);
  P3_MARK("P3_PART_MERGE");
  __syncthreads();
  if (use_cache) {
    // the cache's counts go to the table's entries (the run is there: it was placed before it was cached;
    // a table that overflowed is not used at all), then the memory becomes the k-mer table
    uint32_t *rmeta = reinterpret_cast<uint32_t *>(rtab);
    for (int s = tid; s < DC && rt_fail == 0u; s += P3_THREADS) {
      const uint4 ce = dcache[s];
      if (ce.w == RT_EMPTY || (ce.w >> 6) == 0u) continue;
      uint32_t hh = rtab_slot_k(ce, k, RT_LOG);
      for (int it = 0; it < RT; ++it) {
        const uint4 e = rtab[hh];
        if (rtab_diff(e, ce) == 0u) { atomicAdd(&rmeta[4 * hh + 3], (ce.w >> 6) << 6); break; }
        if (e.w == RT_EMPTY) break;                // (cannot happen)
        hh = (hh + 1u) & (uint32_t)(RT - 1);
      }
    }
    __syncthreads();
    if (SHARED || !(mode & P3_EXPORT))             // (an exporting leaf never touches its k-mer table)
      for (int s = tid; s < TS; s += P3_THREADS) { keys[s] = CFRK_EMPTY_KEY; cnts[s] = 0; }
    __syncthreads();
  }
  P3_MARK("P3_PART_END");
  // ---- phase 2: k-mer by k-mer -- every distinct complete record of the record table (weight =
  //      its multiplicity) and the truncated runs (weight 1).  Both are first listed SORTED BY
  //      LENGTH (counting sort of 16-bit indices in LDS): a wave expands 64 records in lock-step
  //      for as many steps as its longest one, so equal lengths keep every lane busy.
  uint32_t nd = 0xFFFFFFFFu;                     // distinct runs listed in the stream (second chance), ~0: none
  if (!SHARED && (mode & P3_EXPORT)) {
    uint4 *const stream = const_cast<uint4 *>(leaf_rec);
    const bool weighted = (mode & P3_WEIGHTED) != 0u;
    if (big_first) { if (rt_fail == 0u) nd = p3_compact(pool, stream, wsum); }
    else if (rt_fail == 0u) nd = p3_dump_rtab(rtab, stream, wsum);
    else if (n1 >= (uint64_t)BT_MIN_RUNS || (v.dbg & CFRK_DEBUG_FORCE_RT_OVERFLOW)) nd = p3_big_dedupe(pool, stream, n1, wsum, &rt_fail, weighted);
    if (nd == 0xFFFFFFFFu) {
      // nothing to merge (more distinct runs than any table here holds): the runs leave as they are, multiplicity 1
      if (!weighted)
        for (uint64_t i = tid; i < n1; i += P3_THREADS) stream[i].w = (1u << 6) | (stream[i].w & 63u);
      nd = (uint32_t)n1;
    }
    if (tid == 0) v.leaf_n[leaf] = nd;
    return;
  }
  if (big_first || rt_fail != 0u) {              // (rt_fail read after the barrier above: uniform)
    if (!SHARED && !LISTS && !big_first && (n1 >= (uint64_t)BT_MIN_RUNS || (v.dbg & CFRK_DEBUG_FORCE_RT_OVERFLOW))) nd = p3_big_dedupe(pool, const_cast<uint4 *>(leaf_rec), n1, wsum, &rt_fail, (mode & P3_WEIGHTED) != 0u);
    else if (!big_first) __syncthreads();        // (as below)
    else if (rt_fail == 0u) nd = p3_compact(pool, const_cast<uint4 *>(leaf_rec), wsum);
    else __syncthreads();                        // (the pool is cleared below: everybody has read rt_fail and the table)
    for (int s = tid; s < TS; s += P3_THREADS) { keys[s] = CFRK_EMPTY_KEY; cnts[s] = 0; }
    for (int s = tid; s < RT; s += P3_THREADS) rtab[s] = make_uint4(0u, 0u, 0u, RT_EMPTY);
    __syncthreads();
    // (the rare path: the truncated records are asked for again, so that sixteen registers are not kept alive -- or
    //  spilled -- across the pool-wide table's code)
    if constexpr (TREC_EARLY) load_trec(false);
  }
  const bool listed = nd != 0xFFFFFFFFu;
  const bool big = !listed && rt_fail != 0u;
  // Truncated runs (read ends) are most of the leaf's k-mer insertions, one by one with weight 1.
  // But a run that is cut on ONE side is a prefix -- or, read on the other strand, a suffix -- of
  // the complete run of its locus, which sits in the record table: it is looked up there by its
  // first k-mer, and only its LENGTH is noted with its twin.  The twin's expansion then counts its
  // first t k-mers once more: one table lookup per truncated run instead of one per k-mer.
  // Runs without a twin (cut on both sides, shallow loci, forward-strand suffixes) stay k-mer by k-mer.
  const bool anchors_on = !big && !listed && !(v.dbg & CFRK_DEBUG_NO_ANCHORS);
  bool use_anchors = false;
  {
    // (a) record table: occupied slots, longest first (not when the leaf is counted from its streams)
    P3_MARK("P3_PART_LIST");
    const uint4 e = rtab[tid];                       // RT == P3_THREADS
    const bool occ = !big && e.w != RT_EMPTY;
    // STRAND TWINS.  The table is keyed by a run's bases as read, and reads come from both strands: a locus sits in it
    // twice, as a run and as its reverse complement, and both expansions roll, canonicalise, hash and count the SAME
    // canonical k-mers (the second one's every key a match: on C3 every entry has its twin, and 44 % of the expansion's
    // keys are matches).  MEASURED AND NOT KEPT (round 32, profiles/r32): every entry looked its reverse complement up
    // here, of a pair the one with the smaller bases was expanded with both multiplicities and both lists of noted
    // lengths (the twin's mirrored), the other left out of the list.  On top of three lanes per run that made the
    // kernel SLOWER in every round: +0.25 / +0.20 ms of P3's 5.7 with the twin's notes in a walk of their own,
    // +0.08 / +0.13 ms with both walks in one loop, within +-0.07 ms of it without the pass's barrier; four and six
    // lanes per merged run were slower still (+0.36 ... +0.43 / +0.28 ... +0.35 ms).  The expansion is not issue-bound:
    // a wave takes its three steps and its walk whether eight or sixteen waves of the workgroup do so beside it, and
    // the look-up pass and the second list are added to every leaf's critical path.
#ifdef CFRK_ABLATIONS
    if constexpr (CANON && !SHARED && !LISTS) {
      if (anchors_on && (v.dbg & CFRK_ABL_P3_PATHS)) {     // (uniform) the look-up alone, to count the twins
        const uint4 r = revcomp_record(e, (int)(e.w & 31u) + k);
        const bool palin = rtab_diff(r, e) == 0u;          // its own reverse complement
        uint32_t h = (occ && !palin) ? rtab_slot_k(r, k, RT_LOG) : RT_DONE;
        bool found = false;
        // (an entry of the table is always found from its home slot: the twins see each other or neither does)
        for (int it = 0; it < RT && __ballot((int32_t)h >= 0); ++it) {
          const bool p = (int32_t)h >= 0;
          const uint32_t hh = h & (uint32_t)(RT - 1);
          const uint4 e2 = rtab[hh];
          const bool hit = p && rtab_diff(e2, r) == 0u;
          found = found || hit;
          h = (p && !hit && e2.w != RT_EMPTY) ? ((hh + 1u) & (uint32_t)(RT - 1)) : (h | RT_DONE);
        }
        const unsigned long long mo = __ballot(occ), mt = __ballot(found), mp = __ballot(occ && palin);
        if (lane == 0) {
          if (mo) P3_COUNT(P3C_RT_ENTRIES, __popcll(mo));
          if (mt) P3_COUNT(P3C_RT_TWINNED, __popcll(mt));
          if (mp) P3_COUNT(P3C_RT_PALIN, __popcll(mp));
        }
      }
    }
#endif
    uint32_t rank = 0;
    if (occ) rank = atomicAdd(&nhist[e.w & 31u], 1u);
    // (b) truncated runs: the first TL_CAP of the stream, by position
    constexpr uint32_t TW_NONE = 0xFFFFFFFFu, TW_TWIN = 0x80000000u;
    uint32_t tw[TL_PER], trank[TL_PER];              // n-1, or TW_TWIN | twin slot << 8 | n
    // (all of a thread's records are asked for before the first is looked up: one HBM round trip instead of
    //  TL_PER -- the compiler put a full wait behind every load, 4 x ~1.5 us per leaf with two leaves per CU;
    //  the one-GPU counting kernels have asked in front of the cache merge, see there)
    if constexpr (!TREC_EARLY) load_trec(false);
    P3_MARK("P3_PART_ANCHOR");
#pragma unroll
    for (int i = 0; i < TL_PER; ++i) {
      const uint32_t g = (uint32_t)(i * P3_THREADS + tid);
      bool valid = g < tl;
      tw[i] = TW_NONE; trank[i] = 0u;
      uint4 rec = trec[i];
      if (SHARED) valid = valid && mine(rec.w);
      const uint32_t nm1 = rec.w & 31u;
      if (valid) tw[i] = nm1;
      if (anchors_on && __ballot(valid)) {
        const bool lc = (rec.w & 64u) != 0u, rc_ = (rec.w & 128u) != 0u;
        const bool suf = CANON && valid && !lc && rc_;
        if (suf) rec = revcomp_record(rec, (int)nm1 + k);
        const bool anchored = suf || (valid && lc && !rc_);
        uint32_t h = anchored ? rtab_slot_k(rec, k, RT_LOG) : RT_DONE;
        uint32_t found = TW_NONE;
        for (int it = 0; it < 32 && __ballot((int32_t)h >= 0); ++it) {
          const bool p = (int32_t)h >= 0;
          const uint32_t hh = h & (uint32_t)(RT - 1);
          const uint4 e2 = rtab[hh];
          const bool empty = e2.w == RT_EMPTY;
          // the twin holds at least as many k-mers and starts with the same nm1 + k bases
          const bool hit = p && !empty && (e2.w & 31u) >= nm1 && rec_prefix_equal(e2, rec, (int)nm1 + k);
          found = hit ? hh : found;
          h = (p && !hit && !empty) ? ((hh + 1u) & (uint32_t)(RT - 1)) : (h | RT_DONE);
        }
        if (found != TW_NONE) tw[i] = TW_TWIN | (found << 8) | (nm1 + 1u);
        const unsigned long long fb = __ballot(valid && found == TW_NONE);
        if (lane == 0 && fb) atomicAdd(&nfb, (uint32_t)__popcll(fb));
      }
    }
    P3_MARK("P3_PART_GROUP");
    __syncthreads();
    use_anchors = anchors_on && nfb <= (uint32_t)FL_CAP;
    if (use_anchors) {
#pragma unroll
      for (int i = 0; i < TL_PER; ++i) {
        if (tw[i] == TW_NONE) continue;
        if (tw[i] & TW_TWIN) trank[i] = atomicAdd(&th[(tw[i] >> 8) & (uint32_t)(RT - 1)], 1u);
        else flist[atomicAdd(&nfl, 1u)] = (uint16_t)(i * P3_THREADS + tid);
      }
    } else {
#pragma unroll
      for (int i = 0; i < TL_PER; ++i) {
        if (tw[i] == TW_NONE) continue;
        const uint32_t g = (uint32_t)(i * P3_THREADS + tid);
        tw[i] = ld_t(g).w & 31u;                     // (a twin that was found is not used)
        trank[i] = atomicAdd(&thist[tw[i]], 1u);
      }
    }
    __syncthreads();
    if (tid < 64) {
      // exclusive prefix over DEscending length, both histograms (lanes 0..31 / 32..63)
      const uint32_t own = (tid < 32) ? nhist[31 - tid] : thist[63 - tid];
      uint32_t incl = own;
#pragma unroll
      for (int d = 1; d < 32; d <<= 1) {
        const uint32_t y = __shfl_up(incl, d, 32);
        if ((tid & 31) >= d) incl += y;
      }
      if (tid < 32) nhist[31 - tid] = incl - own; else thist[63 - tid] = incl - own;
      if (tid == 31) nocc = incl;
      if (tid == 63 && !use_anchors) nfl = incl;       // entries of the length-sorted list (a shared leaf: this workgroup's only)
    }
    uint32_t goff = 0;
    if (use_anchors) {
      // group starts: exclusive prefix of the groups' sizes over the record table's slots
      const uint32_t own = th[tid];
      uint32_t incl = own;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(incl, d);
        if (lane >= d) incl += y;
      }
      if (lane == 63) wsum[tid >> 6] = incl;
      __syncthreads();
      uint32_t base = 0;
      for (int w = 0; w < (tid >> 6); ++w) base += wsum[w];
      goff = base + incl - own;
      __syncthreads();                               // (everybody has read its group's size)
      th[tid] = goff;
      if (tid == P3_THREADS - 1) th[RT] = goff + own;
    }
    __syncthreads();
    if (occ) occ_list[nhist[e.w & 31u] + rank] = (uint16_t)tid;
    if (use_anchors) {
#pragma unroll
      for (int i = 0; i < TL_PER; ++i)
        if (tw[i] != TW_NONE && (tw[i] & TW_TWIN)) tbytes[th[(tw[i] >> 8) & (uint32_t)(RT - 1)] + trank[i]] = (uint8_t)(tw[i] & 63u);
    } else {
#pragma unroll
      for (int i = 0; i < TL_PER; ++i)
        if (tw[i] != TW_NONE) tlist[thist[tw[i]] + trank[i]] = (uint16_t)(i * P3_THREADS + tid);
    }
    // Key subsets to count: the whole leaf in one pass -- or, when the record table overflowed (it
    // then held ~10^3 distinct runs, i.e. twice as many distinct k-mers as the k-mer table takes),
    // four quarters to begin with.
    if (tid == 0) {
      if (big) {
        // as many key subsets to begin with as the leaf's size suggests (one per ~6000 records, 4 .. 32)
        uint32_t b0 = 2u;
        while (b0 < 5u && ((nt + n1) >> b0) > 6000ull) ++b0;
        for (uint32_t q = 0; q < (1u << b0); ++q) stk[q] = (b0 << 16) | q;
        sp = (int)(1u << b0);
      } else { stk[0] = 0u; sp = 1; }
    }
  }
  __syncthreads();
  constexpr uint32_t SUBSET_BITS_MAX = 8;        // 256 passes at most; beyond: the HBM table
  bool first_pass = true;
  while (true) {
    const int depth = sp;                        // (every thread reads the same value: barriers around)
    if (depth == 0) break;
    const uint32_t item = stk[depth - 1];
    __syncthreads();
    if (tid == 0) { sp = depth - 1; kovf = 0; wg_total = 0; }
    const uint32_t bits = item >> 16;
    const KeySubset ss{(1u << bits) - 1u, item & 0xFFFFu};
    uint32_t *ovf = (bits < SUBSET_BITS_MAX) ? &kovf : nullptr;
    if (!first_pass)
      for (int s = tid; s < TS; s += P3_THREADS) { keys[s] = CFRK_EMPTY_KEY; cnts[s] = 0; }
    first_pass = false;
    __syncthreads();
    {
      if (listed) {
        // distinct complete runs with their multiplicities, from the head of the stream
        for (uint32_t i = tid; i < ((nd + 63u) & ~63u); i += P3_THREADS) {
          const bool valid = i < nd;
          uint4 rec = make_uint4(0u, 0u, 0u, 0u);
          if (valid) rec = leaf_rec[i];
          count_record_v2<CANON>(keys, cnts, rec, rec.w >> 6, valid, k, kmask, rcsh, t, ss, ovf);
        }
      } else if (!big) {
        // ~320 distinct runs for 1024 lanes, and a wave works for as many steps as its longest run
        // has k-mers: up to three lanes share a record, each expanding a share of its k-mers
        const uint32_t nlist = (v.dbg & CFRK_ABL_P3_NO_CEXP) ? 0u : nocc;
        // lanes per run before every canonical leaf took three (the forward-strand instantiation's still: it is out of
        // registers and walks its notes per k-mer pair whatever a lane's share)
        const int parts_by_n = (nlist * 3u <= (uint32_t)P3_THREADS) ? 3 : (nlist * 2u <= (uint32_t)P3_THREADS) ? 2 : 1;
#ifdef CFRK_ABLATIONS
        if (tid == 0 && nlist && (v.dbg & CFRK_ABL_P3_PATHS)) P3_COUNT(P3C_LEAVES_1 + parts_by_n - 1, 1);
#endif
        // Canonical counting: THREE lanes per run however many runs (the list is sorted by length: more than 1024 items
        // take a second trip, of the shortest runs).  With two, the longest runs' lanes hold nine k-mers: their waves
        // miss the one-walk path of the notes (tb_fast: <= 8) and take five steps instead of three.  On C3 a quarter
        // of the leaves list more than 341 runs and 7 % of the expansion's wave-calls walked their notes per k-mer
        // pair: 6.07 -> 5.78 ms per launch (round 32, profiles/r32).  (Four and six lanes for a short list, measured
        // beside the twin merge, lose against three: a setup is issued per lane, and two k-mers make a step.)
        // (The shared-leaf instantiation keeps the lanes it had, like the forward-strand one: with three always it
        //  spilled 18 scratch instructions, over the 16 that tests/test_kernel_resources.py allows; as it stands 13.)
        constexpr bool LANES3 = CANON && !SHARED;
        const int parts = (LANES3 && !(v.dbg & CFRK_ABL_P3_OLD_CEXP)) ? 3 : parts_by_n;
        const uint32_t nitems = nlist * (uint32_t)parts;
        const uint32_t prcp = (1u << 20) / (uint32_t)parts + 1u;        // (i / parts for i < 2^12 by a multiply)
        P3_MARK("P3_PART_CEXP");
        // (PATHS: count_record_v2 counts the paths it takes -- an ablation build with CFRK_ABL_P3_PATHS set)
        auto expand = [&](auto paths_) {
          constexpr bool PATHS = decltype(paths_)::value;
          for (uint32_t i = tid; i < ((nitems + 63u) & ~63u); i += P3_THREADS) {
            const bool valid = i < nitems;
            const uint32_t ri = LANES3 ? ((i * prcp) >> 20) : ((parts == 1) ? i : (parts == 2) ? (i >> 1) : (i / 3u));
            uint4 rec = make_uint4(0u, 0u, 0u, 0u);
            uint32_t slot = 0;
            if (valid) { slot = occ_list[ri]; rec = rtab[slot]; }
            if (use_anchors) {
              // ... plus one for every truncated run of this locus that reaches the k-mer
              const uint32_t g0 = th[slot];
              count_record_v2<CANON, PATHS>(keys, cnts, rec, rec.w >> 6, valid, k, kmask, rcsh, t, ss, ovf,
                                            (int)(i - ri * (uint32_t)parts), parts, tbytes + g0, valid ? th[slot + 1] - g0 : 0u);
            } else {
              count_record_v2<CANON, PATHS>(keys, cnts, rec, rec.w >> 6, valid, k, kmask, rcsh, t, ss, ovf,
                                            (int)(i - ri * (uint32_t)parts), parts);
            }
          }
        };
#ifdef CFRK_ABLATIONS
        if (v.dbg & CFRK_ABL_P3_PATHS) expand(std::true_type{}); else
#endif
        expand(std::false_type{});
      } else {
        // the complete runs straight from their stream, weight 1 each
        for (uint64_t i = tid; i < ((n1 + 63) & ~63ull); i += P3_THREADS) {
          const bool valid = i < n1;
          uint4 rec = make_uint4(0u, 0u, 0u, 0u);
          if (valid) rec = ld_c(i);
          count_record_v2<CANON>(keys, cnts, rec, (!SHARED && (mode & P3_WEIGHTED)) ? (rec.w >> 6) : 1u, valid && mine(rec.w), k, kmask, rcsh, t, ss, ovf);
        }
      }
      // truncated runs: those without a twin (anchored leaf), or all of the sorted list
      const uint32_t ntr = nfl;
      P3_MARK("P3_PART_TRUNC");
      // (measured and not kept, round 27: these two loops one trip ahead of their loads -- an anchored leaf lists at most
      //  FL_CAP = one trip of truncated runs, so nothing was hidden; and the first trip's record asked for in front of
      //  the complete runs' expansion keeps four more registers alive across it: ten spilled)
      for (uint32_t i = tid; i < ((ntr + 63u) & ~63u) && !(v.dbg & CFRK_ABL_P3_NO_TRUNC); i += P3_THREADS) {
        const bool valid = i < ntr;
        uint4 rec = make_uint4(0u, 0u, 0u, 0u);
        if (valid) rec = ld_t(use_anchors ? flist[i] : tlist[i]);
        count_record_v2<CANON>(keys, cnts, rec, 1u, valid, k, kmask, rcsh, t, ss, ovf);
      }
      // truncated runs beyond the sorted list (very large leaves): in stream order
      for (uint64_t i = (uint64_t)tl + tid; i < ((nt + 63) & ~63ull) && tl < nt; i += P3_THREADS) {
        const bool valid = i < nt;
        uint4 rec = make_uint4(0u, 0u, 0u, 0u);
        if (valid) rec = ld_t(i);
        count_record_v2<CANON>(keys, cnts, rec, 1u, valid && mine(rec.w), k, kmask, rcsh, t, ss, ovf);
      }
    }
    P3_MARK("P3_PART_OUT");
    __syncthreads();
    if (kovf) {
      // this subset does not fit the table either: its two halves replace it (the table is discarded)
      if (tid == 0) {
        const int d0 = sp;
        stk[d0] = ((bits + 1u) << 16) | ss.val;
        stk[d0 + 1] = ((bits + 1u) << 16) | ss.val | (1u << bits);
        sp = d0 + 2;
      }
      __syncthreads();
      continue;
    }

    // ---- compact occupied slots to the output list: ONE cursor atomic per workgroup and pass (a
    //      global atomic per wave on the single cursor word serialises the whole grid)
    constexpr int NIT = TS / P3_THREADS;
    uint32_t wbase[NIT];
    if (v.dbg & CFRK_ABL_P3_NO_OUT) continue;
    // A thread reads its NIT slots ONCE, keys and counts, into registers; the wave that comes by last (wg_rank_slots_last:
    // one LDS atomic per wave, no barrier) asks the cursor for the workgroup's places at once, and the counts are read
    // and the places inside the segment worked out while that atomic is on its way to HBM and back.  One barrier
    // publishes wg_base; behind it are only the stores.  (Before: ranking, barrier, thread 0's atomic with sixteen
    // waves parked, barrier, the table read again, stores, barrier.)
    unsigned long long kk[NIT], occ_m[NIT];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      kk[i] = keys[i * P3_THREADS + tid];
      occ_m[i] = __ballot(kk[i] != CFRK_EMPTY_KEY);
    }
    const uint32_t total = wg_rank_slots_last<NIT, P3_THREADS>(wbase, &wg_total, occ_m);
    const bool asks = lane == 0 && total != 0xFFFFFFFFu;         // (every wave has come by: `total` is the workgroup's)
    unsigned long long got = 0ull;
    if (asks) {
      // (the address goes through a vector register the compiler cannot see through: for an address it knows to be
      //  uniform it rewrites the add into "one lane adds for all, readfirstlane, mad", which waits for the atomic on
      //  the spot -- the one thing this order is there to avoid)
      uint32_t opaque0 = 0u;
      asm volatile("" : "+v"(opaque0));
      got = atomicAdd((unsigned long long *)&v.stats[ST_CURSOR] + opaque0, (unsigned long long)total);
    }
    uint32_t cc[NIT];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      cc[i] = cnts[i * P3_THREADS + tid];
      wbase[i] += (uint32_t)__popcll(occ_m[i] & ((1ull << lane) - 1ull));
    }
    if (asks) {
      wg_base = got;
      // a leaf counted in several passes has several segments in the list: no per-leaf index then
      // (a shared leaf: one index entry per sub-value, (leaf << sub_bits) | sub-value)
      uint32_t sg = leaf;
      if (SHARED) sg = (leaf << sub_bits) | rsel;
      if (!LISTS) {                                  // (an owner's result is not kept in leaf form)
        if (nseg == 0) v.leaf_off[sg] = got;
        else if (total) v.stats[ST_MULTISEG] = 1;
      }
      if (total) nseg = nseg + 1;
      leaf_total += total;
      if (!LISTS) v.leaf_n[sg] = leaf_total;
    }
    __syncthreads();
    const unsigned long long list_base = wg_base;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      if (kk[i] == CFRK_EMPTY_KEY) continue;
      const unsigned long long dst = list_base + wbase[i];
      if (dst < v.out_cap) { v.out_keys[dst] = kk[i]; v.out_cnt[dst] = cc[i]; }
      else v.stats[ST_OVERFLOW] = 1;
    }
    // (no barrier here: the table has been read in front of the one above, and two barriers lie between this pass's
    //  reads of wg_base / sp and the next pass's writes)
  }
}

template <bool CANON, bool SHARED>
__global__ __launch_bounds__(P3_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) void msp_p3_kernel(int k, uint32_t mode, MspView v, TableView t) {
  p3_body<CANON, SHARED, false>(k, mode, v, t, P3ListsT<false>{});
}
// the owner of the pipelined runs exchange: workgroup b counts local leaf lx.ll0 + b from the lists its ranks sent
template <bool CANON>
__global__ __launch_bounds__(P3_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) void msp_p3_lists_kernel(int k, MspView v, TableView t, P3ListsT<true> lx) {
  p3_body<CANON, false, true>(k, P3_WEIGHTED, v, t, lx);
}

// ---------------------------------------------------------------------------- multi-GPU by leaf
// Leaves are disjoint in key space on EVERY rank (same k -> same minimizer -> same leaf), so the
// owner of a key can be the owner of its leaf: owner(leaf) = leaf % parts.  Each rank ships its
// leaves' (key,count) lists to their owners, and the owner adds the lists of one leaf in an LDS
// table exactly like P3 does -- no HBM atomics in the merge.

// copy every leaf's entries into owner-major order (dst_off from the host's prefix sum)
// (out_hi: high key words of a two-word result, msp2.hip; NULL otherwise)
__global__ __launch_bounds__(256) void msp_gather_kernel(MspView v, const uint64_t *__restrict__ dst_off,
                                                         uint64_t *__restrict__ out_keys,
                                                         uint64_t *__restrict__ out_hi,
                                                         uint32_t *__restrict__ out_cnt) {
  const uint32_t leaf = blockIdx.x;
  uint64_t dof = dst_off[leaf];
  for (uint32_t j = 0; j < (1u << v.seg_bits); ++j) {          // (one segment unless the leaf was shared by record)
    const uint32_t sg = (leaf << v.seg_bits) | j;
    const uint32_t n = v.leaf_n[sg];
    const uint64_t so = v.leaf_off[sg];
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      out_keys[dof + i] = v.out_keys[so + i];
      if (out_hi) out_hi[dof + i] = v.out_hi[so + i];
      out_cnt[dof + i] = v.out_cnt[so + i];
    }
    dof += n;
  }
}

// one workgroup per owned leaf: add the `parts` incoming lists of that leaf in LDS
__global__ __launch_bounds__(P3_THREADS) void msp_merge_kernel(const uint64_t *__restrict__ in_keys,
                                                               const uint32_t *__restrict__ in_cnt,
                                                               const uint64_t *__restrict__ seg_off,
                                                               const uint32_t *__restrict__ seg_n,
                                                               int parts, int leaves_per_part,
                                                               MspView v, TableView t) {
  __shared__ unsigned long long keys[TS];
  __shared__ uint32_t cnts[TS];
  __shared__ uint32_t wg_total;
  __shared__ unsigned long long wg_base;
  const int tid = threadIdx.x;
  const uint32_t ll = blockIdx.x;                       // local leaf index on this owner
  uint32_t total = 0;
  for (int p = 0; p < parts; ++p) total += seg_n[(size_t)p * leaves_per_part + ll];
  if (total == 0) return;
  for (int s = tid; s < TS; s += P3_THREADS) { keys[s] = CFRK_EMPTY_KEY; cnts[s] = 0; }
  if (tid == 0) wg_total = 0;
  __syncthreads();
  for (int p = 0; p < parts; ++p) {
    const uint32_t n = seg_n[(size_t)p * leaves_per_part + ll];
    const uint64_t off = seg_off[(size_t)p * leaves_per_part + ll];
    for (uint32_t i = tid; i < ((n + 63u) & ~63u); i += P3_THREADS) {
      const bool valid = i < n;
      const uint64_t key = valid ? in_keys[off + i] : 0ull;
      const uint32_t c = valid ? in_cnt[off + i] : 0u;
      kt_count(keys, cnts, key, c, valid && c != 0u, t);
    }
  }
  __syncthreads();
  constexpr int NIT = TS / P3_THREADS;
  uint32_t wbase[NIT];
  auto occupied = [&](int s) { return keys[s] != CFRK_EMPTY_KEY; };
  wg_rank_slots<NIT, P3_THREADS>(wbase, &wg_total, occupied);
  __syncthreads();
  if (tid == 0) wg_base = atomicAdd((unsigned long long *)&v.stats[ST_CURSOR], (unsigned long long)wg_total);
  __syncthreads();
  wg_emit_slots<NIT, P3_THREADS>(wbase, wg_base, occupied, [&](int s, unsigned long long dst) {
    if (dst < v.out_cap) { v.out_keys[dst] = keys[s]; v.out_cnt[dst] = cnts[s]; }
    else v.stats[ST_OVERFLOW] = 1;
  });
}

// ---------------------------------------------------------------------------- multi-GPU by runs
// Strong scaling: with the reads split over N ranks every rank still meets almost every locus, so
// counting on every rank and exchanging (key, count) lists (above) makes each rank expand every
// distinct run and ship ~D entries -- neither shrinks with N.  Here a rank only partitions and
// deduplicates (P1, P2, the leaf kernel in P3_EXPORT mode) and ships, per leaf, its distinct
// complete runs with multiplicities plus its truncated runs to the leaf's owner
// (owner(leaf) = leaf % parts); the owner lines the N lists of each of its leaves up as that
// leaf's streams and runs the ordinary leaf kernel on them (P3_WEIGHTED): expansion and counting
// happen once, for 1/N of the leaves.

// The record format as the stages of the exchange see it (msp_runs.h): 16-byte records, one row of the packed buffer
// each; stream class 1 of a leaf holds its complete runs, class 0 its truncated ones; header word w, a note parks in x.
struct RunsFmt1 {
  typedef uint4 Rec;
  typedef MspView View;
  static constexpr int ROWS = 1, NC = NCLS, COMPLETE = 1;
  static constexpr uint32_t EMPTY = RT_EMPTY, DONE = RT_DONE;
  // (a note names a list position in 11 bits; every position of the 1024-slot record table fits: no limit to test)
  static_assert((((uint32_t)RT - 1u) << 5 | 31u) < RUNS_NO_NOTE, "every list position fits a note that never equals the padding value");
  static __device__ __forceinline__ uint32_t note_pos_max(uint32_t /* dbg */) { return ~0u; }
  static __device__ __forceinline__ uint32_t count(const MspView &v, uint32_t leaf, int cl) {
    return (uint32_t)min((uint64_t)v.cnt2[NCLS * leaf + cl], v.exact ? (uint64_t)v.lcap[NCLS * leaf + cl] : (cl == 1 ? v.cap2c : v.cap2t));
  }
  static __device__ __forceinline__ uint4 *stream(const MspView &v, uint32_t leaf, int cl) {
    if (v.exact) return v.rec2 + v.lbase[NCLS * leaf + cl];
    return v.rec2 + (uint64_t)(leaf >> v.sel_bits) * (v.cap2c + v.cap2t) + (cl == 1 ? 0ull : v.cap2c);
  }
  struct Trunc {                                   // the n truncated runs of a leaf
    uint4 *s; uint64_t n;
    __device__ __forceinline__ uint4 *at(uint64_t g) const { return s + g; }
  };
  static __device__ __forceinline__ Trunc trunc(const MspView &v, uint32_t leaf) { return Trunc{stream(v, leaf, 0), count(v, leaf, 0)}; }
  static __device__ __forceinline__ uint32_t hdr(uint4 r) { return r.w; }
  static __device__ __forceinline__ void set_hdr(uint4 *q, uint32_t w) { q->w = w; }
  static __device__ __forceinline__ uint32_t note(uint4 r) { return r.x; }
  static __device__ __forceinline__ void set_note(uint4 *q, uint32_t note) { q->x = note; q->w = RUN_NOTED; }
  static __device__ __forceinline__ uint32_t slot(uint4 rec, int k, int log) { return rtab_slot_k(rec, k, log); }
  static __device__ __forceinline__ uint4 revcomp(uint4 rec, int len) { return revcomp_record(rec, len); }
  static __device__ __forceinline__ bool prefix_equal(uint4 e, uint4 rec, int len) { return rec_prefix_equal(e, rec, len); }
  // the first len bases of a twin under a header of their own
  static __device__ __forceinline__ uint4 prefix(uint4 twin, int len, uint32_t w) {
    const int rb = 2 * len - 32;                                      // bits of the run beyond the first word: 0 .. 64
    const uint32_t my = (rb >= 32) ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> rb);
    const uint32_t mz = (rb <= 32) ? 0u : ((rb >= 64) ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> (rb - 32)));
    return make_uint4(twin.x, twin.y & my, twin.z & mz, w);
  }
  static __device__ __forceinline__ uint4 zero() { return make_uint4(0u, 0u, 0u, 0u); }
  static __device__ __forceinline__ uint4 load(const uint4 *q) { return *q; }
  static __device__ __forceinline__ void store(uint4 *q, uint4 r) { *q = r; }
  static __device__ __forceinline__ uint4 load_row(const uint4 *rows, uint64_t i) { return rows[i]; }
  static __device__ __forceinline__ void store_row(uint4 *rows, uint64_t i, uint4 r) { rows[i] = r; }
};

// The exporting side of the runs exchange needs none of the leaf kernel's k-mer machinery: a small
// workgroup per leaf (256 threads, 16 KB of LDS: eight or more per CU) deduplicates the leaf's
// complete runs in the 1024-entry record table and leaves the distinct ones, header word =
// multiplicity << 6 | n-1, at the head of the leaf's own stream (leaf_n = their number).  A shard
// of a multi-GPU job holds ~2000 complete runs per leaf; the 65536 workgroups are mostly fixed cost.
// A leaf with more distinct runs than the table holds leaves as it is (multiplicity 1 each): the
// owner's table merges what can be merged.
// Truncated runs (read ends: two per read, each unique -- most of what a rank would ship) are then
// looked up in the same table (runs_find_twin): one that is a prefix of a distinct complete run of
// this rank is replaced by a 16-bit NOTE.  The owner rebuilds the run from its twin.  A noted record
// is marked in place (w = RUN_NOTED, x = the note); leaf_off[leaf] = how many were noted.
constexpr int DX_THREADS = 256, DX_INFL = 4;
__global__ __launch_bounds__(DX_THREADS) void msp_dedupe_export_kernel(int k, int canon, MspView v) {
  typedef RunsFmt1 F;
  __shared__ uint4 rtab[RT];
  __shared__ uint16_t sidx[RT];                    // record-table slot -> position in the leaf's list
  __shared__ uint32_t wsum[DX_THREADS / 64];
  __shared__ uint32_t rt_fail, noted;
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t leaf = blockIdx.x;
  const uint64_t n1 = F::count(v, leaf, 1);
  if (n1 == 0) return;
  uint4 *const stream = F::stream(v, leaf, 1);
  for (int s = tid; s < RT; s += DX_THREADS) rtab[s] = make_uint4(0u, 0u, 0u, RT_EMPTY);
  // (a leaf of 2^19 complete runs or more leaves undeduplicated: see HUGE_LEAF)
  const bool too_many = n1 >= HUGE_LEAF_SENDER;
  if (tid == 0) { rt_fail = ((v.dbg & CFRK_DEBUG_FORCE_RT_OVERFLOW) || too_many) ? 1u : 0u; noted = 0u; }
  __syncthreads();
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  if (!too_many) {
    uint32_t *rmeta = reinterpret_cast<uint32_t *>(rtab);
    uint4 L = zero4;                 // leftover records, lanes [0, c) (see the leaf kernel's phase 1a)
    uint32_t Lh = 0;
    int c = 0;                       // wave-uniform
    auto drain = [&](int cnt) {
      uint32_t h = Lh | ((lane < cnt) ? 0u : RT_DONE);
      rtab_insert_loop(rtab, L, h, RT - 1, RT_TRIPS);
      if ((int32_t)h >= 0) rt_fail = 1u;
    };
    // DX_INFL records per thread are asked for before the first is looked up: a shard's leaf holds a few
    // thousand records, i.e. ~10 trips of one dependent load each -- the kernel was waiting for HBM
    for (uint64_t r0 = 0; r0 < n1; r0 += (uint64_t)DX_INFL * DX_THREADS) {
      uint4 recs[DX_INFL];
#pragma unroll
      for (int u = 0; u < DX_INFL; ++u) {
        const uint64_t r = r0 + (uint64_t)u * DX_THREADS + tid;
        recs[u] = zero4;
        if (r < n1) recs[u] = stream[r];
      }
#pragma unroll
      for (int u = 0; u < DX_INFL; ++u) {
      const uint64_t r = r0 + (uint64_t)u * DX_THREADS + tid;
      const bool valid = r < n1;
      const uint4 rec = recs[u];
      const uint32_t h = rtab_slot_k(rec, k, RT_LOG);
      const uint4 e = rtab[h];
      const bool match = valid && rtab_diff(e, rec) == 0u;
      if (match) atomicAdd(&rmeta[4 * h + 3], 1u << 6);
      const bool left = valid && !match;
      const unsigned long long mask = __ballot(left);
      if (mask == 0ull) continue;
      const int n = __popcll(mask);
      if (c + n > 64) { drain(c); c = 0; }
      uint32_t set[5] = {L.x, L.y, L.z, L.w, Lh};
      const uint32_t mine_[5] = {rec.x, rec.y, rec.z, rec.w, h};
      wave_append<5>(set, mine_, left, mask, c, n);
      L = make_uint4(set[0], set[1], set[2], set[3]); Lh = set[4];
      c += n;
      }
    }
    if (c) drain(c);
  }
  __syncthreads();
  uint32_t nd;
  if (rt_fail) {
    // (every record was read before the barrier; the rewrite touches the header word only)
    for (uint64_t i = tid; i < n1; i += DX_THREADS) F::set_hdr(&stream[i], (1u << 6) | (F::hdr(stream[i]) & 63u));
    nd = (uint32_t)n1;
  } else {
    // occupied slots -> head of the stream (four slots per thread), truncated runs -> notes
    constexpr int PER = RT / DX_THREADS;
    const uint32_t *meta = reinterpret_cast<const uint32_t *>(rtab);
    auto occupied = [&](uint32_t s) { return meta[4 * s + 3] != RT_EMPTY; };
    auto get = [&](uint32_t s) { return rtab[s]; };
    const uint32_t at0 = runs_rank_slots<DX_THREADS, PER>(sidx, wsum, occupied, &nd);
    runs_emit_slots<PER>(at0, occupied, get, [&](uint32_t at, uint4 e) { stream[at] = e; });
    __syncthreads();
    const F::Trunc tr = F::trunc(v, leaf);
    runs_note_truncated<F, DX_THREADS, DX_INFL, RT_LOG>(tr, (v.dbg & CFRK_DEBUG_NO_ANCHORS) ? 0ull : tr.n, k, canon, sidx, F::note_pos_max(v.dbg), get, &noted,
      [&](uint64_t g, bool, uint32_t note) { if (note != RUNS_NO_NOTE) F::set_note(tr.at(g), note); });
    __syncthreads();
  }
  if (tid == 0) { v.leaf_n[leaf] = nd; v.leaf_off[leaf] = noted; }
}

// ------------------------------------------------------------------- multi-GPU by runs, PIPELINED (round 5)
// The sender's half of the pipelined exchange: deduplication AND packing in one kernel, one group of leaves at a
// time, straight into the send buffer -- no rewrite of the streams, no sizes / plan / gather kernels, no host
// round trip (the gather alone was 0.21 ms of a 5.1 ms critical path at N = 8).  (Segments,
// headers and the claim: msp_runs.h, RunsSend.)  Only the used rows of a segment travel.
// A leaf's rows: [distinct complete runs, header word = multiplicity << 6 | n-1][truncated runs that found no twin]
// [notes].  One workgroup per leaf, everything a thread needs of the complete stream in flight at once (DS_INFL
// loads: a shard's leaf is ~2700 records); the truncated runs are looked up once, their verdict (note or record) waits
// in LDS for the leaf's row count, then they are written from a second read that hits the L2.
// SPLIT RECORD TABLE.  With 16-byte entries {bases x 3, meta} the count word of every slot sits in LDS bank 3 mod 4: a
// wave's 64 ds_add on it land on 8 of the 32 banks and serialise 8 ways -- 62 % of this kernel's LDS-active cycles were
// bank conflicts, the LDS was busy for 76 % of its time (profiles/r05/dedupe_send_pmc_before_split_table.txt).  Here the
// bases (12 bytes per slot) and the meta words (4 bytes per slot) are two arrays: the adds spread over all banks.
constexpr int DS_THREADS = 256, DS_INFL = 12, DS_TCAP = 4096;
// insert-or-count one record per lane in the split table (rtab_insert_loop's logic); lanes still without RT_DONE found no place
__device__ __forceinline__ void ds_insert_loop(uint32_t *rb, uint32_t *rm, uint4 rec, uint32_t &h) {
  const uint32_t nm1 = rec.w & 63u;
  for (int it = 0; it < RT_TRIPS && __ballot((int32_t)h >= 0); ++it) {
    const bool p = (int32_t)h >= 0;
    const uint32_t hh = h & (uint32_t)(RT - 1);
    const uint32_t m = rm[hh];
    const uint32_t e0 = rb[3 * hh], e1 = rb[3 * hh + 1], e2 = rb[3 * hh + 2];
    const bool match = ((e0 ^ rec.x) | (e1 ^ rec.y) | (e2 ^ rec.z) | ((m ^ rec.w) & 63u)) == 0u;
    const bool empty = m == RT_EMPTY;
    uint32_t won = 0u;
    if (p && empty) {
      if (atomicCAS(&rm[hh], RT_EMPTY, RT_LOCK) == RT_EMPTY) {
        rb[3 * hh] = rec.x; rb[3 * hh + 1] = rec.y; rb[3 * hh + 2] = rec.z;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        atomicExch(&rm[hh], (1u << 6) | nm1);
        won = 1u;
      }
    }
    atomicAdd(&rm[hh], (p && match) ? (1u << 6) : 0u);
    const bool stay = match || empty || m == RT_LOCK;
    const uint32_t nh = stay ? hh : ((hh + 1) & (uint32_t)(RT - 1));
    h = (p && !match && won == 0u) ? nh : (h | RT_DONE);
  }
}
__global__ __launch_bounds__(DS_THREADS) void msp_dedupe_send_kernel(int k, int canon, MspView v, RunsSend sg) {
  typedef RunsFmt1 F;
  __shared__ uint32_t rb[3 * RT];                  // record table: the bases of slot s at rb[3 s .. 3 s + 2] ...
  __shared__ uint32_t rm[RT];                      // ... its meta word (count << 6 | n-1; RT_EMPTY, RT_LOCK) at rm[s]
  __shared__ uint16_t sidx[RT];                    // record-table slot -> position in the leaf's list
  __shared__ uint16_t tres[DS_TCAP];               // truncated run g: its note, or RUNS_NO_NOTE = travels as a record
  __shared__ uint32_t wsum[DS_THREADS / 64];
  __shared__ uint32_t rt_fail, noted, cu, cn, row0;
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t leaf = sg.leaf0 + blockIdx.x;
  const uint32_t own = leaf % (uint32_t)sg.parts, ll = leaf / (uint32_t)sg.parts;
  uint4 *const seg = sg.packed + (uint64_t)own * sg.seg_cap;
  const uint32_t hrows = 1u + sg.lcount;
  uint4 *const entry = seg + 1u + (ll - sg.ll0);
  const uint64_t n1 = F::count(v, leaf, 1);
  const F::Trunc tr = F::trunc(v, leaf);
  if (n1 + tr.n == 0) { if (tid == 0) *entry = make_uint4(0u, 0u, 0u, 0u); return; }
  const uint4 *const c1 = F::stream(v, leaf, 1);
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  // (a leaf of 2^19 complete runs or more leaves undeduplicated: see HUGE_LEAF)
  const bool too_many = n1 >= HUGE_LEAF_SENDER;
  // the first round of the complete stream is asked for before anything else is done
  uint4 recs[DS_INFL];
#pragma unroll
  for (int u = 0; u < DS_INFL; ++u) {
    const uint64_t r = (uint64_t)u * DS_THREADS + tid;
    recs[u] = zero4;
    if (r < n1 && !too_many) recs[u] = c1[r];
  }
  for (int s2 = tid; s2 < RT; s2 += DS_THREADS) rm[s2] = RT_EMPTY;
  if (tid == 0) { rt_fail = ((v.dbg & CFRK_DEBUG_FORCE_RT_OVERFLOW) || too_many) ? 1u : 0u; noted = 0u; cu = 0u; cn = 0u; }
  __syncthreads();
  if (!too_many) {
    uint4 L = zero4;                 // leftover records, lanes [0, c) (see the leaf kernel's phase 1a)
    uint32_t Lh = 0;
    int c = 0;                       // wave-uniform
    auto drain = [&](int cnt) {
      uint32_t h = Lh | ((lane < cnt) ? 0u : RT_DONE);
      ds_insert_loop(rb, rm, L, h);
      if ((int32_t)h >= 0) rt_fail = 1u;
    };
    for (uint64_t r0 = 0; r0 < n1; r0 += (uint64_t)DS_INFL * DS_THREADS) {
      if (r0) {
#pragma unroll
        for (int u = 0; u < DS_INFL; ++u) {
          const uint64_t r = r0 + (uint64_t)u * DS_THREADS + tid;
          recs[u] = zero4;
          if (r < n1) recs[u] = c1[r];
        }
      }
#pragma unroll
      for (int u = 0; u < DS_INFL; ++u) {
        const uint64_t r = r0 + (uint64_t)u * DS_THREADS + tid;
        if (r0 + (uint64_t)u * DS_THREADS >= n1) break;          // (wave-uniform)
        const bool valid = r < n1;
        const uint4 rec = recs[u];
        const uint32_t h = rtab_slot_k(rec, k, RT_LOG);
        const uint32_t m = rm[h];
        const uint32_t e0 = rb[3 * h], e1 = rb[3 * h + 1], e2 = rb[3 * h + 2];
        // (EMPTY and LOCK carry low bits no record has: they never compare equal; stale bases of an empty slot do not matter)
        const bool match = valid && ((e0 ^ rec.x) | (e1 ^ rec.y) | (e2 ^ rec.z) | ((m ^ rec.w) & 63u)) == 0u;
        if (match) atomicAdd(&rm[h], 1u << 6);
        const bool left = valid && !match;
        const unsigned long long mask = __ballot(left);
        if (mask == 0ull) continue;
        const int n = __popcll(mask);
        if (c + n > 64) { drain(c); c = 0; }
        uint32_t set[5] = {L.x, L.y, L.z, L.w, Lh};
        const uint32_t mine_[5] = {rec.x, rec.y, rec.z, rec.w, h};
        wave_append<5>(set, mine_, left, mask, c, n);
        L = make_uint4(set[0], set[1], set[2], set[3]); Lh = set[4];
        c += n;
      }
    }
    if (c) drain(c);
  }
  __syncthreads();
  const bool plain = rt_fail != 0u;                 // no deduplication: every complete run leaves with multiplicity 1, no notes
  const uint32_t nt = (uint32_t)min(tr.n, (uint64_t)0xFFFFFFFFull);
  const bool anchors = !(v.dbg & CFRK_DEBUG_NO_ANCHORS);
  uint32_t nd = (uint32_t)n1, at0 = 0;
  constexpr int PER = RT / DS_THREADS;
  auto occupied = [&](uint32_t s) { return rm[s] != RT_EMPTY; };
  auto get = [&](uint32_t s) { return make_uint4(rb[3 * s], rb[3 * s + 1], rb[3 * s + 2], rm[s]); };
  if (!plain) {
    // occupied slots -> positions in the leaf's list (four slots per thread); then the first DS_TCAP truncated runs are
    // looked up, their verdict waits in LDS
    at0 = runs_rank_slots<DS_THREADS, PER>(sidx, wsum, occupied, &nd);
    __syncthreads();
    runs_note_truncated<F, DS_THREADS, 1, RT_LOG>(tr, anchors ? min(nt, (uint32_t)DS_TCAP) : 0u, k, canon, sidx, F::note_pos_max(v.dbg), get, &noted,
      [&](uint64_t g, bool valid, uint32_t note) { if (valid) tres[g] = (uint16_t)note; });
    __syncthreads();
  }
  const uint32_t na = plain ? 0u : noted, nu = nt - na;
  if (tid == 0) row0 = runs_claim_rows<F>(sg, own, entry, hrows, nd, nu, na);
  __syncthreads();
  if (row0 == RUNS_NO_ROOM) return;
  uint4 *const dst = seg + hrows + row0;
  if (plain) { runs_write_plain<F, DS_THREADS>(dst, c1, nd, tr, nt); return; }
  runs_emit_slots<PER>(at0, occupied, get, [&](uint32_t at, uint4 e) { dst[at] = e; });
  runs_split_truncated<F, false>(tr, nt, nu, na, dst + nd, &cu, &cn, DS_THREADS,
    [&](uint32_t i, const uint4 &) { return (i < (uint32_t)DS_TCAP && anchors) ? (uint32_t)tres[i] : RUNS_NO_NOTE; });
}

// the shared kernels of the one-shot exchange (msp_runs.h) under the names the profiles know
__global__ __launch_bounds__(256) void msp_runs_sizes_kernel(MspView v, uint4 *__restrict__ sz, unsigned long long *__restrict__ plan_sync) {
  runs_sizes<RunsFmt1>(v, sz, plan_sync);
}
__global__ __launch_bounds__(256) void msp_runs_gather_kernel(MspView v, const uint64_t *__restrict__ dst_off, uint4 *__restrict__ out,
                                                                       const uint64_t *__restrict__ plan_rows, const uint64_t *__restrict__ seg_start, int parts, uint64_t cap_rows) {
  __shared__ uint32_t cu, cn;
  runs_gather<RunsFmt1>(v, dst_off, out, plan_rows, seg_start, parts, cap_rows, &cu, &cn);
}
__global__ __launch_bounds__(256) void msp_runs_scatter_kernel(const uint4 *__restrict__ in, RunsRecv rr, int lpp, int k,
                                                                        const uint64_t *__restrict__ src_off,
                                                                        const uint64_t *__restrict__ dst1, const uint64_t *__restrict__ dst0,
                                                                        uint4 *__restrict__ rec2) {
  runs_scatter<RunsFmt1>(in, rr, lpp, k, src_off, dst1, dst0, rec2);
}

// the few records that did not fit their leaf stream: counted k-mer by k-mer in the HBM table
__global__ __launch_bounds__(256) void msp_spill_list_kernel(const uint4 *__restrict__ recs, uint32_t n, int k,
                                                             int canon, TableView t) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) spill_record(recs[i], k, canon != 0, t);
}

// the first chunk of a batch (behind msp_sum_kernel): what share of its records are truncated runs -- the records
// of sub-region 0 of every level-1 bin (1/64 of the chunk, every bin in it): out[1] += records looked at,
// out[2] += truncated ones among them
__global__ __launch_bounds__(256) void msp_class_sample_kernel(MspView v, unsigned long long *out) {
  const uint32_t reg = l1_reg(blockIdx.x, 0u);
  const uint32_t n = (uint32_t)min((uint64_t)v.cnt1[reg], v.cap1);
  const uint32_t *w = reinterpret_cast<const uint32_t *>(v.rec1 + (uint64_t)reg * v.cap1) + 3;
  uint32_t tr = 0;
  for (uint32_t i = threadIdx.x; i < n; i += 256u) tr += ((w[4 * (size_t)i] & 192u) != 192u) ? 1u : 0u;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) tr += __shfl_xor(tr, d);
  if ((threadIdx.x & 63) == 0 && tr) atomicAdd(&out[2], (unsigned long long)tr);
  if (threadIdx.x == 0) atomicAdd(&out[1], (unsigned long long)n);
}

__global__ void msp_info_kernel(MspView v, uint64_t *out) {
  // diagnostics: record totals / maxima per level (single block)
  __shared__ unsigned long long tot1, max1, tot2, max2;
  if (threadIdx.x == 0) { tot1 = max1 = tot2 = max2 = 0; }
  __syncthreads();
  for (int i = threadIdx.x; i < B1 * (int)v.nxg; i += blockDim.x) {
    atomicAdd(&tot1, (unsigned long long)v.cnt1[i]);
    atomicMax(&max1, (unsigned long long)v.cnt1[i]);
  }
  for (int i = threadIdx.x; i < NCLS * NLEAF; i += blockDim.x) {
    atomicAdd(&tot2, (unsigned long long)v.cnt2[i]);
    atomicMax(&max2, (unsigned long long)v.cnt2[i]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[0] = tot1; out[1] = max1; out[2] = v.cap1; out[3] = tot2; out[4] = max2; out[5] = v.cap2c;
  }
}

}  // namespace

// ------------------------------------------------------------------------------------ host
cfrk_msp *cfrk_msp_get(cfrk_ctx *ctx) {
  if (!ctx->msp) {
    ctx->msp = new (std::nothrow) cfrk_msp();
    if (ctx->msp) memset(ctx->msp, 0, sizeof(cfrk_msp));
  }
  return ctx->msp;
}

bool cfrk_msp_usable(const cfrk_ctx *ctx) {
  return !ctx->g_two && ctx->g_k >= 16 && ctx->g_k <= 32 && !(ctx->g_flags & CFRK_FORCE_HASH);
}

void cfrk_msp_reset(cfrk_ctx *ctx) {
  if (ctx->msp) ctx->msp->view.seg_bits = 0;
  if (ctx->msp) { ctx->msp->pending = false; ctx->msp->table_dirty = false; ctx->msp->list_n_valid = false; ctx->msp->runs_ready = false;
                  ctx->msp->runs_deduped = false; ctx->msp->runs_unchecked = false; ctx->msp->lists_group = 0; }
}

void cfrk_msp_note_table_write(cfrk_ctx *ctx) {
  cfrk_msp *m = cfrk_msp_get(ctx);
  if (m) m->table_dirty = true;
}

bool cfrk_msp_table_written(const cfrk_ctx *ctx) {
  // without msp state nobody tracked the writes: assume written
  return !ctx->msp || ctx->msp->table_dirty;
}

void cfrk_msp_destroy(cfrk_ctx *ctx) {
  delete ctx->msp;
  ctx->msp = nullptr;
}

static void msp_params(int k, int *W, int *m) {
  // The longer the window, the longer the runs (fewer, fuller records): W = k - 12 keeps
  // m = k - W + 1 = 13, the smallest m-mer whose canonical values (3.4e7) rarely repeat across
  // the loci of a genome -- with fewer distinct minimizers the leaves get lumpy (at k = 31: m = 11 gave a
  // 10x heavier leaf, m = 12 2.3x).  W is capped by what a 48-base record holds (49 - k k-mers),
  // which raises m to 14 / 16 for k = 31 / 32.
  // k <= 26 (round 5): m = 12.  There the window is what is short (5 .. 14 k-mers at m = 13: one record per three k-mers
  // at k = 17), and one more k-mer per window is 7 .. 14 % fewer records through all three kernels (10 M reads:
  // k = 17 9.03 -> 8.30 ms, 19 7.62 -> 6.79, 22 6.30 -> 5.98, 25 5.41 -> 5.21; 100 M reads of a 10^8-base genome:
  // k = 20 51.5 -> 48.3 ms, k = 25 35.6 -> 35.0, k = 28 no change; heaviest stream / mean unchanged at 3.3).  m = 11
  // was measured too: k = 17 7.85 ms, but the heaviest stream grows to 4.1 x the mean and outgrows its room.
  *W = std::min(k <= 26 ? k - 11 : k - 12, 49 - k);
  *m = k - *W + 1;
}

// Sub-regions (cursors) per level-1 bin, from the expected number of records.  Many cursors keep
// the chains of returning atomics on one address short and spread the write frontiers (msp_dev.h:
// NXG); P2 reads a bin's sub-regions as one stream, so they cost it nothing.  Tiny batches keep 8
// (every sub-region reserves 2048 records of slack).
static int msp_nxg(double expect_records) { return expect_records >= 2.5e7 ? NXG : NXCD; }

// bytes of pool memory one pipeline pass over `span` base positions needs (the caps below)
static size_t msp_need(const cfrk_ctx *ctx, int64_t span) {
  int W0, m0;
  msp_params(ctx->g_k, &W0, &m0);
  const double expect0 = (double)span * (2.0 / (W0 + 1) + 1.0 / 64.0);
  return (size_t)(expect0 * 1.35 * 16) + (size_t)B1 * msp_nxg(expect0) * 2048 * 16 + (size_t)(expect0 * 2.7 * 16) +
         (size_t)NLEAF * 192 * 16 + (size_t)ctx->g_cap * 12;
}

// one pass of P1 -> P2 -> P3 over the P1 tiles [tile0, tile0 + ntiles): the k-mers that START in
// those tiles (P1 reads its neighbours' bases from the whole buffer, so a tile range produces
// exactly the records it produces in a full launch)
// slack >= 1 widens the per-leaf streams beyond what msp_need() accounts for (memory permitting)
// sel_bits / sel_val: only the leaves with (leaf & (2^sel_bits - 1)) == sel_val are emitted and counted;
// first: the first pass of an add (later passes append to the result list and keep the leaf index)
static int msp_count_tiles(cfrk_ctx *ctx, cfrk_msp *ms, const int8_t *d_data, int64_t nN, int64_t tile0,
                           int64_t ntiles, double slack, int sel_bits = 0, uint32_t sel_val = 0, bool first = true) {
  int rc;
  const int k = ctx->g_k;
  int W, m;
  msp_params(k, &W, &m);
  const int canon = (ctx->g_flags & CFRK_CANONICAL) ? 1 : 0;
  const int64_t span = std::min(nN, ntiles * (int64_t)P1_WAVES * P1_OWN * 32);

  // expected records: one per minimizer change (2/(W+1) per position) plus read ends
  const double dens = 2.0 / (W + 1) + 1.0 / 64.0;
  const double expect_all = (double)span * dens;                 // records of the whole batch
  const double expect = expect_all / (double)(1u << sel_bits);   // ... of this pass (1 / 2^sel_bits of the leaves)
  const int nxg = msp_nxg(expect);
  const uint64_t cap1 = (uint64_t)(expect / (B1 * nxg) * 1.35) + 2048;   // per sub-region
  // per leaf: complete runs dominate at depth; truncated ones are ~2 per read plus invalid bases
  // (a leaf of the pass holds ALL its records: the pass has fewer leaves, not lighter ones)
  const uint64_t cap2c = (uint64_t)(expect_all / NLEAF * 2.1 * slack) + 96;
  const uint64_t cap2t = (uint64_t)(expect_all / NLEAF * 0.6 * slack) + 96;   // truncated runs: ~15 % of the records
  // Large batches are counted in CHUNKS of tiles: P1 on chunk c, then P2 on chunk c, with one
  // level-1 buffer that only ever holds one chunk (C3: 2.7 GB instead of 40 GB); the leaf streams
  // accumulate over the chunks.  Same kernels, same work; anything that overflows a region starts
  // over on the one-chunk path below, whose cursors add up to the batch's exact demand.
  // (What the chunks were built for did not pay: running P1 on chunk c+1 BESIDE P2 on chunk c in one
  // launch -- persistent roles or an interleaved grid -- takes as long as the two one after the other,
  // profiles/r03/persistent_p1_is_slower.txt: a CU is full with three partition workgroups.)
  const bool small_pipe = (ctx->dbg_flags & CFRK_DEBUG_SMALL_PIPELINE) != 0;
  const int64_t chunk_min = small_pipe ? 3 : 16384;            // tiles (16384 = 256 MB of input)
  // as many chunks as keep the level-1 buffer under ~6 GB (each costs ~30 us of launches and kernel
  // tails: 16 chunks +0.5 ms on C3, 64 +2.7 ms -- and nothing comes back from the Infinity Cache
  // even at 512 chunks of 43 MB, profiles/r03/chunk_count_sweep_c3.txt)
  // (a batch whose level-1 records fit ~6 GB anyway -- a shard of a multi-GPU job -- stays in one chunk)
  int nchunks = (int)std::min<int64_t>(small_pipe ? 5 : (int64_t)((double)B1 * nxg * cap1 * 16.0 / 6e9) + 1, ntiles / chunk_min);
  if (ctx->dbg_param[CFRK_PARAM_MSP_CHUNKS] > 0) nchunks = std::max(1, std::min((int)ctx->dbg_param[CFRK_PARAM_MSP_CHUNKS], (int)std::min<int64_t>(4096, ntiles / 8)));   // (experiments)
  const bool pipelined = (nxg == NXG || small_pipe) && nchunks >= 2 && !(ctx->dbg_flags & CFRK_DEBUG_NO_PIPELINE);
  if (!pipelined) nchunks = 1;
  const int64_t chunk_tiles = (ntiles + nchunks - 1) / nchunks;
  // per sub-region of ONE chunk (the cursors of a chunk see 1 / nchunks of the records)
  const uint64_t cap1c = pipelined ? (uint64_t)(expect * ((double)chunk_tiles / (double)ntiles) / (B1 * nxg) * 1.35) + 2048 : cap1;

  void *p;
  MspView &v = ms->view;
  const size_t nreg = (size_t)B1 * nxg;
  if ((rc = cfrk_pool_get(ctx, BUF_MSP_L1, nreg * (pipelined ? cap1c : cap1) * sizeof(uint4), &p))) return rc;
  v.rec1 = (uint4 *)p; v.cap1 = cap1; v.nxg = (uint32_t)nxg; v.dbg = ctx->dbg_flags;
  v.sel_mask = (1u << sel_bits) - 1u; v.sel_val = sel_val; v.sel_bits = (uint32_t)sel_bits;
  // (a chunked batch sizes its leaf streams after the first chunk: whatever the pool already holds will do until then)
  if ((rc = cfrk_pool_get(ctx, BUF_MSP_L2, (pipelined && !small_pipe) ? 16 : (size_t)(NLEAF >> sel_bits) * (cap2c + cap2t) * sizeof(uint4), &p))) return rc;
  v.rec2 = (uint4 *)p; v.cap2c = cap2c; v.cap2t = cap2t;
  uint32_t sub_bits = msp_sub_bits(ctx, ctx->g_cap / NLEAF);
  if (ctx->g_flags & CFRK_RUNS_ONLY) sub_bits = 0;       // (the exchange by runs has no room for the bits in a distinct run's header)
  const bool sub = sub_bits != 0u;
  v.sub_bits = sub_bits; v.seg_bits = sub_bits;
  // (leaf index: one entry per leaf, or per (leaf, sub-value) when leaves are shared)
  const size_t nseg = (size_t)NLEAF << sub_bits;
  if ((rc = msp_aux_buffers(ctx, v, nseg, nxg, (size_t)NCLS * NLEAF))) return rc;
  if ((rc = cfrk_pool_get(ctx, BUF_MSP_OUTK, (size_t)ctx->g_cap * 8, &p))) return rc;
  v.out_keys = (uint64_t *)p;
  if ((rc = cfrk_pool_get(ctx, BUF_MSP_OUTC, (size_t)ctx->g_cap * 4, &p))) return rc;
  v.out_cnt = (uint32_t *)p; v.out_cap = ctx->g_cap;
  v.stats = ctx->g_stats;
  TableView t = cfrk_table_view(ctx);

  if ((rc = msp_aux_clear(ctx, v, nseg, nxg, (size_t)NCLS * NLEAF, first))) return rc;

  // Both levels are laid out for an input that spreads evenly over the minimizer space.  One that
  // does not -- deep coverage of a small genome puts tens of thousands of records into a handful of
  // leaves, a single amplicon into a handful of level-1 bins -- overflows its regions; the cursors
  // keep counting past the capacity, so after P2 the host knows the exact demand of both levels
  // (one 40-byte D2H + stream sync per add).  A few overflowing records (lumpy leaves) were
  // parked in a small buffer and are counted through the HBM table; more than that and the
  // level is laid out again back to back with exactly the room each region needs -- all records
  // together never exceed what the buffers already hold -- and its kernel runs again.
  constexpr uint32_t OVF_CAP = 1u << 20;
  if ((rc = cfrk_pool_get(ctx, BUF_MSP_OVF, (size_t)OVF_CAP * sizeof(uint4), &p))) return rc;
  v.ovf = (uint4 *)p; v.ovf_cap = (uint32_t)std::min<double>((double)OVF_CAP, expect / 256.0);   // "a few": < 0.4 %
  if ((rc = cfrk_pool_get(ctx, BUF_MSP_OVF1, (size_t)OVF_CAP * sizeof(uint4), &p))) return rc;
  v.ovf1 = (uint4 *)p; v.ovf1_cap = v.ovf_cap;
  // a job that only partitions (CFRK_RUNS_ONLY) has no table of its own for parked records: any
  // overflow goes straight to the exact re-layout
  if (ctx->g_flags & CFRK_RUNS_ONLY) v.ovf_cap = v.ovf1_cap = 0;
  v.exact = 0; v.lbase = nullptr; v.lcap = nullptr;
  v.exact1 = 0; v.rbase = nullptr; v.rcap = nullptr;
  // stand-alone P1 over the tiles [t0, t1), one workgroup each
  auto launch_p1 = [&](int64_t t0, int64_t t1, const MspView &vv) -> int {
    const dim3 g1((unsigned)(t1 - t0)), b1(P1_THREADS);
#define CFRK_P1B_CASE(WW) \
    case WW: \
      if (sub) hipLaunchKernelGGL((msp_p1b_kernel<WW, (WW >= 16 ? 4 : WW >= 12 ? 6 : WW >= 8 ? 8 : WW >= 6 ? 10 : 12), true>), g1, b1, 0, ctx->stream, d_data, nN, k, m, canon, t0, vv, t); \
      else hipLaunchKernelGGL((msp_p1b_kernel<WW, (WW >= 16 ? 4 : WW >= 12 ? 6 : WW >= 8 ? 8 : WW >= 6 ? 10 : 12), false>), g1, b1, 0, ctx->stream, d_data, nN, k, m, canon, t0, vv, t); \
      break;
    switch (W) {
      CFRK_P1B_CASE(4) CFRK_P1B_CASE(5) CFRK_P1B_CASE(6) CFRK_P1B_CASE(7) CFRK_P1B_CASE(8) CFRK_P1B_CASE(9)
      CFRK_P1B_CASE(10) CFRK_P1B_CASE(11) CFRK_P1B_CASE(12) CFRK_P1B_CASE(13) CFRK_P1B_CASE(14)
      CFRK_P1B_CASE(15) CFRK_P1B_CASE(16) CFRK_P1B_CASE(17) CFRK_P1B_CASE(18)
      default: return cfrk_fail(ctx, CFRK_ERR_ARG, "no partition kernel for W=%d", W);
    }
#undef CFRK_P1B_CASE
    HIP_TRY(ctx, hipGetLastError());
    return CFRK_OK;
  };
  // exact layout of the leaf streams from the demand their cursors counted (they count on past a
  // stream's capacity): streams back to back, each with exactly the room it needs; the buffer grows
  // when the batch holds more records than it was sized for (a chunked batch's streams were sized from
  // its first chunk)
  auto layout_l2 = [&](uint32_t slack) -> int {
    int rc2;
    void *q;
    if ((rc2 = cfrk_pool_get(ctx, BUF_MSP_LAYOUT, (size_t)NCLS * NLEAF * (sizeof(uint64_t) + sizeof(uint32_t)), &q))) return rc2;
    uint64_t *lbase = (uint64_t *)q;
    uint32_t *lcap = (uint32_t *)(lbase + NCLS * NLEAF);
    hipLaunchKernelGGL(msp_layout_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t *)v.cnt2, (uint32_t)(NCLS * NLEAF), lbase, lcap, slack);
    HIP_TRY(ctx, hipGetLastError());
    if ((rc2 = cfrk_pool_get(ctx, BUF_SCRATCH, 64 * sizeof(uint64_t), &q))) return rc2;
    hipLaunchKernelGGL(msp_sum_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t *)v.cnt2, (uint32_t)(NCLS * NLEAF), (uint64_t *)q);
    HIP_TRY(ctx, hipGetLastError());
    uint64_t all = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&all, q, sizeof all, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    all += (uint64_t)slack * NCLS * NLEAF;
    if ((size_t)all * sizeof(uint4) > ctx->pool[BUF_MSP_L2].cap) {
      if ((rc2 = cfrk_pool_get(ctx, BUF_MSP_L2, (size_t)all * sizeof(uint4), &q))) return rc2;
      v.rec2 = (uint4 *)q;
    }
    HIP_TRY(ctx, hipMemsetAsync(v.cnt2, 0, (size_t)NCLS * NLEAF * sizeof(uint32_t), ctx->stream));
    v.exact = 1; v.lbase = lbase; v.lcap = lcap;
    return CFRK_OK;
  };
  const unsigned p2_grid = 2u * (unsigned)std::max(8, ctx->num_cus / 8 * 8);   // P2: persistent, two workgroups per CU, a multiple of 8
  const bool defer = (ctx->g_flags & CFRK_RUNS_ONLY) && (ctx->g_flags & CFRK_RUNS_DEFER);
  bool run_p1 = true, settled = false, piped = pipelined;
  uint64_t parked1 = 0, parked2 = 0;
  for (int attempt = 0; attempt < 5; ++attempt) {
    if (piped) {
      // ---- chunks: P1(c), P2(c) on the one level-1 buffer
      HIP_TRY(ctx, hipMemsetAsync(ctx->g_stats + ST_L1OVF, 0, 2 * sizeof(uint64_t), ctx->stream));   // ST_L1OVF, ST_OVFN1
      HIP_TRY(ctx, hipMemsetAsync(ctx->g_stats + ST_L2OVF, 0, 2 * sizeof(uint64_t), ctx->stream));   // ST_L2OVF, ST_OVFN
      MspView vc = v;
      vc.cap1 = cap1c;
      for (int c = 0; c < nchunks; ++c) {
        const int64_t t0 = tile0 + (int64_t)c * chunk_tiles, t1 = std::min(tile0 + ntiles, t0 + chunk_tiles);
        if (t0 >= t1) break;
        if (c > 0 || attempt > 0) HIP_TRY(ctx, hipMemsetAsync(vc.cnt1, 0, nreg * sizeof(uint32_t), ctx->stream));   // (chunk 0 of the first attempt: cleared above)
        if ((rc = launch_p1(t0, t1, vc))) return rc;
        if (c == 0 && !small_pipe && !v.exact) {
          // The leaf streams are sized from what the first chunk really made, not from the worst
          // density a batch of unknown read length could have (the estimate above allows for reads
          // as short as 2k: 1.34 x the records 150-base reads make, times 2.7 for lumpy leaves --
          // 79 GB for C3's 21.9 GB of records).  One 24-byte read-back + sync per add.
          if ((rc = cfrk_pool_get(ctx, BUF_SCRATCH, 64 * sizeof(uint64_t), &p))) return rc;
          hipLaunchKernelGGL(msp_sum_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t *)vc.cnt1, (uint32_t)nreg, (uint64_t *)p);
          HIP_TRY(ctx, hipGetLastError());
          hipLaunchKernelGGL(msp_class_sample_kernel, dim3(B1), dim3(256), 0, ctx->stream, vc, (unsigned long long *)p);
          HIP_TRY(ctx, hipGetLastError());
          uint64_t made[3] = {0, 0, 0};               // records of the chunk; records sampled, truncated ones among them
          HIP_TRY(ctx, hipMemcpyAsync(made, p, sizeof made, hipMemcpyDeviceToHost, ctx->stream));
          HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
          // records of this pass's leaves in the whole batch (+3 %: chunks differ a little), per leaf
          const double per_leaf = (double)made[0] * ((double)ntiles / (double)(t1 - t0)) * 1.03 / (double)(NLEAF >> sel_bits);
          // ... split into complete and truncated runs by the sample (truncated: two per read + invalid
          // bases -- 16 % of a deep batch of 150-base reads, half of the records of 50-base reads at
          // k = 31); the heaviest complete stream of a uniform batch is ~1.35 x the mean one
          const double ft = made[1] >= 4096 ? std::min(1.0, (double)made[2] / (double)made[1] + 0.01) : 0.5;
          double fc_slack, ft_slack;
          msp_leaf_slack(ctx, W, &fc_slack, &ft_slack);
          if (ctx->dbg_param[CFRK_PARAM_L2_SLACK_COMPLETE] > 0) fc_slack = ctx->dbg_param[CFRK_PARAM_L2_SLACK_COMPLETE];   // (experiments)
          if (ctx->dbg_param[CFRK_PARAM_L2_SLACK_TRUNCATED] > 0) ft_slack = ctx->dbg_param[CFRK_PARAM_L2_SLACK_TRUNCATED];
          const uint64_t m2c = (uint64_t)(per_leaf * (1.0 - ft) * fc_slack + per_leaf * 0.02) + 512, m2t = (uint64_t)(per_leaf * ft * ft_slack) + 256;
          if (m2c + m2t < v.cap2c + v.cap2t) { v.cap2c = m2c; v.cap2t = m2t; }
          if ((rc = cfrk_pool_get(ctx, BUF_MSP_L2, (size_t)(NLEAF >> sel_bits) * (v.cap2c + v.cap2t) * sizeof(uint4), &p))) return rc;
          v.rec2 = (uint4 *)p;
          vc.cap2c = v.cap2c; vc.cap2t = v.cap2t; vc.rec2 = v.rec2;
        }
        hipLaunchKernelGGL(msp_p2_kernel, dim3(p2_grid), dim3(P2_THREADS), 0, ctx->stream, k, canon, vc, t);
        HIP_TRY(ctx, hipGetLastError());
      }
    } else {
    if (run_p1) {
      HIP_TRY(ctx, hipMemsetAsync(ctx->g_stats + ST_L1OVF, 0, 2 * sizeof(uint64_t), ctx->stream));   // ST_L1OVF, ST_OVFN1
      if ((rc = launch_p1(tile0, tile0 + ntiles, v))) return rc;
    }
    HIP_TRY(ctx, hipMemsetAsync(ctx->g_stats + ST_L2OVF, 0, 2 * sizeof(uint64_t), ctx->stream));   // ST_L2OVF, ST_OVFN
    hipLaunchKernelGGL(msp_p2_kernel, dim3(p2_grid), dim3(P2_THREADS), 0, ctx->stream, k, canon, v, t);
    HIP_TRY(ctx, hipGetLastError());
    }
    // CFRK_RUNS_DEFER: the add ends here, unsynchronised -- whether a region overflowed is looked at by the export
    // (the group epilogue of the pipelined one folds the flags into what the host waits for anyway)
    if (defer) { settled = true; break; }
    uint64_t st[ST_NWORDS];
    if ((rc = cfrk_msp_sync_stats(ctx, st))) return rc;
    if (st[ST_CWRAP]) return CFRK_INTERNAL_FLOOD;      // (nothing of this pass has been counted yet)
    // (level-1 records PARKED in a chunked attempt whose leaf streams overflowed: which records are parked depends on
    //  the order of atomics, so the exact stream sizes counted now need not hold when P1 runs again -- same remedy)
    if (piped && (st[ST_L1OVF] || (st[ST_L2OVF] && st[ST_OVFN1]))) {
      // a level-1 region overflowed by more than the parking buffer takes: the level-1 cursors of a chunk
      // do not add up to the batch's demand (the buffer is reused), so the batch starts over on the
      // one-chunk path, which lays the overflowing level out exactly -- with the leaf streams the
      // density estimate gives (what the first chunk suggested is void)
      piped = false;
      if ((rc = cfrk_pool_get(ctx, BUF_MSP_L1, nreg * cap1 * sizeof(uint4), &p))) return rc;
      v.rec1 = (uint4 *)p;
      v.cap2c = cap2c; v.cap2t = cap2t;
      if ((rc = cfrk_pool_get(ctx, BUF_MSP_L2, (size_t)(NLEAF >> sel_bits) * (cap2c + cap2t) * sizeof(uint4), &p))) return rc;
      v.rec2 = (uint4 *)p;
      HIP_TRY(ctx, hipMemsetAsync(v.cnt1, 0, (nreg + (size_t)NCLS * NLEAF) * sizeof(uint32_t), ctx->stream));   // cnt1 and cnt2
      run_p1 = true;
      continue;
    }
    if (piped && st[ST_L2OVF]) {
      // only leaf streams overflowed (the first chunk was no measure of the batch: reads sorted or
      // clustered, a short-read or N-rich prefix, concatenated libraries).  Their cursors counted on
      // over ALL chunks, so the batch's exact demand is known: lay the streams out back to back and
      // run the chunks again (one more P1 + P2 over the input; the level-1 buffer stays one chunk).
      // (nothing was parked on level 1 -- see above -- so P1 makes the same records again; eight to spare per stream)
      if ((rc = layout_l2(8u))) return rc;
      continue;
    }
    if (st[ST_L1OVF]) {
      // exact level-1 layout; P2 ran on an incomplete level 1 and is redone as well
      uint64_t maxbin;                                 // (unused: P2 is persistent and sizes its work from the cursors)
      if ((rc = msp_layout_level1(ctx, v.cnt1, nxg, (size_t)NCLS * NLEAF, cap1, &v.rec1, &v.rbase, &v.rcap, &maxbin))) return rc;
      v.exact1 = 1;
      run_p1 = true;
      continue;
    }
    parked1 = st[ST_OVFN1];
    if (st[ST_L2OVF]) {
      if ((rc = layout_l2(0u))) return rc;
      run_p1 = false;
      continue;
    }
    parked2 = st[ST_OVFN];
    settled = true;
    break;
  }
  if (!settled) return cfrk_fail(ctx, CFRK_ERR_STATE, "the record regions did not settle after an exact layout");
  if (parked1 && v.ovf1_cap) {
    const uint32_t n = (uint32_t)std::min<uint64_t>(parked1, v.ovf1_cap);
    hipLaunchKernelGGL(msp_spill_list_kernel, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, (const uint4 *)v.ovf1, n, k, canon, t);
    HIP_TRY(ctx, hipGetLastError());
  }
  if (parked2 && v.ovf_cap) {
    const uint32_t n = (uint32_t)std::min<uint64_t>(parked2, v.ovf_cap);
    hipLaunchKernelGGL(msp_spill_list_kernel, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, (const uint4 *)v.ovf, n, k, canon, t);
    HIP_TRY(ctx, hipGetLastError());
  }
  const bool runs_only = (ctx->g_flags & CFRK_RUNS_ONLY) != 0;
  if (runs_only) { if (!defer) hipLaunchKernelGGL(msp_dedupe_export_kernel, dim3(NLEAF), dim3(DX_THREADS), 0, ctx->stream, k, canon, v); }
  else if (sub) {
    const dim3 g3(((unsigned)NLEAF >> sel_bits) << v.sub_bits);
    if (canon) hipLaunchKernelGGL((msp_p3_kernel<true, true>), g3, dim3(P3_THREADS), 0, ctx->stream, k, 0u, v, t);
    else hipLaunchKernelGGL((msp_p3_kernel<false, true>), g3, dim3(P3_THREADS), 0, ctx->stream, k, 0u, v, t);
  }
  else if (canon) hipLaunchKernelGGL((msp_p3_kernel<true, false>), dim3((unsigned)NLEAF >> sel_bits), dim3(P3_THREADS), 0, ctx->stream, k, 0u, v, t);
  else hipLaunchKernelGGL((msp_p3_kernel<false, false>), dim3((unsigned)NLEAF >> sel_bits), dim3(P3_THREADS), 0, ctx->stream, k, 0u, v, t);
  HIP_TRY(ctx, hipGetLastError());
  if (!runs_only) {
    hipLaunchKernelGGL(msp_huge_leaves_kernel, dim3((((unsigned)NLEAF >> sel_bits) + 255u) / 256u), dim3(256), 0, ctx->stream, k, canon, 0, (uint32_t)NLEAF >> sel_bits, v, t);
    HIP_TRY(ctx, hipGetLastError());
  }
  ms->pending = !runs_only;
  ms->runs_ready = runs_only;
  ms->runs_deduped = runs_only && !defer;
  ms->runs_unchecked = defer;
  ms->leaf_form = !runs_only;
  ms->list_n_valid = false;
  return CFRK_OK;
}

// How many passes does a batch of nN base positions take so that one pass's buffers (need_fn) fit
// the memory the pool may use (have: what it holds already)?  0 = not even a minimal pass fits.
int cfrk_msp_plan_groups(cfrk_ctx *ctx, int64_t nN, size_t (*need_fn)(const cfrk_ctx *, int64_t), size_t have, int *groups) {
  *groups = 1;
  if (need_fn(ctx, nN) <= have && !ctx->mem_budget) return CFRK_OK;   // fits what the pool already holds
  size_t free_b = 0, total_b = 0;
  HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
  size_t budget = have + free_b;
  if (ctx->mem_budget) budget = std::min(budget, ctx->mem_budget);
  // a pass over 1/g of the leaves needs the record buffers of 1/g of the batch (power-of-two g:
  // the subset is picked by the leaf id's low bits)
  int g = 1;
  while (need_fn(ctx, (nN + g - 1) / g) > budget) {
    if (g >= 256) {
      *groups = 0;
      return CFRK_OK;
    }
    g *= 2;
  }
  *groups = g;
  return CFRK_OK;
}

int cfrk_msp_count(cfrk_ctx *ctx, const int8_t *d_data, int64_t nN) {
  cfrk_msp *ms = cfrk_msp_get(ctx);
  if (!ms) return cfrk_fail(ctx, CFRK_ERR_NOMEM, "host allocation failed");
  int rc;
  const int64_t nchunks = (nN + 31) / 32;
  const int64_t nwaves = (nchunks + P1_OWN - 1) / P1_OWN;
  const int64_t ntiles = (nwaves + P1_WAVES - 1) / P1_WAVES;
  if (ntiles > 0x7FFFFFFF) return cfrk_fail(ctx, CFRK_ERR_ARG, "batch too large for one add");
  // every buffer a pass needs must fit: decide before touching the pool so that a refusal leaves
  // the context usable for the fallback path
  const size_t have = ctx->pool[BUF_MSP_L1].cap + ctx->pool[BUF_MSP_L2].cap + ctx->pool[BUF_MSP_OUTK].cap +
                      ctx->pool[BUF_MSP_OUTC].cap;
  int groups = 1;
  if ((rc = cfrk_msp_plan_groups(ctx, nN, msp_need, have, &groups))) return rc;
  if (groups == 0) return cfrk_fail(ctx, CFRK_ERR_NOMEM, "partitioned path does not fit device memory");
  const int passes = groups;
  ctx->last_passes = passes;
  if (ctx->g_flags & CFRK_RUNS_ONLY) {
    if (ms->runs_ready) return cfrk_fail(ctx, CFRK_ERR_STATE, "a CFRK_RUNS_ONLY job takes one add");
    if (passes != 1) return cfrk_fail(ctx, CFRK_ERR_RUNS_REFUSED, "a CFRK_RUNS_ONLY job must fit device memory in one pass");
  }
  if (ms->pending && (rc = cfrk_msp_flush_to_table(ctx))) return rc;
  int W0, m0;
  msp_params(ctx->g_k, &W0, &m0);
  const double l2 = (double)nN * (2.0 / (W0 + 1) + 1.0 / 64.0) * 2.7 * 16;      // bytes of the leaf streams
  return msp_for_each_pass(ctx, passes, true, have, msp_need(ctx, nN), l2, [&](double slack, int sel_bits, uint32_t sel_val, bool first) {
    return msp_count_tiles(ctx, ms, d_data, nN, 0, ntiles, slack, sel_bits, sel_val, first);
  });
}

int cfrk_msp_sync_stats(cfrk_ctx *ctx, uint64_t st[ST_NWORDS]) {
  HIP_TRY(ctx, hipMemcpyAsync(st, ctx->g_stats, ST_NWORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CFRK_OK;
}

int cfrk_msp_flush_to_table(cfrk_ctx *ctx) {
  cfrk_msp *ms = ctx->msp;
  if (!ms || !ms->pending) return CFRK_OK;
  uint64_t st[ST_NWORDS];
  int rc = cfrk_msp_sync_stats(ctx, st);
  if (rc) return rc;
  if (st[ST_OVERFLOW]) return cfrk_fail(ctx, CFRK_ERR_TABLE_FULL, "result list of %llu entries overflowed", (unsigned long long)ms->view.out_cap);
  const uint64_t n = st[ST_CURSOR];
  ms->pending = false;
  ms->table_dirty = true;
  if (n == 0) return CFRK_OK;
  return cfrk_hash_merge(ctx, ms->view.out_keys, ctx->g_two ? ms->view.out_hi : nullptr, ms->view.out_cnt, (int64_t)n);
}

int cfrk_msp_resolve(cfrk_ctx *ctx, ResultSrc *src, bool *use_list) {
  *use_list = false;
  if (ctx->g_flags & CFRK_RUNS_ONLY)
    return cfrk_fail(ctx, CFRK_ERR_STATE, "a CFRK_RUNS_ONLY job holds runs, not counts: cfrk_global_export_runs_device");
  cfrk_msp *ms = ctx->msp;
  if (!ms || !ms->pending) return CFRK_OK;
  uint64_t st[ST_NWORDS];
  int rc = cfrk_msp_sync_stats(ctx, st);
  if (rc) return rc;
  if (st[ST_OVERFLOW]) return cfrk_fail(ctx, CFRK_ERR_TABLE_FULL, "result list of %llu entries overflowed", (unsigned long long)ms->view.out_cap);
  if (st[ST_SPILLED] || ms->table_dirty) return cfrk_msp_flush_to_table(ctx);
  src->lo = ms->view.out_keys; src->hi = ctx->g_two ? ms->view.out_hi : nullptr; src->cnt = ms->view.out_cnt;
  src->n = st[ST_CURSOR]; src->kind = ctx->g_two ? 3 : 2; src->stats = ctx->g_stats;
  *use_list = true;
  return CFRK_OK;
}

extern "C" int cfrk_debug_device_bytes(cfrk_ctx *ctx, uint64_t *out_bytes) {
  if (!ctx || !out_bytes) return CFRK_ERR_ARG;
  uint64_t n = 0;
  for (int i = 0; i < BUF_NSLOTS; ++i) n += ctx->pool[i].cap;
  if (ctx->g_keys_lo) n += ctx->g_cap * 8;
  if (ctx->g_keys_hi) n += ctx->g_cap * 8;
  if (ctx->g_counts) n += ctx->g_cap * 4;
  *out_bytes = n;
  return CFRK_OK;
}

extern "C" int cfrk_debug_set_mem_budget(cfrk_ctx *ctx, uint64_t bytes) {
  if (!ctx) return CFRK_ERR_ARG;
  ctx->mem_budget = (size_t)bytes;
  return CFRK_OK;
}

extern "C" int cfrk_debug_set_param(cfrk_ctx *ctx, int which, double value) {
  if (!ctx) return CFRK_ERR_ARG;
  if (which < 0 || which >= 5 || !(value >= 0)) return cfrk_fail(ctx, CFRK_ERR_ARG, "cfrk_debug_set_param: no such parameter / negative value");
  if (value != 0) {
    if (which == CFRK_PARAM_MSP_CHUNKS && !(value >= 1 && value <= 4096)) return cfrk_fail(ctx, CFRK_ERR_ARG, "chunks: 1 .. 4096");
    if ((which == CFRK_PARAM_L2_SLACK_COMPLETE || which == CFRK_PARAM_L2_SLACK_TRUNCATED) && !(value >= 1.0 && value <= 16.0))
      return cfrk_fail(ctx, CFRK_ERR_ARG, "leaf-stream slack: 1 .. 16");
    if (which == CFRK_PARAM_MSP2_SUBVALUE_BITS && !(value >= 1 && value <= 3)) return cfrk_fail(ctx, CFRK_ERR_ARG, "sub-value bits + 1: 1 .. 3");
    if (which == CFRK_PARAM_UNITIG_SPLIT_LOG2 && !(value >= 1 && value <= 20)) return cfrk_fail(ctx, CFRK_ERR_ARG, "unitig splitter bits + 1: 1 .. 20");
  }
  ctx->dbg_param[which] = value;
  return CFRK_OK;
}
extern "C" int cfrk_debug_set_flags(cfrk_ctx *ctx, uint32_t flags) {
  if (!ctx) return CFRK_ERR_ARG;
  // (the timing ablations of msp.h exist in an ablation build only: in the product they are refused, not ignored)
  if (flags & ~CFRK_DEBUG_KNOWN_BITS) return cfrk_fail(ctx, CFRK_ERR_ARG, "cfrk_debug_set_flags: unknown bits 0x%x", flags & ~CFRK_DEBUG_KNOWN_BITS);
  ctx->dbg_flags = flags;
  return CFRK_OK;
}

#ifdef CFRK_ABLATIONS
// ablation build only (tools/p3_paths.py): the leaf kernel's path counters since the last reset, out[0 .. n) in the
// order of P3C_*, of the current device; synchronises it (no context: the counters outlive the ones that counted)
extern "C" int cfrk_debug_p3_paths(uint64_t *out, int n, int reset) {
  if (!out || n < 0 || n > P3C_N) return CFRK_ERR_ARG;
  unsigned long long h[P3C_N] = {};
  if (hipDeviceSynchronize() != hipSuccess) return CFRK_ERR_HIP;
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(p3_paths), sizeof(h)) != hipSuccess) return CFRK_ERR_HIP;
  for (int i = 0; i < n; ++i) out[i] = h[i];
  if (reset) {
    const unsigned long long z[P3C_N] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(p3_paths), z, sizeof(z)) != hipSuccess) return CFRK_ERR_HIP;
  }
  return CFRK_OK;
}
#endif

extern "C" int cfrk_debug_last_add_passes(cfrk_ctx *ctx, int *out_passes) {
  if (!ctx || !out_passes) return CFRK_ERR_ARG;
  *out_passes = ctx->last_passes;
  return CFRK_OK;
}

// diagnostics (not part of the counting path): out[0..5] = L1 records total / max bin / bin
// capacity, L2 records total / max leaf / leaf capacity; out[6] = records spilled to the HBM
// table, out[7] = k-mers spilled by full leaf tables, out[8] = entries in the result list
extern "C" int cfrk_debug_msp_info(cfrk_ctx *ctx, uint64_t out[9]) {
  if (!ctx || !out) return CFRK_ERR_ARG;
  cfrk_msp *ms = ctx->msp;
  for (int i = 0; i < 9; ++i) out[i] = 0;
  if (!ms) return CFRK_OK;
  int rc;
  if (ms->view.cnt1) {                                   // (the two-word path keeps no view of its record levels)
    void *p;
    if ((rc = cfrk_pool_get(ctx, BUF_SCRATCH, 64 * sizeof(uint64_t), &p))) return rc;
    hipLaunchKernelGGL(msp_info_kernel, dim3(1), dim3(1024), 0, ctx->stream, ms->view, (uint64_t *)p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out, p, 6 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  }
  uint64_t st[ST_NWORDS];
  rc = cfrk_msp_sync_stats(ctx, st);
  if (rc) return rc;
  out[6] = st[ST_AUX0]; out[7] = st[ST_AUX1]; out[8] = st[ST_CURSOR];
  return CFRK_OK;
}

// ------------------------------------------------------------------ multi-GPU exchange by leaf
extern "C" int cfrk_global_export_leaves_device(cfrk_ctx *ctx, uint64_t *d_keys, uint64_t *d_keys_hi,
                                                uint32_t *d_counts, uint64_t cap, int parts,
                                                uint64_t *part_counts, uint32_t *d_leaf_counts) {
  if (!ctx || !part_counts || parts < 1 || parts > NLEAF) return CFRK_ERR_ARG;
  if (ctx->g_active && ctx->g_two && !d_keys_hi && cap) return cfrk_fail(ctx, CFRK_ERR_ARG, "two-word keys need d_keys_hi");
  cfrk_msp *ms = ctx->msp;
  if (!ctx->g_active || !ms || !ms->pending || !ms->leaf_form || ms->table_dirty)
    return cfrk_fail(ctx, CFRK_ERR_STATE, "result is not in per-leaf list form");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint64_t st[ST_NWORDS];
  int rc = cfrk_msp_sync_stats(ctx, st);
  if (rc) return rc;
  if (st[ST_OVERFLOW]) return cfrk_fail(ctx, CFRK_ERR_TABLE_FULL, "result list overflowed");
  if (st[ST_SPILLED] || st[ST_ONES]) return cfrk_fail(ctx, CFRK_ERR_STATE, "part of the result lives in the HBM table");
  if (st[ST_MULTISEG]) return cfrk_fail(ctx, CFRK_ERR_STATE, "leaves were counted in several passes: no per-leaf index");
  const int lpp = (NLEAF + parts - 1) / parts;           // leaves per part (owner p: leaves p, p+parts, ...)
  std::vector<uint32_t> ln(NLEAF), ordered((size_t)parts * lpp, 0u);
  std::vector<uint64_t> doff(NLEAF);
  const uint32_t sgb = ms->view.seg_bits;
  if (sgb == 0) {
    HIP_TRY(ctx, hipMemcpyAsync(ln.data(), ms->view.leaf_n, NLEAF * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  } else {
    // a leaf shared by record: its entries sit in 2^seg_bits segments (one per sub-value)
    std::vector<uint32_t> sn((size_t)NLEAF << sgb);
    HIP_TRY(ctx, hipMemcpyAsync(sn.data(), ms->view.leaf_n, sn.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t l = 0; l < (size_t)NLEAF; ++l) {
      uint32_t t = 0;
      for (uint32_t j = 0; j < (1u << sgb); ++j) t += sn[(l << sgb) | j];
      ln[l] = t;
    }
  }
  uint64_t run = 0;
  for (int p = 0; p < parts; ++p) {
    uint64_t pc = 0;
    for (int j = 0; j < lpp; ++j) {
      const int leaf = p + j * parts;
      if (leaf >= NLEAF) break;
      doff[leaf] = run;
      run += ln[leaf]; pc += ln[leaf];
      ordered[(size_t)p * lpp + j] = ln[leaf];
    }
    part_counts[p] = pc;
  }
  if (run != st[ST_CURSOR]) return cfrk_fail(ctx, CFRK_ERR_STATE, "leaf index does not cover the list");
  if (run > cap) return cfrk_fail(ctx, CFRK_ERR_SMALL_BUF, "%llu entries, room for %llu", (unsigned long long)run, (unsigned long long)cap);
  void *p;
  if ((rc = cfrk_pool_get(ctx, BUF_SCRATCH, NLEAF * sizeof(uint64_t), &p))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(p, doff.data(), NLEAF * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
  if (d_leaf_counts)
    HIP_TRY(ctx, hipMemcpyAsync(d_leaf_counts, ordered.data(), ordered.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  if (run) {
    hipLaunchKernelGGL(msp_gather_kernel, dim3(NLEAF), dim3(256), 0, ctx->stream, ms->view, (const uint64_t *)p, d_keys,
                       ctx->g_two ? d_keys_hi : (uint64_t *)nullptr, d_counts);
    HIP_TRY(ctx, hipGetLastError());
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // doff / ordered are host temporaries
  return CFRK_OK;
}

extern "C" int cfrk_global_leaves_per_part(int parts) { return parts >= 1 ? (NLEAF + parts - 1) / parts : 0; }

extern "C" int cfrk_global_merge_leaves_device(cfrk_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_keys_hi,
                                               const uint32_t *d_counts, const uint64_t *recv_counts,
                                               const uint32_t *d_leaf_counts, int parts) {
  if (!ctx || parts < 1 || parts > NLEAF || !recv_counts || !d_leaf_counts) return CFRK_ERR_ARG;
  if (!ctx->g_active) return cfrk_fail(ctx, CFRK_ERR_STATE, "merge_leaves needs an active job");
  ctx->q_valid = false;
  if (ctx->g_two && !d_keys_hi) return cfrk_fail(ctx, CFRK_ERR_ARG, "two-word keys need d_keys_hi");
  cfrk_msp *ms = cfrk_msp_get(ctx);
  if (!ms) return cfrk_fail(ctx, CFRK_ERR_NOMEM, "host allocation failed");
  if (ms->pending || ms->table_dirty) return cfrk_fail(ctx, CFRK_ERR_STATE, "merge_leaves needs an empty job (call cfrk_global_begin first)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int lpp = (NLEAF + parts - 1) / parts;
  int rc;
  void *p;
  MspView &v = ms->view;
  if ((rc = cfrk_pool_get(ctx, BUF_MSP_OUTK, (size_t)ctx->g_cap * 8, &p))) return rc;
  v.out_keys = (uint64_t *)p;
  if (ctx->g_two) {
    if ((rc = cfrk_pool_get(ctx, BUF_MSP_OUTH, (size_t)ctx->g_cap * 8, &p))) return rc;
    v.out_hi = (uint64_t *)p;
  }
  if ((rc = cfrk_pool_get(ctx, BUF_MSP_OUTC, (size_t)ctx->g_cap * 4, &p))) return rc;
  v.out_cnt = (uint32_t *)p; v.out_cap = ctx->g_cap;
  v.stats = ctx->g_stats;
  // segment (source rank, local leaf): counts arrive as [parts][lpp]; data as rank-major runs
  const size_t nseg = (size_t)parts * lpp;
  std::vector<uint32_t> sn(nseg);
  std::vector<uint64_t> so(nseg);
  HIP_TRY(ctx, hipMemcpyAsync(sn.data(), d_leaf_counts, nseg * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t run = 0;
  for (int r = 0; r < parts; ++r) {
    uint64_t got = 0;
    for (int j = 0; j < lpp; ++j) { so[(size_t)r * lpp + j] = run; run += sn[(size_t)r * lpp + j]; got += sn[(size_t)r * lpp + j]; }
    if (got != recv_counts[r]) return cfrk_fail(ctx, CFRK_ERR_ARG, "rank %d sent %llu entries but its leaf counts add up to %llu", r, (unsigned long long)recv_counts[r], (unsigned long long)got);
  }
  if ((rc = cfrk_pool_get(ctx, BUF_SCRATCH, nseg * (sizeof(uint64_t) + sizeof(uint32_t)), &p))) return rc;
  uint64_t *d_so = (uint64_t *)p;
  uint32_t *d_sn = (uint32_t *)(d_so + nseg);
  HIP_TRY(ctx, hipMemcpyAsync(d_so, so.data(), nseg * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_sn, sn.data(), nseg * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(ctx->g_stats + ST_CURSOR, 0, sizeof(uint64_t), ctx->stream));
  TableView t = cfrk_table_view(ctx);
  if (run && ctx->g_two) {
    if ((rc = cfrk_msp2_merge_lists(ctx, d_keys, d_keys_hi, d_counts, d_so, d_sn, parts, lpp))) return rc;
  } else if (run) {
    hipLaunchKernelGGL(msp_merge_kernel, dim3(lpp), dim3(P3_THREADS), 0, ctx->stream, d_keys, d_counts,
                       (const uint64_t *)d_so, (const uint32_t *)d_sn, parts, lpp, v, t);
    HIP_TRY(ctx, hipGetLastError());
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // so / sn are host temporaries
  ctx->h_stats_valid = false;                          // this kernel may have spilled into the table
  ms->pending = true;
  ms->leaf_form = false;
  ms->list_n_valid = false;
  return CFRK_OK;
}

// ------------------------------------------------------------------ multi-GPU exchange by runs

extern "C" int cfrk_global_export_runs_device(cfrk_ctx *ctx, void *d_packed, uint64_t cap_rows, int parts,
                                              uint64_t *part_rows) {
  if (!ctx || !part_rows || parts < 1 || parts > 64) return CFRK_ERR_ARG;
  cfrk_msp *ms = ctx->msp;
  if (!ctx->g_active || !ms || !ms->runs_ready)
    return cfrk_fail(ctx, CFRK_ERR_STATE, "no deduplicated runs to export (begin with CFRK_RUNS_ONLY, then one add)");
  if (!d_packed) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (ctx->g_two) return cfrk_msp2_export_runs(ctx, d_packed, cap_rows, parts, part_rows);
  const MspView &v = ms->view;
  int rc;
  if ((rc = runs_check_deferred(ctx, ms))) return rc;
  if (!ms->runs_deduped) {
    hipLaunchKernelGGL(msp_dedupe_export_kernel, dim3(NLEAF), dim3(DX_THREADS), 0, ctx->stream, ctx->g_k, (ctx->g_flags & CFRK_CANONICAL) ? 1 : 0, v);
    HIP_TRY(ctx, hipGetLastError());
    ms->runs_deduped = true;
  }
  return runs_export_host(ctx, cap_rows, parts, part_rows,
    [&](uint4 *d_sz, unsigned long long *d_sync) {
      hipLaunchKernelGGL(msp_runs_sizes_kernel, dim3(NLEAF / 256), dim3(256), 0, ctx->stream, v, d_sz, d_sync);
    },
    [&](const uint64_t *d_off, const uint64_t *d_rows, const uint64_t *d_seg) {
      hipLaunchKernelGGL(msp_runs_gather_kernel, dim3(NLEAF), dim3(256), 0, ctx->stream, v, d_off, (uint4 *)d_packed, d_rows, d_seg, parts, cap_rows);
    });
}

extern "C" int cfrk_global_merge_runs_device(cfrk_ctx *ctx, const void *d_packed, const uint64_t *recv_rows, int parts) {
  if (!ctx || parts < 1 || parts > 64 || !recv_rows || !d_packed) return CFRK_ERR_ARG;
  if (!ctx->g_active) return cfrk_fail(ctx, CFRK_ERR_STATE, "merge_runs needs an active job");
  ctx->q_valid = false;
  if (cfrk_msp2_usable(ctx) && !(ctx->g_flags & CFRK_RUNS_ONLY)) return cfrk_msp2_merge_runs(ctx, d_packed, recv_rows, parts);
  if (!cfrk_msp_usable(ctx) || (ctx->g_flags & CFRK_RUNS_ONLY)) return cfrk_fail(ctx, CFRK_ERR_ARG, "merge_runs needs a counting job with 16 <= k <= 64");
  cfrk_msp *ms = cfrk_msp_get(ctx);
  if (!ms) return cfrk_fail(ctx, CFRK_ERR_NOMEM, "host allocation failed");
  if (ms->pending || ms->table_dirty) return cfrk_fail(ctx, CFRK_ERR_STATE, "merge_runs needs an empty job (call cfrk_global_begin first)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  const int k = ctx->g_k;
  const int canon = (ctx->g_flags & CFRK_CANONICAL) ? 1 : 0;
  int rc;
  MspView &v = ms->view;
  RunsPlan pl;
  // (one stream of complete and one of truncated runs per leaf, a record a row)
  if ((rc = runs_merge_plan_host<NCLS, 1, 0, 1>(ctx, d_packed, recv_rows, parts, [&](uint64_t **lbase, uint32_t **lcap, uint32_t **cnt2) -> int {
        int rc2;
        void *p;
        memset(&v, 0, sizeof v);
        v.nxg = NXG;
        if ((rc2 = msp_aux_buffers(ctx, v, (size_t)NLEAF, NXG, (size_t)NCLS * NLEAF))) return rc2;
        if ((rc2 = cfrk_pool_get(ctx, BUF_MSP_LAYOUT, (size_t)NCLS * NLEAF * (sizeof(uint64_t) + sizeof(uint32_t)), &p))) return rc2;
        *lbase = (uint64_t *)p; *lcap = (uint32_t *)(*lbase + NCLS * NLEAF);
        v.exact = 1; v.lbase = *lbase; v.lcap = *lcap;
        if ((rc2 = cfrk_pool_get(ctx, BUF_MSP_OUTK, (size_t)ctx->g_cap * 8, &p))) return rc2;
        v.out_keys = (uint64_t *)p;
        if ((rc2 = cfrk_pool_get(ctx, BUF_MSP_OUTC, (size_t)ctx->g_cap * 4, &p))) return rc2;
        v.out_cnt = (uint32_t *)p; v.out_cap = ctx->g_cap;
        v.stats = ctx->g_stats; v.dbg = ctx->dbg_flags;
        *cnt2 = v.cnt2;
        return CFRK_OK;
      }, &pl, &v.rec2))) return rc;
  const int lpp = pl.lpp;
  TableView t = cfrk_table_view(ctx);
  hipLaunchKernelGGL(msp_runs_scatter_kernel, dim3((unsigned)pl.nseg), dim3(256), 0, ctx->stream, (const uint4 *)d_packed, pl.rr, lpp, k,
                     pl.src, pl.d1, pl.d0, v.rec2);
  HIP_TRY(ctx, hipGetLastError());
  if (canon) hipLaunchKernelGGL((msp_p3_kernel<true, false>), dim3(lpp), dim3(P3_THREADS), 0, ctx->stream, k, P3_WEIGHTED, v, t);
  else hipLaunchKernelGGL((msp_p3_kernel<false, false>), dim3(lpp), dim3(P3_THREADS), 0, ctx->stream, k, P3_WEIGHTED, v, t);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(msp_huge_leaves_kernel, dim3(((unsigned)lpp + 255u) / 256u), dim3(256), 0, ctx->stream, k, canon, 1, (uint32_t)lpp, v, t);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  ctx->ev_valid = true;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->h_stats_valid = false;                          // the leaf kernel may have spilled into the table
  ms->pending = true;
  ms->leaf_form = false;
  ms->list_n_valid = false;
  return CFRK_OK;
}

// ------------------------------------------------------------------ multi-GPU exchange by runs, pipelined

extern "C" int cfrk_global_export_runs_async(cfrk_ctx *ctx, void *d_packed, uint64_t seg_cap_rows, int parts, int ngroups) {
  if (!ctx || parts < 1 || parts > 64 || ngroups < 1 || ngroups > CFRK_RUNS_MAX_GROUPS) return CFRK_ERR_ARG;
  cfrk_msp *ms = ctx->msp;
  if (!ctx->g_active || !ms || !ms->runs_ready)
    return cfrk_fail(ctx, CFRK_ERR_STATE, "no runs to export (begin with CFRK_RUNS_ONLY, then one add)");
  if (ms->runs_deduped) return cfrk_fail(ctx, CFRK_ERR_STATE, "the leaf streams were deduplicated in place already (add with CFRK_RUNS_DEFER for the pipelined export)");
  if (!d_packed) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  if (ctx->g_two) return cfrk_msp2_export_runs_async(ctx, d_packed, seg_cap_rows, parts, ngroups);
  const MspView &v = ms->view;
  const int k = ctx->g_k, canon = (ctx->g_flags & CFRK_CANONICAL) ? 1 : 0;
  return runs_export_async_host(ctx, d_packed, seg_cap_rows, parts, ngroups, [&](const RunsSend &sg) {
    hipLaunchKernelGGL(msp_dedupe_send_kernel, dim3(sg.nleaf), dim3(DS_THREADS), 0, ctx->stream, k, canon, v, sg);
  });
}

extern "C" int cfrk_global_export_runs_wait(cfrk_ctx *ctx, int group, uint64_t *part_rows) {
  if (!ctx || !part_rows) return CFRK_ERR_ARG;
  if (group < 0 || group >= ctx->runs_groups || !ctx->h_runs) return cfrk_fail(ctx, CFRK_ERR_STATE, "no such group in flight (cfrk_global_export_runs_async first)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipEventSynchronize(ctx->runs_ev[group]));
  const uint64_t *u = ctx->h_runs + (size_t)group * 65;
  const int parts = ctx->runs_parts;
  if (u[parts]) return cfrk_fail(ctx, CFRK_ERR_STATE, "the add overflowed a record region or spilled: the shard's runs are not all in the leaf streams");
  if (ctx->msp) ctx->msp->runs_unchecked = false;      // (the flags were clean when this group finished: the add held)
  for (int q = 0; q < parts; ++q)
    if (u[q] > ctx->runs_seg_cap) return cfrk_fail(ctx, CFRK_ERR_SMALL_BUF, "segment (group %d, owner %d) needs more than %llu rows", group, q, (unsigned long long)ctx->runs_seg_cap);
  for (int q = 0; q < parts; ++q) part_rows[q] = u[q];
  return CFRK_OK;
}

extern "C" int cfrk_global_merge_runs_group_device(cfrk_ctx *ctx, const void *d_recv, const uint64_t *recv_rows, int parts, int group, int ngroups) {
  if (!ctx || parts < 1 || parts > 64 || !recv_rows || !d_recv || ngroups < 1 || ngroups > CFRK_RUNS_MAX_GROUPS || group < 0 || group >= ngroups) return CFRK_ERR_ARG;
  if (!ctx->g_active) return cfrk_fail(ctx, CFRK_ERR_STATE, "merge_runs_group needs an active job");
  ctx->q_valid = false;
  if (ctx->g_two && !(ctx->g_flags & (CFRK_RUNS_ONLY | CFRK_FORCE_HASH))) return cfrk_msp2_merge_runs_group(ctx, d_recv, recv_rows, parts, group, ngroups);
  if (!cfrk_msp_usable(ctx) || (ctx->g_flags & CFRK_RUNS_ONLY)) return cfrk_fail(ctx, CFRK_ERR_ARG, "merge_runs_group needs a counting job with 16 <= k <= 64");
  cfrk_msp *ms = cfrk_msp_get(ctx);
  if (!ms) return cfrk_fail(ctx, CFRK_ERR_NOMEM, "host allocation failed");
  if (group != ms->lists_group) return cfrk_fail(ctx, CFRK_ERR_STATE, "groups are merged in order: expected group %d", ms->lists_group);
  if (group == 0 && (ms->pending || ms->table_dirty)) return cfrk_fail(ctx, CFRK_ERR_STATE, "merge_runs_group needs an empty job (call cfrk_global_begin first)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int lpp = (NLEAF + parts - 1) / parts;
  if (ngroups > lpp) return cfrk_fail(ctx, CFRK_ERR_ARG, "more groups than leaves per owner");
  int rc;
  void *p;
  MspView &v = ms->view;
  if (group == 0) {
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    memset(&v, 0, sizeof v);
    if ((rc = cfrk_pool_get(ctx, BUF_MSP_OUTK, (size_t)ctx->g_cap * 8, &p))) return rc;
    v.out_keys = (uint64_t *)p;
    if ((rc = cfrk_pool_get(ctx, BUF_MSP_OUTC, (size_t)ctx->g_cap * 4, &p))) return rc;
    v.out_cnt = (uint32_t *)p; v.out_cap = ctx->g_cap;
    v.stats = ctx->g_stats; v.dbg = ctx->dbg_flags;
    HIP_TRY(ctx, hipMemsetAsync(ctx->g_stats + ST_CURSOR, 0, sizeof(uint64_t), ctx->stream));
  }
  const P3ListsT<true> lx = runs_group_lists(d_recv, recv_rows, parts, group, ngroups);
  TableView t = cfrk_table_view(ctx);
  if (lx.lcount) {
    if (ctx->g_flags & CFRK_CANONICAL) hipLaunchKernelGGL((msp_p3_lists_kernel<true>), dim3(lx.lcount), dim3(P3_THREADS), 0, ctx->stream, ctx->g_k, v, t, lx);
    else hipLaunchKernelGGL((msp_p3_lists_kernel<false>), dim3(lx.lcount), dim3(P3_THREADS), 0, ctx->stream, ctx->g_k, v, t, lx);
    HIP_TRY(ctx, hipGetLastError());
  }
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  ctx->ev_valid = true;
  ctx->h_stats_valid = false;                          // the leaf kernel may have spilled into the table
  ms->lists_group = group + 1;
  ms->pending = true;
  ms->leaf_form = false;
  ms->list_n_valid = false;
  return CFRK_OK;
}

// Device time (ms) from the start of the job's add (its first kernel) to the end of group `group` of the pipelined export
// (HIP events on the context stream): the rehearsal tool's clock (tools/scale_emul.py).  Synchronises on that group.
extern "C" int cfrk_global_runs_group_ms(cfrk_ctx *ctx, int group, float *ms) {
  if (!ctx || !ms) return CFRK_ERR_ARG;
  if (group < 0 || group >= ctx->runs_groups || !ctx->ev_valid) return cfrk_fail(ctx, CFRK_ERR_STATE, "no such group in flight");
  HIP_TRY(ctx, hipEventSynchronize(ctx->runs_ev[group]));
  HIP_TRY(ctx, hipEventElapsedTime(ms, ctx->ev0, ctx->runs_ev[group]));
  return CFRK_OK;
}
