// query_dev.h -- the lookup index of a finished global result as the kernels see it: the index descriptor, the slot
// hashes, the probe loops and the canonical form of a two-word key.  Shared by query.hip (which also builds the index),
// read_stats.hip, read_filter.hip and (the window extraction and the key hashes) sketch.hip; the index layout is described at the top of query.hip.
#pragma once

#include "common.h"

struct QIndex {
  const void *p;
  uint64_t mask;
  int shift;                          // 64 - log2(slots)
  int k;
};

// query.hip: the index of the job's current result, built (synchronising) when it is not valid
int cfrk_query_index(cfrk_ctx *ctx, QIndex *q);

#ifdef __HIPCC__
namespace {

constexpr int QB = 8;                 // windows per lane whose first-slot loads are in flight together

__host__ __device__ __forceinline__ uint64_t q_slot1(uint64_t lo, int shift) { return dev_mix64(lo) >> shift; }
__host__ __device__ __forceinline__ uint64_t q_slot2(uint64_t lo, uint64_t hi, int shift) { return dev_mix64(lo ^ dev_mix64(hi)) >> shift; }
__device__ __forceinline__ uint64_t q_lo(uint4 v) { return ((uint64_t)v.y << 32) | v.x; }
__device__ __forceinline__ uint64_t q_hi(uint4 v) { return ((uint64_t)v.w << 32) | v.z; }

// probe from slot h on; 0 when the key is absent (load <= 0.5: an empty slot ends every probe sequence)
__device__ __forceinline__ uint32_t q_find1(const uint4 *__restrict__ s, uint64_t mask, uint64_t h, uint64_t key) {
  for (uint64_t probe = 0; probe <= mask; ++probe) {
    const uint4 v = s[h];
    if (v.z == 0) return 0;
    if (q_lo(v) == key) return v.z;
    h = (h + 1) & mask;
  }
  return 0;
}
__device__ __forceinline__ uint32_t q_find2(const uint4 *__restrict__ s, uint64_t mask, uint64_t h, uint64_t lo,
                                            uint64_t hi) {
  for (uint64_t probe = 0; probe <= mask; ++probe) {
    const uint4 a = s[2 * h], b = s[2 * h + 1];
    if (b.x == 0) return 0;
    if (q_lo(a) == lo && q_hi(a) == hi) return b.x;
    h = (h + 1) & mask;
  }
  return 0;
}

// The same probes returning the SLOT of the key, Q_NO_SLOT when it is absent: what a kernel needs that keeps data of
// its own beside the index, in arrays indexed by slot (unitigs.hip).
constexpr uint64_t Q_NO_SLOT = ~0ull;
__device__ __forceinline__ uint64_t q_find1_slot(const uint4 *__restrict__ s, uint64_t mask, uint64_t h, uint64_t key) {
  for (uint64_t probe = 0; probe <= mask; ++probe) {
    const uint4 v = s[h];
    if (v.z == 0) return Q_NO_SLOT;
    if (q_lo(v) == key) return h;
    h = (h + 1) & mask;
  }
  return Q_NO_SLOT;
}
__device__ __forceinline__ uint64_t q_find2_slot(const uint4 *__restrict__ s, uint64_t mask, uint64_t h, uint64_t lo,
                                                 uint64_t hi) {
  for (uint64_t probe = 0; probe <= mask; ++probe) {
    const uint4 a = s[2 * h], b = s[2 * h + 1];
    if (b.x == 0) return Q_NO_SLOT;
    if (q_lo(a) == lo && q_hi(a) == hi) return h;
    h = (h + 1) & mask;
  }
  return Q_NO_SLOT;
}

// window i (bases i .. i+k-1 of the 64-base string hi:lo) as a key, canonical when asked
template <bool CANON>
__device__ __forceinline__ uint64_t q_window(uint64_t hi, uint64_t lo, int i, int k) {
  const uint64_t x = i ? ((hi << (2 * i)) | (lo >> (64 - 2 * i))) : hi;
  uint64_t key = x >> (64 - 2 * k);
  if (CANON) { const uint64_t rc = dev_revcomp64(key, k); key = rc < key ? rc : key; }
  return key;
}

// canonical form of a two-word key (2k bits, first base most significant): min with its 128-bit reverse complement
__device__ __forceinline__ void q_canon2(uint64_t &lo, uint64_t &hi, int k) {
  const uint64_t rhi = dev_revcomp64(lo, 32), rlo = dev_revcomp64(hi, 32);   // all 64 bases, reversed + complemented
  const int s = 128 - 2 * k;                                                  // 0 .. 62: the k-mer's complement on top
  const uint64_t clo = s ? (rlo >> s) | (rhi << (64 - s)) : rlo;
  const uint64_t chi = s ? rhi >> s : rhi;
  if (chi < hi || (chi == hi && clo < lo)) { lo = clo; hi = chi; }
}

// MODE 0: dense (k <= 12), 1: one-word hash (k <= 32), 2: two-word hash (k > 32)
template <int MODE, bool CANON>
__device__ __forceinline__ uint32_t q_key(const QIndex &q, uint64_t lo, uint64_t hi) {
  const int k = q.k;
  if (MODE < 2) {
    if (hi != 0 || (k < 32 && (lo >> (2 * k)) != 0)) return 0;      // bits at or above 2k: no such k-mer
    if (CANON) { const uint64_t rc = dev_revcomp64(lo, k); lo = rc < lo ? rc : lo; }
    if (MODE == 0) return static_cast<const uint32_t *>(q.p)[lo];
    return q_find1(static_cast<const uint4 *>(q.p), q.mask, q_slot1(lo, q.shift), lo);
  }
  if (k < 64 && (hi >> (2 * k - 64)) != 0) return 0;
  if (CANON) q_canon2(lo, hi, k);
  return q_find2(static_cast<const uint4 *>(q.p), q.mask, q_slot2(lo, hi, q.shift), lo, hi);
}

// The index by slot.  Slots: 4^k (MODE 0, the slot is the key), else mask + 1.  q_slot_of takes a key as the index
// stores it (in range, canonical in a canonical job); the slot of an absent key is Q_NO_SLOT in every mode.
template <int MODE>
__device__ __forceinline__ uint64_t q_nslots(const QIndex &q) { return MODE == 0 ? 1ull << (2 * q.k) : q.mask + 1; }
template <int MODE>
__device__ __forceinline__ uint32_t q_slot_count(const QIndex &q, uint64_t slot) {
  if (MODE == 0) return static_cast<const uint32_t *>(q.p)[slot];
  if (MODE == 1) return static_cast<const uint4 *>(q.p)[slot].z;
  return static_cast<const uint4 *>(q.p)[2 * slot + 1].x;
}
template <int MODE>
__device__ __forceinline__ void q_slot_key(const QIndex &q, uint64_t slot, uint64_t &lo, uint64_t &hi) {
  hi = 0;
  if (MODE == 0) { lo = slot; return; }
  const uint4 v = static_cast<const uint4 *>(q.p)[MODE == 1 ? slot : 2 * slot];
  lo = q_lo(v);
  if (MODE == 2) hi = q_hi(v);
}
template <int MODE>
__device__ __forceinline__ uint64_t q_slot_of(const QIndex &q, uint64_t lo, uint64_t hi) {
  if (MODE == 0) return static_cast<const uint32_t *>(q.p)[lo] ? lo : Q_NO_SLOT;
  if (MODE == 1) return q_find1_slot(static_cast<const uint4 *>(q.p), q.mask, q_slot1(lo, q.shift), lo);
  return q_find2_slot(static_cast<const uint4 *>(q.p), q.mask, q_slot2(lo, hi, q.shift), lo, hi);
}

}  // namespace
#endif  // __HIPCC__
