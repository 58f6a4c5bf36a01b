// unitigs.hip -- the compacted de Bruijn graph of a finished global result: neighbour masks and unitigs (the maximal
// non-branching paths of the solid k-mers) with their abundances, as struct reads.  The contract is in
// include/cfrk_abi.h ("unitigs"); DESIGN 4.19 has the reasoning.
//
// Everything is answered from the lookup index of query.hip, which is not modified.  Beside it the call keeps arrays
// indexed by index SLOT (k <= 12: the slot is the key): a node is a slot, an ORIENTED node is v = 2 * slot + o, o = 1
// the reverse complement of the stored key (canonical jobs only).  One byte of neighbour bits per slot serves both
// orientations (u_mirror), and so do the link bits: the link a -> b exists iff rc(b) -> rc(a) does.
//
// Stages, each a launch of its own on the context stream (a later one reads what an earlier one wrote):
//   1 adjacency   one lane per slot: the 8 neighbour lookups of a solid key -> adj[slot]
//   2 links       one lane per solid slot: a link needs a unique neighbour and, from that neighbour's byte, a unique way
//                 back; no link into the own slot (self-loops, hairpins), none at a palindrome.  A node is a SPLITTER iff
//                 the low s bits of its key's hash are 0; the link on a splitter's predecessor side (stored orientation)
//                 is CUT -- which the mirror link then is as well, by construction (u_link_kernel).
//   3 segments    heads = oriented nodes without an uncut in-link, appended to a list; one lane per head walks the uncut
//                 links to the segment's tail: n, kc, the smallest oriented k-mer and where it lies; nodes are marked.
//   4 stitch      one lane per segment whose head has no in-link at all (a unitig's head) hops from segment to segment
//                 over the cut links, decides the winner of path and mirror (a1 < rc(an)), appends the unitig and, as
//                 the winner, hops again to give every segment its unitig and its offset in it.
//   5 cycles      (a) segments no hop marked lie on rings of segments: each walks its ring at segment level; the one that
//                 holds the ring's smallest k-mer leads, and wins iff that k-mer is smaller than the mirror ring's.
//                 (b) solid nodes no segment walk marked lie on rings without a splitter (short: a ring of n nodes has
//                 none with probability (1 - 2^-s)^n): each walks its ring and gives up at the first smaller k-mer, so
//                 the ring's smallest node alone finishes and appends a circular unitig of one segment.
//   -- the one synchronisation: unitigs, bytes, error bits --
//   6 order       cfrk_sort_export by first k-mer with the record index as payload; lengths scanned into the starts
//   7 emit        one lane per segment walks its nodes again: the node at unitig position j stores its last base at
//                 start + k - 1 + j, the node at 0 its first k - 1 bases as well; terminators with the starts.
// No lane walks more than one segment's nodes or one unitig's segments: with s = 10 a unitig of 5 * 10^6 nodes is
// ~5000 segments of ~1000 nodes.  Every walk is bounded by the number of slots as well, so that a bug cannot spin.
//
// Work memory (BUF_UNITIG), per index slot M and with o = 2 orientations in a canonical job, else 1; S = M (k <= 12)
// or M / 2 (the hash index's load is at most 0.5) bounds the solid nodes: 3 M bytes (adj, link bits, marks) + 8 M (the
// segment of a head, indexed by v) + 64 o S (segments) + 40 S (unitigs).  Canonical hash index: 95 bytes per slot.
#include "staging.h"
#include "unitig_dev.h"

#include <hipcub/hipcub.hpp>

namespace {

constexpr uint32_t U_NONE = 0xFFFFFFFFu;
enum { L_SOLID = 1, L_OUT = 2, L_IN = 4, L_OUT_CUT = 8, L_IN_CUT = 16, L_PAL = 32 };
enum { UC_NSEG = 0, UC_NU, UC_BYTES, UC_ERR, UC_WORDS = 8 };
enum { UE_TOO_LONG = 1, UE_CAPACITY = 2, UE_WALK = 4 };

struct USeg {
  uint64_t head, tail;                // oriented nodes
  uint64_t kc, min_lo, min_hi;        // sum of the counts; the smallest oriented k-mer of the segment
  uint32_t n, min_off;                // nodes; where that k-mer lies
  uint32_t unitig, off;               // U_NONE: not emitted (the mirror image is); offset of the head in the unitig
  uint32_t mark, pad;                 // a hop from a unitig's head came by
};
static_assert(sizeof(USeg) == 64, "USeg is 64 bytes");

struct UWork {
  QIndex q;
  uint64_t M, seg_cap, u_cap, split_mask;
  USolid sol;                         // min_count and the graph mask
  uint8_t *adj, *lk, *vis;
  uint32_t *hid;                      // [2 M]: the segment an oriented node heads
  USeg *seg;
  uint64_t *ulo, *uhi;                // a unitig's first k-mer
  cfrk_unitig *urec;
  uint32_t *urot, *urank;             // rotation D of a circular unitig; its place in the sorted output
  unsigned long long *ctr;            // UC_*
};

__device__ __forceinline__ bool u_splitter(u128 key, uint64_t split_mask) {
  return (dev_mix64((uint64_t)key ^ dev_mix64((uint64_t)(key >> 64))) & split_mask) == 0;
}

// the neighbour byte / the link bits of the reverse complement of the k-mer they were computed for
__device__ __forceinline__ uint32_t u_rev4(uint32_t x) { return ((x & 1) << 3) | ((x & 2) << 1) | ((x & 4) >> 1) | ((x & 8) >> 3); }
__device__ __forceinline__ uint32_t u_mirror(uint32_t m) { return u_rev4(m >> 4) | (u_rev4(m & 15) << 4); }
__device__ __forceinline__ uint32_t u_lbits(uint32_t l, int o) {
  if (!o) return l;
  return (l & (L_SOLID | L_PAL)) | ((l & L_OUT) ? L_IN : 0) | ((l & L_IN) ? L_OUT : 0) | ((l & L_OUT_CUT) ? L_IN_CUT : 0) |
         ((l & L_IN_CUT) ? L_OUT_CUT : 0);
}

// ---- nodes (u_node: unitig_dev.h) -------------------------------------------------------------------------------
template <int MODE>
__device__ __forceinline__ u128 u_slot_key(const QIndex &q, uint64_t slot) {
  uint64_t lo, hi;
  q_slot_key<MODE>(q, slot, lo, hi);
  return u_make(lo, hi);
}
template <int MODE>
__device__ __forceinline__ u128 u_okey(const QIndex &q, uint64_t v) {
  const u128 x = u_slot_key<MODE>(q, v >> 1);
  return (v & 1) ? u_rc(x, q.k) : x;
}

// the neighbour mask of oriented k-mer x, which need not be present itself
template <int MODE, bool CANON, bool MASKED>
__device__ __forceinline__ uint32_t u_neighbors(const QIndex &q, u128 x, const USolid &sol) {
  const int k = q.k;
  uint32_t m = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const u128 z = j < 4 ? u_succ_key(x, j, k) : u_pred_key(x, j - 4, k);
    int o; bool pal;
    const uint64_t s = u_node<MODE, CANON>(q, z, o, pal);
    if (u_solid<MODE, MASKED>(q, sol, s)) m |= 1u << j;
  }
  return m;
}

// the oriented node the out-link of v leads to (v has one: exactly one successor bit)
template <int MODE, bool CANON>
__device__ __forceinline__ uint64_t u_next(const UWork &w, uint64_t v) {
  uint32_t m = w.adj[v >> 1];
  if (v & 1) m = u_mirror(m);
  const int b = __builtin_ctz((m & 15) | 16);
  int o; bool pal;
  const uint64_t s = u_node<MODE, CANON>(w.q, u_succ_key(u_okey<MODE>(w.q, v), b & 3, w.q.k), o, pal);
  return s == Q_NO_SLOT ? ~0ull : 2 * s + o;
}

// ---- the public neighbour masks ---------------------------------------------------------------------------------
template <int MODE, bool CANON, bool MASKED>
__device__ __forceinline__ void u_neighbors_body(const QIndex &q, const uint64_t *__restrict__ keys_lo,
                                                 const uint64_t *__restrict__ keys_hi, int64_t n, const USolid &sol,
                                                 uint8_t *__restrict__ out) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  const int k = q.k;
  for (int64_t i = tid; i < n; i += nthreads) {
    const uint64_t lo = keys_lo[i], hi = keys_hi ? keys_hi[i] : 0;
    bool in_range;
    if (MODE < 2) in_range = hi == 0 && (k == 32 || (lo >> (2 * k)) == 0);
    else in_range = k == 64 || (hi >> (2 * k - 64)) == 0;
    out[i] = in_range ? (uint8_t)u_neighbors<MODE, CANON, MASKED>(q, u_make(lo, hi), sol) : (uint8_t)0;
  }
}
U_SOLID_KERNELS(u_neighbors, (QIndex q, const uint64_t *__restrict__ keys_lo, const uint64_t *__restrict__ keys_hi, int64_t n, USolid sol,
                              uint8_t *__restrict__ out), (q, keys_lo, keys_hi, n, sol, out))

// ---- 1 adjacency ------------------------------------------------------------------------------------------------
template <int MODE, bool CANON, bool MASKED>
__device__ __forceinline__ void u_adj_body(const UWork &w) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t slot = tid; slot < w.M; slot += nthreads) {
    const bool solid = u_solid<MODE, MASKED>(w.q, w.sol, slot);
    w.lk[slot] = solid ? L_SOLID : 0;
    w.vis[slot] = 0;
    w.adj[slot] = solid ? (uint8_t)u_neighbors<MODE, CANON, MASKED>(w.q, u_slot_key<MODE>(w.q, slot), w.sol) : (uint8_t)0;
  }
}
U_SOLID_KERNELS(u_adj, (UWork w), (w))

// ---- 2 links ----------------------------------------------------------------------------------------------------
// A link a -> b (oriented) is cut iff b is a stored key and a splitter, or rc(a) is a stored key and a splitter: the
// two ends of the link and the two ends of its mirror image rc(b) -> rc(a) all compute the same bit from this rule.
template <int MODE, bool CANON>
__global__ __launch_bounds__(256) void u_link_kernel(UWork w) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  const int k = w.q.k;
  for (uint64_t slot = tid; slot < w.M; slot += nthreads) {
    if (!(w.lk[slot] & L_SOLID)) continue;
    const u128 x = u_slot_key<MODE>(w.q, slot);
    uint32_t l = L_SOLID;
    if (CANON && u_rc(x, k) == x) { w.lk[slot] = L_SOLID | L_PAL; continue; }
    const uint32_t m = w.adj[slot];
    const bool xs = u_splitter(x, w.split_mask);
    if (__popc(m & 15) == 1) {                                  // x -> z
      const u128 z = u_succ_key(x, __builtin_ctz(m & 15), k);
      int oz; bool pal;
      const uint64_t sz = u_node<MODE, CANON>(w.q, z, oz, pal);
      if (sz != Q_NO_SLOT && sz != slot && !pal) {
        uint32_t mz = w.adj[sz];
        if (oz) mz = u_mirror(mz);
        if (__popc(mz >> 4) == 1) {
          l |= L_OUT;
          if (oz == 0 && u_splitter(z, w.split_mask)) l |= L_OUT_CUT;
        }
      }
    }
    if (__popc(m >> 4) == 1) {                                  // p -> x
      const u128 p = u_pred_key(x, __builtin_ctz(m >> 4), k);
      int op; bool pal;
      const uint64_t sp = u_node<MODE, CANON>(w.q, p, op, pal);
      if (sp != Q_NO_SLOT && sp != slot && !pal) {
        uint32_t mp = w.adj[sp];
        if (op) mp = u_mirror(mp);
        if (__popc(mp & 15) == 1) {
          l |= L_IN;
          if (xs || (op == 1 && u_splitter(u_rc(p, k), w.split_mask))) l |= L_IN_CUT;
        }
      }
    }
    w.lk[slot] = (uint8_t)l;
  }
}

// ---- 3 segments -------------------------------------------------------------------------------------------------
template <bool CANON>
__global__ __launch_bounds__(256) void u_heads_kernel(UWork w) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t slot = tid; slot < w.M; slot += nthreads) {
    const uint32_t l0 = w.lk[slot];
    if (!(l0 & L_SOLID)) continue;
    for (int o = 0; o < (CANON && !(l0 & L_PAL) ? 2 : 1); ++o) {
      const uint32_t l = u_lbits(l0, o);
      if ((l & L_IN) && !(l & L_IN_CUT)) continue;
      const unsigned long long id = atomicAdd(&w.ctr[UC_NSEG], 1ull);
      if (id >= w.seg_cap) { atomicOr(&w.ctr[UC_ERR], (unsigned long long)UE_CAPACITY); continue; }
      w.hid[2 * slot + o] = (uint32_t)id;
      w.seg[id].head = 2 * slot + o;
    }
  }
}

template <int MODE, bool CANON>
__global__ __launch_bounds__(256) void u_walk_kernel(UWork w) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t nseg = min((uint64_t)w.ctr[UC_NSEG], w.seg_cap);
  for (uint64_t i = tid; i < nseg; i += nthreads) {
    uint64_t v = w.seg[i].head, kc = 0, n = 0, min_off = 0;
    u128 best = ~(u128)0;
    for (;;) {
      const uint64_t slot = v >> 1;
      const u128 key = u_okey<MODE>(w.q, v);
      kc += q_slot_count<MODE>(w.q, slot);
      if (n == 0 || key < best) { best = key; min_off = n; }
      ++n;
      w.vis[slot] = 1;
      const uint32_t l = u_lbits(w.lk[slot], (int)(v & 1));
      if (!(l & L_OUT) || (l & L_OUT_CUT)) break;
      const uint64_t nx = u_next<MODE, CANON>(w, v);
      if (nx == ~0ull || n > 2 * w.M) { atomicOr(&w.ctr[UC_ERR], (unsigned long long)UE_WALK); break; }
      v = nx;
    }
    USeg &s = w.seg[i];
    s.tail = v; s.kc = kc; s.min_lo = (uint64_t)best; s.min_hi = (uint64_t)(best >> 64);
    s.n = (uint32_t)n; s.min_off = (uint32_t)min_off; s.unitig = U_NONE; s.off = 0; s.mark = 0; s.pad = 0;
  }
}

// a new unitig of N nodes: its record index, or U_NONE (too long, or no room: the error bits say which)
__device__ __forceinline__ uint32_t u_append(const UWork &w, u128 first, uint64_t N, uint64_t KC, uint32_t flags, uint32_t rot) {
  const int k = w.q.k;
  if (N + (uint64_t)k - 1 > 0x7FFFFFFFull) { atomicOr(&w.ctr[UC_ERR], (unsigned long long)UE_TOO_LONG); return U_NONE; }
  const unsigned long long u = atomicAdd(&w.ctr[UC_NU], 1ull);
  if (u >= w.u_cap) { atomicOr(&w.ctr[UC_ERR], (unsigned long long)UE_CAPACITY); return U_NONE; }
  atomicAdd(&w.ctr[UC_BYTES], (unsigned long long)(N + (uint64_t)k));
  w.ulo[u] = (uint64_t)first; w.uhi[u] = (uint64_t)(first >> 64);
  cfrk_unitig r; r.kc = KC; r.n_kmers = (uint32_t)N; r.flags = flags;
  w.urec[u] = r;
  w.urot[u] = rot;
  return (uint32_t)u;
}

// the segment behind segment s across the cut link at its tail, U_NONE when the tail has no out-link
template <int MODE, bool CANON>
__device__ __forceinline__ uint32_t u_next_seg(const UWork &w, uint32_t s) {
  const uint64_t t = w.seg[s].tail;
  if (!(u_lbits(w.lk[t >> 1], (int)(t & 1)) & L_OUT)) return U_NONE;
  const uint64_t nx = u_next<MODE, CANON>(w, t);
  return nx == ~0ull ? U_NONE : w.hid[nx];
}

// ---- 4 stitch ---------------------------------------------------------------------------------------------------
template <int MODE, bool CANON>
__global__ __launch_bounds__(256) void u_stitch_kernel(UWork w) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t nseg = min((uint64_t)w.ctr[UC_NSEG], w.seg_cap);
  for (uint64_t i = tid; i < nseg; i += nthreads) {
    const uint64_t h = w.seg[i].head;
    if (u_lbits(w.lk[h >> 1], (int)(h & 1)) & L_IN) continue;
    uint64_t N = 0, KC = 0, hops = 0;
    uint32_t s = (uint32_t)i, last = s;
    while (s != U_NONE && s < nseg && hops++ <= nseg) {
      w.seg[s].mark = 1;
      N += w.seg[s].n; KC += w.seg[s].kc;
      last = s;
      s = u_next_seg<MODE, CANON>(w, s);
    }
    const u128 a1 = u_okey<MODE>(w.q, h);
    if (CANON && u_okey<MODE>(w.q, w.seg[last].tail ^ 1) < a1) continue;       // the mirror image is emitted
    const uint32_t u = u_append(w, a1, N, KC, 0, 0);
    if (u == U_NONE) continue;
    uint64_t off = 0;
    s = (uint32_t)i; hops = 0;
    while (s != U_NONE && s < nseg && hops++ <= nseg) {
      w.seg[s].unitig = u; w.seg[s].off = (uint32_t)off;
      off += w.seg[s].n;
      s = u_next_seg<MODE, CANON>(w, s);
    }
  }
}

// ---- 5a rings of segments ---------------------------------------------------------------------------------------
template <int MODE, bool CANON>
__global__ __launch_bounds__(256) void u_ring_kernel(UWork w) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t nseg = min((uint64_t)w.ctr[UC_NSEG], w.seg_cap);
  for (uint64_t i = tid; i < nseg; i += nthreads) {
    if (w.seg[i].mark) continue;
    uint64_t N = 0, KC = 0, hops = 0;
    u128 best = ~(u128)0, mbest = ~(u128)0;
    uint32_t s = (uint32_t)i, leader = U_NONE;
    bool closed = false;
    while (s != U_NONE && s < nseg && hops++ <= nseg) {
      const USeg &g = w.seg[s];
      const u128 mk = u_make(g.min_lo, g.min_hi);
      if (leader == U_NONE || mk < best) { best = mk; leader = s; }
      if (CANON) {                                              // the mirror segment is headed by the tail's complement
        const USeg &r = w.seg[min((uint64_t)w.hid[g.tail ^ 1], nseg - 1)];
        const u128 rk = u_make(r.min_lo, r.min_hi);
        if (rk < mbest) mbest = rk;
      }
      N += g.n; KC += g.kc;
      s = u_next_seg<MODE, CANON>(w, s);
      if (s == (uint32_t)i) { closed = true; break; }
    }
    if (!closed) { atomicOr(&w.ctr[UC_ERR], (unsigned long long)UE_WALK); continue; }
    if (leader != (uint32_t)i || (CANON && !(best < mbest))) continue;
    const uint32_t u = u_append(w, best, N, KC, CFRK_UNITIG_CIRCULAR, w.seg[i].min_off);
    if (u == U_NONE) continue;
    uint64_t off = 0;
    s = (uint32_t)i; hops = 0;
    do {
      w.seg[s].unitig = u; w.seg[s].off = (uint32_t)off;
      off += w.seg[s].n;
      s = u_next_seg<MODE, CANON>(w, s);
    } while (s != (uint32_t)i && s != U_NONE && s < nseg && hops++ <= nseg);
  }
}

// ---- 5b rings without a splitter --------------------------------------------------------------------------------
template <int MODE, bool CANON>
__global__ __launch_bounds__(256) void u_free_ring_kernel(UWork w) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  const int k = w.q.k;
  for (uint64_t slot = tid; slot < w.M; slot += nthreads) {
    if (!(w.lk[slot] & L_SOLID) || w.vis[slot]) continue;
    const uint64_t v0 = 2 * slot;
    const u128 x0 = u_slot_key<MODE>(w.q, slot);
    uint64_t v = v0, N = 0, KC = 0;
    bool lead = true;
    for (;;) {
      const u128 key = u_okey<MODE>(w.q, v);
      if (key < x0 || (CANON && u_rc(key, k) < x0)) { lead = false; break; }   // a smaller k-mer on the ring or its mirror
      KC += q_slot_count<MODE>(w.q, v >> 1);
      ++N;
      const uint64_t nx = u_next<MODE, CANON>(w, v);
      if (nx == v0) break;
      if (nx == ~0ull || N > 2 * w.M) { atomicOr(&w.ctr[UC_ERR], (unsigned long long)UE_WALK); lead = false; break; }
      v = nx;
    }
    if (!lead) continue;
    const uint32_t u = u_append(w, x0, N, KC, CFRK_UNITIG_CIRCULAR, 0);
    if (u == U_NONE) continue;
    const unsigned long long id = atomicAdd(&w.ctr[UC_NSEG], 1ull);
    if (id >= w.seg_cap) { atomicOr(&w.ctr[UC_ERR], (unsigned long long)UE_CAPACITY); continue; }
    USeg g;
    g.head = v0; g.tail = v; g.kc = KC; g.min_lo = (uint64_t)x0; g.min_hi = (uint64_t)(x0 >> 64);
    g.n = (uint32_t)N; g.min_off = 0; g.unitig = u; g.off = 0; g.mark = 1; g.pad = 0;
    w.seg[id] = g;
  }
}

// ---- 6 order ----------------------------------------------------------------------------------------------------
__global__ void u_iota_kernel(uint32_t *idx, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) idx[i] = (uint32_t)i;
}
// sorted place j holds record perm[j]: its rank, its record and length to the caller, its bytes to the scan
__global__ void u_place_kernel(UWork w, const uint32_t *__restrict__ perm, uint64_t nU, int64_t *__restrict__ len64,
                               int32_t *__restrict__ length_out, cfrk_unitig *__restrict__ rec_out) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nU) return;
  const uint32_t u = perm[j];
  const cfrk_unitig r = w.urec[u];
  w.urank[u] = (uint32_t)j;
  const int32_t len = (int32_t)(r.n_kmers + (uint32_t)w.q.k - 1u);
  length_out[j] = len;
  rec_out[j] = r;
  len64[j] = (int64_t)len + 1;
}
__global__ void u_starts_kernel(const int64_t *__restrict__ st64, const int32_t *__restrict__ length_out, uint64_t nU,
                                int64_t *__restrict__ start_out, int8_t *__restrict__ data_out) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nU) return;
  start_out[j] = st64[j];
  data_out[st64[j] + length_out[j]] = -1;
}

// ---- 7 emit -----------------------------------------------------------------------------------------------------
template <int MODE, bool CANON>
__global__ __launch_bounds__(256) void u_emit_kernel(UWork w, uint64_t nseg, const int64_t *__restrict__ st64,
                                                     int8_t *__restrict__ data_out) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  const int k = w.q.k;
  for (uint64_t i = tid; i < nseg; i += nthreads) {
    const USeg g = w.seg[i];
    if (g.unitig == U_NONE) continue;
    const cfrk_unitig r = w.urec[g.unitig];
    const uint64_t N = r.n_kmers, D = w.urot[g.unitig];
    const bool circ = (r.flags & CFRK_UNITIG_CIRCULAR) != 0;
    int8_t *out = data_out + st64[w.urank[g.unitig]];
    uint64_t v = g.head;
    for (uint64_t p = 0; p < g.n; ++p) {
      const u128 key = u_okey<MODE>(w.q, v);
      uint64_t j = g.off + p;
      if (circ) j = (j + N - D) % N;
      if (j < N) {                                               // (always; a bug must not write outside the unitig)
        out[(uint64_t)k - 1 + j] = (int8_t)((uint32_t)key & 3u);
        if (j == 0)
          for (int t = 0; t < k - 1; ++t) out[t] = (int8_t)((uint32_t)(key >> (2 * (k - 1 - t))) & 3u);
      }
      if (p + 1 < g.n) {
        v = u_next<MODE, CANON>(w, v);
        if (v == ~0ull) break;
      }
    }
  }
}

// the parts of BUF_UNITIG for an index of M slots (the same carve in both steps)
size_t u_carve(void *base, const QIndex &q, bool canon, UWork *w) {
  const bool dense = q.k <= 12;
  const uint64_t M = dense ? 1ull << (2 * q.k) : q.mask + 1;
  const uint64_t S = dense ? M : M / 2 + 16;
  w->q = q; w->M = M; w->u_cap = S; w->seg_cap = S * (canon ? 2 : 1);
  Carve c;
  const size_t o_ctr = c.part(UC_WORDS * 8), o_adj = c.part(M), o_lk = c.part(M), o_vis = c.part(M), o_hid = c.part(2 * M * 4),
               o_seg = c.part(w->seg_cap * sizeof(USeg)), o_ulo = c.part(S * 8), o_uhi = c.part(S * 8),
               o_urec = c.part(S * sizeof(cfrk_unitig)), o_urot = c.part(S * 4), o_urank = c.part(S * 4);
  if (base) {
    w->ctr = carve_at<unsigned long long>(base, o_ctr);
    w->adj = carve_at<uint8_t>(base, o_adj); w->lk = carve_at<uint8_t>(base, o_lk); w->vis = carve_at<uint8_t>(base, o_vis);
    w->hid = carve_at<uint32_t>(base, o_hid); w->seg = carve_at<USeg>(base, o_seg);
    w->ulo = carve_at<uint64_t>(base, o_ulo); w->uhi = carve_at<uint64_t>(base, o_uhi);
    w->urec = carve_at<cfrk_unitig>(base, o_urec); w->urot = carve_at<uint32_t>(base, o_urot); w->urank = carve_at<uint32_t>(base, o_urank);
  }
  return c.end;
}

int u_split_log2(const cfrk_ctx *ctx) {
  const double p = ctx->dbg_param[CFRK_PARAM_UNITIG_SPLIT_LOG2];
  return p > 0 ? (int)p - 1 : CFRK_UNITIG_SPLIT_LOG2_DEFAULT;
}

}  // namespace

int cfrk_neighbors_launch(cfrk_ctx *ctx, const uint64_t *d_lo, const uint64_t *d_hi, int64_t n, uint32_t min_count, uint8_t *d_masks) {
  QIndex q;
  int rc = cfrk_query_index(ctx, &q);
  if (rc || n == 0) return rc;
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  const int mode = q.k <= 12 ? 0 : q.k <= 32 ? 1 : 2;
  const USolid sol = u_solid_rule(ctx, min_count);
  U_DISPATCH_SOLID(u_neighbors, sol, u_grid(ctx, (uint64_t)n), q, d_lo, d_hi, n, sol, d_masks);
  HIP_TRY(ctx, hipGetLastError());
  return CFRK_OK;
}

// stages 1 .. 5 and the synchronisation: the unitigs and their bytes
int cfrk_unitigs_measure(cfrk_ctx *ctx, uint32_t min_count, int64_t *nN, int64_t *nS, uint64_t *nseg) {
  QIndex q;
  int rc = cfrk_query_index(ctx, &q);
  if (rc) return rc;
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  const int mode = q.k <= 12 ? 0 : q.k <= 32 ? 1 : 2;
  UWork w;
  const size_t bytes = u_carve(nullptr, q, canon, &w);
  if (w.M > (1ull << 31)) return cfrk_fail(ctx, CFRK_ERR_ARG, "an index of %llu slots is too large for the unitig call", (unsigned long long)w.M);
  void *base;
  if ((rc = cfrk_pool_get(ctx, BUF_UNITIG, bytes, &base))) return rc;
  u_carve(base, q, canon, &w);
  w.sol = u_solid_rule(ctx, min_count);
  w.split_mask = (1ull << u_split_log2(ctx)) - 1;
  HIP_TRY(ctx, hipMemsetAsync(w.ctr, 0, UC_WORDS * 8, ctx->stream));
  const int gm = u_grid(ctx, w.M), gs = u_grid(ctx, w.seg_cap);
  U_DISPATCH_SOLID(u_adj, w.sol, gm, w);
  U_DISPATCH(u_link_kernel, gm, w);
  if (canon) hipLaunchKernelGGL(u_heads_kernel<true>, dim3(gm), dim3(256), 0, ctx->stream, w);
  else hipLaunchKernelGGL(u_heads_kernel<false>, dim3(gm), dim3(256), 0, ctx->stream, w);
  U_DISPATCH(u_walk_kernel, gs, w);
  U_DISPATCH(u_stitch_kernel, gs, w);
  U_DISPATCH(u_ring_kernel, gs, w);
  U_DISPATCH(u_free_ring_kernel, gm, w);
  HIP_TRY(ctx, hipGetLastError());
  unsigned long long h[UC_WORDS];
  HIP_TRY(ctx, hipMemcpyAsync(h, w.ctr, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (h[UC_ERR] & UE_TOO_LONG) return cfrk_fail(ctx, CFRK_ERR_LAYOUT, "a unitig is longer than 2^31 - 1 bases");
  if (h[UC_ERR]) return cfrk_fail(ctx, CFRK_ERR_STATE, "unitigs: internal error, the graph walk did not close (bits 0x%llx)", h[UC_ERR]);
  if (h[UC_NU] >= (1ull << 32)) return cfrk_fail(ctx, CFRK_ERR_ARG, "%llu unitigs are too many to sort", h[UC_NU]);
  *nN = (int64_t)h[UC_BYTES];
  *nS = (int64_t)h[UC_NU];
  *nseg = std::min<uint64_t>(h[UC_NSEG], w.seg_cap);
  return CFRK_OK;
}

// stages 6 and 7, left enqueued: the nS >= 1 unitigs and the nseg segments cfrk_unitigs_measure reported
int cfrk_unitigs_emit(cfrk_ctx *ctx, int8_t *d_data, int64_t *d_start, int32_t *d_length, cfrk_unitig *d_rec, int64_t nS, uint64_t nseg) {
  QIndex q;
  int rc = cfrk_query_index(ctx, &q);
  if (rc) return rc;
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  const int mode = q.k <= 12 ? 0 : q.k <= 32 ? 1 : 2;
  UWork w;
  u_carve(ctx->pool[BUF_UNITIG].p, q, canon, &w);
  const uint64_t n = (uint64_t)nS;
  size_t scan_tmp = 0;
  HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_tmp, (const int64_t *)nullptr, (int64_t *)nullptr, (int)n, ctx->stream));
  Carve c;
  const size_t o_iota = c.part(n * 4), o_len = c.part(n * 8), o_st = c.part(n * 8), o_tmp = c.part(scan_tmp);
  void *aux;
  if ((rc = cfrk_pool_get(ctx, BUF_UNITIG_AUX, c.end, &aux))) return rc;
  uint32_t *iota = carve_at<uint32_t>(aux, o_iota);
  int64_t *len64 = carve_at<int64_t>(aux, o_len), *st64 = carve_at<int64_t>(aux, o_st);
  const unsigned nb = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(u_iota_kernel, dim3(nb), dim3(256), 0, ctx->stream, iota, n);
  const uint64_t *s_lo, *s_hi;
  const uint32_t *perm;
  if ((rc = cfrk_sort_export(ctx, w.ulo, q.k > 32 ? w.uhi : nullptr, iota, n, &s_lo, &s_hi, &perm))) return rc;
  hipLaunchKernelGGL(u_place_kernel, dim3(nb), dim3(256), 0, ctx->stream, w, perm, n, len64, d_length, d_rec);
  HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(carve_at<void>(aux, o_tmp), scan_tmp, (const int64_t *)len64, st64, (int)n, ctx->stream));
  hipLaunchKernelGGL(u_starts_kernel, dim3(nb), dim3(256), 0, ctx->stream, (const int64_t *)st64, (const int32_t *)d_length, n, d_start, d_data);
  U_DISPATCH(u_emit_kernel, u_grid(ctx, nseg), w, nseg, (const int64_t *)st64, d_data);
  HIP_TRY(ctx, hipGetLastError());
  return CFRK_OK;
}
