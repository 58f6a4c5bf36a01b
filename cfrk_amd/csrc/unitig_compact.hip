// unitig_compact.hip -- the compacted graph of a unitig list without some of its unitigs, from the list itself: the
// sequences and records as cfrk_global_unitigs wrote them, the link CSR as cfrk_global_unitig_links wrote it, and the drop
// bytes.  No index, no counts: what cfrk_global_unitigs rediscovers with its per-slot k-mer passes after
// cfrk_global_mask_unitigs(drop) is a pure function of these.  The contract and the rule are in include/cfrk_abi.h
// ("Unitig compaction"); DESIGN 4.25 has the reasoning.
//
// An ELEMENT is an oriented unitig: x = 2 u + o in a canonical job (o = 1: the reverse complement), x = u otherwise.
// The arrays are untrusted.  Passes, each a launch of its own on the context stream; every pass behind the checks reads
// the error word first and does nothing when it is set, so that only checked rows and ranges are ever followed:
//   1   rows      the check of unitig_graph_dev.h and, not canonical only, the in-rows
//   2   layout    one lane per unitig: length, n_kmers, the range, the ascending starts
//   3   next      one lane per element: its only surviving out-link, the target's only surviving in-link read off the
//                 TARGET's row, the exclusions, the k - 1 overlap in the two end windows -> nxt[x], prv[y]
//   4   rank      pointer doubling over prv, ceil(log2 nS) launches of one lane per element, double-buffered (the launches
//                 behind a round in which no pointer moved return at once): a path
//                 element ends with its head, its offset in k-mers, its summed counts and its index in the chain; a cycle
//                 element with the cycle's smallest element (the leader) and the same three relative to the leader, the
//                 leader itself with the cycle's totals.  No lane ever walks a chain.
//   5   cycles    the windows of cycle members only, scanned into one range and dealt out one window per lane: the
//                 smallest oriented k-mer of a cycle by three atomic-minimum passes (high word, low word, position)
//   6   choose    one lane per element: a path's tail, or a cycle's leader, holds its first k-mer against its mirror's
//                 and, as the winner, appends the component
//   -- the one synchronisation: the error word, the components, the bytes --
//   7   order     cfrk_sort_export by first k-mer; lengths and member counts scanned; every member into its slot of the
//                 members' list (component by component in output order, a component's members in chain order); into[]
//   8   emit      one workgroup per tile of UC_TILE OUTPUT bytes, 16 consecutive bytes per lane, stored as one 16-byte
//                 word where the lane's bytes all exist (the tiles are laid on the 16-byte grid of data_out's address, so
//                 every such store is aligned whatever the pointer): a lane finds its unitig by binary search in the
//                 starts, among the tile's unitigs only (two lanes find the tile's first and last), and its member by
//                 binary search in the members' offsets; behind its first byte it steps forward and searches no more.
//                 Reversed members are read backwards as 3 - c.  Terminators are output bytes like any other.
// Work memory (BUF_UNITIG_COMPACT), per element: 8 (nxt, prv) + 96 (two rank states) + 8 (cycle windows) + 24 (cycle
// minima) + 4 (the root's component); per unitig 44 (components); BUF_UNITIG_COMPACT_AUX per output unitig 44 and per
// unitig 8 (the members' list).  16 bytes of LDS in the emit (a tile's first and last unitig), none elsewhere; no scratch.
#include "unitig_graph_dev.h"

namespace {

constexpr uint32_t UC_NONE = 0xFFFFFFFFu;
constexpr int UC_TILE = CFRK_COMPACT_TILE_BYTES;      // output bytes per workgroup of the emit: 256 lanes x 16
enum { UCC_ERR = UGC_ERR, UCC_NU, UCC_BYTES, UCC_ACTIVE /* one word per rank round: a pointer moved */, UCC_WORDS = UCC_ACTIVE + 32 };
// the error word's own reasons, behind those of unitig_graph_dev.h
enum { UCE_SHORT = 16, UCE_KMERS, UCE_RANGE, UCE_ORDER, UCE_OVERLAP, UCE_LONG };
enum { UCF_PATH = 0, UCF_CYCLE = 1, UCF_DEAD = 2 };

// One element's rank state.  While doubling: ptr = the element 2^r links back (a head points at itself), acc / kacc /
// cnt = the k-mers, counts and elements of the 2^r predecessors; m = the smallest of them, dist / kdist / mcnt = the
// k-mers, counts and elements from m (inclusive) to this one (exclusive).  After uc_finish_kernel: ptr = the root (a
// path's head, a cycle's leader), acc / kacc / cnt relative to the root, m = UCF_*; a leader keeps the cycle's totals in
// dist / kdist / mcnt.
struct UCState {
  uint32_t ptr, m, cnt, mcnt;
  uint64_t acc, kacc, dist, kdist;
};
static_assert(sizeof(UCState) == 48, "UCState is 48 bytes");

struct UCWork : UGraph {
  const int8_t *data;
  const int64_t *start;
  const int32_t *length;
  const uint8_t *drop;                // NULL: nothing is dropped
  int64_t nN;
  uint64_t X;                         // elements
  int k;
  uint32_t *nxt, *prv;                // [X]
  UCState *st[2];                     // [X] each
  unsigned long long *woff;           // [X + 1]: a cycle member's windows, scanned
  unsigned long long *cmin_hi, *cmin_lo, *cpos;   // [X], at the leader: the cycle's smallest k-mer and where it lies
  uint64_t *c_lo, *c_hi;              // [nS] components: the first k-mer
  cfrk_unitig *c_rec;
  uint32_t *c_root, *c_rot, *c_mem;   // the root element, the cut of a cycle, the members
  uint32_t *comp_of;                  // [X], at the root: its component, UC_NONE when the mirror image is written
};

template <bool CANON> __device__ __forceinline__ uint32_t uc_u(uint32_t x) { return CANON ? x >> 1 : x; }
template <bool CANON> __device__ __forceinline__ uint32_t uc_o(uint32_t x) { return CANON ? x & 1u : 0u; }
template <bool CANON> __device__ __forceinline__ uint32_t uc_el(uint32_t u, uint32_t o) { return CANON ? (u << 1) | o : u; }

__device__ __forceinline__ bool uc_dropped(const UCWork &w, uint32_t u) { return w.drop && w.drop[u] != 0; }

// base i of oriented unitig (u,o) of a checked range
__device__ __forceinline__ int uc_base(const UCWork &w, uint32_t u, uint32_t o, int64_t i) {
  const int64_t s = w.start[u];
  const int64_t len = w.length[u];
  return o ? 3 - (int)w.data[s + len - 1 - i] : (int)w.data[s + i];
}
// the k-mer at window p of oriented unitig (u,o)
__device__ __forceinline__ u128 uc_kmer(const UCWork &w, uint32_t u, uint32_t o, int64_t p) {
  u128 x = 0;
  int t = 0;
  for (; t + 8 <= w.k; t += 8) {                        // eight loads in flight: a lane alone with its unitig waits for each
    int b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = uc_base(w, u, o, p + t + j);
#pragma unroll
    for (int j = 0; j < 8; ++j) x = (x << 2) | (u128)((unsigned)b[j] & 3u);
  }
  for (; t < w.k; ++t) x = (x << 2) | (u128)((unsigned)uc_base(w, u, o, p + t) & 3u);
  return x;
}
// the first k-mers of two oriented unitigs compared as uc_kmer spells them, from the first base that differs: most
// pairs differ within a base or two
__device__ __forceinline__ int uc_head_cmp(const UCWork &w, uint32_t u, uint32_t o, uint32_t v, uint32_t p) {
  for (int t = 0; t < w.k; ++t) {
    const unsigned a = (unsigned)uc_base(w, u, o, t) & 3u, b = (unsigned)uc_base(w, v, p, t) & 3u;
    if (a != b) return a < b ? -1 : 1;
  }
  return 0;
}
// do bases [i, i + n) of (u,o) equal bases [j, j + n) of (v,p)
__device__ __forceinline__ bool uc_same(const UCWork &w, uint32_t u, uint32_t o, int64_t i, uint32_t v, uint32_t p, int64_t j, int n) {
  bool same = true;
  int t = 0;
  for (; t + 4 <= n && same; t += 4) {
    int a[4], b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { a[q] = uc_base(w, u, o, i + t + q); b[q] = uc_base(w, v, p, j + t + q); }
#pragma unroll
    for (int q = 0; q < 4; ++q) same &= a[q] == b[q];
  }
  for (; t < n && same; ++t) same = uc_base(w, u, o, i + t) == uc_base(w, v, p, j + t);
  return same;
}

// ---- 2 layout ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void uc_layout_kernel(UCWork w) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = tid; j < w.nS; j += nthreads) {
    const int64_t s = w.start[j], len = w.length[j];
    int why = 0;
    if (len < w.k) why = UCE_SHORT;
    else if ((uint64_t)len != (uint64_t)w.rec[j].n_kmers + (uint64_t)w.k - 1) why = UCE_KMERS;
    else if (s < 0 || s > w.nN || len > w.nN - s) why = UCE_RANGE;
    else if (j) {
      const int64_t ps = w.start[j - 1], pl = w.length[j - 1];
      if (ps >= 0 && ps <= w.nN && pl >= 0 && pl <= w.nN - ps && s < ps + pl) why = UCE_ORDER;   // (a bad predecessor is named itself)
    }
    if (why) ug_fail(w, j, why);
  }
}

// ---- 3 next -----------------------------------------------------------------------------------------------------
// canonical, n = 1, head == rc(head): a palindromic single node never merges
template <bool CANON>
__device__ __forceinline__ bool uc_palindrome(const UCWork &w, uint32_t u) {
  if (!CANON || w.rec[u].n_kmers != 1) return false;
  for (int t = 0; t < w.k; ++t)
    if (uc_base(w, u, 0, t) != uc_base(w, u, 1, t)) return false;
  return true;
}

template <bool CANON>
__global__ __launch_bounds__(256) void uc_next_kernel(UCWork w) {
  if (w.ctr[UGC_ERR] != UG_NONE) return;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t xi = tid; xi < w.X; xi += nthreads) {
    const uint32_t x = (uint32_t)xi, u = uc_u<CANON>(x), o = uc_o<CANON>(x);
    if (uc_dropped(w, u) || (w.rec[u].flags & CFRK_UNITIG_CIRCULAR)) continue;
    // out(x) among the survivors, read off u's row
    uint32_t n_out = 0, y = 0;
    for (int64_t t = w.ptr[u]; t < w.ptr[u + 1]; ++t) {
      const cfrk_unitig_link l = w.links[t];
      if (CANON && ((l.flags & CFRK_LINK_FROM_MINUS) ? 1u : 0u) != o) continue;
      if (uc_dropped(w, l.to)) continue;
      ++n_out;
      y = uc_el<CANON>(l.to, (CANON && (l.flags & CFRK_LINK_TO_MINUS)) ? 1u : 0u);
    }
    if (n_out != 1) continue;
    const uint32_t v = uc_u<CANON>(y), ov = uc_o<CANON>(y);
    if (w.rec[v].flags & CFRK_UNITIG_CIRCULAR) continue;
    if (v == u && (ov != o || w.rec[u].n_kmers == 1)) continue;       // a hairpin; the self-link of a single node
    // in(y) among the survivors, read off v's row: canonical, the links out of (v,!ov), mirrored
    uint32_t n_in = 0, src = 0;
    if (CANON) {
      for (int64_t t = w.ptr[v]; t < w.ptr[v + 1]; ++t) {
        const cfrk_unitig_link l = w.links[t];
        if (((l.flags & CFRK_LINK_FROM_MINUS) ? 1u : 0u) == ov) continue;
        if (uc_dropped(w, l.to)) continue;
        ++n_in;
        src = (l.to << 1) | ((l.flags & CFRK_LINK_TO_MINUS) ? 0u : 1u);
      }
    } else {
      for (unsigned long long t = w.in_off[v]; t < w.in_off[v + 1]; ++t) {
        const uint32_t s = w.in_src[t];
        if (s >= w.nS || uc_dropped(w, s)) continue;
        ++n_in;
        src = s;
      }
    }
    if (n_in != 1 || src != x) continue;
    if (uc_palindrome<CANON>(w, u) || uc_palindrome<CANON>(w, v)) continue;
    const int64_t lu = w.length[u];
    if (!uc_same(w, u, o, lu - (w.k - 1), v, ov, 0, w.k - 1)) { ug_fail(w, u < v ? u : v, UCE_OVERLAP); continue; }
    w.nxt[x] = y;
    w.prv[y] = x;                                       // (in(y) = {x}: no other lane writes it)
  }
}

// ---- 4 rank -----------------------------------------------------------------------------------------------------
template <bool CANON>
__global__ __launch_bounds__(256) void uc_rank_init_kernel(UCWork w) {
  if (w.ctr[UGC_ERR] != UG_NONE) return;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t xi = tid; xi < w.X; xi += nthreads) {
    const uint32_t x = (uint32_t)xi, p = w.prv[x];
    UCState s;
    if (p == UC_NONE) {
      s.ptr = s.m = x; s.cnt = s.mcnt = 0; s.acc = s.kacc = s.dist = s.kdist = 0;
    } else {
      const cfrk_unitig r = w.rec[uc_u<CANON>(p)];
      s.ptr = s.m = p; s.cnt = s.mcnt = 1; s.acc = s.dist = r.n_kmers; s.kacc = s.kdist = r.kc;
    }
    w.st[0][x] = s;
  }
}

// Round r reads st[r & 1] and writes the other.  A round in which no pointer moved has left both states equal in
// everything that is read afterwards (every path element is at its head; a ring whose pointers rest has been seen whole):
// it leaves ctr[UCC_ACTIVE + r] at 0, and every later round returns at once.  The launches are still ceil(log2 nS), the
// work is that of the longest chain's logarithm.  A ring whose size is no power of two keeps all rounds running.
__global__ __launch_bounds__(256) void uc_rank_kernel(UCWork w, int r) {
  if (w.ctr[UGC_ERR] != UG_NONE || (r > 0 && w.ctr[UCC_ACTIVE + r - 1] == 0)) return;
  const UCState *__restrict__ in = w.st[r & 1];
  UCState *__restrict__ out = w.st[(r & 1) ^ 1];
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  // (whole waves turn together: one store per wave says that a pointer moved)
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < w.X; base += nthreads) {
    const uint64_t x = base + threadIdx.x;
    bool moved = false;
    if (x < w.X) {
      UCState a = in[x];
      const UCState b = in[a.ptr];                      // (a head points at itself and holds zeros: nothing changes)
      moved = b.ptr != a.ptr;
      if (b.m < a.m) { a.m = b.m; a.dist = b.dist + a.acc; a.kdist = b.kdist + a.kacc; a.mcnt = b.mcnt + a.cnt; }
      a.ptr = b.ptr; a.acc += b.acc; a.kacc += b.kacc; a.cnt += b.cnt;
      out[x] = a;
    }
    const unsigned long long m = __ballot(moved);
    if (m && (threadIdx.x & 63) == (unsigned)__ffsll((long long)m) - 1u) w.ctr[UCC_ACTIVE + r] = 1;
  }
}

// what the doubling left, brought to one form (see UCState); a cycle member's windows for the scan
template <bool CANON>
__global__ __launch_bounds__(256) void uc_finish_kernel(UCWork w, int at) {
  if (w.ctr[UGC_ERR] != UG_NONE) return;
  UCState *st = w.st[at];
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t xi = tid; xi < w.X; xi += nthreads) {
    const uint32_t x = (uint32_t)xi, u = uc_u<CANON>(x);
    UCState s = st[x];                                  // (only this lane reads or writes st[x] in this pass)
    unsigned long long windows = 0;
    if (uc_dropped(w, u)) s.m = UCF_DEAD;
    else if (w.prv[s.ptr] == UC_NONE) s.m = UCF_PATH;   // 2^rounds >= nS links back: a path element has reached its head
    else {
      const bool leader = s.m == x;
      s.ptr = s.m;
      if (leader) { s.acc = s.kacc = 0; s.cnt = 0; }
      else { s.acc = s.dist; s.kacc = s.kdist; s.cnt = s.mcnt; }
      s.m = UCF_CYCLE;
      windows = w.rec[u].n_kmers;
    }
    st[x] = s;
    w.woff[x] = windows;
    if (xi == 0) w.woff[w.X] = 0;
  }
}

// ---- 5 cycles ---------------------------------------------------------------------------------------------------
// PASS 0: the high words' minimum; 1: the low words' among those; 2: the position of the k-mer that has both
template <bool CANON, int PASS>
__global__ __launch_bounds__(256) void uc_cycle_min_kernel(UCWork w, int at) {
  if (w.ctr[UGC_ERR] != UG_NONE) return;
  const UCState *__restrict__ st = w.st[at];
  const unsigned long long W = w.woff[w.X];
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (unsigned long long g = tid; g < W; g += nthreads) {
    uint64_t lo = 0, hi = w.X;                          // the last x with woff[x] <= g: woff[x] <= g < woff[x + 1]
    while (hi - lo > 1) {
      const uint64_t mid = (lo + hi) >> 1;
      if (w.woff[mid] <= g) lo = mid; else hi = mid;
    }
    const uint32_t x = (uint32_t)lo;
    const UCState s = st[x];
    const unsigned long long p = g - w.woff[x];
    if (s.m != UCF_CYCLE || p >= w.rec[uc_u<CANON>(x)].n_kmers) continue;   // (never)
    const u128 key = uc_kmer(w, uc_u<CANON>(x), uc_o<CANON>(x), (int64_t)p);
    const unsigned long long khi = (unsigned long long)(key >> 64), klo = (unsigned long long)key;
    if (PASS == 0) atomicMin(&w.cmin_hi[s.ptr], khi);
    else if (w.cmin_hi[s.ptr] != khi) continue;
    else if (PASS == 1) atomicMin(&w.cmin_lo[s.ptr], klo);
    else if (w.cmin_lo[s.ptr] == klo) atomicMin(&w.cpos[s.ptr], (unsigned long long)(s.acc + p));
  }
}

// ---- 6 choose ---------------------------------------------------------------------------------------------------
// what a lane that speaks for a written component found
struct UCComp {
  u128 first;
  uint64_t N, KC;
  uint32_t root, flags, rot, members, named;
};

// The components of a wave, appended together: one atomic per wave and counter (millions of lanes adding 1 to ONE word
// serialise at the L2; measured).  Every lane of the wave calls this; `mine` says whether x holds one.
__device__ __forceinline__ void uc_append(const UCWork &w, bool mine, const UCComp &x) {
  if (mine && x.N + (uint64_t)w.k - 1 > 0x7FFFFFFFull) { ug_fail(w, x.named, UCE_LONG); mine = false; }
  const unsigned long long m = __ballot(mine);
  if (!m) return;
  const unsigned lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  const int leader = __ffsll((long long)m) - 1;
  unsigned long long bytes = mine ? x.N + (uint64_t)w.k : 0;
  for (int o = 32; o > 0; o >>= 1) bytes += __shfl_xor(bytes, o);
  unsigned long long base = 0;
  if ((int)lane == leader) {
    base = atomicAdd(&w.ctr[UCC_NU], (unsigned long long)__popcll(m));
    atomicAdd(&w.ctr[UCC_BYTES], bytes);
  }
  base = __shfl(base, leader);
  if (!mine) return;
  const unsigned long long c = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1));
  if (c >= w.nS) return;                                // (never: a component has a member, a member one component)
  w.c_lo[c] = (uint64_t)x.first; w.c_hi[c] = (uint64_t)(x.first >> 64);
  cfrk_unitig r; r.kc = x.KC; r.n_kmers = (uint32_t)x.N; r.flags = x.flags;
  w.c_rec[c] = r;
  w.c_root[c] = x.root; w.c_rot[c] = x.rot; w.c_mem[c] = x.members;
  w.comp_of[x.root] = (uint32_t)c;
}

// does element x speak for a component that is written, and for which
template <bool CANON>
__device__ __forceinline__ bool uc_speaks(const UCWork &w, const UCState *__restrict__ st, uint32_t x, UCComp &c) {
  const uint32_t u = uc_u<CANON>(x), o = uc_o<CANON>(x);
  const UCState s = st[x];
  const cfrk_unitig r = w.rec[u];
  if (s.m == UCF_DEAD) return false;
  if (s.m == UCF_CYCLE) {
    if (s.ptr != x) return false;                       // the leader speaks for the cycle
    const u128 mine = u_make(w.cmin_lo[x], w.cmin_hi[x]);
    if (CANON) {
      const uint32_t ml = st[x ^ 1u].ptr;               // the mirror cycle's leader
      const u128 theirs = u_make(w.cmin_lo[ml], w.cmin_hi[ml]);
      if (!(mine < theirs || (mine == theirs && x < ml))) return false;
    }
    c.first = mine; c.N = s.dist; c.KC = s.kdist; c.root = x; c.flags = CFRK_UNITIG_CIRCULAR; c.rot = (uint32_t)w.cpos[x];
    c.members = s.mcnt; c.named = u;
    return true;
  }
  if (r.flags & CFRK_UNITIG_CIRCULAR) {                 // an input cycle is cut where it has to be: copied
    if (o) return false;
    c.first = uc_kmer(w, u, 0, 0); c.N = r.n_kmers; c.KC = r.kc; c.root = x; c.flags = CFRK_UNITIG_CIRCULAR; c.rot = 0;
    c.members = 1; c.named = u;
    return true;
  }
  if (w.nxt[x] != UC_NONE) return false;                // the tail speaks for the path
  const uint32_t h = s.ptr;
  if (CANON) {
    const uint32_t mh = x ^ 1u;                         // the mirror path's head
    const int cmp = uc_head_cmp(w, uc_u<CANON>(h), uc_o<CANON>(h), u, o ^ 1u);
    if (!(cmp < 0 || (cmp == 0 && h < mh))) return false;
  }
  c.first = uc_kmer(w, uc_u<CANON>(h), uc_o<CANON>(h), 0); c.N = s.acc + r.n_kmers; c.KC = s.kacc + r.kc; c.root = h; c.flags = 0; c.rot = 0;
  c.members = s.cnt + 1; c.named = uc_u<CANON>(h);
  return true;
}

template <bool CANON>
__global__ __launch_bounds__(256) void uc_choose_kernel(UCWork w, int at) {
  if (w.ctr[UGC_ERR] != UG_NONE) return;
  const UCState *__restrict__ st = w.st[at];
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  // (whole waves turn together: the appends of a wave share their atomics)
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < w.X; base += nthreads) {
    const uint64_t xi = base + threadIdx.x;
    UCComp c;
    c.first = 0; c.N = c.KC = 0; c.root = c.flags = c.rot = c.members = c.named = 0;
    const bool mine = xi < w.X && uc_speaks<CANON>(w, st, (uint32_t)xi, c);
    uc_append(w, mine, c);
  }
}

// ---- 7 order ----------------------------------------------------------------------------------------------------
struct UCOut {
  uint64_t nU;
  int64_t nN_out;
  uint32_t *iota, *rank, *s_rot;      // [nU]: the sort's payload; a component's place; the cut, in output order
  int64_t *len64, *st64;              // [nU + 1]: bytes with the terminator, scanned
  int64_t *mem64, *mbase;             // [nU + 1]: members, scanned
  uint32_t *mem_x, *mem_koff;         // [members]: the element, its k-mer offset in the component (a cycle's from the leader)
  int8_t *data_out;
  int64_t *start_out;
  int32_t *length_out;
  cfrk_unitig *rec_out;
  cfrk_unitig_pos *into;              // may be NULL
};

__global__ void uc_iota_kernel(uint32_t *idx, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) idx[i] = (uint32_t)i;
}
__global__ void uc_place_kernel(UCWork w, UCOut o, const uint32_t *__restrict__ perm) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j > o.nU) return;
  if (j == o.nU) { o.len64[j] = 0; o.mem64[j] = 0; return; }
  const uint32_t c = perm[j];
  const cfrk_unitig r = w.c_rec[c];
  o.rank[c] = (uint32_t)j;
  const int32_t len = (int32_t)(r.n_kmers + (uint32_t)w.k - 1u);
  o.length_out[j] = len;
  o.rec_out[j] = r;
  o.len64[j] = (int64_t)len + 1;
  o.mem64[j] = w.c_mem[c];
  o.s_rot[j] = w.c_rot[c];
}
__global__ void uc_starts_kernel(UCOut o) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < o.nU) o.start_out[j] = o.st64[j];
}

template <bool CANON>
__global__ __launch_bounds__(256) void uc_members_kernel(UCWork w, UCOut o, int at) {
  const UCState *__restrict__ st = w.st[at];
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  const cfrk_unitig_pos none = {CFRK_POS_NONE, CFRK_POS_NONE};
  for (uint64_t xi = tid; xi < w.X; xi += nthreads) {
    const uint32_t x = (uint32_t)xi, u = uc_u<CANON>(x), ox = uc_o<CANON>(x);
    const UCState s = st[x];
    if (s.m == UCF_DEAD) {
      if (ox == 0 && o.into) o.into[u] = none;
      continue;
    }
    const uint32_t c = w.comp_of[s.ptr];
    if (c == UC_NONE || c >= o.nU) continue;            // the mirror image is written
    const uint32_t j = o.rank[c];
    const int64_t slot = o.mbase[j] + (int64_t)s.cnt;
    if (slot >= o.mbase[j + 1]) continue;               // (never)
    o.mem_x[slot] = x;
    o.mem_koff[slot] = (uint32_t)s.acc;
    if (o.into) {
      const cfrk_unitig r = w.c_rec[c];
      uint64_t off = s.acc;
      if (r.flags & CFRK_UNITIG_CIRCULAR) off = (off + r.n_kmers - w.c_rot[c]) % r.n_kmers;
      cfrk_unitig_pos p;
      p.unitig = j; p.at = ((uint32_t)off << 1) | ox;
      o.into[u] = p;
    }
  }
}

// ---- 8 emit -----------------------------------------------------------------------------------------------------
// where a lane is: unitig j = [cstart, cend) and the member in `slot` that holds k-mers [mlo, mhi) of it
struct UCCursor {
  int64_t cstart, cend, len, mbeg, mend, slot;
  uint64_t j, N, D, mlo, mhi;
  uint32_t mu, mo;
  bool circ;
};

// the last j of [lo, hi) with st64[j] <= g
__device__ __forceinline__ uint64_t uc_unitig_of(const UCOut &o, uint64_t lo, uint64_t hi, int64_t g) {
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (o.st64[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// Output byte g of [0, nN_out); the tile's bytes lie in unitigs [jlo, jhi].  A lane's bytes ascend: behind the first
// one it steps from a unitig to the next and from a member to the next and searches no more.
template <bool CANON>
__device__ __forceinline__ int uc_out_byte(const UCWork &w, const UCOut &o, UCCursor &c, int64_t g, uint64_t jlo, uint64_t jhi) {
  const int k = w.k;
  if (g >= c.cend) {
    const uint64_t j = c.cend >= 0 && g == c.cend && c.j + 1 < o.nU ? c.j + 1 : uc_unitig_of(o, jlo, jhi + 1, g);
    const cfrk_unitig r = o.rec_out[j];
    c.j = j; c.cstart = o.st64[j]; c.len = o.length_out[j]; c.cend = c.cstart + c.len + 1;
    c.N = r.n_kmers; c.circ = (r.flags & CFRK_UNITIG_CIRCULAR) != 0; c.D = o.s_rot[j];
    c.mbeg = o.mbase[j]; c.mend = o.mbase[j + 1];
    c.mlo = 1; c.mhi = 0; c.slot = -1;
  }
  const int64_t p = g - c.cstart;
  if (p >= c.len) return -1;                             // the terminator
  uint64_t q = p >= k - 1 ? (uint64_t)(p - (k - 1)) : 0; // the k-mer that brings base p, and which of its bases
  const int64_t b = p - (int64_t)q;
  if (c.circ) { q += c.D; if (q >= c.N) q -= c.N; }
  if (q < c.mlo || q >= c.mhi) {
    int64_t lo = c.mbeg, hi = c.mend;                    // the last slot with mem_koff <= q
    if (hi <= lo) return 0;                              // (never)
    if (q == 0) hi = lo + 1;                             // the first member (also where a cycle wraps)
    else if (c.slot >= 0 && q == c.mhi && c.slot + 1 < c.mend) { lo = c.slot + 1; hi = lo + 1; }
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (o.mem_koff[mid] <= q) lo = mid; else hi = mid;
    }
    const uint32_t x = o.mem_x[lo];
    c.slot = lo; c.mu = uc_u<CANON>(x); c.mo = uc_o<CANON>(x);
    c.mlo = o.mem_koff[lo]; c.mhi = c.mlo + w.rec[c.mu].n_kmers;
    if (q < c.mlo || q >= c.mhi) { c.mlo = 1; c.mhi = 0; c.slot = -1; return 0; }   // (never)
  }
  return uc_base(w, c.mu, c.mo, (int64_t)(q - c.mlo) + b);
}

template <bool CANON>
__global__ __launch_bounds__(256) void uc_emit_kernel(UCWork w, UCOut o, uint64_t ntiles, uint32_t skew) {
  __shared__ uint64_t s_j[2];                            // the unitigs of the tile's first and last byte: 16 bytes of LDS
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t t0 = (int64_t)(tile * UC_TILE) - (int64_t)skew;
    __syncthreads();                                     // (the last tile's s_j has been read)
    if (threadIdx.x < 2) {
      const int64_t g = threadIdx.x ? min(t0 + UC_TILE - 1, o.nN_out - 1) : max(t0, (int64_t)0);
      s_j[threadIdx.x] = uc_unitig_of(o, 0, o.nU, g);
    }
    __syncthreads();
    const uint64_t jlo = s_j[0], jhi = s_j[1];
    const int64_t g0 = t0 + (int64_t)threadIdx.x * 16;
    if (g0 >= o.nN_out || g0 + 16 <= 0) continue;
    UCCursor c;
    c.cstart = 0; c.cend = -1; c.len = 0; c.mbeg = c.mend = 0; c.slot = -1; c.j = 0; c.N = 1; c.D = 0; c.mlo = 1; c.mhi = 0;
    c.mu = c.mo = 0; c.circ = false;
    const bool whole = g0 >= 0 && g0 + 16 <= o.nN_out;
    uint64_t w0 = 0, w1 = 0;                             // the lane's 16 bytes, the first in the lowest bits
#pragma unroll 1
    for (int i = 0; i < 16; ++i) {
      const int64_t g = g0 + i;
      if (g < 0 || g >= o.nN_out) continue;
      const int v = uc_out_byte<CANON>(w, o, c, g, jlo, jhi);
      if (!whole) { o.data_out[g] = (int8_t)v; continue; }
      const uint64_t sh = (uint64_t)(uint8_t)v << ((i & 7) * 8);
      if (i < 8) w0 |= sh; else w1 |= sh;
    }
    // (aligned: the tiles lie on the 16-byte grid of data_out's address, see the launch)
    if (whole) *reinterpret_cast<uint4 *>(o.data_out + g0) = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
  }
}

// ---- host side --------------------------------------------------------------------------------------------------
int uc_rounds(uint64_t nS) {
  int r = 0;
  while ((1ull << r) < nS) ++r;
  return r;
}

// the work slot carved for nS unitigs: the same offsets in both steps
int uc_carve(cfrk_ctx *ctx, bool canon, uint64_t nS, int64_t n_links, UCWork *w, void **scan_tmp, size_t *in_scan, size_t *w_scan) {
  const uint64_t X = canon ? 2 * nS : nS;
  *in_scan = *w_scan = 0;
  if (const int rc = ug_scan_bytes(ctx, canon, nS, in_scan)) return rc;
  HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, *w_scan, (unsigned long long *)nullptr, (size_t)(X + 1), ctx->stream));
  const uint64_t in_n = canon ? 0 : nS;
  Carve c;
  const size_t o_ctr = c.part(UCC_WORDS * 8), o_nxt = c.part(X * 4), o_prv = c.part(X * 4), o_s0 = c.part(X * sizeof(UCState)),
               o_s1 = c.part(X * sizeof(UCState)), o_woff = c.part((X + 1) * 8), o_chi = c.part(X * 8), o_clo = c.part(X * 8),
               o_cpos = c.part(X * 8), o_lo = c.part(nS * 8), o_hi = c.part(nS * 8), o_rec = c.part(nS * sizeof(cfrk_unitig)),
               o_root = c.part(nS * 4), o_rot = c.part(nS * 4), o_mem = c.part(nS * 4), o_comp = c.part(X * 4),
               o_off = c.part(canon ? 0 : (in_n + 1) * 8), o_cur = c.part(in_n * 4), o_src = c.part(canon ? 0 : (size_t)n_links * 4),
               o_tmp = c.part(std::max(*in_scan, *w_scan));
  void *base;
  if (const int rc = cfrk_pool_get(ctx, BUF_UNITIG_COMPACT, c.end, &base)) return rc;
  w->X = X;
  w->ctr = carve_at<unsigned long long>(base, o_ctr);
  w->nxt = carve_at<uint32_t>(base, o_nxt); w->prv = carve_at<uint32_t>(base, o_prv);
  w->st[0] = carve_at<UCState>(base, o_s0); w->st[1] = carve_at<UCState>(base, o_s1);
  w->woff = carve_at<unsigned long long>(base, o_woff);
  w->cmin_hi = carve_at<unsigned long long>(base, o_chi); w->cmin_lo = carve_at<unsigned long long>(base, o_clo);
  w->cpos = carve_at<unsigned long long>(base, o_cpos);
  w->c_lo = carve_at<uint64_t>(base, o_lo); w->c_hi = carve_at<uint64_t>(base, o_hi); w->c_rec = carve_at<cfrk_unitig>(base, o_rec);
  w->c_root = carve_at<uint32_t>(base, o_root); w->c_rot = carve_at<uint32_t>(base, o_rot); w->c_mem = carve_at<uint32_t>(base, o_mem);
  w->comp_of = carve_at<uint32_t>(base, o_comp);
  w->in_off = carve_at<unsigned long long>(base, o_off);
  w->in_cur = carve_at<uint32_t>(base, o_cur);
  w->in_src = carve_at<uint32_t>(base, o_src);
  *scan_tmp = carve_at<void>(base, o_tmp);
  return CFRK_OK;
}

void uc_fill_work(const cfrk_ctx *ctx, UCWork *w, const cfrk_unitigs_in &in) {
  w->rec = in.rec; w->ptr = in.link_ptr; w->links = in.links; w->nS = (uint64_t)in.nS; w->n_links = in.n_links;
  w->data = in.data; w->start = in.start; w->length = in.length; w->drop = in.drop; w->nN = in.nN; w->k = ctx->g_k;
}

int uc_layout_error(cfrk_ctx *ctx, unsigned long long word) {
  const unsigned long long j = word >> 8;
  const int why = (int)(word & 255);
  if (why < UCE_SHORT) return ug_layout_error(ctx, word);
  const char *what = why == UCE_SHORT     ? "is shorter than k"
                     : why == UCE_KMERS   ? "has a length that is not n_kmers + k - 1"
                     : why == UCE_RANGE   ? "lies outside [0, nN)"
                     : why == UCE_ORDER   ? "starts before the end of its predecessor"
                     : why == UCE_OVERLAP ? "does not overlap the unitig it merges with in k - 1 bases"
                                          : "heads a component of more than 2^31 - 1 bases";
  return cfrk_fail(ctx, CFRK_ERR_LAYOUT, "unitig %llu %s: not the unitigs and links of one graph", j, what);
}

}  // namespace

// Passes 1 .. 6 and the synchronisation: the components and their bytes.  1 <= nS < 2^31.
int cfrk_unitigs_compact_measure(cfrk_ctx *ctx, const cfrk_unitigs_in &in, int64_t *nN_out, int64_t *nS_out) {
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  UCWork w;
  void *scan_tmp;
  size_t in_scan, w_scan;
  if (const int rc = uc_carve(ctx, canon, (uint64_t)in.nS, in.n_links, &w, &scan_tmp, &in_scan, &w_scan)) return rc;
  uc_fill_work(ctx, &w, in);
  HIP_TRY(ctx, hipMemsetAsync(w.ctr + UCC_NU, 0, (UCC_WORDS - UCC_NU) * 8, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w.nxt, 0xFF, w.X * 4, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w.prv, 0xFF, w.X * 4, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w.comp_of, 0xFF, w.X * 4, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w.cmin_hi, 0xFF, w.X * 8, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w.cmin_lo, 0xFF, w.X * 8, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w.cpos, 0xFF, w.X * 8, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w.woff, 0, (w.X + 1) * 8, ctx->stream));     // (an error leaves the scan zeros)
  const int gu = u_grid(ctx, w.nS), gx = u_grid(ctx, w.X);
  if (const int rc = ug_check_launch(ctx, w, canon, gu, scan_tmp, in_scan)) return rc;
  hipLaunchKernelGGL(uc_layout_kernel, dim3(gu), dim3(256), 0, ctx->stream, w);
  const int rounds = uc_rounds(w.nS), at = rounds & 1;
#define UC_LAUNCH(KERNEL, ...)                                                                                          \
  do {                                                                                                                  \
    if (canon) hipLaunchKernelGGL((KERNEL<true>), dim3(gx), dim3(256), 0, ctx->stream, __VA_ARGS__);                    \
    else hipLaunchKernelGGL((KERNEL<false>), dim3(gx), dim3(256), 0, ctx->stream, __VA_ARGS__);                         \
  } while (0)
  UC_LAUNCH(uc_next_kernel, w);
  UC_LAUNCH(uc_rank_init_kernel, w);
  for (int r = 0; r < rounds; ++r) hipLaunchKernelGGL(uc_rank_kernel, dim3(gx), dim3(256), 0, ctx->stream, w, r);
  UC_LAUNCH(uc_finish_kernel, w, at);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(scan_tmp, w_scan, w.woff, (size_t)(w.X + 1), ctx->stream));
  if (canon) {
    hipLaunchKernelGGL((uc_cycle_min_kernel<true, 0>), dim3(gx), dim3(256), 0, ctx->stream, w, at);
    hipLaunchKernelGGL((uc_cycle_min_kernel<true, 1>), dim3(gx), dim3(256), 0, ctx->stream, w, at);
    hipLaunchKernelGGL((uc_cycle_min_kernel<true, 2>), dim3(gx), dim3(256), 0, ctx->stream, w, at);
  } else {
    hipLaunchKernelGGL((uc_cycle_min_kernel<false, 0>), dim3(gx), dim3(256), 0, ctx->stream, w, at);
    hipLaunchKernelGGL((uc_cycle_min_kernel<false, 1>), dim3(gx), dim3(256), 0, ctx->stream, w, at);
    hipLaunchKernelGGL((uc_cycle_min_kernel<false, 2>), dim3(gx), dim3(256), 0, ctx->stream, w, at);
  }
  UC_LAUNCH(uc_choose_kernel, w, at);
  HIP_TRY(ctx, hipGetLastError());
  unsigned long long h[UCC_WORDS];
  HIP_TRY(ctx, hipMemcpyAsync(h, w.ctr, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (h[UCC_ERR] != UG_NONE) return uc_layout_error(ctx, h[UCC_ERR]);
  *nN_out = (int64_t)h[UCC_BYTES];
  *nS_out = (int64_t)std::min<unsigned long long>(h[UCC_NU], w.nS);
  return CFRK_OK;
}

// Passes 7 and 8, left enqueued, behind a measure of the same arguments that returned CFRK_OK with nS_out >= 1.
int cfrk_unitigs_compact_emit(cfrk_ctx *ctx, const cfrk_unitigs_in &in, int8_t *d_data, int64_t *d_start, int32_t *d_length,
                              cfrk_unitig *d_rec, cfrk_unitig_pos *d_into, int64_t nN_out, int64_t nS_out) {
  const bool canon = (ctx->g_flags & CFRK_CANONICAL) != 0;
  UCWork w;
  void *scan_tmp;
  size_t in_scan, w_scan;
  int rc = uc_carve(ctx, canon, (uint64_t)in.nS, in.n_links, &w, &scan_tmp, &in_scan, &w_scan);
  if (rc) return rc;
  uc_fill_work(ctx, &w, in);
  const int at = uc_rounds(w.nS) & 1;
  const uint64_t n = (uint64_t)nS_out;
  size_t o_scan = 0;
  HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, o_scan, (const int64_t *)nullptr, (int64_t *)nullptr, (size_t)(n + 1), ctx->stream));
  Carve c;
  const size_t o_iota = c.part(n * 4), o_rank = c.part(n * 4), o_rot = c.part(n * 4), o_len = c.part((n + 1) * 8), o_st = c.part((n + 1) * 8),
               o_m64 = c.part((n + 1) * 8), o_mb = c.part((n + 1) * 8), o_mx = c.part(w.nS * 4), o_mk = c.part(w.nS * 4), o_tmp = c.part(o_scan);
  void *aux;
  if ((rc = cfrk_pool_get(ctx, BUF_UNITIG_COMPACT_AUX, c.end, &aux))) return rc;
  UCOut o;
  o.nU = n; o.nN_out = nN_out;
  o.iota = carve_at<uint32_t>(aux, o_iota); o.rank = carve_at<uint32_t>(aux, o_rank); o.s_rot = carve_at<uint32_t>(aux, o_rot);
  o.len64 = carve_at<int64_t>(aux, o_len); o.st64 = carve_at<int64_t>(aux, o_st);
  o.mem64 = carve_at<int64_t>(aux, o_m64); o.mbase = carve_at<int64_t>(aux, o_mb);
  o.mem_x = carve_at<uint32_t>(aux, o_mx); o.mem_koff = carve_at<uint32_t>(aux, o_mk);
  o.data_out = d_data; o.start_out = d_start; o.length_out = d_length; o.rec_out = d_rec; o.into = d_into;
  const unsigned nb = (unsigned)((n + 1 + 255) / 256);
  hipLaunchKernelGGL(uc_iota_kernel, dim3(nb), dim3(256), 0, ctx->stream, o.iota, n);
  const uint64_t *s_lo, *s_hi;
  const uint32_t *perm;
  if ((rc = cfrk_sort_export(ctx, w.c_lo, w.k > 32 ? w.c_hi : nullptr, o.iota, n, &s_lo, &s_hi, &perm))) return rc;
  hipLaunchKernelGGL(uc_place_kernel, dim3(nb), dim3(256), 0, ctx->stream, w, o, perm);
  HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(carve_at<void>(aux, o_tmp), o_scan, (const int64_t *)o.len64, o.st64, (size_t)(n + 1), ctx->stream));
  HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(carve_at<void>(aux, o_tmp), o_scan, (const int64_t *)o.mem64, o.mbase, (size_t)(n + 1), ctx->stream));
  hipLaunchKernelGGL(uc_starts_kernel, dim3(nb), dim3(256), 0, ctx->stream, o);
  const int gx = u_grid(ctx, w.X);
  // the tiles lie on the 16-byte grid of d_data's address: tile 0 begins `skew` bytes in front of it
  const uint32_t skew = (uint32_t)((uintptr_t)d_data & 15);
  const uint64_t ntiles = ((uint64_t)nN_out + skew + UC_TILE - 1) / UC_TILE;
  const int ge = (int)std::max<uint64_t>(1, std::min<uint64_t>(ntiles, (uint64_t)ctx->num_cus * 16));
  if (canon) {
    hipLaunchKernelGGL(uc_members_kernel<true>, dim3(gx), dim3(256), 0, ctx->stream, w, o, at);
    hipLaunchKernelGGL(uc_emit_kernel<true>, dim3(ge), dim3(256), 0, ctx->stream, w, o, ntiles, skew);
  } else {
    hipLaunchKernelGGL(uc_members_kernel<false>, dim3(gx), dim3(256), 0, ctx->stream, w, o, at);
    hipLaunchKernelGGL(uc_emit_kernel<false>, dim3(ge), dim3(256), 0, ctx->stream, w, o, ntiles, skew);
  }
  HIP_TRY(ctx, hipGetLastError());
  return CFRK_OK;
}
