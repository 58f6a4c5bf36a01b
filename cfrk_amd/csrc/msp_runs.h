// msp_runs.h -- the multi-GPU exchange by runs, for both key widths.  Device side: where every leaf's rows go in the
// packed buffer (sender) and where every received segment goes in the owner's leaf streams, and the STAGES that read or
// write records -- slot ranking, twin lookup, note / record split, row claim, the sizes / gather / scatter kernels --
// templated on a description of the record format (RunsFmt1 in msp.hip: 16-byte records, one row each; RunsFmt2 in
// msp2.hip: 32-byte records, two rows each).  The wire format -- note encoding, padding, RUN_NOTED, headers, the claim
// protocol -- is written down here and nowhere else; the two files keep their dedupe kernels' complete-stream scans and
// thin __global__ wrappers that give the shared kernels their names.  Host side: the whole call sequence of the
// one-shot and the pipelined exchange -- scratch buffers, plan and layout kernels, read-backs and the checks of what
// arrived -- with the kernel launches handed in as lambdas.  Included by msp.hip and msp2.hip inside their anonymous
// namespaces; msp_shared.h holds what the two share outside the exchange.
#pragma once

constexpr uint32_t RUN_NOTED = 0xFFFFFFFFu;        // (a record's header word has the top 8 bits clear)
constexpr int NOTES_PER_ROW = 8;
__host__ __device__ constexpr uint32_t runs_note_rows(uint32_t na) { return (na + NOTES_PER_ROW - 1) / NOTES_PER_ROW; }
// Packed form, one segment per owner: [header: the owner's leaves_per_part x (distinct, truncated,
// noted) sizes, uint32 triples, padded to whole 16-byte rows][leaf after leaf: the distinct complete
// runs, the truncated runs, the notes (16 bits each, eight per row)].
static inline int runs_header_rows(int lpp) { return (lpp * 3 * (int)sizeof(uint32_t) + 15) / 16; }

// exclusive prefix sum over a block of 1024 threads (wtot: 16 words of LDS); returns the exclusive
// prefix of x, *total = the block's sum
__device__ __forceinline__ uint64_t block_scan_u64(uint64_t x, unsigned long long *wtot, uint64_t *total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint64_t incl = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t y = __shfl_up(incl, d);
    if (lane >= d) incl += y;
  }
  __syncthreads();                               // (wtot may still be read from a previous scan)
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  uint64_t base = 0, all = 0;
  for (int w = 0; w < 16; ++w) { const uint64_t t = wtot[w]; base += (w < wave) ? t : 0; all += t; }
  *total = all;
  return base + incl - x;
}

// sender: where every leaf's rows go in the packed buffer (owner-major order, a header of hrows rows in
// front of every owner's segment) and where every segment starts.  One item per thread (item i =
// (owner p, j): leaf p + j * parts), ceil(items / 1024) workgroups: a workgroup scans its 1024 sizes,
// publishes their sum and adds up the sums of the workgroups BEFORE it (they were dispatched earlier
// and wait for nobody behind them, so the wait ends whatever is resident) -- one load and one
// look-back deep, where one workgroup walked 64 items per thread three times over (0.19 ms of a
// rank's 4 ms at N = 8).  The header triples are written by the gather kernel (runs_write_header).
constexpr unsigned long long RUNS_PLAN_READY = 1ull << 63;
__global__ __launch_bounds__(1024) void msp_runs_plan_kernel(const uint4 *__restrict__ sz, int parts, int lpp, int hrows,
                                                             uint64_t *__restrict__ dst_off,
                                                             uint64_t *__restrict__ all_rows /* rows of the whole buffer */,
                                                             uint64_t *__restrict__ seg_start /* [parts]: first row of every segment */,
                                                             unsigned long long *__restrict__ sync /* [gridDim.x], zeroed */) {
  __shared__ unsigned long long wtot[16];
  __shared__ unsigned long long before;
  const int tid = threadIdx.x, b = (int)blockIdx.x;
  const int n = parts * lpp;
  const int i = b * 1024 + tid, p = i / lpp, j = i - p * lpp, leaf = p + j * parts;
  uint32_t r = 0u;
  if (i < n && leaf < NLEAF) r = sz[leaf].w;
  uint64_t total;
  const uint64_t excl = block_scan_u64(r, wtot, &total);
  if (tid == 0) __hip_atomic_store(&sync[b], RUNS_PLAN_READY | total, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  if (tid < 64) {                                   // (at most 65 workgroups: parts * ceil(65536 / parts) <= 65536 + 63 items)
    unsigned long long x = 0ull;
    if (tid < b) {
      do x = __hip_atomic_load(&sync[tid], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT); while (!(x & RUNS_PLAN_READY));
      x &= ~RUNS_PLAN_READY;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    if (tid == 0) before = x;
  }
  __syncthreads();
  const uint64_t run = before + excl;
  if (i < n) {
    if (j == 0) seg_start[p] = run + (uint64_t)p * hrows;         // (a segment starts with the first item of its owner)
    if (leaf < NLEAF) dst_off[leaf] = run + (uint64_t)(p + 1) * hrows;
  }
  if (b == (int)gridDim.x - 1 && tid == 0) *all_rows = before + total + (uint64_t)parts * hrows;
}
static inline unsigned runs_plan_grid(int parts, int lpp) { return (unsigned)((parts * lpp + 1023) / 1024); }

// gather kernel, one thread of the leaf's workgroup: the leaf's (distinct, truncated, noted) sizes in its owner's header
__device__ __forceinline__ void runs_write_header(uint4 *packed, const uint64_t *seg_start, int parts, uint32_t leaf,
                                                  uint32_t nd, uint32_t nu, uint32_t na) {
  const uint32_t p = leaf % (uint32_t)parts, j = leaf / (uint32_t)parts;
  uint32_t *hdr = reinterpret_cast<uint32_t *>(packed + seg_start[p]);
  hdr[3 * j] = nd; hdr[3 * j + 1] = nu; hdr[3 * j + 2] = na;
  // (parts does not divide 65536: the last entry of the last owners' headers stands for no leaf)
  const uint32_t lpp = ((uint32_t)NLEAF + (uint32_t)parts - 1u) / (uint32_t)parts;
  if (leaf + (uint32_t)parts >= (uint32_t)NLEAF && j + 1u < lpp) { hdr[3 * j + 3] = 0u; hdr[3 * j + 4] = 0u; hdr[3 * j + 5] = 0u; }
}

// (err = 1 when a rank's header does not add up to the rows it sent)
struct RunsRecv { uint64_t rstart[64]; uint64_t rows[64]; };
// owner: every rank's header says how large its leaves' segments are.  Two kernels: (1) one thread per
// local leaf reads the `parts` header triples of that leaf (coalesced across threads) and writes, per
// (rank, leaf), the segment's rows and where it goes INSIDE the leaf's two streams, and per leaf the
// stream sizes; (2) one workgroup turns those compact arrays into offsets with plain scans.  (One
// workgroup used to do all of it with dependent header loads: 0.27 ms at N = 8.)
// NC streams per leaf, CI1 / CI0: which of them take the complete / the truncated runs; RMUL rows per record
template <int NC, int CI1, int CI0, int RMUL>
__global__ __launch_bounds__(256) void msp_runs_layout1_kernel(const uint4 *__restrict__ packed, RunsRecv rr, int parts, int lpp,
                                                                uint32_t *__restrict__ rows /* [parts][lpp] */,
                                                                uint64_t *__restrict__ d1 /* relative */, uint64_t *__restrict__ d0 /* relative */,
                                                                uint32_t *__restrict__ lcap, uint64_t *__restrict__ out) {
  const int ll = blockIdx.x * 256 + threadIdx.x;
  if (ll >= lpp) return;
  uint64_t n1 = 0, n0 = 0;
  uint32_t err = 0;
  // (the complete streams of all ranks first, then the truncated ones: rank order inside both)
  for (int r = 0; r < parts; ++r) {
    const uint32_t *hdr = reinterpret_cast<const uint32_t *>(packed + rr.rstart[r]);
    const uint32_t a = hdr[3 * ll], b = hdr[3 * ll + 1], c = hdr[3 * ll + 2];
    rows[(size_t)r * lpp + ll] = (uint32_t)RMUL * (a + b) + runs_note_rows(c);
    if (c && !a) err = 1;                                      // notes without a run they could point at
    d1[(size_t)r * lpp + ll] = n1;
    n1 += a;
  }
  for (int r = 0; r < parts; ++r) {
    const uint32_t *hdr = reinterpret_cast<const uint32_t *>(packed + rr.rstart[r]);
    d0[(size_t)r * lpp + ll] = n1 + n0;
    n0 += (uint64_t)hdr[3 * ll + 1] + hdr[3 * ll + 2];         // (a note becomes a record again)
  }
  if (n1 > 0xFFFFFFFFull || n0 > 0xFFFFFFFFull) err = 1;
  lcap[(size_t)NC * ll + CI1] = (uint32_t)n1;
  lcap[(size_t)NC * ll + CI0] = (uint32_t)n0;
  if (err) out[1] = 1;
}

// parts + 1 workgroups: workgroup r < parts scans rank r's segment sizes, the last one the leaves' stream sizes
template <int NC, int CI1, int CI0>
__global__ __launch_bounds__(1024) void msp_runs_layout_kernel(RunsRecv rr, int parts, int lpp, int hrows,
                                                               const uint32_t *__restrict__ rows,
                                                               uint64_t *__restrict__ src, uint64_t *__restrict__ d1, uint64_t *__restrict__ d0,
                                                               uint64_t *__restrict__ lbase, const uint32_t *__restrict__ lcap, uint32_t *__restrict__ cnt2,
                                                               uint64_t *__restrict__ out /* [0]: records in all, [1]: err */) {
  __shared__ unsigned long long wtot[16];
  const int tid = threadIdx.x;
  const int per = (lpp + 1023) / 1024;
  if ((int)blockIdx.x < parts) {
    // (1) rank r's segments: record offsets inside its part of the buffer
    const int r = (int)blockIdx.x;
    uint64_t mine = 0;
    for (int q = 0; q < per; ++q) {
      const int ll = tid * per + q;
      if (ll < lpp) mine += rows[(size_t)r * lpp + ll];
    }
    uint64_t total;
    uint64_t run = block_scan_u64(mine, wtot, &total);
    if (total + (uint64_t)hrows != rr.rows[r]) out[1] = 1;
    for (int q = 0; q < per; ++q) {
      const int ll = tid * per + q;
      if (ll >= lpp) break;
      src[(size_t)r * lpp + ll] = rr.rstart[r] + (uint64_t)hrows + run;
      run += rows[(size_t)r * lpp + ll];
    }
    return;
  }
  // (2) the owner's leaves = local indices: stream (ll, class) = the ranks' parts in rank order, complete stream first
  uint64_t mine = 0;
  for (int q = 0; q < per; ++q) {
    const int ll = tid * per + q;
    if (ll < lpp) mine += (uint64_t)lcap[(size_t)NC * ll + CI0] + lcap[(size_t)NC * ll + CI1];
  }
  uint64_t total;
  uint64_t run = block_scan_u64(mine, wtot, &total);
  for (int q = 0; q < per; ++q) {
    const int ll = tid * per + q;
    if (ll >= lpp) break;
    const uint32_t n1 = lcap[(size_t)NC * ll + CI1], n0 = lcap[(size_t)NC * ll + CI0];
    for (int r = 0; r < parts; ++r) {              // relative -> absolute
      d1[(size_t)r * lpp + ll] += run;
      d0[(size_t)r * lpp + ll] += run;
    }
    lbase[(size_t)NC * ll + CI1] = run; cnt2[(size_t)NC * ll + CI1] = n1;
    lbase[(size_t)NC * ll + CI0] = run + n1; cnt2[(size_t)NC * ll + CI0] = n0;
    run += (uint64_t)n1 + n0;
  }
  if (tid == 0) out[0] = total;
}

// ------------------------------------------------------------------- the PIPELINED exchange (round 5), both key widths
// Sender: the leaves of an owner are cut into `ngroups` ranges of local indices; group g of owner p has its segment at
// rows [(g * parts + p) * seg_cap, ...) of the send buffer: header (row 0 = {rows used, leaves, first local leaf, magic},
// written by msp_runs_group_finish_kernel; then one uint4 {row offset, distinct, truncated, noted} per local leaf)
// followed by the leaves' rows in the order their workgroups CLAIM them (one atomic on the segment's cursor per leaf).
struct RunsSend {
  uint4 *packed;             // this GROUP's segments: owner p's at packed + p * seg_cap
  uint64_t seg_cap;          // rows per segment (header included)
  uint32_t *cursor;          // [parts] rows claimed behind the header (zeroed before the kernel)
  uint32_t leaf0, nleaf;     // the group's leaves [leaf0, leaf0 + nleaf): all owners' local leaves [ll0, ll0 + lcount)
  uint32_t ll0, lcount;
  int parts;
};
// Owner: the leaf kernel reads the N lists of a leaf IN PLACE from the receive buffer (msp.hip: p3_body, msp2.hip: q3_body)
template <bool LISTS> struct P3ListsT {};
template <> struct P3ListsT<true> {
  const uint4 *packed;       // the receive buffer of this group: rank r's segment at row rr.rstart[r], rr.rows[r] rows
  RunsRecv rr;
  int parts;
  uint32_t ll0, lcount;      // the group's local leaves [ll0, ll0 + lcount): workgroup b counts local leaf ll0 + b
};
constexpr uint32_t RUNS2_MAGIC = 0x32535543u;   // "CUS2"

static inline uint32_t runs_ll0(int lpp, int g, int ngroups) { return (uint32_t)(((int64_t)lpp * g) / ngroups); }

// ... and the group's epilogue: row 0 of every segment's header, the rows every segment uses, the job's flags
__global__ __launch_bounds__(64) void msp_runs_group_finish_kernel(RunsSend sg, const uint64_t *__restrict__ stats, uint64_t *__restrict__ used /* [parts + 1] */) {
  const int p = threadIdx.x;
  if (p < sg.parts) {
    const uint64_t u = 1ull + sg.lcount + (uint64_t)sg.cursor[p];
    used[p] = u;
    sg.packed[(uint64_t)p * sg.seg_cap] = make_uint4((uint32_t)min(u, (uint64_t)0xFFFFFFFFull), sg.lcount, sg.ll0, RUNS2_MAGIC);
  }
  if (p == 0) used[sg.parts] = (stats[ST_SPILLED] || stats[ST_ONES] || stats[ST_L1OVF] || stats[ST_L2OVF] || stats[ST_OVFN] ||
                                stats[ST_OVFN1] || stats[ST_CWRAP] || stats[ST_OVERFLOW]) ? 1ull : 0ull;
}

// ------------------------------------------------------------------- the stages that read or write records
// F: the record format (RunsFmt1, RunsFmt2) -- F::Rec, F::View, F::ROWS rows per record, F::NC stream classes per leaf of
// which F::COMPLETE holds the complete runs, F::count / F::stream / F::trunc (the truncated streams, concatenated),
// header and note words, F::slot / F::revcomp / F::prefix_equal / F::prefix, records as rows of the packed buffer.
// A NOTE is 16 bits: position of the twin in the leaf's list << 5 | n-1; 0xFFFF pads the last row and never is a note.
constexpr uint32_t RUNS_NO_NOTE = 0xFFFFu, RUNS_NO_TWIN = 0xFFFFFFFFu, RUNS_NO_ROOM = 0xFFFFFFFFu;

// rank the occupied slots of a record table of PER * THREADS slots, thread t looking at slots [PER t, PER t + PER):
// sidx[slot] = position in the leaf's list, *total = the list's length; returns the position of the thread's first
// occupied slot.  (One barrier inside; wsum: a word per wave.  The caller's barrier makes sidx visible.)
template <int THREADS, int PER, class Occ>
__device__ __forceinline__ uint32_t runs_rank_slots(uint16_t *sidx, uint32_t *wsum, Occ occupied, uint32_t *total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t mine = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) mine += occupied(PER * tid + i) ? 1u : 0u;
  const uint32_t incl = dev_wave_scan_incl(mine);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint32_t base = 0, all = 0;
  for (int w = 0; w < THREADS / 64; ++w) { const uint32_t x = wsum[w]; base += (w < wave) ? x : 0u; all += x; }
  const uint32_t at0 = base + incl - mine;
  uint32_t at = at0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    sidx[PER * tid + i] = (uint16_t)at;
    if (occupied(PER * tid + i)) ++at;
  }
  *total = all;
  return at0;
}
// ... and the occupied slots, in that order: put(position, entry) from at0 on -- to rows of the packed buffer, or to the
// head of the leaf's own stream.  (Two passes over LDS: an array of entries would live in scratch memory.)
template <int PER, class Occ, class Get, class Put>
__device__ __forceinline__ void runs_emit_slots(uint32_t at0, Occ occupied, Get get, Put put) {
  uint32_t at = at0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const uint32_t s = PER * threadIdx.x + i;
    if (occupied(s)) put(at++, get(s));
  }
}

// Is truncated run `rec` a prefix of a distinct complete run of this rank (a suffix, read on the other strand; canonical
// counting only)?  Looked up in the record table of 2^LOG slots (get(slot): the entry) exactly as the leaf kernel anchors
// it: from the slot of its first k-mer, at most 32 trips, an entry at least as long whose first n + k - 1 bases agree.
// Returns the twin's slot or RUNS_NO_TWIN; *nm1 = the run's n-1.
template <class F, int LOG, class Get>
__device__ __forceinline__ uint32_t runs_find_twin(typename F::Rec rec, bool valid, int k, int canon, Get get, uint32_t *nm1_out) {
  constexpr uint32_t MASK = (1u << LOG) - 1u;
  const uint32_t w = F::hdr(rec), nm1 = w & 31u;
  const bool lc = (w & 64u) != 0u, rc_ = (w & 128u) != 0u;
  const bool suf = canon && valid && !lc && rc_;
  if (suf) rec = F::revcomp(rec, (int)nm1 + k);
  const bool anchored = suf || (valid && lc && !rc_);
  uint32_t h = anchored ? F::slot(rec, k, LOG) : F::DONE;
  uint32_t found = RUNS_NO_TWIN;
  for (int it = 0; it < 32 && __ballot((int32_t)h >= 0); ++it) {
    const bool p = (int32_t)h >= 0;
    const uint32_t hh = h & MASK;
    const typename F::Rec e = get(hh);
    const bool empty = F::hdr(e) == F::EMPTY;
    const bool hit = p && !empty && (F::hdr(e) & 31u) >= nm1 && F::prefix_equal(e, rec, (int)nm1 + k);
    found = hit ? hh : found;
    h = (p && !hit && !empty) ? ((hh + 1u) & MASK) : (h | F::DONE);
  }
  *nm1_out = nm1;
  return found;
}
// the first n truncated runs of a leaf: out(g, valid, note) with the note of run g, RUNS_NO_NOTE where it has no twin
// (or one beyond list position pos_max, which a note cannot name); *noted += the notes.  INFL runs per thread are asked
// for before the first is looked up.
template <class F, int THREADS, int INFL, int LOG, class Get, class Out>
__device__ __forceinline__ void runs_note_truncated(const typename F::Trunc &tr, uint64_t n, int k, int canon, const uint16_t *sidx,
                                                    uint32_t pos_max, Get get, uint32_t *noted, Out out) {
  const int tid = threadIdx.x;
  for (uint64_t g0 = 0; g0 < n; g0 += (uint64_t)INFL * THREADS) {
    typename F::Rec recs[INFL];
#pragma unroll
    for (int u = 0; u < INFL; ++u) {
      const uint64_t g = g0 + (uint64_t)u * THREADS + tid;
      recs[u] = F::zero();
      if (g < n) recs[u] = F::load(tr.at(g));
    }
#pragma unroll
    for (int u = 0; u < INFL; ++u) {
      const uint64_t g = g0 + (uint64_t)u * THREADS + tid;
      uint32_t nm1;
      const uint32_t found = runs_find_twin<F, LOG>(recs[u], g < n, k, canon, get, &nm1);
      const uint32_t pos = sidx[found & ((1u << LOG) - 1u)];
      const bool hit = found != RUNS_NO_TWIN && pos <= pos_max;
      out(g, g < n, hit ? ((pos << 5) | nm1) : RUNS_NO_NOTE);
      const unsigned long long hb = __ballot(hit);
      if ((tid & 63) == 0 && hb) atomicAdd(noted, (uint32_t)__popcll(hb));
    }
  }
}

// a leaf's nt truncated runs -> [the nu that travel as records, at rows dt][the na notes, NOTES_PER_ROW per row, the last
// row padded] in stream order.  note_of(i, rec): the note of run i or RUNS_NO_NOTE.  READ_FIRST: the verdict is in the
// run itself (marked in place), so the run is read into rec before note_of is asked; otherwise only the runs that travel
// as records are read.  (cu, cn: two LDS cursors, zero and visible on entry.  nu and na bound both kinds: a stream that
// changed under us cannot write outside the leaf's rows.)
template <class F, bool READ_FIRST, class NoteOf>
__device__ __forceinline__ void runs_split_truncated(const typename F::Trunc &tr, uint32_t nt, uint32_t nu, uint32_t na, uint4 *dt,
                                                     uint32_t *cu, uint32_t *cn, uint32_t threads, NoteOf note_of) {
  const int tid = threadIdx.x, lane = tid & 63;
  uint16_t *const notes = reinterpret_cast<uint16_t *>(dt + (uint64_t)F::ROWS * nu);
  for (uint32_t i = tid; i < ((nt + 63u) & ~63u); i += threads) {
    const bool valid = i < nt;
    typename F::Rec rec = F::zero();
    if (READ_FIRST && valid) rec = F::load(tr.at(i));
    const uint32_t note = valid ? note_of(i, rec) : RUNS_NO_NOTE;
    const bool isn = note != RUNS_NO_NOTE;
    const unsigned long long mn = __ballot(isn), mu = __ballot(valid && !isn);
    uint32_t bn = 0, bu = 0;
    if (lane == 0) {
      if (mn) bn = atomicAdd(cn, (uint32_t)__popcll(mn));
      if (mu) bu = atomicAdd(cu, (uint32_t)__popcll(mu));
    }
    bn = __shfl(bn, 0); bu = __shfl(bu, 0);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (isn) { const uint32_t at = bn + (uint32_t)__popcll(mn & below); if (at < na) notes[at] = (uint16_t)note; }
    else if (valid) {
      const uint32_t at = bu + (uint32_t)__popcll(mu & below);
      if (at < nu) { if (!READ_FIRST) rec = F::load(tr.at(i)); F::store_row(dt, at, rec); }
    }
  }
  const uint32_t pad = (NOTES_PER_ROW - na % NOTES_PER_ROW) % NOTES_PER_ROW;
  if ((uint32_t)tid < pad) notes[na + tid] = (uint16_t)RUNS_NO_NOTE;
}

// pipelined sender, one thread of the leaf's workgroup: claim the leaf's rows behind the header of its owner's segment
// (one atomic) and write the leaf's header entry; returns the first row or RUNS_NO_ROOM.  A segment that runs out of
// room shows in its cursor -- used rows > seg_cap -- and the host takes the classic exchange instead; so does a flood
// whose rows no segment can hold (seg_cap <= 0xFFFFFFF0: runs_export_async_host), which is not claimed at all.
template <class F>
__device__ __forceinline__ uint32_t runs_claim_rows(const RunsSend &sg, uint32_t own, uint4 *entry, uint32_t hrows,
                                                    uint32_t nd, uint32_t nu, uint32_t na) {
  const uint64_t rows = (uint64_t)F::ROWS * ((uint64_t)nd + nu) + runs_note_rows(na);
  const bool unclaimable = rows >= 0xFFFFFFF0ull;
  const uint32_t claim = unclaimable ? 0xFFFFFFFFu : (uint32_t)rows;
  const uint32_t pos = atomicAdd(&sg.cursor[own], claim);
  const bool fits = !unclaimable && (uint64_t)pos + rows <= sg.seg_cap - hrows && pos + claim >= pos;
  if (!fits) atomicMax(&sg.cursor[own], 0xFFFFFFF0u);              // (stays "too many" whatever is added later)
  *entry = fits ? make_uint4(pos, nd, nu, na) : make_uint4(0u, 0u, 0u, 0u);
  return fits ? pos : RUNS_NO_ROOM;
}

// pipelined sender, a leaf that was not deduplicated: its n1 complete runs with multiplicity 1 and its nt truncated runs
// as they are, no notes
template <class F, int THREADS>
__device__ __forceinline__ void runs_write_plain(uint4 *dst, const typename F::Rec *c1, uint32_t n1, const typename F::Trunc &tr, uint32_t nt) {
  for (uint32_t i = threadIdx.x; i < n1; i += THREADS) {
    typename F::Rec r = F::load(c1 + i);
    F::set_hdr(&r, (1u << 6) | (F::hdr(r) & 63u));
    F::store_row(dst, i, r);
  }
  uint4 *const dt = dst + (uint64_t)F::ROWS * n1;
  for (uint32_t i = threadIdx.x; i < nt; i += THREADS) F::store_row(dt, i, F::load(tr.at(i)));
}

// one-shot sender: what every leaf contributes -- n1 distinct complete runs, nt truncated runs as records, na as
// notes, rows in all -- one thread per leaf, coalesced (the plan kernel used to gather these four words per leaf
// itself, three times over, 64 dependent strided loads per thread each time: 0.50 ms of a 5.9 ms critical path at N = 8)
template <class F>
__device__ __forceinline__ void runs_sizes(const typename F::View &v, uint4 *__restrict__ sz, unsigned long long *__restrict__ plan_sync) {
  const uint32_t leaf = blockIdx.x * 256u + threadIdx.x;
  if (leaf < 72u) plan_sync[leaf] = 0ull;                      // (the plan kernel's look-back words)
  if (leaf >= (uint32_t)NLEAF) return;
  uint32_t n1 = 0, na = 0;
  uint32_t nt = (uint32_t)F::trunc(v, leaf).n;
  if (v.cnt2[F::NC * leaf + F::COMPLETE]) {                    // (a leaf without complete runs never wrote its counts)
    n1 = v.leaf_n[leaf];
    na = min((uint32_t)v.leaf_off[leaf], nt);
  }
  nt -= na;
  sz[leaf] = make_uint4(n1, nt, na, (uint32_t)F::ROWS * (n1 + nt) + runs_note_rows(na));
}

// one-shot sender: leaf -> [nd distinct complete runs][nu truncated runs][na notes] at row dst_off[leaf] of the send
// buffer (the truncated streams hold records and noted records mixed: msp_dedupe_export_kernel and its two-word twin
// mark a noted record in place, header word = RUN_NOTED, the note parked in F::note)
template <class F>
__device__ __forceinline__ void runs_gather(const typename F::View &v, const uint64_t *__restrict__ dst_off, uint4 *__restrict__ out,
                                            const uint64_t *__restrict__ plan_rows, const uint64_t *__restrict__ seg_start, int parts,
                                            uint64_t cap_rows, uint32_t *cu, uint32_t *cn) {
  if (plan_rows[parts] > cap_rows) return;         // the buffer is too small: nothing was planned
  const uint32_t leaf = blockIdx.x;
  const bool has1 = v.cnt2[F::NC * leaf + F::COMPLETE] != 0u;
  const uint32_t nd = has1 ? v.leaf_n[leaf] : 0u;
  const typename F::Trunc tr = F::trunc(v, leaf);
  const uint32_t nt = (uint32_t)tr.n;
  const uint32_t na = has1 ? min((uint32_t)v.leaf_off[leaf], nt) : 0u;
  const uint32_t nu = nt - na;
  if (threadIdx.x == 0) runs_write_header(out, seg_start, parts, leaf, nd, nu, na);
  const typename F::Rec *c1 = F::stream(v, leaf, F::COMPLETE);
  uint4 *dst = out + dst_off[leaf];
  for (uint32_t i = threadIdx.x; i < nd; i += blockDim.x) F::store_row(dst, i, F::load(c1 + i));
  uint4 *dt = dst + (uint64_t)F::ROWS * nd;
  if (na == 0u) {
    for (uint32_t i = threadIdx.x; i < nt; i += blockDim.x) F::store_row(dt, i, F::load(tr.at(i)));
    return;
  }
  if (threadIdx.x == 0) { *cu = 0u; *cn = 0u; }
  __syncthreads();
  runs_split_truncated<F, true>(tr, nt, nu, na, dt, cu, cn, blockDim.x, [](uint32_t, const typename F::Rec &r) {
    return F::hdr(r) == RUN_NOTED ? (F::note(r) & 0xFFFFu) : RUNS_NO_NOTE;
  });
}

// owner: segment (source rank, local leaf) of the received buffer -> its place in the leaf's complete stream and its
// (one) stream of truncated runs.  A note becomes the run it stands for: the first n k-mers of its twin, closed on the
// left only (a prefix -- of the twin as the sender stored it, whichever strand the read showed).
template <class F>
__device__ __forceinline__ void runs_scatter(const uint4 *__restrict__ in, const RunsRecv &rr, int lpp, int k, const uint64_t *__restrict__ src_off,
                                             const uint64_t *__restrict__ dst1, const uint64_t *__restrict__ dst0, typename F::Rec *__restrict__ rec2) {
  const uint32_t seg = blockIdx.x;
  const uint32_t r = seg / (uint32_t)lpp, ll = seg - r * (uint32_t)lpp;
  const uint32_t *hdr = reinterpret_cast<const uint32_t *>(in + rr.rstart[r]);
  const uint32_t nd = hdr[3 * ll], nt = hdr[3 * ll + 1], na = hdr[3 * ll + 2];
  const uint4 *src = in + src_off[seg];
  for (uint32_t i = threadIdx.x; i < nd; i += blockDim.x) F::store(&rec2[dst1[seg] + i], F::load_row(src, i));
  const uint4 *st = src + (uint64_t)F::ROWS * nd;
  for (uint32_t i = threadIdx.x; i < nt; i += blockDim.x) F::store(&rec2[dst0[seg] + i], F::load_row(st, i));
  const uint16_t *notes = reinterpret_cast<const uint16_t *>(st + (uint64_t)F::ROWS * nt);
  for (uint32_t i = threadIdx.x; i < na; i += blockDim.x) {        // (nd > 0: the layout kernel checked)
    const uint32_t note = notes[i];
    const typename F::Rec twin = F::load_row(src, min(note >> 5, nd - 1u));   // a position outside the list is not followed
    const uint32_t nm1 = min(note & 31u, F::hdr(twin) & 31u);
    F::store(&rec2[dst0[seg] + nt + i], F::prefix(twin, (int)nm1 + k, 64u | nm1));
  }
}


// host side of cfrk_global_export_runs_async for both key widths: per group, zero headers of the leaves that stand for no
// leaf, the fused dedupe + pack kernel (launch(sg)), the epilogue, the sizes to pinned memory, the group's event
template <class Launch>
static int runs_export_async_host(cfrk_ctx *ctx, void *d_packed, uint64_t seg_cap_rows, int parts, int ngroups, Launch launch) {
  const int lpp = (NLEAF + parts - 1) / parts;
  if (ngroups > lpp) return cfrk_fail(ctx, CFRK_ERR_ARG, "more groups than leaves per owner");
  if (seg_cap_rows < (uint64_t)(lpp + ngroups - 1) / ngroups + 2 || seg_cap_rows > 0xFFFFFFF0ull)
    return cfrk_fail(ctx, CFRK_ERR_ARG, "segment capacity out of range (at least a group's header: leaves per owner / groups + 2 rows)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->h_runs) HIP_TRY(ctx, hipHostMalloc((void **)&ctx->h_runs, (size_t)CFRK_RUNS_MAX_GROUPS * 65 * sizeof(uint64_t), hipHostMallocDefault));
  for (int g = 0; g < ngroups; ++g)
    if (!ctx->runs_ev[g]) HIP_TRY(ctx, hipEventCreate(&ctx->runs_ev[g]));          // (with timing: cfrk_global_runs_group_ms)
  int rc;
  void *p;
  const size_t ncur = (size_t)ngroups * parts;
  if ((rc = cfrk_pool_get(ctx, BUF_RUNS_AUX, ((ncur * sizeof(uint32_t) + 15) & ~(size_t)15) + (size_t)ngroups * 65 * sizeof(uint64_t), &p))) return rc;
  uint32_t *d_cur = (uint32_t *)p;
  uint64_t *d_used = (uint64_t *)((char *)p + ((ncur * sizeof(uint32_t) + 15) & ~(size_t)15));
  HIP_TRY(ctx, hipMemsetAsync(d_cur, 0, ncur * sizeof(uint32_t), ctx->stream));
  for (int g = 0; g < ngroups; ++g) {
    RunsSend sg;
    sg.packed = (uint4 *)d_packed + (uint64_t)g * parts * seg_cap_rows;
    sg.seg_cap = seg_cap_rows;
    sg.cursor = d_cur + (size_t)g * parts;
    sg.ll0 = runs_ll0(lpp, g, ngroups);
    sg.lcount = runs_ll0(lpp, g + 1, ngroups) - sg.ll0;
    sg.leaf0 = sg.ll0 * (uint32_t)parts;
    sg.nleaf = std::min<uint32_t>((sg.ll0 + sg.lcount) * (uint32_t)parts, (uint32_t)NLEAF) - sg.leaf0;
    sg.parts = parts;
    if (sg.nleaf < sg.lcount * (uint32_t)parts) {
      // (parts does not divide 65536: the last local leaf of the last owners stands for no leaf -- its header entry is zero)
      for (uint32_t q = sg.nleaf; q < sg.lcount * (uint32_t)parts; ++q) {
        const uint32_t leaf = sg.leaf0 + q, own = leaf % (uint32_t)parts, ll = leaf / (uint32_t)parts;
        HIP_TRY(ctx, hipMemsetAsync(sg.packed + (uint64_t)own * seg_cap_rows + 1u + (ll - sg.ll0), 0, sizeof(uint4), ctx->stream));
      }
    }
    if (sg.nleaf) {
      launch(sg);
      HIP_TRY(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(msp_runs_group_finish_kernel, dim3(1), dim3(64), 0, ctx->stream, sg, (const uint64_t *)ctx->g_stats, d_used + (size_t)g * 65);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_runs + (size_t)g * 65, d_used + (size_t)g * 65, (size_t)(parts + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->runs_ev[g], ctx->stream));
  }
  ctx->runs_groups = ngroups; ctx->runs_parts = parts; ctx->runs_seg_cap = seg_cap_rows;
  return CFRK_OK;
}

// ------------------------------------------------------------------- host side of the one-shot exchange, both key widths
// a CFRK_RUNS_DEFER add ended unsynchronised: did its regions hold?  (an add without the flag lays an overflowing level out again)
static int runs_check_deferred(cfrk_ctx *ctx, cfrk_msp *ms) {
  if (!ms->runs_unchecked) return CFRK_OK;
  uint64_t st[ST_NWORDS];
  const int rc = cfrk_msp_sync_stats(ctx, st);
  if (rc) return rc;
  if (st[ST_L1OVF] || st[ST_L2OVF] || st[ST_OVFN] || st[ST_OVFN1] || st[ST_CWRAP])
    return cfrk_fail(ctx, CFRK_ERR_STATE, "the CFRK_RUNS_DEFER add overflowed a record region: add again without the flag");
  ms->runs_unchecked = false;
  return CFRK_OK;
}

// sender: offsets, headers and segment sizes are worked out on the device; the host only learns the segment
// sizes -- together with the job's flags, in ONE copy.  launch_sizes(d_sz, d_sync): every leaf's sizes;
// launch_gather(d_off, d_rows, d_seg): the leaves' rows to where the plan put them
template <class Sizes, class Gather>
static int runs_export_host(cfrk_ctx *ctx, uint64_t cap_rows, int parts, uint64_t *part_rows, Sizes launch_sizes, Gather launch_gather) {
  const int lpp = (NLEAF + parts - 1) / parts;           // leaves per part (owner p: leaves p, p+parts, ...)
  const int hrows = runs_header_rows(lpp);
  int rc;
  void *p;
  if ((rc = cfrk_pool_get(ctx, BUF_SCRATCH, (NLEAF + 65 + ST_NWORDS + 1 + 64 + 72) * sizeof(uint64_t) + (size_t)NLEAF * sizeof(uint4), &p))) return rc;
  uint64_t *d_off = (uint64_t *)p, *d_rows = d_off + NLEAF;
  uint64_t *d_seg = d_rows + 65 + ST_NWORDS + 1;
  unsigned long long *d_sync = (unsigned long long *)(d_seg + 64);
  uint4 *d_sz = (uint4 *)(d_sync + 72);      // (16-byte aligned: the pool is, and NLEAF + 65 + ST_NWORDS + 1 is even)
  static_assert((NLEAF + 65 + ST_NWORDS + 1 + 64 + 72) % 2 == 0, "d_sz is 16-byte aligned");
  launch_sizes(d_sz, d_sync);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(msp_runs_plan_kernel, dim3(runs_plan_grid(parts, lpp)), dim3(1024), 0, ctx->stream, (const uint4 *)d_sz, parts, lpp, hrows, d_off,
                     d_rows + parts, d_seg, d_sync);
  HIP_TRY(ctx, hipGetLastError());
  launch_gather((const uint64_t *)d_off, (const uint64_t *)d_rows, (const uint64_t *)d_seg);
  HIP_TRY(ctx, hipGetLastError());
  // [0, 65): all rows at [parts]; then the job's flags; then the segment starts -- ONE copy
  uint64_t h[65 + ST_NWORDS + 1 + 64];
  HIP_TRY(ctx, hipMemcpyAsync(d_rows + 65, ctx->g_stats, ST_NWORDS * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(h, d_rows, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const uint64_t *st = h + 65, *seg = h + 65 + ST_NWORDS + 1;
  if (st[ST_SPILLED] || st[ST_ONES]) return cfrk_fail(ctx, CFRK_ERR_STATE, "part of the batch was counted in the HBM table");
  if (h[parts] > cap_rows) return cfrk_fail(ctx, CFRK_ERR_SMALL_BUF, "%llu rows, room for %llu", (unsigned long long)h[parts], (unsigned long long)cap_rows);
  for (int q = 0; q < parts; ++q) part_rows[q] = (q + 1 < parts ? seg[q + 1] : h[parts]) - seg[q];
  return CFRK_OK;
}

// rank r's rows start where rank r - 1's end; returns the rows of all ranks
static uint64_t runs_recv(RunsRecv *rr, const uint64_t *recv_rows, int parts) {
  memset(rr, 0, sizeof *rr);
  uint64_t at = 0;
  for (int r = 0; r < parts; ++r) { rr->rstart[r] = at; rr->rows[r] = recv_rows[r]; at += recv_rows[r]; }
  return at;
}

// owner: what the scatter kernel needs to copy segment (source rank, local leaf) into the leaf's streams
struct RunsPlan { RunsRecv rr; int lpp; size_t nseg; const uint64_t *src, *d1, *d0; };
// owner: the ranks' headers say how large every segment is; all offsets on the device (msp_runs_layout1_kernel,
// msp_runs_layout_kernel) into the exact layout of the leaf streams.  The headers are checked before anything is
// copied by them: sizes that add up to the rows each rank sent keep every segment inside its rank's part of the
// buffer and every stream inside rec2, which is sized here to what arrived, every note a record again.
// view(&lbase, &lcap, &cnt2): the caller sets up its view once the messages are long enough for their headers and
// hands back the streams' layout arrays (BUF_MSP_LAYOUT) and cursors
template <int NC, int CI1, int CI0, int RMUL, class Rec, class ViewSetup>
static int runs_merge_plan_host(cfrk_ctx *ctx, const void *d_packed, const uint64_t *recv_rows, int parts, ViewSetup view,
                                RunsPlan *pl, Rec **rec2) {
  const int lpp = (NLEAF + parts - 1) / parts;
  const int hrows = runs_header_rows(lpp);
  const size_t nseg = (size_t)parts * lpp;
  for (int r = 0; r < parts; ++r)
    if (recv_rows[r] < (uint64_t)hrows) return cfrk_fail(ctx, CFRK_ERR_ARG, "rank %d sent %llu rows, fewer than its header", r, (unsigned long long)recv_rows[r]);
  const uint64_t rows_all = runs_recv(&pl->rr, recv_rows, parts);
  int rc;
  void *p;
  uint64_t *d_lbase;
  uint32_t *d_lcap, *d_cnt2;
  if ((rc = view(&d_lbase, &d_lcap, &d_cnt2))) return rc;
  if ((rc = cfrk_pool_get(ctx, BUF_SCRATCH, (nseg * 3 + 2) * sizeof(uint64_t) + nseg * sizeof(uint32_t), &p))) return rc;
  uint64_t *d_src = (uint64_t *)p, *d_d1 = d_src + nseg, *d_d0 = d_d1 + nseg, *d_out = d_d0 + nseg;
  uint32_t *d_segrows = (uint32_t *)(d_out + 2);
  HIP_TRY(ctx, hipMemsetAsync(d_out, 0, 2 * sizeof(uint64_t), ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(ctx->g_stats + ST_CURSOR, 0, sizeof(uint64_t), ctx->stream));   // (the result list starts empty)
  hipLaunchKernelGGL((msp_runs_layout1_kernel<NC, CI1, CI0, RMUL>), dim3((unsigned)(lpp + 255) / 256), dim3(256), 0, ctx->stream, (const uint4 *)d_packed, pl->rr, parts, lpp,
                     d_segrows, d_d1, d_d0, d_lcap, d_out);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL((msp_runs_layout_kernel<NC, CI1, CI0>), dim3((unsigned)parts + 1u), dim3(1024), 0, ctx->stream, pl->rr, parts, lpp, hrows, (const uint32_t *)d_segrows,
                     d_src, d_d1, d_d0, d_lbase, (const uint32_t *)d_lcap, d_cnt2, d_out);
  HIP_TRY(ctx, hipGetLastError());
  uint64_t h[2];
  HIP_TRY(ctx, hipMemcpyAsync(h, d_out, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (h[1]) return cfrk_fail(ctx, CFRK_ERR_ARG, "a rank's header does not add up to the rows it sent");
  // (h[0] records; at most eight per row)
  if (h[0] > rows_all * NOTES_PER_ROW) return cfrk_fail(ctx, CFRK_ERR_ARG, "the headers announce more records than the rows can hold");
  if ((rc = cfrk_pool_get(ctx, BUF_MSP_L2, (size_t)(h[0] ? h[0] : 1) * sizeof(Rec), &p))) return rc;
  *rec2 = (Rec *)p;
  pl->lpp = lpp; pl->nseg = nseg; pl->src = d_src; pl->d1 = d_d1; pl->d0 = d_d0;
  return CFRK_OK;
}

// owner, pipelined: the lists of group `group` of `ngroups` in the receive buffer
static P3ListsT<true> runs_group_lists(const void *d_recv, const uint64_t *recv_rows, int parts, int group, int ngroups) {
  const int lpp = (NLEAF + parts - 1) / parts;
  P3ListsT<true> lx;
  memset(&lx, 0, sizeof lx);
  lx.packed = (const uint4 *)d_recv;
  runs_recv(&lx.rr, recv_rows, parts);
  lx.parts = parts;
  lx.ll0 = runs_ll0(lpp, group, ngroups);
  lx.lcount = runs_ll0(lpp, group + 1, ngroups) - lx.ll0;
  return lx;
}
