// msp_runs.h -- the parts of the multi-GPU exchange by runs that do not depend on the record format.  Device side:
// where every leaf's rows go in the packed buffer (sender) and where every received segment goes in the owner's
// leaf streams.  Host side: the whole call sequence of the one-shot and the pipelined exchange -- scratch buffers,
// plan and layout kernels, read-backs and the checks of what arrived -- with the kernels that read or write records
// handed in as launch lambdas.  Included by msp.hip (16-byte records, one row each) and msp2.hip (32-byte records,
// two rows each) inside their anonymous namespaces; msp_shared.h holds what the two share outside the exchange.
#pragma once

constexpr uint32_t RUN_NOTED = 0xFFFFFFFFu;        // (a record's header word has the top 8 bits clear)
constexpr int NOTES_PER_ROW = 8;
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
    rows[(size_t)r * lpp + ll] = (uint32_t)RMUL * (a + b) + (c + NOTES_PER_ROW - 1) / NOTES_PER_ROW;
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
