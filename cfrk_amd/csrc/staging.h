// staging.h -- what the host forms of the ABI pairs share (abi.hip, ingest.hip, ingest_fastq.hip): the check of an
// untrusted struct-read table, the carve of a pool slot into 256-byte aligned parts, the upload of struct-read arguments
// and the download of struct-read results.  A new pair starts from here: check, stage_reads, the _device form's core,
// download.  The first half needs neither HIP nor the context (tools/staging_host_check.cpp runs it under sanitizers).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <thread>
#include <vector>

enum { LAYOUT_OK = 0, LAYOUT_START, LAYOUT_PAST, LAYOUT_NO_TERM, LAYOUT_SUM };
// START: read's start is `got`, its predecessor asks for `want`.  SUM: the table ends at `got`, nN is `want`.
struct LayoutVerdict { int why; int64_t read, got, want; };

inline void layout_message(const LayoutVerdict &v, char *buf, size_t n) {
  if (v.why == LAYOUT_START) snprintf(buf, n, "read %lld: start %lld, expected %lld", (long long)v.read, (long long)v.got, (long long)v.want);
  else if (v.why == LAYOUT_PAST) snprintf(buf, n, "read %lld runs past nN", (long long)v.read);
  else if (v.why == LAYOUT_NO_TERM) snprintf(buf, n, "read %lld has no terminator", (long long)v.read);
  else if (v.why == LAYOUT_SUM) snprintf(buf, n, "sum(length)+nS = %lld but nN = %lld", (long long)v.got, (long long)v.want);
  else if (n) buf[0] = 0;
}

// Struct-read layout (src/fastaIO.h:74-102, src/main.cu:195-200): read i occupies [start[i], start[i]+length[i]) and is
// followed by one terminator byte.  Every read is checked against its predecessor, so ranges of reads are independent:
// up to eight threads check them in the background WHILE the batch is copied (10^7 reads: 16 ms of cache misses that
// used to come first).  Joined by verdict() or by the destructor (the callers leave early on HIP errors).
struct LayoutCheck {
  std::vector<std::thread> th;
  std::vector<int64_t> bad;
  std::vector<int> why;
  const int8_t *data = nullptr; const int64_t *start = nullptr; const int32_t *length = nullptr;
  int64_t nN = 0, nS = 0;
  void begin(const int8_t *d, const int64_t *s, const int32_t *l, int64_t nn, int64_t ns) {
    data = d; start = s; length = l; nN = nn; nS = ns;
    const int64_t piece = 1 << 20;
    unsigned nt = (unsigned)std::min<int64_t>((nS + piece - 1) / piece, 8);
    const unsigned hw = std::thread::hardware_concurrency();
    if (hw && nt > hw) nt = hw;
    if (nt == 0) nt = 1;
    bad.assign(nt, -1);
    why.assign(nt, 0);
    auto piece_fn = [this](unsigned t, unsigned nt) {
      const int64_t i0 = nS * t / nt, i1 = nS * (t + 1) / nt;
      for (int64_t i = i0; i < i1; ++i) {
        // A thread's first read is compared with a predecessor another thread validates: every
        // term is range-checked before it is used, so a corrupt table (negative starts, sums that
        // overflow) never turns into an out-of-bounds read of data[].
        int w = 0;
        if (start[i] < 0 || start[i] > nN || length[i] < 0) w = LAYOUT_START;
        else if (i && (start[i - 1] < 0 || start[i - 1] > nN || length[i - 1] < 0 ||
                       start[i] != start[i - 1] + (int64_t)length[i - 1] + 1)) w = LAYOUT_START;
        else if (!i && start[i] != 0) w = LAYOUT_START;
        else if ((int64_t)length[i] + 1 > nN - start[i]) w = LAYOUT_PAST;
        else { const int8_t term = data[start[i] + length[i]]; if (term >= 0 && term <= 3) w = LAYOUT_NO_TERM; }
        if (w) { bad[t] = i; why[t] = w; return; }
      }
    };
    // std::thread may throw (resource exhaustion): nothing may cross the extern "C" boundary, so
    // the pieces no thread could be started for are checked right here
    unsigned started = 0;
    try {
      for (; started < nt; ++started) th.emplace_back(piece_fn, started, nt);
    } catch (...) {
      for (unsigned t = started; t < nt; ++t) piece_fn(t, nt);
    }
  }
  void join() { for (auto &x : th) if (x.joinable()) x.join(); }
  // the first read that is not the reference's layout, or LAYOUT_OK (also when the check was never begun)
  LayoutVerdict verdict() {
    if (!start) return {LAYOUT_OK, 0, 0, 0};
    join();
    for (size_t t = 0; t < bad.size(); ++t) {
      if (bad[t] < 0) continue;
      const int64_t i = bad[t];
      // (the predecessor's fields may themselves be garbage: wrap-around arithmetic, text only)
      const int64_t want = i ? (int64_t)((uint64_t)start[i - 1] + (uint64_t)(int64_t)length[i - 1] + 1u) : 0;
      return {why[t], i, start[i], want};
    }
    const int64_t pos = nS ? start[nS - 1] + (int64_t)length[nS - 1] + 1 : 0;
    if (pos != nN) return {LAYOUT_SUM, nS, pos, nN};
    return {LAYOUT_OK, 0, 0, 0};
  }
  ~LayoutCheck() { join(); }
};

// N parts in one pool slot, each on a 256-byte boundary: part() returns the next part's offset, `end` is what the slot
// is asked for (the last part is not rounded up).  The first part carries its own padding (+64 staged read data, +16
// text and output data: the kernels read whole 16- / 32-byte chunks).
struct Carve {
  size_t end = 0;
  size_t part(size_t bytes) { const size_t o = (end + 255) & ~(size_t)255; end = o + bytes; return o; }
};
template <class T> inline T *carve_at(void *base, size_t off) { return (T *)((char *)base + off); }

// [first | start | length | extras] in one slot (start and length only with `table`): the staged struct-read arguments
// (first = nN + 64) and the struct-read results (first = nN + 16, the index as the extra)
struct SlotCarve {
  size_t o_start = 0, o_length = 0, o_extra[4] = {0, 0, 0, 0}, total;
  SlotCarve(size_t first, uint64_t nS, bool table, const size_t *extra_bytes, int nextra) {
    Carve c;
    c.part(first);
    if (table) { o_start = c.part((size_t)nS * 8); o_length = c.part((size_t)nS * 4); }
    for (int j = 0; j < nextra && j < 4; ++j) o_extra[j] = c.part(extra_bytes[j]);
    total = c.end;
  }
};

#ifdef __HIPCC__
#include "common.h"

inline bool layout_failed(cfrk_ctx *ctx, LayoutCheck &lc) {
  const LayoutVerdict v = lc.verdict();
  if (v.why == LAYOUT_OK) return false;
  char msg[160];
  layout_message(v, msg, sizeof msg);
  cfrk_fail(ctx, CFRK_ERR_LAYOUT, "%s", msg);
  return true;
}

// a core failed while the host form's copies may still read the caller's buffers: drained before the error is returned
inline int stage_drain(cfrk_ctx *ctx, int rc) {
  if (rc) (void)hipStreamSynchronize(ctx->stream);
  return rc;
}

// an extra part behind the reads: src NULL = room only (nothing copied), bytes 0 = absent (dev stays NULL)
struct StagePart { const void *src; size_t bytes; void *dev; };
struct StagedReads { int8_t *data; int64_t *start; int32_t *length; };   // start / length NULL when only the data is staged
enum { STAGE_TABLE = 1 /* start and length go to the device too */, STAGE_DRAIN_FIRST = 2 /* the slot may still be read */ };

// Struct-read arguments into `slot` as [data | start | length | extras]: sized before any copy is enqueued, the layout
// checked beside the copies (when start and length are given), a bad layout refused only once the copies are done.
inline int stage_reads(cfrk_ctx *ctx, int slot, const int8_t *data, const int64_t *start, const int32_t *length, int64_t nN,
                       int64_t nS, int how, StagePart *extra, int nextra, StagedReads *d) {
  if (nextra > 4) return cfrk_fail(ctx, CFRK_ERR_ARG, "stage_reads: %d extra parts, room for 4", nextra);
  LayoutCheck lc;
  if (start && length) lc.begin(data, start, length, nN, nS);
  if (how & STAGE_DRAIN_FIRST) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const bool table = (how & STAGE_TABLE) != 0;
  size_t xb[4] = {0, 0, 0, 0};
  for (int j = 0; j < nextra; ++j) xb[j] = extra[j].bytes;
  const SlotCarve c((size_t)nN + 64, (uint64_t)nS, table, xb, nextra);
  void *p;
  if (const int rc = cfrk_pool_get(ctx, slot, c.total, &p)) return rc;
  d->data = (int8_t *)p;
  d->start = table ? carve_at<int64_t>(p, c.o_start) : nullptr;
  d->length = table ? carve_at<int32_t>(p, c.o_length) : nullptr;
  if (nN) HIP_TRY(ctx, hipMemcpyAsync(d->data, data, (size_t)nN, hipMemcpyHostToDevice, ctx->stream));
  if (table) {
    HIP_TRY(ctx, hipMemcpyAsync(d->start, start, (size_t)nS * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d->length, length, (size_t)nS * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  for (int j = 0; j < nextra; ++j) {
    extra[j].dev = extra[j].bytes ? carve_at<void>(p, c.o_extra[j]) : nullptr;
    if (extra[j].bytes && extra[j].src) HIP_TRY(ctx, hipMemcpyAsync(extra[j].dev, extra[j].src, extra[j].bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  if (!layout_failed(ctx, lc)) return CFRK_OK;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // (the copies read the caller's buffers)
  return CFRK_ERR_LAYOUT;
}

// Where a measure-then-emit feature writes its struct-read results.  Device form: the caller's pointers (slot < 0).
// Host form: parts of `slot`, carved by reads_out_carve once the sizes are known.
struct ReadsOut {
  int8_t *data; int64_t *start; int32_t *length; int64_t *index;
  uint64_t cap_data, cap_reads;
  int slot; bool index_room;
};

// the arguments the text parsers share (after the format's own flag check); the sizes read 0 until they are measured
inline int parse_check(cfrk_ctx *ctx, const void *text, uint64_t nbytes, const void *data, uint64_t cap_data, const void *start,
                       const void *length, uint64_t cap_reads, int64_t *nN_out, int64_t *nS_out) {
  if (!nN_out || !nS_out) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL size output");
  if (nbytes > 0 && !text) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL text");
  if ((cap_data > 0 && !data) || (cap_reads > 0 && (!start || !length))) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL array with a capacity above 0");
  if (nbytes > ((uint64_t)1 << 62)) return cfrk_fail(ctx, CFRK_ERR_ARG, "nbytes");
  *nN_out = *nS_out = 0;
  return CFRK_OK;
}

// the measured sizes to the caller; CFRK_ERR_SMALL_BUF when they do not fit its capacities
inline int reads_out_fit(cfrk_ctx *ctx, const char *what, const ReadsOut &o, int64_t nN, int64_t nS, int64_t *nN_out, int64_t *nS_out) {
  *nN_out = nN; *nS_out = nS;
  if ((uint64_t)nN > o.cap_data || (uint64_t)nS > o.cap_reads)
    return cfrk_fail(ctx, CFRK_ERR_SMALL_BUF, "%s: %lld bytes of data and %lld reads, room for %llu and %llu", what, (long long)nN, (long long)nS,
                     (unsigned long long)o.cap_data, (unsigned long long)o.cap_reads);
  return CFRK_OK;
}

inline int reads_out_carve(cfrk_ctx *ctx, ReadsOut *o, int64_t nN, int64_t nS) {
  if (o->slot < 0) return CFRK_OK;
  const size_t index_bytes = (size_t)nS * 8;
  const SlotCarve c((size_t)nN + 16, (uint64_t)nS, true, &index_bytes, o->index_room ? 1 : 0);
  void *p;
  if (const int rc = cfrk_pool_get(ctx, o->slot, c.total, &p)) return rc;
  o->data = (int8_t *)p;
  o->start = carve_at<int64_t>(p, c.o_start);
  o->length = carve_at<int32_t>(p, c.o_length);
  o->index = o->index_room ? carve_at<int64_t>(p, c.o_extra[0]) : nullptr;
  return CFRK_OK;
}

// [data | start | length (| index)] down to the caller's arrays; synchronises
inline int download_reads(cfrk_ctx *ctx, const ReadsOut &o, int8_t *data, int64_t *start, int32_t *length, int64_t *index, int64_t nN, int64_t nS) {
  HIP_TRY(ctx, hipMemcpyAsync(data, o.data, (size_t)nN, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(start, o.start, (size_t)nS * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(length, o.length, (size_t)nS * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (index) HIP_TRY(ctx, hipMemcpyAsync(index, o.index, (size_t)nS * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CFRK_OK;
}

#endif  // __HIPCC__
