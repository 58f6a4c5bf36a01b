// abi.hip -- the C-ABI entry points of libcfrk_hip.so (include/cfrk_abi.h).
// Replaces kmer_main() (/root/reference/src/kmer_main.cu:20-128): context + persistent device
// pool instead of per-call cudaMalloc/cudaFree, error codes instead of printf/exit.
#include "common.h"

#include <stdarg.h>
#include <stdlib.h>

#include <algorithm>
#include <thread>
#include <vector>
#include <new>
#include <numeric>

#include "msp.h"
#include "staging.h"
#include "table.h"

int cfrk_fail(cfrk_ctx *ctx, int code, const char *fmt, ...) {
  if (ctx) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ctx->err, sizeof ctx->err, fmt, ap);
    va_end(ap);
  }
  return code;
}

int cfrk_pool_get(cfrk_ctx *ctx, int slot, size_t bytes, void **out) {
  cfrk_buf &b = ctx->pool[slot];
  if (bytes == 0) bytes = 16;
  if (b.cap < bytes) {
    if (b.p) { HIP_TRY(ctx, hipFree(b.p)); b.p = nullptr; b.cap = 0; }
    size_t want = (bytes + 255) & ~(size_t)255;
    HIP_TRY(ctx, hipMalloc(&b.p, want));
    b.cap = want;
  }
  *out = b.p;
  return CFRK_OK;
}

extern "C" {

int cfrk_abi_version(void) { return CFRK_ABI_VERSION; }

const char *cfrk_strerror(int code) {
  switch (code) {
    case CFRK_OK: return "ok";
    case CFRK_ERR_ARG: return "invalid argument";
    case CFRK_ERR_NOMEM: return "out of device or pinned memory";
    case CFRK_ERR_HIP: return "HIP runtime error";
    case CFRK_ERR_STATE: return "call sequence violated";
    case CFRK_ERR_LAYOUT: return "data/start/length do not describe the struct-read layout";
    case CFRK_ERR_TABLE_FULL: return "global table overflowed (raise capacity_hint)";
    case CFRK_ERR_ALIGN: return "device pointer not 16-byte aligned";
    case CFRK_ERR_NO_DEVICE: return "no usable gfx950 device";
    case CFRK_ERR_SMALL_BUF: return "output buffer too small";
    case CFRK_ERR_COUNT_OVERFLOW: return "a key's count reached 2^32 - 2 and was saturated";
    case CFRK_ERR_RUNS_REFUSED: return "the CFRK_RUNS_ONLY add does not fit device memory in one pass";
    default: return "unknown error";
  }
}

const char *cfrk_last_error(const cfrk_ctx *ctx) { return ctx ? ctx->err : ""; }

int cfrk_device_count(int *count) {
  if (!count) return CFRK_ERR_ARG;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { *count = 0; return CFRK_ERR_NO_DEVICE; }
  *count = n;
  return CFRK_OK;
}

int cfrk_ctx_create(int device, void *hip_stream, cfrk_ctx **out) {
  if (!out) return CFRK_ERR_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return CFRK_ERR_NO_DEVICE;
  if (device < 0 || device >= n) return CFRK_ERR_ARG;
  if (hipSetDevice(device) != hipSuccess) return CFRK_ERR_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return CFRK_ERR_NO_DEVICE;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return CFRK_ERR_NO_DEVICE;  // gfx950 code objects only
  cfrk_ctx *ctx = new (std::nothrow) cfrk_ctx();
  if (!ctx) return CFRK_ERR_NOMEM;
  memset(ctx, 0, sizeof *ctx);
  ctx->device = device;
  ctx->num_cus = prop.multiProcessorCount;
  if (hip_stream) {
    ctx->stream = (hipStream_t)hip_stream;
  } else {
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return CFRK_ERR_HIP; }
    ctx->own_stream = true;
  }
  if (hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess ||
      hipMalloc((void **)&ctx->g_stats, ST_NWORDS * sizeof(uint64_t)) != hipSuccess ||
      hipHostMalloc((void **)&ctx->h_stats, ST_NWORDS * sizeof(uint64_t), hipHostMallocDefault) != hipSuccess) {
    cfrk_ctx_destroy(ctx);
    return CFRK_ERR_HIP;
  }
  *out = ctx;
  return CFRK_OK;
}

static void global_release(cfrk_ctx *ctx) {
  if (ctx->g_keys_lo) (void)hipFree(ctx->g_keys_lo);
  if (ctx->g_keys_hi) (void)hipFree(ctx->g_keys_hi);
  if (ctx->g_counts) (void)hipFree(ctx->g_counts);
  ctx->g_keys_lo = ctx->g_keys_hi = nullptr;
  ctx->g_counts = nullptr;
  ctx->g_cap = 0;
  ctx->g_active = false;
  ctx->g_table_cleared = false;
}

void cfrk_ctx_destroy(cfrk_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  cfrk_msp_destroy(ctx);
  global_release(ctx);
  for (int i = 0; i < BUF_NSLOTS; ++i)
    if (ctx->pool[i].p) (void)hipFree(ctx->pool[i].p);
  if (ctx->pinned) (void)hipHostFree(ctx->pinned);
  if (ctx->g_stats) (void)hipFree(ctx->g_stats);
  if (ctx->h_stats) (void)hipHostFree(ctx->h_stats);
  if (ctx->h_runs) (void)hipHostFree(ctx->h_runs);
  for (int g = 0; g < CFRK_RUNS_MAX_GROUPS; ++g) if (ctx->runs_ev[g]) (void)hipEventDestroy(ctx->runs_ev[g]);
  if (ctx->stage_ev[0]) (void)hipEventDestroy(ctx->stage_ev[0]);
  if (ctx->stage_ev[1]) (void)hipEventDestroy(ctx->stage_ev[1]);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

int cfrk_ctx_sync(cfrk_ctx *ctx) {
  if (!ctx) return CFRK_ERR_ARG;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CFRK_OK;
}

int cfrk_device_alloc(cfrk_ctx *ctx, size_t bytes, void **dptr) {
  if (!ctx || !dptr) return CFRK_ERR_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMalloc(dptr, bytes ? bytes : 16));
  return CFRK_OK;
}

int cfrk_device_free(cfrk_ctx *ctx, void *dptr) {
  if (!ctx) return CFRK_ERR_ARG;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (dptr) HIP_TRY(ctx, hipFree(dptr));
  return CFRK_OK;
}

int cfrk_memcpy_h2d(cfrk_ctx *ctx, void *dst, const void *src, size_t bytes) {
  if (!ctx || (bytes && (!dst || !src))) return CFRK_ERR_ARG;
  HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CFRK_OK;
}

// Host memory the runtime cannot pin piece by piece at full rate (a mapped file) goes through a ring of pinned
// buffers of the context's own: eight threads, two 4 MB buffers each; a thread copies its next piece into a buffer
// while the device reads the other one.  All pieces are enqueued on the context stream.
int cfrk_memcpy_h2d_staged(cfrk_ctx *ctx, void *dst, const void *src, size_t bytes) {
  if (!ctx || (bytes && (!dst || !src))) return CFRK_ERR_ARG;
  constexpr size_t CH = (size_t)4 << 20;
  constexpr int NT = 8;
  if (bytes < 2 * CH) return cfrk_memcpy_h2d(ctx, dst, src, bytes);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (ctx->pinned_cap < NT * 2 * CH) {
    if (ctx->pinned) { HIP_TRY(ctx, hipHostFree(ctx->pinned)); ctx->pinned = nullptr; ctx->pinned_cap = 0; }
    HIP_TRY(ctx, hipHostMalloc(&ctx->pinned, NT * 2 * CH, hipHostMallocDefault));
    ctx->pinned_cap = NT * 2 * CH;
  }
  hipEvent_t ev[NT][2] = {};
  auto drop_events = [&] {
    for (int t = 0; t < NT; ++t)
      for (int b = 0; b < 2; ++b) if (ev[t][b]) (void)hipEventDestroy(ev[t][b]);
  };
  for (int t = 0; t < NT; ++t)
    for (int b = 0; b < 2; ++b) {
      const hipError_t e = hipEventCreateWithFlags(&ev[t][b], hipEventDisableTiming);
      if (e != hipSuccess) { ev[t][b] = nullptr; drop_events(); HIP_TRY(ctx, e); }
    }
  const size_t nchunks = (bytes + CH - 1) / CH;
  hipError_t err[NT];
  auto work = [&](int t) {
    err[t] = hipSetDevice(ctx->device);
    size_t round = 0;
    for (size_t c = (size_t)t; c < nchunks && err[t] == hipSuccess; c += NT, ++round) {
      const int b = (int)(round & 1);
      char *stage = (char *)ctx->pinned + ((size_t)t * 2 + (size_t)b) * CH;
      const size_t off = c * CH, len = std::min(CH, bytes - off);
      if (round >= 2 && (err[t] = hipEventSynchronize(ev[t][b])) != hipSuccess) break;
      memcpy(stage, (const char *)src + off, len);
      if ((err[t] = hipMemcpyAsync((char *)dst + off, stage, len, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess) break;
      err[t] = hipEventRecord(ev[t][b], ctx->stream);
    }
  };
  {
    std::vector<std::thread> th;
    int started = 0;
    try {
      for (; started < NT; ++started) th.emplace_back(work, started);
    } catch (...) {
    }
    for (int t = started; t < NT; ++t) work(t);        // (threads that could not be started: their pieces, here)
    for (auto &x : th) x.join();
  }
  const hipError_t se = hipStreamSynchronize(ctx->stream);
  drop_events();
  for (int t = 0; t < NT; ++t) HIP_TRY(ctx, err[t]);
  HIP_TRY(ctx, se);
  return CFRK_OK;
}

int cfrk_memcpy_d2h(cfrk_ctx *ctx, void *dst, const void *src, size_t bytes) {
  if (!ctx || (bytes && (!dst || !src))) return CFRK_ERR_ARG;
  HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CFRK_OK;
}

int cfrk_memcpy_peer(cfrk_ctx *dst_ctx, void *dst, cfrk_ctx *src_ctx, const void *src, size_t bytes) {
  if (!dst_ctx || !src_ctx || (bytes && (!dst || !src))) return CFRK_ERR_ARG;
  if (bytes == 0) return CFRK_OK;
  // every failure is reported on dst_ctx: several owners (threads, each with its own dst_ctx) may copy from ONE
  // source context at the same time, and a context's error text has a single writer -- its own thread
  HIP_TRY(dst_ctx, hipSetDevice(src_ctx->device));
  HIP_TRY(dst_ctx, hipStreamSynchronize(src_ctx->stream));      // (draining a stream from several threads is safe)
  HIP_TRY(dst_ctx, hipSetDevice(dst_ctx->device));
  if (dst_ctx->device != src_ctx->device) {
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, dst_ctx->device, src_ctx->device) == hipSuccess && can) {
      const hipError_t e = hipDeviceEnablePeerAccess(src_ctx->device, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();   // the copy still works, staged by the runtime
      else (void)hipGetLastError();
    }
    HIP_TRY(dst_ctx, hipMemcpyPeerAsync(dst, dst_ctx->device, src, src_ctx->device, bytes, dst_ctx->stream));
  } else {
    HIP_TRY(dst_ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, dst_ctx->stream));
  }
  return CFRK_OK;
}

/* ------------------------------------------------------------------ per-read dense */

static int dense_check(cfrk_ctx *ctx, int64_t nN, int64_t nS, int k) {
  if (!ctx) return CFRK_ERR_ARG;
  if (k < 1 || k > 15) return cfrk_fail(ctx, CFRK_ERR_ARG, "k=%d outside 1..15 (POW(k) is 1U<<2k in an int)", k);
  if (nN < 0 || nS < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  return CFRK_OK;
}

int cfrk_per_read_dense_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start,
                               const int32_t *d_length, int64_t nN, int64_t nS, int k, int flags,
                               int32_t *d_freq) {
  int rc = dense_check(ctx, nN, nS, k);
  if (rc) return rc;
  if (nS == 0) return CFRK_OK;
  if (!d_data || !d_start || !d_length || !d_freq) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cfrk_launch_dense(ctx, d_data, d_start, d_length, nN, nS, k, flags, d_freq);
}

int cfrk_per_read_dense(cfrk_ctx *ctx, const int8_t *data, const int64_t *start,
                        const int32_t *length, int64_t nN, int64_t nS, int k, int flags,
                        int32_t *freq_out) {
  int rc = dense_check(ctx, nN, nS, k);
  if (rc) return rc;
  if (nS == 0) return CFRK_OK;
  if (!data || !start || !length || !freq_out) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t fourk = (size_t)1 << (2 * k);
  const size_t freq_bytes = (size_t)nS * fourk * sizeof(int32_t);
  // the reference's up-front estimate (src/kmer_main.cu:44-56), against free memory
  size_t free_b = 0, total_b = 0;
  HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
  size_t need = (size_t)nN + (size_t)nS * 16 + freq_bytes;
  size_t have = free_b + ctx->pool[BUF_DATA].cap + ctx->pool[BUF_START].cap +
                ctx->pool[BUF_LENGTH].cap + ctx->pool[BUF_FREQ].cap + ctx->pool[BUF_SPILL].cap;
  if (need > have)
    return cfrk_fail(ctx, CFRK_ERR_NOMEM, "required %zu B, available %zu B", need, have);
  void *d_data, *d_start, *d_length, *d_freq;
  if ((rc = cfrk_pool_get(ctx, BUF_DATA, (size_t)nN + 64, &d_data))) return rc;
  if ((rc = cfrk_pool_get(ctx, BUF_START, (size_t)nS * 8, &d_start))) return rc;
  if ((rc = cfrk_pool_get(ctx, BUF_LENGTH, (size_t)nS * 4, &d_length))) return rc;
  if ((rc = cfrk_pool_get(ctx, BUF_FREQ, freq_bytes, &d_freq))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(d_data, data, (size_t)nN, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_start, start, (size_t)nS * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_length, length, (size_t)nS * 4, hipMemcpyHostToDevice, ctx->stream));
  rc = cfrk_launch_dense(ctx, (const int8_t *)d_data, (const int64_t *)d_start,
                         (const int32_t *)d_length, nN, nS, k, flags, (int32_t *)d_freq);
  if (rc) return rc;
  return cfrk_memcpy_d2h(ctx, freq_out, d_freq, freq_bytes);
}

/* ------------------------------------------------------------------ global counting */

int cfrk_global_begin(cfrk_ctx *ctx, int k, int flags, uint64_t capacity_hint) {
  if (!ctx) return CFRK_ERR_ARG;
  if (k < 1 || k > 64) return cfrk_fail(ctx, CFRK_ERR_ARG, "k=%d outside 1..64", k);
  if ((flags & CFRK_RUNS_ONLY) && (k < 16 || k > 64 || (flags & CFRK_FORCE_HASH)))
    return cfrk_fail(ctx, CFRK_ERR_ARG, "CFRK_RUNS_ONLY needs a partitioned path (16 <= k <= 64)");
  if ((flags & CFRK_RUNS_DEFER) && !(flags & CFRK_RUNS_ONLY)) return cfrk_fail(ctx, CFRK_ERR_ARG, "CFRK_RUNS_DEFER goes with CFRK_RUNS_ONLY");
  ctx->q_valid = false;     // (every call that may change the result drops the query index: the next query rebuilds it)
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  // Was the HBM table left untouched by the previous job (the partitioned path only writes it
  // on spill)?  Then it is still all-empty and the 12 B/slot clear below can be skipped.
  // (h_stats = pinned snapshot of the device flags, copied at the end of the last add.)
  const bool table_clean_prev = ctx->g_table_cleared && !cfrk_msp_table_written(ctx) &&
                                ctx->h_stats_valid && ctx->h_stats[ST_SPILLED] == 0;
  bool table_clean = table_clean_prev;
  ctx->h_stats_valid = false;
  cfrk_msp_reset(ctx);
  if (capacity_hint == 0) capacity_hint = 1ull << 24;
  // distinct keys cannot exceed 4^k
  if (k < 31) capacity_hint = std::min<uint64_t>(capacity_hint, 1ull << (2 * k));
  int lg = 10;
  while (lg < 40 && (1ull << lg) < capacity_hint * 2) ++lg;   // load factor <= 0.5 at the hint
  const uint64_t cap = 1ull << lg;
  const bool two = k > 32;
  if (cap != ctx->g_cap || two != ctx->g_two || (two && !ctx->g_keys_hi)) {
    global_release(ctx);
    HIP_TRY(ctx, hipMalloc((void **)&ctx->g_keys_lo, cap * 8));
    if (two) HIP_TRY(ctx, hipMalloc((void **)&ctx->g_keys_hi, cap * 8));
    HIP_TRY(ctx, hipMalloc((void **)&ctx->g_counts, cap * 4));
    ctx->g_cap = cap;
    table_clean = false;
  }
  if (two != ctx->g_two) table_clean = false;
  ctx->g_log2cap = lg;
  ctx->g_k = k;
  ctx->g_flags = flags;
  ctx->g_two = two;
  // one-word: empty = all-ones key.  two-word: the COUNT word is the slot state (0 = empty).
  if (!table_clean) {
    if (!two) HIP_TRY(ctx, hipMemsetAsync(ctx->g_keys_lo, 0xFF, cap * 8, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->g_counts, 0, cap * 4, ctx->stream));
  }
  ctx->g_table_cleared = true;
  HIP_TRY(ctx, hipMemsetAsync(ctx->g_stats, 0, ST_NWORDS * 8, ctx->stream));
  ctx->g_active = true;
  ctx->ev_valid = false;
  return CFRK_OK;
}

int cfrk_global_add_device(cfrk_ctx *ctx, const int8_t *d_data, int64_t nN) {
  if (!ctx) return CFRK_ERR_ARG;
  if (!ctx->g_active) return cfrk_fail(ctx, CFRK_ERR_STATE, "cfrk_global_add before cfrk_global_begin");
  ctx->q_valid = false;
  if (nN < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (nN == 0) return CFRK_OK;
  if (!d_data) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  if (((uintptr_t)d_data & 15) != 0) return cfrk_fail(ctx, CFRK_ERR_ALIGN, "d_data %p", (const void *)d_data);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  int rc;
  rc = CFRK_ERR_NOMEM;
  ctx->last_passes = 0;
  if (cfrk_radix_prefers(ctx, nN)) {
    rc = cfrk_radix_count(ctx, d_data, nN);
    if (rc == CFRK_ERR_NOMEM && cfrk_msp_usable(ctx)) { (void)hipGetLastError(); rc = cfrk_msp_count(ctx, d_data, nN); }   // (k = 16)
  } else if (cfrk_msp_usable(ctx)) rc = cfrk_msp_count(ctx, d_data, nN);
  else if (cfrk_msp2_usable(ctx)) rc = cfrk_msp2_count(ctx, d_data, nN);
  if (rc == CFRK_ERR_NOMEM && (cfrk_msp_usable(ctx) || cfrk_radix_usable(ctx) || cfrk_msp2_usable(ctx)) &&
      !(ctx->msp && ctx->msp->pending)) {     // (CFRK_INTERNAL_FLOOD: no second attempt, straight to the general path)
    // The pool only grows: buffers sized by earlier jobs of this context (another k, a larger batch) may be
    // what stands in the way.  Nothing of the partitioned paths is live between adds unless a result list is
    // pending: give their buffers back and plan the batch once more before giving the fast path up.
    static const int trim[] = {BUF_SCRATCH, BUF_MSP_L1, BUF_MSP_L2, BUF_MSP_OUTK, BUF_MSP_OUTC, BUF_MSP_AUX, BUF_MSP_OUTH,
                               BUF_MSP_ACCK, BUF_MSP_ACCH, BUF_MSP_ACCC, BUF_MSP_LAYOUT, BUF_MSP_OVF, BUF_MSP_OVF1,
                               BUF_MSP_LAYOUT1, BUF_EXPORT_LO, BUF_EXPORT_HI, BUF_EXPORT_CNT};
    size_t freed = 0;
    (void)hipGetLastError();
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int slot : trim) {
      cfrk_buf &b = ctx->pool[slot];
      if (b.p) { freed += b.cap; (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    }
    if (freed) {
      if (cfrk_radix_prefers(ctx, nN)) rc = cfrk_radix_count(ctx, d_data, nN);
      if (rc == CFRK_ERR_NOMEM && cfrk_msp_usable(ctx)) { (void)hipGetLastError(); rc = cfrk_msp_count(ctx, d_data, nN); }
      else if (rc == CFRK_ERR_NOMEM && cfrk_msp2_usable(ctx)) rc = cfrk_msp2_count(ctx, d_data, nN);
    }
  }
  if ((rc == CFRK_ERR_NOMEM || rc == CFRK_INTERNAL_FLOOD) && (ctx->g_flags & CFRK_RUNS_ONLY))
    return cfrk_fail(ctx, CFRK_ERR_RUNS_REFUSED, rc == CFRK_ERR_NOMEM ? "the shard's record buffers do not fit device memory"
                                                                        : "2^32 records in one leaf stream: count without CFRK_RUNS_ONLY");
  if (rc == CFRK_INTERNAL_FLOOD) {
    // a single-key flood wrapped a 32-bit stream cursor before anything of this add was counted: the general path
    // (one saturating HBM atomic per occurrence) counts it instead
    HIP_TRY(ctx, hipMemsetAsync(ctx->g_stats + ST_CWRAP, 0, sizeof(uint64_t), ctx->stream));
    rc = CFRK_ERR_NOMEM;
  }
  if (rc == CFRK_ERR_NOMEM) {
    // no partitioned path for this k, or its record buffers (about 7 bytes per input byte) do
    // not fit next to the caller's data: count with the general HBM-table path instead
    (void)hipGetLastError();
    rc = cfrk_msp_flush_to_table(ctx);
    if (rc) return rc;
    cfrk_msp_note_table_write(ctx);
    rc = cfrk_hash_count(ctx, d_data, nN);
  }
  if (rc) return rc;
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  ctx->ev_valid = true;
  // snapshot of the flags for the next begin(); lands before its stream synchronisation
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_stats, ctx->g_stats, ST_NWORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  ctx->h_stats_valid = true;
  return CFRK_OK;
}

int cfrk_global_add(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length,
                    int64_t nN, int64_t nS) {
  if (!ctx) return CFRK_ERR_ARG;
  if (!ctx->g_active) return cfrk_fail(ctx, CFRK_ERR_STATE, "cfrk_global_add before cfrk_global_begin");
  if (nN < 0 || nS < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (nN == 0) return CFRK_OK;
  if (!data) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // The layout check (staging.h) runs WHILE the previous add drains and the batch is copied; nothing is counted before
  // it has passed.  STAGE_DRAIN_FIRST: the previous add may still be reading BUF_DATA.
  // The runtime's own path for pageable memory moves 46 GB/s here (it pins the caller's pages chunk
  // by chunk); a bounce buffer of our own, filled by one thread, made 26-32 GB/s, filled by eight 45.
  StagedReads d;
  const int rc = stage_reads(ctx, BUF_DATA, data, start, length, nN, nS, STAGE_DRAIN_FIRST, nullptr, 0, &d);
  if (rc) return rc;
  return stage_drain(ctx, cfrk_global_add_device(ctx, d.data, nN));
}

int cfrk_global_merge_device(cfrk_ctx *ctx, const uint64_t *d_lo, const uint64_t *d_hi,
                             const uint32_t *d_cnt, int64_t n) {
  if (!ctx) return CFRK_ERR_ARG;
  if (!ctx->g_active) return cfrk_fail(ctx, CFRK_ERR_STATE, "merge before begin");
  ctx->q_valid = false;
  if (n < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (n == 0) return CFRK_OK;
  if (!d_lo || !d_cnt || (ctx->g_two && !d_hi)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = cfrk_msp_flush_to_table(ctx);
  if (rc) return rc;
  cfrk_msp_note_table_write(ctx);
  return cfrk_hash_merge(ctx, d_lo, d_hi, d_cnt, n);
}

int cfrk_global_finish(cfrk_ctx *ctx, uint64_t *n_distinct) {
  uint64_t d[4] = {0, 0, 0, 0};
  int rc = cfrk_global_digest(ctx, d);
  if (rc && rc != CFRK_ERR_COUNT_OVERFLOW) return rc;
  if (n_distinct) *n_distinct = d[0];     // (a saturated result is complete: every key is there, some counts are CFRK_COUNT_MAX)
  return rc;
}

int cfrk_global_digest(cfrk_ctx *ctx, uint64_t out[4]) {
  if (!ctx || !out) return CFRK_ERR_ARG;
  if (!ctx->g_active) return cfrk_fail(ctx, CFRK_ERR_STATE, "digest before begin");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ResultSrc src;
  bool use_list = false;
  int rc = cfrk_msp_resolve(ctx, &src, &use_list);
  if (rc) return rc;
  uint64_t st[ST_NWORDS];
  if ((rc = cfrk_result_scan(ctx, use_list ? &src : nullptr, st))) return rc;
  if (st[ST_OVERFLOW]) return cfrk_fail(ctx, CFRK_ERR_TABLE_FULL, "table of %llu slots overflowed", (unsigned long long)ctx->g_cap);
  out[0] = st[ST_DIG0]; out[1] = st[ST_DIG1]; out[2] = st[ST_DIG2]; out[3] = st[ST_DIG3];
  if (st[ST_SAT]) return cfrk_fail(ctx, CFRK_ERR_COUNT_OVERFLOW, "a key occurred 2^32 - 2 times or more: its count is held at 0xFFFFFFFE");
  return CFRK_OK;
}

int cfrk_global_export_device(cfrk_ctx *ctx, uint64_t *d_lo, uint64_t *d_hi, uint32_t *d_cnt,
                              uint64_t cap, int parts, uint64_t *part_counts) {
  if (!ctx || !part_counts || parts < 1 || parts > 1024) return CFRK_ERR_ARG;
  if (!ctx->g_active) return cfrk_fail(ctx, CFRK_ERR_STATE, "export before begin");
  if (cap && (!d_lo || !d_cnt || (ctx->g_two && !d_hi))) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ResultSrc src;
  bool use_list = false;
  int rc = cfrk_msp_resolve(ctx, &src, &use_list);
  if (rc) return rc;
  return cfrk_result_export(ctx, use_list ? &src : nullptr, d_lo, d_hi, d_cnt, cap, parts, part_counts);
}

int cfrk_global_export(cfrk_ctx *ctx, uint64_t *keys_lo, uint64_t *keys_hi, uint32_t *counts,
                       uint64_t cap, uint64_t *n_out) {
  return cfrk_global_export_range(ctx, 1, CFRK_COUNT_MAX, keys_lo, keys_hi, counts, cap, n_out);
}

int cfrk_global_export_range(cfrk_ctx *ctx, uint32_t min_count, uint32_t max_count, uint64_t *keys_lo,
                             uint64_t *keys_hi, uint32_t *counts, uint64_t cap, uint64_t *n_out) {
  if (!ctx || !n_out) return CFRK_ERR_ARG;
  if (min_count == 0) min_count = 1;
  uint64_t n = 0;
  int rc = cfrk_global_finish(ctx, &n);
  const bool saturated = rc == CFRK_ERR_COUNT_OVERFLOW;   // the result is exported all the same, the code returned at the end
  if (rc && !saturated) return rc;
  auto done = [&]() { return saturated ? cfrk_fail(ctx, CFRK_ERR_COUNT_OVERFLOW, "a key occurred 2^32 - 2 times or more: its count is held at 0xFFFFFFFE") : CFRK_OK; };
  *n_out = 0;
  if (n == 0 || min_count > max_count) return done();
  // entries kept (one read pass; the digest above resolved the result, so this resolves to the same source)
  ResultSrc src;
  bool use_list = false;
  if ((rc = cfrk_msp_resolve(ctx, &src, &use_list))) return rc;
  const ResultSrc *sp = use_list ? &src : nullptr;
  if ((rc = cfrk_result_export_count(ctx, sp, min_count, max_count, 1, &n))) return rc;
  *n_out = n;
  if (n > cap) return cfrk_fail(ctx, CFRK_ERR_SMALL_BUF, "%llu entries, room for %llu", (unsigned long long)n, (unsigned long long)cap);
  if (n == 0) return done();
  if (!keys_lo || !counts) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  void *d_lo, *d_hi = nullptr, *d_cnt;
  if ((rc = cfrk_pool_get(ctx, BUF_EXPORT_LO, n * 8, &d_lo))) return rc;
  if (ctx->g_two && (rc = cfrk_pool_get(ctx, BUF_EXPORT_HI, n * 8, &d_hi))) return rc;
  if ((rc = cfrk_pool_get(ctx, BUF_EXPORT_CNT, n * 4, &d_cnt))) return rc;
  if ((rc = cfrk_result_export_scatter(ctx, sp, min_count, max_count, 1, &n, (uint64_t *)d_lo, (uint64_t *)d_hi,
                                       (uint32_t *)d_cnt))) return rc;
  // only the kept entries are sorted on the device (export_sort.hip) and copied straight into the caller's buffers
  const uint64_t *s_lo, *s_hi;
  const uint32_t *s_cnt;
  if ((rc = cfrk_sort_export(ctx, (const uint64_t *)d_lo, ctx->g_two ? (const uint64_t *)d_hi : nullptr,
                             (const uint32_t *)d_cnt, n, &s_lo, &s_hi, &s_cnt))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(keys_lo, s_lo, n * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (keys_hi) {
    if (s_hi) HIP_TRY(ctx, hipMemcpyAsync(keys_hi, s_hi, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    else memset(keys_hi, 0, n * 8);
  }
  HIP_TRY(ctx, hipMemcpyAsync(counts, s_cnt, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return done();
}

int cfrk_global_histogram(cfrk_ctx *ctx, uint64_t *hist, uint32_t nbins) {
  if (!ctx) return CFRK_ERR_ARG;
  if (!hist) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  if (nbins < 2 || nbins > (1u << 24)) return cfrk_fail(ctx, CFRK_ERR_ARG, "nbins=%u outside 2..2^24", nbins);
  if (!ctx->g_active) return cfrk_fail(ctx, CFRK_ERR_STATE, "histogram before begin");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ResultSrc src;
  bool use_list = false;
  int rc = cfrk_msp_resolve(ctx, &src, &use_list);
  if (rc) return rc;
  uint64_t st[ST_NWORDS];
  if ((rc = cfrk_result_histogram(ctx, use_list ? &src : nullptr, nbins, hist, st))) return rc;
  if (st[ST_OVERFLOW]) return cfrk_fail(ctx, CFRK_ERR_TABLE_FULL, "table of %llu slots overflowed", (unsigned long long)ctx->g_cap);
  if (st[ST_SAT]) return cfrk_fail(ctx, CFRK_ERR_COUNT_OVERFLOW, "a key occurred 2^32 - 2 times or more: its count is held at 0xFFFFFFFE");
  return CFRK_OK;
}

static int query_check(cfrk_ctx *ctx, int64_t n) {
  if (!ctx->g_active) return cfrk_fail(ctx, CFRK_ERR_STATE, "query before begin");
  if (ctx->g_flags & CFRK_RUNS_ONLY) return cfrk_fail(ctx, CFRK_ERR_STATE, "a CFRK_RUNS_ONLY job holds runs, not counts");
  if (n < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  return CFRK_OK;
}

int cfrk_global_query_device(cfrk_ctx *ctx, const uint64_t *d_keys_lo, const uint64_t *d_keys_hi, int64_t n,
                             uint32_t *d_counts) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = query_check(ctx, n);
  if (rc || n == 0) return rc;
  if (!d_keys_lo || !d_counts || (ctx->g_two && !d_keys_hi)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cfrk_query_keys(ctx, d_keys_lo, d_keys_hi, n, d_counts);
}

int cfrk_global_query(cfrk_ctx *ctx, const uint64_t *keys_lo, const uint64_t *keys_hi, int64_t n, uint32_t *counts) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = query_check(ctx, n);
  if (rc || n == 0) return rc;
  if (!keys_lo || !counts || (ctx->g_two && !keys_hi)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  void *d_in, *d_out;
  const size_t bytes = (size_t)n * 8;
  if ((rc = cfrk_pool_get(ctx, BUF_QUERY_IN, keys_hi ? 2 * bytes : bytes, &d_in))) return rc;
  if ((rc = cfrk_pool_get(ctx, BUF_QUERY_OUT, (size_t)n * 4, &d_out))) return rc;
  uint64_t *d_lo = (uint64_t *)d_in, *d_hi = keys_hi ? d_lo + n : nullptr;
  HIP_TRY(ctx, hipMemcpyAsync(d_lo, keys_lo, bytes, hipMemcpyHostToDevice, ctx->stream));
  if (keys_hi) HIP_TRY(ctx, hipMemcpyAsync(d_hi, keys_hi, bytes, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = cfrk_query_keys(ctx, d_lo, d_hi, n, (uint32_t *)d_out))) return rc;
  return cfrk_memcpy_d2h(ctx, counts, d_out, (size_t)n * 4);
}

int cfrk_global_query_reads_device(cfrk_ctx *ctx, const int8_t *d_data, int64_t nN, uint32_t *d_counts) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = query_check(ctx, nN);
  if (rc || nN == 0) return rc;
  if (!d_data || !d_counts) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  if (((uintptr_t)d_data & 15) != 0) return cfrk_fail(ctx, CFRK_ERR_ALIGN, "d_data %p", (const void *)d_data);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cfrk_query_reads(ctx, d_data, nN, d_counts);
}

int cfrk_global_query_reads(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length,
                            int64_t nN, int64_t nS, uint32_t *counts) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = query_check(ctx, nN);
  if (rc) return rc;
  if (nS < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (nN == 0) return CFRK_OK;
  if (!data || !counts) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // (staged through slots of their own: BUF_DATA may still be read by the job's last add)
  void *d_out;
  StagedReads d;
  if ((rc = cfrk_pool_get(ctx, BUF_QUERY_OUT, (size_t)nN * 4, &d_out))) return rc;
  if ((rc = stage_reads(ctx, BUF_QUERY_IN, data, start, length, nN, nS, 0, nullptr, 0, &d))) return rc;
  if ((rc = cfrk_query_reads(ctx, d.data, nN, (uint32_t *)d_out))) return stage_drain(ctx, rc);
  return cfrk_memcpy_d2h(ctx, counts, d_out, (size_t)nN * 4);
}

static_assert(sizeof(cfrk_read_stats) == 32, "cfrk_read_stats is 32 bytes without padding");

static int read_stats_check(cfrk_ctx *ctx, int64_t nN, int64_t nS, const void *data, const void *start,
                            const void *length, const void *out) {
  int rc = query_check(ctx, nN);
  if (rc) return rc;
  if (nS < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (nS > 0 && (!data || !start || !length || !out)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  return CFRK_OK;
}

int cfrk_global_read_stats_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                                  int64_t nN, int64_t nS, uint32_t threshold, cfrk_read_stats *d_out) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = read_stats_check(ctx, nN, nS, d_data, d_start, d_length, d_out);
  if (rc || nS == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cfrk_read_stats_launch(ctx, d_data, d_start, d_length, nN, nS, threshold, d_out);
}

int cfrk_global_read_stats(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length, int64_t nN,
                           int64_t nS, uint32_t threshold, cfrk_read_stats *out) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = read_stats_check(ctx, nN, nS, data, start, length, out);
  if (rc || nS == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // staged through the query calls' slots: the reads in, the rows out
  void *p_out;
  StagedReads d;
  if ((rc = cfrk_pool_get(ctx, BUF_QUERY_OUT, (size_t)nS * sizeof *out, &p_out))) return rc;
  if ((rc = stage_reads(ctx, BUF_QUERY_IN, data, start, length, nN, nS, STAGE_TABLE, nullptr, 0, &d))) return rc;
  if ((rc = cfrk_read_stats_launch(ctx, d.data, d.start, d.length, nN, nS, threshold, (cfrk_read_stats *)p_out))) return stage_drain(ctx, rc);
  return cfrk_memcpy_d2h(ctx, out, p_out, (size_t)nS * sizeof *out);
}

static_assert(sizeof(cfrk_read_span) == 8, "cfrk_read_span is 8 bytes without padding");

static int read_spans_check(cfrk_ctx *ctx, int64_t nN, int64_t nS, const void *data, const void *start,
                            const void *length, const void *out, int mode) {
  int rc = read_stats_check(ctx, nN, nS, data, start, length, out);
  if (rc) return rc;
  if (mode != CFRK_SPAN_PREFIX && mode != CFRK_SPAN_LONGEST)
    return cfrk_fail(ctx, CFRK_ERR_ARG, "mode %d: CFRK_SPAN_PREFIX or CFRK_SPAN_LONGEST", mode);
  return CFRK_OK;
}

int cfrk_global_read_spans_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                                  int64_t nN, int64_t nS, uint32_t min_count, uint32_t max_count, int mode,
                                  cfrk_read_span *d_out) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = read_spans_check(ctx, nN, nS, d_data, d_start, d_length, d_out, mode);
  if (rc || nS == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cfrk_read_spans_launch(ctx, d_data, d_start, d_length, nN, nS, min_count, max_count, mode, d_out);
}

int cfrk_global_read_spans(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length, int64_t nN,
                           int64_t nS, uint32_t min_count, uint32_t max_count, int mode, cfrk_read_span *out) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = read_spans_check(ctx, nN, nS, data, start, length, out, mode);
  if (rc || nS == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // staged through the query calls' slots: the reads in, the spans out
  void *p_out;
  StagedReads d;
  if ((rc = cfrk_pool_get(ctx, BUF_QUERY_OUT, (size_t)nS * sizeof *out, &p_out))) return rc;
  if ((rc = stage_reads(ctx, BUF_QUERY_IN, data, start, length, nN, nS, STAGE_TABLE, nullptr, 0, &d))) return rc;
  if ((rc = cfrk_read_spans_launch(ctx, d.data, d.start, d.length, nN, nS, min_count, max_count, mode, (cfrk_read_span *)p_out))) return stage_drain(ctx, rc);
  return cfrk_memcpy_d2h(ctx, out, p_out, (size_t)nS * sizeof *out);
}

static_assert(sizeof(cfrk_read_fix) == 8, "cfrk_read_fix is 8 bytes without padding");

static int correct_check(cfrk_ctx *ctx, int64_t nN, int64_t nS, const void *data, const void *start, const void *length,
                         const void *data_out) {
  int rc = query_check(ctx, nN);
  if (rc) return rc;
  if (nS < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (nS > 0 && (!data || !start || !length)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  if (nN > 0 && (!data || !data_out)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL data buffer with nN > 0");
  return CFRK_OK;
}

// what both forms run on device buffers: the copy, then the kernels that store the corrected bases into it
static int correct_core(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                        int64_t nS, uint32_t min_count, int8_t *d_data_out, cfrk_read_fix *d_fix) {
  if (nN > 0) HIP_TRY(ctx, hipMemcpyAsync(d_data_out, d_data, (size_t)nN, hipMemcpyDeviceToDevice, ctx->stream));
  if (nS == 0) return CFRK_OK;
  return cfrk_read_correct_launch(ctx, d_data, d_start, d_length, nN, nS, min_count, d_data_out, d_fix);
}

int cfrk_global_correct_reads_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                                     int64_t nN, int64_t nS, uint32_t min_count, int8_t *d_data_out, cfrk_read_fix *d_fix) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = correct_check(ctx, nN, nS, d_data, d_start, d_length, d_data_out);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return correct_core(ctx, d_data, d_start, d_length, nN, nS, min_count, d_data_out, d_fix);
}

int cfrk_global_correct_reads(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length, int64_t nN,
                              int64_t nS, uint32_t min_count, int8_t *data_out, cfrk_read_fix *fix) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = correct_check(ctx, nN, nS, data, start, length, data_out);
  if (rc) return rc;
  if (nS == 0) {                                        // no read, nothing to look up: the bytes alone
    if (nN > 0) memcpy(data_out, data, (size_t)nN);
    return CFRK_OK;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // staged through the query calls' slot: the reads in, room for the corrected data and the rows behind them
  StagePart x[2] = {{nullptr, (size_t)nN, nullptr}, {nullptr, fix ? (size_t)nS * sizeof *fix : 0, nullptr}};
  StagedReads d;
  if ((rc = stage_reads(ctx, BUF_QUERY_IN, data, start, length, nN, nS, STAGE_TABLE, x, 2, &d))) return rc;
  if ((rc = correct_core(ctx, d.data, d.start, d.length, nN, nS, min_count, (int8_t *)x[0].dev, (cfrk_read_fix *)x[1].dev)))
    return stage_drain(ctx, rc);
  if (fix) HIP_TRY(ctx, hipMemcpyAsync(fix, x[1].dev, (size_t)nS * sizeof *fix, hipMemcpyDeviceToHost, ctx->stream));
  return cfrk_memcpy_d2h(ctx, data_out, x[0].dev, (size_t)nN);
}

static int select_check(cfrk_ctx *ctx, const void *data, const void *start, const void *length, int64_t nN, int64_t nS,
                        int32_t min_len, const void *data_out, uint64_t cap_data, const void *start_out,
                        const void *length_out, uint64_t cap_reads, int64_t *nN_out, int64_t *nS_out) {
  if (nN < 0 || nS < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (min_len < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "min_len %d is negative", (int)min_len);
  if (!nN_out || !nS_out) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL size output");
  if ((nS > 0 && (!start || !length)) || (nN > 0 && !data)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  if ((cap_data > 0 && !data_out) || (cap_reads > 0 && (!start_out || !length_out)))
    return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL array with a capacity above 0");
  *nN_out = *nS_out = 0;
  return CFRK_OK;
}

// measure, refuse or place the outputs, emit: what both forms run on device buffers
static int select_core(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN, int64_t nS,
                       const cfrk_read_span *d_span, const uint8_t *d_keep, int32_t min_len, ReadsOut *o, int64_t *nN_out,
                       int64_t *nS_out) {
  int64_t on = 0, os = 0;
  int rc = cfrk_select_measure(ctx, d_start, d_length, nN, nS, d_span, d_keep, min_len, &on, &os);
  if (rc || (rc = reads_out_fit(ctx, "select", *o, on, os, nN_out, nS_out)) || os == 0) return rc;
  if ((rc = reads_out_carve(ctx, o, on, os))) return rc;
  return cfrk_select_emit(ctx, d_data, d_start, d_length, nN, nS, d_span, d_keep, min_len, o->data, o->start, o->length, o->index, on, os);
}

int cfrk_reads_select_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                             int64_t nN, int64_t nS, const cfrk_read_span *d_span, const uint8_t *d_keep,
                             int32_t min_len, int8_t *d_data_out, uint64_t cap_data, int64_t *d_start_out,
                             int32_t *d_length_out, int64_t *d_index_out, uint64_t cap_reads, int64_t *nN_out,
                             int64_t *nS_out) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = select_check(ctx, d_data, d_start, d_length, nN, nS, min_len, d_data_out, cap_data, d_start_out, d_length_out,
                        cap_reads, nN_out, nS_out);
  if (rc || nS == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ReadsOut o = {d_data_out, d_start_out, d_length_out, d_index_out, cap_data, cap_reads, -1, false};
  return select_core(ctx, d_data, d_start, d_length, nN, nS, d_span, d_keep, min_len, &o, nN_out, nS_out);
}

int cfrk_reads_select(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length, int64_t nN,
                      int64_t nS, const cfrk_read_span *span, const uint8_t *keep, int32_t min_len, int8_t *data_out,
                      uint64_t cap_data, int64_t *start_out, int32_t *length_out, int64_t *index_out, uint64_t cap_reads,
                      int64_t *nN_out, int64_t *nS_out) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = select_check(ctx, data, start, length, nN, nS, min_len, data_out, cap_data, start_out, length_out, cap_reads,
                        nN_out, nS_out);
  if (rc || nS == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  StagePart x[2] = {{span, span ? (size_t)nS * sizeof(cfrk_read_span) : 0, nullptr}, {keep, keep ? (size_t)nS : 0, nullptr}};
  StagedReads d;
  if ((rc = stage_reads(ctx, BUF_SELECT_IN, data, start, length, nN, nS, STAGE_TABLE, x, 2, &d))) return rc;
  for (int64_t i = 0; span && i < nS; ++i) {
    const cfrk_read_span s = span[i];
    if (s.offset < 0 || s.length < 0 || (int64_t)s.offset + (int64_t)s.length > (int64_t)length[i]) {
      cfrk_fail(ctx, CFRK_ERR_LAYOUT, "read %lld: span {%d, %d} does not lie inside its %d bases", (long long)i, (int)s.offset,
                (int)s.length, (int)length[i]);
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // (the copies read the caller's buffers)
      return CFRK_ERR_LAYOUT;
    }
  }
  ReadsOut o = {nullptr, nullptr, nullptr, nullptr, cap_data, cap_reads, BUF_SELECT_OUT, true};
  rc = select_core(ctx, d.data, d.start, d.length, nN, nS, (const cfrk_read_span *)x[0].dev, (const uint8_t *)x[1].dev, min_len, &o, nN_out, nS_out);
  if (rc || *nS_out == 0) return stage_drain(ctx, rc);
  return download_reads(ctx, o, data_out, start_out, length_out, index_out, *nN_out, *nS_out);
}

/* ------------------------------------------------------------------ unitigs */

static_assert(sizeof(cfrk_unitig) == 16, "cfrk_unitig is 16 bytes without padding");

int cfrk_global_neighbors_device(cfrk_ctx *ctx, const uint64_t *d_keys_lo, const uint64_t *d_keys_hi, int64_t n,
                                 uint32_t min_count, uint8_t *d_masks) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = query_check(ctx, n);
  if (rc || n == 0) return rc;
  if (!d_keys_lo || !d_masks || (ctx->g_two && !d_keys_hi)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cfrk_neighbors_launch(ctx, d_keys_lo, d_keys_hi, n, min_count, d_masks);
}

int cfrk_global_neighbors(cfrk_ctx *ctx, const uint64_t *keys_lo, const uint64_t *keys_hi, int64_t n, uint32_t min_count,
                          uint8_t *masks) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = query_check(ctx, n);
  if (rc || n == 0) return rc;
  if (!keys_lo || !masks || (ctx->g_two && !keys_hi)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // staged through the query calls' slots: the keys in, the masks out
  void *d_in, *d_out;
  const size_t bytes = (size_t)n * 8;
  if ((rc = cfrk_pool_get(ctx, BUF_QUERY_IN, keys_hi ? 2 * bytes : bytes, &d_in))) return rc;
  if ((rc = cfrk_pool_get(ctx, BUF_QUERY_OUT, (size_t)n, &d_out))) return rc;
  uint64_t *d_lo = (uint64_t *)d_in, *d_hi = keys_hi ? d_lo + n : nullptr;
  HIP_TRY(ctx, hipMemcpyAsync(d_lo, keys_lo, bytes, hipMemcpyHostToDevice, ctx->stream));
  if (keys_hi) HIP_TRY(ctx, hipMemcpyAsync(d_hi, keys_hi, bytes, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = cfrk_neighbors_launch(ctx, d_lo, d_hi, n, min_count, (uint8_t *)d_out))) return stage_drain(ctx, rc);
  return cfrk_memcpy_d2h(ctx, masks, d_out, (size_t)n);
}

static int unitigs_check(cfrk_ctx *ctx, const void *data_out, uint64_t cap_data, const void *start_out, const void *length_out,
                         const void *rec_out, uint64_t cap_unitigs, int64_t *nN_out, int64_t *nS_out) {
  int rc = query_check(ctx, 0);
  if (rc) return rc;
  if (!nN_out || !nS_out) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL size output");
  if ((cap_data > 0 && !data_out) || (cap_unitigs > 0 && (!start_out || !length_out || !rec_out)))
    return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL array with a capacity above 0");
  *nN_out = *nS_out = 0;
  return CFRK_OK;
}

int cfrk_global_unitigs_device(cfrk_ctx *ctx, uint32_t min_count, int8_t *d_data_out, uint64_t cap_data, int64_t *d_start_out,
                               int32_t *d_length_out, cfrk_unitig *d_rec_out, uint64_t cap_unitigs, int64_t *nN_out,
                               int64_t *nS_out) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = unitigs_check(ctx, d_data_out, cap_data, d_start_out, d_length_out, d_rec_out, cap_unitigs, nN_out, nS_out);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int64_t nN = 0, nS = 0;
  uint64_t nseg = 0;
  if ((rc = cfrk_unitigs_measure(ctx, min_count, &nN, &nS, &nseg))) return rc;
  const ReadsOut o = {d_data_out, d_start_out, d_length_out, nullptr, cap_data, cap_unitigs, -1, false};
  if ((rc = reads_out_fit(ctx, "unitigs", o, nN, nS, nN_out, nS_out)) || nS == 0) return rc;
  return cfrk_unitigs_emit(ctx, d_data_out, d_start_out, d_length_out, d_rec_out, nS, nseg);
}

int cfrk_global_unitigs(cfrk_ctx *ctx, uint32_t min_count, int8_t *data_out, uint64_t cap_data, int64_t *start_out,
                        int32_t *length_out, cfrk_unitig *rec_out, uint64_t cap_unitigs, int64_t *nN_out, int64_t *nS_out) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = unitigs_check(ctx, data_out, cap_data, start_out, length_out, rec_out, cap_unitigs, nN_out, nS_out);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int64_t nN = 0, nS = 0;
  uint64_t nseg = 0;
  if ((rc = cfrk_unitigs_measure(ctx, min_count, &nN, &nS, &nseg))) return rc;
  const ReadsOut fit = {nullptr, nullptr, nullptr, nullptr, cap_data, cap_unitigs, BUF_UNITIG_OUT, false};
  if ((rc = reads_out_fit(ctx, "unitigs", fit, nN, nS, nN_out, nS_out)) || nS == 0) return rc;
  // [data | start | length | records] in a slot of their own, then down to the caller's arrays
  const size_t rec_bytes = (size_t)nS * sizeof(cfrk_unitig);
  const SlotCarve c((size_t)nN + 16, (uint64_t)nS, true, &rec_bytes, 1);
  void *p;
  if ((rc = cfrk_pool_get(ctx, BUF_UNITIG_OUT, c.total, &p))) return rc;
  ReadsOut o = fit;
  o.data = (int8_t *)p; o.start = carve_at<int64_t>(p, c.o_start); o.length = carve_at<int32_t>(p, c.o_length);
  cfrk_unitig *d_rec = carve_at<cfrk_unitig>(p, c.o_extra[0]);
  if ((rc = cfrk_unitigs_emit(ctx, o.data, o.start, o.length, d_rec, nS, nseg))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(rec_out, d_rec, rec_bytes, hipMemcpyDeviceToHost, ctx->stream));
  return download_reads(ctx, o, data_out, start_out, length_out, nullptr, nN, nS);
}

static_assert(sizeof(cfrk_unitig_link) == 8, "cfrk_unitig_link is 8 bytes without padding");

static int unitig_links_check(cfrk_ctx *ctx, const void *data, const void *start, const void *length, int64_t nN, int64_t nS,
                              const void *link_ptr, const void *links, uint64_t cap_links, int64_t *n_links_out) {
  int rc = query_check(ctx, 0);
  if (rc) return rc;
  if (nN < 0 || nS < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (!n_links_out) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL size output");
  if (!link_ptr) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL link_ptr");
  if (nS > 0 && (!data || !start || !length)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  if (cap_links > 0 && !links) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL array with a capacity above 0");
  if ((uint64_t)nS >= (1ull << 32)) return cfrk_fail(ctx, CFRK_ERR_ARG, "%lld unitigs: a link names its target in 32 bits", (long long)nS);
  *n_links_out = 0;
  return CFRK_OK;
}

static int unitig_links_fit(cfrk_ctx *ctx, int64_t n_links, uint64_t cap_links) {
  if ((uint64_t)n_links <= cap_links) return CFRK_OK;
  return cfrk_fail(ctx, CFRK_ERR_SMALL_BUF, "unitig links: %lld links, room for %llu", (long long)n_links, (unsigned long long)cap_links);
}

int cfrk_global_unitig_links_device(cfrk_ctx *ctx, uint32_t min_count, const int8_t *d_data, const int64_t *d_start,
                                    const int32_t *d_length, int64_t nN, int64_t nS, int64_t *d_link_ptr,
                                    cfrk_unitig_link *d_links, uint64_t cap_links, int64_t *n_links_out) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = unitig_links_check(ctx, d_data, d_start, d_length, nN, nS, d_link_ptr, d_links, cap_links, n_links_out);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (nS == 0) { HIP_TRY(ctx, hipMemsetAsync(d_link_ptr, 0, 8, ctx->stream)); return CFRK_OK; }
  if ((rc = cfrk_unitig_links_measure(ctx, min_count, d_data, d_start, d_length, nN, nS, d_link_ptr, n_links_out))) return rc;
  if ((rc = unitig_links_fit(ctx, *n_links_out, cap_links)) || *n_links_out == 0) return rc;
  return cfrk_unitig_links_fill(ctx, min_count, d_data, d_start, d_length, nN, nS, d_links);
}

int cfrk_global_unitig_links(cfrk_ctx *ctx, uint32_t min_count, const int8_t *data, const int64_t *start,
                             const int32_t *length, int64_t nN, int64_t nS, int64_t *link_ptr, cfrk_unitig_link *links,
                             uint64_t cap_links, int64_t *n_links_out) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = unitig_links_check(ctx, data, start, length, nN, nS, link_ptr, links, cap_links, n_links_out);
  if (rc) return rc;
  if (nS == 0) { link_ptr[0] = 0; return CFRK_OK; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // staged through the query calls' slots: the unitigs in with room for link_ptr behind them, the rows out
  const size_t ptr_bytes = ((size_t)nS + 1) * 8;
  StagePart x[1] = {{nullptr, ptr_bytes, nullptr}};
  StagedReads d;
  if ((rc = stage_reads(ctx, BUF_QUERY_IN, data, start, length, nN, nS, STAGE_TABLE, x, 1, &d))) return rc;
  if ((rc = cfrk_unitig_links_measure(ctx, min_count, d.data, d.start, d.length, nN, nS, (int64_t *)x[0].dev, n_links_out)))
    return stage_drain(ctx, rc);
  const int64_t n = *n_links_out;
  const int fit = unitig_links_fit(ctx, n, cap_links);
  if (fit || n == 0) {
    if ((rc = cfrk_memcpy_d2h(ctx, link_ptr, x[0].dev, ptr_bytes))) return rc;
    return fit;
  }
  void *d_links;
  if ((rc = cfrk_pool_get(ctx, BUF_QUERY_OUT, (size_t)n * sizeof *links, &d_links))) return rc;
  if ((rc = cfrk_unitig_links_fill(ctx, min_count, d.data, d.start, d.length, nN, nS, (cfrk_unitig_link *)d_links))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(link_ptr, x[0].dev, ptr_bytes, hipMemcpyDeviceToHost, ctx->stream));
  return cfrk_memcpy_d2h(ctx, links, d_links, (size_t)n * sizeof *links);
}

static_assert(sizeof(cfrk_unitig_pos) == 8, "cfrk_unitig_pos is 8 bytes without padding");
static_assert(sizeof(cfrk_read_hit) == 16, "cfrk_read_hit is 16 bytes without padding");

static int unitig_index_check(cfrk_ctx *ctx, const void *data, const void *start, const void *length, int64_t nN, int64_t nS) {
  int rc = query_check(ctx, 0);
  if (rc) return rc;
  if (nN < 0 || nS < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (nS > 0 && (!data || !start || !length)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  if ((uint64_t)nS >= (1ull << 32)) return cfrk_fail(ctx, CFRK_ERR_ARG, "%lld unitigs: a position names its unitig in 32 bits", (long long)nS);
  return CFRK_OK;
}

int cfrk_global_unitig_index_device(cfrk_ctx *ctx, uint32_t min_count, const int8_t *d_data, const int64_t *d_start,
                                    const int32_t *d_length, int64_t nN, int64_t nS) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = unitig_index_check(ctx, d_data, d_start, d_length, nN, nS);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cfrk_unitig_index_build(ctx, min_count, d_data, d_start, d_length, nN, nS);
}

int cfrk_global_unitig_index(cfrk_ctx *ctx, uint32_t min_count, const int8_t *data, const int64_t *start,
                             const int32_t *length, int64_t nN, int64_t nS) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = unitig_index_check(ctx, data, start, length, nN, nS);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (nS == 0) return cfrk_unitig_index_build(ctx, min_count, nullptr, nullptr, nullptr, 0, 0);
  // staged through the query calls' slot: the unitigs in
  StagedReads d;
  if ((rc = stage_reads(ctx, BUF_QUERY_IN, data, start, length, nN, nS, STAGE_TABLE, nullptr, 0, &d))) return rc;
  return stage_drain(ctx, cfrk_unitig_index_build(ctx, min_count, d.data, d.start, d.length, nN, nS));
}

int cfrk_global_locate_device(cfrk_ctx *ctx, const uint64_t *d_keys_lo, const uint64_t *d_keys_hi, int64_t n,
                              cfrk_unitig_pos *d_out) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = query_check(ctx, n);
  if (rc) return rc;
  if (n > 0 && (!d_keys_lo || !d_out || (ctx->g_two && !d_keys_hi))) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cfrk_unitig_locate_launch(ctx, d_keys_lo, d_keys_hi, n, d_out);
}

int cfrk_global_locate(cfrk_ctx *ctx, const uint64_t *keys_lo, const uint64_t *keys_hi, int64_t n, cfrk_unitig_pos *out) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = query_check(ctx, n);
  if (rc) return rc;
  if (n > 0 && (!keys_lo || !out || (ctx->g_two && !keys_hi))) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (n == 0) return cfrk_unitig_locate_launch(ctx, nullptr, nullptr, 0, nullptr);      // (the state is still checked)
  // staged through the query calls' slots: the keys in, the positions out
  void *d_in, *d_out;
  const size_t bytes = (size_t)n * 8;
  if ((rc = cfrk_pool_get(ctx, BUF_QUERY_IN, keys_hi ? 2 * bytes : bytes, &d_in))) return rc;
  if ((rc = cfrk_pool_get(ctx, BUF_QUERY_OUT, bytes, &d_out))) return rc;
  uint64_t *d_lo = (uint64_t *)d_in, *d_hi = keys_hi ? d_lo + n : nullptr;
  HIP_TRY(ctx, hipMemcpyAsync(d_lo, keys_lo, bytes, hipMemcpyHostToDevice, ctx->stream));
  if (keys_hi) HIP_TRY(ctx, hipMemcpyAsync(d_hi, keys_hi, bytes, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = cfrk_unitig_locate_launch(ctx, d_lo, d_hi, n, (cfrk_unitig_pos *)d_out))) return stage_drain(ctx, rc);
  return cfrk_memcpy_d2h(ctx, out, d_out, bytes);
}

static int read_hits_check(cfrk_ctx *ctx, const void *data, const void *start, const void *length, int64_t nN, int64_t nS,
                           const void *hit_ptr, const void *hits, uint64_t cap_hits, int64_t *n_hits_out) {
  int rc = query_check(ctx, 0);
  if (rc) return rc;
  if (nN < 0 || nS < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (!n_hits_out) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL size output");
  if (!hit_ptr) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL hit_ptr");
  if (nS > 0 && (!data || !start || !length)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  if (cap_hits > 0 && !hits) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL array with a capacity above 0");
  *n_hits_out = 0;
  return CFRK_OK;
}

static int read_hits_fit(cfrk_ctx *ctx, int64_t n_hits, uint64_t cap_hits) {
  if ((uint64_t)n_hits <= cap_hits) return CFRK_OK;
  return cfrk_fail(ctx, CFRK_ERR_SMALL_BUF, "read hits: %lld hits, room for %llu", (long long)n_hits, (unsigned long long)cap_hits);
}

int cfrk_global_read_hits_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                                 int64_t nN, int64_t nS, int64_t *d_hit_ptr, cfrk_read_hit *d_hits, uint64_t cap_hits,
                                 int64_t *n_hits_out) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = read_hits_check(ctx, d_data, d_start, d_length, nN, nS, d_hit_ptr, d_hits, cap_hits, n_hits_out);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if ((rc = cfrk_read_hits_count(ctx, d_data, d_start, d_length, nN, nS, d_hit_ptr, n_hits_out))) return rc;
  if ((rc = read_hits_fit(ctx, *n_hits_out, cap_hits)) || *n_hits_out == 0) return rc;
  return cfrk_read_hits_fill(ctx, d_data, d_start, d_length, nN, nS, d_hit_ptr, d_hits, *n_hits_out);
}

int cfrk_global_read_hits(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length, int64_t nN,
                          int64_t nS, int64_t *hit_ptr, cfrk_read_hit *hits, uint64_t cap_hits, int64_t *n_hits_out) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = read_hits_check(ctx, data, start, length, nN, nS, hit_ptr, hits, cap_hits, n_hits_out);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // staged through the query calls' slots: the reads in with room for hit_ptr behind them, the rows out
  const size_t ptr_bytes = ((size_t)nS + 1) * 8;
  StagePart x[1] = {{nullptr, ptr_bytes, nullptr}};
  StagedReads d;
  if ((rc = stage_reads(ctx, BUF_QUERY_IN, data, start, length, nN, nS, STAGE_TABLE, x, 1, &d))) return rc;
  if ((rc = cfrk_read_hits_count(ctx, d.data, d.start, d.length, nN, nS, (int64_t *)x[0].dev, n_hits_out)))
    return stage_drain(ctx, rc);
  const int64_t n = *n_hits_out;
  const int fit = read_hits_fit(ctx, n, cap_hits);
  if (fit || n == 0) {
    if ((rc = cfrk_memcpy_d2h(ctx, hit_ptr, x[0].dev, ptr_bytes))) return rc;
    return fit;
  }
  void *d_hits;
  if ((rc = cfrk_pool_get(ctx, BUF_QUERY_OUT, (size_t)n * sizeof *hits, &d_hits))) return rc;
  if ((rc = cfrk_read_hits_fill(ctx, d.data, d.start, d.length, nN, nS, (int64_t *)x[0].dev, (cfrk_read_hit *)d_hits, n))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(hit_ptr, x[0].dev, ptr_bytes, hipMemcpyDeviceToHost, ctx->stream));
  return cfrk_memcpy_d2h(ctx, hits, d_hits, (size_t)n * sizeof *hits);
}

/* ------------------------------------------------------------------ graph mask, tips and bubbles */

int cfrk_global_mask_keys_device(cfrk_ctx *ctx, const uint64_t *d_keys_lo, const uint64_t *d_keys_hi, int64_t n) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = query_check(ctx, n);
  if (rc) return rc;
  if (n > 0 && (!d_keys_lo || (ctx->g_two && !d_keys_hi))) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cfrk_mask_keys_launch(ctx, d_keys_lo, d_keys_hi, n);
}

int cfrk_global_mask_keys(cfrk_ctx *ctx, const uint64_t *keys_lo, const uint64_t *keys_hi, int64_t n) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = query_check(ctx, n);
  if (rc) return rc;
  if (n > 0 && (!keys_lo || (ctx->g_two && !keys_hi))) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (n == 0) return cfrk_mask_keys_launch(ctx, nullptr, nullptr, 0);
  // staged through the query calls' slot: the keys in
  void *d_in;
  const size_t bytes = (size_t)n * 8;
  if ((rc = cfrk_pool_get(ctx, BUF_QUERY_IN, keys_hi ? 2 * bytes : bytes, &d_in))) return rc;
  uint64_t *d_lo = (uint64_t *)d_in, *d_hi = keys_hi ? d_lo + n : nullptr;
  HIP_TRY(ctx, hipMemcpyAsync(d_lo, keys_lo, bytes, hipMemcpyHostToDevice, ctx->stream));
  if (keys_hi) HIP_TRY(ctx, hipMemcpyAsync(d_hi, keys_hi, bytes, hipMemcpyHostToDevice, ctx->stream));
  rc = cfrk_mask_keys_launch(ctx, d_lo, d_hi, n);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // (the copies read the caller's buffers)
  return rc;
}

static int mask_unitigs_check(cfrk_ctx *ctx, const void *data, const void *start, const void *length, int64_t nN, int64_t nS,
                              const void *drop) {
  int rc = query_check(ctx, 0);
  if (rc) return rc;
  if (nN < 0 || nS < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (nS > 0 && (!data || !start || !length || !drop)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  return CFRK_OK;
}

int cfrk_global_mask_unitigs_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                                    int64_t nN, int64_t nS, const uint8_t *d_drop) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = mask_unitigs_check(ctx, d_data, d_start, d_length, nN, nS, d_drop);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cfrk_mask_unitigs_launch(ctx, d_data, d_start, d_length, nN, nS, d_drop);
}

int cfrk_global_mask_unitigs(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length, int64_t nN,
                             int64_t nS, const uint8_t *drop) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = mask_unitigs_check(ctx, data, start, length, nN, nS, drop);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (nS == 0) return cfrk_mask_unitigs_launch(ctx, nullptr, nullptr, nullptr, 0, 0, nullptr);
  // staged through the query calls' slot: the unitigs in with the drop bytes behind them
  StagePart x[1] = {{drop, (size_t)nS, nullptr}};
  StagedReads d;
  if ((rc = stage_reads(ctx, BUF_QUERY_IN, data, start, length, nN, nS, STAGE_TABLE, x, 1, &d))) return rc;
  rc = cfrk_mask_unitigs_launch(ctx, d.data, d.start, d.length, nN, nS, (const uint8_t *)x[0].dev);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // (the copies read the caller's buffers)
  return rc;
}

int cfrk_global_mask_clear(cfrk_ctx *ctx) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = query_check(ctx, 0);
  if (rc) return rc;
  return cfrk_mask_clear_now(ctx);
}

int cfrk_global_mask_count(cfrk_ctx *ctx, uint64_t *n_masked) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = query_check(ctx, 0);
  if (rc) return rc;
  if (!n_masked) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL n_masked");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cfrk_mask_count_now(ctx, n_masked);
}

static int unitig_tips_check(cfrk_ctx *ctx, const void *rec, int64_t nS, const void *link_ptr, const void *links, int64_t n_links,
                             uint32_t ratio_q8, const void *tip, int64_t *n_tips_out) {
  if (!ctx->g_active) return cfrk_fail(ctx, CFRK_ERR_STATE, "unitig tips before begin: the job supplies the strand rule");
  if (nS < 0 || n_links < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (!n_tips_out) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL n_tips_out");
  if (nS > 0 && (!rec || !link_ptr || !tip)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  if (n_links > 0 && !links) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL links with n_links above 0");
  if ((uint64_t)nS >= (1ull << 32)) return cfrk_fail(ctx, CFRK_ERR_ARG, "%lld unitigs: a link names its target in 32 bits", (long long)nS);
  if (ratio_q8 > CFRK_TIP_RATIO_Q8_MAX) return cfrk_fail(ctx, CFRK_ERR_ARG, "ratio_q8 %u: at most %d", ratio_q8, CFRK_TIP_RATIO_Q8_MAX);
  *n_tips_out = 0;
  return CFRK_OK;
}

int cfrk_global_unitig_tips_device(cfrk_ctx *ctx, const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr,
                                   const cfrk_unitig_link *d_links, int64_t n_links, uint32_t max_kmers, uint32_t ratio_q8,
                                   uint8_t *d_tip, int64_t *n_tips_out) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = unitig_tips_check(ctx, d_rec, nS, d_link_ptr, d_links, n_links, ratio_q8, d_tip, n_tips_out);
  if (rc || nS == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cfrk_unitig_tips_launch(ctx, d_rec, nS, d_link_ptr, d_links, n_links, max_kmers, ratio_q8, d_tip, n_tips_out);
}

int cfrk_global_unitig_tips(cfrk_ctx *ctx, const cfrk_unitig *rec, int64_t nS, const int64_t *link_ptr,
                            const cfrk_unitig_link *links, int64_t n_links, uint32_t max_kmers, uint32_t ratio_q8, uint8_t *tip,
                            int64_t *n_tips_out) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = unitig_tips_check(ctx, rec, nS, link_ptr, links, n_links, ratio_q8, tip, n_tips_out);
  if (rc || nS == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // [records | link_ptr | links] in a slot of their own, the tip bytes in another
  Carve c;
  const size_t rec_bytes = (size_t)nS * sizeof *rec, ptr_bytes = ((size_t)nS + 1) * 8, link_bytes = (size_t)n_links * sizeof *links;
  const size_t o_rec = c.part(rec_bytes), o_ptr = c.part(ptr_bytes), o_links = c.part(link_bytes);
  void *d_in, *d_out;
  if ((rc = cfrk_pool_get(ctx, BUF_UNITIG_TIPS_IN, c.end, &d_in))) return rc;
  if ((rc = cfrk_pool_get(ctx, BUF_UNITIG_TIPS_OUT, (size_t)nS, &d_out))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(carve_at<void>(d_in, o_rec), rec, rec_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(carve_at<void>(d_in, o_ptr), link_ptr, ptr_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (n_links) HIP_TRY(ctx, hipMemcpyAsync(carve_at<void>(d_in, o_links), links, link_bytes, hipMemcpyHostToDevice, ctx->stream));
  rc = cfrk_unitig_tips_launch(ctx, carve_at<cfrk_unitig>(d_in, o_rec), nS, carve_at<int64_t>(d_in, o_ptr),
                               carve_at<cfrk_unitig_link>(d_in, o_links), n_links, max_kmers, ratio_q8, (uint8_t *)d_out, n_tips_out);
  if (rc) return stage_drain(ctx, rc);
  return cfrk_memcpy_d2h(ctx, tip, d_out, (size_t)nS);
}

static int unitig_bubbles_check(cfrk_ctx *ctx, const void *rec, int64_t nS, const void *link_ptr, const void *links, int64_t n_links,
                                uint32_t ratio_q8, const void *pop, int64_t *n_pop_out) {
  if (!ctx->g_active) return cfrk_fail(ctx, CFRK_ERR_STATE, "unitig bubbles before begin: the job supplies the strand rule");
  if (nS < 0 || n_links < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (!n_pop_out) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL n_pop_out");
  if (nS > 0 && (!rec || !link_ptr || !pop)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  if (n_links > 0 && !links) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL links with n_links above 0");
  if ((uint64_t)nS >= (1ull << 31)) return cfrk_fail(ctx, CFRK_ERR_ARG, "%lld unitigs: a partner names an oriented unitig in 32 bits", (long long)nS);
  if (ratio_q8 > CFRK_TIP_RATIO_Q8_MAX) return cfrk_fail(ctx, CFRK_ERR_ARG, "ratio_q8 %u: at most %d", ratio_q8, CFRK_TIP_RATIO_Q8_MAX);
  *n_pop_out = 0;
  return CFRK_OK;
}

int cfrk_global_unitig_bubbles_device(cfrk_ctx *ctx, const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr,
                                      const cfrk_unitig_link *d_links, int64_t n_links, uint32_t max_kmers, uint32_t max_diff,
                                      uint32_t ratio_q8, uint8_t *d_pop, uint32_t *d_partner, int64_t *n_pop_out) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = unitig_bubbles_check(ctx, d_rec, nS, d_link_ptr, d_links, n_links, ratio_q8, d_pop, n_pop_out);
  if (rc || nS == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cfrk_unitig_bubbles_launch(ctx, d_rec, nS, d_link_ptr, d_links, n_links, max_kmers, max_diff, ratio_q8, d_pop, d_partner, n_pop_out);
}

int cfrk_global_unitig_bubbles(cfrk_ctx *ctx, const cfrk_unitig *rec, int64_t nS, const int64_t *link_ptr,
                               const cfrk_unitig_link *links, int64_t n_links, uint32_t max_kmers, uint32_t max_diff,
                               uint32_t ratio_q8, uint8_t *pop, uint32_t *partner, int64_t *n_pop_out) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = unitig_bubbles_check(ctx, rec, nS, link_ptr, links, n_links, ratio_q8, pop, n_pop_out);
  if (rc || nS == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // [records | link_ptr | links] in a slot of their own, [pop bytes | partners] in another
  Carve c, co;
  const size_t rec_bytes = (size_t)nS * sizeof *rec, ptr_bytes = ((size_t)nS + 1) * 8, link_bytes = (size_t)n_links * sizeof *links;
  const size_t o_rec = c.part(rec_bytes), o_ptr = c.part(ptr_bytes), o_links = c.part(link_bytes);
  const size_t o_pop = co.part((size_t)nS), o_partner = co.part(partner ? (size_t)nS * 4 : 0);
  void *d_in, *d_out;
  if ((rc = cfrk_pool_get(ctx, BUF_UNITIG_BUBBLES_IN, c.end, &d_in))) return rc;
  if ((rc = cfrk_pool_get(ctx, BUF_UNITIG_BUBBLES_OUT, co.end, &d_out))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(carve_at<void>(d_in, o_rec), rec, rec_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(carve_at<void>(d_in, o_ptr), link_ptr, ptr_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (n_links) HIP_TRY(ctx, hipMemcpyAsync(carve_at<void>(d_in, o_links), links, link_bytes, hipMemcpyHostToDevice, ctx->stream));
  uint32_t *d_partner = partner ? carve_at<uint32_t>(d_out, o_partner) : nullptr;
  rc = cfrk_unitig_bubbles_launch(ctx, carve_at<cfrk_unitig>(d_in, o_rec), nS, carve_at<int64_t>(d_in, o_ptr),
                                  carve_at<cfrk_unitig_link>(d_in, o_links), n_links, max_kmers, max_diff, ratio_q8,
                                  carve_at<uint8_t>(d_out, o_pop), d_partner, n_pop_out);
  if (rc) {                                            // refused: pop all 0, no partner
    memset(pop, 0, (size_t)nS);
    if (partner) memset(partner, 0xFF, (size_t)nS * 4);
    return stage_drain(ctx, rc);
  }
  if (partner) HIP_TRY(ctx, hipMemcpyAsync(partner, d_partner, (size_t)nS * 4, hipMemcpyDeviceToHost, ctx->stream));
  return cfrk_memcpy_d2h(ctx, pop, carve_at<uint8_t>(d_out, o_pop), (size_t)nS);
}

static_assert(sizeof(cfrk_bulge_stats) == 24, "cfrk_bulge_stats is 24 bytes without padding");

static int unitig_bulges_check(cfrk_ctx *ctx, const void *rec, int64_t nS, const void *link_ptr, const void *links, int64_t n_links,
                               const cfrk_bulge_params &p, const void *pop, const void *path_ptr, const void *path, uint64_t cap_path,
                               int64_t *n_path_out, cfrk_bulge_stats *stats) {
  if (!ctx->g_active) return cfrk_fail(ctx, CFRK_ERR_STATE, "unitig bulges before begin: the job supplies the strand rule");
  if (nS < 0 || n_links < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (!stats) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL stats");
  if (path_ptr && !n_path_out) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL n_path_out with path_ptr");
  if (nS > 0 && (!rec || !link_ptr || !pop)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  if (n_links > 0 && !links) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL links with n_links above 0");
  if (path_ptr && cap_path > 0 && !path) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL array with a capacity above 0");
  if ((uint64_t)nS >= (1ull << 31)) return cfrk_fail(ctx, CFRK_ERR_ARG, "%lld unitigs: a path names an oriented unitig in 32 bits", (long long)nS);
  if (p.max_hops > CFRK_BULGE_MAX_HOPS) return cfrk_fail(ctx, CFRK_ERR_ARG, "max_hops %u: at most %d", p.max_hops, CFRK_BULGE_MAX_HOPS);
  if (p.max_visits > CFRK_BULGE_MAX_VISITS) return cfrk_fail(ctx, CFRK_ERR_ARG, "max_visits %u: at most %d", p.max_visits, CFRK_BULGE_MAX_VISITS);
  if (p.ratio_q8 > CFRK_TIP_RATIO_Q8_MAX) return cfrk_fail(ctx, CFRK_ERR_ARG, "ratio_q8 %u: at most %d", p.ratio_q8, CFRK_TIP_RATIO_Q8_MAX);
  if (n_path_out) *n_path_out = 0;
  stats->arms = stats->popped = stats->undecided = 0;
  return CFRK_OK;
}

static int unitig_bulges_fit(cfrk_ctx *ctx, int64_t n_path, uint64_t cap_path) {
  if ((uint64_t)n_path <= cap_path) return CFRK_OK;
  return cfrk_fail(ctx, CFRK_ERR_SMALL_BUF, "unitig bulges: %lld path entries, room for %llu", (long long)n_path, (unsigned long long)cap_path);
}

int cfrk_global_unitig_bulges_device(cfrk_ctx *ctx, const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr,
                                     const cfrk_unitig_link *d_links, int64_t n_links, uint32_t max_kmers, uint32_t max_diff,
                                     uint32_t max_hops, uint32_t max_visits, uint32_t ratio_q8, uint8_t *d_pop, uint32_t *d_visits,
                                     int64_t *d_path_ptr, uint32_t *d_path, uint64_t cap_path, int64_t *n_path_out,
                                     cfrk_bulge_stats *stats) {
  if (!ctx) return CFRK_ERR_ARG;
  const cfrk_bulge_params p = {max_kmers, max_diff, max_hops, max_visits, ratio_q8};
  int rc = unitig_bulges_check(ctx, d_rec, nS, d_link_ptr, d_links, n_links, p, d_pop, d_path_ptr, d_path, cap_path, n_path_out, stats);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (nS == 0) {
    if (d_path_ptr) HIP_TRY(ctx, hipMemsetAsync(d_path_ptr, 0, 8, ctx->stream));
    return CFRK_OK;
  }
  int64_t n_path = 0;
  if ((rc = cfrk_unitig_bulges_search(ctx, d_rec, nS, d_link_ptr, d_links, n_links, p, d_pop, d_visits, d_path_ptr, stats, &n_path))) return rc;
  if (!d_path_ptr) return CFRK_OK;
  *n_path_out = n_path;
  if ((rc = unitig_bulges_fit(ctx, n_path, cap_path)) || n_path == 0) return rc;
  return cfrk_unitig_bulges_fill(ctx, d_rec, nS, d_link_ptr, d_links, n_links, p, stats->popped, d_path_ptr, d_path);
}

int cfrk_global_unitig_bulges(cfrk_ctx *ctx, const cfrk_unitig *rec, int64_t nS, const int64_t *link_ptr,
                              const cfrk_unitig_link *links, int64_t n_links, uint32_t max_kmers, uint32_t max_diff,
                              uint32_t max_hops, uint32_t max_visits, uint32_t ratio_q8, uint8_t *pop, uint32_t *visits,
                              int64_t *path_ptr, uint32_t *path, uint64_t cap_path, int64_t *n_path_out, cfrk_bulge_stats *stats) {
  if (!ctx) return CFRK_ERR_ARG;
  const cfrk_bulge_params p = {max_kmers, max_diff, max_hops, max_visits, ratio_q8};
  int rc = unitig_bulges_check(ctx, rec, nS, link_ptr, links, n_links, p, pop, path_ptr, path, cap_path, n_path_out, stats);
  if (rc) return rc;
  if (nS == 0) {
    if (path_ptr) path_ptr[0] = 0;
    return CFRK_OK;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // [records | link_ptr | links] in a slot of their own, [path_ptr | visits | pop] in another, the paths in a third
  Carve c, co;
  const size_t rec_bytes = (size_t)nS * sizeof *rec, ptr_bytes = ((size_t)nS + 1) * 8, link_bytes = (size_t)n_links * sizeof *links;
  const size_t o_rec = c.part(rec_bytes), o_ptr = c.part(ptr_bytes), o_links = c.part(link_bytes);
  const size_t o_pptr = co.part(path_ptr ? ptr_bytes : 0), o_visits = co.part(visits ? (size_t)nS * 4 : 0), o_pop = co.part((size_t)nS);
  void *d_in, *d_out;
  if ((rc = cfrk_pool_get(ctx, BUF_UNITIG_BULGES_IN, c.end, &d_in))) return rc;
  if ((rc = cfrk_pool_get(ctx, BUF_UNITIG_BULGES_OUT, co.end, &d_out))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(carve_at<void>(d_in, o_rec), rec, rec_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(carve_at<void>(d_in, o_ptr), link_ptr, ptr_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (n_links) HIP_TRY(ctx, hipMemcpyAsync(carve_at<void>(d_in, o_links), links, link_bytes, hipMemcpyHostToDevice, ctx->stream));
  const cfrk_unitig *d_rec = carve_at<cfrk_unitig>(d_in, o_rec);
  const int64_t *d_link_ptr = carve_at<int64_t>(d_in, o_ptr);
  const cfrk_unitig_link *d_links = carve_at<cfrk_unitig_link>(d_in, o_links);
  uint8_t *d_pop = carve_at<uint8_t>(d_out, o_pop);
  uint32_t *d_visits = visits ? carve_at<uint32_t>(d_out, o_visits) : nullptr;
  int64_t *d_path_ptr = path_ptr ? carve_at<int64_t>(d_out, o_pptr) : nullptr;
  int64_t n_path = 0;
  rc = cfrk_unitig_bulges_search(ctx, d_rec, nS, d_link_ptr, d_links, n_links, p, d_pop, d_visits, d_path_ptr, stats, &n_path);
  if (rc) {                                            // refused: everything 0
    memset(pop, 0, (size_t)nS);
    if (visits) memset(visits, 0, (size_t)nS * 4);
    if (path_ptr) memset(path_ptr, 0, ptr_bytes);
    return stage_drain(ctx, rc);
  }
  if (visits) HIP_TRY(ctx, hipMemcpyAsync(visits, d_visits, (size_t)nS * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (path_ptr) HIP_TRY(ctx, hipMemcpyAsync(path_ptr, d_path_ptr, ptr_bytes, hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = cfrk_memcpy_d2h(ctx, pop, d_pop, (size_t)nS))) return rc;
  if (!path_ptr) return CFRK_OK;
  *n_path_out = n_path;
  if ((rc = unitig_bulges_fit(ctx, n_path, cap_path)) || n_path == 0) return rc;
  void *d_path;
  if ((rc = cfrk_pool_get(ctx, BUF_UNITIG_BULGES_PATH, (size_t)n_path * 4, &d_path))) return rc;
  if ((rc = cfrk_unitig_bulges_fill(ctx, d_rec, nS, d_link_ptr, d_links, n_links, p, stats->popped, d_path_ptr, (uint32_t *)d_path))) return rc;
  return cfrk_memcpy_d2h(ctx, path, d_path, (size_t)n_path * 4);
}

static_assert(sizeof(cfrk_weak_stats) == 24, "cfrk_weak_stats is 24 bytes without padding");

static int unitig_weak_check(cfrk_ctx *ctx, const void *rec, int64_t nS, const void *link_ptr, const void *links, int64_t n_links,
                             uint32_t ratio_q8, const void *weak, cfrk_weak_stats *stats) {
  if (!ctx->g_active) return cfrk_fail(ctx, CFRK_ERR_STATE, "weak unitigs before begin: the job supplies the strand rule");
  if (nS < 0 || n_links < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (!stats) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL stats");
  if (nS > 0 && (!rec || !link_ptr || !weak)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  if (n_links > 0 && !links) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL links with n_links above 0");
  if ((uint64_t)nS >= (1ull << 32)) return cfrk_fail(ctx, CFRK_ERR_ARG, "%lld unitigs: a link names its target in 32 bits", (long long)nS);
  if (ratio_q8 > CFRK_TIP_RATIO_Q8_MAX) return cfrk_fail(ctx, CFRK_ERR_ARG, "ratio_q8 %u: at most %d", ratio_q8, CFRK_TIP_RATIO_Q8_MAX);
  stats->connections = stats->isolated = stats->candidates = 0;
  return CFRK_OK;
}

int cfrk_global_unitig_weak_device(cfrk_ctx *ctx, const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr,
                                   const cfrk_unitig_link *d_links, int64_t n_links, uint32_t max_kmers, uint32_t ratio_q8,
                                   uint32_t iso_max_kmers, uint32_t iso_mean_q8, uint8_t *d_weak, cfrk_weak_stats *stats) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = unitig_weak_check(ctx, d_rec, nS, d_link_ptr, d_links, n_links, ratio_q8, d_weak, stats);
  if (rc || nS == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cfrk_unitig_weak_launch(ctx, d_rec, nS, d_link_ptr, d_links, n_links, max_kmers, ratio_q8, iso_max_kmers, iso_mean_q8, d_weak, stats);
}

int cfrk_global_unitig_weak(cfrk_ctx *ctx, const cfrk_unitig *rec, int64_t nS, const int64_t *link_ptr,
                            const cfrk_unitig_link *links, int64_t n_links, uint32_t max_kmers, uint32_t ratio_q8,
                            uint32_t iso_max_kmers, uint32_t iso_mean_q8, uint8_t *weak, cfrk_weak_stats *stats) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = unitig_weak_check(ctx, rec, nS, link_ptr, links, n_links, ratio_q8, weak, stats);
  if (rc || nS == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // [records | link_ptr | links] in a slot of their own, the weak bytes in another
  Carve c;
  const size_t rec_bytes = (size_t)nS * sizeof *rec, ptr_bytes = ((size_t)nS + 1) * 8, link_bytes = (size_t)n_links * sizeof *links;
  const size_t o_rec = c.part(rec_bytes), o_ptr = c.part(ptr_bytes), o_links = c.part(link_bytes);
  void *d_in, *d_out;
  if ((rc = cfrk_pool_get(ctx, BUF_UNITIG_WEAK_IN, c.end, &d_in))) return rc;
  if ((rc = cfrk_pool_get(ctx, BUF_UNITIG_WEAK_OUT, (size_t)nS, &d_out))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(carve_at<void>(d_in, o_rec), rec, rec_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(carve_at<void>(d_in, o_ptr), link_ptr, ptr_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (n_links) HIP_TRY(ctx, hipMemcpyAsync(carve_at<void>(d_in, o_links), links, link_bytes, hipMemcpyHostToDevice, ctx->stream));
  rc = cfrk_unitig_weak_launch(ctx, carve_at<cfrk_unitig>(d_in, o_rec), nS, carve_at<int64_t>(d_in, o_ptr),
                               carve_at<cfrk_unitig_link>(d_in, o_links), n_links, max_kmers, ratio_q8, iso_max_kmers, iso_mean_q8,
                               (uint8_t *)d_out, stats);
  if (rc) {                                            // refused: weak all 0
    memset(weak, 0, (size_t)nS);
    return stage_drain(ctx, rc);
  }
  return cfrk_memcpy_d2h(ctx, weak, d_out, (size_t)nS);
}

static int unitigs_compact_check(cfrk_ctx *ctx, const cfrk_unitigs_in &in, const void *data_out, uint64_t cap_data,
                                 const void *start_out, const void *length_out, const void *rec_out, uint64_t cap_unitigs,
                                 int64_t *nN_out, int64_t *nS_out) {
  if (!ctx->g_active) return cfrk_fail(ctx, CFRK_ERR_STATE, "unitig compaction before begin: the job supplies k and the strand rule");
  if (!nN_out || !nS_out) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL size output");
  if (in.nN < 0 || in.nS < 0 || in.n_links < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (in.nS > 0 && (!in.data || !in.start || !in.length || !in.rec || !in.link_ptr)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  if (in.n_links > 0 && !in.links) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL links with n_links above 0");
  if ((cap_data > 0 && !data_out) || (cap_unitigs > 0 && (!start_out || !length_out || !rec_out)))
    return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL array with a capacity above 0");
  if ((uint64_t)in.nS >= (1ull << 31)) return cfrk_fail(ctx, CFRK_ERR_ARG, "%lld unitigs: an oriented unitig is named in 32 bits", (long long)in.nS);
  *nN_out = *nS_out = 0;
  return CFRK_OK;
}

int cfrk_global_unitigs_compact_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                                       const cfrk_unitig *d_rec, int64_t nN, int64_t nS, const int64_t *d_link_ptr,
                                       const cfrk_unitig_link *d_links, int64_t n_links, const uint8_t *d_drop, int8_t *d_data_out,
                                       uint64_t cap_data, int64_t *d_start_out, int32_t *d_length_out, cfrk_unitig *d_rec_out,
                                       uint64_t cap_unitigs, cfrk_unitig_pos *d_into, int64_t *nN_out, int64_t *nS_out) {
  if (!ctx) return CFRK_ERR_ARG;
  const cfrk_unitigs_in in = {d_data, d_start, d_length, d_rec, nN, nS, d_link_ptr, d_links, n_links, d_drop};
  int rc = unitigs_compact_check(ctx, in, d_data_out, cap_data, d_start_out, d_length_out, d_rec_out, cap_unitigs, nN_out, nS_out);
  if (rc || nS == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int64_t nN_new = 0, nS_new = 0;
  if ((rc = cfrk_unitigs_compact_measure(ctx, in, &nN_new, &nS_new))) return rc;
  const ReadsOut o = {d_data_out, d_start_out, d_length_out, nullptr, cap_data, cap_unitigs, -1, false};
  if ((rc = reads_out_fit(ctx, "unitig compaction", o, nN_new, nS_new, nN_out, nS_out))) return rc;
  if (nS_new == 0) {                                   // everything dropped
    if (d_into) HIP_TRY(ctx, hipMemsetAsync(d_into, 0xFF, (size_t)nS * sizeof *d_into, ctx->stream));
    return CFRK_OK;
  }
  return cfrk_unitigs_compact_emit(ctx, in, d_data_out, d_start_out, d_length_out, d_rec_out, d_into, nN_new, nS_new);
}

int cfrk_global_unitigs_compact(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length,
                                const cfrk_unitig *rec, int64_t nN, int64_t nS, const int64_t *link_ptr,
                                const cfrk_unitig_link *links, int64_t n_links, const uint8_t *drop, int8_t *data_out,
                                uint64_t cap_data, int64_t *start_out, int32_t *length_out, cfrk_unitig *rec_out,
                                uint64_t cap_unitigs, cfrk_unitig_pos *into, int64_t *nN_out, int64_t *nS_out) {
  if (!ctx) return CFRK_ERR_ARG;
  const cfrk_unitigs_in host = {data, start, length, rec, nN, nS, link_ptr, links, n_links, drop};
  int rc = unitigs_compact_check(ctx, host, data_out, cap_data, start_out, length_out, rec_out, cap_unitigs, nN_out, nS_out);
  if (rc || nS == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // [data | start | length | records | link_ptr | links | drop] in a slot of their own
  StagePart x[4] = {{rec, (size_t)nS * sizeof *rec, nullptr}, {link_ptr, ((size_t)nS + 1) * 8, nullptr},
                    {links, (size_t)n_links * sizeof *links, nullptr}, {drop, drop ? (size_t)nS : 0, nullptr}};
  StagedReads d;
  if ((rc = stage_reads(ctx, BUF_UNITIG_COMPACT_IN, data, start, length, nN, nS, STAGE_TABLE, x, 4, &d))) return rc;
  const cfrk_unitigs_in in = {d.data, d.start, d.length, (const cfrk_unitig *)x[0].dev, nN, nS, (const int64_t *)x[1].dev,
                              (const cfrk_unitig_link *)x[2].dev, n_links, (const uint8_t *)x[3].dev};
  int64_t nN_new = 0, nS_new = 0;
  if ((rc = cfrk_unitigs_compact_measure(ctx, in, &nN_new, &nS_new))) return stage_drain(ctx, rc);
  const ReadsOut fit = {nullptr, nullptr, nullptr, nullptr, cap_data, cap_unitigs, BUF_UNITIG_COMPACT_OUT, false};
  if ((rc = reads_out_fit(ctx, "unitig compaction", fit, nN_new, nS_new, nN_out, nS_out))) return rc;
  if (nS_new == 0) {
    if (into) memset(into, 0xFF, (size_t)nS * sizeof *into);
    return CFRK_OK;
  }
  // [data | start | length | records | into] in another, then down to the caller's arrays
  const size_t xb[2] = {(size_t)nS_new * sizeof(cfrk_unitig), into ? (size_t)nS * sizeof *into : 0};
  const SlotCarve c((size_t)nN_new + 16, (uint64_t)nS_new, true, xb, 2);
  void *p;
  if ((rc = cfrk_pool_get(ctx, BUF_UNITIG_COMPACT_OUT, c.total, &p))) return rc;
  ReadsOut o = fit;
  o.data = (int8_t *)p; o.start = carve_at<int64_t>(p, c.o_start); o.length = carve_at<int32_t>(p, c.o_length);
  cfrk_unitig *d_rec = carve_at<cfrk_unitig>(p, c.o_extra[0]);
  cfrk_unitig_pos *d_into = into ? carve_at<cfrk_unitig_pos>(p, c.o_extra[1]) : nullptr;
  if ((rc = cfrk_unitigs_compact_emit(ctx, in, o.data, o.start, o.length, d_rec, d_into, nN_new, nS_new))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(rec_out, d_rec, xb[0], hipMemcpyDeviceToHost, ctx->stream));
  if (into) HIP_TRY(ctx, hipMemcpyAsync(into, d_into, xb[1], hipMemcpyDeviceToHost, ctx->stream));
  return download_reads(ctx, o, data_out, start_out, length_out, nullptr, nN_new, nS_new);
}

static_assert(sizeof(cfrk_read_path) == 16, "cfrk_read_path is 16 bytes without padding");
static_assert(sizeof(cfrk_path_stats) == 32, "cfrk_path_stats is 32 bytes without padding");

static int read_paths_check(cfrk_ctx *ctx, const cfrk_read_paths_in &in, const void *path_ptr, const void *paths, uint64_t cap_paths,
                            int64_t *n_paths_out, cfrk_path_stats *stats) {
  if (!ctx->g_active) return cfrk_fail(ctx, CFRK_ERR_STATE, "read paths before begin: the job supplies the strand rule");
  if (in.nR < 0 || in.n_hits < 0 || in.nS < 0 || in.n_links < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (!n_paths_out) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL n_paths_out");
  if (!stats) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL stats");
  if (!in.d_hit_ptr || !path_ptr) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL hit_ptr or path_ptr");
  if (in.n_hits > 0 && !in.d_hits) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL hits with n_hits above 0");
  if (in.nS > 0 && (!in.d_rec || !in.d_link_ptr)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  if (in.n_links > 0 && !in.d_links) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL links with n_links above 0");
  if (cap_paths > 0 && !paths) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL array with a capacity above 0");
  if ((uint64_t)in.nS >= (1ull << 32)) return cfrk_fail(ctx, CFRK_ERR_ARG, "%lld unitigs: a hit names its unitig in 32 bits", (long long)in.nS);
  if ((uint64_t)in.n_hits >= (1ull << 32)) return cfrk_fail(ctx, CFRK_ERR_ARG, "%lld hits: support counts in 32 bits", (long long)in.n_hits);
  *n_paths_out = 0;
  stats->n_paths = stats->n_steps = stats->n_gaps = stats->n_unlinked = 0;
  return CFRK_OK;
}

static int read_paths_fit(cfrk_ctx *ctx, int64_t n_paths, uint64_t cap_paths) {
  if ((uint64_t)n_paths <= cap_paths) return CFRK_OK;
  return cfrk_fail(ctx, CFRK_ERR_SMALL_BUF, "read paths: %lld paths, room for %llu", (long long)n_paths, (unsigned long long)cap_paths);
}

int cfrk_global_read_paths_device(cfrk_ctx *ctx, const int64_t *d_hit_ptr, int64_t nR, const cfrk_read_hit *d_hits, int64_t n_hits,
                                  const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr, const cfrk_unitig_link *d_links,
                                  int64_t n_links, int64_t *d_path_ptr, cfrk_read_path *d_paths, uint64_t cap_paths,
                                  int64_t *n_paths_out, uint32_t *d_support, cfrk_path_stats *stats) {
  if (!ctx) return CFRK_ERR_ARG;
  const cfrk_read_paths_in in = {d_hit_ptr, nR, d_hits, n_hits, d_rec, nS, d_link_ptr, d_links, n_links};
  int rc = read_paths_check(ctx, in, d_path_ptr, d_paths, cap_paths, n_paths_out, stats);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int64_t n_paths = 0;
  if ((rc = cfrk_read_paths_measure(ctx, in, d_path_ptr, d_support, &n_paths, stats))) return rc;
  *n_paths_out = n_paths;
  if ((rc = read_paths_fit(ctx, n_paths, cap_paths)) || n_paths == 0) return rc;
  return cfrk_read_paths_fill(ctx, in, d_paths, n_paths);
}

int cfrk_global_read_paths(cfrk_ctx *ctx, const int64_t *hit_ptr, int64_t nR, const cfrk_read_hit *hits, int64_t n_hits,
                           const cfrk_unitig *rec, int64_t nS, const int64_t *link_ptr, const cfrk_unitig_link *links,
                           int64_t n_links, int64_t *path_ptr, cfrk_read_path *paths, uint64_t cap_paths, int64_t *n_paths_out,
                           uint32_t *support, cfrk_path_stats *stats) {
  if (!ctx) return CFRK_ERR_ARG;
  const cfrk_read_paths_in host = {hit_ptr, nR, hits, n_hits, rec, nS, link_ptr, links, n_links};
  int rc = read_paths_check(ctx, host, path_ptr, paths, cap_paths, n_paths_out, stats);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // [hit_ptr | hits | records | link_ptr | links | support] in a slot of their own, [path_ptr | paths] in another
  Carve c;
  const size_t hptr_bytes = ((size_t)nR + 1) * 8, hit_bytes = (size_t)n_hits * sizeof *hits, rec_bytes = (size_t)nS * sizeof *rec,
               lptr_bytes = nS ? ((size_t)nS + 1) * 8 : 0, link_bytes = (size_t)n_links * sizeof *links,
               sup_bytes = support ? (size_t)n_links * 4 : 0;
  const size_t o_hptr = c.part(hptr_bytes), o_hits = c.part(hit_bytes), o_rec = c.part(rec_bytes), o_lptr = c.part(lptr_bytes),
               o_links = c.part(link_bytes), o_sup = c.part(sup_bytes);
  void *d_in, *d_out;
  if ((rc = cfrk_pool_get(ctx, BUF_READ_PATHS_IN, c.end, &d_in))) return rc;
  const struct { size_t off, bytes; const void *src; } up[6] = {{o_hptr, hptr_bytes, hit_ptr}, {o_hits, hit_bytes, hits}, {o_rec, rec_bytes, rec},
                                                               {o_lptr, lptr_bytes, link_ptr}, {o_links, link_bytes, links},
                                                               {o_sup, sup_bytes, support}};
  for (const auto &u : up)
    if (u.bytes) HIP_TRY(ctx, hipMemcpyAsync(carve_at<void>(d_in, u.off), u.src, u.bytes, hipMemcpyHostToDevice, ctx->stream));
  const cfrk_read_paths_in in = {carve_at<int64_t>(d_in, o_hptr), nR, carve_at<cfrk_read_hit>(d_in, o_hits), n_hits,
                                 carve_at<cfrk_unitig>(d_in, o_rec), nS, carve_at<int64_t>(d_in, o_lptr),
                                 carve_at<cfrk_unitig_link>(d_in, o_links), n_links};
  uint32_t *d_support = sup_bytes ? carve_at<uint32_t>(d_in, o_sup) : nullptr;
  if ((rc = cfrk_pool_get(ctx, BUF_READ_PATHS_OUT, hptr_bytes, &d_out))) return stage_drain(ctx, rc);
  int64_t n_paths = 0;
  if ((rc = cfrk_read_paths_measure(ctx, in, (int64_t *)d_out, d_support, &n_paths, stats))) {
    memset(path_ptr, 0, hptr_bytes);                   // refused: everything 0, support as it was
    return stage_drain(ctx, rc);
  }
  *n_paths_out = n_paths;
  if (sup_bytes) HIP_TRY(ctx, hipMemcpyAsync(support, d_support, sup_bytes, hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = cfrk_memcpy_d2h(ctx, path_ptr, d_out, hptr_bytes))) return rc;
  if ((rc = read_paths_fit(ctx, n_paths, cap_paths)) || n_paths == 0) return rc;
  // (the rows go where path_ptr was: it is down already)
  if ((rc = cfrk_pool_get(ctx, BUF_READ_PATHS_OUT, (size_t)n_paths * sizeof *paths, &d_out))) return rc;
  if ((rc = cfrk_read_paths_fill(ctx, in, (cfrk_read_path *)d_out, n_paths))) return rc;
  return cfrk_memcpy_d2h(ctx, paths, d_out, (size_t)n_paths * sizeof *paths);
}

static_assert(sizeof(cfrk_unitig_component) == 32, "cfrk_unitig_component is 32 bytes without padding");
static_assert(sizeof(cfrk_component_stats) == 32, "cfrk_component_stats is 32 bytes without padding");
static_assert(sizeof(cfrk_read_component) == 16, "cfrk_read_component is 16 bytes without padding");
static_assert(sizeof(cfrk_read_component_stats) == 32, "cfrk_read_component_stats is 32 bytes without padding");

static int unitig_components_check(cfrk_ctx *ctx, const cfrk_unitig_components_in &in, const void *comp, const void *comps,
                                   uint64_t cap_comps, int64_t *n_comps_out, cfrk_component_stats *stats) {
  if (!ctx->g_active) return cfrk_fail(ctx, CFRK_ERR_STATE, "unitig components before begin: the job supplies the strand rule");
  if (in.nS < 0 || in.n_links < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (!n_comps_out) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL n_comps_out");
  if (!stats) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL stats");
  if (in.nS > 0 && (!in.d_rec || !in.d_link_ptr || !comp)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  if (in.n_links > 0 && !in.d_links) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL links with n_links above 0");
  if (cap_comps > 0 && !comps) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL array with a capacity above 0");
  if ((uint64_t)in.nS >= (1ull << 32)) return cfrk_fail(ctx, CFRK_ERR_ARG, "%lld unitigs: a link names its target in 32 bits", (long long)in.nS);
  *n_comps_out = 0;
  stats->n_components = stats->n_unitigs = stats->n_kmers = stats->n_links = 0;
  return CFRK_OK;
}

static int unitig_components_fit(cfrk_ctx *ctx, int64_t n_comps, uint64_t cap_comps) {
  if ((uint64_t)n_comps <= cap_comps) return CFRK_OK;
  return cfrk_fail(ctx, CFRK_ERR_SMALL_BUF, "unitig components: %lld components, room for %llu", (long long)n_comps, (unsigned long long)cap_comps);
}

int cfrk_global_unitig_components_device(cfrk_ctx *ctx, const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr,
                                         const cfrk_unitig_link *d_links, int64_t n_links, const uint8_t *d_drop, uint32_t *d_comp,
                                         cfrk_unitig_component *d_comps, uint64_t cap_comps, int64_t *n_comps_out,
                                         cfrk_component_stats *stats) {
  if (!ctx) return CFRK_ERR_ARG;
  const cfrk_unitig_components_in in = {d_rec, nS, d_link_ptr, d_links, n_links, d_drop};
  int rc = unitig_components_check(ctx, in, d_comp, d_comps, cap_comps, n_comps_out, stats);
  if (rc || nS == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int64_t n_comps = 0;
  if ((rc = cfrk_unitig_components_measure(ctx, in, d_comp, &n_comps, stats))) return rc;
  *n_comps_out = n_comps;
  if ((rc = unitig_components_fit(ctx, n_comps, cap_comps)) || n_comps == 0) return rc;
  return cfrk_unitig_components_fill(ctx, in, d_comp, d_comps, n_comps);
}

int cfrk_global_unitig_components(cfrk_ctx *ctx, const cfrk_unitig *rec, int64_t nS, const int64_t *link_ptr,
                                  const cfrk_unitig_link *links, int64_t n_links, const uint8_t *drop, uint32_t *comp,
                                  cfrk_unitig_component *comps, uint64_t cap_comps, int64_t *n_comps_out, cfrk_component_stats *stats) {
  if (!ctx) return CFRK_ERR_ARG;
  const cfrk_unitig_components_in host = {rec, nS, link_ptr, links, n_links, drop};
  int rc = unitig_components_check(ctx, host, comp, comps, cap_comps, n_comps_out, stats);
  if (rc || nS == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // [records | link_ptr | links | drop] in a slot of their own, comp and then the table in another
  Carve c;
  const size_t rec_bytes = (size_t)nS * sizeof *rec, ptr_bytes = ((size_t)nS + 1) * 8, link_bytes = (size_t)n_links * sizeof *links,
               drop_bytes = drop ? (size_t)nS : 0, comp_bytes = (size_t)nS * 4;
  const size_t o_rec = c.part(rec_bytes), o_ptr = c.part(ptr_bytes), o_links = c.part(link_bytes), o_drop = c.part(drop_bytes),
               o_comp = c.part(comp_bytes);
  void *d_in, *d_out;
  if ((rc = cfrk_pool_get(ctx, BUF_UNITIG_COMP_IN, c.end, &d_in))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(carve_at<void>(d_in, o_rec), rec, rec_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(carve_at<void>(d_in, o_ptr), link_ptr, ptr_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (n_links) HIP_TRY(ctx, hipMemcpyAsync(carve_at<void>(d_in, o_links), links, link_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (drop) HIP_TRY(ctx, hipMemcpyAsync(carve_at<void>(d_in, o_drop), drop, drop_bytes, hipMemcpyHostToDevice, ctx->stream));
  const cfrk_unitig_components_in in = {carve_at<cfrk_unitig>(d_in, o_rec), nS, carve_at<int64_t>(d_in, o_ptr),
                                        carve_at<cfrk_unitig_link>(d_in, o_links), n_links, drop ? carve_at<uint8_t>(d_in, o_drop) : nullptr};
  uint32_t *d_comp = carve_at<uint32_t>(d_in, o_comp);    // (stays on the device for the table pass)
  int64_t n_comps = 0;
  if ((rc = cfrk_unitig_components_measure(ctx, in, d_comp, &n_comps, stats))) {
    memset(comp, 0xFF, comp_bytes);                    // refused: all CFRK_COMP_NONE
    return stage_drain(ctx, rc);
  }
  *n_comps_out = n_comps;
  if ((rc = cfrk_memcpy_d2h(ctx, comp, d_comp, comp_bytes))) return rc;
  if ((rc = unitig_components_fit(ctx, n_comps, cap_comps)) || n_comps == 0) return rc;
  if ((rc = cfrk_pool_get(ctx, BUF_UNITIG_COMP_OUT, (size_t)n_comps * sizeof *comps, &d_out))) return rc;
  if ((rc = cfrk_unitig_components_fill(ctx, in, d_comp, (cfrk_unitig_component *)d_out, n_comps))) return rc;
  return cfrk_memcpy_d2h(ctx, comps, d_out, (size_t)n_comps * sizeof *comps);
}

static int read_components_check(cfrk_ctx *ctx, const void *hit_ptr, int64_t nR, const void *hits, int64_t n_hits, const void *comp,
                                 int64_t nS, const void *out, cfrk_read_component_stats *stats) {
  if (!ctx->g_active) return cfrk_fail(ctx, CFRK_ERR_STATE, "read components before begin");
  if (nR < 0 || n_hits < 0 || nS < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (!stats) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL stats");
  if (!hit_ptr) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL hit_ptr");
  if (n_hits > 0 && !hits) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL hits with n_hits above 0");
  if (nS > 0 && !comp) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL comp with nS above 0");
  if (nR > 0 && !out) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL out with nR above 0");
  if ((uint64_t)nS >= (1ull << 32)) return cfrk_fail(ctx, CFRK_ERR_ARG, "%lld unitigs: a hit names its unitig in 32 bits", (long long)nS);
  if ((uint64_t)n_hits >= (1ull << 32)) return cfrk_fail(ctx, CFRK_ERR_ARG, "%lld hits: a hit's index inside its row is 32 bits", (long long)n_hits);
  stats->n_assigned = stats->n_unassigned = stats->n_split = stats->n_dropped = 0;
  return CFRK_OK;
}

int cfrk_global_read_components_device(cfrk_ctx *ctx, const int64_t *d_hit_ptr, int64_t nR, const cfrk_read_hit *d_hits, int64_t n_hits,
                                       const uint32_t *d_comp, int64_t nS, cfrk_read_component *d_out, cfrk_read_component_stats *stats) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = read_components_check(ctx, d_hit_ptr, nR, d_hits, n_hits, d_comp, nS, d_out, stats);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cfrk_read_components_launch(ctx, d_hit_ptr, nR, d_hits, n_hits, d_comp, nS, d_out, stats);
}

int cfrk_global_read_components(cfrk_ctx *ctx, const int64_t *hit_ptr, int64_t nR, const cfrk_read_hit *hits, int64_t n_hits,
                                const uint32_t *comp, int64_t nS, cfrk_read_component *out, cfrk_read_component_stats *stats) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = read_components_check(ctx, hit_ptr, nR, hits, n_hits, comp, nS, out, stats);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // [hit_ptr | hits | comp] in a slot of their own, the rows in another
  Carve c;
  const size_t hptr_bytes = ((size_t)nR + 1) * 8, hit_bytes = (size_t)n_hits * sizeof *hits, comp_bytes = (size_t)nS * 4,
               out_bytes = (size_t)nR * sizeof *out;
  const size_t o_hptr = c.part(hptr_bytes), o_hits = c.part(hit_bytes), o_comp = c.part(comp_bytes);
  void *d_in, *d_out;
  if ((rc = cfrk_pool_get(ctx, BUF_READ_COMP_IN, c.end, &d_in))) return rc;
  if ((rc = cfrk_pool_get(ctx, BUF_READ_COMP_OUT, out_bytes ? out_bytes : 16, &d_out))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(carve_at<void>(d_in, o_hptr), hit_ptr, hptr_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (hit_bytes) HIP_TRY(ctx, hipMemcpyAsync(carve_at<void>(d_in, o_hits), hits, hit_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (comp_bytes) HIP_TRY(ctx, hipMemcpyAsync(carve_at<void>(d_in, o_comp), comp, comp_bytes, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = cfrk_read_components_launch(ctx, carve_at<int64_t>(d_in, o_hptr), nR, carve_at<cfrk_read_hit>(d_in, o_hits), n_hits,
                                        carve_at<uint32_t>(d_in, o_comp), nS, (cfrk_read_component *)d_out, stats)))
    return stage_drain(ctx, rc);
  return out_bytes ? cfrk_memcpy_d2h(ctx, out, d_out, out_bytes) : CFRK_OK;
}

/* ------------------------------------------------------------------ digital normalisation */

static int normalize_check(cfrk_ctx *ctx, int64_t nN, int64_t nS, int64_t batch_reads, const void *data, const void *start,
                           const void *length, const void *keep, const int64_t *n_kept) {
  if (!ctx->g_active) return cfrk_fail(ctx, CFRK_ERR_STATE, "normalize before begin");
  if (ctx->g_flags & CFRK_RUNS_ONLY) return cfrk_fail(ctx, CFRK_ERR_STATE, "a CFRK_RUNS_ONLY job holds runs, not counts");
  if (nN < 0 || nS < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (batch_reads < 1) return cfrk_fail(ctx, CFRK_ERR_ARG, "batch_reads %lld: at least 1", (long long)batch_reads);
  if (!n_kept) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL n_kept");
  if (nS > 0 && (!data || !start || !length || !keep)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  return CFRK_OK;
}

// what both forms run on device buffers: the result into the HBM table as a merge puts it there, every round enqueued,
// one synchronisation at the end for the kept reads and the overflow flag.  nS >= 1.  mode < 0: reads on their own; else
// interleaved pairs joined by that CFRK_PAIR_* mode, the kept reads being twice the kept pairs the joins counted.
static int normalize_core(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                          int64_t nS, uint32_t cutoff, int64_t batch_reads, int mode, uint8_t *d_keep, int64_t *n_kept) {
  ctx->q_valid = false;
  int rc = cfrk_msp_flush_to_table(ctx);
  if (rc) return rc;
  cfrk_msp_note_table_write(ctx);
  void *p;
  if ((rc = cfrk_pool_get(ctx, BUF_NORMALIZE, 5 * sizeof(unsigned long long), &p))) return rc;
  unsigned long long *d_kept = (unsigned long long *)p;     // [kept reads the judge counted | the joins' four pair counts]
  HIP_TRY(ctx, hipMemsetAsync(d_kept, 0, 5 * sizeof *d_kept, ctx->stream));
  if (mode < 0) rc = cfrk_normalize_launch(ctx, d_data, d_start, d_length, nN, nS, cutoff, batch_reads, d_keep, d_kept);
  else rc = cfrk_normalize_pairs_launch(ctx, d_data, d_start, d_length, nN, nS, cutoff, batch_reads, mode, d_keep, d_kept, d_kept + 1);
  if (rc) return rc;
  // snapshot of the flags for the next begin(), as an add leaves it
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_stats, ctx->g_stats, ST_NWORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  ctx->h_stats_valid = true;
  unsigned long long kept = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&kept, mode < 0 ? d_kept : d_kept + 1, sizeof kept, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *n_kept = (int64_t)(mode < 0 ? kept : 2 * kept);
  if (ctx->h_stats[ST_OVERFLOW]) return cfrk_fail(ctx, CFRK_ERR_TABLE_FULL, "table of %llu slots overflowed", (unsigned long long)ctx->g_cap);
  return CFRK_OK;
}

// what a paired call asks in addition: whole pairs in the call and in every round
static int normalize_pairs_check(cfrk_ctx *ctx, int64_t nS, int64_t batch_reads, int mode) {
  if (mode != CFRK_PAIR_BOTH && mode != CFRK_PAIR_EITHER) return cfrk_fail(ctx, CFRK_ERR_ARG, "mode %d: CFRK_PAIR_BOTH or CFRK_PAIR_EITHER", mode);
  if (nS & 1) return cfrk_fail(ctx, CFRK_ERR_ARG, "%lld interleaved reads: an odd number", (long long)nS);
  if (batch_reads & 1) return cfrk_fail(ctx, CFRK_ERR_ARG, "batch_reads %lld: a round holds whole pairs", (long long)batch_reads);
  return CFRK_OK;
}

// the device and the host form, of reads on their own (mode < 0) and of pairs
static int normalize_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                            int64_t nS, uint32_t cutoff, int64_t batch_reads, int mode, uint8_t *d_keep, int64_t *n_kept) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = normalize_check(ctx, nN, nS, batch_reads, d_data, d_start, d_length, d_keep, n_kept);
  if (rc || (mode >= 0 && (rc = normalize_pairs_check(ctx, nS, batch_reads, mode)))) return rc;
  *n_kept = 0;
  if (nS == 0) return CFRK_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return normalize_core(ctx, d_data, d_start, d_length, nN, nS, cutoff, batch_reads, mode, d_keep, n_kept);
}

static int normalize_host(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length, int64_t nN, int64_t nS,
                          uint32_t cutoff, int64_t batch_reads, int mode, uint8_t *keep, int64_t *n_kept) {
  if (!ctx) return CFRK_ERR_ARG;
  int rc = normalize_check(ctx, nN, nS, batch_reads, data, start, length, keep, n_kept);
  if (rc || (mode >= 0 && (rc = normalize_pairs_check(ctx, nS, batch_reads, mode)))) return rc;
  *n_kept = 0;
  if (nS == 0) return CFRK_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // staged through the query calls' slot: the reads in, room for the keep bytes behind them
  StagePart x[1] = {{nullptr, (size_t)nS, nullptr}};
  StagedReads d;
  if ((rc = stage_reads(ctx, BUF_QUERY_IN, data, start, length, nN, nS, STAGE_TABLE, x, 1, &d))) return rc;
  if ((rc = normalize_core(ctx, d.data, d.start, d.length, nN, nS, cutoff, batch_reads, mode, (uint8_t *)x[0].dev, n_kept)) &&
      rc != CFRK_ERR_TABLE_FULL) return stage_drain(ctx, rc);
  const int rc2 = cfrk_memcpy_d2h(ctx, keep, x[0].dev, (size_t)nS);
  return rc ? rc : rc2;
}

int cfrk_global_normalize_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                                 int64_t nN, int64_t nS, uint32_t cutoff, int64_t batch_reads, uint8_t *d_keep,
                                 int64_t *n_kept) {
  return normalize_device(ctx, d_data, d_start, d_length, nN, nS, cutoff, batch_reads, -1, d_keep, n_kept);
}

int cfrk_global_normalize(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length, int64_t nN,
                          int64_t nS, uint32_t cutoff, int64_t batch_reads, uint8_t *keep, int64_t *n_kept) {
  return normalize_host(ctx, data, start, length, nN, nS, cutoff, batch_reads, -1, keep, n_kept);
}

int cfrk_global_normalize_pairs_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                                       int64_t nN, int64_t nS, uint32_t cutoff, int64_t batch_reads, int mode, uint8_t *d_keep,
                                       int64_t *n_kept) {
  if (ctx && mode < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "mode %d: CFRK_PAIR_BOTH or CFRK_PAIR_EITHER", mode);
  return normalize_device(ctx, d_data, d_start, d_length, nN, nS, cutoff, batch_reads, mode, d_keep, n_kept);
}

int cfrk_global_normalize_pairs(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length, int64_t nN,
                                int64_t nS, uint32_t cutoff, int64_t batch_reads, int mode, uint8_t *keep, int64_t *n_kept) {
  if (ctx && mode < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "mode %d: CFRK_PAIR_BOTH or CFRK_PAIR_EITHER", mode);
  return normalize_host(ctx, data, start, length, nN, nS, cutoff, batch_reads, mode, keep, n_kept);
}

int cfrk_global_last_add_ms(cfrk_ctx *ctx, float *ms) {
  if (!ctx || !ms) return CFRK_ERR_ARG;
  if (!ctx->ev_valid) return cfrk_fail(ctx, CFRK_ERR_STATE, "no add recorded");
  HIP_TRY(ctx, hipEventSynchronize(ctx->ev1));
  HIP_TRY(ctx, hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
  return CFRK_OK;
}

/* ------------------------------------------------------------------ per-read sparse */

static int sparse_check(cfrk_ctx *ctx, int64_t nN, int64_t nS, int k, int flags, const void *row_ptr, const void *keys,
                        const void *counts, uint64_t cap, const uint64_t *nnz_out) {
  if (!ctx) return CFRK_ERR_ARG;
  if (k < 1 || k > 32) return cfrk_fail(ctx, CFRK_ERR_ARG, "k=%d outside 1..32 (per-read sparse keys are one word)", k);
  if (flags & ~CFRK_CANONICAL) return cfrk_fail(ctx, CFRK_ERR_ARG, "flags 0x%x: per-read sparse takes CFRK_CANONICAL only", flags);
  if (nN < 0 || nS < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (!row_ptr || !nnz_out) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  if (cap > 0 && (!keys || !counts)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL keys / counts with cap > 0");
  return CFRK_OK;
}

// count, nnz to the host, refuse or place the rows, compact: what both forms run on device buffers.  The device form
// reads nnz alone; the host form's whole row_ptr comes down with it (h_row), and its rows go to parts of BUF_SPARSE_OUT.
static int sparse_core(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN, int64_t nS,
                       int k, int flags, int64_t *d_row, int64_t *h_row, uint64_t **d_keys, uint32_t **d_counts, uint64_t cap,
                       uint64_t *nnz_out) {
  int rc = cfrk_sparse_count(ctx, d_data, d_start, d_length, nN, nS, k, flags, d_row);
  if (rc) return rc;
  int64_t nnz = 0;
  if (h_row) HIP_TRY(ctx, hipMemcpyAsync(h_row, d_row, (size_t)(nS + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  else HIP_TRY(ctx, hipMemcpyAsync(&nnz, d_row + nS, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (h_row) nnz = h_row[nS];
  *nnz_out = (uint64_t)nnz;
  if ((uint64_t)nnz > cap)
    return cfrk_fail(ctx, CFRK_ERR_SMALL_BUF, "%lld distinct (read, k-mer) pairs, room for %llu", (long long)nnz, (unsigned long long)cap);
  if (nnz == 0) return CFRK_OK;
  if (h_row) {
    Carve c;
    void *p;
    const size_t o_keys = c.part((size_t)nnz * 8), o_cnt = c.part((size_t)nnz * 4);
    if ((rc = cfrk_pool_get(ctx, BUF_SPARSE_OUT, c.end, &p))) return rc;
    *d_keys = carve_at<uint64_t>(p, o_keys);
    *d_counts = carve_at<uint32_t>(p, o_cnt);
  }
  return cfrk_sparse_compact(ctx, d_start, d_row, nS, *d_keys, *d_counts);
}

int cfrk_per_read_sparse_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                                int64_t nN, int64_t nS, int k, int flags, int64_t *d_row_ptr, uint64_t *d_keys,
                                uint32_t *d_counts, uint64_t cap, uint64_t *nnz_out) {
  int rc = sparse_check(ctx, nN, nS, k, flags, d_row_ptr, d_keys, d_counts, cap, nnz_out);
  if (rc) return rc;
  *nnz_out = 0;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (nS == 0) {
    HIP_TRY(ctx, hipMemsetAsync(d_row_ptr, 0, 8, ctx->stream));
    return CFRK_OK;
  }
  if (!d_start || !d_length || (nN > 0 && !d_data)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  return sparse_core(ctx, d_data, d_start, d_length, nN, nS, k, flags, d_row_ptr, nullptr, &d_keys, &d_counts, cap, nnz_out);
}

int cfrk_per_read_sparse(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length, int64_t nN,
                         int64_t nS, int k, int flags, int64_t *row_ptr, uint64_t *keys, uint32_t *counts, uint64_t cap,
                         uint64_t *nnz_out) {
  int rc = sparse_check(ctx, nN, nS, k, flags, row_ptr, keys, counts, cap, nnz_out);
  if (rc) return rc;
  *nnz_out = 0;
  row_ptr[0] = 0;
  if (nS == 0) return CFRK_OK;
  if (!start || !length || (nN > 0 && !data)) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // staged through a slot of its own (BUF_DATA may still be read by an open job's last add), with room for row_ptr
  StagePart row = {nullptr, (size_t)(nS + 1) * 8, nullptr};
  StagedReads d;
  if ((rc = stage_reads(ctx, BUF_SPARSE_IN, data, start, length, nN, nS, STAGE_TABLE, &row, 1, &d))) return rc;
  uint64_t *d_keys = nullptr; uint32_t *d_cnt = nullptr;
  rc = sparse_core(ctx, d.data, d.start, d.length, nN, nS, k, flags, (int64_t *)row.dev, row_ptr, &d_keys, &d_cnt, cap, nnz_out);
  if (rc || *nnz_out == 0) return stage_drain(ctx, rc);
  HIP_TRY(ctx, hipMemcpyAsync(keys, d_keys, (size_t)*nnz_out * 8, hipMemcpyDeviceToHost, ctx->stream));
  return cfrk_memcpy_d2h(ctx, counts, d_cnt, (size_t)*nnz_out * 4);
}

/* ------------------------------------------------------------------ distinct sketch */

static int sketch_check(cfrk_ctx *ctx, int64_t nN, int k, int flags) {
  if (!ctx) return CFRK_ERR_ARG;
  if (k < 1 || k > 64) return cfrk_fail(ctx, CFRK_ERR_ARG, "k=%d outside 1..64", k);
  if (flags & ~CFRK_CANONICAL) return cfrk_fail(ctx, CFRK_ERR_ARG, "flags 0x%x: the distinct sketch takes CFRK_CANONICAL only", flags);
  if (nN < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  return CFRK_OK;
}

int cfrk_distinct_sketch_device(cfrk_ctx *ctx, const int8_t *d_data, int64_t nN, int k, int flags, uint8_t *d_regs,
                                uint64_t *windows_out) {
  int rc = sketch_check(ctx, nN, k, flags);
  if (rc) return rc;
  if (windows_out) *windows_out = 0;
  if (nN == 0) return CFRK_OK;
  if (!d_data || !d_regs) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  if (((uintptr_t)d_data & 15) != 0) return cfrk_fail(ctx, CFRK_ERR_ALIGN, "d_data %p", (const void *)d_data);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint64_t *d_windows;
  if ((rc = cfrk_sketch_launch(ctx, d_data, nN, k, flags, d_regs, &d_windows))) return rc;
  if (windows_out) {
    HIP_TRY(ctx, hipMemcpyAsync(windows_out, d_windows, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  return CFRK_OK;
}

int cfrk_distinct_sketch(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length, int64_t nN,
                         int64_t nS, int k, int flags, uint8_t *regs, uint64_t *windows_out) {
  int rc = sketch_check(ctx, nN, k, flags);
  if (rc) return rc;
  if (nS < 0) return cfrk_fail(ctx, CFRK_ERR_ARG, "negative size");
  if (windows_out) *windows_out = 0;
  if (nN == 0) return CFRK_OK;
  if (!data || !regs) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // (staged through the query calls' slot: BUF_DATA may still be read by an open job's last add)
  uint8_t *d_regs;
  StagedReads d;
  if ((rc = cfrk_sketch_stage(ctx, &d_regs))) return rc;
  if ((rc = stage_reads(ctx, BUF_QUERY_IN, data, start, length, nN, nS, 0, nullptr, 0, &d))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(d_regs, regs, CFRK_SKETCH_REGS, hipMemcpyHostToDevice, ctx->stream));
  const uint64_t *d_windows;
  if ((rc = cfrk_sketch_launch(ctx, d.data, nN, k, flags, d_regs, &d_windows))) return stage_drain(ctx, rc);
  HIP_TRY(ctx, hipMemcpyAsync(regs, d_regs, CFRK_SKETCH_REGS, hipMemcpyDeviceToHost, ctx->stream));
  if (windows_out) HIP_TRY(ctx, hipMemcpyAsync(windows_out, d_windows, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CFRK_OK;
}

/* ------------------------------------------------------------------ synthetic reads */

int cfrk_synth_reads_device(cfrk_ctx *ctx, int64_t r0, int64_t R, int L, int64_t Glen,
                            uint64_t seedG, uint64_t seedR, uint64_t seedS, int uniform,
                            int8_t *d_data, int64_t *d_start, int32_t *d_length) {
  if (!ctx) return CFRK_ERR_ARG;
  if (r0 < 0 || R < 0 || L < 1 || (!uniform && Glen < L)) return cfrk_fail(ctx, CFRK_ERR_ARG, "bad generator parameters");
  if (R == 0) return CFRK_OK;
  if (!d_data) return cfrk_fail(ctx, CFRK_ERR_ARG, "NULL buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cfrk_launch_synth(ctx, r0, R, L, Glen, seedG, seedR, seedS, uniform, d_data, d_start, d_length);
}

/* ------------------------------------------------------------------ the radix path's shape (tests) */

// Read-only: the shape radix.hip's host code chooses for (k, nN) -- the very function cfrk_radix_count lays its buffers
// out by -- and four host-side values the context's most recent radix add left behind.
int cfrk_debug_radix_info(const cfrk_ctx *ctx, int k, int64_t nN, uint64_t out[12]) {
  if (!out || nN < 0) return CFRK_ERR_ARG;
  cfrk_radix_info(ctx, k, nN, out);
  return CFRK_OK;
}

}  // extern "C"
