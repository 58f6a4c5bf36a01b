// cfrk_cli.cpp -- the `cfrk` command (its interface and options: cli_options.h): start-up, the per-read chunk pipeline,
// the global count on one or several devices, --device-parse, --query-db.  What is done with the finished count lives
// in cli_graph.cpp and cli_query.cpp.
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "cli_util.h"

namespace {

// --timing: wall-clock seconds by phase (one file; with --batch the last file's)
struct Timing {
  double parse = 0, add_call = 0, finish_wait = 0, export_ = 0, format = 0, write = 0, per_read = 0, total = 0, histo = 0;
  double query = 0, stats = 0;
  double close = 0, free_batch = 0, open = 0;
  double contexts = 0, begin = 0, wait_parse = 0;   // context creation (beside the parse), cfrk_global_begin, the main thread's wait for the parser
  float count_kernels_ms = 0;
  int64_t fasta_bytes = 0, nN = 0, nS = 0;
  uint64_t entries = 0, out_bytes = 0;
  int attempts = 0;                    // begin / add / finish passes of the global job (above 1: the hint was too small)
  double estimate = 0, distinct_estimate = 0;   // the sketch before the count: seconds, estimated distinct k-mers
  double text_map = 0, text_h2d = 0, device_parse_ms = 0;    // --device-parse: the text's copy to the device (s), the parse there (ms)
  bool device_parse = false;
  int in_format = CFRK_FORMAT_FASTA;   // what the input was read as
  uint64_t hint = 0;                   // capacity hint of the LAST attempt
} g_timing;
double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Worker {            // one context (= one HIP stream + buffer pool) on one device
  cfrk_ctx *ctx = nullptr;
  int device = 0;
};

// the format a file is read as: --format, or its first byte (a file that cannot be opened reads as FASTA: the reader says so)
int file_format(const Options &o, const char *path) {
  if (o.format >= 0) return o.format;
  char c = 0;
  size_t n = 0;
  if (FILE *f = fopen(path, "rb")) { n = fread(&c, 1, 1, f); fclose(f); }
  return cfrk_host_sniff_format(&c, n);
}
// may this run read `path` as `fmt`?  Says why not, before anything is parsed or a device is opened.
bool format_allowed(const Options &o, const char *path, int fmt) {
  if (fmt == CFRK_FORMAT_FASTQ && !(o.native || o.global || o.sparse)) {
    fprintf(stderr, "cfrk: %s is FASTQ: the default per-read mode is the reference's, which reads FASTA only; FASTQ is taken by --native, --global and --sparse (and as --query)\n", path);
    return false;
  }
  if (fmt == CFRK_FORMAT_FASTA && o.min_qual_set) {
    fprintf(stderr, "cfrk: --min-qual applies to FASTQ input: %s is read as FASTA\n", path);
    return false;
  }
  return true;
}
// host parse of either format; a refusal is printed here (1), 0 otherwise
int read_reads(const char *path, int fmt, int fasta_flags, int min_qual, cfrk_batch *b) {
  if (fmt == CFRK_FORMAT_FASTQ) {
    uint64_t where = 0;
    const int rc = cfrk_host_read_fastq(path, min_qual, b, &where);
    char msg[160];
    if (rc && cfrk_host_fastq_message(rc, where, msg, sizeof msg)) { fprintf(stderr, "cfrk: cannot read %s (%s)\n", path, msg); return 1; }
    if (rc) { fprintf(stderr, "cfrk: cannot read %s (error %d)\n", path, rc); return 1; }
    return 0;
  }
  const int rc = cfrk_host_read_fasta(path, fasta_flags, b);
  if (rc) { fprintf(stderr, "cfrk: cannot read %s (error %d)\n", path, rc); return 1; }
  return 0;
}

struct ChunkRange { int64_t first, count; };

// which reads reach the file, in which chunks (src/main.cu:270-305)
std::vector<ChunkRange> plan_chunks(const Options &o, int64_t nS) {
  std::vector<ChunkRange> v;
  const int64_t C = o.chunk_size;
  const int64_t n_full = nS / C;                     // nChunk = floor(gnS/chunkSize), src/main.cu:270
  if (o.all_chunks) {
    for (int64_t c = 0; c <= n_full; ++c) {
      const int64_t first = c * C, count = (c < n_full) ? C : nS - first;
      if (count > 0) v.push_back({first, count});
    }
    return v;
  }
  if (o.native) {                                    // the remainder chunk, where it really is
    if (nS - n_full * C > 0) v.push_back({n_full * C, nS - n_full * C});
    return v;
  }
  // compat: only SelectChunkRemain's chunk is written, located with the narrowed arguments
  const int64_t count = nS - n_full * C;             // chunkRemain, src/main.cu:297
  const int64_t first = (int64_t)(uint16_t)C * (int64_t)(uint16_t)n_full;
  if (count > 0 && first + count <= nS) v.push_back({first, count});
  return v;
}

// per-read modes: the chunks of one batch through `workers` (any number of devices), text in order
int run_per_read(const Options &o, const cfrk_batch &batch, std::vector<Worker> &workers, FILE *out) {
  const std::vector<ChunkRange> chunks = plan_chunks(o, batch.nS);
  const int flags = o.native ? 0 : CFRK_COMPAT;
  const size_t fourk = (size_t)1 << (2 * (o.k > 0 && o.k < 16 ? o.k : 1));
  const size_t n = chunks.size();
  std::vector<std::string> text(n);
  std::vector<char> ready(n, 0);
  const char *call = o.sparse ? "cfrk_per_read_sparse" : "cfrk_per_read_dense";
  std::mutex mu;
  std::condition_variable cv;
  std::atomic<size_t> next{0};
  size_t written = 0;                                // guarded by mu
  int failed = 0;                                    // guarded by mu
  const size_t window = 2 * workers.size() + 2;      // formatted chunks that may wait for the writer
  const int fmt_threads = std::max(1, o.threads / (int)workers.size());

  auto work = [&](Worker &w) {
    std::vector<int64_t> start, row_ptr;
    std::vector<int32_t> freq;
    std::vector<uint64_t> keys;
    std::vector<uint32_t> counts;
    for (;;) {
      const size_t c = next.fetch_add(1);
      if (c >= n) return;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return failed || c < written + window; });
        if (failed) return;
      }
      const int8_t *data; const int32_t *length; int64_t nN;
      start.resize((size_t)chunks[c].count);
      cfrk_host_chunk(&batch, chunks[c].first, chunks[c].count, &data, start.data(), &length, &nN);
      int rc;
      std::string t;
      if (o.sparse) {
        // room for every window of the chunk: always enough (cfrk_abi.h)
        uint64_t room = 0, nnz = 0;
        for (int64_t r = 0; r < chunks[c].count; ++r) room += (uint64_t)std::max<int64_t>((int64_t)length[r] - o.k + 1, 0);
        row_ptr.resize((size_t)chunks[c].count + 1);
        keys.resize(room);
        counts.resize(room);
        rc = cfrk_per_read_sparse(w.ctx, data, start.data(), length, nN, chunks[c].count, o.k, o.canonical ? CFRK_CANONICAL : 0,
                                  row_ptr.data(), keys.data(), counts.data(), room, &nnz);
        if (!rc) {
          format_into(t, [&](char *out, size_t room_t) {
            return cfrk_host_format_sparse_rows_mt(row_ptr.data(), keys.data(), counts.data(), chunks[c].count, out, room_t, fmt_threads);
          });
        }
      } else {
        freq.resize((size_t)chunks[c].count * fourk);
        rc = cfrk_per_read_dense(w.ctx, data, start.data(), length, nN, chunks[c].count, o.k, flags, freq.data());
        if (!rc) {
          format_into(t, [&](char *out, size_t room_t) { return cfrk_host_format_dense_mt(freq.data(), chunks[c].count, o.k, out, room_t, fmt_threads); });
        }
      }
      std::lock_guard<std::mutex> lk(mu);
      if (rc && !failed) failed = die(w.ctx, rc, call);
      text[c].swap(t);
      ready[c] = 1;
      cv.notify_all();
    }
  };
  std::vector<std::thread> th;
  for (size_t i = 1; i < workers.size() && i < n; ++i) th.emplace_back(work, std::ref(workers[i]));
  std::thread first_worker;
  if (n) first_worker = std::thread(work, std::ref(workers[0]));
  for (size_t c = 0; c < n; ++c) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return failed || ready[c]; });
    if (failed) break;
    std::string t;
    t.swap(text[c]);
    lk.unlock();
    if (c && !o.sparse) fputc('\n', out);           // (dense rows are separated, sparse rows terminated by '\n')
    fwrite(t.data(), 1, t.size(), out);
    lk.lock();
    written = c + 1;
    cv.notify_all();
  }
  if (first_worker.joinable()) first_worker.join();
  for (auto &t : th) t.join();
  return failed;
}

// --histo: the exact spectrum without a user-set bound.  The device histogram covers counts below HISTO_W; the few keys
// counted HISTO_W times or more are fetched by a count-range export and binned on the host.  Owners of a multi-device
// job hold disjoint key sets: their spectra add.
constexpr uint32_t HISTO_W = 16384;
struct Spectrum {
  std::vector<uint64_t> hist = std::vector<uint64_t>(HISTO_W, 0);   // exact bins 0 .. HISTO_W - 1
  std::vector<uint32_t> tail;                                       // one count per key counted HISTO_W times or more
  void add(const Spectrum &o) {
    for (uint32_t c = 0; c < HISTO_W; ++c) hist[c] += o.hist[c];
    tail.insert(tail.end(), o.tail.begin(), o.tail.end());
  }
};

// 0, or the exit status (the error reported)
int result_spectrum(cfrk_ctx *ctx, Spectrum &sp) {
  std::vector<uint64_t> h(HISTO_W + 1);
  int rc = cfrk_global_histogram(ctx, h.data(), HISTO_W + 1);
  if (rc && rc != CFRK_ERR_COUNT_OVERFLOW) return die(ctx, rc, "cfrk_global_histogram");
  const uint64_t nt = h[HISTO_W];
  for (uint32_t c = 0; c < HISTO_W; ++c) sp.hist[c] += h[c];
  if (!nt) return 0;
  std::vector<uint64_t> lo(nt);
  std::vector<uint32_t> cnt(nt);
  uint64_t got = 0;
  rc = cfrk_global_export_range(ctx, HISTO_W, CFRK_COUNT_MAX, lo.data(), nullptr, cnt.data(), nt, &got);
  if (rc && rc != CFRK_ERR_COUNT_OVERFLOW) return die(ctx, rc, "cfrk_global_export_range");
  sp.tail.insert(sp.tail.end(), cnt.begin(), cnt.begin() + (ptrdiff_t)got);
  return 0;
}

int write_histo(const Options &o, const Spectrum &sp) {
  std::string buf;
  format_into(buf, [&](char *out, size_t room) { return cfrk_host_format_histo(sp.hist.data(), HISTO_W, sp.tail.data(), sp.tail.size(), out, room); });
  return write_file(o.histo, buf);
}

// the global result (ascending keys) as sparse text or in the binary form
void write_global(const Options &o, const uint64_t *lo, const uint64_t *hi, const uint32_t *cnt, uint64_t n, FILE *out) {
  const uint64_t *hi2 = (o.k > 32) ? hi : nullptr;
  std::string buf;
  const double t0 = now_s();
  format_into(buf, [&](char *to, size_t room) {
    return o.binary ? cfrk_host_write_binary(o.k, o.canonical ? CFRK_BIN_CANONICAL : 0, lo, hi2, cnt, n, to, room)
                    : cfrk_host_format_sparse_mt(lo, hi2, cnt, n, to, room, o.threads);
  });
  const double t1 = now_s();
  fwrite(buf.data(), 1, buf.size(), out);
  fflush(out);
  g_timing.format = t1 - t0; g_timing.write = now_s() - t1; g_timing.entries = n; g_timing.out_bytes = buf.size();
}

// --estimate / --estimate-only / --auto-hint: the batch's distinct sketch.  Context i sketches shard i of the reads (the
// shards of run_global_multi); the registers are merged on the host.
struct Estimate {
  bool have = false;
  double distinct = 0;
  uint64_t windows = 0, hint = 0;
};

// 0, or the exit status (the error reported)
int sketch_batch(const Options &o, const cfrk_batch &batch, const std::vector<cfrk_ctx *> &ctxs, Estimate &e) {
  const double t0 = now_s();
  const int N = (int)ctxs.size();
  std::vector<std::vector<uint8_t>> regs((size_t)N, std::vector<uint8_t>(CFRK_SKETCH_REGS, 0));
  std::vector<uint64_t> windows((size_t)N, 0);
  std::vector<int> status((size_t)N, 0);
  auto shard = [&](int sh) {
    const int64_t r0 = batch.nS * sh / N, r1 = batch.nS * (sh + 1) / N;
    const int64_t b0 = (r0 < batch.nS) ? batch.start[r0] : batch.nN, b1 = (r1 < batch.nS) ? batch.start[r1] : batch.nN;
    if (b1 <= b0) return;
    const int rc = cfrk_distinct_sketch(ctxs[(size_t)sh], batch.data + b0, nullptr, nullptr, b1 - b0, 0, o.k,
                                        o.canonical ? CFRK_CANONICAL : 0, regs[(size_t)sh].data(), &windows[(size_t)sh]);
    if (rc) status[(size_t)sh] = die(ctxs[(size_t)sh], rc, "cfrk_distinct_sketch");
  };
  if (N == 1) shard(0);
  else {
    std::vector<std::thread> th;
    for (int sh = 0; sh < N; ++sh) th.emplace_back(shard, sh);
    for (auto &t : th) t.join();
  }
  for (int r : status) if (r) return r;
  for (int sh = 1; sh < N; ++sh) { cfrk_sketch_merge(regs[0].data(), regs[(size_t)sh].data()); windows[0] += windows[(size_t)sh]; }
  cfrk_sketch_estimate(regs[0].data(), &e.distinct);
  cfrk_sketch_hint(regs[0].data(), &e.hint);
  e.windows = windows[0];
  e.have = true;
  g_timing.estimate = now_s() - t0; g_timing.distinct_estimate = e.distinct;
  fprintf(stderr, "cfrk-estimate distinct=%.0f windows=%llu hint=%llu\n", e.distinct, (unsigned long long)e.windows, (unsigned long long)e.hint);
  return 0;
}

// early_free: the batch is no longer needed once it has been counted -- returning 1.6 GB of pages to the kernel takes
// ~0.17 s, which then runs beside the export, the formatting and the write instead of behind them
// d_data: the batch's codes already on the device (--device-parse: batch then carries nN and nS only)
int run_global(const Options &o, const Inputs &in, const cfrk_batch &batch, Worker &w, FILE *out, const Estimate &est, std::thread *early_free = nullptr,
               cfrk_batch *owned = nullptr, bool on_device = false, const int8_t *d_data = nullptr) {
  int rc;
  cfrk_ctx *ctx = w.ctx;
  // The capacity hint sizes the result list and the spill table (12 B per slot at load <= 0.5).  Distinct k-mers cannot
  // exceed the window starts (nN), but a table for nN keys is 25 - 50 GB for a 1.5 GB batch and allocating it took
  // 5 of the 6 seconds of a k = 31 run (round 5, profiles/r05/end_to_end.txt): the first attempt announces nN / 16 keys
  // (sequencing depth is rarely below that) and an overflowing result (CFRK_ERR_TABLE_FULL) is counted again with
  // eight times the room, up to nN (capped at 2^31 keys).  --auto-hint: the first attempt announces the sketch's hint instead.
  const uint64_t hint_max = std::min<uint64_t>(std::max<uint64_t>((uint64_t)(batch.nN > 0 ? batch.nN : 1), 1ull << 20), 1ull << 31);
  uint64_t hint = std::min<uint64_t>(std::max<uint64_t>(hint_max / 16, 1ull << 20), hint_max);
  if (o.auto_hint && est.have) hint = std::min<uint64_t>(est.hint, hint_max);
  uint64_t n = 0;
  // --normalize-out: the reads go to the device once; every attempt normalises them from there into its fresh job
  DeviceBufs bufs(ctx);
  struct { void *data = nullptr, *start = nullptr, *length = nullptr, *keep = nullptr; } nr;
  if (o.normalize_out && o.paired) {
    if (odd_records(in.npath, batch.nS)) return 1;
    if (o.pair_check && o.normalize_names &&
        (rc = check_mate_names(ctx, batch.nS / 2, text_format_of(in.nformat), in.ntext, in.npath, nullptr, nullptr))) return rc;
  }
  if (o.normalize_out && batch.nS > 0) {
    const char *what = "";
    if ((rc = bufs.upload(batch, &nr.data, &nr.start, &nr.length, &what))) return die(ctx, rc, what);
    if ((rc = bufs.alloc((size_t)batch.nS, &nr.keep))) return die(ctx, rc, "cfrk_device_alloc");
  }
  // (the phase times add up over the attempts: a batch counted three times shows three times the seconds)
  double add_s = 0, finish_s = 0;
  g_timing.begin = 0;
  for (;;) {
    const double tb = now_s();
    ++g_timing.attempts;
    g_timing.hint = hint;
    if ((rc = cfrk_global_begin(ctx, o.k, o.canonical ? CFRK_CANONICAL : 0, hint))) return die(ctx, rc, "cfrk_global_begin");
    const double t0 = now_s();
    g_timing.begin += t0 - tb;
    if (o.normalize_out) {
      int64_t kept = 0;
      if (batch.nS == 0) rc = 0;
      else if (o.paired)
        rc = cfrk_global_normalize_pairs_device(ctx, (const int8_t *)nr.data, (const int64_t *)nr.start, (const int32_t *)nr.length, batch.nN,
                                                batch.nS, o.normalize_cutoff, o.normalize_batch, o.pair_mode, (uint8_t *)nr.keep, &kept);
      else
        rc = cfrk_global_normalize_device(ctx, (const int8_t *)nr.data, (const int64_t *)nr.start, (const int32_t *)nr.length, batch.nN,
                                          batch.nS, o.normalize_cutoff, o.normalize_batch, (uint8_t *)nr.keep, &kept);
      if (rc == CFRK_ERR_TABLE_FULL && hint < hint_max) { hint = std::min<uint64_t>(hint * 8, hint_max); continue; }
      if (rc) return die(ctx, rc, o.paired ? "cfrk_global_normalize_pairs_device" : "cfrk_global_normalize_device");
    }
    else if (on_device) { if (batch.nN > 0 && (rc = cfrk_global_add_device(ctx, d_data, batch.nN))) return die(ctx, rc, "cfrk_global_add_device"); }
    else if ((rc = cfrk_global_add(ctx, batch.data, batch.start, batch.length, batch.nN, batch.nS))) return die(ctx, rc, "cfrk_global_add");
    const double t1 = now_s();
    rc = cfrk_global_finish(ctx, &n);
    add_s += t1 - t0; finish_s += now_s() - t1;
    if (rc == CFRK_ERR_TABLE_FULL && hint < hint_max) { hint = std::min<uint64_t>(hint * 8, hint_max); continue; }
    break;
  }
  // (counts are 32-bit and saturate: the result is complete, the user is told)
  if (rc == CFRK_ERR_COUNT_OVERFLOW) fprintf(stderr, "cfrk: warning: %s\n", cfrk_last_error(ctx));
  else if (rc) return die(ctx, rc, "cfrk_global_finish");
  if (o.normalize_out && (rc = write_normalized(o, ctx, in, batch, nr.data, nr.start, nr.length, nr.keep))) return rc;
  const double t2 = now_s();
  // the spectrum is taken before the batch is freed: its copies do not wait behind the page returns
  if (o.histo) {
    Spectrum sp;
    if ((rc = result_spectrum(ctx, sp)) || (rc = write_histo(o, sp))) return rc;
  }
  g_timing.histo = now_s() - t2;
  if ((o.clip_tips || o.pop_bubbles || o.pop_bulges || o.drop_weak) && (rc = simplify_unitigs(o, ctx))) return rc;
  if (o.min_component_kmers && (rc = drop_small_components(o, ctx))) return rc;
  if ((o.unitigs_out || o.unitigs_gfa) && (rc = write_unitigs(o, ctx))) return rc;
  if (o.unitigs_map && (rc = write_unitigs_map(o, ctx, in.mreads))) return rc;
  if (o.query) {
    const double q0 = now_s();
    if (o.query_out) {
      std::vector<uint32_t> ans;
      if ((rc = query_answers(ctx, in.qreads, ans)) || (rc = write_query(o, in.qreads, o.k, ans.data()))) return rc;
    }
    g_timing.query = now_s() - q0;
    if (o.query_stats) {
      const double s0 = now_s();
      if ((rc = write_query_stats(o, ctx, in.qreads))) return rc;
      g_timing.stats = now_s() - s0;
    }
    if ((rc = check_query_pairs(o, ctx, in))) return rc;
    if (o.filter_out && (rc = write_filter(o, ctx, in, o.k))) return rc;
    if (o.correct_out && (rc = write_correct(o, ctx, in))) return rc;
  }
  if (early_free && owned) *early_free = std::thread([owned] { cfrk_host_free_batch(owned); });
  cfrk_global_last_add_ms(ctx, &g_timing.count_kernels_ms);
  g_timing.add_call = add_s; g_timing.finish_wait = finish_s;
  if (o.histo_only || o.query_only) return 0;
  const double t3 = now_s();
  std::vector<uint64_t> keys(n), hi(n);
  std::vector<uint32_t> cnt(n);
  rc = cfrk_global_export_range(ctx, o.min_count, o.max_count, keys.data(), hi.data(), cnt.data(), n, &n);
  if (rc && rc != CFRK_ERR_COUNT_OVERFLOW) return die(ctx, rc, "cfrk_global_export_range");
  g_timing.export_ = now_s() - t3;
  write_global(o, keys.data(), hi.data(), cnt.data(), n, out);
  return 0;
}

// --global over several devices: shard s of the reads goes to device s (first context of the pair);
// device s then owns the leaves s, s + N, ...: it receives its segment of every shard's packed runs
// and counts them on its second context.  The owners' key sets are disjoint; their sorted lists are
// merged into one ascending output.
int run_global_multi(const Options &o, const Inputs &in, const cfrk_batch &batch, std::vector<std::vector<Worker>> &per_dev, FILE *out, const Estimate &est) {
  const int N = (int)per_dev.size();
  const int flags = o.canonical ? CFRK_CANONICAL : 0;
  // (as in run_global: nN / 16 keys announced first; an owner whose result overflows makes the job count on one device,
  //  where the hint grows)
  uint64_t hint = std::min<uint64_t>(std::max<uint64_t>((uint64_t)(batch.nN > 0 ? batch.nN : 1) / 16, 1ull << 20), 1ull << 31);
  // --auto-hint: the merged sketch's hint; the owners' shares of the leaves are close to even, not even: an eighth on top
  if (o.auto_hint && est.have) hint = std::min<uint64_t>(est.hint + est.hint / 8, 1ull << 31);
  g_timing.attempts = 1; g_timing.hint = hint;
  // shard s: packed rows stay ON ITS DEVICE (16 bytes per row), rows[s][o] = rows of owner o's segment
  std::vector<void *> d_packed((size_t)N, nullptr);
  std::vector<std::vector<uint64_t>> rows((size_t)N, std::vector<uint64_t>((size_t)N, 0));
  std::vector<int> status((size_t)N, 0);
  std::vector<char> refused((size_t)N, 0);           // the shard cannot export runs: count on one device instead
  auto free_packed = [&] {
    for (int sh = 0; sh < N; ++sh)
      if (d_packed[(size_t)sh]) { cfrk_device_free(per_dev[(size_t)sh][0].ctx, d_packed[(size_t)sh]); d_packed[(size_t)sh] = nullptr; }
  };
  {
    std::vector<std::thread> th;
    for (int sh = 0; sh < N; ++sh)
      th.emplace_back([&, sh] {
        cfrk_ctx *ctx = per_dev[(size_t)sh][0].ctx;
        const int64_t r0 = batch.nS * sh / N, r1 = batch.nS * (sh + 1) / N;
        const int64_t b0 = (r0 < batch.nS) ? batch.start[r0] : batch.nN, b1 = (r1 < batch.nS) ? batch.start[r1] : batch.nN;
        int rc;
        if ((rc = cfrk_global_begin(ctx, o.k, flags | CFRK_RUNS_ONLY, hint))) { status[(size_t)sh] = die(ctx, rc, "cfrk_global_begin"); return; }
        if (b1 <= b0) return;
        if ((rc = cfrk_global_add(ctx, batch.data + b0, nullptr, nullptr, b1 - b0, 0))) {
          if (rc == CFRK_ERR_RUNS_REFUSED) { refused[(size_t)sh] = 1; return; }     // (the shard needs several passes)
          status[(size_t)sh] = die(ctx, rc, "cfrk_global_add");
          return;
        }
        // distinct runs never exceed the shard's super-k-mers (about one per 8 bases), plus the headers;
        // a buffer that is too small is retried at four times the size
        // (k > 32: a record is two rows)
        uint64_t cap = (uint64_t)(b1 - b0) / 4 * (o.k > 32 ? 2 : 1) + (uint64_t)N * 70000 + 4096;
        for (int attempt = 0; attempt < 3; ++attempt) {
          void *d = nullptr;
          if ((rc = cfrk_device_alloc(ctx, cap * 16, &d))) { refused[(size_t)sh] = 1; return; }
          rc = cfrk_global_export_runs_device(ctx, d, cap, N, rows[(size_t)sh].data());
          if (!rc) { d_packed[(size_t)sh] = d; return; }
          cfrk_device_free(ctx, d);
          if (rc == CFRK_ERR_SMALL_BUF) { cap *= 4; continue; }
          // (CFRK_ERR_STATE: something of this shard spilled into the HBM table -- its runs are not
          //  all in the leaf streams; the single-device path counts such input as well)
          if (rc == CFRK_ERR_STATE || rc == CFRK_ERR_NOMEM) { refused[(size_t)sh] = 1; return; }
          status[(size_t)sh] = die(ctx, rc, "cfrk_global_export_runs_device");
          return;
        }
        refused[(size_t)sh] = 1;
      });
    for (auto &t : th) t.join();
    for (int r : status) if (r) { free_packed(); return r; }
    for (char r : refused)
      if (r) {
        free_packed();
        fprintf(stderr, "cfrk: a shard could not export its runs; counting on one device\n");
        return run_global(o, in, batch, per_dev[0][0], out, est);
      }
  }
  std::vector<std::vector<uint64_t>> keys((size_t)N), his((size_t)N);
  std::vector<std::vector<uint32_t>> cnts((size_t)N);
  std::vector<Spectrum> spec(o.histo ? (size_t)N : 0);
  std::vector<double> histo_s((size_t)N, 0), export_s((size_t)N, 0), query_s((size_t)N, 0);
  std::vector<std::vector<uint32_t>> qans(o.query ? (size_t)N : 0);
  {
    // owner ow gathers its segment of every shard DEVICE TO DEVICE (xGMI peer-to-peer between the
    // devices of the node; replaces the host staging of round 2), then expands and counts its leaves
    std::vector<std::thread> th;
    for (int ow = 0; ow < N; ++ow)
      th.emplace_back([&, ow] {
        cfrk_ctx *ctx = per_dev[(size_t)ow][1].ctx;
        std::vector<uint64_t> recv((size_t)N);
        uint64_t total = 0;
        for (int sh = 0; sh < N; ++sh) { recv[(size_t)sh] = rows[(size_t)sh][(size_t)ow]; total += recv[(size_t)sh]; }
        int rc;
        if ((rc = cfrk_global_begin(ctx, o.k, flags, hint / (uint64_t)N + 1024))) { status[(size_t)ow] = die(ctx, rc, "cfrk_global_begin"); return; }
        if (total) {
          void *d = nullptr;
          if ((rc = cfrk_device_alloc(ctx, total * 16, &d))) { status[(size_t)ow] = die(ctx, rc, "cfrk_device_alloc"); return; }
          uint64_t at = 0;
          for (int sh = 0; sh < N && !rc; ++sh) {
            uint64_t off = 0;
            for (int q = 0; q < ow; ++q) off += rows[(size_t)sh][(size_t)q];
            if (recv[(size_t)sh])
              rc = cfrk_memcpy_peer(ctx, (char *)d + at * 16, per_dev[(size_t)sh][0].ctx, (const char *)d_packed[(size_t)sh] + off * 16, recv[(size_t)sh] * 16);
            at += recv[(size_t)sh];
          }
          if (!rc) rc = cfrk_global_merge_runs_device(ctx, d, recv.data(), N);
          if (!rc) rc = cfrk_ctx_sync(ctx);
          cfrk_device_free(ctx, d);
          if (rc) { status[(size_t)ow] = die(ctx, rc, "cfrk_global_merge_runs_device"); return; }
        }
        uint64_t n = 0;
        rc = cfrk_global_finish(ctx, &n);
        if (rc == CFRK_ERR_COUNT_OVERFLOW) fprintf(stderr, "cfrk: warning: %s\n", cfrk_last_error(ctx));
        else if (rc == CFRK_ERR_TABLE_FULL) { refused[(size_t)ow] = 1; return; }       // (more distinct k-mers than announced)
        else if (rc) { status[(size_t)ow] = die(ctx, rc, "cfrk_global_finish"); return; }
        const double h0 = now_s();
        if (o.histo && (rc = result_spectrum(ctx, spec[(size_t)ow]))) { status[(size_t)ow] = rc; return; }
        histo_s[(size_t)ow] = now_s() - h0;
        const double q0 = now_s();
        if (o.query && (rc = query_answers(ctx, in.qreads, qans[(size_t)ow]))) { status[(size_t)ow] = rc; return; }
        query_s[(size_t)ow] = now_s() - q0;
        if (o.histo_only || o.query_only) return;
        const double e0 = now_s();
        keys[(size_t)ow].resize(n); cnts[(size_t)ow].resize(n); his[(size_t)ow].resize(n);
        rc = cfrk_global_export_range(ctx, o.min_count, o.max_count, keys[(size_t)ow].data(), his[(size_t)ow].data(),
                                      cnts[(size_t)ow].data(), n, &n);
        if (rc && rc != CFRK_ERR_COUNT_OVERFLOW) { status[(size_t)ow] = die(ctx, rc, "cfrk_global_export_range"); return; }
        keys[(size_t)ow].resize(n); cnts[(size_t)ow].resize(n); his[(size_t)ow].resize(n);
        export_s[(size_t)ow] = now_s() - e0;
      });
    for (auto &t : th) t.join();
    free_packed();
    for (int r : status) if (r) return r;
    for (char r : refused)
      if (r) {
        fprintf(stderr, "cfrk: more distinct k-mers than announced; counting on one device\n");
        return run_global(o, in, batch, per_dev[0][0], out, est);
      }
  }
  g_timing.export_ = *std::max_element(export_s.begin(), export_s.end());
  if (o.histo) {
    const double h0 = now_s();
    for (int ow = 1; ow < N; ++ow) spec[0].add(spec[(size_t)ow]);
    if (int r = write_histo(o, spec[0])) return r;
    g_timing.histo = *std::max_element(histo_s.begin(), histo_s.end()) + (now_s() - h0);
  }
  if (o.query) {
    // owners hold disjoint key sets: at most one answers a window with a count, the others 0; NONE is everyone's
    const double q0 = now_s();
    std::vector<uint32_t> &ans = qans[0];
    for (int ow = 1; ow < N; ++ow)
      for (size_t p = 0; p < ans.size(); ++p)
        if (ans[p] != CFRK_QUERY_NONE) ans[p] += qans[(size_t)ow][p];
    if (int r = write_query(o, in.qreads, o.k, ans.data())) return r;
    g_timing.query = *std::max_element(query_s.begin(), query_s.end()) + (now_s() - q0);
  }
  if (o.histo_only || o.query_only) return 0;
  // N ascending lists with disjoint keys -> one ascending list
  size_t total = 0;
  for (auto &kk : keys) total += kk.size();
  std::vector<uint64_t> mk(total), mh(total);
  std::vector<uint32_t> mc(total);
  std::vector<size_t> at((size_t)N, 0);
  // (the high words are zero for k <= 32)
  auto less = [&](int a, int b) {
    const size_t ia = at[(size_t)a], ib = at[(size_t)b];
    const uint64_t ha = his[(size_t)a][ia], hb = his[(size_t)b][ib];
    return ha != hb ? ha < hb : keys[(size_t)a][ia] < keys[(size_t)b][ib];
  };
  for (size_t i = 0; i < total; ++i) {
    int best = -1;
    for (int q = 0; q < N; ++q)
      if (at[(size_t)q] < keys[(size_t)q].size() && (best < 0 || less(q, best))) best = q;
    const size_t ib = at[(size_t)best]++;
    mk[i] = keys[(size_t)best][ib]; mh[i] = his[(size_t)best][ib]; mc[i] = cnts[(size_t)best][ib];
  }
  write_global(o, mk.data(), mh.data(), mc.data(), total, out);
  return 0;
}

// --device-parse: the file goes to the device as text and is parsed there (cfrk_fasta_parse_device, or for FASTQ
// cfrk_fastq_parse_device); no host batch
struct DeviceText {
  cfrk_ctx *ctx = nullptr;
  void *d_text = nullptr, *d_start = nullptr, *d_length = nullptr, *d_regs = nullptr;
  int8_t *d_data = nullptr;
  size_t n_text = 0;
  ~DeviceText() { for (void *d : {d_text, (void *)d_data, d_start, d_length, d_regs}) if (d) cfrk_device_free(ctx, d); }
  // 0, a negative code of the host parser (the caller prints its message), or the exit status of a reported device error
  int load(const char *in, bool plain_copy, int fmt, int min_qual, int64_t *nN, int64_t *nS, double *map_s, double *h2d_s, double *parse_ms) {
    const bool fq = fmt == CFRK_FORMAT_FASTQ;
    auto parse = [&](int8_t *data, uint64_t cap_data, int64_t *start, int32_t *length, uint64_t cap_reads) {
      return fq ? cfrk_fastq_parse_device(ctx, (const uint8_t *)d_text, n_text, min_qual, data, cap_data, start, length, cap_reads, nN, nS)
                : cfrk_fasta_parse_device(ctx, (const uint8_t *)d_text, n_text, 0, data, cap_data, start, length, cap_reads, nN, nS);
    };
    const int fd = open(in, O_RDONLY);
    if (fd < 0) return -1;
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { close(fd); return -1; }
    const size_t n = (size_t)st.st_size;
    n_text = n;
    *nN = *nS = 0;
    if (n == 0) { close(fd); return 0; }
    int rc;
    if ((rc = cfrk_device_alloc(ctx, n + 16, &d_text))) { close(fd); return die(ctx, rc, "cfrk_device_alloc"); }
    // One copy from the mapping by default.  The ring of pinned staging buffers (--text-copy staged) was built for this
    // and measured: for a mapped, populated file it is no faster than the runtime's own pageable path.
    const double tm = now_s();
    void *m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) return -1;
    const double t0 = now_s();
    *map_s = t0 - tm;
    rc = plain_copy ? cfrk_memcpy_h2d(ctx, d_text, m, n) : cfrk_memcpy_h2d_staged(ctx, d_text, m, n);
    munmap(m, n);
    if (rc) return die(ctx, rc, plain_copy ? "cfrk_memcpy_h2d" : "cfrk_memcpy_h2d_staged");
    *h2d_s = now_s() - t0;
    const double t1 = now_s();
    rc = parse(nullptr, 0, nullptr, nullptr, 0);
    if (rc == CFRK_ERR_SMALL_BUF) {
      void *dd = nullptr;
      if ((rc = cfrk_device_alloc(ctx, (size_t)*nN + 64, &dd))) return die(ctx, rc, "cfrk_device_alloc");
      d_data = (int8_t *)dd;
      if ((rc = cfrk_device_alloc(ctx, (size_t)*nS * 8, &d_start)) || (rc = cfrk_device_alloc(ctx, (size_t)*nS * 4, &d_length)))
        return die(ctx, rc, "cfrk_device_alloc");
      rc = parse(d_data, (uint64_t)*nN, (int64_t *)d_start, (int32_t *)d_length, (uint64_t)*nS);
      if (!rc) rc = cfrk_ctx_sync(ctx);
    }
    // What the host parser refuses with -2 (a sequence line before the first header: the only text it can refuse in native
    // mode short of a record of 2^31 bases) is reported in its words; the wording looked for is pinned at its cfrk_fail in
    // ingest.hip and by tests/test_gpu_ingest.py.  Anything else the device parser refuses is reported in the library's.
    if (rc == CFRK_ERR_LAYOUT) {
      if (strstr(cfrk_last_error(ctx), "before the first header")) return -2;
      fprintf(stderr, "cfrk: cannot read %s (%s)\n", in, cfrk_last_error(ctx));
      return 1;
    }
    if (rc) return die(ctx, rc, fq ? "cfrk_fastq_parse_device" : "cfrk_fasta_parse_device");
    *parse_ms = (now_s() - t1) * 1e3;
    cfrk_device_free(ctx, d_text);                      // (the codes are what is counted)
    d_text = nullptr;
    return 0;
  }
  int sketch(const Options &o, int64_t nN, Estimate &e) {
    const double t0 = now_s();
    std::vector<uint8_t> regs(CFRK_SKETCH_REGS, 0);
    int rc;
    if (nN > 0) {
      if ((rc = cfrk_device_alloc(ctx, CFRK_SKETCH_REGS, &d_regs)) || (rc = cfrk_memcpy_h2d(ctx, d_regs, regs.data(), regs.size())))
        return die(ctx, rc, "cfrk_device_alloc");
      if ((rc = cfrk_distinct_sketch_device(ctx, d_data, nN, o.k, o.canonical ? CFRK_CANONICAL : 0, (uint8_t *)d_regs, &e.windows)))
        return die(ctx, rc, "cfrk_distinct_sketch_device");
      if ((rc = cfrk_memcpy_d2h(ctx, regs.data(), d_regs, regs.size()))) return die(ctx, rc, "cfrk_memcpy_d2h");
    }
    cfrk_sketch_estimate(regs.data(), &e.distinct);
    cfrk_sketch_hint(regs.data(), &e.hint);
    e.have = true;
    g_timing.estimate = now_s() - t0; g_timing.distinct_estimate = e.distinct;
    fprintf(stderr, "cfrk-estimate distinct=%.0f windows=%llu hint=%llu\n", e.distinct, (unsigned long long)e.windows, (unsigned long long)e.hint);
    return 0;
  }
};

// one FASTA file -> one .cfrk file on the given workers
// a FASTA file being parsed on a thread of its own while the caller creates the device contexts (single-file mode: HIP
// start-up and two contexts are ~0.15 s, the parse of a 1.6 GB file ~0.28 s -- they need nothing from each other)
double g_contexts_s = 0, g_wait_parse = 0;
struct Parsed {
  cfrk_batch batch;
  int rc = 0;
  double t0 = 0, seconds = 0;
  std::thread th;
  void start(const Options &o, const char *in, int fmt) {
    t0 = now_s();
    const int flags = (o.native || o.global || o.sparse) ? 0 : CFRK_INGEST_COMPAT, min_qual = o.min_qual;
    th = std::thread([this, in, fmt, flags, min_qual] { rc = read_reads(in, fmt, flags, min_qual, &batch); seconds = now_s() - t0; });
  }
};

int run_file(const Options &o, Inputs &inputs, const char *in, const char *outp, std::vector<Worker> &workers,
             std::vector<std::vector<Worker>> *per_dev = nullptr, Parsed *pre = nullptr, int fmt = -1) {
  cfrk_batch batch;
  if (fmt < 0) {                                        // (--batch: every file is looked at on its own)
    fmt = file_format(o, in);
    if (!format_allowed(o, in, fmt)) return 1;
  }
  if (o.normalize_out) {
    if (o.normalize_format == CFRK_TEXT_FASTQ && fmt != CFRK_FORMAT_FASTQ) {
      fprintf(stderr, "cfrk: --normalize-format fastq needs a FASTQ input: %s is read as FASTA\n", in);
      return 1;
    }
    inputs.nformat = fmt; inputs.npath = in;
    if (o.normalize_names && read_file(in, inputs.ntext)) return 1;
  }
  double t0 = now_s();
  int rc;
  DeviceText dt;
  dt.ctx = workers[0].ctx;
  double text_map = 0, text_h2d = 0, device_parse_ms = 0;
  if (o.device_parse) {
    memset(&batch, 0, sizeof batch);
    rc = dt.load(in, o.text_copy_plain, fmt, o.min_qual, &batch.nN, &batch.nS, &text_map, &text_h2d, &device_parse_ms);
    if (rc > 0) return rc;                              // (a device error, reported)
  } else if (pre) {
    const double w0 = now_s();
    pre->th.join();
    g_wait_parse = now_s() - w0;
    rc = pre->rc; batch = pre->batch; t0 = pre->t0;
    if (rc) return 1;                                   // (read_reads has said why)
  } else {
    if (read_reads(in, fmt, (o.native || o.global || o.sparse) ? 0 : CFRK_INGEST_COMPAT, o.min_qual, &batch)) return 1;
    rc = 0;
  }
  if (rc) { fprintf(stderr, "cfrk: cannot read %s (error %d)\n", in, rc); return 1; }
  const double t1 = pre ? t0 + pre->seconds : now_s();
  g_timing = Timing();
  g_timing.contexts = g_contexts_s; g_timing.wait_parse = g_wait_parse;
  g_timing.parse = t1 - t0; g_timing.nN = batch.nN; g_timing.nS = batch.nS; g_timing.in_format = fmt;
  if (o.device_parse) { g_timing.parse = 0; g_timing.device_parse = true; g_timing.text_map = text_map; g_timing.text_h2d = text_h2d; g_timing.device_parse_ms = device_parse_ms; }
  { FILE *f = fopen(in, "rb"); if (f) { fseek(f, 0, SEEK_END); g_timing.fasta_bytes = (int64_t)ftell(f); fclose(f); } }
  std::thread freer;                                  // (global mode: frees the batch beside the export)
  const double to0 = now_s();
  const bool no_out = o.histo_only || o.query_only || o.estimate_only;
  FILE *out = no_out ? nullptr : fopen(outp, "wb");   // PrintFreq opens with "w" even when empty
  const double t_open = now_s() - to0;
  if (!out && !no_out) { fprintf(stderr, "cfrk: cannot write %s\n", outp); cfrk_host_free_batch(&batch); return 1; }
  const bool multi = o.global && per_dev && per_dev->size() > 1 && o.k >= 16 && o.k <= 64 && batch.nS >= (int64_t)per_dev->size();
  Estimate est;
  rc = 0;
  if (o.estimate || o.estimate_only || o.auto_hint) {
    std::vector<cfrk_ctx *> ctxs;
    if (multi) for (auto &d : *per_dev) ctxs.push_back(d[0].ctx);
    else ctxs.push_back(workers[0].ctx);
    rc = o.device_parse ? dt.sketch(o, batch.nN, est) : sketch_batch(o, batch, ctxs, est);
  }
  if (!rc && !o.estimate_only) {
    if (multi) rc = run_global_multi(o, inputs, batch, *per_dev, out, est);
    else if (o.device_parse) rc = run_global(o, inputs, batch, workers[0], out, est, nullptr, nullptr, true, dt.d_data);
    else if (o.global) rc = run_global(o, inputs, batch, workers[0], out, est, &freer, &batch);
    else { const double p0 = now_s(); rc = run_per_read(o, batch, workers, out); g_timing.per_read = now_s() - p0; }
  }
  if (!o.global && out) { fflush(out); g_timing.out_bytes = (uint64_t)ftell(out); }
  const double tf0 = now_s();
  if (out) fclose(out);
  const double tf1 = now_s();
  if (freer.joinable()) freer.join();
  else cfrk_host_free_batch(&batch);
  g_timing.total = now_s() - t0;
  g_timing.close = tf1 - tf0; g_timing.free_batch = now_s() - tf1; g_timing.open = t_open;
  char query_field[192] = "";     // (only with --query / --device-parse: the line is unchanged otherwise)
  if (g_timing.device_parse) snprintf(query_field, sizeof query_field, "\"text_map_s\": %.4f, \"text_h2d_s\": %.4f, \"device_parse_ms\": %.3f, ", g_timing.text_map, g_timing.text_h2d, g_timing.device_parse_ms);
  const size_t qf = strlen(query_field);
  if (o.query_stats) snprintf(query_field + qf, sizeof query_field - qf, "\"query_s\": %.4f, \"stats_s\": %.4f, ", g_timing.query, g_timing.stats);
  else if (o.query) snprintf(query_field + qf, sizeof query_field - qf, "\"query_s\": %.4f, ", g_timing.query);
  if (o.timing)
    fprintf(stderr, "cfrk-timing {\"fasta_bytes\": %lld, \"reads\": %lld, \"code_bytes\": %lld, \"parse_s\": %.4f, \"add_call_s\": %.4f, "
            "\"finish_wait_s\": %.4f, \"count_kernels_ms\": %.3f, \"export_s\": %.4f, \"format_s\": %.4f, \"write_s\": %.4f, "
            "\"per_read_pipeline_s\": %.4f, \"entries\": %llu, \"out_bytes\": %llu, \"contexts_s\": %.4f, \"wait_for_parser_s\": %.4f, "
            "\"begin_s\": %.4f, \"open_out_s\": %.4f, \"close_out_s\": %.4f, \"free_batch_s\": %.4f, \"histo_s\": %.4f, %s\"attempts\": %d, "
            "\"estimate_s\": %.4f, \"distinct_estimate\": %.0f, \"hint\": %llu, \"format\": \"%s\", \"wall_s\": %.4f}\n",
            (long long)g_timing.fasta_bytes, (long long)g_timing.nS, (long long)g_timing.nN, g_timing.parse, g_timing.add_call,
            g_timing.finish_wait, (double)g_timing.count_kernels_ms, g_timing.export_, g_timing.format, g_timing.write,
            g_timing.per_read, (unsigned long long)g_timing.entries, (unsigned long long)g_timing.out_bytes, g_timing.contexts,
            g_timing.wait_parse, g_timing.begin, g_timing.open, g_timing.close, g_timing.free_batch, g_timing.histo, query_field, g_timing.attempts,
            g_timing.estimate, g_timing.distinct_estimate, (unsigned long long)g_timing.hint, g_timing.in_format == CFRK_FORMAT_FASTQ ? "fastq" : "fasta", g_timing.total);
  return rc;
}

// --query-db: a saved CFRKGLB1 count file merged into a fresh job on one device, then queried
int run_query_db(const Options &o, const Inputs &in) {
  std::vector<char> img;
  if (read_file(o.query_db, img)) return 1;
  int k = 0, bflags = 0;
  uint64_t n = 0;
  if (cfrk_host_read_binary(img.data(), img.size(), &k, &bflags, &n, nullptr, nullptr, nullptr) || k < 1 || k > 64) {
    fprintf(stderr, "cfrk: %s is not a CFRKGLB1 count file\n", o.query_db);
    return 1;
  }
  std::vector<uint64_t> lo(n), hi(n);
  std::vector<uint32_t> cnt(n);
  cfrk_host_read_binary(img.data(), img.size(), &k, &bflags, &n, lo.data(), hi.data(), cnt.data());
  img.clear();
  img.shrink_to_fit();
  cfrk_ctx *ctx = nullptr;
  int rc;
  if ((rc = cfrk_ctx_create(o.device, nullptr, &ctx))) return die(nullptr, rc, "cfrk_ctx_create");
  struct Destroy { cfrk_ctx *c; ~Destroy() { cfrk_ctx_destroy(c); } } destroy{ctx};
  const double q0 = now_s();
  if ((rc = cfrk_global_begin(ctx, k, (bflags & CFRK_BIN_CANONICAL) ? CFRK_CANONICAL : 0, n + 1024)))
    return die(ctx, rc, "cfrk_global_begin");
  if (n) {
    DeviceBufs bufs(ctx);
    void *d_lo = nullptr, *d_hi = nullptr, *d_cnt = nullptr;
    if (!(rc = bufs.alloc(n * 8, &d_lo)) && !(rc = bufs.alloc(n * 8, &d_hi)) &&
        !(rc = bufs.alloc(n * 4, &d_cnt)) && !(rc = cfrk_memcpy_h2d(ctx, d_lo, lo.data(), n * 8)) &&
        !(rc = cfrk_memcpy_h2d(ctx, d_hi, hi.data(), n * 8)) && !(rc = cfrk_memcpy_h2d(ctx, d_cnt, cnt.data(), n * 4)) &&
        !(rc = cfrk_global_merge_device(ctx, (const uint64_t *)d_lo, (const uint64_t *)d_hi, (const uint32_t *)d_cnt, (int64_t)n)))
      rc = cfrk_ctx_sync(ctx);
    bufs.release();
    if (rc) return die(ctx, rc, "loading the count file");
  }
  if (o.query_out) {
    std::vector<uint32_t> ans;
    if ((rc = query_answers(ctx, in.qreads, ans)) || (rc = write_query(o, in.qreads, k, ans.data()))) return rc;
  }
  const double s0 = now_s();
  if (o.query_stats && (rc = write_query_stats(o, ctx, in.qreads))) return rc;
  if ((rc = check_query_pairs(o, ctx, in))) return rc;
  if (o.filter_out && (rc = write_filter(o, ctx, in, k))) return rc;
  if (o.correct_out && (rc = write_correct(o, ctx, in))) return rc;
  if (o.timing && o.query_stats)
    fprintf(stderr, "cfrk-timing {\"entries\": %llu, \"query_s\": %.4f, \"stats_s\": %.4f}\n", (unsigned long long)n, s0 - q0, now_s() - s0);
  else if (o.timing) fprintf(stderr, "cfrk-timing {\"entries\": %llu, \"query_s\": %.4f}\n", (unsigned long long)n, now_s() - q0);
  return 0;
}

// the query, map and second-file inputs, read before the input is counted.  0, or 1 (the error reported)
int read_inputs(const Options &o, Inputs &in) {
  if (o.query) in.qformat = file_format(o, o.query);
  if (o.filter_format == CFRK_TEXT_FASTQ && in.qformat != CFRK_FORMAT_FASTQ) {
    fprintf(stderr, "cfrk: --filter-format fastq needs a FASTQ --query file: %s is read as FASTA\n", o.query);
    return 1;
  }
  if (o.correct_format == CFRK_TEXT_FASTQ && in.qformat != CFRK_FORMAT_FASTQ) {
    fprintf(stderr, "cfrk: --correct-format fastq needs a FASTQ --query file: %s is read as FASTA\n", o.query);
    return 1;
  }
  if (o.query && read_reads(o.query, in.qformat, 0, 0, &in.qreads)) return 1;
  if ((o.filter_names || o.correct_names) && read_file(o.query, in.qtext)) return 1;
  if (o.unitigs_map && read_reads(o.unitigs_map, file_format(o, o.unitigs_map), 0, 0, &in.mreads)) return 1;
  if (o.query2) {
    if (file_format(o, o.query2) != in.qformat) { fprintf(stderr, "cfrk: %s and %s are not of one format\n", o.query, o.query2); return 1; }
    if (read_reads(o.query2, in.qformat, 0, 0, &in.qreads2)) return 1;
    if ((o.filter_names || o.correct_names) && read_file(o.query2, in.qtext2)) return 1;
    if (in.qreads2.nS != in.qreads.nS) {
      fprintf(stderr, "cfrk: %s holds %lld records and %s holds %lld: record j of each is a pair\n", o.query, (long long)in.qreads.nS, o.query2, (long long)in.qreads2.nS);
      return 1;
    }
  }
  if (o.paired && o.query && (o.filter_out || o.correct_out) && odd_records(o.query, in.qreads.nS)) return 1;
  return 0;
}

}  // namespace

// start-up only: the options, the inputs that are read first, the contexts, the mode
int main(int argc, char **argv) {
  Options o;
  Inputs in;
  if (parse_options(argc, argv, o) || check_options(o) || read_inputs(o, in)) return 1;
  if (o.query_db) return run_query_db(o, in);
  if (apply_positionals(o)) return 1;
  const std::vector<const char *> &pos = o.pos;
  const int batch_n = o.batch_n;

  // single-file mode: the parse starts now, beside the creation of the contexts
  int fmt = -1;
  if (batch_n < 0) {
    fmt = file_format(o, pos[0]);
    if (!format_allowed(o, pos[0], fmt)) return 1;
  }
  Parsed pre;
  if (batch_n < 0 && !o.device_parse) pre.start(o, pos[0], fmt);
  struct Joiner { Parsed &p; ~Joiner() { if (p.th.joinable()) { p.th.join(); if (!p.rc) cfrk_host_free_batch(&p.batch); } } } joiner{pre};   // (early returns)
  const double tc0 = now_s();                          // (runtime start-up + the contexts)
  int ndev = 0, rc;
  if ((rc = cfrk_device_count(&ndev))) return die(nullptr, rc, "cfrk_device_count");
  if (!o.same_device && o.device + o.gpus > ndev) {
    fprintf(stderr, "cfrk: --device %d --gpus %d but %d device(s) present\n", o.device, o.gpus, ndev);
    return 1;
  }
  // two contexts (streams) per device: chunk c+1 is copied in while chunk c is counted / copied out / formatted
  std::vector<std::vector<Worker>> per_dev((size_t)o.gpus);
  for (int g = 0; g < o.gpus; ++g)
    for (int s = 0; s < 2; ++s) {
      Worker w;
      w.device = o.same_device ? o.device : o.device + g;
      if ((rc = cfrk_ctx_create(w.device, nullptr, &w.ctx))) return die(nullptr, rc, "cfrk_ctx_create");
      per_dev[(size_t)g].push_back(w);
    }

  g_contexts_s = now_s() - tc0;
  int status = 0;
  if (batch_n < 0) {
    std::vector<Worker> all;
    for (int s = 0; s < 2; ++s)                       // device-major would put both streams of a device first
      for (int g = 0; g < o.gpus; ++g) all.push_back(per_dev[(size_t)g][(size_t)s]);
    status = run_file(o, in, pos[0], pos[1], all, &per_dev, o.device_parse ? nullptr : &pre, fmt);
  } else {
    // file i goes to device i % gpus (swift/cfrk.swf:15-20 starts one cfrk process per file)
    std::vector<int> st((size_t)o.gpus, 0);
    std::vector<std::thread> th;
    for (int g = 0; g < o.gpus; ++g)
      th.emplace_back([&, g] {
        for (int i = g; i < batch_n; i += o.gpus) {
          const std::string file = std::string(pos[0]) + "_" + std::to_string(i) + ".fasta";
          const std::string outp = std::string(pos[1]) + "_" + std::to_string(i) + ".cfrk";
          const int r = run_file(o, in, file.c_str(), outp.c_str(), per_dev[(size_t)g]);
          if (r && !st[(size_t)g]) st[(size_t)g] = r;
        }
      });
    for (auto &t : th) t.join();
    for (int r : st) if (r && !status) status = r;
  }
  for (auto &d : per_dev) for (auto &w : d) cfrk_ctx_destroy(w.ctx);
  return status;
}
