// cli_query.cpp -- what the `cfrk` command does with reads against the finished count: --query-out, --query-stats,
// --filter-out, --correct-out, the kept reads of --normalize-out, and the check of the mates' names (--paired / --query2).
#include "cli_util.h"

// --query: the answers of one result for every window of the query reads q.  0, or the exit status (the error reported)
int query_answers(cfrk_ctx *ctx, const cfrk_batch &q, std::vector<uint32_t> &ans) {
  ans.assign((size_t)q.nN, CFRK_QUERY_NONE);
  if (q.nN == 0) return 0;
  const int rc = cfrk_global_query_reads(ctx, q.data, q.start, q.length, q.nN, q.nS, ans.data());
  return rc ? die(ctx, rc, "cfrk_global_query_reads") : 0;
}

int write_query(const Options &o, const cfrk_batch &q, int k, const uint32_t *ans) {
  std::string buf;
  format_into(buf, [&](char *out, size_t room) { return cfrk_host_format_query(ans, q.start, q.length, q.nS, k, out, room); });
  return write_file(o.query_out, buf);
}

// --query-stats: the query reads' abundance statistics against one result, written to SFILE
int write_query_stats(const Options &o, cfrk_ctx *ctx, const cfrk_batch &q) {
  std::vector<cfrk_read_stats> st((size_t)q.nS);
  if (q.nS) {
    const int rc = cfrk_global_read_stats(ctx, q.data, q.start, q.length, q.nN, q.nS, o.stats_below, st.data());
    if (rc) return die(ctx, rc, "cfrk_global_read_stats");
  }
  std::string buf;
  format_into(buf, [&](char *out, size_t room) { return cfrk_host_format_read_stats(st.data(), q.nS, out, room); });
  return write_file(o.query_stats, buf);
}

namespace {

// The reads that d_span / d_keep / min_len leave of the batch q on the device (only q's sizes are read), as text in buf:
// FASTA named by record number (select, one copy back, formatted here), or -- names -- FASTA / FASTQ text with the names
// and qualities the records have in `text`, the file q was parsed from, written on the device (index, emit, one copy
// back).  What --filter-out and --normalize-out share.  0, or a CFRK_ERR_* code with *what naming the call.
int emit_selected(cfrk_ctx *ctx, const cfrk_batch &q, const void *d_data, const void *d_start, const void *d_length, const void *d_span,
                  const void *d_keep, long min_len, bool names, const std::vector<char> &text, int text_format, int out_format,
                  const char *text_path, std::string &buf, const char **what) {
  const size_t nN = (size_t)q.nN, nS = (size_t)q.nS;
  std::vector<int8_t> data;
  std::vector<int64_t> start, index;
  std::vector<int32_t> length;
  int64_t onN = 0, onS = 0;
  int rc = 0;
  if (nS) {
    DeviceBufs bufs(ctx);
    void *o_data = nullptr, *o_start = nullptr, *o_length = nullptr, *o_index = nullptr;
    void *d_text = nullptr, *d_rec = nullptr, *d_out = nullptr;
    *what = "cfrk_device_alloc";
    if (!(!names && ((rc = bufs.alloc(nN + 16, &o_data)) || (rc = bufs.alloc(nS * 8, &o_start)) ||
                     (rc = bufs.alloc(nS * 4, &o_length)) || (rc = bufs.alloc(nS * 8, &o_index)))) &&
        !(names && ((rc = bufs.alloc(text.size() + 16, &d_text)) || (rc = bufs.alloc(nS * sizeof(cfrk_text_record), &d_rec))))) {
      if (names) {
        // the index of the file's text numbers the records as the host parser did; the emitter sizes, then writes
        int64_t inS = 0;
        uint64_t onb = 0;
        *what = "cfrk_memcpy_h2d";
        if (!(rc = cfrk_memcpy_h2d(ctx, d_text, text.data(), text.size()))) {
          *what = "cfrk_text_index_device";
          rc = cfrk_text_index_device(ctx, (const uint8_t *)d_text, text.size(), text_format, (cfrk_text_record *)d_rec, nS, &inS);
        }
        if (!rc && inS != q.nS) {
          fprintf(stderr, "cfrk: %s: %lld records parsed, %lld indexed\n", text_path, (long long)q.nS, (long long)inS);
          rc = CFRK_ERR_LAYOUT;
        }
        for (int pass = 0; pass < 2 && !rc; ++pass) {
          *what = "cfrk_reads_emit_text_device";
          rc = cfrk_reads_emit_text_device(ctx, (const int8_t *)d_data, (const int64_t *)d_start, (const int32_t *)d_length, q.nN, q.nS,
                                           (const cfrk_read_span *)d_span, (const uint8_t *)d_keep, (int32_t)min_len, (const uint8_t *)d_text,
                                           text.size(), (const cfrk_text_record *)d_rec, out_format, (uint8_t *)d_out, pass ? onb : 0, &onb, &onS);
          if (pass == 0 && rc == CFRK_ERR_SMALL_BUF) { *what = "cfrk_device_alloc"; rc = bufs.alloc(onb + 16, &d_out); }
          else break;
        }
        if (!rc && onb) {
          *what = "cfrk_memcpy_d2h";
          buf.resize((size_t)onb);
          rc = cfrk_memcpy_d2h(ctx, &buf[0], d_out, (size_t)onb);
        }
      } else {
        *what = "cfrk_reads_select_device";
        rc = cfrk_reads_select_device(ctx, (const int8_t *)d_data, (const int64_t *)d_start, (const int32_t *)d_length, q.nN, q.nS,
                                      (const cfrk_read_span *)d_span, (const uint8_t *)d_keep, (int32_t)min_len, (int8_t *)o_data, nN,
                                      (int64_t *)o_start, (int32_t *)o_length, (int64_t *)o_index, nS, &onN, &onS);
        if (!rc) {
          *what = "cfrk_memcpy_d2h";
          data.resize((size_t)onN); start.resize((size_t)onS); length.resize((size_t)onS); index.resize((size_t)onS);
          if (onS && !(rc = cfrk_memcpy_d2h(ctx, data.data(), o_data, (size_t)onN)) && !(rc = cfrk_memcpy_d2h(ctx, start.data(), o_start, (size_t)onS * 8)) &&
              !(rc = cfrk_memcpy_d2h(ctx, length.data(), o_length, (size_t)onS * 4)))
            rc = cfrk_memcpy_d2h(ctx, index.data(), o_index, (size_t)onS * 8);
        }
      }
    }
    const int rc2 = cfrk_ctx_sync(ctx);
    bufs.release();
    if (rc) return rc;
    if (rc2) { *what = "cfrk_ctx_sync"; return rc2; }
  }
  if (!names)
    format_into(buf, [&](char *out, size_t room) { return cfrk_host_format_fasta(data.data(), start.data(), length.data(), index.data(), onS, out, room); });
  return 0;
}

}  // namespace

// --paired / --query2 with a names writer: the mates' names compared on the device.  The text(s) go up and are indexed for
// this alone (the writers index their own copy again behind it); text_b NULL: one interleaved text, pairs are records
// 2j and 2j + 1.  0, or the exit status with the error reported: the first bad pair shows both headers.
int check_mate_names(cfrk_ctx *ctx, int64_t n_pairs, int text_format, const std::vector<char> &text_a, const char *path_a,
                     const std::vector<char> *text_b, const char *path_b) {
  if (n_pairs == 0) return 0;
  const int64_t per = text_b ? n_pairs : 2 * n_pairs;              // records of a text
  const std::vector<char> &tb = text_b ? *text_b : text_a;
  DeviceBufs bufs(ctx);
  void *d_ta = nullptr, *d_tb = nullptr, *d_ra = nullptr, *d_rb = nullptr;
  const char *what = "cfrk_device_alloc";
  int64_t first = -1, bad = 0, got = 0;
  cfrk_text_record ra{}, rb{};
  int rc;
  auto up = [&](const std::vector<char> &t, const char *path, void **d_t, void **d_r) {
    what = "cfrk_device_alloc";
    if ((rc = bufs.alloc(t.size() + 16, d_t)) || (rc = bufs.alloc((size_t)per * sizeof(cfrk_text_record), d_r))) return;
    what = "cfrk_memcpy_h2d";
    if ((rc = cfrk_memcpy_h2d(ctx, *d_t, t.data(), t.size()))) return;
    what = "cfrk_text_index_device";
    if ((rc = cfrk_text_index_device(ctx, (const uint8_t *)*d_t, t.size(), text_format, (cfrk_text_record *)*d_r, (uint64_t)per, &got))) return;
    if (got != per) { fprintf(stderr, "cfrk: %s: %lld records parsed, %lld indexed\n", path, (long long)per, (long long)got); rc = CFRK_ERR_LAYOUT; }
  };
  up(text_a, path_a, &d_ta, &d_ra);
  if (!rc && text_b) up(tb, path_b, &d_tb, &d_rb);
  if (!rc) {
    const cfrk_text_record *rec_a = (const cfrk_text_record *)d_ra, *rec_b = text_b ? (const cfrk_text_record *)d_rb : rec_a + 1;
    what = "cfrk_text_pair_check_device";
    rc = cfrk_text_pair_check_device(ctx, n_pairs, text_b ? 1 : 2, (const uint8_t *)d_ta, text_a.size(), rec_a,
                                     (const uint8_t *)(text_b ? d_tb : d_ta), tb.size(), rec_b, &first, &bad);
    if (!rc && bad) {
      const int64_t stride = text_b ? 1 : 2;
      what = "cfrk_memcpy_d2h";
      if (!(rc = cfrk_memcpy_d2h(ctx, &ra, rec_a + first * stride, sizeof ra))) rc = cfrk_memcpy_d2h(ctx, &rb, rec_b + first * stride, sizeof rb);
    }
  }
  const int rc2 = cfrk_ctx_sync(ctx);
  bufs.release();
  if (rc) return die(ctx, rc, what);
  if (rc2) return die(ctx, rc2, "cfrk_ctx_sync");
  if (!bad) return 0;
  // (the index wrote both records from these very texts: their header ranges lie inside them)
  fprintf(stderr, "cfrk: pair %lld: the mates' names differ: '%.*s' (%s) and '%.*s' (%s); %lld pair(s) in all (--pair-check off skips this check)\n",
          (long long)first, (int)ra.head_len, text_a.data() + ra.head_off, path_a, (int)rb.head_len, tb.data() + rb.head_off, text_b ? path_b : path_a,
          (long long)bad);
  return 1;
}

namespace {

// --filter-out: one file's reads on the device with what the filter computes of them: the solid spans (--filter-trim) and
// the keep bytes of the median rule (--filter-min-median / --filter-max-median); NULL where the run asks for neither
struct FilterSide {
  DeviceBufs bufs;                       // (freed when the side goes: the caller has synchronised)
  void *d_data = nullptr, *d_start = nullptr, *d_length = nullptr, *d_span = nullptr, *d_keep = nullptr, *d_stats = nullptr;
  explicit FilterSide(cfrk_ctx *ctx) : bufs(ctx) {}
  int prepare(const Options &o, const cfrk_batch &q, const char **what) {
    cfrk_ctx *ctx = bufs.ctx;
    const size_t nS = (size_t)q.nS;
    const bool trim = o.filter_trim >= 0;
    int rc = 0;
    if (!nS || (rc = bufs.upload(q, &d_data, &d_start, &d_length, what))) return rc;
    *what = "cfrk_device_alloc";
    if ((trim && (rc = bufs.alloc(nS * sizeof(cfrk_read_span), &d_span))) ||
        (o.filter_median && ((rc = bufs.alloc(nS, &d_keep)) || (rc = bufs.alloc(nS * sizeof(cfrk_read_stats), &d_stats))))) return rc;
    if (trim) {
      *what = "cfrk_global_read_spans_device";
      rc = cfrk_global_read_spans_device(ctx, (const int8_t *)d_data, (const int64_t *)d_start, (const int32_t *)d_length, q.nN, q.nS,
                                         o.filter_min_count, o.filter_max_count, o.filter_trim, (cfrk_read_span *)d_span);
    }
    if (!rc && o.filter_median) {
      // the rows come down (32 bytes per read), the keep bytes go up (1 byte per read)
      *what = "cfrk_global_read_stats_device";
      std::vector<cfrk_read_stats> st(nS);
      std::vector<uint8_t> keep(nS);
      if (!(rc = cfrk_global_read_stats_device(ctx, (const int8_t *)d_data, (const int64_t *)d_start, (const int32_t *)d_length, q.nN, q.nS, 0,
                                               (cfrk_read_stats *)d_stats)) &&
          !(rc = cfrk_memcpy_d2h(ctx, st.data(), d_stats, nS * sizeof(cfrk_read_stats)))) {
        for (size_t i = 0; i < nS; ++i) keep[i] = st[i].median >= o.filter_min_median && st[i].median <= o.filter_max_median;
        rc = cfrk_memcpy_h2d(ctx, d_keep, keep.data(), nS);
      }
    }
    return rc;
  }
};

}  // namespace

// the query reads trimmed to their solid spans and filtered, on the device, written to FFILE as FASTA named by record
// number, or -- --filter-names -- as FASTA / FASTQ text with QFILE's names and qualities (emit_selected).
// --paired / --query2: the spans, --filter-min-len and the median keep bytes are joined per pair on the device
// (CFRK_PAIR_BOTH); FFILE (and FFILE2) receive whole pairs, --filter-orphans' OFILE the survivors whose mate did not
// survive, every file through the same writer with the joined bytes as its keep bytes.
int write_filter(const Options &o, cfrk_ctx *ctx, const Inputs &in, int k) {
  const cfrk_batch &q = in.qreads, &q2 = in.qreads2;
  const size_t nS = (size_t)q.nS;
  const int tf = text_format_of(in.qformat);
  const long min_len = o.filter_min_len >= 0 ? (long)o.filter_min_len : (long)k;
  std::string buf, buf2, orphans;
  FilterSide a(ctx), b(ctx);
  DeviceBufs bufs(ctx);
  void *d_pair = nullptr, *d_orphan = nullptr;
  const char *what = "";
  cfrk_pair_counts pc{};
  auto emit = [&](const cfrk_batch &r, const FilterSide &f, const void *d_keep, const std::vector<char> &text, const char *path, std::string &out) {
    return emit_selected(ctx, r, f.d_data, f.d_start, f.d_length, f.d_span, d_keep, min_len, o.filter_names, text, tf, o.filter_format, path, out, &what);
  };
  int rc = a.prepare(o, q, &what);
  if (!rc && o.query2) rc = b.prepare(o, q2, &what);
  if (!rc && !o.mates()) rc = emit(q, a, a.d_keep, in.qtext, o.query, buf);
  else if (!rc && nS) {
    // mate B of pair j: the next element of the one file's arrays, or element j of QFILE2's; the joined bytes of both
    // layouts lie in one array of a byte per read (QFILE2's behind QFILE's)
    const size_t step = o.query2 ? 0 : 1, total = o.query2 ? 2 * nS : nS, off_b = o.query2 ? nS : 1;
    const FilterSide &fb = o.query2 ? b : a;
    what = "cfrk_device_alloc";
    if (!(rc = bufs.alloc(total, &d_pair)) && !(rc = bufs.alloc(total, &d_orphan))) {
      what = "cfrk_reads_pair_keep_device";
      rc = cfrk_reads_pair_keep_device(ctx, (int64_t)(o.query2 ? nS : nS / 2), o.query2 ? 1 : 2, CFRK_PAIR_BOTH, (int32_t)min_len,
                                       (const uint8_t *)a.d_keep, fb.d_keep ? (const uint8_t *)fb.d_keep + step : nullptr,
                                       (const cfrk_read_span *)a.d_span, fb.d_span ? (const cfrk_read_span *)fb.d_span + step : nullptr,
                                       (const int32_t *)a.d_length, (const int32_t *)fb.d_length + step, (uint8_t *)d_pair,
                                       (uint8_t *)d_pair + off_b, (uint8_t *)d_orphan, (uint8_t *)d_orphan + off_b, &pc);
    }
    if (!rc) rc = emit(q, a, d_pair, in.qtext, o.query, buf);
    if (!rc && o.query2) rc = emit(q2, b, (const uint8_t *)d_pair + nS, in.qtext2, o.query2, buf2);
    if (!rc && o.filter_orphans) rc = emit(q, a, d_orphan, in.qtext, o.query, orphans);
    if (!rc && o.filter_orphans && o.query2) {
      std::string more;
      if (!(rc = emit(q2, b, (const uint8_t *)d_orphan + nS, in.qtext2, o.query2, more))) orphans += more;
    }
  }
  const int rc2 = nS ? cfrk_ctx_sync(ctx) : 0;
  bufs.release();
  if (rc) return die(ctx, rc, what);
  if (rc2) return die(ctx, rc2, "cfrk_ctx_sync");
  if (o.mates())
    fprintf(stderr, "cfrk: filter: %lld pairs kept, %lld orphans (%lld + %lld) %s, %lld pairs dropped\n", (long long)pc.pairs,
            (long long)(pc.orphans_a + pc.orphans_b), (long long)pc.orphans_a, (long long)pc.orphans_b,
            o.filter_orphans ? "written" : "dropped", (long long)pc.dropped);
  if (write_file(o.filter_out, buf)) return 1;
  if (o.query2 && write_file(o.filter_out2, buf2)) return 1;
  return o.filter_orphans ? write_file(o.filter_orphans, orphans) : 0;
}

namespace {

// --correct-out: one file's reads corrected against the whole result on the device; every read is written to out_path through
// emit_selected (the corrected buffer, no span, no keep bytes), the cfrk_read_fix rows appended to --correct-report's text
int correct_file(const Options &o, cfrk_ctx *ctx, int text_fmt, const cfrk_batch &q, const std::vector<char> &qtext, const char *qpath,
                 const char *out_path, std::string *report) {
  const size_t nN = (size_t)q.nN, nS = (size_t)q.nS;
  std::string buf;
  std::vector<cfrk_read_fix> fix(nS);
  DeviceBufs bufs(ctx);
  void *d_data = nullptr, *d_start = nullptr, *d_length = nullptr, *d_out = nullptr, *d_fix = nullptr;
  const char *what = "cfrk_device_alloc";
  int rc = 0;
  if (nS && !(rc = bufs.upload(q, &d_data, &d_start, &d_length, &what))) {
    what = "cfrk_device_alloc";
    if (!(rc = bufs.alloc(nN + 16, &d_out)) && !(rc = bufs.alloc(nS * sizeof(cfrk_read_fix), &d_fix))) {
      what = "cfrk_global_correct_reads_device";
      rc = cfrk_global_correct_reads_device(ctx, (const int8_t *)d_data, (const int64_t *)d_start, (const int32_t *)d_length, q.nN, q.nS,
                                            o.correct_min_count, (int8_t *)d_out, (cfrk_read_fix *)d_fix);
    }
    if (!rc && o.correct_report) {
      what = "cfrk_memcpy_d2h";
      rc = cfrk_memcpy_d2h(ctx, fix.data(), d_fix, nS * sizeof(cfrk_read_fix));
    }
  }
  if (!rc)
    rc = emit_selected(ctx, q, d_out, d_start, d_length, nullptr, nullptr, 0, o.correct_names, qtext, text_fmt, o.correct_format, qpath, buf, &what);
  const int rc2 = nS ? cfrk_ctx_sync(ctx) : 0;
  bufs.release();
  if (rc) return die(ctx, rc, what);
  if (rc2) return die(ctx, rc2, "cfrk_ctx_sync");
  if (write_file(out_path, buf)) return 1;
  if (!o.correct_report) return 0;
  char line[32];
  for (size_t i = 0; i < nS; ++i) {
    snprintf(line, sizeof line, "%u\t%u\n", (unsigned)fix[i].fixed, (unsigned)fix[i].left);
    *report += line;
  }
  return 0;
}

}  // namespace

// QFILE to CFILE and, with --query2, QFILE2 to CFILE2; the report lists QFILE's records, then QFILE2's
int write_correct(const Options &o, cfrk_ctx *ctx, const Inputs &in) {
  std::string report;
  const int tf = text_format_of(in.qformat);
  if (const int rc = correct_file(o, ctx, tf, in.qreads, in.qtext, o.query, o.correct_out, &report)) return rc;
  if (o.query2)
    if (const int rc = correct_file(o, ctx, tf, in.qreads2, in.qtext2, o.query2, o.correct_out2, &report)) return rc;
  return o.correct_report ? write_file(o.correct_report, report) : 0;
}

// --paired / --query2: the names of the query file's mates, where its text is held for a names writer
int check_query_pairs(const Options &o, cfrk_ctx *ctx, const Inputs &in) {
  if (!o.mates() || !o.pair_check || !((o.filter_out && o.filter_names) || (o.correct_out && o.correct_names))) return 0;
  return check_mate_names(ctx, o.query2 ? in.qreads.nS : in.qreads.nS / 2, text_format_of(in.qformat), in.qtext, o.query, o.query2 ? &in.qtext2 : nullptr,
                          o.query2);
}

// --normalize-out: the kept reads (d_keep, as the normalise call left it) of the input b untrimmed, to NFILE
int write_normalized(const Options &o, cfrk_ctx *ctx, const Inputs &in, const cfrk_batch &b, const void *d_data, const void *d_start,
                     const void *d_length, const void *d_keep) {
  std::string buf;
  const char *what = "";
  const int rc = emit_selected(ctx, b, d_data, d_start, d_length, nullptr, d_keep, 0, o.normalize_names, in.ntext, text_format_of(in.nformat),
                               o.normalize_format, in.npath, buf, &what);
  if (rc) return die(ctx, rc, what);
  return write_file(o.normalize_out, buf);
}
