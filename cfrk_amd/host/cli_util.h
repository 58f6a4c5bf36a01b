// cli_util.h -- what the units of the `cfrk` command share: error reporting, whole-file I/O, the two call idioms of the
// library (size then fill; sizes only, then arrays), an owner of device allocations, the query / map / normalise inputs,
// and the writers' entry points (cli_graph.cpp, cli_query.cpp).  Internal to the command.
#pragma once
#include <stdio.h>

#include <string>
#include <vector>

#include "../../include/cfrk_abi.h"
#include "cfrk_host.h"
#include "cli_options.h"

inline int die(cfrk_ctx *ctx, int rc, const char *what) {
  fprintf(stderr, "cfrk: %s: %s (%s)\n", what, cfrk_strerror(rc), ctx ? cfrk_last_error(ctx) : "");
  return 2;
}

// 0, or 1 (the error reported)
inline int write_file(const char *path, const std::string &buf) {
  FILE *f = fopen(path, "wb");
  if (!f) { fprintf(stderr, "cfrk: cannot write %s\n", path); return 1; }
  const bool ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
  if (fclose(f) != 0 || !ok) { fprintf(stderr, "cfrk: cannot write %s\n", path); return 1; }
  return 0;
}
inline int read_file(const char *path, std::vector<char> &buf) {
  FILE *f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cfrk: cannot read %s\n", path); return 1; }
  char tmp[1 << 16];
  size_t got;
  while ((got = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
  fclose(f);
  return 0;
}

// the formatters' call pair, fmt(buffer, room) -> bytes: sized with (NULL, 0), then filled; appended to buf
template <class F> void format_into(std::string &buf, F fmt) {
  const size_t at = buf.size();
  buf.resize(at + fmt((char *)nullptr, (size_t)0));
  fmt(&buf[at], buf.size() - at);
}

// the library's sizes-only call, then the call proper: call() is made with the arrays as they are (empty: CFRK_ERR_SMALL_BUF
// means "now the sizes are known"), grow() gives them those sizes, and call() is made again.  The last call's code
template <class Call, class Grow> int sized_call(Call call, Grow grow) {
  int rc = call();
  if (rc && rc != CFRK_ERR_SMALL_BUF) return rc;
  grow();
  return rc ? call() : 0;
}

// device allocations of one context, freed together: by release() where the caller has just synchronised, at the latest
// when the owner goes
struct DeviceBufs {
  cfrk_ctx *ctx;
  std::vector<void *> held;
  explicit DeviceBufs(cfrk_ctx *c) : ctx(c) {}
  DeviceBufs(const DeviceBufs &) = delete;
  DeviceBufs &operator=(const DeviceBufs &) = delete;
  ~DeviceBufs() { release(); }
  void release() { for (void *d : held) cfrk_device_free(ctx, d); held.clear(); }
  int alloc(size_t bytes, void **d) {
    const int rc = cfrk_device_alloc(ctx, bytes, d);
    if (!rc && *d) held.push_back(*d);
    return rc;
  }
  // a batch's reads on the device: data (16 spare bytes behind it), start and length, allocated and copied; *what names the call
  int upload(const cfrk_batch &b, void **data, void **start, void **length, const char **what) {
    const size_t nN = (size_t)b.nN, nS = (size_t)b.nS;
    int rc;
    *what = "cfrk_device_alloc";
    if ((rc = alloc(nN + 16, data)) || (rc = alloc(nS * 8, start)) || (rc = alloc(nS * 4, length))) return rc;
    *what = "cfrk_memcpy_h2d";
    if ((rc = cfrk_memcpy_h2d(ctx, *data, b.data, nN)) || (rc = cfrk_memcpy_h2d(ctx, *start, b.start, nS * 8))) return rc;
    return cfrk_memcpy_h2d(ctx, *length, b.length, nS * 4);
  }
};

inline int text_format_of(int file_format) { return file_format == CFRK_FORMAT_FASTQ ? CFRK_TEXT_FASTQ : CFRK_TEXT_FASTA; }

// what main reads before the input is counted, and what the writers take from it
struct Inputs {
  cfrk_batch qreads{};                  // --query: QFILE's reads (parsed once, clean parse)
  int qformat = CFRK_FORMAT_FASTA;      // what QFILE was read as
  std::vector<char> qtext;              // --filter-names / --correct-names: QFILE's bytes
  cfrk_batch qreads2{};                 // --query2: QFILE2's reads and bytes (the format is QFILE's)
  std::vector<char> qtext2;
  cfrk_batch mreads{};                  // --unitigs-map: QFILE's reads
  std::vector<char> ntext;              // --normalize-names: the input file's bytes
  int nformat = CFRK_FORMAT_FASTA;      // --normalize-out: the input's format and path
  const char *npath = "";
  Inputs() = default;
  Inputs(const Inputs &) = delete;
  Inputs &operator=(const Inputs &) = delete;
  ~Inputs() { for (cfrk_batch *b : {&qreads, &qreads2, &mreads}) if (b->data) cfrk_host_free_batch(b); }
};

// --paired: an interleaved file holds whole pairs; 1 (the error reported) when it does not
inline int odd_records(const char *path, int64_t nS) {
  if (!(nS & 1)) return 0;
  fprintf(stderr, "cfrk: --paired: %s holds %lld records, an odd number: the last read has no mate\n", path, (long long)nS);
  return 1;
}

// cli_graph.cpp: each 0, or the exit status (the error reported)
int simplify_unitigs(const Options &o, cfrk_ctx *ctx);
int drop_small_components(const Options &o, cfrk_ctx *ctx);
int write_unitigs(const Options &o, cfrk_ctx *ctx);
int write_unitigs_map(const Options &o, cfrk_ctx *ctx, const cfrk_batch &q);

// cli_query.cpp: each 0, or the exit status (the error reported)
int query_answers(cfrk_ctx *ctx, const cfrk_batch &q, std::vector<uint32_t> &ans);
int write_query(const Options &o, const cfrk_batch &q, int k, const uint32_t *ans);
int write_query_stats(const Options &o, cfrk_ctx *ctx, const cfrk_batch &q);
int check_mate_names(cfrk_ctx *ctx, int64_t n_pairs, int text_format, const std::vector<char> &text_a, const char *path_a,
                     const std::vector<char> *text_b, const char *path_b);
int check_query_pairs(const Options &o, cfrk_ctx *ctx, const Inputs &in);
int write_filter(const Options &o, cfrk_ctx *ctx, const Inputs &in, int k);
int write_correct(const Options &o, cfrk_ctx *ctx, const Inputs &in);
int write_normalized(const Options &o, cfrk_ctx *ctx, const Inputs &in, const cfrk_batch &b, const void *d_data, const void *d_start,
                     const void *d_length, const void *d_keep);
