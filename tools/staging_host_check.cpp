// staging_host_check.cpp -- the host-only half of cfrk_amd/csrc/staging.h (the threaded struct-read layout check and the
// carve of a pool slot) under the sanitizers, on the CPU, outside pytest.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o staging_host_check tools/staging_host_check.cpp && ./staging_host_check
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=thread -o staging_host_check_tsan tools/staging_host_check.cpp && ./staging_host_check_tsan
//
// Layout: tables in arrays of exactly their size (so that a read outside them is seen) go through LayoutCheck and through
// a single-threaded restatement; cause, read index and message text must agree.  Carve: for every call site's part list
// the offsets are multiples of 256, the parts do not overlap and the total is the expression the host forms passed to
// cfrk_pool_get before the helper existed.  Prints one summary line; exit status 1 on a disagreement.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../cfrk_amd/csrc/staging.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}

// one read after the other, in 128-bit arithmetic: the first read that is not where its predecessor puts it, runs past
// nN or is followed by a base; then the table's end against nN
static std::string restate(const int8_t *data, const int64_t *start, const int32_t *length, int64_t nN, int64_t nS, int *why, int64_t *read) {
  char buf[160];
  for (int64_t i = 0; i < nS; ++i) {
    const __int128 s = start[i], l = length[i];
    const bool prev_sane = i == 0 || (start[i - 1] >= 0 && start[i - 1] <= nN && length[i - 1] >= 0);
    const __int128 want = i ? (__int128)start[i - 1] + length[i - 1] + 1 : 0;
    *read = i;
    if (s < 0 || s > nN || l < 0 || !prev_sane || s != want) {
      *why = LAYOUT_START;
      snprintf(buf, sizeof buf, "read %lld: start %lld, expected %lld", (long long)i, (long long)start[i], (long long)(int64_t)(uint64_t)want);
      return buf;
    }
    if (s + l + 1 > nN) { *why = LAYOUT_PAST; snprintf(buf, sizeof buf, "read %lld runs past nN", (long long)i); return buf; }
    const int8_t term = data[(int64_t)(s + l)];
    if (term >= 0 && term <= 3) { *why = LAYOUT_NO_TERM; snprintf(buf, sizeof buf, "read %lld has no terminator", (long long)i); return buf; }
  }
  const __int128 pos = nS ? (__int128)start[nS - 1] + length[nS - 1] + 1 : 0;
  *read = nS;
  if (pos != nN) { *why = LAYOUT_SUM; snprintf(buf, sizeof buf, "sum(length)+nS = %lld but nN = %lld", (long long)pos, (long long)nN); return buf; }
  *why = LAYOUT_OK;
  return "";
}

struct Table {
  int64_t nN = 0, nS = 0;
  int8_t *data; int64_t *start; int32_t *length;
  // valid layout of the given lengths; the arrays hold exactly nN / nS elements
  explicit Table(const std::vector<int32_t> &len) {
    nS = (int64_t)len.size();
    for (int32_t l : len) nN += l + 1;
    data = new int8_t[(size_t)nN]; start = new int64_t[(size_t)nS]; length = new int32_t[(size_t)nS];
    int64_t pos = 0;
    for (int64_t i = 0; i < nS; ++i) {
      start[i] = pos; length[i] = len[(size_t)i];
      for (int32_t x = 0; x < length[i]; ++x) data[pos + x] = (int8_t)(rnd() % 4);
      data[pos + length[i]] = -1;
      pos += length[i] + 1;
    }
  }
  ~Table() { delete[] data; delete[] start; delete[] length; }
};

static size_t n_tables = 0, n_refused = 0;

static bool same(const Table &t, int64_t nN, const char *what, int expect_why) {
  int why = 0; int64_t read = 0;
  const std::string want = restate(t.data, t.start, t.length, nN, t.nS, &why, &read);
  LayoutCheck lc;
  lc.begin(t.data, t.start, t.length, nN, t.nS);
  const LayoutVerdict v = lc.verdict();
  char msg[160];
  layout_message(v, msg, sizeof msg);
  ++n_tables; n_refused += v.why != LAYOUT_OK;
  if (v.why != why || (why != LAYOUT_OK && v.read != read) || want != msg || (expect_why >= 0 && why != expect_why)) {
    fprintf(stderr, "%s: check says %d at read %lld \"%s\", restatement %d at read %lld \"%s\" (expected cause %d)\n", what, v.why, (long long)v.read,
            msg, why, (long long)read, want.c_str(), expect_why);
    return false;
  }
  return true;
}

static bool layout_cases() {
  bool ok = true;
  for (int round = 0; round < 300; ++round) {
    std::vector<int32_t> len((size_t)(1 + rnd() % 50));
    for (auto &l : len) l = (rnd() % 4 == 0) ? 0 : (int32_t)(rnd() % 200);
    const size_t j = (size_t)(rnd() % len.size());
    Table t(len);
    ok &= same(t, t.nN, "valid table", LAYOUT_OK);
    { Table b(len); b.start[j] += 1; ok &= same(b, b.nN, "one start off by one", LAYOUT_START); }
    { Table b(len); b.start[0] = 1; ok &= same(b, b.nN, "start[0] != 0", LAYOUT_START); }
    { Table b(len); b.data[b.start[j] + b.length[j]] = 2; ok &= same(b, b.nN, "missing terminator", LAYOUT_NO_TERM); }
    { Table b(len); b.length[len.size() - 1] += 1; ok &= same(b, b.nN, "read running past nN", LAYOUT_PAST); }
    { Table b(len); b.length[j] = -1 - (int32_t)(rnd() % 1000); ok &= same(b, b.nN, "negative length", LAYOUT_START); }
    { Table b(len); b.start[j] = b.nN + 1 + (int64_t)(rnd() % 1000); ok &= same(b, b.nN, "start above nN", LAYOUT_START); }
    { Table b(len); b.start[j] = INT64_MAX; ok &= same(b, b.nN, "start at INT64_MAX", LAYOUT_START); }
    { Table b(len); b.start[j] = INT64_MIN; ok &= same(b, b.nN, "start at INT64_MIN", LAYOUT_START); }
    ok &= same(t, t.nN + 1 + (int64_t)(rnd() % 9), "a sum that does not reach nN", LAYOUT_SUM);
  }
  { Table t(std::vector<int32_t>(7, 0)); ok &= same(t, t.nN, "empty reads only", LAYOUT_OK); }
  { Table t(std::vector<int32_t>{}); ok &= same(t, 0, "nS = 0, nN = 0", LAYOUT_OK); }
  { Table t(std::vector<int32_t>{}); int8_t *d = new int8_t[5](); std::swap(t.data, d); ok &= same(t, 5, "nS = 0, nN > 0", LAYOUT_SUM); std::swap(t.data, d); delete[] d; }
  // several pieces: the table of tests/test_gpu_parity.py (a piece's first read consistent with a negative predecessor)
  const int64_t nS = (1 << 20) + 4096, cut = nS / 2;
  const std::vector<int32_t> len((size_t)nS, 3);
  { Table t(len); ok &= same(t, t.nN, "2^20 + 4096 reads", LAYOUT_OK); }
  { Table t(len); for (int64_t i = cut - 1; i < nS; ++i) t.start[i] -= (int64_t)1 << 40; ok &= same(t, t.nN, "starts shifted by -2^40", LAYOUT_START); }
  { Table t(len); t.length[cut] = -7; ok &= same(t, t.nN, "length -7 at a piece boundary", LAYOUT_START); }
  { Table t(len); for (int64_t i = cut - 1; i < nS; ++i) t.start[i] -= (int64_t)1 << 40; t.length[cut] = -7;
    ok &= same(t, t.nN, "starts shifted by -2^40 and length -7 at the boundary", LAYOUT_START); }
  { Table t(len); t.length[cut - 1] = -7; ok &= same(t, t.nN, "length -7 before a piece boundary", LAYOUT_START); }
  { Table t(len); t.data[t.start[nS - 1] + 3] = 0; ok &= same(t, t.nN, "last read of the last piece without terminator", LAYOUT_NO_TERM); }
  return ok;
}

static size_t up(size_t b) { return (b + 255) & ~(size_t)255; }
static size_t n_carves = 0;

// offsets on 256-byte boundaries, parts in order without overlap, the total as restated
static bool carve_ok(const char *what, const std::vector<size_t> &off, const std::vector<size_t> &bytes, size_t total, size_t want_total) {
  bool ok = total == want_total && off[0] == 0;
  for (size_t j = 0; j < off.size(); ++j) {
    ok &= off[j] % 256 == 0 && off[j] + bytes[j] <= total;
    if (j) ok &= off[j] >= off[j - 1] + bytes[j - 1];
  }
  ++n_carves;
  if (!ok) fprintf(stderr, "carve %s: total %zu, expected %zu\n", what, total, want_total);
  return ok;
}

static bool carve_cases() {
  const uint64_t sizes[] = {0, 1, 255, 256, 257, ((uint64_t)1 << 32) + 12345};
  bool ok = true;
  for (uint64_t nN : sizes)
    for (uint64_t nS : sizes) {
      const size_t n = (size_t)nN, s = (size_t)nS;
      // cfrk_global_add, cfrk_global_query_reads, cfrk_distinct_sketch: the data alone
      { SlotCarve c(n + 64, nS, false, nullptr, 0); ok &= carve_ok("data", {0}, {n + 64}, c.total, n + 64); }
      // cfrk_global_read_stats, cfrk_global_read_spans
      { SlotCarve c(n + 64, nS, true, nullptr, 0);
        ok &= carve_ok("reads", {0, c.o_start, c.o_length}, {n + 64, s * 8, s * 4}, c.total, up(n + 64) + up(s * 8) + s * 4); }
      // cfrk_reads_select, in: spans and keep flags, each present or not
      for (int m = 0; m < 4; ++m) {
        const size_t x[2] = {(m & 1) ? s * 8 : 0, (m & 2) ? s : 0};
        SlotCarve c(n + 64, nS, true, x, 2);
        ok &= carve_ok("select in", {0, c.o_start, c.o_length, c.o_extra[0], c.o_extra[1]}, {n + 64, s * 8, s * 4, x[0], x[1]}, c.total,
                       up(n + 64) + up(s * 8) + up(s * 4) + up(x[0]) + x[1]);
      }
      // cfrk_per_read_sparse, in: room for row_ptr
      { const size_t x = (s + 1) * 8; SlotCarve c(n + 64, nS, true, &x, 1);
        ok &= carve_ok("sparse in", {0, c.o_start, c.o_length, c.o_extra[0]}, {n + 64, s * 8, s * 4, x}, c.total, up(n + 64) + up(s * 8) + up(s * 4) + x); }
      // cfrk_reads_select, out: the index behind the reads
      { const size_t x = s * 8; SlotCarve c(n + 16, nS, true, &x, 1);
        ok &= carve_ok("select out", {0, c.o_start, c.o_length, c.o_extra[0]}, {n + 16, s * 8, s * 4, x}, c.total, up(n + 16) + up(s * 8) + up(s * 4) + x); }
      // cfrk_fasta_parse, cfrk_fastq_parse, out
      { SlotCarve c(n + 16, nS, true, nullptr, 0);
        ok &= carve_ok("parse out", {0, c.o_start, c.o_length}, {n + 16, s * 8, s * 4}, c.total, up(n + 16) + up(s * 8) + s * 4); }
      // cfrk_per_read_sparse, out: keys and counts of nnz entries
      { Carve c; const size_t o_keys = c.part(n * 8), o_cnt = c.part(n * 4);
        ok &= carve_ok("sparse out", {o_keys, o_cnt}, {n * 8, n * 4}, c.end, up(n * 8) + n * 4); }
    }
  return ok;
}

int main() {
  const bool layout = layout_cases(), carve = carve_cases();
  printf("staging_host_check: %zu tables (%zu refused), %zu carves; layout check and restatement %s, carve totals %s\n", n_tables, n_refused,
         n_carves, layout ? "agree" : "DISAGREE", carve ? "agree" : "DISAGREE");
  return layout && carve ? 0 : 1;
}
