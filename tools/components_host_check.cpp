// components_host_check.cpp -- the component table's formatter (cfrk_host_format_components) and the tagger
// (cfrk_host_tag_components) under the sanitizers, on the CPU, outside pytest.  Built and run as tools/weak_host_check.cpp is:
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o components_host_check tools/components_host_check.cpp cfrk_amd/host/cfrk_host.cpp
//   ./components_host_check
//
// Random tables in the native layout -- no row at all, sums up to 2^64 - 1, n_kmers 0, members up to 2^32 - 1, k from 1 to
// 64 -- formatted into buffers of exactly the size the sizing call returned (so that a write past them is seen), from
// arrays of exactly their size, and compared with a restatement through snprintf and std::string.  Prints one summary
// line; exit status 1 on a disagreement.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../cfrk_amd/host/cfrk_host.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}

struct Row { uint64_t kc, n_kmers, n_links; uint32_t first, n_unitigs; };

static uint64_t pick() { return rnd() % 4 == 0 ? rnd() : rnd() % 16 == 0 ? ~0ull : rnd() % 8 == 0 ? 0 : rnd() % 100000; }

int main() {
  static_assert(sizeof(Row) == 32, "the rows are 32 bytes");
  size_t sets = 0, rows = 0, bytes = 0, zero_kmers = 0;
  for (int round = 0; round < 400; ++round) {
    const int64_t n = round == 0 ? 0 : (int64_t)(1 + rnd() % 40);
    const int k = (int)(1 + rnd() % 64);
    Row *table = (Row *)malloc(n ? (size_t)n * sizeof(Row) : 1);              // exactly n rows
    std::string want;
    for (int64_t c = 0; c < n; ++c) {
      Row &r = table[c];
      r.kc = pick(); r.n_kmers = pick(); r.n_links = pick();
      r.first = (uint32_t)pick(); r.n_unitigs = rnd() % 8 == 0 ? ~0u : (uint32_t)(1 + rnd() % 1000);
      zero_kmers += r.n_kmers == 0;
      const uint64_t d = r.n_kmers ? r.n_kmers : 1;
      const unsigned __int128 tenths = ((unsigned __int128)r.kc * 10 + d / 2) / d;
      char line[256];
      snprintf(line, sizeof line, "%lld\t%u\t%u\t%llu\t%llu\t%llu\t%llu.%d\t%llu\n", (long long)c, r.first, r.n_unitigs, (unsigned long long)r.n_kmers,
               (unsigned long long)(r.n_kmers + (uint64_t)r.n_unitigs * (uint64_t)(k - 1)), (unsigned long long)r.kc, (unsigned long long)(tenths / 10),
               (int)(tenths % 10), (unsigned long long)r.n_links);
      want += line;
    }
    const size_t need = cfrk_host_format_components(table, n, k, nullptr, 0);
    if (need != want.size()) { fprintf(stderr, "set %d: sized %zu, expected %zu\n", round, need, want.size()); return 1; }
    char *buf = (char *)malloc(need ? need : 1);                              // exactly the size asked for
    const size_t got = cfrk_host_format_components(table, n, k, buf, need);
    if (got != need || memcmp(buf, want.data(), need) != 0) { fprintf(stderr, "set %d: the text differs\n", round); return 1; }
    free(buf);
    free(table);
    bytes += need;
    ++sets; rows += (size_t)n;
  }
  // the tagger: headers with and without L tags, S lines, a last line without its newline, comp words that say "none",
  // fewer comp words than lines; into buffers of exactly the size asked for
  size_t tagged = 0;
  for (int round = 0; round < 400; ++round) {
    const int gfa = round & 1;
    const int64_t lines = (int64_t)(rnd() % 12), nS = (int64_t)(rnd() % 12);
    uint32_t *comp = (uint32_t *)malloc(nS ? (size_t)nS * 4 : 1);             // exactly nS words
    for (int64_t j = 0; j < nS; ++j) comp[j] = rnd() % 5 == 0 ? ~0u : rnd() % 3 == 0 ? (uint32_t)rnd() : (uint32_t)(rnd() % 50);
    std::string text, want;
    int64_t named = 0;
    for (int64_t i = 0; i < lines; ++i) {
      const bool last = i + 1 == lines && rnd() % 2;                          // no newline behind the last line
      const bool is_named = rnd() % 3 != 0;
      std::string head, tail;
      if (gfa) { head = is_named ? "S\t1\tACGT\tLN:i:4" : (rnd() % 2 ? "L\t0\t+\t1\t-\t3M" : "H\tVN:Z:1.0"); }
      else if (is_named) { head = ">3 LN:i:4 KC:i:7 km:f:1.8"; if (rnd() % 2) head += " CL:i:1"; if (rnd() % 2) tail = " L:+:2:-"; if (rnd() % 4 == 0) tail += " L:-:0:+"; }
      else head = rnd() % 4 ? "ACGTTGCA" : "";
      std::string tag;
      if (is_named) {
        if (named < nS && comp[named] != ~0u) tag = std::string(gfa ? "\t" : " ") + "CC:i:" + std::to_string(comp[named]);
        ++named;
      }
      text += head + tail + (last ? "" : "\n");
      want += head + tag + tail + (last ? "" : "\n");
    }
    char *in = (char *)malloc(text.size() ? text.size() : 1);                 // exactly the text, no terminator
    memcpy(in, text.data(), text.size());
    const size_t need = cfrk_host_tag_components(in, text.size(), gfa, comp, nS, nullptr, 0);
    if (need != want.size()) { fprintf(stderr, "tag set %d: sized %zu, expected %zu\n", round, need, want.size()); return 1; }
    char *buf = (char *)malloc(need ? need : 1);
    const size_t got = cfrk_host_tag_components(in, text.size(), gfa, comp, nS, buf, need);
    if (got != need || memcmp(buf, want.data(), need) != 0) { fprintf(stderr, "tag set %d: the text differs\n", round); return 1; }
    free(buf); free(in); free(comp);
    tagged += need;
  }
  if (!zero_kmers) { fprintf(stderr, "no row with n_kmers 0 occurred\n"); return 1; }
  printf("components_host_check: %zu sets, %zu rows (%zu with n_kmers 0), %zu bytes; 400 tagged texts, %zu bytes; formatter and restatement agree\n",
         sets, rows, zero_kmers, bytes, tagged);
  return 0;
}
