// bubbles_host_check.cpp -- the bubble report's formatter (cfrk_host_format_bubbles) under the sanitizers, on the CPU,
// outside pytest.  Built and run as tools/unitig_links_host_check.cpp is:
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o bubbles_host_check tools/bubbles_host_check.cpp cfrk_amd/host/cfrk_host.cpp
//   ./bubbles_host_check
//
// Random unitig sets in the native layout -- unitigs of one base, invalid codes, n_kmers 0, summed counts up to 2^64 - 1 --
// with random pop bytes and partners: both strands, a unitig as its own partner, pairs of equal length that differ in
// 0, 1 or more bases, partners that name no unitig, NONE.  Everything is formatted into buffers of exactly the size the
// sizing call returned (so that a write past them is seen), from arrays of exactly their size, and compared with a
// restatement through snprintf and std::string.  Prints one summary line; exit status 1 on a disagreement.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../cfrk_amd/host/cfrk_host.h"

static uint64_t rng_state = 0xA0761D6478BD642Full;
static uint64_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}

struct Rec { uint64_t kc; uint32_t n_kmers, flags; };

static std::string mean(const Rec &r) {
  const uint32_t n = r.n_kmers ? r.n_kmers : 1;
  const unsigned __int128 tenths = ((unsigned __int128)r.kc * 10 + n / 2) / n;
  char s[64];
  snprintf(s, sizeof s, "%llu.%d", (unsigned long long)(tenths / 10), (int)(tenths % 10));
  return s;
}

int main() {
  static_assert(sizeof(Rec) == 16, "the rows are 16 bytes");
  size_t sets = 0, unitigs = 0, lines = 0, bytes = 0, kinds[3] = {0, 0, 0};
  for (int round = 0; round < 400; ++round) {
    const int64_t nS = round == 0 ? 0 : (int64_t)(1 + rnd() % 40);
    std::vector<int32_t> length((size_t)nS);
    std::vector<int64_t> start((size_t)nS);
    Rec *rec = (Rec *)malloc(nS ? (size_t)nS * sizeof(Rec) : 1);              // exactly nS rows
    uint8_t *pop = (uint8_t *)malloc(nS ? (size_t)nS : 1);                    // exactly nS bytes
    uint32_t *partner = (uint32_t *)malloc(nS ? (size_t)nS * 4 : 1);          // exactly nS words
    int64_t nN = 0;
    for (int64_t j = 0; j < nS; ++j) {
      // every other unitig as long as its predecessor, so that pairs of equal length are common
      length[(size_t)j] = (j % 2 && rnd() % 4) ? length[(size_t)j - 1] : (rnd() % 7 == 0) ? 1 : (int32_t)(1 + rnd() % 120);
      start[(size_t)j] = nN;
      nN += length[(size_t)j] + 1;
      Rec &r = rec[j];
      r.n_kmers = (rnd() % 9 == 0) ? 0 : (rnd() % 4 == 0) ? (uint32_t)rnd() | 1u : (uint32_t)(1 + rnd() % 1000);
      r.kc = (rnd() % 3 == 0) ? rnd() : rnd() % 100000;
      r.flags = (uint32_t)(rnd() % 2);
    }
    int8_t *data = (int8_t *)malloc(nN ? (size_t)nN : 1);                     // exactly nN bytes: no slack behind the unitigs
    for (int64_t x = 0; x < nN; ++x) data[x] = (rnd() % 50 == 0) ? (int8_t)(rnd() % 256) : (int8_t)(rnd() % 4);
    for (int64_t j = 1; j < nS; j += 2) {
      if (length[(size_t)j] != length[(size_t)j - 1]) continue;
      // the pair of equal length: a copy, or its reverse complement, with 0, 1 or 2 bases changed
      const int32_t L = length[(size_t)j];
      const bool minus = rnd() % 2;
      for (int32_t x = 0; x < L; ++x) {
        const int c = data[start[(size_t)j - 1] + (minus ? L - 1 - x : x)];
        data[start[(size_t)j] + x] = (int8_t)((minus && c >= 0 && c <= 3) ? 3 - c : c);
      }
      for (uint64_t e = rnd() % 3; e > 0; --e) {
        int8_t &c = data[start[(size_t)j] + (int64_t)(rnd() % (uint64_t)L)];
        c = (int8_t)((c + 1) & 3);
      }
    }
    for (int64_t j = 0; j < nS; ++j) data[start[(size_t)j] + length[(size_t)j]] = -1;
    for (int64_t j = 0; j < nS; ++j) {
      pop[j] = (uint8_t)(rnd() % 3 == 0 ? 0 : rnd() % 2 ? 1 : rnd());
      const uint64_t how = rnd() % 8;
      const uint32_t s = how == 0 ? 0x7FFFFFFFu : how == 1 ? (uint32_t)nS : how < 5 ? (uint32_t)(j ^ 1) : (uint32_t)(rnd() % (uint64_t)nS);
      partner[j] = how == 2 ? 0xFFFFFFFFu : (s << 1) | (uint32_t)(rnd() % 2);
    }

    const uint32_t no = (uint32_t)(rnd() % 3 == 0 ? rnd() : 1 + rnd() % 8);
    std::string want;
    auto text = [&](int64_t j, bool minus) {
      std::string seq;
      for (int32_t x = 0; x < length[(size_t)j]; ++x) {
        const int c = data[start[(size_t)j] + (minus ? length[(size_t)j] - 1 - x : x)];
        seq += (c >= 0 && c <= 3) ? "ACGT"[minus ? 3 - c : c] : 'N';
      }
      return seq;
    };
    for (int64_t j = 0; j < nS; ++j) {
      const int64_t s = (int64_t)(partner[j] >> 1);
      if (!pop[j] || s >= nS) continue;
      const bool minus = partner[j] & 1u;
      const std::string a = text(j, false), b = text(s, minus);
      int kind = 2;
      if (a.size() == b.size()) {
        size_t differ = 0;
        for (size_t x = 0; x < a.size(); ++x) differ += a[x] != b[x];
        kind = differ == 1 ? 0 : 1;
      }
      ++kinds[kind];
      char head[256];
      snprintf(head, sizeof head, "%u\t%lld\t%lld\t%c\t%zu\t%zu\t%s\t%s\t%s\t", (unsigned)no, (long long)j, (long long)s, minus ? '-' : '+', a.size(),
               b.size(), mean(rec[j]).c_str(), mean(rec[s]).c_str(), kind == 0 ? "snp" : kind == 1 ? "mnp" : "indel");
      want += head + a + "\t" + b + "\n";
      ++lines;
    }

    const size_t need = cfrk_host_format_bubbles(no, data, start.data(), length.data(), rec, nS, pop, partner, nullptr, 0);
    if (need != want.size()) { fprintf(stderr, "set %d: sized %zu, expected %zu\n", round, need, want.size()); return 1; }
    char *buf = (char *)malloc(need ? need : 1);                              // exactly the size asked for
    const size_t got = cfrk_host_format_bubbles(no, data, start.data(), length.data(), rec, nS, pop, partner, buf, need);
    if (got != need || memcmp(buf, want.data(), need) != 0) { fprintf(stderr, "set %d: the text differs\n", round); return 1; }
    free(buf);
    free(data);
    free(partner);
    free(pop);
    free(rec);
    bytes += need;
    ++sets; unitigs += (size_t)nS;
  }
  if (!kinds[0] || !kinds[1] || !kinds[2]) { fprintf(stderr, "a kind never occurred: %zu snp, %zu mnp, %zu indel\n", kinds[0], kinds[1], kinds[2]); return 1; }
  printf("bubbles_host_check: %zu sets, %zu unitigs, %zu lines (%zu snp, %zu mnp, %zu indel), %zu bytes; formatter and restatement agree\n",
         sets, unitigs, lines, kinds[0], kinds[1], kinds[2], bytes);
  return 0;
}
