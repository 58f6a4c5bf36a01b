// weak_host_check.cpp -- the weak report's formatter (cfrk_host_format_weak) under the sanitizers, on the CPU, outside
// pytest.  Built and run as tools/bubbles_host_check.cpp is:
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o weak_host_check tools/weak_host_check.cpp cfrk_amd/host/cfrk_host.cpp
//   ./weak_host_check
//
// Random unitig sets in the native layout -- unitigs of one base, invalid codes, n_kmers 0, summed counts up to 2^64 - 1 --
// with random weak bytes: 0, connection, isolated and bytes that are neither.  Everything is formatted into buffers of
// exactly the size the sizing call returned (so that a write past them is seen), from arrays of exactly their size, and
// compared with a restatement through snprintf and std::string.  Prints one summary line; exit status 1 on a disagreement.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../cfrk_amd/host/cfrk_host.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
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
  size_t sets = 0, unitigs = 0, lines = 0, bytes = 0, kinds[3] = {0, 0, 0};   // connection, isolated, another byte
  for (int round = 0; round < 400; ++round) {
    const int64_t nS = round == 0 ? 0 : (int64_t)(1 + rnd() % 40);
    std::vector<int32_t> length((size_t)nS);
    std::vector<int64_t> start((size_t)nS);
    Rec *rec = (Rec *)malloc(nS ? (size_t)nS * sizeof(Rec) : 1);              // exactly nS rows
    uint8_t *weak = (uint8_t *)malloc(nS ? (size_t)nS : 1);                   // exactly nS bytes
    int64_t nN = 0;
    for (int64_t j = 0; j < nS; ++j) {
      length[(size_t)j] = (rnd() % 7 == 0) ? 1 : (int32_t)(1 + rnd() % 120);
      start[(size_t)j] = nN;
      nN += length[(size_t)j] + 1;
      Rec &r = rec[j];
      r.n_kmers = (rnd() % 9 == 0) ? 0 : (rnd() % 4 == 0) ? (uint32_t)rnd() | 1u : (uint32_t)(1 + rnd() % 1000);
      r.kc = (rnd() % 3 == 0) ? rnd() : (rnd() % 16 == 0) ? ~0ull : rnd() % 100000;
      r.flags = (uint32_t)(rnd() % 2);
      const uint64_t how = rnd() % 8;
      weak[j] = (uint8_t)(how < 3 ? 0 : how < 5 ? 1 : how < 7 ? 2 : 3 + rnd() % 253);
    }
    int8_t *data = (int8_t *)malloc(nN ? (size_t)nN : 1);                     // exactly nN bytes: no slack behind the unitigs
    for (int64_t x = 0; x < nN; ++x) data[x] = (rnd() % 50 == 0) ? (int8_t)(rnd() % 256) : (int8_t)(rnd() % 4);
    for (int64_t j = 0; j < nS; ++j) data[start[(size_t)j] + length[(size_t)j]] = -1;

    const uint32_t no = (uint32_t)(rnd() % 3 == 0 ? rnd() : 1 + rnd() % 8);
    std::string want;
    for (int64_t j = 0; j < nS; ++j) {
      if (weak[j] != 1 && weak[j] != 2) { kinds[2] += weak[j] != 0; continue; }
      ++kinds[weak[j] - 1];
      std::string seq;
      for (int32_t x = 0; x < length[(size_t)j]; ++x) {
        const int c = data[start[(size_t)j] + x];
        seq += (c >= 0 && c <= 3) ? "ACGT"[c] : 'N';
      }
      char head[256];
      snprintf(head, sizeof head, "%u\t%lld\t%s\t%zu\t%llu\t%s\t", (unsigned)no, (long long)j, weak[j] == 1 ? "connection" : "isolated", seq.size(),
               (unsigned long long)rec[j].kc, mean(rec[j]).c_str());
      want += head + seq + "\n";
      ++lines;
    }

    const size_t need = cfrk_host_format_weak(no, data, start.data(), length.data(), rec, nS, weak, nullptr, 0);
    if (need != want.size()) { fprintf(stderr, "set %d: sized %zu, expected %zu\n", round, need, want.size()); return 1; }
    char *buf = (char *)malloc(need ? need : 1);                              // exactly the size asked for
    const size_t got = cfrk_host_format_weak(no, data, start.data(), length.data(), rec, nS, weak, buf, need);
    if (got != need || memcmp(buf, want.data(), need) != 0) { fprintf(stderr, "set %d: the text differs\n", round); return 1; }
    free(buf);
    free(data);
    free(weak);
    free(rec);
    bytes += need;
    ++sets; unitigs += (size_t)nS;
  }
  if (!kinds[0] || !kinds[1] || !kinds[2]) { fprintf(stderr, "a kind never occurred: %zu connection, %zu isolated, %zu other\n", kinds[0], kinds[1], kinds[2]); return 1; }
  printf("weak_host_check: %zu sets, %zu unitigs, %zu lines (%zu connection, %zu isolated, %zu other bytes), %zu bytes; formatter and restatement agree\n",
         sets, unitigs, lines, kinds[0], kinds[1], kinds[2], bytes);
  return 0;
}
