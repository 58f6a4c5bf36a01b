// unitigs_host_check.cpp -- the FASTA formatter of the unitigs (cfrk_host_format_unitigs) under the sanitizers, on the
// CPU, outside pytest.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o unitigs_host_check tools/unitigs_host_check.cpp cfrk_amd/host/cfrk_host.cpp
//   ./unitigs_host_check
//
// Random unitig sets in the native layout (k-mer counts from 1 to 2^32 - 1, summed counts up to 2^64 - 1, circular
// flags, invalid codes) are formatted into a buffer of exactly the size the sizing call returned (so that a write past
// it is seen), from arrays of exactly their size, and compared with a restatement that prints the mean through
// unsigned __int128 and snprintf.  Prints one summary line; exit status 1 on a disagreement.
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

int main() {
  static_assert(sizeof(Rec) == 16, "the rows are 16 bytes");
  size_t sets = 0, unitigs = 0, bytes = 0;
  for (int round = 0; round < 300; ++round) {
    const int64_t nS = (int64_t)(rnd() % 40);
    std::vector<int32_t> length((size_t)nS);
    std::vector<int64_t> start((size_t)nS);
    Rec *rec = (Rec *)malloc(nS ? (size_t)nS * sizeof(Rec) : 1);      // exactly nS rows
    int64_t nN = 0;
    for (int64_t j = 0; j < nS; ++j) {
      length[(size_t)j] = (rnd() % 7 == 0) ? 1 : (int32_t)(1 + rnd() % 300);
      start[(size_t)j] = nN;
      nN += length[(size_t)j] + 1;
      Rec &r = rec[j];
      r.n_kmers = (rnd() % 4 == 0) ? (uint32_t)rnd() | 1u : (uint32_t)(1 + rnd() % 1000);
      const int kind = (int)(rnd() % 4);
      r.kc = kind == 0 ? rnd() : kind == 1 ? ~0ull - rnd() % 3 : kind == 2 ? (uint64_t)r.n_kmers * (rnd() % 50) + r.n_kmers / 2 : rnd() % 100000;
      r.flags = (uint32_t)(rnd() % 2);
    }
    int8_t *data = (int8_t *)malloc(nN ? (size_t)nN : 1);            // exactly nN bytes: no slack behind the unitigs
    for (int64_t x = 0; x < nN; ++x) data[x] = (rnd() % 50 == 0) ? (int8_t)(rnd() % 256) : (int8_t)(rnd() % 4);
    for (int64_t j = 0; j < nS; ++j) data[start[(size_t)j] + length[(size_t)j]] = -1;
    std::string want;
    for (int64_t j = 0; j < nS; ++j) {
      const Rec &r = rec[j];
      const unsigned __int128 tenths = ((unsigned __int128)r.kc * 10 + r.n_kmers / 2) / r.n_kmers;
      char head[160];
      snprintf(head, sizeof head, ">%lld LN:i:%d KC:i:%llu km:f:%llu.%d%s\n", (long long)j, (int)length[(size_t)j],
               (unsigned long long)r.kc, (unsigned long long)(tenths / 10), (int)(tenths % 10), (r.flags & 1) ? " CL:i:1" : "");
      want += head;
      for (int32_t x = 0; x < length[(size_t)j]; ++x) {
        const int c = data[start[(size_t)j] + x];
        want += (c >= 0 && c <= 3) ? "ACGT"[c] : 'N';
      }
      want += "\n";
    }
    const size_t need = cfrk_host_format_unitigs(data, start.data(), length.data(), rec, nS, nullptr, 0);
    if (need != want.size()) { fprintf(stderr, "set %d: sized %zu, expected %zu\n", round, need, want.size()); return 1; }
    char *buf = (char *)malloc(need ? need : 1);                     // exactly the size asked for
    const size_t got = cfrk_host_format_unitigs(data, start.data(), length.data(), rec, nS, buf, need);
    if (got != need || memcmp(buf, want.data(), need) != 0) { fprintf(stderr, "set %d: text differs\n", round); return 1; }
    free(buf);
    free(data);
    free(rec);
    ++sets; unitigs += (size_t)nS; bytes += need;
  }
  printf("unitigs_host_check: %zu sets, %zu unitigs, %zu bytes of FASTA; formatter and restatement agree\n", sets, unitigs, bytes);
  return 0;
}
