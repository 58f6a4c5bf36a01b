// filter_host_check.cpp -- the FASTA formatter of the selected reads (cfrk_host_format_fasta) under the sanitizers, on
// the CPU, outside pytest.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o filter_host_check tools/filter_host_check.cpp cfrk_amd/host/cfrk_host.cpp
//   ./filter_host_check
//
// Random read sets in the native layout (empty reads, invalid codes, indices above 2^32) are formatted into a buffer of
// exactly the size the sizing call returned (so that a write past it is seen), from arrays of exactly their size, and
// compared with a byte-by-byte restatement.  Prints one summary line; exit status 1 on a disagreement.
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

int main() {
  size_t sets = 0, reads = 0, bytes = 0;
  for (int round = 0; round < 200; ++round) {
    const int64_t nS = (int64_t)(rnd() % 40);
    std::vector<int32_t> length((size_t)nS);
    std::vector<int64_t> start((size_t)nS), index((size_t)nS);
    int64_t nN = 0;
    for (int64_t j = 0; j < nS; ++j) {
      length[(size_t)j] = (rnd() % 5 == 0) ? 0 : (int32_t)(rnd() % 300);
      start[(size_t)j] = nN;
      nN += length[(size_t)j] + 1;
      index[(size_t)j] = (rnd() % 3 == 0) ? (int64_t)((1ull << 32) + rnd() % (1ull << 40)) : (int64_t)(rnd() % 1000);
    }
    int8_t *data = (int8_t *)malloc(nN ? (size_t)nN : 1);     // exactly nN bytes: no slack behind the reads
    for (int64_t x = 0; x < nN; ++x) data[x] = (rnd() % 20 == 0) ? (int8_t)(rnd() % 256) : (int8_t)(rnd() % 4);
    for (int64_t j = 0; j < nS; ++j) data[start[(size_t)j] + length[(size_t)j]] = -1;
    const bool with_index = round % 4 != 0;
    std::string want;
    for (int64_t j = 0; j < nS; ++j) {
      want += ">" + std::to_string((unsigned long long)(with_index ? index[(size_t)j] : j)) + "\n";
      for (int32_t x = 0; x < length[(size_t)j]; ++x) {
        const int c = data[start[(size_t)j] + x];
        want += (c >= 0 && c <= 3) ? "ACGT"[c] : 'N';
      }
      want += "\n";
    }
    const int64_t *ip = with_index ? index.data() : nullptr;
    const size_t need = cfrk_host_format_fasta(data, start.data(), length.data(), ip, nS, nullptr, 0);
    if (need != want.size()) { fprintf(stderr, "set %d: sized %zu, expected %zu\n", round, need, want.size()); return 1; }
    char *buf = (char *)malloc(need ? need : 1);              // exactly the size asked for
    const size_t got = cfrk_host_format_fasta(data, start.data(), length.data(), ip, nS, buf, need);
    if (got != need || memcmp(buf, want.data(), need) != 0) { fprintf(stderr, "set %d: text differs\n", round); return 1; }
    free(buf);
    free(data);
    ++sets; reads += (size_t)nS; bytes += need;
  }
  printf("filter_host_check: %zu read sets, %zu reads, %zu bytes of FASTA; formatter and restatement agree\n", sets, reads, bytes);
  return 0;
}
