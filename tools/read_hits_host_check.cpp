// read_hits_host_check.cpp -- the GAF formatter (cfrk_host_format_gaf) under the sanitizers, on the CPU, outside the
// library's Python loading.  Built and run as tools/unitig_links_host_check.cpp is:
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o read_hits_host_check tools/read_hits_host_check.cpp cfrk_amd/host/cfrk_host.cpp
//   ./read_hits_host_check
//
// Random unitig length lists and random CSR hit sets -- reads without hits, rows of up to 12 hits, both strands, k from
// 1 to 64, offsets and lengths up to the ten-digit range, hits that end at the unitig's last base -- are formatted into
// buffers of exactly the size the sizing call returned (so that a write past them is seen), from arrays of exactly their
// size, and compared with a restatement through snprintf and std::string.  Prints one summary line; exit status 1 on a
// disagreement.
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

struct Hit { uint32_t unitig, unitig_at, read_off, n_windows; };

int main() {
  static_assert(sizeof(Hit) == 16, "the rows are 16 bytes");
  size_t sets = 0, nhits = 0, bytes = 0;
  for (int round = 0; round < 400; ++round) {
    const int64_t nU = 1 + (int64_t)(rnd() % 30), nR = round == 0 ? 0 : (int64_t)(rnd() % 40);
    const int k = (int)(1 + rnd() % 64);
    const bool big = rnd() % 4 == 0;
    int32_t *ulen = (int32_t *)malloc((size_t)nU * 4);               // exactly nU lengths
    for (int64_t j = 0; j < nU; ++j) ulen[j] = big ? (int32_t)(k + rnd() % 2000000000u) : (int32_t)(k + rnd() % 500);
    int32_t *rlen = (int32_t *)malloc(nR ? (size_t)nR * 4 : 1);      // exactly nR lengths
    int64_t *ptr = (int64_t *)malloc(((size_t)nR + 1) * 8);          // exactly nR + 1 offsets
    ptr[0] = 0;
    for (int64_t i = 0; i < nR; ++i) {
      rlen[i] = big ? (int32_t)(rnd() % 2147483647u) : (int32_t)(rnd() % 400);
      ptr[i + 1] = ptr[i] + (int64_t)(rnd() % 3 == 0 ? 0 : rnd() % 13);
    }
    const int64_t nH = ptr[nR];
    Hit *hits = (Hit *)malloc(nH ? (size_t)nH * sizeof(Hit) : 1);     // exactly n_hits rows
    for (int64_t h = 0; h < nH; ++h) {
      Hit &x = hits[h];
      x.unitig = (uint32_t)(rnd() % (uint64_t)nU);
      const uint32_t nk = (uint32_t)(ulen[x.unitig] - k + 1);         // the unitig's k-mers
      x.n_windows = 1 + (uint32_t)(rnd() % nk);
      const uint32_t off = rnd() % 3 == 0 ? nk - x.n_windows : (uint32_t)(rnd() % (nk - x.n_windows + 1));
      x.unitig_at = (off << 1) | (uint32_t)(rnd() & 1);
      x.read_off = big ? (uint32_t)(rnd() % 2000000000u) : (uint32_t)(rnd() % 400);
    }
    std::string want;
    for (int64_t i = 0; i < nR; ++i)
      for (int64_t h = ptr[i]; h < ptr[i + 1]; ++h) {
        const Hit &x = hits[h];
        const unsigned long long m = (unsigned long long)x.n_windows + (unsigned long long)k - 1, off = x.unitig_at >> 1,
                                 ln = (unsigned long long)ulen[x.unitig];
        const bool minus = (x.unitig_at & 1) != 0;
        const unsigned long long ps = minus ? ln - off - m : off;
        char line[400];
        snprintf(line, sizeof line, "%lld\t%d\t%u\t%llu\t+\t%c%u\t%llu\t%llu\t%llu\t%llu\t%llu\t255\tcg:Z:%llu=\n", (long long)i, (int)rlen[i],
                 (unsigned)x.read_off, (unsigned long long)x.read_off + m, minus ? '<' : '>', (unsigned)x.unitig, ln, ps, ps + m, m, m, m);
        want += line;
      }
    const size_t need = cfrk_host_format_gaf(rlen, nR, ptr, hits, ulen, k, nullptr, 0);
    if (need != want.size()) { fprintf(stderr, "set %d: sized %zu, expected %zu\n", round, need, want.size()); return 1; }
    char *buf = (char *)malloc(need ? need : 1);                     // exactly the size asked for
    const size_t got = cfrk_host_format_gaf(rlen, nR, ptr, hits, ulen, k, buf, need);
    if (got != need || memcmp(buf, want.data(), need) != 0) { fprintf(stderr, "set %d: GAF text differs\n", round); return 1; }
    free(buf);
    free(hits);
    free(ptr);
    free(rlen);
    free(ulen);
    ++sets; nhits += (size_t)nH; bytes += need;
  }
  printf("read_hits_host_check: %zu sets, %zu hits, %zu bytes of GAF; formatter and restatement agree\n", sets, nhits, bytes);
  return 0;
}
