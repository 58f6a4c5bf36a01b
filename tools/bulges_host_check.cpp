// bulges_host_check.cpp -- the bulge report's formatter (cfrk_host_format_bulges) under the sanitizers, on the CPU, outside
// pytest.  Built and run as tools/bubbles_host_check.cpp is:
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o bulges_host_check tools/bulges_host_check.cpp cfrk_amd/host/cfrk_host.cpp
//   ./bulges_host_check
//
// Random unitig sets in the native layout -- unitigs of one base and shorter than k - 1, invalid codes, n_kmers 0, summed
// counts up to 2^64 - 1 -- with random pop bytes and path rows: empty rows, rows of up to 64 entries in both strands, a
// unitig on its own path, entries that name no unitig, and paths built to spell the popped sequence with 0, 1 or more
// bases changed.  Everything is formatted into buffers of exactly the size the sizing call returned (so that a write past
// them is seen), from arrays of exactly their size, and compared with a restatement through snprintf and std::string.
// Prints one summary line; exit status 1 on a disagreement.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../cfrk_amd/host/cfrk_host.h"

static uint64_t rng_state = 0x8EBC6AF09C88C6E3ull;
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
    const int64_t nS = round == 0 ? 0 : (int64_t)(2 + rnd() % 40);
    const int k = (int)(1 + rnd() % 12);
    std::vector<int32_t> length((size_t)nS);
    std::vector<int64_t> start((size_t)nS);
    Rec *rec = (Rec *)malloc(nS ? (size_t)nS * sizeof(Rec) : 1);              // exactly nS rows
    uint8_t *pop = (uint8_t *)malloc(nS ? (size_t)nS : 1);                    // exactly nS bytes
    int64_t *path_ptr = (int64_t *)malloc(((size_t)nS + 1) * 8);              // exactly nS + 1 offsets
    std::vector<uint32_t> rows;
    int64_t nN = 0;
    // every third unitig j is to be popped beside the two before it: as long as they spell together
    for (int64_t j = 0; j < nS; ++j) {
      int32_t L = (rnd() % 7 == 0) ? 1 : (int32_t)(1 + rnd() % 60);
      if (j % 3 == 2 && rnd() % 4) {
        const int32_t a = length[(size_t)j - 2], b = length[(size_t)j - 1];
        L = a + (b > k - 1 ? b - (k - 1) : 0) + (rnd() % 5 == 0 ? 1 : 0);
      }
      length[(size_t)j] = L;
      start[(size_t)j] = nN;
      nN += L + 1;
      Rec &r = rec[j];
      r.n_kmers = (rnd() % 9 == 0) ? 0 : (rnd() % 4 == 0) ? (uint32_t)rnd() | 1u : (uint32_t)(1 + rnd() % 1000);
      r.kc = (rnd() % 3 == 0) ? rnd() : rnd() % 100000;
      r.flags = (uint32_t)(rnd() % 2);
    }
    int8_t *data = (int8_t *)malloc(nN ? (size_t)nN : 1);                     // exactly nN bytes: no slack behind the unitigs
    for (int64_t x = 0; x < nN; ++x) data[x] = (rnd() % 50 == 0) ? (int8_t)(rnd() % 256) : (int8_t)(rnd() % 4);
    for (int64_t j = 0; j < nS; ++j) data[start[(size_t)j] + length[(size_t)j]] = -1;

    auto text = [&](int64_t j, bool minus) {
      std::string seq;
      for (int32_t x = 0; x < length[(size_t)j]; ++x) {
        const int c = data[start[(size_t)j] + (minus ? length[(size_t)j] - 1 - x : x)];
        seq += (c >= 0 && c <= 3) ? "ACGT"[minus ? 3 - c : c] : 'N';
      }
      return seq;
    };
    auto spell = [&](const uint32_t *row, int64_t m) {
      std::string seq;
      for (int64_t t = 0; t < m; ++t) {
        const std::string s = text((int64_t)(row[t] >> 1), row[t] & 1u);
        seq += t == 0 ? s : s.size() > (size_t)(k - 1) ? s.substr((size_t)(k - 1)) : std::string();
      }
      return seq;
    };

    path_ptr[0] = 0;
    for (int64_t j = 0; j < nS; ++j) {
      pop[j] = (uint8_t)(rnd() % 3 == 0 ? 0 : rnd() % 2 ? 1 : rnd());
      const uint64_t how = rnd() % 8;
      if (j % 3 == 2 && how < 5) {
        // the two unitigs before j, in either strand; j becomes what they spell, with 0, 1 or 2 bases changed
        const uint32_t o = (uint32_t)(rnd() % 2);
        const uint32_t row[2] = {(uint32_t)(o ? j - 1 : j - 2) << 1 | o, (uint32_t)(o ? j - 2 : j - 1) << 1 | o};
        rows.push_back(row[0]); rows.push_back(row[1]);
        const std::string s = spell(row, 2);
        if ((int32_t)s.size() == length[(size_t)j]) {
          for (size_t x = 0; x < s.size(); ++x) data[start[(size_t)j] + (int64_t)x] = (int8_t)(s[x] == 'N' ? 7 : strchr("ACGT", s[x]) - "ACGT");
          for (uint64_t e = rnd() % 3; e > 0; --e) {
            int8_t &c = data[start[(size_t)j] + (int64_t)(rnd() % s.size())];
            c = (int8_t)((c + 1) & 3);
          }
        }
      } else if (how != 5) {
        const uint64_t m = how == 6 ? 64 : rnd() % 5;
        for (uint64_t t = 0; t < m; ++t) {
          const uint32_t w = rnd() % 16 == 0 ? (uint32_t)nS + (uint32_t)(rnd() % 3) * 0x3FFFFFF0u : (uint32_t)(rnd() % (uint64_t)nS);
          rows.push_back((w << 1) | (uint32_t)(rnd() % 2));
        }
      }
      path_ptr[j + 1] = (int64_t)rows.size();
    }
    uint32_t *path = (uint32_t *)malloc(rows.empty() ? 1 : rows.size() * 4);   // exactly n_path words
    if (!rows.empty()) memcpy(path, rows.data(), rows.size() * 4);

    const uint32_t no = (uint32_t)(rnd() % 3 == 0 ? rnd() : 1 + rnd() % 8);
    std::string want;
    for (int64_t j = 0; j < nS; ++j) {
      const int64_t a = path_ptr[j], m = path_ptr[j + 1] - a;
      if (!pop[j] || m <= 0) continue;
      bool named = true;
      uint64_t kmers = 0;
      std::string names;
      for (int64_t t = 0; t < m; ++t) {
        const int64_t w = (int64_t)(path[a + t] >> 1);
        if (w >= nS) { named = false; break; }
        kmers += rec[w].n_kmers;
        names += (path[a + t] & 1u) ? '<' : '>';
        names += std::to_string(w);
      }
      if (!named) continue;
      const std::string own = text(j, false), beside = spell(path + a, m);
      int kind = 2;
      if (own.size() == beside.size()) {
        size_t differ = 0;
        for (size_t x = 0; x < own.size(); ++x) differ += own[x] != beside[x];
        kind = differ == 1 ? 0 : 1;
      }
      ++kinds[kind];
      char head[256];
      snprintf(head, sizeof head, "%u\t%lld\t%zu\t%s\t%lld\t%llu\t", (unsigned)no, (long long)j, own.size(), mean(rec[j]).c_str(), (long long)m,
               (unsigned long long)kmers);
      want += head + names + "\t" + (kind == 0 ? "snp" : kind == 1 ? "mnp" : "indel") + "\t" + own + "\t" + beside + "\n";
      ++lines;
    }

    const size_t need = cfrk_host_format_bulges(no, data, start.data(), length.data(), rec, nS, pop, path_ptr, path, k, nullptr, 0);
    if (need != want.size()) { fprintf(stderr, "set %d: sized %zu, expected %zu\n", round, need, want.size()); return 1; }
    char *buf = (char *)malloc(need ? need : 1);                              // exactly the size asked for
    const size_t got = cfrk_host_format_bulges(no, data, start.data(), length.data(), rec, nS, pop, path_ptr, path, k, buf, need);
    if (got != need || memcmp(buf, want.data(), need) != 0) { fprintf(stderr, "set %d: the text differs\n", round); return 1; }
    free(buf);
    free(path);
    free(data);
    free(path_ptr);
    free(pop);
    free(rec);
    bytes += need;
    ++sets; unitigs += (size_t)nS;
  }
  if (!kinds[0] || !kinds[1] || !kinds[2]) { fprintf(stderr, "a kind never occurred: %zu snp, %zu mnp, %zu indel\n", kinds[0], kinds[1], kinds[2]); return 1; }
  printf("bulges_host_check: %zu sets, %zu unitigs, %zu lines (%zu snp, %zu mnp, %zu indel), %zu bytes; formatter and restatement agree\n",
         sets, unitigs, lines, kinds[0], kinds[1], kinds[2], bytes);
  return 0;
}
