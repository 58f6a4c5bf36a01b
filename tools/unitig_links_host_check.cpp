// unitig_links_host_check.cpp -- the two link formatters (cfrk_host_format_unitigs_links, cfrk_host_format_gfa) under
// the sanitizers, on the CPU, outside pytest.  Built and run as tools/unitigs_host_check.cpp is:
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o unitig_links_host_check tools/unitig_links_host_check.cpp cfrk_amd/host/cfrk_host.cpp
//   ./unitig_links_host_check
//
// Random unitig sets in the native layout (as in unitigs_host_check.cpp) with random CSR link sets -- empty rows, rows of
// up to 16 links, targets up to 2^32 - 1, all four flag combinations, k from 1 to 64 -- are formatted into buffers of
// exactly the size the sizing call returned (so that a write past them is seen), from arrays of exactly their size, and
// compared with a restatement through snprintf and std::string.  Prints one summary line; exit status 1 on a
// disagreement.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../cfrk_amd/host/cfrk_host.h"

static uint64_t rng_state = 0xD1B54A32D192ED03ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}

struct Rec { uint64_t kc; uint32_t n_kmers, flags; };
struct Link { uint32_t to, flags; };

static std::string mean(const Rec &r) {
  const unsigned __int128 tenths = ((unsigned __int128)r.kc * 10 + r.n_kmers / 2) / r.n_kmers;
  char s[64];
  snprintf(s, sizeof s, "%llu.%d", (unsigned long long)(tenths / 10), (int)(tenths % 10));
  return s;
}

int main() {
  static_assert(sizeof(Rec) == 16 && sizeof(Link) == 8, "the rows are 16 and 8 bytes");
  size_t sets = 0, unitigs = 0, nlinks = 0, bytes = 0;
  for (int round = 0; round < 300; ++round) {
    const int64_t nS = round == 0 ? 0 : (int64_t)(rnd() % 40);
    const int k = (int)(1 + rnd() % 64);
    std::vector<int32_t> length((size_t)nS);
    std::vector<int64_t> start((size_t)nS);
    Rec *rec = (Rec *)malloc(nS ? (size_t)nS * sizeof(Rec) : 1);      // exactly nS rows
    int64_t *link_ptr = (int64_t *)malloc(((size_t)nS + 1) * 8);      // exactly nS + 1 offsets
    int64_t nN = 0;
    link_ptr[0] = 0;
    for (int64_t j = 0; j < nS; ++j) {
      length[(size_t)j] = (rnd() % 7 == 0) ? 1 : (int32_t)(1 + rnd() % 300);
      start[(size_t)j] = nN;
      nN += length[(size_t)j] + 1;
      Rec &r = rec[j];
      r.n_kmers = (rnd() % 4 == 0) ? (uint32_t)rnd() | 1u : (uint32_t)(1 + rnd() % 1000);
      r.kc = (rnd() % 3 == 0) ? rnd() : rnd() % 100000;
      r.flags = (uint32_t)(rnd() % 2);
      link_ptr[j + 1] = link_ptr[j] + (int64_t)(rnd() % 3 == 0 ? 0 : rnd() % 17);
    }
    const int64_t nL = link_ptr[nS];
    Link *links = (Link *)malloc(nL ? (size_t)nL * sizeof(Link) : 1);  // exactly n_links rows
    for (int64_t i = 0; i < nL; ++i) {
      links[i].to = (rnd() % 5 == 0) ? (uint32_t)rnd() : (uint32_t)(rnd() % 1000);
      links[i].flags = (uint32_t)(rnd() % 4);
    }
    int8_t *data = (int8_t *)malloc(nN ? (size_t)nN : 1);            // exactly nN bytes: no slack behind the unitigs
    for (int64_t x = 0; x < nN; ++x) data[x] = (rnd() % 50 == 0) ? (int8_t)(rnd() % 256) : (int8_t)(rnd() % 4);
    for (int64_t j = 0; j < nS; ++j) data[start[(size_t)j] + length[(size_t)j]] = -1;

    std::string fasta, gfa = "H\tVN:Z:1.0\n", gfa_links;
    for (int64_t j = 0; j < nS; ++j) {
      const Rec &r = rec[j];
      std::string seq;
      for (int32_t x = 0; x < length[(size_t)j]; ++x) {
        const int c = data[start[(size_t)j] + x];
        seq += (c >= 0 && c <= 3) ? "ACGT"[c] : 'N';
      }
      char head[200];
      snprintf(head, sizeof head, ">%lld LN:i:%d KC:i:%llu km:f:%s%s", (long long)j, (int)length[(size_t)j], (unsigned long long)r.kc,
               mean(r).c_str(), (r.flags & 1) ? " CL:i:1" : "");
      fasta += head;
      for (int64_t i = link_ptr[j]; i < link_ptr[j + 1]; ++i) {
        const char from = (links[i].flags & 1) ? '-' : '+', to = (links[i].flags & 2) ? '-' : '+';
        char tag[64];
        snprintf(tag, sizeof tag, " L:%c:%u:%c", from, (unsigned)links[i].to, to);
        fasta += tag;
        snprintf(tag, sizeof tag, "L\t%lld\t%c\t%u\t%c\t%dM\n", (long long)j, from, (unsigned)links[i].to, to, k - 1);
        gfa_links += tag;
      }
      fasta += "\n" + seq + "\n";
      snprintf(head, sizeof head, "\tLN:i:%d\tKC:i:%llu\tkm:f:%s\n", (int)length[(size_t)j], (unsigned long long)r.kc, mean(r).c_str());
      gfa += "S\t" + std::to_string(j) + "\t" + seq + head;
    }
    gfa += gfa_links;

    for (int which = 0; which < 2; ++which) {
      const std::string &want = which ? gfa : fasta;
      const size_t need = which ? cfrk_host_format_gfa(data, start.data(), length.data(), rec, nS, link_ptr, links, k, nullptr, 0)
                                : cfrk_host_format_unitigs_links(data, start.data(), length.data(), rec, nS, link_ptr, links, nullptr, 0);
      if (need != want.size()) { fprintf(stderr, "set %d, %s: sized %zu, expected %zu\n", round, which ? "GFA" : "FASTA", need, want.size()); return 1; }
      char *buf = (char *)malloc(need ? need : 1);                   // exactly the size asked for
      const size_t got = which ? cfrk_host_format_gfa(data, start.data(), length.data(), rec, nS, link_ptr, links, k, buf, need)
                               : cfrk_host_format_unitigs_links(data, start.data(), length.data(), rec, nS, link_ptr, links, buf, need);
      if (got != need || memcmp(buf, want.data(), need) != 0) { fprintf(stderr, "set %d: %s text differs\n", round, which ? "GFA" : "FASTA"); return 1; }
      free(buf);
      bytes += need;
    }
    // without link_ptr the FASTA is the plain formatter's
    {
      const size_t a = cfrk_host_format_unitigs_links(data, start.data(), length.data(), rec, nS, nullptr, nullptr, nullptr, 0);
      const size_t b = cfrk_host_format_unitigs(data, start.data(), length.data(), rec, nS, nullptr, 0);
      if (a != b) { fprintf(stderr, "set %d: the formatter without links sizes %zu, the plain one %zu\n", round, a, b); return 1; }
    }
    free(data);
    free(links);
    free(link_ptr);
    free(rec);
    ++sets; unitigs += (size_t)nS; nlinks += (size_t)nL;
  }
  printf("unitig_links_host_check: %zu sets, %zu unitigs, %zu links, %zu bytes of FASTA and GFA; formatters and restatement agree\n",
         sets, unitigs, nlinks, bytes);
  return 0;
}
