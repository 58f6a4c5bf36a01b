// read_paths_host_check.cpp -- the two formatters of the read paths (cfrk_host_format_gaf_paths,
// cfrk_host_format_gfa_support) under the sanitizers, on the CPU, outside the library's Python loading.  Built and run as
// tools/read_hits_host_check.cpp is:
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o read_paths_host_check tools/read_paths_host_check.cpp cfrk_amd/host/cfrk_host.cpp
//   ./read_paths_host_check
//
// Random unitig lists with random link rows (self-links, hairpins, rows with and without their mirror, both strand
// rules), random CSR hit sets cut into random paths, k from 1 to 64, numbers up to the ten-digit range and support
// counters up to 2^32 - 1 are formatted into buffers of exactly the size the sizing call returned (so that a write past
// them is seen), from arrays of exactly their size, and compared with a restatement through snprintf and std::string.  A
// path of one hit is also held to the line cfrk_host_format_gaf writes.  Prints one summary line; exit status 1 on a
// disagreement.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../cfrk_amd/host/cfrk_host.h"

static uint64_t rng_state = 0xD1B54A32D192ED03ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}

struct Hit { uint32_t unitig, unitig_at, read_off, n_windows; };
struct Path { uint32_t hit_first, n_hits, read_off, n_windows; };
struct Link { uint32_t to, flags; };
struct Rec { uint64_t kc; uint32_t n_kmers, flags; };

template <class T> static T *exactly(size_t n) { return (T *)malloc(n ? n * sizeof(T) : 1); }

static int check_gaf_paths(int round, size_t *npaths, size_t *bytes) {
  const int64_t nU = 1 + (int64_t)(rnd() % 30), nR = round == 0 ? 0 : (int64_t)(rnd() % 40);
  const int k = (int)(1 + rnd() % 64);
  const bool big = rnd() % 4 == 0;
  int32_t *ulen = exactly<int32_t>((size_t)nU);
  for (int64_t j = 0; j < nU; ++j) ulen[j] = big ? (int32_t)(k + rnd() % 2000000000u) : (int32_t)(k + rnd() % 500);
  int32_t *rlen = exactly<int32_t>((size_t)nR);
  int64_t *ptr = exactly<int64_t>((size_t)nR + 1), *pptr = exactly<int64_t>((size_t)nR + 1);
  ptr[0] = pptr[0] = 0;
  for (int64_t i = 0; i < nR; ++i) {
    rlen[i] = big ? (int32_t)(rnd() % 2147483647u) : (int32_t)(rnd() % 400);
    ptr[i + 1] = ptr[i] + (int64_t)(rnd() % 3 == 0 ? 0 : rnd() % 13);
  }
  const int64_t nH = ptr[nR];
  Hit *hits = exactly<Hit>((size_t)nH);
  for (int64_t h = 0; h < nH; ++h) {
    Hit &x = hits[h];
    x.unitig = (uint32_t)(rnd() % (uint64_t)nU);
    const uint32_t nk = (uint32_t)(ulen[x.unitig] - k + 1);
    x.n_windows = 1 + (uint32_t)(rnd() % nk);
    const uint32_t off = rnd() % 3 == 0 ? nk - x.n_windows : (uint32_t)(rnd() % (nk - x.n_windows + 1));
    x.unitig_at = (off << 1) | (uint32_t)(rnd() & 1);
    x.read_off = big ? (uint32_t)(rnd() % 2000000000u) : (uint32_t)(rnd() % 400);
  }
  // every read's hits cut into paths at random places (at most nH of them)
  Path *paths = exactly<Path>((size_t)nH);
  int64_t nP = 0;
  for (int64_t i = 0; i < nR; ++i) {
    for (int64_t h = ptr[i]; h < ptr[i + 1];) {
      int64_t e = h + 1;
      while (e < ptr[i + 1] && rnd() % 3 != 0) ++e;
      Path &p = paths[nP++];
      p.hit_first = (uint32_t)(h - ptr[i]); p.n_hits = (uint32_t)(e - h); p.read_off = hits[h].read_off;
      p.n_windows = big ? (uint32_t)(rnd() % 2000000000u) : (uint32_t)(1 + rnd() % 300);
      h = e;
    }
    pptr[i + 1] = nP;
  }
  std::string want;
  for (int64_t i = 0; i < nR; ++i)
    for (int64_t t = pptr[i]; t < pptr[i + 1]; ++t) {
      const Path &p = paths[t];
      const Hit *c = hits + ptr[i] + p.hit_first;
      const unsigned long long m = (unsigned long long)p.n_windows + (unsigned long long)k - 1;
      unsigned long long pl = 0;
      std::string name;
      for (uint32_t x = 0; x < p.n_hits; ++x) {
        pl += (unsigned long long)ulen[c[x].unitig] - (x ? (unsigned long long)k - 1 : 0);
        name += (c[x].unitig_at & 1) ? '<' : '>';
        name += std::to_string(c[x].unitig);
      }
      const unsigned long long off = c[0].unitig_at >> 1, hm = (unsigned long long)c[0].n_windows + (unsigned long long)k - 1,
                               ln = (unsigned long long)ulen[c[0].unitig];
      const unsigned long long ps = (c[0].unitig_at & 1) ? ln - off - hm : off;
      char line[200];
      snprintf(line, sizeof line, "%lld\t%d\t%u\t%llu\t+\t", (long long)i, (int)rlen[i], (unsigned)p.read_off, (unsigned long long)p.read_off + m);
      want += line;
      want += name;
      snprintf(line, sizeof line, "\t%llu\t%llu\t%llu\t%llu\t%llu\t255\tcg:Z:%llu=\n", pl, ps, ps + m, m, m, m);
      want += line;
    }
  const size_t need = cfrk_host_format_gaf_paths(rlen, nR, ptr, hits, pptr, paths, ulen, k, nullptr, 0);
  if (need != want.size()) { fprintf(stderr, "set %d: GAF paths sized %zu, expected %zu\n", round, need, want.size()); return 1; }
  char *buf = exactly<char>(need);
  const size_t got = cfrk_host_format_gaf_paths(rlen, nR, ptr, hits, pptr, paths, ulen, k, buf, need);
  if (got != need || memcmp(buf, want.data(), need) != 0) { fprintf(stderr, "set %d: GAF path text differs\n", round); return 1; }
  free(buf);
  // every hit a path of its own, with the hit's windows: the text of cfrk_host_format_gaf
  Path *one = exactly<Path>((size_t)nH);
  for (int64_t i = 0; i < nR; ++i)
    for (int64_t h = ptr[i]; h < ptr[i + 1]; ++h) one[h] = Path{(uint32_t)(h - ptr[i]), 1u, hits[h].read_off, hits[h].n_windows};
  const size_t n1 = cfrk_host_format_gaf(rlen, nR, ptr, hits, ulen, k, nullptr, 0);
  const size_t n2 = cfrk_host_format_gaf_paths(rlen, nR, ptr, hits, ptr, one, ulen, k, nullptr, 0);
  if (n1 != n2) { fprintf(stderr, "set %d: paths of one hit sized %zu, the hits %zu\n", round, n2, n1); return 1; }
  char *b1 = exactly<char>(n1), *b2 = exactly<char>(n2);
  cfrk_host_format_gaf(rlen, nR, ptr, hits, ulen, k, b1, n1);
  cfrk_host_format_gaf_paths(rlen, nR, ptr, hits, ptr, one, ulen, k, b2, n2);
  if (memcmp(b1, b2, n1) != 0) { fprintf(stderr, "set %d: a path of one hit is not the hit's line\n", round); return 1; }
  free(b1); free(b2); free(one); free(paths); free(hits); free(pptr); free(ptr); free(rlen); free(ulen);
  *npaths += (size_t)nP; *bytes += need;
  return 0;
}

static int check_gfa_support(int round, size_t *nlinks, size_t *bytes) {
  const int64_t nS = round == 0 ? 0 : 1 + (int64_t)(rnd() % 12);
  const int k = (int)(1 + rnd() % 64);
  const bool canonical = rnd() % 2 == 0, big = rnd() % 4 == 0;
  int32_t *length = exactly<int32_t>((size_t)nS);
  int64_t *start = exactly<int64_t>((size_t)nS), *lptr = exactly<int64_t>((size_t)nS + 1);
  Rec *rec = exactly<Rec>((size_t)nS);
  int64_t nN = 0;
  for (int64_t j = 0; j < nS; ++j) { length[j] = (int32_t)(k + rnd() % 40); start[j] = nN; nN += length[j] + 1; }
  int8_t *data = exactly<int8_t>((size_t)nN);
  for (int64_t x = 0; x < nN; ++x) data[x] = (int8_t)(rnd() % 4);
  for (int64_t j = 0; j < nS; ++j) {
    data[start[j] + length[j]] = -1;
    rec[j].n_kmers = (uint32_t)(length[j] - k + 1); rec[j].kc = big ? rnd() : rnd() % 1000; rec[j].flags = 0;
  }
  // rows of up to 16 links: up to three of a unitig's own, and for about half of the links their mirror in the target's row
  lptr[0] = 0;
  Link tmp[12][16];
  int cnt[12] = {0};
  for (int64_t j = 0; j < nS; ++j)
    for (int t = 0, n = (int)(rnd() % 4); t < n; ++t) {
      const uint32_t to = (uint32_t)(rnd() % (uint64_t)nS), flags = canonical ? (uint32_t)(rnd() % 4) : 0u;
      if (cnt[j] < 16) tmp[j][cnt[j]++] = Link{to, flags};
      if (canonical && rnd() % 2 == 0 && cnt[to] < 16)                  // the mirror (to,!tm) -> (j,!fm)
        tmp[to][cnt[to]++] = Link{(uint32_t)j, (uint32_t)(((flags & 2) ? 0 : 1) | ((flags & 1) ? 0 : 2))};
    }
  for (int64_t j = 0; j < nS; ++j) lptr[j + 1] = lptr[j] + cnt[j];
  const int64_t nL = lptr[nS];
  Link *links = exactly<Link>((size_t)nL);
  uint32_t *support = exactly<uint32_t>((size_t)nL);
  for (int64_t j = 0; j < nS; ++j)
    for (int t = 0; t < cnt[j]; ++t) links[lptr[j] + t] = tmp[j][t];
  for (int64_t r = 0; r < nL; ++r) support[r] = big ? (uint32_t)rnd() : (uint32_t)(rnd() % 50);
  // the plain GFA, then RC:i: spliced behind every L line
  const size_t plain_n = cfrk_host_format_gfa(data, start, length, rec, nS, lptr, links, k, nullptr, 0);
  char *plain = exactly<char>(plain_n);
  cfrk_host_format_gfa(data, start, length, rec, nS, lptr, links, k, plain, plain_n);
  std::string want;
  size_t at = 0;
  int64_t r = 0, j = 0;
  while (at < plain_n) {
    const char *nl = (const char *)memchr(plain + at, '\n', plain_n - at);
    const size_t end = (size_t)(nl - plain);
    want.append(plain + at, end - at);
    if (plain[at] == 'L') {
      while (r >= lptr[j + 1]) ++j;
      unsigned long long c = support[r];
      if (canonical) {
        const Link l = links[r];
        const uint32_t mflags = ((l.flags & 2) ? 0u : 1u) | ((l.flags & 1) ? 0u : 2u);
        for (int64_t x = lptr[l.to]; x < lptr[l.to + 1]; ++x)
          if (links[x].to == (uint32_t)j && links[x].flags == mflags) { if (x != r) c += support[x]; break; }
      }
      want += "\tRC:i:" + std::to_string(c);
      ++r;
    }
    want += '\n';
    at = end + 1;
  }
  if (r != nL) { fprintf(stderr, "set %d: %lld L lines for %lld links\n", round, (long long)r, (long long)nL); return 1; }
  const size_t need = cfrk_host_format_gfa_support(data, start, length, rec, nS, lptr, links, support, canonical ? 1 : 0, k, nullptr, 0);
  if (need != want.size()) { fprintf(stderr, "set %d: GFA with support sized %zu, expected %zu\n", round, need, want.size()); return 1; }
  char *buf = exactly<char>(need);
  const size_t got = cfrk_host_format_gfa_support(data, start, length, rec, nS, lptr, links, support, canonical ? 1 : 0, k, buf, need);
  if (got != need || memcmp(buf, want.data(), need) != 0) { fprintf(stderr, "set %d: GFA text with support differs\n", round); return 1; }
  free(buf); free(plain); free(support); free(links); free(data); free(rec); free(lptr); free(start); free(length);
  *nlinks += (size_t)nL; *bytes += need;
  return 0;
}

int main() {
  static_assert(sizeof(Hit) == 16 && sizeof(Path) == 16 && sizeof(Link) == 8 && sizeof(Rec) == 16, "the rows' sizes");
  size_t npaths = 0, nlinks = 0, bytes = 0;
  for (int round = 0; round < 400; ++round) {
    if (check_gaf_paths(round, &npaths, &bytes)) return 1;
    if (check_gfa_support(round, &nlinks, &bytes)) return 1;
  }
  printf("read_paths_host_check: %zu paths, %zu links, %zu bytes of text; formatters and restatement agree\n", npaths, nlinks, bytes);
  return 0;
}
