// cfrk_host.cpp -- FASTA and FASTQ ingest, chunk views and .cfrk formatting (see cfrk_host.h).
#include "cfrk_host.h"

#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

namespace {

struct CodeTable {
  int8_t t[256];
  CodeTable() {
    memset(t, -1, sizeof t);                       // default: -1 (src/fastaIO.h:137-138)
    t['a'] = t['A'] = 0; t['c'] = t['C'] = 1;      // src/fastaIO.h:123-136
    t['g'] = t['G'] = 2; t['t'] = t['T'] = 3;
  }
};
const CodeTable kCodes;

// append decimal digits of v, return new end
inline char *put_u64(char *p, uint64_t v) {
  char tmp[24];
  int n = 0;
  do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
  while (n) *p++ = tmp[--n];
  return p;
}
inline char *put_i32(char *p, int32_t v) {          // "%d"
  if (v < 0) { *p++ = '-'; return put_u64(p, (uint64_t)(-(int64_t)v)); }
  return put_u64(p, (uint64_t)v);
}
inline size_t len_u64(uint64_t v) { size_t n = 1; while (v >= 10) { v /= 10; ++n; } return n; }

// n bytes of sequence text -> codes (src/fastaIO.h:121-140: aA cC gG tT -> 0 1 2 3, anything else -1).
// The AVX2 form does 32 bytes per step (round 5: the byte-at-a-time table look-up was half of the parser's time on a
// 1.6 GB file): clear the case bit, ((c >> 1) & 3) is A 0, C 1, T 2, G 3 for the four letters, x ^ (x >> 1) swaps the
// last two into the reference's order, and a byte that is none of the four letters becomes -1.
static void encode_plain(const unsigned char *src, int8_t *dst, size_t n) {
  for (size_t i = 0; i < n; ++i) dst[i] = kCodes.t[src[i]];
}
#if defined(__x86_64__)
__attribute__((target("avx2"))) static void encode_avx2(const unsigned char *src, int8_t *dst, size_t n) {
  const __m256i up = _mm256_set1_epi8((char)0xDF), three = _mm256_set1_epi8(3), one = _mm256_set1_epi8(1);
  const __m256i cA = _mm256_set1_epi8('A'), cC = _mm256_set1_epi8('C'), cG = _mm256_set1_epi8('G'), cT = _mm256_set1_epi8('T');
  size_t i = 0;
  for (; i + 32 <= n; i += 32) {
    const __m256i c = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i));
    const __m256i u = _mm256_and_si256(c, up);
    const __m256i ok = _mm256_or_si256(_mm256_or_si256(_mm256_cmpeq_epi8(u, cA), _mm256_cmpeq_epi8(u, cC)),
                                       _mm256_or_si256(_mm256_cmpeq_epi8(u, cG), _mm256_cmpeq_epi8(u, cT)));
    const __m256i x = _mm256_and_si256(_mm256_srli_epi16(u, 1), three);            // (the & 3 drops what the 16-bit shift drags in)
    const __m256i code = _mm256_xor_si256(x, _mm256_and_si256(_mm256_srli_epi16(x, 1), one));
    // ok ? code : -1
    _mm256_storeu_si256(reinterpret_cast<__m256i *>(dst + i), _mm256_or_si256(code, _mm256_xor_si256(ok, _mm256_set1_epi8(-1))));
  }
  encode_plain(src + i, dst + i, n - i);
}
#endif
static void encode_bytes(const unsigned char *src, int8_t *dst, size_t n) {
#if defined(__x86_64__)
  static const bool have_avx2 = __builtin_cpu_supports("avx2");
  if (have_avx2) { encode_avx2(src, dst, n); return; }
#endif
  encode_plain(src, dst, n);
}

// (huge-page advice for the batch's arrays was tried and dropped: with MADV_HUGEPAGE the first faults of a fresh process
//  took 0.7 - 1.1 s for a 150 MB array -- compaction at fault time -- against 0.03 s of ordinary first-touch faults)
static void *big_alloc(size_t bytes) {
  if (bytes < ((size_t)8 << 20)) return malloc(bytes ? bytes : 1);
  void *p = nullptr;
  const size_t rounded = (bytes + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
  return posix_memalign(&p, (size_t)2 << 20, rounded) == 0 ? p : nullptr;
}

// threads the parser may use (cfrk_host_set_parse_threads; 0 = min(hardware threads, 64): a 1.63 GB file parses at
// 4.7 / 5.1 / 7.1 GB/s with 8 / 16 / 64 threads on the GPU box's 256-thread host, profiles/r05/end_to_end.txt -- the
// 16-thread cap of rounds 1-4 was binding once the file was mapped instead of copied and the encoding vectorised)
int g_parse_threads = 0;

}  // namespace

extern "C" {

void cfrk_host_set_parse_threads(int n) { g_parse_threads = n > 0 ? n : 0; }

void cfrk_host_free_batch(cfrk_batch *b) {
  if (!b) return;
  free(b->data); free(b->start); free(b->length);
  memset(b, 0, sizeof *b);
}

int cfrk_host_parse_fasta(const char *buf, size_t len, int flags, cfrk_batch *out) {
  if (!out || (!buf && len)) return -4;
  memset(out, 0, sizeof *out);
  const bool compat = (flags & CFRK_INGEST_COMPAT) != 0;
  // pass 1: record extents (sequence bytes as the reference would strcat them).  Large inputs are
  // scanned by several threads, each over a range of whole lines; a sequence line that precedes
  // the first header of its range belongs to the last record of the ranges before it.
  struct Rec { size_t first_line; size_t seq_chars; };
  std::vector<Rec> recs;
  std::vector<std::pair<size_t, size_t>> lines;     // (begin, end incl. newline) of sequence lines
  unsigned nthr = std::thread::hardware_concurrency();
  if (g_parse_threads > 0) { if (nthr == 0 || nthr > (unsigned)g_parse_threads) nthr = (unsigned)g_parse_threads; }
  else if (nthr > 64) nthr = 64;
  if (nthr < 2 || len < ((size_t)8 << 20)) nthr = 1;
  {
    struct Part { std::vector<size_t> rec_first; std::vector<std::pair<size_t, size_t>> lines; };
    std::vector<Part> parts(nthr);
    std::vector<size_t> cut(nthr + 1, len);
    cut[0] = 0;
    for (unsigned t = 1; t < nthr; ++t) {            // cuts at line starts
      size_t c = len / nthr * t;
      if (c < cut[t - 1]) c = cut[t - 1];
      const char *nl = (c < len) ? (const char *)memchr(buf + c, '\n', len - c) : nullptr;
      cut[t] = nl ? (size_t)(nl - buf) + 1 : len;
    }
    auto scan = [&](unsigned t) {
      Part &pt = parts[t];
      size_t pos = cut[t];
      const size_t stop = cut[t + 1];
      while (pos < stop) {
        const char *nl = (const char *)memchr(buf + pos, '\n', stop - pos);
        const size_t end = nl ? (size_t)(nl - buf) + 1 : stop;
        if (buf[pos] == '>') pt.rec_first.push_back(pt.lines.size());
        else pt.lines.push_back({pos, end});
        pos = end;
      }
    };
    if (nthr == 1) {
      scan(0);
    } else {
      std::vector<std::thread> pool;
      for (unsigned t = 0; t < nthr; ++t) pool.emplace_back(scan, t);
      for (auto &th : pool) th.join();
    }
    size_t nrec = 0, nline = 0;
    for (auto &pt : parts) { nrec += pt.rec_first.size(); nline += pt.lines.size(); }
    recs.reserve(nrec);
    lines.reserve(nline);
    for (auto &pt : parts) {
      // (a sequence line before any header at all: the reference would dereference garbage)
      if (recs.empty() && pt.rec_first.empty() && !pt.lines.empty()) return -2;
      if (recs.empty() && !pt.rec_first.empty() && pt.rec_first[0] != 0) return -2;
      const size_t base = lines.size();
      for (size_t f : pt.rec_first) recs.push_back(Rec{base + f, 0});
      lines.insert(lines.end(), pt.lines.begin(), pt.lines.end());
    }
  }
  // per-record code counts
  std::vector<int64_t> rlen(recs.size(), 0);
  auto count = [&](size_t r0, size_t r1) {
    for (size_t r = r0; r < r1; ++r) {
      const size_t l1 = (r + 1 < recs.size()) ? recs[r + 1].first_line : lines.size();
      int64_t n = 0;
      for (size_t li = recs[r].first_line; li < l1; ++li) {
        size_t b = lines[li].first, e = lines[li].second;
        if (!compat) while (e > b && (buf[e - 1] == '\n' || buf[e - 1] == '\r')) --e;
        n += (int64_t)(e - b);
      }
      rlen[r] = n;
    }
  };
  if (nthr == 1) {
    count(0, recs.size());
  } else {
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nthr; ++t)
      pool.emplace_back(count, recs.size() * t / nthr, recs.size() * (t + 1) / nthr);
    for (auto &th : pool) th.join();
  }
  int64_t nN = 0;
  for (size_t r = 0; r < recs.size(); ++r) {
    if (compat) {
      if (rlen[r] == 0) return -3;                  // header without a sequence line
      rlen[r] -= 1;                                 // len = strlen(read) - 1
    }
    if (rlen[r] > 0x7FFFFFFF) return -4;
    nN += rlen[r] + 1;
  }
  const int64_t nS = (int64_t)recs.size();
  out->data = (int8_t *)big_alloc((size_t)(nN > 0 ? nN : 1));
  out->start = (int64_t *)big_alloc(sizeof(int64_t) * (size_t)(nS > 0 ? nS : 1));
  out->length = (int32_t *)big_alloc(sizeof(int32_t) * (size_t)(nS > 0 ? nS : 1));
  if (!out->data || !out->start || !out->length) { cfrk_host_free_batch(out); return -4; }
  out->nN = nN; out->nS = nS;
  // pass 2: encode (ProcessData, src/fastaIO.h:74-102: codes, then one -1 terminator).  Records
  // are independent once their offsets are known: large batches are encoded by several threads.
  {
    int64_t w = 0;
    for (int64_t r = 0; r < nS; ++r) {
      out->start[r] = w;
      out->length[r] = (int32_t)rlen[r];
      w += rlen[r] + 1;
    }
  }
  auto encode = [&](int64_t r0, int64_t r1) {
    for (int64_t r = r0; r < r1; ++r) {
      int64_t w = out->start[r];
      int64_t left = rlen[r];
      const size_t l1 = (r + 1 < nS) ? recs[(size_t)r + 1].first_line : lines.size();
      for (size_t li = recs[(size_t)r].first_line; li < l1; ++li) {
        size_t b = lines[li].first, e = lines[li].second;
        if (!compat) while (e > b && (buf[e - 1] == '\n' || buf[e - 1] == '\r')) --e;
        const size_t n = (size_t)std::min<int64_t>((int64_t)(e - b), left);
        encode_bytes(reinterpret_cast<const unsigned char *>(buf) + b, out->data + w, n);
        w += (int64_t)n; left -= (int64_t)n;
      }
      out->data[w] = -1;
    }
  };
  if (nthr < 2 || nN < (int64_t)(8 << 20)) {
    encode(0, nS);
  } else {
    // split by bytes, not by records: reads may differ in length by orders of magnitude
    std::vector<std::thread> pool;
    int64_t r0 = 0;
    for (unsigned t = 0; t < nthr; ++t) {
      const int64_t target = nN / nthr * (t + 1);
      int64_t r1 = r0;
      if (t + 1 == nthr) r1 = nS;
      else while (r1 < nS && out->start[r1] < target) ++r1;
      if (r1 > r0) pool.emplace_back(encode, r0, r1);
      r0 = r1;
    }
    for (auto &th : pool) th.join();
  }
  return 0;
}

int cfrk_host_read_fasta(const char *path, int flags, cfrk_batch *out) {
  // a regular file is MAPPED (round 5: no copy out of the page cache, no zero-filled buffer -- reading a 1.6 GB file
  // into a std::string was a third of the parse); anything else (a pipe) is read chunk by chunk below
  {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return -1;                          // the reference exits (src/fastaIO.h:36)
    struct stat st;
    if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0) {
      void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fd, 0);
      if (m != MAP_FAILED) {
        (void)madvise(m, (size_t)st.st_size, MADV_SEQUENTIAL);
        const int rc = cfrk_host_parse_fasta((const char *)m, (size_t)st.st_size, flags, out);
        munmap(m, (size_t)st.st_size);
        close(fd);
        return rc;
      }
    }
    close(fd);
  }
  FILE *f = fopen(path, "rb");
  if (!f) return -1;
  // a regular file is read in one piece into a buffer of its size (no growth copies); anything
  // that cannot be sized (a pipe) is appended chunk by chunk
  std::string buf;
  long size = -1;
  if (fseek(f, 0, SEEK_END) == 0) { size = ftell(f); if (fseek(f, 0, SEEK_SET) != 0) size = -1; }
  if (size > 0) {
    buf.resize((size_t)size);
    size_t got = 0, n;
    while (got < (size_t)size && (n = fread(&buf[got], 1, (size_t)size - got, f)) > 0) got += n;
    buf.resize(got);
  }
  char tmp[1 << 16];
  size_t n;
  while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) buf.append(tmp, n);   // growing file / pipe
  fclose(f);
  return cfrk_host_parse_fasta(buf.data(), buf.size(), flags, out);
}

int cfrk_host_sniff_format(const char *buf, size_t len) {
  return (buf && len > 0 && buf[0] == '@') ? CFRK_FORMAT_FASTQ : CFRK_FORMAT_FASTA;
}

size_t cfrk_host_fastq_message(int rc, uint64_t where, char *buf, size_t cap) {
  char tmp[160];
  int n = 0;
  const unsigned long long w = (unsigned long long)where;
  switch (rc) {
    case CFRK_FASTQ_NO_AT: n = snprintf(tmp, sizeof tmp, "FASTQ: line %llu does not begin with '@'", w); break;
    case CFRK_FASTQ_NO_PLUS: n = snprintf(tmp, sizeof tmp, "FASTQ: line %llu does not begin with '+'", w); break;
    case CFRK_FASTQ_TRUNCATED: n = snprintf(tmp, sizeof tmp, "FASTQ: %llu lines, not a multiple of four", w); break;
    case CFRK_FASTQ_LENGTHS: n = snprintf(tmp, sizeof tmp, "FASTQ: record %llu has sequence and quality lines of different lengths", w); break;
    case CFRK_FASTQ_LONG: n = snprintf(tmp, sizeof tmp, "FASTQ: record %llu is longer than 2^31 - 1 bases", w); break;
    case CFRK_FASTQ_MIN_QUAL: n = snprintf(tmp, sizeof tmp, "FASTQ: min_qual outside 0 .. 93"); break;
    default: break;
  }
  if (n <= 0) return 0;
  if (buf && cap > 0) {
    const size_t m = std::min((size_t)n, cap - 1);
    memcpy(buf, tmp, m);
    buf[m] = 0;
  }
  return (size_t)n;
}

int cfrk_host_parse_fastq(const char *buf, size_t len, int min_qual, cfrk_batch *out, uint64_t *where) {
  uint64_t where_unused;
  if (!where) where = &where_unused;
  *where = 0;
  if (!out || (!buf && len)) return -4;
  memset(out, 0, sizeof *out);
  if (min_qual < 0 || min_qual > 93) return CFRK_FASTQ_MIN_QUAL;
  // an explicit thread count holds for a text of any size (slices may be empty); the default threads large texts only
  unsigned nthr;
  if (g_parse_threads > 0) {
    nthr = (unsigned)std::min(g_parse_threads, 256);
  } else {
    nthr = std::thread::hardware_concurrency();
    if (nthr > 64) nthr = 64;
    if (nthr < 2 || len < ((size_t)8 << 20)) nthr = 1;
  }
  auto run = [&](auto &&fn) {
    if (nthr == 1) { fn(0u); return; }
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nthr; ++t) pool.emplace_back(fn, t);
    for (auto &th : pool) th.join();
  };
  std::vector<size_t> cut(nthr + 1, len);
  for (unsigned t = 0; t < nthr; ++t) cut[t] = len / nthr * t;
  // pass 1: the newlines of every slice; the lines in front of a slice are the newlines in front of it
  std::vector<uint64_t> lines_before(nthr + 1, 0);
  run([&](unsigned t) {
    uint64_t c = 0;
    for (const char *p = buf + cut[t], *e = buf + cut[t + 1]; p < e;) {
      const char *nl = (const char *)memchr(p, '\n', (size_t)(e - p));
      if (!nl) break;
      ++c; p = nl + 1;
    }
    lines_before[t + 1] = c;
  });
  for (unsigned t = 0; t < nthr; ++t) lines_before[t + 1] += lines_before[t];
  // pass 2: a slice handles the lines that START in it, to their ends; the kind of a line is its number mod 4
  struct Line { size_t pos, n; };
  struct Part { std::vector<Line> seq, qual; uint64_t bad_line = ~(uint64_t)0; };
  std::vector<Part> parts(nthr);
  run([&](unsigned t) {
    Part &pt = parts[t];
    size_t pos = cut[t];
    const size_t stop = cut[t + 1];
    uint64_t line = lines_before[t];
    if (pos >= stop) return;
    if (pos > 0 && buf[pos - 1] != '\n') {                // in the middle of a line that an earlier slice handles
      const char *nl = (const char *)memchr(buf + pos, '\n', stop - pos);
      if (!nl) return;
      pos = (size_t)(nl - buf) + 1; ++line;
    }
    while (pos < stop) {
      const char *nl = (const char *)memchr(buf + pos, '\n', len - pos);
      size_t e = nl ? (size_t)(nl - buf) : len;
      const size_t next = nl ? e + 1 : len;
      if (e > pos && buf[e - 1] == '\r') --e;               // in front of the '\n', or the text's last byte
      switch (line & 3) {
        case 0: if (buf[pos] != '@' && pt.bad_line == ~(uint64_t)0) pt.bad_line = line; break;
        case 1: pt.seq.push_back(Line{pos, e - pos}); break;
        case 2: if (buf[pos] != '+' && pt.bad_line == ~(uint64_t)0) pt.bad_line = line; break;
        default: pt.qual.push_back(Line{pos, e - pos}); break;
      }
      pos = next; ++line;
    }
  });
  for (const Part &pt : parts)
    if (pt.bad_line != ~(uint64_t)0) { *where = pt.bad_line; return (pt.bad_line & 3) ? CFRK_FASTQ_NO_PLUS : CFRK_FASTQ_NO_AT; }
  const uint64_t lines = lines_before[nthr] + ((len > 0 && buf[len - 1] != '\n') ? 1 : 0);
  if (lines & 3) { *where = lines; return CFRK_FASTQ_TRUNCATED; }
  const int64_t nS = (int64_t)(lines >> 2);
  std::vector<Line> seq, qual;
  seq.reserve((size_t)nS); qual.reserve((size_t)nS);
  for (const Part &pt : parts) {
    seq.insert(seq.end(), pt.seq.begin(), pt.seq.end());
    qual.insert(qual.end(), pt.qual.begin(), pt.qual.end());
  }
  if (seq.size() != (size_t)nS || qual.size() != (size_t)nS) return -4;       // (cannot happen: every line has one owner)
  for (int64_t r = 0; r < nS; ++r)
    if (seq[(size_t)r].n != qual[(size_t)r].n) { *where = (uint64_t)r; return CFRK_FASTQ_LENGTHS; }
  int64_t nN = 0;
  for (int64_t r = 0; r < nS; ++r) {
    if (seq[(size_t)r].n > 0x7FFFFFFF) { *where = (uint64_t)r; return CFRK_FASTQ_LONG; }
    nN += (int64_t)seq[(size_t)r].n + 1;
  }
  out->data = (int8_t *)big_alloc((size_t)(nN > 0 ? nN : 1));
  out->start = (int64_t *)big_alloc(sizeof(int64_t) * (size_t)(nS > 0 ? nS : 1));
  out->length = (int32_t *)big_alloc(sizeof(int32_t) * (size_t)(nS > 0 ? nS : 1));
  if (!out->data || !out->start || !out->length) { cfrk_host_free_batch(out); return -4; }
  out->nN = nN; out->nS = nS;
  {
    int64_t w = 0;
    for (int64_t r = 0; r < nS; ++r) {
      out->start[r] = w;
      out->length[r] = (int32_t)seq[(size_t)r].n;
      w += (int64_t)seq[(size_t)r].n + 1;
    }
  }
  // pass 3: encode and mask; records are independent, split by bytes
  const int low = 33 + min_qual;
  auto encode = [&](int64_t r0, int64_t r1) {
    for (int64_t r = r0; r < r1; ++r) {
      const Line s = seq[(size_t)r];
      int8_t *d = out->data + out->start[r];
      encode_bytes(reinterpret_cast<const unsigned char *>(buf) + s.pos, d, s.n);
      if (min_qual > 0) {
        const unsigned char *q = reinterpret_cast<const unsigned char *>(buf) + qual[(size_t)r].pos;
        for (size_t j = 0; j < s.n; ++j)
          if ((int)q[j] < low) d[j] = -1;
      }
      d[s.n] = -1;
    }
  };
  if (nthr < 2) {
    encode(0, nS);
  } else {
    std::vector<std::thread> pool;
    int64_t r0 = 0;
    for (unsigned t = 0; t < nthr; ++t) {
      const int64_t target = nN / nthr * (t + 1);
      int64_t r1 = r0;
      if (t + 1 == nthr) r1 = nS;
      else while (r1 < nS && out->start[r1] < target) ++r1;
      if (r1 > r0) pool.emplace_back(encode, r0, r1);
      r0 = r1;
    }
    for (auto &th : pool) th.join();
  }
  return 0;
}

int cfrk_host_read_fastq(const char *path, int min_qual, cfrk_batch *out, uint64_t *where) {
  // as cfrk_host_read_fasta: a regular file is mapped, anything else (a pipe) is read chunk by chunk
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return -1;
  struct stat st;
  if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0) {
    void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fd, 0);
    if (m != MAP_FAILED) {
      (void)madvise(m, (size_t)st.st_size, MADV_SEQUENTIAL);
      const int rc = cfrk_host_parse_fastq((const char *)m, (size_t)st.st_size, min_qual, out, where);
      munmap(m, (size_t)st.st_size);
      close(fd);
      return rc;
    }
  }
  std::string text;
  char tmp[1 << 16];
  ssize_t n;
  while ((n = read(fd, tmp, sizeof tmp)) > 0) text.append(tmp, (size_t)n);
  close(fd);
  return cfrk_host_parse_fastq(text.data(), text.size(), min_qual, out, where);
}

int cfrk_host_chunk(const cfrk_batch *b, int64_t first, int64_t count, const int8_t **data,
                    int64_t *start_out, const int32_t **length, int64_t *nN) {
  if (!b || first < 0 || count < 0 || first + count > b->nS) return -1;
  if (count == 0) { *data = b->data; *length = b->length; *nN = 0; return 0; }
  const int64_t base = b->start[first];
  int64_t pos = 0;
  for (int64_t i = 0; i < count; ++i) {             // chunk-relative offsets, src/main.cu:191-200
    start_out[i] = pos;
    pos += (int64_t)b->length[first + i] + 1;
  }
  *data = b->data + base;
  *length = b->length + first;
  *nN = pos;
  return 0;
}

// rows [r0, r1) of the dense text; row i > 0 starts with the '\n' that separates it from row i-1
static size_t dense_rows_size(const int32_t *freq, int64_t r0, int64_t r1, int64_t fourk) {
  size_t n = 0;
  for (int64_t i = r0; i < r1; ++i) {
    if (i) ++n;
    for (int64_t b = 0; b < fourk; ++b) {
      int32_t v = freq[i * fourk + b];
      n += len_u64((uint64_t)b) + 2 + (v < 0 ? 1 + len_u64((uint64_t)(-(int64_t)v)) : len_u64((uint64_t)v));
    }
  }
  return n;
}
static char *dense_rows_put(const int32_t *freq, int64_t r0, int64_t r1, int64_t fourk, char *p) {
  for (int64_t i = r0; i < r1; ++i) {
    if (i) *p++ = '\n';
    for (int64_t b = 0; b < fourk; ++b) {
      p = put_u64(p, (uint64_t)b);
      *p++ = ':';
      p = put_i32(p, freq[i * fourk + b]);
      *p++ = ' ';
    }
  }
  return p;
}

size_t cfrk_host_format_dense(const int32_t *freq, int64_t nS, int k, char *buf, size_t cap) {
  return cfrk_host_format_dense_mt(freq, nS, k, buf, cap, 1);
}

size_t cfrk_host_format_dense_mt(const int32_t *freq, int64_t nS, int k, char *buf, size_t cap, int threads) {
  const int64_t fourk = (int64_t)1 << (2 * k);
  (void)cap;
  int T = threads < 1 ? 1 : threads;
  if ((int64_t)T > nS) T = nS > 0 ? (int)nS : 1;
  if (T == 1) {
    if (!buf) return dense_rows_size(freq, 0, nS, fourk);
    return (size_t)(dense_rows_put(freq, 0, nS, fourk, buf) - buf);
  }
  // row ranges per thread: sizes first (the text of a range starts where the previous ends)
  std::vector<size_t> sz((size_t)T);
  std::vector<std::thread> th;
  auto r_of = [&](int t) { return nS * t / T; };
  for (int t = 0; t < T; ++t)
    th.emplace_back([&, t] { sz[(size_t)t] = dense_rows_size(freq, r_of(t), r_of(t + 1), fourk); });
  for (auto &x : th) x.join();
  size_t total = 0;
  std::vector<size_t> off((size_t)T);
  for (int t = 0; t < T; ++t) { off[(size_t)t] = total; total += sz[(size_t)t]; }
  if (!buf) return total;
  th.clear();
  for (int t = 0; t < T; ++t)
    th.emplace_back([&, t] { dense_rows_put(freq, r_of(t), r_of(t + 1), fourk, buf + off[(size_t)t]); });
  for (auto &x : th) x.join();
  return total;
}

size_t cfrk_host_format_sparse(const uint64_t *keys, const uint32_t *counts, uint64_t n, char *buf,
                               size_t cap) {
  if (!buf) {
    size_t s = 0;
    for (uint64_t i = 0; i < n; ++i) s += len_u64(keys[i]) + 1 + len_u64(counts[i]) + 1;
    return s;
  }
  char *p = buf;
  (void)cap;
  for (uint64_t i = 0; i < n; ++i) {
    p = put_u64(p, keys[i]); *p++ = ':';
    p = put_u64(p, counts[i]); *p++ = '\n';
  }
  return (size_t)(p - buf);
}

size_t cfrk_host_format_sparse2(const uint64_t *keys_lo, const uint64_t *keys_hi, const uint32_t *counts,
                                uint64_t n, char *buf, size_t cap) {
  if (!keys_hi) return cfrk_host_format_sparse(keys_lo, counts, n, buf, cap);
  if (!buf) {
    size_t s = 0;
    for (uint64_t i = 0; i < n; ++i) s += len_u64(keys_hi[i]) + 1 + len_u64(keys_lo[i]) + 1 + len_u64(counts[i]) + 1;
    return s;
  }
  char *p = buf;
  (void)cap;
  for (uint64_t i = 0; i < n; ++i) {
    p = put_u64(p, keys_hi[i]); *p++ = ':';
    p = put_u64(p, keys_lo[i]); *p++ = ':';
    p = put_u64(p, counts[i]); *p++ = '\n';
  }
  return (size_t)(p - buf);
}

size_t cfrk_host_format_sparse_mt(const uint64_t *keys_lo, const uint64_t *keys_hi, const uint32_t *counts,
                                  uint64_t n, char *buf, size_t cap, int threads) {
  int T = threads < 1 ? 1 : threads;
  if ((uint64_t)T > n / 65536 + 1) T = (int)(n / 65536 + 1);      // (a thread per 64 K entries at least)
  if (T == 1) return cfrk_host_format_sparse2(keys_lo, keys_hi, counts, n, buf, cap);
  // entry ranges per thread: sizes first (the text of a range starts where the previous one ends)
  auto e_of = [&](int t) { return n * (uint64_t)t / (uint64_t)T; };
  auto part = [&](int t, char *dst) {
    const uint64_t e0 = e_of(t), e1 = e_of(t + 1);
    return cfrk_host_format_sparse2(keys_lo + e0, keys_hi ? keys_hi + e0 : nullptr, counts + e0, e1 - e0, dst, dst ? (size_t)-1 : 0);
  };
  std::vector<size_t> sz((size_t)T), off((size_t)T);
  {
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t) th.emplace_back([&, t] { sz[(size_t)t] = part(t, nullptr); });
    for (auto &x : th) x.join();
  }
  size_t total = 0;
  for (int t = 0; t < T; ++t) { off[(size_t)t] = total; total += sz[(size_t)t]; }
  if (!buf) return total;
  if (cap < total) return 0;
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t) th.emplace_back([&, t] { part(t, buf + off[(size_t)t]); });
  for (auto &x : th) x.join();
  return total;
}

size_t cfrk_host_format_sparse_rows(const int64_t *row_ptr, const uint64_t *keys, const uint32_t *counts, int64_t nS,
                                    char *buf, size_t cap) {
  size_t s = 0;
  char *p = buf;
  (void)cap;
  for (int64_t i = 0; i < nS; ++i) {
    for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
      if (buf) {
        if (e != row_ptr[i]) *p++ = ' ';
        p = put_u64(p, keys[e]); *p++ = ':';
        p = put_u64(p, counts[e]);
      } else {
        s += (e != row_ptr[i] ? 1 : 0) + len_u64(keys[e]) + 1 + len_u64(counts[e]);
      }
    }
    if (buf) *p++ = '\n';
    else s += 1;
  }
  return buf ? (size_t)(p - buf) : s;
}

size_t cfrk_host_format_sparse_rows_mt(const int64_t *row_ptr, const uint64_t *keys, const uint32_t *counts, int64_t nS,
                                       char *buf, size_t cap, int threads) {
  int T = threads < 1 ? 1 : threads;
  if ((int64_t)T > nS / 1024 + 1) T = (int)(nS / 1024 + 1);       // (a thread per 1024 rows at least)
  if (T == 1) return cfrk_host_format_sparse_rows(row_ptr, keys, counts, nS, buf, cap);
  // row ranges per thread: sizes first (the text of a range starts where the previous one ends)
  auto r_of = [&](int t) { return nS * t / T; };
  auto part = [&](int t, char *dst) {
    const int64_t r0 = r_of(t), r1 = r_of(t + 1);
    return cfrk_host_format_sparse_rows(row_ptr + r0, keys, counts, r1 - r0, dst, dst ? (size_t)-1 : 0);
  };
  std::vector<size_t> sz((size_t)T), off((size_t)T);
  {
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t) th.emplace_back([&, t] { sz[(size_t)t] = part(t, nullptr); });
    for (auto &x : th) x.join();
  }
  size_t total = 0;
  for (int t = 0; t < T; ++t) { off[(size_t)t] = total; total += sz[(size_t)t]; }
  if (!buf) return total;
  if (cap < total) return 0;
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t) th.emplace_back([&, t] { part(t, buf + off[(size_t)t]); });
  for (auto &x : th) x.join();
  return total;
}

size_t cfrk_host_format_histo(const uint64_t *hist, uint64_t nbins, const uint32_t *tail_counts, uint64_t n_tail,
                              char *buf, size_t cap) {
  // the tail: one count per key, binned here (sorted, then runs of equal counts)
  std::vector<uint32_t> t(tail_counts, tail_counts + (tail_counts ? n_tail : 0));
  std::sort(t.begin(), t.end());
  size_t j = 0;
  while (j < t.size() && t[j] == 0) ++j;
  size_t s = 0;
  char *p = buf;
  (void)cap;
  auto line = [&](uint64_t c, uint64_t n) {
    if (!n) return;
    if (buf) { p = put_u64(p, c); *p++ = '\t'; p = put_u64(p, n); *p++ = '\n'; }
    else s += len_u64(c) + 1 + len_u64(n) + 1;
  };
  for (uint64_t c = 1; c < (hist ? nbins : 0); ++c) {
    uint64_t n = hist[c];
    while (j < t.size() && t[j] == c) { ++n; ++j; }
    line(c, n);
  }
  while (j < t.size()) {
    const size_t j0 = j;
    while (j < t.size() && t[j] == t[j0]) ++j;
    line(t[j0], j - j0);
  }
  return buf ? (size_t)(p - buf) : s;
}

size_t cfrk_host_format_query(const uint32_t *counts, const int64_t *start, const int32_t *length, int64_t nS, int k,
                              char *buf, size_t cap) {
  size_t s = 0;
  char *p = buf;
  (void)cap;
  for (int64_t i = 0; i < nS; ++i) {
    const int64_t w = (int64_t)length[i] - k + 1;
    for (int64_t j = 0; j < w; ++j) {
      const uint32_t c = counts[start[i] + j];
      if (buf) {
        if (j) *p++ = ' ';
        if (c == 0xFFFFFFFFu) *p++ = '-';
        else p = put_u64(p, c);
      } else {
        s += (j ? 1 : 0) + (c == 0xFFFFFFFFu ? 1 : len_u64(c));
      }
    }
    if (buf) *p++ = '\n';
    else s += 1;
  }
  return buf ? (size_t)(p - buf) : s;
}

size_t cfrk_host_format_read_stats(const void *stats, int64_t nS, char *buf, size_t cap) {
  size_t s = 0;
  char *p = buf;
  (void)cap;
  const char *row = static_cast<const char *>(stats);
  for (int64_t i = 0; i < nS; ++i, row += 32) {
    uint32_t w[6];
    uint64_t sum;
    memcpy(w, row, 24);
    memcpy(&sum, row + 24, 8);
    for (int j = 0; j < 6; ++j) {
      if (buf) { p = put_u64(p, w[j]); *p++ = '\t'; }
      else s += len_u64(w[j]) + 1;
    }
    if (buf) { p = put_u64(p, sum); *p++ = '\n'; }
    else s += len_u64(sum) + 1;
  }
  return buf ? (size_t)(p - buf) : s;
}

size_t cfrk_host_format_fasta(const int8_t *data, const int64_t *start, const int32_t *length, const int64_t *index,
                              int64_t nS, char *buf, size_t cap) {
  size_t s = 0;
  char *p = buf;
  (void)cap;
  for (int64_t j = 0; j < nS; ++j) {
    const uint64_t id = (uint64_t)(index ? index[j] : j);
    const int64_t L = length[j] > 0 ? (int64_t)length[j] : 0;
    if (!buf) { s += 1 + len_u64(id) + 1 + (size_t)L + 1; continue; }
    *p++ = '>';
    p = put_u64(p, id);
    *p++ = '\n';
    const int8_t *r = data + start[j];
    for (int64_t x = 0; x < L; ++x) { const int c = r[x]; *p++ = (c >= 0 && c <= 3) ? "ACGT"[c] : 'N'; }
    *p++ = '\n';
  }
  return buf ? (size_t)(p - buf) : s;
}

// the FASTA of the unitigs; with link_ptr, the L tags of row j behind its header
static size_t format_unitigs(const int8_t *data, const int64_t *start, const int32_t *length, const void *rec, int64_t nS,
                             const int64_t *link_ptr, const void *links, char *buf);

size_t cfrk_host_format_unitigs(const int8_t *data, const int64_t *start, const int32_t *length, const void *rec, int64_t nS,
                                char *buf, size_t cap) {
  (void)cap;
  return format_unitigs(data, start, length, rec, nS, nullptr, nullptr, buf);
}

size_t cfrk_host_format_unitigs_links(const int8_t *data, const int64_t *start, const int32_t *length, const void *rec,
                                      int64_t nS, const int64_t *link_ptr, const void *links, char *buf, size_t cap) {
  (void)cap;
  return format_unitigs(data, start, length, rec, nS, link_ptr, links, buf);
}

// row i of cfrk_unitig_link (8 bytes: to, flags as uint32)
static void get_link(const void *links, int64_t i, uint32_t *to, bool *from_minus, bool *to_minus) {
  uint32_t w[2];
  memcpy(w, (const char *)links + 8 * i, 8);
  *to = w[0]; *from_minus = (w[1] & 1u) != 0; *to_minus = (w[1] & 2u) != 0;
}

static size_t format_unitigs(const int8_t *data, const int64_t *start, const int32_t *length, const void *rec, int64_t nS,
                             const int64_t *link_ptr, const void *links, char *buf) {
  size_t s = 0;
  char *p = buf;
  for (int64_t j = 0; j < nS; ++j) {
    uint64_t kc;
    uint32_t w[2];                                       // n_kmers, flags
    memcpy(&kc, (const char *)rec + 16 * j, 8);
    memcpy(w, (const char *)rec + 16 * j + 8, 8);
    const uint64_t L = length[j] > 0 ? (uint64_t)length[j] : 0, n = w[0] ? w[0] : 1;
    // kc / n to one decimal, halves rounded up, in integers (kc * 10 may pass 2^64)
    const unsigned __int128 tenths = ((unsigned __int128)kc * 10 + n / 2) / n;
    const uint64_t whole = (uint64_t)(tenths / 10), frac = (uint64_t)(tenths % 10);
    const bool circ = (w[1] & 1u) != 0;
    const int64_t l0 = link_ptr ? link_ptr[j] : 0, l1 = link_ptr ? link_ptr[j + 1] : 0;
    if (!buf) {
      s += 1 + len_u64((uint64_t)j) + 6 + len_u64(L) + 6 + len_u64(kc) + 6 + len_u64(whole) + 2 + (circ ? 7 : 0) + 1 + (size_t)L + 1;
      for (int64_t i = l0; i < l1; ++i) {                // " L:<+|->:<v>:<+|->"
        uint32_t to; bool fm, tm;
        get_link(links, i, &to, &fm, &tm);
        s += 7 + len_u64(to);
      }
      continue;
    }
    *p++ = '>';
    p = put_u64(p, (uint64_t)j);
    memcpy(p, " LN:i:", 6); p = put_u64(p + 6, L);
    memcpy(p, " KC:i:", 6); p = put_u64(p + 6, kc);
    memcpy(p, " km:f:", 6); p = put_u64(p + 6, whole);
    *p++ = '.';
    *p++ = (char)('0' + frac);
    if (circ) { memcpy(p, " CL:i:1", 7); p += 7; }
    for (int64_t i = l0; i < l1; ++i) {
      uint32_t to; bool fm, tm;
      get_link(links, i, &to, &fm, &tm);
      memcpy(p, " L:", 3); p[3] = fm ? '-' : '+'; p[4] = ':';
      p = put_u64(p + 5, to);
      *p++ = ':'; *p++ = tm ? '-' : '+';
    }
    *p++ = '\n';
    const int8_t *r = data + start[j];
    for (uint64_t x = 0; x < L; ++x) { const int c = r[x]; *p++ = (c >= 0 && c <= 3) ? "ACGT"[c] : 'N'; }
    *p++ = '\n';
  }
  return buf ? (size_t)(p - buf) : s;
}

// the GFA text; with `support`, "\tRC:i:<c>" behind every L line (cfrk_host_format_gfa_support has the rule for c)
static size_t format_gfa(const int8_t *data, const int64_t *start, const int32_t *length, const void *rec, int64_t nS,
                         const int64_t *link_ptr, const void *links, const uint32_t *support, bool canonical, int k, char *buf) {
  size_t s = 11;                                         // "H\tVN:Z:1.0\n"
  char *p = buf;
  if (buf) { memcpy(p, "H\tVN:Z:1.0\n", 11); p += 11; }
  for (int64_t j = 0; j < nS; ++j) {
    uint64_t kc;
    uint32_t w[2];                                       // n_kmers, flags
    memcpy(&kc, (const char *)rec + 16 * j, 8);
    memcpy(w, (const char *)rec + 16 * j + 8, 8);
    const uint64_t L = length[j] > 0 ? (uint64_t)length[j] : 0, n = w[0] ? w[0] : 1;
    const unsigned __int128 tenths = ((unsigned __int128)kc * 10 + n / 2) / n;      // as in the FASTA header
    const uint64_t whole = (uint64_t)(tenths / 10), frac = (uint64_t)(tenths % 10);
    if (!buf) { s += 2 + len_u64((uint64_t)j) + 1 + (size_t)L + 6 + len_u64(L) + 6 + len_u64(kc) + 6 + len_u64(whole) + 2 + 1; continue; }
    *p++ = 'S'; *p++ = '\t';
    p = put_u64(p, (uint64_t)j);
    *p++ = '\t';
    const int8_t *r = data + start[j];
    for (uint64_t x = 0; x < L; ++x) { const int c = r[x]; *p++ = (c >= 0 && c <= 3) ? "ACGT"[c] : 'N'; }
    memcpy(p, "\tLN:i:", 6); p = put_u64(p + 6, L);
    memcpy(p, "\tKC:i:", 6); p = put_u64(p + 6, kc);
    memcpy(p, "\tkm:f:", 6); p = put_u64(p + 6, whole);
    *p++ = '.';
    *p++ = (char)('0' + frac);
    *p++ = '\n';
  }
  const uint64_t overlap = k > 0 ? (uint64_t)k - 1 : 0;
  for (int64_t j = 0; j < nS; ++j)
    for (int64_t i = link_ptr[j]; i < link_ptr[j + 1]; ++i) {
      uint32_t to; bool fm, tm;
      get_link(links, i, &to, &fm, &tm);
      uint64_t c = 0;
      if (support) {
        c = support[i];
        if (canonical && (int64_t)to < nS)               // the mirror (to,!tm) -> (j,!fm), where it is another row
          for (int64_t x = link_ptr[to]; x < link_ptr[to + 1]; ++x) {
            uint32_t mt; bool mfm, mtm;
            get_link(links, x, &mt, &mfm, &mtm);
            if (mt != (uint32_t)j || mfm == tm || mtm == fm) continue;
            if (x != i) c += support[x];
            break;
          }
      }
      if (!buf) { s += 2 + len_u64((uint64_t)j) + 3 + len_u64(to) + 3 + len_u64(overlap) + 2 + (support ? 6 + len_u64(c) : 0); continue; }
      *p++ = 'L'; *p++ = '\t';
      p = put_u64(p, (uint64_t)j);
      *p++ = '\t'; *p++ = fm ? '-' : '+'; *p++ = '\t';
      p = put_u64(p, to);
      *p++ = '\t'; *p++ = tm ? '-' : '+'; *p++ = '\t';
      p = put_u64(p, overlap);
      *p++ = 'M';
      if (support) { memcpy(p, "\tRC:i:", 6); p = put_u64(p + 6, c); }
      *p++ = '\n';
    }
  return buf ? (size_t)(p - buf) : s;
}

size_t cfrk_host_format_gfa(const int8_t *data, const int64_t *start, const int32_t *length, const void *rec, int64_t nS,
                            const int64_t *link_ptr, const void *links, int k, char *buf, size_t cap) {
  (void)cap;
  return format_gfa(data, start, length, rec, nS, link_ptr, links, nullptr, false, k, buf);
}

size_t cfrk_host_format_gfa_support(const int8_t *data, const int64_t *start, const int32_t *length, const void *rec, int64_t nS,
                                    const int64_t *link_ptr, const void *links, const uint32_t *support, int canonical, int k,
                                    char *buf, size_t cap) {
  (void)cap;
  return format_gfa(data, start, length, rec, nS, link_ptr, links, support, canonical != 0, k, buf);
}

size_t cfrk_host_format_gaf(const int32_t *read_length, int64_t n_reads, const int64_t *hit_ptr, const void *hits,
                            const int32_t *unitig_length, int k, char *buf, size_t cap) {
  (void)cap;
  size_t s = 0;
  char *p = buf;
  const uint64_t k1 = k > 0 ? (uint64_t)k - 1 : 0;
  for (int64_t i = 0; i < n_reads; ++i) {
    const uint64_t rl = read_length[i] > 0 ? (uint64_t)read_length[i] : 0;
    for (int64_t h = hit_ptr[i]; h < hit_ptr[i + 1]; ++h) {
      uint32_t w[4];                                     // unitig, unitig_at, read_off, n_windows
      memcpy(w, (const char *)hits + 16 * h, 16);
      const uint64_t j = w[0], off = w[1] >> 1, a = w[2], m = (uint64_t)w[3] + k1;
      const bool minus = (w[1] & 1u) != 0;
      const uint64_t ln = unitig_length[j] > 0 ? (uint64_t)unitig_length[j] : 0;
      // on the reverse-complemented unitig the hit begins where it ends on the unitig as written
      const uint64_t ps = minus ? (ln >= off + m ? ln - off - m : 0) : off;
      if (!buf) {
        s += len_u64((uint64_t)i) + 1 + len_u64(rl) + 1 + len_u64(a) + 1 + len_u64(a + m) + 3 + 1 + len_u64(j) + 1 + len_u64(ln) + 1 +
             len_u64(ps) + 1 + len_u64(ps + m) + 1 + 2 * (len_u64(m) + 1) + 4 + 5 + len_u64(m) + 2;
        continue;
      }
      p = put_u64(p, (uint64_t)i); *p++ = '\t';
      p = put_u64(p, rl); *p++ = '\t';
      p = put_u64(p, a); *p++ = '\t';
      p = put_u64(p, a + m); *p++ = '\t';
      *p++ = '+'; *p++ = '\t';
      *p++ = minus ? '<' : '>';
      p = put_u64(p, j); *p++ = '\t';
      p = put_u64(p, ln); *p++ = '\t';
      p = put_u64(p, ps); *p++ = '\t';
      p = put_u64(p, ps + m); *p++ = '\t';
      p = put_u64(p, m); *p++ = '\t';
      p = put_u64(p, m); *p++ = '\t';
      memcpy(p, "255\t", 4); p += 4;
      memcpy(p, "cg:Z:", 5); p = put_u64(p + 5, m);
      *p++ = '='; *p++ = '\n';
    }
  }
  return buf ? (size_t)(p - buf) : s;
}

size_t cfrk_host_format_gaf_paths(const int32_t *read_length, int64_t n_reads, const int64_t *hit_ptr, const void *hits,
                                  const int64_t *path_ptr, const void *paths, const int32_t *unitig_length, int k, char *buf, size_t cap) {
  (void)cap;
  size_t s = 0;
  char *p = buf;
  const uint64_t k1 = k > 0 ? (uint64_t)k - 1 : 0;
  for (int64_t i = 0; i < n_reads; ++i) {
    const uint64_t rl = read_length[i] > 0 ? (uint64_t)read_length[i] : 0;
    for (int64_t t = path_ptr[i]; t < path_ptr[i + 1]; ++t) {
      uint32_t w[4];                                     // hit_first, n_hits, read_off, n_windows
      memcpy(w, (const char *)paths + 16 * t, 16);
      const int64_t h0 = hit_ptr[i] + (int64_t)w[0], h1 = h0 + (int64_t)w[1];
      const uint64_t a = w[2], m = (uint64_t)w[3] + k1;
      uint64_t pl = 0, ps = 0;
      size_t names = 0;
      for (int64_t h = h0; h < h1; ++h) {
        uint32_t x[4];                                   // unitig, unitig_at, read_off, n_windows
        memcpy(x, (const char *)hits + 16 * h, 16);
        const uint64_t ln = unitig_length[x[0]] > 0 ? (uint64_t)unitig_length[x[0]] : 0;
        pl += h == h0 ? ln : (ln >= k1 ? ln - k1 : 0);   // every segment after the first overlaps k - 1 bases
        names += 1 + len_u64(x[0]);
        if (h == h0) {                                   // ps of cfrk_host_format_gaf, for the first hit
          const uint64_t off = x[1] >> 1, hm = (uint64_t)x[3] + k1;
          ps = (x[1] & 1u) ? (ln >= off + hm ? ln - off - hm : 0) : off;
        }
      }
      if (!buf) {
        s += len_u64((uint64_t)i) + 1 + len_u64(rl) + 1 + len_u64(a) + 1 + len_u64(a + m) + 3 + names + 1 + len_u64(pl) + 1 +
             len_u64(ps) + 1 + len_u64(ps + m) + 1 + 2 * (len_u64(m) + 1) + 4 + 5 + len_u64(m) + 2;
        continue;
      }
      p = put_u64(p, (uint64_t)i); *p++ = '\t';
      p = put_u64(p, rl); *p++ = '\t';
      p = put_u64(p, a); *p++ = '\t';
      p = put_u64(p, a + m); *p++ = '\t';
      *p++ = '+'; *p++ = '\t';
      for (int64_t h = h0; h < h1; ++h) {
        uint32_t x[2];
        memcpy(x, (const char *)hits + 16 * h, 8);
        *p++ = (x[1] & 1u) ? '<' : '>';
        p = put_u64(p, x[0]);
      }
      *p++ = '\t';
      p = put_u64(p, pl); *p++ = '\t';
      p = put_u64(p, ps); *p++ = '\t';
      p = put_u64(p, ps + m); *p++ = '\t';
      p = put_u64(p, m); *p++ = '\t';
      p = put_u64(p, m); *p++ = '\t';
      memcpy(p, "255\t", 4); p += 4;
      memcpy(p, "cg:Z:", 5); p = put_u64(p + 5, m);
      *p++ = '='; *p++ = '\n';
    }
  }
  return buf ? (size_t)(p - buf) : s;
}

size_t cfrk_host_format_bubbles(uint32_t round, const int8_t *data, const int64_t *start, const int32_t *length, const void *rec,
                                int64_t nS, const uint8_t *pop, const uint32_t *partner, char *buf, size_t cap) {
  (void)cap;
  size_t s = 0;
  char *p = buf;
  for (int64_t j = 0; j < nS; ++j) {
    if (!pop[j] || (int64_t)(partner[j] >> 1) >= nS) continue;          // (a partner that names no unitig: no line)
    const int64_t t = (int64_t)(partner[j] >> 1);
    const bool minus = (partner[j] & 1u) != 0;
    const int64_t at[2] = {j, t};
    uint64_t L[2], whole[2], frac[2];
    for (int i = 0; i < 2; ++i) {
      uint64_t kc;
      uint32_t n;
      memcpy(&kc, (const char *)rec + 16 * at[i], 8);
      memcpy(&n, (const char *)rec + 16 * at[i] + 8, 4);
      if (!n) n = 1;
      const unsigned __int128 tenths = ((unsigned __int128)kc * 10 + n / 2) / n;    // as in the S line
      whole[i] = (uint64_t)(tenths / 10); frac[i] = (uint64_t)(tenths % 10);
      L[i] = length[at[i]] > 0 ? (uint64_t)length[at[i]] : 0;
    }
    const int8_t *a = data + start[j], *b = data + start[t];
    // the kept unitig's base x, oriented like the popped one: 0..3, or 4 for any other code
    auto code = [](int c) { return (c >= 0 && c <= 3) ? c : 4; };
    auto kept = [&](uint64_t x) { const int c = code(minus ? b[L[1] - 1 - x] : b[x]); return (minus && c < 4) ? 3 - c : c; };
    const char *kind = "indel";
    if (L[0] == L[1]) {
      uint64_t differ = 0;
      for (uint64_t x = 0; x < L[0] && differ < 2; ++x) differ += code(a[x]) != kept(x);
      kind = differ == 1 ? "snp" : "mnp";
    }
    const size_t kind_len = strlen(kind);
    if (!buf) {
      s += len_u64(round) + 1 + len_u64((uint64_t)j) + 1 + len_u64((uint64_t)t) + 3 + len_u64(L[0]) + 1 + len_u64(L[1]) + 1 +
           len_u64(whole[0]) + 3 + len_u64(whole[1]) + 3 + kind_len + 1 + (size_t)L[0] + 1 + (size_t)L[1] + 1;
      continue;
    }
    p = put_u64(p, round); *p++ = '\t';
    p = put_u64(p, (uint64_t)j); *p++ = '\t';
    p = put_u64(p, (uint64_t)t); *p++ = '\t';
    *p++ = minus ? '-' : '+'; *p++ = '\t';
    p = put_u64(p, L[0]); *p++ = '\t';
    p = put_u64(p, L[1]); *p++ = '\t';
    for (int i = 0; i < 2; ++i) { p = put_u64(p, whole[i]); *p++ = '.'; *p++ = (char)('0' + frac[i]); *p++ = '\t'; }
    memcpy(p, kind, kind_len); p += kind_len; *p++ = '\t';
    for (uint64_t x = 0; x < L[0]; ++x) *p++ = "ACGTN"[code(a[x])];
    *p++ = '\t';
    for (uint64_t x = 0; x < L[1]; ++x) *p++ = "ACGTN"[kept(x)];
    *p++ = '\n';
  }
  return buf ? (size_t)(p - buf) : s;
}

size_t cfrk_host_format_bulges(uint32_t round, const int8_t *data, const int64_t *start, const int32_t *length, const void *rec,
                               int64_t nS, const uint8_t *pop, const int64_t *path_ptr, const uint32_t *path, int k, char *buf, size_t cap) {
  (void)cap;
  size_t s = 0;
  char *p = buf;
  const uint64_t k1 = k > 1 ? (uint64_t)k - 1 : 0;
  auto code = [](int c) { return (c >= 0 && c <= 3) ? c : 4; };
  std::string spelled;                                  // the path's sequence as codes 0..4
  for (int64_t j = 0; j < nS; ++j) {
    const int64_t a = path_ptr[j], b = path_ptr[j + 1];
    if (!pop[j] || b <= a) continue;
    bool named = true;                                  // (a path entry that names no unitig: no line)
    for (int64_t t = a; t < b; ++t) named = named && (int64_t)(path[t] >> 1) < nS;
    if (!named) continue;
    uint64_t kc, path_kmers = 0;
    uint32_t n;
    memcpy(&kc, (const char *)rec + 16 * j, 8);
    memcpy(&n, (const char *)rec + 16 * j + 8, 4);
    if (!n) n = 1;
    const unsigned __int128 tenths = ((unsigned __int128)kc * 10 + n / 2) / n;    // as in the S line
    const uint64_t whole = (uint64_t)(tenths / 10), frac = (uint64_t)(tenths % 10);
    const uint64_t L = length[j] > 0 ? (uint64_t)length[j] : 0;
    spelled.clear();
    size_t names = 0;
    for (int64_t t = a; t < b; ++t) {
      const int64_t w = (int64_t)(path[t] >> 1);
      const bool minus = (path[t] & 1u) != 0;
      uint32_t wn;
      memcpy(&wn, (const char *)rec + 16 * w + 8, 4);
      path_kmers += wn;
      names += 1 + len_u64((uint64_t)w);
      const uint64_t wl = length[w] > 0 ? (uint64_t)length[w] : 0;
      const int8_t *q = data + start[w];
      for (uint64_t x = (t == a ? 0 : k1); x < wl; ++x) {               // every unitig after the first overlaps k - 1 bases
        const int c = code(minus ? q[wl - 1 - x] : q[x]);
        spelled.push_back((char)((minus && c < 4) ? 3 - c : c));
      }
    }
    const int8_t *own = data + start[j];
    const char *kind = "indel";
    if (L == spelled.size()) {
      uint64_t differ = 0;
      for (uint64_t x = 0; x < L && differ < 2; ++x) differ += code(own[x]) != spelled[x];
      kind = differ == 1 ? "snp" : "mnp";
    }
    const size_t kind_len = strlen(kind);
    if (!buf) {
      s += len_u64(round) + 1 + len_u64((uint64_t)j) + 1 + len_u64(L) + 1 + len_u64(whole) + 3 + len_u64((uint64_t)(b - a)) + 1 +
           len_u64(path_kmers) + 1 + names + 1 + kind_len + 1 + (size_t)L + 1 + spelled.size() + 1;
      continue;
    }
    p = put_u64(p, round); *p++ = '\t';
    p = put_u64(p, (uint64_t)j); *p++ = '\t';
    p = put_u64(p, L); *p++ = '\t';
    p = put_u64(p, whole); *p++ = '.'; *p++ = (char)('0' + frac); *p++ = '\t';
    p = put_u64(p, (uint64_t)(b - a)); *p++ = '\t';
    p = put_u64(p, path_kmers); *p++ = '\t';
    for (int64_t t = a; t < b; ++t) { *p++ = (path[t] & 1u) ? '<' : '>'; p = put_u64(p, (uint64_t)(path[t] >> 1)); }
    *p++ = '\t';
    memcpy(p, kind, kind_len); p += kind_len; *p++ = '\t';
    for (uint64_t x = 0; x < L; ++x) *p++ = "ACGTN"[code(own[x])];
    *p++ = '\t';
    for (size_t x = 0; x < spelled.size(); ++x) *p++ = "ACGTN"[(int)spelled[x]];
    *p++ = '\n';
  }
  return buf ? (size_t)(p - buf) : s;
}

size_t cfrk_host_format_weak(uint32_t round, const int8_t *data, const int64_t *start, const int32_t *length, const void *rec,
                             int64_t nS, const uint8_t *weak, char *buf, size_t cap) {
  (void)cap;
  size_t s = 0;
  char *p = buf;
  for (int64_t j = 0; j < nS; ++j) {
    if (weak[j] != 1 && weak[j] != 2) continue;         // CFRK_WEAK_CONNECTION, CFRK_WEAK_ISOLATED; any other byte: no line
    const char *kind = weak[j] == 1 ? "connection" : "isolated";
    const size_t kind_len = strlen(kind);
    uint64_t kc;
    uint32_t n;
    memcpy(&kc, (const char *)rec + 16 * j, 8);
    memcpy(&n, (const char *)rec + 16 * j + 8, 4);
    if (!n) n = 1;
    const unsigned __int128 tenths = ((unsigned __int128)kc * 10 + n / 2) / n;      // as in the S line
    const uint64_t whole = (uint64_t)(tenths / 10), frac = (uint64_t)(tenths % 10);
    const uint64_t L = length[j] > 0 ? (uint64_t)length[j] : 0;
    if (!buf) {
      s += len_u64(round) + 1 + len_u64((uint64_t)j) + 1 + kind_len + 1 + len_u64(L) + 1 + len_u64(kc) + 1 + len_u64(whole) + 3 + (size_t)L + 1;
      continue;
    }
    p = put_u64(p, round); *p++ = '\t';
    p = put_u64(p, (uint64_t)j); *p++ = '\t';
    memcpy(p, kind, kind_len); p += kind_len; *p++ = '\t';
    p = put_u64(p, L); *p++ = '\t';
    p = put_u64(p, kc); *p++ = '\t';
    p = put_u64(p, whole); *p++ = '.'; *p++ = (char)('0' + frac); *p++ = '\t';
    const int8_t *a = data + start[j];
    for (uint64_t x = 0; x < L; ++x) { const int c = a[x]; *p++ = "ACGTN"[(c >= 0 && c <= 3) ? c : 4]; }
    *p++ = '\n';
  }
  return buf ? (size_t)(p - buf) : s;
}

size_t cfrk_host_format_components(const void *table, int64_t n_comps, int k, char *buf, size_t cap) {
  (void)cap;
  size_t s = 0;
  char *p = buf;
  for (int64_t c = 0; c < n_comps; ++c) {
    uint64_t kc, nk, nl;
    uint32_t first, nu;
    const char *row = (const char *)table + 32 * c;
    memcpy(&kc, row, 8); memcpy(&nk, row + 8, 8); memcpy(&nl, row + 16, 8); memcpy(&first, row + 24, 4); memcpy(&nu, row + 28, 4);
    const uint64_t bases = nk + (uint64_t)nu * (uint64_t)(k > 0 ? k - 1 : 0);
    const uint64_t n = nk ? nk : 1;
    const unsigned __int128 tenths = ((unsigned __int128)kc * 10 + n / 2) / n;      // as in the S line
    const uint64_t whole = (uint64_t)(tenths / 10), frac = (uint64_t)(tenths % 10);
    if (!buf) {
      s += len_u64((uint64_t)c) + 1 + len_u64(first) + 1 + len_u64(nu) + 1 + len_u64(nk) + 1 + len_u64(bases) + 1 + len_u64(kc) + 1 + len_u64(whole) + 3 +
           len_u64(nl) + 1;
      continue;
    }
    p = put_u64(p, (uint64_t)c); *p++ = '\t';
    p = put_u64(p, first); *p++ = '\t';
    p = put_u64(p, nu); *p++ = '\t';
    p = put_u64(p, nk); *p++ = '\t';
    p = put_u64(p, bases); *p++ = '\t';
    p = put_u64(p, kc); *p++ = '\t';
    p = put_u64(p, whole); *p++ = '.'; *p++ = (char)('0' + frac); *p++ = '\t';
    p = put_u64(p, nl); *p++ = '\n';
  }
  return buf ? (size_t)(p - buf) : s;
}

size_t cfrk_host_tag_components(const char *text, size_t n, int gfa, const uint32_t *comp, int64_t nS, char *buf, size_t cap) {
  (void)cap;
  size_t s = 0;
  char *p = buf;
  int64_t j = 0;                                          // the next header / S line's unitig
  for (size_t at = 0; at < n;) {
    const char *nl = (const char *)memchr(text + at, '\n', n - at);
    const size_t end = nl ? (size_t)(nl - text) : n;      // the line is text[at, end), its '\n' (if any) at end
    const bool named = gfa ? (end - at >= 2 && text[at] == 'S' && text[at + 1] == '\t') : (end > at && text[at] == '>');
    size_t cut = end;                                     // where the tag goes: the end of the line, in FASTA before the first L tag
    bool tag = false;
    if (named) {
      tag = j < nS && comp[j] != 0xFFFFFFFFu;
      if (tag && !gfa)
        for (size_t x = at; x + 2 < end; ++x)
          if (text[x] == ' ' && text[x + 1] == 'L' && text[x + 2] == ':') { cut = x; break; }
    }
    const size_t tag_len = tag ? 6 + len_u64(comp[j]) : 0;    // " CC:i:" or "\tCC:i:" and the number
    const size_t whole = (end - at) + tag_len + (nl ? 1 : 0);
    if (!buf) s += whole;
    else {
      memcpy(p, text + at, cut - at); p += cut - at;
      if (tag) { *p++ = gfa ? '\t' : ' '; memcpy(p, "CC:i:", 5); p += 5; p = put_u64(p, comp[j]); }
      memcpy(p, text + cut, end - cut); p += end - cut;
      if (nl) *p++ = '\n';
    }
    if (named) ++j;
    at = end + (nl ? 1 : 0);
  }
  return buf ? (size_t)(p - buf) : s;
}

static void put_le(char *p, uint64_t x, int bytes) { for (int i = 0; i < bytes; ++i) p[i] = (char)(x >> (8 * i)); }
static uint64_t get_le(const char *p, int bytes) {
  uint64_t x = 0;
  for (int i = 0; i < bytes; ++i) x |= (uint64_t)(unsigned char)p[i] << (8 * i);
  return x;
}

size_t cfrk_host_write_binary(int k, int flags, const uint64_t *keys_lo, const uint64_t *keys_hi,
                              const uint32_t *counts, uint64_t n, char *buf, size_t cap) {
  const bool two = k > 32;
  const size_t rec = two ? 20 : 12, need = 32 + (size_t)n * rec;
  if (!buf) return need;
  if (cap < need) return 0;
  memcpy(buf, "CFRKGLB1", 8);
  put_le(buf + 8, (uint64_t)k, 4);
  put_le(buf + 12, (uint64_t)((flags & CFRK_BIN_CANONICAL) | (two ? CFRK_BIN_TWO_WORD : 0)), 4);
  put_le(buf + 16, n, 8);
  uint64_t sum = 0;
  char *p = buf + 32;
  for (uint64_t i = 0; i < n; ++i) {
    if (two) { put_le(p, keys_hi ? keys_hi[i] : 0, 8); p += 8; }
    put_le(p, keys_lo[i], 8); p += 8;
    put_le(p, counts[i], 4); p += 4;
    sum += counts[i];
  }
  put_le(buf + 24, sum, 8);
  return need;
}

int cfrk_host_read_binary(const char *buf, size_t len, int *k, int *flags, uint64_t *n, uint64_t *keys_lo,
                          uint64_t *keys_hi, uint32_t *counts) {
  if (!buf || len < 32 || memcmp(buf, "CFRKGLB1", 8) != 0) return -1;
  const int kk = (int)get_le(buf + 8, 4), ff = (int)get_le(buf + 12, 4);
  const uint64_t nn = get_le(buf + 16, 8);
  const bool two = (ff & CFRK_BIN_TWO_WORD) != 0;
  if (kk < 1 || kk > 64 || two != (kk > 32)) return -1;
  const size_t rec = two ? 20 : 12;
  if (nn > (len - 32) / rec || len != 32 + (size_t)nn * rec) return -1;
  if (k) *k = kk;
  if (flags) *flags = ff;
  if (n) *n = nn;
  const char *p = buf + 32;
  uint64_t sum = 0;
  for (uint64_t i = 0; i < nn; ++i) {
    uint64_t hi = 0;
    if (two) { hi = get_le(p, 8); p += 8; }
    const uint64_t lo = get_le(p, 8); p += 8;
    const uint32_t c = (uint32_t)get_le(p, 4); p += 4;
    if (keys_lo) keys_lo[i] = lo;
    if (keys_hi) keys_hi[i] = hi;
    if (counts) counts[i] = c;
    sum += c;
  }
  return sum == get_le(buf + 24, 8) ? 0 : -1;
}

}  // extern "C"
