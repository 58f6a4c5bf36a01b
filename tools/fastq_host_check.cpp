// fastq_host_check.cpp -- the host FASTQ parser (cfrk_host_parse_fastq) under the sanitizers, on the CPU, outside pytest.
//
//   python -m tests.fastq_cases --dump cases.bin
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o fastq_host_check tools/fastq_host_check.cpp cfrk_amd/host/cfrk_host.cpp
//   ./fastq_host_check cases.bin
//
// cases.bin holds length-prefixed texts (a little-endian uint64, then the bytes).  Every text is copied into a buffer of
// exactly its size (so that a read past its end is seen) and parsed with 1 and 4 threads at min_qual 0 and 20; the two
// thread counts must agree on the return code, the place and every array.  Prints one summary line; exit status 1 on a
// disagreement or a malformed file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../cfrk_amd/host/cfrk_host.h"

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 1; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
  size_t cases = 0, accepted = 0, refused = 0, bytes = 0;
  for (;;) {
    unsigned char lenb[8];
    const size_t got = fread(lenb, 1, 8, f);
    if (got == 0) break;
    if (got != 8) { fprintf(stderr, "truncated length in case %zu\n", cases); return 1; }
    uint64_t len = 0;
    for (int i = 0; i < 8; ++i) len |= (uint64_t)lenb[i] << (8 * i);
    char *text = (char *)malloc(len ? len : 1);       // exactly len bytes: no slack behind the text
    if (!text || fread(text, 1, len, f) != len) { fprintf(stderr, "truncated text in case %zu\n", cases); return 1; }
    for (int min_qual : {0, 20}) {
      cfrk_batch b[2];
      uint64_t where[2] = {0, 0};
      int rc[2];
      const int threads[2] = {1, 4};
      for (int i = 0; i < 2; ++i) {
        cfrk_host_set_parse_threads(threads[i]);
        rc[i] = cfrk_host_parse_fastq(len ? text : nullptr, len, min_qual, &b[i], &where[i]);
      }
      bool same = rc[0] == rc[1] && where[0] == where[1];
      if (same && rc[0] == 0) {
        same = b[0].nN == b[1].nN && b[0].nS == b[1].nS && !memcmp(b[0].data, b[1].data, (size_t)b[0].nN) &&
               !memcmp(b[0].start, b[1].start, (size_t)b[0].nS * 8) && !memcmp(b[0].length, b[1].length, (size_t)b[0].nS * 4);
        ++accepted;
      } else {
        ++refused;
      }
      for (int i = 0; i < 2; ++i) if (rc[i] == 0) cfrk_host_free_batch(&b[i]);
      if (!same) { fprintf(stderr, "case %zu (min_qual %d): 1 and 4 threads disagree (rc %d / %d, where %llu / %llu)\n", cases, min_qual, rc[0], rc[1],
                           (unsigned long long)where[0], (unsigned long long)where[1]); return 1; }
    }
    free(text);
    ++cases; bytes += len;
  }
  fclose(f);
  printf("fastq_host_check: %zu texts, %zu bytes; %zu parses accepted, %zu refused; 1 and 4 threads agree\n", cases, bytes, accepted, refused);
  return cases ? 0 : 1;
}
