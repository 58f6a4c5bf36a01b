// glue.cpp -- the thread coordinates of the CUDA stand-in (cuda.h) and a C entry to the reference's
// kmer_main(); TEST INFRASTRUCTURE ONLY.  Built into oracle/_ref/libcfrk_ref.so next to the reference's
// own kmer_main / kmer_kernel sources, and (with -DREF_GLUE_ENTRY=..., -DREF_GLUE_FREE=free) next to the
// product's kmer_main() of INTEGRATION.md, so that both are called on the same struct.
#include "cuda.h"
#include "tipos.h"
#include "kmer.cuh"

thread_local shim_dim3 threadIdx, blockIdx, blockDim, gridDim;

#ifndef REF_GLUE_ENTRY
#define REF_GLUE_ENTRY ref_kmer_main
#endif
#ifndef REF_GLUE_FREE
#define REF_GLUE_FREE cudaFreeHost      // the reference allocates rd->Freq with cudaMallocHost
#endif

// fills a `struct read` as the reference's callers do, calls kmer_main() and copies rd->Freq
// (nS * 4^k ints) out; the inputs are not modified
extern "C" int REF_GLUE_ENTRY(const signed char *data, const long *start, const int *length, long nN, long nS,
                              int k, int *freq_out) {
  struct read rd;
  rd.data = (char *)data;
  rd.length = (int *)length;
  rd.start = (lint *)start;
  rd.Freq = NULL;
  rd.next = NULL;
  kmer_main(&rd, nN, nS, k, 0);
  if (!rd.Freq) return -1;
  memcpy(freq_out, rd.Freq, (size_t)nS * POW(k) * sizeof(int));
  REF_GLUE_FREE(rd.Freq);
  return 0;
}
