/* cuda.h -- stand-in for the CUDA toolkit header, TEST INFRASTRUCTURE ONLY (see ../Makefile, target
 * `ref`).  With it g++ builds the reference's own sources for the CPU: kernels are ordinary functions,
 * a launch is a serial loop over gridDim.x * blockDim.x (the reference's kernels have no cross-thread
 * dependency but one atomicAdd), device memory is the heap.  Nothing here is taken from the reference.
 *
 * Every allocation carries SHIM_PAD bytes of 0xEE on both sides, so the reference's stray accesses are
 * defined and inert instead of undefined:
 *   - ComputeFreqNew reads Index[start + threadIdx.x] for all 1024 threads before it tests the bound
 *     (src/kmer_kernel.cu:83-85): up to 4 KiB beyond d_Index;
 *   - an invalid window of the FIRST read is added to Freq[-1] (src/kmer_kernel.cu:84,87): the padding
 *     takes it and it is never copied out -- the oracle's "first-read spill dropped";
 *   - an all-T window of the LAST read whose float index rounds up to 4^k (k >= 13) is added to
 *     Freq[nS * 4^k]: likewise.
 * 0xEE is neither 0 nor -1, so a stray read can pass neither for a valid zero nor for the invalid mark.
 * Pinned host allocations carry SHIM_HOST_PAD instead: the reference CLI sizes a chunk's length / start
 * tables by the chunk size NARROWED to unsigned short and fills them by the unnarrowed one
 * (src/main.cu:160,180-181,196-200; 110,130-131,147-151), so with chunkSize = 65536 + 3 it writes 65539
 * entries (512 KiB of longs) behind a 3-entry table and reads them back for the count; the padding makes
 * that a private, consistent piece of memory, as pinned pages evidently were for the reference. */
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

struct shim_dim3 { unsigned x, y, z; };           /* unsigned as in CUDA: `threadIdx.x < length[i]-1` is
                                                     an unsigned comparison (src/kmer_kernel.cu:85) */
extern thread_local shim_dim3 threadIdx, blockIdx, blockDim, gridDim;   /* defined in glue.cpp */
#define __global__

typedef int cudaError_t;
enum { cudaSuccess = 0 };
enum cudaMemcpyKind { cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost };
struct cudaDeviceProp {
  char name[64];
  size_t totalGlobalMem;
  int maxGridSize[3], maxThreadsDim[3], warpSize, maxThreadsPerMultiProcessor;
};

#define SHIM_PAD 8192
#define SHIM_HOST_PAD (1 << 20)
#define SHIM_FILL 0xEE
static inline void *shim_alloc(size_t n, size_t pad) {
  char *b = (char *)malloc(n + 2 * pad);
  if (!b) { fprintf(stderr, "ref shim: out of memory (%zu bytes)\n", n); abort(); }
  memset(b, SHIM_FILL, n + 2 * pad);
  return b + pad;
}
static inline cudaError_t cudaMalloc(void **p, size_t n) { *p = shim_alloc(n, SHIM_PAD); return cudaSuccess; }
static inline cudaError_t cudaMallocHost(void **p, size_t n) { *p = shim_alloc(n, SHIM_HOST_PAD); return cudaSuccess; }
static inline cudaError_t cudaFree(void *p) { if (p) free((char *)p - SHIM_PAD); return cudaSuccess; }
static inline cudaError_t cudaFreeHost(void *p) { if (p) free((char *)p - SHIM_HOST_PAD); return cudaSuccess; }
static inline cudaError_t cudaMemcpy(void *d, const void *s, size_t n, int) { memcpy(d, s, n); return cudaSuccess; }
#define cudaMemcpyAsync cudaMemcpy
static inline cudaError_t cudaSetDevice(int) { return cudaSuccess; }
static inline cudaError_t cudaDeviceReset() { return cudaSuccess; }
static inline cudaError_t cudaGetDeviceCount(int *n) { *n = 1; return cudaSuccess; }
static inline cudaError_t cudaStreamSynchronize(int) { return cudaSuccess; }
static inline cudaError_t cudaGetLastError() { return cudaSuccess; }
static inline const char *cudaGetErrorString(cudaError_t) { return "no error"; }
static inline cudaError_t cudaGetDeviceProperties(cudaDeviceProp *p, int) {
  memset(p, 0, sizeof *p);
  strcpy(p->name, "cpu shim");
  p->totalGlobalMem = (size_t)1 << 40;
  p->maxGridSize[0] = 2147483647;
  p->maxThreadsDim[0] = 1024;
  p->warpSize = 32;
  return cudaSuccess;
}
static inline int atomicAdd(int *a, int v) { int o = *a; *a = o + v; return o; }

/* `K<<<g, b>>>(args)` is rewritten to SHIM_LAUNCH(K, g, b, args) when the sources are copied */
#define SHIM_LAUNCH(K, G, B, ...)                                          \
  do {                                                                     \
    gridDim.x = (unsigned)(G);                                             \
    blockDim.x = (unsigned)(B);                                            \
    for (unsigned b_ = 0; b_ < gridDim.x; ++b_)                            \
      for (unsigned t_ = 0; t_ < blockDim.x; ++t_) {                       \
        blockIdx.x = b_;                                                   \
        threadIdx.x = t_;                                                  \
        K(__VA_ARGS__);                                                    \
      }                                                                    \
  } while (0)

#ifdef SHIM_HOST_MALLOC
/* The reference CLI's FASTA reader appends to fresh malloc memory with strcat and copies a string into
 * a buffer one byte short (src/fastaIO.h:51-52,59-60,62-63): defined only where the heap happens to hand
 * out zeroed, roomy blocks.  Built with -DSHIM_HOST_MALLOC (the CLI only) plain malloc returns zeroed
 * memory with slack behind it, which is that lucky heap made certain (DESIGN.md "Oracle"). */
static inline void *shim_host_malloc(size_t n) { return calloc(1, n + 64); }
#define malloc(n) shim_host_malloc(n)
#endif
