/*
 * cfrk_abi.h -- C ABI of libcfrk_hip.so, the MI355X (gfx950) replacement for the
 * reference's device hot path.
 *
 * What it replaces (paths under /root/reference/):
 *   void kmer_main(struct read *rd, lint nN, lint nS, int k, ushort device);
 *        declared src/kmer.cuh:6, defined src/kmer_main.cu:20-128, called from
 *        src/main.cu:222,294,300; launches SetMatrix / ComputeIndex / ComputeFreqNew
 *        (src/kmer_kernel.cu:6-90).
 *   struct read { char *data; int *length; lint *start; int *Freq; ... }   src/tipos.h:23-30
 *
 * Data contract (identical to struct read):
 *   data    int8 codes, A=0 C=1 G=2 T=3 (src/fastaIO.h:121-140); any other value (the
 *           reference uses -1) is an invalid base AND the per-read terminator
 *           (src/fastaIO.h:96).
 *   length  bases per read, terminator excluded (src/fastaIO.h:98).
 *   start   byte offset of read i in data; start[0]=0,
 *           start[i]=start[i-1]+length[i-1]+1 (src/main.cu:195-200).
 *   nN      bytes in data = sum(length)+nS (src/fastaIO.h:145).
 *   k-mer index = sum_i code[i] * 4^(k-1-i), first base most significant
 *           (src/kmer_kernel.cu:38).
 *
 * Conventions: every function returns CFRK_OK (0) or a negative CFRK_ERR_* code; the
 * library never prints and never calls exit() (the reference does both:
 * src/kmer_main.cu:51-63).  A cfrk_ctx owns one HIP stream and a device memory pool that
 * persists across calls (the reference mallocs/frees per call, src/kmer_main.cu:59-63,
 * 120-124).  Different contexts may be used concurrently from different threads; one
 * context may not.  Plain pointers and sizes only: no torch / C++ types cross this boundary.
 */
#ifndef CFRK_ABI_H
#define CFRK_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CFRK_ABI_VERSION 1

/* error codes */
#define CFRK_OK              0
#define CFRK_ERR_ARG        -1   /* bad argument (k out of range, NULL pointer, negative size) */
#define CFRK_ERR_NOMEM      -2   /* device (or pinned host) allocation failed / would not fit   */
#define CFRK_ERR_HIP        -3   /* a HIP runtime call failed; see cfrk_last_error              */
#define CFRK_ERR_STATE      -4   /* call sequence violated (e.g. add before begin)              */
#define CFRK_ERR_LAYOUT     -5   /* data/start/length inconsistent with the struct-read layout  */
#define CFRK_ERR_TABLE_FULL -6   /* global table overflowed; re-run with a larger capacity_hint */
#define CFRK_ERR_ALIGN      -7   /* device data pointer not 16-byte aligned                      */
#define CFRK_ERR_NO_DEVICE  -8   /* no usable gfx950 device                                      */
#define CFRK_ERR_SMALL_BUF  -9   /* output buffer smaller than the result                        */
#define CFRK_ERR_COUNT_OVERFLOW -10 /* a key occurred 2^32 - 2 times or more: counts are 32-bit and SATURATE at
                                    2^32 - 2 (0xFFFFFFFE) instead of wrapping; finish / digest / export report it */
#define CFRK_ERR_RUNS_REFUSED -11 /* a CFRK_RUNS_ONLY add that does not fit device memory in one pass: nothing was
                                    counted, the job is still empty; count without the flag (leaf / key exchange)   */
#define CFRK_COUNT_MAX 0xFFFFFFFE   /* (an unsigned int: a hexadecimal constant that does not fit int) */

/* flags */
#define CFRK_COMPAT     0x1  /* per-read dense only: reproduce ComputeFreqNew exactly (no -1 guard ->
                                spill into the previous row's last bin, bound length-1, 1024-window
                                cap; src/kmer_kernel.cu:73-90, src/kmer_main.cu:82-83).  Without it:
                                the guarded ComputeFreq semantics (src/kmer_kernel.cu:52-70).        */
#define CFRK_CANONICAL  0x2  /* global and per-read sparse: key = min(kmer, reverse complement)      */
#define CFRK_FORCE_HASH 0x4  /* global only: count with one HBM atomic per occurrence (the general
                                path) even where the minimizer-partitioned LDS path applies          */
#define CFRK_RUNS_ONLY  0x8  /* global only, 16 <= k <= 64: the job partitions and deduplicates ONE add
                                (which must fit device memory in one pass) and stops there; its result
                                leaves through cfrk_global_export_runs_device (multi-GPU exchange)   */
#define CFRK_RUNS_DEFER 0x20  /* with CFRK_RUNS_ONLY (16 <= k <= 64): the add only PARTITIONS -- no
                                deduplication kernel and, when the leaf streams have their fixed stride (a batch that fits
                                one pass that way; not a chunked or count-first add of a two-word job, which needs its
                                read-backs), no host synchronisation at its end (its overflow flags are looked at by the
                                export).  The shard then leaves through the PIPELINED export,
                                cfrk_global_export_runs_async / _wait (deduplication and packing in one kernel per group of
                                leaves), or through cfrk_global_export_runs_device, which deduplicates first.             */
#define CFRK_FLOAT_INDEX 0x10 /* per-read dense only, matters for k = 13..15: the window index is accumulated
                                through float exactly as ComputeIndex does (index += nuc * powf(4, k-1-i),
                                src/kmer_kernel.cu:38), rounding errors, the all-T window's carry into the
                                next row and all -- byte-identical to what the reference computes where the
                                reference is numerically wrong.  Without it: exact integers (for k <= 12 the
                                two agree).  Combine with CFRK_COMPAT for ComputeFreqNew's semantics.        */

typedef struct cfrk_ctx cfrk_ctx;

/* ---- context ------------------------------------------------------------------------- */

/* Replaces cudaSetDevice + GetDeviceProp + per-call cudaMalloc (src/kmer_main.cu:40-63).
 * hip_stream == NULL: the context creates its own non-blocking stream; otherwise it
 * launches on the caller's hipStream_t (e.g. torch.cuda.current_stream().cuda_stream). */
int  cfrk_ctx_create(int device, void *hip_stream, cfrk_ctx **out);
void cfrk_ctx_destroy(cfrk_ctx *ctx);
int  cfrk_abi_version(void);
const char *cfrk_strerror(int code);
const char *cfrk_last_error(const cfrk_ctx *ctx);   /* detail of the last failure on ctx */
int  cfrk_device_count(int *count);
int  cfrk_ctx_sync(cfrk_ctx *ctx);                  /* cudaStreamSynchronize(0) at src/main.cu:223 */

/* plain device buffers on the context's device (for callers without another allocator) */
int  cfrk_device_alloc(cfrk_ctx *ctx, size_t bytes, void **dptr);
int  cfrk_device_free(cfrk_ctx *ctx, void *dptr);
int  cfrk_memcpy_h2d(cfrk_ctx *ctx, void *dst_device, const void *src_host, size_t bytes);
int  cfrk_memcpy_d2h(cfrk_ctx *ctx, void *dst_host, const void *src_device, size_t bytes);
/* cfrk_memcpy_h2d through a ring of pinned staging buffers (64 MB, allocated on the first call and kept by the context),
 * filled by eight host threads.  Synchronous; copies of less than 8 MB take cfrk_memcpy_h2d.  Prefer cfrk_memcpy_h2d: on
 * the MI355X hosts measured the runtime copies ordinary and mapped-file memory at 56 GB/s by itself and
 * this ring reaches 43-46 GB/s.  It is for a host where the runtime's pageable path is the slow one -- measure both
 * (tools/bench_ingest.py, `cfrk --device-parse --text-copy plain|staged`) before choosing it. */
int  cfrk_memcpy_h2d_staged(cfrk_ctx *ctx, void *dst_device, const void *src_host, size_t bytes);
/* Device-to-device copy between two contexts, possibly on different GPUs of the node: over xGMI
 * peer-to-peer (hipMemcpyPeerAsync; peer access is enabled on first use where the topology allows it),
 * enqueued on dst_ctx's stream.  src_ctx's stream is drained first, so whatever src_ctx was asked to
 * write is complete in the copy; the call returns once the copy is enqueued (dst_ctx's later work is
 * ordered behind it).  src_ctx is only read: several threads may copy from one source context at the same time, each
 * into its own dst_ctx, and every failure is reported on dst_ctx (cfrk_last_error(dst_ctx)).  This is the exchange
 * step of a one-process multi-GPU host (the `cfrk` CLI); one process per GPU uses RCCL instead (cfrk_amd/sharded.py). */
int  cfrk_memcpy_peer(cfrk_ctx *dst_ctx, void *dst_device, cfrk_ctx *src_ctx, const void *src_device, size_t bytes);

/* ---- per-read dense counting: the drop-in for kmer_main ------------------------------- */

/* Host buffers in, host buffer out; synchronous like kmer_main (blocking D2H at
 * src/kmer_main.cu:116).  freq_out is CALLER-allocated, nS * 4^k int32 (the reference
 * allocates rd->Freq itself and never frees it, src/kmer_main.cu:115).  1 <= k <= 15
 * (src/tipos.h:5).  Index arithmetic is exact integer for every k (the reference's float
 * accumulation, src/kmer_kernel.cu:38, is exact only for k <= 12). */
int cfrk_per_read_dense(cfrk_ctx *ctx, const int8_t *data, const int64_t *start,
                        const int32_t *length, int64_t nN, int64_t nS, int k, int flags,
                        int32_t *freq_out);

/* Same with every buffer already resident on the context's device; asynchronous on the
 * context stream. */
int cfrk_per_read_dense_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start,
                               const int32_t *d_length, int64_t nN, int64_t nS, int k, int flags,
                               int32_t *d_freq_out);

/* ---- per-read sparse counting: the rows of the dense form without their zeros, 1 <= k <= 32 ---- */

/* For every read its DISTINCT k-mers in ascending order with their multiplicities, as CSR:
 *   row_ptr[0] = 0, row_ptr[i+1] - row_ptr[i] = distinct k-mers of read i, *nnz_out = row_ptr[nS];
 *   keys / counts [row_ptr[i], row_ptr[i+1]) = read i's keys, strictly ascending, and how often each occurs in it.
 * Semantics: the guarded ComputeFreq (src/kmer_kernel.cu:52-70), i.e. cfrk_per_read_dense without CFRK_COMPAT: a
 * window of read i counts iff it starts inside the read and all its k codes are 0..3 (the terminator is an invalid
 * code: no window crosses a read); key = sum code[j] * 4^(k-1-j).  For k <= 15 without flags row i is exactly the
 * non-zero bins of row i of the native dense result -- at 12 bytes per distinct k-mer instead of 4^k * 4 per read, so
 * k = 21 or 31 and chunks of millions of reads are ordinary.  With CFRK_CANONICAL the key is min(key, reverse
 * complement), as in global mode.  Counts are uint32 and cannot saturate (a count never exceeds the read's length).
 * The compat quirks of the dense form (spill into the previous row, length-1 bound, 1024-window cap) and
 * CFRK_FLOAT_INDEX have no sparse form: any flag other than CFRK_CANONICAL is CFRK_ERR_ARG, and so are k < 1, k > 32
 * (two-word keys, k > 32, are out of scope of these calls), negative sizes, a NULL row_ptr / nnz_out and NULL keys or
 * counts with cap > 0.  nS = 0 is fine (row_ptr[0] = 0, nnz 0).
 * cap = entries available in keys and counts.  cap = sum over reads of max(length[i] - k + 1, 0) -- the number of
 * windows -- is always enough.  When nnz > cap the call returns CFRK_ERR_SMALL_BUF: row_ptr and *nnz_out are complete
 * all the same and nothing is written to keys or counts, so a caller can size exactly and call again; keys or counts
 * NULL with cap = 0 is that "sizes only" call.
 * Device form: every buffer on the context's device, no alignment requirement on d_data.  It synchronises ONCE, to
 * read nnz back; it returns with the last kernel (the move of the rows into d_keys / d_counts) enqueued on the context
 * stream.  start / length are not checked: a read whose range does not lie inside [0, nN) gets an empty row; ranges
 * that overlap give undefined rows (never an access outside the buffers).  Temporary device memory: 12 bytes per byte
 * of data, kept in the context's pool.
 * Host form: checks start and length against the terminators in data like cfrk_global_add (CFRK_ERR_LAYOUT), stages
 * through the pool and is synchronous.
 * Neither call touches a global job that is open on the same context.
 * Reads of up to CFRK_SPARSE_FAST_WINDOWS windows are counted in LDS by a group of lanes; longer reads are exact too,
 * on a slower path (one workgroup per read, sorting in device memory). */
#define CFRK_SPARSE_FAST_WINDOWS 2048
int cfrk_per_read_sparse_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                                int64_t nN, int64_t nS, int k, int flags,
                                int64_t *d_row_ptr /* nS+1 */, uint64_t *d_keys, uint32_t *d_counts,
                                uint64_t cap, uint64_t *nnz_out);
int cfrk_per_read_sparse(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length,
                         int64_t nN, int64_t nS, int k, int flags,
                         int64_t *row_ptr, uint64_t *keys, uint32_t *counts, uint64_t cap, uint64_t *nnz_out);

/* ---- global counting: sum over reads of the per-read rows, any 1 <= k <= 64 ------------ */

/* Semantics: the guarded ComputeFreq (src/kmer_kernel.cu:52-70) summed over all reads of all
 * cfrk_global_add calls since begin; a window counts iff its k codes are all valid, so no
 * window crosses a terminator.  Result = set of (key, count), count < 2^32.
 * capacity_hint = expected number of DISTINCT keys (0: library default).  It sizes the result list
 * and the HBM table, and the partitioned paths (k >= 16) read it as the job's shape: a hint above
 * ~2.7e8 makes them share every leaf between several workgroups (~2000 distinct k-mers each; one-
 * and two-word keys alike), and the room a chunked batch's leaf streams get beyond their measured
 * mean grows when the hint says that a leaf holds few distinct runs.  A job that holds far more
 * distinct k-mers than it announced still counts exactly, but splits overfull leaves by key. */
int cfrk_global_begin(cfrk_ctx *ctx, int k, int flags, uint64_t capacity_hint);

/* Host buffers (struct read fields).  start/length may be NULL; when given they are checked
 * against the terminators in data (CFRK_ERR_LAYOUT).  Stages through pinned memory, H2D on the
 * context stream, then counts; returns after the counting kernels are enqueued. */
int cfrk_global_add(cfrk_ctx *ctx, const int8_t *data, const int64_t *start,
                    const int32_t *length, int64_t nN, int64_t nS);

/* Device-resident data (16-byte aligned).  The kernels run on the context stream and the call does not wait for the
 * last of them (cfrk_global_finish / digest / export do), but it is NOT free of host synchronisation: the partitioned
 * paths (k <= 64 without CFRK_FORCE_HASH) read a few words back per add -- the region cursors after the second-level
 * kernel (did anything overflow?) and, for a batch large enough to be counted in chunks, the record count of the first
 * chunk, from which the leaf streams are sized -- each a small D2H copy + hipStreamSynchronize in the middle of the call.
 * A batch whose first chunk is no measure of the rest (sorted or clustered reads, an N-rich or short-read prefix) costs
 * one more partition pass over the input: its leaf streams are then laid out exactly, in a buffer that grows to fit. */
int cfrk_global_add_device(cfrk_ctx *ctx, const int8_t *d_data, int64_t nN);

/* Add pre-counted (key, count) pairs, e.g. another GPU's export received over RCCL.
 * d_keys_hi may be NULL for k <= 32. */
int cfrk_global_merge_device(cfrk_ctx *ctx, const uint64_t *d_keys_lo, const uint64_t *d_keys_hi,
                             const uint32_t *d_counts, int64_t n);

/* Wait for all adds; report the number of distinct keys.  CFRK_ERR_TABLE_FULL if the table
 * overflowed.  CFRK_ERR_COUNT_OVERFLOW if a count saturated: *n_distinct is written all the same
 * and the job can be digested / exported (the same code comes back from those calls, their outputs
 * filled, the saturated counts reading CFRK_COUNT_MAX). */
int cfrk_global_finish(cfrk_ctx *ctx, uint64_t *n_distinct);

/* Sorted ascending by (hi, lo).  keys_hi may be NULL for k <= 32.  cap = entries available.
 * CFRK_ERR_COUNT_OVERFLOW: the arrays are complete, at least one count reads CFRK_COUNT_MAX. */
int cfrk_global_export(cfrk_ctx *ctx, uint64_t *keys_lo, uint64_t *keys_hi, uint32_t *counts,
                       uint64_t cap, uint64_t *n_out);

/* cfrk_global_export restricted to entries with min_count <= count <= max_count (min_count 0 reads as 1; min > max
 * keeps nothing).  Sorted ascending by (hi, lo); *n_out = entries kept; CFRK_ERR_SMALL_BUF when they exceed cap
 * (*n_out set); CFRK_ERR_COUNT_OVERFLOW as cfrk_global_export.  Only the kept entries are sorted and copied. */
int cfrk_global_export_range(cfrk_ctx *ctx, uint32_t min_count, uint32_t max_count, uint64_t *keys_lo,
                             uint64_t *keys_hi, uint32_t *counts, uint64_t cap, uint64_t *n_out);

/* Abundance histogram of the job's result (k-mer spectrum).  hist[c] = distinct keys counted exactly c times for
 * 1 <= c <= nbins-2, hist[nbins-1] = distinct keys counted nbins-1 times or more, hist[0] = 0; sum(hist) = distinct.
 * 2 <= nbins <= 2^24.  Errors as cfrk_global_digest: CFRK_ERR_TABLE_FULL, CFRK_ERR_STATE (before begin, RUNS_ONLY job);
 * CFRK_ERR_COUNT_OVERFLOW with hist filled (saturated keys land in the top bin).  Read-only: may be called any number
 * of times, before or after digest / export.  One read pass over the result on the device; synchronises. */
int cfrk_global_histogram(cfrk_ctx *ctx, uint64_t *hist, uint32_t nbins);

/* Point queries on the job's result: how often does a k-mer occur?  The first query after begin / add / merge builds a
 * read-only lookup index from the result (one synchronisation: the resolve and a stats read); later queries use it
 * until the result changes.  Digest, histogram and export read the same result afterwards.
 *   keys: counts[i] = count of key i (keys_hi may be NULL for k <= 32); a key with bits set at or above 2k reads 0.
 *   reads: counts[p] = count of the k-mer at bases p .. p+k-1 when all k codes are valid, 0 when it is absent,
 *          CFRK_QUERY_NONE otherwise (terminators are invalid codes: no window crosses a read).  nN entries.
 * In a CFRK_CANONICAL job the k-mer is canonicalised first: a k-mer and its reverse complement read the same count.
 * A saturated key reads CFRK_COUNT_MAX ("at least"); queries never return CFRK_ERR_COUNT_OVERFLOW.  Errors:
 * CFRK_ERR_STATE before begin and on a CFRK_RUNS_ONLY job, CFRK_ERR_TABLE_FULL as cfrk_global_digest, CFRK_ERR_ARG
 * for NULL buffers and negative sizes (n = 0 is fine), CFRK_ERR_NOMEM when the index does not fit (the job is kept).
 * The host forms synchronise; cfrk_global_query_reads checks start / length like cfrk_global_add (CFRK_ERR_LAYOUT;
 * both may be NULL) and stages through buffers of its own.  The _device forms return with the lookup kernel enqueued
 * on the context stream; d_data must be 16-byte aligned (CFRK_ERR_ALIGN). */
#define CFRK_QUERY_NONE 0xFFFFFFFF   /* read query: the window holds an invalid base or runs past nN (unsigned, as CFRK_COUNT_MAX) */
int cfrk_global_query(cfrk_ctx *ctx, const uint64_t *keys_lo, const uint64_t *keys_hi, int64_t n, uint32_t *counts);
int cfrk_global_query_device(cfrk_ctx *ctx, const uint64_t *d_keys_lo, const uint64_t *d_keys_hi, int64_t n,
                             uint32_t *d_counts);
int cfrk_global_query_reads(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length,
                            int64_t nN, int64_t nS, uint32_t *counts /* nN entries */);
int cfrk_global_query_reads_device(cfrk_ctx *ctx, const int8_t *d_data, int64_t nN, uint32_t *d_counts);

/* Per-read abundance statistics against the job's result: what cfrk_global_query_reads answers for the windows of a
 * read, reduced on the device to one 32-byte row per read (digital normalisation by the median, error / contamination
 * screening by `below` and `present`, per-read coverage by sum / windows).  Same job, same lookup index, same
 * canonicalisation in a CFRK_CANONICAL job; a saturated key reads CFRK_COUNT_MAX; never CFRK_ERR_COUNT_OVERFLOW.
 * The windows of read i are the starts p in [start[i], start[i] + length[i] - k] whose k codes are all 0..3; a read
 * without one gets an all-zero row.  threshold = 0 gives below = 0 everywhere.  1 <= k <= 64, reads of any length:
 * reads of up to CFRK_STATS_FAST_WINDOWS windows are looked up and reduced by a group of lanes in LDS, longer ones by a
 * workgroup on a slower, exact path.
 * start and length are required.  Errors: CFRK_ERR_STATE before begin and on a CFRK_RUNS_ONLY job, CFRK_ERR_TABLE_FULL
 * and CFRK_ERR_NOMEM as the query calls, CFRK_ERR_ARG for NULL buffers with nS > 0 and negative sizes (nS = 0 is fine).
 * The job stays usable for digest, histogram, export and queries.
 * Device form: no alignment requirement on d_data; start / length are not checked: a read whose range does not lie
 * inside [0, nN) gets a zero row (never an access outside the buffers).  Returns with the last kernel enqueued on the
 * context stream (the index build of a job's first query synchronises).
 * Host form: checks start and length like cfrk_global_add (CFRK_ERR_LAYOUT), stages through the pool, synchronous. */
typedef struct cfrk_read_stats {   /* 32 bytes, no padding */
  uint32_t windows;   /* windows of the read whose k codes are all valid                       */
  uint32_t present;   /* of those: count >= 1                                                  */
  uint32_t below;     /* of those: count < threshold (an absent k-mer counts 0)                */
  uint32_t min, median, max;   /* over the `windows` counts; median = LOWER median:           */
                               /* element (windows-1)/2 of the counts sorted ascending         */
  uint64_t sum;       /* sum of the counts (saturated keys add CFRK_COUNT_MAX)                 */
} cfrk_read_stats;
#define CFRK_STATS_FAST_WINDOWS 2048
int cfrk_global_read_stats_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                                  int64_t nN, int64_t nS, uint32_t threshold, cfrk_read_stats *d_out);
int cfrk_global_read_stats(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length,
                           int64_t nN, int64_t nS, uint32_t threshold, cfrk_read_stats *out);

/* Solid spans: which part of each read the job's counts support (the trim rule of filter-abund / trim-low-abund).
 * The windows of read i are those of cfrk_global_read_stats: the starts p in [0, length[i] - k] relative to the read.
 * A window is SOLID iff its k codes are all 0..3 and its count c satisfies min_count <= c <= max_count; the count comes
 * from the same lookup index as the read query, canonicalised in a CFRK_CANONICAL job; an absent k-mer counts 0, a
 * saturated key reads CFRK_COUNT_MAX.  There are no special cases: min_count = 0 makes every valid window solid,
 * min_count > max_count makes none solid and is not an error.
 * A run of solid windows a..b gives the span {a, (b - a + 1) + k - 1}: bases [offset, offset + length) of the read.
 *   CFRK_SPAN_PREFIX   the run that begins at window 0 (empty when window 0 is not solid)
 *   CFRK_SPAN_LONGEST  the longest run, the earliest one on a tie
 * A read without a solid window -- every read shorter than k -- gets {0, 0}.  A span never holds an invalid code and
 * holds at least k bases when it is not empty.  1 <= k <= 64, reads of any length: reads of up to
 * CFRK_SPANS_FAST_WINDOWS windows are looked up and reduced by a group of lanes in LDS, longer ones by a workgroup.
 * Errors and job state are those of cfrk_global_read_stats: CFRK_ERR_STATE before begin and on a CFRK_RUNS_ONLY job,
 * CFRK_ERR_TABLE_FULL and CFRK_ERR_NOMEM as the query calls, CFRK_ERR_ARG for NULL buffers with nS > 0, negative sizes
 * and a mode other than the two (nS = 0 is fine).  The job stays usable for digest, histogram, export and queries.
 * Device form: no alignment requirement; start / length are not checked: a read whose range does not lie inside
 * [0, nN) gets {0, 0} (never an access outside the buffers).  Returns with the last kernel enqueued on the context
 * stream (the index build of a job's first query synchronises).
 * Host form: checks start and length like cfrk_global_add (CFRK_ERR_LAYOUT), stages through the pool, synchronous. */
typedef struct cfrk_read_span {   /* 8 bytes: bases [offset, offset + length) of the read */
  int32_t offset;
  int32_t length;
} cfrk_read_span;
#define CFRK_SPAN_PREFIX 0
#define CFRK_SPAN_LONGEST 1
#define CFRK_SPANS_FAST_WINDOWS 2048
int cfrk_global_read_spans_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                                  int64_t nN, int64_t nS, uint32_t min_count, uint32_t max_count, int mode,
                                  cfrk_read_span *d_out);
int cfrk_global_read_spans(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length,
                           int64_t nN, int64_t nS, uint32_t min_count, uint32_t max_count, int mode,
                           cfrk_read_span *out);

/* Spectral correction of substitution errors: the base that a counted spectrum supports is written back where one wrong
 * base explains an isolated stretch of weak windows (the rule of Quake, Musket, Lighter and BFC, without state between
 * reads).  A read has L bases, codes c[0..L), and windows w = 0 .. W-1 with W = L - k + 1: the windows of
 * cfrk_global_read_stats.  The count comes from the job's index, canonicalised in a CFRK_CANONICAL job; an absent k-mer
 * counts 0, a saturated key reads CFRK_COUNT_MAX.
 *   A window is INVALID when one of its k codes is not 0..3.  A valid window is SOLID when count >= min_count and WEAK
 *   otherwise.  A WEAK RUN [a, b] is a maximal stretch of consecutive weak windows, of n = b - a + 1 windows.  Its left
 *   neighbour is none (a == 0), solid or invalid; its right neighbour is none (b == W-1), solid or invalid.
 * A run is ATTEMPTED in exactly three cases; each names one position p, and all windows of the run contain p:
 *   interior   left solid, right solid, n == k    p = b
 *   head       left none,  right solid, n <= k    p = b
 *   tail       left solid, right none,  n <= k    p = a + k - 1
 * Every other run is not attempted: n > k, an interior run shorter than k, a run with an invalid neighbour, a run that
 * is the whole read (left none and right none).
 * For an attempted run, take each of the three bases x != c[p].  Base x PASSES iff every window of [a, b], read with c[p]
 * replaced by x, has count >= min_count.  If exactly one x passes, the output read has x at p and the run is FIXED; with
 * none or more than one, nothing is written.
 * Every run is judged against the ORIGINAL read.  Two attempted runs never share a base (their positions lie at least
 * k + 1 apart, because a non-weak window separates them), so the result does not depend on any order.  min_count = 0
 * makes nothing weak and the output equals the input.  Indels are out of scope; two errors within k bases of each other
 * give one run longer than k and are left alone.
 * Output: data_out is data, byte for byte (terminators and bytes that belong to no read included), except the corrected
 * bases; start and length do not change.  data_out must not overlap data.  fix (may be NULL) gets one row per read.
 * 1 <= k <= 64, reads of any length: reads of up to CFRK_SPANS_FAST_WINDOWS windows are handled by a group of lanes in
 * LDS, longer ones by a workgroup on a slower, exact path.  No temporary device memory beyond the job's index.
 * Errors and job state are those of cfrk_global_read_spans: CFRK_ERR_STATE before begin and on a CFRK_RUNS_ONLY job,
 * CFRK_ERR_TABLE_FULL and CFRK_ERR_NOMEM as the query calls, CFRK_ERR_ARG for negative sizes, for NULL data / start /
 * length with nS > 0 and for NULL data_out with nN > 0.  nS = 0 still copies the bytes.  The job is only read: its digest
 * is the same before and after.
 * Device form: no alignment requirement; start / length are not checked: a read whose range does not lie inside
 * [0, nN) gets {0, 0} and its bytes are only copied (never an access outside the buffers).  The copy and the kernels are
 * enqueued on the context stream; returns with the last kernel enqueued (the index build of a job's first query
 * synchronises).
 * Host form: checks start and length like cfrk_global_add (CFRK_ERR_LAYOUT), stages through the pool, synchronous. */
typedef struct cfrk_read_fix {   /* 8 bytes, no padding */
  uint32_t fixed;   /* weak runs of the read that were corrected (= bases changed)          */
  uint32_t left;    /* weak runs that were not: not attempted, no base passed, or ambiguous */
} cfrk_read_fix;
int cfrk_global_correct_reads_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                                     int64_t nN, int64_t nS, uint32_t min_count,
                                     int8_t *d_data_out /* nN bytes */, cfrk_read_fix *d_fix /* nS rows, may be NULL */);
int cfrk_global_correct_reads(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length,
                              int64_t nN, int64_t nS, uint32_t min_count, int8_t *data_out, cfrk_read_fix *fix);

/* Digital normalisation (normalize-by-median): the reads of the call are counted into the job ONLY while the k-mers they
 * carry are still rare among the reads kept so far, and keep[i] says which were.  The reads are taken in rounds of
 * batch_reads consecutive reads; round r holds the reads [r * batch_reads, min((r + 1) * batch_reads, nS)).
 *   judge    every read of the round against the job's counts as they stand at the beginning of the round: everything
 *            added, merged or normalised into the job before, plus the kept reads of this call's earlier rounds.  The
 *            windows of read i are those of cfrk_global_read_stats (the starts p in [start[i], start[i] + length[i] - k]
 *            whose k codes are all 0..3, canonicalised in a CFRK_CANONICAL job); an absent k-mer counts 0, a saturated
 *            key reads CFRK_COUNT_MAX.  The read is KEPT iff it has a valid window and the lower median of its windows'
 *            counts (cfrk_read_stats.median) is below cutoff.
 *   insert   every valid window of every kept read of the round adds 1 to its key (saturating, as an add).
 * batch_reads = 1 is the streaming rule of khmer's normalize-by-median, with exact counts; a larger batch can over-admit
 * only reads of one round that cover the same locus, and is faster.  cutoff = 0 keeps nothing, cutoff = 0xFFFFFFFF keeps
 * every read with a valid window.  Keep bytes and counts do not depend on scheduling.  1 <= k <= 64, reads of any length.
 * A result held by a partitioned path is folded into the HBM table first, as cfrk_global_merge_device does, so the table
 * must have room for it (capacity_hint).  After the call the job is an ordinary job that also holds the counts of the
 * kept reads: finish, digest, export, histogram, queries, read statistics and spans, further adds, merges and
 * normalise calls all work on it.
 * Errors: CFRK_ERR_STATE before begin and on a CFRK_RUNS_ONLY job; CFRK_ERR_ARG for negative sizes, batch_reads < 1, a
 * NULL n_kept and NULL arrays with nS > 0 (nS = 0 is fine: *n_kept = 0, nothing changes); CFRK_ERR_TABLE_FULL when the
 * table overflowed during the call: the keep bytes of the rounds judged after the overflow are unspecified, nothing
 * outside the buffers is accessed, and finish / digest report the same code.
 * Device form: no alignment requirement; start / length are not checked: a read whose range does not lie inside
 * [0, nN) gets keep 0 (never an access outside the buffers).  Every keep byte is written (0 or 1).  All rounds are
 * enqueued on the context stream without a host synchronisation between them; the call synchronises once at the end
 * for *n_kept and the overflow flag.
 * Host form: checks start and length like cfrk_global_add (CFRK_ERR_LAYOUT), stages through the pool, synchronous. */
#define CFRK_NORMALIZE_BATCH 262144  /* what the Python and CLI layers pass when the caller names no batch */
int cfrk_global_normalize_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                                 int64_t nN, int64_t nS, uint32_t cutoff, int64_t batch_reads,
                                 uint8_t *d_keep /* nS bytes, 0 or 1 */, int64_t *n_kept);
int cfrk_global_normalize(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length,
                          int64_t nN, int64_t nS, uint32_t cutoff, int64_t batch_reads,
                          uint8_t *keep, int64_t *n_kept);

/* Paired normalisation: cfrk_global_normalize for interleaved paired-end reads, the mates of pair j being reads 2j and
 * 2j + 1 (the pairs section below; mode is CFRK_PAIR_EITHER or CFRK_PAIR_BOTH).  Each round
 *   judges   every mate on its own, exactly as above (the mates of a pair may fall into different size classes);
 *   joins    the two verdicts of every pair of the round: CFRK_PAIR_EITHER keeps both mates if either would be kept
 *            (khmer's normalize-by-median --paired), CFRK_PAIR_BOTH keeps both only if both would be; keep[2j] ==
 *            keep[2j + 1] afterwards;
 *   inserts  every valid window of every kept read, as above.  A mate without a valid window that is kept through its
 *            partner inserts nothing.
 * *n_kept counts reads and is even.  Everything else -- rounds, job state, scheduling independence, errors, the device
 * form's unchecked ranges, the single synchronisation at the end -- is that of cfrk_global_normalize; in addition an odd
 * nS or an odd batch_reads is CFRK_ERR_ARG (a round always holds whole pairs), and so is a mode other than the two. */
int cfrk_global_normalize_pairs_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                                       int64_t nN, int64_t nS, uint32_t cutoff, int64_t batch_reads, int mode,
                                       uint8_t *d_keep /* nS bytes, 0 or 1 */, int64_t *n_kept);
int cfrk_global_normalize_pairs(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length,
                                int64_t nN, int64_t nS, uint32_t cutoff, int64_t batch_reads, int mode,
                                uint8_t *keep, int64_t *n_kept);

/* ---- unitigs: the compacted de Bruijn graph of the counted k-mers ---------------------------------------------- */

/* Definitions.  The job has k (1 <= k <= 64) and a strand rule; min_count >= 1 (0 reads as 1).
 *   Solid keys: the stored keys with count >= min_count that are not masked ("Graph mask", below; without a mask call
 *   no key is masked).
 *   Oriented k-mers O: the solid keys; in a CFRK_CANONICAL job every solid key x and rc(x).
 *   node(a) = a, or min(a, rc(a)) in a canonical job.  a is palindromic iff the job is canonical and a == rc(a).
 *   succ(a) = { a[1:] + b in O },  pred(a) = { b + a[:-1] in O }.
 *   LINK a -> b iff succ(a) = {b}, pred(b) = {a}, node(a) != node(b) (no self-loops, no hairpins x -> rc(x)) and neither
 *   a nor b is palindromic.  Links form disjoint directed paths and cycles over O; in a canonical job every component
 *   has a distinct mirror image (the two exclusions are exactly what rules out a component that is its own mirror).
 * A UNITIG is one component, written once:
 *   path a1 -> ... -> an: as it stands; in a canonical job, of the path and its mirror the one whose first k-mer is
 *     smaller (a1 < rc(an)); a single palindromic node is written once.
 *   cycle: cut so that it starts at the smallest oriented k-mer of the cycle (canonical: and of its mirror); flagged
 *     CFRK_UNITIG_CIRCULAR.
 *   Sequence = a1 followed by the last base of every further k-mer: n_kmers + k - 1 bases.  kc = the sum of the n_kmers
 *   stored counts.  Every solid key lies in exactly one unitig, once.
 *   ORDER: ascending by first k-mer (first base most significant, A < C < G < T).  First k-mers are distinct, so this is
 *   the ascending lexicographic order of the sequences: one deterministic byte string for a given result.
 * Output: the struct-read layout of the parsers and of cfrk_reads_select -- codes 0..3, one -1 terminator behind each
 *   unitig, start_out[j], length_out[j] (bases), rec_out[j] -- so that it goes straight into cfrk_global_add_device,
 *   cfrk_per_read_sparse_device, the select, or a count at another k.  *nS_out = unitigs, *nN_out = bases + *nS_out.
 * Capacities: *nS_out <= solid keys and *nN_out <= solid keys * (k + 1) always.  When *nN_out > cap_data or *nS_out >
 *   cap_unitigs the call returns CFRK_ERR_SMALL_BUF with both sizes complete and nothing written to the arrays; NULL
 *   arrays with zero capacities are that "sizes only" call.
 * State: that of cfrk_global_query -- the lookup index is built on demand (and kept), the job is untouched, its digest
 *   is the same before and after; adds may follow.  CFRK_ERR_STATE: no job, or a CFRK_RUNS_ONLY job.
 * CFRK_ERR_ARG: NULL size outputs, a NULL array with a capacity above 0, 2^32 unitigs or more, an index of more than
 *   2^31 slots.  CFRK_ERR_LAYOUT: a unitig of more than 2^31 - 1 bases.  No alignment requirement on data_out.
 * Device form: seven stages, every one its own launches on the context stream (cfrk_amd/csrc/unitigs.hip): neighbour
 *   bytes; links, cut at "splitter" nodes (a 2^-s sample of the keys by hash); segments between cuts walked one lane
 *   each; segments stitched to unitigs one lane per unitig; cycles; the sort by first k-mer and the scan of the
 *   lengths; the emit, one lane per segment.  No lane's work grows with the longest unitig beyond its number of
 *   segments (n_kmers / 2^s).  It synchronises ONCE, for the sizes, and returns with the emit enqueued.
 *   Temporary device memory, kept in the context's pool, per slot of the lookup index (2^ceil(log2(2 * keys)) slots,
 *   4^k for k <= 12): 11 bytes + per orientation (2 in a canonical job, else 1) 32 bytes (64 for k <= 12) + 20 bytes
 *   (40 for k <= 12), i.e. 95 bytes per slot for a canonical job of k > 12; 20 bytes per unitig and the sort's scratch.
 * Host form: stages through the pool; synchronous.
 *
 * Neighbour masks.  Key i is taken as an oriented k-mer exactly as given (it need not be present itself):
 *   bit b (0..3) of masks[i] is set iff key[1:] + b is present with count >= min_count, bit 4 + b iff b + key[:-1] is;
 *   a canonical job canonicalises the NEIGHBOUR for the lookup; a key with bits at or above 2k gives 0.
 *   keys_hi may be NULL for k <= 32.  State and errors as cfrk_global_query; the device form returns with the kernel
 *   enqueued. */
typedef struct {
  uint64_t kc;        /* sum of the stored counts of the unitig's k-mers */
  uint32_t n_kmers;   /* its k-mers: length - k + 1                      */
  uint32_t flags;     /* CFRK_UNITIG_*                                   */
} cfrk_unitig;        /* 16 bytes */
#define CFRK_UNITIG_CIRCULAR 0x1
#define CFRK_UNITIG_SPLIT_LOG2_DEFAULT 10   /* s: one key in 2^s is a splitter */
int cfrk_global_neighbors_device(cfrk_ctx *ctx, const uint64_t *d_keys_lo, const uint64_t *d_keys_hi, int64_t n,
                                 uint32_t min_count, uint8_t *d_masks);
int cfrk_global_neighbors(cfrk_ctx *ctx, const uint64_t *keys_lo, const uint64_t *keys_hi, int64_t n,
                          uint32_t min_count, uint8_t *masks);
int cfrk_global_unitigs_device(cfrk_ctx *ctx, uint32_t min_count, int8_t *d_data_out, uint64_t cap_data,
                               int64_t *d_start_out, int32_t *d_length_out, cfrk_unitig *d_rec_out, uint64_t cap_unitigs,
                               int64_t *nN_out, int64_t *nS_out);
int cfrk_global_unitigs(cfrk_ctx *ctx, uint32_t min_count, int8_t *data_out, uint64_t cap_data, int64_t *start_out,
                        int32_t *length_out, cfrk_unitig *rec_out, uint64_t cap_unitigs, int64_t *nN_out,
                        int64_t *nS_out);

/* Unitig links: the edges of the compacted graph.  The job, k, the strand rule, min_count, the solid keys, O, rc, succ
 * and pred are those above.  The input is the unitig list of this job at this min_count as cfrk_global_unitigs wrote
 * it: unitig j has the sequence s_j of length[j] >= k codes at start[j].
 *   Orientations: + and - of every unitig in a canonical job, + alone otherwise.
 *   head(j,+) = s_j[0:k], tail(j,+) = s_j[len-k:len], head(j,-) = rc(tail(j,+)), tail(j,-) = rc(head(j,+)).
 *   LINK (u,ou) -> (v,ov) iff head(v,ov) is in succ(tail(u,ou)): tail(u,ou)[1:] + b == head(v,ov) for a base b, that
 *   k-mer being in O.  The overlap is always k - 1 bases.  This is the plain set, with no special cases; it follows that
 *   - every k-mer of succ(tail(u,ou)) is the head of at least one oriented unitig (a tail has no out-link, so its
 *     successors have no in-link), and of two only when it is a palindromic single-node unitig: then (v,+) and (v,-)
 *     are both targets;
 *   - a CFRK_UNITIG_CIRCULAR unitig has the link (j,+) -> (j,+), in a canonical job (j,-) -> (j,-) as well (GFA's way
 *     to state a circle); a homopolymer node has (j,+) -> (j,+), a hairpin x -> rc(x) gives (j,+) -> (j,-);
 *   - in a canonical job the mirror (v,!ov) -> (u,!ou) of every link is a link as well; both are written, as BCALM does;
 *   - an oriented end has at most 8 links (4 bases x 2): n_links <= 16 nS in a canonical job, <= 4 nS otherwise.
 * Output: CSR over unitigs.  link_ptr[0] = 0, link_ptr[j + 1] - link_ptr[j] = links out of unitig j, *n_links_out =
 *   link_ptr[nS]; links[] holds rows of cfrk_unitig_link.  Inside row j the links out of (j,+) come before those out of
 *   (j,-); within an end they ascend by the appended base b (A < C < G < T); for one b the target + comes before -.
 *   One byte string for a given result.
 * Capacity (the select's protocol): when n_links > cap_links the call returns CFRK_ERR_SMALL_BUF with link_ptr and
 *   *n_links_out complete and nothing written to links; NULL links with cap_links 0 is that "sizes only" call.
 * State: that of cfrk_global_unitigs -- the index is built on demand and kept, the job is only read (same digest before
 *   and after), adds may follow.  CFRK_ERR_STATE: no job, or a CFRK_RUNS_ONLY job.
 * CFRK_ERR_ARG: negative sizes, NULL n_links_out, NULL link_ptr, NULL data / start / length with nS > 0, NULL links with
 *   cap_links > 0, nS >= 2^32, an index of more than 2^31 slots.  nS = 0 is fine: link_ptr[0] = 0, no links.
 * Consistency check (cheap; necessary, not sufficient): CFRK_ERR_LAYOUT, cfrk_last_error naming the first offending
 *   unitig, when some unitig has length < k or a range outside [0, nN), an invalid code in an end window, an end k-mer
 *   that is not solid at min_count, an end node another unitig end of the input claims as well, or a solid successor of
 *   a tail that is the head of no oriented unitig of the input: unitigs of another job or threshold, edited sequences.
 *   Named is the first unitig whose own ends are wrong; when there is none, the first with such a successor.
 *   The error is found before the sizes are known and wins over CFRK_ERR_SMALL_BUF; after it the arrays are
 *   unspecified.  For any input whatever nothing outside the buffers is accessed and no loop is unbounded.
 * Device form (cfrk_amd/csrc/unitig_links.hip): no alignment requirement on d_data, all offsets 64-bit.  A tag pass (one
 *   lane per unitig end writes the unitig and four end bits at the end node's index slot), a count pass (one lane per
 *   oriented end: at most 4 successor lookups), a scan into link_ptr, and a fill pass.  No lane's work depends on a
 *   unitig's length beyond its 2k end bases.  It synchronises ONCE, for n_links and the error word, and returns with
 *   the fill pass enqueued.  Temporary device memory, kept in the context's pool: 8 bytes per slot of the lookup index
 *   and 8 bytes per oriented unitig plus the scan's scratch.
 * Host form: stages through the pool, checks start / length against the terminators as cfrk_global_add does
 *   (CFRK_ERR_LAYOUT); synchronous. */
typedef struct cfrk_unitig_link {   /* 8 bytes, no padding */
  uint32_t to;      /* target unitig v */
  uint32_t flags;   /* bit 0 (CFRK_LINK_FROM_MINUS): the link leaves (j,-); bit 1 (CFRK_LINK_TO_MINUS): it enters (v,-) */
} cfrk_unitig_link;
#define CFRK_LINK_FROM_MINUS 0x1
#define CFRK_LINK_TO_MINUS 0x2
int cfrk_global_unitig_links_device(cfrk_ctx *ctx, uint32_t min_count, const int8_t *d_data, const int64_t *d_start,
                                    const int32_t *d_length, int64_t nN, int64_t nS, int64_t *d_link_ptr /* nS + 1 */,
                                    cfrk_unitig_link *d_links, uint64_t cap_links, int64_t *n_links_out);
int cfrk_global_unitig_links(cfrk_ctx *ctx, uint32_t min_count, const int8_t *data, const int64_t *start,
                             const int32_t *length, int64_t nN, int64_t nS, int64_t *link_ptr /* nS + 1 */,
                             cfrk_unitig_link *links, uint64_t cap_links, int64_t *n_links_out);

/* Unitig positions and read hits: where a k-mer, and therefore a read, lies on the graph.  The job, k, the strand rule,
 * min_count, the solid keys, O, rc and node() are those above; the input of cfrk_global_unitig_index is the unitig list
 * of this job at this min_count as cfrk_global_unitigs wrote it.  Unitig j has the sequence s_j and n_j = length[j] - k
 * + 1 k-mers, kmer(j,p) = s_j[p : p+k] for 0 <= p < n_j.
 *   POSITION of an oriented k-mer x, taken exactly as given: NONE when x is not in O (the key is absent, counted below
 *   min_count, or has bits at or above 2k).  Otherwise there is exactly one (j,p) with node(kmer(j,p)) = node(x), every
 *   solid key lying in one unitig once, and the position is (j, p, minus): minus = 0 iff x == kmer(j,p), 1 iff x ==
 *   rc(kmer(j,p)) != x.  minus is always 0 in a job that is not canonical.  A palindromic k-mer is a single-node unitig
 *   (links exclude palindromes): p = 0, minus = 0, no special case anywhere.  As cfrk_unitig_pos: at = p << 1 | minus;
 *   NONE is both words 0xFFFFFFFF (CFRK_POS_NONE).  p < 2^31 because a unitig has at most 2^31 - 1 bases.
 *   HITS of a read.  The windows w = 0 .. W-1 are those of cfrk_global_read_stats; pos(w) is the position of the
 *   window's k-mer as the read spells it, NONE when a code is invalid.  Windows w and w+1 are COLINEAR iff both are
 *   located, on the same unitig with the same minus, and p(w+1) = p(w) + 1 (minus = 0) or p(w) - 1 (minus = 1); there is
 *   no wrap-around.  A HIT is a maximal stretch a..b of windows in which every two neighbours are colinear; its row is
 *   cfrk_read_hit with unitig_at = off << 1 | minus, off = min(p(a), p(b)), read_off = a, n_windows = b - a + 1.  So
 *   read bases [a, a + n + k - 1) equal s_j[off : off + n + k - 1], or its reverse complement when minus is set.  The
 *   n_windows of a read's hits sum to its windows whose k-mer is in O; hits ascend by read_off and do not overlap in
 *   windows; a read that crosses the cut of a circular unitig gives two hits; a read of fewer than k bases gives none.
 * cfrk_global_unitig_index builds the position map: one cfrk_unitig_pos per slot of the lookup index, kept by the
 *   context.  It is valid until the job's result changes (any add, merge or normalise call, a new job) or it is built
 *   again; it dies with the lookup index.  The job is only read: same digest before and after.  nS = 0 is fine for a
 *   job without solid keys.
 *   Consistency check (necessary and sufficient): CFRK_ERR_LAYOUT, cfrk_last_error naming the first offending unitig,
 *   when a unitig is shorter than k, lies outside [0, nN) or before the end of its predecessor; has a code outside 0..3;
 *   has a k-mer that is not solid at min_count; or has a k-mer whose node another k-mer of the input claims as well
 *   (named is the later of the two claimants).  When none of these holds but a solid key lies in no unitig of the input,
 *   CFRK_ERR_LAYOUT names no unitig.  After CFRK_OK every x in O has a position.  After an error there is no map.
 *   CFRK_ERR_ARG: negative sizes, NULL arrays with nS > 0, nS >= 2^32, an index of more than 2^31 slots.
 *   CFRK_ERR_STATE: no job, or a CFRK_RUNS_ONLY job.  For any input whatever nothing outside the buffers is accessed and
 *   no loop is unbounded.
 *   Device form (cfrk_amd/csrc/unitig_locate.hip): one workgroup per tile of 8192 window starts of the unitig bytes, 32
 *   consecutive starts per lane, so the work is balanced by bases and no lane's work grows with a unitig's length; every
 *   window finds its slot and claims it with a compare-and-swap; one pass over the slots finds a solid key left out.
 *   It synchronises ONCE, for the error word.  Temporary device memory: 8 bytes per slot of the lookup index.
 * cfrk_global_locate: one lane per key, as cfrk_global_neighbors; keys_hi may be NULL for k <= 32.  CFRK_ERR_STATE when
 *   there is no valid map.  The device form returns with the kernel enqueued.
 * cfrk_global_read_hits: CSR over reads.  hit_ptr[0] = 0, hit_ptr[i + 1] - hit_ptr[i] = hits of read i in ascending
 *   read_off, *n_hits_out = hit_ptr[nS].  Capacity (the select's protocol): when n_hits > cap_hits the call returns
 *   CFRK_ERR_SMALL_BUF with hit_ptr and *n_hits_out complete and nothing written to hits; NULL hits with cap_hits 0 is
 *   that "sizes only" call; cap_hits = the number of windows is always enough.  1 <= k <= 64, reads of any length.
 *   CFRK_ERR_STATE without a valid map; CFRK_ERR_ARG: negative sizes, NULL n_hits_out or hit_ptr, NULL data / start /
 *   length with nS > 0, NULL hits with cap_hits > 0.
 *   Device form: no alignment requirement on d_data; start and length are not checked: a read outside [0, nN) gets an
 *   empty row.  A count pass (three launches over the read size classes), the scan of the counts in hit_ptr, ONE
 *   synchronisation for n_hits, then a fill pass that repeats the lookups and a pass over the rows; it returns with
 *   those enqueued.  Host form: stages through the pool, checks the layout as cfrk_global_add does; synchronous. */
typedef struct cfrk_unitig_pos {   /* 8 bytes, no padding */
  uint32_t unitig;   /* j */
  uint32_t at;       /* p << 1 | minus */
} cfrk_unitig_pos;
#define CFRK_POS_NONE 0xFFFFFFFF   /* both words of the position of a k-mer that is not in O */
typedef struct cfrk_read_hit {     /* 16 bytes, no padding */
  uint32_t unitig;      /* j */
  uint32_t unitig_at;   /* off << 1 | minus: the hit covers s_j[off : off + n_windows + k - 1] */
  uint32_t read_off;    /* its first window = its first base in the read */
  uint32_t n_windows;
} cfrk_read_hit;
int cfrk_global_unitig_index_device(cfrk_ctx *ctx, uint32_t min_count, const int8_t *d_data, const int64_t *d_start,
                                    const int32_t *d_length, int64_t nN, int64_t nS);
int cfrk_global_unitig_index(cfrk_ctx *ctx, uint32_t min_count, const int8_t *data, const int64_t *start,
                             const int32_t *length, int64_t nN, int64_t nS);
int cfrk_global_locate_device(cfrk_ctx *ctx, const uint64_t *d_keys_lo, const uint64_t *d_keys_hi /* NULL for k <= 32 */,
                              int64_t n, cfrk_unitig_pos *d_out);
int cfrk_global_locate(cfrk_ctx *ctx, const uint64_t *keys_lo, const uint64_t *keys_hi, int64_t n, cfrk_unitig_pos *out);
int cfrk_global_read_hits_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                                 int64_t nN, int64_t nS, int64_t *d_hit_ptr /* nS + 1 */, cfrk_read_hit *d_hits,
                                 uint64_t cap_hits, int64_t *n_hits_out);
int cfrk_global_read_hits(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length, int64_t nN,
                          int64_t nS, int64_t *hit_ptr /* nS + 1 */, cfrk_read_hit *hits, uint64_t cap_hits,
                          int64_t *n_hits_out);

/* Graph mask: stored keys that are no longer part of the graph.  A stored key may be MASKED; a masked key is not solid.
 *   Scope: the mask is seen by the six calls that read solidity -- cfrk_global_neighbors, cfrk_global_unitigs,
 *   cfrk_global_unitig_links, cfrk_global_unitig_index and, through the position map, cfrk_global_locate and
 *   cfrk_global_read_hits -- and by nothing else.  Counts are untouched: digest, export, histogram, query, read
 *   statistics, spans, correction, normalisation and merge never see the mask; a masked key still answers
 *   cfrk_global_query with its count; the job's digest is the same before and after every call of this section.
 *   Storage and lifetime: one byte per slot of the lookup index, in the context's pool.  The mask belongs to one build of
 *   the index, as the position map does: when the result changes (any add, merge or normalise call, a new job) the index
 *   is rebuilt, the mask is gone and every key is unmasked again.  A mask call on a job without a valid index builds
 *   the index, as a query does.
 *   Position map: every change of the mask drops it.  cfrk_global_locate and cfrk_global_read_hits return
 *   CFRK_ERR_STATE until cfrk_global_unitig_index is called again with the unitigs of the masked graph.
 *   Without a mask, every byte the six calls write is what it is without this section.
 * cfrk_global_mask_keys adds keys to the mask.  A key is canonicalised in a CFRK_CANONICAL job; a key that is not stored,
 *   or has bits at or above 2k, is ignored; duplicates are fine.  keys_hi may be NULL for k <= 32.  One lane per key,
 *   plain byte stores.
 * cfrk_global_mask_unitigs adds every k-mer of every unitig j with drop[j] != 0 to the mask.  The list is any
 *   struct-read list with ascending starts (it is NOT checked to be this job's unitigs); windows with an invalid code,
 *   and k-mers that are not stored, are skipped; a read outside [0, nN) is skipped.  Balanced by bytes like the claim
 *   pass of the position map (one workgroup per tile of 8192 window starts of the bytes), so no lane's work grows with a
 *   unitig's length.  The host form checks start / length against the terminators as cfrk_global_add does
 *   (CFRK_ERR_LAYOUT).
 * cfrk_global_mask_clear unmasks everything; fine without a mask.  cfrk_global_mask_count: the stored keys that are
 *   masked; one pass over the slots; synchronises.
 * CFRK_ERR_STATE: no job, or a CFRK_RUNS_ONLY job.  CFRK_ERR_ARG: negative sizes, NULL arrays with n or nS above 0, NULL
 *   n_masked.  CFRK_ERR_TABLE_FULL and CFRK_ERR_NOMEM as for cfrk_global_query.  n = 0 and nS = 0 are fine.  Nothing
 *   outside the buffers is accessed for any input whatever.  The device forms return with their kernel enqueued; the
 *   host forms stage through the pool and are synchronous. */
int cfrk_global_mask_keys_device(cfrk_ctx *ctx, const uint64_t *d_keys_lo, const uint64_t *d_keys_hi /* NULL for k <= 32 */,
                                 int64_t n);
int cfrk_global_mask_keys(cfrk_ctx *ctx, const uint64_t *keys_lo, const uint64_t *keys_hi, int64_t n);
int cfrk_global_mask_unitigs_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                                    int64_t nN, int64_t nS, const uint8_t *d_drop /* nS */);
int cfrk_global_mask_unitigs(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length, int64_t nN,
                             int64_t nS, const uint8_t *drop /* nS */);
int cfrk_global_mask_clear(cfrk_ctx *ctx);
int cfrk_global_mask_count(cfrk_ctx *ctx, uint64_t *n_masked);

/* Unitig tips: short dead-end branches that hang off a better-supported path.  The rule is a pure function of the
 * compacted graph: the unitigs' records (kc, n_kmers, CFRK_UNITIG_CIRCULAR), the link CSR as cfrk_global_unitig_links
 * wrote it, and the job's strand rule.  It needs neither sequences nor the index; the job only supplies the strand rule.
 *   Oriented unitigs: (j,+), and in a canonical job also (j,-).
 *   out(a) = the links that leave oriented unitig a; in(a) = the links that enter it.  In a canonical job the rows hold
 *   every link's mirror, so in(j,+) is read off row j: its CFRK_LINK_FROM_MINUS links, mirrored.  In a job that is not
 *   canonical in() is built from the rows (a count pass, a scan, a fill pass; the order inside an in-row does not matter).
 *   right(j) = |out(j,+)|, left(j) = |in(j,+)|.  n_j = n_kmers, kc_j = kc.  Means are compared exactly by
 *   cross-multiplying in 128 bits: mean(w) > mean(j) iff kc_w n_j > kc_j n_w.
 *   CANDIDATE: j is not CFRK_UNITIG_CIRCULAR, n_j <= max_kmers, and exactly one of left(j), right(j) is 0.  (A unitig
 *   with both ends dead is isolated, not a tip: it stays.)
 *   ATTACHMENTS and SIBLINGS of a candidate.  right(j) = 0: every link (u,ou) -> (j,+) of in(j,+) is an attachment, its
 *   siblings are the targets (w,ow) of out(u,ou) with w != j.  left(j) = 0: every link (j,+) -> (v,ov) of out(j,+) is an
 *   attachment, its siblings are the sources (w,ow) of in(v,ov) with w != j.
 *   BEATS: sibling w beats j iff 256 kc_w n_j >= ratio_q8 kc_j n_w, and w is not a candidate, or mean(w) > mean(j), or
 *   the means are equal and w < j.
 *   TIP: j is a candidate and, at some attachment, some sibling beats it.  tip[j] = 1 for a tip, else 0; every byte is
 *   written; *n_tips_out = the tips.
 *   Every decision reads the input graph only: the result does not depend on any order.  Among candidates that compete
 *   for one anchor end the best-ranked always survives unless a sibling that is no candidate exists: a fork at the very
 *   end of a contig keeps one arm.  ratio_q8 = 0 is the purely topological rule, 512 asks the sibling for twice the
 *   tip's mean coverage; ratio_q8 > CFRK_TIP_RATIO_Q8_MAX (65536) is CFRK_ERR_ARG: the bound keeps every product
 *   inside 128 bits.  max_kmers = 0 makes nothing a tip.
 * Untrusted input, checked in a pass before anything is decided: CFRK_ERR_LAYOUT, cfrk_last_error naming the first
 *   offending unitig, for a link_ptr that does not ascend from 0 to n_links, a row longer than 16 links (4 when not
 *   canonical), a target >= nS, flag bits beyond the two defined ones or any flag bit in a job that is not canonical, an
 *   in-degree above 4 when not canonical.  After the check one lane per unitig does at most 8 x 8 comparisons.  No loop
 *   is unbounded and nothing outside the arrays is accessed.  After an error tip[] is all 0.
 * CFRK_ERR_STATE: no job.  CFRK_ERR_ARG: NULL n_tips_out, NULL rec / link_ptr / tip with nS > 0, NULL links with n_links
 *   > 0, negative sizes, nS >= 2^32, ratio_q8 above its bound.  nS = 0 is fine: no tips.
 * Device form (cfrk_amd/csrc/unitig_tips.hip): n_tips_out is host memory; the call synchronises ONCE, for n_tips and the
 *   error word.  Temporary device memory, kept in the context's pool: one byte per unitig; not canonical: 12 more bytes
 *   per unitig, 4 per link and the scan's scratch.  Host form: stages through the pool; synchronous. */
#define CFRK_TIP_RATIO_Q8_MAX 65536
int cfrk_global_unitig_tips_device(cfrk_ctx *ctx, const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr /* nS + 1 */,
                                   const cfrk_unitig_link *d_links, int64_t n_links, uint32_t max_kmers, uint32_t ratio_q8,
                                   uint8_t *d_tip /* nS bytes, every one written 0 or 1 */, int64_t *n_tips_out);
int cfrk_global_unitig_tips(cfrk_ctx *ctx, const cfrk_unitig *rec, int64_t nS, const int64_t *link_ptr /* nS + 1 */,
                            const cfrk_unitig_link *links, int64_t n_links, uint32_t max_kmers, uint32_t ratio_q8,
                            uint8_t *tip /* nS */, int64_t *n_tips_out);

/* Unitig bubbles: the weaker of two parallel single-unitig paths between the same two oriented unitigs -- what a
 * substitution or a small indel in the middle of a read leaves behind after compaction, or, with balanced coverage, a
 * heterozygous site.  Like the tip rule a pure function of the unitigs' records (kc, n_kmers, CFRK_UNITIG_CIRCULAR), the
 * link CSR as cfrk_global_unitig_links wrote it, and the job's strand rule; no sequence, no index.  Oriented unitigs,
 * out(), in(), the mirror convention, n_j and kc_j are those of "Unitig tips".
 *   ARM: oriented unitig x = (j,o) is an arm iff j is not CFRK_UNITIG_CIRCULAR, n_j <= max_kmers, |in(x)| = 1 and
 *   |out(x)| = 1, and neither the source src(x) of that in-link nor the target dst(x) of that out-link is unitig j in
 *   either orientation (no self-loop, hairpin or homopolymer node).  In a canonical job (j,-) is an arm iff (j,+) is,
 *   with src(j,-) = mirror(dst(j,+)) and dst(j,-) = mirror(src(j,+)): one record per unitig suffices.
 *   PARALLEL: arms x = (j,o) and y = (s,p), s != j, are parallel iff src(x) == src(y) and dst(x) == dst(y) as oriented
 *   unitigs and |n_j - n_s| <= max_diff.  (max_diff makes this non-transitive: arms of 10, 12 and 14 k-mers with
 *   max_diff 2 are not all pairwise parallel.  That is intended.)
 *   BEATS: y beats x iff 256 kc_s n_j >= ratio_q8 kc_j n_s, and s ranks above j: kc_s n_j > kc_j n_s, or they are equal
 *   and s < j.  All products in 128 bits; ratio_q8 <= CFRK_TIP_RATIO_Q8_MAX as for tips.  Every ratio_q8 <= 256 means
 *   "the weaker arm always goes"; 512 leaves a balanced heterozygous site alone.
 *   pop[j] = 1 iff (j,+) is an arm and some parallel arm beats it, else 0.  partner[j] = s << 1 | p for the best-ranked
 *   arm (s,p) that beats it, p being the partner's orientation when j is read as (j,+); p = 0 when both orientations of
 *   one s qualify, and always in a job that is not canonical; CFRK_BUBBLE_NONE (0xFFFFFFFF) when pop[j] = 0.
 *   *n_pop_out = the popped unitigs.  The parallel arms of x are sought among the targets of out(src(x)), which in the
 *   rows of a real link set are all of them.
 *   Every decision reads the input graph only: the result depends on no order.  The best-ranked arm of any (src, dst)
 *   class is never popped, so src and dst stay joined.  A popped unitig has no dead end, so it is never also a tip:
 *   tip[] and pop[] of one graph are disjoint and may be dropped together.  max_kmers = 0 pops nothing.
 * Untrusted input: the check of the tip rule runs in front, with the same five CFRK_ERR_LAYOUT reasons naming the first
 *   offending unitig, and only checked rows are followed.  After the check one lane per unitig looks at the at most 16
 *   links of one row.  No loop is unbounded, nothing outside the arrays is accessed, every byte of pop and partner is
 *   written whatever is refused (pop 0, partner NONE after an error).  Rows that pass the check without being a real
 *   link set (canonical rows that lack their mirrors, say) give CFRK_OK, partners below 2 nS or NONE, and whatever the
 *   rule says of the rows as given.
 * CFRK_ERR_STATE: no job.  CFRK_ERR_ARG: NULL n_pop_out, NULL rec / link_ptr / pop with nS > 0, NULL links with n_links
 *   > 0, negative sizes, nS >= 2^31 (a partner names an oriented unitig in 32 bits), ratio_q8 above its bound.  partner
 *   may be NULL.  nS = 0 is fine: nothing popped.
 * Device form (cfrk_amd/csrc/unitig_bubbles.hip): n_pop_out is host memory; the call synchronises ONCE, for n_pop and
 *   the error word.  Temporary device memory, kept in the context's pool: 9 bytes per unitig; not canonical: 12 more
 *   bytes per unitig, 4 per link and the scan's scratch.  Host form: stages through the pool; synchronous. */
#define CFRK_BUBBLE_NONE 0xFFFFFFFF
int cfrk_global_unitig_bubbles_device(cfrk_ctx *ctx, const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr /* nS + 1 */,
                                      const cfrk_unitig_link *d_links, int64_t n_links, uint32_t max_kmers, uint32_t max_diff,
                                      uint32_t ratio_q8, uint8_t *d_pop /* nS bytes, every one written 0 or 1 */,
                                      uint32_t *d_partner /* nS words, every one written; may be NULL */, int64_t *n_pop_out);
int cfrk_global_unitig_bubbles(cfrk_ctx *ctx, const cfrk_unitig *rec, int64_t nS, const int64_t *link_ptr /* nS + 1 */,
                               const cfrk_unitig_link *links, int64_t n_links, uint32_t max_kmers, uint32_t max_diff,
                               uint32_t ratio_q8, uint8_t *pop /* nS */, uint32_t *partner /* nS; may be NULL */,
                               int64_t *n_pop_out);

/* Unitig bulges: an arm beside a CHAIN of better-supported unitigs between the same two oriented ends.  An error's arm
 * is one unitig, but the true path beside it is cut by its neighbours' branch points, so the bubble rule, which compares
 * single unitigs, rarely sees it.  Like the tip and the bubble rule a pure function of the unitigs' records (kc, n_kmers,
 * CFRK_UNITIG_CIRCULAR), the link CSR as cfrk_global_unitig_links wrote it, and the job's strand rule; no sequence, no
 * index.  Oriented unitigs, out(), in(), the mirror convention, n_j, kc_j and the 128-bit cross-multiplied means are
 * those of "Unitig tips".
 *   ARM: exactly the bubble rule's arm for x = (j,+): j is not CFRK_UNITIG_CIRCULAR, n_j <= max_kmers, |in(x)| = 1 and
 *   |out(x)| = 1, and neither s = src(x) nor t = dst(x) is unitig j.
 *   ELIGIBLE: oriented unitig (w,o) is eligible for j iff 256 kc_w n_j >= ratio_q8 kc_j n_w, and w ranks above j:
 *   kc_w n_j > kc_j n_w, or they are equal and w < j.
 *   PATH for x: oriented unitigs w_1 .. w_m, 1 <= m <= max_hops, such that the links s -> w_1, w_i -> w_i+1 and w_m -> t
 *   exist; every w_i is eligible; no w_i is unitig j, unitig(s) or unitig(t) in either orientation; the w_i are pairwise
 *   distinct as unitigs; n_j - max_diff <= sum of n_w_i <= n_j + max_diff.  A direct link s -> t (m = 0) is no path.
 *   SEARCH: depth-first and pre-order from s, in one fixed order.  out(cur) is walked in row order: for (u,+) in a
 *   canonical job the links of row u without CFRK_LINK_FROM_MINUS, for (u,-) those with it, in a job that is not
 *   canonical row u.  Every link looked at adds 1 to `visits`.  For a link cur -> y: if y == t, the depth (the unitigs
 *   on the path so far) is >= 1 and the running sum is >= n_j - max_diff, the path is found and the search ends;
 *   otherwise, if y is eligible, not excluded, the depth is < max_hops and sum + n_y <= n_j + max_diff, the search
 *   descends into y at once; otherwise it takes the next link.  A row that is done returns to the row above it.  When
 *   `visits` would exceed max_visits the arm is UNDECIDED: not popped, and visits[j] = max_visits + 1.
 *   pop[j] = 1 iff (j,+) is an arm and the search found a path, else 0.  visits[j] = the links looked at for an arm, 0
 *   for a unitig that is no arm.  path_ptr is a CSR over unitigs: path_ptr[0] = 0, path_ptr[j + 1] - path_ptr[j] = m for
 *   a popped j and 0 otherwise, *n_path_out = path_ptr[nS]; row j of path holds that first-found path as w << 1 | o, in
 *   order from s to t.  stats: the arms, the popped and the undecided ones.
 *   Only (j,+) is searched.  In a canonical job the mirrored search, from mirror(t) to mirror(s), decides the same
 *   whenever neither runs out of budget.
 *   Every interior unitig of a popped arm's path ranks strictly above the arm, and rank is a total order: by induction
 *   from the top rank down, in the graph without the popped unitigs there is still a walk from s to t through unpopped
 *   unitigs.  That holds for all arms popped from one graph at once, and for pop[] of this rule OR-ed with pop[] of the
 *   bubble rule, since a bubble's partner ranks above it too.  A popped unitig has no dead end, and neither has any
 *   interior unitig of a path: the result is disjoint from tip[], and all three may go into one mask call.  With equal
 *   max_kmers, max_diff and ratio_q8 every unitig the bubble rule pops is popped here or undecided.  max_kmers = 0 or
 *   max_hops = 0 pops nothing.
 * Capacity (the select's protocol): when n_path > cap_path the call returns CFRK_ERR_SMALL_BUF with pop, visits,
 *   path_ptr, stats and *n_path_out complete and nothing written to path; NULL path with cap_path 0 is that "sizes only"
 *   call.  visits may be NULL.  path_ptr may be NULL: then no paths are wanted, no scan runs, path and cap_path are
 *   ignored and *n_path_out (which may then be NULL as well) is 0.
 * Untrusted input: the check of the tip rule runs in front, with the same five CFRK_ERR_LAYOUT reasons naming the first
 *   offending unitig, and only checked rows are followed.  After the check one lane per arm looks at no more than
 *   max_visits links of rows of at most 16, on a stack of at most max_hops levels.  No loop is unbounded, nothing
 *   outside the arrays is accessed, every byte of pop, visits and path_ptr is written whatever is refused (all 0 after
 *   an error, with stats and *n_path_out 0).  Rows that pass the check without being a real link set (canonical rows
 *   that lack their mirrors, say) give CFRK_OK, path entries below 2 nS, and whatever the rule says of the rows as given.
 * CFRK_ERR_STATE: no job.  CFRK_ERR_ARG: NULL stats, NULL rec / link_ptr / pop with nS > 0, NULL links with n_links > 0,
 *   NULL n_path_out with path_ptr given, NULL path with cap_path > 0, negative sizes, nS >= 2^31 (a path names an
 *   oriented unitig in 32 bits), max_hops > CFRK_BULGE_MAX_HOPS, max_visits > CFRK_BULGE_MAX_VISITS, ratio_q8 above
 *   CFRK_TIP_RATIO_Q8_MAX.  nS = 0 is fine: nothing popped (path_ptr[0] = 0 in the host form).
 * Device form (cfrk_amd/csrc/unitig_bulges.hip): stats and n_path_out are host memory; the call synchronises ONCE, for
 *   the error word, the counts and n_path, and returns with the pass that writes path enqueued.  The search's stack is
 *   in LDS, 20 KB for the 64 arms of a wave.  Temporary device memory, kept in the context's pool: 16 bytes per unitig
 *   and the scan's scratch; not canonical: 12 more bytes per unitig and 4 per link.  Host form: stages through the pool;
 *   synchronous. */
#define CFRK_BULGE_MAX_HOPS 64
#define CFRK_BULGE_MAX_VISITS 65536
typedef struct cfrk_bulge_stats {   /* 24 bytes, no padding */
  int64_t arms;        /* unitigs j whose (j,+) is an arm      */
  int64_t popped;      /* arms beside which a path was found   */
  int64_t undecided;   /* arms whose search ran out of budget  */
} cfrk_bulge_stats;
int cfrk_global_unitig_bulges_device(cfrk_ctx *ctx, const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr /* nS + 1 */,
                                     const cfrk_unitig_link *d_links, int64_t n_links, uint32_t max_kmers, uint32_t max_diff,
                                     uint32_t max_hops, uint32_t max_visits, uint32_t ratio_q8,
                                     uint8_t *d_pop /* nS bytes, every one written 0 or 1 */,
                                     uint32_t *d_visits /* nS words, every one written; may be NULL */,
                                     int64_t *d_path_ptr /* nS + 1; may be NULL */, uint32_t *d_path, uint64_t cap_path,
                                     int64_t *n_path_out, cfrk_bulge_stats *stats);
int cfrk_global_unitig_bulges(cfrk_ctx *ctx, const cfrk_unitig *rec, int64_t nS, const int64_t *link_ptr /* nS + 1 */,
                              const cfrk_unitig_link *links, int64_t n_links, uint32_t max_kmers, uint32_t max_diff,
                              uint32_t max_hops, uint32_t max_visits, uint32_t ratio_q8, uint8_t *pop /* nS */,
                              uint32_t *visits /* nS; may be NULL */, int64_t *path_ptr /* nS + 1; may be NULL */,
                              uint32_t *path, uint64_t cap_path, int64_t *n_path_out, cfrk_bulge_stats *stats);

/* Weak unitigs: erroneous connections and isolated low-coverage pieces.  An erroneous connection is a short, thin
 * unitig that is linked at both ends (so it is no tip), possibly by several links at an end (so it is no arm of the
 * bubble or the bulge rule), and that at each of those links sits beside a much better-covered way out of the same
 * neighbour: what a chimeric read or an error whose own neighbours are errors leaves behind.  An isolated piece is a
 * short, thin unitig without any link, as clipping leaves them floating.  Like the other three rules a pure function of
 * the unitigs' records (kc, n_kmers, CFRK_UNITIG_CIRCULAR), the link CSR as cfrk_global_unitig_links wrote it, and the
 * job's strand rule; no sequence, no index.  Oriented unitigs, out(), in(), the mirror convention, left(j), right(j),
 * n_j, kc_j and the 128-bit cross-multiplied means are exactly those of "Unitig tips".
 *   SELF-FREE: no link of row j has target j, in either orientation; in a job that is not canonical no link of j's
 *   in-row has source j either (no self-loop, hairpin or homopolymer node).
 *   ISOLATED: j is not CFRK_UNITIG_CIRCULAR, left(j) = right(j) = 0, n_j <= iso_max_kmers and 256 kc_j < iso_mean_q8 n_j
 *   (mean coverage below iso_mean_q8 / 256).  Then weak[j] = CFRK_WEAK_ISOLATED.
 *   CANDIDATE: j is not CFRK_UNITIG_CIRCULAR, n_j <= max_kmers, left(j) >= 1 and right(j) >= 1, and j is self-free.
 *   ATTACHMENTS and SIBLINGS of a candidate, at BOTH ends.  Right end: every link (j,+) -> (v,ov) of out(j,+) is an
 *   attachment, its siblings are the sources (w,ow) of in(v,ov) with w != j.  Left end: every link (u,ou) -> (j,+) of
 *   in(j,+) is an attachment, its siblings are the targets (w,ow) of out(u,ou) with w != j.  In a canonical job the left
 *   end of (j,+) is the right end of (j,-): every link of row j is an attachment of one end or the other, and at its
 *   target (v,ov) the siblings are the targets of v's links that leave (v,!ov).
 *   BEATS (the bubble rule's): w beats j iff 256 kc_w n_j >= ratio_q8 kc_j n_w, and w ranks above j: kc_w n_j > kc_j n_w,
 *   or they are equal and w < j.  ratio_q8 <= CFRK_TIP_RATIO_Q8_MAX as for tips.
 *   WEAK CONNECTION: j is a candidate and at EVERY attachment of BOTH ends some sibling beats it.  Then weak[j] =
 *   CFRK_WEAK_CONNECTION.
 *   Everything else is 0; every byte is written.  stats: the connections, the isolated ones, and the candidates.
 *   max_kmers = 0 makes no connection; iso_max_kmers = 0 or iso_mean_q8 = 0 makes nothing isolated (a unitig's record has
 *   n_kmers >= 1).
 *   Every decision reads the input graph only: the result depends on no order.
 *   The best-ranked neighbour at any oriented end is never a weak connection through that end, because "every
 *   attachment" includes this one and no sibling there ranks above it.  So the rule alone never leaves a neighbour with a
 *   new dead end: an oriented end that had a link keeps one.
 *   weak[] and tip[] of one graph are disjoint: a tip has exactly one dead end, a connection none, an isolated unitig two.
 *   All four rules' results may go into one mask call.
 *   At equal max_kmers and ratio_q8 every unitig the bubble rule pops (whatever its max_diff) is a weak connection: an
 *   arm is self-free, and its one in-link and its one out-link each have the parallel arm, which beats it, as a sibling.
 *   The converse is false.  That superset is why a caller wants a HIGH ratio here (the Python and CLI default is 4.0,
 *   against 0 for bubbles): at a low one the rule eats a heterozygous site's weaker arm and more.
 * Untrusted input: the check of the tip rule runs in front, with the same five CFRK_ERR_LAYOUT reasons naming the first
 *   offending unitig, and only checked rows are followed.  After the check one lane per unitig looks at the at most 16
 *   links of its row and, at each target, at that row's at most 16 links, of which in a real link set at most 8 are on
 *   the entering side: 128 comparisons.  No loop is unbounded, nothing outside the arrays is accessed, every byte of
 *   weak is written whatever is refused (all 0 after an error, with stats 0).  Rows that pass the check without being a
 *   real link set (canonical rows that lack their mirrors, say) give CFRK_OK and whatever the rule says of the rows as
 *   given, in() of a canonical job being read off the rows by the mirror convention.
 * CFRK_ERR_STATE: no job.  CFRK_ERR_ARG: NULL stats, NULL rec / link_ptr / weak with nS > 0, NULL links with n_links > 0,
 *   negative sizes, nS >= 2^32, ratio_q8 above its bound.  nS = 0 is fine: nothing found.
 * Device form (cfrk_amd/csrc/unitig_weak.hip): stats is host memory; the call synchronises ONCE, for the counts and the
 *   error word.  Temporary device memory, kept in the context's pool: four words; not canonical: 12 bytes per unitig, 4
 *   per link and the scan's scratch.  Host form: stages through the pool; synchronous. */
#define CFRK_WEAK_CONNECTION 1
#define CFRK_WEAK_ISOLATED 2
typedef struct cfrk_weak_stats {   /* 24 bytes, no padding */
  int64_t connections;   /* weak[j] == CFRK_WEAK_CONNECTION */
  int64_t isolated;      /* weak[j] == CFRK_WEAK_ISOLATED   */
  int64_t candidates;    /* the candidates for a connection */
} cfrk_weak_stats;
int cfrk_global_unitig_weak_device(cfrk_ctx *ctx, const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr /* nS + 1 */,
                                   const cfrk_unitig_link *d_links, int64_t n_links, uint32_t max_kmers, uint32_t ratio_q8,
                                   uint32_t iso_max_kmers, uint32_t iso_mean_q8, uint8_t *d_weak /* nS bytes, every one written */,
                                   cfrk_weak_stats *stats);
int cfrk_global_unitig_weak(cfrk_ctx *ctx, const cfrk_unitig *rec, int64_t nS, const int64_t *link_ptr /* nS + 1 */,
                            const cfrk_unitig_link *links, int64_t n_links, uint32_t max_kmers, uint32_t ratio_q8,
                            uint32_t iso_max_kmers, uint32_t iso_mean_q8, uint8_t *weak /* nS */, cfrk_weak_stats *stats);

/* Unitig compaction: the unitigs of the graph WITHOUT some of its unitigs, computed from the unitig list itself.  After
 * a rule has chosen what to drop, the compacted graph of the remaining keys differs from the old one only where a
 * dropped unitig was the reason two others could not merge.  It is a pure function of the unitigs' sequences and records
 * as cfrk_global_unitigs wrote them (data, start, length, rec, nN, nS), the link CSR as cfrk_global_unitig_links wrote it
 * (link_ptr, links, n_links), drop[nS] (a byte per unitig, nonzero: dropped; NULL: nothing is dropped), k and the strand
 * rule.  It needs neither the index nor the counts; the job only supplies k and the strand rule.
 *   DEFINING PROPERTY: the output is byte for byte what cfrk_global_unitigs(min_count) returns after
 *   cfrk_global_mask_unitigs(drop) on the job the inputs came from: sequences, terminators, start, length, kc, n_kmers,
 *   CFRK_UNITIG_CIRCULAR and the order.
 * The rule.  Oriented unitigs, head(), tail(), out() and in() are those of "Unitig links" and "Unitig tips", all links
 *   taken among the SURVIVORS (drop[j] == 0) only.  n_u = n_kmers of u.
 *   MERGE (u,ou) -> (v,ov) iff out(u,ou) = {(v,ov)} and in(v,ov) = {(u,ou)}; it is not a hairpin (v = u with ov != ou);
 *   it is not the self-link of a single-node unitig (v = u, ov = ou, n_u = 1); neither u nor v is a palindromic single
 *   node (a canonical job, n = 1, head = rc(head)); neither is CFRK_UNITIG_CIRCULAR.  A self-link (u,+) -> (u,+) with
 *   n_u > 1 that has become the only link on both sides IS a merge: the unitig closes to a cycle (a tip fell off it).
 *   Why this is the k-mer rule: the links inside a surviving unitig stay links, since removing keys only shrinks succ()
 *   and pred(); at an end, succ(tail(u,ou)) among the remaining keys is exactly the heads of the surviving targets of
 *   out(u,ou), and the exclusions are node(a) == node(b) and the palindromes of the k-mer rule, stated for ends.
 *   Merges form disjoint paths and cycles over the oriented unitigs; in a canonical job each has a distinct mirror.  A
 *   COMPONENT is written once: the members' sequences spelled with their k - 1 overlaps, kc and n_kmers summed.
 *   path: as it stands; in a canonical job, of the path and its mirror the one whose first k-mer is smaller.
 *   cycle (also one that closes only now): cut at the smallest oriented k-mer of the cycle (canonical: and of its
 *     mirror), flagged CFRK_UNITIG_CIRCULAR.  A cycle of fewer than k k-mers is legal.
 *   A CFRK_UNITIG_CIRCULAR input is a component of its own and is copied.  ORDER: ascending by first k-mer.
 * Output: a unitig list in the layout of cfrk_global_unitigs (data_out / cap_data, start_out, length_out, rec_out /
 *   cap_unitigs, *nN_out, *nS_out), and, unless NULL, into[nS]: where input unitig j went, as cfrk_unitig_pos.  unitig =
 *   the index in the output, at = off << 1 | minus: input j covers s_new[off : off + length[j]], or that is its reverse
 *   complement when minus is set (always 0 in a job that is not canonical).  In a circular output the positions are
 *   taken mod n_kmers: a member that the cut splits wraps around the end.  A dropped unitig has CFRK_POS_NONE in both
 *   words.
 * Capacities: *nS_out <= the survivors and *nN_out <= the sum of their lengths plus their number, always.  The select's
 *   protocol: when *nN_out > cap_data or *nS_out > cap_unitigs the call returns CFRK_ERR_SMALL_BUF with both sizes
 *   complete and nothing written to the arrays (into included); NULL arrays with zero capacities are that "sizes only"
 *   call.  Outputs must not overlap inputs.  No alignment requirement on data or data_out.
 * Untrusted input.  The rows go through the check of "Unitig tips" (the same five CFRK_ERR_LAYOUT reasons).  Beyond it,
 *   CFRK_ERR_LAYOUT, cfrk_last_error naming the first offending unitig (dropped ones are checked like the others), for a
 *   unitig with length < k, with length != n_kmers + k - 1, with a range outside [0, nN) or a start before the end of
 *   its predecessor; for a merge whose k - 1 overlap does not match in the two end windows (named is the lower of the
 *   two unitigs); for a component of more than 2^31 - 1 bases (named is the unitig it begins with).  A merge is taken
 *   only when the out-condition read off u's row and the in-condition read off v's row (not canonical: off v's in-row,
 *   built from all rows) name each other, so rows that pass the check without being a link set still give well-formed
 *   paths and cycles, every survivor in exactly one written component.  Interior codes are not checked: the check is
 *   necessary, not sufficient; cfrk_global_unitig_index on the result is the sufficient one.  For any input whatever
 *   nothing outside the buffers is accessed and no loop is unbounded.  An error wins over CFRK_ERR_SMALL_BUF; after it
 *   the arrays are unspecified and the sizes are 0.
 * CFRK_ERR_STATE: no job.  CFRK_ERR_ARG: NULL size outputs, negative sizes, NULL data / start / length / rec / link_ptr
 *   with nS > 0, NULL links with n_links > 0, a NULL output array with a capacity above 0, nS >= 2^31.  nS = 0 is fine:
 *   both sizes 0.
 * Device form (cfrk_amd/csrc/unitig_compact.hip): after the checks one lane per oriented unitig finds its merge from two
 *   rows of at most 16 links and the 2k end bases; the chains are ranked by pointer doubling, ceil(log2 nS) launches of
 *   one lane per oriented unitig, so no lane's work grows with the members of a chain; the smallest k-mer of a cycle is
 *   found one window per lane over the cycles' members only; the components are sorted by first k-mer; the emit runs one
 *   workgroup per CFRK_COMPACT_TILE_BYTES of OUTPUT bytes, so one member of 10^6 bases among short ones costs what its
 *   bytes cost.  It synchronises ONCE, for the sizes and the error word, and returns with the order, into and the emit
 *   enqueued.  Temporary device memory, kept in the context's pool: 140 bytes per oriented unitig (2 nS of them in a
 *   canonical job, else nS), 52 per unitig, 44 per output unitig, the sort's and the scans' scratch; not canonical: 12
 *   more bytes per unitig and 4 per link.  16 bytes of LDS in the emit, no scratch.
 * Host form: stages through the pool, checks start / length against the terminators as cfrk_global_add does
 *   (CFRK_ERR_LAYOUT); synchronous. */
#define CFRK_COMPACT_TILE_BYTES 4096
int cfrk_global_unitigs_compact_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                                       const cfrk_unitig *d_rec, int64_t nN, int64_t nS, const int64_t *d_link_ptr /* nS + 1 */,
                                       const cfrk_unitig_link *d_links, int64_t n_links, const uint8_t *d_drop /* nS; may be NULL */,
                                       int8_t *d_data_out, uint64_t cap_data, int64_t *d_start_out, int32_t *d_length_out,
                                       cfrk_unitig *d_rec_out, uint64_t cap_unitigs, cfrk_unitig_pos *d_into /* nS; may be NULL */,
                                       int64_t *nN_out, int64_t *nS_out);
int cfrk_global_unitigs_compact(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length,
                                const cfrk_unitig *rec, int64_t nN, int64_t nS, const int64_t *link_ptr /* nS + 1 */,
                                const cfrk_unitig_link *links, int64_t n_links, const uint8_t *drop /* nS; may be NULL */,
                                int8_t *data_out, uint64_t cap_data, int64_t *start_out, int32_t *length_out,
                                cfrk_unitig *rec_out, uint64_t cap_unitigs, cfrk_unitig_pos *into /* nS; may be NULL */,
                                int64_t *nN_out, int64_t *nS_out);

/* Read paths and link support: the hits of a read joined across links into walks through the graph, and how many reads
 * walk across every link.  A pure function of the hit CSR as cfrk_global_read_hits wrote it for nR reads (hit_ptr[nR + 1],
 * hits[n_hits]), the unitigs' records (rec[nS]; only n_kmers is read), a link CSR (link_ptr[nS + 1], links[n_links]) and
 * the job's strand rule, which is used for the row check alone.  It needs no sequence, no index, no position map and no
 * counts.  The link CSR is the one cfrk_global_unitig_links wrote OR ANY SUB-CSR of it: a caller may have removed rows;
 * the call then says where reads break.
 *   ENDS of a hit (j, off, m, n), m = unitig_at & 1, off = unitig_at >> 1, n = n_windows, N = rec[j].n_kmers: its first
 *   window lies at pf = m ? off + n - 1 : off, its last at pl = m ? off : off + n - 1.  It ENTERS AT THE HEAD of (j,m) iff
 *   pf == (m ? N - 1 : 0) and LEAVES AT THE END of (j,m) iff pl == (m ? 0 : N - 1).
 *   STEP: two consecutive hits h, h' of one read are JOINED iff (a) h'.read_off == h.read_off + h.n_windows, (b) h leaves
 *   at the end of (j,m), (c) h' enters at the head of (j',m'), and (d) row j of the link CSR holds a link whose
 *   CFRK_LINK_FROM_MINUS bit equals m, whose `to` equals j' and whose CFRK_LINK_TO_MINUS bit equals m'.  The first such
 *   row in CSR order is the step's link r, an index into links.  Everything is read literally: a read across the cut of
 *   a circular unitig joins through (j,+) -> (j,+), a hairpin through (j,+) -> (j,-); a palindromic single-node unitig is
 *   always entered and left as (v,+), because its hits have minus = 0.
 *   PATH: a maximal chain of joined hits of one read, so a range of consecutive hits.  path_ptr[nR + 1] and
 *   paths[n_paths] are a CSR over reads, path_ptr[0] = 0, *n_paths_out = path_ptr[nR]; a row is cfrk_read_path: hit_first
 *   (index inside the read's hit row), n_hits, read_off, n_windows (the sum of its hits' windows, which are contiguous by
 *   (a)).  Paths ascend by hit_first; the n_hits of a read's paths sum to its hits.
 *   LINK SUPPORT: support[r] is INCREMENTED by the number of steps whose link is r.  The call adds and never clears: the
 *   caller zeroes support[n_links] once, batches of reads then accumulate.  NULL support skips the output.  Counting is
 *   directional, as the read spells it; nothing is mirrored here.  n_hits < 2^32, so one call cannot overflow a counter
 *   it found at zero.
 *   STATISTICS (cfrk_path_stats): n_paths; n_steps = joined pairs; n_gaps = consecutive hits of a read that fail (a);
 *   n_unlinked = pairs that pass (a) but fail (b), (c) or (d).  Sum of support added = n_steps.
 *   CONSEQUENCE: with the library's own hits and its own complete link CSR of the same graph n_unlinked is 0, and a
 *   read's paths are its maximal runs of located windows: two located neighbouring windows that are not colinear are the
 *   tail of one oriented unitig and a solid successor of it, and that is a link; the hit before the break therefore
 *   leaves at an end, the one behind it enters at a head.
 * Capacity (the select's protocol): when n_paths > cap_paths the call returns CFRK_ERR_SMALL_BUF with path_ptr,
 *   *n_paths_out, stats and support complete and nothing written to paths; NULL paths with cap_paths 0 is that "sizes
 *   only" call (give it a NULL support, or the exact call adds the steps a second time); cap_paths = n_hits is always
 *   enough.
 * Untrusted input.  The row check of "Unitig tips" runs in front (the same five CFRK_ERR_LAYOUT reasons naming the first
 *   offending unitig).  Then the hits: CFRK_ERR_LAYOUT, cfrk_last_error naming the first offending read, when hit_ptr
 *   does not start at 0, descends or leaves [0, n_hits] (hit_ptr[nR] may lie below n_hits: the hits behind it belong to
 *   no read and are not looked at); when a hit's unitig is >= nS, its n_windows is 0, or off + n_windows > n_kmers.  A
 *   refused row wins over a refused hit_ptr, that over a refused hit.  After an error path_ptr is all 0, the sizes and
 *   stats are 0 and support is UNTOUCHED: the hits are checked in a pass of their own in front of the one that counts.
 *   For any input whatever nothing outside the buffers is accessed and no loop is unbounded.
 * CFRK_ERR_ARG: negative sizes, NULL n_paths_out / stats / hit_ptr / path_ptr, NULL hits with n_hits > 0, NULL rec /
 *   link_ptr with nS > 0, NULL links with n_links > 0, NULL paths with cap_paths > 0, nS >= 2^32, n_hits >= 2^32.
 *   CFRK_ERR_STATE: no job.  nR = 0 and n_hits = 0 are fine.  The job, the index, the position map and the mask are
 *   neither read nor changed: same digest before and after.
 * Device form (cfrk_amd/csrc/read_paths.hip): balanced by HITS, one lane per hit in the check, the join (at most 16
 *   links of one row, one atomic add on support[r]) and the pass that writes the rows, so a read of 10^5 hits costs what
 *   its hits cost; a hipCUB exclusive sum over the start flags numbers the paths.  No alignment requirement on any array
 *   beyond that of its element type (4 bytes for hits, paths and support).  n_paths_out and stats are host memory; the
 *   call synchronises ONCE, for n_paths, the statistics and the error words, and returns with the passes that write
 *   paths enqueued.  Temporary device memory, kept in the context's pool: 4 bytes per hit and the scan's scratch; not
 *   canonical: 8 bytes per unitig for the in-degrees the row check counts (the in-rows are not built: nothing here
 *   reads them).  Host form: stages through the pool; synchronous. */
typedef struct cfrk_read_path {    /* 16 bytes, no padding */
  uint32_t hit_first;   /* index inside the read's hit row */
  uint32_t n_hits;
  uint32_t read_off;    /* its first window = its first base in the read */
  uint32_t n_windows;   /* the path covers read bases [read_off, read_off + n_windows + k - 1) */
} cfrk_read_path;
typedef struct cfrk_path_stats {   /* 32 bytes, no padding */
  uint64_t n_paths;
  uint64_t n_steps;      /* joined pairs of consecutive hits            */
  uint64_t n_gaps;       /* consecutive hits of a read that fail (a)    */
  uint64_t n_unlinked;   /* pairs that pass (a) but fail (b), (c) or (d) */
} cfrk_path_stats;
int cfrk_global_read_paths_device(cfrk_ctx *ctx, const int64_t *d_hit_ptr /* nR + 1 */, int64_t nR, const cfrk_read_hit *d_hits,
                                  int64_t n_hits, const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr /* nS + 1 */,
                                  const cfrk_unitig_link *d_links, int64_t n_links, int64_t *d_path_ptr /* nR + 1 */,
                                  cfrk_read_path *d_paths, uint64_t cap_paths, int64_t *n_paths_out,
                                  uint32_t *d_support /* n_links, added to; may be NULL */, cfrk_path_stats *stats);
int cfrk_global_read_paths(cfrk_ctx *ctx, const int64_t *hit_ptr /* nR + 1 */, int64_t nR, const cfrk_read_hit *hits,
                           int64_t n_hits, const cfrk_unitig *rec, int64_t nS, const int64_t *link_ptr /* nS + 1 */,
                           const cfrk_unitig_link *links, int64_t n_links, int64_t *path_ptr /* nR + 1 */,
                           cfrk_read_path *paths, uint64_t cap_paths, int64_t *n_paths_out,
                           uint32_t *support /* n_links, added to; may be NULL */, cfrk_path_stats *stats);

/* Unitig components: which unitigs of the graph belong together.  Like the four rules a pure function of the unitigs'
 * records (rec[nS]; kc and n_kmers are summed, nothing else is read), the link CSR (link_ptr[nS + 1], links[n_links]) and
 * the job's strand rule, which is used for the row check alone.  No sequence, no index, no counts.
 *   KEPT: unitig j is kept iff drop is NULL or drop[j] == 0.
 *   CONNECTED: two kept unitigs are connected iff some link of either row names the other.  Strand flags and direction
 *   are ignored: in a job that is not canonical the rows are directed, and the classes are the WEAKLY connected
 *   components.  A link whose source or target is not kept does not exist.  Self-links, hairpins and
 *   CFRK_UNITIG_CIRCULAR change nothing.
 *   COMPONENT: a class of the transitive closure over the kept unitigs.  Components are numbered 0, 1, ... ascending by
 *   their smallest unitig; comp[j] is that number, CFRK_COMP_NONE for a unitig that is not kept.  Every word of comp is
 *   written.  The output is one byte string for a given input: it depends neither on scheduling nor on the order of the
 *   links inside a row.
 *   TABLE: comps[c] is cfrk_unitig_component: the sums of the members' kc (modulo 2^64) and n_kmers, the links of the
 *   members' rows whose target is kept, as written (so with the mirrors a canonical link set holds), the smallest member
 *   and the number of members.  STATISTICS (cfrk_component_stats): the components, and the kept unitigs, their k-mers and
 *   their links to kept targets: the sums of the table's columns.
 *   With drop, the components are those of the graph cfrk_global_unitigs_compact makes of the same arguments, pulled
 *   back through its `into`: compaction merges only unitigs that a link joined.
 * Capacity (the select's protocol): when n_comps > cap_comps the call returns CFRK_ERR_SMALL_BUF with comp, *n_comps_out
 *   and stats complete and nothing written to comps; NULL comps with cap_comps 0 is that "sizes only" call; cap_comps =
 *   nS is always enough.
 * Untrusted input: the row check of "Unitig tips" runs in front, with the same five CFRK_ERR_LAYOUT reasons naming the
 *   first offending unitig, and only checked rows are followed.  After a refusal comp is all CFRK_COMP_NONE and the
 *   sizes and stats are 0.  For any input whatever nothing outside the buffers is accessed and no loop is unbounded
 *   (cfrk_amd/csrc/unitig_components.hip states the bound of the union-find).
 * CFRK_ERR_STATE: no job.  CFRK_ERR_ARG: negative sizes, NULL n_comps_out or stats, NULL rec / link_ptr / comp with
 *   nS > 0, NULL links with n_links > 0, NULL comps with cap_comps > 0, nS >= 2^32.  nS = 0 is fine.  The job, the index,
 *   the position map and the mask are neither read nor changed: same digest before and after.
 * Device form: a lock-free union-find over the rows (init, hook, flatten), a hipCUB exclusive sum over the roots'
 *   flags, a pass that writes comp and sums the statistics per wave; n_comps_out and stats are host memory, the call
 *   synchronises ONCE, for them and the error word, and returns with the passes that zero and fill comps enqueued.
 *   d_comps is 8-byte aligned.  Temporary device memory, kept in the context's pool: 8 bytes per unitig and the scan's
 *   scratch; not canonical: 8 more per unitig for the in-degrees the row check counts.  Host form: stages through the
 *   pool; synchronous. */
#define CFRK_COMP_NONE 0xFFFFFFFF
typedef struct cfrk_unitig_component {   /* 32 bytes, no padding */
  uint64_t kc;          /* sum of the members' kc                                      */
  uint64_t n_kmers;     /* sum of the members' n_kmers                                 */
  uint64_t n_links;     /* links of the members' rows whose target is kept, as written */
  uint32_t first;       /* the smallest member unitig                                  */
  uint32_t n_unitigs;   /* number of member unitigs                                    */
} cfrk_unitig_component;
typedef struct cfrk_component_stats {    /* 32 bytes, no padding */
  uint64_t n_components;
  uint64_t n_unitigs;   /* kept                          */
  uint64_t n_kmers;     /* of the kept unitigs           */
  uint64_t n_links;     /* of kept rows, to kept targets */
} cfrk_component_stats;
int cfrk_global_unitig_components_device(cfrk_ctx *ctx, const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr /* nS + 1 */,
                                         const cfrk_unitig_link *d_links, int64_t n_links, const uint8_t *d_drop /* nS; may be NULL */,
                                         uint32_t *d_comp /* nS, every one written */, cfrk_unitig_component *d_comps /* may be NULL */,
                                         uint64_t cap_comps, int64_t *n_comps_out, cfrk_component_stats *stats);
int cfrk_global_unitig_components(cfrk_ctx *ctx, const cfrk_unitig *rec, int64_t nS, const int64_t *link_ptr /* nS + 1 */,
                                  const cfrk_unitig_link *links, int64_t n_links, const uint8_t *drop /* nS; may be NULL */,
                                  uint32_t *comp /* nS */, cfrk_unitig_component *comps /* may be NULL */, uint64_t cap_comps,
                                  int64_t *n_comps_out, cfrk_component_stats *stats);

/* Read components: which read goes with which component (khmer's partitioning of reads), from the hit CSR as
 * cfrk_global_read_hits wrote it for nR reads (hit_ptr[nR + 1], hits[n_hits]; of a hit only unitig and n_windows are
 * read) and comp[nS] of cfrk_global_unitig_components alone.  Needs no job state beyond a begun job.
 *   ELIGIBLE: a hit whose unitig has a component, comp[unitig] != CFRK_COMP_NONE.
 *   The read's DECIDING HIT is the eligible hit with the most windows, on a tie the earliest.  A row of out is
 *   cfrk_read_component: comp = that hit's component, hit = its index inside the read's row, n_windows = its window
 *   count, flags: CFRK_READ_COMP_SPLIT when some other eligible hit of the read lies in a different component,
 *   CFRK_READ_COMP_DROPPED when some hit of the read is not eligible.  A read with no eligible hit gets comp = hit =
 *   0xFFFFFFFF and n_windows = 0 (and CFRK_READ_COMP_DROPPED iff it has a hit at all).
 *   STATISTICS (cfrk_read_component_stats), counting reads: n_assigned, n_unassigned, n_split, n_dropped.
 * Untrusted input: CFRK_ERR_LAYOUT, cfrk_last_error naming the first offending read, when hit_ptr does not start at 0,
 *   descends or leaves [0, n_hits] (hit_ptr[nR] may lie below n_hits: the hits behind it belong to no read and are not
 *   looked at), when a hit's unitig is >= nS or its n_windows is 0.  A refused hit_ptr wins over a refused hit.  After
 *   a refusal out is unspecified and the stats are 0.  Any value of comp[] is taken as given: nothing is indexed by it.
 * CFRK_ERR_ARG: negative sizes, NULL stats or hit_ptr, NULL hits with n_hits > 0, NULL comp with nS > 0, NULL out with
 *   nR > 0, nS >= 2^32, n_hits >= 2^32 (a hit's index inside its row is 32 bits).  CFRK_ERR_STATE: no job.  nR = 0 and
 *   n_hits = 0 are fine.  The job is neither read nor changed.
 * Device form (cfrk_amd/csrc/unitig_components.hip): balanced by HITS.  One lane per hit finds its read by binary
 *   search in hit_ptr and offers (n_windows << 32) | (0xFFFFFFFF - index in row) to a 64-bit atomic maximum per read; a
 *   second pass per hit compares its component with the winner's and ORs the flag bits; one lane per read writes the
 *   row.  A read of 10^5 hits costs what its hits cost.  stats is host memory; the call synchronises ONCE.  Temporary
 *   device memory, kept in the context's pool: 12 bytes per read.  Host form: stages through the pool; synchronous. */
#define CFRK_READ_COMP_SPLIT 1
#define CFRK_READ_COMP_DROPPED 2
typedef struct cfrk_read_component {     /* 16 bytes, no padding */
  uint32_t comp;        /* the deciding hit's component; 0xFFFFFFFF: none */
  uint32_t hit;         /* its index inside the read's hit row; 0xFFFFFFFF: none */
  uint32_t n_windows;   /* its windows */
  uint32_t flags;       /* CFRK_READ_COMP_* */
} cfrk_read_component;
typedef struct cfrk_read_component_stats {   /* 32 bytes, no padding */
  uint64_t n_assigned;
  uint64_t n_unassigned;
  uint64_t n_split;
  uint64_t n_dropped;
} cfrk_read_component_stats;
int cfrk_global_read_components_device(cfrk_ctx *ctx, const int64_t *d_hit_ptr /* nR + 1 */, int64_t nR, const cfrk_read_hit *d_hits,
                                       int64_t n_hits, const uint32_t *d_comp /* nS */, int64_t nS,
                                       cfrk_read_component *d_out /* nR */, cfrk_read_component_stats *stats);
int cfrk_global_read_components(cfrk_ctx *ctx, const int64_t *hit_ptr /* nR + 1 */, int64_t nR, const cfrk_read_hit *hits,
                                int64_t n_hits, const uint32_t *comp /* nS */, int64_t nS, cfrk_read_component *out /* nR */,
                                cfrk_read_component_stats *stats);

/* ---- distinct k-mer estimate: a HyperLogLog sketch of the reads, 1 <= k <= 64 --------------------------------- */

/* How many DISTINCT k-mers will a job hold?  One streaming pass over the reads answers it to about 1 % before anything
 * is counted, so that cfrk_global_begin can be given a capacity_hint that fits (cfrk_sketch_hint) instead of a guess
 * that ends in CFRK_ERR_TABLE_FULL and a second pass.
 * The sketch is CFRK_SKETCH_REGS registers of one byte, in a fixed format:
 *   key      the window's k-mer as in global mode (canonicalised first under CFRK_CANONICAL); the k = 32 all-T key is
 *            an ordinary key here
 *   hash     h = mix(lo) for k <= 32, h = mix(lo ^ mix(hi)) for k > 32: cfrk_debug_hash_info's out[2] / out[3]
 *   bucket   h >> (64 - CFRK_SKETCH_LOG2M)
 *   rank     w = h << CFRK_SKETCH_LOG2M; rank = clz64(w) + 1 when w != 0, otherwise 64 - CFRK_SKETCH_LOG2M + 1 (51)
 *   register the largest rank seen in its bucket (0: none)
 * A window counts by the guarded ComputeFreq rule of global mode: all k codes 0..3, inside [0, nN); terminators are
 * invalid codes, so no window crosses a read.  Two sketches of two read sets merge into the sketch of their union by
 * the element-wise maximum (cfrk_sketch_merge; across processes an all-reduce with MAX).
 * Estimate (cfrk_sketch_estimate): m = CFRK_SKETCH_REGS, alpha = 0.7213 / (1 + 1.079 / m),
 * E = alpha * m^2 / sum(2^-register); when E <= 2.5 m and V > 0 registers are zero, E = m * ln(m / V) (linear
 * counting).  No large-range correction: the hash has 64 bits.  All-zero registers give 0.  The standard error is
 * 1.04 / sqrt(m) = 0.81 %.
 * Hint (cfrk_sketch_hint): ceil(E * (1 + 4 * 1.04 / sqrt(m))) -- four standard errors, 3.25 % -- clamped to
 * [2^20, 2^31]: a capacity_hint that the job's distinct k-mers exceed with negligible probability.
 *
 * cfrk_distinct_sketch_device: d_data 16-byte aligned (CFRK_ERR_ALIGN), flags 0 or CFRK_CANONICAL (anything else, k
 * outside 1..64, negative nN, a NULL d_data or d_regs with nN > 0: CFRK_ERR_ARG).  d_regs = CFRK_SKETCH_REGS bytes on
 * the device, MERGED BY MAXIMUM, not overwritten: the caller zeroes it for a fresh sketch, several calls accumulate
 * into one.  windows_out (may be NULL) receives the exact number of valid windows of THIS call; asking for it
 * synchronises, without it the call returns with the kernels enqueued on the context stream.  nN = 0 is fine.
 * cfrk_distinct_sketch: host buffers, regs on the host (merged by maximum as well); start / length may be NULL and are
 * checked like cfrk_global_add (CFRK_ERR_LAYOUT); stages through the pool; synchronous.
 * Neither call touches a global job that is open on the same context.
 * cfrk_sketch_estimate / _merge / _hint are pure host functions: no context, no device (NULL: CFRK_ERR_ARG). */
#define CFRK_SKETCH_LOG2M 14
#define CFRK_SKETCH_REGS 16384
int cfrk_distinct_sketch_device(cfrk_ctx *ctx, const int8_t *d_data, int64_t nN, int k, int flags, uint8_t *d_regs,
                                uint64_t *windows_out);
int cfrk_distinct_sketch(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length, int64_t nN,
                         int64_t nS, int k, int flags, uint8_t *regs, uint64_t *windows_out);
int cfrk_sketch_estimate(const uint8_t *regs, double *distinct);
int cfrk_sketch_merge(uint8_t *dst, const uint8_t *src);
int cfrk_sketch_hint(const uint8_t *regs, uint64_t *hint);

/* ---- FASTA text parsed on the device: text in, struct-read buffers out --------------------------------------- */

/* nbytes of FASTA text -> data (codes, one -1 terminator behind every read), start, length, nN, nS: byte for byte what
 * the host parser (cfrk_host_parse_fasta, cfrk_amd/host/cfrk_host.h) makes of the same bytes and flags.
 * Grammar: a line ends at '\n' or at the end of the text; a line whose first byte is '>' is a header and starts a
 * record, every other line is a sequence line of the current record; a '>' elsewhere is an ordinary invalid base.
 * aA cC gG tT -> 0 1 2 3, anything else -> -1.
 *   flags 0 (native): a sequence line contributes its bytes without its trailing run of '\n' / '\r' (an interior '\r'
 *     stays and encodes as -1, an empty line contributes nothing); a record may be empty (length 0) and still gets
 *     its terminator; start[r] = kept bytes before record r + r; nN = kept bytes + nS.
 *   CFRK_COMPAT (the reference's ReadFasta, src/fastaIO.h:60-102): a sequence line contributes all its bytes, newline
 *     included (-1); length[r] = contributed bytes - 1, the record's last contributed byte holds the terminator;
 *     start[r] = contributed bytes before record r; nN = contributed bytes.
 * CFRK_ERR_LAYOUT (cfrk_last_error names the cause and the byte offset or the record): non-empty text that does not
 * begin with '>' (a sequence line before the first header), in compat mode a record without a contributed byte, a
 * record of more than 2^31 - 1 bases, and -- the one thing the host parser accepts and this one refuses -- in native
 * mode a SEQUENCE line that holds more than CFRK_FASTA_MAX_CR_RUN carriage returns in a row (the look ahead from a
 * '\r' to its line's end is bounded, so that no text can keep a kernel busy without end).  The bound is exact: a run of
 * CFRK_FASTA_MAX_CR_RUN is parsed as the host parser parses it, a run of one more is refused, wherever it lies; the
 * error names the run's first byte (the first such run's).  Header lines and compat mode have no bound.
 * Empty text: nS = nN = 0.
 * Any flag other than CFRK_COMPAT, a NULL text with nbytes > 0, NULL size outputs and a NULL array with a capacity
 * above 0 are CFRK_ERR_ARG; d_text must be 16-byte aligned (CFRK_ERR_ALIGN), d_data need not be.
 * Capacities: cap_data = nbytes and cap_reads = (nbytes + 1) / 2 always suffice.  A record needs its '>' and, unless
 * it is the text's last line, the '\n' behind it: nS records take at least 2 nS - 1 bytes, so nS <= (nbytes + 1) / 2.
 * A '>' contributes no code, so a record's terminator takes the place of its header's '>' (native: nN = kept + nS <=
 * nbytes; compat: nN = contributed bytes < nbytes).  When nN > cap_data or nS > cap_reads the call returns
 * CFRK_ERR_SMALL_BUF with *nN_out / *nS_out complete and nothing written to the arrays; NULL arrays with zero
 * capacities are that "sizes only" call (as in cfrk_per_read_sparse).
 * Device form: reduce, scan, scatter and a length pass as separate launches on the context stream (no workgroup waits
 * for another one).  It synchronises ONCE, to read the sizes and error words back, and returns with the last kernel
 * enqueued; only a text of 2^31 bytes or more, which alone can hold an over-long record, is waited for at the end as
 * well.  Temporary device memory, kept in the context's pool: 64 bytes + 32 bytes per tile of CFRK_FASTA_TILE_BYTES
 * (an aggregate and its scan: 2 MB per GB of text); the scan walks the tiles in blocks of CFRK_FASTA_SCAN_TILES.
 * Host form: host text in, host arrays out; stages through the pool (the text, then data / start / length); synchronous.
 * Neither call touches a global job that is open on the same context. */
#define CFRK_FASTA_TILE_BYTES 16384
#define CFRK_FASTA_SCAN_TILES 1024
#define CFRK_FASTA_MAX_CR_RUN 4096
int cfrk_fasta_parse_device(cfrk_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, int flags,
                            int8_t *d_data, uint64_t cap_data, int64_t *d_start, int32_t *d_length, uint64_t cap_reads,
                            int64_t *nN_out, int64_t *nS_out);
int cfrk_fasta_parse(cfrk_ctx *ctx, const char *text, uint64_t nbytes, int flags,
                     int8_t *data, uint64_t cap_data, int64_t *start, int32_t *length, uint64_t cap_reads,
                     int64_t *nN_out, int64_t *nS_out);

/* ---- FASTQ text parsed on the device: text in, struct-read buffers out, low-quality bases masked -------------- */

/* nbytes of strict four-line FASTQ text -> data, start, length, nN, nS in the native layout of the FASTA parser above:
 * byte for byte what the host parser (cfrk_host_parse_fastq, cfrk_amd/host/cfrk_host.h) makes of the same bytes.
 * Wrapped (multi-line) FASTQ is refused, not guessed at.  There is no compat mode: the reference reads no FASTQ.
 * Lines: a line ends at '\n' or at the end of the text; the number of lines is the number of '\n', plus one if the
 *   text is non-empty and does not end in '\n' (a trailing '\n' opens no further line; a final EMPTY quality line needs
 *   its '\n').  Lines and records are numbered from 0.
 * Carriage returns: a '\r' directly in front of a '\n', or as the text's last byte, is dropped from its line (one
 *   only); every other '\r' is an ordinary byte of its line.
 * Records: record r is lines 4r .. 4r+3: a line whose first byte is '@' (an empty line fails), the sequence line, a
 *   line whose first byte is '+' (the rest of it is ignored), the quality line.  The kind of a line follows from its
 *   number alone: a quality line that begins with '@', '+' or '>' is an ordinary quality line.
 * Output: data = the codes of the sequence line (aA cC gG tT -> 0 1 2 3, anything else -> -1) and one -1 terminator;
 *   length[r] = bytes of the sequence line; start[r] = bases before record r, plus r; nN = bases + nS; a record may be
 *   empty (length 0).  Empty text: nS = nN = 0.
 * Masking: qualities are Phred+33 (CFRK_FASTQ_QUAL_BASE); min_qual is 0 .. CFRK_FASTQ_MAX_QUAL, anything else is
 *   CFRK_ERR_ARG.  With min_qual >= 1 base j of a record gets code -1 when (int)(unsigned char)qual[j] - 33 < min_qual
 *   (a quality byte below 33 masks, a byte of 128 or more never does); length and start do not change.  With
 *   min_qual = 0 the quality line is only measured and masks nothing, whatever bytes it holds.
 * CFRK_ERR_LAYOUT (cfrk_last_error names the cause and the place; cfrk_host_parse_fastq reports the same cause and
 * place), in this order:
 *   1. structural faults, the one on the earliest line: line 4r does not begin with '@', line 4r+2 does not begin with
 *      '+' (the message names the line and the byte offset of its first byte); a number of lines that is not a
 *      multiple of four (names the number) -- this one counts as lying behind every line;
 *   2. in a structurally sound text, the first record whose sequence and quality lines differ in length;
 *   3. then a record of more than 2^31 - 1 bases.
 * After an error the contents of the output arrays are unspecified; nothing outside the capacities is ever written.
 * A NULL text with nbytes > 0, NULL size outputs and a NULL array with a capacity above 0 are CFRK_ERR_ARG; d_text
 * must be 16-byte aligned (CFRK_ERR_ALIGN), d_data need not be.
 * Capacities: cap_data = nbytes / 2 and cap_reads = (nbytes + 1) / 6 always suffice.  A record of L bases takes
 * '@', '\n', L, '\n', '+', '\n', L and, unless it ends the text, '\n': nS records with B bases in all take at least
 * 2 B + 6 nS - 1 bytes, so nS <= (nbytes + 1) / 6 and, for nS >= 1, nN = B + nS <= (nbytes + 1) / 2 - 2 nS <= nbytes / 2.
 * When nN > cap_data or nS > cap_reads the call returns CFRK_ERR_SMALL_BUF with *nN_out / *nS_out complete and nothing
 * written to the arrays; NULL arrays with zero capacities are that "sizes only" call.  The structural faults are found
 * before the sizes are known and win over CFRK_ERR_SMALL_BUF; the length comparison (2.) and the over-long check (3.)
 * run with the scatter pass, so a sizes-only call on such a text returns its sizes and the call with arrays refuses it.
 * Device form: reduce, one-workgroup scan, scatter, (min_qual > 0) a masking pass and a length pass as separate
 * launches on the context stream (no workgroup waits for another one).  It synchronises TWICE: once to read the sizes
 * and the structural verdict back, and once at its end for the verdict of the length comparison, so the arrays are
 * complete when it returns.  Temporary device memory, kept in the context's pool (the FASTA parser's slot): 128 bytes +
 * 56 bytes per tile of CFRK_FASTQ_TILE_BYTES (3.5 MB per GB of text); the scan walks the tiles in blocks of
 * CFRK_FASTQ_SCAN_TILES.
 * Host form: host text in, host arrays out; stages through the pool (the text, then data / start / length); synchronous.
 * Neither call touches a global job that is open on the same context. */
#define CFRK_FASTQ_TILE_BYTES 16384
#define CFRK_FASTQ_SCAN_TILES 1024
#define CFRK_FASTQ_QUAL_BASE 33
#define CFRK_FASTQ_MAX_QUAL 93
int cfrk_fastq_parse_device(cfrk_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, int min_qual,
                            int8_t *d_data, uint64_t cap_data, int64_t *d_start, int32_t *d_length, uint64_t cap_reads,
                            int64_t *nN_out, int64_t *nS_out);
int cfrk_fastq_parse(cfrk_ctx *ctx, const char *text, uint64_t nbytes, int min_qual,
                     int8_t *data, uint64_t cap_data, int64_t *start, int32_t *length, uint64_t cap_reads,
                     int64_t *nN_out, int64_t *nS_out);

/* ---- select: compact the kept (and trimmed) reads into new struct-read buffers -------------------------------- */

/* Read i is KEPT iff keep is NULL or keep[i] != 0, its span lies inside the read (0 <= offset, 0 <= length,
 * offset + length <= length[i]) and span.length >= min_len; span NULL stands for whole reads ({0, length[i]}).
 * min_len = 0 keeps empty reads as well, which the native layout allows; a negative min_len is CFRK_ERR_ARG.
 * Output: the kept reads in input order in the native layout of the parsers above: the span's bytes copied verbatim
 * and one -1 terminator each; start_out[j] = bytes kept before read j, plus j; length_out[j] = the span's length;
 * *nN_out = kept bytes + *nS_out; index_out[j] (may be NULL) = the input index of output read j.
 * Capacities: cap_data = nN and cap_reads = nS always suffice.  When *nN_out > cap_data or *nS_out > cap_reads the call
 * returns CFRK_ERR_SMALL_BUF with both sizes complete and nothing written to the arrays; NULL arrays with zero
 * capacities are that "sizes only" call.  The output arrays MUST NOT OVERLAP the input arrays.
 * CFRK_ERR_ARG: negative sizes or min_len, NULL size outputs, NULL start / length with nS > 0, NULL data with nN > 0,
 * a NULL output array with a capacity above 0.  nS = 0 is fine.  No alignment requirement on any byte array.
 * Device form: a per-read pass reduced per tile of CFRK_SELECT_TILE_READS reads, a one-workgroup scan of the tile
 * aggregates in blocks of CFRK_SELECT_SCAN_TILES, a pass that writes start_out / length_out / index_out, and the copy,
 * as separate launches on the context stream (no workgroup waits for another one).  The copy is balanced by OUTPUT
 * bytes: one workgroup takes one tile of CFRK_SELECT_TILE_BYTES of data_out and finds the reads that intersect it by a
 * search in start_out.  It synchronises ONCE, for the sizes, and returns with the copy enqueued.  start / length /
 * span are not checked: a read whose range does not lie inside [0, nN), or whose span does not lie inside
 * [0, length[i]] (a negative field included), is dropped silently; nothing outside the buffers is ever accessed.
 * Temporary device memory, kept in the context's pool: 64 bytes, 32 bytes per tile of reads, 8 bytes per kept read.
 * Host form: checks start and length like cfrk_global_add; a span outside its read is CFRK_ERR_LAYOUT as well
 * (cfrk_last_error names the read); stages through the pool; synchronous.
 * Neither call needs a global job or touches one that is open on the same context. */
#define CFRK_SELECT_TILE_BYTES 16384
#define CFRK_SELECT_TILE_READS 256
#define CFRK_SELECT_SCAN_TILES 1024
int cfrk_reads_select_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                             int64_t nN, int64_t nS, const cfrk_read_span *d_span, const uint8_t *d_keep,
                             int32_t min_len, int8_t *d_data_out, uint64_t cap_data, int64_t *d_start_out,
                             int32_t *d_length_out, int64_t *d_index_out, uint64_t cap_reads,
                             int64_t *nN_out, int64_t *nS_out);
int cfrk_reads_select(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length,
                      int64_t nN, int64_t nS, const cfrk_read_span *span, const uint8_t *keep,
                      int32_t min_len, int8_t *data_out, uint64_t cap_data, int64_t *start_out,
                      int32_t *length_out, int64_t *index_out, uint64_t cap_reads,
                      int64_t *nN_out, int64_t *nS_out);

/* ---- text out: the record index of a text, and the kept reads written back as FASTA / FASTQ text ---------------- */

/* The parsers keep no names and no qualities.  The INDEX of a text says where each record's header line and quality
 * line lie in it; the EMITTER writes kept (and trimmed) reads back out as text with their original names and the
 * matching slice of their quality line.  Text stays on the device from file to filtered file.
 *
 * Index.  Defined for EVERY text, not only for the texts a parser accepts: it validates no grammar.
 * Lines (both formats, the FASTQ grammar above): a line ends at '\n' or at the text's end; a trailing '\n' opens no
 *   line; a line's length excludes its '\n' and one '\r' directly in front of that '\n', or one '\r' that is the
 *   text's last byte.  Lines and records are numbered from 0.
 * CFRK_TEXT_FASTA: record r is the r-th line whose first byte is '>' (lines in front of the first header belong to no
 *   record); qual_off = -1, qual_len = 0.  The record numbering of cfrk_fasta_parse_device, in both of its modes.
 * CFRK_TEXT_FASTQ: nS = (number of lines) / 4, rounded down; record r's header is line 4r and its quality line is line
 *   4r + 3, whatever bytes they begin with; an empty line has length 0 and the offset at which it would begin.  For a
 *   text cfrk_fastq_parse_device accepts this is its numbering, and qual_len == length[r].
 * CFRK_ERR_LAYOUT: a header or quality line of more than 2^31 - 1 bytes (cfrk_last_error names the record; only a text
 *   of 2^31 bytes or more can hold one, and only for such a text does the call wait at its end as well).
 * CFRK_ERR_ARG: a format other than the two, a NULL size output, a NULL text with nbytes > 0, a NULL array with
 *   cap_reads > 0.  CFRK_ERR_ALIGN: d_text not 16-byte aligned.  Empty text: nS = 0.
 * Capacities: cap_reads = (nbytes + 1) / 2 (FASTA) and (nbytes + 1) / 4 (FASTQ: four lines take at least three '\n')
 *   always suffice; for a text its parser accepts, so does the parser's bound.  When nS > cap_reads the call returns CFRK_ERR_SMALL_BUF with *nS_out complete and
 *   nothing written; a NULL array with capacity 0 is that "sizes only" call.
 * Device form: a tile reduce, a one-workgroup scan of the tile aggregates in blocks of CFRK_TEXT_SCAN_TILES and a
 *   scatter, as separate launches on the context stream (no workgroup waits for another one; the work per thread is
 *   bounded whatever the text holds).  The thread on a line's closing '\n' (or on the text's last byte) writes the
 *   line's fields; the line may have begun any number of tiles before, so the scan carries the start of the line that
 *   is open at a tile's beginning, whether that line is a header (FASTA) and the count that numbers the records (FASTQ:
 *   newlines, FASTA: header lines).  It synchronises ONCE, for nS, and returns with the scatter enqueued.  Temporary
 *   device memory, kept in the context's pool: 64 bytes + 24 bytes per tile of CFRK_TEXT_TILE_BYTES.
 * Host form: host text in, host records out; stages through the pool; synchronous.
 *
 * Emitter.  Read i is KEPT by exactly the rule of cfrk_reads_select (keep, span inside the read, min_len; span NULL =
 * whole reads); its name and qualities come from rec[i], the index of the text the reads were parsed from (nS entries).
 * Output, the kept reads in input order:
 *   CFRK_TEXT_FASTA   '>' name '\n' bases '\n'
 *   CFRK_TEXT_FASTQ   '@' name '\n' bases "\n+\n" quals '\n'
 *   name  = the header line without its first byte: head_len - 1 bytes from head_off + 1 (nothing when head_len is 0),
 *           copied verbatim;  bases = the span's codes as ACGT, N for any other code (cfrk_host_format_fasta's rule: a
 *           base masked by min_qual reads N);  quals = text[qual_off + span.offset .. + span.length), copied verbatim.
 *   *nbytes_out = bytes of text, *nS_out = reads written.
 * Capacities: when *nbytes_out > cap_out the call returns CFRK_ERR_SMALL_BUF with both sizes complete and nothing
 *   written; NULL with capacity 0 is the "sizes only" call.  d_out must not overlap the inputs.
 * A record's header range is [head_off, head_off + head_len), its quality range [qual_off, qual_off + qual_len); the
 *   pair {-1, 0} (what the FASTA index writes) stands for "no quality line" and is a valid quality range.
 * Device form: checks nothing and never reads or writes outside its buffers.  In addition to the select's silent
 *   drops, a read is dropped when its record's header or quality range does not lie inside [0, nbytes] (a negative
 *   field included), or when the output is FASTQ and the record has no quality line or qual_len != length[i].
 *   A per-read measure pass reduced per tile of CFRK_SELECT_TILE_READS reads, a one-workgroup scan in blocks of
 *   CFRK_SELECT_SCAN_TILES, a pass that writes each kept read's output offset and input index (8 + 8 bytes per kept
 *   read in the pool), and the copy, balanced by OUTPUT bytes: one workgroup per CFRK_EMIT_TILE_BYTES of d_out finds the
 *   reads that meet its tile by a search in the output offsets, gathers name bytes, translated codes, literal bytes and
 *   quality bytes through LDS and writes whole 16-byte blocks.  It synchronises ONCE, for the sizes, and returns with
 *   the copy enqueued.  No alignment requirement on any byte array.
 * Host form: refuses all of the above with CFRK_ERR_LAYOUT (cfrk_last_error names the read), for every read whatever
 *   its keep byte; checks start / length like cfrk_global_add; stages through the pool; synchronous.
 * CFRK_ERR_ARG: as the select (negative sizes or min_len, NULL size outputs, NULL start / length with nS > 0, NULL data
 *   with nN > 0, NULL output with a capacity above 0), an out_format other than the two, a NULL rec with nS > 0, a NULL
 *   text with nbytes > 0.  nS = 0 is fine.
 * None of the four calls needs a global job or touches one that is open on the same context. */
#define CFRK_TEXT_FASTA 0
#define CFRK_TEXT_FASTQ 1
#define CFRK_TEXT_TILE_BYTES 16384
#define CFRK_TEXT_SCAN_TILES 1024
#define CFRK_EMIT_TILE_BYTES 16384
typedef struct cfrk_text_record {   /* 24 bytes, no padding */
  int64_t head_off;   /* offset in the text of the header line's first byte (its '>' / '@')        */
  int64_t qual_off;   /* FASTQ: offset of the quality line's first byte; FASTA: -1                 */
  int32_t head_len;   /* bytes of the header line, marker included, line end excluded              */
  int32_t qual_len;   /* FASTQ: bytes of the quality line, line end excluded; FASTA: 0             */
} cfrk_text_record;
int cfrk_text_index_device(cfrk_ctx *ctx, const uint8_t *d_text, uint64_t nbytes, int format,
                           cfrk_text_record *d_rec, uint64_t cap_reads, int64_t *nS_out);
int cfrk_text_index(cfrk_ctx *ctx, const char *text, uint64_t nbytes, int format,
                    cfrk_text_record *rec, uint64_t cap_reads, int64_t *nS_out);
int cfrk_reads_emit_text_device(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                                int64_t nN, int64_t nS, const cfrk_read_span *d_span, const uint8_t *d_keep,
                                int32_t min_len, const uint8_t *d_text, uint64_t nbytes,
                                const cfrk_text_record *d_rec, int out_format, uint8_t *d_out, uint64_t cap_out,
                                uint64_t *nbytes_out, int64_t *nS_out);
int cfrk_reads_emit_text(cfrk_ctx *ctx, const int8_t *data, const int64_t *start, const int32_t *length,
                         int64_t nN, int64_t nS, const cfrk_read_span *span, const uint8_t *keep,
                         int32_t min_len, const char *text, uint64_t nbytes,
                         const cfrk_text_record *rec, int out_format, char *out, uint64_t cap_out,
                         uint64_t *nbytes_out, int64_t *nS_out);

/* ---- paired-end reads: the two mates of a pair are kept or dropped together ----------------------------------- */

/* Addressing, for every call of this section: mate A of pair j is element j * stride of the *_a arrays and mate B is
 * element j * stride of the *_b arrays.  One form serves both layouts a caller has:
 *   interleaved   one array of 2 * n_pairs elements, b = a + 1, stride = 2 (mates are reads 2j and 2j + 1)
 *   split         two arrays of n_pairs elements, stride = 1
 *
 * Join of keep decisions.  A read SURVIVES iff keep is NULL or its keep byte is non-zero, and
 *   with a span: the span lies inside the read (0 <= offset, 0 <= length, offset + length <= length[i]) and
 *                span.length >= min_len;
 *   with span NULL: length[i] >= min_len (length may be NULL when min_len is 0: nothing is asked of the read then).
 * This is the rule of cfrk_reads_select and of the emitter WITHOUT their range check of start: neither the data nor
 * start is an argument here, so a read whose [start, start + length) does not lie inside its buffer survives the join
 * and is still dropped by the select / the emitter.  The host forms of those refuse such a table; a caller of their
 * device forms who does not trust start checks it first.
 * With sA and sB the survival of the two mates of a pair:
 *   CFRK_PAIR_BOTH     pair = sA & sB;  orphan_a = sA & !sB;  orphan_b = sB & !sA
 *   CFRK_PAIR_EITHER   pair = sA | sB;  orphan_a = orphan_b = 0   (khmer's --paired rule: a pair stays whole)
 * pair_a[j * stride] = pair_b[j * stride] = pair; orphan_a / orphan_b (each may be NULL) likewise.  Every byte
 * written is 0 or 1; with stride 2 the bytes between the addressed ones are not touched.  counts (may be NULL) gets
 * pairs kept, orphans A, orphans B and pairs dropped (pair = 0 and no orphan): the four sum to n_pairs under
 * CFRK_PAIR_BOTH, the first and the last do under CFRK_PAIR_EITHER.
 * The outputs MAY ALIAS the keep inputs (pair_a = keep_a, pair_b = keep_b: the in-place use; every thread reads both
 * mates before it writes either) and must not overlap anything else, nor each other.
 * CFRK_ERR_ARG: negative n_pairs or min_len, a stride other than 1 or 2, a mode other than the two, a NULL length_a /
 * length_b with that side's span or with min_len > 0, NULL pair_a / pair_b with n_pairs > 0.  keep, span and orphan
 * arrays are NULL or not side by side.  n_pairs = 0 is fine (counts = 0).
 * Device form: one launch on the context stream, one thread per pair and turn; the counts are reduced per wave, then
 * per workgroup, and added once per workgroup; it synchronises once, for the counts row, and not at all when counts is NULL.  Nothing is
 * checked and nothing outside the addressed elements is accessed.
 * Host form: gathers the addressed elements, runs the device form, scatters the results; synchronous.
 *
 * Mate-name check.  The IDENTIFIER of a record is the bytes of its header line behind the marker (head_len - 1 bytes
 * from head_off + 1) up to but not including the first space or tab; head_len <= 1 gives the empty identifier.  If A's
 * identifier ends in "/1" and B's ends in "/2", both suffixes are dropped.  A pair is GOOD iff both header ranges lie
 * inside their text ([0, nbytes], a negative field is outside) and the two identifiers are byte-equal and not empty.
 * So "name/1" pairs with "name/2" and the Casava-1.8 form "name 1:N:0:.." pairs with "name 2:N:0:.."; "/2" in front of
 * "/1" is bad.  *first_bad = the smallest bad pair index or -1, *n_bad = the number of bad pairs; CFRK_OK either way.
 * The mates may live in one text (text_b = text_a) or in two.
 * CFRK_ERR_ARG: negative n_pairs, a stride other than 1 or 2, NULL outputs, NULL records with n_pairs > 0, a NULL text
 * with nbytes > 0.  No alignment requirement.
 * Device form: never reads outside the two texts.  Two launches over all pairs: pairs whose names are both at most
 * CFRK_PAIR_NAME_FAST bytes go to a group of 16 lanes, a lane comparing one 16-byte piece; a pair with a longer name
 * goes to a whole workgroup.  Synchronises once, for the two results.
 * Neither call needs a global job or touches one that is open on the same context. */
#define CFRK_PAIR_BOTH 0
#define CFRK_PAIR_EITHER 1
#define CFRK_PAIR_NAME_FAST 256
typedef struct cfrk_pair_counts {   /* 32 bytes, no padding */
  int64_t pairs;       /* pairs kept                                  */
  int64_t orphans_a;   /* A mates that survive alone (CFRK_PAIR_BOTH) */
  int64_t orphans_b;   /* B mates that survive alone (CFRK_PAIR_BOTH) */
  int64_t dropped;     /* pairs of which nothing is kept              */
} cfrk_pair_counts;
int cfrk_reads_pair_keep_device(cfrk_ctx *ctx, int64_t n_pairs, int stride, int mode, int32_t min_len,
                                const uint8_t *d_keep_a, const uint8_t *d_keep_b,
                                const cfrk_read_span *d_span_a, const cfrk_read_span *d_span_b,
                                const int32_t *d_length_a, const int32_t *d_length_b,
                                uint8_t *d_pair_a, uint8_t *d_pair_b, uint8_t *d_orphan_a, uint8_t *d_orphan_b,
                                cfrk_pair_counts *counts);
int cfrk_reads_pair_keep(cfrk_ctx *ctx, int64_t n_pairs, int stride, int mode, int32_t min_len,
                         const uint8_t *keep_a, const uint8_t *keep_b,
                         const cfrk_read_span *span_a, const cfrk_read_span *span_b,
                         const int32_t *length_a, const int32_t *length_b,
                         uint8_t *pair_a, uint8_t *pair_b, uint8_t *orphan_a, uint8_t *orphan_b,
                         cfrk_pair_counts *counts);
int cfrk_text_pair_check_device(cfrk_ctx *ctx, int64_t n_pairs, int stride,
                                const uint8_t *d_text_a, uint64_t nbytes_a, const cfrk_text_record *d_rec_a,
                                const uint8_t *d_text_b, uint64_t nbytes_b, const cfrk_text_record *d_rec_b,
                                int64_t *first_bad, int64_t *n_bad);
int cfrk_text_pair_check(cfrk_ctx *ctx, int64_t n_pairs, int stride,
                         const char *text_a, uint64_t nbytes_a, const cfrk_text_record *rec_a,
                         const char *text_b, uint64_t nbytes_b, const cfrk_text_record *rec_b,
                         int64_t *first_bad, int64_t *n_bad);

/* Unsorted export into device buffers, grouped into `parts` contiguous segments by
 * owner(key) = (mix(key) >> 32) % parts (key-owner partition for the multi-GPU
 * merge).  part_counts (host, `parts` entries) receives the segment sizes.  Synchronises. */
int cfrk_global_export_device(cfrk_ctx *ctx, uint64_t *d_keys_lo, uint64_t *d_keys_hi,
                              uint32_t *d_counts, uint64_t cap, int parts, uint64_t *part_counts);

/* Multi-GPU exchange by LEAF (the partitioned path's unit of disjoint key space; same k => same
 * leaf on every rank): owner(leaf) = leaf % parts.  Export writes this rank's result grouped by
 * owner (part p = leaves p, p+parts, ... in that order), part_counts[p] entries each, and the
 * per-leaf entry counts in the same order to d_leaf_counts (parts * cfrk_global_leaves_per_part
 * uint32).  d_keys_hi receives / supplies the high key words for k > 32 and is NULL otherwise.
 * CFRK_ERR_STATE when the result is not in per-leaf list form (k < 16, something spilled to the
 * HBM table, several adds or passes): use cfrk_global_export_device instead.
 * Merge, on a context fresh from cfrk_global_begin: d_keys/d_counts = the received runs in rank
 * order (recv_counts[r] entries from rank r), d_leaf_counts = the received per-leaf counts
 * ([parts][leaves_per_part]); every leaf's lists are added in an LDS table (no HBM atomics). */
int cfrk_global_leaves_per_part(int parts);
int cfrk_global_export_leaves_device(cfrk_ctx *ctx, uint64_t *d_keys, uint64_t *d_keys_hi, uint32_t *d_counts,
                                     uint64_t cap, int parts, uint64_t *part_counts, uint32_t *d_leaf_counts);
int cfrk_global_merge_leaves_device(cfrk_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_keys_hi,
                                    const uint32_t *d_counts, const uint64_t *recv_counts,
                                    const uint32_t *d_leaf_counts, int parts);

/* Multi-GPU exchange at RUN granularity -- the strong-scaling form (replaces the pthread fan-out of
 * src/main.cu:277-295; the reference has no merge step).  With the reads of ONE job split over N
 * ranks every rank still meets almost every locus, so counting per rank and exchanging counted
 * k-mers makes every rank expand every distinct k-mer.  Instead a rank begins with CFRK_RUNS_ONLY,
 * adds its shard once (partition + deduplication only) and exports, per leaf, its distinct complete
 * runs with multiplicities followed by its truncated runs (read ends).  A truncated run that is a
 * prefix of one of the rank's own distinct complete runs is sent as a 16-bit NOTE (position of that
 * run in the leaf's list << 5 | k-mers - 1) instead of a 16-byte record.  The export is PACKED for
 * one all-to-all: 16-byte rows, one segment per owner (owner p = leaves p, p+parts, ...) = a header
 * (the owner's leaves_per_part x (distinct, truncated, noted) sizes as uint32 triples, padded to
 * whole rows) followed, leaf after leaf, by the distinct runs, the truncated runs and the notes
 * (eight per row); part_rows[p] = rows of segment p.  The owner, on a context fresh from
 * cfrk_global_begin (same k and strand flag, without CFRK_RUNS_ONLY), passes the received segments
 * in rank order (recv_rows[r] rows from rank r): the lists of each of its leaves become that leaf's
 * streams and are expanded and counted once.  Afterwards the owner holds the final counts of its
 * leaves' k-mers (finish / export / digest as usual).  parts <= 64.  CFRK_ERR_STATE from the export
 * when part of the shard was counted in the HBM table instead: use the leaf or key-owner exchange. */
int cfrk_global_export_runs_device(cfrk_ctx *ctx, void *d_packed, uint64_t cap_rows, int parts,
                                   uint64_t *part_rows);
int cfrk_global_merge_runs_device(cfrk_ctx *ctx, const void *d_packed, const uint64_t *recv_rows, int parts);

/* PIPELINED form of the exchange by runs (round 5; both key widths, a 32-byte record of k > 32 travels as two rows).  The owners' leaves are cut into `ngroups` ranges of
 * local leaf indices (group g = local leaves [lpp * g / ngroups, lpp * (g + 1) / ngroups), lpp = cfrk_global_leaves_per_part);
 * a rank deduplicates and packs group after group straight into the send buffer and hands every finished group to the
 * wire while the next one is in the works, the owner counts every received group while the next one is on the wire:
 *     rank:  begin(CFRK_RUNS_ONLY | CFRK_RUNS_DEFER), add_device (returns with the kernels enqueued),
 *            export_runs_async (enqueues everything, returns at once),
 *            for g: export_runs_wait(g) -> rows per owner -> all-to-all of group g (segment (g, p) to owner p)
 *     owner: begin (same k and strand flag), for g: merge_runs_group_device(g) (enqueued, no host synchronisation)
 * Send buffer: segment (g, p) = rows [(g * parts + p) * seg_cap_rows, ...), 16-byte rows; only its first part_rows[p]
 * rows travel.  Segment = header (row 0: {rows used, local leaves of the group, first local leaf, magic}; then per local
 * leaf a uint4 {row offset behind the header, distinct, truncated, noted}) + the leaves' rows in the order they were
 * claimed: [distinct complete runs with multiplicities][truncated runs][16-bit notes, eight per row].
 * export_runs_wait: waits for group g only (one event); CFRK_ERR_SMALL_BUF when a segment of the group ran out of room
 * (seg_cap_rows too small), CFRK_ERR_STATE when the add overflowed a region or spilled (the shard's runs are not all in
 * the leaf streams): in both cases nothing of the group may be sent -- add again without CFRK_RUNS_DEFER and take
 * cfrk_global_export_runs_device, or count the shard and exchange counts.  The leaf streams stay as the add left them,
 * so cfrk_global_export_runs_device may follow on the same job.
 * merge_runs_group_device: d_recv = the `parts` received segments of group g in rank order (recv_rows[r] rows from rank
 * r).  Groups must be merged in order, 0 .. ngroups-1, on a context fresh from cfrk_global_begin; the call returns with
 * the leaf kernel enqueued (it reads the lists in place: d_recv must stay untouched until the context is synchronised).
 * A segment whose header does not add up is not followed and makes finish / digest fail with CFRK_ERR_TABLE_FULL.
 * parts <= 64, ngroups <= 16.  Replaces the pthread fan-out of src/main.cu:277-295 (which has no merge step). */
int cfrk_global_export_runs_async(cfrk_ctx *ctx, void *d_packed, uint64_t seg_cap_rows, int parts, int ngroups);
int cfrk_global_export_runs_wait(cfrk_ctx *ctx, int group, uint64_t *part_rows);
int cfrk_global_merge_runs_group_device(cfrk_ctx *ctx, const void *d_recv, const uint64_t *recv_rows, int parts,
                                        int group, int ngroups);
/* Device time (ms, HIP events) from the start of the job's add to the end of group `group` of the pipelined export;
 * synchronises on that group.  (cfrk_global_last_add_ms after cfrk_global_merge_runs_group_device: the owner's kernels
 * from group 0 up to the last group merged.) */
int cfrk_global_runs_group_ms(cfrk_ctx *ctx, int group, float *ms);

/* Order-independent digest: out[0]=distinct, out[1]=sum count,
 * out[2]=sum count*splitmix64(kh) mod 2^64, out[3]=xor splitmix64(kh ^ count);
 * kh = lo (k<=32) or lo + splitmix64(hi). Synchronises.  CFRK_ERR_COUNT_OVERFLOW: out[] is
 * filled, computed over the saturated counts. */
int cfrk_global_digest(cfrk_ctx *ctx, uint64_t out[4]);

/* Device time (ms, HIP events on the context stream) of the counting kernels of the most
 * recent cfrk_global_add / cfrk_global_add_device; synchronises. */
int cfrk_global_last_add_ms(cfrk_ctx *ctx, float *ms);

/* Diagnostics of the minimizer-partitioned path after the most recent add (synchronises):
 * out[0..2] = level-1 records: total, largest bin, bin capacity; out[3..5] = level-2 records:
 * total, largest leaf, leaf capacity; out[6] = records and out[7] = k-mer insertions (each may
 * carry a multiplicity) that were counted in the HBM table instead (spill); out[8] = entries in
 * the leaf-output list. */
int cfrk_debug_msp_info(cfrk_ctx *ctx, uint64_t out[9]);

/* Cap (bytes, 0 = none) on the device memory the partitioned counting paths may use for their
 * record buffers.  A batch whose buffers exceed what is available is counted in several passes
 * over ranges of the input, each pass folded into the HBM table; this knob makes that
 * behaviour reachable with small inputs (tests) and lets a host that shares the GPU hold the
 * library to a budget.  out_passes (may be NULL) receives the passes of the most recent add. */
int cfrk_debug_set_mem_budget(cfrk_ctx *ctx, uint64_t bytes);
/* Device memory the context holds right now: its pool (record buffers, result list, staging) plus the
 * global table.  The caller's own buffers (the reads handed to cfrk_global_add_device) are not in it. */
int cfrk_debug_device_bytes(cfrk_ctx *ctx, uint64_t *out_bytes);
int cfrk_debug_last_add_passes(cfrk_ctx *ctx, int *out_passes);

/* Read-only introspection of the hashed structures, so that a test can craft keys that collide and notices when the
 * hash or a sizing rule changes.  out[0] = log2 of the slots of the job's HBM table (0 before cfrk_global_begin);
 * out[1] = log2 of the slots of the job's query index (0 while no hash index is valid: before the first query, after
 * every call that changes the result, and for k <= 12, whose index is a dense array); out[2] = the 64-bit hash of the
 * one-word key lo, out[3] = that of the two-word key (lo, hi) -- a key's home slot in a structure of 2^n slots is the
 * hash's top n bits.  The hashes are evaluated on the host by the very function the kernels call, need no device and
 * no context: ctx may be NULL (out[0] = out[1] = 0).  Touches nothing; never synchronises. */
int cfrk_debug_hash_info(const cfrk_ctx *ctx, uint64_t lo, uint64_t hi, uint64_t out[4]);

/* Read-only introspection of the radix path (global jobs with k <= 16), so that a test can craft keys for a chosen
 * leaf and counter, and notices when the scramble or a sizing rule changes.  The shape is evaluated on the host by the
 * very function the add chooses it with, from k and the batch size nN (bytes of reads) alone; it needs no device and no
 * context: ctx may be NULL.  out[0] = b1, out[1] = b2 (bits of the two partition levels), out[2] = idx (bits that
 * address a leaf's counters: a scrambled key is bin : sub-bin : counter, top to bottom); out[3] = the odd multiplier
 * of the scramble x * mul mod 4^k, out[4] = its inverse mod 2^32; out[5] = cap1, out[6] = cap2 (elements a level-1
 * region and a leaf hold before the level is laid out again with exact sizes); out[7] = flags: bit 0 a batch of nN at
 * this k is counted by the radix path (every k <= 15; k = 16 up to ~3.5e9 bases; the job's flags and debug bits, which
 * can also keep k = 16 away from it, are not looked at), bit 1 k <= 7 (no partition: one dense table in LDS; out[0..6]
 * are 0), bit 2 level 1 keeps an 8-bit plane beside its 16-bit plane.  k outside 1..16: all of out[0..7] are 0.
 * With a context, out[8..11] tell what its most recent radix add did (0 without one, or before the first): out[8] =
 * attempts of the layout loop (1: every region and leaf fitted its fixed stride; 0 for k <= 7), out[9] = 1 when level 1
 * was laid out again, out[10] = 1 when the leaves were, out[11] = workgroups of the leaf kernel (k <= 7: of the
 * counting kernel) -- workgroup w walks leaves w, w + out[11], ...  Host-side values the add had in hand: touches
 * nothing, never synchronises. */
int cfrk_debug_radix_info(const cfrk_ctx *ctx, int k, int64_t nN, uint64_t out[12]);

/* Test switches for rarely taken device paths (0 = normal operation).  Bit 0: every leaf of the
 * one-word partitioned path (16 <= k <= 32) is treated as if its complete runs had overflowed the
 * record table, i.e. takes the second-chance deduplication over the whole LDS pool. */
#define CFRK_DEBUG_FORCE_RT_OVERFLOW 0x1
/* Bit 1: the first partition kernel (k >= 16) holds one trip's worth (64) of a wave's runs in
 * registers instead of 4..8: the rest takes the direct-append path meant for pathological waves. */
#define CFRK_DEBUG_SMALL_WAVE_CAP 0x2
/* Bit 2: the leaf kernel of the one-word partitioned path counts every truncated run k-mer by k-mer
 * instead of noting it with the complete run it is a prefix of (same result; for A/B timing and tests). */
#define CFRK_DEBUG_NO_ANCHORS 0x4
/* Bit 3: the two-word partitioned path (33 <= k <= 64) writes extra minimizer-hash bits into its
 * records and lets four workgroups share every leaf, each taking the records its bits name,
 * whatever the capacity hint (normally only for hints above ~2.7e8 distinct k-mers, 2..32
 * workgroups per leaf): makes that path reachable with small inputs (tests). */
#define CFRK_DEBUG_RECORD_SUBSETS 0x8
/* Bit 4: the partitioned paths (k >= 16) never count in chunks (a large batch is normally cut into
 * chunks of tiles -- partition kernel on chunk c, then second-level kernel on chunk c -- so that the
 * level-1 buffer holds one chunk and the leaf streams are sized from the first chunk's records); same
 * result, for A/B timing.  Bit 5: count in chunks of a few tiles whatever the batch size: makes the
 * chunked path reachable with small inputs (tests). */
#define CFRK_DEBUG_NO_PIPELINE 0x10
#define CFRK_DEBUG_SMALL_PIPELINE 0x20
/* Bit 6: k = 16 never takes the radix path (normally it does for adds of up to ~4e9 bases: the minimizer window of
 * the partitioned path is only four k-mers at k = 16); makes the partitioned path at k = 16 reachable with small
 * inputs (tests). */
#define CFRK_DEBUG_NO_RADIX16 0x40
/* Bit 7: the two-word leaf kernel keeps its 4096-slot k-mer table (one workgroup per CU) also for jobs that announce few
 * distinct k-mers per leaf, which normally take the 1024-slot instantiation (two per CU); keeps the large instantiation
 * reachable with small inputs (tests). */
#define CFRK_DEBUG_NO_SMALL_LEAVES 0x80
/* Any other bit is refused with CFRK_ERR_ARG.  (The timing ablations that skip a kernel phase and so produce WRONG
 * counts -- cfrk_amd/csrc/msp.h: CFRK_ABL_* -- are compiled into a separate ablation build only, `make -C
 * cfrk_amd/csrc abl`; the product library does not contain them.) */
int cfrk_debug_set_flags(cfrk_ctx *ctx, uint32_t flags);

/* Sizing knobs of the partitioned paths for experiments and tests (value 0 = the library's own choice;
 * out-of-range values are refused with CFRK_ERR_ARG).  The library reads NO environment variables. */
#define CFRK_PARAM_MSP_CHUNKS          0  /* 1 .. 4096: chunks a large batch is counted in (16 <= k <= 32)            */
#define CFRK_PARAM_L2_SLACK_COMPLETE   1  /* 1 .. 16: leaf-stream room for complete runs, x the measured mean share   */
#define CFRK_PARAM_L2_SLACK_TRUNCATED  2  /* 1 .. 16: the same for truncated runs                                     */
#define CFRK_PARAM_MSP2_SUBVALUE_BITS  3  /* 1 .. 3: log2(sub-values one workgroup of a shared leaf counts) + 1
                                             (33 <= k <= 64; normally chosen from the expected runs per leaf)         */
#define CFRK_PARAM_UNITIG_SPLIT_LOG2   4  /* 1 .. 20: s + 1, s = log2 of the unitig call's splitter period (s = 0:
                                             every node is a splitter); 0 = CFRK_UNITIG_SPLIT_LOG2_DEFAULT            */
int cfrk_debug_set_param(cfrk_ctx *ctx, int which, double value);

/* ---- synthetic reads, generated on device ----------------------------------- */

/* Reads [r0, r0+R) of the deterministic generator, struct-read layout: d_data R*(L+1) bytes,
 * d_start R int64 (may be NULL), d_length R int32 (may be NULL). */
int cfrk_synth_reads_device(cfrk_ctx *ctx, int64_t r0, int64_t R, int L, int64_t Glen,
                            uint64_t seedG, uint64_t seedR, uint64_t seedS, int uniform,
                            int8_t *d_data, int64_t *d_start, int32_t *d_length);

#ifdef __cplusplus
}
#endif
#endif
