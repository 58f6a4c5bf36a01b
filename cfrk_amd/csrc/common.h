// common.h -- context, error plumbing and device helpers shared by the gfx950 kernels.
// Product code: must never include or link anything under oracle/.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/cfrk_abi.h"

#define CFRK_EMPTY_KEY 0xFFFFFFFFFFFFFFFFull
// internal (never leaves the library): a partitioned path found 2^32 records in one stream (ST_CWRAP) -- a single-key
// flood; cfrk_global_add_device counts the add through the HBM table instead
#define CFRK_INTERNAL_FLOOD (-100)
#define CFRK_MAX_PROBE (1u << 22)
#define CFRK_RUNS_MAX_GROUPS 16

enum {  // pool slots
  BUF_DATA = 0,                               // staging of cfrk_global_add and cfrk_per_read_dense (reads in)
  BUF_START, BUF_LENGTH, BUF_FREQ,            // staging of cfrk_per_read_dense alone
  BUF_SPILL, BUF_EXPORT_LO, BUF_EXPORT_HI,
  BUF_EXPORT_CNT, BUF_SCRATCH, BUF_MSP_L1, BUF_MSP_L2, BUF_MSP_OUTK, BUF_MSP_OUTC, BUF_MSP_AUX, BUF_MSP_OUTH,
  BUF_MSP_ACCK, BUF_MSP_ACCH, BUF_MSP_ACCC,   // lists of the passes of a multi-pass add, merged per leaf at the end
  BUF_MSP_LAYOUT,                             // exact second-level layout (stream bases and sizes)
  BUF_MSP_OVF,                                // records that did not fit their leaf stream (a few)
  BUF_MSP_OVF1, BUF_MSP_LAYOUT1,              // the same for the level-1 regions
  BUF_RUNS_AUX,                               // pipelined runs exchange: segment cursors, used rows per group
  BUF_QUERY_INDEX,                            // read-only lookup index of the result (query.hip)
  BUF_QUERY_IN, BUF_QUERY_OUT,                // staging of host forms (staging.h).  IN: cfrk_global_query (keys), _query_reads, _read_stats,
                                              // _read_spans, cfrk_distinct_sketch (reads), cfrk_global_normalize (reads and keep bytes),
                                              // cfrk_global_correct_reads (reads in; corrected data and rows out);
                                              // OUT: the first four (counts or rows)
  BUF_SPARSE_KEYS, BUF_SPARSE_CNT,            // per-read sparse (sparse.hip): the rows at their reads' offsets, nN entries
  BUF_SPARSE_AUX,                             // block sums of the row-pointer scan
  BUF_SPARSE_IN, BUF_SPARSE_OUT,              // staging of cfrk_per_read_sparse alone (data, start, length, row_ptr in; keys, counts out)
  BUF_SKETCH,                                 // distinct sketch (sketch.hip): the workgroups' merged registers as words, the window count, the host form's registers
  BUF_FASTA,                                  // FASTA and FASTQ parsers (ingest.hip, ingest_fastq.hip), both forms: size / error words, tile aggregates, their scan
  BUF_FASTA_IN, BUF_FASTA_OUT,                // staging of cfrk_fasta_parse and cfrk_fastq_parse (text in; data, start, length out)
  BUF_SELECT,                                 // select (read_filter.hip): size words, the read tiles' aggregates, their scan
  BUF_SELECT_SRC,                             // the kept reads' source offsets
  BUF_SELECT_IN, BUF_SELECT_OUT,              // staging of cfrk_reads_select alone (reads, spans, keep in; the selected reads and their index out)
  BUF_TEXT_INDEX,                             // text index (text_out.hip), both forms: size / error words, tile aggregates, their scan
  BUF_TEXT_IN, BUF_TEXT_OUT,                  // staging of cfrk_text_index alone (text in; records out)
  BUF_EMIT,                                   // text emitter (text_out.hip): size words, the read tiles' aggregates, their scan
  BUF_EMIT_OFF,                               // the kept reads' output offsets and input indices
  BUF_EMIT_IN, BUF_EMIT_OUT,                  // staging of cfrk_reads_emit_text alone (reads, spans, keep, records, text in; text out)
  BUF_NORMALIZE,                              // normalise (normalize.hip): the call's kept-read counter; a paired call's four pair counts behind it
  BUF_PAIRS,                                  // pairs (pairs.hip): the join's four counts, the name check's two results
  BUF_PAIRS_IN,                               // staging of cfrk_reads_pair_keep and cfrk_text_pair_check alone
  BUF_UNITIG,                                 // unitigs (unitigs.hip): counters, the per-slot bytes, segments, unitig records
  BUF_UNITIG_AUX,                             // the sort's payload, the lengths and their scan
  BUF_UNITIG_OUT,                             // staging of cfrk_global_unitigs alone (data, start, length, records out)
  BUF_UNITIG_LINKS,                           // unitig links (unitig_links.hip): error / size words, the per-slot tags, the ends' counts and their scan
  BUF_UNITIG_POS,                             // position map (unitig_locate.hip): error words, one cfrk_unitig_pos per slot of the lookup index;
                                              // valid while ctx->upos_epoch is the index's epoch
  BUF_READ_HITS,                              // read hits (unitig_locate.hip): the scratch of the hit_ptr scan
  BUF_UNITIG_MASK,                            // graph mask (unitig_mask.hip): one byte per slot of the lookup index; valid while
                                              // ctx->umask_epoch is the index's epoch
  BUF_UNITIG_MASK_AUX,                        // the mask count's word
  BUF_UNITIG_TIPS,                            // tip rule (unitig_tips.hip): error / size words, in-degrees, in-row offsets and rows, the scan's scratch
  BUF_UNITIG_TIPS_IN, BUF_UNITIG_TIPS_OUT,    // staging of cfrk_global_unitig_tips alone (records, link_ptr, links in; tip bytes out)
  BUF_UNITIG_BUBBLES,                         // bubble rule (unitig_bubbles.hip): error / size words, arm bytes and records, the in-rows, the scan's scratch
  BUF_UNITIG_BUBBLES_IN, BUF_UNITIG_BUBBLES_OUT,  // staging of cfrk_global_unitig_bubbles alone (records, link_ptr, links in; pop bytes and partners out)
  BUF_UNITIG_BULGES,                          // bulge rule (unitig_bulges.hip): error / size words, the arm list, the popped list, the in-rows, the scans' scratch
  BUF_UNITIG_BULGES_IN, BUF_UNITIG_BULGES_OUT,  // staging of cfrk_global_unitig_bulges alone (records, link_ptr, links in; pop, visits, path_ptr out)
  BUF_UNITIG_BULGES_PATH,                     // ... and its paths, sized once n_path is known
  BUF_UNITIG_COMPACT,                         // unitig compaction (unitig_compact.hip): error / size words, links between elements, the rank states, the cycles' minima, the components, the in-rows, the scans' scratch
  BUF_UNITIG_COMPACT_AUX,                     // the sort's payload, lengths and member counts with their scans, the members' list
  BUF_UNITIG_COMPACT_IN, BUF_UNITIG_COMPACT_OUT,  // staging of cfrk_global_unitigs_compact alone (the unitigs, records, link_ptr, links, drop in; the unitigs, records, into out)
  BUF_READ_PATHS,                             // read paths (read_paths.hip): error / size words, the start flags and their scan, the in-rows, the scans' scratch
  BUF_READ_PATHS_IN, BUF_READ_PATHS_OUT,      // staging of cfrk_global_read_paths alone (hit_ptr, hits, records, link_ptr, links, support in; path_ptr, paths out)
  BUF_UNITIG_WEAK,                            // weak rule (unitig_weak.hip): error / count words, the in-rows, the scan's scratch
  BUF_UNITIG_WEAK_IN, BUF_UNITIG_WEAK_OUT,    // staging of cfrk_global_unitig_weak alone (records, link_ptr, links in; weak bytes out)
  BUF_UNITIG_COMP,                            // components (unitig_components.hip): error / count words, parent[], the roots' flags and their scan, the in-degrees, the scan's scratch
  BUF_UNITIG_COMP_IN, BUF_UNITIG_COMP_OUT,    // staging of cfrk_global_unitig_components alone (records, link_ptr, links, drop in; comp, then the table out)
  BUF_READ_COMP,                              // read components (unitig_components.hip): error / count words, the reads' best offers and flag words
  BUF_READ_COMP_IN, BUF_READ_COMP_OUT,        // staging of cfrk_global_read_components alone (hit_ptr, hits, comp in; rows out)
  BUF_NSLOTS
};

enum {  // device stats words (uint64 each)
  ST_OVERFLOW = 0, ST_ONES, ST_CURSOR, ST_DIG0, ST_DIG1, ST_DIG2, ST_DIG3, ST_SPILLED, ST_AUX0,
  ST_AUX1, ST_L2OVF /* leaf streams were too small by a lot: the second level is redone with exact sizes */,
  ST_OVFN /* records parked in the overflow buffer (leaf streams too small by a little) */,
  ST_MULTISEG /* a leaf was counted in several key-subset passes: its list entries are not contiguous */,
  ST_L1OVF /* level-1 regions were too small by a lot: the first level is redone with exact sizes */,
  ST_OVFN1 /* records parked because their level-1 region was full (a few) */,
  ST_SAT /* a count reached CFRK_COUNT_MAX and was held there (finish / digest / export: CFRK_ERR_COUNT_OVERFLOW) */,
  ST_CWRAP /* a 32-bit region / stream cursor of a partitioned path wrapped (>= 2^32 records in one region: a
              single-key flood): the add is counted again through the HBM table */,
  ST_NWORDS = 18
};

struct cfrk_buf { void *p; size_t cap; };

struct cfrk_ctx {
  int device;
  hipStream_t stream;
  bool own_stream;
  char err[512];
  cfrk_buf pool[BUF_NSLOTS];
  void *pinned; size_t pinned_cap;
  int num_cus;
  // global-count state
  bool g_active;
  int g_k, g_flags;
  bool g_two;            // two-word keys (k > 32)
  int g_log2cap;
  uint64_t g_cap;
  uint64_t *g_keys_lo, *g_keys_hi;
  uint32_t *g_counts;
  uint64_t *g_stats;     // device, ST_NWORDS
  bool g_table_cleared;  // the table was cleared by the last begin()
  uint64_t *h_stats;     // pinned host snapshot of g_stats taken at the end of the last add
  bool h_stats_valid;
  hipEvent_t ev0, ev1;
  bool ev_valid;
  hipEvent_t stage_ev[2];   // H2D staging (cfrk_global_add)
  // pipelined runs exchange (cfrk_global_export_runs_async / _wait): one event per group, the groups' used rows in pinned memory
  hipEvent_t runs_ev[CFRK_RUNS_MAX_GROUPS];
  uint64_t *h_runs;         // pinned, CFRK_RUNS_MAX_GROUPS x (64 + 1) words
  int runs_groups, runs_parts;
  uint64_t runs_seg_cap;
  // minimizer-partitioned fast path (msp.hip)
  struct cfrk_msp *msp;
  int last_passes;       // passes the most recent add took on a partitioned path (1 unless memory was short)
  uint32_t dbg_flags;    // cfrk_debug_set_flags
  size_t mem_budget;     // 0 = what the device has free; else a cap on the partitioned paths' buffers (diagnostics)
  double dbg_param[5];   // cfrk_debug_set_param (0 = the library's own choice)
  // query index (query.hip): built on the first query of a job, cleared by every call that changes the result
  bool q_valid;
  int q_log2cap;         // hash index: log2 of its slots (0: the dense array of k <= 12)
  uint64_t q_epoch;      // builds of the index so far: what is kept by slot beside the index names the build it belongs to
  uint64_t upos_epoch;   // the build the position map of BUF_UNITIG_POS belongs to (0: there is no map)
  uint64_t umask_epoch;  // the build the graph mask of BUF_UNITIG_MASK belongs to (0: no key is masked)
};

int cfrk_fail(cfrk_ctx *ctx, int code, const char *fmt, ...);
int cfrk_pool_get(cfrk_ctx *ctx, int slot, size_t bytes, void **out);

#define HIP_TRY(ctx, expr)                                                                   \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return cfrk_fail((ctx), (e_ == hipErrorOutOfMemory) ? CFRK_ERR_NOMEM : CFRK_ERR_HIP,   \
                       "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);  \
  } while (0)

// ---- kernels' host-side launchers (one per .hip file) ------------------------------------
int cfrk_launch_dense(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start,
                      const int32_t *d_length, int64_t nN, int64_t nS, int k, int flags,
                      int32_t *d_freq);
// sparse.hip: count (row_ptr complete on the stream, rows parked in BUF_SPARSE_KEYS / _CNT), then the move to the caller's arrays
int cfrk_sparse_count(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                      int64_t nS, int k, int flags, int64_t *d_row_ptr);
int cfrk_sparse_compact(cfrk_ctx *ctx, const int64_t *d_start, const int64_t *d_row_ptr, int64_t nS, uint64_t *d_keys,
                        uint32_t *d_counts);
int cfrk_launch_synth(cfrk_ctx *ctx, int64_t r0, int64_t R, int L, int64_t Glen, uint64_t seedG,
                      uint64_t seedR, uint64_t seedS, int uniform, int8_t *d_data, int64_t *d_start,
                      int32_t *d_length);
int cfrk_hash_count(cfrk_ctx *ctx, const int8_t *d_data, int64_t nN);
int cfrk_hash_merge(cfrk_ctx *ctx, const uint64_t *lo, const uint64_t *hi, const uint32_t *cnt,
                    int64_t n);
int cfrk_sort_export(cfrk_ctx *ctx, const uint64_t *d_lo, const uint64_t *d_hi, const uint32_t *d_cnt, uint64_t n,
                     const uint64_t **s_lo, const uint64_t **s_hi, const uint32_t **s_cnt);
struct ResultSrc;   // table.h: the table itself (NULL) or a compact (key,count) list
int cfrk_result_scan(cfrk_ctx *ctx, const ResultSrc *src, uint64_t stats_host[ST_NWORDS]);
int cfrk_result_export(cfrk_ctx *ctx, const ResultSrc *src, uint64_t *d_lo, uint64_t *d_hi,
                       uint32_t *d_cnt, uint64_t cap, int parts, uint64_t *part_counts);
// count-range export in two steps: entries with min_count <= count <= max_count per owner part (host part_counts;
// synchronises), then the scatter into the owner segments of d_lo / d_hi / d_cnt (room for sum(part_counts) entries)
int cfrk_result_export_count(cfrk_ctx *ctx, const ResultSrc *src, uint32_t min_count, uint32_t max_count, int parts,
                             uint64_t *part_counts);
int cfrk_result_export_scatter(cfrk_ctx *ctx, const ResultSrc *src, uint32_t min_count, uint32_t max_count, int parts,
                               const uint64_t *part_counts, uint64_t *d_lo, uint64_t *d_hi, uint32_t *d_cnt);
// abundance histogram of the result into host hist[nbins] (2 <= nbins <= 2^24), the stats words into stats_host
int cfrk_result_histogram(cfrk_ctx *ctx, const ResultSrc *src, uint32_t nbins, uint64_t *hist, uint64_t stats_host[ST_NWORDS]);
// query.hip: counts of keys / of every read window from the lookup index, built (synchronising) when it is not valid;
// the lookup kernel is left enqueued.  Arguments are checked by the callers (abi.hip).
int cfrk_query_keys(cfrk_ctx *ctx, const uint64_t *d_lo, const uint64_t *d_hi, int64_t n, uint32_t *d_out);
int cfrk_query_reads(cfrk_ctx *ctx, const int8_t *d_data, int64_t nN, uint32_t *d_out);
// read_stats.hip: one cfrk_read_stats row per read from the same index; the kernels are left enqueued.  nS >= 1.
int cfrk_read_stats_launch(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                           int64_t nN, int64_t nS, uint32_t threshold, cfrk_read_stats *d_out);
// read_filter.hip: one cfrk_read_span per read from the same index; the kernels are left enqueued.  nS >= 1.
int cfrk_read_spans_launch(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                           int64_t nN, int64_t nS, uint32_t min_count, uint32_t max_count, int mode, cfrk_read_span *d_out);
// read_filter.hip: the select in two steps: the sizes (synchronises), then the index pass and the copy, left enqueued
int cfrk_select_measure(cfrk_ctx *ctx, const int64_t *d_start, const int32_t *d_length, int64_t nN, int64_t nS,
                        const cfrk_read_span *d_span, const uint8_t *d_keep, int32_t min_len, int64_t *nN_out, int64_t *nS_out);
int cfrk_select_emit(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                     int64_t nS, const cfrk_read_span *d_span, const uint8_t *d_keep, int32_t min_len, int8_t *d_data_out,
                     int64_t *d_start_out, int32_t *d_length_out, int64_t *d_index_out, int64_t nN_out, int64_t nS_out);
// read_correct.hip: the corrected bases into d_data_out (a copy of d_data by stream order) and one cfrk_read_fix per read
// (d_fix may be NULL) from the same index; the kernels are left enqueued.  nS >= 1.
int cfrk_read_correct_launch(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length,
                             int64_t nN, int64_t nS, uint32_t min_count, int8_t *d_data_out, cfrk_read_fix *d_fix);
// normalize.hip: every round of a normalise call (judge into d_keep, insert the kept reads), left enqueued; the kept reads
// are added to *d_kept.  The result must live in the HBM table.  nS >= 1, batch_reads >= 1.
int cfrk_normalize_launch(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                          int64_t nS, uint32_t cutoff, int64_t batch_reads, uint8_t *d_keep, unsigned long long *d_kept);
// normalize.hip: the same for interleaved pairs (nS and batch_reads even): a join launch between judge and insert applies
// `mode` to the keep bytes in place.  The judge kernels' own count goes to *d_scratch; the kept PAIRS are added to *d_pairs.
int cfrk_normalize_pairs_launch(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                                int64_t nS, uint32_t cutoff, int64_t batch_reads, int mode, uint8_t *d_keep,
                                unsigned long long *d_scratch, unsigned long long *d_pairs);
// pairs.hip: the join of n_pairs >= 1 pairs left enqueued, its four counts ADDED to d_counts[0 .. 4)
int cfrk_pair_join_launch(cfrk_ctx *ctx, int64_t n_pairs, int stride, int mode, int32_t min_len, const uint8_t *d_keep_a,
                          const uint8_t *d_keep_b, const cfrk_read_span *d_span_a, const cfrk_read_span *d_span_b,
                          const int32_t *d_length_a, const int32_t *d_length_b, uint8_t *d_pair_a, uint8_t *d_pair_b,
                          uint8_t *d_orphan_a, uint8_t *d_orphan_b, unsigned long long *d_counts);
// unitigs.hip: the neighbour masks of n >= 0 keys from the same index, left enqueued; the unitigs in two steps: the sizes
// and the segments to emit (synchronises), then order and emit into arrays with room for them, left enqueued (nS >= 1)
int cfrk_neighbors_launch(cfrk_ctx *ctx, const uint64_t *d_lo, const uint64_t *d_hi, int64_t n, uint32_t min_count, uint8_t *d_masks);
int cfrk_unitigs_measure(cfrk_ctx *ctx, uint32_t min_count, int64_t *nN, int64_t *nS, uint64_t *nseg);
int cfrk_unitigs_emit(cfrk_ctx *ctx, int8_t *d_data, int64_t *d_start, int32_t *d_length, cfrk_unitig *d_rec, int64_t nS, uint64_t nseg);
// unitig_links.hip: the links between the unitigs of the job, in two steps: tags, counts and their scan into d_link_ptr
// (nS + 1 entries), the consistency check (synchronises: *n_links, or CFRK_ERR_LAYOUT); then the rows into d_links (room
// for *n_links >= 1 of them), left enqueued.  1 <= nS < 2^32.
int cfrk_unitig_links_measure(cfrk_ctx *ctx, uint32_t min_count, const int8_t *d_data, const int64_t *d_start,
                              const int32_t *d_length, int64_t nN, int64_t nS, int64_t *d_link_ptr, int64_t *n_links);
int cfrk_unitig_links_fill(cfrk_ctx *ctx, uint32_t min_count, const int8_t *d_data, const int64_t *d_start,
                           const int32_t *d_length, int64_t nN, int64_t nS, cfrk_unitig_link *d_links);
// unitig_locate.hip: the position map of the unitig list into BUF_UNITIG_POS with its consistency check (synchronises:
// CFRK_ERR_LAYOUT, or the map valid for the index as built); the positions of n >= 0 keys, left enqueued; the hits of
// nS >= 0 reads in two steps: counts and their scan into d_hit_ptr (nS + 1 entries; synchronises: *n_hits), then the rows
// into d_hits (room for n_hits >= 1 of them), left enqueued.  The last three are CFRK_ERR_STATE without a valid map.
int cfrk_unitig_index_build(cfrk_ctx *ctx, uint32_t min_count, const int8_t *d_data, const int64_t *d_start,
                            const int32_t *d_length, int64_t nN, int64_t nS);
int cfrk_unitig_locate_launch(cfrk_ctx *ctx, const uint64_t *d_lo, const uint64_t *d_hi, int64_t n, cfrk_unitig_pos *d_out);
int cfrk_read_hits_count(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                         int64_t nS, int64_t *d_hit_ptr, int64_t *n_hits);
int cfrk_read_hits_fill(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                        int64_t nS, int64_t *d_hit_ptr, cfrk_read_hit *d_hits, int64_t n_hits);
// unitig_mask.hip: the graph mask of the index as built (the index is built, the mask created and cleared on demand; the
// position map is dropped): n >= 0 keys / the k-mers of the dropped reads of a struct-read list added, left enqueued;
// the mask forgotten; the masked stored keys counted (synchronises).  Arguments are checked by the callers (abi.hip).
int cfrk_mask_keys_launch(cfrk_ctx *ctx, const uint64_t *d_lo, const uint64_t *d_hi, int64_t n);
int cfrk_mask_unitigs_launch(cfrk_ctx *ctx, const int8_t *d_data, const int64_t *d_start, const int32_t *d_length, int64_t nN,
                             int64_t nS, const uint8_t *d_drop);
int cfrk_mask_clear_now(cfrk_ctx *ctx);
int cfrk_mask_count_now(cfrk_ctx *ctx, uint64_t *n_masked);
// unitig_tips.hip: the tip rule over nS >= 1 records and their link rows into d_tip[nS]; synchronises once, for the
// error word (CFRK_ERR_LAYOUT) and *n_tips
int cfrk_unitig_tips_launch(cfrk_ctx *ctx, const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr,
                            const cfrk_unitig_link *d_links, int64_t n_links, uint32_t max_kmers, uint32_t ratio_q8,
                            uint8_t *d_tip, int64_t *n_tips);
// unitig_bubbles.hip: the bubble rule over 1 <= nS < 2^31 records and their link rows into d_pop[nS] and, unless NULL,
// d_partner[nS]; synchronises once, for the error word (CFRK_ERR_LAYOUT) and *n_pop
int cfrk_unitig_bubbles_launch(cfrk_ctx *ctx, const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr,
                               const cfrk_unitig_link *d_links, int64_t n_links, uint32_t max_kmers, uint32_t max_diff,
                               uint32_t ratio_q8, uint8_t *d_pop, uint32_t *d_partner, int64_t *n_pop);
// unitig_weak.hip: the weak rule over 1 <= nS < 2^32 records and their link rows into d_weak[nS]; synchronises once, for
// the error word (CFRK_ERR_LAYOUT) and *stats
int cfrk_unitig_weak_launch(cfrk_ctx *ctx, const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr,
                            const cfrk_unitig_link *d_links, int64_t n_links, uint32_t max_kmers, uint32_t ratio_q8,
                            uint32_t iso_max_kmers, uint32_t iso_mean_q8, uint8_t *d_weak, cfrk_weak_stats *stats);
// unitig_bulges.hip: the bulge rule over 1 <= nS < 2^31 records and their link rows.  The search writes d_pop[nS] and,
// unless NULL, d_visits[nS] and d_path_ptr[nS + 1]; it synchronises once, for the error word (CFRK_ERR_LAYOUT), the
// counts and *n_path.  The fill pass behind it writes the rows of d_path_ptr into d_path and is left enqueued.
struct cfrk_bulge_params { uint32_t max_kmers, max_diff, max_hops, max_visits, ratio_q8; };
int cfrk_unitig_bulges_search(cfrk_ctx *ctx, const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr,
                              const cfrk_unitig_link *d_links, int64_t n_links, const cfrk_bulge_params &p, uint8_t *d_pop,
                              uint32_t *d_visits, int64_t *d_path_ptr, cfrk_bulge_stats *stats, int64_t *n_path);
int cfrk_unitig_bulges_fill(cfrk_ctx *ctx, const cfrk_unitig *d_rec, int64_t nS, const int64_t *d_link_ptr,
                            const cfrk_unitig_link *d_links, int64_t n_links, const cfrk_bulge_params &p, int64_t n_popped,
                            const int64_t *d_path_ptr, uint32_t *d_path);
// unitig_compact.hip: the compaction of 1 <= nS < 2^31 unitigs, their link rows and drop bytes (NULL: none) in two steps:
// the checks, the merges, their ranking and the components (synchronises once: CFRK_ERR_LAYOUT, or the sizes); then the
// order, the members' list, d_into (unless NULL) and the emit into arrays with room for nS_out >= 1 unitigs, left enqueued
struct cfrk_unitigs_in {
  const int8_t *data; const int64_t *start; const int32_t *length; const cfrk_unitig *rec; int64_t nN, nS;
  const int64_t *link_ptr; const cfrk_unitig_link *links; int64_t n_links; const uint8_t *drop;
};
int cfrk_unitigs_compact_measure(cfrk_ctx *ctx, const cfrk_unitigs_in &in, int64_t *nN_out, int64_t *nS_out);
int cfrk_unitigs_compact_emit(cfrk_ctx *ctx, const cfrk_unitigs_in &in, int8_t *d_data, int64_t *d_start, int32_t *d_length,
                              cfrk_unitig *d_rec, cfrk_unitig_pos *d_into, int64_t nN_out, int64_t nS_out);
// read_paths.hip: the paths of nR >= 0 reads through the link rows in two steps: the checks, the join, support (unless
// NULL), the scan and d_path_ptr (synchronises once: CFRK_ERR_LAYOUT, or *n_paths and *stats); then the rows into
// d_paths (room for n_paths >= 1 of them), left enqueued.  The fill step reads what the measure step left in the pool.
struct cfrk_read_paths_in {
  const int64_t *d_hit_ptr; int64_t nR; const cfrk_read_hit *d_hits; int64_t n_hits;
  const cfrk_unitig *d_rec; int64_t nS; const int64_t *d_link_ptr; const cfrk_unitig_link *d_links; int64_t n_links;
};
int cfrk_read_paths_measure(cfrk_ctx *ctx, const cfrk_read_paths_in &in, int64_t *d_path_ptr, uint32_t *d_support,
                            int64_t *n_paths, cfrk_path_stats *stats);
int cfrk_read_paths_fill(cfrk_ctx *ctx, const cfrk_read_paths_in &in, cfrk_read_path *d_paths, int64_t n_paths);
// unitig_components.hip: the components of 1 <= nS < 2^32 unitigs in two steps: the row check, the union-find, the scan and
// d_comp (synchronises once: CFRK_ERR_LAYOUT, or *n_comps and *stats); then the table into d_comps (room for n_comps >= 1
// rows), left enqueued.  The fill step reads what the measure step left in the pool.
struct cfrk_unitig_components_in {
  const cfrk_unitig *d_rec; int64_t nS; const int64_t *d_link_ptr; const cfrk_unitig_link *d_links; int64_t n_links; const uint8_t *d_drop;
};
int cfrk_unitig_components_measure(cfrk_ctx *ctx, const cfrk_unitig_components_in &in, uint32_t *d_comp, int64_t *n_comps,
                                   cfrk_component_stats *stats);
int cfrk_unitig_components_fill(cfrk_ctx *ctx, const cfrk_unitig_components_in &in, const uint32_t *d_comp,
                                cfrk_unitig_component *d_comps, int64_t n_comps);
// ... and the component of every one of nR >= 0 reads from its hits and d_comp; synchronises once, for the error word
// (CFRK_ERR_LAYOUT naming the read) and *stats
int cfrk_read_components_launch(cfrk_ctx *ctx, const int64_t *d_hit_ptr, int64_t nR, const cfrk_read_hit *d_hits, int64_t n_hits,
                                const uint32_t *d_comp, int64_t nS, cfrk_read_component *d_out, cfrk_read_component_stats *stats);
// sketch.hip: fold the valid windows of d_data into the HyperLogLog registers d_regs (max-merged); the kernels are left
// enqueued, the call's window count in *d_windows (a word of BUF_SKETCH).  Arguments are checked by the callers (abi.hip).
int cfrk_sketch_launch(cfrk_ctx *ctx, const int8_t *d_data, int64_t nN, int k, int flags, uint8_t *d_regs,
                       const uint64_t **d_windows);
int cfrk_sketch_stage(cfrk_ctx *ctx, uint8_t **d_stage);   // device room for the host form's registers

// ---- device helpers -----------------------------------------------------------------------
#ifdef __HIPCC__

// Diagnostics counter bumped by many lanes at once: the active lanes elect one that adds their
// number (10^9 atomics on ONE word take seconds: they serialise at the L2).  Counts events.
__device__ __forceinline__ void dev_count_event(uint64_t *word) {
  const unsigned long long m = __ballot(1);
  const unsigned lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  if (lane == (unsigned)__ffsll((long long)m) - 1u)
    atomicAdd((unsigned long long *)word, (unsigned long long)__popcll(m));
}

// Neighbour-lane reads as DPP wave shifts (one VALU instruction; __shfl_down(x, 1) compiles to
// ds_bpermute + address arithmetic).  The lane without a neighbour reads 0.
__device__ __forceinline__ uint32_t dev_lane_next(uint32_t x) {       // value of lane + 1
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x130, 0xF, 0xF, true);   // wave_shl:1
}
__device__ __forceinline__ uint32_t dev_lane_prev(uint32_t x) {       // value of lane - 1
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x138, 0xF, 0xF, true);   // wave_shr:1
}

// Inclusive prefix sum over the 64 lanes of a wave in six DPP adds (row_shr 1/2/4/8 inside the
// rows of 16 lanes, then row_bcast:15 / row_bcast:31 carry the row totals on): no LDS traffic.
// __shfl_up() compiles to ds_bpermute_b32 + address arithmetic + a select -- five instructions and
// an LDS round trip per step, six dependent steps per scan.
__device__ __forceinline__ uint32_t dev_wave_scan_incl(uint32_t x) {
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false);   // row_shr:1
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false);   // row_shr:2
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false);   // row_shr:4
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false);   // row_shr:8
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);   // row_bcast:15 -> rows 1, 3
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);   // row_bcast:31 -> rows 2, 3
  return x;
}

__device__ __forceinline__ uint64_t dev_splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// slot / owner hash of a key (host as well: cfrk_debug_hash_info evaluates this very function for the tests)
__host__ __device__ __forceinline__ uint64_t dev_mix64(uint64_t x) {
  x ^= x >> 32; x *= 0xD6E8FEB86659FD93ull;
  x ^= x >> 32; x *= 0xD6E8FEB86659FD93ull;
  x ^= x >> 32;
  return x;
}

// 4 code bytes (first base in the lowest byte) -> 8 bits, first base most significant
__device__ __forceinline__ uint32_t dev_pack4(uint32_t w) {
  return ((w & 0x03030303u) * 0x40100401u) >> 24;
}
// 4 code bytes -> 4 bits, bit 3 = first base; set where the byte is not in 0..3
__device__ __forceinline__ uint32_t dev_bad4(uint32_t w) {
  // bit 7 of a byte <- (bits 2..6 nonzero) | bit 7: the add cannot carry out of a byte (0x7C + 0x7F)
  const uint32_t f = (((w & 0x7C7C7C7Cu) + 0x7F7F7F7Fu) | w) & 0x80808080u;
  // the flags at bits 7, 15, 23, 31 land on bits 35, 34, 33, 32 of the product (every partial
  // product hits its own bit: no carries); bits 4.. of the high word hold other partial products
  return __umulhi(f, 0x10080402u) & 15u;
}
__device__ __forceinline__ void dev_pack16(uint4 v, uint32_t &bases, uint32_t &bad) {
  bases = (dev_pack4(v.x) << 24) | (dev_pack4(v.y) << 16) | (dev_pack4(v.z) << 8) | dev_pack4(v.w);
  bad = (dev_bad4(v.x) << 12) | (dev_bad4(v.y) << 8) | (dev_bad4(v.z) << 4) | dev_bad4(v.w);
}

// One lane's 32-byte chunk at byte offset off (multiple of 32) of the flat code buffer:
// b0,b1 = bases 0..15 / 16..31 packed 2 bits each, first base most significant;
// bad bit (31-j) set when base j is invalid or lies at/after nN.
__device__ __forceinline__ void dev_load_chunk32(const int8_t *__restrict__ data, int64_t off,
                                                 int64_t nN, uint32_t &b0, uint32_t &b1,
                                                 uint32_t &bad) {
  if (off + 32 <= nN) {
    // The eight words as dev_pack4 / dev_bad4 would do them one by one, without the moves to their places:
    // eight instructions per word and three per 16 bases.
    const uint4 *p = reinterpret_cast<const uint4 *>(data + off);
    const uint4 v0 = p[0], v1 = p[1];
    const uint32_t w[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    // bases: the packed byte of a word is the TOP byte of its product; two v_perm_b32 put four of them side by
    // side (selector bytes 4..7 = bytes of the first operand, 0..3 = of the second, 0x0c = zero)
    uint32_t pr[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) pr[i] = (w[i] & 0x03030303u) * 0x40100401u;
    b0 = __builtin_amdgcn_perm(pr[0], pr[1], 0x07030c0cu) | __builtin_amdgcn_perm(pr[2], pr[3], 0x0c0c0703u);
    b1 = __builtin_amdgcn_perm(pr[4], pr[5], 0x07030c0cu) | __builtin_amdgcn_perm(pr[6], pr[7], 0x0c0c0703u);
    // invalid flags: the gather of dev_bad4 leaves a word's four flags in bits 0..3 with other partial products
    // above them.  From the last word to the first, each v_alignbit takes the low nibble in at the top and
    // moves the earlier ones down by four: the junk falls out, word 0 ends in the top nibble.
    uint32_t acc = 0;
#pragma unroll
    for (int i = 7; i >= 0; --i) {
      const uint32_t f = (((w[i] & 0x7C7C7C7Cu) + 0x7F7F7F7Fu) | w[i]) & 0x80808080u;
      acc = __builtin_amdgcn_alignbit(__umulhi(f, 0x10080402u), acc, 4);
    }
    bad = acc;
  } else {
    b0 = 0; b1 = 0; bad = 0;
    for (int j = 0; j < 32; ++j) {
      int c = (off + j < nN) ? (int)data[off + j] : -1;
      bool inv = (c < 0 || c > 3);
      uint32_t v = inv ? 0u : (uint32_t)c;
      if (j < 16) b0 |= v << (30 - 2 * j); else b1 |= v << (30 - 2 * (j - 16));
      if (inv) bad |= 1u << (31 - j);
    }
  }
}

// reverse complement of a k-mer held in the low 2k bits (first base most significant)
__device__ __forceinline__ uint64_t dev_revcomp64(uint64_t x, int k) {
  uint64_t r = __brevll(x);
  r = ((r >> 1) & 0x5555555555555555ull) | ((r & 0x5555555555555555ull) << 1);
  r = ~r;
  return r >> (64 - 2 * k);
}

#endif  // __HIPCC__
