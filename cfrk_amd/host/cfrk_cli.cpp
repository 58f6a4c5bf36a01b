// cfrk_cli.cpp -- the `cfrk` command: same positional interface as the reference binary
// (/root/reference/src/main.cu:232-309), counting done by libcfrk_hip.so.
//
//   cfrk dataset.fasta out.cfrk k [threads] [chunkSize] [options]
//   cfrk --batch N dataset_prefix out_prefix k [threads] [chunkSize] [options]
//
// Default = byte-exact reference behaviour: compat ingest (src/fastaIO.h quirks), chunks of
// chunkSize reads (default 8192, src/main.cu:235), ComputeFreqNew semantics, and ONLY the last
// partial chunk in the file -- the reference's second PrintFreq re-opens the file with "w"
// (src/main.cu:303-305), so a read count that is a multiple of chunkSize gives an empty file.
// chunkSize is narrowed to unsigned short where the reference narrows it (SelectChunkRemain's
// `ushort chunkSize, ushort it`, src/main.cu:110): the chunk that reaches the file starts at read
// (chunkSize mod 65536) * (nChunk mod 65536) and holds gnS - nChunk * chunkSize reads.
// Options:
//   --all-chunks     write every chunk (what the reference evidently meant to do)
//   --native         guarded per-read counting (src/kmer_kernel.cu:52-70) + clean FASTA parsing
//   --global         one sparse table over all reads, k up to 64: "key:count" lines (k <= 32),
//                    "hi:lo:count" lines (k > 32: key = hi * 2^64 + lo), ascending by key
//   --binary         (global) the CFRKGLB1 binary form instead of text (cfrk_host.h: 32-byte header,
//                    then 12-byte (k <= 32) or 20-byte records, ascending)
//   --canonical      (global, sparse) count min(kmer, reverse complement)
//   --sparse         per-read counting in sparse form, 1 <= k <= 32 (cfrk_per_read_sparse): one line per read, in read
//                    order, its distinct k-mers as "key:count" tokens separated by single spaces, ascending by key (keys
//                    in decimal, as PrintFreq prints indices); a read without a valid window gives an empty line.  Clean
//                    FASTA parsing and guarded semantics as --native, every chunk is written; runs through the per-read
//                    chunk pipeline (--gpus, --batch, --timing).  Not with --global, --binary, --histo, --query* or
//                    --min/--max-count
//   --device N       first GPU ordinal (the reference picks the GPU with most memory, src/main.cu:83-108)
//   --gpus N         chunks (per-read modes) or files (--batch) are dealt round-robin to N devices,
//                    one cfrk_ctx pair per device; replaces the reference's pthread fan-out, whose
//                    threads all use the same device (src/main.cu:208-230,277-295).  With --global
//                    (16 <= k <= 64) the reads are range-partitioned over the N devices, every device
//                    partitions and deduplicates its shard, and the owner of a leaf counts it (the
//                    runs exchange of cfrk_abi.h, staged through host memory here)
//   --timing         one line on stderr, `cfrk-timing {json}`: seconds spent parsing the FASTA, in the counting calls
//                    (H2D copy + kernels), in the export (device sort + D2H) and in formatting + writing the output --
//                    the wall-clock breakdown the reference has as commented-out printf()s (src/main.cu:259-268,303-305)
//   --parse-threads N  host threads of the FASTA parser (default min(hardware threads, 64))
//   --histo FILE     (global) the exact abundance histogram (k-mer spectrum) of the result: "c<TAB>n_c" lines, ascending in
//                    c, for every c with n_c > 0 (`jellyfish histo`'s shape without its upper cut-off)
//   --histo-only     (global, with --histo) write the spectrum only: the counts are not exported and the output path is
//                    left untouched
//   --unitigs-out UFILE [--unitigs-min-count T]  (global, one device) after the count, the compacted de Bruijn graph of
//                    the k-mers counted T times or more (default 1; 0 reads as 1) as FASTA: the unitigs ascending by
//                    first k-mer, ">j LN:i:<bases> KC:i:<summed count> km:f:<KC / k-mers>" and " CL:i:1" on a circular
//                    one, the sequence on one line (cfrk_global_unitigs, cfrk_host_format_unitigs).  Every other output
//                    is what it is without the option
//   --unitigs-links  (with --unitigs-out) BCALM's L tags at the end of every header: " L:<+|->:<v>:<+|->" for every link
//                    out of the unitig, the links out of its + end first (cfrk_global_unitig_links,
//                    cfrk_host_format_unitigs_links)
//   --unitigs-gfa GFILE [--unitigs-min-count T]  (global, one device; with or without --unitigs-out) the same graph as
//                    GFA 1.0: an S line per unitig with the LN / KC / km tags, an L line per link with the overlap
//                    <k-1>M (cfrk_host_format_gfa)
//   --unitigs-map QFILE --unitigs-map-out MFILE [--unitigs-min-count T]  (global, one device; with or without --unitigs-out
//                    and --unitigs-gfa) where the reads of QFILE (FASTA or FASTQ, sniffed as for --query) lie on that
//                    graph, as GAF: one line per hit, a maximal stretch of a read's k-mers that step along one unitig on
//                    one strand, the segment names those of --unitigs-gfa (cfrk_global_unitig_index_device,
//                    cfrk_global_read_hits, cfrk_host_format_gaf)
//   --unitigs-clip-tips [--tip-max-kmers M] [--tip-ratio R] [--tip-rounds N] [--tip-report RFILE]  (with --unitigs-out,
//                    --unitigs-gfa or --unitigs-map) clip tips off the graph before anything is written: up to N rounds
//                    (default 4) of unitigs, links, the tip rule and a mask of the tips' k-mers, ended by the first
//                    round without a tip.  A tip has at most M k-mers (default k), one dead end, and at its other end a
//                    sibling of at least R times its mean coverage (default 2.0, 0 .. 256; 0: topology alone).  UFILE,
//                    the L tags, the GFA and the GAF then describe the clipped graph; the counts' own output is what
//                    it is without the option.  RFILE: one line per round, "round<TAB>unitigs<TAB>tips<TAB>masked
//                    k-mers so far" (cfrk_global_unitig_tips, cfrk_global_mask_unitigs)
//   --unitigs-pop-bubbles [--bubble-max-kmers M] [--bubble-max-diff D] [--bubble-ratio R] [--bubble-report BFILE]
//                    [--simplify-rounds N]  (with --unitigs-out, --unitigs-gfa or --unitigs-map) pop simple bubbles before
//                    anything is written: up to N rounds (default 4) of unitigs, links, the tip rule (iff
//                    --unitigs-clip-tips is given as well) and the bubble rule on that same graph, then one mask of the
//                    k-mers of both, ended by the first round that finds neither.  A popped arm has at most M k-mers
//                    (default k), one link in and one out, and beside it another such unitig between the same two ends,
//                    at most D k-mers longer or shorter (default 0), of at least R times its mean coverage (default 0:
//                    the weaker arm always goes -- a choice, not a measured optimum; 2.0 leaves a balanced heterozygous
//                    site alone).  --tip-rounds is refused here: --simplify-rounds sets the rounds.  --tip-report lines
//                    get a fifth field, "round<TAB>unitigs<TAB>tips<TAB>bubbles<TAB>masked k-mers so far".  BFILE: one
//                    line per popped unitig (cfrk_host_format_bubbles: round, popped and kept S names of that round, kept
//                    strand, lengths, km, snp / mnp / indel, both sequences)  (cfrk_global_unitig_bubbles)
//   --min-count N / --max-count N  (global) write only the entries with N_min <= count <= N_max (text and --binary; the
//                    binary header's n and sum describe the records written)
//   --query QFILE --query-out OFILE  (global) how often does each k-mer of the reads of QFILE (FASTA, clean parse) occur
//                    in the whole result (whatever --min-count / --max-count keep)?  OFILE: one line per query record, in
//                    record order, the counts of its windows separated by single spaces, "-" for a window that holds a
//                    non-ACGT base; a record shorter than k gives an empty line
//   --query-stats SFILE  (with --query; --query-out becomes optional) per-read abundance statistics of the reads of QFILE
//                    against the whole result (cfrk_global_read_stats): one line per query record, in record order, seven
//                    tab-separated decimal fields -- valid windows, present (count >= 1), below (count < T), min, lower
//                    median, max and sum of the windows' counts; a record without a valid window gives zeros.  One device
//                    (not with --gpus above 1), not with --batch or --sparse
//   --stats-below T  (with --query-stats) the threshold of the `below` field, 0 .. 4294967295 (default 0: below is 0)
//   --filter-out FFILE  (with --query; --query-out becomes optional) the reads of QFILE trimmed to their solid spans and
//                    filtered by abundance against the whole result, as FASTA: ">" + the record's number in QFILE, then
//                    its kept bases on one line.  On the device: cfrk_global_read_spans_device, cfrk_reads_select_device,
//                    one copy back, cfrk_host_format_fasta.  One device (not with --gpus above 1), not with --batch or --sparse
//   --filter-names   (with --filter-out) the output records keep the names they have in QFILE: the whole header line behind
//                    its '>' / '@', verbatim.  QFILE's text goes to the device, cfrk_text_index_device finds every record's
//                    header and quality line in it, and cfrk_reads_emit_text_device writes the output text there in place of
//                    the select: one copy back, no formatting on the host
//   --filter-format fasta|fastq  (with --filter-out) the output format.  fasta is the default and alone changes nothing;
//                    fastq writes '@' name, the kept bases, '+' and the matching slice of the record's quality line: it
//                    needs a FASTQ QFILE and implies --filter-names.  A base that --min-qual masked for counting is not
//                    masked here (QFILE is read unmasked); any other invalid base reads N
//   --filter-min-count T / --filter-max-count U  a window is solid when T <= count <= U (defaults 2 and no upper bound)
//   --filter-trim longest|prefix|none  keep the longest solid run (the default; the earliest on a tie), the run that
//                    begins at the read's first window (khmer's filter-abund), or the whole read (no spans)
//   --filter-min-len L  drop a read whose kept part is shorter than L bases (default k)
//   --filter-min-median A / --filter-max-median B  keep only the reads whose median window count (cfrk_global_read_stats;
//                    0 for a read without a valid window) is at least A / at most B
//   --correct-out CFILE --correct-min-count T  (with --query; --query-out becomes optional) spectral error correction
//                    (cfrk_global_correct_reads_device): the reads of QFILE go to the device, and wherever one wrong base
//                    explains an isolated run of weak windows (count < T in the whole result) and exactly one other base makes
//                    all of them solid, that base is written back.  ALL reads of QFILE are written to CFILE, corrected or
//                    not, through the writer of --filter-out (no span, no keep bytes, minimum length 0): FASTA, ">" + the
//                    record's number in QFILE.  A base that is not ACGT (QFILE is read unmasked, as for --filter-out) is an
//                    invalid code: a weak run next to it is not attempted, and it is written as N.  One device (not with
//                    --gpus above 1), not with --batch or --sparse
//   --correct-names / --correct-format fasta|fastq  (with --correct-out) CFILE keeps the names -- and, as fastq, the quality
//                    lines, unchanged -- the records have in QFILE, as --filter-names and --filter-format do for FFILE.
//                    fastq needs a FASTQ QFILE and implies --correct-names
//   --correct-report RFILE  (with --correct-out) one line per query record, in record order: the weak runs of the read that
//                    were corrected and those that were left alone (cfrk_read_fix), tab-separated
//   --normalize-out NFILE --normalize-cutoff C  (global, one device) digital normalisation: the input reads are NORMALISED
//                    instead of added (cfrk_global_normalize_device): taken in rounds of B reads, a read is kept -- and only
//                    then counted -- iff it has a valid window and the median count of its k-mers among the reads kept before
//                    its round is below C.  out.cfrk, --binary and --histo then describe the kept reads; NFILE receives the
//                    kept reads untrimmed, through the writer of --filter-out: FASTA, ">" + the record's number in the input.
//                    The capacity hint and its retry on an overflowing table are those of a plain run.  Not with --gpus
//                    above 1, --batch, --device-parse, --sparse or --query-db
//   --normalize-batch B  reads per round (default CFRK_NORMALIZE_BATCH); 1 is the streaming rule of khmer's
//                    normalize-by-median, a larger B is faster and can over-admit only reads of one round that cover the
//                    same locus
//   --normalize-names / --normalize-format fasta|fastq  (with --normalize-out) NFILE keeps the names -- and, as fastq, the
//                    qualities -- the records have in the input: the input's text goes to the device and
//                    cfrk_text_index_device / cfrk_reads_emit_text_device write NFILE there, exactly as --filter-names and
//                    --filter-format do for FFILE.  Either option selects this writer; fastq needs a FASTQ input
//   --paired         paired-end reads, interleaved: records 2j and 2j + 1 of the file the reads come from are the mates of
//                    pair j.  That file is QFILE for --filter-out and --correct-out and the input for --normalize-out.  An odd
//                    number of records is an error.  Where the file's text is on the device (the --*-names / --*-format
//                    writers) the mates' names are compared there (cfrk_text_pair_check_device: the header up to the first
//                    blank, a trailing /1 with /2 dropped) and the first pair that does not match is an error that shows both
//                    headers.  --filter-out: FFILE receives a read only together with its mate (cfrk_reads_pair_keep_device,
//                    CFRK_PAIR_BOTH, on the spans, --filter-min-len and the median keep bytes), so FFILE stays a valid
//                    interleaved file.  --normalize-out: cfrk_global_normalize_pairs_device replaces the single-read call: a
//                    pair is kept or dropped as a whole.  --correct-out writes every read: pairing is only checked.  One of
//                    the three outputs is needed.  Not with --gpus above 1 or --batch
//   --pair-check on|off  (with --paired / --query2) off skips the comparison of the mates' names
//   --pair-mode either|both  (with --paired --normalize-out) keep a pair if either mate would be kept (the default: khmer's
//                    normalize-by-median --paired) or only if both would be
//   --query2 QFILE2  (with --query and --filter-out / --correct-out) paired-end reads in two files: record j of QFILE and
//                    record j of QFILE2 are the mates of pair j; unequal record counts are an error.  Spans, statistics and
//                    correction run per file; the join runs on the two files' arrays side by side
//   --filter-out2 FFILE2  (with --query2, required with --filter-out) QFILE2's mates of the kept pairs, written from
//                    QFILE2's own text
//   --filter-orphans OFILE  (with --paired / --query2 and --filter-out) the reads that pass the filter while their mate does
//                    not, in input order (QFILE's, then QFILE2's), through the same writer.  Without it they are dropped; a
//                    line on stderr says how many there were either way
//   --correct-out2 CFILE2  (with --query2, required with --correct-out) QFILE2's reads, corrected; --correct-report lists
//                    QFILE's records, then QFILE2's
//   --query-only     (with --query) write OFILE / SFILE / FFILE / CFILE only: the counts are not exported and the output path is left
//                    untouched
//   --query-db DB.bin  (with --query, no positional arguments) query a saved --binary count file without recounting; k and
//                    the canonical bit come from its header
//   --estimate       (global) sketch the batch before it is counted (cfrk_distinct_sketch: one streaming pass, HyperLogLog
//                    with 2^14 registers, standard error 0.81 %) and print one line on stderr,
//                    `cfrk-estimate distinct=<n> windows=<n> hint=<n>`: the estimated distinct k-mers, the exact number of
//                    valid windows, and the capacity hint cfrk_sketch_hint derives (estimate + 3.25 %, at least 2^20)
//   --estimate-only  (global) print that line and stop: nothing is counted, the output path is left untouched
//   --auto-hint      (global) the first cfrk_global_begin announces that hint instead of nN / 16 keys, so that input with
//                    few repeats (low coverage, metagenomes) is counted once instead of up to three times; the retry with
//                    eight times the room stays behind it.  With --gpus N every device sketches its shard and the
//                    registers are merged on the host before the owners begin
//   --device-parse   (global, one device) the file is copied to the device as text and parsed there
//                    (cfrk_fasta_parse_device), then counted with the _device calls on that buffer: no host batch; same
//                    output files, same messages for a file the parser refuses.  Not with --gpus above 1 or --batch.
//                    Query files keep the host parser.  --timing then reports text_map_s (mapping the file), text_h2d_s
//                    and device_parse_ms (parse_s 0)
//   --text-copy plain|staged   (with --device-parse) how the mapped text goes to the device: by one copy from the mapping
//                    (plain, the default: measured the faster one) or through the context's ring of pinned staging
//                    buffers (staged, cfrk_memcpy_h2d_staged)
//   --format fasta|fastq|auto   the format of the input and of the --query file.  auto (the default) goes by each file's
//                    first byte: '@' is FASTQ, anything else FASTA.  FASTQ is strict four-line FASTQ (the grammar of
//                    cfrk_fastq_parse_device, cfrk_abi.h) and is taken by --native, --global (with --device-parse too:
//                    cfrk_fastq_parse_device) and --sparse, and as the --query file; the default per-read mode is the
//                    reference's drop-in, which reads FASTA only, and refuses a FASTQ file
//   --min-qual Q     (FASTQ input, 0 .. 93) a base whose Phred+33 quality is below Q counts as an invalid base: it breaks
//                    its k-mer windows, as an N does.  An error with FASTA input.  The --query file is read unmasked
//   --batch N        the Swift/T workflow's loop (swift/cfrk.swf:15-20) in one process: for i < N
//                    count <dataset_prefix>_<i>.fasta into <out_prefix>_<i>.cfrk
// Chunk pipeline: every device runs two contexts (two HIP streams), each on a host thread of its
// own, so the H2D copy of chunk c+1 overlaps the kernel / D2H / text formatting of chunk c; the
// main thread writes the formatted chunks in order.
// The threads argument is the number of host threads that format the .cfrk text (the reference
// uses it for host memcpy only, src/main.cu:137,186); like the reference, with 5 positional
// arguments the 5th is chunkSize and the 4th is not parsed (src/main.cu:246-249).
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/cfrk_abi.h"
#include "cfrk_host.h"

namespace {

struct Options {
  int k = 0, threads = 12;
  long chunk_size = 8192;
  bool all_chunks = false, native = false, global = false, canonical = false, same_device = false, binary = false, timing = false, sparse = false;
  int device = 0, gpus = 1;
  const char *histo = nullptr;       // --histo FILE
  const char *unitigs_out = nullptr;  // --unitigs-out UFILE
  uint32_t unitigs_min_count = 1;     // --unitigs-min-count T
  bool unitigs_links = false;         // --unitigs-links
  const char *unitigs_gfa = nullptr;  // --unitigs-gfa GFILE
  const char *unitigs_map = nullptr;      // --unitigs-map QFILE
  const char *unitigs_map_out = nullptr;  // --unitigs-map-out MFILE
  bool clip_tips = false;             // --unitigs-clip-tips
  uint32_t tip_max_kmers = 0;         // --tip-max-kmers M (0: k)
  uint32_t tip_ratio_q8 = 512;        // --tip-ratio R, in 256ths
  uint32_t tip_rounds = 4;            // --tip-rounds N
  const char *tip_report = nullptr;   // --tip-report RFILE
  bool pop_bubbles = false;           // --unitigs-pop-bubbles
  uint32_t bubble_max_kmers = 0;      // --bubble-max-kmers M (0: k)
  uint32_t bubble_max_diff = 0;       // --bubble-max-diff D
  uint32_t bubble_ratio_q8 = 0;       // --bubble-ratio R, in 256ths
  uint32_t simplify_rounds = 4;       // --simplify-rounds N
  const char *bubble_report = nullptr;  // --bubble-report BFILE
  bool histo_only = false;
  uint32_t min_count = 1, max_count = CFRK_COUNT_MAX;
  const char *query = nullptr, *query_out = nullptr, *query_db = nullptr;   // --query QFILE --query-out OFILE --query-db DB
  bool query_only = false;
  const char *query_stats = nullptr;   // --query-stats SFILE
  uint32_t stats_below = 0;            // --stats-below T
  const char *filter_out = nullptr;    // --filter-out FFILE
  uint32_t filter_min_count = 2, filter_max_count = CFRK_COUNT_MAX;   // --filter-min-count T, --filter-max-count U
  int filter_trim = CFRK_SPAN_LONGEST; // --filter-trim: CFRK_SPAN_LONGEST / CFRK_SPAN_PREFIX, -1 = none
  long filter_min_len = -1;            // --filter-min-len L (-1: k)
  bool filter_names = false;           // --filter-names (implied by --filter-format fastq)
  int filter_format = CFRK_TEXT_FASTA; // --filter-format: CFRK_TEXT_FASTA / CFRK_TEXT_FASTQ
  bool filter_median = false;          // --filter-min-median A / --filter-max-median B
  uint32_t filter_min_median = 0, filter_max_median = 0xFFFFFFFFu;
  const char *correct_out = nullptr;   // --correct-out CFILE
  uint32_t correct_min_count = 0;      // --correct-min-count T
  bool correct_names = false;          // --correct-names (implied by --correct-format fastq)
  int correct_format = CFRK_TEXT_FASTA;   // --correct-format: CFRK_TEXT_FASTA / CFRK_TEXT_FASTQ
  const char *correct_report = nullptr;   // --correct-report RFILE
  const char *normalize_out = nullptr; // --normalize-out NFILE
  uint32_t normalize_cutoff = 0;       // --normalize-cutoff C
  long long normalize_batch = CFRK_NORMALIZE_BATCH;   // --normalize-batch B
  bool normalize_names = false;        // --normalize-names, --normalize-format
  int normalize_format = CFRK_TEXT_FASTA;             // --normalize-format: CFRK_TEXT_FASTA / CFRK_TEXT_FASTQ
  bool estimate = false, estimate_only = false, auto_hint = false;   // --estimate, --estimate-only, --auto-hint
  bool device_parse = false;                                        // --device-parse
  bool text_copy_plain = true;                                      // --text-copy plain (the default) | staged
  int format = -1;                                                  // --format: CFRK_FORMAT_FASTA / _FASTQ, -1 = by the first byte
  int min_qual = 0;                                                 // --min-qual
  bool min_qual_set = false;
  bool paired = false, pair_check = true;                           // --paired, --pair-check on|off
  int pair_mode = CFRK_PAIR_EITHER;                                 // --pair-mode (the normalise call's; the filter joins by CFRK_PAIR_BOTH)
  const char *query2 = nullptr, *filter_out2 = nullptr, *filter_orphans = nullptr, *correct_out2 = nullptr;
  bool mates() const { return paired || query2; }
};

// --timing: wall-clock seconds by phase (one file; with --batch the last file's)
struct Timing {
  double parse = 0, add_call = 0, finish_wait = 0, export_ = 0, format = 0, write = 0, per_read = 0, total = 0, histo = 0;
  double query = 0, stats = 0;
  double close = 0, free_batch = 0, open = 0;
  double contexts = 0, begin = 0, wait_parse = 0;   // context creation (beside the parse), cfrk_global_begin, the main thread's wait for the parser
  float count_kernels_ms = 0;
  int64_t fasta_bytes = 0, nN = 0, nS = 0;
  uint64_t entries = 0, out_bytes = 0;
  int attempts = 0;                    // begin / add / finish passes of the global job (above 1: the hint was too small)
  double estimate = 0, distinct_estimate = 0;   // the sketch before the count: seconds, estimated distinct k-mers
  double text_map = 0, text_h2d = 0, device_parse_ms = 0;    // --device-parse: the text's copy to the device (s), the parse there (ms)
  bool device_parse = false;
  int in_format = CFRK_FORMAT_FASTA;   // what the input was read as
  uint64_t hint = 0;                   // capacity hint of the LAST attempt
} g_timing;
double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Worker {            // one context (= one HIP stream + buffer pool) on one device
  cfrk_ctx *ctx = nullptr;
  int device = 0;
};

// the format a file is read as: --format, or its first byte (a file that cannot be opened reads as FASTA: the reader says so)
int file_format(const Options &o, const char *path) {
  if (o.format >= 0) return o.format;
  char c = 0;
  size_t n = 0;
  if (FILE *f = fopen(path, "rb")) { n = fread(&c, 1, 1, f); fclose(f); }
  return cfrk_host_sniff_format(&c, n);
}
// may this run read `path` as `fmt`?  Says why not, before anything is parsed or a device is opened.
bool format_allowed(const Options &o, const char *path, int fmt) {
  if (fmt == CFRK_FORMAT_FASTQ && !(o.native || o.global || o.sparse)) {
    fprintf(stderr, "cfrk: %s is FASTQ: the default per-read mode is the reference's, which reads FASTA only; FASTQ is taken by --native, --global and --sparse (and as --query)\n", path);
    return false;
  }
  if (fmt == CFRK_FORMAT_FASTA && o.min_qual_set) {
    fprintf(stderr, "cfrk: --min-qual applies to FASTQ input: %s is read as FASTA\n", path);
    return false;
  }
  return true;
}
// host parse of either format; a refusal is printed here (1), 0 otherwise
int read_reads(const char *path, int fmt, int fasta_flags, int min_qual, cfrk_batch *b) {
  if (fmt == CFRK_FORMAT_FASTQ) {
    uint64_t where = 0;
    const int rc = cfrk_host_read_fastq(path, min_qual, b, &where);
    char msg[160];
    if (rc && cfrk_host_fastq_message(rc, where, msg, sizeof msg)) { fprintf(stderr, "cfrk: cannot read %s (%s)\n", path, msg); return 1; }
    if (rc) { fprintf(stderr, "cfrk: cannot read %s (error %d)\n", path, rc); return 1; }
    return 0;
  }
  const int rc = cfrk_host_read_fasta(path, fasta_flags, b);
  if (rc) { fprintf(stderr, "cfrk: cannot read %s (error %d)\n", path, rc); return 1; }
  return 0;
}

int die(cfrk_ctx *ctx, int rc, const char *what) {
  fprintf(stderr, "cfrk: %s: %s (%s)\n", what, cfrk_strerror(rc), ctx ? cfrk_last_error(ctx) : "");
  return 2;
}

// a count option's value: decimal digits only, below 2^32
bool parse_count(const char *v, uint32_t *out) {
  if (!*v || strlen(v) > 10) return false;
  uint64_t x = 0;
  for (const char *p = v; *p; ++p) {
    if (*p < '0' || *p > '9') return false;
    x = x * 10 + (uint64_t)(*p - '0');
  }
  if (x > 0xFFFFFFFFull) return false;
  *out = (uint32_t)x;
  return true;
}

struct ChunkRange { int64_t first, count; };

// which reads reach the file, in which chunks (src/main.cu:270-305)
std::vector<ChunkRange> plan_chunks(const Options &o, int64_t nS) {
  std::vector<ChunkRange> v;
  const int64_t C = o.chunk_size;
  const int64_t n_full = nS / C;                     // nChunk = floor(gnS/chunkSize), src/main.cu:270
  if (o.all_chunks) {
    for (int64_t c = 0; c <= n_full; ++c) {
      const int64_t first = c * C, count = (c < n_full) ? C : nS - first;
      if (count > 0) v.push_back({first, count});
    }
    return v;
  }
  if (o.native) {                                    // the remainder chunk, where it really is
    if (nS - n_full * C > 0) v.push_back({n_full * C, nS - n_full * C});
    return v;
  }
  // compat: only SelectChunkRemain's chunk is written, located with the narrowed arguments
  const int64_t count = nS - n_full * C;             // chunkRemain, src/main.cu:297
  const int64_t first = (int64_t)(uint16_t)C * (int64_t)(uint16_t)n_full;
  if (count > 0 && first + count <= nS) v.push_back({first, count});
  return v;
}

// per-read modes: the chunks of one batch through `workers` (any number of devices), text in order
int run_per_read(const Options &o, const cfrk_batch &batch, std::vector<Worker> &workers, FILE *out) {
  const std::vector<ChunkRange> chunks = plan_chunks(o, batch.nS);
  const int flags = o.native ? 0 : CFRK_COMPAT;
  const size_t fourk = (size_t)1 << (2 * (o.k > 0 && o.k < 16 ? o.k : 1));
  const size_t n = chunks.size();
  std::vector<std::string> text(n);
  std::vector<char> ready(n, 0);
  const char *call = o.sparse ? "cfrk_per_read_sparse" : "cfrk_per_read_dense";
  std::mutex mu;
  std::condition_variable cv;
  std::atomic<size_t> next{0};
  size_t written = 0;                                // guarded by mu
  int failed = 0;                                    // guarded by mu
  const size_t window = 2 * workers.size() + 2;      // formatted chunks that may wait for the writer
  const int fmt_threads = std::max(1, o.threads / (int)workers.size());

  auto work = [&](Worker &w) {
    std::vector<int64_t> start, row_ptr;
    std::vector<int32_t> freq;
    std::vector<uint64_t> keys;
    std::vector<uint32_t> counts;
    for (;;) {
      const size_t c = next.fetch_add(1);
      if (c >= n) return;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return failed || c < written + window; });
        if (failed) return;
      }
      const int8_t *data; const int32_t *length; int64_t nN;
      start.resize((size_t)chunks[c].count);
      cfrk_host_chunk(&batch, chunks[c].first, chunks[c].count, &data, start.data(), &length, &nN);
      int rc;
      std::string t;
      if (o.sparse) {
        // room for every window of the chunk: always enough (cfrk_abi.h)
        uint64_t room = 0, nnz = 0;
        for (int64_t r = 0; r < chunks[c].count; ++r) room += (uint64_t)std::max<int64_t>((int64_t)length[r] - o.k + 1, 0);
        row_ptr.resize((size_t)chunks[c].count + 1);
        keys.resize(room);
        counts.resize(room);
        rc = cfrk_per_read_sparse(w.ctx, data, start.data(), length, nN, chunks[c].count, o.k, o.canonical ? CFRK_CANONICAL : 0,
                                  row_ptr.data(), keys.data(), counts.data(), room, &nnz);
        if (!rc) {
          t.resize(cfrk_host_format_sparse_rows_mt(row_ptr.data(), keys.data(), counts.data(), chunks[c].count, nullptr, 0, fmt_threads));
          cfrk_host_format_sparse_rows_mt(row_ptr.data(), keys.data(), counts.data(), chunks[c].count, &t[0], t.size(), fmt_threads);
        }
      } else {
        freq.resize((size_t)chunks[c].count * fourk);
        rc = cfrk_per_read_dense(w.ctx, data, start.data(), length, nN, chunks[c].count, o.k, flags, freq.data());
        if (!rc) {
          t.resize(cfrk_host_format_dense_mt(freq.data(), chunks[c].count, o.k, nullptr, 0, fmt_threads));
          cfrk_host_format_dense_mt(freq.data(), chunks[c].count, o.k, &t[0], t.size(), fmt_threads);
        }
      }
      std::lock_guard<std::mutex> lk(mu);
      if (rc && !failed) failed = die(w.ctx, rc, call);
      text[c].swap(t);
      ready[c] = 1;
      cv.notify_all();
    }
  };
  std::vector<std::thread> th;
  for (size_t i = 1; i < workers.size() && i < n; ++i) th.emplace_back(work, std::ref(workers[i]));
  std::thread first_worker;
  if (n) first_worker = std::thread(work, std::ref(workers[0]));
  for (size_t c = 0; c < n; ++c) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return failed || ready[c]; });
    if (failed) break;
    std::string t;
    t.swap(text[c]);
    lk.unlock();
    if (c && !o.sparse) fputc('\n', out);           // (dense rows are separated, sparse rows terminated by '\n')
    fwrite(t.data(), 1, t.size(), out);
    lk.lock();
    written = c + 1;
    cv.notify_all();
  }
  if (first_worker.joinable()) first_worker.join();
  for (auto &t : th) t.join();
  return failed;
}

// --histo: the exact spectrum without a user-set bound.  The device histogram covers counts below HISTO_W; the few keys
// counted HISTO_W times or more are fetched by a count-range export and binned on the host.  Owners of a multi-device
// job hold disjoint key sets: their spectra add.
constexpr uint32_t HISTO_W = 16384;
struct Spectrum {
  std::vector<uint64_t> hist = std::vector<uint64_t>(HISTO_W, 0);   // exact bins 0 .. HISTO_W - 1
  std::vector<uint32_t> tail;                                       // one count per key counted HISTO_W times or more
  void add(const Spectrum &o) {
    for (uint32_t c = 0; c < HISTO_W; ++c) hist[c] += o.hist[c];
    tail.insert(tail.end(), o.tail.begin(), o.tail.end());
  }
};

// 0, or the exit status (the error reported)
int result_spectrum(cfrk_ctx *ctx, Spectrum &sp) {
  std::vector<uint64_t> h(HISTO_W + 1);
  int rc = cfrk_global_histogram(ctx, h.data(), HISTO_W + 1);
  if (rc && rc != CFRK_ERR_COUNT_OVERFLOW) return die(ctx, rc, "cfrk_global_histogram");
  const uint64_t nt = h[HISTO_W];
  for (uint32_t c = 0; c < HISTO_W; ++c) sp.hist[c] += h[c];
  if (!nt) return 0;
  std::vector<uint64_t> lo(nt);
  std::vector<uint32_t> cnt(nt);
  uint64_t got = 0;
  rc = cfrk_global_export_range(ctx, HISTO_W, CFRK_COUNT_MAX, lo.data(), nullptr, cnt.data(), nt, &got);
  if (rc && rc != CFRK_ERR_COUNT_OVERFLOW) return die(ctx, rc, "cfrk_global_export_range");
  sp.tail.insert(sp.tail.end(), cnt.begin(), cnt.begin() + (ptrdiff_t)got);
  return 0;
}

int write_histo(const Options &o, const Spectrum &sp) {
  std::string buf;
  buf.resize(cfrk_host_format_histo(sp.hist.data(), HISTO_W, sp.tail.data(), sp.tail.size(), nullptr, 0));
  cfrk_host_format_histo(sp.hist.data(), HISTO_W, sp.tail.data(), sp.tail.size(), &buf[0], buf.size());
  FILE *f = fopen(o.histo, "wb");
  if (!f) { fprintf(stderr, "cfrk: cannot write %s\n", o.histo); return 1; }
  const bool ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
  if (fclose(f) != 0 || !ok) { fprintf(stderr, "cfrk: cannot write %s\n", o.histo); return 1; }
  return 0;
}

// --unitigs-out: the unitigs of the finished result through the host form (a sizes-only call, then arrays of that size),
// formatted on one thread: the text of a compacted graph is small beside the count's input.  --unitigs-links and
// --unitigs-gfa: the links between them as well, the same way.
int write_text_file(const char *path, const std::string &buf) {
  FILE *f = fopen(path, "wb");
  if (!f) { fprintf(stderr, "cfrk: cannot write %s\n", path); return 1; }
  const bool ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
  if (fclose(f) != 0 || !ok) { fprintf(stderr, "cfrk: cannot write %s\n", path); return 1; }
  return 0;
}

// --unitigs-clip-tips, --unitigs-pop-bubbles: rounds of unitigs, links, each enabled rule on that same graph and one mask of
// the k-mers of the tips and the popped arms through the host forms, before anything is written.  The mask stays set, so
// what write_unitigs and write_unitigs_map compute afterwards is the simplified graph.  Without --unitigs-pop-bubbles
// this is the tip loop as it always was, four-field report included.
int simplify_unitigs(const Options &o, cfrk_ctx *ctx) {
  std::string report, bubbles;
  const uint32_t rounds = o.pop_bubbles ? o.simplify_rounds : o.tip_rounds;
  for (uint32_t round = 1; round <= rounds; ++round) {
    int64_t nN = 0, nS = 0, n_links = 0, n_tips = 0, n_pop = 0;
    int rc = cfrk_global_unitigs(ctx, o.unitigs_min_count, nullptr, 0, nullptr, nullptr, nullptr, 0, &nN, &nS);
    if (rc && rc != CFRK_ERR_SMALL_BUF) return die(ctx, rc, "cfrk_global_unitigs");
    std::vector<int8_t> data((size_t)nN);
    std::vector<int64_t> start((size_t)nS), link_ptr((size_t)nS + 1);
    std::vector<int32_t> length((size_t)nS);
    std::vector<cfrk_unitig> rec((size_t)nS);
    std::vector<uint8_t> tip((size_t)nS);
    if (rc && (rc = cfrk_global_unitigs(ctx, o.unitigs_min_count, data.data(), data.size(), start.data(), length.data(), rec.data(),
                                        rec.size(), &nN, &nS))) return die(ctx, rc, "cfrk_global_unitigs");
    rc = cfrk_global_unitig_links(ctx, o.unitigs_min_count, data.data(), start.data(), length.data(), nN, nS, link_ptr.data(), nullptr, 0, &n_links);
    if (rc && rc != CFRK_ERR_SMALL_BUF) return die(ctx, rc, "cfrk_global_unitig_links");
    std::vector<cfrk_unitig_link> links((size_t)n_links);
    if (rc && (rc = cfrk_global_unitig_links(ctx, o.unitigs_min_count, data.data(), start.data(), length.data(), nN, nS, link_ptr.data(),
                                             links.data(), links.size(), &n_links))) return die(ctx, rc, "cfrk_global_unitig_links");
    if (o.clip_tips &&
        (rc = cfrk_global_unitig_tips(ctx, rec.data(), nS, link_ptr.data(), links.data(), n_links, o.tip_max_kmers ? o.tip_max_kmers : (uint32_t)o.k,
                                      o.tip_ratio_q8, tip.data(), &n_tips))) return die(ctx, rc, "cfrk_global_unitig_tips");
    if (o.pop_bubbles) {
      std::vector<uint8_t> pop((size_t)nS);
      std::vector<uint32_t> partner((size_t)nS);
      if ((rc = cfrk_global_unitig_bubbles(ctx, rec.data(), nS, link_ptr.data(), links.data(), n_links,
                                           o.bubble_max_kmers ? o.bubble_max_kmers : (uint32_t)o.k, o.bubble_max_diff, o.bubble_ratio_q8,
                                           pop.data(), partner.data(), &n_pop))) return die(ctx, rc, "cfrk_global_unitig_bubbles");
      if (o.bubble_report && n_pop) {
        const size_t at = bubbles.size();
        bubbles.resize(at + cfrk_host_format_bubbles(round, data.data(), start.data(), length.data(), rec.data(), nS, pop.data(),
                                                     partner.data(), nullptr, 0));
        cfrk_host_format_bubbles(round, data.data(), start.data(), length.data(), rec.data(), nS, pop.data(), partner.data(), &bubbles[at],
                                 bubbles.size() - at);
      }
      for (size_t j = 0; j < (size_t)nS; ++j) tip[j] |= pop[j];       // (a popped unitig is never a tip: the rules' sets are disjoint)
    }
    if ((n_tips || n_pop) && (rc = cfrk_global_mask_unitigs(ctx, data.data(), start.data(), length.data(), nN, nS, tip.data())))
      return die(ctx, rc, "cfrk_global_mask_unitigs");
    uint64_t masked = 0;
    if ((rc = cfrk_global_mask_count(ctx, &masked))) return die(ctx, rc, "cfrk_global_mask_count");
    char line[128];
    if (o.pop_bubbles)
      snprintf(line, sizeof line, "%u\t%lld\t%lld\t%lld\t%llu\n", round, (long long)nS, (long long)n_tips, (long long)n_pop, (unsigned long long)masked);
    else
      snprintf(line, sizeof line, "%u\t%lld\t%lld\t%llu\n", round, (long long)nS, (long long)n_tips, (unsigned long long)masked);
    report += line;
    if (!n_tips && !n_pop) break;
  }
  if (o.bubble_report) { if (const int rc = write_text_file(o.bubble_report, bubbles)) return rc; }
  return o.tip_report ? write_text_file(o.tip_report, report) : 0;
}

int write_unitigs(const Options &o, cfrk_ctx *ctx) {
  int64_t nN = 0, nS = 0;
  int rc = cfrk_global_unitigs(ctx, o.unitigs_min_count, nullptr, 0, nullptr, nullptr, nullptr, 0, &nN, &nS);
  if (rc && rc != CFRK_ERR_SMALL_BUF) return die(ctx, rc, "cfrk_global_unitigs");
  std::vector<int8_t> data((size_t)nN);
  std::vector<int64_t> start((size_t)nS);
  std::vector<int32_t> length((size_t)nS);
  std::vector<cfrk_unitig> rec((size_t)nS);
  if (rc && (rc = cfrk_global_unitigs(ctx, o.unitigs_min_count, data.data(), data.size(), start.data(), length.data(), rec.data(),
                                      rec.size(), &nN, &nS))) return die(ctx, rc, "cfrk_global_unitigs");
  std::string buf;
  if (!o.unitigs_links && !o.unitigs_gfa) {
    buf.resize(cfrk_host_format_unitigs(data.data(), start.data(), length.data(), rec.data(), nS, nullptr, 0));
    cfrk_host_format_unitigs(data.data(), start.data(), length.data(), rec.data(), nS, &buf[0], buf.size());
    return write_text_file(o.unitigs_out, buf);
  }
  std::vector<int64_t> link_ptr((size_t)nS + 1);
  int64_t n_links = 0;
  rc = cfrk_global_unitig_links(ctx, o.unitigs_min_count, data.data(), start.data(), length.data(), nN, nS, link_ptr.data(), nullptr, 0, &n_links);
  if (rc && rc != CFRK_ERR_SMALL_BUF) return die(ctx, rc, "cfrk_global_unitig_links");
  std::vector<cfrk_unitig_link> links((size_t)n_links);
  if (rc && (rc = cfrk_global_unitig_links(ctx, o.unitigs_min_count, data.data(), start.data(), length.data(), nN, nS, link_ptr.data(),
                                           links.data(), links.size(), &n_links))) return die(ctx, rc, "cfrk_global_unitig_links");
  if (o.unitigs_out) {
    const int64_t *lp = o.unitigs_links ? link_ptr.data() : nullptr;     // (without --unitigs-links: the bytes as they were)
    buf.resize(cfrk_host_format_unitigs_links(data.data(), start.data(), length.data(), rec.data(), nS, lp, links.data(), nullptr, 0));
    cfrk_host_format_unitigs_links(data.data(), start.data(), length.data(), rec.data(), nS, lp, links.data(), &buf[0], buf.size());
    if ((rc = write_text_file(o.unitigs_out, buf))) return rc;
  }
  if (o.unitigs_gfa) {
    buf.resize(cfrk_host_format_gfa(data.data(), start.data(), length.data(), rec.data(), nS, link_ptr.data(), links.data(), o.k, nullptr, 0));
    cfrk_host_format_gfa(data.data(), start.data(), length.data(), rec.data(), nS, link_ptr.data(), links.data(), o.k, &buf[0], buf.size());
    if ((rc = write_text_file(o.unitigs_gfa, buf))) return rc;
  }
  return 0;
}

// --unitigs-map QFILE --unitigs-map-out MFILE: the unitigs into device arrays (a sizes-only call, then arrays of that
// size), where they stay; the position map from them (cfrk_global_unitig_index_device); the hits of QFILE's reads
// (cfrk_global_read_hits) as GAF, the segment names those of --unitigs-gfa (cfrk_host_format_gaf)
cfrk_batch g_mreads{};     // QFILE, parsed before the input is read
int write_unitigs_map(const Options &o, cfrk_ctx *ctx) {
  int64_t nN = 0, nS = 0;
  int rc = cfrk_global_unitigs_device(ctx, o.unitigs_min_count, nullptr, 0, nullptr, nullptr, nullptr, 0, &nN, &nS);
  if (rc && rc != CFRK_ERR_SMALL_BUF) return die(ctx, rc, "cfrk_global_unitigs_device");
  void *d[4] = {nullptr, nullptr, nullptr, nullptr};      // data, start, length, records
  struct Free { cfrk_ctx *c; void **d; ~Free() { for (int j = 0; j < 4; ++j) if (d[j]) cfrk_device_free(c, d[j]); } } free_d{ctx, d};
  std::vector<int32_t> ulen((size_t)nS);
  if (nS > 0) {
    const size_t bytes[4] = {(size_t)nN, (size_t)nS * 8, (size_t)nS * 4, (size_t)nS * sizeof(cfrk_unitig)};
    for (int j = 0; j < 4; ++j)
      if ((rc = cfrk_device_alloc(ctx, bytes[j], &d[j]))) return die(ctx, rc, "cfrk_device_alloc");
    if ((rc = cfrk_global_unitigs_device(ctx, o.unitigs_min_count, (int8_t *)d[0], (uint64_t)nN, (int64_t *)d[1], (int32_t *)d[2],
                                         (cfrk_unitig *)d[3], (uint64_t)nS, &nN, &nS))) return die(ctx, rc, "cfrk_global_unitigs_device");
  }
  if ((rc = cfrk_global_unitig_index_device(ctx, o.unitigs_min_count, (const int8_t *)d[0], (const int64_t *)d[1], (const int32_t *)d[2],
                                            nN, nS))) return die(ctx, rc, "cfrk_global_unitig_index_device");
  if (nS > 0 && (rc = cfrk_memcpy_d2h(ctx, ulen.data(), d[2], (size_t)nS * 4))) return die(ctx, rc, "cfrk_memcpy_d2h");
  const cfrk_batch &q = g_mreads;
  std::vector<int64_t> hit_ptr((size_t)q.nS + 1);
  int64_t n_hits = 0;
  rc = cfrk_global_read_hits(ctx, q.data, q.start, q.length, q.nN, q.nS, hit_ptr.data(), nullptr, 0, &n_hits);
  if (rc && rc != CFRK_ERR_SMALL_BUF) return die(ctx, rc, "cfrk_global_read_hits");
  std::vector<cfrk_read_hit> hits((size_t)n_hits);
  if (rc && (rc = cfrk_global_read_hits(ctx, q.data, q.start, q.length, q.nN, q.nS, hit_ptr.data(), hits.data(), hits.size(), &n_hits)))
    return die(ctx, rc, "cfrk_global_read_hits");
  std::string buf;
  buf.resize(cfrk_host_format_gaf(q.length, q.nS, hit_ptr.data(), hits.data(), ulen.data(), o.k, nullptr, 0));
  cfrk_host_format_gaf(q.length, q.nS, hit_ptr.data(), hits.data(), ulen.data(), o.k, &buf[0], buf.size());
  return write_text_file(o.unitigs_map_out, buf);
}

// --query: the query reads (parsed once, clean FASTA) and the answers of one result for every window of them
cfrk_batch g_qreads{};
int g_qformat = CFRK_FORMAT_FASTA;       // what QFILE was read as
std::vector<char> g_qtext;              // --filter-names: QFILE's bytes
cfrk_batch g_qreads2{};                 // --query2: QFILE2's reads and bytes (the format is QFILE's)
std::vector<char> g_qtext2;

// --paired: an interleaved file holds whole pairs; 1 (the error reported) when it does not
int odd_records(const char *path, int64_t nS) {
  if (!(nS & 1)) return 0;
  fprintf(stderr, "cfrk: --paired: %s holds %lld records, an odd number: the last read has no mate\n", path, (long long)nS);
  return 1;
}

// 0, or 1 (the error reported)
int read_whole_file(const char *path, std::vector<char> &buf) {
  FILE *f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cfrk: cannot read %s\n", path); return 1; }
  char tmp[1 << 16];
  size_t got;
  while ((got = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
  fclose(f);
  return 0;
}

// 0, or the exit status (the error reported)
int query_answers(cfrk_ctx *ctx, std::vector<uint32_t> &ans) {
  ans.assign((size_t)g_qreads.nN, CFRK_QUERY_NONE);
  if (g_qreads.nN == 0) return 0;
  const int rc = cfrk_global_query_reads(ctx, g_qreads.data, g_qreads.start, g_qreads.length, g_qreads.nN, g_qreads.nS,
                                         ans.data());
  return rc ? die(ctx, rc, "cfrk_global_query_reads") : 0;
}

int write_query(const Options &o, int k, const uint32_t *ans) {
  std::string buf;
  const cfrk_batch &q = g_qreads;
  buf.resize(cfrk_host_format_query(ans, q.start, q.length, q.nS, k, nullptr, 0));
  cfrk_host_format_query(ans, q.start, q.length, q.nS, k, &buf[0], buf.size());
  FILE *f = fopen(o.query_out, "wb");
  if (!f) { fprintf(stderr, "cfrk: cannot write %s\n", o.query_out); return 1; }
  const bool ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
  if (fclose(f) != 0 || !ok) { fprintf(stderr, "cfrk: cannot write %s\n", o.query_out); return 1; }
  return 0;
}

// --query-stats: the query reads' abundance statistics against one result, written to SFILE
int write_query_stats(const Options &o, cfrk_ctx *ctx) {
  const cfrk_batch &q = g_qreads;
  std::vector<cfrk_read_stats> st((size_t)q.nS);
  if (q.nS) {
    const int rc = cfrk_global_read_stats(ctx, q.data, q.start, q.length, q.nN, q.nS, o.stats_below, st.data());
    if (rc) return die(ctx, rc, "cfrk_global_read_stats");
  }
  std::string buf;
  buf.resize(cfrk_host_format_read_stats(st.data(), q.nS, nullptr, 0));
  cfrk_host_format_read_stats(st.data(), q.nS, &buf[0], buf.size());
  FILE *f = fopen(o.query_stats, "wb");
  if (!f) { fprintf(stderr, "cfrk: cannot write %s\n", o.query_stats); return 1; }
  const bool ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
  if (fclose(f) != 0 || !ok) { fprintf(stderr, "cfrk: cannot write %s\n", o.query_stats); return 1; }
  return 0;
}

// 0, or 1 (the error reported)
int write_whole_file(const char *path, const std::string &buf) {
  FILE *f = fopen(path, "wb");
  if (!f) { fprintf(stderr, "cfrk: cannot write %s\n", path); return 1; }
  const bool ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
  if (fclose(f) != 0 || !ok) { fprintf(stderr, "cfrk: cannot write %s\n", path); return 1; }
  return 0;
}

// The reads that d_span / d_keep / min_len leave of the batch q on the device (only q's sizes are read), as text in buf:
// FASTA named by record number (select, one copy back, formatted here), or -- names -- FASTA / FASTQ text with the names
// and qualities the records have in `text`, the file q was parsed from, written on the device (index, emit, one copy
// back).  What --filter-out and --normalize-out share.  0, or a CFRK_ERR_* code with *what naming the call.
int emit_selected(cfrk_ctx *ctx, const cfrk_batch &q, const void *d_data, const void *d_start, const void *d_length, const void *d_span,
                  const void *d_keep, long min_len, bool names, const std::vector<char> &text, int text_format, int out_format,
                  const char *text_path, std::string &buf, const char **what) {
  const size_t nN = (size_t)q.nN, nS = (size_t)q.nS;
  std::vector<int8_t> data;
  std::vector<int64_t> start, index;
  std::vector<int32_t> length;
  int64_t onN = 0, onS = 0;
  int rc = 0;
  if (nS) {
    void *o_data = nullptr, *o_start = nullptr, *o_length = nullptr, *o_index = nullptr;
    void *d_text = nullptr, *d_rec = nullptr, *d_out = nullptr;
    *what = "cfrk_device_alloc";
    if (!(!names && ((rc = cfrk_device_alloc(ctx, nN + 16, &o_data)) || (rc = cfrk_device_alloc(ctx, nS * 8, &o_start)) ||
                     (rc = cfrk_device_alloc(ctx, nS * 4, &o_length)) || (rc = cfrk_device_alloc(ctx, nS * 8, &o_index)))) &&
        !(names && ((rc = cfrk_device_alloc(ctx, text.size() + 16, &d_text)) || (rc = cfrk_device_alloc(ctx, nS * sizeof(cfrk_text_record), &d_rec))))) {
      if (names) {
        // the index of the file's text numbers the records as the host parser did; the emitter sizes, then writes
        int64_t inS = 0;
        uint64_t onb = 0;
        *what = "cfrk_memcpy_h2d";
        if (!(rc = cfrk_memcpy_h2d(ctx, d_text, text.data(), text.size()))) {
          *what = "cfrk_text_index_device";
          rc = cfrk_text_index_device(ctx, (const uint8_t *)d_text, text.size(), text_format, (cfrk_text_record *)d_rec, nS, &inS);
        }
        if (!rc && inS != q.nS) {
          fprintf(stderr, "cfrk: %s: %lld records parsed, %lld indexed\n", text_path, (long long)q.nS, (long long)inS);
          rc = CFRK_ERR_LAYOUT;
        }
        for (int pass = 0; pass < 2 && !rc; ++pass) {
          *what = "cfrk_reads_emit_text_device";
          rc = cfrk_reads_emit_text_device(ctx, (const int8_t *)d_data, (const int64_t *)d_start, (const int32_t *)d_length, q.nN, q.nS,
                                           (const cfrk_read_span *)d_span, (const uint8_t *)d_keep, (int32_t)min_len, (const uint8_t *)d_text,
                                           text.size(), (const cfrk_text_record *)d_rec, out_format, (uint8_t *)d_out, pass ? onb : 0, &onb, &onS);
          if (pass == 0 && rc == CFRK_ERR_SMALL_BUF) { *what = "cfrk_device_alloc"; rc = cfrk_device_alloc(ctx, onb + 16, &d_out); }
          else break;
        }
        if (!rc && onb) {
          *what = "cfrk_memcpy_d2h";
          buf.resize((size_t)onb);
          rc = cfrk_memcpy_d2h(ctx, &buf[0], d_out, (size_t)onb);
        }
      } else {
        *what = "cfrk_reads_select_device";
        rc = cfrk_reads_select_device(ctx, (const int8_t *)d_data, (const int64_t *)d_start, (const int32_t *)d_length, q.nN, q.nS,
                                      (const cfrk_read_span *)d_span, (const uint8_t *)d_keep, (int32_t)min_len, (int8_t *)o_data, nN,
                                      (int64_t *)o_start, (int32_t *)o_length, (int64_t *)o_index, nS, &onN, &onS);
        if (!rc) {
          *what = "cfrk_memcpy_d2h";
          data.resize((size_t)onN); start.resize((size_t)onS); length.resize((size_t)onS); index.resize((size_t)onS);
          if (onS && !(rc = cfrk_memcpy_d2h(ctx, data.data(), o_data, (size_t)onN)) && !(rc = cfrk_memcpy_d2h(ctx, start.data(), o_start, (size_t)onS * 8)) &&
              !(rc = cfrk_memcpy_d2h(ctx, length.data(), o_length, (size_t)onS * 4)))
            rc = cfrk_memcpy_d2h(ctx, index.data(), o_index, (size_t)onS * 8);
        }
      }
    }
    const int rc2 = cfrk_ctx_sync(ctx);
    for (void *d : {o_data, o_start, o_length, o_index, d_text, d_rec, d_out}) if (d) cfrk_device_free(ctx, d);
    if (rc) return rc;
    if (rc2) { *what = "cfrk_ctx_sync"; return rc2; }
  }
  if (!names) {
    buf.resize(cfrk_host_format_fasta(data.data(), start.data(), length.data(), index.data(), onS, nullptr, 0));
    cfrk_host_format_fasta(data.data(), start.data(), length.data(), index.data(), onS, &buf[0], buf.size());
  }
  return 0;
}

// --paired / --query2 with a names writer: the mates' names compared on the device.  The text(s) go up and are indexed for
// this alone (the writers index their own copy again behind it); text_b NULL: one interleaved text, pairs are records
// 2j and 2j + 1.  0, or the exit status with the error reported: the first bad pair shows both headers.
int check_mate_names(cfrk_ctx *ctx, int64_t n_pairs, int text_format, const std::vector<char> &text_a, const char *path_a,
                     const std::vector<char> *text_b, const char *path_b) {
  if (n_pairs == 0) return 0;
  const int64_t per = text_b ? n_pairs : 2 * n_pairs;              // records of a text
  const std::vector<char> &tb = text_b ? *text_b : text_a;
  void *d_ta = nullptr, *d_tb = nullptr, *d_ra = nullptr, *d_rb = nullptr;
  const char *what = "cfrk_device_alloc";
  int64_t first = -1, bad = 0, got = 0;
  cfrk_text_record ra{}, rb{};
  int rc;
  auto up = [&](const std::vector<char> &t, const char *path, void **d_t, void **d_r) {
    what = "cfrk_device_alloc";
    if ((rc = cfrk_device_alloc(ctx, t.size() + 16, d_t)) || (rc = cfrk_device_alloc(ctx, (size_t)per * sizeof(cfrk_text_record), d_r))) return;
    what = "cfrk_memcpy_h2d";
    if ((rc = cfrk_memcpy_h2d(ctx, *d_t, t.data(), t.size()))) return;
    what = "cfrk_text_index_device";
    if ((rc = cfrk_text_index_device(ctx, (const uint8_t *)*d_t, t.size(), text_format, (cfrk_text_record *)*d_r, (uint64_t)per, &got))) return;
    if (got != per) { fprintf(stderr, "cfrk: %s: %lld records parsed, %lld indexed\n", path, (long long)per, (long long)got); rc = CFRK_ERR_LAYOUT; }
  };
  up(text_a, path_a, &d_ta, &d_ra);
  if (!rc && text_b) up(tb, path_b, &d_tb, &d_rb);
  if (!rc) {
    const cfrk_text_record *rec_a = (const cfrk_text_record *)d_ra, *rec_b = text_b ? (const cfrk_text_record *)d_rb : rec_a + 1;
    what = "cfrk_text_pair_check_device";
    rc = cfrk_text_pair_check_device(ctx, n_pairs, text_b ? 1 : 2, (const uint8_t *)d_ta, text_a.size(), rec_a,
                                     (const uint8_t *)(text_b ? d_tb : d_ta), tb.size(), rec_b, &first, &bad);
    if (!rc && bad) {
      const int64_t stride = text_b ? 1 : 2;
      what = "cfrk_memcpy_d2h";
      if (!(rc = cfrk_memcpy_d2h(ctx, &ra, rec_a + first * stride, sizeof ra))) rc = cfrk_memcpy_d2h(ctx, &rb, rec_b + first * stride, sizeof rb);
    }
  }
  const int rc2 = cfrk_ctx_sync(ctx);
  for (void *d : {d_ta, d_tb, d_ra, d_rb}) if (d) cfrk_device_free(ctx, d);
  if (rc) return die(ctx, rc, what);
  if (rc2) return die(ctx, rc2, "cfrk_ctx_sync");
  if (!bad) return 0;
  // (the index wrote both records from these very texts: their header ranges lie inside them)
  fprintf(stderr, "cfrk: pair %lld: the mates' names differ: '%.*s' (%s) and '%.*s' (%s); %lld pair(s) in all (--pair-check off skips this check)\n",
          (long long)first, (int)ra.head_len, text_a.data() + ra.head_off, path_a, (int)rb.head_len, tb.data() + rb.head_off, text_b ? path_b : path_a,
          (long long)bad);
  return 1;
}

// --filter-out: one file's reads on the device with what the filter computes of them: the solid spans (--filter-trim) and
// the keep bytes of the median rule (--filter-min-median / --filter-max-median); NULL where the run asks for neither
struct FilterSide {
  cfrk_ctx *ctx;
  void *d_data = nullptr, *d_start = nullptr, *d_length = nullptr, *d_span = nullptr, *d_keep = nullptr, *d_stats = nullptr;
  ~FilterSide() { for (void *d : {d_data, d_start, d_length, d_span, d_keep, d_stats}) if (d) cfrk_device_free(ctx, d); }   // (the caller has synchronised)
  int prepare(const Options &o, const cfrk_batch &q, const char **what) {
    const size_t nN = (size_t)q.nN, nS = (size_t)q.nS;
    const bool trim = o.filter_trim >= 0;
    int rc = 0;
    *what = "cfrk_device_alloc";
    if (nS && !(rc = cfrk_device_alloc(ctx, nN + 16, &d_data)) && !(rc = cfrk_device_alloc(ctx, nS * 8, &d_start)) &&
        !(rc = cfrk_device_alloc(ctx, nS * 4, &d_length)) &&
        !(trim && (rc = cfrk_device_alloc(ctx, nS * sizeof(cfrk_read_span), &d_span))) &&
        !(o.filter_median && ((rc = cfrk_device_alloc(ctx, nS, &d_keep)) || (rc = cfrk_device_alloc(ctx, nS * sizeof(cfrk_read_stats), &d_stats))))) {
      *what = "cfrk_memcpy_h2d";
      if (!(rc = cfrk_memcpy_h2d(ctx, d_data, q.data, nN)) && !(rc = cfrk_memcpy_h2d(ctx, d_start, q.start, nS * 8)))
        rc = cfrk_memcpy_h2d(ctx, d_length, q.length, nS * 4);
      if (!rc && trim) {
        *what = "cfrk_global_read_spans_device";
        rc = cfrk_global_read_spans_device(ctx, (const int8_t *)d_data, (const int64_t *)d_start, (const int32_t *)d_length, q.nN, q.nS,
                                           o.filter_min_count, o.filter_max_count, o.filter_trim, (cfrk_read_span *)d_span);
      }
      if (!rc && o.filter_median) {
        // the rows come down (32 bytes per read), the keep bytes go up (1 byte per read)
        *what = "cfrk_global_read_stats_device";
        std::vector<cfrk_read_stats> st(nS);
        std::vector<uint8_t> keep(nS);
        if (!(rc = cfrk_global_read_stats_device(ctx, (const int8_t *)d_data, (const int64_t *)d_start, (const int32_t *)d_length, q.nN, q.nS, 0,
                                                 (cfrk_read_stats *)d_stats)) &&
            !(rc = cfrk_memcpy_d2h(ctx, st.data(), d_stats, nS * sizeof(cfrk_read_stats)))) {
          for (size_t i = 0; i < nS; ++i) keep[i] = st[i].median >= o.filter_min_median && st[i].median <= o.filter_max_median;
          rc = cfrk_memcpy_h2d(ctx, d_keep, keep.data(), nS);
        }
      }
    }
    return rc;
  }
};

// the query reads trimmed to their solid spans and filtered, on the device, written to FFILE as FASTA named by record
// number, or -- --filter-names -- as FASTA / FASTQ text with QFILE's names and qualities (emit_selected).
// --paired / --query2: the spans, --filter-min-len and the median keep bytes are joined per pair on the device
// (CFRK_PAIR_BOTH); FFILE (and FFILE2) receive whole pairs, --filter-orphans' OFILE the survivors whose mate did not
// survive, every file through the same writer with the joined bytes as its keep bytes.
int write_filter(const Options &o, cfrk_ctx *ctx, int k) {
  const cfrk_batch &q = g_qreads, &q2 = g_qreads2;
  const size_t nS = (size_t)q.nS;
  const int tf = g_qformat == CFRK_FORMAT_FASTQ ? CFRK_TEXT_FASTQ : CFRK_TEXT_FASTA;
  const long min_len = o.filter_min_len >= 0 ? o.filter_min_len : (long)k;
  std::string buf, buf2, orphans;
  FilterSide a{ctx}, b{ctx};
  void *d_pair = nullptr, *d_orphan = nullptr;
  const char *what = "";
  cfrk_pair_counts pc{};
  auto emit = [&](const cfrk_batch &r, const FilterSide &f, const void *d_keep, const std::vector<char> &text, const char *path, std::string &out) {
    return emit_selected(ctx, r, f.d_data, f.d_start, f.d_length, f.d_span, d_keep, min_len, o.filter_names, text, tf, o.filter_format, path, out, &what);
  };
  int rc = a.prepare(o, q, &what);
  if (!rc && o.query2) rc = b.prepare(o, q2, &what);
  if (!rc && !o.mates()) rc = emit(q, a, a.d_keep, g_qtext, o.query, buf);
  else if (!rc && nS) {
    // mate B of pair j: the next element of the one file's arrays, or element j of QFILE2's; the joined bytes of both
    // layouts lie in one array of a byte per read (QFILE2's behind QFILE's)
    const size_t step = o.query2 ? 0 : 1, total = o.query2 ? 2 * nS : nS, off_b = o.query2 ? nS : 1;
    const FilterSide &fb = o.query2 ? b : a;
    what = "cfrk_device_alloc";
    if (!(rc = cfrk_device_alloc(ctx, total, &d_pair)) && !(rc = cfrk_device_alloc(ctx, total, &d_orphan))) {
      what = "cfrk_reads_pair_keep_device";
      rc = cfrk_reads_pair_keep_device(ctx, (int64_t)(o.query2 ? nS : nS / 2), o.query2 ? 1 : 2, CFRK_PAIR_BOTH, (int32_t)min_len,
                                       (const uint8_t *)a.d_keep, fb.d_keep ? (const uint8_t *)fb.d_keep + step : nullptr,
                                       (const cfrk_read_span *)a.d_span, fb.d_span ? (const cfrk_read_span *)fb.d_span + step : nullptr,
                                       (const int32_t *)a.d_length, (const int32_t *)fb.d_length + step, (uint8_t *)d_pair,
                                       (uint8_t *)d_pair + off_b, (uint8_t *)d_orphan, (uint8_t *)d_orphan + off_b, &pc);
    }
    if (!rc) rc = emit(q, a, d_pair, g_qtext, o.query, buf);
    if (!rc && o.query2) rc = emit(q2, b, (const uint8_t *)d_pair + nS, g_qtext2, o.query2, buf2);
    if (!rc && o.filter_orphans) rc = emit(q, a, d_orphan, g_qtext, o.query, orphans);
    if (!rc && o.filter_orphans && o.query2) {
      std::string more;
      if (!(rc = emit(q2, b, (const uint8_t *)d_orphan + nS, g_qtext2, o.query2, more))) orphans += more;
    }
  }
  const int rc2 = nS ? cfrk_ctx_sync(ctx) : 0;
  for (void *d : {d_pair, d_orphan}) if (d) cfrk_device_free(ctx, d);
  if (rc) return die(ctx, rc, what);
  if (rc2) return die(ctx, rc2, "cfrk_ctx_sync");
  if (o.mates())
    fprintf(stderr, "cfrk: filter: %lld pairs kept, %lld orphans (%lld + %lld) %s, %lld pairs dropped\n", (long long)pc.pairs,
            (long long)(pc.orphans_a + pc.orphans_b), (long long)pc.orphans_a, (long long)pc.orphans_b,
            o.filter_orphans ? "written" : "dropped", (long long)pc.dropped);
  if (write_whole_file(o.filter_out, buf)) return 1;
  if (o.query2 && write_whole_file(o.filter_out2, buf2)) return 1;
  return o.filter_orphans ? write_whole_file(o.filter_orphans, orphans) : 0;
}

// --correct-out: the query reads corrected against the whole result on the device; every read is written to CFILE through
// emit_selected (the corrected buffer, no span, no keep bytes), the cfrk_read_fix rows to --correct-report's RFILE
int write_correct(const Options &o, cfrk_ctx *ctx, const cfrk_batch &q, const std::vector<char> &qtext, const char *qpath, const char *out_path,
                  std::string *report) {
  const size_t nN = (size_t)q.nN, nS = (size_t)q.nS;
  std::string buf;
  std::vector<cfrk_read_fix> fix(nS);
  void *d_data = nullptr, *d_start = nullptr, *d_length = nullptr, *d_out = nullptr, *d_fix = nullptr;
  const char *what = "cfrk_device_alloc";
  int rc = 0;
  if (nS && !(rc = cfrk_device_alloc(ctx, nN + 16, &d_data)) && !(rc = cfrk_device_alloc(ctx, nS * 8, &d_start)) &&
      !(rc = cfrk_device_alloc(ctx, nS * 4, &d_length)) && !(rc = cfrk_device_alloc(ctx, nN + 16, &d_out)) &&
      !(rc = cfrk_device_alloc(ctx, nS * sizeof(cfrk_read_fix), &d_fix))) {
    what = "cfrk_memcpy_h2d";
    if (!(rc = cfrk_memcpy_h2d(ctx, d_data, q.data, nN)) && !(rc = cfrk_memcpy_h2d(ctx, d_start, q.start, nS * 8)))
      rc = cfrk_memcpy_h2d(ctx, d_length, q.length, nS * 4);
    if (!rc) {
      what = "cfrk_global_correct_reads_device";
      rc = cfrk_global_correct_reads_device(ctx, (const int8_t *)d_data, (const int64_t *)d_start, (const int32_t *)d_length, q.nN, q.nS,
                                            o.correct_min_count, (int8_t *)d_out, (cfrk_read_fix *)d_fix);
    }
    if (!rc && o.correct_report) {
      what = "cfrk_memcpy_d2h";
      rc = cfrk_memcpy_d2h(ctx, fix.data(), d_fix, nS * sizeof(cfrk_read_fix));
    }
  }
  if (!rc)
    rc = emit_selected(ctx, q, d_out, d_start, d_length, nullptr, nullptr, 0, o.correct_names, qtext,
                       g_qformat == CFRK_FORMAT_FASTQ ? CFRK_TEXT_FASTQ : CFRK_TEXT_FASTA, o.correct_format, qpath, buf, &what);
  const int rc2 = nS ? cfrk_ctx_sync(ctx) : 0;
  for (void *d : {d_data, d_start, d_length, d_out, d_fix}) if (d) cfrk_device_free(ctx, d);
  if (rc) return die(ctx, rc, what);
  if (rc2) return die(ctx, rc2, "cfrk_ctx_sync");
  if (write_whole_file(out_path, buf)) return 1;
  if (!o.correct_report) return 0;
  char line[32];
  for (size_t i = 0; i < nS; ++i) {
    snprintf(line, sizeof line, "%u\t%u\n", (unsigned)fix[i].fixed, (unsigned)fix[i].left);
    *report += line;
  }
  return 0;
}

// QFILE to CFILE and, with --query2, QFILE2 to CFILE2; the report lists QFILE's records, then QFILE2's
int write_correct(const Options &o, cfrk_ctx *ctx) {
  std::string report;
  if (const int rc = write_correct(o, ctx, g_qreads, g_qtext, o.query, o.correct_out, &report)) return rc;
  if (o.query2)
    if (const int rc = write_correct(o, ctx, g_qreads2, g_qtext2, o.query2, o.correct_out2, &report)) return rc;
  return o.correct_report ? write_whole_file(o.correct_report, report) : 0;
}

// --paired / --query2: the names of the query file's mates, where its text is held for a names writer
int check_query_pairs(const Options &o, cfrk_ctx *ctx) {
  if (!o.mates() || !o.pair_check || !((o.filter_out && o.filter_names) || (o.correct_out && o.correct_names))) return 0;
  const int tf = g_qformat == CFRK_FORMAT_FASTQ ? CFRK_TEXT_FASTQ : CFRK_TEXT_FASTA;
  return check_mate_names(ctx, o.query2 ? g_qreads.nS : g_qreads.nS / 2, tf, g_qtext, o.query, o.query2 ? &g_qtext2 : nullptr, o.query2);
}

// --normalize-out: the input's text and format, as the writer of the kept reads needs them
std::vector<char> g_ntext;              // --normalize-names: the input file's bytes
int g_nformat = CFRK_FORMAT_FASTA;
const char *g_npath = "";

// the kept reads (d_keep, as the normalise call left it) untrimmed, to NFILE
int write_normalized(const Options &o, cfrk_ctx *ctx, const cfrk_batch &b, const void *d_data, const void *d_start, const void *d_length,
                     const void *d_keep) {
  std::string buf;
  const char *what = "";
  const int rc = emit_selected(ctx, b, d_data, d_start, d_length, nullptr, d_keep, 0, o.normalize_names, g_ntext,
                               g_nformat == CFRK_FORMAT_FASTQ ? CFRK_TEXT_FASTQ : CFRK_TEXT_FASTA, o.normalize_format, g_npath, buf, &what);
  if (rc) return die(ctx, rc, what);
  return write_whole_file(o.normalize_out, buf);
}

// the global result (ascending keys) as sparse text or in the binary form
void write_global(const Options &o, const uint64_t *lo, const uint64_t *hi, const uint32_t *cnt, uint64_t n, FILE *out) {
  const uint64_t *hi2 = (o.k > 32) ? hi : nullptr;
  std::string buf;
  const double t0 = now_s();
  if (o.binary) {
    buf.resize(cfrk_host_write_binary(o.k, o.canonical ? CFRK_BIN_CANONICAL : 0, lo, hi2, cnt, n, nullptr, 0));
    cfrk_host_write_binary(o.k, o.canonical ? CFRK_BIN_CANONICAL : 0, lo, hi2, cnt, n, &buf[0], buf.size());
  } else {
    buf.resize(cfrk_host_format_sparse_mt(lo, hi2, cnt, n, nullptr, 0, o.threads));
    cfrk_host_format_sparse_mt(lo, hi2, cnt, n, &buf[0], buf.size(), o.threads);
  }
  const double t1 = now_s();
  fwrite(buf.data(), 1, buf.size(), out);
  fflush(out);
  g_timing.format = t1 - t0; g_timing.write = now_s() - t1; g_timing.entries = n; g_timing.out_bytes = buf.size();
}

// --estimate / --estimate-only / --auto-hint: the batch's distinct sketch.  Context i sketches shard i of the reads (the
// shards of run_global_multi); the registers are merged on the host.
struct Estimate {
  bool have = false;
  double distinct = 0;
  uint64_t windows = 0, hint = 0;
};

// 0, or the exit status (the error reported)
int sketch_batch(const Options &o, const cfrk_batch &batch, const std::vector<cfrk_ctx *> &ctxs, Estimate &e) {
  const double t0 = now_s();
  const int N = (int)ctxs.size();
  std::vector<std::vector<uint8_t>> regs((size_t)N, std::vector<uint8_t>(CFRK_SKETCH_REGS, 0));
  std::vector<uint64_t> windows((size_t)N, 0);
  std::vector<int> status((size_t)N, 0);
  auto shard = [&](int sh) {
    const int64_t r0 = batch.nS * sh / N, r1 = batch.nS * (sh + 1) / N;
    const int64_t b0 = (r0 < batch.nS) ? batch.start[r0] : batch.nN, b1 = (r1 < batch.nS) ? batch.start[r1] : batch.nN;
    if (b1 <= b0) return;
    const int rc = cfrk_distinct_sketch(ctxs[(size_t)sh], batch.data + b0, nullptr, nullptr, b1 - b0, 0, o.k,
                                        o.canonical ? CFRK_CANONICAL : 0, regs[(size_t)sh].data(), &windows[(size_t)sh]);
    if (rc) status[(size_t)sh] = die(ctxs[(size_t)sh], rc, "cfrk_distinct_sketch");
  };
  if (N == 1) shard(0);
  else {
    std::vector<std::thread> th;
    for (int sh = 0; sh < N; ++sh) th.emplace_back(shard, sh);
    for (auto &t : th) t.join();
  }
  for (int r : status) if (r) return r;
  for (int sh = 1; sh < N; ++sh) { cfrk_sketch_merge(regs[0].data(), regs[(size_t)sh].data()); windows[0] += windows[(size_t)sh]; }
  cfrk_sketch_estimate(regs[0].data(), &e.distinct);
  cfrk_sketch_hint(regs[0].data(), &e.hint);
  e.windows = windows[0];
  e.have = true;
  g_timing.estimate = now_s() - t0; g_timing.distinct_estimate = e.distinct;
  fprintf(stderr, "cfrk-estimate distinct=%.0f windows=%llu hint=%llu\n", e.distinct, (unsigned long long)e.windows, (unsigned long long)e.hint);
  return 0;
}

// early_free: the batch is no longer needed once it has been counted -- returning 1.6 GB of pages to the kernel takes
// ~0.17 s, which then runs beside the export, the formatting and the write instead of behind them
// d_data: the batch's codes already on the device (--device-parse: batch then carries nN and nS only)
int run_global(const Options &o, const cfrk_batch &batch, Worker &w, FILE *out, const Estimate &est, std::thread *early_free = nullptr, cfrk_batch *owned = nullptr,
               bool on_device = false, const int8_t *d_data = nullptr) {
  int rc;
  cfrk_ctx *ctx = w.ctx;
  // The capacity hint sizes the result list and the spill table (12 B per slot at load <= 0.5).  Distinct k-mers cannot
  // exceed the window starts (nN), but a table for nN keys is 25 - 50 GB for a 1.5 GB batch and allocating it took
  // 5 of the 6 seconds of a k = 31 run (round 5, profiles/r05/end_to_end.txt): the first attempt announces nN / 16 keys
  // (sequencing depth is rarely below that) and an overflowing result (CFRK_ERR_TABLE_FULL) is counted again with
  // eight times the room, up to nN (capped at 2^31 keys).  --auto-hint: the first attempt announces the sketch's hint instead.
  const uint64_t hint_max = std::min<uint64_t>(std::max<uint64_t>((uint64_t)(batch.nN > 0 ? batch.nN : 1), 1ull << 20), 1ull << 31);
  uint64_t hint = std::min<uint64_t>(std::max<uint64_t>(hint_max / 16, 1ull << 20), hint_max);
  if (o.auto_hint && est.have) hint = std::min<uint64_t>(est.hint, hint_max);
  uint64_t n = 0;
  // --normalize-out: the reads go to the device once; every attempt normalises them from there into its fresh job
  struct DeviceReads {
    cfrk_ctx *ctx;
    void *data = nullptr, *start = nullptr, *length = nullptr, *keep = nullptr;
    ~DeviceReads() { for (void *d : {data, start, length, keep}) if (d) cfrk_device_free(ctx, d); }
  } nr{ctx};
  if (o.normalize_out && o.paired) {
    if (odd_records(g_npath, batch.nS)) return 1;
    if (o.pair_check && o.normalize_names &&
        (rc = check_mate_names(ctx, batch.nS / 2, g_nformat == CFRK_FORMAT_FASTQ ? CFRK_TEXT_FASTQ : CFRK_TEXT_FASTA, g_ntext, g_npath, nullptr, nullptr))) return rc;
  }
  if (o.normalize_out && batch.nS > 0) {
    const size_t nN = (size_t)batch.nN, nS = (size_t)batch.nS;
    if ((rc = cfrk_device_alloc(ctx, nN + 16, &nr.data)) || (rc = cfrk_device_alloc(ctx, nS * 8, &nr.start)) ||
        (rc = cfrk_device_alloc(ctx, nS * 4, &nr.length)) || (rc = cfrk_device_alloc(ctx, nS, &nr.keep))) return die(ctx, rc, "cfrk_device_alloc");
    if ((rc = cfrk_memcpy_h2d(ctx, nr.data, batch.data, nN)) || (rc = cfrk_memcpy_h2d(ctx, nr.start, batch.start, nS * 8)) ||
        (rc = cfrk_memcpy_h2d(ctx, nr.length, batch.length, nS * 4))) return die(ctx, rc, "cfrk_memcpy_h2d");
  }
  // (the phase times add up over the attempts: a batch counted three times shows three times the seconds)
  double add_s = 0, finish_s = 0;
  g_timing.begin = 0;
  for (;;) {
    const double tb = now_s();
    ++g_timing.attempts;
    g_timing.hint = hint;
    if ((rc = cfrk_global_begin(ctx, o.k, o.canonical ? CFRK_CANONICAL : 0, hint))) return die(ctx, rc, "cfrk_global_begin");
    const double t0 = now_s();
    g_timing.begin += t0 - tb;
    if (o.normalize_out) {
      int64_t kept = 0;
      if (batch.nS == 0) rc = 0;
      else if (o.paired)
        rc = cfrk_global_normalize_pairs_device(ctx, (const int8_t *)nr.data, (const int64_t *)nr.start, (const int32_t *)nr.length, batch.nN,
                                                batch.nS, o.normalize_cutoff, o.normalize_batch, o.pair_mode, (uint8_t *)nr.keep, &kept);
      else
        rc = cfrk_global_normalize_device(ctx, (const int8_t *)nr.data, (const int64_t *)nr.start, (const int32_t *)nr.length, batch.nN,
                                          batch.nS, o.normalize_cutoff, o.normalize_batch, (uint8_t *)nr.keep, &kept);
      if (rc == CFRK_ERR_TABLE_FULL && hint < hint_max) { hint = std::min<uint64_t>(hint * 8, hint_max); continue; }
      if (rc) return die(ctx, rc, o.paired ? "cfrk_global_normalize_pairs_device" : "cfrk_global_normalize_device");
    }
    else if (on_device) { if (batch.nN > 0 && (rc = cfrk_global_add_device(ctx, d_data, batch.nN))) return die(ctx, rc, "cfrk_global_add_device"); }
    else if ((rc = cfrk_global_add(ctx, batch.data, batch.start, batch.length, batch.nN, batch.nS))) return die(ctx, rc, "cfrk_global_add");
    const double t1 = now_s();
    rc = cfrk_global_finish(ctx, &n);
    add_s += t1 - t0; finish_s += now_s() - t1;
    if (rc == CFRK_ERR_TABLE_FULL && hint < hint_max) { hint = std::min<uint64_t>(hint * 8, hint_max); continue; }
    break;
  }
  // (counts are 32-bit and saturate: the result is complete, the user is told)
  if (rc == CFRK_ERR_COUNT_OVERFLOW) fprintf(stderr, "cfrk: warning: %s\n", cfrk_last_error(ctx));
  else if (rc) return die(ctx, rc, "cfrk_global_finish");
  if (o.normalize_out && (rc = write_normalized(o, ctx, batch, nr.data, nr.start, nr.length, nr.keep))) return rc;
  const double t2 = now_s();
  // the spectrum is taken before the batch is freed: its copies do not wait behind the page returns
  if (o.histo) {
    Spectrum sp;
    if ((rc = result_spectrum(ctx, sp)) || (rc = write_histo(o, sp))) return rc;
  }
  g_timing.histo = now_s() - t2;
  if ((o.clip_tips || o.pop_bubbles) && (rc = simplify_unitigs(o, ctx))) return rc;
  if ((o.unitigs_out || o.unitigs_gfa) && (rc = write_unitigs(o, ctx))) return rc;
  if (o.unitigs_map && (rc = write_unitigs_map(o, ctx))) return rc;
  if (o.query) {
    const double q0 = now_s();
    if (o.query_out) {
      std::vector<uint32_t> ans;
      if ((rc = query_answers(ctx, ans)) || (rc = write_query(o, o.k, ans.data()))) return rc;
    }
    g_timing.query = now_s() - q0;
    if (o.query_stats) {
      const double s0 = now_s();
      if ((rc = write_query_stats(o, ctx))) return rc;
      g_timing.stats = now_s() - s0;
    }
    if ((rc = check_query_pairs(o, ctx))) return rc;
    if (o.filter_out && (rc = write_filter(o, ctx, o.k))) return rc;
    if (o.correct_out && (rc = write_correct(o, ctx))) return rc;
  }
  if (early_free && owned) *early_free = std::thread([owned] { cfrk_host_free_batch(owned); });
  cfrk_global_last_add_ms(ctx, &g_timing.count_kernels_ms);
  g_timing.add_call = add_s; g_timing.finish_wait = finish_s;
  if (o.histo_only || o.query_only) return 0;
  const double t3 = now_s();
  std::vector<uint64_t> keys(n), hi(n);
  std::vector<uint32_t> cnt(n);
  rc = cfrk_global_export_range(ctx, o.min_count, o.max_count, keys.data(), hi.data(), cnt.data(), n, &n);
  if (rc && rc != CFRK_ERR_COUNT_OVERFLOW) return die(ctx, rc, "cfrk_global_export_range");
  g_timing.export_ = now_s() - t3;
  write_global(o, keys.data(), hi.data(), cnt.data(), n, out);
  return 0;
}

// --global over several devices: shard s of the reads goes to device s (first context of the pair);
// device s then owns the leaves s, s + N, ...: it receives its segment of every shard's packed runs
// and counts them on its second context.  The owners' key sets are disjoint; their sorted lists are
// merged into one ascending output.
int run_global_multi(const Options &o, const cfrk_batch &batch, std::vector<std::vector<Worker>> &per_dev, FILE *out, const Estimate &est) {
  const int N = (int)per_dev.size();
  const int flags = o.canonical ? CFRK_CANONICAL : 0;
  // (as in run_global: nN / 16 keys announced first; an owner whose result overflows makes the job count on one device,
  //  where the hint grows)
  uint64_t hint = std::min<uint64_t>(std::max<uint64_t>((uint64_t)(batch.nN > 0 ? batch.nN : 1) / 16, 1ull << 20), 1ull << 31);
  // --auto-hint: the merged sketch's hint; the owners' shares of the leaves are close to even, not even: an eighth on top
  if (o.auto_hint && est.have) hint = std::min<uint64_t>(est.hint + est.hint / 8, 1ull << 31);
  g_timing.attempts = 1; g_timing.hint = hint;
  // shard s: packed rows stay ON ITS DEVICE (16 bytes per row), rows[s][o] = rows of owner o's segment
  std::vector<void *> d_packed((size_t)N, nullptr);
  std::vector<std::vector<uint64_t>> rows((size_t)N, std::vector<uint64_t>((size_t)N, 0));
  std::vector<int> status((size_t)N, 0);
  std::vector<char> refused((size_t)N, 0);           // the shard cannot export runs: count on one device instead
  auto free_packed = [&] {
    for (int sh = 0; sh < N; ++sh)
      if (d_packed[(size_t)sh]) { cfrk_device_free(per_dev[(size_t)sh][0].ctx, d_packed[(size_t)sh]); d_packed[(size_t)sh] = nullptr; }
  };
  {
    std::vector<std::thread> th;
    for (int sh = 0; sh < N; ++sh)
      th.emplace_back([&, sh] {
        cfrk_ctx *ctx = per_dev[(size_t)sh][0].ctx;
        const int64_t r0 = batch.nS * sh / N, r1 = batch.nS * (sh + 1) / N;
        const int64_t b0 = (r0 < batch.nS) ? batch.start[r0] : batch.nN, b1 = (r1 < batch.nS) ? batch.start[r1] : batch.nN;
        int rc;
        if ((rc = cfrk_global_begin(ctx, o.k, flags | CFRK_RUNS_ONLY, hint))) { status[(size_t)sh] = die(ctx, rc, "cfrk_global_begin"); return; }
        if (b1 <= b0) return;
        if ((rc = cfrk_global_add(ctx, batch.data + b0, nullptr, nullptr, b1 - b0, 0))) {
          if (rc == CFRK_ERR_RUNS_REFUSED) { refused[(size_t)sh] = 1; return; }     // (the shard needs several passes)
          status[(size_t)sh] = die(ctx, rc, "cfrk_global_add");
          return;
        }
        // distinct runs never exceed the shard's super-k-mers (about one per 8 bases), plus the headers;
        // a buffer that is too small is retried at four times the size
        // (k > 32: a record is two rows)
        uint64_t cap = (uint64_t)(b1 - b0) / 4 * (o.k > 32 ? 2 : 1) + (uint64_t)N * 70000 + 4096;
        for (int attempt = 0; attempt < 3; ++attempt) {
          void *d = nullptr;
          if ((rc = cfrk_device_alloc(ctx, cap * 16, &d))) { refused[(size_t)sh] = 1; return; }
          rc = cfrk_global_export_runs_device(ctx, d, cap, N, rows[(size_t)sh].data());
          if (!rc) { d_packed[(size_t)sh] = d; return; }
          cfrk_device_free(ctx, d);
          if (rc == CFRK_ERR_SMALL_BUF) { cap *= 4; continue; }
          // (CFRK_ERR_STATE: something of this shard spilled into the HBM table -- its runs are not
          //  all in the leaf streams; the single-device path counts such input as well)
          if (rc == CFRK_ERR_STATE || rc == CFRK_ERR_NOMEM) { refused[(size_t)sh] = 1; return; }
          status[(size_t)sh] = die(ctx, rc, "cfrk_global_export_runs_device");
          return;
        }
        refused[(size_t)sh] = 1;
      });
    for (auto &t : th) t.join();
    for (int r : status) if (r) { free_packed(); return r; }
    for (char r : refused)
      if (r) {
        free_packed();
        fprintf(stderr, "cfrk: a shard could not export its runs; counting on one device\n");
        return run_global(o, batch, per_dev[0][0], out, est);
      }
  }
  std::vector<std::vector<uint64_t>> keys((size_t)N), his((size_t)N);
  std::vector<std::vector<uint32_t>> cnts((size_t)N);
  std::vector<Spectrum> spec(o.histo ? (size_t)N : 0);
  std::vector<double> histo_s((size_t)N, 0), export_s((size_t)N, 0), query_s((size_t)N, 0);
  std::vector<std::vector<uint32_t>> qans(o.query ? (size_t)N : 0);
  {
    // owner ow gathers its segment of every shard DEVICE TO DEVICE (xGMI peer-to-peer between the
    // devices of the node; replaces the host staging of round 2), then expands and counts its leaves
    std::vector<std::thread> th;
    for (int ow = 0; ow < N; ++ow)
      th.emplace_back([&, ow] {
        cfrk_ctx *ctx = per_dev[(size_t)ow][1].ctx;
        std::vector<uint64_t> recv((size_t)N);
        uint64_t total = 0;
        for (int sh = 0; sh < N; ++sh) { recv[(size_t)sh] = rows[(size_t)sh][(size_t)ow]; total += recv[(size_t)sh]; }
        int rc;
        if ((rc = cfrk_global_begin(ctx, o.k, flags, hint / (uint64_t)N + 1024))) { status[(size_t)ow] = die(ctx, rc, "cfrk_global_begin"); return; }
        if (total) {
          void *d = nullptr;
          if ((rc = cfrk_device_alloc(ctx, total * 16, &d))) { status[(size_t)ow] = die(ctx, rc, "cfrk_device_alloc"); return; }
          uint64_t at = 0;
          for (int sh = 0; sh < N && !rc; ++sh) {
            uint64_t off = 0;
            for (int q = 0; q < ow; ++q) off += rows[(size_t)sh][(size_t)q];
            if (recv[(size_t)sh])
              rc = cfrk_memcpy_peer(ctx, (char *)d + at * 16, per_dev[(size_t)sh][0].ctx, (const char *)d_packed[(size_t)sh] + off * 16, recv[(size_t)sh] * 16);
            at += recv[(size_t)sh];
          }
          if (!rc) rc = cfrk_global_merge_runs_device(ctx, d, recv.data(), N);
          if (!rc) rc = cfrk_ctx_sync(ctx);
          cfrk_device_free(ctx, d);
          if (rc) { status[(size_t)ow] = die(ctx, rc, "cfrk_global_merge_runs_device"); return; }
        }
        uint64_t n = 0;
        rc = cfrk_global_finish(ctx, &n);
        if (rc == CFRK_ERR_COUNT_OVERFLOW) fprintf(stderr, "cfrk: warning: %s\n", cfrk_last_error(ctx));
        else if (rc == CFRK_ERR_TABLE_FULL) { refused[(size_t)ow] = 1; return; }       // (more distinct k-mers than announced)
        else if (rc) { status[(size_t)ow] = die(ctx, rc, "cfrk_global_finish"); return; }
        const double h0 = now_s();
        if (o.histo && (rc = result_spectrum(ctx, spec[(size_t)ow]))) { status[(size_t)ow] = rc; return; }
        histo_s[(size_t)ow] = now_s() - h0;
        const double q0 = now_s();
        if (o.query && (rc = query_answers(ctx, qans[(size_t)ow]))) { status[(size_t)ow] = rc; return; }
        query_s[(size_t)ow] = now_s() - q0;
        if (o.histo_only || o.query_only) return;
        const double e0 = now_s();
        keys[(size_t)ow].resize(n); cnts[(size_t)ow].resize(n); his[(size_t)ow].resize(n);
        rc = cfrk_global_export_range(ctx, o.min_count, o.max_count, keys[(size_t)ow].data(), his[(size_t)ow].data(),
                                      cnts[(size_t)ow].data(), n, &n);
        if (rc && rc != CFRK_ERR_COUNT_OVERFLOW) { status[(size_t)ow] = die(ctx, rc, "cfrk_global_export_range"); return; }
        keys[(size_t)ow].resize(n); cnts[(size_t)ow].resize(n); his[(size_t)ow].resize(n);
        export_s[(size_t)ow] = now_s() - e0;
      });
    for (auto &t : th) t.join();
    free_packed();
    for (int r : status) if (r) return r;
    for (char r : refused)
      if (r) {
        fprintf(stderr, "cfrk: more distinct k-mers than announced; counting on one device\n");
        return run_global(o, batch, per_dev[0][0], out, est);
      }
  }
  g_timing.export_ = *std::max_element(export_s.begin(), export_s.end());
  if (o.histo) {
    const double h0 = now_s();
    for (int ow = 1; ow < N; ++ow) spec[0].add(spec[(size_t)ow]);
    if (int r = write_histo(o, spec[0])) return r;
    g_timing.histo = *std::max_element(histo_s.begin(), histo_s.end()) + (now_s() - h0);
  }
  if (o.query) {
    // owners hold disjoint key sets: at most one answers a window with a count, the others 0; NONE is everyone's
    const double q0 = now_s();
    std::vector<uint32_t> &ans = qans[0];
    for (int ow = 1; ow < N; ++ow)
      for (size_t p = 0; p < ans.size(); ++p)
        if (ans[p] != CFRK_QUERY_NONE) ans[p] += qans[(size_t)ow][p];
    if (int r = write_query(o, o.k, ans.data())) return r;
    g_timing.query = *std::max_element(query_s.begin(), query_s.end()) + (now_s() - q0);
  }
  if (o.histo_only || o.query_only) return 0;
  // N ascending lists with disjoint keys -> one ascending list
  size_t total = 0;
  for (auto &kk : keys) total += kk.size();
  std::vector<uint64_t> mk(total), mh(total);
  std::vector<uint32_t> mc(total);
  std::vector<size_t> at((size_t)N, 0);
  // (the high words are zero for k <= 32)
  auto less = [&](int a, int b) {
    const size_t ia = at[(size_t)a], ib = at[(size_t)b];
    const uint64_t ha = his[(size_t)a][ia], hb = his[(size_t)b][ib];
    return ha != hb ? ha < hb : keys[(size_t)a][ia] < keys[(size_t)b][ib];
  };
  for (size_t i = 0; i < total; ++i) {
    int best = -1;
    for (int q = 0; q < N; ++q)
      if (at[(size_t)q] < keys[(size_t)q].size() && (best < 0 || less(q, best))) best = q;
    const size_t ib = at[(size_t)best]++;
    mk[i] = keys[(size_t)best][ib]; mh[i] = his[(size_t)best][ib]; mc[i] = cnts[(size_t)best][ib];
  }
  write_global(o, mk.data(), mh.data(), mc.data(), total, out);
  return 0;
}

// --device-parse: the file goes to the device as text and is parsed there (cfrk_fasta_parse_device, or for FASTQ
// cfrk_fastq_parse_device); no host batch
struct DeviceText {
  cfrk_ctx *ctx = nullptr;
  void *d_text = nullptr, *d_start = nullptr, *d_length = nullptr, *d_regs = nullptr;
  int8_t *d_data = nullptr;
  size_t n_text = 0;
  ~DeviceText() { for (void *d : {d_text, (void *)d_data, d_start, d_length, d_regs}) if (d) cfrk_device_free(ctx, d); }
  // 0, a negative code of the host parser (the caller prints its message), or the exit status of a reported device error
  int load(const char *in, bool plain_copy, int fmt, int min_qual, int64_t *nN, int64_t *nS, double *map_s, double *h2d_s, double *parse_ms) {
    const bool fq = fmt == CFRK_FORMAT_FASTQ;
    auto parse = [&](int8_t *data, uint64_t cap_data, int64_t *start, int32_t *length, uint64_t cap_reads) {
      return fq ? cfrk_fastq_parse_device(ctx, (const uint8_t *)d_text, n_text, min_qual, data, cap_data, start, length, cap_reads, nN, nS)
                : cfrk_fasta_parse_device(ctx, (const uint8_t *)d_text, n_text, 0, data, cap_data, start, length, cap_reads, nN, nS);
    };
    const int fd = open(in, O_RDONLY);
    if (fd < 0) return -1;
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { close(fd); return -1; }
    const size_t n = (size_t)st.st_size;
    n_text = n;
    *nN = *nS = 0;
    if (n == 0) { close(fd); return 0; }
    int rc;
    if ((rc = cfrk_device_alloc(ctx, n + 16, &d_text))) { close(fd); return die(ctx, rc, "cfrk_device_alloc"); }
    // One copy from the mapping by default.  The ring of pinned staging buffers (--text-copy staged) was built for this
    // and measured: for a mapped, populated file it is no faster than the runtime's own pageable path.
    const double tm = now_s();
    void *m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) return -1;
    const double t0 = now_s();
    *map_s = t0 - tm;
    rc = plain_copy ? cfrk_memcpy_h2d(ctx, d_text, m, n) : cfrk_memcpy_h2d_staged(ctx, d_text, m, n);
    munmap(m, n);
    if (rc) return die(ctx, rc, plain_copy ? "cfrk_memcpy_h2d" : "cfrk_memcpy_h2d_staged");
    *h2d_s = now_s() - t0;
    const double t1 = now_s();
    rc = parse(nullptr, 0, nullptr, nullptr, 0);
    if (rc == CFRK_ERR_SMALL_BUF) {
      void *dd = nullptr;
      if ((rc = cfrk_device_alloc(ctx, (size_t)*nN + 64, &dd))) return die(ctx, rc, "cfrk_device_alloc");
      d_data = (int8_t *)dd;
      if ((rc = cfrk_device_alloc(ctx, (size_t)*nS * 8, &d_start)) || (rc = cfrk_device_alloc(ctx, (size_t)*nS * 4, &d_length)))
        return die(ctx, rc, "cfrk_device_alloc");
      rc = parse(d_data, (uint64_t)*nN, (int64_t *)d_start, (int32_t *)d_length, (uint64_t)*nS);
      if (!rc) rc = cfrk_ctx_sync(ctx);
    }
    // What the host parser refuses with -2 (a sequence line before the first header: the only text it can refuse in native
    // mode short of a record of 2^31 bases) is reported in its words; the wording looked for is pinned at its cfrk_fail in
    // ingest.hip and by tests/test_gpu_ingest.py.  Anything else the device parser refuses is reported in the library's.
    if (rc == CFRK_ERR_LAYOUT) {
      if (strstr(cfrk_last_error(ctx), "before the first header")) return -2;
      fprintf(stderr, "cfrk: cannot read %s (%s)\n", in, cfrk_last_error(ctx));
      return 1;
    }
    if (rc) return die(ctx, rc, fq ? "cfrk_fastq_parse_device" : "cfrk_fasta_parse_device");
    *parse_ms = (now_s() - t1) * 1e3;
    cfrk_device_free(ctx, d_text);                      // (the codes are what is counted)
    d_text = nullptr;
    return 0;
  }
  int sketch(const Options &o, int64_t nN, Estimate &e) {
    const double t0 = now_s();
    std::vector<uint8_t> regs(CFRK_SKETCH_REGS, 0);
    int rc;
    if (nN > 0) {
      if ((rc = cfrk_device_alloc(ctx, CFRK_SKETCH_REGS, &d_regs)) || (rc = cfrk_memcpy_h2d(ctx, d_regs, regs.data(), regs.size())))
        return die(ctx, rc, "cfrk_device_alloc");
      if ((rc = cfrk_distinct_sketch_device(ctx, d_data, nN, o.k, o.canonical ? CFRK_CANONICAL : 0, (uint8_t *)d_regs, &e.windows)))
        return die(ctx, rc, "cfrk_distinct_sketch_device");
      if ((rc = cfrk_memcpy_d2h(ctx, regs.data(), d_regs, regs.size()))) return die(ctx, rc, "cfrk_memcpy_d2h");
    }
    cfrk_sketch_estimate(regs.data(), &e.distinct);
    cfrk_sketch_hint(regs.data(), &e.hint);
    e.have = true;
    g_timing.estimate = now_s() - t0; g_timing.distinct_estimate = e.distinct;
    fprintf(stderr, "cfrk-estimate distinct=%.0f windows=%llu hint=%llu\n", e.distinct, (unsigned long long)e.windows, (unsigned long long)e.hint);
    return 0;
  }
};

// one FASTA file -> one .cfrk file on the given workers
// a FASTA file being parsed on a thread of its own while the caller creates the device contexts (single-file mode: HIP
// start-up and two contexts are ~0.15 s, the parse of a 1.6 GB file ~0.28 s -- they need nothing from each other)
double g_contexts_s = 0, g_wait_parse = 0;
struct Parsed {
  cfrk_batch batch;
  int rc = 0;
  double t0 = 0, seconds = 0;
  std::thread th;
  void start(const Options &o, const char *in, int fmt) {
    t0 = now_s();
    const int flags = (o.native || o.global || o.sparse) ? 0 : CFRK_INGEST_COMPAT, min_qual = o.min_qual;
    th = std::thread([this, in, fmt, flags, min_qual] { rc = read_reads(in, fmt, flags, min_qual, &batch); seconds = now_s() - t0; });
  }
};

int run_file(const Options &o, const char *in, const char *outp, std::vector<Worker> &workers,
             std::vector<std::vector<Worker>> *per_dev = nullptr, Parsed *pre = nullptr, int fmt = -1) {
  cfrk_batch batch;
  if (fmt < 0) {                                        // (--batch: every file is looked at on its own)
    fmt = file_format(o, in);
    if (!format_allowed(o, in, fmt)) return 1;
  }
  if (o.normalize_out) {
    if (o.normalize_format == CFRK_TEXT_FASTQ && fmt != CFRK_FORMAT_FASTQ) {
      fprintf(stderr, "cfrk: --normalize-format fastq needs a FASTQ input: %s is read as FASTA\n", in);
      return 1;
    }
    g_nformat = fmt; g_npath = in;
    if (o.normalize_names && read_whole_file(in, g_ntext)) return 1;
  }
  double t0 = now_s();
  int rc;
  DeviceText dt;
  dt.ctx = workers[0].ctx;
  double text_map = 0, text_h2d = 0, device_parse_ms = 0;
  if (o.device_parse) {
    memset(&batch, 0, sizeof batch);
    rc = dt.load(in, o.text_copy_plain, fmt, o.min_qual, &batch.nN, &batch.nS, &text_map, &text_h2d, &device_parse_ms);
    if (rc > 0) return rc;                              // (a device error, reported)
  } else if (pre) {
    const double w0 = now_s();
    pre->th.join();
    g_wait_parse = now_s() - w0;
    rc = pre->rc; batch = pre->batch; t0 = pre->t0;
    if (rc) return 1;                                   // (read_reads has said why)
  } else {
    if (read_reads(in, fmt, (o.native || o.global || o.sparse) ? 0 : CFRK_INGEST_COMPAT, o.min_qual, &batch)) return 1;
    rc = 0;
  }
  if (rc) { fprintf(stderr, "cfrk: cannot read %s (error %d)\n", in, rc); return 1; }
  const double t1 = pre ? t0 + pre->seconds : now_s();
  g_timing = Timing();
  g_timing.contexts = g_contexts_s; g_timing.wait_parse = g_wait_parse;
  g_timing.parse = t1 - t0; g_timing.nN = batch.nN; g_timing.nS = batch.nS; g_timing.in_format = fmt;
  if (o.device_parse) { g_timing.parse = 0; g_timing.device_parse = true; g_timing.text_map = text_map; g_timing.text_h2d = text_h2d; g_timing.device_parse_ms = device_parse_ms; }
  { FILE *f = fopen(in, "rb"); if (f) { fseek(f, 0, SEEK_END); g_timing.fasta_bytes = (int64_t)ftell(f); fclose(f); } }
  std::thread freer;                                  // (global mode: frees the batch beside the export)
  const double to0 = now_s();
  const bool no_out = o.histo_only || o.query_only || o.estimate_only;
  FILE *out = no_out ? nullptr : fopen(outp, "wb");   // PrintFreq opens with "w" even when empty
  const double t_open = now_s() - to0;
  if (!out && !no_out) { fprintf(stderr, "cfrk: cannot write %s\n", outp); cfrk_host_free_batch(&batch); return 1; }
  const bool multi = o.global && per_dev && per_dev->size() > 1 && o.k >= 16 && o.k <= 64 && batch.nS >= (int64_t)per_dev->size();
  Estimate est;
  rc = 0;
  if (o.estimate || o.estimate_only || o.auto_hint) {
    std::vector<cfrk_ctx *> ctxs;
    if (multi) for (auto &d : *per_dev) ctxs.push_back(d[0].ctx);
    else ctxs.push_back(workers[0].ctx);
    rc = o.device_parse ? dt.sketch(o, batch.nN, est) : sketch_batch(o, batch, ctxs, est);
  }
  if (!rc && !o.estimate_only) {
    if (multi) rc = run_global_multi(o, batch, *per_dev, out, est);
    else if (o.device_parse) rc = run_global(o, batch, workers[0], out, est, nullptr, nullptr, true, dt.d_data);
    else if (o.global) rc = run_global(o, batch, workers[0], out, est, &freer, &batch);
    else { const double p0 = now_s(); rc = run_per_read(o, batch, workers, out); g_timing.per_read = now_s() - p0; }
  }
  if (!o.global && out) { fflush(out); g_timing.out_bytes = (uint64_t)ftell(out); }
  const double tf0 = now_s();
  if (out) fclose(out);
  const double tf1 = now_s();
  if (freer.joinable()) freer.join();
  else cfrk_host_free_batch(&batch);
  g_timing.total = now_s() - t0;
  g_timing.close = tf1 - tf0; g_timing.free_batch = now_s() - tf1; g_timing.open = t_open;
  char query_field[192] = "";     // (only with --query / --device-parse: the line is unchanged otherwise)
  if (g_timing.device_parse) snprintf(query_field, sizeof query_field, "\"text_map_s\": %.4f, \"text_h2d_s\": %.4f, \"device_parse_ms\": %.3f, ", g_timing.text_map, g_timing.text_h2d, g_timing.device_parse_ms);
  const size_t qf = strlen(query_field);
  if (o.query_stats) snprintf(query_field + qf, sizeof query_field - qf, "\"query_s\": %.4f, \"stats_s\": %.4f, ", g_timing.query, g_timing.stats);
  else if (o.query) snprintf(query_field + qf, sizeof query_field - qf, "\"query_s\": %.4f, ", g_timing.query);
  if (o.timing)
    fprintf(stderr, "cfrk-timing {\"fasta_bytes\": %lld, \"reads\": %lld, \"code_bytes\": %lld, \"parse_s\": %.4f, \"add_call_s\": %.4f, "
            "\"finish_wait_s\": %.4f, \"count_kernels_ms\": %.3f, \"export_s\": %.4f, \"format_s\": %.4f, \"write_s\": %.4f, "
            "\"per_read_pipeline_s\": %.4f, \"entries\": %llu, \"out_bytes\": %llu, \"contexts_s\": %.4f, \"wait_for_parser_s\": %.4f, "
            "\"begin_s\": %.4f, \"open_out_s\": %.4f, \"close_out_s\": %.4f, \"free_batch_s\": %.4f, \"histo_s\": %.4f, %s\"attempts\": %d, "
            "\"estimate_s\": %.4f, \"distinct_estimate\": %.0f, \"hint\": %llu, \"format\": \"%s\", \"wall_s\": %.4f}\n",
            (long long)g_timing.fasta_bytes, (long long)g_timing.nS, (long long)g_timing.nN, g_timing.parse, g_timing.add_call,
            g_timing.finish_wait, (double)g_timing.count_kernels_ms, g_timing.export_, g_timing.format, g_timing.write,
            g_timing.per_read, (unsigned long long)g_timing.entries, (unsigned long long)g_timing.out_bytes, g_timing.contexts,
            g_timing.wait_parse, g_timing.begin, g_timing.open, g_timing.close, g_timing.free_batch, g_timing.histo, query_field, g_timing.attempts,
            g_timing.estimate, g_timing.distinct_estimate, (unsigned long long)g_timing.hint, g_timing.in_format == CFRK_FORMAT_FASTQ ? "fastq" : "fasta", g_timing.total);
  return rc;
}

// --query-db: a saved CFRKGLB1 count file merged into a fresh job on one device, then queried
int run_query_db(const Options &o) {
  std::string img;
  {
    FILE *f = fopen(o.query_db, "rb");
    if (!f) { fprintf(stderr, "cfrk: cannot read %s\n", o.query_db); return 1; }
    char tmp[1 << 16];
    size_t got;
    while ((got = fread(tmp, 1, sizeof tmp, f)) > 0) img.append(tmp, got);
    fclose(f);
  }
  int k = 0, bflags = 0;
  uint64_t n = 0;
  if (cfrk_host_read_binary(img.data(), img.size(), &k, &bflags, &n, nullptr, nullptr, nullptr) || k < 1 || k > 64) {
    fprintf(stderr, "cfrk: %s is not a CFRKGLB1 count file\n", o.query_db);
    return 1;
  }
  std::vector<uint64_t> lo(n), hi(n);
  std::vector<uint32_t> cnt(n);
  cfrk_host_read_binary(img.data(), img.size(), &k, &bflags, &n, lo.data(), hi.data(), cnt.data());
  img.clear();
  img.shrink_to_fit();
  cfrk_ctx *ctx = nullptr;
  int rc;
  if ((rc = cfrk_ctx_create(o.device, nullptr, &ctx))) return die(nullptr, rc, "cfrk_ctx_create");
  struct Destroy { cfrk_ctx *c; ~Destroy() { cfrk_ctx_destroy(c); } } destroy{ctx};
  const double q0 = now_s();
  if ((rc = cfrk_global_begin(ctx, k, (bflags & CFRK_BIN_CANONICAL) ? CFRK_CANONICAL : 0, n + 1024)))
    return die(ctx, rc, "cfrk_global_begin");
  if (n) {
    void *d_lo = nullptr, *d_hi = nullptr, *d_cnt = nullptr;
    if (!(rc = cfrk_device_alloc(ctx, n * 8, &d_lo)) && !(rc = cfrk_device_alloc(ctx, n * 8, &d_hi)) &&
        !(rc = cfrk_device_alloc(ctx, n * 4, &d_cnt)) && !(rc = cfrk_memcpy_h2d(ctx, d_lo, lo.data(), n * 8)) &&
        !(rc = cfrk_memcpy_h2d(ctx, d_hi, hi.data(), n * 8)) && !(rc = cfrk_memcpy_h2d(ctx, d_cnt, cnt.data(), n * 4)) &&
        !(rc = cfrk_global_merge_device(ctx, (const uint64_t *)d_lo, (const uint64_t *)d_hi, (const uint32_t *)d_cnt, (int64_t)n)))
      rc = cfrk_ctx_sync(ctx);
    for (void *d : {d_lo, d_hi, d_cnt}) if (d) cfrk_device_free(ctx, d);
    if (rc) return die(ctx, rc, "loading the count file");
  }
  if (o.query_out) {
    std::vector<uint32_t> ans;
    if ((rc = query_answers(ctx, ans)) || (rc = write_query(o, k, ans.data()))) return rc;
  }
  const double s0 = now_s();
  if (o.query_stats && (rc = write_query_stats(o, ctx))) return rc;
  if ((rc = check_query_pairs(o, ctx))) return rc;
  if (o.filter_out && (rc = write_filter(o, ctx, k))) return rc;
  if (o.correct_out && (rc = write_correct(o, ctx))) return rc;
  if (o.timing && o.query_stats)
    fprintf(stderr, "cfrk-timing {\"entries\": %llu, \"query_s\": %.4f, \"stats_s\": %.4f}\n", (unsigned long long)n, s0 - q0, now_s() - s0);
  else if (o.timing) fprintf(stderr, "cfrk-timing {\"entries\": %llu, \"query_s\": %.4f}\n", (unsigned long long)n, now_s() - q0);
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  std::vector<const char *> pos;
  Options o;
  int batch_n = -1;
  bool unitigs_opt_set = false;
  bool tip_opt_set = false, tip_rounds_set = false, bubble_opt_set = false;
  bool range_set = false, stats_below_set = false, filter_opt_set = false, correct_opt_set = false, correct_min_count_set = false, normalize_opt_set = false, normalize_cutoff_set = false;
  bool pair_opt_set = false, pair_mode_set = false;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--all-chunks")) o.all_chunks = true;
    else if (!strcmp(argv[i], "--native")) o.native = true;
    else if (!strcmp(argv[i], "--global")) o.global = true;
    else if (!strcmp(argv[i], "--canonical")) o.canonical = true;
    else if (!strcmp(argv[i], "--sparse")) o.sparse = true;
    else if (!strcmp(argv[i], "--binary")) o.binary = true;
    else if (!strcmp(argv[i], "--timing")) o.timing = true;
    else if (!strcmp(argv[i], "--parse-threads") && i + 1 < argc) cfrk_host_set_parse_threads(atoi(argv[++i]));
    else if (!strcmp(argv[i], "--same-device")) o.same_device = true;   // rehearsal: every "device" is --device
    else if (!strcmp(argv[i], "--device") && i + 1 < argc) o.device = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--gpus") && i + 1 < argc) o.gpus = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--batch") && i + 1 < argc) batch_n = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--histo-only")) o.histo_only = true;
    else if (!strcmp(argv[i], "--estimate")) o.estimate = true;
    else if (!strcmp(argv[i], "--estimate-only")) o.estimate_only = true;
    else if (!strcmp(argv[i], "--auto-hint")) o.auto_hint = true;
    else if (!strcmp(argv[i], "--device-parse")) o.device_parse = true;
    else if (!strcmp(argv[i], "--text-copy") && i + 1 < argc) {
      const char *v = argv[++i];
      if (strcmp(v, "plain") && strcmp(v, "staged")) { fprintf(stderr, "cfrk: --text-copy takes plain or staged, not '%s'\n", v); return 1; }
      o.text_copy_plain = !strcmp(v, "plain");
    }
    else if (!strcmp(argv[i], "--format") && i + 1 < argc) {
      const char *v = argv[++i];
      if (!strcmp(v, "fasta")) o.format = CFRK_FORMAT_FASTA;
      else if (!strcmp(v, "fastq")) o.format = CFRK_FORMAT_FASTQ;
      else if (!strcmp(v, "auto")) o.format = -1;
      else { fprintf(stderr, "cfrk: --format takes fasta, fastq or auto, not '%s'\n", v); return 1; }
    }
    else if (!strcmp(argv[i], "--min-qual") && i + 1 < argc) {
      const char *v = argv[++i];
      char *end = nullptr;
      const long q = strtol(v, &end, 10);
      if (!*v || *end || q < 0 || q > CFRK_FASTQ_MAX_QUAL) { fprintf(stderr, "cfrk: --min-qual needs an integer from 0 to %d, not '%s'\n", CFRK_FASTQ_MAX_QUAL, v); return 1; }
      o.min_qual = (int)q; o.min_qual_set = true;
    }
    else if (!strcmp(argv[i], "--query-only")) o.query_only = true;
    else if (!strcmp(argv[i], "--paired")) o.paired = true;
    else if (!strcmp(argv[i], "--pair-check") || !strcmp(argv[i], "--pair-mode") || !strcmp(argv[i], "--query2")) {
      if (i + 1 >= argc) { fprintf(stderr, "cfrk: %s needs a value\n", argv[i]); return 1; }
      const char *opt = argv[i], *v = argv[++i];
      if (!strcmp(opt, "--query2")) o.query2 = v;
      else if (!strcmp(opt, "--pair-check")) {
        if (strcmp(v, "on") && strcmp(v, "off")) { fprintf(stderr, "cfrk: --pair-check takes on or off, not '%s'\n", v); return 1; }
        o.pair_check = !strcmp(v, "on"); pair_opt_set = true;
      } else {
        if (strcmp(v, "either") && strcmp(v, "both")) { fprintf(stderr, "cfrk: --pair-mode takes either or both, not '%s'\n", v); return 1; }
        o.pair_mode = !strcmp(v, "both") ? CFRK_PAIR_BOTH : CFRK_PAIR_EITHER; pair_mode_set = true;
      }
    }
    else if (!strcmp(argv[i], "--query") || !strcmp(argv[i], "--query-out") || !strcmp(argv[i], "--query-db")) {
      if (i + 1 >= argc) { fprintf(stderr, "cfrk: %s needs a value\n", argv[i]); return 1; }
      const char *opt = argv[i], *v = argv[++i];
      if (!strcmp(opt, "--query")) o.query = v;
      else if (!strcmp(opt, "--query-out")) o.query_out = v;
      else o.query_db = v;
    }
    else if (!strcmp(argv[i], "--query-stats") || !strcmp(argv[i], "--stats-below")) {
      if (i + 1 >= argc) { fprintf(stderr, "cfrk: %s needs a value\n", argv[i]); return 1; }
      const char *opt = argv[i], *v = argv[++i];
      if (!strcmp(opt, "--query-stats")) { o.query_stats = v; continue; }
      if (!parse_count(v, &o.stats_below)) { fprintf(stderr, "cfrk: %s needs a count (an integer from 0 to 4294967295), not '%s'\n", opt, v); return 1; }
      stats_below_set = true;
    }
    else if (!strncmp(argv[i], "--filter-", 9)) {
      const char *opt = argv[i];
      static const char *const known[] = {"--filter-out", "--filter-min-count", "--filter-max-count", "--filter-trim", "--filter-min-len",
                                          "--filter-min-median", "--filter-max-median", "--filter-names", "--filter-format",
                                          "--filter-out2", "--filter-orphans"};
      bool is_known = false;
      for (const char *n : known) is_known = is_known || !strcmp(opt, n);
      if (!is_known) { fprintf(stderr, "cfrk: unknown option %s\n", opt); return 1; }
      if (!strcmp(opt, "--filter-names")) { o.filter_names = true; filter_opt_set = true; continue; }
      if (i + 1 >= argc) { fprintf(stderr, "cfrk: %s needs a value\n", opt); return 1; }
      const char *v = argv[++i];
      if (!strcmp(opt, "--filter-out")) { o.filter_out = v; continue; }
      if (!strcmp(opt, "--filter-out2")) { o.filter_out2 = v; continue; }
      if (!strcmp(opt, "--filter-orphans")) { o.filter_orphans = v; continue; }
      filter_opt_set = true;
      if (!strcmp(opt, "--filter-format")) {
        if (!strcmp(v, "fasta")) o.filter_format = CFRK_TEXT_FASTA;
        else if (!strcmp(v, "fastq")) { o.filter_format = CFRK_TEXT_FASTQ; o.filter_names = true; }
        else { fprintf(stderr, "cfrk: --filter-format takes fasta or fastq, not '%s'\n", v); return 1; }
      } else if (!strcmp(opt, "--filter-trim")) {
        if (!strcmp(v, "longest")) o.filter_trim = CFRK_SPAN_LONGEST;
        else if (!strcmp(v, "prefix")) o.filter_trim = CFRK_SPAN_PREFIX;
        else if (!strcmp(v, "none")) o.filter_trim = -1;
        else { fprintf(stderr, "cfrk: --filter-trim takes longest, prefix or none, not '%s'\n", v); return 1; }
      } else if (!strcmp(opt, "--filter-min-len")) {
        char *end = nullptr;
        const long long L = strtoll(v, &end, 10);
        if (!*v || *end || L < 0 || L > 0x7FFFFFFFll) { fprintf(stderr, "cfrk: --filter-min-len needs a length (an integer from 0 to 2147483647), not '%s'\n", v); return 1; }
        o.filter_min_len = (long)L;
      } else {
        uint32_t x;
        if (!parse_count(v, &x)) { fprintf(stderr, "cfrk: %s needs a count (an integer from 0 to 4294967295), not '%s'\n", opt, v); return 1; }
        if (!strcmp(opt, "--filter-min-count")) o.filter_min_count = x;
        else if (!strcmp(opt, "--filter-max-count")) o.filter_max_count = x;
        else if (!strcmp(opt, "--filter-min-median")) { o.filter_min_median = x; o.filter_median = true; }
        else { o.filter_max_median = x; o.filter_median = true; }
      }
    }
    else if (!strncmp(argv[i], "--correct-", 10)) {
      const char *opt = argv[i];
      static const char *const known[] = {"--correct-out", "--correct-min-count", "--correct-names", "--correct-format", "--correct-report",
                                          "--correct-out2"};
      bool is_known = false;
      for (const char *n : known) is_known = is_known || !strcmp(opt, n);
      if (!is_known) { fprintf(stderr, "cfrk: unknown option %s\n", opt); return 1; }
      if (!strcmp(opt, "--correct-names")) { o.correct_names = true; correct_opt_set = true; continue; }
      if (i + 1 >= argc) { fprintf(stderr, "cfrk: %s needs a value\n", opt); return 1; }
      const char *v = argv[++i];
      if (!strcmp(opt, "--correct-out")) { o.correct_out = v; continue; }
      if (!strcmp(opt, "--correct-out2")) { o.correct_out2 = v; continue; }
      correct_opt_set = true;
      if (!strcmp(opt, "--correct-format")) {
        if (!strcmp(v, "fasta")) o.correct_format = CFRK_TEXT_FASTA;
        else if (!strcmp(v, "fastq")) { o.correct_format = CFRK_TEXT_FASTQ; o.correct_names = true; }
        else { fprintf(stderr, "cfrk: --correct-format takes fasta or fastq, not '%s'\n", v); return 1; }
      } else if (!strcmp(opt, "--correct-report")) {
        o.correct_report = v;
      } else {
        if (!parse_count(v, &o.correct_min_count)) { fprintf(stderr, "cfrk: %s needs a count (an integer from 0 to 4294967295), not '%s'\n", opt, v); return 1; }
        correct_min_count_set = true;
      }
    }
    else if (!strncmp(argv[i], "--normalize-", 12)) {
      const char *opt = argv[i];
      static const char *const known[] = {"--normalize-out", "--normalize-cutoff", "--normalize-batch", "--normalize-names", "--normalize-format"};
      bool is_known = false;
      for (const char *n : known) is_known = is_known || !strcmp(opt, n);
      if (!is_known) { fprintf(stderr, "cfrk: unknown option %s\n", opt); return 1; }
      if (!strcmp(opt, "--normalize-names")) { o.normalize_names = true; normalize_opt_set = true; continue; }
      if (i + 1 >= argc) { fprintf(stderr, "cfrk: %s needs a value\n", opt); return 1; }
      const char *v = argv[++i];
      if (!strcmp(opt, "--normalize-out")) { o.normalize_out = v; continue; }
      normalize_opt_set = true;
      if (!strcmp(opt, "--normalize-format")) {
        if (!strcmp(v, "fasta")) o.normalize_format = CFRK_TEXT_FASTA;
        else if (!strcmp(v, "fastq")) o.normalize_format = CFRK_TEXT_FASTQ;
        else { fprintf(stderr, "cfrk: --normalize-format takes fasta or fastq, not '%s'\n", v); return 1; }
        o.normalize_names = true;
      } else if (!strcmp(opt, "--normalize-batch")) {
        char *end = nullptr;
        const long long B = strtoll(v, &end, 10);
        if (!*v || *end || B < 1) { fprintf(stderr, "cfrk: --normalize-batch needs a number of reads (an integer from 1), not '%s'\n", v); return 1; }
        o.normalize_batch = B;
      } else {
        if (!parse_count(v, &o.normalize_cutoff)) { fprintf(stderr, "cfrk: %s needs a count (an integer from 0 to 4294967295), not '%s'\n", opt, v); return 1; }
        normalize_cutoff_set = true;
      }
    }
    else if (!strcmp(argv[i], "--histo") || !strcmp(argv[i], "--min-count") || !strcmp(argv[i], "--max-count")) {
      if (i + 1 >= argc) { fprintf(stderr, "cfrk: %s needs a value\n", argv[i]); return 1; }
      const char *opt = argv[i], *v = argv[++i];
      if (!strcmp(opt, "--histo")) { o.histo = v; continue; }
      uint32_t x;
      if (!parse_count(v, &x)) { fprintf(stderr, "cfrk: %s needs a count (an integer from 0 to 4294967295), not '%s'\n", opt, v); return 1; }
      if (!strcmp(opt, "--min-count")) o.min_count = x;     // (0 reads as 1: cfrk_global_export_range)
      else o.max_count = x;
      range_set = true;
    }
    else if (!strcmp(argv[i], "--unitigs-links")) o.unitigs_links = true;
    else if (!strcmp(argv[i], "--unitigs-clip-tips")) o.clip_tips = true;
    else if (!strcmp(argv[i], "--tip-max-kmers") || !strcmp(argv[i], "--tip-ratio") || !strcmp(argv[i], "--tip-rounds") ||
             !strcmp(argv[i], "--tip-report")) {
      if (i + 1 >= argc) { fprintf(stderr, "cfrk: %s needs a value\n", argv[i]); return 1; }
      const char *opt = argv[i], *v = argv[++i];
      if (!strcmp(opt, "--tip-report")) { o.tip_report = v; continue; }
      tip_opt_set = true;
      if (!strcmp(opt, "--tip-ratio")) {
        char *end = nullptr;
        const double r = strtod(v, &end);
        if (end == v || *end || !(r >= 0.0 && r <= 256.0)) { fprintf(stderr, "cfrk: --tip-ratio needs a number from 0 to 256, not '%s'\n", v); return 1; }
        o.tip_ratio_q8 = (uint32_t)(r * 256.0 + 0.5);
        continue;
      }
      uint32_t x;
      if (!parse_count(v, &x) || x < 1) { fprintf(stderr, "cfrk: %s needs a count (an integer from 1 to 4294967295), not '%s'\n", opt, v); return 1; }
      if (!strcmp(opt, "--tip-max-kmers")) o.tip_max_kmers = x; else { o.tip_rounds = x; tip_rounds_set = true; }
    }
    else if (!strcmp(argv[i], "--unitigs-pop-bubbles")) o.pop_bubbles = true;
    else if (!strcmp(argv[i], "--bubble-max-kmers") || !strcmp(argv[i], "--bubble-max-diff") || !strcmp(argv[i], "--bubble-ratio") ||
             !strcmp(argv[i], "--bubble-report") || !strcmp(argv[i], "--simplify-rounds")) {
      if (i + 1 >= argc) { fprintf(stderr, "cfrk: %s needs a value\n", argv[i]); return 1; }
      const char *opt = argv[i], *v = argv[++i];
      bubble_opt_set = true;
      if (!strcmp(opt, "--bubble-report")) { o.bubble_report = v; continue; }
      if (!strcmp(opt, "--bubble-ratio")) {
        char *end = nullptr;
        const double r = strtod(v, &end);
        if (end == v || *end || !(r >= 0.0 && r <= 256.0)) { fprintf(stderr, "cfrk: --bubble-ratio needs a number from 0 to 256, not '%s'\n", v); return 1; }
        o.bubble_ratio_q8 = (uint32_t)(r * 256.0 + 0.5);
        continue;
      }
      uint32_t x;
      const uint32_t least = strcmp(opt, "--bubble-max-diff") ? 1u : 0u;
      if (!parse_count(v, &x) || x < least) {
        fprintf(stderr, "cfrk: %s needs a count (an integer from %u to 4294967295), not '%s'\n", opt, least, v);
        return 1;
      }
      if (!strcmp(opt, "--bubble-max-kmers")) o.bubble_max_kmers = x;
      else if (!strcmp(opt, "--bubble-max-diff")) o.bubble_max_diff = x;
      else o.simplify_rounds = x;
    }
    else if (!strcmp(argv[i], "--unitigs-out") || !strcmp(argv[i], "--unitigs-min-count") || !strcmp(argv[i], "--unitigs-gfa") ||
             !strcmp(argv[i], "--unitigs-map") || !strcmp(argv[i], "--unitigs-map-out")) {
      if (i + 1 >= argc) { fprintf(stderr, "cfrk: %s needs a value\n", argv[i]); return 1; }
      const char *opt = argv[i], *v = argv[++i];
      if (!strcmp(opt, "--unitigs-out")) { o.unitigs_out = v; continue; }
      if (!strcmp(opt, "--unitigs-gfa")) { o.unitigs_gfa = v; continue; }
      if (!strcmp(opt, "--unitigs-map")) { o.unitigs_map = v; continue; }
      if (!strcmp(opt, "--unitigs-map-out")) { o.unitigs_map_out = v; continue; }
      if (!parse_count(v, &o.unitigs_min_count)) { fprintf(stderr, "cfrk: %s needs a count (an integer from 0 to 4294967295), not '%s'\n", opt, v); return 1; }
      unitigs_opt_set = true;
    }
    else pos.push_back(argv[i]);
  }
  // (refused here: before the input is parsed or a device is opened)
  if (o.unitigs_out && (!o.global || o.gpus > 1 || batch_n >= 0 || o.sparse)) {
    fprintf(stderr, "cfrk: --unitigs-out needs --global on one device: not with --gpus above 1, --batch or --sparse\n");
    return 1;
  }
  if (o.unitigs_gfa && (!o.global || o.gpus > 1 || batch_n >= 0 || o.sparse)) {
    fprintf(stderr, "cfrk: --unitigs-gfa needs --global on one device: not with --gpus above 1, --batch or --sparse\n");
    return 1;
  }
  if ((o.unitigs_map != nullptr) != (o.unitigs_map_out != nullptr)) {
    fprintf(stderr, "cfrk: --unitigs-map QFILE and --unitigs-map-out MFILE go together\n");
    return 1;
  }
  if (o.unitigs_map && (!o.global || o.gpus > 1 || batch_n >= 0 || o.sparse)) {
    fprintf(stderr, "cfrk: --unitigs-map needs --global on one device: not with --gpus above 1, --batch or --sparse\n");
    return 1;
  }
  if (o.clip_tips && !o.unitigs_out && !o.unitigs_gfa && !o.unitigs_map) {
    fprintf(stderr, "cfrk: --unitigs-clip-tips needs --unitigs-out UFILE, --unitigs-gfa GFILE or --unitigs-map QFILE\n");
    return 1;
  }
  if (o.pop_bubbles && !o.unitigs_out && !o.unitigs_gfa && !o.unitigs_map) {
    fprintf(stderr, "cfrk: --unitigs-pop-bubbles needs --unitigs-out UFILE, --unitigs-gfa GFILE or --unitigs-map QFILE\n");
    return 1;
  }
  if (bubble_opt_set && !o.pop_bubbles) {
    fprintf(stderr, "cfrk: --bubble-max-kmers, --bubble-max-diff, --bubble-ratio, --bubble-report and --simplify-rounds need --unitigs-pop-bubbles\n");
    return 1;
  }
  if (tip_rounds_set && o.pop_bubbles) {
    fprintf(stderr, "cfrk: --tip-rounds is the tip loop's own: with --unitigs-pop-bubbles the rounds are set by --simplify-rounds N\n");
    return 1;
  }
  if ((tip_opt_set && !o.clip_tips) || (o.tip_report && !o.clip_tips && !o.pop_bubbles)) {
    fprintf(stderr, "cfrk: --tip-max-kmers, --tip-ratio, --tip-rounds and --tip-report need --unitigs-clip-tips\n");
    return 1;
  }
  if (o.unitigs_links && !o.unitigs_out) { fprintf(stderr, "cfrk: --unitigs-links needs --unitigs-out UFILE\n"); return 1; }
  if (unitigs_opt_set && !o.unitigs_out && !o.unitigs_gfa && !o.unitigs_map) { fprintf(stderr, "cfrk: --unitigs-min-count needs --unitigs-out UFILE\n"); return 1; }
  if (o.sparse && (o.global || o.binary || o.histo || o.histo_only || range_set || o.query || o.query_out || o.query_only ||
                   o.query_db || o.query_stats || stats_below_set || o.filter_out || filter_opt_set || o.correct_out || correct_opt_set)) {
    fprintf(stderr, "cfrk: --sparse is a per-read mode: not with --global, --binary, --histo, --query or --min-count / --max-count\n");
    return 1;
  }
  if ((o.histo || o.histo_only || range_set) && !o.global) {
    fprintf(stderr, "cfrk: --histo, --histo-only, --min-count and --max-count need --global\n");
    return 1;
  }
  if ((o.estimate || o.estimate_only || o.auto_hint) && !o.global) {
    fprintf(stderr, "cfrk: --estimate, --estimate-only and --auto-hint need --global\n");
    return 1;
  }
  if (o.device_parse && (!o.global || o.gpus > 1 || batch_n >= 0)) {
    fprintf(stderr, "cfrk: --device-parse needs --global on one device: not with --gpus above 1 or --batch\n");
    return 1;
  }
  if (o.estimate_only && batch_n >= 0) { fprintf(stderr, "cfrk: --estimate-only prints one estimate: not with --batch\n"); return 1; }
  if (o.histo_only && !o.histo) { fprintf(stderr, "cfrk: --histo-only needs --histo FILE\n"); return 1; }
  if (o.min_count > o.max_count) {
    fprintf(stderr, "cfrk: --min-count %u is above --max-count %u\n", o.min_count, o.max_count);
    return 1;
  }
  if (o.histo && batch_n >= 0) { fprintf(stderr, "cfrk: --histo writes one file: not with --batch\n"); return 1; }
  if (o.query && !o.global && !o.query_db) { fprintf(stderr, "cfrk: --query needs --global or --query-db\n"); return 1; }
  if ((o.query_out || o.query_only || o.query_db) && !o.query) {
    fprintf(stderr, "cfrk: --query-out, --query-only and --query-db need --query QFILE\n");
    return 1;
  }
  if ((o.query_stats || stats_below_set) && !o.query) { fprintf(stderr, "cfrk: --query-stats and --stats-below need --query QFILE\n"); return 1; }
  if (stats_below_set && !o.query_stats) { fprintf(stderr, "cfrk: --stats-below needs --query-stats SFILE\n"); return 1; }
  if ((o.filter_out || filter_opt_set) && !o.query) { fprintf(stderr, "cfrk: --filter-out and the --filter- options need --query QFILE\n"); return 1; }
  if (filter_opt_set && !o.filter_out) { fprintf(stderr, "cfrk: the --filter- options need --filter-out FFILE\n"); return 1; }
  if (correct_opt_set && !o.correct_out) { fprintf(stderr, "cfrk: the --correct- options need --correct-out CFILE\n"); return 1; }
  if (o.correct_out && !o.query) { fprintf(stderr, "cfrk: --correct-out and the --correct- options need --query QFILE\n"); return 1; }
  if (o.correct_out && !correct_min_count_set) { fprintf(stderr, "cfrk: --correct-out needs --correct-min-count T\n"); return 1; }
  // paired-end reads
  if (o.paired && o.query2) { fprintf(stderr, "cfrk: --paired says the mates are interleaved in one file, --query2 that they are in two: one of them\n"); return 1; }
  if (o.query2 && o.normalize_out && !o.filter_out && !o.correct_out) {
    fprintf(stderr, "cfrk: --normalize-out takes ONE input file: mates in two files are not supported, interleave them and say --paired\n");
    return 1;
  }
  if (o.query2 && !o.query) { fprintf(stderr, "cfrk: --query2 needs --query QFILE\n"); return 1; }
  if (o.paired && o.gpus > 1) { fprintf(stderr, "cfrk: --paired runs on one device: not with --gpus above 1\n"); return 1; }
  if (o.paired && batch_n >= 0) { fprintf(stderr, "cfrk: --paired reads one file: not with --batch\n"); return 1; }
  if (o.paired && !o.filter_out && !o.correct_out && !o.normalize_out) {
    fprintf(stderr, "cfrk: --paired needs --filter-out FFILE, --correct-out CFILE or --normalize-out NFILE\n");
    return 1;
  }
  if (o.query2 && !o.filter_out && !o.correct_out) { fprintf(stderr, "cfrk: --query2 needs --filter-out FFILE or --correct-out CFILE\n"); return 1; }
  if (o.query2 && o.filter_out && !o.filter_out2) { fprintf(stderr, "cfrk: --query2 needs --filter-out2 FFILE2 beside --filter-out\n"); return 1; }
  if (o.query2 && o.correct_out && !o.correct_out2) { fprintf(stderr, "cfrk: --query2 needs --correct-out2 CFILE2 beside --correct-out\n"); return 1; }
  if ((o.filter_out2 && !(o.query2 && o.filter_out)) || (o.correct_out2 && !(o.query2 && o.correct_out))) {
    fprintf(stderr, "cfrk: --filter-out2 and --correct-out2 receive QFILE2's reads: they need --query2 and --filter-out / --correct-out\n");
    return 1;
  }
  if (o.filter_orphans && !(o.mates() && o.filter_out)) { fprintf(stderr, "cfrk: --filter-orphans needs --paired or --query2, and --filter-out\n"); return 1; }
  if ((pair_opt_set && !o.mates()) || (pair_mode_set && !(o.paired && o.normalize_out))) {
    fprintf(stderr, "cfrk: --pair-check needs --paired or --query2; --pair-mode needs --paired with --normalize-out\n");
    return 1;
  }
  if (o.paired && o.normalize_out && (o.normalize_batch & 1)) {
    fprintf(stderr, "cfrk: --normalize-batch %lld: a round of --paired reads holds whole pairs, an even number\n", o.normalize_batch);
    return 1;
  }
  if (o.query && !o.query_out && !o.query_stats && !o.filter_out && !o.correct_out) { fprintf(stderr, "cfrk: --query needs --query-out OFILE, --query-stats SFILE, --filter-out FFILE or --correct-out CFILE\n"); return 1; }
  if (o.correct_out && o.gpus > 1) { fprintf(stderr, "cfrk: --correct-out runs on one device: not with --gpus above 1\n"); return 1; }
  if (o.filter_out && o.gpus > 1) { fprintf(stderr, "cfrk: --filter-out runs on one device: not with --gpus above 1\n"); return 1; }
  if (o.query_stats && o.gpus > 1) { fprintf(stderr, "cfrk: --query-stats runs on one device: not with --gpus above 1\n"); return 1; }
  if (o.query && batch_n >= 0) { fprintf(stderr, "cfrk: --query writes one file: not with --batch\n"); return 1; }
  if (o.query_db && !pos.empty()) { fprintf(stderr, "cfrk: --query-db takes no positional arguments\n"); return 1; }
  if (o.query_db && o.min_qual_set) { fprintf(stderr, "cfrk: --min-qual applies to the FASTQ input that is counted: not with --query-db\n"); return 1; }
  if ((o.normalize_out || normalize_opt_set) && (!o.global || o.sparse)) { fprintf(stderr, "cfrk: --normalize-out and the --normalize- options need --global\n"); return 1; }
  if (normalize_opt_set && !o.normalize_out) { fprintf(stderr, "cfrk: the --normalize- options need --normalize-out NFILE\n"); return 1; }
  if (o.normalize_out && !normalize_cutoff_set) { fprintf(stderr, "cfrk: --normalize-out needs --normalize-cutoff C\n"); return 1; }
  if (o.normalize_out && (o.gpus > 1 || batch_n >= 0 || o.device_parse || o.query_db)) {
    fprintf(stderr, "cfrk: --normalize-out runs on one device and writes one file: not with --gpus above 1, --batch, --device-parse or --query-db\n");
    return 1;
  }
  if (o.query) g_qformat = file_format(o, o.query);
  if (o.filter_format == CFRK_TEXT_FASTQ && g_qformat != CFRK_FORMAT_FASTQ) {
    fprintf(stderr, "cfrk: --filter-format fastq needs a FASTQ --query file: %s is read as FASTA\n", o.query);
    return 1;
  }
  if (o.correct_format == CFRK_TEXT_FASTQ && g_qformat != CFRK_FORMAT_FASTQ) {
    fprintf(stderr, "cfrk: --correct-format fastq needs a FASTQ --query file: %s is read as FASTA\n", o.query);
    return 1;
  }
  if (o.query && read_reads(o.query, g_qformat, 0, 0, &g_qreads)) return 1;
  if ((o.filter_names || o.correct_names) && read_whole_file(o.query, g_qtext)) return 1;
  struct QFree { ~QFree() { for (cfrk_batch *b : {&g_qreads, &g_qreads2, &g_mreads}) if (b->data) cfrk_host_free_batch(b); } } qfree;
  if (o.unitigs_map && read_reads(o.unitigs_map, file_format(o, o.unitigs_map), 0, 0, &g_mreads)) return 1;
  if (o.query2) {
    if (file_format(o, o.query2) != g_qformat) { fprintf(stderr, "cfrk: %s and %s are not of one format\n", o.query, o.query2); return 1; }
    if (read_reads(o.query2, g_qformat, 0, 0, &g_qreads2)) return 1;
    if ((o.filter_names || o.correct_names) && read_whole_file(o.query2, g_qtext2)) return 1;
    if (g_qreads2.nS != g_qreads.nS) {
      fprintf(stderr, "cfrk: %s holds %lld records and %s holds %lld: record j of each is a pair\n", o.query, (long long)g_qreads.nS, o.query2, (long long)g_qreads2.nS);
      return 1;
    }
  }
  if (o.paired && o.query && (o.filter_out || o.correct_out) && odd_records(o.query, g_qreads.nS)) return 1;
  if (o.query_db) return run_query_db(o);
  if (pos.size() < 3) {
    // src/main.cu:239-243
    printf("Usage: ./cfrk [dataset.fasta] [file_out.cfrk] [k] <number of threads: Default 12> <chunkSize: Default 8192>");
    return 1;
  }
  o.k = atoi(pos[2]);
  if (o.sparse && (o.k < 1 || o.k > 32)) { fprintf(stderr, "cfrk: --sparse needs 1 <= k <= 32 (one-word keys), not %d\n", o.k); return 1; }
  if (o.sparse) { o.native = true; o.all_chunks = true; }   // clean parse, guarded semantics, every chunk
  if (pos.size() >= 4) o.threads = atoi(pos[3]);
  if (o.threads < 1) o.threads = 1;
  { const unsigned hw = std::thread::hardware_concurrency(); if (hw && (unsigned)o.threads > hw) o.threads = (int)hw; }
  if (pos.size() == 5) o.chunk_size = atol(pos[4]);     // argc == 6 in the reference
  if (o.chunk_size <= 0) { fprintf(stderr, "cfrk: chunkSize must be positive\n"); return 1; }
  if (o.gpus < 1) { fprintf(stderr, "cfrk: --gpus must be positive\n"); return 1; }
  if (batch_n == 0 || batch_n < -1) { fprintf(stderr, "cfrk: --batch needs a positive file count\n"); return 1; }

  // single-file mode: the parse starts now, beside the creation of the contexts
  int fmt = -1;
  if (batch_n < 0) {
    fmt = file_format(o, pos[0]);
    if (!format_allowed(o, pos[0], fmt)) return 1;
  }
  Parsed pre;
  if (batch_n < 0 && !o.device_parse) pre.start(o, pos[0], fmt);
  struct Joiner { Parsed &p; ~Joiner() { if (p.th.joinable()) { p.th.join(); if (!p.rc) cfrk_host_free_batch(&p.batch); } } } joiner{pre};   // (early returns)
  const double tc0 = now_s();                          // (runtime start-up + the contexts)
  int ndev = 0, rc;
  if ((rc = cfrk_device_count(&ndev))) return die(nullptr, rc, "cfrk_device_count");
  if (!o.same_device && o.device + o.gpus > ndev) {
    fprintf(stderr, "cfrk: --device %d --gpus %d but %d device(s) present\n", o.device, o.gpus, ndev);
    return 1;
  }
  // two contexts (streams) per device: chunk c+1 is copied in while chunk c is counted / copied out / formatted
  std::vector<std::vector<Worker>> per_dev((size_t)o.gpus);
  for (int g = 0; g < o.gpus; ++g)
    for (int s = 0; s < 2; ++s) {
      Worker w;
      w.device = o.same_device ? o.device : o.device + g;
      if ((rc = cfrk_ctx_create(w.device, nullptr, &w.ctx))) return die(nullptr, rc, "cfrk_ctx_create");
      per_dev[(size_t)g].push_back(w);
    }

  g_contexts_s = now_s() - tc0;
  int status = 0;
  if (batch_n < 0) {
    std::vector<Worker> all;
    for (int s = 0; s < 2; ++s)                       // device-major would put both streams of a device first
      for (int g = 0; g < o.gpus; ++g) all.push_back(per_dev[(size_t)g][(size_t)s]);
    status = run_file(o, pos[0], pos[1], all, &per_dev, o.device_parse ? nullptr : &pre, fmt);
  } else {
    // file i goes to device i % gpus (swift/cfrk.swf:15-20 starts one cfrk process per file)
    std::vector<int> st((size_t)o.gpus, 0);
    std::vector<std::thread> th;
    for (int g = 0; g < o.gpus; ++g)
      th.emplace_back([&, g] {
        for (int i = g; i < batch_n; i += o.gpus) {
          const std::string in = std::string(pos[0]) + "_" + std::to_string(i) + ".fasta";
          const std::string outp = std::string(pos[1]) + "_" + std::to_string(i) + ".cfrk";
          const int r = run_file(o, in.c_str(), outp.c_str(), per_dev[(size_t)g]);
          if (r && !st[(size_t)g]) st[(size_t)g] = r;
        }
      });
    for (auto &t : th) t.join();
    for (int r : st) if (r && !status) status = r;
  }
  for (auto &d : per_dev) for (auto &w : d) cfrk_ctx_destroy(w.ctx);
  return status;
}
