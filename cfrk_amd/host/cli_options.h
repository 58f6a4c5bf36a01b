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
//   --unitigs-map-paths  (with --unitigs-map) MFILE gets one line per PATH, not per hit: a read's consecutive hits that
//                    leave one oriented unitig at its end and enter the next at its head one window later, across a
//                    link of the graph that is written, are one walk, spelled >3<7>9 (cfrk_global_read_paths,
//                    cfrk_host_format_gaf_paths).  A path of one hit is the line it was
//   --unitigs-link-support  (with --unitigs-map and --unitigs-gfa) every L line of GFILE gets "\tRC:i:<c>": the reads of
//                    QFILE that walk across the link, in a --canonical run together with those that walk across its
//                    mirror (cfrk_host_format_gfa_support)
//   --unitigs-map-stats SFILE  (with --unitigs-map) one line of six tab-separated numbers: reads, hits, paths, steps
//                    (joined pairs of hits), gaps (pairs that are not window-adjacent) and unlinked (adjacent pairs
//                    without a link: 0 on the graph's own complete links).  All three act on the graph that is
//                    written, after any tip, bubble or bulge loop; without them every byte written is what it was
//   --unitigs-components CFILE  (with --unitigs-out) the connected components of the graph that is written, after any
//                    loop (cfrk_global_unitig_components, cfrk_host_format_components): one line per component in id
//                    order, ids ascending by the component's smallest unitig, eight tab-separated fields -- id, first
//                    (that unitig), n_unitigs, n_kmers, bases = n_kmers + n_unitigs (k - 1), kc, mean = kc / n_kmers as
//                    the km:f: tag prints it, n_links (the members' links as the rows hold them, mirrors included)
//   --unitigs-component-tags  (with --unitigs-out) every header of UFILE gets " CC:i:<id>", the unitig's component, behind
//                    its km:f: (and CL:i:1) tag and in front of any L: tag, and every S line of GFILE "\tCC:i:<id>" as
//                    its last tag (cfrk_host_tag_components)
//   --unitigs-min-component-kmers N  (with --unitigs-out) after the loop (or with none) every component of fewer than N
//                    k-mers is dropped as a whole: unitigs, links, components, one mask of all their unitigs.  Whole
//                    components go, so no remaining unitig gains or loses a neighbour: UFILE, the L tags, GFILE, MFILE,
//                    CFILE and RFILE describe exactly the unitigs that are left, renumbered
//   --unitigs-map-components RFILE  (with --unitigs-out and --unitigs-map) which read of QFILE goes with which component
//                    (cfrk_global_read_components): one line per read, four tab-separated fields -- id, hit, n_windows,
//                    flags: the component of the read's hit with the most windows (the earliest on a tie), that hit's
//                    index among the read's hits, its windows, and 1 when another hit of the read lies in a different
//                    component.  A read with no hit gets "*\t*\t0\t0"
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
//   --unitigs-pop-bulges [--bulge-max-kmers M] [--bulge-max-diff D] [--bulge-max-hops H] [--bulge-max-visits V]
//                    [--bulge-ratio R] [--bulge-report FILE] [--simplify-rounds N]  (with --unitigs-out, --unitigs-gfa or
//                    --unitigs-map) pop arms that run beside a CHAIN of unitigs, in the same loop as --unitigs-clip-tips
//                    and --unitigs-pop-bubbles and combined with either: every enabled rule sees the same graph of a
//                    round, one mask takes the k-mers of all of them.  A popped arm has at most M k-mers (default k),
//                    one link in and one out, and beside it a path of at most H unitigs (default min(M + D, 64), at
//                    most 64) between the same two ends, each of at least R times its mean coverage (default 0) and
//                    ranking above it, whose k-mers sum to the arm's within D (default 0).  The depth-first search
//                    looks at V links at most (default 1024, at most 65536: a choice with headroom, not a measured
//                    optimum); an arm it cannot decide within V stays.  --tip-report lines get six fields,
//                    "round<TAB>unitigs<TAB>tips<TAB>bubbles<TAB>bulges<TAB>masked k-mers so far".  FILE: one line per
//                    popped unitig (cfrk_host_format_bulges: round, S name, LN, km, hops, the path's k-mers, the path
//                    as >3<7>9, snp / mnp / indel, both sequences)  (cfrk_global_unitig_bulges)
//   --unitigs-drop-weak [--weak-max-kmers M] [--weak-ratio R] [--weak-iso-max-kmers I] [--weak-iso-mean A]
//                    [--weak-report FILE] [--simplify-rounds N]  (with --unitigs-out, --unitigs-gfa or --unitigs-map) drop
//                    erroneous connections and isolated low-coverage unitigs, in the same loop as the three rules above
//                    and combined with any of them: every enabled rule sees the same graph of a round, one mask takes
//                    the k-mers of all of them, the first round in which no enabled rule finds anything ends the loop.
//                    A connection has at most M k-mers (default k), links at both ends and none to itself, and at EVERY
//                    one of those links a sibling -- another way out of the same neighbour's end -- of at least R times
//                    its mean coverage (default 4.0, 0 .. 256) that ranks above it.  At an equal ratio that contains
//                    everything --unitigs-pop-bubbles pops, hence the high default.  An isolated unitig has no link at
//                    all, at most I k-mers (default 2 k; 0: none) and a mean coverage below A (default 2.0, 0 .. 256;
//                    0: none).  All four defaults are choices, not measured optima.  --tip-rounds is refused here:
//                    --simplify-rounds sets the rounds.  --tip-report lines get two further fields at their end,
//                    "...<TAB>connections<TAB>isolated".  FILE: one line per dropped unitig (cfrk_host_format_weak: round,
//                    S name, connection / isolated, LN, KC, km, the sequence)  (cfrk_global_unitig_weak)
//   --simplify-recompact  (with --unitigs-clip-tips, --unitigs-pop-bubbles, --unitigs-pop-bulges or --unitigs-drop-weak) between two rounds of
//                    the loop, take the next round's unitigs from the last round's graph and what it dropped
//                    (cfrk_global_unitigs_compact) and not from the k-mer passes of cfrk_global_unitigs.  Every file
//                    written is byte for byte the same either way.
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
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/cfrk_abi.h"

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
  bool map_paths = false;             // --unitigs-map-paths
  bool link_support = false;          // --unitigs-link-support
  const char *map_stats = nullptr;    // --unitigs-map-stats SFILE
  const char *unitigs_components = nullptr;      // --unitigs-components CFILE
  const char *map_components = nullptr;          // --unitigs-map-components RFILE
  bool component_tags = false;                   // --unitigs-component-tags
  uint32_t min_component_kmers = 0;              // --unitigs-min-component-kmers N (0: nothing is dropped)
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
  bool pop_bulges = false;            // --unitigs-pop-bulges
  bool simplify_recompact = false;    // --simplify-recompact
  uint32_t bulge_max_kmers = 0;       // --bulge-max-kmers M (0: k)
  uint32_t bulge_max_diff = 0;        // --bulge-max-diff D
  uint32_t bulge_max_hops = 0;        // --bulge-max-hops H (0: min(M + D, 64))
  uint32_t bulge_max_visits = 1024;   // --bulge-max-visits V
  uint32_t bulge_ratio_q8 = 0;        // --bulge-ratio R, in 256ths
  const char *bulge_report = nullptr; // --bulge-report FILE
  bool drop_weak = false;             // --unitigs-drop-weak
  uint32_t weak_max_kmers = 0;        // --weak-max-kmers M (0: k)
  uint32_t weak_ratio_q8 = 1024;      // --weak-ratio R, in 256ths
  uint32_t weak_iso_max_kmers = 0;    // --weak-iso-max-kmers I (without weak_iso_max_set: 2 k)
  uint32_t weak_iso_mean_q8 = 512;    // --weak-iso-mean A, in 256ths
  const char *weak_report = nullptr;  // --weak-report FILE
  bool histo_only = false;
  uint32_t min_count = 1, max_count = CFRK_COUNT_MAX;
  const char *query = nullptr, *query_out = nullptr, *query_db = nullptr;   // --query QFILE --query-out OFILE --query-db DB
  bool query_only = false;
  const char *query_stats = nullptr;   // --query-stats SFILE
  uint32_t stats_below = 0;            // --stats-below T
  const char *filter_out = nullptr;    // --filter-out FFILE
  uint32_t filter_min_count = 2, filter_max_count = CFRK_COUNT_MAX;   // --filter-min-count T, --filter-max-count U
  int filter_trim = CFRK_SPAN_LONGEST; // --filter-trim: CFRK_SPAN_LONGEST / CFRK_SPAN_PREFIX, -1 = none
  long long filter_min_len = -1;       // --filter-min-len L (-1: k)
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
  int text_copy_plain = 1;                                          // --text-copy plain (the default, 1) | staged (0)
  int format = -1;                                                  // --format: CFRK_FORMAT_FASTA / _FASTQ, -1 = by the first byte
  long long min_qual = 0;                                           // --min-qual
  bool paired = false;                                              // --paired
  int pair_check = 1;                                               // --pair-check on (1) | off (0)
  int pair_mode = CFRK_PAIR_EITHER;                                 // --pair-mode (the normalise call's; the filter joins by CFRK_PAIR_BOTH)
  const char *query2 = nullptr, *filter_out2 = nullptr, *filter_orphans = nullptr, *correct_out2 = nullptr;
  bool mates() const { return paired || query2; }
  int parse_threads = 0;                                            // --parse-threads N (handed to cfrk_host_set_parse_threads as it is read)
  int batch_n = -1;                                                 // --batch N (-1: not given)
  std::vector<const char *> pos;                                    // the positional arguments, in order
  // raised by the options that were given: what the cross-option rules ask about
  bool unitigs_opt_set = false, tip_opt_set = false, tip_rounds_set = false, bubble_opt_set = false, simplify_rounds_set = false, bulge_opt_set = false, weak_opt_set = false, weak_iso_max_set = false, component_opt_set = false, range_set = false, stats_below_set = false;
  bool filter_opt_set = false, correct_opt_set = false, correct_min_count_set = false, normalize_opt_set = false, normalize_cutoff_set = false;
  bool pair_opt_set = false, pair_mode_set = false, min_qual_set = false;
};

// Every function here returns 0, or 1 with the refusal on stderr.
// argv into o, one row of the option table (cli_options.cpp) per option; values are checked in argv order.  An argument
// that is no option is a positional, whatever it looks like
int parse_options(int argc, char **argv, Options &o);
// the rules between options, in a fixed order: the first one broken is the one reported.  Reads o alone
int check_options(const Options &o);
// k, threads and chunkSize from the positionals; --sparse's implications; --gpus and --batch in range
int apply_positionals(Options &o);
// the spelling of the i-th row of the option table and whether it takes a value; NULL behind the last row (for the checker in tools/)
const char *option_at(size_t i, bool *takes_value);
