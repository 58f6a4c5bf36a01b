// cfrk_host.h -- host side of the cfrk drop-in: FASTA / FASTQ ingest, chunking, .cfrk output.
//
// Mirrors the reference's host code around kmer_main() (paths under /root/reference/):
//   ReadFasta / ReadFASTASequences / ProcessData   src/fastaIO.h:24-148
//   SelectChunk / SelectChunkRemain                src/main.cu:110-206
//   PrintFreq                                      src/main.cu:26-62
// Plain C ABI so that the CPU tests (ctypes) and the CLI share one implementation.
// Pure host code: no HIP, no oracle.
#ifndef CFRK_HOST_H
#define CFRK_HOST_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CFRK_INGEST_COMPAT 0x1   /* reproduce ReadFasta's quirks (see cfrk_host_read_fasta) */

typedef struct cfrk_batch {      /* struct read (src/tipos.h:23-30) with owned storage */
  int8_t  *data;                 /* nN codes, -1 = invalid base / terminator */
  int64_t *start;                /* nS */
  int32_t *length;               /* nS */
  int64_t nN, nS;
} cfrk_batch;

/* Parse a FASTA file (or memory image) into the struct-read layout.
 * CFRK_INGEST_COMPAT (what the reference does, src/fastaIO.h:24-71,105-148):
 *   - a record starts at a line BEGINNING with '>' (fastaIO.h:40);
 *   - every other line, newline included, is appended to the record (fastaIO.h:49-66), so the
 *     newlines inside a multi-line record and trailing blank lines become -1 codes;
 *   - length = strlen - 1 (fastaIO.h:53,65): the last char is dropped, which is the final
 *     newline, or the last BASE when the file has no final newline.
 * Without the flag: sequence lines are joined without their line ends ('\n', '\r'), nothing
 * is dropped.  Both: aA cC gG tT -> 0 1 2 3, anything else -1 (fastaIO.h:121-140).
 * Returns 0, -1 (cannot open), -2 (sequence before the first header), -3 (header without
 * sequence: undefined behaviour in the reference, rejected here), -4 (out of memory). */
int  cfrk_host_read_fasta(const char *path, int flags, cfrk_batch *out);
int  cfrk_host_parse_fasta(const char *buf, size_t len, int flags, cfrk_batch *out);
void cfrk_host_free_batch(cfrk_batch *b);
/* threads the parser may use for large inputs (0 = the default, min(hardware threads, 64)) */
void cfrk_host_set_parse_threads(int n);

/* Parse strict four-line FASTQ (the grammar of cfrk_fastq_parse_device, include/cfrk_abi.h: records of an '@' line, a
 * sequence line, a '+' line and a quality line; one '\r' in front of a '\n' or at the text's end dropped per line) into
 * the native struct-read layout.  min_qual 0 .. 93: with min_qual >= 1 a base whose Phred+33 quality is below it
 * becomes -1.  Threaded like the FASTA parser (cfrk_host_set_parse_threads; an explicit thread count is honoured for
 * texts of any size); the result does not depend on the thread count.
 * Returns 0, -1 (cannot open), -4 (out of memory, NULL argument), or, with the place in *where (may be NULL):
 *   CFRK_FASTQ_NO_AT     line *where (a multiple of four, counted from 0) does not begin with '@'
 *   CFRK_FASTQ_NO_PLUS   line *where does not begin with '+'
 *   CFRK_FASTQ_TRUNCATED *where lines, not a multiple of four
 *   CFRK_FASTQ_LENGTHS   record *where (from 0): sequence and quality lines differ in length
 *   CFRK_FASTQ_LONG      record *where has more than 2^31 - 1 bases
 *   CFRK_FASTQ_MIN_QUAL  min_qual outside 0 .. 93
 * in the order of the device parser: the structural fault (the first three) on the earliest line, the truncated record
 * behind every line; then the first record of differing lengths; then the first over-long one.
 * cfrk_host_fastq_message writes the one-line text of such a code ("FASTQ: ..."), in the device parser's words, and
 * returns its length (0 for a code that is none of these). */
#define CFRK_FASTQ_NO_AT (-5)
#define CFRK_FASTQ_NO_PLUS (-6)
#define CFRK_FASTQ_TRUNCATED (-7)
#define CFRK_FASTQ_LENGTHS (-8)
#define CFRK_FASTQ_LONG (-9)
#define CFRK_FASTQ_MIN_QUAL (-10)
int  cfrk_host_parse_fastq(const char *buf, size_t len, int min_qual, cfrk_batch *out, uint64_t *where);
int  cfrk_host_read_fastq(const char *path, int min_qual, cfrk_batch *out, uint64_t *where);
size_t cfrk_host_fastq_message(int rc, uint64_t where, char *buf, size_t cap);
/* the format of a text by its first byte: '@' is FASTQ, anything else, the empty text included, FASTA */
#define CFRK_FORMAT_FASTA 0
#define CFRK_FORMAT_FASTQ 1
int  cfrk_host_sniff_format(const char *buf, size_t len);

/* Chunk [first, first+count) of a batch with chunk-relative start[] (SelectChunk,
 * src/main.cu:160-206): views into the batch, nothing is copied; start_out needs count slots. */
int cfrk_host_chunk(const cfrk_batch *b, int64_t first, int64_t count, const int8_t **data,
                    int64_t *start_out, const int32_t **length, int64_t *nN);

/* PrintFreq (src/main.cu:26-62): "<idx>:<count> " for every bin, '\n' between rows, none at the
 * end.  Returns bytes needed/written (buf may be NULL to size). */
size_t cfrk_host_format_dense(const int32_t *freq, int64_t nS, int k, char *buf, size_t cap);
/* the same text, formatted by `threads` host threads (row ranges) */
size_t cfrk_host_format_dense_mt(const int32_t *freq, int64_t nS, int k, char *buf, size_t cap, int threads);
/* Sparse global form (what the commented-out `if (Freq[i] != 0)` of src/main.cu:51-56 was heading
 * for): one line per distinct key, ascending.
 *   k <= 32:  "<key>:<count>\n"            key = the 2k-bit k-mer value in decimal (as PrintFreq prints indices)
 *   k  > 32:  "<hi>:<lo>:<count>\n"        key = hi * 2^64 + lo, both words in decimal (keys_hi != NULL) */
size_t cfrk_host_format_sparse(const uint64_t *keys, const uint32_t *counts, uint64_t n, char *buf,
                               size_t cap);
size_t cfrk_host_format_sparse2(const uint64_t *keys_lo, const uint64_t *keys_hi, const uint32_t *counts,
                                uint64_t n, char *buf, size_t cap);
/* the same text, formatted by `threads` host threads (entry ranges); keys_hi may be NULL (k <= 32) */
size_t cfrk_host_format_sparse_mt(const uint64_t *keys_lo, const uint64_t *keys_hi, const uint32_t *counts,
                                  uint64_t n, char *buf, size_t cap, int threads);

/* Per-read sparse rows (cfrk_per_read_sparse: CSR row_ptr[nS+1], keys, counts) as text (`cfrk --sparse`): one line per
 * read, in read order, its "<key>:<count>" tokens separated by single spaces, ascending by key as the rows are, keys
 * in decimal; a read without a valid window gives an empty line.  Returns bytes needed / written (buf may be NULL to
 * size).  _mt: the same text, formatted by `threads` host threads (row ranges). */
size_t cfrk_host_format_sparse_rows(const int64_t *row_ptr, const uint64_t *keys, const uint32_t *counts, int64_t nS,
                                    char *buf, size_t cap);
size_t cfrk_host_format_sparse_rows_mt(const int64_t *row_ptr, const uint64_t *keys, const uint32_t *counts, int64_t nS,
                                       char *buf, size_t cap, int threads);

/* Abundance histogram (k-mer spectrum) as text: "<c>\t<n_c>\n" for every c >= 1 with n_c > 0, ascending in c (the shape
 * of `jellyfish histo`).  n_c = hist[c] for c < nbins (hist[0] is ignored; hist may be NULL with nbins 0) plus the keys of
 * tail_counts (one count per key, any order; those below nbins are added to their bin).  Returns bytes needed /
 * written (buf may be NULL to size). */
size_t cfrk_host_format_histo(const uint64_t *hist, uint64_t nbins, const uint32_t *tail_counts, uint64_t n_tail,
                              char *buf, size_t cap);

/* Read-query answers as text (`cfrk --query`): one line per read i, the counts of its windows
 * counts[start[i]], .. counts[start[i] + length[i] - k] separated by single spaces, "-" for 0xFFFFFFFF (CFRK_QUERY_NONE:
 * the window holds an invalid base); a read shorter than k gives an empty line.  Returns bytes needed / written (buf
 * may be NULL to size). */
size_t cfrk_host_format_query(const uint32_t *counts, const int64_t *start, const int32_t *length, int64_t nS, int k,
                              char *buf, size_t cap);

/* Per-read abundance statistics as text (`cfrk --query-stats`): stats = nS rows of cfrk_read_stats (cfrk_abi.h: 32
 * bytes -- windows, present, below, min, median, max as uint32, sum as uint64).  One line per record, in record order,
 * the seven fields in struct order, in decimal, separated by tabs.  Returns bytes needed / written (buf may be NULL to
 * size). */
size_t cfrk_host_format_read_stats(const void *stats, int64_t nS, char *buf, size_t cap);

/* Selected reads as FASTA text (`cfrk --filter-out`): one record per read j, ">" + index[j] in decimal (the input
 * record number: the parsers keep no names; index NULL numbers the reads 0, 1, ..) + "\n" + the bases
 * data[start[j]] .. data[start[j] + length[j] - 1] as ACGT, N for any other code, on one line + "\n" (an empty read
 * gives an empty line).  Returns bytes needed / written (buf may be NULL to size). */
size_t cfrk_host_format_fasta(const int8_t *data, const int64_t *start, const int32_t *length, const int64_t *index,
                              int64_t nS, char *buf, size_t cap);

/* Unitigs as FASTA text (`cfrk --unitigs-out`): rec = nS rows of cfrk_unitig (cfrk_abi.h: 16 bytes -- kc as uint64,
 * n_kmers and flags as uint32).  One record per unitig j, in order:
 *   ">" j " LN:i:" length[j] " KC:i:" kc " km:f:" kc / n_kmers with one decimal (halves rounded up)
 *   and " CL:i:1" when flags has CFRK_UNITIG_CIRCULAR, "\n", then the bases as ACGT (N for any other code) on ONE line.
 * (The tags are BCALM's.)  One thread: the text is a few bytes per base of a compacted graph.  Returns bytes needed /
 * written (buf may be NULL to size). */
size_t cfrk_host_format_unitigs(const int8_t *data, const int64_t *start, const int32_t *length, const void *rec, int64_t nS,
                                char *buf, size_t cap);

/* The same FASTA with BCALM's L tags (`cfrk --unitigs-out UFILE --unitigs-links`): link_ptr = nS + 1 offsets, links =
 * rows of cfrk_unitig_link (cfrk_abi.h: 8 bytes -- to and flags as uint32; flags bit 0: the link leaves (j,-), bit 1: it
 * enters (to,-)).  For every link of row j, in row order, " L:<+|->:<to>:<+|->" is appended at the very end of the
 * header, behind " CL:i:1" where that is present.  Returns bytes needed / written (buf may be NULL to size). */
size_t cfrk_host_format_unitigs_links(const int8_t *data, const int64_t *start, const int32_t *length, const void *rec,
                                      int64_t nS, const int64_t *link_ptr, const void *links, char *buf, size_t cap);

/* The graph as GFA 1.0 (`cfrk --unitigs-gfa GFILE`): "H\tVN:Z:1.0\n"; one "S\t<j>\t<SEQ>\tLN:i:<len>\tKC:i:<kc>\tkm:f:<x.y>\n"
 * per unitig (the mean as in the FASTA header, N for any code outside 0..3); then one
 * "L\t<u>\t<+|->\t<v>\t<+|->\t<k-1>M\n" per link, in CSR order.  Returns bytes needed / written (buf may be NULL to
 * size). */
size_t cfrk_host_format_gfa(const int8_t *data, const int64_t *start, const int32_t *length, const void *rec, int64_t nS,
                            const int64_t *link_ptr, const void *links, int k, char *buf, size_t cap);

/* Popped bubbles as text (`cfrk --bubble-report BFILE`): the unitig list of one round (rec = nS rows of cfrk_unitig) with
 * pop[nS] and partner[nS] as cfrk_global_unitig_bubbles wrote them (partner = s << 1 | p).  One line per unitig j with
 * pop[j] != 0, in order, eleven fields separated by tabs:
 *   <round> <j> <s> <'+' or '-': the kept unitig's strand relative to the popped one> <LN_j> <LN_s> <km_j> <km_s> <kind>
 *   <the popped sequence> <the kept sequence, oriented like the popped one: reverse-complemented when p is set>
 * km is kc / n_kmers with one decimal as in the S line; the names are the S names of cfrk_host_format_gfa for that
 * round's list.  kind: "snp" -- equal lengths, Hamming distance 1; "mnp" -- equal lengths, any other distance;
 * "indel" -- the lengths differ.  A code outside 0..3 prints as N and equals only another such code.  A popped unitig
 * whose partner names no unitig of the list gives no line.  Returns bytes needed / written (buf may be NULL to size). */
size_t cfrk_host_format_bubbles(uint32_t round, const int8_t *data, const int64_t *start, const int32_t *length, const void *rec,
                                int64_t nS, const uint8_t *pop, const uint32_t *partner, char *buf, size_t cap);

/* Popped bulges as text (`cfrk --bulge-report FILE`): the unitig list of one round with pop[nS], path_ptr[nS + 1] and path
 * as cfrk_global_unitig_bulges wrote them (a path entry = w << 1 | o).  One line per unitig j with pop[j] != 0 and a row
 * that is not empty, in order, ten fields separated by tabs:
 *   <round> <j> <LN_j> <km_j> <hops> <the path's k-mers: the sum of its unitigs' n_kmers> <the path in GAF segment
 *   notation, '>' w for (w,+) and '<' w for (w,-), as in ">3<7>9"> <kind> <the popped sequence> <the path's sequence>
 * The path's sequence is spelled from s to t, so it is oriented like the popped unitig: the first unitig whole, of every
 * further one what follows its first k - 1 bases, a unitig entered as (w,-) reverse-complemented.  km, the names and
 * kind (the popped sequence against the path's) are those of cfrk_host_format_bubbles.  A row with an entry that names
 * no unitig of the list gives no line.  Returns bytes needed / written (buf may be NULL to size). */
size_t cfrk_host_format_bulges(uint32_t round, const int8_t *data, const int64_t *start, const int32_t *length, const void *rec,
                               int64_t nS, const uint8_t *pop, const int64_t *path_ptr, const uint32_t *path, int k, char *buf, size_t cap);

/* Dropped weak unitigs as text (`cfrk --weak-report FILE`): the unitig list of one round with weak[nS] as
 * cfrk_global_unitig_weak wrote it.  One line per unitig j with weak[j] = 1 (CFRK_WEAK_CONNECTION) or 2
 * (CFRK_WEAK_ISOLATED), in order, seven fields separated by tabs:
 *   <round> <j> <"connection" or "isolated"> <LN_j> <KC_j> <km_j> <the sequence>
 * LN, KC and km are those of the S line of cfrk_host_format_gfa for that round's list (km = kc / n_kmers with one decimal);
 * a code outside 0..3 prints as N.  Any other byte of weak gives no line.  Returns bytes needed / written (buf may be
 * NULL to size). */
size_t cfrk_host_format_weak(uint32_t round, const int8_t *data, const int64_t *start, const int32_t *length, const void *rec,
                             int64_t nS, const uint8_t *weak, char *buf, size_t cap);

/* The component table as text (`cfrk --unitigs-components CFILE`): table = n_comps rows of cfrk_unitig_component
 * (cfrk_abi.h: 32 bytes -- kc, n_kmers, n_links as uint64, first, n_unitigs as uint32) as cfrk_global_unitig_components
 * wrote them.  One line per component in id order, eight fields separated by tabs:
 *   <id> <first> <n_unitigs> <n_kmers> <bases> <kc> <mean> <n_links>
 * bases = n_kmers + n_unitigs (k - 1), the bases of the members' sequences; mean = kc / n_kmers with one decimal, printed
 * as the km:f: tag of the S line prints it (n_kmers 0 divides by 1).  Returns bytes needed / written (buf may be NULL to
 * size). */
size_t cfrk_host_format_components(const void *table, int64_t n_comps, int k, char *buf, size_t cap);

/* The component of every unitig as a tag in a text that is already formatted (`cfrk --unitigs-component-tags`): text =
 * n bytes as cfrk_host_format_unitigs / _unitigs_links wrote them (gfa = 0) or as cfrk_host_format_gfa / _gfa_support did
 * (gfa = 1), comp = nS words as cfrk_global_unitig_components wrote them.  The j-th header line (it begins with '>')
 * gets " CC:i:<comp[j]>" behind its km:f: (and CL:i:1) tag, in front of its first " L:" tag; the j-th S line gets
 * "\tCC:i:<comp[j]>" as its last tag.  Every other byte is copied.  A unitig with comp[j] = 0xFFFFFFFF, and a line
 * beyond nS, gets no tag.  Returns bytes needed / written (buf may be NULL to size). */
size_t cfrk_host_tag_components(const char *text, size_t n, int gfa, const uint32_t *comp, int64_t nS, char *buf, size_t cap);

/* Read hits as GAF (`cfrk --unitigs-map QFILE --unitigs-map-out MFILE`): hit_ptr = n_reads + 1 offsets, hits = rows of
 * cfrk_read_hit (cfrk_abi.h: 16 bytes -- unitig, unitig_at = off << 1 | minus, read_off, n_windows as uint32),
 * unitig_length = the unitig list's lengths (every hit's unitig is an index into it).  One line per hit, in CSR order,
 * with m = n_windows + k - 1:
 *   "<read i, 0-based>\t<read_length[i]>\t<read_off>\t<read_off+m>\t+\t<'>' or '<'><j>\t<LN_j>\t<ps>\t<pe>\t<m>\t<m>\t255\tcg:Z:<m>=\n"
 * '>' (minus clear): ps = off.  '<' (minus set), coordinates on the reverse-complemented unitig: ps = LN_j - off - m.
 * pe = ps + m.  The segment names are the S names of cfrk_host_format_gfa.  Returns bytes needed / written (buf may be
 * NULL to size). */
size_t cfrk_host_format_gaf(const int32_t *read_length, int64_t n_reads, const int64_t *hit_ptr, const void *hits,
                            const int32_t *unitig_length, int k, char *buf, size_t cap);

/* Read paths as GAF (`cfrk --unitigs-map QFILE --unitigs-map-out MFILE --unitigs-map-paths`): the arguments of
 * cfrk_host_format_gaf and path_ptr = n_reads + 1 offsets, paths = rows of cfrk_read_path (cfrk_abi.h: 16 bytes --
 * hit_first inside the read's hit row, n_hits, read_off, n_windows as uint32) as cfrk_global_read_paths wrote them.  One
 * line per path, in CSR order, with m = n_windows + k - 1:
 *   "<read i>\t<read_length[i]>\t<read_off>\t<read_off+m>\t+\t<path>\t<PL>\t<ps>\t<ps+m>\t<m>\t<m>\t255\tcg:Z:<m>=\n"
 * <path> is its hits' segments in GAF notation as cfrk_host_format_bulges spells them (">3<7>9"); PL is the sum of the
 * segments' LN minus (n_hits - 1)(k - 1); ps is the first hit's ps as cfrk_host_format_gaf defines it.  A path of one hit
 * gives exactly the line cfrk_host_format_gaf gives for that hit.  Returns bytes needed / written (buf may be NULL to
 * size). */
size_t cfrk_host_format_gaf_paths(const int32_t *read_length, int64_t n_reads, const int64_t *hit_ptr, const void *hits,
                                  const int64_t *path_ptr, const void *paths, const int32_t *unitig_length, int k, char *buf, size_t cap);

/* The GFA of cfrk_host_format_gfa with the reads that walk every link (`cfrk --unitigs-gfa GFILE --unitigs-map QFILE
 * --unitigs-link-support`): the same text with "\tRC:i:<c>" appended to every L line; support = n_links counters as
 * cfrk_global_read_paths left them (must not be NULL).  Not canonical, or the link is its own mirror: c = support[r].
 * Canonical: c = support[r] + support[r'] where r' is the mirror row (v,!ov) -> (u,!ou) of r = (u,ou) -> (v,ov), when
 * that row exists and is another row; a read and its reverse complement then tag the same two lines alike.  The one
 * exception: at even k, rows into or out of a palindromic single-node unitig keep per-strand numbers, because its hits
 * are always '+': a read and its reverse complement enter it through different rows that are not each other's mirror.
 * Returns bytes needed / written (buf may be NULL to size). */
size_t cfrk_host_format_gfa_support(const int8_t *data, const int64_t *start, const int32_t *length, const void *rec, int64_t nS,
                                    const int64_t *link_ptr, const void *links, const uint32_t *support, int canonical, int k,
                                    char *buf, size_t cap);

/* Binary global form, little endian, everything in one file:
 *   header, 32 bytes:  char magic[8] = "CFRKGLB1"; uint32 k; uint32 flags (bit 0: canonical counting,
 *                      bit 1: two-word keys, i.e. k > 32); uint64 n (records); uint64 sum of counts
 *   n records, ascending by key:   k <= 32: { uint64 key; uint32 count }            12 bytes, packed
 *                                   k  > 32: { uint64 hi; uint64 lo; uint32 count }  20 bytes, packed
 * (12 / 20 bytes are the slot sizes S of the algorithmic-byte budget)
 * write: returns bytes needed / written (buf may be NULL to size); keys_hi may be NULL for k <= 32.
 * read:  parses a whole image; on success (0) *k, *flags, *n are set and, when the arrays are not NULL,
 *        n entries are stored (keys_hi gets zeros for k <= 32).  -1: not a CFRKGLB1 image or truncated. */
#define CFRK_BIN_CANONICAL 0x1
#define CFRK_BIN_TWO_WORD 0x2
size_t cfrk_host_write_binary(int k, int flags, const uint64_t *keys_lo, const uint64_t *keys_hi,
                              const uint32_t *counts, uint64_t n, char *buf, size_t cap);
int cfrk_host_read_binary(const char *buf, size_t len, int *k, int *flags, uint64_t *n, uint64_t *keys_lo,
                          uint64_t *keys_hi, uint32_t *counts);

#ifdef __cplusplus
}
#endif
#endif
