"""ctypes binding of libcfrk_hip.so and the host-side mirror of the reference interface.

Reference interface mirrored here (paths under /root/reference/):
  struct read { char *data; int *length; lint *start; int *Freq; }      src/tipos.h:23-30
  void kmer_main(struct read *rd, lint nN, lint nS, int k, ushort device) src/kmer_main.cu:20
"""
import ctypes as C
import os
import re

import numpy as np

CFRK_COMPAT = 0x1
CFRK_CANONICAL = 0x2
CFRK_FORCE_HASH = 0x4
CFRK_RUNS_ONLY = 0x8
CFRK_FLOAT_INDEX = 0x10
CFRK_RUNS_DEFER = 0x20
CFRK_DEBUG_FORCE_RT_OVERFLOW = 0x1   # cfrk_debug_set_flags
CFRK_DEBUG_SMALL_WAVE_CAP = 0x2
CFRK_DEBUG_NO_ANCHORS = 0x4
CFRK_DEBUG_RECORD_SUBSETS = 0x8
CFRK_DEBUG_NO_PIPELINE = 0x10
CFRK_DEBUG_SMALL_PIPELINE = 0x20
CFRK_DEBUG_NO_RADIX16 = 0x40
CFRK_DEBUG_NO_SMALL_LEAVES = 0x80
CFRK_ERR_COUNT_OVERFLOW = -10        # finish / digest / export: some count was held at CFRK_COUNT_MAX
CFRK_ERR_RUNS_REFUSED = -11          # a CFRK_RUNS_ONLY add that needs more than one pass
CFRK_COUNT_MAX = 0xFFFFFFFE
CFRK_QUERY_NONE = 0xFFFFFFFF         # read query: the window holds an invalid base or runs past nN
CFRK_ERR_SMALL_BUF = -9
CFRK_SPARSE_FAST_WINDOWS = 2048      # per-read sparse: windows per read the LDS path holds (longer reads: slower, exact)
CFRK_STATS_FAST_WINDOWS = 2048       # read stats: windows per read a lane group holds (longer reads: slower, exact)
# cfrk_read_stats: one row per read of GlobalCounter.read_stats()
READ_STATS_DTYPE = np.dtype([("windows", "<u4"), ("present", "<u4"), ("below", "<u4"), ("min", "<u4"),
                             ("median", "<u4"), ("max", "<u4"), ("sum", "<u8")])
CFRK_SPAN_PREFIX = 0                 # read spans: the solid run that begins at window 0 (the filter-abund rule)
CFRK_SPAN_LONGEST = 1                # the longest solid run, the earliest one on a tie
CFRK_SPANS_FAST_WINDOWS = 2048       # read spans: windows per read a lane group takes (longer reads: a workgroup each)
CFRK_NORMALIZE_BATCH = 262144        # normalise: reads per round when the caller names no batch
# cfrk_read_span: bases [offset, offset + length) of a read
READ_SPAN_DTYPE = np.dtype([("offset", "<i4"), ("length", "<i4")])
# cfrk_read_fix: weak runs of a read that were corrected / left alone
READ_FIX_DTYPE = np.dtype([("fixed", "<u4"), ("left", "<u4")])
CFRK_SELECT_TILE_BYTES = 16384       # select: bytes of data_out per workgroup of the copy
CFRK_SELECT_TILE_READS = 256         # reads per workgroup of its per-read passes
CFRK_SELECT_SCAN_TILES = 1024        # tiles of reads per block of its tile scan
CFRK_TEXT_FASTA = 0                  # text index / emitter: the format of a text
CFRK_TEXT_FASTQ = 1
CFRK_TEXT_TILE_BYTES = 16384         # text index: text bytes per workgroup
CFRK_TEXT_SCAN_TILES = 1024          # tiles per block of its tile scan
CFRK_EMIT_TILE_BYTES = 16384         # text emitter: bytes of output per workgroup of the copy
# cfrk_text_record: where a record's header line and quality line lie in its text
TEXT_RECORD_DTYPE = np.dtype([("head_off", "<i8"), ("qual_off", "<i8"), ("head_len", "<i4"), ("qual_len", "<i4")])
CFRK_PAIR_BOTH = 0                   # paired reads: a pair is kept iff both mates survive, a lone survivor is an orphan
CFRK_PAIR_EITHER = 1                 # a pair is kept iff either mate survives (khmer's --paired rule); no orphans
CFRK_PAIR_NAME_FAST = 256            # mate-name check: bytes of a name a 16-lane group takes (longer: a workgroup)
# cfrk_pair_counts, 32 bytes
PAIR_COUNTS_DTYPE = np.dtype([("pairs", "<i8"), ("orphans_a", "<i8"), ("orphans_b", "<i8"), ("dropped", "<i8")])
CFRK_SKETCH_LOG2M = 14               # distinct sketch: log2 of its registers
CFRK_SKETCH_REGS = 16384             # one uint8 register per bucket
CFRK_FASTA_TILE_BYTES = 16384        # device FASTA parser: text bytes per workgroup
CFRK_FASTA_SCAN_TILES = 1024         # tiles per block of its tile scan
CFRK_FASTA_MAX_CR_RUN = 4096         # native mode: carriage returns in a row it follows to the line's end
CFRK_FASTQ_TILE_BYTES = 16384        # device FASTQ parser: text bytes per workgroup
CFRK_FASTQ_SCAN_TILES = 1024         # tiles per block of its tile scan
CFRK_FASTQ_QUAL_BASE = 33            # qualities are Phred+33
CFRK_FASTQ_MAX_QUAL = 93             # min_qual is 0 .. this
CFRK_PARAM_MSP_CHUNKS, CFRK_PARAM_L2_SLACK_COMPLETE, CFRK_PARAM_L2_SLACK_TRUNCATED, CFRK_PARAM_MSP2_SUBVALUE_BITS = 0, 1, 2, 3   # cfrk_debug_set_param
CFRK_PARAM_UNITIG_SPLIT_LOG2 = 4     # s + 1: log2 of the unitig call's splitter period, plus one (0: the default)
CFRK_UNITIG_CIRCULAR = 0x1           # cfrk_unitig.flags
CFRK_UNITIG_SPLIT_LOG2_DEFAULT = 10
# one row per unitig (cfrk_unitig)
UNITIG_DTYPE = np.dtype([("kc", "<u8"), ("n_kmers", "<u4"), ("flags", "<u4")])
CFRK_LINK_FROM_MINUS = 0x1           # cfrk_unitig_link.flags: the link leaves (j,-)
CFRK_LINK_TO_MINUS = 0x2             # it enters (to,-)
# one row per link (cfrk_unitig_link)
UNITIG_LINK_DTYPE = np.dtype([("to", "<u4"), ("flags", "<u4")])
CFRK_POS_NONE = 0xFFFFFFFF           # both words of the position of a k-mer that lies on no unitig
# where a k-mer lies (cfrk_unitig_pos): at = p << 1 | minus
UNITIG_POS_DTYPE = np.dtype([("unitig", "<u4"), ("at", "<u4")])
# one row per hit of a read (cfrk_read_hit): unitig_at = off << 1 | minus
READ_HIT_DTYPE = np.dtype([("unitig", "<u4"), ("unitig_at", "<u4"), ("read_off", "<u4"), ("n_windows", "<u4")])
CFRK_TIP_RATIO_Q8_MAX = 65536        # tip rule: the largest ratio_q8 (256 = the sibling's mean coverage at least the tip's)
CFRK_BUBBLE_NONE = 0xFFFFFFFF        # bubble rule: the partner of a unitig that is not popped
CFRK_BULGE_MAX_HOPS = 64             # bulge rule: the longest path, in unitigs
CFRK_BULGE_MAX_VISITS = 65536        # the largest search budget, in links looked at
# what one bulge call found (cfrk_bulge_stats)
BULGE_STATS_DTYPE = np.dtype([("arms", "<i8"), ("popped", "<i8"), ("undecided", "<i8")])
CFRK_WEAK_CONNECTION = 1             # weak rule: weak[j] of an erroneous connection
CFRK_WEAK_ISOLATED = 2               # ... and of an isolated low-coverage unitig
# what one weak call found (cfrk_weak_stats)
WEAK_STATS_DTYPE = np.dtype([("connections", "<i8"), ("isolated", "<i8"), ("candidates", "<i8")])
CFRK_COMP_NONE = 0xFFFFFFFF          # unitig components: comp[j] of a dropped unitig
# cfrk_unitig_component / cfrk_component_stats: a row of the component table; what one components call counted
UNITIG_COMPONENT_DTYPE = np.dtype([("kc", "<u8"), ("n_kmers", "<u8"), ("n_links", "<u8"), ("first", "<u4"), ("n_unitigs", "<u4")])
COMPONENT_STATS_DTYPE = np.dtype([("n_components", "<u8"), ("n_unitigs", "<u8"), ("n_kmers", "<u8"), ("n_links", "<u8")])
CFRK_READ_COMP_SPLIT = 1             # read components: another eligible hit lies in a different component
CFRK_READ_COMP_DROPPED = 2           # ... some hit lies on a unitig without a component
READ_COMPONENT_DTYPE = np.dtype([("comp", "<u4"), ("hit", "<u4"), ("n_windows", "<u4"), ("flags", "<u4")])
READ_COMPONENT_STATS_DTYPE = np.dtype([("n_assigned", "<u8"), ("n_unassigned", "<u8"), ("n_split", "<u8"), ("n_dropped", "<u8")])
CFRK_COMPACT_TILE_BYTES = 4096      # unitig compaction: bytes of data_out per workgroup of the emit
# cfrk_read_path / cfrk_path_stats: a read's walk through the graph as a range of its hits; what a read_paths call counted
READ_PATH_DTYPE = np.dtype([("hit_first", "<u4"), ("n_hits", "<u4"), ("read_off", "<u4"), ("n_windows", "<u4")])
PATH_STATS_DTYPE = np.dtype([("n_paths", "<u8"), ("n_steps", "<u8"), ("n_gaps", "<u8"), ("n_unlinked", "<u8")])

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libcfrk_hip.so")
_HEADER = os.path.join(os.path.dirname(_HERE), "include", "cfrk_abi.h")

_lib = None


class CfrkError(RuntimeError):
    def __init__(self, code, what, detail=""):
        self.code = code
        super().__init__(f"{what}: {detail}" if detail else what)


def library_path():
    return _SO


def abi_symbols():
    """every function include/cfrk_abi.h declares"""
    text = open(_HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cfrk_[a-z0-9_]+)\s*\(", text)))


def load_library():
    """dlopen libcfrk_hip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise CfrkError(-100, "libcfrk_hip.so is missing",
                        "build it with `make -C cfrk_amd/csrc` or __graft_entry__.build(); "
                        "there is no CPU fallback")
    L = C.CDLL(_SO)
    vp, i64, i32, u64 = C.c_void_p, C.c_int64, C.c_int, C.c_uint64
    sig = {
        "cfrk_abi_version": ([], C.c_int),
        "cfrk_strerror": ([C.c_int], C.c_char_p),
        "cfrk_last_error": ([vp], C.c_char_p),
        "cfrk_device_count": ([C.POINTER(C.c_int)], C.c_int),
        "cfrk_ctx_create": ([C.c_int, vp, C.POINTER(vp)], C.c_int),
        "cfrk_ctx_destroy": ([vp], None),
        "cfrk_ctx_sync": ([vp], C.c_int),
        "cfrk_device_alloc": ([vp, C.c_size_t, C.POINTER(vp)], C.c_int),
        "cfrk_device_free": ([vp, vp], C.c_int),
        "cfrk_memcpy_h2d": ([vp, vp, vp, C.c_size_t], C.c_int),
        "cfrk_memcpy_d2h": ([vp, vp, vp, C.c_size_t], C.c_int),
        "cfrk_memcpy_h2d_staged": ([vp, vp, vp, C.c_size_t], C.c_int),
        "cfrk_memcpy_peer": ([vp, vp, vp, vp, C.c_size_t], C.c_int),
        "cfrk_per_read_dense": ([vp, vp, vp, vp, i64, i64, i32, i32, vp], C.c_int),
        "cfrk_per_read_dense_device": ([vp, vp, vp, vp, i64, i64, i32, i32, vp], C.c_int),
        "cfrk_per_read_sparse": ([vp, vp, vp, vp, i64, i64, i32, i32, vp, vp, vp, u64, C.POINTER(u64)], C.c_int),
        "cfrk_per_read_sparse_device": ([vp, vp, vp, vp, i64, i64, i32, i32, vp, vp, vp, u64, C.POINTER(u64)], C.c_int),
        "cfrk_global_begin": ([vp, i32, i32, u64], C.c_int),
        "cfrk_global_add": ([vp, vp, vp, vp, i64, i64], C.c_int),
        "cfrk_global_add_device": ([vp, vp, i64], C.c_int),
        "cfrk_global_merge_device": ([vp, vp, vp, vp, i64], C.c_int),
        "cfrk_global_finish": ([vp, C.POINTER(u64)], C.c_int),
        "cfrk_global_export": ([vp, vp, vp, vp, u64, C.POINTER(u64)], C.c_int),
        "cfrk_global_export_range": ([vp, C.c_uint32, C.c_uint32, vp, vp, vp, u64, C.POINTER(u64)], C.c_int),
        "cfrk_global_histogram": ([vp, vp, C.c_uint32], C.c_int),
        "cfrk_global_query": ([vp, vp, vp, i64, vp], C.c_int),
        "cfrk_global_query_device": ([vp, vp, vp, i64, vp], C.c_int),
        "cfrk_global_neighbors": ([vp, vp, vp, i64, C.c_uint32, vp], C.c_int),
        "cfrk_global_neighbors_device": ([vp, vp, vp, i64, C.c_uint32, vp], C.c_int),
        "cfrk_global_unitigs": ([vp, C.c_uint32, vp, u64, vp, vp, vp, u64, C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "cfrk_global_unitigs_device": ([vp, C.c_uint32, vp, u64, vp, vp, vp, u64, C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "cfrk_global_unitig_links": ([vp, C.c_uint32, vp, vp, vp, i64, i64, vp, vp, u64, C.POINTER(i64)], C.c_int),
        "cfrk_global_unitig_links_device": ([vp, C.c_uint32, vp, vp, vp, i64, i64, vp, vp, u64, C.POINTER(i64)], C.c_int),
        "cfrk_global_unitig_index": ([vp, C.c_uint32, vp, vp, vp, i64, i64], C.c_int),
        "cfrk_global_unitig_index_device": ([vp, C.c_uint32, vp, vp, vp, i64, i64], C.c_int),
        "cfrk_global_locate": ([vp, vp, vp, i64, vp], C.c_int),
        "cfrk_global_locate_device": ([vp, vp, vp, i64, vp], C.c_int),
        "cfrk_global_read_hits": ([vp, vp, vp, vp, i64, i64, vp, vp, u64, C.POINTER(i64)], C.c_int),
        "cfrk_global_read_hits_device": ([vp, vp, vp, vp, i64, i64, vp, vp, u64, C.POINTER(i64)], C.c_int),
        "cfrk_global_mask_keys": ([vp, vp, vp, i64], C.c_int),
        "cfrk_global_mask_keys_device": ([vp, vp, vp, i64], C.c_int),
        "cfrk_global_mask_unitigs": ([vp, vp, vp, vp, i64, i64, vp], C.c_int),
        "cfrk_global_mask_unitigs_device": ([vp, vp, vp, vp, i64, i64, vp], C.c_int),
        "cfrk_global_mask_clear": ([vp], C.c_int),
        "cfrk_global_mask_count": ([vp, C.POINTER(u64)], C.c_int),
        "cfrk_global_unitig_tips": ([vp, vp, i64, vp, vp, i64, C.c_uint32, C.c_uint32, vp, C.POINTER(i64)], C.c_int),
        "cfrk_global_unitig_tips_device": ([vp, vp, i64, vp, vp, i64, C.c_uint32, C.c_uint32, vp, C.POINTER(i64)], C.c_int),
        "cfrk_global_unitig_bubbles": ([vp, vp, i64, vp, vp, i64, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.POINTER(i64)], C.c_int),
        "cfrk_global_unitig_bubbles_device": ([vp, vp, i64, vp, vp, i64, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.POINTER(i64)], C.c_int),
        "cfrk_global_unitig_weak": ([vp, vp, i64, vp, vp, i64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp], C.c_int),
        "cfrk_global_unitig_weak_device": ([vp, vp, i64, vp, vp, i64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp], C.c_int),
        "cfrk_global_unitig_components": ([vp, vp, i64, vp, vp, i64, vp, vp, vp, u64, C.POINTER(i64), vp], C.c_int),
        "cfrk_global_unitig_components_device": ([vp, vp, i64, vp, vp, i64, vp, vp, vp, u64, C.POINTER(i64), vp], C.c_int),
        "cfrk_global_read_components": ([vp, vp, i64, vp, i64, vp, i64, vp, vp], C.c_int),
        "cfrk_global_read_components_device": ([vp, vp, i64, vp, i64, vp, i64, vp, vp], C.c_int),
        "cfrk_global_unitig_bulges": ([vp, vp, i64, vp, vp, i64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, u64, C.POINTER(i64), vp], C.c_int),
        "cfrk_global_unitig_bulges_device": ([vp, vp, i64, vp, vp, i64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, u64, C.POINTER(i64), vp], C.c_int),
        "cfrk_global_unitigs_compact": ([vp, vp, vp, vp, vp, i64, i64, vp, vp, i64, vp, vp, u64, vp, vp, vp, u64, vp, C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "cfrk_global_unitigs_compact_device": ([vp, vp, vp, vp, vp, i64, i64, vp, vp, i64, vp, vp, u64, vp, vp, vp, u64, vp, C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "cfrk_global_read_paths": ([vp, vp, i64, vp, i64, vp, i64, vp, vp, i64, vp, vp, u64, C.POINTER(i64), vp, vp], C.c_int),
        "cfrk_global_read_paths_device": ([vp, vp, i64, vp, i64, vp, i64, vp, vp, i64, vp, vp, u64, C.POINTER(i64), vp, vp], C.c_int),
        "cfrk_global_query_reads": ([vp, vp, vp, vp, i64, i64, vp], C.c_int),
        "cfrk_global_query_reads_device": ([vp, vp, i64, vp], C.c_int),
        "cfrk_global_read_stats": ([vp, vp, vp, vp, i64, i64, C.c_uint32, vp], C.c_int),
        "cfrk_global_read_stats_device": ([vp, vp, vp, vp, i64, i64, C.c_uint32, vp], C.c_int),
        "cfrk_global_read_spans": ([vp, vp, vp, vp, i64, i64, C.c_uint32, C.c_uint32, i32, vp], C.c_int),
        "cfrk_global_read_spans_device": ([vp, vp, vp, vp, i64, i64, C.c_uint32, C.c_uint32, i32, vp], C.c_int),
        "cfrk_global_correct_reads": ([vp, vp, vp, vp, i64, i64, C.c_uint32, vp, vp], C.c_int),
        "cfrk_global_correct_reads_device": ([vp, vp, vp, vp, i64, i64, C.c_uint32, vp, vp], C.c_int),
        "cfrk_global_normalize": ([vp, vp, vp, vp, i64, i64, C.c_uint32, i64, vp, C.POINTER(i64)], C.c_int),
        "cfrk_global_normalize_device": ([vp, vp, vp, vp, i64, i64, C.c_uint32, i64, vp, C.POINTER(i64)], C.c_int),
        "cfrk_global_normalize_pairs": ([vp, vp, vp, vp, i64, i64, C.c_uint32, i64, i32, vp, C.POINTER(i64)], C.c_int),
        "cfrk_global_normalize_pairs_device": ([vp, vp, vp, vp, i64, i64, C.c_uint32, i64, i32, vp, C.POINTER(i64)], C.c_int),
        "cfrk_reads_pair_keep": ([vp, i64, i32, i32, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "cfrk_reads_pair_keep_device": ([vp, i64, i32, i32, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "cfrk_text_pair_check": ([vp, i64, i32, vp, u64, vp, vp, u64, vp, C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "cfrk_text_pair_check_device": ([vp, i64, i32, vp, u64, vp, vp, u64, vp, C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "cfrk_reads_select": ([vp, vp, vp, vp, i64, i64, vp, vp, C.c_int32, vp, u64, vp, vp, vp, u64, C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "cfrk_reads_select_device": ([vp, vp, vp, vp, i64, i64, vp, vp, C.c_int32, vp, u64, vp, vp, vp, u64, C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "cfrk_text_index": ([vp, vp, u64, i32, vp, u64, C.POINTER(i64)], C.c_int),
        "cfrk_text_index_device": ([vp, vp, u64, i32, vp, u64, C.POINTER(i64)], C.c_int),
        "cfrk_reads_emit_text": ([vp, vp, vp, vp, i64, i64, vp, vp, C.c_int32, vp, u64, vp, i32, vp, u64, C.POINTER(u64), C.POINTER(i64)], C.c_int),
        "cfrk_reads_emit_text_device": ([vp, vp, vp, vp, i64, i64, vp, vp, C.c_int32, vp, u64, vp, i32, vp, u64, C.POINTER(u64), C.POINTER(i64)], C.c_int),
        "cfrk_global_export_device": ([vp, vp, vp, vp, u64, C.c_int, C.POINTER(u64)], C.c_int),
        "cfrk_global_digest": ([vp, C.POINTER(u64)], C.c_int),
        "cfrk_global_last_add_ms": ([vp, C.POINTER(C.c_float)], C.c_int),
        "cfrk_global_leaves_per_part": ([C.c_int], C.c_int),
        "cfrk_global_export_leaves_device": ([vp, vp, vp, vp, u64, C.c_int, C.POINTER(u64), vp], C.c_int),
        "cfrk_global_merge_leaves_device": ([vp, vp, vp, vp, C.POINTER(u64), vp, C.c_int], C.c_int),
        "cfrk_global_export_runs_device": ([vp, vp, u64, C.c_int, C.POINTER(u64)], C.c_int),
        "cfrk_global_merge_runs_device": ([vp, vp, C.POINTER(u64), C.c_int], C.c_int),
        "cfrk_global_export_runs_async": ([vp, vp, u64, C.c_int, C.c_int], C.c_int),
        "cfrk_global_export_runs_wait": ([vp, C.c_int, C.POINTER(u64)], C.c_int),
        "cfrk_global_merge_runs_group_device": ([vp, vp, C.POINTER(u64), C.c_int, C.c_int, C.c_int], C.c_int),
        "cfrk_global_runs_group_ms": ([vp, C.c_int, C.POINTER(C.c_float)], C.c_int),
        "cfrk_debug_msp_info": ([vp, C.POINTER(u64)], C.c_int),
        "cfrk_debug_set_mem_budget": ([vp, u64], C.c_int),
        "cfrk_debug_device_bytes": ([vp, C.POINTER(u64)], C.c_int),
        "cfrk_debug_hash_info": ([vp, u64, u64, C.POINTER(u64)], C.c_int),
        "cfrk_debug_radix_info": ([vp, C.c_int, i64, C.POINTER(u64)], C.c_int),
        "cfrk_debug_set_flags": ([vp, C.c_uint32], C.c_int),
        "cfrk_debug_set_param": ([vp, C.c_int, C.c_double], C.c_int),
        "cfrk_debug_last_add_passes": ([vp, C.POINTER(C.c_int)], C.c_int),
        "cfrk_distinct_sketch_device": ([vp, vp, i64, i32, i32, vp, C.POINTER(u64)], C.c_int),
        "cfrk_distinct_sketch": ([vp, vp, vp, vp, i64, i64, i32, i32, vp, C.POINTER(u64)], C.c_int),
        "cfrk_sketch_estimate": ([vp, C.POINTER(C.c_double)], C.c_int),
        "cfrk_sketch_merge": ([vp, vp], C.c_int),
        "cfrk_sketch_hint": ([vp, C.POINTER(u64)], C.c_int),
        "cfrk_fasta_parse_device": ([vp, vp, u64, i32, vp, u64, vp, vp, u64, C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "cfrk_fasta_parse": ([vp, vp, u64, i32, vp, u64, vp, vp, u64, C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "cfrk_fastq_parse_device": ([vp, vp, u64, i32, vp, u64, vp, vp, u64, C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "cfrk_fastq_parse": ([vp, vp, u64, i32, vp, u64, vp, vp, u64, C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "cfrk_synth_reads_device": ([vp, i64, i64, i32, i64, u64, u64, u64, i32, vp, vp, vp], C.c_int),
    }
    for name, (args, res) in sig.items():
        f = getattr(L, name, None)
        if f is None:       # an OLDER build swapped in by tools/ab.sh: the entry point raises when it is called
            continue        # (tests/test_abi_cpu.py checks that the product exports every symbol the header declares)
        f.argtypes = args
        f.restype = res
    _lib = L
    return L


def device_count():
    """usable devices (hipGetDeviceCount through the C ABI); raises when the library is missing"""
    n = C.c_int(0)
    L = load_library()
    rc = L.cfrk_device_count(C.byref(n))
    if rc != 0:
        raise CfrkError(rc, "cfrk_device_count", L.cfrk_strerror(rc).decode())
    return n.value


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def hash_info(lo, hi=0, ctx=None):
    """cfrk_debug_hash_info -> (log2 table slots, log2 index slots, hash of the one-word key lo, hash of the two-word
    key (lo, hi)); the hashes are the kernels' own function evaluated on the host, a key's home slot in 2^n slots is the
    hash's top n bits.  Without a Context (no device needed) both slot counts read 0."""
    out = (C.c_uint64 * 4)()
    rc = load_library().cfrk_debug_hash_info(ctx._h if ctx is not None else None, int(lo), int(hi), out)
    if rc != 0:
        raise CfrkError(rc, "cfrk_debug_hash_info")
    return tuple(int(x) for x in out)


def radix_info(k, nN, ctx=None):
    """cfrk_debug_radix_info -> dict: the shape radix.hip's host code chooses for a global add of nN bytes at k (b1, b2,
    idx, mul, inv, cap1, cap2; takes: the radix path counts such a batch; direct: k <= 7; hi8: level 1 keeps an 8-bit
    plane) -- pure host arithmetic, no device needed -- and, with a Context, what its most recent radix add did
    (attempts of the layout loop, relaid1 / relaid2: level 1 / the leaves were laid out again, grid of the leaf kernel)."""
    out = (C.c_uint64 * 12)()
    rc = load_library().cfrk_debug_radix_info(ctx._h if ctx is not None else None, int(k), int(nN), out)
    if rc != 0:
        raise CfrkError(rc, "cfrk_debug_radix_info")
    o = [int(x) for x in out]
    return {"b1": o[0], "b2": o[1], "idx": o[2], "mul": o[3], "inv": o[4], "cap1": o[5], "cap2": o[6],
            "takes": bool(o[7] & 1), "direct": bool(o[7] & 2), "hi8": bool(o[7] & 4),
            "attempts": o[8], "relaid1": bool(o[9]), "relaid2": bool(o[10]), "grid": o[11]}


def _sketch_regs(regs):
    regs = np.ascontiguousarray(regs, np.uint8)
    if regs.shape != (CFRK_SKETCH_REGS,):
        raise ValueError(f"a sketch is {CFRK_SKETCH_REGS} uint8 registers")
    return regs


def _sketch_call(name, rc):
    if rc != 0:
        raise CfrkError(rc, name, load_library().cfrk_strerror(rc).decode())


def sketch_estimate(regs):
    """distinct k-mers a sketch (Context.distinct_sketch) stands for: HyperLogLog with 2^14 registers, standard error
    0.81 %; all-zero registers give 0.0.  A host function: no device needed."""
    out = C.c_double()
    _sketch_call("cfrk_sketch_estimate", load_library().cfrk_sketch_estimate(_ptr(_sketch_regs(regs)), C.byref(out)))
    return out.value


def sketch_merge(dst, src):
    """dst = element-wise maximum of dst and src, in place: the sketch of the union of the two read sets -> dst"""
    if not (isinstance(dst, np.ndarray) and dst.dtype == np.uint8 and dst.flags.c_contiguous and dst.flags.writeable):
        raise ValueError("dst must be a writable contiguous uint8 array")
    _sketch_call("cfrk_sketch_merge", load_library().cfrk_sketch_merge(_ptr(_sketch_regs(dst)), _ptr(_sketch_regs(src))))
    return dst


def sketch_hint(regs):
    """a capacity_hint for GlobalCounter from a sketch: the estimate plus four standard errors (3.25 %), clamped to
    [2^20, 2^31]"""
    out = C.c_uint64()
    _sketch_call("cfrk_sketch_hint", load_library().cfrk_sketch_hint(_ptr(_sketch_regs(regs)), C.byref(out)))
    return out.value


class Context:
    """One HIP stream + persistent device pool on one GPU (cfrk_ctx)."""

    def __init__(self, device=0, stream=None):
        self._L = load_library()
        h = C.c_void_p()
        rc = self._L.cfrk_ctx_create(int(device), C.c_void_p(stream) if stream else None, C.byref(h))
        if rc != 0:
            raise CfrkError(rc, "cfrk_ctx_create", self._L.cfrk_strerror(rc).decode())
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._L.cfrk_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def check(self, rc, what):
        if rc != 0:
            raise CfrkError(rc, f"{what}: {self._L.cfrk_strerror(rc).decode()}",
                            self._L.cfrk_last_error(self._h).decode())

    def sync(self):
        self.check(self._L.cfrk_ctx_sync(self._h), "cfrk_ctx_sync")

    def device_bytes(self):
        """device memory the context holds (pool + global table), without the caller's buffers"""
        n = C.c_uint64()
        self.check(self._L.cfrk_debug_device_bytes(self._h, C.byref(n)), "cfrk_debug_device_bytes")
        return n.value

    # -- raw device buffers --------------------------------------------------------------
    def alloc(self, nbytes):
        p = C.c_void_p()
        self.check(self._L.cfrk_device_alloc(self._h, nbytes, C.byref(p)), "cfrk_device_alloc")
        return p.value

    def free(self, dptr):
        self.check(self._L.cfrk_device_free(self._h, C.c_void_p(dptr)), "cfrk_device_free")

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self.check(self._L.cfrk_memcpy_h2d(self._h, C.c_void_p(dptr), _ptr(arr), arr.nbytes), "cfrk_memcpy_h2d")

    def h2d_staged(self, dptr, arr):
        """h2d through the context's ring of pinned staging buffers (for memory the runtime copies slowly: a mapped file)"""
        arr = np.ascontiguousarray(arr)
        self.check(self._L.cfrk_memcpy_h2d_staged(self._h, C.c_void_p(dptr), _ptr(arr), arr.nbytes), "cfrk_memcpy_h2d_staged")

    def d2h(self, arr, dptr):
        self.check(self._L.cfrk_memcpy_d2h(self._h, _ptr(arr), C.c_void_p(dptr), arr.nbytes), "cfrk_memcpy_d2h")

    # -- per-read dense (kmer_main) --------------------------------------------------------
    def per_read_dense(self, data, start, length, k, flags=CFRK_COMPAT):
        data = np.ascontiguousarray(data, np.int8)
        start = np.ascontiguousarray(start, np.int64)
        length = np.ascontiguousarray(length, np.int32)
        nS = len(length)
        if len(start) != nS:
            raise ValueError("start and length differ in size")
        freq = np.empty(nS * 4 ** k if 1 <= k <= 15 else 0, np.int32)
        self.check(self._L.cfrk_per_read_dense(self._h, _ptr(data), _ptr(start), _ptr(length),
                                               len(data), nS, k, flags, _ptr(freq)),
                   "cfrk_per_read_dense")
        return freq.reshape(nS, -1) if nS else freq.reshape(0, 4 ** k)

    # -- per-read sparse (CSR rows of distinct k-mers, 1 <= k <= 32) -----------------------
    def per_read_sparse(self, data, start, length, k, flags=0):
        """-> (row_ptr int64[nS+1], keys uint64[nnz], counts uint32[nnz]): row i = the distinct k-mers of read i,
        ascending, with their multiplicities.  Sized by a sizes-only call, then filled by a second one."""
        data = np.ascontiguousarray(data, np.int8)
        start = np.ascontiguousarray(start, np.int64)
        length = np.ascontiguousarray(length, np.int32)
        nS = len(length)
        if len(start) != nS:
            raise ValueError("start and length differ in size")
        row_ptr = np.zeros(nS + 1, np.int64)
        nnz = C.c_uint64()
        args = (self._h, _ptr(data), _ptr(start), _ptr(length), len(data), nS, k, flags, _ptr(row_ptr))
        rc = self._L.cfrk_per_read_sparse(*args, None, None, 0, C.byref(nnz))
        if rc != CFRK_ERR_SMALL_BUF:
            self.check(rc, "cfrk_per_read_sparse")
            return row_ptr, np.empty(0, np.uint64), np.empty(0, np.uint32)
        keys = np.empty(nnz.value, np.uint64)
        counts = np.empty(nnz.value, np.uint32)
        self.check(self._L.cfrk_per_read_sparse(*args, _ptr(keys), _ptr(counts), len(keys), C.byref(nnz)),
                   "cfrk_per_read_sparse")
        return row_ptr, keys, counts

    def per_read_sparse_device(self, d_data, d_start, d_length, nN, nS, k, flags, d_row_ptr, d_keys, d_counts, cap):
        """device form -> nnz; d_keys / d_counts may be 0 with cap 0 (sizes only).  Raises CfrkError (code
        CFRK_ERR_SMALL_BUF, with .nnz set; d_row_ptr is complete) when nnz > cap.  Synchronises once, returns with
        the move of the rows enqueued on the context stream."""
        nnz = C.c_uint64()
        vp = lambda p: C.c_void_p(p) if p else None
        rc = self._L.cfrk_per_read_sparse_device(self._h, vp(d_data), vp(d_start), vp(d_length), nN, nS, k, flags,
                                                 vp(d_row_ptr), vp(d_keys), vp(d_counts), cap, C.byref(nnz))
        try:
            self.check(rc, "cfrk_per_read_sparse_device")
        except CfrkError as e:
            e.nnz = nnz.value
            raise
        return nnz.value

    # -- distinct k-mer estimate (HyperLogLog sketch, 1 <= k <= 64) ---------------------------
    def distinct_sketch(self, data, k, flags=0, start=None, length=None, regs=None):
        """-> (regs uint8[CFRK_SKETCH_REGS], valid windows of this call).  regs: a sketch to accumulate into (merged by
        maximum, in place when it is a contiguous uint8 array); None starts a fresh one.  sketch_estimate(regs) is the
        number of distinct k-mers, sketch_hint(regs) a capacity_hint for GlobalCounter."""
        data = np.ascontiguousarray(data, np.int8)
        if start is not None:
            start = np.ascontiguousarray(start, np.int64)
            length = np.ascontiguousarray(length, np.int32)
        nS = 0 if length is None else len(length)
        regs = np.zeros(CFRK_SKETCH_REGS, np.uint8) if regs is None else _sketch_regs(regs)
        windows = C.c_uint64()
        self.check(self._L.cfrk_distinct_sketch(self._h, _ptr(data), _ptr(start), _ptr(length), len(data), nS, k, flags,
                                                _ptr(regs), C.byref(windows)), "cfrk_distinct_sketch")
        return regs, windows.value

    def distinct_sketch_device(self, d_data, nN, k, flags, d_regs, want_windows=True):
        """device form: d_data 16-byte aligned, d_regs CFRK_SKETCH_REGS bytes on the device, merged by maximum (zero
        them for a fresh sketch) -> the call's valid windows (synchronises), or None with want_windows=False (returns
        with the kernels enqueued on the context stream)"""
        windows = C.c_uint64()
        self.check(self._L.cfrk_distinct_sketch_device(self._h, C.c_void_p(d_data) if d_data else None, nN, k, flags,
                                                       C.c_void_p(d_regs) if d_regs else None,
                                                       C.byref(windows) if want_windows else None),
                   "cfrk_distinct_sketch_device")
        return windows.value if want_windows else None

    # -- FASTA text parsed on the device -------------------------------------------------------
    def parse_fasta_device(self, d_text, nbytes, flags, d_data, cap_data, d_start, d_length, cap_reads):
        """device form: d_text 16-byte aligned -> (nN, nS); d_data / d_start / d_length may be 0 with zero capacities
        (sizes only).  Raises CfrkError (code CFRK_ERR_SMALL_BUF, with .nN and .nS set, nothing written) when the
        arrays are too small.  Synchronises once, returns with the last kernel enqueued on the context stream."""
        nN, nS = C.c_int64(), C.c_int64()
        vp = lambda p: C.c_void_p(p) if p else None
        rc = self._L.cfrk_fasta_parse_device(self._h, vp(d_text), nbytes, flags, vp(d_data), cap_data, vp(d_start),
                                             vp(d_length), cap_reads, C.byref(nN), C.byref(nS))
        try:
            self.check(rc, "cfrk_fasta_parse_device")
        except CfrkError as e:
            e.nN, e.nS = nN.value, nS.value
            raise
        return nN.value, nS.value

    def parse_fasta(self, text, flags=0):
        """FASTA text (bytes or a uint8 array) -> host (data int8[nN], start int64[nS], length int32[nS]), what the
        host parser makes of it: flags 0 = native, CFRK_COMPAT = the reference's reader.  A sizes-only call, then
        the parse into arrays of exactly that size."""
        text = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, np.uint8)
        nN, nS = C.c_int64(), C.c_int64()
        rc = self._L.cfrk_fasta_parse(self._h, _ptr(text), text.size, flags, None, 0, None, None, 0, C.byref(nN), C.byref(nS))
        if rc != CFRK_ERR_SMALL_BUF:
            self.check(rc, "cfrk_fasta_parse")
        data, start, length = np.empty(nN.value, np.int8), np.empty(nS.value, np.int64), np.empty(nS.value, np.int32)
        if rc == CFRK_ERR_SMALL_BUF:
            self.check(self._L.cfrk_fasta_parse(self._h, _ptr(text), text.size, flags, _ptr(data), data.size, _ptr(start),
                                                _ptr(length), start.size, C.byref(nN), C.byref(nS)), "cfrk_fasta_parse")
        return data, start, length

    # -- FASTQ text parsed on the device, low-quality bases masked ------------------------------
    def parse_fastq_device(self, d_text, nbytes, min_qual, d_data, cap_data, d_start, d_length, cap_reads):
        """device form: strict four-line FASTQ, d_text 16-byte aligned -> (nN, nS) in the native layout; with
        min_qual >= 1 a base whose Phred+33 quality is below it gets code -1.  d_data / d_start / d_length may be 0
        with zero capacities (sizes only).  Raises CfrkError (code CFRK_ERR_SMALL_BUF, with .nN and .nS set, nothing
        written) when the arrays are too small.  Synchronises twice; the arrays are complete when it returns."""
        nN, nS = C.c_int64(), C.c_int64()
        vp = lambda p: C.c_void_p(p) if p else None
        rc = self._L.cfrk_fastq_parse_device(self._h, vp(d_text), nbytes, min_qual, vp(d_data), cap_data, vp(d_start),
                                             vp(d_length), cap_reads, C.byref(nN), C.byref(nS))
        try:
            self.check(rc, "cfrk_fastq_parse_device")
        except CfrkError as e:
            e.nN, e.nS = nN.value, nS.value
            raise
        return nN.value, nS.value

    def parse_fastq(self, text, min_qual=0):
        """FASTQ text (bytes or a uint8 array) -> host (data int8[nN], start int64[nS], length int32[nS]), what the
        host parser (cfrk_host_parse_fastq) makes of it.  A sizes-only call, then the parse into arrays of exactly
        that size."""
        text = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, np.uint8)
        nN, nS = C.c_int64(), C.c_int64()
        rc = self._L.cfrk_fastq_parse(self._h, _ptr(text), text.size, min_qual, None, 0, None, None, 0, C.byref(nN), C.byref(nS))
        if rc != CFRK_ERR_SMALL_BUF:
            self.check(rc, "cfrk_fastq_parse")
        data, start, length = np.empty(nN.value, np.int8), np.empty(nS.value, np.int64), np.empty(nS.value, np.int32)
        if rc == CFRK_ERR_SMALL_BUF:
            self.check(self._L.cfrk_fastq_parse(self._h, _ptr(text), text.size, min_qual, _ptr(data), data.size, _ptr(start),
                                                _ptr(length), start.size, C.byref(nN), C.byref(nS)), "cfrk_fastq_parse")
        return data, start, length

    # -- select: the kept, trimmed reads compacted into new struct-read buffers ------------------
    def select_reads(self, data, start, length, spans=None, keep=None, min_len=0):
        """-> (data int8[nN'], start int64[nS'], length int32[nS'], index int64[nS']): the reads with keep[i] != 0
        (None: all) whose span (READ_SPAN_DTYPE, None: the whole read) holds at least min_len bases, trimmed to their
        spans, in input order in the native layout; index[j] = the input index of output read j.  A span that does not
        lie inside its read raises CfrkError (CFRK_ERR_LAYOUT).  Needs no job."""
        data = np.ascontiguousarray(data, np.int8)
        start = np.ascontiguousarray(start, np.int64)
        length = np.ascontiguousarray(length, np.int32)
        nS = len(length)
        if len(start) != nS:
            raise ValueError("start and length differ in size")
        if spans is not None:
            spans = np.ascontiguousarray(spans, READ_SPAN_DTYPE)
            if len(spans) != nS:
                raise ValueError("one span per read")
        if keep is not None:
            keep = np.ascontiguousarray(np.asarray(keep) != 0, np.uint8)
            if len(keep) != nS:
                raise ValueError("one keep byte per read")
        nN_o, nS_o = C.c_int64(), C.c_int64()
        head = (self._h, _ptr(data), _ptr(start), _ptr(length), len(data), nS, _ptr(spans), _ptr(keep), int(min_len))
        rc = self._L.cfrk_reads_select(*head, None, 0, None, None, None, 0, C.byref(nN_o), C.byref(nS_o))
        if rc != CFRK_ERR_SMALL_BUF:
            self.check(rc, "cfrk_reads_select")
        o_data, o_start = np.empty(nN_o.value, np.int8), np.empty(nS_o.value, np.int64)
        o_length, o_index = np.empty(nS_o.value, np.int32), np.empty(nS_o.value, np.int64)
        if rc == CFRK_ERR_SMALL_BUF:
            self.check(self._L.cfrk_reads_select(*head, _ptr(o_data), o_data.size, _ptr(o_start), _ptr(o_length),
                                                 _ptr(o_index), o_start.size, C.byref(nN_o), C.byref(nS_o)),
                       "cfrk_reads_select")
        return o_data, o_start, o_length, o_index

    def select_reads_device(self, d_data, d_start, d_length, nN, nS, d_span, d_keep, min_len, d_data_out, cap_data,
                            d_start_out, d_length_out, d_index_out, cap_reads):
        """device form -> (nN', nS'); d_span 0: whole reads, d_keep 0: all, d_index_out may be 0; the output arrays may
        be 0 with zero capacities (sizes only) and must not overlap the input.  Raises CfrkError (code
        CFRK_ERR_SMALL_BUF, with .nN and .nS set, nothing written) when the arrays are too small.  Synchronises once,
        returns with the copy enqueued on the context stream."""
        nN_o, nS_o = C.c_int64(), C.c_int64()
        vp = lambda p: C.c_void_p(p) if p else None
        rc = self._L.cfrk_reads_select_device(self._h, vp(d_data), vp(d_start), vp(d_length), nN, nS, vp(d_span),
                                              vp(d_keep), int(min_len), vp(d_data_out), cap_data, vp(d_start_out),
                                              vp(d_length_out), vp(d_index_out), cap_reads, C.byref(nN_o), C.byref(nS_o))
        try:
            self.check(rc, "cfrk_reads_select_device")
        except CfrkError as e:
            e.nN, e.nS = nN_o.value, nS_o.value
            raise
        return nN_o.value, nS_o.value

    # -- text out: the record index of a text, the kept reads written back as FASTA / FASTQ text ---
    def index_text(self, text, fmt):
        """text (bytes or a uint8 array), fmt CFRK_TEXT_FASTA / CFRK_TEXT_FASTQ -> np.ndarray[nS] of TEXT_RECORD_DTYPE:
        where each record's header line and quality line lie in the text.  Defined for every text (no grammar is
        checked).  A sizes-only call, then the call into an array of exactly that size."""
        text = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, np.uint8)
        nS = C.c_int64()
        rc = self._L.cfrk_text_index(self._h, _ptr(text), text.size, int(fmt), None, 0, C.byref(nS))
        if rc != CFRK_ERR_SMALL_BUF:
            self.check(rc, "cfrk_text_index")
        rec = np.zeros(nS.value, TEXT_RECORD_DTYPE)
        if rc == CFRK_ERR_SMALL_BUF:
            self.check(self._L.cfrk_text_index(self._h, _ptr(text), text.size, int(fmt), _ptr(rec), rec.size, C.byref(nS)),
                       "cfrk_text_index")
        return rec

    def index_text_device(self, d_text, nbytes, fmt, d_rec, cap_reads):
        """device form: d_text 16-byte aligned, d_rec room for cap_reads records of 24 bytes -> nS; d_rec may be 0 with
        capacity 0 (sizes only).  Raises CfrkError (code CFRK_ERR_SMALL_BUF, with .nS set, nothing written) when the
        array is too small.  Synchronises once, returns with the scatter enqueued on the context stream."""
        nS = C.c_int64()
        vp = lambda p: C.c_void_p(p) if p else None
        rc = self._L.cfrk_text_index_device(self._h, vp(d_text), nbytes, int(fmt), vp(d_rec), cap_reads, C.byref(nS))
        try:
            self.check(rc, "cfrk_text_index_device")
        except CfrkError as e:
            e.nS = nS.value
            raise
        return nS.value

    def emit_reads(self, data, start, length, text, rec, spans=None, keep=None, min_len=0, out_format=CFRK_TEXT_FASTA):
        """-> bytes: the reads select_reads() would keep, trimmed to their spans, as FASTA or FASTQ text (out_format) in
        input order, named as in `text` (the text they were parsed from) and, as FASTQ, with the matching slice of
        their quality line; rec = index_text(text, its format).  A span outside its read, a record outside the text and
        FASTQ output without a quality line as long as the read raise CfrkError (CFRK_ERR_LAYOUT).  Needs no job."""
        data = np.ascontiguousarray(data, np.int8)
        start = np.ascontiguousarray(start, np.int64)
        length = np.ascontiguousarray(length, np.int32)
        text = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, np.uint8)
        rec = np.ascontiguousarray(rec, TEXT_RECORD_DTYPE)
        nS = len(length)
        if len(start) != nS or len(rec) != nS:
            raise ValueError("start, length and rec differ in size")
        if spans is not None:
            spans = np.ascontiguousarray(spans, READ_SPAN_DTYPE)
            if len(spans) != nS:
                raise ValueError("one span per read")
        if keep is not None:
            keep = np.ascontiguousarray(np.asarray(keep) != 0, np.uint8)
            if len(keep) != nS:
                raise ValueError("one keep byte per read")
        nb, ns = C.c_uint64(), C.c_int64()
        head = (self._h, _ptr(data), _ptr(start), _ptr(length), len(data), nS, _ptr(spans), _ptr(keep), int(min_len),
                _ptr(text), text.size, _ptr(rec), int(out_format))
        rc = self._L.cfrk_reads_emit_text(*head, None, 0, C.byref(nb), C.byref(ns))
        if rc != CFRK_ERR_SMALL_BUF:
            self.check(rc, "cfrk_reads_emit_text")
            return b""
        out = np.empty(nb.value, np.uint8)
        self.check(self._L.cfrk_reads_emit_text(*head, _ptr(out), out.size, C.byref(nb), C.byref(ns)), "cfrk_reads_emit_text")
        return out.tobytes()

    def emit_reads_device(self, d_data, d_start, d_length, nN, nS, d_span, d_keep, min_len, d_text, nbytes, d_rec,
                          out_format, d_out, cap_out):
        """device form -> (bytes of text, reads written); d_span 0: whole reads, d_keep 0: all; d_out may be 0 with
        capacity 0 (sizes only) and must not overlap the input.  Raises CfrkError (code CFRK_ERR_SMALL_BUF, with
        .nbytes and .nS set, nothing written) when d_out is too small.  Synchronises once, returns with the copy
        enqueued on the context stream."""
        nb, ns = C.c_uint64(), C.c_int64()
        vp = lambda p: C.c_void_p(p) if p else None
        rc = self._L.cfrk_reads_emit_text_device(self._h, vp(d_data), vp(d_start), vp(d_length), nN, nS, vp(d_span), vp(d_keep),
                                                 int(min_len), vp(d_text), nbytes, vp(d_rec), int(out_format), vp(d_out),
                                                 cap_out, C.byref(nb), C.byref(ns))
        try:
            self.check(rc, "cfrk_reads_emit_text_device")
        except CfrkError as e:
            e.nbytes, e.nS = nb.value, ns.value
            raise
        return nb.value, ns.value

    # -- paired-end reads: the join of the mates' keep decisions, the mate-name check ---------------
    def pair_keep(self, keep_a=None, keep_b=None, spans_a=None, spans_b=None, length_a=None, length_b=None, min_len=0,
                  mode=CFRK_PAIR_BOTH, n_pairs=None):
        """split layout: one array per side, element j of each is pair j -> (pair uint8[n], orphan_a uint8[n],
        orphan_b uint8[n], counts: one PAIR_COUNTS_DTYPE row).  A read survives iff its keep byte is non-zero (None:
        all), its span lies inside the read and span.length >= min_len (spans None: length >= min_len).  BOTH: pair =
        sA & sB and a lone survivor is an orphan; EITHER: pair = sA | sB, no orphans.  Interleaved arrays are passed as
        x[0::2], x[1::2].  n_pairs is needed only when every array is None.  Needs no job."""
        arrs = {"keep_a": (keep_a, np.uint8), "keep_b": (keep_b, np.uint8), "spans_a": (spans_a, READ_SPAN_DTYPE),
                "spans_b": (spans_b, READ_SPAN_DTYPE), "length_a": (length_a, np.int32), "length_b": (length_b, np.int32)}
        got = {k: np.ascontiguousarray(a, t) for k, (a, t) in arrs.items() if a is not None}
        sizes = {len(a) for a in got.values()} | ({int(n_pairs)} if n_pairs is not None else set())
        if len(sizes) != 1:
            raise ValueError("the arrays of a pair join differ in size (or none was given and n_pairs is missing)")
        n = sizes.pop()
        out = [np.zeros(n, np.uint8) for _ in range(4)]
        counts = np.zeros(1, PAIR_COUNTS_DTYPE)
        g = lambda k: _ptr(got.get(k))
        self.check(self._L.cfrk_reads_pair_keep(self._h, n, 1, int(mode), int(min_len), g("keep_a"), g("keep_b"), g("spans_a"),
                                                g("spans_b"), g("length_a"), g("length_b"), _ptr(out[0]), _ptr(out[1]),
                                                _ptr(out[2]), _ptr(out[3]), _ptr(counts)), "cfrk_reads_pair_keep")
        assert (out[0] == out[1]).all()
        return out[0], out[2], out[3], counts[0]

    def pair_keep_device(self, n_pairs, stride, mode, min_len, d_keep_a, d_keep_b, d_span_a, d_span_b, d_length_a, d_length_b,
                         d_pair_a, d_pair_b, d_orphan_a=0, d_orphan_b=0, want_counts=True):
        """device form: mate A of pair j is element j * stride of the *_a arrays, mate B of the *_b arrays (interleaved:
        b = a + one element, stride 2; split: stride 1); 0 for an absent array.  The outputs may be the keep arrays (in
        place).  One launch on the context stream; synchronises only for the counts row (want_counts), which it returns"""
        vp = lambda p: C.c_void_p(p) if p else None
        counts = np.zeros(1, PAIR_COUNTS_DTYPE)
        self.check(self._L.cfrk_reads_pair_keep_device(self._h, n_pairs, int(stride), int(mode), int(min_len), vp(d_keep_a),
                                                       vp(d_keep_b), vp(d_span_a), vp(d_span_b), vp(d_length_a), vp(d_length_b),
                                                       vp(d_pair_a), vp(d_pair_b), vp(d_orphan_a), vp(d_orphan_b),
                                                       _ptr(counts) if want_counts else None), "cfrk_reads_pair_keep_device")
        return counts[0] if want_counts else None

    def check_pairs(self, text_a, rec_a, text_b=None, rec_b=None):
        """mate names -> (first_bad, n_bad): first_bad is the smallest index of a pair whose mates do not carry the same
        identifier (the header up to the first space or tab, a trailing /1 on A with /2 on B dropped), or -1.  With
        text_b / rec_b None the one text is interleaved (records 2j and 2j + 1); else record j of each text is a pair
        and the two record arrays must be of one size.  rec = index_text(text, its format).  Needs no job."""
        as_text = lambda t: np.frombuffer(t, np.uint8) if isinstance(t, (bytes, bytearray, memoryview)) else np.ascontiguousarray(t, np.uint8)
        text_a = as_text(text_a)
        rec_a = np.ascontiguousarray(rec_a, TEXT_RECORD_DTYPE)
        if rec_b is None:
            if text_b is not None:
                raise ValueError("text_b without rec_b")
            if len(rec_a) % 2:
                raise ValueError(f"{len(rec_a)} interleaved records: an odd number")
            n, stride, text_b = len(rec_a) // 2, 2, text_a
            pa, pb = _ptr(rec_a), (rec_a.ctypes.data + TEXT_RECORD_DTYPE.itemsize) if n else None
        else:
            text_b = text_a if text_b is None else as_text(text_b)
            rec_b = np.ascontiguousarray(rec_b, TEXT_RECORD_DTYPE)
            if len(rec_a) != len(rec_b):
                raise ValueError(f"{len(rec_a)} and {len(rec_b)} records: the two sides differ in size")
            n, stride, pa, pb = len(rec_a), 1, _ptr(rec_a), _ptr(rec_b)
        first, bad = C.c_int64(), C.c_int64()
        self.check(self._L.cfrk_text_pair_check(self._h, n, stride, _ptr(text_a), text_a.size, pa, _ptr(text_b), text_b.size, pb,
                                                C.byref(first), C.byref(bad)), "cfrk_text_pair_check")
        return int(first.value), int(bad.value)

    def check_pairs_device(self, n_pairs, stride, d_text_a, nbytes_a, d_rec_a, d_text_b, nbytes_b, d_rec_b):
        """device form -> (first_bad, n_bad); never reads outside the two texts; synchronises once"""
        vp = lambda p: C.c_void_p(p) if p else None
        first, bad = C.c_int64(), C.c_int64()
        self.check(self._L.cfrk_text_pair_check_device(self._h, n_pairs, int(stride), vp(d_text_a), nbytes_a, vp(d_rec_a),
                                                       vp(d_text_b), nbytes_b, vp(d_rec_b), C.byref(first), C.byref(bad)),
                   "cfrk_text_pair_check_device")
        return int(first.value), int(bad.value)

    def synth_reads_device(self, r0, R, L, Glen, d_data, d_start=None, d_length=None,
                           seedG=1, seedR=2, seedS=3, uniform=False):
        self.check(self._L.cfrk_synth_reads_device(self._h, r0, R, L, Glen, seedG, seedR, seedS,
                                                   int(uniform), C.c_void_p(d_data),
                                                   C.c_void_p(d_start) if d_start else None,
                                                   C.c_void_p(d_length) if d_length else None),
                   "cfrk_synth_reads_device")


class GlobalCounter:
    """Global (all-reads) k-mer counts: begin / add* / finish / export."""

    def __init__(self, ctx, k, flags=0, capacity_hint=0):
        self.ctx, self.k, self.flags = ctx, k, flags
        self._L = ctx._L
        ctx.check(self._L.cfrk_global_begin(ctx._h, k, flags, capacity_hint), "cfrk_global_begin")

    def add(self, data, start=None, length=None):
        data = np.ascontiguousarray(data, np.int8)
        if start is not None:
            start = np.ascontiguousarray(start, np.int64)
            length = np.ascontiguousarray(length, np.int32)
        nS = 0 if length is None else len(length)
        self.ctx.check(self._L.cfrk_global_add(self.ctx._h, _ptr(data), _ptr(start), _ptr(length),
                                               len(data), nS), "cfrk_global_add")

    def add_device(self, d_data, nN):
        self.ctx.check(self._L.cfrk_global_add_device(self.ctx._h, C.c_void_p(d_data), nN),
                       "cfrk_global_add_device")

    def merge_device(self, d_lo, d_hi, d_cnt, n):
        self.ctx.check(self._L.cfrk_global_merge_device(self.ctx._h, C.c_void_p(d_lo),
                                                        C.c_void_p(d_hi) if d_hi else None,
                                                        C.c_void_p(d_cnt), n),
                       "cfrk_global_merge_device")

    def finish(self, allow_saturated=False):
        n = C.c_uint64()
        rc = self._L.cfrk_global_finish(self.ctx._h, C.byref(n))
        if not (allow_saturated and rc == CFRK_ERR_COUNT_OVERFLOW):
            self.ctx.check(rc, "cfrk_global_finish")
        return n.value

    def digest(self, allow_saturated=False):
        """allow_saturated: a result with counts held at CFRK_COUNT_MAX (CFRK_ERR_COUNT_OVERFLOW) is returned
        instead of raised -- the digest is that of the saturated result"""
        out = (C.c_uint64 * 4)()
        rc = self._L.cfrk_global_digest(self.ctx._h, out)
        if not (allow_saturated and rc == CFRK_ERR_COUNT_OVERFLOW):
            self.ctx.check(rc, "cfrk_global_digest")
        return tuple(int(x) for x in out)

    def leaves_per_part(self, parts):
        return int(self._L.cfrk_global_leaves_per_part(parts))

    def export_leaves_device(self, d_keys, d_cnt, cap, parts, d_leaf_counts, d_keys_hi=0):
        """per-leaf owner export (d_keys_hi: high key words, k > 32); raises CfrkError(code -4)
        when the result is not in leaf form"""
        pc = (C.c_uint64 * parts)()
        self.ctx.check(self._L.cfrk_global_export_leaves_device(self.ctx._h, C.c_void_p(d_keys),
                                                                C.c_void_p(d_keys_hi) if d_keys_hi else None,
                                                                C.c_void_p(d_cnt), cap, parts, pc,
                                                                C.c_void_p(d_leaf_counts)),
                       "cfrk_global_export_leaves_device")
        return [int(x) for x in pc]

    def merge_leaves_device(self, d_keys, d_cnt, recv_counts, d_leaf_counts, d_keys_hi=0):
        parts = len(recv_counts)
        rc = (C.c_uint64 * parts)(*[int(x) for x in recv_counts])
        self.ctx.check(self._L.cfrk_global_merge_leaves_device(self.ctx._h, C.c_void_p(d_keys),
                                                               C.c_void_p(d_keys_hi) if d_keys_hi else None,
                                                               C.c_void_p(d_cnt), rc,
                                                               C.c_void_p(d_leaf_counts), parts),
                       "cfrk_global_merge_leaves_device")

    def export_runs_device(self, d_packed, cap_rows, parts):
        """CFRK_RUNS_ONLY job: per-leaf deduplicated runs, one packed segment per owner -> rows per
        segment; raises CfrkError(code -4) when the shard's runs are not all in the leaf streams"""
        pr = (C.c_uint64 * parts)()
        self.ctx.check(self._L.cfrk_global_export_runs_device(self.ctx._h, C.c_void_p(d_packed), cap_rows, parts, pr),
                       "cfrk_global_export_runs_device")
        return [int(x) for x in pr]

    def merge_runs_device(self, d_packed, recv_rows):
        parts = len(recv_rows)
        rr = (C.c_uint64 * parts)(*[int(x) for x in recv_rows])
        self.ctx.check(self._L.cfrk_global_merge_runs_device(self.ctx._h, C.c_void_p(d_packed), rr, parts),
                       "cfrk_global_merge_runs_device")

    # -- pipelined runs exchange (CFRK_RUNS_ONLY | CFRK_RUNS_DEFER jobs; one-word keys) ----------------------
    def export_runs_async(self, d_packed, seg_cap_rows, parts, ngroups):
        """enqueue deduplication + packing of every group of leaves into the send buffer; returns at once"""
        self.ctx.check(self._L.cfrk_global_export_runs_async(self.ctx._h, C.c_void_p(d_packed), seg_cap_rows, parts, ngroups),
                       "cfrk_global_export_runs_async")
        self._runs_parts = parts

    def export_runs_wait(self, group):
        """wait for group `group` only -> rows per owner segment; CfrkError -9 (segment too small) / -4 (overflow, spill)"""
        pr = (C.c_uint64 * self._runs_parts)()
        self.ctx.check(self._L.cfrk_global_export_runs_wait(self.ctx._h, group, pr), "cfrk_global_export_runs_wait")
        return [int(x) for x in pr]

    def merge_runs_group_device(self, d_recv, recv_rows, group, ngroups):
        """owner: count group `group` from the received segments, read in place; enqueued, no host synchronisation"""
        parts = len(recv_rows)
        rr = (C.c_uint64 * parts)(*[int(x) for x in recv_rows])
        self.ctx.check(self._L.cfrk_global_merge_runs_group_device(self.ctx._h, C.c_void_p(d_recv), rr, parts, group, ngroups),
                       "cfrk_global_merge_runs_group_device")

    def runs_group_ms(self, group):
        ms = C.c_float()
        self.ctx.check(self._L.cfrk_global_runs_group_ms(self.ctx._h, group, C.byref(ms)), "cfrk_global_runs_group_ms")
        return ms.value

    def msp_info(self):
        out = (C.c_uint64 * 9)()
        self.ctx.check(self._L.cfrk_debug_msp_info(self.ctx._h, out), "cfrk_debug_msp_info")
        names = ("l1_records", "l1_max_bin", "l1_cap", "l2_records", "l2_max_leaf", "l2_cap",
                 "spilled_records", "spilled_kmers", "list_entries")
        return dict(zip(names, (int(x) for x in out)))

    def hash_geometry(self):
        """(log2 slots of the HBM table, log2 slots of the query index or 0 while no hash index is valid)"""
        return hash_info(0, 0, self.ctx)[:2]

    def set_mem_budget(self, nbytes):
        self.ctx.check(self._L.cfrk_debug_set_mem_budget(self.ctx._h, int(nbytes)), "cfrk_debug_set_mem_budget")

    def set_debug_flags(self, flags):
        self.ctx.check(self._L.cfrk_debug_set_flags(self.ctx._h, int(flags)), "cfrk_debug_set_flags")

    def set_debug_param(self, which, value):
        self.ctx.check(self._L.cfrk_debug_set_param(self.ctx._h, int(which), float(value)), "cfrk_debug_set_param")

    def last_add_passes(self):
        n = C.c_int()
        self.ctx.check(self._L.cfrk_debug_last_add_passes(self.ctx._h, C.byref(n)), "cfrk_debug_last_add_passes")
        return n.value

    def last_add_ms(self):
        ms = C.c_float()
        self.ctx.check(self._L.cfrk_global_last_add_ms(self.ctx._h, C.byref(ms)), "cfrk_global_last_add_ms")
        return ms.value

    def export(self, allow_saturated=False, min_count=1, max_count=CFRK_COUNT_MAX):
        """-> (keys_lo, keys_hi, counts) sorted by (hi, lo); only entries with min_count <= count <= max_count
        (min_count 0 reads as 1)"""
        n = self.finish(allow_saturated)
        lo = np.empty(n, np.uint64)
        hi = np.empty(n, np.uint64)
        cnt = np.empty(n, np.uint32)
        got = C.c_uint64()
        rc = self._L.cfrk_global_export_range(self.ctx._h, int(min_count), int(max_count), _ptr(lo), _ptr(hi),
                                              _ptr(cnt), n, C.byref(got))
        if not (allow_saturated and rc == CFRK_ERR_COUNT_OVERFLOW):
            self.ctx.check(rc, "cfrk_global_export_range")
        m = got.value
        assert m <= n
        return lo[:m], hi[:m], cnt[:m]

    def export_range(self, min_count, max_count, cap, allow_saturated=False):
        """cfrk_global_export_range into buffers of `cap` entries -> (keys_lo, keys_hi, counts); raises CfrkError
        (CFRK_ERR_SMALL_BUF, with .n_out = entries kept) when they do not fit"""
        lo = np.empty(cap, np.uint64)
        hi = np.empty(cap, np.uint64)
        cnt = np.empty(cap, np.uint32)
        got = C.c_uint64()
        rc = self._L.cfrk_global_export_range(self.ctx._h, int(min_count), int(max_count), _ptr(lo), _ptr(hi),
                                              _ptr(cnt), cap, C.byref(got))
        if not (allow_saturated and rc == CFRK_ERR_COUNT_OVERFLOW):
            try:
                self.ctx.check(rc, "cfrk_global_export_range")
            except CfrkError as e:
                e.n_out = got.value
                raise
        m = got.value
        return lo[:m], hi[:m], cnt[:m]

    def histogram(self, nbins, allow_saturated=False):
        """abundance histogram (k-mer spectrum) -> np.uint64[nbins]: h[c] = keys counted c times, the last bin
        every key counted nbins - 1 times or more (2 <= nbins <= 2^24)"""
        nbins = int(nbins)
        h = np.zeros(nbins if 2 <= nbins <= 1 << 24 else 1, np.uint64)
        rc = self._L.cfrk_global_histogram(self.ctx._h, _ptr(h), nbins if 0 <= nbins < 1 << 32 else 0)
        if not (allow_saturated and rc == CFRK_ERR_COUNT_OVERFLOW):
            self.ctx.check(rc, "cfrk_global_histogram")
        return h

    def query(self, keys_lo, keys_hi=None):
        """count of every key -> np.uint32[n] (0: absent; CFRK_COUNT_MAX: at least that); canonicalised in a
        CFRK_CANONICAL job"""
        lo = np.ascontiguousarray(keys_lo, np.uint64)
        hi = None if keys_hi is None else np.ascontiguousarray(keys_hi, np.uint64)
        if hi is not None and len(hi) != len(lo):
            raise ValueError("keys_lo and keys_hi differ in length")
        out = np.empty(len(lo), np.uint32)
        self.ctx.check(self._L.cfrk_global_query(self.ctx._h, _ptr(lo), _ptr(hi), len(lo), _ptr(out)),
                       "cfrk_global_query")
        return out

    def query_device(self, d_lo, d_hi, n, d_out):
        """device form of query(): returns with the lookup kernel enqueued on the context stream"""
        self.ctx.check(self._L.cfrk_global_query_device(self.ctx._h, C.c_void_p(d_lo) if d_lo else None,
                                                        C.c_void_p(d_hi) if d_hi else None, n,
                                                        C.c_void_p(d_out) if d_out else None),
                       "cfrk_global_query_device")

    def neighbors(self, keys_lo, keys_hi=None, min_count=1):
        """neighbour mask of every key, taken as an oriented k-mer exactly as given -> np.uint8[n]: bit b (0..3) is set
        iff key[1:] + b is present with count >= min_count, bit 4 + b iff b + key[:-1] is (the neighbour is
        canonicalised in a CFRK_CANONICAL job); 0 for a key with bits at or above 2k"""
        lo = np.ascontiguousarray(keys_lo, np.uint64)
        hi = None if keys_hi is None else np.ascontiguousarray(keys_hi, np.uint64)
        if hi is not None and len(hi) != len(lo):
            raise ValueError("keys_lo and keys_hi differ in length")
        out = np.empty(len(lo), np.uint8)
        self.ctx.check(self._L.cfrk_global_neighbors(self.ctx._h, _ptr(lo), _ptr(hi), len(lo), int(min_count), _ptr(out)),
                       "cfrk_global_neighbors")
        return out

    def neighbors_device(self, d_lo, d_hi, n, min_count, d_masks):
        """device form of neighbors(): returns with the kernel enqueued on the context stream"""
        vp = lambda p: C.c_void_p(p) if p else None
        self.ctx.check(self._L.cfrk_global_neighbors_device(self.ctx._h, vp(d_lo), vp(d_hi), n, int(min_count), vp(d_masks)),
                       "cfrk_global_neighbors_device")

    def unitigs(self, min_count=1):
        """the compacted de Bruijn graph of the keys with count >= min_count -> (data int8[nN], start int64[nS],
        length int32[nS], rec UNITIG_DTYPE[nS]): the unitigs in the native struct-read layout (codes 0..3, one -1 behind
        each), ascending by first k-mer; rec: summed count, k-mers, CFRK_UNITIG_CIRCULAR.  A sizes-only call, then the
        call into arrays of exactly that size."""
        nN, nS = C.c_int64(), C.c_int64()
        rc = self._L.cfrk_global_unitigs(self.ctx._h, int(min_count), None, 0, None, None, None, 0, C.byref(nN), C.byref(nS))
        if rc != CFRK_ERR_SMALL_BUF:
            self.ctx.check(rc, "cfrk_global_unitigs")
        data, start = np.empty(nN.value, np.int8), np.empty(nS.value, np.int64)
        length, rec = np.empty(nS.value, np.int32), np.zeros(nS.value, UNITIG_DTYPE)
        if rc == CFRK_ERR_SMALL_BUF:
            self.ctx.check(self._L.cfrk_global_unitigs(self.ctx._h, int(min_count), _ptr(data), data.size, _ptr(start), _ptr(length),
                                                       _ptr(rec), rec.size, C.byref(nN), C.byref(nS)), "cfrk_global_unitigs")
        return data, start, length, rec

    def unitigs_device(self, min_count, d_data_out, cap_data, d_start_out, d_length_out, d_rec_out, cap_unitigs):
        """device form -> (nN, nS); the arrays may be 0 with zero capacities (sizes only).  Raises CfrkError (code
        CFRK_ERR_SMALL_BUF, with .nN and .nS set, nothing written) when they are too small.  Synchronises once, returns
        with the emit enqueued on the context stream."""
        nN, nS = C.c_int64(), C.c_int64()
        vp = lambda p: C.c_void_p(p) if p else None
        rc = self._L.cfrk_global_unitigs_device(self.ctx._h, int(min_count), vp(d_data_out), cap_data, vp(d_start_out),
                                                vp(d_length_out), vp(d_rec_out), cap_unitigs, C.byref(nN), C.byref(nS))
        try:
            self.ctx.check(rc, "cfrk_global_unitigs_device")
        except CfrkError as e:
            e.nN, e.nS = nN.value, nS.value
            raise
        return nN.value, nS.value

    def unitig_links(self, data, start, length, min_count=1):
        """the links between the unitigs of this job at this min_count, as unitigs() returned them -> (link_ptr
        int64[nS + 1], links UNITIG_LINK_DTYPE[n_links]): CSR over unitigs; a row holds the links out of (j,+), then those
        out of (j,-) (CFRK_LINK_FROM_MINUS), ascending by appended base, target + before - (CFRK_LINK_TO_MINUS).  A
        sizes-only call, then the call into an array of exactly that size."""
        data = np.ascontiguousarray(data, np.int8)
        start = np.ascontiguousarray(start, np.int64)
        length = np.ascontiguousarray(length, np.int32)
        nS, n = len(length), C.c_int64()
        link_ptr = np.zeros(nS + 1, np.int64)
        args = (self.ctx._h, int(min_count), _ptr(data), _ptr(start), _ptr(length), len(data), nS, _ptr(link_ptr))
        rc = self._L.cfrk_global_unitig_links(*args, None, 0, C.byref(n))
        if rc != CFRK_ERR_SMALL_BUF:
            self.ctx.check(rc, "cfrk_global_unitig_links")
        links = np.zeros(n.value, UNITIG_LINK_DTYPE)
        if rc == CFRK_ERR_SMALL_BUF:
            self.ctx.check(self._L.cfrk_global_unitig_links(*args, _ptr(links), links.size, C.byref(n)), "cfrk_global_unitig_links")
        return link_ptr, links

    def unitig_links_device(self, min_count, d_data, d_start, d_length, nN, nS, d_link_ptr, d_links, cap_links):
        """device form -> n_links; d_links may be 0 with cap_links 0 (sizes only).  Raises CfrkError (code
        CFRK_ERR_SMALL_BUF, with .n_links set, d_link_ptr complete, nothing written to d_links) when cap_links is too
        small.  Synchronises once, returns with the fill pass enqueued on the context stream."""
        n = C.c_int64()
        vp = lambda p: C.c_void_p(p) if p else None
        rc = self._L.cfrk_global_unitig_links_device(self.ctx._h, int(min_count), vp(d_data), vp(d_start), vp(d_length), nN, nS,
                                                     vp(d_link_ptr), vp(d_links), cap_links, C.byref(n))
        try:
            self.ctx.check(rc, "cfrk_global_unitig_links_device")
        except CfrkError as e:
            e.n_links = n.value
            raise
        return n.value

    def unitig_index(self, data, start, length, min_count=1):
        """build the position map from the unitigs of this job at this min_count, as unitigs() returned them: afterwards
        locate() and read_hits() answer until the result changes.  Raises CfrkError (CFRK_ERR_LAYOUT, the message naming
        the first offending unitig) when the list is not exactly the unitigs of this job at this min_count."""
        data = np.ascontiguousarray(data, np.int8)
        start = np.ascontiguousarray(start, np.int64)
        length = np.ascontiguousarray(length, np.int32)
        self.ctx.check(self._L.cfrk_global_unitig_index(self.ctx._h, int(min_count), _ptr(data), _ptr(start), _ptr(length),
                                                        len(data), len(length)), "cfrk_global_unitig_index")

    def unitig_index_device(self, min_count, d_data, d_start, d_length, nN, nS):
        """device form of unitig_index(): synchronises once, for the consistency check"""
        vp = lambda p: C.c_void_p(p) if p else None
        self.ctx.check(self._L.cfrk_global_unitig_index_device(self.ctx._h, int(min_count), vp(d_data), vp(d_start), vp(d_length),
                                                               nN, nS), "cfrk_global_unitig_index_device")

    def locate(self, keys_lo, keys_hi=None):
        """where every key, taken as an oriented k-mer exactly as given, lies on the unitigs -> UNITIG_POS_DTYPE[n]:
        unitig j and at = p << 1 | minus (minus: the key is the reverse complement of the unitig's k-mer p); both words
        CFRK_POS_NONE for a key that is not solid or has bits at or above 2k.  Needs unitig_index()."""
        lo = np.ascontiguousarray(keys_lo, np.uint64)
        hi = None if keys_hi is None else np.ascontiguousarray(keys_hi, np.uint64)
        if hi is not None and len(hi) != len(lo):
            raise ValueError("keys_lo and keys_hi differ in length")
        out = np.empty(len(lo), UNITIG_POS_DTYPE)
        self.ctx.check(self._L.cfrk_global_locate(self.ctx._h, _ptr(lo), _ptr(hi), len(lo), _ptr(out)), "cfrk_global_locate")
        return out

    def locate_device(self, d_lo, d_hi, n, d_out):
        """device form of locate(): returns with the kernel enqueued on the context stream"""
        vp = lambda p: C.c_void_p(p) if p else None
        self.ctx.check(self._L.cfrk_global_locate_device(self.ctx._h, vp(d_lo), vp(d_hi), n, vp(d_out)), "cfrk_global_locate_device")

    def read_hits(self, data, start, length):
        """the hits of every read on the unitigs -> (hit_ptr int64[nS + 1], hits READ_HIT_DTYPE[n_hits]): CSR over reads; a
        hit is a maximal stretch of windows that step along one unitig on one strand: unitig, unitig_at = off << 1 |
        minus, read_off, n_windows.  Needs unitig_index().  A sizes-only call, then the call into an array of exactly
        that size."""
        data = np.ascontiguousarray(data, np.int8)
        start = np.ascontiguousarray(start, np.int64)
        length = np.ascontiguousarray(length, np.int32)
        nS, n = len(length), C.c_int64()
        hit_ptr = np.zeros(nS + 1, np.int64)
        args = (self.ctx._h, _ptr(data), _ptr(start), _ptr(length), len(data), nS, _ptr(hit_ptr))
        rc = self._L.cfrk_global_read_hits(*args, None, 0, C.byref(n))
        if rc != CFRK_ERR_SMALL_BUF:
            self.ctx.check(rc, "cfrk_global_read_hits")
        hits = np.zeros(n.value, READ_HIT_DTYPE)
        if rc == CFRK_ERR_SMALL_BUF:
            self.ctx.check(self._L.cfrk_global_read_hits(*args, _ptr(hits), hits.size, C.byref(n)), "cfrk_global_read_hits")
        return hit_ptr, hits

    def read_hits_device(self, d_data, d_start, d_length, nN, nS, d_hit_ptr, d_hits, cap_hits):
        """device form -> n_hits; d_hits may be 0 with cap_hits 0 (sizes only).  Raises CfrkError (code
        CFRK_ERR_SMALL_BUF, with .n_hits set, d_hit_ptr complete, nothing written to d_hits) when cap_hits is too small.
        Synchronises once, returns with the fill pass enqueued on the context stream."""
        n = C.c_int64()
        vp = lambda p: C.c_void_p(p) if p else None
        rc = self._L.cfrk_global_read_hits_device(self.ctx._h, vp(d_data), vp(d_start), vp(d_length), nN, nS, vp(d_hit_ptr),
                                                  vp(d_hits), cap_hits, C.byref(n))
        try:
            self.ctx.check(rc, "cfrk_global_read_hits_device")
        except CfrkError as e:
            e.n_hits = n.value
            raise
        return n.value

    def read_paths(self, hit_ptr, hits, rec, link_ptr, links, support=None):
        """the hits of every read (read_hits()) joined across the links -> (path_ptr int64[nR + 1], paths
        READ_PATH_DTYPE[n_paths], support uint32[n_links], stats): CSR over reads; a path is a maximal chain of
        consecutive hits of a read in which each leaves its oriented unitig at the end, the next enters its own at the
        head one window later, and a link of (link_ptr, links) joins the two: hit_first (inside the read's hit row),
        n_hits, read_off, n_windows.  links may be any sub-CSR of unitig_links(): the reads then break where rows are
        missing.  support[r] is INCREMENTED by the steps across link r: pass the array of an earlier batch to
        accumulate, None starts from zero.  stats = {"n_paths", "n_steps", "n_gaps", "n_unlinked"}.  Raises CfrkError
        (CFRK_ERR_LAYOUT, the message naming the unitig or the read) when the rows are not link rows or the hits not
        hits on these unitigs; support is then untouched.  A sizes-only call, then the call into an array of exactly
        that size."""
        hit_ptr = np.ascontiguousarray(hit_ptr, np.int64)
        hits = np.ascontiguousarray(hits, READ_HIT_DTYPE)
        rec = np.ascontiguousarray(rec, UNITIG_DTYPE)
        link_ptr = np.ascontiguousarray(link_ptr, np.int64)
        links = np.ascontiguousarray(links, UNITIG_LINK_DTYPE)
        if len(hit_ptr) < 1 or len(link_ptr) != len(rec) + 1:
            raise ValueError("hit_ptr is empty, or link_ptr has not one entry more than rec")
        if support is None:
            support = np.zeros(len(links), np.uint32)
        if support.dtype != np.uint32 or not support.flags.c_contiguous or len(support) != len(links):
            raise ValueError("support is not a contiguous uint32 array with one entry per link")
        nR, n = len(hit_ptr) - 1, C.c_int64()
        path_ptr, stats = np.zeros(nR + 1, np.int64), np.zeros(1, PATH_STATS_DTYPE)
        args = (self.ctx._h, _ptr(hit_ptr), nR, _ptr(hits), len(hits), _ptr(rec), len(rec), _ptr(link_ptr), _ptr(links), len(links),
                _ptr(path_ptr))
        rc = self._L.cfrk_global_read_paths(*args, None, 0, C.byref(n), None, _ptr(stats))       # (no support: counted below)
        if rc != CFRK_ERR_SMALL_BUF:
            self.ctx.check(rc, "cfrk_global_read_paths")
        paths = np.zeros(n.value, READ_PATH_DTYPE)
        self.ctx.check(self._L.cfrk_global_read_paths(*args, _ptr(paths), paths.size, C.byref(n), _ptr(support), _ptr(stats)),
                       "cfrk_global_read_paths")
        assert n.value == int(path_ptr[nR]) == int(stats["n_paths"][0])
        return path_ptr, paths, support, {f: int(stats[f][0]) for f in PATH_STATS_DTYPE.names}

    def read_paths_device(self, d_hit_ptr, nR, d_hits, n_hits, d_rec, nS, d_link_ptr, d_links, n_links, d_path_ptr, d_paths, cap_paths,
                          d_support=0):
        """device form -> (n_paths, stats); d_paths may be 0 with cap_paths 0 (sizes only); d_support may be 0 (no
        support wanted), else its n_links words are added to.  Raises CfrkError (code CFRK_ERR_SMALL_BUF, with .n_paths
        and .stats set, d_path_ptr and d_support complete, nothing written to d_paths) when cap_paths is too small.
        Synchronises once, returns with the passes that write d_paths enqueued on the context stream."""
        n, stats = C.c_int64(), np.zeros(1, PATH_STATS_DTYPE)
        vp = lambda p: C.c_void_p(p) if p else None
        rc = self._L.cfrk_global_read_paths_device(self.ctx._h, vp(d_hit_ptr), nR, vp(d_hits), n_hits, vp(d_rec), nS, vp(d_link_ptr),
                                                   vp(d_links), n_links, vp(d_path_ptr), vp(d_paths), cap_paths, C.byref(n),
                                                   vp(d_support), _ptr(stats))
        st = {f: int(stats[f][0]) for f in PATH_STATS_DTYPE.names}
        try:
            self.ctx.check(rc, "cfrk_global_read_paths_device")
        except CfrkError as e:
            e.n_paths, e.stats = n.value, st
            raise
        return n.value, st

    def unitig_components(self, rec, link_ptr, links, drop=None):
        """the connected components of the unitig graph -> (comp uint32[nS], table UNITIG_COMPONENT_DTYPE[n_comps],
        stats): two unitigs with drop[j] == 0 (all of them when drop is None) belong together iff a chain of links, read
        without strand or direction, joins them through such unitigs.  Components are numbered ascending by their
        smallest unitig; comp[j] is CFRK_COMP_NONE for a dropped unitig.  A table row sums its members' kc and n_kmers
        and counts their links to kept targets (n_links), names the smallest member (first) and counts the members
        (n_unitigs).  stats = {"n_components", "n_unitigs", "n_kmers", "n_links"} over the kept unitigs.  Raises CfrkError
        (CFRK_ERR_LAYOUT, the message naming the unitig) when the rows are not link rows.  A sizes-only call, then the
        call into an array of exactly that size."""
        rec = np.ascontiguousarray(rec, UNITIG_DTYPE)
        link_ptr = np.ascontiguousarray(link_ptr, np.int64)
        links = np.ascontiguousarray(links, UNITIG_LINK_DTYPE)
        if len(link_ptr) != len(rec) + 1:
            raise ValueError("link_ptr has not one entry more than rec")
        if drop is not None:
            drop = np.ascontiguousarray(drop, np.uint8)
            if len(drop) != len(rec):
                raise ValueError("drop and rec differ in length")
        comp, stats, n = np.zeros(len(rec), np.uint32), np.zeros(1, COMPONENT_STATS_DTYPE), C.c_int64()
        args = (self.ctx._h, _ptr(rec), len(rec), _ptr(link_ptr), _ptr(links), len(links), _ptr(drop) if drop is not None else None,
                _ptr(comp))
        rc = self._L.cfrk_global_unitig_components(*args, None, 0, C.byref(n), _ptr(stats))
        if rc != CFRK_ERR_SMALL_BUF:
            self.ctx.check(rc, "cfrk_global_unitig_components")
        table = np.zeros(n.value, UNITIG_COMPONENT_DTYPE)
        self.ctx.check(self._L.cfrk_global_unitig_components(*args, _ptr(table), table.size, C.byref(n), _ptr(stats)),
                       "cfrk_global_unitig_components")
        assert n.value == len(table) == int(stats["n_components"][0])
        return comp, table, {f: int(stats[f][0]) for f in COMPONENT_STATS_DTYPE.names}

    def unitig_components_device(self, d_rec, nS, d_link_ptr, d_links, n_links, d_drop, d_comp, d_comps=0, cap_comps=0):
        """device form -> (n_comps, stats); d_drop may be 0 (nothing dropped); d_comps may be 0 with cap_comps 0 (sizes
        only).  Raises CfrkError (code CFRK_ERR_SMALL_BUF, with .n_comps and .stats set, d_comp complete, nothing written
        to d_comps) when cap_comps is too small.  Synchronises once, returns with the table's passes enqueued."""
        n, stats = C.c_int64(), np.zeros(1, COMPONENT_STATS_DTYPE)
        vp = lambda p: C.c_void_p(p) if p else None
        rc = self._L.cfrk_global_unitig_components_device(self.ctx._h, vp(d_rec), nS, vp(d_link_ptr), vp(d_links), n_links, vp(d_drop),
                                                          vp(d_comp), vp(d_comps), cap_comps, C.byref(n), _ptr(stats))
        st = {f: int(stats[f][0]) for f in COMPONENT_STATS_DTYPE.names}
        try:
            self.ctx.check(rc, "cfrk_global_unitig_components_device")
        except CfrkError as e:
            e.n_comps, e.stats = n.value, st
            raise
        return n.value, st

    def read_components(self, hit_ptr, hits, comp):
        """the component every read goes with -> (rows READ_COMPONENT_DTYPE[nR], stats): from the hits of read_hits() and
        comp of unitig_components().  A read's deciding hit is the one with the most windows among those whose unitig
        has a component, the earliest on a tie: comp, hit (its index inside the read's row), n_windows; flags has
        CFRK_READ_COMP_SPLIT when another such hit lies in a different component and CFRK_READ_COMP_DROPPED when some hit
        lies on a unitig without one.  A read with no deciding hit gets comp = hit = 0xFFFFFFFF, n_windows = 0.  stats =
        {"n_assigned", "n_unassigned", "n_split", "n_dropped"}, counting reads.  Raises CfrkError (CFRK_ERR_LAYOUT, the
        message naming the read) when the hits are not hits on a list of len(comp) unitigs."""
        hit_ptr = np.ascontiguousarray(hit_ptr, np.int64)
        hits = np.ascontiguousarray(hits, READ_HIT_DTYPE)
        comp = np.ascontiguousarray(comp, np.uint32)
        if len(hit_ptr) < 1:
            raise ValueError("hit_ptr is empty")
        nR = len(hit_ptr) - 1
        rows, stats = np.zeros(nR, READ_COMPONENT_DTYPE), np.zeros(1, READ_COMPONENT_STATS_DTYPE)
        self.ctx.check(self._L.cfrk_global_read_components(self.ctx._h, _ptr(hit_ptr), nR, _ptr(hits), len(hits), _ptr(comp), len(comp),
                                                           _ptr(rows), _ptr(stats)), "cfrk_global_read_components")
        return rows, {f: int(stats[f][0]) for f in READ_COMPONENT_STATS_DTYPE.names}

    def read_components_device(self, d_hit_ptr, nR, d_hits, n_hits, d_comp, nS, d_out):
        """device form -> stats; synchronises once, for the counts and the check of the hits"""
        stats = np.zeros(1, READ_COMPONENT_STATS_DTYPE)
        vp = lambda p: C.c_void_p(p) if p else None
        self.ctx.check(self._L.cfrk_global_read_components_device(self.ctx._h, vp(d_hit_ptr), nR, vp(d_hits), n_hits, vp(d_comp), nS,
                                                                  vp(d_out), _ptr(stats)), "cfrk_global_read_components_device")
        return {f: int(stats[f][0]) for f in READ_COMPONENT_STATS_DTYPE.names}

    def drop_small_components(self, min_kmers, min_count=1):
        """drop every component of fewer than min_kmers k-mers from the graph: unitigs -> links -> components, one
        mask_unitigs() call with every unitig of such a component, unitigs again -> ((data, start, length, rec) of what is
        left, (n_components_dropped, n_unitigs_dropped)).  Whole components go, so no remaining unitig gains or loses a
        neighbour: the returned list is the kept unitigs of the first list, byte for byte and in their order."""
        data, start, length, rec = self.unitigs(min_count)
        link_ptr, links = self.unitig_links(data, start, length, min_count)
        comp, table, _ = self.unitig_components(rec, link_ptr, links)
        small = table["n_kmers"] < np.uint64(min_kmers)
        drop = small[comp].astype(np.uint8) if len(comp) else np.zeros(0, np.uint8)
        if drop.any():
            self.mask_unitigs(data, start, length, drop)
        return self.unitigs(min_count), (int(small.sum()), int(drop.sum()))

    def mask_keys(self, keys_lo, keys_hi=None):
        """add keys to the graph mask: a masked key is no longer solid for neighbors(), unitigs(), unitig_links(),
        unitig_index(), locate() and read_hits(); its count is untouched.  Canonicalised in a CFRK_CANONICAL job; a key
        that is not stored or has bits at or above 2k is ignored.  Drops the position map."""
        lo = np.ascontiguousarray(keys_lo, np.uint64)
        hi = None if keys_hi is None else np.ascontiguousarray(keys_hi, np.uint64)
        if hi is not None and len(hi) != len(lo):
            raise ValueError("keys_lo and keys_hi differ in length")
        self.ctx.check(self._L.cfrk_global_mask_keys(self.ctx._h, _ptr(lo), _ptr(hi), len(lo)), "cfrk_global_mask_keys")

    def mask_keys_device(self, d_lo, d_hi, n):
        """device form of mask_keys(): returns with the kernel enqueued on the context stream"""
        vp = lambda p: C.c_void_p(p) if p else None
        self.ctx.check(self._L.cfrk_global_mask_keys_device(self.ctx._h, vp(d_lo), vp(d_hi), n), "cfrk_global_mask_keys_device")

    def mask_unitigs(self, data, start, length, drop):
        """add every k-mer of every unitig j with drop[j] != 0 to the graph mask (any struct-read list; k-mers that are not
        stored and windows with an invalid code are skipped).  Drops the position map."""
        data = np.ascontiguousarray(data, np.int8)
        start = np.ascontiguousarray(start, np.int64)
        length = np.ascontiguousarray(length, np.int32)
        drop = np.ascontiguousarray(drop, np.uint8)
        if len(drop) != len(length):
            raise ValueError("drop and length differ in length")
        self.ctx.check(self._L.cfrk_global_mask_unitigs(self.ctx._h, _ptr(data), _ptr(start), _ptr(length), len(data), len(length),
                                                        _ptr(drop)), "cfrk_global_mask_unitigs")

    def mask_unitigs_device(self, d_data, d_start, d_length, nN, nS, d_drop):
        """device form of mask_unitigs(): one launch over tiles of the bytes, left enqueued on the context stream"""
        vp = lambda p: C.c_void_p(p) if p else None
        self.ctx.check(self._L.cfrk_global_mask_unitigs_device(self.ctx._h, vp(d_data), vp(d_start), vp(d_length), nN, nS, vp(d_drop)),
                       "cfrk_global_mask_unitigs_device")

    def mask_clear(self):
        """unmask every key; fine without a mask"""
        self.ctx.check(self._L.cfrk_global_mask_clear(self.ctx._h), "cfrk_global_mask_clear")

    def mask_count(self):
        """the stored keys that are masked; synchronises"""
        n = C.c_uint64()
        self.ctx.check(self._L.cfrk_global_mask_count(self.ctx._h, C.byref(n)), "cfrk_global_mask_count")
        return n.value

    def unitig_tips(self, rec, link_ptr, links, max_kmers, ratio_q8=512):
        """the tip rule over the unitigs' records and their links, as unitigs() and unitig_links() returned them ->
        np.uint8[nS], 1 where unitig j is a tip: not circular, at most max_kmers k-mers, exactly one dead end, and at an
        attachment a sibling with 256 * mean(sibling) >= ratio_q8 * mean(j) that is no candidate itself or ranks above j.
        Raises CfrkError (CFRK_ERR_LAYOUT, the message naming the unitig) when the rows are not link rows."""
        rec = np.ascontiguousarray(rec, UNITIG_DTYPE)
        link_ptr = np.ascontiguousarray(link_ptr, np.int64)
        links = np.ascontiguousarray(links, UNITIG_LINK_DTYPE)
        if len(link_ptr) != len(rec) + 1:
            raise ValueError("link_ptr has not one entry more than rec")
        tip, n = np.zeros(len(rec), np.uint8), C.c_int64()
        self.ctx.check(self._L.cfrk_global_unitig_tips(self.ctx._h, _ptr(rec), len(rec), _ptr(link_ptr), _ptr(links), len(links),
                                                       int(max_kmers), int(ratio_q8), _ptr(tip), C.byref(n)), "cfrk_global_unitig_tips")
        assert n.value == int(tip.sum())
        return tip

    def unitig_tips_device(self, d_rec, nS, d_link_ptr, d_links, n_links, max_kmers, ratio_q8, d_tip):
        """device form -> n_tips; synchronises once, for n_tips and the check of the rows"""
        n = C.c_int64()
        vp = lambda p: C.c_void_p(p) if p else None
        self.ctx.check(self._L.cfrk_global_unitig_tips_device(self.ctx._h, vp(d_rec), nS, vp(d_link_ptr), vp(d_links), n_links,
                                                              int(max_kmers), int(ratio_q8), vp(d_tip), C.byref(n)),
                       "cfrk_global_unitig_tips_device")
        return n.value

    def clip_tips(self, min_count=1, max_kmers=None, ratio=2.0, rounds=4, recompact=False):
        """clip tips off the graph: up to `rounds` rounds of unitigs -> links -> tips -> mask_unitigs(tips), stopping at the
        first round without a tip -> ((data, start, length, rec) of the clipped graph, [(unitigs, tips, masked keys so
        far) per round]).  max_kmers=None means k; ratio is the mean coverage a sibling must have relative to the tip
        (Minia's convention; 0: topology alone).  The mask stays set: links, the position map and further rounds see
        the clipped graph; mask_clear() brings the full one back.  recompact=True takes the next round's unitigs from
        compact_unitigs() on this round's graph and tips in place of the unitigs() call; the result is the same."""
        if rounds < 1:
            raise ValueError("rounds: at least 1")
        ratio_q8 = int(round(float(ratio) * 256))
        if not 0 <= ratio_q8 <= CFRK_TIP_RATIO_Q8_MAX:
            raise ValueError("ratio: 0 .. 256")
        max_kmers = self.k if max_kmers is None else int(max_kmers)
        report = []
        u = self.unitigs(min_count)
        for _ in range(rounds):
            data, start, length, rec = u
            link_ptr, links = self.unitig_links(data, start, length, min_count)
            tip = self.unitig_tips(rec, link_ptr, links, max_kmers, ratio_q8)
            n_tips = int(tip.sum())
            if n_tips:
                self.mask_unitigs(data, start, length, tip)
            report.append((len(rec), n_tips, self.mask_count()))
            if not n_tips:
                break
            u = self.compact_unitigs(data, start, length, rec, link_ptr, links, tip)[:4] if recompact else self.unitigs(min_count)
        return u, report

    def unitig_bubbles(self, rec, link_ptr, links, max_kmers, max_diff=0, ratio_q8=0):
        """the bubble rule over the unitigs' records and their links -> (pop np.uint8[nS], partner np.uint32[nS]): pop[j] =
        1 where unitig j is an arm (not circular, at most max_kmers k-mers, one link in, one link out, neither to itself)
        and a parallel arm (same source, same target, lengths within max_diff) with 256 * mean(it) >= ratio_q8 * mean(j)
        ranks above it; partner[j] = s << 1 | p names the best such arm and its orientation relative to (j,+),
        CFRK_BUBBLE_NONE where pop[j] = 0.  Raises CfrkError (CFRK_ERR_LAYOUT, the message naming the unitig) when the
        rows are not link rows."""
        rec = np.ascontiguousarray(rec, UNITIG_DTYPE)
        link_ptr = np.ascontiguousarray(link_ptr, np.int64)
        links = np.ascontiguousarray(links, UNITIG_LINK_DTYPE)
        if len(link_ptr) != len(rec) + 1:
            raise ValueError("link_ptr has not one entry more than rec")
        pop, partner, n = np.zeros(len(rec), np.uint8), np.full(len(rec), CFRK_BUBBLE_NONE, np.uint32), C.c_int64()
        self.ctx.check(self._L.cfrk_global_unitig_bubbles(self.ctx._h, _ptr(rec), len(rec), _ptr(link_ptr), _ptr(links), len(links),
                                                          int(max_kmers), int(max_diff), int(ratio_q8), _ptr(pop), _ptr(partner),
                                                          C.byref(n)), "cfrk_global_unitig_bubbles")
        assert n.value == int(pop.sum())
        return pop, partner

    def unitig_bubbles_device(self, d_rec, nS, d_link_ptr, d_links, n_links, max_kmers, max_diff, ratio_q8, d_pop, d_partner=0):
        """device form -> n_pop; d_partner may be 0; synchronises once, for n_pop and the check of the rows"""
        n = C.c_int64()
        vp = lambda p: C.c_void_p(p) if p else None
        self.ctx.check(self._L.cfrk_global_unitig_bubbles_device(self.ctx._h, vp(d_rec), nS, vp(d_link_ptr), vp(d_links), n_links,
                                                                 int(max_kmers), int(max_diff), int(ratio_q8), vp(d_pop),
                                                                 vp(d_partner), C.byref(n)),
                       "cfrk_global_unitig_bubbles_device")
        return n.value

    def unitig_bulges(self, rec, link_ptr, links, max_kmers, max_diff=0, max_hops=None, max_visits=1024, ratio_q8=0):
        """the bulge rule over the unitigs' records and their links -> (pop np.uint8[nS], visits np.uint32[nS], path_ptr
        np.int64[nS + 1], path np.uint32[n_path], stats): pop[j] = 1 where unitig j is an arm of the bubble rule and the
        depth-first search from its source finds a chain of 1 .. max_hops distinct unitigs to its target, each with 256 *
        mean(it) >= ratio_q8 * mean(j) and ranking above j, their k-mers summing to n_j within max_diff.  visits[j] = the
        links the search looked at, max_visits + 1 for an arm it left undecided; row j of the CSR (path_ptr, path) holds
        the first-found path as w << 1 | o; stats = {"arms", "popped", "undecided"}.  max_hops=None means min(max_kmers
        + max_diff, 64).  The default of 1024 for max_visits is a choice with headroom over the 55 that small CPU cases
        needed at k = 31, not a measured optimum.  Raises CfrkError (CFRK_ERR_LAYOUT, the message naming the unitig) when
        the rows are not link rows.  A sizes-only call, then the call into an array of exactly that size."""
        rec = np.ascontiguousarray(rec, UNITIG_DTYPE)
        link_ptr = np.ascontiguousarray(link_ptr, np.int64)
        links = np.ascontiguousarray(links, UNITIG_LINK_DTYPE)
        if len(link_ptr) != len(rec) + 1:
            raise ValueError("link_ptr has not one entry more than rec")
        max_hops = min(int(max_kmers) + int(max_diff), CFRK_BULGE_MAX_HOPS) if max_hops is None else int(max_hops)
        nS, n = len(rec), C.c_int64()
        pop, visits, path_ptr = np.zeros(nS, np.uint8), np.zeros(nS, np.uint32), np.zeros(nS + 1, np.int64)
        stats = np.zeros(1, BULGE_STATS_DTYPE)
        args = (self.ctx._h, _ptr(rec), nS, _ptr(link_ptr), _ptr(links), len(links), int(max_kmers), int(max_diff), max_hops,
                int(max_visits), int(ratio_q8), _ptr(pop), _ptr(visits), _ptr(path_ptr))
        rc = self._L.cfrk_global_unitig_bulges(*args, None, 0, C.byref(n), _ptr(stats))
        if rc != CFRK_ERR_SMALL_BUF:
            self.ctx.check(rc, "cfrk_global_unitig_bulges")
        path = np.zeros(n.value, np.uint32)
        if rc == CFRK_ERR_SMALL_BUF:
            self.ctx.check(self._L.cfrk_global_unitig_bulges(*args, _ptr(path), path.size, C.byref(n), _ptr(stats)),
                           "cfrk_global_unitig_bulges")
        assert int(stats["popped"][0]) == int(pop.sum()) and n.value == int(path_ptr[nS])
        return pop, visits, path_ptr, path, {f: int(stats[f][0]) for f in BULGE_STATS_DTYPE.names}

    def unitig_bulges_device(self, d_rec, nS, d_link_ptr, d_links, n_links, max_kmers, max_diff, max_hops, max_visits, ratio_q8, d_pop,
                             d_visits=0, d_path_ptr=0, d_path=0, cap_path=0):
        """device form -> (n_path, stats); d_visits may be 0; d_path_ptr may be 0 (no paths wanted); d_path may be 0 with
        cap_path 0 (sizes only).  Raises CfrkError (code CFRK_ERR_SMALL_BUF, with .n_path and .stats set, d_pop, d_visits
        and d_path_ptr complete, nothing written to d_path) when cap_path is too small.  Synchronises once, returns with
        the pass that writes d_path enqueued on the context stream."""
        n, stats = C.c_int64(), np.zeros(1, BULGE_STATS_DTYPE)
        vp = lambda p: C.c_void_p(p) if p else None
        rc = self._L.cfrk_global_unitig_bulges_device(self.ctx._h, vp(d_rec), nS, vp(d_link_ptr), vp(d_links), n_links, int(max_kmers),
                                                      int(max_diff), int(max_hops), int(max_visits), int(ratio_q8), vp(d_pop),
                                                      vp(d_visits), vp(d_path_ptr), vp(d_path), cap_path, C.byref(n), _ptr(stats))
        st = {f: int(stats[f][0]) for f in BULGE_STATS_DTYPE.names}
        try:
            self.ctx.check(rc, "cfrk_global_unitig_bulges_device")
        except CfrkError as e:
            e.n_path, e.stats = n.value, st
            raise
        return n.value, st

    def unitig_weak(self, rec, link_ptr, links, max_kmers, ratio_q8=1024, iso_max_kmers=0, iso_mean_q8=0):
        """the weak rule over the unitigs' records and their links -> (weak np.uint8[nS], stats): weak[j] =
        CFRK_WEAK_CONNECTION where unitig j is not circular, has at most max_kmers k-mers, a link at both ends and none
        to itself, and at every one of those links a sibling (another way out of the same neighbour's end) with 256 *
        mean(it) >= ratio_q8 * mean(j) that ranks above j; CFRK_WEAK_ISOLATED where it is not circular, has no link at
        all, at most iso_max_kmers k-mers and 256 * mean(j) < iso_mean_q8; 0 elsewhere.  stats = {"connections",
        "isolated", "candidates"}.  At equal max_kmers and ratio_q8 this contains everything unitig_bubbles() pops, so the
        default ratio_q8 of 1024 (four times the coverage) is deliberately high; like the isolated thresholds' default of
        0 (off) it is a choice, not a measured optimum.  Raises CfrkError (CFRK_ERR_LAYOUT, the message naming the unitig)
        when the rows are not link rows."""
        rec = np.ascontiguousarray(rec, UNITIG_DTYPE)
        link_ptr = np.ascontiguousarray(link_ptr, np.int64)
        links = np.ascontiguousarray(links, UNITIG_LINK_DTYPE)
        if len(link_ptr) != len(rec) + 1:
            raise ValueError("link_ptr has not one entry more than rec")
        weak, stats = np.zeros(len(rec), np.uint8), np.zeros(1, WEAK_STATS_DTYPE)
        self.ctx.check(self._L.cfrk_global_unitig_weak(self.ctx._h, _ptr(rec), len(rec), _ptr(link_ptr), _ptr(links), len(links),
                                                       int(max_kmers), int(ratio_q8), int(iso_max_kmers), int(iso_mean_q8), _ptr(weak),
                                                       _ptr(stats)), "cfrk_global_unitig_weak")
        st = {f: int(stats[f][0]) for f in WEAK_STATS_DTYPE.names}
        assert st["connections"] == int((weak == CFRK_WEAK_CONNECTION).sum()) and st["isolated"] == int((weak == CFRK_WEAK_ISOLATED).sum())
        return weak, st

    def unitig_weak_device(self, d_rec, nS, d_link_ptr, d_links, n_links, max_kmers, ratio_q8, iso_max_kmers, iso_mean_q8, d_weak):
        """device form -> stats; synchronises once, for the counts and the check of the rows"""
        stats = np.zeros(1, WEAK_STATS_DTYPE)
        vp = lambda p: C.c_void_p(p) if p else None
        self.ctx.check(self._L.cfrk_global_unitig_weak_device(self.ctx._h, vp(d_rec), nS, vp(d_link_ptr), vp(d_links), n_links,
                                                              int(max_kmers), int(ratio_q8), int(iso_max_kmers), int(iso_mean_q8),
                                                              vp(d_weak), _ptr(stats)), "cfrk_global_unitig_weak_device")
        return {f: int(stats[f][0]) for f in WEAK_STATS_DTYPE.names}

    def compact_unitigs(self, data, start, length, rec, link_ptr, links, drop=None):
        """the unitigs of the graph without the unitigs j with drop[j] != 0, from the list, its records and its links as
        unitigs() and unitig_links() returned them -> (data, start, length, rec, into): byte for byte what unitigs()
        returns after mask_unitigs(drop), without the k-mer passes; into UNITIG_POS_DTYPE[nS] says where input unitig j
        went: the new index and at = off << 1 | minus (mod n_kmers in a circular unitig), both words CFRK_POS_NONE for a
        dropped one.  drop=None drops nothing.  The job only supplies k and the strand rule.  Raises CfrkError
        (CFRK_ERR_LAYOUT, the message naming the unitig) when the arrays are not a unitig list with its links.  A
        sizes-only call, then the call into arrays of exactly that size."""
        data = np.ascontiguousarray(data, np.int8)
        start = np.ascontiguousarray(start, np.int64)
        length = np.ascontiguousarray(length, np.int32)
        rec = np.ascontiguousarray(rec, UNITIG_DTYPE)
        link_ptr = np.ascontiguousarray(link_ptr, np.int64)
        links = np.ascontiguousarray(links, UNITIG_LINK_DTYPE)
        drop = None if drop is None else np.ascontiguousarray(drop, np.uint8)
        nS = len(rec)
        if len(start) != nS or len(length) != nS or len(link_ptr) != nS + 1 or (drop is not None and len(drop) != nS):
            raise ValueError("start, length, rec and drop have one entry per unitig, link_ptr one more")
        into = np.full(nS, CFRK_POS_NONE, UNITIG_POS_DTYPE)      # (both words)
        head = (self.ctx._h, _ptr(data), _ptr(start), _ptr(length), _ptr(rec), len(data), nS, _ptr(link_ptr), _ptr(links), len(links), _ptr(drop))
        nN, n = C.c_int64(), C.c_int64()
        rc = self._L.cfrk_global_unitigs_compact(*head, None, 0, None, None, None, 0, None, C.byref(nN), C.byref(n))
        if rc != CFRK_ERR_SMALL_BUF:
            self.ctx.check(rc, "cfrk_global_unitigs_compact")
        out, ostart = np.empty(nN.value, np.int8), np.empty(n.value, np.int64)
        olength, orec = np.empty(n.value, np.int32), np.zeros(n.value, UNITIG_DTYPE)
        if rc == CFRK_ERR_SMALL_BUF:
            self.ctx.check(self._L.cfrk_global_unitigs_compact(*head, _ptr(out), out.size, _ptr(ostart), _ptr(olength), _ptr(orec), orec.size,
                                                               _ptr(into), C.byref(nN), C.byref(n)), "cfrk_global_unitigs_compact")
        return out, ostart, olength, orec, into

    def compact_unitigs_device(self, d_data, d_start, d_length, d_rec, nN, nS, d_link_ptr, d_links, n_links, d_drop, d_data_out, cap_data,
                               d_start_out, d_length_out, d_rec_out, cap_unitigs, d_into=0):
        """device form -> (nN, nS) of the result; d_drop may be 0 (nothing dropped), d_into may be 0, the output arrays may be
        0 with zero capacities (sizes only).  Raises CfrkError (code CFRK_ERR_SMALL_BUF, with .nN and .nS set, nothing
        written) when they are too small.  Synchronises once, returns with the order and the emit enqueued on the context
        stream."""
        nN_out, nS_out = C.c_int64(), C.c_int64()
        vp = lambda p: C.c_void_p(p) if p else None
        rc = self._L.cfrk_global_unitigs_compact_device(self.ctx._h, vp(d_data), vp(d_start), vp(d_length), vp(d_rec), nN, nS, vp(d_link_ptr),
                                                        vp(d_links), n_links, vp(d_drop), vp(d_data_out), cap_data, vp(d_start_out),
                                                        vp(d_length_out), vp(d_rec_out), cap_unitigs, vp(d_into), C.byref(nN_out),
                                                        C.byref(nS_out))
        try:
            self.ctx.check(rc, "cfrk_global_unitigs_compact_device")
        except CfrkError as e:
            e.nN, e.nS = nN_out.value, nS_out.value
            raise
        return nN_out.value, nS_out.value

    def simplify(self, min_count=1, tips=True, bubbles=True, rounds=4, tip_max_kmers=None, tip_ratio=2.0,
                 bubble_max_kmers=None, bubble_max_diff=0, bubble_ratio=0.0, bulges=False, bulge_max_kmers=None, bulge_max_diff=0,
                 bulge_max_hops=None, bulge_max_visits=1024, bulge_ratio=0.0, recompact=False, weak=False, weak_max_kmers=None,
                 weak_ratio=4.0, weak_iso_max_kmers=None, weak_iso_mean=2.0):
        """simplify the graph: up to `rounds` rounds of unitigs -> links -> each enabled rule on that same graph -> one
        mask_unitigs(tip | pop), stopping at the first round that finds neither a tip nor a bubble -> ((data, start,
        length, rec) of the simplified graph, [(unitigs, tips, bubbles, masked keys so far) per round], [(round, popped
        unitig, partner, popped record, partner's record, popped sequence, partner's sequence oriented like the popped
        one) per popped unitig]).  tip_* as clip_tips(); bubble_max_kmers=None means k; bubble_ratio is the mean coverage
        the stronger arm must have relative to the popped one: the default 0 pops the weaker arm whatever the coverages
        are (a choice, not a measured optimum); 2.0 leaves a balanced heterozygous site alone.  The mask stays set, as
        after clip_tips().
        bulges=True runs the bulge rule on that same graph as well (unitig_bulges(); bulge_max_kmers=None means k,
        bulge_max_hops=None means min(bulge_max_kmers + bulge_max_diff, 64), bulge_ratio as bubble_ratio; the default of
        1024 for bulge_max_visits is a choice with headroom, not a measured optimum) and masks tip | pop | bulge in the
        one call per round.  The per-round tuples are then (unitigs, tips, bubbles, bulges, masked keys so far), and a
        fourth value is returned: [(round, popped unitig, path as a list of w << 1 | o, popped record, popped sequence,
        the path's sequence spelled with k - 1 overlaps) per unitig the bulge rule popped].
        weak=True runs the weak rule on that same graph as well (unitig_weak(); weak_max_kmers=None means k,
        weak_iso_max_kmers=None means 2 k, weak_ratio is the mean coverage a sibling must have relative to the
        connection, weak_iso_mean the mean coverage below which an isolated unitig goes) and masks tip | pop | bulge |
        (weak != 0) in the one call per round.  The rule contains the bubble rule at an equal ratio, hence the high default
        of 4.0; that, 2.0 and 2 k are choices, not measured optima.  The per-round tuples then end in two more counts,
        (..., masked keys so far, connections, isolated), the loop stops at the first round in which no enabled rule
        finds anything, and one more value is returned last: [(round, unitig, CFRK_WEAK_CONNECTION or CFRK_WEAK_ISOLATED,
        record, sequence) per unitig the weak rule dropped].
        recompact=True takes the next round's unitigs from compact_unitigs() on this round's graph and drop bytes in
        place of the unitigs() call; mask_unitigs() still runs (links and the position map live on the mask).  Every
        returned value is the same either way."""
        if rounds < 1:
            raise ValueError("rounds: at least 1")
        tip_q8, bub_q8 = int(round(float(tip_ratio) * 256)), int(round(float(bubble_ratio) * 256))
        bulge_q8 = int(round(float(bulge_ratio) * 256))
        weak_q8, weak_iso_q8 = int(round(float(weak_ratio) * 256)), int(round(float(weak_iso_mean) * 256))
        if weak and (not 0 <= weak_q8 <= CFRK_TIP_RATIO_Q8_MAX or not 0 <= weak_iso_q8 <= 0xFFFFFFFF):
            raise ValueError("weak_ratio: 0 .. 256; weak_iso_mean: 0 .. 2^24")
        weak_max_kmers = self.k if weak_max_kmers is None else int(weak_max_kmers)
        weak_iso_max_kmers = 2 * self.k if weak_iso_max_kmers is None else int(weak_iso_max_kmers)
        if not 0 <= tip_q8 <= CFRK_TIP_RATIO_Q8_MAX or not 0 <= bub_q8 <= CFRK_TIP_RATIO_Q8_MAX or not 0 <= bulge_q8 <= CFRK_TIP_RATIO_Q8_MAX:
            raise ValueError("ratio: 0 .. 256")
        tip_max_kmers = self.k if tip_max_kmers is None else int(tip_max_kmers)
        bubble_max_kmers = self.k if bubble_max_kmers is None else int(bubble_max_kmers)
        bulge_max_kmers = self.k if bulge_max_kmers is None else int(bulge_max_kmers)
        text = lambda data, at, n: "".join("ACGT"[c] for c in data[at:at + n])
        comp = str.maketrans("ACGT", "TGCA")
        report, rows, bulge_rows, weak_rows = [], [], [], []
        u = self.unitigs(min_count)
        for rnd in range(1, rounds + 1):
            data, start, length, rec = u
            link_ptr, links = self.unitig_links(data, start, length, min_count)
            drop = np.zeros(len(rec), np.uint8)
            n_tips = n_pop = n_bulge = n_conn = n_iso = 0
            if tips:
                tip = self.unitig_tips(rec, link_ptr, links, tip_max_kmers, tip_q8)
                n_tips = int(tip.sum())
                drop |= tip
            if bubbles:
                pop, partner = self.unitig_bubbles(rec, link_ptr, links, bubble_max_kmers, bubble_max_diff, bub_q8)
                n_pop = int(pop.sum())
                drop |= pop
                for j in np.flatnonzero(pop).tolist():
                    s, p = int(partner[j]) >> 1, int(partner[j]) & 1
                    kept = text(data, int(start[s]), int(length[s]))
                    rows.append((rnd, j, int(partner[j]), tuple(rec[j].tolist()), tuple(rec[s].tolist()),
                                 text(data, int(start[j]), int(length[j])), kept.translate(comp)[::-1] if p else kept))
            if bulges:
                bulge, _, path_ptr, path, _ = self.unitig_bulges(rec, link_ptr, links, bulge_max_kmers, bulge_max_diff, bulge_max_hops,
                                                                 bulge_max_visits, bulge_q8)
                n_bulge = int(bulge.sum())
                drop |= bulge
                for j in np.flatnonzero(bulge).tolist():
                    p = path[path_ptr[j]:path_ptr[j + 1]].tolist()
                    spelled = ""
                    for w in p:
                        s = text(data, int(start[w >> 1]), int(length[w >> 1]))
                        s = s.translate(comp)[::-1] if w & 1 else s
                        spelled += s[self.k - 1:] if spelled else s
                    bulge_rows.append((rnd, j, p, tuple(rec[j].tolist()), text(data, int(start[j]), int(length[j])), spelled))
            if weak:
                wk, st = self.unitig_weak(rec, link_ptr, links, weak_max_kmers, weak_q8, weak_iso_max_kmers, weak_iso_q8)
                n_conn, n_iso = st["connections"], st["isolated"]
                drop |= (wk != 0).astype(np.uint8)
                for j in np.flatnonzero(wk).tolist():
                    weak_rows.append((rnd, j, int(wk[j]), tuple(rec[j].tolist()), text(data, int(start[j]), int(length[j]))))
            found = n_tips or n_pop or n_bulge or n_conn or n_iso
            if found:
                self.mask_unitigs(data, start, length, drop)
            row = (len(rec), n_tips, n_pop, n_bulge, self.mask_count()) if bulges else (len(rec), n_tips, n_pop, self.mask_count())
            report.append(row + (n_conn, n_iso) if weak else row)
            if not found:
                break
            u = self.compact_unitigs(data, start, length, rec, link_ptr, links, drop)[:4] if recompact else self.unitigs(min_count)
        out = (u, report, rows, bulge_rows) if bulges else (u, report, rows)
        return out + (weak_rows,) if weak else out

    def query_reads(self, data, start=None, length=None):
        """count of the k-mer starting at every base -> np.uint32[nN]: CFRK_QUERY_NONE where the window holds an
        invalid base or runs past the end, 0 where the k-mer is absent"""
        data = np.ascontiguousarray(data, np.int8)
        if start is not None:
            start = np.ascontiguousarray(start, np.int64)
            length = np.ascontiguousarray(length, np.int32)
        nS = 0 if length is None else len(length)
        out = np.empty(len(data), np.uint32)
        self.ctx.check(self._L.cfrk_global_query_reads(self.ctx._h, _ptr(data), _ptr(start), _ptr(length),
                                                       len(data), nS, _ptr(out)), "cfrk_global_query_reads")
        return out

    def query_reads_device(self, d_data, nN, d_out):
        """device form of query_reads(): d_data 16-byte aligned, d_out nN uint32; returns with the kernel enqueued"""
        self.ctx.check(self._L.cfrk_global_query_reads_device(self.ctx._h, C.c_void_p(d_data) if d_data else None,
                                                              nN, C.c_void_p(d_out) if d_out else None),
                       "cfrk_global_query_reads_device")

    def read_stats(self, data, start, length, threshold=0):
        """per-read abundance statistics against the job's result -> np.ndarray[nS] of READ_STATS_DTYPE: valid
        windows, how many of their k-mers are present / counted below `threshold`, and min, lower median, max and sum
        of their counts; a read without a valid window gives an all-zero row"""
        data = np.ascontiguousarray(data, np.int8)
        start = np.ascontiguousarray(start, np.int64)
        length = np.ascontiguousarray(length, np.int32)
        nS = len(length)
        if len(start) != nS:
            raise ValueError("start and length differ in size")
        if not 0 <= int(threshold) <= 0xFFFFFFFF:
            raise ValueError("threshold outside 0 .. 2^32 - 1")
        out = np.zeros(nS, READ_STATS_DTYPE)
        self.ctx.check(self._L.cfrk_global_read_stats(self.ctx._h, _ptr(data), _ptr(start), _ptr(length), len(data), nS,
                                                      int(threshold), _ptr(out)), "cfrk_global_read_stats")
        return out

    def read_stats_device(self, d_data, d_start, d_length, nN, nS, threshold, d_out):
        """device form of read_stats(): d_out nS rows of 32 bytes; no alignment requirement on d_data; returns with
        the last kernel enqueued on the context stream"""
        vp = lambda p: C.c_void_p(p) if p else None
        self.ctx.check(self._L.cfrk_global_read_stats_device(self.ctx._h, vp(d_data), vp(d_start), vp(d_length), nN, nS,
                                                             int(threshold), vp(d_out)),
                       "cfrk_global_read_stats_device")

    def read_spans(self, data, start, length, min_count=1, max_count=CFRK_COUNT_MAX, mode=CFRK_SPAN_LONGEST):
        """the solid span of every read against the job's result -> np.ndarray[nS] of READ_SPAN_DTYPE: the bases that
        a run of windows with min_count <= count <= max_count covers -- the longest run (CFRK_SPAN_LONGEST, the
        earliest on a tie) or the run that begins at window 0 (CFRK_SPAN_PREFIX); {0, 0} when there is none"""
        data = np.ascontiguousarray(data, np.int8)
        start = np.ascontiguousarray(start, np.int64)
        length = np.ascontiguousarray(length, np.int32)
        nS = len(length)
        if len(start) != nS:
            raise ValueError("start and length differ in size")
        if not (0 <= int(min_count) <= 0xFFFFFFFF and 0 <= int(max_count) <= 0xFFFFFFFF):
            raise ValueError("count bound outside 0 .. 2^32 - 1")
        out = np.zeros(nS, READ_SPAN_DTYPE)
        self.ctx.check(self._L.cfrk_global_read_spans(self.ctx._h, _ptr(data), _ptr(start), _ptr(length), len(data), nS,
                                                      int(min_count), int(max_count), int(mode), _ptr(out)),
                       "cfrk_global_read_spans")
        return out

    def read_spans_device(self, d_data, d_start, d_length, nN, nS, min_count, max_count, mode, d_out):
        """device form of read_spans(): d_out nS spans of 8 bytes; no alignment requirement on d_data; returns with
        the last kernel enqueued on the context stream"""
        vp = lambda p: C.c_void_p(p) if p else None
        self.ctx.check(self._L.cfrk_global_read_spans_device(self.ctx._h, vp(d_data), vp(d_start), vp(d_length), nN, nS,
                                                             int(min_count), int(max_count), int(mode), vp(d_out)),
                       "cfrk_global_read_spans_device")

    def correct_reads(self, data, start, length, min_count):
        """spectral correction of substitution errors against the job's result -> (data_out, fix): data_out is data with
        the base written back wherever one wrong base explains an isolated run of weak windows (count < min_count) and
        exactly one other base makes all of them solid; fix is np.ndarray[nS] of READ_FIX_DTYPE, the weak runs of every
        read that were corrected / left alone.  The rule is in include/cfrk_abi.h; the job is only read."""
        data = np.ascontiguousarray(data, np.int8)
        start = np.ascontiguousarray(start, np.int64)
        length = np.ascontiguousarray(length, np.int32)
        nS = len(length)
        if len(start) != nS:
            raise ValueError("start and length differ in size")
        if not 0 <= int(min_count) <= 0xFFFFFFFF:
            raise ValueError("min_count outside 0 .. 2^32 - 1")
        out = np.empty_like(data)
        fix = np.zeros(nS, READ_FIX_DTYPE)
        self.ctx.check(self._L.cfrk_global_correct_reads(self.ctx._h, _ptr(data), _ptr(start), _ptr(length), len(data), nS,
                                                         int(min_count), _ptr(out), _ptr(fix)),
                       "cfrk_global_correct_reads")
        return out, fix

    def correct_reads_device(self, d_data, d_start, d_length, nN, nS, min_count, d_data_out, d_fix=None):
        """device form of correct_reads(): d_data_out nN bytes that do not overlap d_data, d_fix nS rows of 8 bytes or
        None; no alignment requirement; returns with the copy and the last kernel enqueued on the context stream"""
        vp = lambda p: C.c_void_p(p) if p else None
        self.ctx.check(self._L.cfrk_global_correct_reads_device(self.ctx._h, vp(d_data), vp(d_start), vp(d_length), nN, nS,
                                                                int(min_count), vp(d_data_out), vp(d_fix)),
                       "cfrk_global_correct_reads_device")

    def normalize(self, data, start, length, cutoff, batch_reads=CFRK_NORMALIZE_BATCH):
        """digital normalisation (normalize-by-median) -> (keep, n_kept): the reads are taken in rounds of batch_reads;
        a read is kept (keep[i] = 1) iff it has a valid window and the lower median of its windows' counts in the job,
        as it stands at the beginning of the read's round, is below `cutoff`; only kept reads are counted into the job"""
        data = np.ascontiguousarray(data, np.int8)
        start = np.ascontiguousarray(start, np.int64)
        length = np.ascontiguousarray(length, np.int32)
        nS = len(length)
        if len(start) != nS:
            raise ValueError("start and length differ in size")
        if not 0 <= int(cutoff) <= 0xFFFFFFFF:
            raise ValueError("cutoff outside 0 .. 2^32 - 1")
        keep = np.zeros(nS, np.uint8)
        n = C.c_int64(0)
        self.ctx.check(self._L.cfrk_global_normalize(self.ctx._h, _ptr(data), _ptr(start), _ptr(length), len(data), nS,
                                                     int(cutoff), int(batch_reads), _ptr(keep), C.byref(n)),
                       "cfrk_global_normalize")
        return keep, int(n.value)

    def normalize_device(self, d_data, d_start, d_length, nN, nS, cutoff, d_keep, batch_reads=CFRK_NORMALIZE_BATCH):
        """device form of normalize(): d_keep nS bytes; no alignment requirement; every round is enqueued on the
        context stream, one synchronisation at the end; returns the number of kept reads"""
        vp = lambda p: C.c_void_p(p) if p else None
        n = C.c_int64(0)
        self.ctx.check(self._L.cfrk_global_normalize_device(self.ctx._h, vp(d_data), vp(d_start), vp(d_length), nN, nS,
                                                            int(cutoff), int(batch_reads), vp(d_keep), C.byref(n)),
                       "cfrk_global_normalize_device")
        return int(n.value)

    def normalize_pairs(self, data, start, length, cutoff, batch_reads=CFRK_NORMALIZE_BATCH, mode=CFRK_PAIR_EITHER):
        """normalize() for interleaved paired-end reads (mates 2j and 2j + 1) -> (keep, n_kept): every mate is judged on
        its own, then the pair is kept or dropped as a whole -- kept if either mate would be (CFRK_PAIR_EITHER, khmer's
        --paired rule) or only if both would be (CFRK_PAIR_BOTH) -- and every kept read is counted into the job.  The
        number of reads and batch_reads must be even."""
        data = np.ascontiguousarray(data, np.int8)
        start = np.ascontiguousarray(start, np.int64)
        length = np.ascontiguousarray(length, np.int32)
        nS = len(length)
        if len(start) != nS:
            raise ValueError("start and length differ in size")
        if not 0 <= int(cutoff) <= 0xFFFFFFFF:
            raise ValueError("cutoff outside 0 .. 2^32 - 1")
        keep = np.zeros(nS, np.uint8)
        n = C.c_int64(0)
        self.ctx.check(self._L.cfrk_global_normalize_pairs(self.ctx._h, _ptr(data), _ptr(start), _ptr(length), len(data), nS,
                                                           int(cutoff), int(batch_reads), int(mode), _ptr(keep), C.byref(n)),
                       "cfrk_global_normalize_pairs")
        return keep, int(n.value)

    def normalize_pairs_device(self, d_data, d_start, d_length, nN, nS, cutoff, d_keep, batch_reads=CFRK_NORMALIZE_BATCH,
                               mode=CFRK_PAIR_EITHER):
        """device form of normalize_pairs(): as normalize_device(), one join launch more per round; returns the number of
        kept reads (even)"""
        vp = lambda p: C.c_void_p(p) if p else None
        n = C.c_int64(0)
        self.ctx.check(self._L.cfrk_global_normalize_pairs_device(self.ctx._h, vp(d_data), vp(d_start), vp(d_length), nN, nS,
                                                                  int(cutoff), int(batch_reads), int(mode), vp(d_keep), C.byref(n)),
                       "cfrk_global_normalize_pairs_device")
        return int(n.value)

    def export_device(self, d_lo, d_hi, d_cnt, cap, parts=1):
        pc = (C.c_uint64 * parts)()
        self.ctx.check(self._L.cfrk_global_export_device(self.ctx._h, C.c_void_p(d_lo),
                                                         C.c_void_p(d_hi) if d_hi else None,
                                                         C.c_void_p(d_cnt), cap, parts, pc),
                       "cfrk_global_export_device")
        return [int(x) for x in pc]


class Read:
    """Mirror of `struct read` (src/tipos.h:23-30): data / length / start in, Freq out."""

    def __init__(self, data, length, start):
        self.data = np.ascontiguousarray(data, np.int8)
        self.length = np.ascontiguousarray(length, np.int32)
        self.start = np.ascontiguousarray(start, np.int64)
        self.Freq = None


_default_ctx = {}


def kmer_main(rd, nN, nS, k, device=0, flags=CFRK_COMPAT):
    """Drop-in mirror of kmer_main (src/kmer_main.cu:20): fills rd.Freq (nS x 4^k int32).

    Same argument meaning as the reference; errors raise CfrkError instead of printing and
    continuing (src/kmer_main.cu:59-63) or exit(1) (src/kmer_main.cu:51-56)."""
    if nN != len(rd.data) or nS != len(rd.length):
        raise ValueError("nN / nS do not match the buffers")
    ctx = _default_ctx.get(device)
    if ctx is None:
        ctx = _default_ctx[device] = Context(device)
    rd.Freq = ctx.per_read_dense(rd.data, rd.start, rd.length, k, flags).reshape(-1)
    return rd
