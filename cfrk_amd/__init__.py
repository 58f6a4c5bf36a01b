"""cfrk_amd -- MI355X-native k-mer counting behind the reference's kmer_main() boundary.

The compute lives in libcfrk_hip.so (hand-written HIP for gfx950, C ABI in
include/cfrk_abi.h); this package is the thin host-side mirror used by tests, bench.py and
Python callers.  There is NO CPU fallback: if the HIP library is missing or no gfx950 device
is present, every compute entry point raises.
"""
from .lib import (CFRK_CANONICAL, CFRK_COMPAT, CFRK_COUNT_MAX, CFRK_ERR_COUNT_OVERFLOW, CFRK_QUERY_NONE, CFRK_ERR_RUNS_REFUSED, CFRK_ERR_SMALL_BUF, CFRK_SPARSE_FAST_WINDOWS, CFRK_STATS_FAST_WINDOWS, READ_STATS_DTYPE, CFRK_SPAN_PREFIX, CFRK_SPAN_LONGEST, CFRK_SPANS_FAST_WINDOWS, READ_SPAN_DTYPE, CFRK_SELECT_TILE_BYTES, CFRK_SELECT_TILE_READS, CFRK_SELECT_SCAN_TILES, CFRK_TEXT_FASTA, CFRK_TEXT_FASTQ, CFRK_TEXT_TILE_BYTES, CFRK_TEXT_SCAN_TILES, CFRK_EMIT_TILE_BYTES, TEXT_RECORD_DTYPE, CFRK_DEBUG_FORCE_RT_OVERFLOW, CFRK_DEBUG_NO_PIPELINE, CFRK_DEBUG_NO_RADIX16, CFRK_DEBUG_SMALL_PIPELINE, CFRK_DEBUG_SMALL_WAVE_CAP, CFRK_FLOAT_INDEX, CFRK_FORCE_HASH, CFRK_RUNS_DEFER, CFRK_RUNS_ONLY, CFRK_SKETCH_LOG2M, CFRK_SKETCH_REGS, CfrkError, Context, GlobalCounter, Read,
                  abi_symbols, device_count, hash_info, kmer_main, load_library, library_path,
                  sketch_estimate, sketch_hint, sketch_merge)

__all__ = ["CFRK_CANONICAL", "CFRK_COMPAT", "CFRK_COUNT_MAX", "CFRK_ERR_COUNT_OVERFLOW", "CFRK_QUERY_NONE", "CFRK_ERR_RUNS_REFUSED", "CFRK_ERR_SMALL_BUF", "CFRK_SPARSE_FAST_WINDOWS", "CFRK_STATS_FAST_WINDOWS", "READ_STATS_DTYPE", "CFRK_SPAN_PREFIX", "CFRK_SPAN_LONGEST", "CFRK_SPANS_FAST_WINDOWS", "READ_SPAN_DTYPE", "CFRK_SELECT_TILE_BYTES", "CFRK_SELECT_TILE_READS", "CFRK_SELECT_SCAN_TILES", "CFRK_TEXT_FASTA", "CFRK_TEXT_FASTQ", "CFRK_TEXT_TILE_BYTES", "CFRK_TEXT_SCAN_TILES", "CFRK_EMIT_TILE_BYTES", "TEXT_RECORD_DTYPE", "CFRK_DEBUG_FORCE_RT_OVERFLOW", "CFRK_DEBUG_NO_PIPELINE", "CFRK_DEBUG_NO_RADIX16", "CFRK_DEBUG_SMALL_PIPELINE", "CFRK_DEBUG_SMALL_WAVE_CAP", "CFRK_FLOAT_INDEX", "CFRK_FORCE_HASH", "CFRK_RUNS_DEFER", "CFRK_RUNS_ONLY", "CFRK_SKETCH_LOG2M", "CFRK_SKETCH_REGS", "CfrkError", "Context", "GlobalCounter", "Read",
           "abi_symbols", "device_count", "hash_info", "kmer_main", "load_library", "library_path",
           "sketch_estimate", "sketch_hint", "sketch_merge"]
