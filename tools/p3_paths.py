#!/usr/bin/env python3
"""Path counters of the leaf kernel (msp.hip: P3C_*) over one bench run: how many leaves would take one, two or three
lanes per run by the number of runs alone, how many wave-calls of the complete runs' expansion leave the one-walk path of
the noted lengths, how many of that expansion's keys claim an empty slot of the k-mer table against how many find their
key there, and how many entries of the record table have their reverse complement in it too.

The counters exist in an ABLATION BUILD only (`make -C cfrk_amd/csrc abl`), which must be installed as
cfrk_amd/libcfrk_hip.so for the run (tools/ablate.sh shows how to swap it in and back), and there only with the debug
bit CFRK_ABL_P3_PATHS, which this tool sets: they are global atomics, so the run's times mean nothing.  --old adds
CFRK_ABL_P3_OLD_CEXP: the expansion as it was before every canonical leaf took three lanes per run (both bits count
right, unlike the timing ablations).

usage (GPU box, repo root): python tools/p3_paths.py [--old] [bench args, default: --reads 20000000 --steps 1 --warmup 0 --cpu-reads 0]"""
import ctypes
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["leaves_1_lane", "leaves_2_lanes", "leaves_3_lanes", "cexp_wave_calls_with_notes", "cexp_wave_calls_slow_walk",
         "cexp_keys_claimed", "cexp_keys_matched", "rt_entries", "rt_entries_with_twin", "rt_entries_palindromic"]
CFRK_ABL_P3_OLD_CEXP, CFRK_ABL_P3_PATHS = 0x8000, 0x800000     # cfrk_amd/csrc/msp.h


def main():
    args = sys.argv[1:]
    old = "--old" in args
    args = [x for x in args if x != "--old"] or ["--reads", "20000000", "--steps", "1", "--warmup", "0", "--cpu-reads", "0"]
    sys.path.insert(0, ROOT)
    import cfrk_amd
    # (the library is opened only behind the run: bench.py imports torch first, whose HIP runtime the library then shares)
    if b"cfrk_debug_p3_paths" not in open(cfrk_amd.library_path(), "rb").read():
        raise SystemExit("cfrk_amd/libcfrk_hip.so is not an ablation build: it has no path counters")
    os.environ["CFRK_DEBUG_FLAGS"] = hex(int(os.environ.get("CFRK_DEBUG_FLAGS", "0"), 0) | CFRK_ABL_P3_PATHS |
                                         (CFRK_ABL_P3_OLD_CEXP if old else 0))
    sys.argv = [os.path.join(ROOT, "bench.py")] + args
    try:
        runpy.run_path(sys.argv[0], run_name="__main__")
    except SystemExit as e:
        if e.code not in (None, 0):
            raise
    lib = ctypes.CDLL(cfrk_amd.library_path())
    out = (ctypes.c_uint64 * len(NAMES))()
    rc = lib.cfrk_debug_p3_paths(out, len(NAMES), 1)
    if rc:
        raise SystemExit("cfrk_debug_p3_paths: %d" % rc)
    c = dict(zip(NAMES, (int(x) for x in out)))
    print("leaf kernel path counters (%s expansion), bench %s" % ("old" if old else "new", " ".join(args)))
    for n in NAMES:
        print("  %-28s %d" % (n, c[n]))
    leaves = c["leaves_1_lane"] + c["leaves_2_lanes"] + c["leaves_3_lanes"]
    keys = c["cexp_keys_claimed"] + c["cexp_keys_matched"]
    if leaves and keys and c["rt_entries"] and c["cexp_wave_calls_with_notes"]:
        print("  leaves below three lanes per run by their number of runs: %.1f %%" % (100.0 * (leaves - c["leaves_3_lanes"]) / leaves))
        print("  wave-calls off the one-walk path: %.2f %%" % (100.0 * c["cexp_wave_calls_slow_walk"] / c["cexp_wave_calls_with_notes"]))
        print("  keys of the expansion that matched: %.1f %%" % (100.0 * c["cexp_keys_matched"] / keys))
        print("  record-table entries with their strand twin present: %.1f %%" % (100.0 * c["rt_entries_with_twin"] / c["rt_entries"]))
        print("  record-table entries per listed leaf: %.1f" % (c["rt_entries"] / leaves))


if __name__ == "__main__":
    main()
