"""ctypes binding of oracle/_ref/libcfrk_ref.so and a runner for oracle/_ref/cfrk_ref -- the REFERENCE'S OWN
sources, built for the CPU by `make -C oracle ref` (oracle/ref_shim/).  TEST INFRASTRUCTURE ONLY.

oracle/_ref/ is a build product: __graft_entry__.build() makes it where a checkout of the reference exists.
Tests ask have_ref() and skip with SKIP_REASON where it is absent; nothing here builds it or reads the
reference's checkout.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(os.path.dirname(_HERE), "oracle", "_ref")
REF_SO = os.path.join(REF_DIR, "libcfrk_ref.so")
REF_CLI = os.path.join(REF_DIR, "cfrk_ref")
REF_SRC = os.path.join(REF_DIR, "src")          # the reference's headers as the build copied them (tipos.h)
SKIP_REASON = "oracle/_ref/ is not built (`make -C oracle ref` needs a checkout of the reference)"

_lib = None


def have_ref():
    return os.path.exists(REF_SO) and os.access(REF_CLI, os.X_OK)


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(REF_SO)
        L.ref_kmer_main.argtypes = [C.POINTER(C.c_int8), C.POINTER(C.c_long), C.POINTER(C.c_int), C.c_long, C.c_long,
                                    C.c_int, C.POINTER(C.c_int)]
        L.ref_kmer_main.restype = C.c_int
        _lib = L
    return _lib


def call_kmer_main(entry, data, start, length, k):
    """entry(data, start, length, nN, nS, k, freq_out) -- the C entry of oracle/ref_shim/glue.cpp around some
    kmer_main() -> Freq as an (nS, 4^k) int32 array"""
    data = np.ascontiguousarray(data, np.int8)
    start = np.ascontiguousarray(start, np.int64)
    length = np.ascontiguousarray(length, np.int32)
    nS = len(length)
    freq = np.empty(nS * 4 ** k, np.int32)
    rc = entry(data.ctypes.data_as(C.POINTER(C.c_int8)), start.ctypes.data_as(C.POINTER(C.c_long)),
               length.ctypes.data_as(C.POINTER(C.c_int)), len(data), nS, k, freq.ctypes.data_as(C.POINTER(C.c_int)))
    if rc != 0:
        raise RuntimeError(f"kmer_main entry rc={rc}")
    return freq.reshape(nS, 4 ** k)


def kmer_main(data, start, length, k):
    """the reference's kmer_main(&rd, nN, nS, k, 0) on the CPU -> rd.Freq as (nS, 4^k) int32"""
    return call_kmer_main(lib().ref_kmer_main, data, start, length, k)


def run_cli(fasta, out, args, timeout=120):
    """`cfrk_ref fasta out args...` as a child process (CPU only; it never opens a GPU) -> the bytes of `out`.
    The file is removed first, so a child that writes nothing cannot pass for one that wrote an old result."""
    if os.path.exists(out):
        os.remove(out)
    r = subprocess.run([REF_CLI, str(fasta), str(out)] + [str(a) for a in args], timeout=timeout,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        raise RuntimeError(f"cfrk_ref {args} exited with {r.returncode}: {r.stderr[-400:]!r}")
    with open(out, "rb") as f:
        return f.read()
