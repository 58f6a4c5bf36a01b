"""GPU: the product against THE REFERENCE ITSELF (its own kmer_main() and CLI, built for the CPU into
oracle/_ref/ by `make -C oracle ref`), not against this project's oracle.

Context.per_read_dense(CFRK_COMPAT), the kmer_main() shim of INTEGRATION.md and the `cfrk` command must give
what the reference gives, bit for bit and byte for byte, on the chunks and FASTA files of tests/ref_cases.py
(the same ones on which test_reference_cpu.py holds the oracle to the reference).  Only oracle/_ref/ is used,
never a checkout of the reference; cfrk_ref runs on the CPU and opens no GPU; the product's CLI runs one
child at a time, each under its own timeout.  Run with `pytest -m gpu` on an MI355X.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from . import ref_cases as cases
from . import ref_lib as ref
from .conftest import ROOT

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.have_ref(), reason=ref.SKIP_REASON)]


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """cfrk_amd/host/kmer_main_shim.cpp (INTEGRATION.md's kmer_main()) behind the same C entry that fronts the
    reference's kmer_main() in libcfrk_ref.so (oracle/ref_shim/glue.cpp), compiled against the reference's own
    tipos.h as the build copied it: both are handed the same `struct read`"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    lib = os.path.join(ROOT, "cfrk_amd")
    so = str(tmp_path_factory.mktemp("shim") / "libkmer_main_shim.so")
    shim_dir = os.path.join(ROOT, "oracle", "ref_shim")
    subprocess.check_call([gxx, "-O1", "-std=gnu++14", "-fPIC", "-shared", "-w", "-pthread",
                           "-DREF_GLUE_ENTRY=shim_kmer_main", "-DREF_GLUE_FREE=free",
                           "-I" + shim_dir, "-I" + ref.REF_SRC, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(shim_dir, "glue.cpp"), os.path.join(lib, "host", "kmer_main_shim.cpp"),
                           "-L" + lib, "-lcfrk_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", so],
                          timeout=300)
    L = C.CDLL(so)
    L.shim_kmer_main.argtypes = [C.POINTER(C.c_int8), C.POINTER(C.c_long), C.POINTER(C.c_int), C.c_long, C.c_long,
                                 C.c_int, C.POINTER(C.c_int)]
    L.shim_kmer_main.restype = C.c_int
    return L.shim_kmer_main


def _diff(got, want, length, k, what, who):
    if not (got == want).all():
        bad = np.argwhere(got != want)
        i, b = bad[0]
        raise AssertionError(f"k={k} {what}: {who} differs from the reference in {len(bad)} bins, first at read {i} "
                             f"bin {b}: {got[i, b]} against {want[i, b]}; lengths {length[:12].tolist()}")


def _check(ctx, shim, reads, k, what):
    import cfrk_amd
    data, start, length = cases.flatten(reads)
    want = ref.kmer_main(data, start, length, k)
    _diff(ctx.per_read_dense(data, start, length, k, cfrk_amd.CFRK_COMPAT), want, length, k, what, "per_read_dense")
    if shim is not None:
        _diff(ref.call_kmer_main(shim, data, start, length, k), want, length, k, what, "the kmer_main() shim")


@pytest.mark.parametrize("k", range(1, 11))
def test_dense_compat_equals_reference_kmer_main_on_random_chunks(ctx, k):
    for n, reads in enumerate(cases.random_chunks(k, cases.RANDOM_CHUNKS[k])):
        _check(ctx, None, reads, k, f"random chunk {n}")


@pytest.mark.parametrize("k", range(1, 11))
def test_dense_compat_and_kmer_main_shim_equal_reference_kmer_main_on_directed_shapes(ctx, shim, k):
    for name, reads in cases.directed_chunks(k):
        _check(ctx, shim, reads, k, name)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_dense_compat_and_kmer_main_shim_equal_reference_kmer_main_above_1024_reads(ctx, shim, k):
    _check(ctx, shim, cases.many_reads_chunk(k), k, "1100 reads")


def test_kmer_main_shim_equals_reference_kmer_main_on_random_chunks(shim):
    """the shim on its own context (one per calling thread), a few random chunks per k"""
    import cfrk_amd  # noqa: F401  (the library the shim links is the one the package loads)
    for k in range(1, 11):
        for n, reads in enumerate(cases.random_chunks(k, 6)):
            data, start, length = cases.flatten(reads)
            _diff(ref.call_kmer_main(shim, data, start, length, k), ref.kmer_main(data, start, length, k), length, k,
                  f"random chunk {n}", "the kmer_main() shim")


def test_dense_compat_equals_reference_kmer_main_on_a_chunk_of_8192_reads_k4(ctx, shim):
    """the reference's default chunk (src/main.cu:235) at k = 4"""
    rng = np.random.default_rng(7)
    reads = [cases._read(rng, int(L), 0.005) for L in rng.integers(140, 160, 8192)]
    _check(ctx, shim, reads, 4, "8192 reads")


@pytest.mark.parametrize("k", [12, 13, 14])
def test_dense_float_index_equals_reference_kmer_main(ctx, k):
    """CFRK_COMPAT | CFRK_FLOAT_INDEX, one read: the reference's float-accumulated index (src/kmer_kernel.cu:38),
    as its own code computes it with libm's powf (exact for powers of 4; the claim is about the arithmetic as
    written, a CUDA device's powf need not be exact)"""
    import cfrk_amd
    data, start, length = cases.flatten(cases.float_index_reads(k, 1))
    want = ref.kmer_main(data, start, length, k)
    got = ctx.per_read_dense(data, start, length, k, cfrk_amd.CFRK_COMPAT | cfrk_amd.CFRK_FLOAT_INDEX)
    _diff(got, want, length, k, "one read", "per_read_dense(CFRK_FLOAT_INDEX)")
    if k >= 13:
        plain = ctx.per_read_dense(data, start, length, k, cfrk_amd.CFRK_COMPAT)
        assert (plain != want).any()          # without the flag the product counts exact integers: not the reference


# ------------------------------------------------------------------ the cfrk command against cfrk_ref

def _cli():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def _run_product(cli, fasta, out, args, timeout):
    if os.path.exists(out):
        os.remove(out)
    subprocess.run([cli, str(fasta), str(out)] + [str(a) for a in args], check=True, timeout=timeout,
                   stdout=subprocess.DEVNULL)
    with open(out, "rb") as f:
        return f.read()


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_cli_writes_the_file_the_reference_cli_writes(tmp_path, k):
    cli = _cli()
    out, rout = tmp_path / "out.cfrk", tmp_path / "ref.cfrk"
    nonempty = 0
    for name, raw in cases.fasta_files().items():
        fa = tmp_path / (name + ".fasta")
        fa.write_bytes(raw)
        for tail, _ in cases.cli_forms():
            args = (k,) + tuple(tail)
            want = ref.run_cli(fa, rout, args, timeout=60)
            got = _run_product(cli, fa, out, args, timeout=120)
            assert got == want, f"{name} k={k} args={tail}: cfrk wrote {len(got)} bytes, cfrk_ref {len(want)}"
            nonempty += bool(want)
    assert nonempty > 30


@pytest.mark.parametrize("n,tail,chunk", cases.BIG_CLI_CASES)
def test_cli_writes_the_file_the_reference_cli_writes_on_thousands_of_reads(tmp_path, n, tail, chunk):
    """on and above a multiple of the default chunk size; chunk size 65536 + 3, narrowed to 3 by the reference"""
    cli = _cli()
    raw = cases.big_fasta(n, 31 + n)
    fa, out, rout = tmp_path / "big.fasta", tmp_path / "big.cfrk", tmp_path / "ref.cfrk"
    fa.write_bytes(raw)
    for k in (1, 2):
        args = (k,) + tuple(tail)
        want = ref.run_cli(fa, rout, args, timeout=300)
        got = _run_product(cli, fa, out, args, timeout=300)
        assert got == want, f"{n} reads k={k} args={tail}"


@pytest.mark.parametrize("name", ["seq1", "seq2"])
def test_cli_and_reference_cli_agree_on_the_golden_preimages(derived_fasta, tmp_path, name):
    """reference test/test.sh:13-19, both commands on the same input; k = 2 as the goldens, and k = 4"""
    cli = _cli()
    for k in (2, 4):
        want = ref.run_cli(derived_fasta[name], tmp_path / "ref.cfrk", (k, 12, 8192), timeout=300)
        got = _run_product(cli, derived_fasta[name], tmp_path / "out.cfrk", (k, 12, 8192), timeout=300)
        assert want and got == want
