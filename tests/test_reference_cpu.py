"""The oracle and the host restatement against THE REFERENCE ITSELF, executed on the CPU.

oracle/cfrk_oracle.c and tests/refsem.py are this project's reading of the reference; every other test rests
on them.  Here the reference's own kmer_main() / kernels / CLI, built for the CPU into oracle/_ref/ (`make -C
oracle ref`: its sources against the stand-in for <cuda.h> of oracle/ref_shim/, kernels as serial loops), say
whether that reading is right: the spill of invalid windows into the previous row's last bin, the `length-1`
bound, the 1024-window cap, the float index accumulation, the unsigned-short narrowing of the chunk arguments,
"only the remainder chunk reaches the file", the FASTA ingest that keeps line breaks and drops the last
character.  Bit for bit and byte for byte: this is integer work.

Input shapes that are undefined in the reference are a fixed list, ref_cases.EXCLUDED (shape, reference line).
CPU only; skipped, with the reason, where oracle/_ref/ has not been built.
"""
import os

import numpy as np
import pytest

from . import oracle_lib as orc
from . import ref_cases as cases
from . import ref_lib as ref
from . import refsem
from .conftest import GOLDEN

pytestmark = pytest.mark.skipif(not ref.have_ref(), reason=ref.SKIP_REASON)

RANDOM_CHUNKS = cases.RANDOM_CHUNKS


def test_the_random_cases_number_at_least_500():
    assert sorted(RANDOM_CHUNKS) == list(range(1, 11)) and sum(RANDOM_CHUNKS.values()) >= 500


def _assert_same(reads, k, flags, what):
    data, start, length = cases.flatten(reads)
    want = ref.kmer_main(data, start, length, k)
    got = orc.per_read_dense(data, start, length, k, flags)
    if not (got == want).all():
        bad = np.argwhere(got != want)
        i, b = bad[0]
        raise AssertionError(f"k={k} {what}: {len(bad)} bins differ, first at read {i} bin {b}: oracle {got[i, b]}, "
                             f"reference {want[i, b]}; lengths {length[:12].tolist()}")


@pytest.mark.parametrize("k", range(1, 11))
def test_oracle_compat_equals_reference_kmer_main_on_random_chunks(k):
    for n, reads in enumerate(cases.random_chunks(k, RANDOM_CHUNKS[k])):
        _assert_same(reads, k, orc.ORC_COMPAT, f"random chunk {n}")


@pytest.mark.parametrize("k", range(1, 11))
def test_oracle_compat_equals_reference_kmer_main_on_directed_shapes(k):
    for name, reads in cases.directed_chunks(k):
        _assert_same(reads, k, orc.ORC_COMPAT, name)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_oracle_compat_equals_reference_kmer_main_above_1024_reads(k):
    reads = cases.many_reads_chunk(k)
    assert len(reads) > 1024
    _assert_same(reads, k, orc.ORC_COMPAT, "1100 reads")


def test_directed_shapes_do_what_their_names_say():
    """the directed chunks really produce a first-row spill, a spill into a previous row, and a capped read
    (seen in the REFERENCE's result, so that a generator gone stale cannot hollow the tests out)"""
    k = 3
    shapes = dict(cases.directed_chunks(k))
    reads = shapes["invalid kth, L=150, behind a clean first read"]
    data, start, length = cases.flatten(reads)
    f = ref.kmer_main(data, start, length, k)
    # row 0: its own 148 valid windows + the 149 invalid windows of read 1 in its last bin
    assert f[0].sum() == 148 + 149 and f[1].sum() == 149 and f[2].sum() == 0
    reads = shapes["invalid kth, L=150, first read"]
    data, start, length = cases.flatten(reads)
    f = ref.kmer_main(data, start, length, k)
    assert f[0].sum() == 1 and f[1].sum() == 148 + 149           # read 0's own spill is gone; 1 = read 1's last window
    data, start, length = cases.flatten(shapes["one read of length 3000"])
    assert ref.kmer_main(data, start, length, k).sum() == 1024    # blockDim.x windows, not 2998
    data, start, length = cases.flatten(shapes["one read of length 1026"])
    assert ref.kmer_main(data, start, length, k).sum() == 1024    # length-1 = 1025 threads wanted
    data, start, length = cases.flatten(shapes["one read of length 1024"])
    assert ref.kmer_main(data, start, length, k).sum() == 1022    # L-1 threads, the last one's window is invalid ...
    data, start, length = cases.flatten([np.zeros(10, np.int8), np.zeros(1024, np.int8)])
    assert ref.kmer_main(data, start, length, k)[0, -1] == 1      # ... and lands in the row before


# k = 11..14 with the float accumulation.  The CPU build calls libm's powf, which is exact for powers of 4; a
# CUDA device's powf need not be.  The claim is about the arithmetic AS WRITTEN (src/kmer_kernel.cu:38: the
# running index converted to float, added, truncated back), not about one GPU's powf.
# k = 14 is one read (a row is 1 GiB).  k = 15 is NOT run: one read is a 4 GiB row in the reference, in the
# oracle and in the copies between them, and it alone took 53 s here against 11 s for k = 14 and 141 s for the
# whole CPU suite before this file; k = 15 adds no arithmetic that k = 14 lacks (both exceed 2^24 by the same path).
FLOAT_INDEX_CASES = [(11, 2), (12, 2), (13, 2), (14, 1)]


@pytest.mark.parametrize("k,nreads", FLOAT_INDEX_CASES)
def test_oracle_float_index_equals_reference_kmer_main(k, nreads):
    data, start, length = cases.flatten(cases.float_index_reads(k, nreads))
    want = ref.kmer_main(data, start, length, k)
    got = orc.per_read_dense(data, start, length, k, orc.ORC_COMPAT | orc.ORC_FLOAT_INDEX)
    assert (got == want).all(), f"k={k}: ORC_COMPAT|ORC_FLOAT_INDEX differs from the reference"
    if k <= 12:
        del got
        exact = orc.per_read_dense(data, start, length, k, orc.ORC_COMPAT)
        assert (exact == want).all(), f"k={k}: the exact-integer oracle differs from the reference"


def test_exact_index_oracle_differs_from_the_reference_at_k13():
    """from k = 13 the reference's float index leaves the exact integer (most windows land in a neighbouring
    bin): plain ORC_COMPAT is NOT the reference there, ORC_FLOAT_INDEX is (the case above)"""
    data, start, length = cases.flatten(cases.float_index_reads(13, 2))
    want = ref.kmer_main(data, start, length, 13)
    exact = orc.per_read_dense(data, start, length, 13, orc.ORC_COMPAT)
    assert (exact != want).any()


# ------------------------------------------------------------------ the CLI: refsem against cfrk_ref

def _want(raw, k, chunk):
    return refsem.reference_cfrk_bytes(raw, k, chunk)


@pytest.fixture(scope="module")
def fasta_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("ref_fasta")
    paths = {}
    for name, raw in cases.fasta_files().items():
        p = d / (name + ".fasta")
        p.write_bytes(raw)
        paths[name] = (str(p), raw)
    return d, paths


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_refsem_equals_the_file_the_reference_cli_writes(fasta_dir, k):
    d, paths = fasta_dir
    out = str(d / f"out_k{k}.cfrk")
    nonempty = 0
    for name, (path, raw) in paths.items():
        for tail, chunk in cases.cli_forms():
            got = ref.run_cli(path, out, (k,) + tuple(tail), timeout=60)
            want = _want(raw, k, chunk)
            assert got == want, f"{name} k={k} args={tail}: reference wrote {len(got)} bytes, refsem says {len(want)}"
            nonempty += bool(got)
    assert nonempty > len(paths) * 3          # (chunk size 1 and exact multiples give empty files; most do not)


@pytest.mark.parametrize("n,tail,chunk", cases.BIG_CLI_CASES)
def test_refsem_equals_the_reference_cli_on_thousands_of_reads(tmp_path, n, tail, chunk):
    """read counts on and above a multiple of the default chunk size; chunk size 65536 + 3, which SelectChunk*
    narrow to unsigned short (src/main.cu:110,160): with 65544 reads the chunk that reaches the file starts at
    read 3 * 1, not at read 65539"""
    raw = cases.big_fasta(n, 31 + n)
    fa, out = tmp_path / "big.fasta", tmp_path / "big.cfrk"
    fa.write_bytes(raw)
    for k in (1, 2):
        got = ref.run_cli(fa, out, (k,) + tuple(tail), timeout=300)
        assert got == _want(raw, k, chunk), f"{n} reads k={k} args={tail}"
    if n == 65539 + 5:
        reads = refsem.read_fasta_compat(raw)
        first = refsem.remainder_chunk(reads, chunk)
        assert len(first) == 5 and first[0] is reads[3]
        assert got.count(b"\n") + 1 == 5


@pytest.mark.parametrize("name", ["seq1", "seq2"])
def test_reference_cli_reproduces_its_own_goldens(derived_fasta, tmp_path, name):
    """reference test/test.sh:13-19 run by the reference's own CLI on the golden-derived FASTA pre-images.
    seq2 is the input on which the unpadded build dies in ReadFasta (src/fastaIO.h:51-52: strcat onto fresh
    malloc memory); the build's zeroing malloc makes it defined (oracle/ref_shim/cuda.h, DESIGN.md "Oracle")"""
    got = ref.run_cli(derived_fasta[name], tmp_path / "out.cfrk", (2, 12, 8192), timeout=300)
    assert got == open(os.path.join(GOLDEN, f"out-{name}.cfrk"), "rb").read()


def test_excluded_shapes_are_a_fixed_documented_list():
    assert len(cases.EXCLUDED) == 7
    for shape, why in cases.EXCLUDED:
        assert shape and "src/" in why and ":" in why         # every exclusion names the reference line
    # ... and the generators keep to it: no zero-length read, terminator last, codes in {-1, 0..3}
    for k in (1, 4, 10):
        chunks = [r for _, r in cases.directed_chunks(k)] + cases.random_chunks(k, 20) + [cases.many_reads_chunk(k)]
        for reads in chunks:
            assert all(len(r) >= 1 for r in reads)
            data, _, _ = cases.flatten(reads)
            assert data[-1] == -1 and data.min() >= -1 and data.max() <= 3
    for raw in cases.fasta_files().values():
        assert all(len(r) >= 1 for r in refsem.read_fasta_compat(raw))
