"""CPU: the properties of the correction rule itself (tests/correct_ref.py, the reference the GPU tests hold the library
to), on seeded inputs: a random 20 000-base genome, reads at coverage 30 from both strands, a canonical count of the clean
reads, min_count 2.  At k >= 21 a 20 kb genome has no chance-solid alternatives to speak of, so a single substitution is
restored at every position, two substitutions more than k apart are both restored, and two within k bases of each other
make one run longer than k (or an interior run shorter than k) and leave the read alone.  A bad seed shows up here and
not on the GPU.  The CLI's refusals that are raised before a device is opened are here too."""
import functools
import os
import subprocess

import numpy as np
import pytest

from . import correct_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(100, 21), (150, 31), (120, 33)]
SAMPLE = 400
MIN_COUNT = 2


@functools.lru_cache(maxsize=None)
def _world(L, k):
    """(clean reads, counts): coverage 30 of a 20 kb genome, half the reads reverse-complemented"""
    rng = np.random.default_rng([20000, L, k])
    genome = rng.integers(0, 4, 20000).astype(np.int8)
    reads = []
    for _ in range(30 * len(genome) // L):
        a = int(rng.integers(0, len(genome) - L + 1))
        r = genome[a:a + L].copy()
        reads.append(cr.revcomp(r) if rng.integers(0, 2) else r)
    counts = cr.count_reads(*cr.flatten(reads), k, True)
    return reads, counts


@functools.lru_cache(maxsize=None)
def _covered(L, k):
    """the reads whose every window is solid as they are.  The rule can only put back a base whose windows the spectrum
    supports: at the two ends of a linear genome the coverage runs out (a window of the last few bases is seen once),
    and a read from there is outside the premise of the restoration properties.  Nearly every read qualifies."""
    reads, counts = _world(L, k)
    ok = [i for i, r in enumerate(reads) if all(c == cr.SOLID for c in cr.window_classes(r.tolist(), k, True, counts, MIN_COUNT))]
    assert len(ok) >= 0.95 * len(reads)
    return ok


def _sample(L, k, salt):
    reads, counts = _world(L, k)
    rng = np.random.default_rng([salt, L, k])
    return [reads[i] for i in rng.choice(_covered(L, k), SAMPLE, replace=False)], counts, rng


@pytest.mark.parametrize("L,k", SHAPES)
def test_clean_reads_come_back_unchanged(L, k):
    reads, counts = _world(L, k)
    rng = np.random.default_rng([1, L, k])
    for r in [reads[i] for i in rng.choice(len(reads), SAMPLE, replace=False)]:       # (any read, covered or not)
        out, fixed, _ = cr.correct_codes(r.tolist(), k, True, counts, MIN_COUNT)
        assert out == r.tolist() and fixed == 0


@pytest.mark.parametrize("L,k", SHAPES)
def test_one_substitution_is_restored_at_any_position(L, k):
    sample, counts, rng = _sample(L, k, 2)
    edge = [0, 1, k - 2, k - 1, k, L - k - 1, L - k, L - k + 1, L - 2, L - 1]
    for j, r in enumerate(sample):
        p = edge[j] if j < len(edge) else int(rng.integers(0, L))
        out, fixed, left = cr.correct_codes(cr.substitute(r, p, rng).tolist(), k, True, counts, MIN_COUNT)
        assert out == r.tolist(), (j, p)
        assert (fixed, left) == (1, 0), (j, p, fixed, left)


@pytest.mark.parametrize("L,k", SHAPES)
def test_two_substitutions_more_than_k_apart_are_both_restored(L, k):
    sample, counts, rng = _sample(L, k, 3)
    for j, r in enumerate(sample):
        d = k + 1 if j < 50 else int(rng.integers(k + 1, L))
        p = int(rng.integers(0, L - d))
        bad = cr.substitute(cr.substitute(r, p, rng), p + d, rng)
        out, fixed, left = cr.correct_codes(bad.tolist(), k, True, counts, MIN_COUNT)
        assert out == r.tolist(), (j, p, d)
        assert (fixed, left) == (2, 0), (j, p, d, fixed, left)


@pytest.mark.parametrize("L,k", SHAPES)
def test_two_substitutions_within_k_leave_the_read_untouched(L, k):
    sample, counts, rng = _sample(L, k, 4)
    for j, r in enumerate(sample):
        d = (k, k - 1, 1)[j] if j < 3 else int(rng.integers(1, k + 1))
        p = int(rng.integers(0, L - d))
        bad = cr.substitute(cr.substitute(r, p, rng), p + d, rng)
        out, fixed, left = cr.correct_codes(bad.tolist(), k, True, counts, MIN_COUNT)
        assert out == bad.tolist(), (j, p, d)
        assert fixed == 0 and left >= 1, (j, p, d, fixed, left)


def test_min_count_zero_is_the_identity():
    reads, counts = _world(100, 21)
    rng = np.random.default_rng(5)
    bad = cr.substitute(reads[0], 40, rng)
    assert cr.correct_codes(bad.tolist(), 21, True, counts, 0) == (bad.tolist(), 0, 0)
    assert cr.correct_codes(bad.tolist(), 21, True, {}, 0) == (bad.tolist(), 0, 0)


def test_the_table_of_attempted_runs():
    I, W, S = cr.INVALID, cr.WEAK, cr.SOLID
    k = 3
    pos = lambda cls: [cr.attempted_position(cls, a, b, k) for a, b in cr.weak_runs(cls)]
    assert pos([S, W, W, W, S]) == [3]                    # interior, n == k: p = b
    assert pos([S, W, W, S]) == [None]                    # interior, shorter than k
    assert pos([S, W, W, W, W, S]) == [None]              # longer than k
    assert pos([W, S, S]) == [0] and pos([W, W, W, S]) == [2]          # head: p = b
    assert pos([W, W, W, W, S]) == [None]
    assert pos([S, S, W]) == [4] and pos([S, W, W, W]) == [3]          # tail: p = a + k - 1
    assert pos([S, W, W, W, W]) == [None]
    assert pos([W, W]) == [None] and pos([W]) == [None]                # the whole read
    assert pos([I, W, W, W, S]) == [None] and pos([S, W, W, W, I]) == [None]
    assert pos([I, W, S]) == [None] and pos([S, W, I]) == [None]
    assert pos([W, I, S]) == [None] and pos([S, I, W]) == [None]
    assert pos([W, S, W, W, W, S, W]) == [0, 4, 8]


# ------------------------------------------------------------------ the ABI's names and the CLI's refusals (no device is opened)

@pytest.fixture(scope="module")
def built():
    import cfrk_amd
    if not os.path.exists(cfrk_amd.library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return cfrk_amd


@pytest.fixture(scope="module")
def cli(built):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def test_abi_declares_and_exports_the_correction_calls(built):
    import ctypes as C
    syms = built.abi_symbols()
    L = C.CDLL(built.library_path())
    for s in ("cfrk_global_correct_reads", "cfrk_global_correct_reads_device"):
        assert s in syms
        assert hasattr(L, s)
    assert built.READ_FIX_DTYPE.itemsize == 8 and built.READ_FIX_DTYPE.names == ("fixed", "left")
    assert built.READ_FIX_DTYPE == cr.FIX_DTYPE


Q = ["--global", "--query", "q.fa"]
C_OUT = Q + ["--correct-out", "c.fa"]


@pytest.mark.parametrize("args, msg", [
    (Q + ["--query-out", "o.q", "--correct-min-count", "2"], b"need --correct-out CFILE"),
    (Q + ["--query-out", "o.q", "--correct-names"], b"need --correct-out CFILE"),
    (Q + ["--query-out", "o.q", "--correct-report", "r.txt"], b"need --correct-out CFILE"),
    (Q + ["--query-out", "o.q", "--correct-format", "fasta"], b"need --correct-out CFILE"),
    (C_OUT, b"--correct-out needs --correct-min-count T"),
    (C_OUT + ["--correct-names"], b"--correct-out needs --correct-min-count T"),
    (["--query", "q.fa", "--correct-out", "c.fa", "--correct-min-count", "2"], b"--query needs --global or --query-db"),
    (["--global", "--correct-out", "c.fa", "--correct-min-count", "2"], b"need --query QFILE"),
    (C_OUT + ["--correct-min-count", "2", "--correct-format", "fastq"], b"--correct-format fastq needs a FASTQ --query file"),
    (C_OUT + ["--correct-min-count", "two"], b"--correct-min-count needs a count"),
    (C_OUT + ["--correct-min-count", "-1"], b"--correct-min-count needs a count"),
    (C_OUT + ["--correct-min-count", "4294967296"], b"--correct-min-count needs a count"),
    (C_OUT + ["--correct-min-count", "2", "--correct-format", "sam"], b"--correct-format takes fasta or fastq"),
    (C_OUT + ["--correct-min-count"], b"--correct-min-count needs a value"),
    (C_OUT + ["--correct-bogus", "1"], b"unknown option --correct-bogus"),
    (C_OUT + ["--correct-min-count", "2", "--gpus", "2"], b"not with --gpus"),
    (C_OUT + ["--correct-min-count", "2", "--batch", "2"], b"not with --batch"),
    (["--sparse", "--query", "q.fa", "--correct-out", "c.fa", "--correct-min-count", "2"], b"--sparse is a per-read mode"),
    (["--query-db", "db.bin", "--query", "q.fa", "--correct-out", "c.fa"], b"--correct-out needs --correct-min-count T"),
    (["--query-db", "db.bin", "--query", "q.fa", "--query-out", "o.q", "--correct-report", "r.txt"], b"need --correct-out CFILE"),
])
def test_cli_refuses_bad_correct_options_before_reading_input(cli, tmp_path, args, msg):
    """refused with status 1 and a message before any input is read or a device is opened: neither the input nor the
    query file exists, and no output file is created"""
    out = tmp_path / "o.txt"
    p = subprocess.run([cli, str(tmp_path / "missing.fasta"), str(out), "15"] + args, cwd=tmp_path,
                       capture_output=True, timeout=60)
    assert p.returncode == 1
    assert msg in p.stderr
    for name in ("o.txt", "o.q", "c.fa", "r.txt"):
        assert not (tmp_path / name).exists()
