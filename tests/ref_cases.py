"""The inputs on which the reference itself (oracle/_ref/) referees the oracle (test_reference_cpu.py) and the
product (test_gpu_reference.py): seeded random chunks, directed chunk shapes, and a matrix of FASTA files and
command lines.  Everything is generated here from fixed seeds; no case is dropped at run time.

EXCLUDED is the fixed list of input shapes that are UNDEFINED IN THE REFERENCE (it reads or writes memory it
does not own, with effects no padding makes inert), with the line that makes each undefined; the generators
below never produce them.
"""
import numpy as np

# shape                                    | undefined because (reference line)
EXCLUDED = (
    ("a read of length 0 in a chunk",
     "src/kmer_kernel.cu:85 compares unsigned threadIdx.x < length[i]-1 = 0xFFFFFFFF: all 1024 threads add to "
     "Freq[fourk*i + Index[start+t]], Index read far past the read and the buffer; the CPU build segfaults"),
    ("a chunk whose last byte is not the -1 terminator",
     "src/kmer_kernel.cu:35 reads Seq[i + id] up to k-1 bytes past nN for the windows that start in the last read"),
    ("a FASTA header with no sequence line (also: a sequence line before the first header)",
     "src/fastaIO.h:51-53 never runs for that record; seq[count].read stays an uninitialised pointer that "
     "src/fastaIO.h:123 dereferences (before the first header: seq[-1], src/fastaIO.h:51)"),
    ("a FASTA record whose sequence is one line break, or one character with no line break, i.e. len = 0",
     "src/fastaIO.h:53 len = strlen - 1 = 0, then as a read of length 0"),
    ("a '>' inside a sequence line",
     "src/fastaIO.h:16-21 sizes the record table by `grep -c '>'`, src/fastaIO.h:40 fills it by lines that START "
     "with '>'"),
    ("codes other than 0..3 and -1 in a chunk",
     "src/fastaIO.h:123-139 produces no others; src/kmer_kernel.cu:36-38 would add them into the index"),
    ("k = 15 with more than one read, k = 14 with more than 7",
     "src/kmer_main.cu:90 int nF = nS * 4^k overflows, SetMatrix (src/kmer_kernel.cu:15) then leaves Freq unset"),
)

# seeded random chunks per k (545 in all)
RANDOM_CHUNKS = {1: 60, 2: 60, 3: 60, 4: 60, 5: 60, 6: 60, 7: 60, 8: 50, 9: 25, 10: 25}
LENGTH_POOL = (1, 2, 30, 150, 1023, 1024, 1025, 1026, 1500)


def flatten(reads):
    """codes + one -1 terminator per read, start / length tables (as src/fastaIO.h:74-102 lays a chunk out)"""
    nS = len(reads)
    length = np.array([len(r) for r in reads], np.int32)
    start = np.zeros(nS, np.int64)
    if nS > 1:
        start[1:] = np.cumsum(length[:-1].astype(np.int64) + 1)
    data = np.full(int(length.astype(np.int64).sum()) + nS, -1, np.int8)
    for i, r in enumerate(reads):
        data[start[i]:start[i] + len(r)] = r
    return data, start, length


def _read(rng, L, p_invalid=0.0):
    r = rng.integers(0, 4, L).astype(np.int8)
    if p_invalid:
        r[rng.random(L) < p_invalid] = -1
    return r


def random_chunk(rng, k):
    """1..39 reads (1..5 for k >= 9, whose rows are large), lengths from LENGTH_POOL and k-1, k, k+1 (never 0),
    5 % invalid bases in half of the reads"""
    nS = int(rng.integers(1, 40 if k <= 8 else 6))
    pool = LENGTH_POOL + tuple(x for x in (k - 1, k, k + 1) if x >= 1)
    reads = []
    for _ in range(nS):
        L = int(rng.choice(pool))
        reads.append(_read(rng, L, 0.05 if rng.random() < 0.5 else 0.0))
    return reads


def random_chunks(k, n):
    rng = np.random.default_rng(9000 + k)
    return [random_chunk(rng, k) for _ in range(n)]


def directed_chunks(k):
    """(name, reads) pairs: the shapes at which the reference's quirks show"""
    rng = np.random.default_rng(7000 + k)
    out = []
    lens = sorted({L for L in (1, 2, k - 1, k, k + 1, 1023, 1024, 1025, 1026, 3000) if L >= 1})
    out.append(("every length, clean", [_read(rng, L) for L in lens]))
    out.append(("every length, 3 % invalid", [_read(rng, L, 0.03) for L in lens]))
    for L in lens:
        out.append((f"one read of length {L}", [_read(rng, L)]))

    def bad(L, where):
        r = _read(rng, L)
        if where == "first":
            r[0] = -1
        elif where == "last":
            r[-1] = -1
        elif where == "kth":
            r[k - 1::k] = -1                      # every k-th position: no window is valid
        elif where == "run":
            r[L // 3:L // 3 + k + 5] = -1         # a run longer than k
        elif where == "all":
            r[:] = -1
        return r

    for L in (150, 1500):
        clean = _read(rng, L)
        for where in ("first", "last", "kth", "run", "all"):
            # as the FIRST read (its invalid windows go to Freq[-1]) and behind a clean first read (they go to
            # the previous row's last bin)
            out.append((f"invalid {where}, L={L}, first read", [bad(L, where), clean.copy(), bad(L, where)]))
            out.append((f"invalid {where}, L={L}, behind a clean first read", [clean.copy(), bad(L, where), bad(L, where)]))
    r = _read(rng, 200)
    r[::k] = -1
    r[-1] = -1
    out.append(("invalid at first, last and every k-th in one read", [_read(rng, 80), r]))
    for c in range(4):
        # homopolymers: all-T fills the row's LAST bin, the one the next read's invalid windows are added to
        out.append((f"homopolymers of {'ACGT'[c]}", [np.full(200, c, np.int8), bad(150, "kth"), np.full(1100, c, np.int8),
                                                    bad(150, "first"), np.full(k, c, np.int8), np.full(k + 1, c, np.int8)]))
    out.append(("invalid windows beyond the 1024-window cap only", [_read(rng, 50), np.concatenate([_read(rng, 1100), np.full(400, -1, np.int8)])]))
    out.append(("invalid windows astride the cap", [_read(rng, 50), np.concatenate([_read(rng, 1020), np.full(k + 8, -1, np.int8), _read(rng, 300)])]))
    return out


def many_reads_chunk(k, n=1100):
    """more than 1024 reads: a second row of 1024-thread blocks in every launch sized by the read count"""
    rng = np.random.default_rng(5000 + k)
    return [_read(rng, int(L), 0.05 if i % 3 == 0 else 0.0) for i, L in enumerate(rng.integers(1, 70, n))]


def float_index_reads(k, nreads):
    """one or two reads for k = 11..15: all-T windows (the float index rounds up to 4^k for k >= 13: into the
    next row, or past the last one), an invalid base, otherwise random"""
    rng = np.random.default_rng(1300 + k)
    reads = [_read(rng, int(L)) for L in rng.integers(300, 1500, nreads)]
    reads[0][50:50 + k + 3] = 3
    reads[-1][-(k + 2):] = 3
    reads[-1][120] = -1
    return reads


# ------------------------------------------------------------------ FASTA files and command lines

def _seq(rng, L, alphabet=b"ACGT"):
    a = np.frombuffer(alphabet, np.uint8)
    return a[rng.integers(0, len(a), L)].tobytes()


def fasta_files():
    """name -> bytes.  Record counts 5, 7, 13, 14, 16 sit below, on and above multiples of chunk size 7."""
    rng = np.random.default_rng(4242)
    f = {}

    def records(n, lo=2, hi=70, alphabet=b"ACGT", width=0, eol=b"\n"):
        parts = []
        for i in range(n):
            s = _seq(rng, int(rng.integers(lo, hi)), alphabet)
            parts.append(b">r%d some text\n" % i)
            if width:
                parts.extend(s[o:o + width] + eol for o in range(0, len(s), width))
            else:
                parts.append(s + eol)
        return b"".join(parts)

    f["plain5"] = records(5)
    f["plain7"] = records(7)
    f["plain13"] = records(13)
    f["plain14"] = records(14)
    f["plain16"] = records(16)
    f["multiline16"] = records(16, 25, 200, width=17)          # line breaks stay in the read as invalid bases
    f["lowercase_and_other_letters9"] = records(9, 10, 90, alphabet=b"ACGTacgtNnRYKMU-*.")
    f["crlf6"] = records(6, 10, 60, width=20, eol=b"\r\n")
    f["no_final_newline8"] = records(8)[:-1]                   # the last base goes instead of the line break
    f["short_reads10"] = b"".join(b">s%d\n%s\n" % (i, s) for i, s in enumerate(
        [b"A", b"AC", b"ACG", b"T", b"NN", b"ACGTA", b"G", b"TT", b"ACGTACGTAC", b"C"]))
    f["blank_lines_and_gt_in_header7"] = records(3) + b">h > more > text\nACGTTGCA\n\n\n>x\nAC\n\nGT\n" + records(2) + b"\n\n"
    return f


def cli_forms(chunk_sizes=(1, 7, 8192)):
    """argument lists behind `cfrk in out k`, with the chunk size each one means:
    three arguments: defaults; four: nt is parsed, the chunk size stays 8192 (src/main.cu:247-248); five: the
    chunk size is parsed and the fourth argument never is (src/main.cu:249-250)"""
    forms = [((), 8192), (("2",), 8192)]
    forms += [(("12", str(c)), c) for c in chunk_sizes]
    forms.append((("not-a-number", "7"), 7))
    return forms


def big_fasta(n, seed):
    """n short single-line records (8..13 bases), for the chunk sizes that need thousands of reads"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(8, 14, n)
    body = _seq(rng, int(lens.sum()))
    parts, o = [], 0
    for i, L in enumerate(lens):
        parts.append(b">r%d\n%s\n" % (i, body[o:o + int(L)]))
        o += int(L)
    return b"".join(parts)


# (records, command-line tail, chunk size): read counts on and above a multiple of the default chunk size, and
# chunk size 65536 + 3, which SelectChunk* narrow to 3 (src/main.cu:110,160) while nChunk is computed unnarrowed
BIG_CLI_CASES = (
    (8192, (), 8192),
    (8195, ("12", "8192"), 8192),
    (8192 * 2 + 3, ("4",), 8192),
    (65539 + 5, ("12", "65539"), 65539),
    (1000, ("12", "65539"), 65539),
)
