"""Expected results for texts and read sets of more than 2^32 bytes, by arithmetic -- TEST INFRASTRUCTURE ONLY.

A text of that size cannot go through the plain references (tests/ingest_cases.py's host parser, tests/fastq_ref.py,
tests/text_out_ref.py, tests/filter_ref.py: Python loops, or copies of the whole text).  A text that is `reps` copies of
one block of whole records can: the parse of the tiled text is the block's parse repeated with every offset moved on
by the block's size, so the references run on ONE block and the helpers here do the moving.  tests/test_far_offsets_cpu.py
holds every helper equal to the plain references on a tiled text small enough for them; tests/test_gpu_far_offsets.py
then uses the helpers as its oracle.  Plain numpy; nothing from cfrk_amd."""
import numpy as np

RECORD_DTYPE = np.dtype([("head_off", "<i8"), ("qual_off", "<i8"), ("head_len", "<i4"), ("qual_len", "<i4")])

FAR_N = (1 << 32) + (1 << 20)         # bytes of the far-offset tests' buffers
SEAMS = (1 << 31, 1 << 32)
COMPOSITES = (((1 << 32) - 700, 1400), ((1 << 31) - 3000, 6000), ((1 << 32) - 20000, 40000))


def tiled_text(block: bytes, reps):
    """the text of `reps` copies of `block`, as a uint8 array"""
    return np.tile(np.frombuffer(block, np.uint8), int(reps))


def _tiled_range(block_arr, a, b):
    """elements [a, b) of the endless repetition of block_arr"""
    n = len(block_arr)
    a, b = int(a), int(b)
    if b <= a:
        return block_arr[:0].copy()
    first = a // n
    reps = (b - 1) // n - first + 1
    return np.tile(block_arr, reps)[a - first * n:b - first * n]


def _tiled_reads(data, start, length, reps):
    """the struct-read buffers (native layout: the reads one behind the other, a terminator behind each) of a block's
    parse, repeated -> (start, length, nN, nS, data_range)"""
    data = np.ascontiguousarray(data, np.int8)
    start = np.asarray(start, np.int64)
    length = np.asarray(length, np.int32)
    nNb, nSb, reps = len(data), len(start), int(reps)
    assert nSb > 0 and nNb == int(length.astype(np.int64).sum()) + nSb, "the block's parse is not in the native layout"
    t_start = (start[None, :] + (np.arange(reps, dtype=np.int64) * nNb)[:, None]).reshape(-1)
    t_length = np.tile(length, reps)
    nN = nNb * reps

    def data_range(a, b):
        assert 0 <= a <= b <= nN
        return _tiled_range(data, a, b)

    return t_start, t_length, nN, nSb * reps, data_range


def _whole_records(block, first):
    assert len(block) > 0 and block[:1] == first and block[-1:] == b"\n", "a block is whole records: it begins with a record's first byte and ends with a newline"


def tiled_fasta_expect(block: bytes, block_parse, reps):
    """block_parse = (data, start, length): the NATIVE parse of `block` by the plain reference (the host parser,
    tests/ingest_cases.host_parse).  The block begins with '>' and ends with '\\n', so no line and no record crosses
    from one copy into the next -> (start, length, nN, nS, data_range) of the text of `reps` copies; data_range(a, b)
    is the expected data[a:b]."""
    _whole_records(block, b">")
    return _tiled_reads(*block_parse, reps)


def tiled_fastq_expect(block: bytes, block_parse, reps):
    """as tiled_fasta_expect; block_parse = (data, start, length) of tests/fastq_ref.parse(block, min_qual)"""
    _whole_records(block, b"@")
    assert block.count(b"\n") % 4 == 0, "a FASTQ block is whole four-line records"
    return _tiled_reads(*block_parse, reps)


def tiled_index_expect(block_rows, block_len, reps):
    """the cfrk_text_record rows of the tiled text from the rows of one block (tests/text_out_ref.index_ref): every
    offset moves on by the block's size, the FASTA rows' qual_off of -1 stays"""
    rows = np.asarray(block_rows, RECORD_DTYPE)
    shift = (np.arange(int(reps), dtype=np.int64) * int(block_len))[:, None]
    out = np.empty((int(reps), len(rows)), RECORD_DTYPE)
    out["head_off"] = rows["head_off"][None, :] + shift
    out["qual_off"] = np.where(rows["qual_off"][None, :] == -1, np.int64(-1), rows["qual_off"][None, :] + shift)
    out["head_len"] = rows["head_len"][None, :]
    out["qual_len"] = rows["qual_len"][None, :]
    return out.reshape(-1)


def select_expect(start, length, keep=None, span=None, min_len=0, nN=None):
    """cfrk_reads_select's rule, vectorised -> (start_out, length_out, index_out, nN_out, nS_out): read i is kept iff
    keep[i] != 0 (None: all), its range lies inside [0, nN) (nN None: not looked at), its span (None: the whole read)
    lies inside the read and holds at least min_len bases; output read j takes length_out[j] bases and a terminator,
    the reads one behind the other in input order"""
    start = np.asarray(start, np.int64)
    length = np.asarray(length, np.int64)
    ok = (start >= 0) & (length >= 0)
    if nN is not None:
        ok &= start <= int(nN) - length
    if keep is not None:
        ok &= np.asarray(keep) != 0
    if span is None:
        n = length
    else:
        off, n = np.asarray(span["offset"], np.int64), np.asarray(span["length"], np.int64)
        ok &= (off >= 0) & (n >= 0) & (off + n <= length)
    ok &= n >= int(min_len)
    index = np.flatnonzero(ok).astype(np.int64)
    length_out = n[index].astype(np.int32)
    ends = np.cumsum(length_out.astype(np.int64) + 1)
    start_out = ends - (length_out.astype(np.int64) + 1)
    return start_out, length_out, index, int(ends[-1]) if len(ends) else 0, len(index)


def seam_reads(N, L):
    """indices of the generator's reads (read i = bytes [i (L + 1), i (L + 1) + L] with its terminator) that hold byte
    2^31 - 1 or 2^31, and 2^32 - 1 or 2^32"""
    return sorted({(s - d) // (L + 1) for s in SEAMS for d in (1, 0) if s < N})


def invalid_entries(N, L):
    """(start, length) of the four entries a device form answers with its empty result"""
    return ((N, L), (N - 100, L), (-7, L), ((1 << 32) + 12345, 0))


def pick_reads(N, R, L, seed):
    """the read set of the far-offset tests over the generator's buffer (R reads of L bases, N bytes) -> (start int64[],
    length int32[]) in shuffled order: the seam reads with eight neighbours on each side; read 0, read R - 1 and a
    range that ends on byte N - 1; 2 000 reads that begin at or above 2^31; the three composite ranges that lie across
    terminators (the 64-lane class twice, the long class once); the four invalid entries.  An even number of entries."""
    rng = np.random.default_rng(seed)
    stride = L + 1
    fixed = set()
    for i in seam_reads(N, L):
        fixed.update(range(i - 8, i + 9))
    fixed.update((0, R - 1))
    first_far = -(-(1 << 31) // stride)
    pool = np.setdiff1d(np.arange(first_far, R, dtype=np.int64), np.array(sorted(fixed), np.int64))
    far = rng.choice(pool, 2000, replace=False)
    idx = np.concatenate([np.array(sorted(fixed), np.int64), far])
    entries = [(int(i) * stride, L) for i in idx] + [(N - 2 * L, 2 * L)] + list(COMPOSITES) + list(invalid_entries(N, L))
    if len(entries) % 2:
        entries.append((stride, L))
    order = rng.permutation(len(entries))
    start = np.array([entries[j][0] for j in order], np.int64)
    length = np.array([entries[j][1] for j in order], np.int32)
    return start, length


# ---- blocks of whole records, for the tiled texts ------------------------------------------------

def _bases(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def _odd(records, first, fill):
    """the records joined, of odd size: a block of odd size meets the 16 KiB tiles (and the 16-byte pieces of a lane)
    in every phase as it repeats; `fill` lengthens the first record's header line by one byte"""
    block = b"".join(records)
    if len(block) % 2 == 0:
        nl = records[0].index(b"\n")
        block = records[0][:nl] + fill + records[0][nl:] + b"".join(records[1:])
    assert len(block) % 2 == 1 and block[:1] == first
    return block


def fastq_block(seed, lengths):
    """a canonical FASTQ block (bare '+' lines, upper-case ACGT, no '\\r') with one record per entry of `lengths`;
    qualities are Phred 0 .. 40, so quality lines may begin with '+' or '@' and some bases fall below a min_qual of 20"""
    rng = np.random.default_rng(seed)
    recs = []
    for i, n in enumerate(lengths):
        q = (33 + rng.integers(0, 41, int(n))).astype(np.uint8).tobytes()
        recs.append(b"@q%d/%d len=%d\n" % (i // 2, 1 + i % 2, n) + _bases(rng, int(n)) + b"\n+\n" + q + b"\n")
    return _odd(recs, b"@", b"x")


def fasta_block(seed, n_plain, L=150):
    """a FASTA block of n_plain one-line records of L upper-case bases, and in between a few records that are wrapped,
    end their lines with '\\r\\n', or hold lower-case and N bases"""
    rng = np.random.default_rng(seed)
    recs = [b">s%d\n" % i + _bases(rng, L) + b"\n" for i in range(n_plain)]
    wrapped = _bases(rng, 333)
    extras = [b">wrapped text\n" + b"".join(wrapped[o:o + 60] + b"\n" for o in range(0, len(wrapped), 60)),
              b">crlf\r\n" + _bases(rng, 70) + b"\r\n" + _bases(rng, 31) + b"\r\n",
              b">lower and N\n" + _bases(rng, 200, b"ACGTacgtNn") + b"\n",
              b">one\nA\n"]
    for j, e in enumerate(extras):
        recs.insert(1 + (j * 7919) % max(n_plain - 1, 1), e)
    return _odd(recs, b">", b"x")
