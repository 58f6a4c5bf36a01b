"""The FASTQ grammar of include/cfrk_abi.h (cfrk_fastq_parse_device) restated in plain Python, from the text of the
grammar and not from the parsers: the yardstick test_fastq_cpu.py and test_gpu_fastq.py hold both parsers against.

parse(raw, min_qual) -> ("ok", data int8[nN], start int64[nS], length int32[nS]) or (cause, where) with cause one of
"no_at" / "no_plus" (where = the line, from 0), "truncated" (where = the number of lines), "lengths" (where = the
record, from 0), "min_qual" (where = 0).  (A record of 2^31 bases is beyond a test.)"""
import functools

import numpy as np

QUAL_BASE, MAX_QUAL = 33, 93

_CODES = np.full(256, -1, np.int8)
for _i, _c in enumerate(b"ACGT"):
    _CODES[_c] = _CODES[_c + 32] = _i


def lines_of(raw):
    """[(offset of the line, the line without its line end)]: a line ends at '\\n' or at the end of the text; a trailing
    '\\n' opens no further line; one '\\r' directly in front of the '\\n', or as the text's last byte, is dropped"""
    out, pos, n = [], 0, len(raw)
    while pos < n:
        nl = raw.find(b"\n", pos)
        end = n if nl < 0 else nl
        body = raw[pos:end]
        if body.endswith(b"\r"):         # (end is the '\n' or the end of the text)
            body = body[:-1]
        out.append((pos, body))
        pos = end + 1
    return out


@functools.lru_cache(maxsize=4)
def _unmasked(raw):
    """the verdict without masking: a refusal, or ("ok", data, the quality byte of every base (of the terminators:
    255), start, length) -- kept for the text parsed last, which the tests parse again with every min_qual"""
    lines = lines_of(raw)
    # structural faults: the earliest line; the truncated record lies behind every line
    for i, (pos, _) in enumerate(lines):
        if i % 4 == 0 and raw[pos:pos + 1] != b"@":
            return ("no_at", i)
        if i % 4 == 2 and raw[pos:pos + 1] != b"+":
            return ("no_plus", i)
    if len(lines) % 4:
        return ("truncated", len(lines))
    nS = len(lines) // 4
    for r in range(nS):
        if len(lines[4 * r + 1][1]) != len(lines[4 * r + 3][1]):
            return ("lengths", r)
    length = np.array([len(lines[4 * r + 1][1]) for r in range(nS)], np.int32)
    start = np.zeros(nS, np.int64)
    if nS:
        start[1:] = np.cumsum(length[:-1].astype(np.int64) + 1)
    # every record's line and one more byte: the terminator's place
    seq = np.frombuffer(b"".join(lines[4 * r + 1][1] + b"\n" for r in range(nS)), np.uint8)
    qual = np.frombuffer(b"".join(lines[4 * r + 3][1] + b"\xff" for r in range(nS)), np.uint8)
    return ("ok", _CODES[seq], qual, start, length, seq)


def parse(raw, min_qual=0):
    if not 0 <= min_qual <= MAX_QUAL:
        return ("min_qual", 0)
    res = _unmasked(bytes(raw))
    if res[0] != "ok":
        return res
    _, data, qual, start, length, _ = res
    if min_qual > 0:                     # (min_qual 0: the quality line is only measured)
        data = np.where(qual.astype(np.int64) - QUAL_BASE < min_qual, np.int8(-1), data)
    return ("ok", data.copy(), start.copy(), length.copy())


def equivalent_fasta(raw, min_qual=0):
    """the FASTA text that says what a VALID four-line FASTQ text says: one record per read, its sequence on one line,
    every base whose quality is below min_qual replaced by N -- and so is every byte that is no base anyway but means
    something to a FASTA reader (a '\\r', a '>' ), so that the line survives the FASTA grammar as it is"""
    res = _unmasked(bytes(raw))
    assert res[0] == "ok"
    _, _, qual, _, _, seq = res          # (the sequence lines, a '\n' behind each; the quality lines, 0xFF behind each)
    if not seq.size:
        return b""
    swap = (seq == 13) | (seq == ord(">"))
    if min_qual > 0:
        swap |= qual.astype(np.int64) - QUAL_BASE < min_qual
    lines = np.where(swap, np.uint8(ord("N")), seq).tobytes()[:-1].split(b"\n")
    return b"".join(b">r\n" + line + b"\n" for line in lines)
