"""Plain Python / numpy references of the text index (cfrk_text_index) and the text emitter (cfrk_reads_emit_text), written
from the definitions in include/cfrk_abi.h.  The library's own calls are never the reference."""
import numpy as np

TEXT_FASTA, TEXT_FASTQ = 0, 1
RECORD_DTYPE = np.dtype([("head_off", "<i8"), ("qual_off", "<i8"), ("head_len", "<i4"), ("qual_len", "<i4")])
SPAN_DTYPE = np.dtype([("offset", "<i4"), ("length", "<i4")])


def lines_ref(text):
    """-> [(offset, length)] of every line: a line ends at '\\n' or at the text's end, a trailing '\\n' opens no line;
    the length excludes the '\\n' and one '\\r' directly in front of it, or one '\\r' that is the text's last byte"""
    text = bytes(text)
    out, p, n = [], 0, len(text)
    while p < n:
        e = text.find(b"\n", p)
        if e < 0:
            e = n
        ln = e - p
        if ln > 0 and text[e - 1] == 13:
            ln -= 1
        out.append((p, ln))
        p = e + 1
    return out


def index_ref(text, fmt):
    text = bytes(text)
    lines = lines_ref(text)
    if fmt == TEXT_FASTA:
        rows = [(o, -1, n, 0) for o, n in lines if text[o:o + 1] == b">"]
    else:
        assert fmt == TEXT_FASTQ
        rows = [(lines[4 * r][0], lines[4 * r + 3][0], lines[4 * r][1], lines[4 * r + 3][1]) for r in range(len(lines) // 4)]
    return np.array(rows, RECORD_DTYPE) if rows else np.zeros(0, RECORD_DTYPE)


def _range_ok(off, n, nbytes):
    return off >= 0 and n >= 0 and off + n <= nbytes


def record_fault(rec, L, nbytes, fastq):
    """0 = fine, 1 = a range outside the text, 2 = FASTQ output without a quality line as long as the read"""
    ho, qo, hl, ql = (int(rec[f]) for f in ("head_off", "qual_off", "head_len", "qual_len"))
    no_qual = qo == -1 and ql == 0
    if not _range_ok(ho, hl, nbytes) or not (no_qual or _range_ok(qo, ql, nbytes)):
        return 1
    if fastq and (no_qual or ql != L):
        return 2
    return 0


_LETTERS = np.full(256, ord("N"), np.uint8)
_LETTERS[:4] = np.frombuffer(b"ACGT", np.uint8)


def emit_ref(data, start, length, text, rec, spans=None, keep=None, min_len=0, out_format=TEXT_FASTA):
    """-> (text bytes, [input index of every read written]): a read that the device form drops is left out"""
    text = bytes(text)
    nN, nbytes, fastq = len(data), len(text), out_format == TEXT_FASTQ
    out, index = [], []
    for i in range(len(start)):
        s, L = int(start[i]), int(length[i])
        if keep is not None and not keep[i]:
            continue
        if s < 0 or L < 0 or s + L > nN:
            continue
        off, n = (0, L) if spans is None else (int(spans[i]["offset"]), int(spans[i]["length"]))
        if off < 0 or n < 0 or off + n > L or n < min_len:
            continue
        if record_fault(rec[i], L, nbytes, fastq):
            continue
        ho, hl = int(rec[i]["head_off"]), int(rec[i]["head_len"])
        name = text[ho + 1:ho + hl] if hl > 0 else b""
        bases = _LETTERS[np.asarray(data[s + off:s + off + n]).view(np.uint8)].tobytes()
        if fastq:
            q = int(rec[i]["qual_off"]) + off
            out.append(b"@" + name + b"\n" + bases + b"\n+\n" + text[q:q + n] + b"\n")
        else:
            out.append(b">" + name + b"\n" + bases + b"\n")
        index.append(i)
    return b"".join(out), index
