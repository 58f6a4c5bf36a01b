"""CPU-side check of the partition front end's word arithmetic: tools/front_end_host_check.cpp restates the chunk loader
(common.h: dev_load_chunk32), the canonical m-mers (msp_dev.h: msp_minimizers) and the validity smear (msp.hip: p1_tile)
in their earlier and their present form, with v_alignbit_b32, v_perm_b32 and v_mul_hi_u32 emulated, and compares them with
each other and with the base-by-base definitions.  Built with the sanitizers and run as a program of its own."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_check_program_under_sanitizers(tmp_path):
    """>= 10^6 chunks with every invalid byte value, all-one-base and period-2/4 strings, strings followed by their reverse
    complement, m = 12, 13, 14, 16, k = 16..32; the program exits non-zero on the first difference"""
    exe = tmp_path / "front_end_host_check"
    # (the runtimes linked into the program itself: it is a stand-alone program, whatever else the process loads)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", str(exe), os.path.join(ROOT, "tools", "front_end_host_check.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"old and new front end agree: (\d+) chunks \((\d+) invalid bytes, every value seen\), (\d+) m-mers \((\d+) palindromic\)", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) >= 1_000_000 and int(m.group(4)) >= 10_000


def test_the_kernels_and_the_host_check_state_the_same_forms():
    """the lines that carry the rewritten arithmetic are in the device sources as the host check restates them"""
    src = lambda *p: open(os.path.join(ROOT, *p)).read()
    check = src("tools", "front_end_host_check.cpp")
    common, dev, msp = src("cfrk_amd", "csrc", "common.h"), src("cfrk_amd", "csrc", "msp_dev.h"), src("cfrk_amd", "csrc", "msp.hip")
    for text in ("0x07030c0cu", "0x0c0c0703u", "0x10080402u", "0x40100401u", "0x7C7C7C7Cu"):
        assert text in common and text in check, text
    squeeze = lambda s: re.sub(r"__builtin_amdgcn_|\s+", "", s)
    for line, where in (("acc = alignbit(umulhi(f, 0x10080402u), acc, 4);", common),
                        ("RS[i] = fsh ? alignbit(R[i], R[i + 1], 32 - fsh) : R[i];", dev),
                        ("Q0 |= alignbit(Q0, Q1, 32 - w);", msp), ("Q1 |= alignbit(Q1, Q2, 32 - w);", msp), ("Q2 |= Q2 << w;", msp),
                        ("Q0 |= alignbit(Q0, Q1, 32 - (k - w));", msp), ("Q1 |= alignbit(Q1, Q2, 32 - (k - w));", msp)):
        assert squeeze(line) in squeeze(check), line
        assert squeeze(line).replace("umulhi", "__umulhi") in squeeze(where), line
