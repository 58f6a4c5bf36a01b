"""The leaf kernel keeps its occupancy -- 64 VGPRs (eight waves per SIMD), LDS for two workgroups per CU, a handful of
spills at phase boundaries -- and its scan of the complete stream stays marked part by part.

Runs tools/p3_isa_account.py on the committed source (cross-compile to gfx950 assembly, no GPU).  It asserts the
resources and that every part of the scan is found, not the instruction counts the tool prints: those are an account
to work from, not a contract.
"""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TOOL = os.path.join(ROOT, "tools", "p3_isa_account.py")


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    """msp.hip compiled once for the cases below"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("p3") / "msp.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "cfrk_amd", "csrc", "msp.hip"), "-o", out], check=True, capture_output=True)
    return out


def _account(asm, *args):
    out = subprocess.run([sys.executable, TOOL, "--asm", asm, "--json"] + list(args), check=True, capture_output=True, text=True).stdout
    return json.loads(out.strip().split("\n")[-1])


@pytest.mark.parametrize("canon", [1, 0])
def test_p3_headline_instantiation_resources_and_parts(assembly, canon):
    acc = _account(assembly, "--canon", str(canon))
    print(acc["kernel"], "VGPRs", acc["vgprs"], "LDS", acc["lds_bytes"], "scratch", acc["scratch_bytes"], acc["scan"])
    assert acc["vgprs"] <= 64
    assert acc["lds_bytes"] <= 80 * 1024                       # two workgroups in a CU's 160 KB
    assert acc["scratch_instructions"] <= 10 and acc["scratch_bytes"] <= 48
    parts = acc["parts"]
    for p in ("before", "LOAD", "HOME", "CACHE", "APPEND", "DRAIN", "MERGE", "after"):
        assert p in parts and parts[p]["segments"] >= 1, p
    # the specialised scan and the general one, two steps per trip each, and the peeled tail
    assert parts["HOME"]["segments"] >= 5 and parts["CACHE"]["segments"] == parts["HOME"]["segments"]
    # a home-slot step reads the table and adds to it: LDS instructions in its text, and vector ones for the hash
    assert parts["HOME"]["lds"] >= parts["HOME"]["segments"] and parts["HOME"]["vector"] > 0
    assert parts["DRAIN"]["lds"] > 0 and parts["APPEND"]["vector"] > 0
    # classes are told apart by prefix only, and everything in the kernel's text is in exactly one part
    total = sum(q[c] for q in parts.values() for c in ("vector", "scalar", "lds", "global"))
    assert total > 4000 and all(acc["scan"][c] == sum(parts[p][c] for p in parts if p not in ("before", "after"))
                                for c in ("vector", "scalar", "lds", "global"))


def test_p3_account_table_and_unknown_instantiation(assembly):
    txt = subprocess.run([sys.executable, TOOL, "--asm", assembly], check=True, capture_output=True, text=True).stdout
    assert "msp_p3_kernel<true, false>" in txt and "home-slot step" in txt and "VGPRs" in txt
    r = subprocess.run([sys.executable, TOOL, "--asm", assembly, "--canon", "7"], capture_output=True, text=True)
    assert r.returncode != 0 and "no instantiation" in (r.stderr + r.stdout)
