"""What the device FASTA parser's tests rest on, checked without a GPU: the host parser says about every generated text
what tests/ingest_cases.py expects, the capacities the ABI promises hold for the host parser, --device-parse refuses
its bad combinations before a device is opened, and the new constants are mirrored."""
import os
import re
import subprocess

import pytest

from . import ingest_cases as ic

ROOT = ic.ROOT
CLI = os.path.join(ROOT, "cfrk_amd", "cfrk")


@pytest.fixture(scope="module")
def random_texts():
    return ic.random_texts()


def test_host_parser_accepts_and_rejects_the_cases_as_stated():
    for name, raw, want_native, want_compat in ic.grammar_cases() + ic.seam_cases():
        assert ic.host_parse(raw, ic.NATIVE)[0] == want_native, name
        assert ic.host_parse(raw, ic.COMPAT)[0] == want_compat, name
    for name, raw, _ in ic.cr_run_cases():             # (the device parser refuses some of these: the host parser none)
        assert ic.host_parse(raw, ic.NATIVE)[0] == 0 and ic.host_parse(raw, ic.COMPAT)[0] == 0, name
    raw = ic.scan_block_case()
    assert len(raw) == (ic.SCAN_TILES + 3) * ic.T
    assert ic.host_parse(raw, ic.NATIVE)[0] == 0


def test_capacity_bound_holds_for_the_host_parser(random_texts):
    """cap_data = nbytes and cap_reads = (nbytes + 1) / 2 always suffice (include/cfrk_abi.h)"""
    texts = random_texts + [c[1] for c in ic.grammar_cases() + ic.seam_cases()]
    ok = 0
    for raw in texts:
        for flags in (ic.NATIVE, ic.COMPAT):
            rc, got = ic.host_parse(raw, flags)
            if rc:
                assert rc in (-2, -3)
                continue
            data, start, length = got
            assert len(data) <= len(raw) and len(start) <= (len(raw) + 1) // 2, (len(raw), len(data), len(start))
            ok += 1
    assert ok > 150          # (the generator must not drift into texts that are all refused)
    assert ic.host_parse(b">\n" * 50 + b">", ic.NATIVE)[1][1].size == 51      # the bound on the reads is met: 101 bytes


def test_random_texts_cover_errors_and_both_line_endings(random_texts):
    rcs = [ic.host_parse(raw, ic.COMPAT)[0] for raw in random_texts]
    assert rcs.count(0) > 40 and rcs.count(-2) > 5 and rcs.count(-3) > 10
    assert sum(b"\r\n" in t for t in random_texts) > 40 and sum(b"\r" not in t for t in random_texts) > 20


@pytest.mark.parametrize("args", [
    ["--device-parse"],                                     # without --global
    ["--global", "--device-parse", "--gpus", "2"],
    ["--global", "--device-parse", "--batch", "2"],
    ["--sparse", "--device-parse"],
    ["--native", "--device-parse"],
])
def test_device_parse_usage_errors_exit_before_a_device_is_opened(tmp_path, args):
    out = tmp_path / "out.cfrk"
    # (the input does not exist: a run that got as far as reading it would say so instead)
    r = subprocess.run([CLI, str(tmp_path / "missing.fasta"), str(out), "15"] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert "--device-parse needs --global on one device" in r.stderr or "--sparse is a per-read mode" in r.stderr
    assert "cannot read" not in r.stderr and not out.exists()


def test_constants_are_mirrored():
    import cfrk_amd
    from cfrk_amd import lib
    text = open(os.path.join(ROOT, "include", "cfrk_abi.h")).read()
    for name in ("CFRK_FASTA_TILE_BYTES", "CFRK_FASTA_SCAN_TILES", "CFRK_FASTA_MAX_CR_RUN"):
        assert getattr(lib, name) == int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert lib.CFRK_FASTA_TILE_BYTES % 4096 == 0
    assert {"cfrk_fasta_parse", "cfrk_fasta_parse_device", "cfrk_memcpy_h2d_staged"} <= set(cfrk_amd.abi_symbols())
