"""The option stage of the `cfrk` command against what the commit before the option table did: the fixture
tests/golden/cli_option_stage.jsonl was recorded by tools/record_cli_refusals.py from a build of that commit (its first
line says which) and is replayed here against the built command.  A case the recorded command refused before reading its
input must be refused with the identical exit status and stderr; a case it accepted (it got as far as the input, which
does not exist) must get as far again.  No device is needed.  The one intended difference is pinned on its own: an option
that takes a value and is the last argument is refused for every such option.  The parser and the rules under the
sanitizers, in a stand-alone program."""
import concurrent.futures
import importlib.util
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "cli_option_stage.jsonl")
SLICES = 8

_spec = importlib.util.spec_from_file_location("record_cli_refusals", os.path.join(ROOT, "tools", "record_cli_refusals.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

HEAD, CASES, _ = rec.load(FIXTURE)      # (the fixture names its cases by key: joined with the tool's corpus here)


LAST_VALUE_NOW_REFUSED = ["--device", "--gpus", "--batch", "--parse-threads", "--text-copy", "--format", "--min-qual"]


@pytest.fixture(scope="module")
def cli():
    import cfrk_amd
    if not os.path.exists(cfrk_amd.library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def test_fixture_is_whole_and_says_where_it_comes_from():
    assert len(HEAD["recorded_from"]) == 40 and HEAD["tool"] == "tools/record_cli_refusals.py"
    assert (HEAD["seed"], HEAD["pairs"]) == (rec.SEED, rec.PAIRS)
    assert HEAD["refused"] == sum(c["class"] == "refused" for c in CASES) and len(CASES) == HEAD["refused"] + len(HEAD["accepted"])
    # at most one case in twenty was dropped
    assert len(HEAD["dropped"]) * 20 <= len(CASES) + len(HEAD["dropped"])
    # every option of the table is there, and no recorded case ends in one of the seven options whose missing value the
    # recorded command let through: the fixture holds nothing that is meant to differ
    for opt, value in rec.OPTIONS:
        assert any(opt in c["args"] for c in CASES), opt
    assert not any(c["args"][-1] in LAST_VALUE_NOW_REFUSED for c in CASES)


@pytest.mark.parametrize("part", range(SLICES))
def test_option_stage_is_what_it_was(cli, part):
    mine = CASES[part::SLICES]
    # (an accepted case opens the devices where there are some before it reports the missing input: few at a time)
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        got = list(pool.map(lambda c: rec.run_case(cli, c), mine))
    wrong = []
    for c, (status, stderr) in zip(mine, got):
        if c["class"] == "refused" and (status, stderr) != (c["status"], c["stderr"]):
            wrong.append((c["args"], c["status"], c["stderr"], status, stderr))
        if c["class"] == "accepted" and c["stderr"] not in stderr:
            wrong.append((c["args"], "accepted", c["stderr"], status, stderr))
    assert not wrong, f"{len(wrong)} of {len(mine)} differ; the first: {wrong[0]}"


# the only intended difference from the recorded command: these seven used to let their own name through as a positional
# argument when no value followed (`cfrk in out 15 --gpus` ran with threads = atoi("--gpus"))
@pytest.mark.parametrize("opt", LAST_VALUE_NOW_REFUSED)
def test_a_missing_value_is_refused_for_every_value_option(cli, opt):
    for front in ([], ["--global"]):
        case = {"args": rec.HEAD + front + [opt], "files": {}}
        assert rec.run_case(cli, case) == (1, f"cfrk: {opt} needs a value\n")


def test_a_missing_value_is_refused_for_the_others_as_before(cli):
    for opt, value in rec.OPTIONS:
        if value is not None:
            assert rec.run_case(cli, {"args": rec.HEAD + [opt], "files": {}}) == (1, f"cfrk: {opt} needs a value\n"), opt


def test_host_check_program_under_sanitizers(tmp_path):
    """tools/cli_options_host_check.cpp: the parser and the rules on a few hundred argument vectors, under ASan and UBSan"""
    exe = tmp_path / "cli_options_host_check"
    host = os.path.join(ROOT, "cfrk_amd", "host")
    # (the runtimes linked into the program itself: it is a stand-alone program, whatever else the process loads)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", str(exe), os.path.join(ROOT, "tools", "cli_options_host_check.cpp"),
                           os.path.join(host, "cli_options.cpp"), os.path.join(host, "cfrk_host.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr[-2000:]
    assert "parser and rules held" in p.stdout
