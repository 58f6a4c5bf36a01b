#!/usr/bin/env python3
"""Record what a `cfrk` binary does at its option stage: exit status and stderr over a fixed corpus of argument lists.

  python tools/record_cli_refusals.py CFRK [--commit REV] [--out tests/golden/cli_option_stage.jsonl]

The fixture tests/golden/cli_option_stage.jsonl is recorded with this tool from a build of the commit BEFORE a change to
the command's option handling, never from the code under test; tests/test_cli_options_cpu.py replays it against the
built command.  No device is needed: every case either is refused before the input is read, or gets as far as the input,
which does not exist.

Every case runs in an empty temporary directory of its own, with the input `<TMP>/missing.fasta` missing; a case may
first write small files there (a query file, or -- the cases of tests/test_fastq_cpu.py, which sniff the input -- the
input itself).  stderr is recorded with the directory's path replaced by <TMP>.

The corpus, in this order (deterministic: the tables below, the tests' own parametrisations in file order, SEED):
  1. every option alone, with a valid value where it takes one, without and with --global;
  2. every option that takes a value, with each of BAD_VALUES, under --global;
  3. every case of the `test_cli_refus*` parametrisations of tests/*_cpu.py, built as the test builds it;
  4. PAIRS unordered pairs of options, sampled by random.Random(SEED).sample from all pairs in table order, each with
     valid values under --global.

Each case is classified from the recorded run itself:
  refused   exit status 1 and no "cannot read" on stderr: the replay demands the identical status and stderr;
  accepted  stderr names the missing input ("cannot read <TMP>/missing.fasta"): the replay demands that string;
  anything else (a run that needs a device or a real count file to get further) is dropped, and counted.

The fixture is small on purpose: a first line (the commit, the corpus' size, the keys of the accepted and of the dropped
cases), then one line per distinct refusal with the keys of the cases that got it.  load() joins it with corpus() again.
"""
import argparse
import hashlib
import importlib
import inspect
import itertools
import json
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261020
PAIRS = 300
BAD_VALUES = ["", "x", "-1", "0", "257", "4294967296"]
QUERY_TEXT = ">a\nACGTACGTACGTACGTACGT\n>b\nTTGCATGCATGCATGCATGC\n"      # q.fa / q2.fa: two records, so that --paired has whole pairs
FILES = {"q.fa": QUERY_TEXT, "q2.fa": QUERY_TEXT}

# (option, a valid value or None for a flag); a value that names q.fa / q2.fa makes the case write that file first
OPTIONS = [
    ("--all-chunks", None), ("--native", None), ("--global", None), ("--canonical", None), ("--sparse", None), ("--binary", None),
    ("--timing", None), ("--parse-threads", "2"), ("--same-device", None), ("--device", "0"), ("--gpus", "1"), ("--batch", "2"),
    ("--histo-only", None), ("--estimate", None), ("--estimate-only", None), ("--auto-hint", None), ("--device-parse", None),
    ("--text-copy", "staged"), ("--format", "fasta"), ("--min-qual", "20"), ("--query-only", None), ("--paired", None),
    ("--pair-check", "off"), ("--pair-mode", "both"), ("--query2", "q2.fa"), ("--query", "q.fa"), ("--query-out", "o.q"),
    ("--query-db", "db.bin"), ("--query-stats", "s.tsv"), ("--stats-below", "2"), ("--filter-out", "f.fa"), ("--filter-out2", "f2.fa"),
    ("--filter-orphans", "orph.fa"), ("--filter-names", None), ("--filter-format", "fasta"), ("--filter-trim", "prefix"),
    ("--filter-min-len", "20"), ("--filter-min-count", "2"), ("--filter-max-count", "100"), ("--filter-min-median", "2"),
    ("--filter-max-median", "100"), ("--correct-out", "c.fa"), ("--correct-out2", "c2.fa"), ("--correct-names", None),
    ("--correct-format", "fasta"), ("--correct-report", "c.tsv"), ("--correct-min-count", "2"), ("--normalize-out", "n.fa"),
    ("--normalize-names", None), ("--normalize-format", "fasta"), ("--normalize-batch", "64"), ("--normalize-cutoff", "20"),
    ("--histo", "h.tsv"), ("--min-count", "2"), ("--max-count", "100"), ("--unitigs-links", None), ("--unitigs-clip-tips", None),
    ("--tip-report", "t.tsv"), ("--tip-ratio", "1.5"), ("--tip-max-kmers", "30"), ("--tip-rounds", "2"), ("--unitigs-pop-bubbles", None),
    ("--bubble-report", "b.tsv"), ("--bubble-ratio", "1.5"), ("--bubble-max-kmers", "30"), ("--bubble-max-diff", "1"),
    ("--simplify-rounds", "2"), ("--unitigs-out", "u.fa"), ("--unitigs-gfa", "g.gfa"), ("--unitigs-map", "q.fa"),
    ("--unitigs-map-out", "m.gaf"), ("--unitigs-min-count", "2"),
]
HEAD = ["<TMP>/missing.fasta", "<TMP>/o.txt", "15"]


def _case(args, files=None):
    files = dict(files or {})
    for a in args:
        if a in FILES:
            files[a] = FILES[a]
    return {"args": list(args), "files": files}


def _with(opt, value):
    return [opt] if value is None else [opt, value]


def _test_cases():
    """the `test_cli_refus*` parametrisations of tests/*_cpu.py, each case built as its test builds its command line"""
    sys.path.insert(0, ROOT)
    cases, skipped = [], []
    for name in sorted(f[:-3] for f in os.listdir(os.path.join(ROOT, "tests")) if f.endswith("_cpu.py")):
        with open(os.path.join(ROOT, "tests", name + ".py")) as f:
            if "def test_cli_refus" not in f.read():
                continue
        mod = importlib.import_module("tests." + name)
        for fname, fn in sorted(vars(mod).items()):
            if not fname.startswith("test_cli_refus") or not callable(fn):
                continue
            marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
            if len(marks) != 1:
                skipped.append(f"{name}::{fname}")               # (not parametrised: its cases live in its body)
                continue
            names = [n.strip() for n in marks[0].args[0].split(",")]
            bare = "[cli] + args" in inspect.getsource(fn)      # (the --query-db tests: no positional arguments in front)
            for row in marks[0].args[1]:
                row = dict(zip(names, row if len(names) > 1 else (row,)))
                args = list(row["args"]) if "args" in row else [row["opt"]]
                head, files = list(HEAD), {}
                if "k" in row:
                    head[2] = row["k"]
                if row.get("qtext") is not None:
                    files["q.txt"] = row["qtext"].decode()
                if "qtext" in row:
                    args = ["<TMP>/q.txt" if a == "Q" else a for a in args]
                if "text" in row:                                # (the input is there: its first byte decides the format)
                    head[0] = "<TMP>/in.txt"
                    files["in.txt"] = row["text"].decode()
                cases.append({"args": ([] if bare else head) + args, "files": files})
    return cases, skipped


def corpus():
    cases = []
    for opt, v in OPTIONS:                                                                   # 1
        cases.append(_case(HEAD + _with(opt, v)))
        cases.append(_case(HEAD + ["--global"] + _with(opt, v)))
    for opt, v in OPTIONS:                                                                   # 2
        if v is not None:
            cases += [_case(HEAD + ["--global", opt, bad]) for bad in BAD_VALUES]
    from_tests, skipped = _test_cases()                                                      # 3
    cases += from_tests
    pairs = list(itertools.combinations(OPTIONS, 2))                                         # 4
    for (a, va), (b, vb) in random.Random(SEED).sample(pairs, PAIRS):
        cases.append(_case(HEAD + ["--global"] + _with(a, va) + _with(b, vb)))
    return cases, skipped


def run_case(cfrk, case, timeout=60):
    """-> (exit status, stderr with the temporary directory's path replaced by <TMP>)"""
    with tempfile.TemporaryDirectory(prefix="cfrk_opt_") as tmp:
        for name, text in case["files"].items():
            with open(os.path.join(tmp, name), "w") as f:
                f.write(text)
        args = [a.replace("<TMP>", tmp) for a in case["args"]]
        p = subprocess.run([cfrk] + args, cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=timeout)
        return p.returncode, p.stderr.decode("utf-8", "replace").replace(tmp, "<TMP>")


def classify(status, stderr):
    if "cannot read <TMP>/missing.fasta" in stderr:
        return "accepted"
    if status == 1 and "cannot read" not in stderr:
        return "refused"
    return None


def key(case):
    """a case's name in the fixture: it survives cases that later tests add to the corpus around it"""
    return hashlib.sha256(json.dumps(case, sort_keys=True).encode()).hexdigest()[:8]


def load(path):
    """-> (head, cases, unrecorded): the fixture's first line; a case {"class", "args", "files", "status", "stderr"} for every
    case of corpus() that the recording kept, in corpus order; the cases of corpus() the fixture does not know (refusal tests
    added since).  The fixture holds no argument lists: it names cases by key(), and holds every distinct refusal once with
    the keys of its cases.  A recorded case that corpus() no longer builds is an error: record again, from the parent."""
    with open(path) as f:
        head, *groups = [json.loads(line) for line in f]
    kept = {k: {"class": "accepted", "status": None, "stderr": "cannot read <TMP>/missing.fasta"} for k in head["accepted"]}
    for g in groups:
        for k in g["cases"]:
            assert k not in kept and k not in head["dropped"], k
            kept[k] = {"class": "refused", "status": g["status"], "stderr": g["stderr"]}
    cases, seen = [], set()
    unrecorded = []
    for c in corpus()[0]:
        k = key(c)
        if k in kept and k not in seen:
            cases.append(dict(c, **kept[k]))
        elif k not in kept and k not in head["dropped"]:
            unrecorded.append(c)
        seen.add(k)
    gone = (set(kept) | set(head["dropped"])) - seen
    assert not gone, f"corpus() no longer builds {len(gone)} recorded case(s)"
    return head, cases, unrecorded


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("cfrk")
    ap.add_argument("--commit", default="unknown", help="the commit the binary was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "cli_option_stage.jsonl"))
    a = ap.parse_args()
    cases, skipped = corpus()
    accepted, dropped, refused = [], [], {}
    for c in cases:
        status, stderr = run_case(os.path.abspath(a.cfrk), c)
        kind = classify(status, stderr)
        if key(c) in accepted + dropped or any(key(c) in v for v in refused.values()):
            continue                                             # (two tests hold the same case)
        if kind == "refused":
            refused.setdefault((status, stderr), []).append(key(c))
        else:
            (accepted if kind else dropped).append(key(c))
    head = {"recorded_from": a.commit, "tool": "tools/record_cli_refusals.py", "seed": SEED, "pairs": PAIRS, "corpus": len(cases), "refused": sum(len(v) for v in refused.values()), "accepted": accepted, "dropped": dropped}
    with open(a.out, "w") as f:
        f.write(json.dumps(head) + "\n")
        for (status, stderr), which in refused.items():
            f.write(json.dumps({"status": status, "stderr": stderr, "cases": which}) + "\n")
    print(json.dumps(dict(head, accepted=len(accepted), dropped=len(dropped))))
    for s in skipped:
        print("not parametrised, not taken:", s)
    for c in cases:
        if key(c) in dropped:
            print("dropped:", " ".join(c["args"]))
    if len(dropped) * 20 > len(cases):
        sys.exit(f"{len(dropped)} of {len(cases)} cases dropped: more than one in twenty -- mend the corpus")
