#!/usr/bin/env python3
"""Call by call: the launches of the leaf kernel in the newest `rocprofv3 --kernel-trace` run under a directory -- the
timed ones' mean, standard deviation, minimum and maximum, every call's duration (warm-up included), and the mean of
the partition kernels' timed launches beside them.  One line, for same-box A/B rounds (tools/ab.sh prints averages
over all calls, warm-up included).

usage: python tools/kcalls.py <dir> <label> [--warmup W] [--log bench.log] [--kernel msp_p3_kernel]
  --warmup W   leading steps that are not timed (bench.py --warmup): the first W of the kernel's calls, and the same
               share of the partition kernels' calls
  --log FILE   the bench run's output: its JSON line's ms_per_step and digest are appended"""
import argparse
import csv
import glob
import json
import statistics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("label")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log")
    ap.add_argument("--kernel", default="msp_p3_kernel")
    a = ap.parse_args()
    f = sorted(glob.glob(a.dir + "/*/*kernel_trace.csv"))[-1]
    calls = {}
    for r in csv.DictReader(open(f)):
        name = r["Kernel_Name"]
        for key in (a.kernel, "msp_p1", "msp_p2"):
            if key in name:
                calls.setdefault(key, []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    p3 = [d for _, d in sorted(calls.get(a.kernel, []))]
    if len(p3) <= a.warmup:
        raise SystemExit("%s: %d calls of %s" % (f, len(p3), a.kernel))
    timed = p3[a.warmup:]
    out = "%-7s p3 timed n %d mean %.4f sd %.4f min %.4f max %.4f | all %s" % (
        a.label, len(timed), statistics.mean(timed), statistics.stdev(timed) if len(timed) > 1 else 0.0, min(timed), max(timed),
        " ".join("%.3f" % d for d in p3))
    for key, tag in (("msp_p1", "p1"), ("msp_p2", "p2")):
        ds = [d for _, d in sorted(calls.get(key, []))]
        ds = ds[len(ds) * a.warmup // len(p3):]
        out += (" | " if tag == "p1" else " ") + "%s %.4f" % (tag, statistics.mean(ds) if ds else float("nan"))
    if a.log:
        for ln in open(a.log):
            if ln.startswith("{") and "ms_per_step" in ln:
                j = json.loads(ln)
                out += " | ms_per_step %.3f digest %s" % (j["ms_per_step"], "/".join(x.lstrip("0") for x in j["digest"]))
    print(out)


if __name__ == "__main__":
    main()
