#!/usr/bin/env python3
"""Resource table of every kernel in two builds of the same .hip sources (device assembly, gfx950): VGPRs, SGPRs, LDS
and scratch bytes from the code-object metadata, waves per SIMD as the VGPRs alone allow (LDS, which bounds the 16-lane
kernels' workgroups per CU, is listed but not turned into waves), instruction lines between a kernel's symbol and its
.Lfunc_end, and whether the two bodies are the same text once labels are renumbered.  No GPU needed.

usage: python tools/kres_diff.py OLD_TREE NEW_TREE file.hip [file.hip ...]     (trees: repository roots)
Prints a markdown table; exit status 1 when LDS differs, scratch is not 0 or the waves per SIMD went down."""
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cfrk_amd", "csrc")


def flags():
    """HIPFLAGS of cfrk_amd/csrc/Makefile (its ARCH substituted), plus what stops the compiler at device assembly"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    var = lambda name: re.search(r"^" + name + r"\s*\?=\s*(.*)$", mk, re.M).group(1)
    return var("HIPFLAGS").replace("$(ARCH)", var("ARCH")).split() + ["-S", "--cuda-device-only"]


def assembly(tree, name):
    src = os.path.join(tree, "cfrk_amd", "csrc", name)
    with tempfile.NamedTemporaryFile(suffix=".s") as f:
        subprocess.check_call([HIPCC] + flags() + [src, "-o", f.name], stderr=subprocess.DEVNULL)
        return open(f.name).read()


def kernels(text):
    """{kernel symbol: (vgprs, sgprs, lds, scratch, instruction lines, normalised body)}"""
    meta = {}
    for blk in re.split(r"\n  - \.", text[text.index(".amdgpu_metadata"):]):
        sym = re.search(r"\.symbol:\s+(\S+)\.kd", blk)
        if sym:
            field = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
            meta[sym.group(1)] = (field("vgpr_count"), field("sgpr_count"), field("group_segment_fixed_size"),
                                  field("private_segment_fixed_size"))
    out = {}
    for name, m in meta.items():
        body = text[text.index("\n" + name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        lines, labels = [], {}
        for ln in body.split("\n")[2:]:                    # (behind the symbol's own line)
            ln = ln.split(";")[0].strip()
            if not ln or (ln.startswith(".") and not re.match(r"\.LBB\d+_\d+:", ln)):
                continue                                       # (comments, directives)
            lines.append(ln)
        text_ = "\n".join(lines)
        for lab in re.findall(r"\.LBB\d+_\d+", text_):       # labels renumbered in order of appearance
            labels.setdefault(lab, ".L%d" % len(labels))
        text_ = re.sub(r"\.LBB\d+_\d+", lambda x: labels[x.group(0)], text_)
        out[name] = m + (sum(not ln.endswith(":") for ln in lines), text_)
    return out


def waves(vgprs):
    return min(8, 512 // max(8, -(-vgprs // 8) * 8))       # 512 VGPRs per lane and SIMD, allocated in eights


def demangled(names):
    """_ZN12_GLOBAL__N_117read_stats_kernelILi16ELi0ELb1EEvPKa... -> read_stats_kernel<16,0,1>"""
    out = {}
    for n in names:
        m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", n)
        if not m:                                            # (not in an anonymous namespace: the symbol as it is)
            out[n] = n
            continue
        rest = n[m.end():]
        name, rest = rest[:int(m.group(1))], rest[int(m.group(1)):]
        args = re.match(r"I((?:L[ib]\d+E)+)E", rest)
        out[n] = name + ("<" + ",".join(re.findall(r"L[ib](\d+)E", args.group(1))) + ">" if args else "")
    return out


def main():
    old_tree, new_tree, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    bad = 0
    for f in files:
        old, new = kernels(assembly(old_tree, f)), kernels(assembly(new_tree, f))
        assert sorted(old) == sorted(new), (f, sorted(set(old) ^ set(new)))
        nice = demangled(sorted(old))
        print(f"\n`{f}`\n")
        print("| kernel | VGPRs | waves/SIMD | SGPRs | LDS bytes | scratch | instructions | same text |")
        print("|---|---|---|---|---|---|---|---|")
        for k in sorted(old, key=lambda n: nice[n]):
            a, b = old[k], new[k]
            pair = lambda i: f"{a[i]}" if a[i] == b[i] else f"{a[i]} -> {b[i]}"
            wa, wb = waves(a[0]), waves(b[0])
            print(f"| `{nice[k]}` | {pair(0)} | {wa if wa == wb else f'{wa} -> {wb}'} | {pair(1)} | {pair(2)} | {pair(3)} | "
                  f"{pair(4)} | {'yes' if a[5] == b[5] else 'no'} |")
            bad |= a[2] != b[2] or a[3] != 0 or b[3] != 0 or wb < wa
    return bad


if __name__ == "__main__":
    sys.exit(main())
