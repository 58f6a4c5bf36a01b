"""CPU: the component rules (tests/components_ref.py, include/cfrk_abi.h "Unitig components" and "Read components")
against a breadth-first search and their stated properties on random rows and on the planted graphs; the compaction
property on the reference compaction; the ABI and the Python mirror as far as they go without a GPU; the formatter of
libcfrk_host.so against the reference text; the host-check program under the sanitizers; the CLI's refusals; the kernels
of unitig_components.hip use no scratch memory and no LDS, and the hook kernel touches parent[] through atomics only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from . import compact_ref as cr
from . import components_ref as cc
from . import tips_ref as tr
from . import unitig_links_ref as lr
from . import unitig_ref as ur
from . import weak_ref as wr
from .test_kernel_resources import CSRC, HIPCC, ROOT, _functions
from .weak_cases import PARAMS, ref

NEW_CALLS = ("cfrk_global_unitig_components", "cfrk_global_unitig_components_device", "cfrk_global_read_components",
             "cfrk_global_read_components_device")
REC_DTYPE = np.dtype([("kc", "<u8"), ("n_kmers", "<u4"), ("flags", "<u4")])


@pytest.fixture(scope="module")
def built():
    import cfrk_amd
    if not os.path.exists(cfrk_amd.library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return cfrk_amd


@pytest.fixture(scope="module")
def host():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host"), "../libcfrk_host.so"], stdout=subprocess.DEVNULL)
    L = C.CDLL(os.path.join(ROOT, "cfrk_amd", "libcfrk_host.so"))
    L.cfrk_host_format_components.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_char_p, C.c_size_t]
    L.cfrk_host_format_components.restype = C.c_size_t
    L.cfrk_host_tag_components.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_void_p, C.c_int64, C.c_char_p, C.c_size_t]
    L.cfrk_host_tag_components.restype = C.c_size_t
    return L


@pytest.fixture(scope="module")
def cli(built):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def test_abi_declares_and_exports_the_component_calls(built):
    syms = built.abi_symbols()
    L = C.CDLL(built.library_path())
    for s in NEW_CALLS:
        assert s in syms and hasattr(L, s), s
    assert built.UNITIG_COMPONENT_DTYPE.itemsize == 32 and built.COMPONENT_STATS_DTYPE.itemsize == 32
    assert built.READ_COMPONENT_DTYPE.itemsize == 16 and built.READ_COMPONENT_STATS_DTYPE.itemsize == 32
    assert built.UNITIG_COMPONENT_DTYPE == cc.UNITIG_COMPONENT_DTYPE and built.READ_COMPONENT_DTYPE == cc.READ_COMPONENT_DTYPE
    assert (built.CFRK_COMP_NONE, built.CFRK_READ_COMP_SPLIT, built.CFRK_READ_COMP_DROPPED) == (cc.COMP_NONE, cc.SPLIT, cc.DROPPED)
    for name in ("unitig_components", "unitig_components_device", "read_components", "read_components_device", "drop_small_components"):
        assert callable(getattr(built.GlobalCounter, name))


# ------------------------------------------------------------------ the rule on random rows

def _random_graph(rng, nS, canonical, density):
    m = int(nS * density)
    frm, to = np.sort(rng.integers(0, nS, m)), rng.integers(0, nS, m)
    flags = rng.integers(0, 4, m).astype(np.uint32) if canonical else np.zeros(m, np.uint32)
    rows = np.zeros(m, lr.UNITIG_LINK_DTYPE)
    rows["to"], rows["flags"] = to, flags
    ptr = np.zeros(nS + 1, np.int64)
    np.cumsum(np.bincount(frm, minlength=nS), out=ptr[1:])
    rec = np.zeros(nS, REC_DTYPE)
    rec["n_kmers"] = rng.integers(1, 40, nS)
    rec["kc"] = rng.integers(1, 1 << 40, nS)
    return rec, ptr, rows


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("density", [0.0, 0.3, 0.7, 1.5])
def test_reference_against_a_breadth_first_search(canonical, density):
    rng = np.random.default_rng(int(density * 10) + 100 * canonical)
    for nS in (1, 2, 63, 300):
        rec, ptr, rows = _random_graph(rng, nS, canonical, density)
        for drop in (None, (rng.integers(0, 3, nS) == 0).astype(np.uint8), np.ones(nS, np.uint8)):
            comp, table, stats = cc.components(rec, ptr, rows, drop)
            assert (comp == cc.components_bfs(nS, ptr, rows, drop)).all()
            kept = comp != cc.COMP_NONE
            assert (kept == (np.ones(nS, bool) if drop is None else drop == 0)).all()
            # ids ascend by first; first is the smallest member; every id below n_components is used
            assert (np.diff(table["first"].astype(np.int64)) > 0).all()
            for c, row in enumerate(table):
                members = np.flatnonzero(comp == c)
                assert len(members) == row["n_unitigs"] >= 1 and members[0] == row["first"]
                assert int(rec["n_kmers"][members].sum()) == row["n_kmers"]
                assert sum(int(x) for x in rec["kc"][members]) % 2 ** 64 == row["kc"]
            # the table's sums are the kept totals
            src = np.repeat(np.arange(nS), np.diff(ptr))
            live = kept[src] & kept[rows["to"]]
            assert stats == {"n_components": len(table), "n_unitigs": int(kept.sum()), "n_kmers": int(rec["n_kmers"][kept].sum()),
                             "n_links": int(live.sum())}
            assert int(table["n_links"].sum()) == stats["n_links"] and int(table["n_unitigs"].sum()) == stats["n_unitigs"]
            # the order of the links inside a row changes nothing
            perm = rows.copy()
            for j in range(nS):
                perm[ptr[j]:ptr[j + 1]] = rng.permutation(perm[ptr[j]:ptr[j + 1]])
            again = cc.components(rec, ptr, perm, drop)
            assert again[0].tobytes() == comp.tobytes() and again[1].tobytes() == table.tobytes() and again[2] == stats


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [12, 21, 33])
def test_compaction_keeps_the_partition(k, canonical):
    """with drop, the partition of the kept unitigs is the partition of the reference compaction's unitigs, under the links
    of the reduced dictionary, pulled back through `into`: compaction merges only what a link joined"""
    table, units, link_ptr, links = ref(k, canonical)
    rec = ur.layout(units)[3]
    drop = (wr.weak(units, link_ptr, links, canonical, *PARAMS(k)[4])[0] != 0).astype(np.uint8)
    assert drop.any()
    comp = cc.components(rec, link_ptr, links, drop)[0]
    new, into, stats = cr.compact(units, link_ptr, links, drop, k, canonical)
    gone = [x for j in np.flatnonzero(drop) for x in tr.unit_kmers(units[j][0], k, canonical)]
    new_ptr, new_links = lr.links(new, tr.masked_table(table, gone, canonical), k, canonical)
    comp_new = cc.components(ur.layout(new)[3], new_ptr, new_links)[0]
    number, pulled = {}, np.full(len(units), cc.COMP_NONE, np.uint32)
    for j in np.flatnonzero(drop == 0):
        pulled[j] = number.setdefault(int(comp_new[int(into[j]["unitig"])]), len(number))
    assert (pulled == comp).all() and len(number) >= 3


# ------------------------------------------------------------------ reads

def test_read_rule_by_hand():
    HIT = np.dtype([("unitig", "<u4"), ("unitig_at", "<u4"), ("read_off", "<u4"), ("n_windows", "<u4")])
    comp = np.array([0, 0, 1, cc.COMP_NONE], np.uint32)
    rows = [[], [(2, 3), (0, 7), (1, 7)], [(3, 9)], [(3, 9), (2, 1)], [(0, 1), (1, 1)]]
    hits = np.array([(u, 0, 0, n) for r in rows for u, n in r], HIT)
    ptr = np.cumsum([0] + [len(r) for r in rows])
    out, stats = cc.read_components(ptr, hits, comp)
    N = cc.COMP_NONE
    assert out.tolist() == [(N, N, 0, 0), (0, 1, 7, cc.SPLIT), (N, N, 0, cc.DROPPED), (1, 1, 1, cc.DROPPED), (0, 0, 1, 0)]
    assert stats == {"n_assigned": 3, "n_unassigned": 2, "n_split": 1, "n_dropped": 2}
    assert cc.read_components_text(out) == "*\t*\t0\t0\n0\t1\t7\t1\n*\t*\t0\t2\n1\t1\t1\t2\n0\t0\t1\t0\n"


# ------------------------------------------------------------------ the formatter, the host check

def _format(L, table, k):
    table = np.ascontiguousarray(table, cc.UNITIG_COMPONENT_DTYPE)
    p = table.ctypes.data_as(C.c_void_p)
    n = L.cfrk_host_format_components(p, len(table), k, None, 0)
    buf = C.create_string_buffer(n + 1)
    assert L.cfrk_host_format_components(p, len(table), k, buf, n) == n
    assert buf.raw[n:] == b"\0"                                  # nothing behind the size it asked for
    return buf.raw[:n]


def test_components_formatter(host):
    assert _format(host, np.zeros(0, cc.UNITIG_COMPONENT_DTYPE), 21) == b""
    edge = np.array([(2 ** 64 - 1, 1, 0, 0, 1), (5, 0, 2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1), (15, 10, 3, 7, 2), (14, 10, 3, 8, 2), (1, 20, 0, 9, 1)],
                    cc.UNITIG_COMPONENT_DTYPE)
    for k in (1, 21, 64):
        assert _format(host, edge, k).decode() == cc.components_text(edge, k)
    assert cc.components_text(edge[2:5], 21) == "0\t7\t2\t10\t50\t15\t1.5\t3\n1\t8\t2\t10\t50\t14\t1.4\t3\n2\t9\t1\t20\t40\t1\t0.1\t0\n"
    lines = 0
    for k, canonical in ((12, False), (21, True), (33, False)):
        _, units, link_ptr, links = ref(k, canonical)
        table = cc.components(ur.layout(units)[3], link_ptr, links)[1]
        text = _format(host, table, k).decode()
        assert text == cc.components_text(table, k)
        # bases is what the members' sequences hold
        comp = cc.components(ur.layout(units)[3], link_ptr, links)[0]
        for c, line in enumerate(text.splitlines()):
            assert int(line.split("\t")[4]) == sum(len(units[j][0]) for j in np.flatnonzero(comp == c))
        lines += len(table)
    assert lines >= 9


def _tag(L, text, gfa, comp):
    comp = np.ascontiguousarray(comp, np.uint32)
    p = comp.ctypes.data_as(C.c_void_p)
    n = L.cfrk_host_tag_components(text, len(text), gfa, p, len(comp), None, 0)
    buf = C.create_string_buffer(n + 1)
    assert L.cfrk_host_tag_components(text, len(text), gfa, p, len(comp), buf, n) == n
    assert buf.raw[n:] == b"\0"
    return buf.raw[:n]


def test_component_tags(host):
    """the tags go behind km:f: / CL:i:1 and in front of the L tags of a header, and last on an S line; every other byte stays"""
    for k, canonical in ((12, False), (21, True), (33, False)):
        _, units, link_ptr, links = ref(k, canonical)
        comp = cc.components(ur.layout(units)[3], link_ptr, links)[0]
        for text in (ur.fasta_text(units), lr.fasta_text_links(units, link_ptr, links)):
            got = _tag(host, text, 0, comp)
            assert got == cc.tagged_fasta(text, comp) and got.count(b" CC:i:") == len(units)
            assert re.sub(rb" CC:i:\d+", b"", got) == text
        text = lr.gfa_text(units, k, link_ptr, links)
        got = _tag(host, text, 1, comp)
        assert got == cc.tagged_gfa(text, comp) and got.count(b"\tCC:i:") == len(units) and re.sub(rb"\tCC:i:\d+", b"", got) == text
    hand = b">0 LN:i:5 KC:i:9 km:f:9.0 CL:i:1 L:+:1:-\nACGTA\n>1 LN:i:4 KC:i:1 km:f:1.0\nACGT\n>2 LN:i:4 KC:i:1 km:f:1.0\nAAAA"
    assert _tag(host, hand, 0, [7, cc.COMP_NONE]) == b">0 LN:i:5 KC:i:9 km:f:9.0 CL:i:1 CC:i:7 L:+:1:-\nACGTA\n>1 LN:i:4 KC:i:1 km:f:1.0\nACGT\n>2 LN:i:4 KC:i:1 km:f:1.0\nAAAA"
    assert _tag(host, b"", 0, [1]) == b"" and _tag(host, b"H\tVN:Z:1.0\nS\t0\tAC\tLN:i:2\nL\t0\t+\t0\t+\t1M\n", 1, [4294967294]) == \
        b"H\tVN:Z:1.0\nS\t0\tAC\tLN:i:2\tCC:i:4294967294\nL\t0\t+\t0\t+\t1M\n"


def test_host_check_program_under_sanitizers(tmp_path):
    """tools/components_host_check.cpp: the formatter into buffers of exactly the size it asked for, under ASan and UBSan"""
    exe = tmp_path / "components_host_check"
    # (the runtimes linked into the program itself: it is a stand-alone program, whatever else the process loads)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", str(exe), os.path.join(ROOT, "tools", "components_host_check.cpp"),
                           os.path.join(ROOT, "cfrk_amd", "host", "cfrk_host.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "formatter and restatement agree" in p.stdout


# ------------------------------------------------------------------ the CLI's refusals

G = ["--global", "--unitigs-gfa", "g.gfa"]
U = ["--global", "--unitigs-out", "u.fa"]


@pytest.mark.parametrize("args, msg", [
    (["--global", "--unitigs-components", "c.tsv"], b"--unitigs-components needs --unitigs-out UFILE"),
    (G + ["--unitigs-components", "c.tsv"], b"--unitigs-components needs --unitigs-out UFILE"),
    (G + ["--unitigs-min-component-kmers", "5"], b"--unitigs-min-component-kmers needs --unitigs-out UFILE"),
    (U + ["--unitigs-map-components", "r.tsv"], b"--unitigs-map-components needs --unitigs-out UFILE and --unitigs-map QFILE"),
    (G + ["--unitigs-map", "q.fa", "--unitigs-map-out", "m.gaf", "--unitigs-map-components", "r.tsv"],
     b"--unitigs-map-components needs --unitigs-out UFILE and --unitigs-map QFILE"),
    (U + ["--unitigs-components"], b"--unitigs-components needs a value"),
    (G + ["--unitigs-component-tags"], b"--unitigs-component-tags needs --unitigs-out UFILE"),
    (U + ["--unitigs-min-component-kmers", "-1"], b"--unitigs-min-component-kmers needs a count"),
    (U + ["--unitigs-min-component-kmers", "x"], b"--unitigs-min-component-kmers needs a count"),
    (["--unitigs-out", "u.fa", "--unitigs-components", "c.tsv"], b"--unitigs-out needs --global on one device"),
])
def test_cli_refusals(cli, tmp_path, args, msg):
    p = subprocess.run([cli, str(tmp_path / "absent.fa"), str(tmp_path / "out"), "21"] + args, cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode == 1 and msg in p.stderr, p.stderr
    assert not any((tmp_path / f).exists() for f in ("out", "c.tsv", "r.tsv", "u.fa", "g.gfa"))


@pytest.mark.parametrize("args", [
    U + ["--unitigs-components", "c.tsv"],
    U + ["--unitigs-min-component-kmers", "0"],
    U + G[1:] + ["--unitigs-component-tags", "--unitigs-links"],
    U + G[1:] + ["--unitigs-components", "c.tsv", "--unitigs-min-component-kmers", "42", "--unitigs-drop-weak", "--unitigs-clip-tips"],
    U + ["--unitigs-map", "q.fa", "--unitigs-map-out", "m.gaf", "--unitigs-map-components", "r.tsv", "--unitigs-map-paths"],
])
def test_cli_accepts(cli, tmp_path, args):
    """accepted: the command gets as far as its input, which does not exist"""
    p = subprocess.run([cli, str(tmp_path / "absent.fa"), str(tmp_path / "out"), "21"] + args, cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode != 0 and b"needs" not in p.stderr and b"need " not in p.stderr, p.stderr
    assert b"absent.fa" in p.stderr or b"cannot read q.fa" in p.stderr                      # (the query file is read first)


# ------------------------------------------------------------------ the kernels' resources, the hook's accesses

def test_component_kernels_use_no_scratch_and_no_lds(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "unitig_components.hip.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "unitig_components.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    names = []
    for name, ops, size in _functions(asm):
        if not re.search(r"\d(u[ct]|rc)_[a-z_]+_kernel", name):  # (the library scan is not this project's kernel)
            continue
        names.append(name)
        assert ops == 0, f"{name} has {ops} scratch instructions"
        assert not size, f"{name} reserves {size} bytes of scratch per thread"
    mine = ("uc_init_kernel", "uc_hook_kernel", "uc_flatten_kernel", "uc_label_kernel", "uc_table_kernel", "rc_mark_kernel", "rc_offer_kernel",
            "rc_split_kernel", "rc_rows_kernel")
    for kern in mine + ("ut_check_kernel",):
        assert sum(kern in x for x in names) == (2 if kern == "ut_check_kernel" else 1), kern
    for name in (x for x in names if any(m in x for m in mine)):
        tail = asm[asm.index("\n%s:" % name):]
        tail = tail[:tail.index(".Lfunc_end") + 4000]
        lds = re.search(r"; LDSByteSize: ?(\d+)", tail)
        vgprs = re.search(r"; NumVgprs: ?(\d+)", tail)
        assert lds and int(lds.group(1)) == 0, name
        assert vgprs and int(vgprs.group(1)) < 64, (name, vgprs and vgprs.group(1))


def test_hook_and_flatten_touch_parent_through_atomics_only():
    """read off the source: inside the hook and flatten kernels and the helpers they call, parent[] appears only as the
    operand of an agent-scope atomic"""
    text = open(os.path.join(CSRC, "unitig_components.hip")).read()
    for fn in ("uc_load", "uc_find", "uc_unite", "uc_hook_kernel", "uc_flatten_kernel"):
        at = text.index(" %s(" % fn)
        body = text[at:text.index("\n}\n", at)]
        for line in body.splitlines():
            code = line.split("//")[0]
            for m in re.finditer(r"parent\[", code):
                assert re.search(r"__hip_atomic_\w+\(&(w\.)?parent\[", code) and "__HIP_MEMORY_SCOPE_AGENT" in code, (fn, line)
        assert "parent" in body
