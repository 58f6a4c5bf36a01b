"""CPU-side checks of the distinct sketch: the host functions of libcfrk_hip.so (estimate, merge, hint: no device
needed) against the numpy restatement of tests/sketch_ref.py, the accuracy of the format itself on read sets, the
two-rank merge of cfrk_amd/sharded.py over gloo, and the CLI's refusal of the new options without --global."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from . import hash_craft as hc
from . import sketch_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFRK_ERR_ARG = -1


@pytest.fixture(scope="module")
def built():
    import cfrk_amd
    if not os.path.exists(cfrk_amd.library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "csrc"), "-j4"],
                              stdout=subprocess.DEVNULL)
    return cfrk_amd


@pytest.fixture(scope="module")
def cli(built):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def _keys(n, seed):
    """n distinct one-word keys (their hashes are as good as random)"""
    return np.arange(n, dtype=np.uint64) + np.uint64(seed << 40)


def _regime_registers():
    """name -> registers: every regime of the estimator"""
    regs = {"empty": np.zeros(sr.M, np.uint8),
            "100 keys": sr.registers(_keys(100, 1), None, 31),
            "10^6 keys": sr.registers(_keys(1_000_000, 2), None, 31),
            "every register at 51": np.full(sr.M, sr.RANK_MAX, np.uint8),
            "every register at 1": np.ones(sr.M, np.uint8)}
    # both sides of the switch between linear counting and the harmonic mean (raw estimate 2.5 m), close to it
    for n in (34000, 38000, 40000, 41000, 42000, 44000, 48000):
        regs[f"{n} keys"] = sr.registers(_keys(n, 3), None, 31)
    return regs


def test_constants_are_mirrored_and_symbols_exported(built):
    assert built.CFRK_SKETCH_LOG2M == sr.LOG2M == 14 and built.CFRK_SKETCH_REGS == sr.M == 16384
    syms = built.abi_symbols()
    L = C.CDLL(built.library_path())
    for s in ("cfrk_distinct_sketch", "cfrk_distinct_sketch_device", "cfrk_sketch_estimate", "cfrk_sketch_merge",
              "cfrk_sketch_hint"):
        assert s in syms and hasattr(L, s)
    for name in ("distinct_sketch", "distinct_sketch_device"):
        assert callable(getattr(built.Context, name))


def test_restated_rank_and_bucket_follow_the_format():
    """the restatement itself, on hashes whose bucket and rank are plain to see"""
    h = np.array([0, 1, (1 << 50) - 1, 1 << 49, 1 << 50, ((sr.M - 1) << 50) | 1, (5 << 50) | (1 << 20)], np.uint64)
    regs = sr.registers_from_hashes(h)
    assert regs[0] == 51          # h = 0: the low 50 bits are zero -> rank 51 (beats 50, 1 and 1 of the same bucket)
    assert regs[1] == 51          # 1 << 50: bucket 1, low bits zero
    assert regs[sr.M - 1] == 50 and regs[5] == 30
    assert sr.registers_from_hashes(h[1:4])[0] == 50 and sr.registers_from_hashes(h[2:4])[0] == 1
    assert np.count_nonzero(regs) == 4


def test_estimate_equals_the_restatement_in_every_regime(built):
    seen = set()
    for name, regs in _regime_registers().items():
        want = sr.estimate(regs)
        got = built.sketch_estimate(regs)
        assert got == pytest.approx(want, rel=1e-12, abs=0), name
        if regs.any():
            seen.add(bool(sr.raw_estimate(regs) <= 2.5 * sr.M and (regs == 0).any()))
    assert seen == {True, False}
    assert built.sketch_estimate(np.zeros(sr.M, np.uint8)) == 0.0
    # the switch is taken on both sides of 2.5 m by sketches close to it
    near = [sr.raw_estimate(r) / sr.M for n, r in _regime_registers().items() if n.endswith("000 keys")]
    assert min(near) < 2.5 < max(near) and 2.0 < min(near) and max(near) < 3.2
    # every register at 51 has no zero register: the harmonic mean, not linear counting
    assert built.sketch_estimate(np.full(sr.M, 51, np.uint8)) == pytest.approx(
        0.7213 / (1 + 1.079 / sr.M) * sr.M * 2.0 ** 51, rel=1e-12)


def test_merge_equals_numpy_maximum(built):
    rng = np.random.default_rng(5)
    a = rng.integers(0, 52, sr.M).astype(np.uint8)
    b = rng.integers(0, 52, sr.M).astype(np.uint8)
    want = np.maximum(a, b)
    b0 = b.copy()
    out = built.sketch_merge(a, b)
    assert out is a and (a == want).all() and (b == b0).all()
    # the merge of two sketches is the sketch of the union
    k1, k2 = _keys(5000, 7), _keys(9000, 7)[3000:]
    u = sr.registers(np.union1d(k1, k2), None, 31)
    m = built.sketch_merge(sr.registers(k1, None, 31), sr.registers(k2, None, 31))
    assert (m == u).all()


def test_hint_equals_its_formula_and_is_clamped(built):
    for name, regs in _regime_registers().items():
        e = sr.estimate(regs)
        want = min(max(math.ceil(e * (1 + 4 * 1.04 / math.sqrt(sr.M))), 1 << 20), 1 << 31)
        assert built.sketch_hint(regs) == want == sr.hint(regs), name
    assert built.sketch_hint(np.zeros(sr.M, np.uint8)) == 1 << 20                  # clamped from below
    assert built.sketch_hint(np.full(sr.M, 51, np.uint8)) == 1 << 31               # and from above
    big = sr.registers(_keys(3_000_000, 9), None, 31)                             # unclamped: above 2^20
    assert (1 << 20) < built.sketch_hint(big) == math.ceil(sr.estimate(big) * 1.0325) < (1 << 31)


def test_null_arguments_are_refused(built):
    L = built.load_library()
    regs = np.zeros(sr.M, np.uint8)
    p = regs.ctypes.data_as(C.c_void_p)
    d, h = C.c_double(), C.c_uint64()
    assert L.cfrk_sketch_estimate(None, C.byref(d)) == CFRK_ERR_ARG
    assert L.cfrk_sketch_estimate(p, None) == CFRK_ERR_ARG
    assert L.cfrk_sketch_merge(None, p) == CFRK_ERR_ARG and L.cfrk_sketch_merge(p, None) == CFRK_ERR_ARG
    assert L.cfrk_sketch_hint(None, C.byref(h)) == CFRK_ERR_ARG and L.cfrk_sketch_hint(p, None) == CFRK_ERR_ARG
    assert L.cfrk_distinct_sketch_device(None, None, 0, 31, 0, None, None) == CFRK_ERR_ARG      # no context
    assert L.cfrk_distinct_sketch(None, None, None, None, 0, 0, 31, 0, None, None) == CFRK_ERR_ARG
    with pytest.raises(ValueError):
        built.sketch_estimate(np.zeros(100, np.uint8))


# (k, canonical, genome length, reads, read length): reads of a random genome with 1 % substitutions, half of them
# reverse-complemented; between 10^3 and 10^6 distinct keys
ACCURACY_CASES = [
    (8, False, 1500, 30, 100), (8, True, 60000, 3000, 100), (16, False, 20000, 500, 120), (16, True, 120000, 4000, 150),
    (31, True, 3000, 80, 150), (31, True, 60000, 1500, 150), (31, True, 500000, 14000, 150), (31, False, 40000, 700, 150),
    (33, False, 8000, 150, 150), (33, True, 150000, 5000, 150), (63, False, 500000, 14000, 150), (63, True, 30000, 900, 150),
]


@pytest.mark.parametrize("case", range(len(ACCURACY_CASES)))
def test_accuracy_of_the_format_on_read_sets(built, case):
    """|E - exact| / exact <= 4 * 1.04 / sqrt(m) on every read set: the hash alone stays within two standard errors
    on such inputs, so a failure means that the hash, the rank or the estimator changed"""
    k, canon, G, R, L = ACCURACY_CASES[case]
    data = sr.genome_reads(100 + case, G, R, L)
    lo, hi = sr.windows(data, k, canon)
    exact = sr.distinct(lo, hi)
    assert 1000 <= exact <= 1_500_000
    e = built.sketch_estimate(sr.registers(lo, hi, k))
    err = abs(e - exact) / exact
    print(f"k={k} canonical={canon}: exact {exact}, estimate {e:.1f}, relative error {err:.5f} (bound {sr.BOUND:.5f})")
    assert err <= sr.BOUND
    assert built.sketch_hint(sr.registers(lo, hi, k)) >= min(exact, 1 << 31)


def test_accuracy_cases_cover_the_range():
    assert {(8, False), (16, False), (31, True), (33, False), (63, False)} <= {(c[0], c[1]) for c in ACCURACY_CASES}
    sizes = [sr.distinct(*sr.windows(sr.genome_reads(100 + i, *ACCURACY_CASES[i][2:]), *ACCURACY_CASES[i][:2]))
             for i in (0, 6)]
    assert sizes[0] < 3000 and sizes[1] > 900_000


def test_window_enumerator_against_a_plain_loop():
    """the enumerator the GPU tests rely on, for both key widths, against base-by-base Python"""
    rng = np.random.default_rng(11)
    data = rng.integers(0, 4, 400, dtype=np.int8)
    data[[17, 90, 91, 250]] = -1
    data[300] = 4
    for k, canon in ((1, False), (5, True), (32, False), (32, True), (33, True), (64, False), (64, True)):
        want = []
        for p in range(len(data) - k + 1):
            w = data[p:p + k]
            if ((w < 0) | (w > 3)).any():
                continue
            x = 0
            for c in w:
                x = (x << 2) | int(c)
            if canon:
                x = min(x, hc.revcomp_int(x, k))
            want.append(x)
        lo, hi = sr.windows(data, k, canon)
        assert [int(h) << 64 | int(l) for l, h in zip(lo, hi)] == want, (k, canon)


def _gloo_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from cfrk_amd import sharded
    from tests import sketch_ref
    keys = np.arange(60000, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    lo, hi = sharded.shard_range(len(keys), rank, world)
    mine = sketch_ref.registers(keys[lo:hi], None, 31)
    before = mine.copy()
    got = sharded.merge_sketch(mine)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and (mine == before).all()
    got_t = sharded.merge_sketch(torch.from_numpy(mine), wire_device="cpu")
    assert torch.is_tensor(got_t) and (got_t.numpy() == got).all()
    q.put((rank, got.tobytes()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_merge_sketch_over_gloo():
    """each rank holds the registers of half the keys; merge_sketch gives every rank the registers of all keys"""
    import torch.multiprocessing as mp
    keys = np.arange(60000, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    want = sr.registers(keys, None, 31)
    assert (sr.registers(keys[:30000], None, 31) != want).any()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + ((os.getpid() + 977) % 2000)
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in range(2):
        assert (np.frombuffer(got[r], np.uint8) == want).all()


@pytest.mark.parametrize("opt", ["--auto-hint", "--estimate", "--estimate-only"])
def test_cli_refuses_the_estimate_options_without_global(cli, tmp_path, opt):
    """refused with status 1 and a message before any input is read or a device is opened"""
    out = tmp_path / "o.txt"
    p = subprocess.run([cli, str(tmp_path / "missing.fasta"), str(out), "15", opt], cwd=tmp_path, capture_output=True,
                       timeout=60)
    assert p.returncode == 1
    assert b"--estimate, --estimate-only and --auto-hint need --global" in p.stderr
    assert not out.exists()


def test_cli_refuses_estimate_only_with_other_outputs(cli, tmp_path):
    p = subprocess.run([cli, str(tmp_path / "missing.fasta"), str(tmp_path / "o.txt"), "15", "--global",
                        "--estimate-only", "--batch", "2"], cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode == 1 and b"not with --batch" in p.stderr


def test_sketch_kernels_use_no_scratch_and_the_small_lds_layout(tmp_path):
    from .test_kernel_resources import CSRC, HIPCC, _functions
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "sketch.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "sketch.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    names = []
    for name, ops, size in _functions(text):
        names.append(name)
        assert ops == 0, f"{name} has {ops} scratch instructions"
        assert not size, f"{name} reserves {size} bytes of scratch per thread"
    assert sum("sketch1_kernel" in n for n in names) == 2 and sum("sketch2_kernel" in n for n in names) == 2
    assert any("sketch_merge_kernel" in n for n in names)
    # the product holds the registers as packed bytes: 16 KiB + the four wave sums per workgroup
    import re
    lds = [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", text)]
    assert sorted(lds) == [0, 16400, 16400, 16400, 16400]
