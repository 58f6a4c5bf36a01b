"""The partition kernel keeps its occupancy: no scratch, at most 80 VGPRs and 51 KB of LDS per workgroup
(three workgroups per CU, six waves per SIMD at __launch_bounds__(512, 6)).

Runs tools/p1_isa_account.py on the committed source (cross-compile to gfx950 assembly, no GPU).  It asserts the
resources only, not the instruction counts the tool prints: those are an account to work from, not a contract.
"""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_p1_headline_instantiation_resources():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "p1_isa_account.py"), "--json"],
                         check=True, capture_output=True, text=True, env=dict(os.environ, HIPCC=HIPCC)).stdout
    acc = json.loads(out.strip().split("\n")[-1])
    print(acc["kernel"], "VGPRs", acc["vgprs"], "LDS", acc["lds_bytes"], "scratch", acc["scratch_bytes"],
          "hot-path vector instructions per wave", acc["hot_vector_per_wave"])
    assert acc["scratch_bytes"] == 0 and acc["vgpr_spills"] == 0
    assert acc["vgprs"] <= 80
    assert acc["lds_bytes"] <= 51 * 1024
