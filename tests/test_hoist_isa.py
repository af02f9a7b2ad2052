"""Static guard on the gfx950 code of the hoisted rotations' stage B (CPU-only: hipcc cross-compiles, nothing runs):
hoist_mac_kernel keeps its values in registers (no scratch) although it indexes its exponent table, a kernel argument, at
run time.  Only the `.set` resource lines of the assembly are read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def resources(text, symbol):
    """{field: value} of the `.set <symbol>.<field>, <value>` lines of one kernel."""
    return {f: v for f, v in re.findall(r"\.set %s\.(\w+), (\d+)" % re.escape(symbol), text)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_hoisted_stage_b_uses_no_scratch(tmp_path):
    asm = tmp_path / "hoist_probe.s"
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-Wno-unused-function", "-I", os.path.join(ROOT, "fhe.rs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "isa", "hoist_probe.cpp"), "-o", str(asm)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()
    names = sorted(set(re.findall(r"\.set (_ZN3fhe1k\d+hoist_mac_kernel\w*)\.private_seg_size", text)))
    assert len(names) == 1, names
    res = resources(text, names[0])
    # (for comparison: ks_mac_keyed_kernel has 84 VGPRs / 40 SGPRs)
    print(names[0], "vgpr", res.get("num_vgpr"), "sgpr", res.get("numbered_sgpr"), "scratch", res.get("private_seg_size"))
    assert int(res["private_seg_size"]) == 0, (names[0], res)
