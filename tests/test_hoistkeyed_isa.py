"""Static guard on the gfx950 code of the keyed hoisted stage B kernels (CPU-only: hipcc cross-compiles, nothing runs):
hoist_mac_keyed_kernel and hoist_matvec_keyed_kernel look their key up in a client-major table through a block-uniform
index and must still keep every value in registers (no scratch), at or below 128 VGPRs -- four waves per SIMD, the bar
hoist_matvec_kernel sits at.  Their register counts are printed next to the single-client siblings' from the same
compile.  Only the `.set` resource lines of the assembly are read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

KEYED = ("hoist_mac_keyed_kernel", "hoist_matvec_keyed_kernel")
SIBLINGS = ("hoist_mac_kernel", "hoist_matvec_kernel")


def resources(text, symbol):
    """{field: value} of the `.set <symbol>.<field>, <value>` lines of one kernel."""
    return {f: v for f, v in re.findall(r"\.set %s\.(\w+), (\d+)" % re.escape(symbol), text)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_keyed_hoisted_stage_b_stays_in_registers(tmp_path):
    asm = tmp_path / "hoistkeyed_probe.s"
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-Wno-unused-function", "-I", os.path.join(ROOT, "fhe.rs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "isa", "hoistkeyed_probe.cpp"), "-o", str(asm)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()
    for kernel in KEYED + SIBLINGS:
        # (the length prefix of the mangled name keeps hoist_mac_kernel from matching hoist_mac_keyed_kernel)
        names = sorted(set(re.findall(r"\.set (_ZN3fhe1k%d%s\w*)\.private_seg_size" % (len(kernel), kernel), text)))
        assert len(names) == 1, (kernel, names)
        res = resources(text, names[0])
        print(names[0], "vgpr", res.get("num_vgpr"), "sgpr", res.get("numbered_sgpr"), "scratch", res.get("private_seg_size"))
        if kernel in KEYED:
            assert int(res["private_seg_size"]) == 0, (names[0], res)
            assert int(res["num_vgpr"]) <= 128, (names[0], res)
