"""Static guard on the gfx950 code of the hoisted matrix-vector product's stage B (CPU-only: hipcc cross-compiles, nothing
runs): hoist_matvec_kernel carries a second set of four 128-bit accumulators across hoist_mac_kernel's digit loop and must
still keep every value in registers (no scratch), at or below 128 VGPRs -- four waves per SIMD.  Only the `.set`
resource lines of the assembly are read."""
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
def test_fused_stage_b_uses_no_scratch(tmp_path):
    asm = tmp_path / "hoistmv_probe.s"
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-Wno-unused-function", "-I", os.path.join(ROOT, "fhe.rs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "isa", "hoistmv_probe.cpp"), "-o", str(asm)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()
    for kernel in ("hoist_matvec_kernel", "mbfv_sum_kernel"):
        names = sorted(set(re.findall(r"\.set (_ZN3fhe1k\d+%s\w*)\.private_seg_size" % kernel, text)))
        assert len(names) == 1, (kernel, names)
        res = resources(text, names[0])
        # (for comparison: hoist_mac_kernel has 79 VGPRs / 40 SGPRs)
        print(names[0], "vgpr", res.get("num_vgpr"), "sgpr", res.get("numbered_sgpr"), "scratch", res.get("private_seg_size"))
        assert int(res["private_seg_size"]) == 0, (names[0], res)
        if kernel == "hoist_matvec_kernel":
            assert int(res["num_vgpr"]) <= 128, (names[0], res)
