"""Static guard on the gfx950 code of the baby-step/giant-step stage B kernels (CPU-only: hipcc cross-compiles, nothing
runs): bsgs_baby_kernel<GT> carries GT sets of four 128-bit accumulators across hoist_matvec_kernel's digit loop and
bsgs_giant_kernel carries hoist_mac_kernel's four across the giants; every shipped instance must keep every value in
registers (no scratch), and bsgs_baby_kernel<1> and bsgs_giant_kernel stay at or below 128 VGPRs -- four waves per SIMD,
the siblings' bar (the bodies they start from sit at 128 and 79).  The wider tiles' counts are printed, not pinned.  Only
the `.set` resource lines of the assembly are read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TILES = (1, 2, 4)   # the shipped instances of bsgs_baby_kernel (engine.hpp: matvec_bsgs)


def resources(text, symbol):
    """{field: value} of the `.set <symbol>.<field>, <value>` lines of one kernel."""
    return {f: v for f, v in re.findall(r"\.set %s\.(\w+), (\d+)" % re.escape(symbol), text)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_bsgs_stage_b_uses_no_scratch(tmp_path):
    asm = tmp_path / "bsgs_probe.s"
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-Wno-unused-function", "-I", os.path.join(ROOT, "fhe.rs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "isa", "bsgs_probe.cpp"), "-o", str(asm)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()
    baby = sorted(set(re.findall(r"\.set (_ZN3fhe1k\d+bsgs_baby_kernelILi(\d+)E\w*)\.private_seg_size", text)))
    assert sorted(int(gt) for _, gt in baby) == list(TILES), baby
    giant = sorted(set(re.findall(r"\.set (_ZN3fhe1k\d+bsgs_giant_kernel\w*)\.private_seg_size", text)))
    assert len(giant) == 1, giant
    for name, gt in baby + [(giant[0], "1")]:
        res = resources(text, name)
        print(name, "vgpr", res.get("num_vgpr"), "agpr", res.get("num_agpr"), "sgpr", res.get("numbered_sgpr"),
              "scratch", res.get("private_seg_size"))
        assert int(res["private_seg_size"]) == 0, (name, res)
        if int(gt) == 1:
            assert int(res["num_vgpr"]) <= 128, (name, res)
    # every engine launch site names an instance the probe covers
    engine = open(os.path.join(ROOT, "fhe.rs_amd", "csrc", "engine.hpp")).read()
    body = engine[engine.index("inline void matvec_bsgs("):]
    body = body[:body.index("\n}\n")]
    assert sorted(int(v) for v in re.findall(r"launch\(int_c<(\d+)>\{\}\)", body)) == list(TILES), "probe and engine disagree"
