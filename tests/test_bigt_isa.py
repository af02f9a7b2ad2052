"""Static guard on the gfx950 code of the kernels for plaintext moduli above 64 bits (CPU-only: hipcc cross-compiles,
nothing runs): the compile-time bigt_tail_kernel instances for the (P, W_t) of the five parameter sets of
tests/bigt_ref.py and bigt_project_kernel<2 | 3 | 4> keep their limbs in registers -- zero private segment, no spills."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_bigt_instances_stay_in_registers(tmp_path):
    asm = tmp_path / "bigt_probe.s"
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-Wno-unused-function", "-I", os.path.join(ROOT, "fhe.rs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "isa", "bigt_probe.cpp"), "-o", str(asm)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()
    tail = r"_ZN3fhe1k16bigt_tail_kernelILi(\d+)ELi(\d+)E\w+"
    proj = r"_ZN3fhe1k19bigt_project_kernelILi(\d+)E\w+"
    scratch = {(int(p), int(w)): int(v) for p, w, v in re.findall(r"\.set " + tail + r"\.private_seg_size, (\d+)", text)}
    assert sorted(scratch) == [(3, 2), (4, 2), (4, 3), (6, 2), (6, 4)], sorted(scratch)
    assert all(v == 0 for v in scratch.values()), scratch
    scratch = {int(w): int(v) for w, v in re.findall(r"\.set " + proj + r"\.private_seg_size, (\d+)", text)}
    assert sorted(scratch) == [2, 3, 4], sorted(scratch)
    assert all(v == 0 for v in scratch.values()), scratch
    # the kernels' metadata: no spilled registers
    for sym, count in ((tail, 5), (proj, 3)):
        spills = re.findall(r"\.name:\s+(" + sym + r")\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", text)
        assert len(spills) == count, len(spills)
        assert all(s[-2] == "0" and s[-1] == "0" for s in spills), spills
