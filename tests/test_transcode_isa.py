"""Static guard on the gfx950 code of the bit-stream kernels (CPU-only: hipcc cross-compiles, nothing runs): every
whole-row instance of encode_stream_kernel the stock parameter sets launch -- integer and F64, 4096 ... 16384 points -- and
transcode_ew_kernel keep their values in registers (no scratch)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_transcode_instances_use_no_scratch(tmp_path):
    asm = tmp_path / "transcode_probe.s"
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-Wno-unused-function", "-I", os.path.join(ROOT, "fhe.rs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "isa", "transcode_probe.cpp"), "-o", str(asm)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()
    scratch = dict(re.findall(r"\.set (_ZN3fhe1k20encode_stream_kernelILi\w+)\.private_seg_size, (\d+)", text))
    assert len(scratch) == 15, sorted(scratch)     # 3 tile sizes x 5 (narrow, general, F64 x 3)
    for name, b in scratch.items():
        assert int(b) == 0, (name, b)
    found = re.findall(r"\.set _ZN3fhe1k19transcode_ew_kernel\w*\.private_seg_size, (\d+)", text)
    assert found == ["0"], found
