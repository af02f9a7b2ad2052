"""Static guard on the gfx950 code of the lift kernels (CPU-only: hipcc cross-compiles, nothing runs): the instances
for 3, 4, 5, 9 and 16 moduli -- the stock parameter sets, C2 and C5's chain --, with and without the limb output, keep their digit and
limb arrays in registers (zero private segment, no spills), and every scalar instruction they issue is a load, an ALU
operation or control flow: nothing writes memory from the scalar unit."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# the scalar mnemonics a kernel may use: loads from memory, waits, ALU and control flow
SCALAR_OK = re.compile(
    r"s_(load_dword(x\d+)?|buffer_load_dword(x\d+)?|waitcnt\w*|nop|endpgm|barrier|branch|cbranch_\w+|setprio|sleep|"
    r"(mov|movk|cmov|cmovk|not|wqm|brev|bcnt\d|ff\d|flbit|sext|abs|and|or|xor|nand|nor|xnor|andn2|orn2|add|addc|addk|sub|"
    r"subb|mul|mulk|mul_hi|min|max|lshl|lshl\d_add|lshr|ashr|bfe|bfm|cselect|cmp_\w+|cmpk_\w+|bitcmp\d|bitset\d|"
    r"pack_\w+|getpc|and_saveexec|or_saveexec|xor_saveexec|andn2_saveexec|orn2_saveexec|andn\d_wrexec)_?[a-z]?\d*(_[a-z]\d+)?)$")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_lift_instances_stay_in_registers(tmp_path):
    asm = tmp_path / "noise_probe.s"
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-Wno-unused-function", "-I", os.path.join(ROOT, "fhe.rs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "isa", "noise_probe.cpp"), "-o", str(asm)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()
    sym = r"_ZN3fhe1k11lift_kernelILi(\d+)ELb([01])E\w+"
    scratch = {(int(l), int(b)): int(v) for l, b, v in re.findall(r"\.set " + sym + r"\.private_seg_size, (\d+)", text)}
    assert sorted(scratch) == [(l, b) for l in (3, 4, 5, 9, 16) for b in (0, 1)], sorted(scratch)
    assert all(v == 0 for v in scratch.values()), scratch
    # the kernels' metadata: no spilled registers
    spills = re.findall(r"\.name:\s+" + sym + r"\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert len(spills) == 10, len(spills)
    assert all(s == "0" and v == "0" for _l, _b, s, v in spills), spills
    # the kernels' bodies: what the scalar unit does
    bodies = re.findall(r"^(" + sym + r"):[^\n]*\n(.*?)^\.Lfunc_end", text, flags=re.M | re.S)
    assert len(bodies) == 10, len(bodies)
    for name, _l, _b, body in bodies:
        mnemonics = set(re.findall(r"^\s+(s_[a-z0-9_]+)", body, flags=re.M))
        assert mnemonics and any(m.startswith("s_load_dword") for m in mnemonics), name
        bad = sorted(m for m in mnemonics if not SCALAR_OK.match(m))
        assert not bad, (name, bad)
