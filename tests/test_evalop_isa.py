"""The table of tests/evalop_shapes.py against what the release build compiles (CPU-only: nothing runs on a device).

The kernel symbols of the seven evaluation families in the gfx950 code object of fhe.rs_amd/libfhe_hip.so must be
exactly the reachable cells plus UNREACHABLE: an instance that a later change of the dispatcher adds fails here until
it is in the table -- and then in the census of tests/test_evalop_shapes_gpu.py until a shape reaches it.

Only symbol names are read: the offload bundle inside the library is located by its magic, the gfx950 entry's ELF
symbol table is walked, and the template arguments are decoded from the mangled names.  No instruction is inspected
and nothing is compiled (the library is the one __graft_entry__.build() made)."""
import os
import re
import struct

import pytest

import evalop_shapes as S
from helpers import HIP_LIB

BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(blob, arch="gfx950"):
    """The device code objects for `arch` in a host library: every uncompressed clang offload bundle is a 24-byte magic,
    a 64-bit entry count and per entry (offset, size, length of the target id, target id)."""
    out, at = [], blob.find(BUNDLE_MAGIC)
    while at >= 0:
        (count,) = struct.unpack_from("<Q", blob, at + len(BUNDLE_MAGIC))
        p = at + len(BUNDLE_MAGIC) + 8
        for _ in range(count):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            target = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if target.startswith("hip") and arch in target and size:
                out.append(blob[at + off:at + off + size])
        at = blob.find(BUNDLE_MAGIC, at + 1)
    return out


def elf_function_symbols(elf):
    """Names of the STT_FUNC symbols of a little-endian ELF64 image."""
    assert elf[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64 code object"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for _name, stype, _flags, _addr, off, size, link, _info, _align, entsize in sections:
        if stype not in (2, 11):    # SHT_SYMTAB, SHT_DYNSYM
            continue
        stroff = sections[link][4]
        for i in range(size // entsize):
            st_name, st_info = struct.unpack_from("<IB", elf, off + i * entsize)
            if st_info & 0xF == 2:  # STT_FUNC
                end = elf.index(b"\0", stroff + st_name)
                names.add(elf[stroff + st_name:end].decode())
    return names


_MANGLED = re.compile(r"^_ZN3fhe1k(\d+)")                    # fhe::k::<length><name>
_TEMPLATE = re.compile(r"(?:I((?:L[bi]\d+E)+)E)?E")          # <bool / int template arguments>, the end of the nested name


def cell_of_mangled(name):
    """_ZN3fhe1k10ntt_kernelILb1ELi12ELb0ELi1ELb0ELi0EEv... -> ("ntt_kernel", "true, 12, false, 1, false, 0"); None for
    a symbol of another family."""
    m = _MANGLED.match(name)
    if not m:
        return None
    family = name[m.end():m.end() + int(m.group(1))]
    if family not in S.FAMILIES:
        return None
    t = _TEMPLATE.match(name, m.end() + len(family))
    assert t, name
    args = [("true" if v == "1" else "false") if k == "b" else v for k, v in re.findall(r"L([bi])(\d+)E", t.group(1) or "")]
    return family, ", ".join(args)


def test_mangled_names_decode():
    assert cell_of_mangled("_ZN3fhe1k10ntt_kernelILb1ELi12ELb0ELi1ELb0ELi0EEEvPKmPmNS0_6RowMapE") == \
        ("ntt_kernel", "true, 12, false, 1, false, 0")
    assert cell_of_mangled("_ZN3fhe1k13ks_mac_kernelEPKmPmS3_m") == ("ks_mac_kernel", "")
    assert cell_of_mangled("_ZN3fhe1k17ntt_global_kernelILb0ELi3EEEvPKmPm") == ("ntt_global_kernel", "false, 3")
    assert cell_of_mangled("_ZN3fhe1k11lift_kernelILi3ELb0EEEvPKm") is None
    assert cell_of_mangled("_ZN3fhe1k20ks_mac_keyed_kernelEPKm") is None


@pytest.mark.skipif(not os.path.exists(HIP_LIB), reason="the HIP library is not built (__graft_entry__.build())")
def test_compiled_instances_equal_the_table():
    with open(HIP_LIB, "rb") as f:
        blob = f.read()
    objs = code_objects(blob)
    assert objs, "no uncompressed gfx950 code object in the library"
    compiled = set()
    for elf in objs:
        compiled |= {cell_of_mangled(s) for s in elf_function_symbols(elf)} - {None}
    table = S.all_cells() | set(S.UNREACHABLE)
    assert compiled - table == set(), ("compiled but in no table", sorted(compiled - table))
    assert table - compiled == set(), ("in a table but not compiled", sorted(table - compiled))
    for fam in S.FAMILIES:
        assert len({c for c in compiled if c[0] == fam}) == S.COUNTS[fam] + sum(1 for c in S.UNREACHABLE if c[0] == fam), fam
