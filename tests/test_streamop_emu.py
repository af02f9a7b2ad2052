"""The streaming kernels (dot product, ct x pt, modulus switching, substitution, wire format) at their accumulator,
rounding and shape edges, and stage B of the key switch with seventeen 62-bit digits at the top: the kernel sources under
host emulation against the Python-int restatements of tests/streamop_ref.py (tests/streamop_cases.py has the cases and
what each shape is for).  tests/test_streamop_gpu.py runs the same cases on the MI355X and reads which kernels ran."""
import os
import subprocess
import sys

import pytest

import streamop_cases as S
from helpers import ROOT, load_engine

FORMS = [False, "abi"]   # numpy arrays (staged by the wrappers) and DeviceArrays
IDS = ["host", "abi"]


@pytest.fixture(scope="module")
def fhe():
    return load_engine("emu")


# ---- dot product ---------------------------------------------------------------------------------------------------------
def test_dot_thresholds():
    """ceil(2^128 / (q - 1)^2) for the moduli generate_moduli gives: 17 terms at 62 bits, 65 at 61, 257 at 60; far beyond
    any count here for 50 bits and less."""
    assert S.case_dot_thresholds_are_what_they_are("n8-62-61-60") == {62: 17, 61: 65, 60: 257}
    assert S.case_dot_thresholds_are_what_they_are("n256-62-61-60") == {62: 17, 61: 65, 60: 257}
    assert set(S.case_dot_thresholds_are_what_they_are("n8-62-62").values()) == {17}
    assert min(S.case_dot_thresholds_are_what_they_are("n8-50-40-20").values()) > 1 << 27
    # every context's cases: the counts on both sides of every threshold, and the part counts of both kernels
    cases = S.dot_all_cases("n8-62-61-60")
    assert {c.count for c in cases if c.pattern == "max"} == {16, 17, 18, 64, 65, 66, 256, 257, 258, 4096}
    assert {c.count for c in cases if c.pattern == "random"} == {1, 2, 7, 300, 4096}
    assert {c.parts for c in cases} == {1, 2, 3, 4, 5} and {c.form for c in cases} == {None, "cts", "pts", "both"}


@pytest.mark.parametrize("group", S.DOT_GROUPS)
@pytest.mark.parametrize("name", list(S.DOT_CONTEXTS))
def test_dot(fhe, name, group):
    for i, case in enumerate(S.dot_cases(name, group)):
        S.run_dot(fhe, FORMS[i % 2], case)


# ---- ct x pt -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", FORMS, ids=IDS)
@pytest.mark.parametrize("n", S.MUL_PLAIN_N)
def test_mul_plain(fhe, dev, n):
    S.case_mul_plain(fhe, dev, n)


# ---- modulus switching ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", FORMS, ids=IDS)
@pytest.mark.parametrize("name", list(S.SD_SETS))
def test_switch_down(fhe, dev, name):
    S.case_switch_down(fhe, dev, name)


# ---- substitution --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", FORMS, ids=IDS)
@pytest.mark.parametrize("n", S.SUB_N)
def test_substitute(fhe, dev, n):
    S.case_substitute(fhe, dev, n)


# ---- wire format ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.WIRE_N)
@pytest.mark.parametrize("widths", S.WIRE_CONTEXTS, ids=lambda w: "-".join(map(str, w)))
def test_wire(fhe, widths, n):
    """DeviceArrays: the emulated device's buffers are host memory, so the byte buffer 8 bytes and 1 byte past a 16-byte
    boundary takes launch_wire's byte-kernel branch here too."""
    S.case_wire(fhe, "abi", widths, n)


@pytest.mark.parametrize("n", S.WIRE_N)
def test_wire_host_arrays(fhe, n):
    S.case_wire(fhe, False, S.WIRE_MIXED, n)


def test_wire_kernels_stay_inside_the_byte_buffer():
    """streamop_cases.case_wire_guarded in a process of its own: the payload ends where a page without access rights
    begins, so the process ends on a signal if a wire kernel touches a byte past it (the values cannot tell)."""
    paths = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(paths + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    run = subprocess.run([sys.executable, "-c", "import streamop_cases as S; S.main_wire_guarded()"], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    assert "guarded wire buffers ok" in run.stdout


# ---- seventeen digits at the top -----------------------------------------------------------------------------------------
def test_seventeen_digits_saturate_the_window():
    """Python ints only: sixteen products and a canonical word fit 128 bits, the seventeenth product does not."""
    _p, least = S.top17_saturation()
    assert least > 1 << 61


def test_seventeen_digits_at_the_top_keyed(fhe):
    S.case_top17_keyed(fhe, "abi")


@pytest.mark.parametrize("mode", ["UNFUSED", "FUSED"])
def test_seventeen_digits_at_the_top_plain(fhe, mode):
    S.case_top17_plain(fhe, "abi", getattr(fhe.KeySwitchingKey, mode))


def test_seventeen_digits_at_the_top_hoisted(fhe):
    S.case_top17_hoisted(fhe, "abi")
