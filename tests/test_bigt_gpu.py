"""Plaintext moduli above 64 bits on the MI355X (the HIP build): the cases of tests/test_bigt_emu.py at N = 16 on the
five parameter sets of tests/bigt_ref.py, at N = 1024 (four workgroups per polynomial in the tail) on A, B and D, at
N = 4096 on E (F64 on and off) and B with the W_t / P instances the profiler saw, and at N = 32768 (rows larger than one
LDS tile) on A."""
import re

import pytest

import bigt_cases as B
import bigt_ref as R
import encode_cases as E
from helpers import HIP_LIB, load_engine

pytestmark = pytest.mark.gpu

SETS = sorted(R.SETS)


@pytest.fixture(scope="module")
def fhe():
    eng = load_engine("hip")
    from fhe_rs_amd import _lib
    assert _lib.loaded_path() == HIP_LIB, "GPU tests must run on the HIP build"
    assert eng.device_count() >= 1, "no HIP device visible"
    return eng


@pytest.fixture(autouse=True)
def release_scratch(fhe):
    """The engine's retained scratch and torch's cached blocks go back after every test: later files run batches of
    1,024 at n = 16384 and need the memory."""
    yield
    import torch
    torch.cuda.synchronize()
    fhe.workspace_trim()
    torch.cuda.empty_cache()


def instances(fhe, fn):
    """({W_t of bigt_project_kernel}, {(P, W_t) of bigt_tail_kernel}) launched while fn() ran, from the profiler's
    kernel symbols."""
    fhe.prof_reset()
    fhe.prof_enable(True)
    try:
        fn()
        symbols = [sym for _label, sym, _n, _ms in fhe.prof_entries()]
    finally:
        fhe.prof_enable(False)
        fhe.prof_reset()
    proj = {int(m.group(1)) for m in (re.search(r"bigt_project_kernel<(\d+)>", s) for s in symbols) if m}
    tail = {(int(m.group(1)), int(m.group(2))) for m in (re.search(r"bigt_tail_kernel<(\d+), (\d+)>", s) for s in symbols) if m}
    return proj, tail


@pytest.mark.parametrize("name", SETS)
def test_n16_reduce_encode(fhe, name):
    opar, par = B.params(fhe, name, 16)
    B.case_reduce(fhe, True, opar, par)
    B.case_reduce(fhe, False, opar, par)
    B.case_encode(fhe, True, opar, par, batch=3)
    B.case_encode(fhe, False, opar, par, batch=3)


@pytest.mark.parametrize("name", SETS)
def test_n16_roundtrip_arithmetic(fhe, name):
    opar, par = B.params(fhe, name, 16)
    B.case_roundtrip(fhe, True, opar, par, level=0, batch=3)
    B.case_roundtrip(fhe, "abi", opar, par, level=B.deepest_level(opar) if name != "D" else 0, batch=3, seed=12)
    B.case_arithmetic(fhe, True, opar, par, batch=3, decrypts=name != "D")


@pytest.mark.parametrize("name", SETS)
def test_n16_noise(fhe, name):
    B.case_noise(fhe, True, *B.params(fhe, name, 16), batch=3)


def test_n16_multiparty(fhe):
    opar, par = B.params(fhe, "A", 16)
    B.case_multiparty(fhe, True, opar, par)
    B.case_multiparty(fhe, False, opar, par, seed=23)


def test_n16_statuses(fhe):
    for name in SETS:
        opar, par = B.params(fhe, name, 16)
        B.case_statuses(fhe, opar, par, *E.params(fhe, 16, 1153, moduli=opar.moduli))
    B.case_one_limb(fhe, E.params(fhe, 16, 1153, moduli_sizes=[62] * 3)[0])


def test_generic_instance(fhe):
    """Nine 30-bit rows under a 200-bit t: the run-time-P instance of the tail."""
    opar, par = E.params(fhe, 1024, (1 << 200) - 75, moduli_sizes=[30] * 12)
    proj, tail = instances(fhe, lambda: B.case_reduce(fhe, True, opar, par))
    assert tail == {(0, 4)}, tail


@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_n1024(fhe, name):
    """Four workgroups per polynomial in the tail; batch 2."""
    opar, par = B.params(fhe, name, 1024)
    _, _, wt, p = R.SETS[name]
    proj, tail = instances(fhe, lambda: (B.case_reduce(fhe, True, opar, par),
                                         B.case_encode(fhe, True, opar, par, batch=2)))
    assert proj == {wt} and tail == {(p, wt)}, (proj, tail)


@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_n1024_roundtrip_arithmetic(fhe, name):
    opar, par = B.params(fhe, name, 1024)
    B.case_roundtrip(fhe, True, opar, par, level=0, batch=2, columns=list(range(0, 1024, 37)) + [255, 256, 1023])
    B.case_arithmetic(fhe, True, opar, par, batch=2, decrypts=name != "D", parity_items=[1])


@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_n1024_noise(fhe, name):
    B.case_noise(fhe, True, *B.params(fhe, name, 1024), batch=2)


@pytest.mark.parametrize("name,f64", [("E", True), ("E", False), ("B", True)], ids=["E-f64", "E-int", "B"])
def test_n4096_whole_rows(fhe, name, f64):
    """The whole-row transforms: set E on the F64 instances and on the integer ones, set B on the general ones."""
    n = 4096
    opar, par = B.params(fhe, name, n)
    _, _, wt, p = R.SETS[name]
    cols = list(range(0, n, 131)) + [255, 256, n - 1]
    fhe.set_f64(f64)
    try:
        proj, tail = instances(fhe, lambda: (
            B.case_encode(fhe, True, opar, par, batch=1, levels=(0,)),
            B.case_roundtrip(fhe, True, opar, par, level=0, batch=1, columns=cols)))
    finally:
        fhe.set_f64(True)
    assert proj == {wt} and tail == {(p, wt)}, (proj, tail)


def test_n32768_rows_larger_than_lds(fhe):
    n = 32768
    opar, par = B.params(fhe, "A", n)
    B.case_encode(fhe, "abi", opar, par, batch=1, levels=(0,))
    B.case_roundtrip(fhe, "abi", opar, par, level=0, batch=1, columns=list(range(0, n, 1021)) + [255, 256, n - 1])


@pytest.mark.parametrize("t,sizes", [(1 << 64, [50, 50, 50]), (1 << 128, [60] * 5)], ids=["2^64", "2^128"])
def test_power_of_the_base(fhe, t, sizes):
    B.case_power_of_the_base(fhe, True, 16, t, sizes)


@pytest.mark.parametrize("n", [16, 1024])
def test_256_bit_modulus(fhe, n):
    """t = 2^256 - 189 on 7 x 60 bits: every limb of t full."""
    opar, par = E.params(fhe, n, R.T256[0], moduli_sizes=R.T256[1])
    assert par.plaintext_limbs == 4
    B.case_reduce(fhe, True, opar, par)
    B.case_encode(fhe, True, opar, par, batch=2, levels=(0,))
    B.case_roundtrip(fhe, True, opar, par, level=0, batch=2, columns=None if n == 16 else list(range(0, n, 37)) + [255, 256, n - 1])
    if n == 16:
        B.case_noise(fhe, True, opar, par, batch=2)
