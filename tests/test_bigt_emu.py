"""Plaintext moduli above 64 bits (fhe_params_create_big, fhe_bfv_encode_big_dev, fhe_bfv_reduce_big_dev,
fhe_bfv_decrypt_big_dev, fhe_mbfv_decrypt_big_dev, measure_noise on a big encoder): the kernel sources under host
emulation at N = 16 ... 64 on the five parameter sets of tests/bigt_ref.py, against bigt_ref and the oracle on Python
integers.  tests/test_bigt_gpu.py runs the same cases on the MI355X."""
import pytest

import bigt_cases as B
import bigt_ref as R
import encode_cases as E
from helpers import load_engine

SETS = sorted(R.SETS)


@pytest.fixture(scope="module")
def fhe():
    return load_engine("emu")


@pytest.mark.parametrize("name", SETS)
def test_sets_match_the_oracle(fhe, name):
    """W_t, P, q_mod_t below t and delta per level as the oracle builds them from a Python-int t."""
    opar, par = B.params(fhe, name, 16)
    t = opar.plaintext
    assert all(0 <= q < t for q in opar.q_mod_t)
    assert R.tail(opar, 0) == 0 and R.tail(opar, opar.plaintext_context.modulus() - 1) == t - 1


@pytest.mark.parametrize("name", SETS)
def test_reduce(fhe, name):
    B.case_reduce(fhe, False, *B.params(fhe, name, 16))


def test_reduce_two_workgroups(fhe):
    """N = 512: the crafted value on either side of the workgroup boundary; limbs in and out on DeviceArrays."""
    B.case_reduce(fhe, "abi", *B.params(fhe, "B", 512))


def test_reduce_generic_instance(fhe):
    """Nine 30-bit rows under a 200-bit t: more plaintext-context rows than the compile-time instances, W_t = 4."""
    t = (1 << 200) - 75
    opar, par = E.params(fhe, 16, t, moduli_sizes=[30] * 12)
    assert par.plaintext_limbs == 4 and len(opar.plaintext_context.moduli) == 9
    B.case_reduce(fhe, False, opar, par)


@pytest.mark.parametrize("name", SETS)
def test_encode(fhe, name):
    B.case_encode(fhe, False, *B.params(fhe, name, 16), batch=3)


def test_encode_limbs_in(fhe):
    B.case_encode(fhe, "abi", *B.params(fhe, "D", 64), batch=2)


@pytest.mark.parametrize("name", SETS)
def test_roundtrip(fhe, name):
    opar, par = B.params(fhe, name, 16)
    B.case_roundtrip(fhe, False, opar, par, level=0, batch=3)
    B.case_roundtrip(fhe, "abi", opar, par, level=B.deepest_level(opar) if name != "D" else 0, batch=2, seed=12)


@pytest.mark.parametrize("name", SETS)
def test_arithmetic(fhe, name):
    B.case_arithmetic(fhe, False if name != "B" else "abi", *B.params(fhe, name, 16), batch=3, decrypts=name != "D")


@pytest.mark.parametrize("name", SETS)
def test_noise(fhe, name):
    B.case_noise(fhe, False if name != "C" else "abi", *B.params(fhe, name, 16), batch=2)


def test_multiparty(fhe):
    opar, par = B.params(fhe, "A", 16)
    B.case_multiparty(fhe, False, opar, par)
    B.case_multiparty(fhe, "abi", opar, par, seed=23)


def test_one_limb_equals_u64(fhe):
    opar, _ = E.params(fhe, 16, 1153, moduli_sizes=[62] * 3)
    B.case_one_limb(fhe, opar)


@pytest.mark.parametrize("name", SETS)
def test_statuses(fhe, name):
    opar, par = B.params(fhe, name, 16)
    opar_small, par_small = E.params(fhe, 16, 1153, moduli=opar.moduli)
    B.case_statuses(fhe, opar, par, opar_small, par_small)


@pytest.mark.parametrize("t,sizes", [(1 << 64, [50, 50, 50]), (1 << 128, [60] * 5)], ids=["2^64", "2^128"])
def test_power_of_the_base(fhe, t, sizes):
    B.case_power_of_the_base(fhe, False, 16, t, sizes)


def test_256_bit_modulus(fhe):
    """t = 2^256 - 189 on 7 x 60 bits: every limb of t full."""
    opar, par = E.params(fhe, 16, R.T256[0], moduli_sizes=R.T256[1])
    assert par.plaintext_limbs == 4
    B.case_reduce(fhe, False, opar, par)
    B.case_encode(fhe, "abi", opar, par, batch=2)
    B.case_roundtrip(fhe, False, opar, par, level=0, batch=2)
    B.case_noise(fhe, False, opar, par, batch=1)
