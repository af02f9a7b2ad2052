"""Key creation from given words (fhe_ksk_create, fhe_ksk_create_dev, fhe_mbfv_relin_key_aggregate_dev): the kernel
sources under host emulation against the Python oracle's twins.  tests/test_kskcreate_gpu.py runs the same cases on the
MI355X, and the F64 words there."""
import pytest

import kskcreate_cases as K
from helpers import load_engine

FORMS = [False, "abi"]   # the host form and the device form (DeviceArrays)


@pytest.fixture(scope="module")
def fhe():
    return load_engine("emu")


@pytest.mark.parametrize("dev", FORMS, ids=["host", "abi"])
def test_created_handle_holds_the_oracles_twins(fhe, dev):
    """N = 16 over three moduli (one partial workgroup), a key level below the ciphertext level (Lk = 3, two digits) and
    a decomposition key (one modulus, log_base != 0)."""
    opar, par = K.params(fhe, 16, [62, 60, 55], 1153)
    assert K.case_created_arrays(fhe, dev, opar, par) < K.EW_THREADS
    K.case_created_arrays(fhe, dev, opar, par, 1, 0)
    K.case_created_arrays(fhe, dev, opar, par, 2, 2)


@pytest.mark.parametrize("dev", FORMS, ids=["host", "abi"])
def test_created_handle_several_workgroups(fhe, dev):
    """N = 256 over three moduli: 1,152 pairs, four workgroups and a half."""
    opar, par = K.params(fhe, 256, [62, 60, 55])
    pairs = K.case_created_arrays(fhe, dev, opar, par)
    assert pairs == 1152 and pairs % K.EW_THREADS == K.EW_THREADS // 2


@pytest.mark.parametrize("dev", FORMS, ids=["host", "abi"])
def test_refusals(fhe, dev):
    opar, par = K.params(fhe, 16, [62, 60, 55], 1153)
    K.case_refusals(fhe, dev, opar, par)


@pytest.mark.parametrize("dev", FORMS, ids=["host", "abi"])
def test_aggregate_refuses_unreduced_round_one_word(fhe, dev):
    opar, par = K.params(fhe, 16, [62, 60], 1153)
    K.case_aggregate_refusal(fhe, dev, opar, par)
