"""Key creation from given words on the MI355X (the HIP build): tests/test_kskcreate_emu.py's cases through the host
form, torch tensors and DeviceArrays, and the F64 words of an eligible key at N = 4096 (the smallest F64 row) against
the Python oracle's key_switch."""
import pytest

import kskcreate_cases as K
from helpers import HIP_LIB, load_engine

pytestmark = pytest.mark.gpu
FORMS = [False, True, "abi"]
IDS = ["host", "torch", "abi"]


@pytest.fixture(scope="module")
def fhe():
    eng = load_engine("hip")
    from fhe_rs_amd import _lib
    assert _lib.loaded_path() == HIP_LIB, "GPU tests must run on the HIP build"
    assert eng.device_count() >= 1, "no HIP device visible"
    return eng


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_created_handle_holds_the_oracles_twins(fhe, dev):
    """N = 16 over three moduli (one partial workgroup), a key level below the ciphertext level (Lk = 3, two digits) and
    a decomposition key (one modulus, log_base != 0)."""
    opar, par = K.params(fhe, 16, [62, 60, 55], 1153)
    assert K.case_created_arrays(fhe, dev, opar, par) < K.EW_THREADS
    K.case_created_arrays(fhe, dev, opar, par, 1, 0)
    K.case_created_arrays(fhe, dev, opar, par, 2, 2)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_created_handle_several_workgroups(fhe, dev):
    """N = 256 over three moduli: 1,152 pairs, four workgroups and a half."""
    opar, par = K.params(fhe, 256, [62, 60, 55])
    pairs = K.case_created_arrays(fhe, dev, opar, par)
    assert pairs == 1152 and pairs % K.EW_THREADS == K.EW_THREADS // 2


def test_f64_words(fhe):
    """N = 4096, every modulus below 2^50, created through the host form and through the device form."""
    opar, par = K.params(fhe, 4096, [50, 49, 45])
    for dev in (False, True):
        K.case_f64_words(fhe, dev, opar, par)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_refusals(fhe, dev):
    opar, par = K.params(fhe, 16, [62, 60, 55], 1153)
    K.case_refusals(fhe, dev, opar, par)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "torch"])
def test_aggregate_refuses_unreduced_round_one_word(fhe, dev):
    opar, par = K.params(fhe, 16, [62, 60], 1153)
    K.case_aggregate_refusal(fhe, dev, opar, par)
