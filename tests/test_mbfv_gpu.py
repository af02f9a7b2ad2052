"""Multiparty BFV on the MI355X (fhe_mbfv_*_dev, the HIP build): the cases of tests/test_mbfv_emu.py on torch tensors,
plus what only the device runs in seconds -- the stock parameter sets at batch 1,024 (F64 instances, and the integer
ones after set_f64(False)), rows of 32768 points (the element-wise path) and the protocols at stock n = 8192."""
import pytest

import encode_cases as E
import mbfv_cases as M
import ref_params
from helpers import load_engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fhe():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load_engine("hip")


def arc(fhe, nmod, n):
    return E.params(fhe, n, 1153, moduli_sizes=[62] * nmod)


def stock(fhe, n):
    return E.params(fhe, n, ref_params.plaintext_modulus(n), moduli=ref_params.DEFAULT_128[n])


SMALL = [(1, 16), (6, 32)]


@pytest.mark.parametrize("nmod,n", SMALL)
def test_share_parity(fhe, nmod, n):
    opar, par = arc(fhe, nmod, n)
    M.case_share_parity(fhe, True, opar, par)


@pytest.mark.parametrize("n", [4096, 8192, 16384])
def test_stock_batch_forms(fhe, n):
    """Batch 1,024, items 0 and 1,023: one secret shared and a secret per item, every share of the table (the public-key-switch
    share included) and both relin rounds; the integer instances (set_f64(False)) give the identical words."""
    opar, par = stock(fhe, n)
    on, want = M.case_batch_forms(fhe, opar, par)
    fhe.set_f64(False)
    try:
        off, _ = M.case_batch_forms(fhe, opar, par, ref=want)
    finally:
        fhe.set_f64(True)
    assert sorted(on) == sorted(off)


@pytest.mark.parametrize("n", [4096, 8192, 16384])
def test_stock_share_parity(fhe, n):
    """Every share and aggregation of the small-shape case at the stock sets (F64 instances), the switch shares at the
    first and the last level."""
    opar, par = stock(fhe, n)
    M.case_share_parity(fhe, True, opar, par, parties=1, cts=1, levels=sorted({0, opar.max_level()}))


def test_share_parity_large_rows(fhe):
    """Rows of 32768 points: the element-wise epilogue around launch_ntt."""
    n = 32768
    opar, par = E.params(fhe, n, E.stock_t(n), moduli_sizes=[50, 55, 60])
    M.case_share_parity(fhe, True, opar, par, parties=2, cts=1, levels=[0])


@pytest.mark.parametrize("n", [8, 4096])
def test_sum_overflow(fhe, n):
    opar, par = E.params(fhe, n, 1153 if n == 8 else E.stock_t(n), moduli_sizes=[62, 62])
    assert all(int(m).bit_length() == 62 for m in par.moduli)
    M.case_sum_overflow(fhe, True, par, n)


@pytest.mark.parametrize("nmod,n", SMALL)
def test_encrypt_decrypt(fhe, nmod, n):
    opar, par = arc(fhe, nmod, n)
    M.case_encrypt_decrypt(fhe, True, opar, par)


@pytest.mark.parametrize("nmod,n", SMALL)
def test_encrypt_keyswitch_decrypt(fhe, nmod, n):
    opar, par = arc(fhe, nmod, n)
    M.case_keyswitch_decrypt(fhe, True, opar, par)


@pytest.mark.parametrize("nmod,n", [(3, 16), (6, 32)])
def test_relinearization_works(fhe, nmod, n):
    opar, par = arc(fhe, nmod, n)
    M.case_relinearization(fhe, True, opar, par)


def test_protocols_stock_8192(fhe):
    """encrypt_decrypt and relinearization_works with 3 parties at the stock n = 8192 set: the F64 instances carry a
    whole protocol.  (The BigUint tail is restated at the small sets; here the plaintext is the check.)"""
    opar, par = stock(fhe, 8192)
    M.case_encrypt_decrypt(fhe, True, opar, par, parties=3, levels=[0], restate_tail=False)
    M.case_relinearization(fhe, True, opar, par, parties=3)
