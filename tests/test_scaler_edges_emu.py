"""tests/scaler_edge_cases.py on the kernel sources compiled for the host (tests/emu): the scaler on columns that sit on
its rounding thresholds and walk its tables, bit for bit against the oracle.  Every case of the GPU file runs here too
(64 source moduli at N = 16 and the N = 4096 decryption pin included: none needs more than a few seconds emulated); what
only the GPU file can check is which scale_kernel instance a launch took."""
import pytest

import scaler_edge_cases as E
import scaler_edge_inputs as I
from helpers import load_engine


@pytest.fixture(scope="module")
def fhe():
    return load_engine("emu")


@pytest.mark.parametrize("name", [s.name for s in I.all_scalers()])
def test_scaler_on_its_thresholds(fhe, name):
    E.case_scaler(fhe, False, next(s for s in I.all_scalers() if s.name == name))


def test_decrypt_on_the_threshold(fhe):
    E.case_decrypt_on_threshold(fhe, False)
