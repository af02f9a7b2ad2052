"""Hoisted rotations (fhe_bfv_galois_hoisted_dev, KeySet.relinearize_hoisted, EvaluationKey.hoisted): the kernel sources
under host emulation against the restatement tests/hoist_ref.py on the Python oracle, every shape up to N = 1024.
tests/test_hoist_gpu.py runs the same cases on the MI355X and the larger row kinds."""
import pytest

import hoist_cases as H
from fhe_oracle import bfv as obfv
from helpers import load_engine

FORMS = [False, "abi"]   # numpy arrays (staged by the wrappers) and DeviceArrays
IDS = ["host", "abi"]


@pytest.fixture(scope="module")
def fhe():
    return load_engine("emu")


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_anchor_to_the_reference(fhe, dev):
    """N = 16 over [62, 60, 55], exponents (1, 3, 9, 31, 3), batch 2.  Noise differences (hoisted - reference, bits) seen
    over the eight pairs: within -1 ... +1."""
    noise = H.case_anchor(fhe, dev)
    assert len(noise) == 8


def test_deepest_level_with_rns_digits(fhe):
    """Keys and ciphertexts both at level 1 of the three-modulus set."""
    H.case_anchor(fhe, "abi", cl=1, kl=1, seed=131)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_forms(fhe, dev):
    H.case_forms(fhe, dev)


def test_more_rotations_than_an_argument_table_holds(fhe):
    H.case_more_rotations_than_a_table(fhe, "abi")


def test_grid_tail(fhe):
    """N = 1024 over three moduli: two lane chunks per row, six key ranges in a grid rounded up to eight."""
    q = obfv.generate_moduli([62, 60, 55], 1024)
    H.case_synthetic(fhe, "abi", q, 1024, 2, 1, seed=137)


def test_seventeen_digits(fhe):
    """17 digits of 58-bit moduli at N = 128: the accumulators fold after sixteen terms."""
    q = obfv.generate_moduli([58] * 17, 128)
    H.case_synthetic(fhe, "abi", q, 128, 2, 1, seed=139)


def test_sixteen_digits_at_the_top(fhe):
    """Sixteen 62-bit digits, every ciphertext word and every key word at q_i - 1."""
    q = obfv.generate_moduli([62] * 16, 128)
    H.case_synthetic(fhe, "abi", q, 128, 2, 1, seed=149, top=True, exps=(3, 255))


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_w_budget(fhe, dev):
    H.case_w_budget(fhe, dev)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_refusals(fhe, dev):
    H.case_refusals(fhe, dev)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_matrix_times_encrypted_vector(fhe, dev):
    H.case_matrix_vector(fhe, dev)
