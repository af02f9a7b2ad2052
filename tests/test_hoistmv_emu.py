"""Hoisted matrix-vector product (fhe_bfv_matvec_hoisted_dev, KeySet.matvec_hoisted, HoistedRotations.matvec): the kernel
sources under host emulation against the restatement tests/hoistmv_ref.py and the engine's own composition (hoisted
rotations, then dot_product_scalar), every shape up to N = 1024.  tests/test_hoistmv_gpu.py runs the same cases on the
MI355X, counts the launches and adds the larger row kinds."""
import pytest

import hoistmv_cases as M
from fhe_oracle import bfv as obfv
from helpers import load_engine

FORMS = [False, "abi"]   # numpy arrays (staged by the wrappers) and DeviceArrays
IDS = ["host", "abi"]


@pytest.fixture(scope="module")
def fhe():
    return load_engine("emu")


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_anchor(fhe, dev):
    """N = 16 over [62, 60, 55], exponents (1, 3, 9, 31, 3), batch 2: shared / per-item diagonals, with / without pt0."""
    M.case_anchor(fhe, dev)


def test_deepest_level(fhe):
    """Keys and ciphertexts both at level 1 of the three-modulus set."""
    M.case_anchor(fhe, "abi", cl=1, kl=1, seed=205, variants=[(False, True)])


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_forms(fhe, dev):
    M.case_forms(fhe, dev)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_matrix_times_encrypted_vector(fhe, dev):
    M.case_matrix_vector(fhe, dev)


def test_both_folds_at_the_top(fhe):
    """Sixteen 62-bit digits at N = 128, R = 17 in one rotation group, every ciphertext, key and plaintext word at
    q_j - 1: the digit fold sees sixteen terms, the rotation fold a seventeenth after a fold."""
    q = obfv.generate_moduli([62] * 16, 128)
    M.case_synthetic(fhe, "abi", q, 128, 17, 1, seed=219, top=True, rot_split=1)


def test_seventeen_digits(fhe):
    """17 digits of 58-bit moduli at N = 128, R = 2: the digit accumulators fold after sixteen terms."""
    q = obfv.generate_moduli([58] * 17, 128)
    M.case_synthetic(fhe, "abi", q, 128, 2, 1, seed=221, rot_split=1)


def test_table_boundary(fhe):
    M.case_table_boundary(fhe, "abi")


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_rotation_groups(fhe, dev):
    M.case_rot_split(fhe, dev)


def test_grid_tail(fhe):
    """N = 1024 over three moduli, R = 2, batch 1: two lane chunks per row, six key ranges in a grid rounded up to eight."""
    q = obfv.generate_moduli([62, 60, 55], 1024)
    M.case_synthetic(fhe, "abi", q, 1024, 2, 1, seed=223)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_w_budget(fhe, dev):
    M.case_w_budget(fhe, dev)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_refusals(fhe, dev):
    M.case_refusals(fhe, dev)
