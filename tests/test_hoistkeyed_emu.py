"""Hoisted rotations and the hoisted matrix-vector product with one Galois key set per client
(fhe_bfv_galois_hoisted_keyed_dev, fhe_bfv_matvec_hoisted_keyed_dev; KeySet.relinearize_hoisted_keyed, KeySet.
matvec_hoisted_keyed, EvaluationKeySet.hoisted): the kernel sources under host emulation against one single-client call per
client -- the specification -- and the restatements tests/hoist_ref.py / tests/hoistmv_ref.py under the owner's keys, every
shape up to N = 1024.  tests/test_hoistkeyed_gpu.py runs the same cases on the MI355X, counts the launches and adds the
larger row kinds."""
import pytest

import hoistkeyed_cases as HK
from fhe_oracle import bfv as obfv
from helpers import load_engine

FORMS = [False, "abi"]   # numpy arrays (staged by the wrappers) and DeviceArrays
IDS = ["host", "abi"]


@pytest.fixture(scope="module")
def fhe():
    return load_engine("emu")


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_anchor(fhe, dev):
    """N = 16 over [62, 60, 55], three clients with their own secret keys, exponents (1, 3, 9, 31, 3), batch 6."""
    HK.case_anchor(fhe, dev)


def test_deepest_level(fhe):
    """Keys and ciphertexts both at level 1 of the three-modulus set."""
    HK.case_anchor(fhe, "abi", cl=1, kl=1, seed=302)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_one_client_is_the_unkeyed_call(fhe, dev):
    HK.case_one_client(fhe, dev)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_one_ciphertext_per_client(fhe, dev):
    HK.case_one_ciphertext_per_client(fhe, dev)


def test_more_rotations_than_a_table(fhe):
    HK.case_more_rotations_than_a_table(fhe, "abi")


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_chunk_straddles_clients(fhe, dev):
    HK.case_straddle(fhe, dev)


def test_grid_tail(fhe):
    """N = 1024 over three moduli, 2 clients x 2 rotations, batch 2: two lane chunks per row, six key ranges in a grid
    rounded up to eight."""
    HK.case_rotations(fhe, "abi", obfv.generate_moduli([62, 60, 55], 1024), 1024, 2, 2, 1, seed=323)


def test_seventeen_digits(fhe):
    """17 digits of 58-bit moduli at N = 128, 2 clients x 2 rotations: the accumulators fold after sixteen digits."""
    HK.case_rotations(fhe, "abi", obfv.generate_moduli([58] * 17, 128), 128, 2, 2, 1, seed=325)


def test_sixteen_digits_at_the_top(fhe):
    """Sixteen 62-bit digits at N = 128, every word q_i - 1, 2 clients: sixteen products of the largest size, no fold."""
    HK.case_rotations(fhe, "abi", obfv.generate_moduli([62] * 16, 128), 128, 2, 2, 1, seed=327, top=True)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_matvec(fhe, dev):
    HK.case_matvec_anchor(fhe, dev)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_matvec_rotation_groups(fhe, dev):
    HK.case_matvec_rot_split(fhe, dev)


def test_matvec_table_boundary(fhe):
    HK.case_matvec_table_boundary(fhe, "abi")


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_matvec_chunk_straddles_clients(fhe, dev):
    HK.case_matvec_straddle(fhe, dev)


def test_matvec_seventeen_digits(fhe):
    HK.case_matvec(fhe, "abi", obfv.generate_moduli([58] * 17, 128), 128, 2, 2, 1, seed=329, rot_split=1)


def test_matvec_both_folds_at_the_top(fhe):
    """Sixteen 62-bit digits at N = 128, R = 17 in one rotation group, every word q_j - 1, 2 clients: the second quad folds
    after sixteen rotations with all factors q_j - 1."""
    HK.case_matvec(fhe, "abi", obfv.generate_moduli([62] * 16, 128), 128, 2, 17, 1, seed=331, top=True, rot_split=1)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_refusals(fhe, dev):
    HK.case_refusals(fhe, dev)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_evaluation_key_set(fhe, dev):
    HK.case_evaluation_key_set_errors(fhe, dev)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_end_to_end(fhe, dev):
    HK.case_end_to_end(fhe, dev)
