"""Keyed batches (one key per client in one batch: fhe_kskset_*, fhe_*_keyed_dev, KeySet, EvaluationKey.batched): the
kernel sources under host emulation against the Python oracle client by client and the single-key engine calls, every
shape up to N = 1024.  tests/test_keyed_gpu.py runs the same cases on the MI355X and the larger row kinds."""
import pytest

import keyed_cases as K
from fhe_oracle import bfv as obfv
from helpers import load_engine

FORMS = [False, "abi"]   # numpy arrays (staged by the wrappers) and DeviceArrays
IDS = ["host", "abi"]
SMALL = (16, [62, 60, 55])


@pytest.fixture(scope="module")
def fhe():
    return load_engine("emu")


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
@pytest.mark.parametrize("nkeys,per_key", [(3, 1), (3, 2)])
def test_key_mapping(fhe, dev, nkeys, per_key):
    """N = 16 over [62, 60, 55]: one partial workgroup per row (2 * ci >= n), three clients with one and with two items."""
    opar, par = K.params(fhe, *SMALL)
    K.case_relin(fhe, dev, opar, par, nkeys, per_key)


def test_more_keys_than_an_argument_table_holds(fhe):
    """65 clients x 1 item at N = 16: the key table lives in device memory."""
    opar, par = K.params(fhe, *SMALL)
    K.case_relin(fhe, "abi", opar, par, 65, 1)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_evaluation_key_set(fhe, dev):
    """Rotations, inner sum, and expansion to sizes 4 and 3 with 3 clients x 2 queries at N = 16."""
    opar, par = K.params(fhe, *SMALL)
    K.case_evaluation_key(fhe, dev, opar, par, 3, 2)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_rotations_copying_path(fhe, dev):
    """Exponents 3 and 2N - 1 at N = 16 (below N = 4096 the substitution is a separate pass)."""
    opar, par = K.params(fhe, *SMALL)
    K.case_galois(fhe, dev, opar, par, 3, 2, (3, 31))


@pytest.mark.parametrize("cl,kl", [(1, 0), (1, 1)])
def test_levels(fhe, cl, kl):
    """Keys at level 0 on ciphertexts at level 1 (key_switch_add through switch_down_to_ntt), and keys and ciphertexts
    both at the deepest level that still has RNS digits."""
    opar, par = K.params(fhe, *SMALL)
    K.case_relin(fhe, "abi", opar, par, 3, 2, cl, kl)
    K.case_galois(fhe, "abi", opar, par, 3, 1, (3,), cl, kl)


def test_grid_tail(fhe):
    """N = 1024 over three moduli: two lane chunks per row, six key ranges in a grid rounded up to eight (kr >= nkr)."""
    q = obfv.generate_moduli([62, 60, 55], 1024)
    K.case_synthetic(fhe, "abi", q, 1024, 2, 1, seed=61, exps=(3,))


def test_seventeen_digits(fhe):
    """17 digits of 58-bit moduli at N = 128: the accumulators fold after sixteen terms."""
    q = obfv.generate_moduli([58] * 17, 128)
    K.case_synthetic(fhe, "abi", q, 128, 2, 2, seed=67)


def test_sixteen_digits_at_the_top(fhe):
    """Sixteen 62-bit digits, every input word and every key word at q_i - 1: sixteen products of the largest size in
    each 128-bit accumulator."""
    q = obfv.generate_moduli([62] * 16, 128)
    K.case_synthetic(fhe, "abi", q, 128, 2, 2, seed=71, top=True)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_w_budget_cuts_inside_a_client(fhe, dev):
    """3 clients x 4 items at N = 16 under a W budget of seven polynomials of one key modulus: chunks of six polynomials
    (not a multiple of four) and groups of one key modulus, against the default budget."""
    q = obfv.generate_moduli([62, 60, 55], 16)
    K.case_synthetic(fhe, dev, q, 16, 3, 4, seed=73, exps=(3, 31), w_budget=7 * 3 * 16 * 8)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_multiply_then_keyed_relinearization(fhe, dev):
    opar, par = K.params(fhe, *SMALL)
    K.case_multiply(fhe, dev, opar, par, 3, 2)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_refusals(fhe, dev):
    K.case_refusals(fhe, dev)
