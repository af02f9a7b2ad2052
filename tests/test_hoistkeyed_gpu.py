"""Hoisted rotations and the hoisted matrix-vector product with one Galois key set per client on the MI355X (the HIP
build): tests/test_hoistkeyed_emu.py's cases through numpy arrays, torch tensors and DeviceArrays, and the row kinds only
the GPU suite reaches, each against hoist_cases.composed client by client with the launches counted from the engine's
profiler -- one stage A per chunk and key-modulus group, one keyed stage B per pair and 64 rotations however many clients
there are, never an unkeyed or single-key kernel."""
import pytest

import hoistkeyed_cases as HK
import ref_params
from fhe_oracle import bfv as obfv
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
def test_anchor(fhe, dev):
    """N = 16 over [62, 60, 55], three clients with their own secret keys, exponents (1, 3, 9, 31, 3), batch 6."""
    HK.case_anchor(fhe, dev)


def test_deepest_level(fhe):
    """Keys and ciphertexts both at level 1 of the three-modulus set."""
    HK.case_anchor(fhe, True, cl=1, kl=1, seed=302)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_one_client_is_the_unkeyed_call(fhe, dev):
    HK.case_one_client(fhe, dev)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_one_ciphertext_per_client(fhe, dev):
    HK.case_one_ciphertext_per_client(fhe, dev)


def test_more_rotations_than_a_table(fhe):
    HK.case_more_rotations_than_a_table(fhe, True)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_chunk_straddles_clients(fhe, dev):
    HK.case_straddle(fhe, dev)


def test_grid_tail(fhe):
    """N = 1024 over three moduli, 2 clients x 2 rotations, batch 2: two lane chunks per row, six key ranges in a grid
    rounded up to eight."""
    HK.case_rotations(fhe, True, obfv.generate_moduli([62, 60, 55], 1024), 1024, 2, 2, 1, seed=323)


def test_seventeen_digits(fhe):
    """17 digits of 58-bit moduli at N = 128, 2 clients x 2 rotations: the accumulators fold after sixteen digits."""
    HK.case_rotations(fhe, True, obfv.generate_moduli([58] * 17, 128), 128, 2, 2, 1, seed=325)


def test_sixteen_digits_at_the_top(fhe):
    """Sixteen 62-bit digits at N = 128, every word q_i - 1, 2 clients: sixteen products of the largest size, no fold."""
    HK.case_rotations(fhe, True, obfv.generate_moduli([62] * 16, 128), 128, 2, 2, 1, seed=327, top=True)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_matvec(fhe, dev):
    HK.case_matvec_anchor(fhe, dev)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_matvec_rotation_groups(fhe, dev):
    HK.case_matvec_rot_split(fhe, dev)


def test_matvec_table_boundary(fhe):
    HK.case_matvec_table_boundary(fhe, True)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_matvec_chunk_straddles_clients(fhe, dev):
    HK.case_matvec_straddle(fhe, dev)


def test_matvec_seventeen_digits(fhe):
    HK.case_matvec(fhe, True, obfv.generate_moduli([58] * 17, 128), 128, 2, 2, 1, seed=329, rot_split=1)


def test_matvec_both_folds_at_the_top(fhe):
    """Sixteen 62-bit digits at N = 128, R = 17 in one rotation group, every word q_j - 1, 2 clients: the second quad folds
    after sixteen rotations with all factors q_j - 1."""
    HK.case_matvec(fhe, True, obfv.generate_moduli([62] * 16, 128), 128, 2, 17, 1, seed=331, top=True, rot_split=1)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_refusals(fhe, dev):
    HK.case_refusals(fhe, dev)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_evaluation_key_set(fhe, dev):
    HK.case_evaluation_key_set_errors(fhe, dev)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_end_to_end(fhe, dev):
    HK.case_end_to_end(fhe, dev)


# ---- the row kinds of the larger shapes: H.composed per client, the launches counted -------------------------------------------
@pytest.mark.parametrize("f64", [True, False], ids=["f64", "integer"])
def test_stock_4096(fhe, f64):
    """The stock n = 4096 set, 2 clients x 1 ciphertext, R = 3, with the F64 option on -- stage A on doubles -- and off."""
    fhe.set_f64(f64)
    try:
        symbols = HK.case_large(fhe, True, ref_params.DEFAULT_128[4096], 4096, 2, 3, 1, seed=333)
    finally:
        fhe.set_f64(True)
    stage_a = [s[s.index("ks_ntt_kernel<"):] for s in symbols if "ks_ntt_kernel<" in s]
    last = [a[a.index("<") + 1:a.index(">")].split(",")[-1].strip() for a in stage_a]
    assert last and all((a != "0") == f64 for a in last), symbols


def test_n8192_four_60_bit_moduli(fhe):
    """The benchmark's row size: 2 clients x 2 ciphertexts, R = 3."""
    HK.case_large(fhe, True, obfv.generate_moduli([60] * 4, 8192), 8192, 2, 3, 2, seed=335)


def test_client_boundary_inside_a_launch(fhe):
    """N = 4096 over three moduli, 3 clients x 1 ciphertext, R = 2 under a budget of two ciphertexts of one key modulus:
    chunks of two, so the first launch holds clients 0 and 1 and the second starts at client 2."""
    q = obfv.generate_moduli([62, 60, 55], 4096)
    assert HK.K.chunk_rule(3, 3, 3, 4096, 2 * 3 * 4096 * 8) == (2, 1)
    HK.case_large(fhe, True, q, 4096, 3, 2, 1, seed=337, w_budget=2 * 3 * 4096 * 8)
