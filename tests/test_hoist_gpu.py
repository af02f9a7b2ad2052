"""Hoisted rotations on the MI355X (the HIP build): tests/test_hoist_emu.py's cases through numpy arrays, torch tensors
and DeviceArrays, and the row kinds only the GPU suite reaches -- the F64 and integer stage A of the stock n = 4096 set,
N = 8192 over four 60-bit moduli, both tile choices at N = 16384 and the sub-block stage A at N = 32768 -- each against
a composition of entry points with their own oracle tests, with the launches counted from the engine's profiler: one stage
A per chunk and key-modulus group, never one per rotation."""
import pytest

import hoist_cases as H
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
def test_anchor_to_the_reference(fhe, dev):
    """N = 16 over [62, 60, 55], exponents (1, 3, 9, 31, 3), batch 2.  Noise differences (hoisted - reference, bits) seen
    over the eight pairs: within -1 ... +1."""
    noise = H.case_anchor(fhe, dev)
    assert len(noise) == 8


def test_deepest_level_with_rns_digits(fhe):
    """Keys and ciphertexts both at level 1 of the three-modulus set."""
    H.case_anchor(fhe, True, cl=1, kl=1, seed=131)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_forms(fhe, dev):
    H.case_forms(fhe, dev)


def test_more_rotations_than_an_argument_table_holds(fhe):
    H.case_more_rotations_than_a_table(fhe, True)


def test_grid_tail(fhe):
    """N = 1024 over three moduli: two lane chunks per row, six key ranges in a grid rounded up to eight."""
    q = obfv.generate_moduli([62, 60, 55], 1024)
    H.case_synthetic(fhe, True, q, 1024, 2, 1, seed=137)


def test_seventeen_digits(fhe):
    """17 digits of 58-bit moduli at N = 128: the accumulators fold after sixteen terms."""
    q = obfv.generate_moduli([58] * 17, 128)
    H.case_synthetic(fhe, True, q, 128, 2, 1, seed=139)


def test_sixteen_digits_at_the_top(fhe):
    """Sixteen 62-bit digits, every ciphertext word and every key word at q_i - 1."""
    q = obfv.generate_moduli([62] * 16, 128)
    H.case_synthetic(fhe, True, q, 128, 2, 1, seed=149, top=True, exps=(3, 255))


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_w_budget(fhe, dev):
    H.case_w_budget(fhe, dev)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_refusals(fhe, dev):
    H.case_refusals(fhe, dev)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_matrix_times_encrypted_vector(fhe, dev):
    H.case_matrix_vector(fhe, dev)


# ---- the row kinds of the larger shapes ------------------------------------------------------------------------------------
def stage_a_instances(symbols):
    return [s[s.index("ks_ntt_kernel<"):] for s in symbols if "ks_ntt_kernel<" in s]


@pytest.mark.parametrize("f64", [True, False], ids=["f64", "integer"])
def test_stock_4096(fhe, f64):
    """The stock n = 4096 set, batch 2, R = 3, with the F64 option on -- stage A on doubles -- and off."""
    fhe.set_f64(f64)
    try:
        symbols = H.case_large(fhe, True, ref_params.DEFAULT_128[4096], 4096, 3, 2, seed=151)
    finally:
        fhe.set_f64(True)
    # (ks_ntt_kernel<LOGM, G0, NARROW, RNS, F64>: the last template argument is non-zero on the F64 instances)
    last = [a[a.index("<") + 1:a.index(">")].split(",")[-1].strip() for a in stage_a_instances(symbols)]
    assert last and all((a != "0") == f64 for a in last), symbols


def test_n8192_four_60_bit_moduli(fhe):
    """The benchmark's row size, batch 1, R = 3."""
    H.case_large(fhe, True, obfv.generate_moduli([60] * 4, 8192), 8192, 3, 1, seed=157)


@pytest.mark.parametrize("batch,logm", [(1, 13), (2, 14)], ids=["sub14", "whole-rows"])
def test_stock_16384_both_tile_choices(fhe, batch, logm):
    """Stock n = 16384 (nine moduli), R = 2: one ciphertext is small enough for 8192-point sub-block tiles in stage A
    (2 x 81 rows <= the compute units); two are not."""
    symbols = H.case_large(fhe, True, ref_params.DEFAULT_128[16384], 16384, 2, batch, seed=163)
    assert all(a.startswith("ks_ntt_kernel<%d," % logm) for a in stage_a_instances(symbols)), symbols


def test_n32768_sub_block_stage_a(fhe):
    """N = 32768 over [55, 60], batch 1, R = 2: rows above one LDS tile, stage A with two folded stages."""
    symbols = H.case_large(fhe, True, obfv.generate_moduli([55, 60], 32768), 32768, 2, 1, seed=167)
    assert any(a.startswith("ks_ntt_kernel<13, 2") for a in stage_a_instances(symbols)), symbols


def test_w_budget_counts_launches(fhe):
    """N = 4096 over three moduli, batch 3, R = 2 under a budget of two ciphertexts of one key modulus: two chunks x three
    groups = six stage-A launches and six stage-B launches."""
    q = obfv.generate_moduli([62, 60, 55], 4096)
    assert H.K.chunk_rule(3, 3, 3, 4096, 2 * 3 * 4096 * 8) == (2, 1)
    H.case_large(fhe, True, q, 4096, 2, 3, seed=173, w_budget=2 * 3 * 4096 * 8)
