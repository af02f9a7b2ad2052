"""Hoisted matrix-vector product on the MI355X (the HIP build): tests/test_hoistmv_emu.py's cases through numpy arrays,
torch tensors and DeviceArrays with the launches counted from the engine's profiler -- one stage A per chunk and
key-modulus group, one fused stage B per table of rotations, the summing kernel exactly when the call has more than one
rotation group, never hoist_mac_kernel or the dot product -- and the row kinds only the GPU suite reaches, each against the
composition of the two existing engine calls."""
import pytest

import hoistmv_cases as M
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
    """N = 16 over [62, 60, 55], exponents (1, 3, 9, 31, 3), batch 2: shared / per-item diagonals, with / without pt0."""
    M.case_anchor(fhe, dev)


def test_deepest_level(fhe):
    """Keys and ciphertexts both at level 1 of the three-modulus set."""
    M.case_anchor(fhe, True, cl=1, kl=1, seed=205, variants=[(False, True)])


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
    M.case_synthetic(fhe, True, q, 128, 17, 1, seed=219, top=True, rot_split=1)


def test_seventeen_digits(fhe):
    """17 digits of 58-bit moduli at N = 128, R = 2: the digit accumulators fold after sixteen terms."""
    q = obfv.generate_moduli([58] * 17, 128)
    M.case_synthetic(fhe, True, q, 128, 2, 1, seed=221, rot_split=1)


def test_table_boundary(fhe):
    M.case_table_boundary(fhe, True)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_rotation_groups(fhe, dev):
    M.case_rot_split(fhe, dev, profiled=True)


def test_grid_tail(fhe):
    """N = 1024 over three moduli, R = 2, batch 1: two lane chunks per row, six key ranges in a grid rounded up to eight."""
    q = obfv.generate_moduli([62, 60, 55], 1024)
    M.case_synthetic(fhe, True, q, 1024, 2, 1, seed=223)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_w_budget(fhe, dev):
    M.case_w_budget(fhe, dev, profiled=True)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_refusals(fhe, dev):
    M.case_refusals(fhe, dev)


# ---- the row kinds of the larger shapes ------------------------------------------------------------------------------------
def stage_a_instances(symbols):
    return [s[s.index("ks_ntt_kernel<"):] for s in symbols if "ks_ntt_kernel<" in s]


@pytest.mark.parametrize("f64", [True, False], ids=["f64", "integer"])
def test_stock_4096(fhe, f64):
    """The stock n = 4096 set, batch 2, R = 3, with the F64 option on -- stage A on doubles -- and off."""
    fhe.set_f64(f64)
    try:
        symbols = M.case_large(fhe, True, ref_params.DEFAULT_128[4096], 4096, 3, 2, seed=225)
    finally:
        fhe.set_f64(True)
    last = [a[a.index("<") + 1:a.index(">")].split(",")[-1].strip() for a in stage_a_instances(symbols)]
    assert last and all((a != "0") == f64 for a in last), symbols


@pytest.mark.parametrize("split", [0, 1], ids=["rule", "one-group"])
def test_n8192_four_60_bit_moduli(fhe, split):
    """The benchmark's row size, batch 1, R = 3: under the rule (64 blocks: cut into groups) and in one group."""
    M.case_large(fhe, True, obfv.generate_moduli([60] * 4, 8192), 8192, 3, 1, seed=227, rot_split=split)


@pytest.mark.parametrize("batch,logm", [(1, 13), (2, 14)], ids=["sub14", "whole-rows"])
def test_stock_16384_both_tile_choices(fhe, batch, logm):
    """Stock n = 16384 (nine moduli), R = 2: one ciphertext is small enough for 8192-point sub-block tiles in stage A
    (2 x 81 rows <= the compute units); two are not."""
    symbols = M.case_large(fhe, True, ref_params.DEFAULT_128[16384], 16384, 2, batch, seed=229, shared=batch == 1)
    assert all(a.startswith("ks_ntt_kernel<%d," % logm) for a in stage_a_instances(symbols)), symbols


def test_n32768_sub_block_stage_a(fhe):
    """N = 32768 over [55, 60], batch 1, R = 2: rows above one LDS tile, stage A with two folded stages."""
    symbols = M.case_large(fhe, True, obfv.generate_moduli([55, 60], 32768), 32768, 2, 1, seed=231)
    assert any(a.startswith("ks_ntt_kernel<13, 2") for a in stage_a_instances(symbols)), symbols


def test_w_budget_counts_launches(fhe):
    """N = 4096 over three moduli, batch 3, R = 2 under a budget of two ciphertexts of one key modulus: two chunks x three
    groups = six stage-A launches and six fused stage-B launches."""
    q = obfv.generate_moduli([62, 60, 55], 4096)
    assert M.K.chunk_rule(3, 3, 3, 4096, 2 * 3 * 4096 * 8) == (2, 1)
    M.case_large(fhe, True, q, 4096, 2, 3, seed=233, w_budget=2 * 3 * 4096 * 8, shared=False)
