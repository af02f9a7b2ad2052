"""Baby-step/giant-step hoisted matrix-vector product on the MI355X (the HIP build): tests/test_bsgs_emu.py's cases through
numpy arrays, torch tensors and DeviceArrays with the launches counted from the engine's profiler -- two passes' worth of
stage A, one bsgs_baby_kernel and one bsgs_giant_kernel per W, the summing kernel exactly when the giants were cut, never
the flat call's or the composition's kernels -- and the row kinds only the GPU suite reaches, each against the engine's
composition of existing calls."""
import pytest

import bsgs_cases as M
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
    """N = 16 over [62, 60, 55], baby exponents (1, 9), giant exponents (3, 3), batch 2: shared and per-item grids."""
    M.case_anchor(fhe, dev)


def test_deepest_level(fhe):
    """Keys and ciphertexts both at level 1 of the three-modulus set."""
    M.case_anchor(fhe, True, cl=1, kl=1, seed=302, variants=(False,))


def test_differs_from_the_flat_product_in_a_word(fhe):
    """The flat call over the composed exponents differs word for word."""
    M.case_anchor(fhe, True, seed=304, variants=(True,), flat=True)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_forms(fhe, dev):
    M.case_forms(fhe, dev)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_matrix_times_encrypted_vector(fhe, dev):
    M.case_matrix_vector(fhe, dev)


@pytest.mark.parametrize("ngiant", [2, 4], ids=["G3", "G5"])
def test_every_tile_instance_and_its_tail(fhe, ngiant):
    M.case_tiles(fhe, True, ngiant, profiled=True)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_giant_groups(fhe, dev):
    M.case_giant_groups(fhe, dev, profiled=True)


def test_baby_fold_at_the_top(fhe):
    """Sixteen 62-bit digits at N = 128, nbaby = 17, ngiant = 1, tile 2, every word at q_j - 1: the baby fold sees a
    seventeenth rotation after a fold, in both accumulator sets."""
    q = obfv.generate_moduli([62] * 16, 128)
    M.case_synthetic(fhe, True, q, 128, 17, 1, 1, seed=321, top=True, tile=2)


def test_giant_fold_at_the_top(fhe):
    """The same moduli, nbaby = 1, ngiant = 17 in one group: the carried giant accumulators pass sixteen products and
    sixteen addends."""
    q = obfv.generate_moduli([62] * 16, 128)
    M.case_synthetic(fhe, True, q, 128, 1, 17, 1, seed=323, top=True, rot_split=1)


def test_seventeen_digits(fhe):
    """17 digits of 58-bit moduli at N = 128, nbaby = ngiant = 1: both digit loops fold after sixteen terms."""
    q = obfv.generate_moduli([58] * 17, 128)
    M.case_synthetic(fhe, True, q, 128, 1, 1, 1, seed=325, rot_split=1)


def test_grid_tail(fhe):
    """N = 1024 over three moduli, batch 1, nbaby = ngiant = 1: two lane chunks per row, six key ranges in a grid rounded
    up to eight."""
    q = obfv.generate_moduli([62, 60, 55], 1024)
    M.case_synthetic(fhe, True, q, 1024, 1, 1, 1, seed=327)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_w_budget(fhe, dev):
    M.case_w_budget(fhe, dev, profiled=True)


def test_table_limits(fhe):
    M.case_table_limits(fhe, True)


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
def test_refusals(fhe, dev):
    M.case_refusals(fhe, dev)


# ---- the row kinds of the larger shapes ------------------------------------------------------------------------------------
def stage_a_instances(symbols):
    return [s[s.index("ks_ntt_kernel<"):] for s in symbols if "ks_ntt_kernel<" in s]


@pytest.mark.parametrize("f64", [True, False], ids=["f64", "integer"])
def test_stock_4096(fhe, f64):
    """The stock n = 4096 set, batch 2, nbaby = ngiant = 2, with the F64 option on -- stage A on doubles -- and off."""
    fhe.set_f64(f64)
    try:
        symbols = M.case_large(fhe, True, ref_params.DEFAULT_128[4096], 4096, 2, 2, 2, seed=329)
    finally:
        fhe.set_f64(True)
    last = [a[a.index("<") + 1:a.index(">")].split(",")[-1].strip() for a in stage_a_instances(symbols)]
    assert last and all((a != "0") == f64 for a in last), symbols


@pytest.mark.parametrize("tile", [0, 4], ids=["rule", "tile-4"])
def test_n8192_four_60_bit_moduli(fhe, tile):
    """The benchmark's row size, batch 1, nbaby = 2, ngiant = 4 (G = 5): under the rule and with tile 4 (4 + 1 groups)."""
    M.case_large(fhe, True, obfv.generate_moduli([60] * 4, 8192), 8192, 2, 4, 1, seed=331, tile=tile)


@pytest.mark.parametrize("batch,logm", [(1, 13), (2, 14)], ids=["sub14", "whole-rows"])
def test_stock_16384_both_tile_choices(fhe, batch, logm):
    """Stock n = 16384 (nine moduli), nbaby = 2, ngiant = 1: one ciphertext (and its one giant item) is small enough for
    8192-point sub-block tiles in stage A (2 x 81 rows <= the compute units); two are not."""
    symbols = M.case_large(fhe, True, ref_params.DEFAULT_128[16384], 16384, 2, 1, batch, seed=333, shared=batch == 1)
    assert all(a.startswith("ks_ntt_kernel<%d," % logm) for a in stage_a_instances(symbols)), symbols


def test_n32768_sub_block_stage_a(fhe):
    """N = 32768 over [55, 60], batch 1, nbaby = ngiant = 1: rows above one LDS tile, stage A with two folded stages."""
    symbols = M.case_large(fhe, True, obfv.generate_moduli([55, 60], 32768), 32768, 1, 1, 1, seed=335)
    assert any(a.startswith("ks_ntt_kernel<13, 2") for a in stage_a_instances(symbols)), symbols
