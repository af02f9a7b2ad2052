"""Keyed batches on the MI355X (the HIP build): tests/test_keyed_emu.py's cases through numpy arrays, torch tensors and
DeviceArrays, and the row kinds only the GPU suite reaches -- the folded Galois gathers at N = 4096, the F64 stage A of
the stock n = 4096 set, N = 8192 over four 60-bit moduli, and the sub-block stage A at N = 32768 -- each with the launched
kernel symbols read back from the engine's profiler."""
import re

import pytest

import keyed_cases as K
import ref_params
from fhe_oracle import bfv as obfv
from helpers import HIP_LIB, load_engine

pytestmark = pytest.mark.gpu
FORMS = [False, True, "abi"]
IDS = ["host", "torch", "abi"]
SMALL = (16, [62, 60, 55])


@pytest.fixture(scope="module")
def fhe():
    eng = load_engine("hip")
    from fhe_rs_amd import _lib
    assert _lib.loaded_path() == HIP_LIB, "GPU tests must run on the HIP build"
    assert eng.device_count() >= 1, "no HIP device visible"
    return eng


@pytest.mark.parametrize("dev", FORMS, ids=IDS)
@pytest.mark.parametrize("nkeys,per_key", [(3, 1), (3, 2)])
def test_key_mapping(fhe, dev, nkeys, per_key):
    """N = 16 over [62, 60, 55]: one partial workgroup per row (2 * ci >= n), three clients with one and with two items."""
    opar, par = K.params(fhe, *SMALL)
    K.case_relin(fhe, dev, opar, par, nkeys, per_key)


def test_more_keys_than_an_argument_table_holds(fhe):
    """65 clients x 1 item at N = 16: the key table lives in device memory."""
    opar, par = K.params(fhe, *SMALL)
    K.case_relin(fhe, True, opar, par, 65, 1)


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
    K.case_relin(fhe, True, opar, par, 3, 2, cl, kl)
    K.case_galois(fhe, True, opar, par, 3, 1, (3,), cl, kl)


def test_grid_tail(fhe):
    """N = 1024 over three moduli: two lane chunks per row, six key ranges in a grid rounded up to eight (kr >= nkr)."""
    q = obfv.generate_moduli([62, 60, 55], 1024)
    K.case_synthetic(fhe, True, q, 1024, 2, 1, seed=61, exps=(3,))


def test_seventeen_digits(fhe):
    """17 digits of 58-bit moduli at N = 128: the accumulators fold after sixteen terms."""
    q = obfv.generate_moduli([58] * 17, 128)
    K.case_synthetic(fhe, True, q, 128, 2, 2, seed=67)


def test_sixteen_digits_at_the_top(fhe):
    """Sixteen 62-bit digits, every input word and every key word at q_i - 1: sixteen products of the largest size in
    each 128-bit accumulator."""
    q = obfv.generate_moduli([62] * 16, 128)
    K.case_synthetic(fhe, True, q, 128, 2, 2, seed=71, top=True)


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


# ---- the row kinds of the larger shapes: the single-key engine call is the reference -------------------------------------
def keyed_calls(fhe, sy, per_key, n, exps):
    """One keyed key_switch, relinearization and rotation on zeroed device arrays (the kernels that run, not the values)."""
    import torch
    L, b = len(sy.q), sy.nkeys * per_key
    p = torch.zeros((b, L, n), dtype=torch.int64, device="cuda")
    ct3 = torch.zeros((b, 3, L, n), dtype=torch.int64, device="cuda")
    sy.set.key_switch(p)
    sy.set.relinearizes(ct3)
    for e in exps:
        sy.set.relinearize(e, ct3[:, :2].contiguous())
    torch.cuda.synchronize()


@pytest.mark.parametrize("dev", [True, "abi"], ids=["torch", "abi"])
def test_folded_galois_gathers(fhe, dev):
    """N = 4096 over three moduli, exponents 3 and 2N - 1: the substitution read as a gather by stage B's own-row and
    addend reads, with `out` apart from `ct` and with out == ct (the copying path)."""
    q = obfv.generate_moduli([62, 60, 55], 4096)
    sy = K.case_synthetic(fhe, dev, q, 4096, 3, 2, seed=79, exps=(3, 8191), oracle=False, in_place=True)
    K.assert_keyed_kernels(K.kernels_of(fhe, lambda: keyed_calls(fhe, sy, 2, 4096, (3,))))


@pytest.mark.parametrize("f64", [True, False], ids=["f64", "integer"])
def test_stock_4096(fhe, f64):
    """The stock n = 4096 set (36 / 36 / 37-bit moduli) with the F64 option on -- stage A on doubles -- and off."""
    fhe.set_f64(f64)
    try:
        sy = K.case_synthetic(fhe, True, ref_params.DEFAULT_128[4096], 4096, 3, 2, seed=83, exps=(3,), oracle=False)
        symbols = K.kernels_of(fhe, lambda: keyed_calls(fhe, sy, 2, 4096, (3,)))
    finally:
        fhe.set_f64(True)
    K.assert_keyed_kernels(symbols)
    # (ks_ntt_kernel<LOGM, G0, NARROW, RNS, F64>: the last template argument is non-zero on the F64 instances)
    stage_a = [re.search(r"ks_ntt_kernel<([^>]*)>", s).group(1).split(",")[-1].strip() for s in symbols if "ks_ntt_kernel<" in s]
    assert stage_a and all((a != "0") == f64 for a in stage_a), symbols


def test_n8192_five_clients(fhe):
    """N = 8192 over 4 x 60 bits, 5 clients x 3 items."""
    q = obfv.generate_moduli([60] * 4, 8192)
    sy = K.case_synthetic(fhe, True, q, 8192, 5, 3, seed=89, exps=(3,), oracle=False)
    K.assert_keyed_kernels(K.kernels_of(fhe, lambda: keyed_calls(fhe, sy, 3, 8192, (3,))))


def test_n32768_sub_block_stage_a(fhe):
    """N = 32768 over [55, 60], 3 clients x 1 item: stage A on 8192-point sub-blocks with two folded stages."""
    q = obfv.generate_moduli([55, 60], 32768)
    sy = K.case_synthetic(fhe, True, q, 32768, 3, 1, seed=97, exps=(3,), oracle=False)
    symbols = K.kernels_of(fhe, lambda: keyed_calls(fhe, sy, 1, 32768, (3,)))
    K.assert_keyed_kernels(symbols)
    assert any("ks_ntt_kernel<13, 2" in s for s in symbols), symbols


def test_multiply_then_keyed_relinearization_stock_4096(fhe):
    """The composition on the stock n = 4096 set against Multiplicator.default(par, rk_c).multiply client by client."""
    K.case_multiply_engine(fhe, True, ref_params.params(fhe, 4096), 3, 2)
