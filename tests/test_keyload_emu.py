"""Key-switching keys from and to their wire bytes (fhe_ksk_load_wire_dev, fhe_ksk_serialize_dev): the kernel sources
under host emulation (N <= 2048, and one key above one LDS tile) against tests/keyload_ref.py.
tests/test_keyload_gpu.py runs the same cases on the MI355X, on every kernel instance."""
import numpy as np
import pytest

import devop_cases as D
import encode_cases as E
import keygen_cases as G
import keygen_ref as R
import keyload_cases as K
import keyload_ref as KR
from fhe_oracle.rq import NTT_SHOUP, poly_from_wire
from helpers import load_engine


@pytest.fixture(scope="module")
def fhe():
    return load_engine("emu")


def params(fhe, n, sizes, t=None):
    return G.params(fhe, n, t or E.stock_t(n), moduli_sizes=sizes)


# ---- the expectation itself --------------------------------------------------------------------------------------------
def test_expectation_is_the_oracles_wire_format():
    """The packed bytes parse back (the oracle's TryConvertFrom<&Rq>) to the key's words, and the seeded c1 is
    generate_c1 of K."""
    from fhe_oracle import bfv as obfv
    opar = obfv.BfvParameters(16, 1153, moduli_sizes=[62, 60, 55])
    for cl, kl in ((0, 0), (1, 0), (2, 2)):
        k = KR.key(opar, cl, kl, 1)
        kc = opar.ctx[kl]
        assert k["w0"].shape == (k["nd"], KR.poly_bytes(kc))
        for i in range(k["nd"]):
            assert poly_from_wire(kc, k["w0"][i].tobytes(), NTT_SHOUP).coefficients == k["c0"][i].tolist()
            assert poly_from_wire(kc, k["w1"][i].tobytes(), NTT_SHOUP).coefficients == k["c1"][i].tolist()
        assert np.array_equal(KR.seeded_c1(kc, k["K"], k["nd"]), k["c1"])
        assert (k["lb"] != 0) == (kl == 2) and k["nd"] == R.digits(opar.ctx[cl], kc)[0]


# ---- the engine against it ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cl,kl", [(0, 0), (1, 0), (1, 1), (2, 2)], ids=["00", "10", "11", "decomposition"])
def test_load_small(fhe, cl, kl):
    opar, par = params(fhe, 16, [62, 60, 55], 1153)
    K.case_load(fhe, False, opar, par, cl, kl, key_seeds=(1, 2))


def test_load_single_key_shape(fhe):
    opar, par = params(fhe, 16, [62, 60, 55], 1153)
    K.case_single(fhe, False, opar, par)


@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "offset1"])
def test_rows_at_odd_byte_offsets(fhe, misalign):
    """N = 8 over moduli of three bit lengths: a row is nbits bytes, so rows start at odd offsets (the byte path)."""
    opar, par = params(fhe, 8, [61, 35, 27], 1153)
    kc = opar.ctx[0]
    assert [KR.wire_bits(q) for q in kc.moduli] == [61, 35, 27]
    K.case_load(fhe, False, opar, par, 0, 0, misalign=misalign)


def test_decomposition_key_8_points(fhe):
    opar, par = params(fhe, 8, [45], 1153)
    k = KR.key(opar, 0, 0, 1)
    assert k["lb"] != 0
    K.case_load(fhe, False, opar, par, 0, 0, misalign=True)


@pytest.mark.parametrize("n,misalign", [(64, False), (64, True), (128, False), (128, True)])
def test_word_path_threshold(fhe, n, misalign):
    """N = 64 always reads bytes; N = 128 reads words from an aligned pointer and bytes from a misaligned one."""
    opar, par = params(fhe, n, [62, 53, 36])
    K.case_load(fhe, False, opar, par, 0, 0, misalign=misalign)


@pytest.mark.parametrize("sizes", [[62, 45], [58, 40], [50, 44]], ids=["general", "narrow", "below_2p50"])
def test_2048_points(fhe, sizes):
    opar, par = params(fhe, 2048, sizes)
    K.case_load(fhe, False, opar, par, 0, 0)


def test_rows_larger_than_lds(fhe):
    """N = 32768 over two moduli: unpack into the handle, the compare on the PowerBasis words, launch_ntt, the
    element-wise twins -- and the range check on that route, whose transform would hide an unreduced word."""
    opar, par = params(fhe, 32768, [50, 55])
    K.case_load(fhe, False, opar, par, 0, 0, switch=False)
    K.case_range(fhe, False, opar, par, nkeys=1, rows=(1,), coeffs=(32767,))


def test_one_more_key_than_a_launch_group(fhe):
    """33 keys at N = 8: the group rule splits them 17 + 16; both neighbours of the boundary and the ends."""
    opar, par = params(fhe, 8, [62, 60], 1153)
    nkeys = D.KG_KEYS + 1
    g = D.launch_group(2, 8, 2, nkeys, 1 << 30, D.KG_KEYS)
    assert g == 17 and D.boundary_items(nkeys, g) == [0, 16, 17, 32]
    K.case_load(fhe, False, opar, par, 0, 0, key_seeds=tuple(range(100, 100 + nkeys)), check={0, 16, 17, 32})


def test_generated_key_round_trip(fhe):
    opar, par = params(fhe, 16, [62, 60, 55], 1153)
    K.case_generated_to_wire(fhe, False, opar, par)


def test_key_types(fhe):
    opar, par = params(fhe, 16, [62, 60, 55], 1153)
    K.case_types(fhe, False, opar, par)


@pytest.mark.parametrize("n,sizes", [(8, [61, 35, 27]), (128, [62, 53]), (8, [45])], ids=["bytes", "words", "decomposition"])
def test_range_check(fhe, n, sizes):
    opar, par = params(fhe, n, sizes, 1153 if n == 8 else None)
    K.case_range(fhe, False, opar, par)


def test_statuses(fhe):
    opar, par = params(fhe, 16, [62, 60, 55], 1153)
    K.case_statuses(fhe, False, opar, par)
