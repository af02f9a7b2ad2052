"""Plaintexts from packed bits (fhe_bfv_encode_bytes_dev, fhe_bfv_encode_words_dev, fhe_transcode_dev): the kernel
sources under host emulation against tests/transcode_ref.py, every output word, at the smallest shapes at which each
mistake shows.  tests/test_transcode_gpu.py runs the same cases on the MI355X, on every kernel instance."""
import pytest

import transcode_cases as TC
import transcode_ref as T
from helpers import load_engine

SMALL = [62, 60, 55]
THREE = [62, 52, 40]      # (general at level 0; the deepest level alone is narrow)
T_BITS = (2, 14, 21, 34, 61)


@pytest.fixture(scope="module")
def fhe():
    return load_engine("emu")


def shape(fhe, n, sizes, t_bits):
    return TC.params(fhe, n, TC.plaintext_modulus(t_bits, n, sizes), sizes)


# ---- fhe_transcode_dev -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_bits", TC.WIDTHS)
def test_transcode_every_pair(fhe, in_bits):
    """nin 1 ... 257: partial last elements at both ends of a workgroup of 256 lanes."""
    TC.case_transcode(fhe, False, in_widths=(in_bits,), seed=in_bits)


def test_transcode_device_arrays(fhe):
    TC.case_transcode(fhe, "abi", in_widths=(8, 20, 36), out_widths=(8, 20, 36), nins=(9, 257))


def test_transcode_shapes_and_counts(fhe):
    TC.case_transcode_misc(fhe, False)


# ---- fhe_bfv_encode_bytes_dev ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_bits", T_BITS)
@pytest.mark.parametrize("n,sizes", [(8, SMALL), (16, SMALL), (256, THREE)], ids=["8", "16", "256"])
def test_encode_bytes(fhe, n, sizes, t_bits):
    opar, par = shape(fhe, n, sizes, t_bits)
    assert TC.ilog2(opar.plaintext) == t_bits - 1
    partial = TC.case_encode_bytes(fhe, False, opar, par, seed=n + t_bits)
    if t_bits in (14, 21, 34):
        assert partial      # an item whose bits are no multiple of nbits: a partial last value


def test_encode_bytes_defaults(fhe):
    opar, par = shape(fhe, 16, SMALL, 21)
    TC.case_encode_bytes_defaults(fhe, False, opar, par)


# ---- fhe_bfv_encode_words_dev ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_bits", [21, 34])
def test_encode_words(fhe, t_bits):
    """N = 16: (36, 20) is the examples' ratio -- M = 29 values per segment, no multiple of N, so with two segments the
    join falls inside plaintext 1 and the fourth plaintext is padded; seg_len 5 and 37 put several joins in one plaintext
    and a segment across three."""
    opar, par = shape(fhe, 16, SMALL, t_bits)
    seen = TC.case_encode_words(fhe, False, opar, par, seg_lens=(5, 37))
    assert T.count(16, 36, 20) == 29 and seen[(36, 20, 2, 16)] == 4 and seen[(36, 20, 1, 16)] == 2
    assert seen[(20, 20, 2, 16)] == 2 and seen[(13, 34, 2, 16)] == 1 and seen[(13, 34, 2, 37)] == 2


def test_encode_words_256(fhe):
    opar, par = shape(fhe, 256, THREE, 21)
    TC.case_encode_words(fhe, False, opar, par, pairs=((36, 20),), nsegs=(2,), batch=2)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_statuses(fhe):
    import bigt_cases as B
    opar, par = shape(fhe, 16, SMALL, 21)
    _obig, par_big = B.params(fhe, "C", 16)
    TC.case_statuses(fhe, False, opar, par, par_big)


# ---- rows larger than one LDS tile -------------------------------------------------------------------------------------
def test_rows_larger_than_lds(fhe):
    """N = 32768, batch 2: the values through transcode_ew_kernel into scratch, encode_lift_ew_kernel, launch_ntt."""
    import random

    import numpy as np
    from fhe_oracle import coracle
    n = 32768
    opar, par = TC.params(fhe, n, 2056193, [50, 55])
    enc = par.encoder()
    cctx = coracle.CCtx(opar.ctx[0])
    rng = random.Random(7)
    ib = 1001
    TC.check_bytes(fhe, False, opar, enc, cctx, TC.rand_bytes(rng, ib + 333), ib, 20, 2, 0, True, what="32768 bytes")
    w = np.array([[[rng.getrandbits(64) for _ in range(n)] for _ in range(2)] for _ in range(2)], dtype=np.uint64)
    assert TC.check_words(fhe, False, opar, enc, cctx, w, 36, 20, 0, False, what="32768 words") == 4


# ---- one SealPIR round -------------------------------------------------------------------------------------------------
def test_sealpir_round(fhe):
    assert TC.case_sealpir_round(fhe, False, 64) == 4
