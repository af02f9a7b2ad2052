"""CPU pins of tests/transcode_ref.py -- the restatement of fhe-util's transcoders the packed-bits tests compare with --
against the oracle's transcode_from_bytes / transcode_to_bytes, and of the restated encode_database and SealPIR fold
(tests/transcode_cases.py) on the examples' own figures.  (Every test here calls the engine's new interface at least
for its counts: fhe_transcode_count, fhe_bfv_encode_words_count, number_elements_per_plaintext.)"""
import random

import numpy as np
import pytest

import transcode_cases as TC
import transcode_ref as T
from fhe_oracle import bfv as obfv
from fhe_oracle.rq import Poly, transcode_from_bytes, transcode_to_bytes
from helpers import load_engine


@pytest.fixture(scope="module")
def fhe():
    return load_engine("emu")


def test_equals_the_oracles_byte_transcoders(fhe):
    """Every nbits in 1 ... 64, lengths that leave a partial last element included."""
    from fhe_rs_amd import _lib
    rng = random.Random(1)
    for nbits in range(1, 65):
        for nbytes in (1, 2, 7, 8, 9, 31):
            b = rng.randbytes(nbytes)
            want = transcode_from_bytes(b, nbits)
            assert T.transcode(b, 8, nbits) == want, (nbits, nbytes)
            assert _lib.lib().fhe_transcode_count(8, nbytes, nbits) == len(want)
        for n in (1, 2, 5, 8, 17):
            a = [rng.getrandbits(64) for _ in range(n)]   # (bits above nbits: both mask them off)
            want = transcode_to_bytes(a, nbits)
            assert bytes(T.transcode(a, nbits, 8)) == want, (nbits, n)
            assert _lib.lib().fhe_transcode_count(nbits, n, 8) == len(want)


def test_round_trip_every_pair(fhe):
    from fhe_rs_amd import _lib
    rng = random.Random(2)
    for i in range(1, 65):
        a = [rng.getrandbits(i) for _ in range(11)]
        for o in range(1, 65):
            there = T.transcode(a, i, o)
            assert len(there) == _lib.lib().fhe_transcode_count(i, len(a), o)
            assert T.transcode(there, o, i)[:len(a)] == a, (i, o)


# the examples' figures: N = 4096, t = 2056193 (nbits 20), a 36-bit q_0, 288-byte elements
N, T_MOD, SIZES = 4096, 2056193, [36, 36, 37]


@pytest.fixture(scope="module")
def opar():
    return obfv.BfvParameters(N, T_MOD, moduli_sizes=SIZES)


def oracle_plain(opar, values, level):
    """Plaintext::try_encode(values, Encoding::poly_at_level(level)).poly_ntt from the oracle's Poly alone."""
    ctx = opar.ctx[level]
    v = list(values) + [0] * (opar.degree() - len(values))
    return np.array(Poly.from_u64(ctx, v).into_ntt().coefficients, dtype=np.uint64)


def test_encode_database_on_the_examples_figures(fhe, opar):
    nbits = TC.ilog2(T_MOD)
    per = fhe.number_elements_per_plaintext(N, nbits, 288)
    assert nbits == 20 and per == 35
    item_bytes = per * 288
    assert item_bytes == 10080 and (item_bytes * 8) % nbits == 0 and item_bytes * 8 // nbits == 4032 < N
    rng = random.Random(3)
    data = rng.randbytes(item_bytes + 288 * 3)            # one full plaintext and a short one
    vals = TC.database_values(data, item_bytes, nbits, 3)
    assert [len(v) for v in vals] == [4032, -(-288 * 3 * 8 // nbits), 0]
    assert vals[0] == transcode_from_bytes(data[:item_bytes], nbits)
    for v in vals[:2]:
        assert np.array_equal(TC.plaintext_rows(opar, v, 1, False), oracle_plain(opar, v, 1))


def test_fold_on_the_examples_figures(fhe, opar):
    from fhe_rs_amd import _lib
    nbits = 20
    q0 = opar.moduli[0]
    assert q0.bit_length() == 36
    m = T.count(N, 36, nbits)
    assert m == 7373 == _lib.lib().fhe_transcode_count(36, N, nbits)
    rng = random.Random(4)
    c = [[rng.randrange(q0) for _ in range(N)] for _ in range(2)]
    chunks = TC.fold_values(c, 36, nbits, N)
    assert [len(v) for v in chunks] == [N, N, N, 2 * m - 3 * N]    # four plaintexts per folded ciphertext
    par = fhe.BfvParameters(N, T_MOD, moduli=opar.moduli)
    assert _lib.lib().fhe_bfv_encode_words_count(par.encoder()._h, 36, 2, N, nbits) == 4
    flat = sum(chunks, [])
    assert T.transcode(flat[:m], nbits, 36)[:N] == c[0] and T.transcode(flat[m:], nbits, 36)[:N] == c[1]
    for v in (chunks[1], chunks[3]):                               # the join of c0 and c1 lies in chunk 1
        assert np.array_equal(TC.plaintext_rows(opar, v, 1, False), oracle_plain(opar, v, 1))
