"""Encryption on the device (fhe_bfv_sample_small_dev, fhe_bfv_encrypt_sk_dev, fhe_bfv_encrypt_pk_dev): the kernel
sources under host emulation against the test-side restatement (tests/encrypt_ref.py) and against pins that do not
depend on it (sample statistics, round trips through the engine's and the oracle's decryption, fresh noise).
tests/test_encrypt_gpu.py runs the same cases on the MI355X."""
import ctypes as C
import random

import numpy as np
import pytest

import encode_cases as E
import encrypt_cases as X
import encrypt_ref as R
from fhe_oracle import bfv as obfv
from helpers import load_engine


@pytest.fixture(scope="module")
def fhe():
    return load_engine("emu")


VARIANCES = (1, 3, 10, 16, 17, 32)


def test_restatement_poly_forms():
    opar = obfv.BfvParameters.default_arc(3, 16)
    R.check_poly_forms(opar, bytes(range(32)))
    R.check_poly_forms(opar, bytes(range(32, 64)), level=2)


def test_restatement_stream_layout():
    """sample i of variance v <= 16 reads bits [4v i, 4v (i + 1)) of the next_u64 stream; v > 16 reads two words."""
    seed = bytes(range(7, 39))
    for v in (3, 17):
        g = R.generator(seed)
        words = [g.getrandbits(64) for _ in range(64)]
        bits = sum(w << (64 * i) for i, w in enumerate(words))
        xs = R.samples(seed, 16, v)[0]
        for i, x in enumerate(xs):
            pool = (bits >> (4 * v * i)) if v <= 16 else (bits >> (128 * i))
            m = (1 << (2 * v)) - 1
            assert x == bin(pool & m).count("1") - bin((pool >> (2 * v)) & m).count("1")


@pytest.mark.parametrize("n", [16, 256, 4096])
def test_sampler_parity(fhe, n):
    sizes = [50, 50, 40] if n == 4096 else [62, 60, 55]
    opar, par = E.params(fhe, n, E.stock_t(n) if n >= 256 else 1153, moduli_sizes=sizes)
    X.case_sampler_parity(fhe, False, opar, par, VARIANCES if n < 4096 else (3, 17), batch=2 if n < 4096 else 1)


@pytest.mark.parametrize("v", [1, 10, 32])
def test_sampler_consistency(fhe, v):
    opar, par = E.params(fhe, 16, 1153, moduli_sizes=[62] * 3)
    X.case_sampler_consistency(fhe, False, par, v, total=1 << 14)


def test_sampler_consistency_large(fhe):
    """About 2^20 samples, on a one-modulus context (the emulator's time goes into the lift of every row)."""
    opar, par = E.params(fhe, 4096, E.stock_t(4096), moduli_sizes=[62])
    X.case_sampler_consistency(fhe, False, par, 10, total=1 << 20)


@pytest.mark.parametrize("n,sizes", [(16, [62] * 3), (64, [62, 60, 55]), (4096, [50, 50, 40])], ids=["16", "64", "4096f64"])
def test_encrypt_parity(fhe, n, sizes):
    opar, par = E.params(fhe, n, 1153 if n == 16 else E.stock_t(n), moduli_sizes=sizes)
    X.case_encrypt_parity(fhe, False, opar, par, batch=3 if n < 4096 else 1)


def test_encrypt_f64_off_identical(fhe):
    n = 4096
    opar, par = E.params(fhe, n, E.stock_t(n), moduli_sizes=[50, 50, 40])
    sk = fhe.SecretKey.random(par, bytes(32))
    pk = fhe.PublicKey(sk, bytes(range(32)), bytes(range(1, 33)))
    pt = par.encoder().encode(E.values(random.Random(3), opar.plaintext, 1, n), "simd", 0, True)
    sd = [bytes([i] * 32) for i in range(1, 4)]

    def run():
        return [sk.encrypt(pt, 0, sd[0:1], sd[1:2]), pk.encrypt(pt, 0, sd[2:3]),
                par.context_at_level(0).sample_small(np.frombuffer(sd[0], dtype=np.uint8), 10)]
    on = run()
    fhe.set_f64(False)
    try:
        off = run()
    finally:
        fhe.set_f64(True)
    for a, b in zip(on, off):
        assert np.array_equal(a, b)


def test_roundtrip(fhe):
    opar, par = E.params(fhe, 16, 1153, moduli_sizes=[62] * 3)
    X.case_roundtrip(fhe, False, opar, par, level=0)
    X.case_roundtrip(fhe, False, opar, par, level=1, batch=1)


def test_parity_large_rows(fhe):
    """Rows of 32768 points: the element-wise passes around launch_ntt, against the restatement."""
    n = 32768
    opar, par = E.params(fhe, n, E.stock_t(n), moduli_sizes=[60])
    X.case_encrypt_parity(fhe, False, opar, par, levels=[0], batch=1)


def _code(fn):
    with pytest.raises(Exception) as err:
        fn()
    return getattr(err.value, "code", None)


def test_errors(fhe):
    from fhe_rs_amd import _lib
    L = _lib.lib()
    n = 16
    opar, par = E.params(fhe, n, 1153, moduli_sizes=[62] * 3)
    ctx = par.context_at_level(0)
    sd = fhe.DeviceArray.from_numpy(np.zeros((1, 32), dtype=np.uint8))
    key = fhe.DeviceArray.from_numpy(np.zeros((2, 3, n), dtype=np.uint64))
    out = fhe.DeviceArray((1, 2, 3, n))
    p = lambda a: C.c_void_p(a.data_ptr())   # noqa: E731
    for v in (0, 33):
        assert L.fhe_bfv_sample_small_dev(ctx._h, v, p(sd), 1, p(out), 1, None) == -24
        assert L.fhe_bfv_encrypt_sk_dev(ctx._h, v, p(key), p(sd), p(sd), None, 0, p(out), 1, None) == -24
        assert L.fhe_bfv_encrypt_pk_dev(ctx._h, v, p(key), p(sd), None, 0, p(out), 1, None) == -24
    bad = fhe.BfvParameters(n, 1153, moduli=opar.moduli, variance=40)
    assert _code(lambda: fhe.SecretKey.random(bad)) == -24
    # null handles and buffers
    assert L.fhe_bfv_sample_small_dev(None, 10, p(sd), 1, p(out), 1, None) == -1
    assert L.fhe_bfv_sample_small_dev(ctx._h, 10, None, 1, p(out), 1, None) == -1
    assert L.fhe_bfv_sample_small_dev(ctx._h, 10, p(sd), 1, None, 1, None) == -1
    assert L.fhe_bfv_encrypt_sk_dev(None, 10, p(key), p(sd), p(sd), None, 0, p(out), 1, None) == -1
    assert L.fhe_bfv_encrypt_sk_dev(ctx._h, 10, None, p(sd), p(sd), None, 0, p(out), 1, None) == -1
    assert L.fhe_bfv_encrypt_sk_dev(ctx._h, 10, p(key), None, p(sd), None, 0, p(out), 1, None) == -1
    assert L.fhe_bfv_encrypt_sk_dev(ctx._h, 10, p(key), p(sd), None, None, 0, p(out), 1, None) == -1
    assert L.fhe_bfv_encrypt_sk_dev(ctx._h, 10, p(key), p(sd), p(sd), None, 0, None, 1, None) == -1
    assert L.fhe_bfv_encrypt_pk_dev(None, 10, p(key), p(sd), None, 0, p(out), 1, None) == -1
    assert L.fhe_bfv_encrypt_pk_dev(ctx._h, 10, None, p(sd), None, 0, p(out), 1, None) == -1
    assert L.fhe_bfv_encrypt_pk_dev(ctx._h, 10, p(key), None, None, 0, p(out), 1, None) == -1
    assert L.fhe_bfv_encrypt_pk_dev(ctx._h, 10, p(key), p(sd), None, 0, None, 1, None) == -1
    # batch 0: OK, nothing written, NULL buffers accepted
    assert L.fhe_bfv_sample_small_dev(ctx._h, 10, None, 1, None, 0, None) == 0
    assert L.fhe_bfv_encrypt_sk_dev(ctx._h, 10, None, None, None, None, 0, None, 0, None) == 0
    assert L.fhe_bfv_encrypt_pk_dev(ctx._h, 10, None, None, None, 0, None, 0, None) == 0
    # a host-only context
    host = fhe.Context(opar.moduli, n, device=-1)
    assert L.fhe_bfv_sample_small_dev(host._h, 10, p(sd), 1, p(out), 1, None) == -18
    assert L.fhe_bfv_encrypt_sk_dev(host._h, 10, p(key), p(sd), p(sd), None, 0, p(out), 1, None) == -18
    assert L.fhe_bfv_encrypt_pk_dev(host._h, 10, p(key), p(sd), None, 0, p(out), 1, None) == -18
    # the Python layer: one seed per plaintext, the plaintext at the encryption level
    sk = fhe.SecretKey.random(par)
    pt = np.zeros((2, 3, n), dtype=np.uint64)
    with pytest.raises(Exception):
        sk.encrypt(pt, 0, [bytes(32)], [bytes(32)])
    with pytest.raises(Exception):
        sk.encrypt(pt, 1)
    # one e seed per a seed: a short e seed array would be read past its end
    three = [bytes([i]) * 32 for i in range(3)]
    with pytest.raises(fhe.FheError):
        sk.encrypt(pt[:1].repeat(3, axis=0), 0, three, three[:1])
    with pytest.raises(fhe.FheError):
        sk.encrypt(None, 0, three, three[:2])
    with pytest.raises(fhe.FheError):
        sk.encrypt(pt[:1].repeat(3, axis=0), 0, three, np.zeros((4, 32), dtype=np.uint8))
    dev_e = fhe.DeviceArray.from_numpy(np.zeros((1, 32), dtype=np.uint8))
    with pytest.raises(fhe.FheError):
        sk.encrypt(pt[:1].repeat(3, axis=0), 0, three, dev_e)
    pk = fhe.PublicKey(sk)
    with pytest.raises(fhe.FheError):
        pk.encrypt(pt[:1].repeat(3, axis=0), 0, three[:2])


@pytest.mark.parametrize("v", [3, 17])
def test_draws_start_at_word_boundaries(fhe, v):
    """N = 8 with odd v: a draw of 8 samples leaves 32 bits of its last word unused, and the next draw (e1, e2 of a
    public-key encryption) starts at the next word, as each sample_vec_cbd call starts a fresh pool."""
    from fhe_oracle import bfv as ob
    opar = ob.BfvParameters(8, 1153, moduli_sizes=[62, 60], variance=v)
    par = fhe.BfvParameters(8, 1153, moduli=opar.moduli, variance=v)
    assert (8 * 4 * v) % 64 != 0 or v > 16
    X.case_sampler_parity(fhe, False, opar, par, (v,), batch=2)
    X.case_encrypt_parity(fhe, False, opar, par, batch=3)
