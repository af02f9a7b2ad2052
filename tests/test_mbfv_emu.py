"""Multiparty BFV on the device (fhe_mbfv_*_dev): the kernel sources under host emulation against the test-side
restatement of crates/fhe/src/mbfv/ (tests/mbfv_ref.py) and against the protocols' own ends -- a threshold decryption
gives the plaintext back, a switched ciphertext decrypts under the output secret, the collective relinearization key
relinearizes.  tests/test_mbfv_gpu.py runs the same cases, and the full-size ones, on the MI355X."""
import ctypes as C

import numpy as np
import pytest

import encode_cases as E
import mbfv_cases as M
from fhe_oracle import bfv as obfv
from helpers import load_engine


@pytest.fixture(scope="module")
def fhe():
    return load_engine("emu")


def arc(fhe, nmod, n):
    """The reference's test sets: BfvParameters::default_arc(nmod, n), t = 1153 and 62-bit moduli."""
    return E.params(fhe, n, 1153, moduli_sizes=[62] * nmod)


SMALL = [(1, 16), (6, 32)]


@pytest.mark.parametrize("nmod,n", SMALL)
def test_share_parity(fhe, nmod, n):
    opar, par = arc(fhe, nmod, n)
    M.case_share_parity(fhe, False, opar, par)


def test_share_parity_4096_f64(fhe):
    """One item of the stock n = 4096 set (every modulus below 2^50: the F64 instances), and the integer instances
    after set_f64(False): both equal the restatement."""
    import ref_params
    opar, par = E.params(fhe, 4096, ref_params.plaintext_modulus(4096), moduli=ref_params.DEFAULT_128[4096])
    M.case_share_parity(fhe, False, opar, par, parties=1, cts=1, levels=[0])
    fhe.set_f64(False)
    try:
        M.case_share_parity(fhe, False, opar, par, parties=1, cts=1, levels=[0])
    finally:
        fhe.set_f64(True)


@pytest.mark.parametrize("n", [8, 4096])
def test_sum_overflow(fhe, n):
    """The largest 62-bit primes generate_moduli yields, every word q - 1."""
    opar, par = E.params(fhe, n, 1153 if n == 8 else E.stock_t(n), moduli_sizes=[62, 62])
    assert all(int(m).bit_length() == 62 for m in par.moduli)
    M.case_sum_overflow(fhe, False, par, n)


@pytest.mark.parametrize("nmod,n", SMALL)
def test_encrypt_decrypt(fhe, nmod, n):
    opar, par = arc(fhe, nmod, n)
    M.case_encrypt_decrypt(fhe, False, opar, par)


@pytest.mark.parametrize("nmod,n", SMALL)
def test_encrypt_keyswitch_decrypt(fhe, nmod, n):
    opar, par = arc(fhe, nmod, n)
    M.case_keyswitch_decrypt(fhe, False, opar, par)


@pytest.mark.parametrize("nmod,n", [(3, 16), (6, 32)])
def test_relinearization_works(fhe, nmod, n):
    opar, par = arc(fhe, nmod, n)
    M.case_relinearization(fhe, False, opar, par)


def _code(fn):
    with pytest.raises(Exception) as err:
        fn()
    return getattr(err.value, "code", None)


def test_errors(fhe):
    from fhe_rs_amd import _lib
    L = _lib.lib()
    n = 16
    opar, par = arc(fhe, 3, n)
    ctx = par.context_at_level(0)
    sd = fhe.DeviceArray.from_numpy(np.zeros((1, 32), dtype=np.uint8))
    a = fhe.DeviceArray.from_numpy(np.zeros((3, 3, n), dtype=np.uint64))   # any [L][L][N] operand
    o0, o1 = fhe.DeviceArray((3, 3, n)), fhe.DeviceArray((3, 3, n))
    p = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
    sc = par.plain_scaler(0)
    calls = {   # name -> (arguments of a valid call, indices of its non-optional buffers)
        "fhe_mbfv_pk_share_dev": ([ctx._h, 10, p(a), p(a), 1, p(sd), p(o0), 1, None], (2, 3, 5, 6)),
        "fhe_mbfv_sks_share_dev": ([ctx._h, 10, p(a), p(a), 1, p(a), 0, p(sd), p(o0), 1, None], (2, 5, 7, 8)),
        "fhe_mbfv_pks_share_dev": ([ctx._h, 10, p(a), 1, p(a), p(a), 1, p(sd), p(o0), 1, None], (2, 4, 5, 7, 8)),
        "fhe_mbfv_rlk_round1_dev": ([ctx._h, 10, p(a), p(a), 1, p(a), p(sd), p(o0), p(o1), 1, None], (2, 3, 5, 6, 7, 8)),
        "fhe_mbfv_rlk_round2_dev": ([ctx._h, 10, p(a), p(a), 1, p(a), p(a), p(sd), p(o0), p(o1), 1, None],
                                    (2, 3, 5, 6, 7, 8, 9)),
    }
    host_ctx = fhe.Context(opar.moduli, n, device=-1)
    one_mod = fhe.Context(opar.moduli[:1], n)
    for name, (args, bufs) in calls.items():
        f = getattr(L, name)
        assert f(*args) == 0, name
        for v in (0, 33):                                     # the variance
            assert f(*(args[:1] + [v] + args[2:])) == -24, (name, v)
        assert f(*([None] + args[1:])) == -1, name            # a NULL handle
        for i in bufs:                                        # NULL buffers
            assert f(*(args[:i] + [None] + args[i + 1:])) == -1, (name, i)
        empty = [None if i in bufs else x for i, x in enumerate(args)]
        empty[-2] = 0
        assert f(*empty) == 0, name                           # batch 0: a no-op, NULL buffers allowed
        assert f(*([host_ctx._h] + args[1:])) == -18, name    # a host-only handle
    assert L.fhe_mbfv_sks_share_dev(ctx._h, 10, p(a), None, 1, p(a), 0, p(sd), p(o0), 1, None) == 0   # no output key
    for name in ("fhe_mbfv_rlk_round1_dev", "fhe_mbfv_rlk_round2_dev"):   # a single-modulus context
        assert getattr(L, name)(*([one_mod._h] + calls[name][0][1:])) == -17, name
    # the aggregations: no shares, NULL buffers, host-only handles
    agg = [ctx._h, p(a), 3, 3 * n, 1, None, p(o0), None]
    assert L.fhe_mbfv_aggregate_dev(*agg) == 0
    assert L.fhe_mbfv_aggregate_dev(*(agg[:2] + [0] + agg[3:])) == -1
    assert L.fhe_mbfv_aggregate_dev(*(agg[:3] + [3 * n + 1] + agg[4:])) == -1      # an odd stride
    for i in (0, 1, 6):
        assert L.fhe_mbfv_aggregate_dev(*(agg[:i] + [None] + agg[i + 1:])) == -1, i
    assert L.fhe_mbfv_aggregate_dev(*([host_ctx._h] + agg[1:])) == -18
    key = C.c_void_p()
    rk = [ctx._h, p(a), p(a), 1, 9 * n, p(a), None, C.byref(key)]
    assert L.fhe_mbfv_relin_key_aggregate_dev(*rk) == 0 and key.value
    L.fhe_ksk_destroy(key)
    assert L.fhe_mbfv_relin_key_aggregate_dev(*(rk[:3] + [0] + rk[4:])) == -1 and not key.value
    for i in (0, 1, 2, 5, 7):
        assert L.fhe_mbfv_relin_key_aggregate_dev(*(rk[:i] + [None] + rk[i + 1:])) == -1, i
    assert L.fhe_mbfv_relin_key_aggregate_dev(*([one_mod._h] + rk[1:])) == -17
    assert L.fhe_mbfv_relin_key_aggregate_dev(*([host_ctx._h] + rk[1:])) == -18
    out = fhe.DeviceArray((n,))
    dec = [sc._h, 1153, p(a), p(a), 1, 3 * n, p(out), 1, None]
    assert L.fhe_mbfv_decrypt_dev(*dec) == 0
    assert L.fhe_mbfv_decrypt_dev(*(dec[:4] + [0] + dec[5:])) == -1
    for i in (0, 2, 3, 6):
        assert L.fhe_mbfv_decrypt_dev(*(dec[:i] + [None] + dec[i + 1:])) == -1, i
    assert L.fhe_mbfv_decrypt_dev(sc._h, 1153, None, None, 1, 0, None, 0, None) == 0
    hpar = fhe.BfvParameters(n, 1153, moduli=opar.moduli, device=-1)
    assert L.fhe_mbfv_decrypt_dev(*([hpar.plain_scaler(0)._h] + dec[1:])) == -18
    # the Python layer: the CRP vector's length, the relin protocol's single-modulus refusal, seeds per party
    sk = fhe.SecretKey.random(par, bytes(32))
    short = fhe.CommonRandomPoly(par, np.zeros((2, 3, n), dtype=np.uint64))
    assert _code(lambda: fhe.RelinKeyGenerator(sk, short)) == -1
    opar1, par1 = arc(fhe, 1, n)
    sk1 = fhe.SecretKey.random(par1, bytes(32))
    crp1 = fhe.CommonRandomPoly(par1, np.zeros((1, 1, n), dtype=np.uint64))
    assert _code(lambda: fhe.RelinKeyGenerator(sk1, crp1)) == -17
    with pytest.raises(fhe.FheError):
        fhe.CommonRandomPoly(par, np.zeros((2, n), dtype=np.uint64))
    crp = fhe.CommonRandomPoly.from_seed(par, bytes(range(32)))
    assert np.array_equal(crp.poly, par.context_at_level(0).random_from_seed(np.arange(32, dtype=np.uint8))[0])
    with pytest.raises(fhe.FheError):
        fhe.PublicKeyShare(sk, crp, [bytes(32)] * 2)
    with pytest.raises(fhe.FheError):
        fhe.DecryptionShare(sk, np.zeros((3, 3, n), dtype=np.uint64))
    with pytest.raises(fhe.FheError):
        fhe.DecryptionShare.aggregate([])
