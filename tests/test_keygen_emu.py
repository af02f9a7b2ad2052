"""Key generation on the device (fhe_ksk_generate_dev, fhe_bfv_relin_key_generate_dev, fhe_bfv_galois_keys_generate_dev,
fhe_ksk_export_dev): the kernel sources under host emulation against the test-side restatement (tests/keygen_ref.py),
which is itself pinned against the reference's order of operations and against oracle decryption.
tests/test_keygen_gpu.py runs the same cases on the MI355X."""
import ctypes as C
import random

import numpy as np
import pytest

import encode_cases as E
import encrypt_cases as X
import keygen_cases as G
import keygen_ref as R
from helpers import load_engine


@pytest.fixture(scope="module")
def fhe():
    return load_engine("emu")


SMALL = dict(n=16, t=1153, moduli_sizes=[62, 60, 55])


def small(fhe, variance=10):
    return G.params(fhe, SMALL["n"], SMALL["t"], moduli_sizes=SMALL["moduli_sizes"], variance=variance)


# ---- the restatement itself -------------------------------------------------------------------------------------------
def test_restatement_order_of_operations():
    from fhe_oracle import bfv as obfv
    opar = obfv.BfvParameters(16, 1153, moduli_sizes=[62, 60, 55])
    s = R.ER.samples(bytes(range(32)), 16, opar.variance)[0]
    for cl, kl in ((0, 0), (1, 0)):
        R.check_order_of_operations(opar, s, R.relin_from(opar, s, cl, kl), bytes(range(1, 33)), cl, kl)
        R.check_order_of_operations(opar, s, R.galois_from(opar, s, 3, cl, kl), bytes(range(2, 34)), cl, kl)
    top = opar.max_level()   # single-modulus decomposition key
    R.check_order_of_operations(opar, s, R.galois_from(opar, s, 31, top, top), bytes(range(3, 35)), top, top)


def _negacyclic(a, b, t):
    n = len(a)
    out = [0] * n
    for i in range(n):
        for j in range(n):
            k = i + j
            if k < n:
                out[k] = (out[k] + a[i] * b[j]) % t
            else:
                out[k - n] = (out[k - n] - a[i] * b[j]) % t
    return out


def _substituted(a, e, t):
    n = len(a)
    out = [0] * n
    for j, v in enumerate(a):
        p = (j * e) % (2 * n)
        out[p % n] = (-v if p >= n else v) % t
    return out


def test_restatement_decrypts():
    from fhe_oracle import bfv as obfv
    opar = obfv.BfvParameters(16, 1153, moduli_sizes=[62, 60, 55])
    t = opar.plaintext
    s = R.ER.samples(bytes(range(5, 37)), 16, opar.variance)[0]
    for cl, kl in ((0, 0), (1, 0)):
        got, (a, b) = R.check_decrypts(opar, s, bytes(range(32)), cl, kl)
        assert got == _negacyclic(a, b, t), (cl, kl)
        for e in (31, 3, 9):
            got, a = R.check_decrypts(opar, s, bytes(range(1, 33)), cl, kl, exponent=e)
            assert got == _substituted(a, e, t), (cl, kl, e)


# ---- the engine against the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("cl,kl", [(0, 0), (1, 0)])
def test_relin_parity(fhe, cl, kl):
    opar, par = small(fhe)
    rk = G.case_relin(fhe, False, opar, par, cl, kl)
    G.case_same_as_host_handle(fhe, False, opar, par, rk.ksk, relin=True)


@pytest.mark.parametrize("cl,kl", [(0, 0), (1, 0), (2, 2)], ids=["00", "10", "single_modulus"])
def test_galois_parity(fhe, cl, kl):
    opar, par = small(fhe)
    n = opar.degree()
    exps = [2 * n - 1] + [pow(3, i, 2 * n) for i in (1, 2, 4)] + [(n >> l) + 1 for l in range(3)]
    gks = G.case_galois(fhe, False, opar, par, exps, cl, kl)
    assert gks[0].ksk.log_base == (0 if kl < 2 else 31)
    G.case_same_as_host_handle(fhe, False, opar, par, gks[0].ksk, exponent=gks[0].exponent)
    G.case_same_as_host_handle(fhe, False, opar, par, gks[1].ksk, exponent=gks[1].exponent)


@pytest.mark.parametrize("cl,kl", [(0, 0), (1, 0), (2, 2)], ids=["00", "10", "single_modulus"])
def test_generic_parity(fhe, cl, kl):
    opar, par = small(fhe)
    keys = G.case_generic(fhe, False, opar, par, cl, kl)
    G.case_same_as_host_handle(fhe, False, opar, par, keys[0])


@pytest.mark.parametrize("v", [1, 10, 17, 32])
def test_variances(fhe, v):
    opar, par = small(fhe, variance=v)
    G.case_relin(fhe, False, opar, par, 0, 0, seed=60 + v)
    G.case_galois(fhe, False, opar, par, [3], 0, 0, seed=70 + v)


def test_batch_larger_than_one_launch_group(fhe):
    """More keys than one launch group (KG_KEYS = 32) in one call: the groups split evenly (40 keys: 20 + 20) and the
    keys on both sides of that boundary are right, as are those around key 32."""
    import devop_cases as D
    opar, par = G.params(fhe, 8, 1153, moduli_sizes=[62, 60])
    n = 8
    exps = (list(range(1, 2 * n, 2)) * 5)[:40]   # 40 keys (exponents repeat: each key has its own seed)
    g = D.launch_group(2, n, 2, len(exps), 1 << 30, D.KG_KEYS)
    assert 1 < g < len(exps)
    G.case_galois(fhe, False, opar, par, exps, 0, 0, check={0, 31, 32, 39} | set(D.boundary_items(len(exps), g)))


def test_f64_and_4096_points(fhe):
    """n = 4096 over moduli below 2^50: the F64 transform and the F64 key words; F64 on and off give the same key,
    and the generated handle's F64 key switch equals the host-made handle's."""
    n = 4096
    opar, par = G.params(fhe, n, E.stock_t(n), moduli_sizes=[50, 50, 40])
    rk = G.case_relin(fhe, False, opar, par, 0, 0)
    sk, _ = G.secret(fhe, opar, par, 21)
    sd = bytes(X.seeds(random.Random(22), 1)[0])   # (case_relin's seed)
    fhe.set_f64(False)
    try:
        off = fhe.RelinearizationKey.generate(sk, sd)
    finally:
        fhe.set_f64(True)
    for a, b in zip(G.exported(fhe, rk.ksk), G.exported(fhe, off.ksk)):
        assert np.array_equal(a, b)
    G.case_same_as_host_handle(fhe, False, opar, par, rk.ksk, relin=True)


def test_rows_larger_than_lds(fhe):
    """N = 32768: the element-wise passes around launch_ntt."""
    n = 32768
    opar, par = G.params(fhe, n, E.stock_t(n), moduli_sizes=[50, 55])
    G.case_galois(fhe, False, opar, par, [2 * n - 1], 0, 0)


def test_evaluation_key_index_set(fhe):
    opar, par = small(fhe)
    n = opar.degree()
    assert fhe.EvaluationKey.exponents(n, inner_sum=True) == sorted({2 * n - 1, 3, 9, 81 % (2 * n)})
    assert fhe.EvaluationKey.exponents(n, expansion_level=2) == [n // 2 + 1, n + 1]
    assert fhe.EvaluationKey.exponents(n, column_rotations=[1], row_rotation=True) == [3, 2 * n - 1]
    sk, _ = G.secret(fhe, opar, par, 3)
    ek = fhe.EvaluationKey.generate(sk, inner_sum=True, row_rotation=True, expansion_level=4)
    assert sorted(ek.gk) == fhe.EvaluationKey.exponents(n, inner_sum=True, expansion_level=4)
    assert ek.supports_expansion(4)
    with pytest.raises(fhe.FheError):
        fhe.EvaluationKey.exponents(n, column_rotations=[n // 2])
    with pytest.raises(fhe.FheError):
        fhe.EvaluationKey.exponents(n, expansion_level=5)


def test_errors(fhe):
    from fhe_rs_amd import _lib
    L = _lib.lib()
    opar, par = small(fhe)
    n = opar.degree()
    c0, c1, c2 = (par.context_at_level(i) for i in range(3))
    sk = fhe.SecretKey.random(par, bytes(32))
    s = C.c_void_p(sk.s_ntt.data_ptr())
    sd = fhe.DeviceArray.from_numpy(np.zeros((2, 32), dtype=np.uint8))
    frm = fhe.DeviceArray.from_numpy(np.zeros((2, 3, n), dtype=np.uint64))
    p = lambda a: C.c_void_p(a.data_ptr())   # noqa: E731
    hs = (C.c_void_p * 2)()
    exps = (C.c_size_t * 2)(3, 5)
    even = (C.c_size_t * 2)(3, 4)
    gen = lambda ct, kc, v, *a: L.fhe_ksk_generate_dev(ct._h, kc._h, v, *a)   # noqa: E731
    for v in (0, 33):
        assert gen(c0, c0, v, s, p(frm), p(sd), 2, None, None, hs) == -24
        assert L.fhe_bfv_relin_key_generate_dev(c0._h, c0._h, v, s, p(sd), None, None, hs) == -24
        assert L.fhe_bfv_galois_keys_generate_dev(c0._h, c0._h, v, s, exps, p(sd), 2, None, None, hs) == -24
    # relinearization over a single-modulus key context
    assert L.fhe_bfv_relin_key_generate_dev(c2._h, c2._h, 10, s, p(sd), None, None, hs) == -17
    with pytest.raises(fhe.FheError) as err:
        fhe.RelinearizationKey.generate(sk, bytes(32), 2, 2)
    assert err.value.code == -17
    # even exponent
    assert L.fhe_bfv_galois_keys_generate_dev(c0._h, c0._h, 10, s, even, p(sd), 2, None, None, hs) == -10
    assert list(hs) == [None, None]
    # key level above the ciphertext level
    assert gen(c0, c1, 10, s, p(frm), p(sd), 2, None, None, hs) == -9
    assert L.fhe_bfv_relin_key_generate_dev(c0._h, c1._h, 10, s, p(sd), None, None, hs) == -9
    assert L.fhe_bfv_galois_keys_generate_dev(c0._h, c1._h, 10, s, exps, p(sd), 2, None, None, hs) == -9
    # NULL handles and buffers
    assert L.fhe_ksk_generate_dev(None, c0._h, 10, s, p(frm), p(sd), 2, None, None, hs) == -1
    assert L.fhe_ksk_generate_dev(c0._h, None, 10, s, p(frm), p(sd), 2, None, None, hs) == -1
    assert gen(c0, c0, 10, None, p(frm), p(sd), 2, None, None, hs) == -1
    assert gen(c0, c0, 10, s, None, p(sd), 2, None, None, hs) == -1
    assert gen(c0, c0, 10, s, p(frm), None, 2, None, None, hs) == -1
    assert gen(c0, c0, 10, s, p(frm), p(sd), 2, None, None, None) == -1
    assert L.fhe_bfv_relin_key_generate_dev(c0._h, c0._h, 10, None, p(sd), None, None, hs) == -1
    assert L.fhe_bfv_relin_key_generate_dev(c0._h, c0._h, 10, s, None, None, None, hs) == -1
    assert L.fhe_bfv_relin_key_generate_dev(c0._h, c0._h, 10, s, p(sd), None, None, None) == -1
    assert L.fhe_bfv_galois_keys_generate_dev(c0._h, c0._h, 10, s, None, p(sd), 2, None, None, hs) == -1
    assert L.fhe_bfv_galois_keys_generate_dev(c0._h, c0._h, 10, None, exps, p(sd), 2, None, None, hs) == -1
    assert L.fhe_bfv_galois_keys_generate_dev(c0._h, c0._h, 10, s, exps, None, 2, None, None, hs) == -1
    assert L.fhe_ksk_export_dev(None, p(frm), p(frm), None, None, None) == -1
    # nkeys == 0: a no-op, NULL buffers accepted
    assert gen(c0, c0, 10, None, None, None, 0, None, None, None) == 0
    assert L.fhe_bfv_galois_keys_generate_dev(c0._h, c0._h, 10, None, None, None, 0, None, None, None) == 0
    # a host-only context
    host = fhe.Context(opar.moduli, n, device=-1)
    assert L.fhe_ksk_generate_dev(host._h, host._h, 10, s, p(frm), p(sd), 2, None, None, hs) == -18
    # the Python layer: one seed per key
    with pytest.raises(fhe.FheError):
        fhe.GaloisKey.generate(sk, [3, 5], [bytes(32)])
