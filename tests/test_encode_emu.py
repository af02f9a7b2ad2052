"""Plaintext encoding on the device (fhe_encoder_create, fhe_bfv_encode_dev / decode_dev, fhe_bfv_add_plain_dev): the
kernel sources under host emulation against the test-side restatement (tests/encode_ref.py) and against functional
pins that do not depend on it (rotations, ct x pt, ct +- pt, round trips).  tests/test_encode_gpu.py runs the same
cases on the MI355X."""
import random

import numpy as np
import pytest

import encode_cases as E
import encode_ref as R
from fhe_oracle import bfv as obfv
from fhe_oracle import ntt as ontt
from fhe_oracle.zq import Modulus
from helpers import load_engine


@pytest.fixture(scope="module")
def fhe():
    return load_engine("emu")


def test_index_map():
    assert R.index_map(8) == [0, 4, 1, 5, 7, 3, 6, 2]
    assert R.index_map(16) == [0, 8, 2, 11, 1, 9, 3, 10, 15, 7, 13, 4, 14, 6, 12, 5]
    for logn in range(3, 13):
        n = 1 << logn
        assert sorted(R.index_map(n)) == list(range(n))


def test_restatement_poly_forms():
    opar = obfv.BfvParameters.default_arc(3, 16)
    rng = random.Random(2)
    for level in (0, 2):
        for nv in (0, 5, 16):
            R.check_poly_forms(opar, [rng.randrange(opar.plaintext) for _ in range(nv)], level)


# (N, t, moduli sizes): the reference's default_arc at N = 16; 50 / 40-bit moduli at 4096 put the lift and the
# transforms mod t on the F64 instances
SHAPES = [(16, 1153, [62] * 3), (1024, E.stock_t(1024), [62, 60, 55]), (4096, E.stock_t(4096), [50, 50, 40])]


@pytest.mark.parametrize("n,t,sizes", SHAPES, ids=[str(s[0]) for s in SHAPES])
def test_encode_parity(fhe, n, t, sizes):
    opar, par = E.params(fhe, n, t, moduli_sizes=sizes)
    R.check_poly_forms(opar, [3, 1, t - 1])
    E.case_parity(fhe, False, opar, par, batches=(0, 1, 5), nvalues_list=(0, 1, n // 2 + 3, n))


def test_encode_f64_off_identical(fhe):
    n = 4096
    opar, par = E.params(fhe, n, E.stock_t(n), moduli_sizes=[50, 50, 40])
    enc = par.encoder()
    v = E.values(random.Random(4), opar.plaintext, 2, n)
    on = [enc.encode(v, e, 0, s) for e in ("poly", "simd") for s in (False, True)] + [enc.decode(v, "simd")]
    fhe.set_f64(False)
    try:
        off = [enc.encode(v, e, 0, s) for e in ("poly", "simd") for s in (False, True)] + [enc.decode(v, "simd")]
    finally:
        fhe.set_f64(True)
    for a, b in zip(on, off):
        assert np.array_equal(a, b)


def test_rotations_mul_plain_roundtrip(fhe):
    opar, par = E.params(fhe, 16, 1153, moduli_sizes=[62] * 3)
    E.case_roundtrip_and_rotations(fhe, False, opar, par, level=0)
    E.case_roundtrip_and_rotations(fhe, False, opar, par, level=1)


def test_add_sub_plain(fhe):
    opar, par = E.params(fhe, 16, 1153, moduli_sizes=[62] * 3)
    E.case_add_plain(fhe, False, opar, par, level=0)
    E.case_add_plain(fhe, False, opar, par, level=1, batch=2)
    E.case_add_plain_in_place_abi(fhe, opar, par)


def _code(fn):
    with pytest.raises(Exception) as err:
        fn()
    return getattr(err.value, "code", None)


def test_errors(fhe):
    import ctypes as C
    from fhe_rs_amd import _lib
    L = _lib.lib()
    n, t = 16, 1031                      # prime, 1031 mod 32 == 7: no degree-16 NTT mod t
    opar, par = E.params(fhe, n, t, moduli_sizes=[62] * 2)
    enc = par.encoder()
    v = E.values(random.Random(9), t, 2, n)
    assert _code(lambda: enc.encode(v, "simd")) == -22
    assert _code(lambda: enc.decode(v, "simd")) == -22
    assert np.array_equal(enc.encode(v, "poly")[1], R.encode(opar, v[1], "poly"))
    assert np.array_equal(enc.encode(v, "poly", 1, True)[0], R.encode(opar, v[0], "poly", 1, True))
    opar, par = E.params(fhe, n, 1153, moduli_sizes=[62] * 3)
    enc = par.encoder()
    assert _code(lambda: enc.encode(E.values(random.Random(1), 1153, 1, n + 1), "poly")) == -23
    assert _code(lambda: enc.encode(E.values(random.Random(1), 1153, 1, n + 1), "simd")) == -23
    assert _code(lambda: enc.encode(v, "simd", 3)) == -12
    out = fhe.DeviceArray((1, 3, n))
    vals = fhe.DeviceArray.from_numpy(v)
    assert L.fhe_bfv_encode_dev(None, 1, 0, 0, C.c_void_p(vals.data_ptr()), n, C.c_void_p(out.data_ptr()), 1, None) == -1
    assert L.fhe_bfv_encode_dev(enc._h, 1, 0, 0, None, n, C.c_void_p(out.data_ptr()), 1, None) == -1
    assert L.fhe_bfv_encode_dev(enc._h, 1, 0, 0, C.c_void_p(vals.data_ptr()), n, None, 1, None) == -1
    assert L.fhe_bfv_encode_dev(enc._h, 2, 0, 0, C.c_void_p(vals.data_ptr()), n, C.c_void_p(out.data_ptr()), 1, None) == -1
    assert L.fhe_bfv_decode_dev(enc._h, 1, None, C.c_void_p(out.data_ptr()), 1, None) == -1
    assert L.fhe_bfv_add_plain_dev(None, 0, 2, None, None, 0, None, 1, None) == -1
    h = C.c_void_p()
    assert L.fhe_encoder_create(None, _lib.NTT_TABLES_FN(), None, C.byref(h)) == -1
    # batch 0: OK, nothing written, NULL buffers accepted
    assert L.fhe_bfv_encode_dev(enc._h, 1, 1, 0, None, n, None, 0, None) == 0
    assert L.fhe_bfv_decode_dev(enc._h, 1, None, None, 0, None) == 0
    assert enc.encode(np.zeros((0, n), dtype=np.uint64), "simd").shape == (0, 3, n)
    # host-only parameter set
    host = fhe.BfvParameters(n, 1153, moduli=opar.moduli, device=-1)
    assert _code(lambda: host.encoder()) == -18
    # a failing tables callback
    assert _code(lambda: par.encoder(tables_fn=lambda m, d: 1 / 0)) == -5


def test_host_tables_for_t(fhe):
    """fhe_encoder_create's callback: with psi^3 for t the SIMD encodings change, equal the restatement under that
    psi, and still round-trip; inputs >= t are reduced mod t first."""
    n, t = 16, 1153
    opar, par = E.params(fhe, n, t, moduli_sizes=[62] * 3)
    seen = []
    psi3 = pow(ontt.NttOperator(Modulus(t), n).psi, 3, t)

    def tables(modulus, degree):
        seen.append(modulus)
        op = ontt.NttOperator(Modulus(modulus), degree, psi=psi3)
        return dict(omegas=op.omegas, omegas_shoup=op.omegas_shoup, zetas_inv=op.zetas_inv,
                    zetas_inv_shoup=op.zetas_inv_shoup, size_inv=op.size_inv, size_inv_shoup=op.size_inv_shoup)

    alt, ref = par.encoder(tables_fn=tables), par.encoder()
    assert seen == [t]
    v = E.values(random.Random(12), t, 3, n)
    a, b = alt.encode(v, "simd"), ref.encode(v, "simd")
    assert not np.array_equal(a, b)
    for i in range(3):
        assert np.array_equal(a[i], R.encode(opar, v[i], "simd", psi=psi3))
        assert np.array_equal(b[i], R.encode(opar, v[i], "simd"))
    c = R.coefficients(v[0], t, n, "simd", psi=psi3)
    assert alt.decode(c[None], "simd")[0].tolist() == v[0].tolist()
    assert np.array_equal(alt.decode(v, "simd")[1], R.decode(v[1], t, n, "simd", psi=psi3))
    wide = E.values(random.Random(13), t, 2, n, wide=True)
    assert (wide >= t).any()
    for e in ("poly", "simd"):
        for s in (False, True):
            assert np.array_equal(ref.encode(wide, e, 0, s), ref.encode(wide % np.uint64(t), e, 0, s))
        assert np.array_equal(ref.decode(wide, e), ref.decode(wide % np.uint64(t), e))
