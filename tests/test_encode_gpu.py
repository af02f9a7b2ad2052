"""Plaintext encoding on the MI355X (the HIP build): the parity cases of tests/test_encode_emu.py on every stock set of
tests/ref_params.py and on N = 32768 (rows larger than one LDS tile: the gather-pass path), F64 on versus off, a
PIR-shaped chain entirely on the device, the rotation pin at stock n = 4096, and the frozen digests of
tests/golden/encode_default128_digest.json."""
import json
import os
import random

import numpy as np
import pytest

import encode_cases as E
import encode_ref as R
import ref_params
from fhe_oracle import bfv as obfv
from fhe_oracle.rq import Poly, NTT
from helpers import HIP_LIB, Xfer, arr, ct_arr, load_engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fhe():
    eng = load_engine("hip")
    from fhe_rs_amd import _lib
    assert _lib.loaded_path() == HIP_LIB, "GPU tests must run on the HIP build"
    assert eng.device_count() >= 1, "no HIP device visible"
    return eng


def stock(fhe, n):
    return E.params(fhe, n, ref_params.plaintext_modulus(n), moduli=ref_params.DEFAULT_128[n])


def _sample(batch):
    return sorted({0, batch // 2, batch - 1}) if batch else []


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("n", sorted(ref_params.DEFAULT_128))
def test_parity_stock(fhe, n, dev):
    opar, par = stock(fhe, n)
    E.case_parity(fhe, dev, opar, par, batches=(1, 7), nvalues_list=(n // 2 + 3, n), check_items=_sample)
    # (a batch of 1024 at the deepest level: one row per item keeps the downloaded arrays small)
    E.case_parity(fhe, dev, opar, par, batches=(1024,), nvalues_list=(n,), levels=(opar.max_level(),), check_items=_sample,
                  seed=2)


def test_parity_rows_larger_than_lds(fhe):
    n = 32768
    opar, par = E.params(fhe, n, E.stock_t(n), moduli_sizes=[50, 55, 60])
    E.case_parity(fhe, "abi", opar, par, batches=(1, 7), nvalues_list=(1, n), check_items=_sample)


@pytest.mark.parametrize("n", sorted(ref_params.DEFAULT_128))
def test_f64_on_off_identical(fhe, n):
    opar, par = stock(fhe, n)
    enc = par.encoder()
    v = E.values(random.Random(n), opar.plaintext, 7, n)

    def run():
        return [enc.encode(v, e, lv, s) for e in ("poly", "simd") for s in (False, True) for lv in (0, opar.max_level())] \
            + [enc.decode(v, "simd"), enc.decode(v, "poly")]

    assert fhe.get_f64()
    on = run()
    fhe.set_f64(False)
    try:
        off = run()
    finally:
        fhe.set_f64(True)
    for a, b in zip(on, off):
        assert np.array_equal(a, b)


def test_pir_chain_on_device(fhe):
    """SIMD-encode a database -> dot_product_scalar_dev with encrypted selection vectors -> decrypt_dev -> decode_dev,
    every step on device buffers (DeviceArrays on the ABI's allocator), stock n = 8192; the result is the plaintext
    computation sum_k q_k * db_k slot by slot."""
    n = 8192
    opar, par = stock(fhe, n)
    t = opar.plaintext
    rng = random.Random(81)
    x = Xfer("abi")
    enc = par.encoder()
    ctx = par.context_at_level(0)
    sk = obfv.SecretKey.random(opar, rng)
    count = 3
    db = E.values(rng, t, count, n)
    q = E.values(rng, t, count, n)
    with fhe.Stream(0):
        pts = enc.encode(x.to(db), "simd")                                      # [count][L][N] poly_ntt, on the device
        qpt = x.back(enc.encode(x.to(q), "simd", 0, scaled=True))
        cts = np.stack([ct_arr(sk.encrypt_poly(Poly(opar.ctx[0], NTT, [[int(w) for w in r] for r in qpt[k]]), rng))
                        for k in range(count)])
        acc = ctx.dot_product_scalar(x.to(cts), pts)                             # [2][L][N]
        d = par.decrypt(x.to(arr(sk._s(opar.ctx[0]))), acc.reshape(1, 2, len(opar.moduli), n), 0)
        got = x.back(enc.decode(d, "simd"))[0]
    want = np.zeros(n, dtype=object)
    for k in range(count):
        want = (want + q[k].astype(object) * db[k].astype(object)) % t
    assert got.tolist() == [int(w) for w in want]


def test_rotation_pin_stock_4096(fhe):
    opar, par = stock(fhe, 4096)
    E.case_roundtrip_and_rotations(fhe, True, opar, par, level=0)


def test_add_plain_stock(fhe):
    opar, par = stock(fhe, 4096)
    E.case_add_plain(fhe, True, opar, par, level=0, batch=2)
    E.case_add_plain_in_place_abi(fhe, opar, par)


def test_golden_digests(fhe):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_encode_golden as G
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encode_default128_digest.json")) as f:
        gold = json.load(f)
    opar, par = stock(fhe, G.N)
    assert gold["t"] == opar.plaintext and gold["moduli"] == opar.moduli
    v = G.golden_values(opar.plaintext)
    enc = par.encoder()
    assert G.sha(enc.encode(v, "simd", 0)) == gold["simd"]
    assert G.sha(enc.encode(v, "simd", 0, scaled=True)) == gold["simd_scaled"]
