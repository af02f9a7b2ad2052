"""Key generation on the MI355X (the HIP build): the parity cases of tests/test_keygen_emu.py on every stock set of
tests/ref_params.py and on N = 32768 (rows larger than one LDS tile), F64 on versus off, one batched
EvaluationKey.generate, a PIR chain with no host key generation and the frozen digests of
tests/golden/keygen_default128_digest.json."""
import json
import os
import random
import sys

import numpy as np
import pytest

import encode_cases as E
import encrypt_cases as X
import keygen_cases as G
import ref_params
from helpers import HIP_LIB, Xfer, load_engine

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fhe():
    eng = load_engine("hip")
    from fhe_rs_amd import _lib
    assert _lib.loaded_path() == HIP_LIB, "GPU tests must run on the HIP build"
    assert eng.device_count() >= 1, "no HIP device visible"
    return eng


def stock(fhe, n):
    return G.params(fhe, n, ref_params.plaintext_modulus(n), moduli=ref_params.DEFAULT_128[n])


@pytest.fixture
def some_digits(request):
    """At n = 16384 (9 x 9 digit rows) the restatement checks digits 0, 7 and 8 only (those that exist)."""
    G.ONLY = None
    yield lambda n: setattr(G, "ONLY", {0, 7, 8} if n >= 16384 else None)
    G.ONLY = None


@pytest.mark.parametrize("n", sorted(ref_params.DEFAULT_128))
def test_parity_stock(fhe, n, some_digits):
    some_digits(n)
    opar, par = stock(fhe, n)
    top = opar.max_level()
    exps = [2 * n - 1, 3, n + 1]
    if top == 0:   # one modulus: decomposition keys only; relinearization is KeySwitchingNotSupported
        gks = G.case_galois(fhe, True, opar, par, exps, 0, 0)
        assert gks[0].ksk.log_base > 0
        G.case_same_as_host_handle(fhe, True, opar, par, gks[0].ksk, exponent=gks[0].exponent)
        return
    rk = G.case_relin(fhe, True, opar, par, 0, 0)
    G.case_same_as_host_handle(fhe, True, opar, par, rk.ksk, relin=True)
    G.case_relin(fhe, True, opar, par, 1, 0)
    gks = G.case_galois(fhe, True, opar, par, exps, 0, 0)
    G.case_same_as_host_handle(fhe, True, opar, par, gks[1].ksk, exponent=gks[1].exponent)
    G.case_galois(fhe, True, opar, par, [5], top, top)   # single-modulus decomposition key at the last level
    G.case_generic(fhe, True, opar, par, 0, 0, nkeys=1)


def test_parity_rows_larger_than_lds(fhe):
    n = 32768
    opar, par = G.params(fhe, n, E.stock_t(n), moduli_sizes=[50, 55, 60])
    G.case_relin(fhe, "abi", opar, par, 0, 0)
    G.case_galois(fhe, "abi", opar, par, [3], 0, 0)


@pytest.mark.parametrize("n", [4096, 8192, 16384])
def test_f64_on_off_identical(fhe, n):
    opar, par = stock(fhe, n)
    sk, _ = G.secret(fhe, opar, par, 5)
    sd = X.seeds(random.Random(n), 3)

    def run():
        keys = [fhe.RelinearizationKey.generate(sk, bytes(sd[0])).ksk]
        keys += [g.ksk for g in fhe.GaloisKey.generate(sk, [3, 2 * n - 1], sd[1:])]
        return [G.exported(fhe, k) for k in keys]
    on = run()
    fhe.set_f64(False)
    try:
        off = run()
    finally:
        fhe.set_f64(True)
    for a, b in zip(on, off):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_evaluation_key_batched(fhe):
    """One EvaluationKey.generate of the PIR set at stock n = 8192 (expansion level log2 N, inner sum, row rotation):
    one batched call; the first and last keys against the restatement."""
    n = 8192
    opar, par = stock(fhe, n)
    sk, s = G.secret(fhe, opar, par, 9)
    exps = fhe.EvaluationKey.exponents(n, row_rotation=True, inner_sum=True, expansion_level=13)
    sd = X.seeds(random.Random(10), len(exps))
    ek = fhe.EvaluationKey.generate(sk, row_rotation=True, inner_sum=True, expansion_level=13, seeds=sd)
    assert sorted(ek.gk) == exps
    assert ek.supports_expansion(13)
    import keygen_ref as R
    for b in (0, len(exps) - 1):
        e = exps[b]
        G.check_key(fhe, ek.gk[e].ksk, opar, 0, 0, s, R.galois_from(opar, s, e, 0, 0), sd[b], ("ek", e))


def test_pir_chain_no_host_key_generation(fhe):
    """SecretKey.random -> RelinearizationKey.generate / EvaluationKey.generate -> pk-encrypt -> dot product ->
    multiply-relinearize -> inner sum -> decrypt -> decode, at stock n = 8192, every key and ciphertext made on the
    device: every slot holds the sum over the slots of (sum_k q_k db_k) * w."""
    n = 8192
    opar, par = stock(fhe, n)
    t = opar.plaintext
    rng = random.Random(83)
    x = Xfer("abi")
    enc = par.encoder()
    ctx = par.context_at_level(0)
    count = 3
    db, q, w = E.values(rng, t, count, n), E.values(rng, t, count, n), E.values(rng, t, 1, n)
    with fhe.Stream(0):
        sk = fhe.SecretKey.random(par)
        rk = fhe.RelinearizationKey.generate(sk)
        ek = fhe.EvaluationKey.generate(sk, inner_sum=True)
        pk = fhe.PublicKey(sk)
        pts = enc.encode(x.to(db), "simd")
        qcts = pk.encrypt(enc.encode(x.to(q), "simd", 0, scaled=True))
        wct = pk.encrypt(enc.encode(x.to(w), "simd", 0, scaled=True))
        acc = ctx.dot_product_scalar(qcts, pts).reshape(1, 2, len(opar.moduli), n)
        prod = fhe.Multiplicator.default(par, rk, 0).multiply(acc, wct)
        summed = ek.computes_inner_sum(prod)
        got = x.back(enc.decode(sk.decrypt(summed, 0), "simd"))[0]
    want = np.zeros(n, dtype=object)
    for k in range(count):
        want = (want + q[k].astype(object) * db[k].astype(object)) % t
    total = int(((want * w[0].astype(object)) % t).sum() % t)
    assert got.tolist() == [total] * n


def test_golden_digests(fhe):
    sys.path.insert(0, GOLDEN)
    import make_keygen_golden as KG
    import make_encode_golden as EG
    with open(os.path.join(GOLDEN, "keygen_default128_digest.json")) as f:
        gold = json.load(f)
    opar, par = stock(fhe, KG.N)
    assert gold["t"] == opar.plaintext and gold["moduli"] == opar.moduli and gold["variance"] == par.variance
    sk = fhe.SecretKey.random(par, KG.seed(KG.SK))
    rk = fhe.RelinearizationKey.generate(sk, KG.seed(KG.RK)).ksk
    gk = fhe.GaloisKey.generate(sk, [gold["exponent"]], [KG.seed(KG.GK)])[0].ksk
    for name, k in (("rk", rk), ("gk", gk)):
        c0, c1, _, _ = G.exported(fhe, k)
        assert EG.sha(c0) == gold[name]["c0"], name
        assert EG.sha(c1) == gold[name]["c1"], name
        assert k.seed.hex() == gold[name]["seed"], name
