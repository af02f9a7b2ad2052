"""Cases of the key-generation entry points (fhe_ksk_generate_dev, fhe_bfv_relin_key_generate_dev,
fhe_bfv_galois_keys_generate_dev, fhe_ksk_export_dev) and their Python wrappers, shared by tests/test_keygen_emu.py
(kernel sources under host emulation) and tests/test_keygen_gpu.py (the HIP build).  `dev`: as helpers.Xfer."""
import random

import numpy as np

import encrypt_cases as X
import keygen_ref as R
from fhe_oracle import bfv as obfv
from helpers import Xfer

_opar = {}


def params(fhe, n, t, moduli=None, moduli_sizes=None, variance=10):
    key = (n, t, tuple(moduli or ()), tuple(moduli_sizes or ()), variance)
    if key not in _opar:
        _opar[key] = obfv.BfvParameters(n, t, moduli=moduli, moduli_sizes=moduli_sizes, variance=variance)
    opar = _opar[key]
    return opar, fhe.BfvParameters(n, t, moduli=opar.moduli, variance=variance)


def secret(fhe, opar, par, seed):
    """(engine SecretKey, its coefficients) from one 32-byte seed."""
    sd = bytes(X.seeds(random.Random(seed), 1)[0])
    return fhe.SecretKey.random(par, sd), R.ER.samples(sd, opar.degree(), opar.variance)[0]


def exported(fhe, key):
    return [X._host(fhe, a) for a in key.export()]


ONLY = None   # the digits check_key compares (None: all); the GPU suite narrows it at n = 16384


def check_key(fhe, key, opar, cl, kl, s_coeffs, from_ntt, seed, what):
    c0, c1, c0s, c1s = exported(fhe, key)
    w0, w1, K = R.ksk(opar.ctx[cl], opar.ctx[kl], opar.variance, s_coeffs, from_ntt, seed, ONLY)
    if ONLY is not None:
        sel = sorted(d for d in ONLY if d < len(c0))
        c0, c1, c0s, c1s, w0, w1 = (a[sel] for a in (c0, c1, c0s, c1s, w0, w1))
    assert c1.shape == w1.shape, (what, c1.shape, w1.shape)
    assert np.array_equal(c1, w1), what
    assert np.array_equal(c0, w0), what
    assert key.seed == K, what
    kc = opar.ctx[kl]
    assert np.array_equal(c0s, np.array([R.shoup(p, kc) for p in w0])), what
    assert np.array_equal(c1s, np.array([R.shoup(p, kc) for p in w1])), what


def case_relin(fhe, dev, opar, par, cl, kl, seed=21):
    x = Xfer(dev)
    sk, s = secret(fhe, opar, par, seed)
    sd = X.seeds(random.Random(seed + 1), 1)
    rk = fhe.RelinearizationKey.generate(sk, x.to_bytes(sd[0]), cl, kl)
    check_key(fhe, rk.ksk, opar, cl, kl, s, R.relin_from(opar, s, cl, kl), sd[0], ("relin", cl, kl))
    return rk


def case_galois(fhe, dev, opar, par, exps, cl, kl, seed=31, check=None):
    x = Xfer(dev)
    sk, s = secret(fhe, opar, par, seed)
    sd = X.seeds(random.Random(seed + 1), len(exps))
    gks = fhe.GaloisKey.generate(sk, exps, x.to_bytes(sd), cl, kl)
    assert [g.exponent for g in gks] == [e % (2 * opar.degree()) for e in exps]
    for b, (g, e) in enumerate(zip(gks, exps)):
        if check is None or b in check:
            check_key(fhe, g.ksk, opar, cl, kl, s, R.galois_from(opar, s, e, cl, kl), sd[b], ("galois", e, cl, kl))
    return gks


def case_generic(fhe, dev, opar, par, cl, kl, nkeys=2, seed=41):
    """KeySwitchingKey.generate of uniformly random `from` polynomials."""
    x = Xfer(dev)
    rng = random.Random(seed)
    sk, s = secret(fhe, opar, par, seed)
    kc = opar.ctx[kl]
    frm = np.array([[[rng.randrange(q) for _ in range(kc.degree)] for q in kc.moduli] for _ in range(nkeys)],
                   dtype=np.uint64)
    sd = X.seeds(rng, nkeys)
    keys = fhe.KeySwitchingKey.generate(sk, x.to(frm), cl, kl, x.to_bytes(sd))
    assert len(keys) == nkeys
    for b in range(nkeys):
        check_key(fhe, keys[b], opar, cl, kl, s, frm[b], sd[b], ("generic", b))
    return keys


def host_twin(fhe, key):
    """The same key made by fhe_ksk_create from the exported arrays (host path)."""
    c0, c1, c0s, c1s = exported(fhe, key)
    return fhe.KeySwitchingKey(key.ctx_ciphertext, key.ctx_ksk, c0, c1, c0s, c1s, key.log_base)


def case_same_as_host_handle(fhe, dev, opar, par, key, exponent=None, relin=False, seed=51):
    """A generated handle and fhe_ksk_create of its exported arrays give identical key switches, relinearizations and
    rotations in AUTO, FUSED and UNFUSED modes."""
    x = Xfer(dev)
    rng = random.Random(seed)
    twin = host_twin(fhe, key)
    ct = key.ctx_ciphertext
    L, n = ct.nmoduli, ct.degree
    p = np.array([[rng.randrange(q) for _ in range(n)] for q in ct.moduli], dtype=np.uint64)[None]
    cts = np.array([[[rng.randrange(q) for _ in range(n)] for q in ct.moduli] for _ in range(3)], dtype=np.uint64)
    for mode in (fhe.KeySwitchingKey.AUTO, fhe.KeySwitchingKey.FUSED, fhe.KeySwitchingKey.UNFUSED):
        if mode == fhe.KeySwitchingKey.UNFUSED and key.log_base:
            continue
        outs = []
        for k in (key, twin):
            k.set_mode(mode)
            r = [x.back(v) for v in k.key_switch(x.to(p))]
            if relin:
                r.append(x.back(fhe.RelinearizationKey(k).relinearizes(x.to(cts[None]))))
            if exponent is not None:
                r.append(x.back(fhe.GaloisKey(k, exponent).relinearize(x.to(cts[None, :2]))))
            outs.append(r)
        for a, b in zip(*outs):
            assert np.array_equal(a, b), mode
        key.set_mode(fhe.KeySwitchingKey.AUTO)
