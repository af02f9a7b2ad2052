"""Cases of the encryption entry points (fhe_bfv_sample_small_dev, fhe_bfv_encrypt_sk_dev, fhe_bfv_encrypt_pk_dev)
and their Python wrappers, shared by tests/test_encrypt_emu.py (kernel sources under host emulation) and
tests/test_encrypt_gpu.py (the HIP build).  `dev`: as helpers.Xfer -- False (numpy in, numpy out), True (torch
tensors) or "abi" (DeviceArrays)."""
import random

import numpy as np

import encode_cases as E
import encode_ref as ER
import encrypt_ref as R
from fhe_oracle import bfv as obfv
from fhe_oracle.rq import Poly, NTT
from helpers import Xfer


def seeds(rng, count):
    return np.frombuffer(bytes(rng.getrandbits(8) for _ in range(32 * count)), dtype=np.uint8).reshape(count, 32).copy()


def signed(rows, ctx):
    """[L][N] residues of small integers -> the integers (row 0), checking every row holds the same one."""
    q = np.array(ctx.moduli, dtype=object)[:, None]
    r = np.asarray(rows).astype(object)
    x = np.where(r > q // 2, r - q, r)
    assert all((x[i] == x[0]).all() for i in range(1, len(ctx.moduli)))
    return x[0].astype(np.int64)


def case_sampler_parity(fhe, dev, opar, par, variances, batch=2, seed=1):
    """Poly::small, PowerBasis and Ntt, against the restatement for every variance, at level 0 and the top level."""
    x = Xfer(dev)
    rng = random.Random(seed)
    for level in sorted({0, opar.max_level()}):
        ctx, octx = par.context_at_level(level), opar.ctx[level]
        for v in variances:
            sd = seeds(rng, batch)
            for ntt in (False, True):
                got = x.back(ctx.sample_small(x.to_bytes(sd), v, ntt))
                assert got.shape == (batch, len(octx.moduli), opar.degree())
                for b in range(batch):
                    assert np.array_equal(got[b], R.small(octx, v, sd[b], ntt)), (v, ntt, level, b)


def case_sampler_consistency(fhe, dev, par, v, total=1 << 20, seed=2):
    """Without the restatement: every row holds the same small integer, |x| <= 2v, and over `total` samples the mean
    is about 0 and the variance about v (the centered binomial of 4v coins)."""
    x = Xfer(dev)
    ctx = par.context_at_level(0)
    n = par.degree
    batch = max(1, total // n)
    sd = seeds(random.Random(seed + v), batch)
    got = x.back(ctx.sample_small(x.to_bytes(sd), v, False))
    octx = type("C", (), {"moduli": par.moduli})
    xs = np.concatenate([signed(got[b], octx) for b in range(batch)])
    assert np.abs(xs).max() <= 2 * v
    mean, var = xs.mean(), xs.var()
    sd_mean = (v / xs.size) ** 0.5
    assert abs(mean) < 6 * sd_mean, (v, mean)
    assert abs(var - v) < 0.02 * v + 6 * v * (2.0 / xs.size) ** 0.5, (v, var)


def keys(fhe, opar, par, seed=5):
    """(engine SecretKey, its restated oracle SecretKey, s_ntt on the host)."""
    sk_seed = bytes(random.Random(seed).getrandbits(8) for _ in range(32))
    sk = fhe.SecretKey.random(par, sk_seed)
    s_host = sk.s_ntt.download() if isinstance(sk.s_ntt, fhe.DeviceArray) else sk.s_ntt.cpu().numpy().view(np.uint64)
    return sk, R.secret_key(opar, sk_seed), s_host


def case_encrypt_parity(fhe, dev, opar, par, levels=None, batch=3, check_items=None, seed=7,
                        modes=("each", "shared", "none")):
    """SecretKey.random, SecretKey.encrypt and PublicKey / PublicKey.encrypt against the restatement, bit for bit:
    pt given per item, shared, and None (the zero plaintext); c1 of the secret-key form equals fhe_poly_from_seed for
    the whole batch.  check_items(batch) -> item indices compared (default: all)."""
    x = Xfer(dev)
    rng = random.Random(seed)
    n, t, v = opar.degree(), opar.plaintext, opar.variance
    sk, osk, s_host = keys(fhe, opar, par, seed)
    assert np.array_equal(s_host, R.small(opar.ctx[0], v, bytes(random.Random(seed).getrandbits(8) for _ in range(32))))
    pk_seeds = seeds(rng, 2)
    pk = fhe.PublicKey(sk, bytes(pk_seeds[0]), bytes(pk_seeds[1]))
    pk0 = R.encrypt_sk(opar.ctx[0], v, s_host, pk_seeds[0], pk_seeds[1])
    assert np.array_equal(_host(fhe, pk.c), pk0)
    enc = par.encoder()
    items = range(batch) if check_items is None else check_items(batch)
    for level in (sorted({0, opar.max_level()}) if levels is None else levels):
        octx = opar.ctx[level]
        L = len(octx.moduli)
        s_l = s_host[:L]
        pk_l = _host(fhe, pk.at_level(level))
        if level and n <= 1024:   # (the pure-Python switch: small sets only)
            switched = [Poly(opar.ctx[0], NTT, [[int(w) for w in r] for r in pk0[i]]) for i in range(2)]
            oct_ = obfv.Ciphertext(opar, switched, 0)
            oct_.switch_to_level(level)
            assert pk_l.tolist() == [p.coefficients for p in oct_.c]
        vals = E.values(rng, t, batch, n)
        pts = x.back(enc.encode(x.to(vals), "simd", level, True))
        for mode in modes:
            a_sd, e_sd, p_sd = seeds(rng, batch), seeds(rng, batch), seeds(rng, batch)
            if mode == "each":
                pt_in, pt_of = x.to(pts), (lambda b: pts[b])
            elif mode == "shared":
                pt_in, pt_of = x.to(pts[0]), (lambda b: pts[0])
            else:
                pt_in, pt_of = None, (lambda b: None)
            cs = x.back(sk.encrypt(pt_in, level, x.to_bytes(a_sd), x.to_bytes(e_sd)))
            cp = x.back(pk.encrypt(pt_in, level, x.to_bytes(p_sd)))
            if mode == "shared" and batch == 1:   # (one shared plaintext and one seed: no batch dimension)
                cs, cp = cs[None], cp[None]
            assert cs.shape == cp.shape == (batch, 2, L, n), (cs.shape, mode)
            c1 = x.back(par.context_at_level(level).random_from_seed(x.to_bytes(a_sd)))
            assert np.array_equal(cs[:, 1], c1)
            for b in items:
                assert np.array_equal(cs[b], R.encrypt_sk(octx, v, s_l, a_sd[b], e_sd[b], pt_of(b))), (level, mode, b)
                assert np.array_equal(cp[b], R.encrypt_pk(octx, v, pk_l, p_sd[b], pt_of(b))), (level, mode, b)


def _host(fhe, a):
    if isinstance(a, np.ndarray):
        return a
    return a.download() if isinstance(a, fhe.DeviceArray) else a.cpu().numpy().view(np.uint64)


def case_roundtrip(fhe, dev, opar, par, level=0, batch=2, seed=11):
    """Pins that do not depend on the restatement: SIMD-encode -> encrypt (sk and pk) -> the engine's decrypt ->
    decode is the identity; the oracle's SecretKey.decrypt of the engine's ciphertexts agrees, and their fresh noise
    is within the bound of the errors drawn (sk: |e| <= 2v; pk: |u e + e1 + e2 s| <= 2N (2v)^2 + 2v)."""
    x = Xfer(dev)
    rng = random.Random(seed)
    n, t, v = opar.degree(), opar.plaintext, opar.variance
    sk, osk, s_host = keys(fhe, opar, par, seed)
    pk = fhe.PublicKey(sk)
    enc = par.encoder()
    vals = E.values(rng, t, batch, n)
    pts = enc.encode(x.to(vals), "simd", level, True)
    L = len(opar.ctx[level].moduli)
    for ct in (sk.encrypt(pts, level), pk.encrypt(pts, level)):
        assert tuple(ct.shape) == (batch, 2, L, n)
        dec = x.back(enc.decode(sk.decrypt(ct, level), "simd"))
        assert np.array_equal(dec, vals)
    cts = {"sk": x.back(sk.encrypt(pts, level)), "pk": x.back(pk.encrypt(pts, level))}
    bound = {"sk": (2 * v).bit_length() + 1, "pk": (2 * n * (2 * v) ** 2 + 2 * v).bit_length() + 1}
    for kind, ct in cts.items():
        for b in range(batch):
            oct_ = obfv.Ciphertext(opar, [Poly(opar.ctx[level], NTT, [[int(w) for w in r] for r in ct[b][i]])
                                          for i in range(2)], level)
            coeffs = ER.coefficients(vals[b], t, n, "simd")
            assert osk.decrypt(oct_) == [int(c) for c in coeffs], kind
            assert osk.measure_noise(oct_, [int(c) for c in coeffs]) <= bound[kind], kind
