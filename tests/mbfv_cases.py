"""Cases of the multiparty BFV entry points (fhe_mbfv_*_dev) and their Python classes, shared by
tests/test_mbfv_emu.py (kernel sources under host emulation) and tests/test_mbfv_gpu.py (the HIP build).  `dev`: False
(numpy public inputs in, numpy out; secrets in DeviceArrays) or True (torch tensors throughout)."""
import random

import numpy as np

import encode_cases as E
import encrypt_cases as X
import encrypt_ref as R
import mbfv_ref as MR
from helpers import Xfer


def dev_arr(fhe, x, a):
    """A device array of `a` whatever `dev` is: secrets live on the device."""
    return x.to(a) if x.dev else fhe.DeviceArray.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint64)))


def host(fhe, a):
    return X._host(fhe, a)


def uniform(g, moduli, n, lead=()):
    """Uniform canonical residues [lead..., L, N]."""
    rows = [g.integers(0, int(q) - 1, size=tuple(lead) + (n,), dtype=np.uint64, endpoint=True) for q in moduli]
    return np.ascontiguousarray(np.stack(rows, axis=-2))


def secrets_of(fhe, x, opar, par, rng, count):
    """`count` parties' SecretKey::random draws: (SecretKey holding [count, L, N], the host copy, the seeds)."""
    sd = X.seeds(rng, count)
    s = np.stack([R.small(opar.ctx[0], opar.variance, sd[p]) for p in range(count)])
    return fhe.SecretKey(par, dev_arr(fhe, x, s)), s, sd


def one(fhe, x, par, s_host, p=0):
    return fhe.SecretKey(par, dev_arr(fhe, x, s_host[p]))


def case_share_parity(fhe, dev, opar, par, parties=3, cts=2, levels=None, rlk=True, seed=1):
    """Every share of the table -- public key, secret-key switch, decryption, public-key switch, both relin rounds --
    and every aggregation against the restatement, bit for bit: P parties in one call (a secret per item), one party
    with a batch of ciphertexts (one secret shared), and both at once."""
    x = Xfer(dev)
    rng = random.Random(seed)
    g = np.random.default_rng(seed)
    n, v = opar.degree(), opar.variance
    P = parties
    sk, s, _ = secrets_of(fhe, x, opar, par, rng, P)
    sk_out, s_out, _ = secrets_of(fhe, x, opar, par, rng, P)
    octx0 = opar.ctx[0]

    # PublicKeyShare::new and PublicKey::from_shares
    crp = uniform(g, octx0.moduli, n)
    sd = X.seeds(rng, P)
    shares = fhe.PublicKeyShare(sk, fhe.CommonRandomPoly(par, x.to(crp)), x.to_bytes(sd))
    got = x.back(shares.p0_share)
    want = [MR.pk_share(octx0, v, crp, s[p], sd[p]) for p in range(P)]
    assert got.shape == (P, len(octx0.moduli), n)
    for p in range(P):
        assert np.array_equal(got[p], want[p]), ("pk share", p)
    single = fhe.PublicKeyShare(one(fhe, x, par, s), fhe.CommonRandomPoly(par, x.to(crp)), x.to_bytes(sd[:1]))
    assert np.array_equal(x.back(single.p0_share), want[0])
    pk = fhe.PublicKeyShare.aggregate(shares)
    assert np.array_equal(host(fhe, pk.c), np.stack([MR.add_all(octx0, want), crp]))
    singles = [fhe.PublicKeyShare(one(fhe, x, par, s, p), fhe.CommonRandomPoly(par, x.to(crp)), x.to_bytes(sd[p:p + 1]))
               for p in range(P)]
    assert np.array_equal(host(fhe, fhe.PublicKeyShare.aggregate(singles).c), host(fhe, pk.c))

    pk_any = fhe.PublicKey.from_ciphertext(par, dev_arr(fhe, x, uniform(g, octx0.moduli, n, (2,))))
    for level in (range(opar.max_level() + 1) if levels is None else levels):
        octx = opar.ctx[level]
        L = len(octx.moduli)
        ct = uniform(g, octx.moduli, n, (cts, 2))
        sl, sol = s[:, :L], s_out[:, :L]
        sd = X.seeds(rng, P * cts)
        # DecryptionShare::new: P parties x cts ciphertexts; one party x cts; P parties x one ciphertext
        d = fhe.DecryptionShare(sk, x.to(ct), level, x.to_bytes(sd))
        got = x.back(d.h_share)
        assert got.shape == (P, cts, L, n)
        want = [[MR.sks_share(octx, v, sl[p], None, ct[j][1], sd[p * cts + j]) for j in range(cts)] for p in range(P)]
        for p in range(P):
            for j in range(cts):
                assert np.array_equal(got[p][j], want[p][j]), ("decryption share", level, p, j)
        d0 = fhe.DecryptionShare(one(fhe, x, par, s), x.to(ct), level, x.to_bytes(sd[:cts]))
        assert np.array_equal(x.back(d0.h_share), got[0]), ("one party", level)
        d1 = fhe.DecryptionShare(sk, x.to(ct[0]), level, x.to_bytes(sd[::cts]))
        assert np.array_equal(x.back(d1.h_share), got[:, 0]), ("one ciphertext", level)
        # Ciphertext::from_shares
        agg = x.back(fhe.SecretKeySwitchShare.aggregate(d))
        for j in range(cts):
            assert np.array_equal(agg[j][0], MR.add_all(octx, [want[p][j] for p in range(P)], base=ct[j][0])), (level, j)
            assert np.array_equal(agg[j][1], ct[j][1])
        # SecretKeySwitchShare::new
        k = fhe.SecretKeySwitchShare(sk, sk_out, x.to(ct), level, x.to_bytes(sd))
        got = x.back(k.h_share)
        for p in range(P):
            for j in range(cts):
                assert np.array_equal(got[p][j], MR.sks_share(octx, v, sl[p], sol[p], ct[j][1], sd[p * cts + j])), \
                    ("key-switch share", level, p, j)
        # PublicKeySwitchShare::new and its aggregation
        pk_l = host(fhe, pk_any.at_level(level))
        h = fhe.PublicKeySwitchShare(sk, pk_any, x.to(ct), level, x.to_bytes(sd))
        got = x.back(h.h)
        assert got.shape == (P, cts, 2, L, n)
        want = [[MR.pks_share(octx, v, sl[p], pk_l, ct[j], sd[p * cts + j]) for j in range(cts)] for p in range(P)]
        for p in range(P):
            for j in range(cts):
                assert np.array_equal(got[p][j], want[p][j]), ("public-key-switch share", level, p, j)
        h0 = fhe.PublicKeySwitchShare(one(fhe, x, par, s), pk_any, x.to(ct), level, x.to_bytes(sd[:cts]))
        assert np.array_equal(x.back(h0.h), got[0])
        agg = x.back(fhe.PublicKeySwitchShare.aggregate(h))
        for j in range(cts):
            assert np.array_equal(agg[j][0], MR.add_all(octx, [want[p][j][0] for p in range(P)], base=ct[j][0]))
            assert np.array_equal(agg[j][1], MR.add_all(octx, [want[p][j][1] for p in range(P)]))

    if rlk and len(octx0.moduli) >= 2:
        case_relin_parity(fhe, dev, opar, par, sk, s, rng, g)


def case_relin_parity(fhe, dev, opar, par, sk, s, rng, g):
    """RelinKeyGenerator::new, both rounds and both aggregations against the restatement; the collective key's exported
    arrays are RelinearizationKey::from_shares'."""
    x = Xfer(dev)
    octx0 = opar.ctx[0]
    n, v, L, P = opar.degree(), opar.variance, len(octx0.moduli), s.shape[0]
    crp = uniform(g, octx0.moduli, n, (L,))
    u_sd, sd1, sd2 = X.seeds(rng, P), X.seeds(rng, P), X.seeds(rng, P)
    gen = fhe.RelinKeyGenerator(sk, fhe.CommonRandomPoly(par, x.to(crp)), x.to_bytes(u_sd))
    u = host(fhe, gen.u)
    for p in range(P):
        assert np.array_equal(u[p], R.small(octx0, v, u_sd[p])), ("u", p)
    r1 = gen.round_1(x.to_bytes(sd1))
    want1 = [MR.rlk_round1(octx0, v, s[p], u[p], crp, sd1[p]) for p in range(P)]
    g0, g1 = x.back(r1.h0), x.back(r1.h1)
    assert g0.shape == g1.shape == (P, L, L, n)
    for p in range(P):
        assert np.array_equal(g0[p], want1[p][0]), ("round 1 h0", p)
        assert np.array_equal(g1[p], want1[p][1]), ("round 1 h1", p)
    a1 = fhe.RelinKeyShare.aggregate_round_1(r1)
    H0 = np.stack([MR.add_all(octx0, [w[0][i] for w in want1]) for i in range(L)])
    H1 = np.stack([MR.add_all(octx0, [w[1][i] for w in want1]) for i in range(L)])
    assert np.array_equal(x.back(a1.h0), H0) and np.array_equal(x.back(a1.h1), H1)
    r2 = gen.round_2(a1, x.to_bytes(sd2))
    want2 = [MR.rlk_round2(octx0, v, s[p], u[p], H0, H1, sd2[p]) for p in range(P)]
    g0, g1 = x.back(r2.h0), x.back(r2.h1)
    for p in range(P):
        assert np.array_equal(g0[p], want2[p][0]), ("round 2 h0", p)
        assert np.array_equal(g1[p], want2[p][1]), ("round 2 h1", p)
    # one party's generator makes the same share as its slice of the batched call
    gen0 = fhe.RelinKeyGenerator(one(fhe, x, par, s), fhe.CommonRandomPoly(par, x.to(crp)), x.to_bytes(u_sd[:1]))
    assert np.array_equal(x.back(gen0.round_1(x.to_bytes(sd1[:1])).h0), want1[0][0])
    assert np.array_equal(x.back(gen0.round_2(a1, x.to_bytes(sd2[:1])).h1), want2[0][1])
    rk = fhe.RelinKeyShare.aggregate(r2)
    c0, c1 = MR.relin_key(octx0, [w[0] for w in want2], [w[1] for w in want2], H1)
    e0, e1, e0s, e1s = (host(fhe, a) for a in rk.ksk.export())
    assert np.array_equal(e0, c0) and np.array_equal(e1, c1)
    ring = R.Ring.of(octx0).c
    assert np.array_equal(e0s, np.stack([ring.shoup(p) for p in c0]))
    assert np.array_equal(e1s, np.stack([ring.shoup(p) for p in c1]))


def case_batch_forms(fhe, opar, par, batch=1024, level=0, seed=3, ref=None):
    """The batch forms at full size on the device (torch tensors): `batch` ciphertexts with one secret shared, and
    `batch` parties with a secret per item, items 0 and batch - 1 against the restatement (whose ChaCha is Python).
    Returns (the checked items of every share, the restated items): a second run -- the integer kernels after
    set_f64(False) -- passes `ref` back in and is compared with the first by the caller."""
    import torch
    x = Xfer(True)
    rng = random.Random(seed)
    n, v = opar.degree(), opar.variance
    octx, ctx = opar.ctx[level], par.context_at_level(level)
    octx0, ctx0 = opar.ctx[0], par.context_at_level(0)
    L, L0 = len(octx.moduli), len(octx0.moduli)
    items = (0, batch - 1)
    pick = lambda t: x.back(torch.stack([t[i] for i in items]))   # noqa: E731
    sk_sd = x.to_bytes(X.seeds(rng, batch))
    s_all = ctx0.sample_small(sk_sd, v, True)                     # [batch, L0, N] on the device
    u_sd = x.to_bytes(X.seeds(rng, batch))
    sks = fhe.SecretKey(par, s_all)
    sk0 = fhe.SecretKey(par, s_all[0])
    s = pick(s_all)
    ct_all = ctx.synth_uniform(seed, 0, 0, 2, batch)
    ct = pick(ct_all)
    crp_all = ctx0.synth_uniform(seed + 1, 0, 0, L0 + 1, 1)[0]    # [L0 + 1, L0, N]: one CRP and a vector of L0
    crp, crpv = crp_all[0], crp_all[1:].contiguous()
    crp_h, crpv_h = x.back(crp), x.back(crpv)
    sd = X.seeds(rng, batch)
    sdd = x.to_bytes(sd)
    got, want = {}, {}
    got["pk"] = pick(fhe.PublicKeyShare(sks, fhe.CommonRandomPoly(par, crp), sdd).p0_share)
    got["dec_shared"] = pick(fhe.DecryptionShare(sk0, ct_all, level, sdd).h_share)
    got["dec_each"] = pick(fhe.DecryptionShare(sks, ct_all[0], level, sdd).h_share)
    s2_all = ctx0.sample_small(u_sd, v, True)                     # (a second set of secrets: the switch's output keys)
    s2 = pick(s2_all)
    got["sks"] = pick(fhe.SecretKeySwitchShare(sks, fhe.SecretKey(par, s2_all), ct_all[0], level, sdd).h_share)
    pk_any = fhe.PublicKey.from_ciphertext(par, ctx0.synth_uniform(seed + 2, 0, 0, 2, 1)[0])
    pk_l = x.back(pk_any.at_level(level))
    got["pks"] = pick(fhe.PublicKeySwitchShare(sk0, pk_any, ct_all, level, sdd).h)
    gen = fhe.RelinKeyGenerator(sks, fhe.CommonRandomPoly(par, crpv), u_sd)
    u = pick(gen.u)
    r1 = gen.round_1(sdd)
    got["r1_h0"], got["r1_h1"] = pick(r1.h0), pick(r1.h1)
    # (round 2 reads public aggregated shares: any canonical polynomials do; the round-1 shares of item 0 serve)
    a1 = fhe.RelinKeyShare(par, r1.h0[0].clone(), r1.h1[0].clone())
    del r1   # (L x L rows per item: the two rounds' outputs need not be resident together)
    r2 = gen.round_2(a1, sdd)
    got["r2_h0"], got["r2_h1"] = pick(r2.h0), pick(r2.h1)
    if ref is None:
        H0, H1 = got["r1_h0"][0], got["r1_h1"][0]
        want["pk"] = np.stack([MR.pk_share(octx0, v, crp_h, s[i], sd[b]) for i, b in enumerate(items)])
        want["dec_shared"] = np.stack([MR.sks_share(octx, v, s[0][:L], None, ct[i][1], sd[b]) for i, b in enumerate(items)])
        want["dec_each"] = np.stack([MR.sks_share(octx, v, s[i][:L], None, ct[0][1], sd[b]) for i, b in enumerate(items)])
        want["sks"] = np.stack([MR.sks_share(octx, v, s[i][:L], s2[i][:L], ct[0][1], sd[b]) for i, b in enumerate(items)])
        want["pks"] = np.stack([MR.pks_share(octx, v, s[0][:L], pk_l, ct[i], sd[b]) for i, b in enumerate(items)])
        w1 = [MR.rlk_round1(octx0, v, s[i], u[i], crpv_h, sd[b]) for i, b in enumerate(items)]
        want["r1_h0"], want["r1_h1"] = np.stack([w[0] for w in w1]), np.stack([w[1] for w in w1])
        w2 = [MR.rlk_round2(octx0, v, s[i], u[i], H0, H1, sd[b]) for i, b in enumerate(items)]
        want["r2_h0"], want["r2_h1"] = np.stack([w[0] for w in w2]), np.stack([w[1] for w in w2])
    else:
        want = ref
    for name in got:
        assert np.array_equal(got[name], want[name]), name
    return got, want


def case_sum_overflow(fhe, dev, par, n):
    """Every share word q_row - 1: the closed form (nshares (+ 1)) (q - 1) mod q, with and without base, for the share
    counts around every multiple of the lazy-reduction window; then 11 shares of random canonical words against numpy
    object arithmetic, and out == base."""
    x = Xfer(dev)
    ctx = par.context_at_level(0)
    q = np.array(par.moduli, dtype=object)[:, None]
    L = len(par.moduli)
    top = np.broadcast_to(np.array([int(m) - 1 for m in par.moduli], dtype=np.uint64)[:, None], (L, n))
    from fhe_rs_amd import _lib
    import ctypes as C
    lib = _lib.lib()
    p = lambda a: C.c_void_p(a.data_ptr())   # noqa: E731
    counts = (1, 2, 3, 4, 5, 16, 17, 255)
    shares = dev_arr(fhe, x, np.broadcast_to(top, (max(counts), L, n)))
    base = dev_arr(fhe, x, top)
    out = dev_arr(fhe, x, np.zeros((L, n), dtype=np.uint64))
    for k in counts:
        for with_base in (False, True):
            assert lib.fhe_mbfv_aggregate_dev(ctx._h, p(shares), k, L * n, 1, p(base) if with_base else None, p(out),
                                              None) == 0
            got = host(fhe, out)
            want = ((k + (1 if with_base else 0)) * (q - 1)) % q
            assert (got.astype(object) == np.broadcast_to(want, (L, n))).all(), (k, with_base)
    g = np.random.default_rng(n)
    sh = uniform(g, par.moduli, n, (11, 2))   # 11 shares of 2 polynomials
    bs = uniform(g, par.moduli, n, (2,))
    d_sh, d_bs = dev_arr(fhe, x, sh), dev_arr(fhe, x, bs)
    assert lib.fhe_mbfv_aggregate_dev(ctx._h, p(d_sh), 11, 2 * L * n, 2, p(d_bs), p(d_bs), None) == 0   # out == base
    want = (sh.astype(object).sum(axis=0) + bs.astype(object)) % q
    assert (host(fhe, d_bs).astype(object) == want).all()


def summed_key(fhe, x, opar, par, s):
    """The SecretKey of the summed secret (the key the collective public key belongs to)."""
    return fhe.SecretKey(par, dev_arr(fhe, x, MR.add_all(opar.ctx[0], list(s))))


def headroom(fhe, par, level, noise_bits):
    """At least 2 bits below bitlen(q) - bitlen(t): a wrong plaintext is then a bug, not noise.  noise_bits: what
    SecretKey.measure_noise returned (an int, a numpy array or a device array)."""
    if not isinstance(noise_bits, (int, np.integer)):
        noise_bits = host(fhe, noise_bits).reshape(-1).max()
    q = 1
    for m in par.moduli[:len(par.moduli) - level]:
        q *= int(m)
    assert int(noise_bits) + 2 <= q.bit_length() - int(par.plaintext).bit_length(), (level, int(noise_bits))


def case_encrypt_decrypt(fhe, dev, opar, par, parties=11, levels=None, seed=5, restate_tail=True):
    """The reference's `encrypt_decrypt` (secret_key_switch.rs tests): collective public key -> PublicKey.encrypt of a
    random plaintext -> one decryption share per party -> fhe_mbfv_decrypt_dev gives the plaintext back.  The collective
    key is the PublicKey of the summed secret and the summed errors of the restatement; the decrypted coefficients are
    those of Plaintext::from_shares' BigUint tail (restate_tail: pure Python, small sets only)."""
    x = Xfer(dev)
    rng = random.Random(seed)
    g = np.random.default_rng(seed)
    n, v, t = opar.degree(), opar.variance, opar.plaintext
    octx0 = opar.ctx[0]
    P = parties
    sk, s, _ = secrets_of(fhe, x, opar, par, rng, P)
    crp = uniform(g, octx0.moduli, n)
    sd = X.seeds(rng, P)
    pk = fhe.PublicKeyShare.aggregate(fhe.PublicKeyShare(sk, fhe.CommonRandomPoly(par, x.to(crp)), x.to_bytes(sd)))
    ring = R.Ring.of(octx0).c
    e_sum = MR.add_all(octx0, [MR.draws(octx0, v, sd[p], 1)[0] for p in range(P)])
    s_sum = MR.add_all(octx0, list(s))
    assert np.array_equal(host(fhe, pk.c), np.stack([ring.poly_sub(e_sum, ring.poly_mul(crp, s_sum)), crp]))
    sk_sum = summed_key(fhe, x, opar, par, s)
    enc = par.encoder()
    for level in (range(opar.max_level() + 1) if levels is None else levels):
        vals = E.values(rng, t, 1, n)
        pt = enc.encode(x.to(vals), "simd", level, True)
        ct = pk.encrypt(pt, level, x.to_bytes(X.seeds(rng, 1)))
        headroom(fhe, par, level, sk_sum.measure_noise(ct, level))
        d = fhe.DecryptionShare(sk, ct[0], level, x.to_bytes(X.seeds(rng, P)))
        coeffs = fhe.DecryptionShare.aggregate(d)
        assert np.array_equal(x.back(enc.decode(coeffs, "simd")), vals[0]), level
        assert np.array_equal(x.back(coeffs), host(fhe, sk_sum.decrypt(ct[0], level))), level
        if restate_tail:
            cth, dh = x.back(ct), x.back(d.h_share)
            assert np.array_equal(x.back(coeffs), MR.plaintext_from_shares(opar, level, cth[0][0], list(dh))), level


def case_keyswitch_decrypt(fhe, dev, opar, par, parties=11, levels=None, seed=7):
    """The reference's `encrypt_keyswitch_decrypt` for both switch protocols: a ciphertext under the collective key is
    switched to the summed output secrets (secret-key switch) and to a fresh single key's public key (public-key
    switch), and decrypts under the output secret with the existing SecretKey.decrypt."""
    x = Xfer(dev)
    rng = random.Random(seed)
    g = np.random.default_rng(seed)
    n, v, t = opar.degree(), opar.variance, opar.plaintext
    octx0 = opar.ctx[0]
    P = parties
    sk, s, _ = secrets_of(fhe, x, opar, par, rng, P)
    sk_out, s_out, _ = secrets_of(fhe, x, opar, par, rng, P)
    crp = fhe.CommonRandomPoly(par, x.to(uniform(g, octx0.moduli, n)))
    pk = fhe.PublicKeyShare.aggregate(fhe.PublicKeyShare(sk, crp, x.to_bytes(X.seeds(rng, P))))
    sk_sum, out_sum = summed_key(fhe, x, opar, par, s), summed_key(fhe, x, opar, par, s_out)
    final = fhe.SecretKey.random(par, bytes(rng.getrandbits(8) for _ in range(32)))
    final_pk = fhe.PublicKey(final, bytes(range(32)), bytes(range(32, 64)))
    enc = par.encoder()
    for level in (range(opar.max_level() + 1) if levels is None else levels):
        vals = E.values(rng, t, 1, n)
        ct = pk.encrypt(enc.encode(x.to(vals), "simd", level, True), level, x.to_bytes(X.seeds(rng, 1)))
        headroom(fhe, par, level, sk_sum.measure_noise(ct, level))
        k = fhe.SecretKeySwitchShare(sk, sk_out, ct[0], level, x.to_bytes(X.seeds(rng, P)))
        ct2 = fhe.SecretKeySwitchShare.aggregate(k)
        headroom(fhe, par, level, out_sum.measure_noise(ct2, level))
        assert np.array_equal(x.back(enc.decode(out_sum.decrypt(ct2, level), "simd")), vals[0]), ("sks", level)
        h = fhe.PublicKeySwitchShare(sk, final_pk, ct[0], level, x.to_bytes(X.seeds(rng, P)))
        ct3 = fhe.PublicKeySwitchShare.aggregate(h)
        headroom(fhe, par, level, final.measure_noise(ct3, level))
        assert np.array_equal(x.back(enc.decode(final.decrypt(ct3, level), "simd")), vals[0]), ("pks", level)


def case_relinearization(fhe, dev, opar, par, parties=5, seed=9):
    """The reference's `relinearization_works`: the two-round collective relinearization key ->
    Multiplicator.default(params, rk) -> the product of two ciphertexts under the collective key -> threshold
    decryption equals the slot-wise product of the plaintexts mod t."""
    x = Xfer(dev)
    rng = random.Random(seed)
    g = np.random.default_rng(seed)
    n, v, t = opar.degree(), opar.variance, opar.plaintext
    octx0 = opar.ctx[0]
    L, P = len(octx0.moduli), parties
    sk, s, _ = secrets_of(fhe, x, opar, par, rng, P)
    crp = fhe.CommonRandomPoly(par, x.to(uniform(g, octx0.moduli, n)))
    pk = fhe.PublicKeyShare.aggregate(fhe.PublicKeyShare(sk, crp, x.to_bytes(X.seeds(rng, P))))
    crpv = fhe.CommonRandomPoly(par, x.to(uniform(g, octx0.moduli, n, (L,))))
    gen = fhe.RelinKeyGenerator(sk, crpv, x.to_bytes(X.seeds(rng, P)))
    a1 = fhe.RelinKeyShare.aggregate_round_1(gen.round_1(x.to_bytes(X.seeds(rng, P))))
    rk = fhe.RelinKeyShare.aggregate(gen.round_2(a1, x.to_bytes(X.seeds(rng, P))))
    mul = fhe.Multiplicator.default(par, rk)
    enc = par.encoder()
    vals = E.values(rng, t, 2, n)
    cts = pk.encrypt(enc.encode(x.to(vals), "simd", 0, True), 0, x.to_bytes(X.seeds(rng, 2)))
    prod = mul.multiply(cts[0], cts[1])
    assert tuple(prod.shape) == (2, L, n)
    sk_sum = summed_key(fhe, x, opar, par, s)
    headroom(fhe, par, 0, sk_sum.measure_noise(prod, 0))
    d = fhe.DecryptionShare(sk, prod, 0, x.to_bytes(X.seeds(rng, P)))
    got = x.back(enc.decode(fhe.DecryptionShare.aggregate(d), "simd"))
    want = (vals[0].astype(object) * vals[1].astype(object)) % t
    assert (got.astype(object) == want).all()
