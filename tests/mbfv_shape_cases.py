"""The multiparty share kernels beyond the stock parameter sets: one shape of tests/devop_shapes.py through
mbfv_cases.case_share_parity, and the cases that cross launch groups -- every share, the aggregator and
fhe_mbfv_decrypt_dev over batches that one launch does not take.  Shared by tests/test_mbfv_shapes_gpu.py (the HIP build),
tests/test_mbfv_shapes_emu.py (kernel sources under host emulation) and the `mbfv` family of tests/random_sweep_gpu.py.
`dev`: as in mbfv_cases."""
import random

import numpy as np

import encode_cases as E
import encrypt_cases as X
import mbfv_ref as MR
from helpers import Xfer
from mbfv_cases import case_share_parity, dev_arr, headroom, host, secrets_of, summed_key, uniform


def shape_counts(n):
    """(parties, ciphertexts) of the matrix case: 2 x 2 below N = 4096, 1 x 1 from there on (the restatement draws
    every sample in Python)."""
    return (2, 2) if n < 4096 else (1, 1)


def case_shape(fhe, dev, shp, seed=1):
    """One shape of devop_shapes through case_share_parity at level 0 and the deepest level, the relin rounds on (they
    need two moduli: a single-modulus shape runs everything else), with the shape's own variance."""
    import devop_cases as D
    opar, par = D.params(fhe, shp)
    assert par.variance == shp[3]
    parties, cts = shape_counts(shp[0])
    case_share_parity(fhe, dev, opar, par, parties=parties, cts=cts, levels=sorted({0, opar.max_level()}), rlk=True,
                      seed=seed)


def case_random_shape(fhe, dev, idx):
    """Shape idx of the `mbfv` sweep family (tests/random_sweep_gpu.py; its first indices are fixed tests)."""
    import devop_shapes as S
    case_shape(fhe, dev, S.random_shape(idx), seed=idx + 1)


def bulk_seeds(g, count):
    """[count][32] seed bytes from a numpy generator (encrypt_cases.seeds draws byte by byte in Python)."""
    return g.integers(0, 255, size=(count, 32), dtype=np.uint8, endpoint=True)


SAMPLE_MOST = 65535   # Context.sample_small's most seeds per call


def sampled_secrets(fhe, x, par, g, count):
    """`count` SecretKey::random draws made by the device sampler, in calls of at most SAMPLE_MOST seeds: (the secrets
    [count, L0, N] where SecretKey wants them -- a torch tensor, or on the emulation a host array that secret_part
    uploads --, their host copy)."""
    ctx0 = par.context_at_level(0)
    sd = bulk_seeds(g, count)
    parts = [ctx0.sample_small(x.to_bytes(sd[i:i + SAMPLE_MOST]), par.variance, True) for i in range(0, count, SAMPLE_MOST)]
    if x.dev:
        s = x.torch.cat(parts) if len(parts) > 1 else parts[0]
        return s, x.back(s)
    s = np.concatenate(parts)
    return s, s


def secret_part(fhe, x, s, lo, hi):
    """Items [lo, hi) of sampled_secrets' first result as a device array."""
    return s[lo:hi] if x.dev else dev_arr(fhe, x, s[lo:hi])


def dev_empty(fhe, x, shape):
    return x.torch.empty(shape, dtype=x.torch.int64, device="cuda") if x.dev else fhe.DeviceArray(shape)


def dev_bytes(fhe, x, a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return x.to_bytes(a) if x.dev else fhe.DeviceArray.from_numpy(a)


def split_invariant(fhe, make, batch, cut):
    """make(lo, hi) -> the outputs [hi - lo, ...] of one call over items [lo, hi).  The call over the whole batch must
    equal, word for word, the calls over [0, cut) and [cut, batch) put together: `cut` is no boundary between launch
    groups, so an offset that is wrong from some group on shows at every item behind it.  Returns the whole-batch
    outputs on the host."""
    assert 0 < cut < batch
    whole = [host(fhe, o) for o in make(0, batch)]
    for lo, hi in ((0, cut), (cut, batch)):
        for i, o in enumerate(make(lo, hi)):
            o = host(fhe, o)
            assert whole[i].shape[0] == batch and o.shape == (hi - lo,) + whole[i].shape[1:], (i, o.shape)
            assert np.array_equal(whole[i][lo:hi], o), ("the call over items [%d, %d) differs" % (lo, hi), i)
    return whole


GROUP_KINDS = ("pk", "dec", "dec_shared", "sks", "pks", "rlk")


def case_share_groups(fhe, dev, opar, par, kind, batch, items, cut, seed=21, restate=None):
    """One share of the table over `batch` items in one call, at level 0: `items` against the restatement and the whole
    batch through split_invariant.  A secret per item (P parties x one ciphertext), drawn by the device sampler;
    "dec_shared": one secret for `batch` ciphertexts (a_stride != 0, s_stride == 0).  "rlk": both relin rounds through
    the C entry points (RelinKeyGenerator draws its u in one sample_small call, which takes at most 65535 seeds), with
    one set of seeds for both rounds so the restated draws are made once.  restate: the output names compared with the
    restatement (default: all)."""
    import ctypes as C
    from fhe_rs_amd import _lib
    assert kind in GROUP_KINDS
    x = Xfer(dev)
    g = np.random.default_rng(seed)
    n, v = opar.degree(), opar.variance
    octx = opar.ctx[0]
    L = len(octx.moduli)
    sd = bulk_seeds(g, batch)
    crp = lambda a: fhe.CommonRandomPoly(par, x.to(a))   # noqa: E731
    nsec = 1 if kind == "dec_shared" else batch
    s_dev, s = sampled_secrets(fhe, x, par, g, nsec)
    key = lambda a, lo, hi: fhe.SecretKey(par, secret_part(fhe, x, a, lo, hi))   # noqa: E731
    want = {}
    if kind == "pk":
        a = uniform(g, octx.moduli, n)
        make = lambda lo, hi: (fhe.PublicKeyShare(key(s_dev, lo, hi), crp(a), x.to_bytes(sd[lo:hi])).p0_share,)   # noqa: E731
        want["pk"] = lambda b: MR.pk_share(octx, v, a, s[b], sd[b])   # noqa: E731
    elif kind == "dec":
        ct = uniform(g, octx.moduli, n, (2,))
        make = lambda lo, hi: (fhe.DecryptionShare(key(s_dev, lo, hi), x.to(ct), 0, x.to_bytes(sd[lo:hi])).h_share,)   # noqa: E731
        want["dec"] = lambda b: MR.sks_share(octx, v, s[b], None, ct[1], sd[b])   # noqa: E731
    elif kind == "dec_shared":
        cts = uniform(g, octx.moduli, n, (batch, 2))
        sk1 = fhe.SecretKey(par, dev_arr(fhe, x, s[0]))
        make = lambda lo, hi: (fhe.DecryptionShare(sk1, x.to(cts[lo:hi]), 0, x.to_bytes(sd[lo:hi])).h_share,)   # noqa: E731
        want["dec_shared"] = lambda b: MR.sks_share(octx, v, s[0], None, cts[b][1], sd[b])   # noqa: E731
    elif kind == "sks":
        ct = uniform(g, octx.moduli, n, (2,))
        s2_dev, s2 = sampled_secrets(fhe, x, par, g, batch)
        make = lambda lo, hi: (fhe.SecretKeySwitchShare(key(s_dev, lo, hi), key(s2_dev, lo, hi), x.to(ct), 0,   # noqa: E731
                                                        x.to_bytes(sd[lo:hi])).h_share,)
        want["sks"] = lambda b: MR.sks_share(octx, v, s[b], s2[b], ct[1], sd[b])   # noqa: E731
    elif kind == "pks":
        ct = uniform(g, octx.moduli, n, (2,))
        pk_h = uniform(g, octx.moduli, n, (2,))
        pk = fhe.PublicKey.from_ciphertext(par, dev_arr(fhe, x, pk_h))
        make = lambda lo, hi: (fhe.PublicKeySwitchShare(key(s_dev, lo, hi), pk, x.to(ct), 0, x.to_bytes(sd[lo:hi])).h,)   # noqa: E731
        want["pks"] = lambda b: MR.pks_share(octx, v, s[b], pk_h, ct, sd[b])   # noqa: E731
    if kind != "rlk":
        got, = split_invariant(fhe, make, batch, cut)
        for name, w in want.items():
            for b in items:
                assert np.array_equal(got[b], w(b)), (name, b)
        return
    lib = _lib.lib()
    ctx0 = par.context_at_level(0)
    p = lambda a: C.c_void_p(a.data_ptr())   # noqa: E731
    a = uniform(g, octx.moduli, n, (L,))
    a_dev = dev_arr(fhe, x, a)
    u_dev, u = sampled_secrets(fhe, x, par, g, batch)

    def rounds(fn, publics):
        def make(lo, hi):
            h0, h1 = dev_empty(fhe, x, (hi - lo, L, L, n)), dev_empty(fhe, x, (hi - lo, L, L, n))
            keep = [secret_part(fhe, x, s_dev, lo, hi), secret_part(fhe, x, u_dev, lo, hi), dev_bytes(fhe, x, sd[lo:hi])]
            assert fn(ctx0._h, v, p(keep[0]), p(keep[1]), 0, *[p(q) for q in publics], p(keep[2]), p(h0), p(h1), hi - lo,
                      None) == 0
            out = host(fhe, h0), host(fhe, h1)   # (read back before the inputs of the call go)
            return out
        return make

    names = ("r1_h0", "r1_h1", "r2_h0", "r2_h1") if restate is None else restate
    g0, g1 = split_invariant(fhe, rounds(lib.fhe_mbfv_rlk_round1_dev, [a_dev]), batch, cut)
    for b in items:
        w0, w1 = MR.rlk_round1(octx, v, s[b], u[b], a, sd[b])
        assert "r1_h0" not in names or np.array_equal(g0[b], w0), ("round 1 h0", b)
        assert "r1_h1" not in names or np.array_equal(g1[b], w1), ("round 1 h1", b)
    # (round 2 reads public aggregated shares: any canonical polynomials do; the round-1 shares of item 0 serve)
    H0, H1 = g0[0].copy(), g1[0].copy()
    del g0, g1
    g0, g1 = split_invariant(fhe, rounds(lib.fhe_mbfv_rlk_round2_dev, [dev_arr(fhe, x, H0), dev_arr(fhe, x, H1)]), batch, cut)
    for b in items:
        w0, w1 = MR.rlk_round2(octx, v, s[b], u[b], H0, H1, sd[b])
        assert "r2_h0" not in names or np.array_equal(g0[b], w0), ("round 2 h0", b)
        assert "r2_h1" not in names or np.array_equal(g1[b], w1), ("round 2 h1", b)


def case_sum_groups(fhe, dev, par, n, npolys, nshares=4, seed=31):
    """fhe_mbfv_aggregate_dev over `npolys` polynomials (the grid's second dimension is cut into launches): random
    canonical words with a sprinkling of q - 1, without a base, with one, and with out == base, the whole output
    against numpy object arithmetic."""
    import ctypes as C
    from fhe_rs_amd import _lib
    x = Xfer(dev)
    lib = _lib.lib()
    ctx = par.context_at_level(0)
    L = len(par.moduli)
    g = np.random.default_rng(seed)
    top = np.array([int(m) - 1 for m in par.moduli], dtype=np.uint64)[:, None]

    def words(lead):
        a = uniform(g, par.moduli, n, lead)
        return np.where(g.random(a.shape) < 1 / 16, top, a)

    sh, bs = words((nshares, npolys)), words((npolys,))
    assert (sh == top).any() and (bs == top).any()
    q = np.array(par.moduli, dtype=object)[:, None]
    plain = sh[0].astype(object)
    for k in range(1, nshares):
        plain = plain + sh[k].astype(object)
    based = (plain + bs.astype(object)) % q
    plain = plain % q
    p = lambda a: C.c_void_p(a.data_ptr())   # noqa: E731
    d_sh, d_bs = dev_arr(fhe, x, sh), dev_arr(fhe, x, bs)
    out = dev_arr(fhe, x, np.zeros_like(bs))
    stride = npolys * L * n
    assert lib.fhe_mbfv_aggregate_dev(ctx._h, p(d_sh), nshares, stride, npolys, None, p(out), None) == 0
    assert (host(fhe, out).astype(object) == plain).all(), "no base"
    assert lib.fhe_mbfv_aggregate_dev(ctx._h, p(d_sh), nshares, stride, npolys, p(d_bs), p(out), None) == 0
    assert (host(fhe, out).astype(object) == based).all(), "base"
    assert np.array_equal(host(fhe, d_bs), bs)
    assert lib.fhe_mbfv_aggregate_dev(ctx._h, p(d_sh), nshares, stride, npolys, p(d_bs), p(d_bs), None) == 0
    assert (host(fhe, d_bs).astype(object) == based).all(), "out == base"


def case_decrypt_groups(fhe, dev, opar, par, batch, items, parties=3, seed=41):
    """fhe_mbfv_decrypt_dev through DecryptionShare.aggregate over `batch` ciphertexts under the collective key of
    `parties` parties: `items` against Plaintext::from_shares restated, the whole batch against the summed key's
    SecretKey.decrypt of the same ciphertexts and against the encoded values."""
    x = Xfer(dev)
    rng = random.Random(seed)
    g = np.random.default_rng(seed)
    n, t = opar.degree(), opar.plaintext
    octx0 = opar.ctx[0]
    P = parties
    sk, s, _ = secrets_of(fhe, x, opar, par, rng, P)
    crp = fhe.CommonRandomPoly(par, x.to(uniform(g, octx0.moduli, n)))
    pk = fhe.PublicKeyShare.aggregate(fhe.PublicKeyShare(sk, crp, x.to_bytes(X.seeds(rng, P))))
    sk_sum = summed_key(fhe, x, opar, par, s)
    enc = par.encoder()
    vals = E.values(rng, t, batch, n)
    ct = pk.encrypt(enc.encode(x.to(vals), "simd", 0, True), 0, x.to_bytes(bulk_seeds(g, batch)))
    headroom(fhe, par, 0, sk_sum.measure_noise(ct, 0))
    d = fhe.DecryptionShare(sk, ct, 0, x.to_bytes(bulk_seeds(g, P * batch)))
    coeffs = fhe.DecryptionShare.aggregate(d)
    got = x.back(coeffs)
    assert got.shape == (batch, n)
    assert np.array_equal(got, host(fhe, sk_sum.decrypt(ct, 0)))
    assert np.array_equal(x.back(enc.decode(coeffs, "simd")), vals)
    cth, dh = x.back(ct), x.back(d.h_share)
    assert dh.shape == (P, batch, len(octx0.moduli), n)
    for b in items:
        assert np.array_equal(got[b], MR.plaintext_from_shares(opar, 0, cth[b][0], [dh[q][b] for q in range(P)])), b
