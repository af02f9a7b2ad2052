"""Test-side restatement of key-switching-key generation (crates/fhe/src/bfv/keys/key_switching_key.rs:71-236
`KeySwitchingKey::new`, relinearization_key.rs:43-64, galois_key.rs:26-58) with rng = ChaCha8Rng::from_seed(S), built
from the oracle's pieces: `seeded.ChaCha8Rng` for K and the digit seeds, `seeded.random_from_seed` for c1,
`bfv.sample_vec_cbd` behind encrypt_ref's next_u64 adapter for the errors (continuing the stream of S after K),
`rns.RnsContext.get_garner` for the digit scalars, and the oracle's `Switcher` and `Poly.substitute` for `from`.

`ksk` takes the engine's shortcut c0 = NTT(e) - c1 (.) s + g (.) NTT(from) on the plain-C oracle (fast at full size);
`check_order_of_operations` pins it against the reference's own order (b = e - INTT(c1 s) + g from in PowerBasis, then
NTT) on the pure-Python Poly, and `check_decrypts` checks a restated key independently: an oracle relinearization or
rotation with it decrypts correctly.

Shared by tests/test_keygen_emu.py, tests/test_keygen_gpu.py and tests/golden/make_keygen_golden.py."""
import numpy as np

import encrypt_ref as ER
from fhe_oracle import bfv as obfv
from fhe_oracle import seeded
from fhe_oracle.rns import RnsContext
from fhe_oracle.rq import NTT, NTT_SHOUP, Poly, SubstitutionExponent, Switcher


def le_bytes(words):
    return b"".join(int(w).to_bytes(8, "little") for w in words)


def derive(seed):
    """(K, the rng positioned after K): `rng.fill(&mut seed)` takes the first four next_u64 words of S's stream."""
    rng = seeded.ChaCha8Rng(bytes(seed))
    return le_bytes(rng.next_u64() for _ in range(4)), rng


def digit_seeds(K, ndigits):
    """generate_c1: seed_i = bytes [32 i, 32 i + 32) of ChaCha8Rng::from_seed(K)."""
    rng = seeded.ChaCha8Rng(K)
    words = [rng.next_u64() for _ in range(4 * ndigits)]
    return [le_bytes(words[4 * i:4 * i + 4]) for i in range(ndigits)]


def digits(ctx_ct, ctx_k):
    """(ndigits, log_base): RNS digits, or the decomposition of a single-modulus key context (:97-110)."""
    if len(ctx_k.moduli) == 1:
        lm = (ctx_k.moduli[0] - 1).bit_length()   # == q.next_power_of_two().ilog2()
        return -(-lm // (lm // 2)), lm // 2
    return len(ctx_ct.moduli), 0


def scalars(ctx_ct, ctx_k):
    """[ndigits][Lk] digit scalars mod q_j: get_garner(i) of the ciphertext moduli, or 2^(i log_base)."""
    nd, lb = digits(ctx_ct, ctx_k)
    if lb:
        return [[(1 << (i * lb)) % q for q in ctx_k.moduli] for i in range(nd)]
    rns = RnsContext(list(ctx_ct.moduli))
    return [[rns.get_garner(i) % q for q in ctx_k.moduli] for i in range(nd)]


def s_ntt(ctx, s_coeffs):
    return ER.Ring.of(ctx).c.poly_ntt_forward(ER.lift(ctx, s_coeffs))


def ksk(ctx_ct, ctx_k, variance, s_coeffs, from_ntt, seed, only=None):
    """KeySwitchingKey::new(sk, from, ...) with rng = ChaCha8Rng::from_seed(seed): (c0, c1 [nd][Lk][N], K).  `only`:
    the digits to compute (the others are zero; their errors are still drawn), for full-size sets."""
    r = ER.Ring.of(ctx_k).c
    n = ctx_k.degree
    nd, _ = digits(ctx_ct, ctx_k)
    K, rng = derive(seed)
    bits = ER.Bits(rng)
    s = s_ntt(ctx_k, s_coeffs)
    g = scalars(ctx_ct, ctx_k)
    q = np.array(ctx_k.moduli, dtype=object)[:, None]
    f = np.asarray(from_ntt).astype(object)
    c0, c1 = [], []
    for i, sd in enumerate(digit_seeds(K, nd)):
        xs = obfv.sample_vec_cbd(n, variance, bits)
        if only is not None and i not in only:
            c0.append(np.zeros((len(ctx_k.moduli), n), dtype=np.uint64))
            c1.append(c0[-1])
            continue
        a = np.array(seeded.random_from_seed(ctx_k.moduli, n, sd), dtype=np.uint64)
        e = r.poly_ntt_forward(ER.lift(ctx_k, xs))
        gf = (f * np.array(g[i], dtype=object)[:, None] % q).astype(np.uint64)
        c0.append(r.poly_add(r.poly_sub(e, r.poly_mul(a, s)), gf))
        c1.append(a)
    return np.array(c0), np.array(c1), K


def shoup(a, ctx):
    """floor(c 2^64 / q) row by row."""
    q = np.array(ctx.moduli, dtype=object)[:, None]
    return ((np.asarray(a).astype(object) << 64) // q).astype(np.uint64)


def relin_from(opar, s_coeffs, cl, kl):
    """RelinearizationKey::new_leveled's `from` in Ntt form over the key context."""
    ct, kc = opar.ctx[cl], opar.ctx[kl]
    s = s_ntt(ct, s_coeffs)
    s2 = ER.Ring.of(ct).c.poly_mul(s, s)
    if cl == kl:
        return s2
    pb = Poly(ct, NTT, [[int(w) for w in row] for row in s2]).into_power_basis()
    return np.array(pb.switch(Switcher(ct, kc)).into_ntt().coefficients, dtype=np.uint64)


def galois_from(opar, s_coeffs, exponent, cl, kl):
    """GaloisKey::new's `from` in Ntt form over the key context."""
    ct, kc = opar.ctx[cl], opar.ctx[kl]
    sub = Poly.from_i64(ct, s_coeffs).substitute(SubstitutionExponent(ct, exponent))
    if cl != kl:
        sub = sub.switch(Switcher(ct, kc))
    return np.array(sub.into_ntt().coefficients, dtype=np.uint64)


def oracle_key(opar, c0, c1, cl, kl):
    """The restated key as an oracle KeySwitchingKey."""
    kc = opar.ctx[kl]
    _, lb = digits(opar.ctx[cl], kc)
    polys = lambda a: [Poly(kc, NTT_SHOUP, [[int(w) for w in row] for row in p]) for p in a]   # noqa: E731
    return obfv.KeySwitchingKey.from_parts(opar, polys(c0), polys(c1), cl, kl, lb)


def check_order_of_operations(opar, s_coeffs, from_ntt, seed, cl, kl):
    """`ksk` equals the reference's order of operations on the pure-Python Poly: a_s = INTT(c1 (.) s),
    b = small - a_s + g from (PowerBasis), c0 = NTT(b)."""
    ct, kc = opar.ctx[cl], opar.ctx[kl]
    c0, c1, K = ksk(ct, kc, opar.variance, s_coeffs, from_ntt, seed)
    nd, _ = digits(ct, kc)
    _, rng = derive(seed)
    bits = ER.Bits(rng)
    s = Poly.from_i64(kc, s_coeffs).into_ntt()
    f = Poly(kc, NTT, [[int(w) for w in row] for row in from_ntt]).into_power_basis()
    g = scalars(ct, kc)
    for i, sd in enumerate(digit_seeds(K, nd)):
        a = Poly(kc, NTT, seeded.random_from_seed(kc.moduli, kc.degree, sd))
        assert c1[i].tolist() == a.coefficients
        a_s = a.mul(s).into_power_basis()
        b = Poly.from_i64(kc, obfv.sample_vec_cbd(kc.degree, opar.variance, bits)).sub(a_s)
        gf = Poly(kc, f.rep, [[x * gj % q for x in row] for row, gj, q in zip(f.coefficients, g[i], kc.moduli)])
        assert c0[i].tolist() == b.add(gf).into_ntt().coefficients, i


def check_decrypts(opar, s_coeffs, seed, cl=0, kl=0, exponent=None, rng_seed=1):
    """Independent of the restated layout: a relinearization key (exponent None) or a Galois key made by `ksk` works in
    the oracle's own relinearize / rotate, and the result decrypts to the expected values."""
    import random
    rng = random.Random(rng_seed)
    sk = obfv.SecretKey(opar, list(s_coeffs))
    ct_ctx, kc = opar.ctx[cl], opar.ctx[kl]
    n, t = opar.degree(), opar.plaintext
    if exponent is None:
        frm = relin_from(opar, s_coeffs, cl, kl)
    else:
        frm = galois_from(opar, s_coeffs, exponent, cl, kl)
    c0, c1, _ = ksk(ct_ctx, kc, opar.variance, s_coeffs, frm, seed)
    key = oracle_key(opar, c0, c1, cl, kl)
    a = [rng.randrange(t) for _ in range(n)]
    ca = sk.encrypt(a, rng, cl)
    if exponent is None:
        b = [rng.randrange(t) for _ in range(n)]
        prod = ca.mul(sk.encrypt(b, rng, cl))
        obfv.RelinearizationKey(ksk=key).relinearizes(prod)
        return sk.decrypt(prod), (a, b)
    rot = obfv.GaloisKey(ksk=key, exponent=exponent, ciphertext_level=cl, par=opar).relinearize(ca)
    return sk.decrypt(rot), a
