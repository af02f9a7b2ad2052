"""Test-side restatement of the multiparty BFV protocols (crates/fhe/src/mbfv/: public_key_gen.rs:32-77,
secret_key_switch.rs:38-186, public_key_switch.rs:33-113, relin_key_gen.rs:112-351), in the order of operations of the
reference's text.  Built from encrypt_ref.py's generator, sampler and `Ring` (the plain-C oracle over one context), so
every random polynomial is a Poly::small draw of ChaCha8Rng::from_seed(seed) and consecutive draws of one share come
from one generator.  The common random polynomial is an input, as in the engine.

Shared by tests/test_mbfv_emu.py and tests/test_mbfv_gpu.py."""
import numpy as np

import encrypt_ref as R
from fhe_oracle import bfv as obfv
from fhe_oracle.rns import RnsContext
from fhe_oracle.rq import Poly, NTT


_drawn = {}


def draws(ctx, variance, seed, count):
    """`count` consecutive Poly::<Ntt>::small(ctx, variance, rng) of rng = ChaCha8Rng::from_seed(seed): [count][L][N].
    (The generator and the draws made so far are kept per (context, variance, seed): the shares of one test item reuse
    one seed, and the Python ChaCha is what a full-size restatement costs.)"""
    key = (id(ctx), variance, bytes(seed))
    if key not in _drawn:
        if len(_drawn) >= 64:
            _drawn.clear()
        _drawn[key] = (R.generator(seed), [])
    g, have = _drawn[key]
    r = R.Ring.of(ctx).c
    while len(have) < count:
        have.append(r.poly_ntt_forward(R.lift(ctx, obfv.sample_vec_cbd(ctx.degree, variance, g))))
    return have[:count]


def pk_share(ctx, variance, crp, s, seed):
    """PublicKeyShare::new: p0 = -crp; p0 *= s; p0 += e."""
    r = R.Ring.of(ctx).c
    e, = draws(ctx, variance, seed, 1)
    return r.poly_add(r.poly_mul(r.poly_neg(crp), s), e)


def sks_share(ctx, variance, s_in, s_out, c1, seed):
    """SecretKeySwitchShare::new: h = s_in - s_out; h *= ct[1]; h += e.  s_out None: DecryptionShare::new, whose output
    key is SecretKey::new(vec![0; N]) -- the zero polynomial."""
    r = R.Ring.of(ctx).c
    if s_out is None:
        s_out = np.zeros_like(s_in)
    e, = draws(ctx, variance, seed, 1)
    return r.poly_add(r.poly_mul(r.poly_sub(s_in, s_out), c1), e)


def pks_share(ctx, variance, s, pk, ct, seed):
    """PublicKeySwitchShare::new: u, e0, e1 in this order; h0 = pk0 u + s c1 + e0, h1 = pk1 u + e1: [2][L][N]."""
    r = R.Ring.of(ctx).c
    u, e0, e1 = draws(ctx, variance, seed, 3)
    h0 = r.poly_add(r.poly_add(r.poly_mul(pk[0], u), r.poly_mul(s, ct[1])), e0)
    h1 = r.poly_add(r.poly_mul(pk[1], u), e1)
    return np.stack([h0, h1])


def garner_times(ctx, i, s):
    """w * s for the BigUint w = RnsContext(moduli).get_garner(i): every row times w mod q_r."""
    r = R.Ring.of(ctx).c
    w = RnsContext(list(ctx.moduli)).get_garner(i)
    wp = np.array([[w % q] * ctx.degree for q in ctx.moduli], dtype=np.uint64)
    return r.poly_mul(wp, s)


def rlk_round1(ctx, variance, s, u, crp, seed):
    """RelinKeyShare<R1>::new: generate_h0 draws L errors, then generate_h1 draws L more from the same generator.
    h0_i = -a_i; h0_i *= u; h0_i += w_i s; h0_i += e_i.  h1_i = a_i; h1_i *= s; h1_i += e'_i.  -> (h0, h1) [L][L][N]."""
    r = R.Ring.of(ctx).c
    L = len(ctx.moduli)
    e = draws(ctx, variance, seed, 2 * L)
    h0 = [r.poly_add(r.poly_add(r.poly_mul(r.poly_neg(crp[i]), u), garner_times(ctx, i, s)), e[i]) for i in range(L)]
    h1 = [r.poly_add(r.poly_mul(crp[i], s), e[L + i]) for i in range(L)]
    return np.stack(h0), np.stack(h1)


def rlk_round2(ctx, variance, s, u, r1_h0, r1_h1, seed):
    """RelinKeyShare<R2>::new: h0'_i = H0_i s + e_i; h1'_i = H1_i (u - s) + e'_i; draws as round 1."""
    r = R.Ring.of(ctx).c
    L = len(ctx.moduli)
    e = draws(ctx, variance, seed, 2 * L)
    u_s = r.poly_sub(u, s)
    h0 = [r.poly_add(r.poly_mul(r1_h0[i], s), e[i]) for i in range(L)]
    h1 = [r.poly_add(r.poly_mul(r1_h1[i], u_s), e[L + i]) for i in range(L)]
    return np.stack(h0), np.stack(h1)


def add_all(ctx, polys, base=None):
    """base + the polynomials, one `+=` after the other (every from_shares)."""
    r = R.Ring.of(ctx).c
    it = iter(polys)
    acc = base if base is not None else next(it)
    for p in it:
        acc = r.poly_add(acc, p)
    return acc


def relin_key(ctx, r2_h0s, r2_h1s, r1_h1):
    """RelinearizationKey::from_shares: c0_i = sum h0_i + sum h1_i, c1_i = the aggregated round-1 h1_i."""
    L = len(ctx.moduli)
    c0 = [add_all(ctx, [add_all(ctx, [h[i] for h in r2_h0s]), add_all(ctx, [h[i] for h in r2_h1s])]) for i in range(L)]
    return np.stack(c0), np.asarray(r1_h1)


def plaintext_from_shares(opar, level, c0, shares):
    """Plaintext::from_shares (secret_key_switch.rs:145-186), with its BigUint tail: c = c0 + sum h in PowerBasis,
    d = c.scale(cipher_plain scaler), v_i = lift(d_i) + t, w_i = v_i mod q(d's context), then mod t: [N]."""
    ctx = opar.ctx[level]
    c = add_all(ctx, shares, base=c0)
    c = Poly(ctx, NTT, [[int(x) for x in row] for row in c]).into_power_basis()
    d = c.scale(opar.plain_scaler[level])
    t = opar.plaintext
    q_poly = d.ctx.modulus()
    w = [(vi + t) % q_poly for vi in d.to_biguints()[:opar.degree()]]
    return np.array([wi % t for wi in w], dtype=np.uint64)
