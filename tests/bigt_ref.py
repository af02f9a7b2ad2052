"""The two reference items the oracle has no `Large` branch for, restated on Python integers over the oracle's own
classes (BfvParameters with a Python-int t, Scaler, Poly.from_biguints / to_biguints, SecretKey.phase):
Plaintext::to_poly for a plaintext modulus of more than 64 bits (F/bfv/plaintext.rs:172-197, with the unscaled
poly_ntt of F/bfv/plaintext_vec.rs:105-132) and the Large branch of SecretKey::try_decrypt
(F/bfv/keys/secret_key.rs:238-250)."""
from fhe_oracle.rq import Poly

A_T = (1 << 127) - 1
B_T = 340282366920938463463374607431768211507
# name -> (t, moduli sizes, W_t, P): the reference's own test (A), its 129-bit modulus on 62-bit rows (B), the smallest
# big t (C), W_t = 4 (D) and F64-class rows (E)
SETS = {
    "A": (A_T, [60] * 5, 2, 4),
    "B": (B_T, [62] * 5, 3, 4),
    "C": ((1 << 64) + 13, [50, 50, 50], 2, 3),
    "D": ((1 << 255) - 19, [60] * 7, 4, 6),
    "E": (A_T, [36] * 7 + [37], 2, 6),
}
# a t with the top bit of its fourth limb set: the smallest Barrett constant and the largest carries
T256 = ((1 << 256) - 189, [60] * 7)


def limbs_of(t):
    return (t.bit_length() + 63) // 64


def poly_ntt(opar, values, level=0):
    """Plaintext::poly_ntt of Vec<BigUint> values, each taken modulo t first (as the engine's u64 encoder does)."""
    t = opar.plaintext
    return Poly.from_biguints(opar.ctx[level], [v % t for v in values]).into_ntt()


def scaled_coefficients(opar, values, level=0):
    """m' = (v q_mod_t) mod t per coefficient, zero-padded to the degree."""
    t = opar.plaintext
    return [(v % t) * opar.q_mod_t[level] % t for v in values] + [0] * (opar.degree() - len(values))


def to_poly(opar, values, level=0):
    """Plaintext::to_poly, Large branch: NTT(m' mod q_i) (.) delta."""
    m = Poly.from_biguints(opar.ctx[level], scaled_coefficients(opar, values, level)).into_ntt()
    return m.mul(opar.delta[level])


def to_poly_power_basis(opar, values, level=0):
    """The same polynomial in PowerBasis, without a transform: (m' mod q_i) delta_i mod q_i, delta_i = (-t)^-1 mod q_i."""
    t = opar.plaintext
    mp = scaled_coefficients(opar, values, level)
    rows = []
    for q in opar.ctx[level].moduli:
        d = pow((-t) % q, -1, q)
        rows.append([(m % q) * d % q for m in mp])
    return rows


def tail(opar, x):
    """((x + t) mod Q_p) mod t for x in [0, Q_p)."""
    t, qp = opar.plaintext, opar.plaintext_context.modulus()
    return ((x + t) % qp) % t


def decrypt(sk, ct):
    """SecretKey::try_decrypt, Large branch: the phase scaled into the plaintext context, lifted, then the tail."""
    par = sk.par
    d = sk.phase(ct).scale(par.plain_scaler[ct.level])
    return [tail(par, x) for x in d.to_biguints()]


def decrypt_columns(sk, ct_rows, level, columns):
    """decrypt() for the coefficients `columns` of one ciphertext given as words [nparts][L][N]: phase and scale through
    the oracle's C restatement (large degrees), lift and tail on Python integers."""
    import numpy as np
    from fhe_oracle import coracle
    par = sk.par
    ctx = par.ctx[level]
    cc = coracle.CCtx(ctx)
    s = cc.poly_ntt_forward(Poly.from_i64(ctx, sk.coeffs).coefficients)
    acc = np.asarray(ct_rows[-1], dtype=np.uint64)
    for i in range(len(ct_rows) - 2, -1, -1):   # (Horner: the same canonical value as the running power of s)
        acc = cc.poly_add(cc.poly_mul(acc, s), ct_rows[i])
    d = coracle.CScaler(par.plain_scaler[level]).scale(cc.poly_ntt_backward(acc), False)
    rns = par.plaintext_context.rns
    return [tail(par, rns.lift([int(d[i][j]) for i in range(d.shape[0])])) for j in columns]


def measure_noise(sk, ct, values):
    """SecretKey::measure_noise (secret_key.rs:55-98) with to_poly above."""
    s = sk._s(ct[0].ctx)
    si, c = s, ct[0]
    for i in range(1, len(ct)):
        c = c.add(ct[i].mul(si))
        si = si.mul(s)
    c = c.sub(to_poly(sk.par, values, ct.level)).into_power_basis()
    q = ct[0].ctx.modulus()
    return max(min(x.bit_length(), (q - x).bit_length()) for x in c.to_biguints())
