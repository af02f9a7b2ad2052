"""The specification of the hoisted rotations (fhe_bfv_galois_hoisted_dev) restated on the Python oracle's Poly: every
rotation of a ciphertext from ONE digit decomposition of c1.  Not GaloisKey::relinearize's words (it lifts the digits of
substitute(c1); this substitutes the lifted digits of c1): equal to it at exponent 1, and by decryption elsewhere."""
from fhe_oracle.rq import NTT, POWER_BASIS, Poly, SubstitutionExponent


def digit_rows(c1):
    """W[i] = NTT(p_i lifted to every modulus), p = PowerBasis(c1): row j is NTT_j(p_i mod q_j), row i is c1's row i."""
    ctx = c1.ctx
    p = c1.into_power_basis()
    return [Poly(ctx, POWER_BASIS, [qj.reduce_vec(row) for qj in ctx.q]).into_ntt() for row in p.coefficients]


def hoisted(c0, c1, keys, exponents, w=None):
    """[(out0, out1) per rotation]: keys[r] an oracle KeySwitchingKey (NttShoup c0 / c1 per digit) for exponents[r]."""
    ctx = c0.ctx
    w = digit_rows(c1) if w is None else w
    out = []
    for key, e in zip(keys, exponents):
        el = SubstitutionExponent(ctx, e)
        o0, o1 = c0.substitute(el), Poly.zero(ctx, NTT)
        for wi, k0, k1 in zip(w, key.c0, key.c1):
            s = wi.substitute(el)
            o0, o1 = o0.add(s.mul(k0)), o1.add(s.mul(k1))
        out.append((o0, o1))
    return out
