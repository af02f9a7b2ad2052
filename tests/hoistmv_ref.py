"""The specification of the hoisted matrix-vector product (fhe_bfv_matvec_hoisted_dev) restated on Python ints: the
rotations of tests/hoist_ref.py, each times its diagonal, summed, plus the identity diagonal times the ciphertext itself."""
import hoist_ref


def matvec(c0, c1, keys, exponents, pts, pt0=None):
    """c0, c1 oracle Polys (Ntt); keys[r] an oracle KeySwitchingKey for exponents[r]; pts[r] and pt0 rows [L][N] of ints
    (Plaintext::poly_ntt).  -> (out0, out1) as rows [L][N] of canonical ints."""
    q = [int(m) for m in c0.ctx.moduli]
    terms = [(c0.coefficients, c1.coefficients, pt0)] if pt0 is not None else []
    terms += [(o0.coefficients, o1.coefficients, p) for (o0, o1), p in zip(hoist_ref.hoisted(c0, c1, keys, exponents), pts)]
    out = []
    for part in (0, 1):
        out.append([[sum(int(t[part][j][k]) * int(t[2][j][k]) for t in terms) % qj for k in range(len(terms[0][0][j]))]
                    for j, qj in enumerate(q)])
    return out[0], out[1]
