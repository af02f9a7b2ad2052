"""The specification of the baby-step/giant-step hoisted matrix-vector product (fhe_bfv_matvec_bsgs_dev) restated on Python
ints, on top of the two restatements it composes: G inner sums as hoistmv_ref.matvec forms them over the baby keys, every
inner sum but the first rotated under its own giant key through hoist_ref.hoisted, and the canonical sum of the results.

The G inner sums share their baby rotations, which hoistmv_ref.matvec would recompute for every group: they are formed
once through hoist_ref.hoisted and summed here in hoistmv_ref.matvec's words (tests/test_bsgs_emu.py holds inner_sums
against hoistmv_ref.matvec group by group).  Likewise the digit rows of equal inner sums are formed once."""
import hoist_ref
from fhe_oracle.rq import NTT, Poly


def inner_sums(c0, c1, baby_keys, baby_exps, pts):
    """[(inner0, inner1) per group]: pts[g][0] * (c0, c1) + sum_r pts[g][r + 1] * rotation_r, rows [L][N] of canonical ints."""
    q = [int(m) for m in c0.ctx.moduli]
    rots = [(o0.coefficients, o1.coefficients) for o0, o1 in hoist_ref.hoisted(c0, c1, baby_keys, baby_exps)]
    terms = [(c0.coefficients, c1.coefficients)] + rots
    out = []
    for row in pts:
        assert len(row) == len(terms)
        out.append(tuple([[sum(int(t[part][j][k]) * int(p[j][k]) for t, p in zip(terms, row)) % qj for k in range(len(row[0][j]))]
                          for j, qj in enumerate(q)] for part in (0, 1)))
    return out


def matvec(c0, c1, baby_keys, baby_exps, giant_keys, giant_exps, pts):
    """c0, c1 oracle Polys (Ntt); baby_keys[r] / giant_keys[g] oracle KeySwitchingKeys for baby_exps[r] / giant_exps[g];
    pts[g][b] rows [L][N] of ints (Plaintext::poly_ntt), g <= len(giant_keys), b <= len(baby_keys): column 0 the identity
    diagonal of a group, row 0 the group without a giant rotation.  -> (out0, out1) as rows [L][N] of canonical ints."""
    ctx = c0.ctx
    q = [int(m) for m in ctx.moduli]
    assert len(pts) == len(giant_keys) + 1
    inner = inner_sums(c0, c1, baby_keys, baby_exps, pts)
    out = [inner[0][0], inner[0][1]]
    rows = {}   # hoist_ref.digit_rows by the words of c1
    for g, (i0, i1) in enumerate(inner[1:]):
        p1 = Poly(ctx, NTT, i1)
        words = tuple(map(tuple, i1))
        if words not in rows:
            rows[words] = hoist_ref.digit_rows(p1)
        (r0, r1), = hoist_ref.hoisted(Poly(ctx, NTT, i0), p1, [giant_keys[g]], [giant_exps[g]], rows[words])
        for part, r in enumerate((r0, r1)):
            out[part] = [[(int(a) + int(b)) % qj for a, b in zip(ra, rb)] for ra, rb, qj in zip(out[part], r.coefficients, q)]
    return out[0], out[1]
