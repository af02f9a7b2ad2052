"""Cases of the hoisted matrix-vector product (fhe_bfv_matvec_hoisted_dev; KeySet.matvec_hoisted, HoistedRotations.matvec):
the rotations of a ciphertext, their products with the diagonals and the sum in one stage B.  Shared by
tests/test_hoistmv_emu.py (kernel sources under host emulation) and tests/test_hoistmv_gpu.py (the HIP build).  `dev`: as
helpers.Xfer.

Two references: the restatement tests/hoistmv_ref.py (Python ints on hoist_ref's rotations), and the engine's own
composition KeySet.relinearize_hoisted then Context.dot_product_scalar, which the call must equal word for word."""
import ctypes as C

import numpy as np
import pytest

import hoist_cases as H
import hoistmv_ref
import keyed_cases as K
from fhe_oracle import bfv as obfv
from fhe_oracle.rq import NTT, Poly
from helpers import Xfer, ct_arr

TABLE = H.TABLE
SMALL = H.SMALL
same = K.same


def reference(octx, ct, okeys, exps, pts, pt0):
    """hoistmv_ref over a batch: ct [batch, 2, L, N]; pts [R, L, N] or [batch, R, L, N]; pt0 None, [L, N] or [batch, L, N]."""
    out = []
    for b, c in enumerate(ct):
        c0, c1 = (Poly(octx, NTT, part.tolist()) for part in c)
        p = pts if pts.ndim == 3 else pts[b]
        p0 = None if pt0 is None else (pt0 if pt0.ndim == 2 else pt0[b])
        o0, o1 = hoistmv_ref.matvec(c0, c1, okeys, exps, p.tolist(), None if p0 is None else p0.tolist())
        out.append(np.array([o0, o1], dtype=np.uint64))
    return np.stack(out)


def composition(ks, ctx, exps, ct, pts, pt0):
    """The engine's own two calls on host arrays: the specification of the fused call."""
    cts = ks.relinearize_hoisted(exps, ct)                       # [batch, R, 2, L, N]
    p = pts
    if pt0 is not None:
        cts = np.concatenate([ct[:, None], cts], axis=1)
        p = np.concatenate([pt0[..., None, :, :], pts], axis=-3)
    return ctx.dot_product_scalar(np.ascontiguousarray(cts), np.ascontiguousarray(p))


def diagonals(rng, q, n, nrot, batch, shared, top=False):
    """(pts, pt0): uniform words (`top`: q_j - 1), shared by the batch or one set per item."""
    lead = () if shared else (batch,)
    if top:
        row = np.array(q, dtype=np.uint64)[:, None] - np.uint64(1)
        return (np.broadcast_to(row, lead + (nrot, len(q), n)).copy(), np.broadcast_to(row, lead + (len(q), n)).copy())
    return K.uniform(rng, q, n, lead + (nrot,)), K.uniform(rng, q, n, lead)


def run(x, ks, exps, ct, pts, pt0):
    return x.back(ks.matvec_hoisted(exps, x.to(ct), x.to(pts), None if pt0 is None else x.to(pt0)))


def case_anchor(fhe, dev, cl=0, kl=0, exps=(1, 3, 9, 31, 3), batch=2, seed=201, variants=None):
    """Real keys from the oracle at N = 16 over [62, 60, 55]: shared and per-item diagonals, with and without pt0, every
    word against hoistmv_ref and against relinearize_hoisted + dot_product_scalar."""
    x = Xfer(dev)
    opar, par = K.params(fhe, *SMALL)
    cs = K.Clients(fhe, opar, par, 1, seed)
    ogk, gks = cs.galois_keys(exps, cl, kl)
    ogk, gks = ogk[0], gks[0]
    cts = [cs.encrypt(0, cl) for _ in range(batch)]
    inp = np.stack([ct_arr(c) for c in cts])
    ks = fhe.KeySet([g.ksk for g in gks])
    octx = opar.context_at_level(cl)
    ctx = par.context_at_level(cl)
    q = [int(m) for m in octx.moduli]
    g = np.random.default_rng(seed)
    for shared, with0 in (variants or [(True, True), (True, False), (False, True), (False, False)]):
        pts, pt0 = diagonals(g, q, opar.degree(), len(exps), batch, shared)
        pt0 = pt0 if with0 else None
        got = run(x, ks, exps, inp, pts, pt0)
        assert got.shape == inp.shape
        same(got, reference(octx, inp, [ogk[e].ksk for e in exps], exps, pts, pt0), ("hoistmv_ref", shared, with0, cl))
        same(got, composition(ks, ctx, exps, inp, pts, pt0), ("composition", shared, with0, cl))


def case_forms(fhe, dev, seed=203):
    """HoistedRotations.matvec: a result of the input's kind, one ciphertext without a batch dimension, shapes refused."""
    x = Xfer(dev)
    opar, par = K.params(fhe, *SMALL)
    n = opar.degree()
    cs = K.Clients(fhe, opar, par, 1, seed)
    exps = [pow(3, 1, 2 * n), pow(3, 2, 2 * n)]
    _, gks = cs.galois_keys(exps)
    h = fhe.EvaluationKey(n, gks[0]).hoisted(column_rotations=(1, 2))
    inp = np.stack([ct_arr(cs.encrypt(0)) for _ in range(2)])
    ctx = par.context_at_level(0)
    q = [int(m) for m in opar.context_at_level(0).moduli]
    pts, pt0 = diagonals(np.random.default_rng(seed), q, n, 2, 2, True)
    want = composition(h.set, ctx, h.exponents, inp, pts, pt0)
    out = h.matvec(x.to(inp), x.to(pts), x.to(pt0))
    assert type(out) is type(x.to(inp))
    same(x.back(out), want, "HoistedRotations.matvec")
    one = x.back(h.matvec(x.to(inp[1]), x.to(pts), x.to(pt0)))
    assert one.shape == inp.shape[1:]
    same(one, want[1], "one ciphertext")
    for bad in (pts[:1], np.concatenate([pts, pts])[None]):
        with pytest.raises(fhe.FheError) as err:
            h.matvec(x.to(inp), x.to(np.ascontiguousarray(bad)))
        assert err.value.code == -1 and "DotProductLengthMismatch" in str(err.value)
    with pytest.raises(fhe.FheError) as err:
        h.matvec(x.to(inp), x.to(pts), x.to(np.stack([pt0, pt0])))
    assert err.value.code == -1 and "identity diagonal" in str(err.value)


def case_matrix_vector(fhe, dev, seed=127):
    """hoist_cases.case_matrix_vector's 4 x 4 matrix at N = 16 through HoistedRotations.matvec with diagonal 0 as pt0:
    decrypted and decoded, against numpy modulo t."""
    x = Xfer(dev)
    n, sizes = SMALL
    opar, par = K.params(fhe, n, sizes)
    t, d, cols = opar.plaintext, 4, n // 2
    g = np.random.default_rng(seed)
    M, v = g.integers(0, t, size=(d, d), dtype=np.uint64), g.integers(0, t, size=d, dtype=np.uint64)
    enc = par.encoder()
    sk = fhe.SecretKey.random(par, bytes(range(32)))
    ek = fhe.EvaluationKey.generate(sk, column_rotations=(1, 2, 3), seeds=[bytes([i + 1] * 32) for i in range(3)])
    slots = np.tile(v, n // d)
    ct = sk.encrypt(enc.encode(slots[None], scaled=True), a_seeds=[bytes([7] * 32)], e_seeds=[bytes([8] * 32)])
    ramp = np.arange(n, dtype=np.uint64)[None]
    rc = sk.encrypt(enc.encode(ramp, scaled=True), a_seeds=[bytes([9] * 32)], e_seeds=[bytes([10] * 32)])
    turned = enc.decode(sk.decrypt(ek.rotates_columns_by(rc, 1)))[0]
    step = int(turned[0])
    assert step in (1, cols - 1) and list(turned[:cols]) == [(k + step) % cols for k in range(cols)], turned
    diag = np.stack([np.array([M[k % d][(k + i * step) % d] for k in range(n)], dtype=np.uint64) for i in range(d)])
    pts = np.asarray(enc.encode(diag))                       # [4, L, N] poly_ntt
    h = ek.hoisted(column_rotations=(1, 2, 3))
    prod = h.matvec(x.to(ct), x.to(np.ascontiguousarray(pts[1:])), x.to(np.ascontiguousarray(pts[0])))
    got = enc.decode(sk.decrypt(x.back(prod)))[0]
    want = (M.astype(object) @ v.astype(object)) % t
    assert [int(a) for a in got] == [int(want[k % d]) for k in range(n)], (got, want)


def synthetic(fhe, q, n, nrot, batch, seed, top=False, shared=True, exps=None):
    sy = K.Synthetic(fhe, q, n, nrot, seed, top)
    exps = list(exps) if exps is not None else H.odd_exponents(n, nrot, seed)
    g = np.random.default_rng(seed + 1000)
    if top:
        ct = np.broadcast_to(np.array(sy.q, dtype=np.uint64)[:, None] - np.uint64(1), (batch, 2, len(sy.q), n)).copy()
    else:
        ct = K.uniform(g, sy.q, n, (batch, 2))
    pts, pt0 = diagonals(g, sy.q, n, nrot, batch, shared, top)
    return sy, exps, ct, pts, pt0


def case_synthetic(fhe, dev, q, n, nrot, batch, seed, top=False, shared=True, exps=None, rot_split=0, with0=True):
    """Uniform synthetic keys, random odd exponents: every word against hoistmv_ref."""
    x = Xfer(dev)
    sy, exps, ct, pts, pt0 = synthetic(fhe, q, n, nrot, batch, seed, top, shared, exps)
    pt0 = pt0 if with0 else None
    assert sy.set.set_rot_split(rot_split).rot_split() == rot_split
    got = run(x, sy.set, exps, ct, pts, pt0)
    same(got, reference(_octx(sy), ct, [sy.oracle_key(r) for r in range(nrot)], exps, pts, pt0), ("hoistmv_ref", n, nrot, batch))
    return sy, exps, ct, pts, pt0, got


def _octx(sy):
    sy.oracle_key(0)
    return sy.octx


def case_table_boundary(fhe, dev):
    """R = table size + 1 at N = 16, batch 2: two launches on one W, their partial sums added."""
    q = obfv.generate_moduli(SMALL[1], SMALL[0])
    case_synthetic(fhe, dev, q, SMALL[0], TABLE + 1, 2, seed=207, shared=False)


MV_FAMILIES = ("hoist_matvec_kernel", "hoist_mac_kernel", "mbfv_sum_kernel", "ks_ntt_kernel", "ks_mac", "ks_fused", "dot_kernel")


def launches(fhe, call):
    """{kernel family: launches} inside call(), from the engine's profiler."""
    symbols = []
    fhe.prof_reset()
    fhe.prof_enable(True)
    try:
        call()
    finally:
        fhe.prof_enable(False)
    count = {}
    for _, sym, n, _ in fhe.prof_entries():
        if n:
            symbols.append(sym)
        for fam in MV_FAMILIES:
            if fam in sym:
                count[fam] = count.get(fam, 0) + n
    fhe.prof_reset()
    return count, symbols


def assert_launches(count, symbols, pairs, nrot, groups_per_launch):
    """Stage A once per (chunk, key-modulus group); the fused stage B once per (pair, table of rotations); the summing
    kernel exactly when the call has more than one group; nothing of the composition."""
    tables = -(-nrot // TABLE)
    assert count.get("ks_ntt_kernel") == pairs, (count, symbols)
    assert count.get("hoist_matvec_kernel") == pairs * tables, (count, symbols)
    assert count.get("mbfv_sum_kernel", 0) == (1 if groups_per_launch > 1 or tables > 1 else 0), (count, symbols)
    for fam in ("hoist_mac_kernel", "ks_mac", "ks_fused", "dot_kernel"):
        assert fam not in count, (fam, symbols)


def case_rot_split(fhe, dev, profiled=False):
    """R = 5 at N = 16, batch 2 under rot_split 0, 1, 2, 3 (groups of 2, 2, 1) and 9 (clamped to 5): identical words,
    equal to hoistmv_ref; `profiled`: the launches counted."""
    x = Xfer(dev)
    n, sizes = SMALL
    q = obfv.generate_moduli(sizes, n)
    sy, exps, ct, pts, pt0, first = case_synthetic(fhe, dev, q, n, 5, 2, seed=211)
    for split, groups in ((0, None), (1, 1), (2, 2), (3, 3), (9, 5)):
        assert sy.set.set_rot_split(split).rot_split() == split
        box = {}
        call = lambda: box.setdefault("got", run(x, sy.set, exps, ct, pts, pt0))   # noqa: E731
        if profiled:
            count, symbols = launches(fhe, call)
            if groups is not None:
                assert_launches(count, symbols, 1, 5, groups)
            else:   # the rule: whatever it picks, the summing kernel runs exactly when it cut the launch
                assert count.get("hoist_matvec_kernel") == 1 and "hoist_mac_kernel" not in count, (count, symbols)
        else:
            call()
        same(box["got"], first, ("rot_split", split))
    sy.set.set_rot_split(0)


def case_w_budget(fhe, dev, profiled=False):
    """N = 16, batch 5, R = 3 under hoist_cases.case_w_budget's budget (chunks of two ciphertexts, groups of one key
    modulus) with rot_split 1 and 2, against the default budget's words."""
    x = Xfer(dev)
    n, sizes = SMALL
    q = obfv.generate_moduli(sizes, n)
    budget = 2 * 3 * n * 8
    assert K.chunk_rule(5, 3, 3, n, budget) == (2, 1)
    sy, exps, ct, pts, pt0, first = case_synthetic(fhe, dev, q, n, 3, 5, seed=213, shared=False)
    assert sy.set.set_w_budget(budget).w_budget() == budget
    for split in (1, 2):
        sy.set.set_rot_split(split)
        box = {}
        call = lambda: box.setdefault("got", run(x, sy.set, exps, ct, pts, pt0))   # noqa: E731
        if profiled:
            count, symbols = launches(fhe, call)
            assert_launches(count, symbols, 3 * 3, 3, split)
        else:
            call()
        same(box["got"], first, ("W budget", split))
    sy.set.set_w_budget(0).set_rot_split(0)


def case_large(fhe, dev, q, n, nrot, batch, seed, w_budget=0, rot_split=0, shared=True):
    """A size the oracle is too slow for: every word against the composition of the two existing engine calls (each with
    its own oracle tests), the launches counted from the profiler.  Returns the symbols."""
    x = Xfer(dev)
    sy, exps, ct, pts, pt0 = synthetic(fhe, q, n, nrot, batch, seed, shared=shared)
    L = len(sy.q)
    sy.set.set_w_budget(w_budget).set_rot_split(rot_split)
    ind, pd, p0d = x.to(ct), x.to(pts), x.to(pt0)
    box = {}
    count, symbols = launches(fhe, lambda: box.setdefault("got", sy.set.matvec_hoisted(exps, ind, pd, p0d)))
    got = x.back(box["got"])
    pc, jg = K.chunk_rule(batch, L, L, n, w_budget)
    pairs = -(-batch // pc) * -(-L // jg)
    assert count.get("ks_ntt_kernel") == pairs, (count, symbols)
    assert count.get("hoist_matvec_kernel") == pairs * -(-nrot // TABLE), (count, symbols)
    assert count.get("mbfv_sum_kernel", 0) <= 1, (count, symbols)
    if rot_split == 1 and nrot <= TABLE:
        assert "mbfv_sum_kernel" not in count, (count, symbols)
    for fam in ("hoist_mac_kernel", "ks_mac", "ks_fused", "dot_kernel"):
        assert fam not in count, (fam, symbols)
    sy.set.set_w_budget(0).set_rot_split(0)
    same(got, composition(sy.set, sy.ctx, exps, ct, pts, pt0), ("composition", n, batch, nrot))
    return symbols


# ---- refusals ------------------------------------------------------------------------------------------------------------
def case_refusals(fhe, dev):
    """Status, fhe_last_error text and an untouched `out` for every refusal; the empty batch; a repeated exponent."""
    n, sizes = SMALL
    opar, par = K.params(fhe, n, sizes)
    cs = K.Clients(fhe, opar, par, 1, 217)
    exps = [3, 9]
    _, gks = cs.galois_keys(exps)
    ks = fhe.KeySet([g.ksk for g in gks[0]])
    L = 3
    PLB = L * n * 8
    mark = np.full((2, 2, L, n), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)   # twice the output: room for overlapping operands
    out = fhe.DeviceArray.from_numpy(mark)
    ct = fhe.DeviceArray.from_numpy(np.zeros((1, 2, L, n), dtype=np.uint64))
    pts = fhe.DeviceArray.from_numpy(np.zeros((2, L, n), dtype=np.uint64))
    pt0 = fhe.DeviceArray.from_numpy(np.zeros((L, n), dtype=np.uint64))
    po, pc, pp, p0 = (C.c_void_p(a.data_ptr()) for a in (out, ct, pts, pt0))
    ex = (C.c_size_t * 2)(*exps)
    name = "fhe_bfv_matvec_hoisted_dev"

    def refused(args, code, text):
        st, msg = K.raw(fhe, name, *args)
        assert st == code and text in msg, (args, st, msg)
        same(out.download(), mark, ("out was written by a refused call", text))

    refused((None, ex, 2, pc, pp, 1, p0, po, 1, None), -1, "null argument: gks")
    refused((ks._h, None, 2, pc, pp, 1, p0, po, 1, None), -1, "null argument: exponents")
    refused((ks._h, ex, 1, pc, pp, 1, p0, po, 1, None), -1, "1 exponents for a set of 2 keys")
    refused((ks._h, ex, 3, pc, pp, 1, p0, po, 1, None), -1, "3 exponents for a set of 2 keys")
    refused((ks._h, (C.c_size_t * 2)(3, 4), 2, pc, pp, 1, p0, po, 1, None), -10, "InvalidSubstitutionExponent")
    refused((ks._h, (C.c_size_t * 2)(3, 2 * n), 2, pc, pp, 1, p0, po, 0, None), -10, "InvalidSubstitutionExponent")
    refused((ks._h, ex, 2, None, pp, 1, p0, po, 1, None), -1, "null argument: ct")
    refused((ks._h, ex, 2, pc, None, 1, p0, po, 1, None), -1, "null argument: pts")
    refused((ks._h, ex, 2, pc, pp, 1, p0, None, 1, None), -1, "null argument: out")
    # `out` overlapping an operand: the operand starting inside the output, and the output starting inside the operand
    inside = C.c_void_p(out.data_ptr() + PLB)
    refused((ks._h, ex, 2, inside, pp, 1, p0, po, 1, None), -1, "`out` overlaps `ct`")
    refused((ks._h, ex, 2, po, pp, 1, p0, inside, 1, None), -1, "`out` overlaps `ct`")
    refused((ks._h, ex, 2, pc, inside, 1, p0, po, 1, None), -1, "`out` overlaps `pts`")
    refused((ks._h, ex, 2, pc, po, 1, p0, inside, 1, None), -1, "`out` overlaps `pts`")
    refused((ks._h, ex, 2, pc, pp, 1, inside, po, 1, None), -1, "`out` overlaps `pt0`")
    refused((ks._h, ex, 2, pc, pp, 1, po, C.c_void_p(out.data_ptr() + PLB // 2), 1, None), -1, "`out` overlaps `pt0`")
    # keys above the ciphertext's level (ciphertexts at level 1, keys at level 0)
    _, up = cs.galois_keys(exps, 1, 0)
    above = fhe.KeySet([g.ksk for g in up[0]])
    refused((above._h, ex, 2, pc, pp, 1, p0, po, 1, None), -1,
            "the keys must sit at the ciphertext's level (2 moduli), not above it (3)")
    with pytest.raises(fhe.FheError) as err:
        above.matvec_hoisted(exps, Xfer(dev).to(np.zeros((1, 2, 2, n), dtype=np.uint64)),
                             Xfer(dev).to(np.zeros((2, 2, n), dtype=np.uint64)))
    assert err.value.code == -1 and "at the ciphertext's level" in str(err.value)
    with pytest.raises(fhe.FheError) as err:
        ks.matvec_hoisted(exps, Xfer(dev).to(np.zeros((1, 3, L, n), dtype=np.uint64)), Xfer(dev).to(np.zeros((2, L, n), dtype=np.uint64)))
    assert err.value.code == -13
    # the option's own refusals
    g = C.c_size_t(7)
    assert K.raw(fhe, "fhe_kskset_get_rot_split", ks._h, C.byref(g)) == (0, "") and g.value == 0
    assert K.raw(fhe, "fhe_kskset_set_rot_split", None, 1)[0] == -1 and K.raw(fhe, "fhe_kskset_get_rot_split", ks._h, None)[0] == -1
    # the empty batch: a no-op with NULL buffers; a repeated exponent is no refusal
    assert K.raw(fhe, name, ks._h, ex, 2, None, None, 1, None, None, 0, None) == (0, "")
    assert K.raw(fhe, name, ks._h, (C.c_size_t * 2)(1, 1), 2, pc, pp, 1, None, po, 1, None) == (0, "")
