"""Cases of the baby-step/giant-step hoisted matrix-vector product (fhe_bfv_matvec_bsgs_dev; KeySet.matvec_bsgs,
EvaluationKey.bsgs, BsgsRotations.matvec).  Shared by tests/test_bsgs_emu.py (kernel sources under host emulation) and
tests/test_bsgs_gpu.py (the HIP build).  `dev`: as helpers.Xfer.

Two references: the restatement tests/bsgs_ref.py (Python ints on hoistmv_ref's sums and hoist_ref's rotations), and the
engine's own composition -- G KeySet.matvec_hoisted calls, one-key KeySet.relinearize_hoisted calls and Context.add --
which the call must equal word for word."""
import ctypes as C

import numpy as np
import pytest

import bsgs_ref
import hoist_cases as H
import keyed_cases as K
from fhe_oracle import bfv as obfv
from fhe_oracle.rq import NTT, Poly
from helpers import Xfer, ct_arr

TABLE = H.TABLE
SMALL = H.SMALL
same = K.same


def reference(octx, ct, obaby, bexps, ogiant, gexps, pts):
    """bsgs_ref over a batch: ct [batch, 2, L, N]; pts [G, B, L, N] or [batch, G, B, L, N]."""
    out = []
    for b, c in enumerate(ct):
        c0, c1 = (Poly(octx, NTT, part.tolist()) for part in c)
        p = pts if pts.ndim == 4 else pts[b]
        o0, o1 = bsgs_ref.matvec(c0, c1, obaby, bexps, ogiant, gexps, p.tolist())
        out.append(np.array([o0, o1], dtype=np.uint64))
    return np.stack(out)


def composition(fhe, ctx, baby, bexps, giant_keys, gexps, ct, pts):
    """The specification on host arrays through the engine's existing calls."""
    L, n = ct.shape[-2:]
    inner = [baby.matvec_hoisted(bexps, ct, np.ascontiguousarray(pts[..., g, 1:, :, :]), np.ascontiguousarray(pts[..., g, 0, :, :]))
             for g in range(len(gexps) + 1)]
    out = inner[0]
    for g, e in enumerate(gexps):
        turned = fhe.KeySet([giant_keys[g]]).relinearize_hoisted([e], inner[g + 1])[:, 0]
        out = ctx.add(out.reshape(-1, L, n), np.ascontiguousarray(turned).reshape(-1, L, n)).reshape(ct.shape)
    return out


def grid(rng, q, n, G, B, batch, shared, top=False):
    """pts: uniform words (`top`: q_j - 1), [G, B, L, N] shared by the batch or one grid per item."""
    lead = () if shared else (batch,)
    if top:
        row = np.array(q, dtype=np.uint64)[:, None] - np.uint64(1)
        return np.broadcast_to(row, lead + (G, B, len(q), n)).copy()
    return K.uniform(rng, q, n, lead + (G, B))


def run(x, baby, bexps, giant, gexps, ct, pts):
    return x.back(baby.matvec_bsgs(bexps, giant, gexps, x.to(ct), x.to(pts)))


# ---- real keys from the oracle ---------------------------------------------------------------------------------------------
def case_anchor(fhe, dev, cl=0, kl=0, bexps=(1, 9), gexps=(3, 3), batch=2, seed=301, variants=(True, False), flat=False):
    """N = 16 over [62, 60, 55], nbaby = ngiant = 2, exponents including 1 and a repeat: shared and per-item grids, every
    word against bsgs_ref and against the engine's composition.  `flat`: also against fhe_bfv_matvec_hoisted_dev over
    the G B - 1 composed exponents and the giant-substituted diagonals, which must differ in a word."""
    x = Xfer(dev)
    opar, par = K.params(fhe, *SMALL)
    n = opar.degree()
    cs = K.Clients(fhe, opar, par, 1, seed)
    bexps, gexps = list(bexps), list(gexps)
    obk, bks = cs.galois_keys(bexps, cl, kl)
    ogk, gks = cs.galois_keys(gexps, cl, kl)
    obk, bks, ogk, gks = obk[0], bks[0], ogk[0], gks[0]
    cts = [cs.encrypt(0, cl) for _ in range(batch)]
    inp = np.stack([ct_arr(c) for c in cts])
    baby, giant = fhe.KeySet([g.ksk for g in bks]), fhe.KeySet([g.ksk for g in gks])
    octx, ctx = opar.context_at_level(cl), par.context_at_level(cl)
    q = [int(m) for m in octx.moduli]
    g = np.random.default_rng(seed)
    G, B = len(gexps) + 1, len(bexps) + 1
    for shared in variants:
        pts = grid(g, q, n, G, B, batch, shared)
        got = run(x, baby, bexps, giant, gexps, inp, pts)
        assert got.shape == inp.shape
        same(got, reference(octx, inp, [obk[e].ksk for e in bexps], bexps, [ogk[e].ksk for e in gexps], gexps, pts),
             ("bsgs_ref", shared, cl))
        same(got, composition(fhe, ctx, baby, bexps, [k.ksk for k in gks], gexps, inp, pts), ("composition", shared, cl))
        if not flat:
            continue
        # the flat product: exponent e_g e_b per diagonal, the diagonal of group g >= 1 turned by its giant
        one = [1] + bexps
        comp = [(gi, bi, (eg * eb) % (2 * n)) for gi, eg in enumerate([1] + gexps) for bi, eb in enumerate(one)][1:]
        _, fks = cs.galois_keys(sorted({e for _, _, e in comp}), cl, kl)
        by_e = {k.exponent: k for k in fks[0]}
        fset = fhe.KeySet([by_e[e].ksk for _, _, e in comp])
        p = pts if shared else pts[0]
        turned = [p[gi, bi] if gi == 0 else ctx.substitute(gexps[gi - 1], p[gi, bi][None], ntt=True)[0] for gi, bi, _ in comp]
        one_ct = inp[:1]
        fl = fset.matvec_hoisted([e for _, _, e in comp], one_ct, np.stack(turned), np.ascontiguousarray(p[0, 0]))
        # (uniform diagonal words drown the plaintext, so nothing is decrypted here: case_matrix_vector decrypts both)
        K.differ(got[:1], fl, "a build that routes to the flat call would give the flat call's words")


def case_forms(fhe, dev, seed=303):
    """EvaluationKey.bsgs(2, 2): its keys and exponents, a result of the input's kind, one ciphertext without a batch
    dimension, shapes refused, a missing key."""
    x = Xfer(dev)
    opar, par = K.params(fhe, *SMALL)
    n = opar.degree()
    cs = K.Clients(fhe, opar, par, 1, seed)
    exps = [pow(3, 1, 2 * n), pow(3, 2, 2 * n)]
    _, gks = cs.galois_keys(exps)
    ek = fhe.EvaluationKey(n, gks[0])
    h = ek.bsgs(2, 2)
    assert h.baby_exponents == [exps[0]] and h.giant_exponents == [exps[1]] and h.shape == (2, 2)
    inp = np.stack([ct_arr(cs.encrypt(0)) for _ in range(2)])
    ctx = par.context_at_level(0)
    q = [int(m) for m in opar.context_at_level(0).moduli]
    pts = grid(np.random.default_rng(seed), q, n, 2, 2, 2, True)
    want = composition(fhe, ctx, h.baby, h.baby_exponents, [k.ksk for k in h.giant_keys], h.giant_exponents, inp, pts)
    out = h.matvec(x.to(inp), x.to(pts))
    assert type(out) is type(x.to(inp))
    same(x.back(out), want, "BsgsRotations.matvec")
    one = x.back(h.matvec(x.to(inp[1]), x.to(pts)))
    assert one.shape == inp.shape[1:]
    same(one, want[1], "one ciphertext")
    for bad in (pts[:1], pts[:, :1], np.concatenate([pts, pts], axis=1), np.stack([pts] * 3)):
        with pytest.raises(fhe.FheError) as err:
            h.matvec(x.to(inp), x.to(np.ascontiguousarray(bad)))
        assert err.value.code == -1 and "DotProductLengthMismatch" in str(err.value)
    with pytest.raises(fhe.FheError) as err:
        ek.bsgs(2, 3)          # giants 2 and 4: no key for 4
    assert err.value.code == -11 and "Unsupported(ColumnRotation)" in str(err.value)
    with pytest.raises(fhe.FheError) as err:
        ek.bsgs(4, 4)          # giant step 8 = N / 2
    assert err.value.code in (-1, -11)


def case_matrix_vector(fhe, dev, seed=127):
    """hoistmv_cases.case_matrix_vector's 4 x 4 matrix at N = 16 as B = 2 x G = 2 -- one baby key (step 1), one giant key
    (step 2) -- the diagonals pre-rotated in the slot domain, through KeySet.matvec_bsgs and EvaluationKey.bsgs(2, 2):
    decrypted and decoded, against numpy modulo t.  Prints the measured noise of this result and of the flat call's."""
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
    B, G = 2, 2
    # diagonal i = g B + b, slot k: M[k][k + i step]; the caller's pre-rotation rot_{-gB}: slot k takes slot k - g B step
    # (d divides the row length, so the index arithmetic may stay modulo d)
    diag = np.stack([np.stack([np.array([M[(k - gi * B * step) % d][(k - gi * B * step + (gi * B + bi) * step) % d] for k in range(n)],
                                        dtype=np.uint64) for bi in range(B)]) for gi in range(G)])
    pts = np.asarray(enc.encode(diag.reshape(G * B, n))).reshape((G, B) + (len(sizes), n))
    want = (M.astype(object) @ v.astype(object)) % t
    expect = [int(want[k % d]) for k in range(n)]
    h = ek.bsgs(B, G)
    for what, prod in (("BsgsRotations.matvec", h.matvec(x.to(ct), x.to(pts))),
                       ("KeySet.matvec_bsgs", h.baby.matvec_bsgs(h.baby_exponents, h.giant, h.giant_exponents, x.to(ct), x.to(pts)))):
        res = x.back(prod)
        assert [int(a) for a in enc.decode(sk.decrypt(res))[0]] == expect, (what, want)
    flat_diag = np.stack([np.array([M[k % d][(k + i * step) % d] for k in range(n)], dtype=np.uint64) for i in range(d)])
    fp = np.asarray(enc.encode(flat_diag))
    flat = x.back(ek.hoisted(column_rotations=(1, 2, 3)).matvec(x.to(ct), x.to(np.ascontiguousarray(fp[1:])),
                                                                 x.to(np.ascontiguousarray(fp[0]))))
    assert [int(a) for a in enc.decode(sk.decrypt(flat))[0]] == expect
    print("noise bits: bsgs 2 x 2 %s, flat R = 3 %s, fresh %s" % (sk.measure_noise(res), sk.measure_noise(flat), sk.measure_noise(ct)))


# ---- synthetic keys --------------------------------------------------------------------------------------------------------
class Sets:
    """One keyed_cases.Synthetic of nbaby + ngiant keys, two KeySets cut from it, inputs and a grid of diagonals."""

    def __init__(self, fhe, q, n, nbaby, ngiant, batch, seed, top=False, shared=True):
        self.fhe = fhe
        self.sy = sy = K.Synthetic(fhe, q, n, nbaby + ngiant, seed, top)
        self.nbaby, self.ngiant = nbaby, ngiant
        exps = H.odd_exponents(n, nbaby + ngiant, seed)
        self.bexps, self.gexps = exps[:nbaby], exps[nbaby:]
        self.baby, self.giant = fhe.KeySet(sy.keys[:nbaby]), fhe.KeySet(sy.keys[nbaby:])
        g = np.random.default_rng(seed + 1000)
        if top:
            self.ct = np.broadcast_to(np.array(sy.q, dtype=np.uint64)[:, None] - np.uint64(1), (batch, 2, len(sy.q), n)).copy()
        else:
            self.ct = K.uniform(g, sy.q, n, (batch, 2))
        self.pts = grid(g, sy.q, n, ngiant + 1, nbaby + 1, batch, shared, top)

    def run(self, x):
        return run(x, self.baby, self.bexps, self.giant, self.gexps, self.ct, self.pts)

    def reference(self):
        ok = [self.sy.oracle_key(r) for r in range(self.nbaby + self.ngiant)]
        return reference(self.sy.octx, self.ct, ok[:self.nbaby], self.bexps, ok[self.nbaby:], self.gexps, self.pts)

    def composition(self):
        return composition(self.fhe, self.sy.ctx, self.baby, self.bexps, self.sy.keys[self.nbaby:], self.gexps, self.ct, self.pts)


def case_synthetic(fhe, dev, q, n, nbaby, ngiant, batch, seed, top=False, shared=True, tile=0, rot_split=0):
    """Uniform synthetic keys, random odd exponents: every word against bsgs_ref."""
    s = Sets(fhe, q, n, nbaby, ngiant, batch, seed, top, shared)
    assert s.baby.set_bsgs_tile(tile).bsgs_tile() == tile
    s.giant.set_rot_split(rot_split)
    got = s.run(Xfer(dev))
    same(got, s.reference(), ("bsgs_ref", n, nbaby, ngiant, batch, tile, rot_split))
    return s, got


FAMILIES = ("bsgs_baby_kernel", "bsgs_giant_kernel", "mbfv_sum_kernel", "ks_ntt_kernel", "hoist_matvec_kernel", "hoist_mac_kernel",
            "ks_mac", "ks_fused", "dot_kernel")
NEVER = ("hoist_matvec_kernel", "hoist_mac_kernel", "ks_mac", "ks_fused", "dot_kernel")


def launches(fhe, call):
    """({kernel family: launches}, symbols) inside call(), from the engine's profiler."""
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
        for fam in FAMILIES:
            if fam in sym:
                count[fam] = count.get(fam, 0) + n
    fhe.prof_reset()
    return count, symbols


def assert_launches(count, symbols, baby_pairs, giant_pairs, summed=None):
    """Two passes' worth of stage A; one baby and one giant stage B per W; the summing kernel exactly when the giants were
    cut (`summed`; None: at most once); nothing of the composition or the flat call."""
    assert count.get("ks_ntt_kernel") == baby_pairs + giant_pairs, (count, symbols)
    assert count.get("bsgs_baby_kernel") == baby_pairs, (count, symbols)
    assert count.get("bsgs_giant_kernel") == giant_pairs, (count, symbols)
    if summed is None:
        assert count.get("mbfv_sum_kernel", 0) <= 1, (count, symbols)
    else:
        assert count.get("mbfv_sum_kernel", 0) == (1 if summed else 0), (count, symbols)
    for fam in NEVER:
        assert fam not in count, (fam, symbols)


def baby_instances(symbols):
    return sorted({s[s.index("bsgs_baby_kernel<") + 17:].split(">")[0] for s in symbols if "bsgs_baby_kernel<" in s})


def case_tiles(fhe, dev, ngiant, profiled=False):
    """N = 16, batch 2, nbaby = 2 under bsgs_tile 0, 1, 2, 4: identical words, equal to bsgs_ref.  G = 3: GT = 2 with a
    one-group tail, GT = 4 as one cut tile; G = 5: GT = 4 as 4 + 1.  `profiled`: the launched instance read from the symbols
    (at this size the rule says 1)."""
    x = Xfer(dev)
    n, sizes = SMALL
    q = obfv.generate_moduli(sizes, n)
    s, first = case_synthetic(fhe, dev, q, n, 2, ngiant, 2, seed=305 + ngiant, shared=False)
    for tile in (0, 1, 2, 4):
        assert s.baby.set_bsgs_tile(tile).bsgs_tile() == tile
        box = {}
        call = lambda: box.setdefault("got", s.run(x))   # noqa: E731
        if profiled:
            count, symbols = launches(fhe, call)
            assert_launches(count, symbols, 1, 1)
            assert baby_instances(symbols) == [str(tile or 1)], symbols
        else:
            call()
        same(box["got"], first, ("bsgs_tile", tile, ngiant))
    s.baby.set_bsgs_tile(0)


def case_giant_groups(fhe, dev, profiled=False):
    """ngiant = 5, nbaby = 1 at N = 16, batch 2 under the giant set's rot_split 0, 1, 2, 3 (groups of 2, 2, 1) and 9
    (clamped to 5): identical words, equal to bsgs_ref; `profiled`: mbfv_sum_kernel exactly when the call has more than one
    group."""
    x = Xfer(dev)
    n, sizes = SMALL
    q = obfv.generate_moduli(sizes, n)
    s, first = case_synthetic(fhe, dev, q, n, 1, 5, 2, seed=311)
    for split, groups in ((0, None), (1, 1), (2, 2), (3, 3), (9, 5)):
        assert s.giant.set_rot_split(split).rot_split() == split
        box = {}
        call = lambda: box.setdefault("got", s.run(x))   # noqa: E731
        if profiled:
            count, symbols = launches(fhe, call)
            assert_launches(count, symbols, 1, 1, None if groups is None else groups > 1)
        else:
            call()
        same(box["got"], first, ("giant rot_split", split))
    s.giant.set_rot_split(0)


def case_w_budget(fhe, dev, profiled=False):
    """N = 16, batch 5, nbaby = ngiant = 2: the baby set under a budget of two ciphertexts at one key modulus, the giant set
    under one ciphertext's giants at one key modulus (a giant chunk holds whole ciphertexts), against the default budget's
    words."""
    x = Xfer(dev)
    n, sizes = SMALL
    q = obfv.generate_moduli(sizes, n)
    nd = lk = len(q)
    ngiant = 2
    bbudget, gbudget = 2 * nd * n * 8, ngiant * nd * n * 8
    assert K.chunk_rule(5, nd, lk, n, bbudget) == (2, 1)
    assert K.chunk_rule(5, nd * ngiant, lk, n, gbudget) == (1, 1)            # (a ciphertext costs its ngiant items)
    assert K.chunk_rule(5, nd * ngiant, lk, n, gbudget // 2) == (1, 1)       # (below one ciphertext's giants: still one)
    s, first = case_synthetic(fhe, dev, q, n, 2, ngiant, 5, seed=313, shared=False)
    for gb, split in ((gbudget, 1), (gbudget // 2, 2)):
        assert s.baby.set_w_budget(bbudget).w_budget() == bbudget and s.giant.set_w_budget(gb).w_budget() == gb
        s.giant.set_rot_split(split)
        box = {}
        call = lambda: box.setdefault("got", s.run(x))   # noqa: E731
        if profiled:
            count, symbols = launches(fhe, call)
            assert_launches(count, symbols, 3 * 3, 5 * 3, split > 1)
        else:
            call()
        same(box["got"], first, ("W budget", gb, split))
    s.baby.set_w_budget(0)
    s.giant.set_w_budget(0).set_rot_split(0)


def case_table_limits(fhe, dev):
    """nbaby = 64 and ngiant = 64 at N = 16 -- 65 x 65 diagonals, the most one call takes -- against the engine's
    composition; 65 of either is refused."""
    n, sizes = SMALL
    q = obfv.generate_moduli(sizes, n)
    s = Sets(fhe, q, n, TABLE, TABLE, 1, seed=317)
    same(s.run(Xfer(dev)), s.composition(), "65 x 65 diagonals")
    keys = s.sy.keys
    more = fhe.KeySet(keys[:TABLE] + keys[:1])
    few = fhe.KeySet(keys[:1])
    ct = Xfer(dev).to(s.ct)
    for baby, giant in ((more, few), (few, more)):
        nb, ng = len(baby), len(giant)
        pts = Xfer(dev).to(np.zeros((ng + 1, nb + 1, len(q), n), dtype=np.uint64))
        with pytest.raises(fhe.FheError) as err:
            baby.matvec_bsgs([3] * nb, giant, [3] * ng, ct, pts)
        assert err.value.code == -1 and "at most 64 baby and 64 giant rotations" in str(err.value)


def case_large(fhe, dev, q, n, nbaby, ngiant, batch, seed, tile=0, shared=True):
    """A size the oracle is too slow for: every word against the engine's composition (each of its calls has its own
    oracle tests), the launches counted from the profiler.  Returns the symbols."""
    x = Xfer(dev)
    s = Sets(fhe, q, n, nbaby, ngiant, batch, seed, shared=shared)
    s.baby.set_bsgs_tile(tile)
    ind, pd = x.to(s.ct), x.to(s.pts)
    box = {}
    count, symbols = launches(fhe, lambda: box.setdefault("got", s.baby.matvec_bsgs(s.bexps, s.giant, s.gexps, ind, pd)))
    got = x.back(box["got"])
    assert_launches(count, symbols, 1, 1)
    if tile:
        assert baby_instances(symbols) == [str(tile)], symbols
    s.baby.set_bsgs_tile(0)
    same(got, s.composition(), ("composition", n, batch, nbaby, ngiant))
    return symbols


# ---- refusals --------------------------------------------------------------------------------------------------------------
def case_refusals(fhe, dev):
    """Status, fhe_last_error text and an untouched `out` for every refusal; the empty batch; the option's own refusals."""
    n, sizes = SMALL
    opar, par = K.params(fhe, n, sizes)
    cs = K.Clients(fhe, opar, par, 1, 319)
    bexps, gexps = [3, 9], [27]
    _, bks = cs.galois_keys(bexps)
    _, gks = cs.galois_keys(gexps)
    baby, giant = fhe.KeySet([g.ksk for g in bks[0]]), fhe.KeySet([g.ksk for g in gks[0]])
    L = 3
    PLB = L * n * 8
    mark = np.full((2, 2, L, n), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)   # twice the output: room for overlapping operands
    out = fhe.DeviceArray.from_numpy(mark)
    ct = fhe.DeviceArray.from_numpy(np.zeros((2, 2, L, n), dtype=np.uint64))
    pts = fhe.DeviceArray.from_numpy(np.zeros((2, 3, L, n), dtype=np.uint64))
    po, pc, pp = (C.c_void_p(a.data_ptr()) for a in (out, ct, pts))
    bx, gx = (C.c_size_t * 2)(*bexps), (C.c_size_t * 1)(*gexps)
    name = "fhe_bfv_matvec_bsgs_dev"

    def refused(args, code, text):
        st, msg = K.raw(fhe, name, *args)
        assert st == code and text in msg, (args, st, msg)
        same(out.download(), mark, ("out was written by a refused call", text))

    B, G = baby._h, giant._h
    refused((None, bx, 2, G, gx, 1, pc, pp, 1, po, 1, None), -1, "null argument: baby")
    refused((B, None, 2, G, gx, 1, pc, pp, 1, po, 1, None), -1, "null argument: baby_exps")
    refused((B, bx, 2, None, gx, 1, pc, pp, 1, po, 1, None), -1, "null argument: giant")
    refused((B, bx, 2, G, None, 1, pc, pp, 1, po, 1, None), -1, "null argument: giant_exps")
    refused((B, bx, 1, G, gx, 1, pc, pp, 1, po, 1, None), -1, "1 baby exponents for a set of 2 keys")
    refused((B, bx, 2, G, gx, 2, pc, pp, 1, po, 1, None), -1, "2 giant exponents for a set of 1 keys")
    refused((B, bx, 2, G, gx, 1, None, pp, 1, po, 1, None), -1, "null argument: ct")
    refused((B, bx, 2, G, gx, 1, pc, None, 1, po, 1, None), -1, "null argument: pts")
    refused((B, bx, 2, G, gx, 1, pc, pp, 1, None, 1, None), -1, "null argument: out")
    # `out` overlapping an operand: the operand starting inside the output, and the output starting inside the operand
    inside = C.c_void_p(out.data_ptr() + PLB)
    refused((B, bx, 2, G, gx, 1, inside, pp, 1, po, 1, None), -1, "`out` overlaps `ct`")
    refused((B, bx, 2, G, gx, 1, po, pp, 1, inside, 1, None), -1, "`out` overlaps `ct`")
    refused((B, bx, 2, G, gx, 1, pc, inside, 1, po, 1, None), -1, "`out` overlaps `pts`")
    refused((B, bx, 2, G, gx, 1, pc, po, 1, inside, 1, None), -1, "`out` overlaps `pts`")
    # a buffer not 16-byte aligned: each of the three
    off = lambda a: C.c_void_p(a.data_ptr() + 8)   # noqa: E731
    refused((B, bx, 2, G, gx, 1, off(ct), pp, 1, po, 1, None), -1, "16-byte aligned")
    refused((B, bx, 2, G, gx, 1, pc, off(pts), 1, po, 1, None), -1, "16-byte aligned")
    spare = fhe.DeviceArray.from_numpy(np.zeros((2, 2, L, n), dtype=np.uint64))
    refused((B, bx, 2, G, gx, 1, pc, pp, 1, off(spare), 1, None), -1, "16-byte aligned")
    # an even exponent in either list
    refused((B, (C.c_size_t * 2)(3, 4), 2, G, gx, 1, pc, pp, 1, po, 1, None), -10, "InvalidSubstitutionExponent")
    refused((B, bx, 2, G, (C.c_size_t * 1)(2 * n), 1, pc, pp, 1, po, 1, None), -10, "InvalidSubstitutionExponent")
    # either set's keys above the ciphertext's level (ciphertexts at level 1, keys at level 0)
    _, ub = cs.galois_keys(bexps, 1, 0)
    _, ug = cs.galois_keys(gexps, 1, 0)
    ab, ag = fhe.KeySet([g.ksk for g in ub[0]]), fhe.KeySet([g.ksk for g in ug[0]])
    refused((ab._h, bx, 2, ag._h, gx, 1, pc, pp, 1, po, 1, None), -1,
            "the keys must sit at the ciphertext's level (2 moduli), not above it (3)")
    # the two sets differ: one a level down on both sides (ring, levels and digit count), then in the ciphertext's ring only
    _, lg = cs.galois_keys(gexps, 1, 1)
    low = fhe.KeySet([g.ksk for g in lg[0]])
    refused((B, bx, 2, low._h, gx, 1, pc, pp, 1, po, 1, None), -11, "the baby and giant sets differ")
    refused((low._h, gx, 1, G, gx, 1, pc, pp, 1, po, 1, None), -11, "the baby and giant sets differ")
    refused((B, bx, 2, ag._h, gx, 1, pc, pp, 1, po, 1, None), -11, "the baby and giant sets differ")
    refused((ab._h, bx, 2, G, gx, 1, pc, pp, 1, po, 1, None), -11, "the baby and giant sets differ")
    with pytest.raises(fhe.FheError) as err:
        baby.matvec_bsgs(bexps, giant, gexps, Xfer(dev).to(np.zeros((1, 3, L, n), dtype=np.uint64)),
                         Xfer(dev).to(np.zeros((2, 3, L, n), dtype=np.uint64)))
    assert err.value.code == -13
    # the option's own refusals
    g = C.c_size_t(7)
    assert K.raw(fhe, "fhe_kskset_get_bsgs_tile", B, C.byref(g)) == (0, "") and g.value == 0
    assert K.raw(fhe, "fhe_kskset_set_bsgs_tile", None, 1)[0] == -1 and K.raw(fhe, "fhe_kskset_get_bsgs_tile", B, None)[0] == -1
    for bad in (3, 5, 8, 64):
        st, msg = K.raw(fhe, "fhe_kskset_set_bsgs_tile", B, bad)
        assert st == -1 and "bsgs tile" in msg, (bad, st, msg)
    assert baby.bsgs_tile() == 0
    for ok in (1, 2, 4, 0):
        assert baby.set_bsgs_tile(ok).bsgs_tile() == ok
    # the empty batch: a no-op with NULL buffers; a repeated exponent is no refusal
    assert K.raw(fhe, name, B, bx, 2, G, gx, 1, None, None, 1, None, 0, None) == (0, "")
    assert K.raw(fhe, name, B, (C.c_size_t * 2)(1, 1), 2, G, (C.c_size_t * 1)(1), 1, pc, pp, 1, po, 1, None) == (0, "")
