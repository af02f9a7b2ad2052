"""Cases of the hoisted rotations (fhe_bfv_galois_hoisted_dev; KeySet.relinearize_hoisted, EvaluationKey.hoisted): many
Galois elements of each ciphertext from one digit decomposition.  Shared by tests/test_hoist_emu.py (kernel sources under
host emulation) and tests/test_hoist_gpu.py (the HIP build).  `dev`: as helpers.Xfer.

The output is NOT GaloisKey::relinearize's words, so every output word is compared with the restatement tests/hoist_ref.py,
which is anchored to the reference at exponent 1 (word for word) and elsewhere by decryption and noise."""
import ctypes as C
import random

import numpy as np
import pytest

import hoist_ref
import keyed_cases as K
from fhe_oracle import bfv as obfv
from fhe_oracle.rq import NTT, Poly
from helpers import Xfer, arr, ct_arr

TABLE = 64   # k::HOIST_ROTS (kernels_kshoist.hpp): rotations per stage-B launch
SMALL = (16, [62, 60, 55])
same, differ = K.same, K.differ


def ref_rotations(octx, ct_words, okeys, exps):
    """hoist_ref over a batch of ciphertext words [batch, 2, L, N] -> [batch, R, 2, L, N]."""
    out = []
    for c in ct_words:
        c0, c1 = (Poly(octx, NTT, part.tolist()) for part in c)
        out.append(np.stack([np.stack([arr(o0), arr(o1)]) for o0, o1 in hoist_ref.hoisted(c0, c1, okeys, exps)]))
    return np.stack(out)


def case_anchor(fhe, dev, cl=0, kl=0, exps=(1, 3, 9, 31, 3), batch=2, seed=101):
    """Real keys from the oracle at N = 16 (a partial workgroup per row): every rotation against hoist_ref; exponent 1
    word for word against the oracle's GaloisKey.relinearize and the single-rotation engine call; every other exponent by
    decryption, by at least one differing word, and by measure_noise <= the oracle rotation's + 2 bits.  Returns the
    noise differences seen."""
    x = Xfer(dev)
    opar, par = K.params(fhe, *SMALL)
    cs = K.Clients(fhe, opar, par, 1, seed)
    ogk, gks = cs.galois_keys(exps, cl, kl)
    ogk, gks = ogk[0], gks[0]
    values = [[cs.rng[0].randrange(opar.plaintext) for _ in range(opar.degree())] for _ in range(batch)]
    cts = [cs.sk[0].encrypt(v, cs.rng[0], cl) for v in values]
    inp = np.stack([ct_arr(c) for c in cts])
    oracle = [[ogk[e].relinearize(c) for e in exps] for c in cts]
    differ(ct_arr(oracle[0][1]), ct_arr(oracle[0][2]), ("two exponents", exps[1], exps[2]))
    ks = fhe.KeySet([g.ksk for g in gks])
    got = x.back(ks.relinearize_hoisted(exps, x.to(inp)))
    assert got.shape == (batch, len(exps)) + inp.shape[1:]
    differ(got[0][1], got[0][2], ("two exponents", exps[1], exps[2]))
    octx = opar.context_at_level(cl)
    same(got, ref_rotations(octx, inp, [ogk[e].ksk for e in exps], exps), ("hoist_ref", cl, kl))
    noise = []
    for b, c in enumerate(cts):
        for r, e in enumerate(exps):
            want = oracle[b][r]
            if e == 1:
                same(got[b][r], ct_arr(want), "exponent 1 against GaloisKey.relinearize")
                same(x.back(gks[r].relinearize(x.to(inp[b]))), got[b][r], "exponent 1 against the single rotation")
                continue
            mine = obfv.Ciphertext(opar, [Poly(octx, NTT, part.tolist()) for part in got[b][r]], cl)
            plain = cs.sk[0].decrypt(want)
            assert cs.sk[0].decrypt(mine) == plain, ("decryption", b, e)
            differ(got[b][r], ct_arr(want), ("a loop of single rotations would give the reference's words", e))
            n_mine, n_ref = cs.sk[0].measure_noise(mine, plain), cs.sk[0].measure_noise(want, plain)
            print("noise: exponent %d ciphertext %d hoisted %d reference %d" % (e, b, n_mine, n_ref))
            assert n_mine <= n_ref + 2, (e, b, n_mine, n_ref)
            noise.append(n_mine - n_ref)
    return noise


def case_forms(fhe, dev, seed=103):
    """KeySet.relinearize_hoisted and EvaluationKey.hoisted(...).rotate on numpy arrays, torch tensors or DeviceArrays:
    the same words, a result of the input's kind, one ciphertext without a batch dimension, a missing key."""
    x = Xfer(dev)
    opar, par = K.params(fhe, *SMALL)
    n = opar.degree()
    cs = K.Clients(fhe, opar, par, 1, seed)
    exps = [pow(3, 1, 2 * n), pow(3, 2, 2 * n), 2 * n - 1]
    ogk, gks = cs.galois_keys(exps)
    ek = fhe.EvaluationKey(n, gks[0])
    h = ek.hoisted(column_rotations=(2, 1), row_rotation=True)
    assert h.exponents == [exps[1], exps[0], exps[2]] and len(h) == 3
    inp = np.stack([ct_arr(cs.encrypt(0)) for _ in range(2)])
    want = ref_rotations(opar.context_at_level(0), inp, [ogk[0][e].ksk for e in h.exponents], h.exponents)
    out = h.rotate(x.to(inp))
    assert type(out) is type(x.to(inp))
    same(x.back(out), want, "EvaluationKey.hoisted.rotate")
    same(x.back(h.set.relinearize_hoisted(h.exponents, x.to(inp))), want, "KeySet.relinearize_hoisted")
    one = x.back(h.rotate(x.to(inp[1])))
    assert one.shape == (3,) + inp.shape[1:]
    same(one, want[1], "one ciphertext")
    for kw, what in ((dict(column_rotations=(3,)), "ColumnRotation"), (dict(row_rotation=True), "RowRotation")):
        with pytest.raises(fhe.FheError) as err:
            fhe.EvaluationKey(n, gks[0][:2]).hoisted(**kw)
        assert err.value.code == -11 and "Unsupported(%s)" % what in str(err.value)
    with pytest.raises(fhe.FheError) as err:
        ek.hoisted(column_rotations=(n // 2,))
    assert err.value.code == -1 and "InvalidRotationStep" in str(err.value)


def odd_exponents(n, count, seed):
    rng = random.Random(seed)
    return [2 * rng.randrange(n) + 1 for _ in range(count)]


def case_synthetic(fhe, dev, q, n, nrot, batch, seed, top=False, check=None, w_budget=None, exps=None):
    """`nrot` distinct synthetic keys (uniform words; `top`: q_j - 1 everywhere, inputs too) and random odd exponents:
    the rotations `check` (default all) of every ciphertext against hoist_ref.  w_budget: the call again under that W
    budget, against the default budget's words."""
    x = Xfer(dev)
    sy = K.Synthetic(fhe, q, n, nrot, seed, top)
    L = len(sy.q)
    exps = list(exps) if exps is not None else odd_exponents(n, nrot, seed)
    if top:
        ct = np.broadcast_to(np.array(sy.q, dtype=np.uint64)[:, None] - np.uint64(1), (batch, 2, L, n)).copy()
    else:
        ct = K.uniform(np.random.default_rng(seed + 1000), sy.q, n, (batch, 2))
    got = x.back(sy.set.relinearize_hoisted(exps, x.to(ct)))
    assert got.shape == (batch, nrot, 2, L, n)
    check = list(range(nrot)) if check is None else list(check)
    okeys = [sy.oracle_key(r) for r in check]
    want = ref_rotations(sy.octx, ct, okeys, [exps[r] for r in check])
    for i, r in enumerate(check):
        same(got[:, r], want[:, i], ("rotation", r, exps[r], n, batch))
    if w_budget is not None:
        assert sy.set.set_w_budget(w_budget).w_budget() == w_budget
        cut = x.back(sy.set.relinearize_hoisted(exps, x.to(ct)))
        assert sy.set.set_w_budget(0).w_budget() == 0
        same(cut, got, "W budget")
    return sy, exps, ct, got


def case_more_rotations_than_a_table(fhe, dev):
    """R = table size + 1 at N = 16, batch 2: two stage-B launches on one W; the first and last rotation of each."""
    q = obfv.generate_moduli(SMALL[1], SMALL[0])
    case_synthetic(fhe, dev, q, SMALL[0], TABLE + 1, 2, seed=107, check=(0, TABLE - 1, TABLE))


def case_w_budget(fhe, dev):
    """N = 16, batch 5, R = 3 under a budget that cuts the batch into chunks of two ciphertexts and the key moduli into
    groups of one."""
    n, sizes = SMALL
    q = obfv.generate_moduli(sizes, n)
    budget = 2 * 3 * n * 8
    assert K.chunk_rule(5, 3, 3, n, budget) == (2, 1) and K.chunk_rule(5, 3, 3, n, 0) == (5, 3)
    case_synthetic(fhe, dev, q, n, 3, 5, seed=109, w_budget=budget)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def case_refusals(fhe, dev):
    """Status, fhe_last_error text and an untouched `out` for every refusal; the empty batch."""
    n, sizes = SMALL
    opar, par = K.params(fhe, n, sizes)
    cs = K.Clients(fhe, opar, par, 1, 113)
    exps = [3, 9]
    _, gks = cs.galois_keys(exps)
    ks = fhe.KeySet([g.ksk for g in gks[0]])
    L = 3
    mark = np.full((1, 2, 2, L, n), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    out = fhe.DeviceArray.from_numpy(mark)
    ct = fhe.DeviceArray.from_numpy(np.zeros((1, 2, L, n), dtype=np.uint64))
    po, pc = C.c_void_p(out.data_ptr()), C.c_void_p(ct.data_ptr())
    ex = (C.c_size_t * 2)(*exps)

    def refused(args, code, text):
        st, msg = K.raw(fhe, "fhe_bfv_galois_hoisted_dev", *args)
        assert st == code and text in msg, (args, st, msg)
        same(out.download(), mark, ("out was written by a refused call", text))

    refused((None, ex, 2, pc, po, 1, None), -1, "null argument: gks")
    refused((ks._h, None, 2, pc, po, 1, None), -1, "null argument: exponents")
    refused((ks._h, ex, 1, pc, po, 1, None), -1, "1 exponents for a set of 2 keys")
    refused((ks._h, ex, 3, pc, po, 1, None), -1, "3 exponents for a set of 2 keys")
    refused((ks._h, (C.c_size_t * 2)(3, 4), 2, pc, po, 1, None), -10, "InvalidSubstitutionExponent")
    refused((ks._h, (C.c_size_t * 2)(3, 2 * n), 2, pc, po, 0, None), -10, "InvalidSubstitutionExponent")
    refused((ks._h, ex, 2, None, po, 1, None), -1, "null argument: ct")
    refused((ks._h, ex, 2, pc, None, 1, None), -1, "null argument: out")
    # `out` overlapping `ct`: the input inside the output block, and the output starting inside the input
    inside = C.c_void_p(out.data_ptr() + 2 * L * n * 8)
    refused((ks._h, ex, 2, inside, po, 1, None), -1, "`out` overlaps `ct`")
    refused((ks._h, ex, 2, po, C.c_void_p(out.data_ptr() + L * n * 8), 1, None), -1, "`out` overlaps `ct`")
    # keys above the ciphertext's level (ciphertexts at level 1, keys at level 0)
    _, up = cs.galois_keys(exps, 1, 0)
    above = fhe.KeySet([g.ksk for g in up[0]])
    refused((above._h, ex, 2, pc, po, 1, None), -1, "the keys must sit at the ciphertext's level (2 moduli), not above it (3)")
    with pytest.raises(fhe.FheError) as err:
        above.relinearize_hoisted(exps, Xfer(dev).to(np.zeros((1, 2, 2, n), dtype=np.uint64)))
    assert err.value.code == -1 and "at the ciphertext's level" in str(err.value)
    with pytest.raises(fhe.FheError) as err:
        ks.relinearize_hoisted(exps, Xfer(dev).to(np.zeros((1, 3, L, n), dtype=np.uint64)))
    assert err.value.code == -13
    # the empty batch: a no-op with NULL buffers; exponent 1 repeated is no refusal
    assert K.raw(fhe, "fhe_bfv_galois_hoisted_dev", ks._h, ex, 2, None, None, 0, None) == (0, "")
    assert K.raw(fhe, "fhe_bfv_galois_hoisted_dev", ks._h, (C.c_size_t * 2)(1, 1), 2, pc, po, 1, None) == (0, "")


# ---- end to end ----------------------------------------------------------------------------------------------------------
def case_matrix_vector(fhe, dev, seed=127):
    """A 4 x 4 plaintext matrix times an encrypted SIMD vector at N = 16 by the diagonal method: the rotations from
    EvaluationKey.hoisted(...).rotate, the products and their sum from Context.dot_product_scalar; decrypted and decoded,
    against numpy modulo t."""
    x = Xfer(dev)
    n, sizes = SMALL
    opar, par = K.params(fhe, n, sizes)
    t, d, cols = opar.plaintext, 4, n // 2
    g = np.random.default_rng(seed)
    M, v = g.integers(0, t, size=(d, d), dtype=np.uint64), g.integers(0, t, size=d, dtype=np.uint64)
    enc = par.encoder()
    sk = fhe.SecretKey.random(par, bytes(range(32)))
    ek = fhe.EvaluationKey.generate(sk, column_rotations=(1, 2, 3), seeds=[bytes([i + 1] * 32) for i in range(3)])
    slots = np.tile(v, n // d)                              # both rows of n / 2 columns hold v with period 4
    ct = sk.encrypt(enc.encode(slots[None], scaled=True), a_seeds=[bytes([7] * 32)], e_seeds=[bytes([8] * 32)])
    # the direction of a column rotation, read from the single-rotation call (which has its own oracle tests)
    ramp = np.arange(n, dtype=np.uint64)[None]
    rc = sk.encrypt(enc.encode(ramp, scaled=True), a_seeds=[bytes([9] * 32)], e_seeds=[bytes([10] * 32)])
    turned = enc.decode(sk.decrypt(ek.rotates_columns_by(rc, 1)))[0]
    step = int(turned[0])
    assert step in (1, cols - 1) and list(turned[:cols]) == [(k + step) % cols for k in range(cols)], turned
    # rotation i of the ciphertext holds v[(k + i * step) mod 4] in slot k: diagonal i is M[k][(k + i * step) mod 4]
    diag = np.stack([np.array([M[k % d][(k + i * step) % d] for k in range(n)], dtype=np.uint64) for i in range(d)])
    pts = enc.encode(diag)[None]                            # [1, 4, L, N] poly_ntt
    h = ek.hoisted(column_rotations=(1, 2, 3))
    ctd = x.to(ct)
    rot = x.back(h.rotate(ctd))                             # [1, 3, 2, L, N]
    cts = np.concatenate([np.asarray(ct)[:, None], rot], axis=1)
    prod = par.context_at_level(0).dot_product_scalar(x.to(cts), x.to(pts))
    got = enc.decode(sk.decrypt(x.back(prod)))[0]
    want = (M.astype(object) @ v.astype(object)) % t
    assert [int(a) for a in got] == [int(want[k % d]) for k in range(n)], (got, want)


# ---- shapes the Python oracle is too slow for: the expected words composed from engine calls with their own oracle tests ---
def composed(fhe, ctx, q, ct, k0, k1, exps):
    """hoist_ref through Context.ntt_backward, a row broadcast reduced per modulus, ntt_forward, substitute, mul and add
    (host forms): ct [batch, 2, L, N], k0 / k1 [R][digits, L, N] -> [batch, R, 2, L, N]."""
    qcol = np.array(q, dtype=np.uint64)[None, :, None]
    c0, c1 = np.ascontiguousarray(ct[:, 0]), np.ascontiguousarray(ct[:, 1])
    p = ctx.ntt_backward(c1)
    w = [ctx.ntt_forward(np.ascontiguousarray(np.broadcast_to(p[:, i:i + 1], p.shape) % qcol)) for i in range(len(q))]
    out = []
    for r, e in enumerate(exps):
        o0, o1 = ctx.substitute(e, c0), np.zeros_like(c1)
        for i, wi in enumerate(w):
            s = ctx.substitute(e, wi)
            o0 = ctx.add(o0, ctx.mul(s, np.ascontiguousarray(np.broadcast_to(k0[r][i], s.shape))))
            o1 = ctx.add(o1, ctx.mul(s, np.ascontiguousarray(np.broadcast_to(k1[r][i], s.shape))))
        out.append(np.stack([o0, o1], axis=1))
    return np.stack(out, axis=1)


def launches(fhe, call):
    """{kernel family: launches} inside call(), from the engine's profiler (fhe_prof_get_symbol)."""
    fhe.prof_reset()
    fhe.prof_enable(True)
    try:
        call()
    finally:
        fhe.prof_enable(False)
    count = {}
    for _, sym, n, _ in fhe.prof_entries():
        for fam in ("hoist_mac_kernel", "ks_ntt_kernel", "ks_mac", "ks_fused"):
            if fam in sym:
                count[fam] = count.get(fam, 0) + n
    symbols = [sym for _, sym, n, _ in fhe.prof_entries() if n]
    fhe.prof_reset()
    return count, symbols


def case_large(fhe, dev, q, n, nrot, batch, seed, w_budget=0):
    """Uniform keys and ciphertext words at a size the oracle is too slow for: every word against `composed`, and the
    launches counted -- stage A once per (chunk, key-modulus group), stage B once per (chunk, group, rotation group),
    never once per rotation."""
    x = Xfer(dev)
    sy = K.Synthetic(fhe, q, n, nrot, seed)
    L = len(sy.q)
    exps = odd_exponents(n, nrot, seed)
    ct = K.uniform(np.random.default_rng(seed + 1000), sy.q, n, (batch, 2))
    sy.set.set_w_budget(w_budget)
    inp = x.to(ct)
    box = {}
    count, symbols = launches(fhe, lambda: box.setdefault("got", sy.set.relinearize_hoisted(exps, inp)))
    got = x.back(box["got"])
    pc, jg = K.chunk_rule(batch, L, L, n, w_budget)
    pairs = -(-batch // pc) * -(-L // jg)
    assert count.get("ks_ntt_kernel") == pairs, (count, symbols)
    assert count.get("hoist_mac_kernel") == pairs * -(-nrot // TABLE), (count, symbols)
    assert "ks_mac" not in count and "ks_fused" not in count, symbols
    same(got, composed(fhe, sy.ctx, sy.q, ct, sy.c0, sy.c1, exps), ("composed", n, batch, nrot))
    return symbols
