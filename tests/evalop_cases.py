"""Cases of the evaluation kernels' census (tests/evalop_shapes.py), shared by tests/test_evalop_shapes_emu.py (kernel
sources under host emulation) and tests/test_evalop_shapes_gpu.py (the HIP build).  `dev`: as helpers.Xfer -- False
(numpy in, numpy out) or True (torch tensors).

case_shape runs a shape's ops through the public entry points and compares every word with the plain-C oracle
(fhe_oracle.coracle, as tests/full_size.py uses it): synthetic operands and keys from the shared counter generator,
transforms on random residues and on the word patterns of cases.case_f64_ntt (0, 1, q - 1, alternating).  Batches above
four compare items {0, b // 3, 2b // 3, b - 1}; smaller batches compare every item."""
import functools
import re

import numpy as np

import evalop_shapes as S
import full_size
from fhe_oracle import coracle
from fhe_oracle.rq import Context as OCtx
from helpers import Xfer

SEED = 0xF4E5E7A1


def sample(batch):
    """The items compared with the oracle: all of a batch of at most four, else a fixed four."""
    items = sorted({0, batch // 3, 2 * batch // 3, batch - 1}) if batch > 4 else list(range(batch))
    assert len(items) == min(batch, 4)
    return items


@functools.lru_cache(maxsize=4)
def c_context(n, moduli):
    return coracle.CCtx(OCtx(list(moduli), n))


def seed_of(shape):
    return SEED + 97 * (shape.n.bit_length() - 1) + shape.mode


_SYMBOL = re.compile(r"\b(\w+_kernel)(?:<([^>]*)>)?\(")


def cell_of_symbol(symbol):
    """A profiler entry's demangled kernel symbol -> (family, template arguments) for the seven evaluation families;
    None for every other kernel."""
    m = _SYMBOL.search(symbol)
    if not m or m.group(1) not in S.FAMILIES:
        return None
    return m.group(1), m.group(2) or ""


# ---- the ops: each returns {name: array} of engine outputs for the sampled items, and the oracle's values -------------
def op_ntt(fhe, x, shape, want):
    n, q = shape.n, list(shape.moduli)
    cc = c_context(n, shape.moduli)
    if want is None:
        rng = np.random.default_rng(seed_of(shape))
        qa = np.array(q, dtype=np.uint64)[:, None]
        rand = [np.stack([rng.integers(0, m, size=n, dtype=np.uint64) for m in q]) for _ in range(shape.batch)]
        alt = np.where(np.arange(n)[None, :] % 2 == 0, qa - 1, 0).astype(np.uint64)
        polys = np.stack(rand + [np.broadcast_to(qa - 1, (len(q), n)).copy(), alt, np.ones((len(q), n), dtype=np.uint64),
                                 np.zeros((len(q), n), dtype=np.uint64)])
        want = dict(polys=polys, fwd=np.stack([cc.poly_ntt_forward(p) for p in polys]))
        assert all(np.array_equal(cc.poly_ntt_backward(f), p) for f, p in zip(want["fwd"], polys))
    c = fhe.Context(q, n)
    f = x.back(c.ntt_forward(x.to(want["polys"])))
    assert np.array_equal(f, want["fwd"]), ("forward transform", shape)
    b = x.back(c.ntt_backward(x.to(want["fwd"])))
    assert np.array_equal(b, want["polys"]), ("inverse transform", shape)
    return want


def op_mul(fhe, x, shape, want):
    n, q, batch = shape.n, list(shape.moduli), shape.batch
    t = full_size.plaintext_modulus(n)
    seed = seed_of(shape)
    items = sample(batch)
    if want is None:
        o = full_size.oracle_level(n, q, t, 0)
        assert o["mul"].moduli == S.mul_basis(n, q)
        cb = o["cb"]
        ops = np.stack([np.stack([cb.synth_poly(seed, i, p) for p in range(4)]) for i in range(batch)])
        cm = coracle.CMul(cb, o["cm"], o["cel"], o["cel"], o["cdn"], None, False)
        want = dict(ops=ops, out={i: cm.multiply(ops[i, :2], ops[i, 2:]) for i in items})
    par = fhe.BfvParameters(n, t, moduli=q)
    assert par.moduli == q and par.mul_context_at_level(0).moduli == S.mul_basis(n, q)
    m = fhe.Multiplicator.default(par, None, 0, False)
    ops = want["ops"]
    out = m.multiply(x.to(np.ascontiguousarray(ops[:, :2])), x.to(np.ascontiguousarray(ops[:, 2:])))
    out = x.back(out)
    for i in items:
        assert np.array_equal(out[i], want["out"][i]), ("multiply", i, shape)
    return want


def _key(fhe, x, shape, cc, seed):
    L = len(shape.moduli)
    ck = full_size.host_key(cc, seed, L)
    ctx = fhe.Context(list(shape.moduli), shape.n)
    ksk = fhe.KeySwitchingKey(ctx, ctx, x.to(ck.c0), x.to(ck.c1)).set_mode(shape.mode)
    assert ksk.mode()["mode"] == shape.mode
    return ck, ksk


def op_key(fhe, x, shape, want, ops):
    """"ks", "relin" and "rot" under one synthetic key (the mode forced on the handle)."""
    n, batch = shape.n, shape.batch
    cc = c_context(n, shape.moduli)
    seed = seed_of(shape)
    items = sample(batch)
    ck, ksk = _key(fhe, x, shape, cc, seed)
    if want is None:
        ct3 = np.stack([np.stack([cc.synth_poly(seed, i, p) for p in range(3)]) for i in range(batch)])
        want = dict(ct3=ct3)
        if "ks" in ops:
            want["ks"] = {i: ck.key_switch(ct3[i, 0]) for i in items}
        if "relin" in ops:
            def relin(i):
                k0, k1 = ck.key_switch(cc.poly_ntt_backward(ct3[i, 2]))
                return np.stack([cc.poly_add(ct3[i, 0], k0), cc.poly_add(ct3[i, 1], k1)])
            want["relin"] = {i: relin(i) for i in items}
        if "rot" in ops:
            want["rot"] = {i: ck.galois_relinearize(3, ct3[i, :2]) for i in items}
    ct3 = want["ct3"]
    if "ks" in ops:
        g0, g1 = ksk.key_switch(x.to(np.ascontiguousarray(ct3[:, 0])))
        g0, g1 = x.back(g0), x.back(g1)
        for i in items:
            assert np.array_equal(g0[i], want["ks"][i][0]) and np.array_equal(g1[i], want["ks"][i][1]), ("key_switch", i, shape)
    if "relin" in ops:
        got = x.back(fhe.RelinearizationKey(ksk).relinearizes(x.to(ct3)))
        for i in items:
            assert np.array_equal(got[i], want["relin"][i]), ("relinearize", i, shape)
    if "rot" in ops:
        got = x.back(fhe.GaloisKey(ksk, 3).relinearize(x.to(np.ascontiguousarray(ct3[:, :2]))))
        for i in items:
            assert np.array_equal(got[i], want["rot"][i]), ("rotate", i, shape)
    return want


def op_ksb(fhe, x, shape, want):
    """key_switch under a base-2^k decomposition key of one modulus (cases.case_key_switch_decomposition_rows): the
    digits by numpy, transforms, products and sums by the C oracle."""
    n, batch, lb = shape.n, shape.batch, shape.log_base
    (q,) = shape.moduli
    cc = c_context(n, shape.moduli)
    seed = seed_of(shape) + 1
    nd = -(-(q - 1).bit_length() // lb)
    c0 = np.stack([cc.synth_poly(seed, 0, 8 + 2 * i) for i in range(nd)])
    c1 = np.stack([cc.synth_poly(seed, 0, 9 + 2 * i) for i in range(nd)])
    if want is None:
        p = np.stack([cc.synth_poly(seed, i, 0) for i in range(batch)])
        mask = np.uint64((1 << lb) - 1)
        outs = []
        for b in range(batch):
            w0, w1 = np.zeros((1, n), dtype=np.uint64), np.zeros((1, n), dtype=np.uint64)
            for i in range(nd):
                d = cc.poly_ntt_forward((p[b] >> np.uint64(i * lb)) & mask)
                w0 = cc.poly_add(w0, cc.poly_mul(d, c0[i]))
                w1 = cc.poly_add(w1, cc.poly_mul(d, c1[i]))
            outs.append((w0, w1))
        want = dict(p=p, out=outs)
    ctx = fhe.Context([q], n)
    ksk = fhe.KeySwitchingKey(ctx, ctx, x.to(c0), x.to(c1), log_base=lb).set_mode(shape.mode)
    g0, g1 = ksk.key_switch(x.to(want["p"]))
    g0, g1 = x.back(g0), x.back(g1)
    for b in range(batch):
        assert np.array_equal(g0[b], want["out"][b][0]) and np.array_equal(g1[b], want["out"][b][1]), ("decomposition key", b, shape)
    return want


def case_shape(fhe, dev, shape, wants=None):
    """Every op of the shape against the oracle.  Returns the oracle's values, which a second run of the same shape (the
    F64 switch off) takes back as `wants`: the engine must produce the same words."""
    x = Xfer(dev)
    wants = dict(wants or {})
    key_ops = tuple(op for op in shape.ops if op in ("ks", "relin", "rot"))
    for op in shape.ops:
        if op == "ntt":
            wants["ntt"] = op_ntt(fhe, x, shape, wants.get("ntt"))
        elif op == "mul":
            wants["mul"] = op_mul(fhe, x, shape, wants.get("mul"))
        elif op == "ksb":
            wants["ksb"] = op_ksb(fhe, x, shape, wants.get("ksb"))
    if key_ops:
        wants["key"] = op_key(fhe, x, shape, wants.get("key"), key_ops)
    return wants


def check_shape(fhe, dev, shape):
    """case_shape, and for F64-eligible shapes once more on the integer kernels: the same words."""
    assert fhe.get_f64()
    wants = case_shape(fhe, dev, shape)
    if S.f64_eligible(shape):
        fhe.set_f64(False)
        try:
            case_shape(fhe, dev, shape, wants)
        finally:
            fhe.set_f64(True)
