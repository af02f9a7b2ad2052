"""Cases of the keyed batches (fhe_kskset_*, fhe_*_keyed_dev; KeySet, EvaluationKey.batched): one key per client in one
batch.  Shared by tests/test_keyed_emu.py (kernel sources under host emulation) and tests/test_keyed_gpu.py (the HIP
build).  `dev`: as helpers.Xfer -- False hands numpy arrays over (staged through the device by the wrappers), True torch
tensors, "abi" DeviceArrays.

Every comparison is word for word, between the keyed call, the Python oracle client by client (KeySwitchingKey.key_switch,
RelinearizationKey.relinearizes, GaloisKey.relinearize, inner_sum, expands, Multiplicator.multiply of
oracle/fhe_oracle/bfv.py) and -- on the synthetic shapes -- the single-key engine call for the same client.  Clients have
distinct secret keys and seeds (distinct uniform key words on the synthetic shapes), and every case first asserts that
two clients' single-key results for one input differ, so a wrong key index cannot pass."""
import ctypes as C
import random
import types

import numpy as np
import pytest

import keygen_cases as G
from fhe_oracle import bfv as obfv
from fhe_oracle.rq import NTT, NTT_SHOUP, POWER_BASIS, Context as OCtx, Poly
from helpers import Xfer, arr, ct_arr, ksk_arrays, rand_poly

KS_W_BUDGET_DEFAULT = 4 << 30   # engine.hpp


def params(fhe, n, sizes, t=None):
    import encode_cases as E
    return G.params(fhe, n, t or (1153 if n <= 64 else E.stock_t(n)), moduli_sizes=list(sizes))


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert diff.size == 0, (what, "first differing word", int(diff[0]), "of", want.size)


def differ(a, b, what):
    assert not np.array_equal(np.asarray(a), np.asarray(b)), ("two clients' results for one input are equal", what)


def chunk_rule(npolys, nd, lk, n, budget):
    """(pc, jg) of engine.hpp's W budget rule (key_switch_polys_unfused / _keyed), restated: polynomials per chunk and
    key moduli per group, equal chunks and equal groups."""
    budget = budget or KS_W_BUDGET_DEFAULT
    row = n * 8
    pc, jg = npolys, lk
    if pc * nd * jg * row > budget:
        jg = min(max(1, budget // (pc * nd * row)), lk)
        if pc * nd * jg * row > budget:
            pc = max(1, budget // (nd * jg * row))
    jg = -(-lk // -(-lk // jg))
    pc = -(-npolys // -(-npolys // pc))
    return pc, jg


# ---- clients of a parameter set: real keys from the Python oracle --------------------------------------------------------
class Clients:
    """`count` clients of one parameter set, each with its own secret key and rng (seeded by its index)."""

    def __init__(self, fhe, opar, par, count, seed):
        self.fhe, self.opar, self.par, self.count = fhe, opar, par, count
        self.rng = [random.Random(seed * 4099 + c) for c in range(count)]
        self.sk = [obfv.SecretKey.random(opar, r) for r in self.rng]

    def engine_ksk(self, oksk, cl, kl):
        c0, _, c1, _ = ksk_arrays(oksk)
        return self.fhe.KeySwitchingKey(self.par.context_at_level(cl), self.par.context_at_level(kl), c0, c1)

    def relin_keys(self, cl=0, kl=0):
        ork = [obfv.RelinearizationKey(s, r, cl, kl) for s, r in zip(self.sk, self.rng)]
        return ork, [self.fhe.RelinearizationKey(self.engine_ksk(o.ksk, cl, kl)) for o in ork]

    def galois_keys(self, exps, cl=0, kl=0):
        """([{e: oracle key} per client], [[engine GaloisKey per e] per client])"""
        ogk = [{e: obfv.GaloisKey(s, e, cl, kl, r) for e in exps} for s, r in zip(self.sk, self.rng)]
        return ogk, [[self.fhe.GaloisKey(self.engine_ksk(o[e].ksk, cl, kl), e) for e in exps] for o in ogk]

    def encrypt(self, c, level=0, nvalues=None):
        n, t = self.opar.degree(), self.opar.plaintext
        return self.sk[c].encrypt([self.rng[c].randrange(t) for _ in range(nvalues or n)], self.rng[c], level)


def case_relin(fhe, dev, opar, par, nkeys, per_key, cl=0, kl=0, seed=31):
    """key_switch and relinearizes (the own-row read from the Ntt c2) with `nkeys` clients x `per_key` items."""
    x = Xfer(dev)
    cs = Clients(fhe, opar, par, nkeys, seed)
    ork, rks = cs.relin_keys(cl, kl)
    ks = fhe.KeySet(rks)
    assert len(ks) == nkeys
    batch = nkeys * per_key
    rng = random.Random(seed)
    p = [rand_poly(opar.ctx[cl], POWER_BASIS, rng) for _ in range(batch)]
    w = [ork[b // per_key].ksk.key_switch(q) for b, q in enumerate(p)]
    if nkeys > 1:
        differ(arr(w[0][0]), arr(ork[1].ksk.key_switch(p[0])[0]), "key_switch")
    g0, g1 = ks.key_switch(x.to(np.stack([arr(q) for q in p])))
    same(x.back(g0), np.stack([arr(v[0]) for v in w]), ("key_switch c0", nkeys, per_key, cl, kl))
    same(x.back(g1), np.stack([arr(v[1]) for v in w]), ("key_switch c1", nkeys, per_key, cl, kl))
    cts = [obfv.Ciphertext(opar, [rand_poly(opar.ctx[cl], NTT, rng) for _ in range(3)], cl) for _ in range(batch)]
    inp = np.stack([ct_arr(c) for c in cts])
    if nkeys > 1:
        a, b = cts[0].clone(), cts[0].clone()
        ork[0].relinearizes(a), ork[1].relinearizes(b)
        differ(ct_arr(a), ct_arr(b), "relinearizes")
    for b, c in enumerate(cts):
        ork[b // per_key].relinearizes(c)
    same(x.back(ks.relinearizes(x.to(inp))), np.stack([ct_arr(c) for c in cts]), ("relinearizes", nkeys, per_key, cl, kl))


def case_galois(fhe, dev, opar, par, nkeys, per_key, exps, cl=0, kl=0, seed=37):
    """GaloisKey::relinearize per client, one set per exponent (the copying path below N = 4096)."""
    x = Xfer(dev)
    cs = Clients(fhe, opar, par, nkeys, seed)
    ogk, gks = cs.galois_keys(exps, cl, kl)
    cts = [cs.encrypt(b // per_key, cl) for b in range(nkeys * per_key)]
    inp = x.to(np.stack([ct_arr(c) for c in cts]))
    for i, e in enumerate(exps):
        differ(ct_arr(ogk[0][e].relinearize(cts[0])), ct_arr(ogk[1][e].relinearize(cts[0])), ("rotation", e))
        ks = fhe.KeySet([g[i] for g in gks])
        want = np.stack([ct_arr(ogk[b // per_key][e].relinearize(c)) for b, c in enumerate(cts)])
        same(x.back(ks.relinearize(e, inp)), want, ("rotation", e, nkeys, per_key, cl, kl))


def case_evaluation_key(fhe, dev, opar, par, nkeys, per_key, seed=41):
    """EvaluationKey.batched: rotates_rows, rotates_columns_by, computes_inner_sum, and expands to size 4 and to size 3
    (nhigh < step) with `nkeys` clients x `per_key` queries: the slot-major wrap of the key index."""
    x = Xfer(dev)
    n = opar.degree()
    logn = n.bit_length() - 1
    exps = fhe.EvaluationKey.exponents(n, column_rotations=(1,), row_rotation=True, inner_sum=True, expansion_level=2)
    cs = Clients(fhe, opar, par, nkeys, seed)
    ogk, gks = cs.galois_keys(exps)
    eks = [fhe.EvaluationKey(n, g) for g in gks]
    eset = fhe.EvaluationKey.batched(eks)
    assert eset.supports_expansion(2) and not eset.supports_expansion(3) and logn >= 3
    batch = nkeys * per_key
    cts = [cs.encrypt(b // per_key, 0, 4) for b in range(batch)]
    inp = x.to(np.stack([ct_arr(c) for c in cts]))
    client = lambda b: ogk[b // per_key]   # noqa: E731
    differ(ct_arr(obfv.inner_sum(cts[0], ogk[0], n)), ct_arr(obfv.inner_sum(cts[0], ogk[1], n)), "inner sum")
    same(x.back(eset.rotates_rows(inp)), np.stack([ct_arr(client(b)[2 * n - 1].relinearize(c)) for b, c in enumerate(cts)]),
         "rotates_rows")
    same(x.back(eset.rotates_columns_by(inp, 1)), np.stack([ct_arr(client(b)[3].relinearize(c)) for b, c in enumerate(cts)]),
         "rotates_columns_by")
    same(x.back(eset.computes_inner_sum(inp)), np.stack([ct_arr(obfv.inner_sum(c, client(b), n)) for b, c in enumerate(cts)]),
         "inner sum")
    for size in (4, 3):
        differ(ct_arr(obfv.expands(cts[0], size, ogk[0])[size - 1]), ct_arr(obfv.expands(cts[0], size, ogk[1])[size - 1]),
               ("expands", size))
        got = x.back(eset.expands(inp, size))
        assert got.shape[:2] == (size, batch)
        want = [obfv.expands(c, size, client(b)) for b, c in enumerate(cts)]
        same(got, np.stack([np.stack([ct_arr(want[b][i]) for b in range(batch)]) for i in range(size)]), ("expands", size))
    other = Clients(fhe, opar, par, 1, seed + 1)
    _, g2 = other.galois_keys(exps[:-1])
    with pytest.raises(fhe.FheError) as err:
        fhe.EvaluationKey.batched([eks[0], fhe.EvaluationKey(n, g2[0])])
    assert err.value.code == -1 and "exponents" in str(err.value)


def case_multiply(fhe, dev, opar, par, nkeys, per_key, level=0, seed=43):
    """Per client Multiplicator::default(rk_c).multiply (ops/mul.rs:165-243), against the composition over the whole batch:
    a multiplicator without a key (three parts), the keyed relinearization, then switch_down for the mod_switch form."""
    x = Xfer(dev)
    cs = Clients(fhe, opar, par, nkeys, seed)
    ork, rks = cs.relin_keys(level, level)
    ks = fhe.KeySet(rks)
    batch = nkeys * per_key
    A = [cs.encrypt(b // per_key, level) for b in range(batch)]
    B = [cs.encrypt(b // per_key, level) for b in range(batch)]
    lhs, rhs = x.to(np.stack([ct_arr(c) for c in A])), x.to(np.stack([ct_arr(c) for c in B]))
    differ(ct_arr(obfv.Multiplicator.default(ork[0]).multiply(A[0], B[0])),
           ct_arr(obfv.Multiplicator.default(ork[1]).multiply(A[0], B[0])), "multiply")
    ct3 = fhe.Multiplicator.default(par, None, level).multiply(lhs, rhs)
    got = ks.relinearizes(ct3)
    down = par.context_at_level(level).ciphertext_switch_down(got)
    for mod_switch, g in ((False, got), (True, down)):
        want = []
        for b in range(batch):
            om = obfv.Multiplicator.default(ork[b // per_key])
            if mod_switch:
                om.enable_mod_switching()
            want.append(ct_arr(om.multiply(A[b], B[b])))
        same(x.back(g), np.stack(want), ("multiply", mod_switch))


# ---- synthetic clients over raw contexts: uniform key words, the single-key engine call as the second reference ----------
def uniform(rng, q, n, lead=()):
    return np.stack([rng.integers(0, m, size=tuple(lead) + (n,), dtype=np.uint64) for m in q], axis=-2)


class Synthetic:
    """`nkeys` clients over the context of moduli `q`: key c holds uniform words drawn from generator seed + c (or q_j - 1
    everywhere: `top`), created through fhe_ksk_create_dev."""

    def __init__(self, fhe, q, n, nkeys, seed, top=False):
        self.fhe, self.q, self.n, self.nkeys = fhe, list(q), n, nkeys
        self.ctx = fhe.Context(self.q, n)
        self.octx = None
        self.c0, self.c1, self.keys = [], [], []
        L = len(self.q)
        for c in range(nkeys):
            g = np.random.default_rng(seed + c)
            if top:
                k0 = k1 = np.broadcast_to(np.array(self.q, dtype=np.uint64)[None, :, None] - np.uint64(1), (L, L, n)).copy()
            else:
                k0, k1 = uniform(g, self.q, n, (L,)), uniform(g, self.q, n, (L,))
            self.c0.append(k0), self.c1.append(k1)
            self.keys.append(fhe.KeySwitchingKey(self.ctx, self.ctx, fhe.DeviceArray.from_numpy(k0),
                                                 fhe.DeviceArray.from_numpy(k1)))
        self.set = fhe.KeySet(self.keys)

    def oracle_key(self, c):
        if self.octx is None:
            self.octx = OCtx(self.q, self.n)
            self.opar = types.SimpleNamespace(context_at_level=lambda level: self.octx)
        polys = lambda k: [Poly(self.octx, NTT_SHOUP, row.tolist()) for row in k]   # noqa: E731
        return obfv.KeySwitchingKey.from_parts(self.opar, polys(self.c0[c]), polys(self.c1[c]), 0, 0)


def case_synthetic(fhe, dev, q, n, nkeys, per_key, seed, exps=(), top=False, oracle=True, w_budget=None, in_place=False):
    """key_switch, relinearizes and the rotations of `exps` over `nkeys` synthetic clients x `per_key` items: the keyed call
    against the single-key engine call per client, and against the Python oracle when `oracle`.  top: every key word and
    every input word at q_i - 1.  w_budget: the same calls again under that W budget, compared with the default budget's.
    in_place (device forms): the rotations with out == ct as well."""
    x = Xfer(dev)
    sy = Synthetic(fhe, q, n, nkeys, seed, top)
    L, batch = len(sy.q), nkeys * per_key
    g = np.random.default_rng(seed + 1000)
    if top:
        top_row = np.array(sy.q, dtype=np.uint64)[:, None] - np.uint64(1)
        p = np.broadcast_to(top_row, (batch, L, n)).copy()
        ct3 = np.broadcast_to(top_row, (batch, 3, L, n)).copy()
    else:
        p, ct3 = uniform(g, sy.q, n, (batch,)), uniform(g, sy.q, n, (batch, 3))
    ct2 = np.ascontiguousarray(ct3[:, :2])
    piece = lambda a, c: x.to(a[c * per_key:(c + 1) * per_key])   # noqa: E731
    cat = lambda parts: np.concatenate([x.back(v) for v in parts])   # noqa: E731
    rks = [fhe.RelinearizationKey(k) for k in sy.keys]

    def run():
        out = {"key_switch": [x.back(v) for v in sy.set.key_switch(x.to(p))],
               "relinearizes": x.back(sy.set.relinearizes(x.to(ct3)))}
        for e in exps:
            out[("rotation", e)] = x.back(sy.set.relinearize(e, x.to(ct2)))
        return out

    got = run()
    # the single-key engine call, client by client
    single = [sy.keys[c].key_switch(piece(p, c)) for c in range(nkeys)]
    want = {"key_switch": [cat([s[0] for s in single]), cat([s[1] for s in single])],
            "relinearizes": cat([rks[c].relinearizes(piece(ct3, c)) for c in range(nkeys)])}
    for e in exps:
        want[("rotation", e)] = cat([fhe.GaloisKey(sy.keys[c], e).relinearize(piece(ct2, c)) for c in range(nkeys)])
    if nkeys > 1 and not top:   # (`top`: all keys hold the same words)
        differ(want["key_switch"][0][0], x.back(sy.keys[1].key_switch(x.to(p[:1]))[0])[0], "key_switch")
        differ(want["relinearizes"][0], x.back(rks[1].relinearizes(x.to(ct3[:1])))[0], "relinearizes")
        for e in exps:
            differ(want[("rotation", e)][0], x.back(fhe.GaloisKey(sy.keys[1], e).relinearize(x.to(ct2[:1])))[0], ("rotation", e))
    for name in want:
        if name == "key_switch":
            same(got[name][0], want[name][0], (name, "c0", n, nkeys, per_key))
            same(got[name][1], want[name][1], (name, "c1", n, nkeys, per_key))
        else:
            same(got[name], want[name], (name, n, nkeys, per_key))
    if oracle:
        from fhe_oracle.rq import SubstitutionExponent
        for b in range(batch):
            ok = sy.oracle_key(b // per_key)
            w0, w1 = ok.key_switch(Poly(sy.octx, POWER_BASIS, p[b].tolist()))
            same(got["key_switch"][0][b], arr(w0), ("oracle key_switch c0", b))
            same(got["key_switch"][1][b], arr(w1), ("oracle key_switch c1", b))
            c = obfv.Ciphertext(sy.opar, [Poly(sy.octx, NTT, r.tolist()) for r in ct3[b]], 0)
            obfv.RelinearizationKey(ksk=ok).relinearizes(c)
            same(got["relinearizes"][b], ct_arr(c), ("oracle relinearizes", b))
            for e in exps:
                ogk = obfv.GaloisKey.__new__(obfv.GaloisKey)
                ogk.ksk, ogk.element = ok, SubstitutionExponent(sy.octx, e)
                c = obfv.Ciphertext(sy.opar, [Poly(sy.octx, NTT, r.tolist()) for r in ct2[b]], 0)
                same(got[("rotation", e)][b], ct_arr(ogk.relinearize(c)), ("oracle rotation", e, b))
    if w_budget is not None:
        pc, jg = chunk_rule(batch, L, L, n, w_budget)
        assert pc % per_key != 0 and pc < batch and jg < L, (pc, jg)   # chunks end inside a client; groups of key moduli
        assert chunk_rule(batch, L, L, n, 0) == (batch, L)
        assert sy.set.set_w_budget(w_budget).w_budget() == w_budget
        cut = run()
        assert sy.set.set_w_budget(0).w_budget() == 0
        for name in got:
            same(np.asarray(cut[name]), np.asarray(got[name]), ("W budget", name))
    if in_place and dev:
        for e in exps:
            buf = x.to(ct2)
            assert sy.set.relinearize(e, buf, out=buf) is buf
            same(x.back(buf), got[("rotation", e)], ("in place rotation", e))
    return sy


def kernels_of(fhe, call):
    """The demangled kernel symbols launched inside call() (the engine's profiler, fhe_prof_get_symbol)."""
    fhe.prof_reset()
    fhe.prof_enable(True)
    try:
        call()
    finally:
        fhe.prof_enable(False)
    symbols = [sym for _, sym, launches, _ in fhe.prof_entries() if launches]
    fhe.prof_reset()
    return symbols


def assert_keyed_kernels(symbols):
    assert any("ks_mac_keyed_kernel" in s for s in symbols), symbols
    assert not any("ks_mac_kernel" in s or "ks_fused" in s for s in symbols), symbols


# ---- refusals ------------------------------------------------------------------------------------------------------------
def raw(fhe, name, *args):
    """(status, fhe_last_error()) of one raw ABI call."""
    from fhe_rs_amd import _lib
    L = _lib.lib()
    st = getattr(L, name)(*args)
    return st, (L.fhe_last_error().decode(errors="replace") if st else "")


def handles(keys):
    return (C.c_void_p * max(len(keys), 1))(*[k._h.value if k is not None else None for k in keys])


def create_refused(fhe, keys, code, text, null_list=False):
    out = C.c_void_p(1)
    st, msg = raw(fhe, "fhe_kskset_create", None if null_list else handles(keys), len(keys), C.byref(out))
    assert st == code and text in msg and out.value is None, (st, msg, out.value)


def case_refusals(fhe, dev):
    """Status and fhe_last_error text of every refusal of the keyed entry points."""
    x = Xfer(dev)
    n = 16
    opar, par = params(fhe, n, [62, 60, 55])
    cs = Clients(fhe, opar, par, 3, 47)
    ork, rks = cs.relin_keys()
    k = [r.ksk for r in rks]
    create_refused(fhe, [], -1, "at least one key")
    create_refused(fhe, [], -1, "at least one key", null_list=True)
    create_refused(fhe, [k[0], None], -1, "null argument: keys[i]")
    st, msg = raw(fhe, "fhe_kskset_create", handles(k), 3, None)
    assert st == -1 and "null argument: out" in msg
    # a decomposition key (one modulus, log_base != 0)
    last = par.context_at_level(2)
    assert last.nmoduli == 1
    lb = (last.moduli[0] - 1).bit_length() // 2
    nd = -(-(last.moduli[0] - 1).bit_length() // lb)
    z = np.zeros((nd, 1, n), dtype=np.uint64)
    dk = fhe.KeySwitchingKey(last, last, z, z, log_base=lb)
    create_refused(fhe, [dk], -1, "keyed batches take RNS-digit keys")
    # keys of two levels (ciphertext level 1 next to level 0), and of two parameter sets
    _, rk1 = Clients(fhe, opar, par, 1, 48).relin_keys(1, 0)
    create_refused(fhe, [k[0], rk1[0].ksk], -11, "the keys differ in parameters, levels or digit count")
    opar2, par2 = params(fhe, n, [61, 59, 54])
    _, rk2 = Clients(fhe, opar2, par2, 1, 49).relin_keys()
    create_refused(fhe, [k[0], rk2[0].ksk], -11, "the keys differ in parameters, levels or digit count")
    with pytest.raises(fhe.FheError) as err:
        fhe.KeySet([k[0], rk2[0].ksk])
    assert err.value.code == -11
    # batch not a multiple of the set's size; a NULL buffer with a non-empty batch; an empty batch with NULL buffers
    ks = fhe.KeySet(rks)
    ct3 = x.to(np.zeros((4, 3, 3, n), dtype=np.uint64))
    with pytest.raises(fhe.FheError) as err:
        ks.relinearizes(ct3)
    assert err.value.code == -1 and "batch 4 is not a multiple of the set's 3 keys" in str(err.value)
    buf = fhe.DeviceArray((3, 3, 3, n))
    ptr = C.c_void_p(buf.data_ptr())
    assert raw(fhe, "fhe_bfv_relinearize_keyed_dev", ks._h, ptr, ptr, 4, None)[0] == -1
    for name, args, what in (("fhe_key_switch_keyed_dev", (ks._h, None, ptr, ptr, 3, None), "p"),
                             ("fhe_key_switch_keyed_dev", (ks._h, ptr, ptr, None, 3, None), "c1_out"),
                             ("fhe_bfv_relinearize_keyed_dev", (ks._h, ptr, None, 3, None), "out"),
                             ("fhe_bfv_galois_keyed_dev", (ks._h, 3, None, ptr, 3, None), "ct")):
        st, msg = raw(fhe, name, *args)
        assert st == -1 and "null argument: " + what in msg, (name, st, msg)
    assert raw(fhe, "fhe_bfv_relinearize_keyed_dev", ks._h, None, None, 0, None) == (0, "")
    assert raw(fhe, "fhe_key_switch_keyed_dev", ks._h, None, None, None, 0, None) == (0, "")
    assert raw(fhe, "fhe_bfv_relinearize_keyed_dev", None, ptr, ptr, 3, None)[0] == -1
    # inner-sum / expand sets of different sizes, a NULL set in the list, NULL buffers
    two = fhe.KeySet(rks[:2])
    sets = (C.c_void_p * 2)(ks._h.value, two._h.value)
    exps = (C.c_size_t * 2)(3, 2 * n - 1)
    st, msg = raw(fhe, "fhe_bfv_inner_sum_keyed_dev", sets, exps, 2, ptr, ptr, 6, None)
    assert st == -11 and "the sets of one call must have the same size" in msg, (st, msg)
    st, msg = raw(fhe, "fhe_bfv_expand_keyed_dev", sets, 2, ptr, ptr, 2, 6, None)
    assert st == -11 and "the sets of one call must have the same size" in msg, (st, msg)
    sets = (C.c_void_p * 2)(ks._h.value, None)
    assert raw(fhe, "fhe_bfv_inner_sum_keyed_dev", sets, exps, 2, ptr, ptr, 3, None)[0] == -1
    sets = (C.c_void_p * 2)(ks._h.value, ks._h.value)
    st, msg = raw(fhe, "fhe_bfv_inner_sum_keyed_dev", sets, exps, 2, ptr, None, 3, None)
    assert st == -1 and "null argument: out" in msg
    st, msg = raw(fhe, "fhe_bfv_expand_keyed_dev", sets, 2, None, ptr, 2, 3, None)
    assert st == -1 and "null argument: ct" in msg
    assert raw(fhe, "fhe_bfv_inner_sum_keyed_dev", sets, exps, 0, ptr, ptr, 3, None)[0] == -1
    assert raw(fhe, "fhe_bfv_inner_sum_keyed_dev", sets, exps, 2, None, None, 0, None) == (0, "")
    # the set's own options
    w = C.c_size_t(7)
    assert raw(fhe, "fhe_kskset_get_w_budget", ks._h, C.byref(w)) == (0, "") and w.value == 0
    assert raw(fhe, "fhe_kskset_set_w_budget", None, 1)[0] == -1 and raw(fhe, "fhe_kskset_get_w_budget", ks._h, None)[0] == -1
    from fhe_rs_amd import _lib
    assert _lib.lib().fhe_kskset_size(None) == 0 and _lib.lib().fhe_kskset_size(ks._h) == 3
    _lib.lib().fhe_kskset_destroy(None)


def case_multiply_engine(fhe, dev, par, nkeys, per_key, seed=53):
    """The composition of case_multiply on a parameter set too large for the Python oracle: uniform key words and uniform
    ciphertext words, against the engine's own Multiplicator.default(par, rk_c).multiply client by client, with and
    without mod_switch."""
    x = Xfer(dev)
    ctx = par.context_at_level(0)
    q, n = list(ctx.moduli), ctx.degree
    g = np.random.default_rng(seed)
    rks = []
    for _ in range(nkeys):
        k0, k1 = uniform(g, q, n, (len(q),)), uniform(g, q, n, (len(q),))
        rks.append(fhe.RelinearizationKey(fhe.KeySwitchingKey(ctx, ctx, k0, k1)))
    ks = fhe.KeySet(rks)
    batch = nkeys * per_key
    A, B = uniform(g, q, n, (batch, 2)), uniform(g, q, n, (batch, 2))
    piece = lambda a, c: x.to(a[c * per_key:(c + 1) * per_key])   # noqa: E731
    got = ks.relinearizes(fhe.Multiplicator.default(par, None, 0).multiply(x.to(A), x.to(B)))
    down = ctx.ciphertext_switch_down(got)
    for mod_switch, gv in ((False, got), (True, down)):
        ms = [fhe.Multiplicator.default(par, rk, 0, mod_switch) for rk in rks]
        want = [x.back(ms[c].multiply(piece(A, c), piece(B, c))) for c in range(nkeys)]
        if not mod_switch:
            differ(want[0][0], x.back(ms[1].multiply(piece(A, 0), piece(B, 0)))[0], "multiply")
        same(x.back(gv), np.concatenate(want), ("multiply", mod_switch))
