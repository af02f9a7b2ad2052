"""Cases of the hoisted rotations and the hoisted matrix-vector product with one Galois key set per client
(fhe_bfv_galois_hoisted_keyed_dev, fhe_bfv_matvec_hoisted_keyed_dev; KeySet.relinearize_hoisted_keyed, KeySet.
matvec_hoisted_keyed, EvaluationKeySet.hoisted).  Shared by tests/test_hoistkeyed_emu.py (kernel sources under host
emulation) and tests/test_hoistkeyed_gpu.py (the HIP build).  `dev`: as helpers.Xfer.

The specification is a composition: one single-client call per client on the client's keys and slice of the batch, word
for word.  So every case compares with those calls, and with the restatements tests/hoist_ref.py / tests/hoistmv_ref.py
under the owning client's keys (entry c * R + r of the client-major set).  The clients hold distinct keys, and the cases
assert that two clients' outputs for the same ciphertext words differ, so a build that ignores the client index fails."""
import ctypes as C

import numpy as np
import pytest

import hoist_cases as H
import hoistmv_cases as M
import keyed_cases as K
from fhe_oracle import bfv as obfv
from fhe_oracle.rq import NTT, Poly
from helpers import Xfer, ct_arr

TABLE = H.TABLE
SMALL = H.SMALL
same, differ = K.same, K.differ
STRADDLE_BUDGET = 2 * 3 * 16 * 8   # N = 16, three digits: two ciphertexts of one key modulus per chunk


def small_moduli():
    return obfv.generate_moduli(SMALL[1], SMALL[0])


# ---- real keys from the oracle ---------------------------------------------------------------------------------------------
def case_anchor(fhe, dev, cl=0, kl=0, exps=(1, 3, 9, 31, 3), nclients=3, per_client=2, seed=301):
    """N = 16 over [62, 60, 55], three clients with their own secret keys, two ciphertexts each: every word against
    hoist_ref under the owner's oracle keys and against the owner's KeySet.relinearize_hoisted; exponent 1 against the
    oracle's GaloisKey.relinearize; the other exponents by decryption under the owner's secret key; the same ciphertext
    words under two clients give different outputs."""
    x = Xfer(dev)
    opar, par = K.params(fhe, *SMALL)
    cs = K.Clients(fhe, opar, par, nclients, seed)
    ogk, gks = cs.galois_keys(exps, cl, kl)
    batch, R = nclients * per_client, len(exps)
    owner = lambda b: b // per_client   # noqa: E731
    cts = [cs.encrypt(owner(b), cl) for b in range(batch)]
    inp = np.stack([ct_arr(c) for c in cts])
    kset = fhe.KeySet([g.ksk for c in range(nclients) for g in gks[c]])
    assert len(kset) == nclients * R
    got = x.back(kset.relinearize_hoisted_keyed(nclients, exps, x.to(inp)))
    assert got.shape == (batch, R) + inp.shape[1:]
    octx = opar.context_at_level(cl)
    for c in range(nclients):
        sl = slice(c * per_client, (c + 1) * per_client)
        same(got[sl], H.ref_rotations(octx, inp[sl], [ogk[c][e].ksk for e in exps], exps), ("hoist_ref", c, cl, kl))
        single = fhe.KeySet([g.ksk for g in gks[c]])
        same(got[sl], x.back(single.relinearize_hoisted(exps, x.to(inp[sl]))), ("the client's own call", c, cl, kl))
    for b, ct in enumerate(cts):
        c = owner(b)
        for r, e in enumerate(exps):
            want = ogk[c][e].relinearize(ct)
            if e == 1:
                same(got[b][r], ct_arr(want), ("exponent 1 against GaloisKey.relinearize", b))
                continue
            mine = obfv.Ciphertext(opar, [Poly(octx, NTT, part.tolist()) for part in got[b][r]], cl)
            assert cs.sk[c].decrypt(mine) == cs.sk[c].decrypt(want), ("decryption under the owner's key", b, e)
    # one ciphertext's words handed to every client: equal within a client, different between clients
    rep = np.stack([inp[0]] * batch)
    out = x.back(kset.relinearize_hoisted_keyed(nclients, exps, x.to(rep)))
    same(out[0], out[per_client - 1], "one client, one input")
    for c in range(1, nclients):
        for r in range(R):
            differ(out[0][r], out[c * per_client][r], ("clients 0 and %d" % c, exps[r]))


# ---- synthetic keys: a client-major set of nclients x nrot uniform keys --------------------------------------------------------
class Keyed:
    """K.Synthetic with nclients * nrot keys: `set` is the client-major set, single(c) client c's own KeySet."""

    def __init__(self, fhe, q, n, nclients, nrot, seed, top=False):
        self.fhe, self.nclients, self.nrot, self.n = fhe, nclients, nrot, n
        self.sy = K.Synthetic(fhe, q, n, nclients * nrot, seed, top)
        self.q, self.set, self.ctx = self.sy.q, self.sy.set, self.sy.ctx
        self._single = {}

    def single(self, c):
        if c not in self._single:
            self._single[c] = self.fhe.KeySet(self.sy.keys[c * self.nrot:(c + 1) * self.nrot])
        return self._single[c]

    def oracle_keys(self, c, rots):
        return [self.sy.oracle_key(c * self.nrot + r) for r in rots]

    @property
    def octx(self):
        self.sy.oracle_key(0)
        return self.sy.octx

    def inputs(self, batch, seed, top=False):
        if top:
            return np.broadcast_to(np.array(self.q, dtype=np.uint64)[:, None] - np.uint64(1), (batch, 2, len(self.q), self.n)).copy()
        return K.uniform(np.random.default_rng(seed + 1000), self.q, self.n, (batch, 2))


def rotate_per_client(x, ky, exps, ct):
    m = len(ct) // ky.nclients
    return np.concatenate([x.back(ky.single(c).relinearize_hoisted(exps, x.to(ct[c * m:(c + 1) * m]))) for c in range(ky.nclients)])


def case_rotations(fhe, dev, q, n, nclients, nrot, per_client, seed, top=False, check=None, w_budget=None, oracle=True):
    """`nclients` x `nrot` synthetic keys, random odd exponents: the keyed call against one unkeyed call per client, and
    the rotations `check` (default all) against hoist_ref under entries c * nrot + r.  w_budget: the call again under
    that W budget, against the default budget's words.  Returns (ky, exps, ct, got)."""
    x = Xfer(dev)
    ky = Keyed(fhe, q, n, nclients, nrot, seed, top)
    exps = H.odd_exponents(n, nrot, seed)
    batch = nclients * per_client
    ct = ky.inputs(batch, seed, top)
    got = x.back(ky.set.relinearize_hoisted_keyed(nclients, exps, x.to(ct)))
    assert got.shape == (batch, nrot, 2, len(ky.q), n)
    same(got, rotate_per_client(x, ky, exps, ct), ("one unkeyed call per client", n, nclients, nrot, per_client))
    if nclients > 1 and not top:
        rep = np.stack([ct[0]] * batch)
        out = x.back(ky.set.relinearize_hoisted_keyed(nclients, exps, x.to(rep)))
        differ(out[0], out[per_client], "clients 0 and 1 on one ciphertext's words")
    if oracle:
        check = list(range(nrot)) if check is None else list(check)
        for c in range(nclients):
            sl = slice(c * per_client, (c + 1) * per_client)
            want = H.ref_rotations(ky.octx, ct[sl], ky.oracle_keys(c, check), [exps[r] for r in check])
            for i, r in enumerate(check):
                same(got[sl, r], want[:, i], ("hoist_ref", "client", c, "rotation", r, n))
    if w_budget is not None:
        assert ky.set.set_w_budget(w_budget).w_budget() == w_budget
        cut = x.back(ky.set.relinearize_hoisted_keyed(nclients, exps, x.to(ct)))
        assert ky.set.set_w_budget(0).w_budget() == 0
        same(cut, got, "W budget")
    return ky, exps, ct, got


def case_one_client(fhe, dev):
    """nclients = 1: word for word the unkeyed call on the same set (N = 16, R = 3, batch 2)."""
    x = Xfer(dev)
    ky, exps, ct, got = case_rotations(fhe, dev, small_moduli(), SMALL[0], 1, 3, 2, seed=303)
    same(got, x.back(ky.set.relinearize_hoisted(exps, x.to(ct))), "the unkeyed call on the same set")


def case_one_ciphertext_per_client(fhe, dev):
    """per_client = 1: three clients, batch 3."""
    case_rotations(fhe, dev, small_moduli(), SMALL[0], 3, 2, 1, seed=305)


def case_more_rotations_than_a_table(fhe, dev):
    """2 clients x 65 rotations at N = 16, batch 2 (130 keys): two stage-B launches on one W, the second with rot0 = 64;
    rotations 0, 63 and 64 of each client against hoist_ref under entries c * 65 + r."""
    case_rotations(fhe, dev, small_moduli(), SMALL[0], 2, TABLE + 1, 1, seed=307, check=(0, TABLE - 1, TABLE))


def case_straddle(fhe, dev):
    """N = 16, 2 clients x 3 ciphertexts, R = 3 under a budget of two ciphertexts of one key modulus: the middle chunk
    [2, 4) starts inside client 0's run and ends in client 1's."""
    assert K.chunk_rule(6, 3, 3, 16, STRADDLE_BUDGET) == (2, 1) and K.chunk_rule(6, 3, 3, 16, 0) == (6, 3)
    case_rotations(fhe, dev, small_moduli(), SMALL[0], 2, 3, 3, seed=309, w_budget=STRADDLE_BUDGET)


# ---- matvec ----------------------------------------------------------------------------------------------------------------
def matvec_per_client(x, ky, exps, ct, pts, pt0):
    m = len(ct) // ky.nclients
    out = []
    for c in range(ky.nclients):
        sl = slice(c * m, (c + 1) * m)
        p = pts if pts.ndim == 3 else pts[sl]
        p0 = None if pt0 is None else (pt0 if pt0.ndim == 2 else pt0[sl])
        out.append(x.back(ky.single(c).matvec_hoisted(exps, x.to(ct[sl]), x.to(p), None if p0 is None else x.to(p0))))
    return np.concatenate(out)


def keyed_composition(x, ky, exps, ct, pts, pt0):
    """The keyed rotations, then Context.dot_product_scalar (host arrays)."""
    cts = x.back(ky.set.relinearize_hoisted_keyed(ky.nclients, exps, x.to(ct)))
    p = pts
    if pt0 is not None:
        cts = np.concatenate([ct[:, None], cts], axis=1)
        p = np.concatenate([pt0[..., None, :, :], pts], axis=-3)
    return ky.ctx.dot_product_scalar(np.ascontiguousarray(cts), np.ascontiguousarray(p))


def run_matvec(x, ky, exps, ct, pts, pt0):
    return x.back(ky.set.matvec_hoisted_keyed(ky.nclients, exps, x.to(ct), x.to(pts), None if pt0 is None else x.to(pt0)))


def case_matvec(fhe, dev, q, n, nclients, nrot, per_client, seed, top=False, variants=None, rot_split=0, w_budget=None,
                oracle=False, composed=True):
    """The keyed matvec against one KeySet.matvec_hoisted call per client and against the keyed rotations followed by
    dot_product_scalar; `variants`: (pts shared, pt0 given) pairs.  oracle: hoistmv_ref under the owner's keys too."""
    x = Xfer(dev)
    ky = Keyed(fhe, q, n, nclients, nrot, seed, top)
    exps = H.odd_exponents(n, nrot, seed)
    batch = nclients * per_client
    ct = ky.inputs(batch, seed, top)
    g = np.random.default_rng(seed + 2000)
    assert ky.set.set_rot_split(rot_split).rot_split() == rot_split
    first = None
    for shared, with0 in (variants or [(True, True)]):
        pts, pt0 = M.diagonals(g, ky.q, n, nrot, batch, shared, top)
        pt0 = pt0 if with0 else None
        got = run_matvec(x, ky, exps, ct, pts, pt0)
        assert got.shape == ct.shape
        same(got, matvec_per_client(x, ky, exps, ct, pts, pt0), ("one unkeyed call per client", shared, with0, n, nrot))
        if composed:
            same(got, keyed_composition(x, ky, exps, ct, pts, pt0), ("keyed rotations, then the dot product", shared, with0))
        if oracle:
            for c in range(nclients):
                sl = slice(c * per_client, (c + 1) * per_client)
                p = pts if shared else pts[sl]
                p0 = None if pt0 is None else (pt0 if shared else pt0[sl])
                same(got[sl], M.reference(ky.octx, ct[sl], ky.oracle_keys(c, range(nrot)), exps, p, p0), ("hoistmv_ref", c))
        if nclients > 1 and not top and shared:
            rep = np.stack([ct[0]] * batch)
            out = run_matvec(x, ky, exps, rep, pts, pt0)
            differ(out[0], out[per_client], "clients 0 and 1 on one ciphertext's words")
        if w_budget is not None:
            assert ky.set.set_w_budget(w_budget).w_budget() == w_budget
            cut = run_matvec(x, ky, exps, ct, pts, pt0)
            assert ky.set.set_w_budget(0).w_budget() == 0
            same(cut, got, ("W budget", shared, with0))
        first = first if first is not None else (ky, exps, ct, pts, pt0, got)
    ky.set.set_rot_split(0)
    return first


ALL_FORMS = [(True, True), (True, False), (False, True), (False, False)]


def case_matvec_anchor(fhe, dev):
    """N = 16, 2 clients x 2 ciphertexts, R = 5: diagonals shared and per item, pt0 absent, shared and per item."""
    case_matvec(fhe, dev, small_moduli(), SMALL[0], 2, 5, 2, seed=311, variants=ALL_FORMS, oracle=True)


def case_matvec_rot_split(fhe, dev):
    """rot_split 0, 1, 2, 3 and 9 (clamped to 5): the same words."""
    x = Xfer(dev)
    ky, exps, ct, pts, pt0, first = case_matvec(fhe, dev, small_moduli(), SMALL[0], 2, 5, 2, seed=313)
    for split in (0, 1, 2, 3, 9):
        assert ky.set.set_rot_split(split).rot_split() == split
        same(run_matvec(x, ky, exps, ct, pts, pt0), first, ("rot_split", split))
    ky.set.set_rot_split(0)


def case_matvec_table_boundary(fhe, dev):
    """R = 65 over two clients, batch 2, with and without pt0: two launches on one W, their partial sums added."""
    case_matvec(fhe, dev, small_moduli(), SMALL[0], 2, TABLE + 1, 1, seed=315, variants=[(False, True), (True, False)], composed=False)


def case_matvec_straddle(fhe, dev):
    assert K.chunk_rule(6, 3, 3, 16, STRADDLE_BUDGET) == (2, 1)
    case_matvec(fhe, dev, small_moduli(), SMALL[0], 2, 3, 3, seed=317, variants=[(False, True)], w_budget=STRADDLE_BUDGET, rot_split=2)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def case_refusals(fhe, dev):
    """Status, fhe_last_error text and an untouched marked `out` for every refusal of both entry points; the empty batch
    with NULL buffers."""
    n, sizes = SMALL
    opar, par = K.params(fhe, n, sizes)
    cs = K.Clients(fhe, opar, par, 2, 319)
    exps = [3, 9]
    _, gks = cs.galois_keys(exps)
    ks = fhe.KeySet([g.ksk for c in range(2) for g in gks[c]])       # 2 clients x 2 exponents
    L = 3
    PLB = L * n * 8
    mark = np.full((2, 2, 2, L, n), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)   # room for either output and an overlapping operand
    out = fhe.DeviceArray.from_numpy(mark)
    ct = fhe.DeviceArray.from_numpy(np.zeros((2, 2, L, n), dtype=np.uint64))
    pts = fhe.DeviceArray.from_numpy(np.zeros((2, L, n), dtype=np.uint64))
    pt0 = fhe.DeviceArray.from_numpy(np.zeros((L, n), dtype=np.uint64))
    po, pc, pp, p0 = (C.c_void_p(a.data_ptr()) for a in (out, ct, pts, pt0))
    ex = (C.c_size_t * 2)(*exps)
    rot, mv = "fhe_bfv_galois_hoisted_keyed_dev", "fhe_bfv_matvec_hoisted_keyed_dev"

    def refused(name, args, code, text):
        st, msg = K.raw(fhe, name, *args)
        assert st == code and text in msg, (name, args, st, msg)
        same(out.download(), mark, ("out was written by a refused call", name, text))

    def both(head, tail_rot, tail_mv, code, text):
        """head: (gks, nclients, exponents, nrot, ct); the tails hold the rest of each call's arguments."""
        refused(rot, tuple(head) + tuple(tail_rot), code, text)
        refused(mv, tuple(head) + tuple(tail_mv), code, text)

    def tails(o=po, batch=2, pts_=pp, pt0_=p0):
        return (o, batch, None), (pts_, 1, pt0_, o, batch, None)

    both((None, 2, ex, 2, pc), *tails(), -1, "null argument: gks")
    both((ks._h, 2, None, 2, pc), *tails(), -1, "null argument: exponents")
    # the three refusals of the client count, each naming both numbers
    both((ks._h, 0, ex, 2, pc), *tails(), -1, "0 clients for a set of 4 keys")
    both((ks._h, 2, ex, 1, pc), *tails(), -1, "2 clients x 1 exponents for a set of 4 keys")
    both((ks._h, 3, ex, 2, pc), *tails(), -1, "3 clients x 2 exponents for a set of 4 keys")
    both((ks._h, 1, ex, 2, pc), *tails(), -1, "1 clients x 2 exponents for a set of 4 keys")
    both((ks._h, 2, ex, 2, pc), *tails(batch=3), -1, "batch 3 is not a multiple of the 2 clients")
    both((ks._h, 2, ex, 2, pc), *tails(batch=1), -1, "batch 1 is not a multiple of the 2 clients")
    # what the unkeyed calls refuse, with their texts
    both((ks._h, 2, (C.c_size_t * 2)(3, 4), 2, pc), *tails(), -10, "InvalidSubstitutionExponent")
    both((ks._h, 2, (C.c_size_t * 2)(3, 2 * n), 2, pc), *tails(batch=0), -10, "InvalidSubstitutionExponent")
    both((ks._h, 2, ex, 2, None), *tails(), -1, "null argument: ct")
    both((ks._h, 2, ex, 2, pc), *tails(o=None), -1, "null argument: out")
    refused(mv, (ks._h, 2, ex, 2, pc, None, 1, p0, po, 2, None), -1, "null argument: pts")
    inside = C.c_void_p(out.data_ptr() + PLB)
    both((ks._h, 2, ex, 2, inside), *tails(), -1, "`out` overlaps `ct`")
    both((ks._h, 2, ex, 2, po), *tails(o=inside), -1, "`out` overlaps `ct`")
    refused(mv, (ks._h, 2, ex, 2, pc, inside, 1, p0, po, 2, None), -1, "`out` overlaps `pts`")
    refused(mv, (ks._h, 2, ex, 2, pc, po, 1, p0, inside, 2, None), -1, "`out` overlaps `pts`")
    refused(mv, (ks._h, 2, ex, 2, pc, pp, 1, inside, po, 2, None), -1, "`out` overlaps `pt0`")
    refused(mv, (ks._h, 2, ex, 2, pc, pp, 1, po, C.c_void_p(out.data_ptr() + PLB // 2), 2, None), -1, "`out` overlaps `pt0`")
    # keys above the ciphertext's level (ciphertexts at level 1, keys at level 0)
    _, up = cs.galois_keys(exps, 1, 0)
    above = fhe.KeySet([g.ksk for c in range(2) for g in up[c]])
    both((above._h, 2, ex, 2, pc), *tails(), -1, "the keys must sit at the ciphertext's level (2 moduli), not above it (3)")
    x = Xfer(dev)
    with pytest.raises(fhe.FheError) as err:
        above.relinearize_hoisted_keyed(2, exps, x.to(np.zeros((2, 2, 2, n), dtype=np.uint64)))
    assert err.value.code == -1 and "at the ciphertext's level" in str(err.value)
    with pytest.raises(fhe.FheError) as err:
        ks.relinearize_hoisted_keyed(2, exps, x.to(np.zeros((2, 3, L, n), dtype=np.uint64)))
    assert err.value.code == -13
    with pytest.raises(fhe.FheError) as err:
        ks.matvec_hoisted_keyed(2, exps, x.to(np.zeros((2, 3, L, n), dtype=np.uint64)), x.to(np.zeros((2, L, n), dtype=np.uint64)))
    assert err.value.code == -13
    with pytest.raises(fhe.FheError) as err:
        ks.matvec_hoisted_keyed(2, exps, x.to(np.zeros((2, 2, L, n), dtype=np.uint64)), x.to(np.zeros((1, L, n), dtype=np.uint64)))
    assert err.value.code == -1 and "DotProductLengthMismatch" in str(err.value)
    with pytest.raises(fhe.FheError) as err:
        ks.relinearize_hoisted_keyed(2, exps, x.to(np.zeros((3, 2, L, n), dtype=np.uint64)))
    assert err.value.code == -1 and "batch 3 is not a multiple of the 2 clients" in str(err.value)
    # the empty batch: a no-op with NULL buffers; a repeated exponent is no refusal
    assert K.raw(fhe, rot, ks._h, 2, ex, 2, None, None, 0, None) == (0, "")
    assert K.raw(fhe, mv, ks._h, 2, ex, 2, None, None, 1, None, None, 0, None) == (0, "")
    assert K.raw(fhe, rot, ks._h, 2, (C.c_size_t * 2)(1, 1), 2, pc, po, 2, None) == (0, "")


def case_evaluation_key_set_errors(fhe, dev, seed=321):
    """EvaluationKeySet.hoisted: its fields, and the errors of EvaluationKey.hoisted for a missing key or a bad step."""
    x = Xfer(dev)
    opar, par = K.params(fhe, *SMALL)
    n = opar.degree()
    cs = K.Clients(fhe, opar, par, 2, seed)
    exps = [pow(3, 1, 2 * n), pow(3, 2, 2 * n), 2 * n - 1]
    ogk, gks = cs.galois_keys(exps)
    eset = fhe.EvaluationKey.batched([fhe.EvaluationKey(n, g) for g in gks])
    h = eset.hoisted(column_rotations=(2, 1), row_rotation=True)
    assert isinstance(h, fhe.KeyedHoistedRotations)
    assert h.nclients == 2 and h.exponents == [exps[1], exps[0], exps[2]] and len(h) == 3 and len(h.set) == 6
    inp = np.stack([ct_arr(cs.encrypt(b)) for b in range(2)])
    out = h.rotate(x.to(inp))
    assert type(out) is type(x.to(inp))
    octx = opar.context_at_level(0)
    for c in range(2):
        same(x.back(out)[c:c + 1], H.ref_rotations(octx, inp[c:c + 1], [ogk[c][e].ksk for e in h.exponents], h.exponents),
             ("EvaluationKeySet.hoisted.rotate", c))
    short = fhe.EvaluationKey.batched([fhe.EvaluationKey(n, g[:2]) for g in gks])
    for kw, what in ((dict(column_rotations=(3,)), "ColumnRotation"), (dict(row_rotation=True), "RowRotation")):
        with pytest.raises(fhe.FheError) as err:
            short.hoisted(**kw)
        assert err.value.code == -11 and "Unsupported(%s)" % what in str(err.value)
    with pytest.raises(fhe.FheError) as err:
        eset.hoisted(column_rotations=(n // 2,))
    assert err.value.code == -1 and "InvalidRotationStep" in str(err.value)
    with pytest.raises(fhe.FheError) as err:
        eset.hoisted()
    assert err.value.code == -1 and "no rotation was asked for" in str(err.value)


# ---- end to end ------------------------------------------------------------------------------------------------------------
def case_end_to_end(fhe, dev, seed=127):
    """Two clients with their own secret and evaluation keys, each encrypting their own 4-periodic SIMD vector at N = 16;
    the server multiplies its 4 x 4 matrix (encoded as in hoist_cases.case_matrix_vector) by both in ONE call.  Each client
    decrypts and decodes their own item to M v_c mod t; the other client's secret key does not give that."""
    x = Xfer(dev)
    n, sizes = SMALL
    opar, par = K.params(fhe, n, sizes)
    t, d, cols = opar.plaintext, 4, n // 2
    g = np.random.default_rng(seed)
    Mx = g.integers(0, t, size=(d, d), dtype=np.uint64)
    vs = [g.integers(0, t, size=d, dtype=np.uint64) for _ in range(2)]
    enc = par.encoder()
    sks = [fhe.SecretKey.random(par, bytes([c * 64 + i for i in range(32)])) for c in range(2)]
    eks = [fhe.EvaluationKey.generate(sk, column_rotations=(1, 2, 3), seeds=[bytes([16 * c + i + 1] * 32) for i in range(3)])
           for c, sk in enumerate(sks)]
    cts = [sk.encrypt(enc.encode(np.tile(v, n // d)[None], scaled=True), a_seeds=[bytes([7 + c] * 32)], e_seeds=[bytes([9 + c] * 32)])
           for c, (sk, v) in enumerate(zip(sks, vs))]
    # the direction of a column rotation, read from the single-rotation call (which has its own oracle tests)
    ramp = np.arange(n, dtype=np.uint64)[None]
    rc = sks[0].encrypt(enc.encode(ramp, scaled=True), a_seeds=[bytes([11] * 32)], e_seeds=[bytes([12] * 32)])
    turned = enc.decode(sks[0].decrypt(eks[0].rotates_columns_by(rc, 1)))[0]
    step = int(turned[0])
    assert step in (1, cols - 1) and list(turned[:cols]) == [(k + step) % cols for k in range(cols)], turned
    diag = np.stack([np.array([Mx[k % d][(k + i * step) % d] for k in range(n)], dtype=np.uint64) for i in range(d)])
    pts = np.asarray(enc.encode(diag))                       # [4, L, N] poly_ntt
    ct = np.concatenate([np.asarray(c) for c in cts])        # [2, 2, L, N]
    h = fhe.EvaluationKey.batched(eks).hoisted(column_rotations=(1, 2, 3))
    prod = x.back(h.matvec(x.to(ct), x.to(np.ascontiguousarray(pts[1:])), x.to(np.ascontiguousarray(pts[0]))))
    assert prod.shape == ct.shape
    for c in range(2):
        want = (Mx.astype(object) @ vs[c].astype(object)) % t
        want = [int(want[k % d]) for k in range(n)]
        got = enc.decode(sks[c].decrypt(prod[c:c + 1]))[0]
        assert [int(a) for a in got] == want, (c, got, want)
        wrong = enc.decode(sks[1 - c].decrypt(prod[c:c + 1]))[0]
        assert [int(a) for a in wrong] != want, ("item %d decrypts under the other client's key" % c)


# ---- shapes the Python oracle is too slow for (GPU suite): H.composed per client, the launches counted ------------------------
FAMILIES = ("hoist_mac_keyed_kernel", "hoist_matvec_keyed_kernel", "hoist_mac_kernel", "hoist_matvec_kernel", "ks_ntt_kernel",
            "ks_mac", "ks_fused", "mbfv_sum_kernel", "dot_kernel")


def launches(fhe, call):
    """({kernel family: launches}, symbols) inside call(), from the engine's profiler."""
    fhe.prof_reset()
    fhe.prof_enable(True)
    try:
        call()
    finally:
        fhe.prof_enable(False)
    count, symbols = {}, []
    for _, sym, n, _ in fhe.prof_entries():
        if n:
            symbols.append(sym)
        for fam in FAMILIES:
            if n and fam in sym:
                count[fam] = count.get(fam, 0) + n
    fhe.prof_reset()
    return count, symbols


def case_large(fhe, dev, q, n, nclients, nrot, per_client, seed, w_budget=0):
    """Uniform keys and ciphertext words: the keyed rotations against H.composed client by client, the keyed matvec
    against those rotations through Context.dot_product_scalar; stage A once per (chunk, key-modulus group), the keyed
    stage B once per pair and table of rotations whatever the client count, nothing of the unkeyed or single-key paths.
    Returns the symbols seen."""
    x = Xfer(dev)
    ky = Keyed(fhe, q, n, nclients, nrot, seed)
    L, batch = len(ky.q), nclients * per_client
    exps = H.odd_exponents(n, nrot, seed)
    ct = ky.inputs(batch, seed)
    pts, pt0 = M.diagonals(np.random.default_rng(seed + 2000), ky.q, n, nrot, batch, True)
    want = np.concatenate([H.composed(fhe, ky.ctx, ky.q, ct[c * per_client:(c + 1) * per_client],
                                      ky.sy.c0[c * nrot:(c + 1) * nrot], ky.sy.c1[c * nrot:(c + 1) * nrot], exps)
                           for c in range(nclients)])
    want_mv = ky.ctx.dot_product_scalar(np.ascontiguousarray(np.concatenate([ct[:, None], want], axis=1)),
                                        np.ascontiguousarray(np.concatenate([pt0[None], pts])))
    ky.set.set_w_budget(w_budget)
    pc, jg = K.chunk_rule(batch, L, L, n, w_budget)
    pairs = -(-batch // pc) * -(-L // jg)
    tables = -(-nrot // TABLE)
    ind, pd, p0d = x.to(ct), x.to(pts), x.to(pt0)
    seen = []
    for fam, call in (("hoist_mac_keyed_kernel", lambda: ky.set.relinearize_hoisted_keyed(nclients, exps, ind)),
                      ("hoist_matvec_keyed_kernel", lambda: ky.set.matvec_hoisted_keyed(nclients, exps, ind, pd, p0d))):
        box = {}
        count, symbols = launches(fhe, lambda: box.setdefault("got", call()))
        seen += symbols
        assert count.get("ks_ntt_kernel") == pairs, (fam, count, symbols)
        assert count.get(fam) == pairs * tables, (fam, count, symbols)
        for other in FAMILIES:
            if other not in (fam, "ks_ntt_kernel", "mbfv_sum_kernel"):
                assert other not in count, (fam, other, symbols)
        same(x.back(box["got"]), want if fam == "hoist_mac_keyed_kernel" else want_mv, (fam, n, nclients, nrot, per_client))
    ky.set.set_w_budget(0)
    return seen
