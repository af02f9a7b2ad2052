"""Cases of the lift and noise entry points (fhe_poly_lift_dev, fhe_poly_centered_bits_dev, fhe_bfv_measure_noise_dev)
and their Python wrappers, shared by tests/test_noise_emu.py (kernel sources under host emulation) and
tests/test_noise_gpu.py (the HIP build).  `dev`: as helpers.Xfer -- False (numpy in, numpy out), True (torch tensors) or
"abi" (DeviceArrays).  Every comparison is on integers: the oracle's RnsContext.lift / Poly.to_biguints /
SecretKey.measure_noise, or the formula min(bits(x), bits(q - x)) on Python ints."""
import ctypes as C
import random

import numpy as np

import encode_cases as E
import encrypt_cases as X
from fhe_oracle import bfv as obfv
from fhe_oracle.bfv import generate_moduli
from fhe_oracle.rns import RnsContext
from fhe_oracle.rq import Context as OCtx, Poly, NTT, POWER_BASIS
from helpers import Xfer

# (L, sizes): every L the issue names, moduli of 36 ... 62 bits, and per multi-limb L three sets whose bitlen(q) lands
# just below, on and just above a multiple of 64 (lift_sets() checks the three residues are really met)
LIFT_SIZES = [
    [36], [62],
    [36, 36], [62, 62], [36, 62],
    [43, 42, 42], [44, 42, 42], [45, 42, 42], [50, 50, 40],
    [48, 48, 48, 47], [48, 48, 48, 48], [49, 48, 48, 48], [60, 60, 60, 60],
    [51, 51, 51, 51, 51], [52, 51, 51, 51, 51], [53, 51, 51, 51, 51],
    [57] * 7 + [56, 56], [57] * 8 + [56], [57] * 9,
    [60] * 15 + [59], [60] * 16, [61] + [60] * 15, [62] * 16,
]


def bitlen_q(moduli):
    q = 1
    for m in moduli:
        q *= m
    return q.bit_length()


def lift_sets(n):
    """[(moduli)] for LIFT_SIZES over degree n; asserts the coverage the sizes were chosen for."""
    sets = [generate_moduli(s, n) for s in LIFT_SIZES]
    assert {len(m) for m in sets} == {1, 2, 3, 4, 5, 9, 16}
    assert min(min(m).bit_length() for m in sets) == 36 and max(max(m).bit_length() for m in sets) == 62
    for L in (3, 4, 5, 9, 16):
        res = {bitlen_q(m) % 64 for m in sets if len(m) == L}
        assert res >= {63, 0, 1}, (L, sorted(res))
    return sets


# The compile-time instances lift_kernel<L, BITS> that no set above reaches (with_int_or_generic<1, 16> makes L = 1 ... 16):
# one set per L, widths that mix general, narrow and sub-2^50 moduli, at N = 256 (one workgroup per polynomial).
LIFT_MORE_N = 256
LIFT_MORE_SIZES = [
    [62, 60, 55, 50, 45, 36],
    [61] * 3 + [49] * 4,
    [60] * 8,
    [62, 61, 60, 59, 58, 57, 56, 55, 54, 53],
    [48] * 11,
    [62] * 6 + [36] * 6,
    [58] * 13,
    [50, 62] * 7,
    [62] * 15,
]


def lift_more_sets(n=LIFT_MORE_N):
    """[(moduli)] for LIFT_MORE_SIZES over degree n: exactly the L that lift_sets() leaves out."""
    sets = [generate_moduli(s, n) for s in LIFT_MORE_SIZES]
    assert [len(m) for m in sets] == [6, 7, 8, 10, 11, 12, 13, 14, 15]
    assert {len(m) for m in sets} | {len(s) for s in LIFT_SIZES} == set(range(1, 17))
    return sets


def ints_of(fhe, x, got, w):
    """What Context.lift returned -> [batch][N] Python ints (numpy in: already ints; device in: W limbs each)."""
    if not x.dev:
        return [[int(v) for v in row] for row in got]
    limbs = x.back(got)
    assert limbs.shape[-1] == w
    return [[sum(int(limbs[b][j][k]) << (64 * k) for k in range(w)) for j in range(limbs.shape[1])]
            for b in range(limbs.shape[0])]


def residues(moduli, ints):
    """[N] Python ints -> [L][N] uint64 residues."""
    return np.array([[v % m for v in ints] for m in moduli], dtype=np.uint64)


def case_lift(fhe, dev, n, moduli, batch=2, seed=1, columns=None):
    """Context.lift against the oracle's RnsContext.lift per column (on rows up to 1024 points also through
    Poly.to_biguints): random residues, plus one polynomial of extreme residues (0 and q_i - 1 in every combination
    the columns allow).  columns: the coefficient indices compared (default: all)."""
    x = Xfer(dev)
    rng = random.Random(seed + len(moduli))
    rns = RnsContext(moduli)
    ctx = fhe.Context(moduli, n)
    w = -(-bitlen_q(moduli) // 64)
    assert ctx.lift_limbs == w
    g = np.random.default_rng(rng.getrandbits(64))
    polys = np.stack([np.stack([g.integers(0, m, size=n, dtype=np.uint64) for m in moduli]) for _ in range(batch)])
    ext = np.array([[(m - 1) if (j >> (i % 4)) & 1 else 0 for j in range(n)] for i, m in enumerate(moduli)], dtype=np.uint64)
    polys = np.concatenate([polys, ext[None]])
    inp = x.to(polys)
    got = ints_of(fhe, x, ctx.lift(inp), w)
    if dev:
        assert np.array_equal(x.back(inp), polys)   # polys is not modified
    cols = range(n) if columns is None else columns
    for b in range(len(polys)):
        for j in cols:
            assert got[b][j] == rns.lift([int(polys[b][i][j]) for i in range(len(moduli))]), (moduli, b, j)
        if n <= 1024:
            assert got[b] == Poly(OCtx(moduli, n), POWER_BASIS, [[int(v) for v in r] for r in polys[b]]).to_biguints()


def cbits(v, q):
    return min(v.bit_length(), (q - v).bit_length())


def crafted_values(q):
    """The coefficients of the issue's list: 0, 1, 2, q-1, q-2, (q-1)/2, (q+1)/2 and 2^k - 1, 2^k, q - 2^k, q - 2^k + 1
    for every k that is a limb boundary +- 1 and below bits(q)."""
    vals = [0, 1, 2, q - 1, q - 2, (q - 1) // 2, (q + 1) // 2]
    for j in range(1, q.bit_length() // 64 + 2):
        for k in (64 * j - 1, 64 * j, 64 * j + 1):
            if k < q.bit_length():
                vals += [(1 << k) - 1, 1 << k, q - (1 << k), q - (1 << k) + 1]
    return [v for v in vals if 0 <= v < q]


def case_centered_bits(fhe, dev, n, moduli, seed=2):
    """One polynomial per crafted value: the value sits at the first index, the last, or either side of a workgroup
    boundary (256 coefficients per workgroup; n / 2 on shorter rows), every other coefficient is small (centered bits
    <= 2, 0 where the crafted value itself is that small).  Expected: the formula on Python ints, per polynomial -- a
    wrong reduction, or a maximum leaking across the batch, shows."""
    x = Xfer(dev)
    rng = random.Random(seed)
    q = 1
    for m in moduli:
        q *= m
    ctx = fhe.Context(moduli, n)
    spots = [0, n - 1, 255, 256] if n > 256 else [0, n - 1, n // 2 - 1, n // 2]
    polys, want = [], []
    for i, v in enumerate(crafted_values(q)):
        small = [0] if cbits(v, q) <= 2 else [0, 1, 2, q - 1, q - 2]
        coeffs = [rng.choice(small) for _ in range(n)]
        coeffs[spots[i % 4]] = v
        polys.append(residues(moduli, coeffs))
        want.append(max(cbits(c, q) for c in coeffs))
    assert len(set(want)) > 3
    got = x.back(ctx.centered_bits(x.to(np.stack(polys))))
    assert [int(g) for g in got] == want, (moduli, [(i, int(g), w_) for i, (g, w_) in enumerate(zip(got, want)) if int(g) != w_])
    # without batch dimensions
    one = ctx.centered_bits(x.to(polys[-1]))
    assert int(one if not dev else x.back(one)[0]) == want[-1]


def oracle_ct(opar, rows, level):
    """[nparts][L][N] Ntt words -> the oracle's Ciphertext."""
    return obfv.Ciphertext(opar, [Poly(opar.ctx[level], NTT, [[int(w) for w in r] for r in p]) for p in rows], level)


def noise_of(x, sk, ct, level, m=None):
    """SecretKey.measure_noise as a list of ints; m: host coefficients [batch][N] or None."""
    got = sk.measure_noise(ct, level, plaintext=None if m is None else x.to(m))
    return [int(v) for v in np.atleast_1d(x.back(got))]


_memo = {}


def _memoised(kind, opar, host_ct, level, extra, fn):
    """The oracle runs in Python (seconds per call on the stock sets): one evaluation per distinct input -- the F64-off
    pass of a case feeds it the same ciphertexts."""
    import hashlib
    key = (kind, id(opar), level, hashlib.sha256(np.ascontiguousarray(host_ct).tobytes()).hexdigest(), extra)
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def oracle_noise(opar, osk, host_ct, level, coeffs):
    m = [int(c) for c in coeffs]
    return _memoised("noise", opar, host_ct, level, tuple(m), lambda: osk.measure_noise(oracle_ct(opar, host_ct, level), m))


def oracle_decrypt(opar, osk, host_ct, level):
    return _memoised("decrypt", opar, host_ct, level, None, lambda: osk.decrypt(oracle_ct(opar, host_ct, level)))


def check_noise(x, opar, osk, sk, ct, level, coeffs, items, what):
    """measure_noise with m given == the oracle's SecretKey.measure_noise(ct, values), item by item."""
    got = noise_of(x, sk, ct, level, coeffs)
    host = x.back(ct)
    assert len(got) == host.shape[0]
    for b in items:
        want = oracle_noise(opar, osk, host[b], level, coeffs[b])
        assert got[b] == want, (what, level, b, got[b], want)
    return got


def case_noise_parity(fhe, dev, opar, par, level=0, batch=2, check_items=None, seed=3):
    """Fresh secret-key and public-key ciphertexts, ct x ct without relinearisation (three parts), after
    relinearisation and after a rotation, at `level`: the noise against the expected plaintext equals the oracle's.
    (Keys come from the engine's device key generation; the expected plaintext of ct x ct is the product of the plaintexts; those of the
    relinearised and the rotated ciphertexts are the oracle's decryption of the engine's ciphertexts.)"""
    x = Xfer(dev)
    rng = random.Random(seed)
    n, t = opar.degree(), opar.plaintext
    sk, osk, _ = X.keys(fhe, opar, par, seed)
    sd = lambda count=1: X.seeds(rng, count)   # noqa: E731  (every seed from `rng`: a second pass sees the same ciphertexts)
    pk = fhe.PublicKey(sk, bytes(sd()[0]), bytes(sd()[0]))
    enc = par.encoder()
    items = list(range(batch) if check_items is None else check_items(batch))
    ma, mb = E.values(rng, t, batch, n), E.values(rng, t, batch, n)
    pa, pb = (enc.encode(x.to(m), "poly", level, True) for m in (ma, mb))
    ca, cb = sk.encrypt(pa, level, sd(batch), sd(batch)), pk.encrypt(pb, level, sd(batch))
    fresh_sk = check_noise(x, opar, osk, sk, ca, level, ma, items, "sk")
    fresh_pk = check_noise(x, opar, osk, sk, cb, level, mb, items, "pk")
    assert max(fresh_sk[b] for b in items) <= (2 * opar.variance).bit_length() + 1   # |e| <= 2v

    def decrypted(ct):
        host = x.back(ct)
        out = np.zeros((batch, n), dtype=np.uint64)
        for b in items:
            out[b] = oracle_decrypt(opar, osk, host[b], level)
        return out

    nmod = len(opar.ctx[level].moduli)
    prod3 = fhe.Multiplicator.default(par, None, level).multiply(ca, cb)
    assert tuple(prod3.shape) == (batch, 3, nmod, n)
    # The expected plaintext of the product is the product of the plaintexts, computed here, not the product's own
    # decryption: at a one-modulus level a product no longer decrypts (stock n = 4096, level 2, q of 36 bits, t of 20:
    # 35 bits against the true product, while against its own decryption the figure cannot pass log q - log t = 16
    # bits, the fresh public-key noise of that level), and it is the noise against the plaintext the caller expects
    # that grows with the multiplication (44 > 12 bits at level 0, 48 > 16 at level 1, 35 > 16 at level 2).
    mp = np.zeros((batch, n), dtype=np.uint64)
    for b in items:
        mp[b] = negacyclic_mul(ma[b], mb[b], t)
    n3 = check_noise(x, opar, osk, sk, prod3, level, mp, items, "ct x ct")
    assert min(n3[b] for b in items) > max(fresh_pk[b] for b in items)
    if nmod >= 2:
        rk = fhe.RelinearizationKey.generate(sk, bytes(sd()[0]), level, level)
        prod2 = rk.relinearizes(prod3)
        check_noise(x, opar, osk, sk, prod2, level, decrypted(prod2), items, "relinearised")
    gk = fhe.GaloisKey.generate(sk, [3], sd(), level, level)[0]
    rot = gk.relinearize(ca)
    check_noise(x, opar, osk, sk, rot, level, decrypted(rot), items, "rotated")


def case_null_vs_given(fhe, dev, opar, par, level=0, batch=2, seed=4, decrypts=True):
    """With m NULL the result equals the call with m = the engine's own decrypt output, and the oracle's value for that
    output; the call with m = the encrypted plaintext equals the oracle's value for it.  decrypts (shapes with room
    for the fresh noise): the decryption is the encrypted plaintext, so all of these are one value.  decrypts=False (a
    parameter set whose q leaves no room for a fresh public-key noise above t, stock n = 1024: 27 bits against 20): only
    that one assertion, dec == m, is left out."""
    x = Xfer(dev)
    rng = random.Random(seed)
    n, t = opar.degree(), opar.plaintext
    sk, osk, _ = X.keys(fhe, opar, par, seed)
    sd = lambda count=1: X.seeds(rng, count)   # noqa: E731  (every seed from `rng`: a second pass sees the same ciphertexts)
    pk = fhe.PublicKey(sk, bytes(sd()[0]), bytes(sd()[0]))
    enc = par.encoder()
    m = E.values(rng, t, batch, n)
    pts = enc.encode(x.to(m), "poly", level, True)
    for kind, ct in (("sk", sk.encrypt(pts, level, sd(batch), sd(batch))), ("pk", pk.encrypt(pts, level, sd(batch)))):
        dec = x.back(sk.decrypt(ct, level))
        if decrypts:
            assert np.array_equal(dec, m), kind
        null = noise_of(x, sk, ct, level)
        assert null == check_noise(x, opar, osk, sk, ct, level, dec, range(batch), kind + ", own decryption")
        given = check_noise(x, opar, osk, sk, ct, level, m, range(batch), kind)
        if decrypts:
            assert null == given, kind


def negacyclic_mul(a, b, t):
    """a b mod (x^n + 1, t) for coefficient lists in [0, t)."""
    n = len(a)
    if n * t * t < (1 << 63):   # every partial sum fits an int64: numpy's convolution
        c = np.convolve(np.asarray(a, dtype=np.uint64).astype(np.int64), np.asarray(b, dtype=np.uint64).astype(np.int64))
        c = np.concatenate([c, np.zeros(2 * n - len(c), dtype=np.int64)])
        return [int(v) for v in (c[:n] % t - c[n:] % t) % t]
    out = [0] * n
    for i, u in enumerate(a):
        for j, v in enumerate(b):
            if i + j < n:
                out[i + j] = (out[i + j] + int(u) * int(v)) % t
            else:
                out[i + j - n] = (out[i + j - n] - int(u) * int(v)) % t
    return out


def case_past_decryption_failure(fhe, dev, opar, par, seed=5):
    """Repeated squaring without relinearisation at the one-modulus level until the ciphertext stops decrypting to
    the plaintext product: at every step both forms are checked against the oracle's formula with the respective m --
    the true product for m given, the engine's decryption for m NULL."""
    x = Xfer(dev)
    rng = random.Random(seed)
    n, t = opar.degree(), opar.plaintext
    level = opar.max_level()
    assert len(opar.ctx[level].moduli) == 1
    sk, osk, _ = X.keys(fhe, opar, par, seed)
    enc = par.encoder()
    m = [int(v) for v in E.values(rng, t, 1, n)[0]]
    ct = sk.encrypt(enc.encode(x.to(np.array([m], dtype=np.uint64)), "poly", level, True), level)
    mul = fhe.Multiplicator.default(par, None, level)
    failed = False
    for step in range(4):
        host = x.back(ct)
        oct_ = oracle_ct(opar, host[0], level)
        dec = [int(v) for v in x.back(sk.decrypt(ct, level))[0]]
        given = noise_of(x, sk, ct, level, np.array([m], dtype=np.uint64))[0]
        null = noise_of(x, sk, ct, level)[0]
        assert given == osk.measure_noise(oct_, m), step
        assert null == osk.measure_noise(oct_, dec), step
        if dec != m:
            failed = True
            assert given >= null, (step, given, null)   # m NULL measures against the plaintext it decrypts to
            break
        assert given == null, step
        ct = mul.tensor(ct, ct)
        m = negacyclic_mul(m, m, t)
    assert failed, "the noise never passed decryption failure"


def case_statuses(fhe, opar, par):
    """NULL handle or buffer -> FHE_E_ARG; batch == 0 is a no-op with NULL buffers; a host-only handle ->
    FHE_E_NO_DEVICE; nparts == 0 -> FHE_E_ARG; a scaler whose `from` is not a level of the encoder's parameter set ->
    FHE_E_PARAMETER_MISMATCH."""
    from fhe_rs_amd import _lib
    L = _lib.lib()
    n, nmod = opar.degree(), len(opar.moduli)
    ctx = par.context_at_level(0)
    enc, sc = par.encoder(), par.plain_scaler(0)
    w = ctx.lift_limbs
    polys = fhe.DeviceArray.from_numpy(np.zeros((1, nmod, n), dtype=np.uint64))
    ct = fhe.DeviceArray.from_numpy(np.zeros((1, 2, nmod, n), dtype=np.uint64))
    limbs, bits = fhe.DeviceArray((1, n, w)), fhe.DeviceArray((1,))
    m = fhe.DeviceArray.from_numpy(np.zeros((1, n), dtype=np.uint64))
    p = lambda a: C.c_void_p(a.data_ptr())   # noqa: E731
    assert L.fhe_ctx_lift_limbs(None) == 0
    assert L.fhe_poly_lift_dev(None, p(polys), p(limbs), 1, None) == -1
    assert L.fhe_poly_lift_dev(ctx._h, None, p(limbs), 1, None) == -1
    assert L.fhe_poly_lift_dev(ctx._h, p(polys), None, 1, None) == -1
    assert L.fhe_poly_centered_bits_dev(None, p(polys), p(bits), 1, None) == -1
    assert L.fhe_poly_centered_bits_dev(ctx._h, None, p(bits), 1, None) == -1
    assert L.fhe_poly_centered_bits_dev(ctx._h, p(polys), None, 1, None) == -1
    args = [enc._h, sc._h, p(polys), p(ct), 2, p(m), p(bits), 1, None]
    assert L.fhe_bfv_measure_noise_dev(*args) == 0
    for i in (0, 1, 2, 3, 6):
        bad = list(args)
        bad[i] = None
        assert L.fhe_bfv_measure_noise_dev(*bad) == -1, i
    assert L.fhe_bfv_measure_noise_dev(*(args[:5] + [None] + args[6:])) == 0   # m NULL: the reference's form
    assert L.fhe_bfv_measure_noise_dev(*(args[:4] + [0] + args[5:])) == -1     # nparts == 0
    # batch == 0
    assert L.fhe_poly_lift_dev(ctx._h, None, None, 0, None) == 0
    assert L.fhe_poly_centered_bits_dev(ctx._h, None, None, 0, None) == 0
    assert L.fhe_bfv_measure_noise_dev(enc._h, sc._h, None, None, 2, None, None, 0, None) == 0
    # host-only handles
    host = fhe.Context(opar.moduli, n, device=-1)
    assert host.lift_limbs == w
    assert L.fhe_poly_lift_dev(host._h, p(polys), p(limbs), 1, None) == -18
    assert L.fhe_poly_centered_bits_dev(host._h, p(polys), p(bits), 1, None) == -18
    hsc = fhe.Scaler(host, fhe.Context(opar.moduli[:1], n, device=-1), opar.plaintext, 1 << 40)
    assert L.fhe_bfv_measure_noise_dev(enc._h, hsc._h, p(polys), p(ct), 2, p(m), p(bits), 1, None) == -18
    # a ciphertext context that is no level of the encoder's parameter set
    other = generate_moduli([45] * nmod, n)
    assert other != opar.moduli
    octx = fhe.Context(other, n)
    osc = fhe.Scaler(octx, fhe.Context(other[:1], n), opar.plaintext, 1 << 40)
    assert L.fhe_bfv_measure_noise_dev(enc._h, osc._h, p(polys), p(ct), 2, p(m), p(bits), 1, None) == -11
    # the Python layer: one plaintext row per ciphertext
    sk = fhe.SecretKey.random(par, bytes(32))
    try:
        sk.measure_noise(np.zeros((2, 2, nmod, n), dtype=np.uint64), 0, plaintext=np.zeros((1, n), dtype=np.uint64))
        raise AssertionError("a short plaintext array was accepted")
    except fhe.FheError as err:
        assert err.code == -1
