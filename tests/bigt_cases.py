"""Cases of the entry points for plaintext moduli above 64 bits (fhe_params_create_big, fhe_bfv_encode_big_dev,
fhe_bfv_reduce_big_dev, fhe_bfv_decrypt_big_dev, fhe_mbfv_decrypt_big_dev, fhe_bfv_measure_noise_dev on a big
encoder) and their Python wrappers, shared by tests/test_bigt_emu.py (kernel sources under host emulation) and
tests/test_bigt_gpu.py (the HIP build).  Everything is compared on Python integers with tests/bigt_ref.py and the
oracle.  `dev`: as helpers.Xfer -- False (Python ints in and out, staged through DeviceArrays), True (torch tensors
of limbs) or "abi" (DeviceArrays of limbs)."""
import ctypes as C
import random

import numpy as np

import bigt_ref as R
import encode_cases as E
import encrypt_cases as X
import mbfv_cases as M
from fhe_oracle import bfv as obfv
from fhe_oracle.rq import Poly, NTT
from helpers import Xfer


def params(fhe, name, n):
    """(oracle parameters, engine parameters) of set `name` (bigt_ref.SETS) at degree n, with W_t and P as listed there."""
    t, sizes, wt, p = R.SETS[name]
    opar, par = E.params(fhe, n, t, moduli_sizes=sizes)
    assert par.plaintext == t and par.plaintext_limbs == wt == R.limbs_of(t)
    assert len(opar.plaintext_context.moduli) == p == par.plaintext_context().nmoduli
    return opar, par


def deepest_level(opar):
    """The deepest level whose Q exceeds t."""
    return max(lv for lv in range(opar.max_level() + 1) if opar.ctx[lv].modulus() > opar.plaintext)


def to_limbs(v, wt):
    v = np.asarray(v, dtype=object)
    return np.stack([np.array([(int(a) >> (64 * k)) & (2 ** 64 - 1) for a in v.reshape(-1)], dtype=np.uint64).reshape(v.shape)
                     for k in range(wt)], axis=-1)


def from_limbs(a):
    a = np.asarray(a).astype(object)
    return sum(a[..., k] << (64 * k) for k in range(a.shape[-1]))


def big_in(x, v, wt):
    """Values as the call should see them: Python ints (dev False) or limbs on the device."""
    return x.to(to_limbs(v, wt)) if x.dev else np.asarray(v, dtype=object)


def big_out(x, r):
    return from_limbs(x.back(r)) if x.dev else np.asarray(r, dtype=object)


def oracle_ct(opar, rows, level):
    return obfv.Ciphertext(opar, [Poly(opar.ctx[level], NTT, [[int(w) for w in r] for r in part]) for part in rows], level)


def crafted(opar):
    """The values of the reduction case: the ends of [0, Q_p), both sides of t, of Q_p - t and of multiples of t, the
    middle, and every limb boundary below Q_p."""
    t, qp = opar.plaintext, opar.plaintext_context.modulus()
    xs = [0, 1, t - 1, t, t + 1, qp - t - 1, qp - t, qp - t + 1, qp - 1, qp // 2]
    for j in (2, (qp - 1) // t):
        xs += [(j * t + d - t) % qp for d in (-1, 0, 1)]
    k = 1
    while (1 << (64 * k)) + 1 < qp:
        xs += [(1 << (64 * k)) + d for d in (-1, 0, 1)]
        k += 1
    return xs


def case_reduce(fhe, dev, opar, par):
    """fhe_bfv_reduce_big_dev: one polynomial per crafted x, the value at the first index, the last one or either side
    of a workgroup boundary, small values elsewhere; expected ((x + t) mod Q_p) mod t."""
    x = Xfer(dev)
    n, t = opar.degree(), opar.plaintext
    pm = opar.plaintext_context.moduli
    qp = opar.plaintext_context.modulus()
    xs = crafted(opar)
    assert all(0 <= v < qp for v in xs)
    spots = [0, n - 1] + ([255, 256] if n > 256 else [n // 2 - 1, n // 2])
    cols = np.array([[j % 7 for j in range(n)] for _ in xs], dtype=object)
    for b, v in enumerate(xs):
        cols[b][spots[b % 4]] = v
    polys = np.stack([(cols % q).astype(np.uint64) for q in pm], axis=1)
    got = big_out(x, par.encoder().reduce(x.to(polys)))
    want = np.array([[R.tail(opar, int(v)) for v in row] for row in cols], dtype=object)
    assert got.shape == want.shape == (len(xs), n)
    bad = np.argwhere(got != want)
    assert not len(bad), [(int(b), int(j), hex(int(cols[b][j]))) for b, j in bad[:4]]


def special_values(opar, rng, count):
    t, wt = opar.plaintext, R.limbs_of(opar.plaintext)
    sp = [0, 1, t - 1, t // 2, t, t + 1, (1 << (64 * wt)) - 1]
    return sp + [rng.randrange(t) for _ in range(max(0, count - len(sp)))]


def case_encode(fhe, dev, opar, par, batch=2, seed=1, levels=None):
    """fhe_bfv_encode_big_dev, unscaled and scaled, at level 0 and the deepest level whose Q exceeds t, nvalues 1 and
    N: the Ntt words against the oracle's at N <= 1024; above, ntt_backward of the result against
    (m' mod q_i) delta_i mod q_i -- to_poly in PowerBasis -- on Python integers."""
    x = Xfer(dev)
    rng = random.Random(seed)
    n, t = opar.degree(), opar.plaintext
    wt = R.limbs_of(t)
    enc = par.encoder()
    sp = special_values(opar, rng, 0)
    full = [special_values(opar, rng, n)[:n] for _ in range(batch)]
    if n < len(sp):   # (every special value appears in some item)
        full[-1] = (sp[n:] + full[-1])[:n]
    for level in ((0, deepest_level(opar)) if levels is None else levels):
        L = len(opar.ctx[level].moduli)
        ctx = par.context_at_level(level)
        for vals in (full, [[v] for v in sp]):
            for scaled in (False, True):
                got = x.back(enc.encode(big_in(x, vals, wt), "poly", level, scaled))
                assert got.shape == (len(vals), L, n)
                if n > 1024:
                    got = Xfer(False).back(ctx.ntt_backward(got.copy()))
                for b, v in enumerate(vals):
                    if n <= 1024:
                        want = (R.to_poly if scaled else R.poly_ntt)(opar, v, level).coefficients
                    elif scaled:
                        want = R.to_poly_power_basis(opar, v, level)
                    else:
                        want = [[(a % t) % q for a in v] + [0] * (n - len(v)) for q in opar.ctx[level].moduli]
                    for i in range(L):
                        assert got[b][i].tolist() == [int(w) for w in want[i]], (level, scaled, len(v), b, i)
    # the SIMD encoding does not exist for a big t
    try:
        enc.encode(big_in(x, [[1]], wt), "simd", 0, False)
        raise AssertionError("SIMD encoding of a big t must fail")
    except fhe.FheError as e:
        assert e.code == -22


def keys(fhe, opar, par, seed=5):
    """(engine SecretKey, the oracle's SecretKey with the same coefficients)."""
    sk, osk, _ = X.keys(fhe, opar, par, seed)
    return sk, osk


def case_power_of_the_base(fhe, dev, n, t, sizes):
    """t = 2^(64 (W_t - 1)): the one shape of t whose Barrett constant has W_t + 2 limbs; the tail and the encoder."""
    assert t & (t - 1) == 0 and (t.bit_length() - 1) % 64 == 0
    opar, par = E.params(fhe, n, t, moduli_sizes=sizes)
    assert par.plaintext_limbs == R.limbs_of(t)
    case_reduce(fhe, dev, opar, par)
    case_encode(fhe, dev, opar, par, batch=2)
    case_roundtrip(fhe, dev, opar, par, level=0, batch=2)


def case_roundtrip(fhe, dev, opar, par, level=0, batch=3, seed=11, columns=None):
    """Secret-key and public-key encryption -> decrypt gives the values back and equals bigt_ref's decryption of the
    same ciphertext words; columns: the coefficient indices compared with bigt_ref (default: all)."""
    x = Xfer(dev)
    rng = random.Random(seed)
    n, t = opar.degree(), opar.plaintext
    wt = R.limbs_of(t)
    sk, osk = keys(fhe, opar, par, seed)
    pk = fhe.PublicKey(sk)
    enc = par.encoder()
    vals = [special_values(opar, rng, n)[:4] + [rng.randrange(t) for _ in range(n - 4)] for _ in range(batch)]
    pts = enc.encode(big_in(x, vals, wt), "poly", level, True)
    for ct in (sk.encrypt(pts, level), pk.encrypt(pts, level)):
        dec = big_out(x, enc.decode(sk.decrypt(ct, level), "poly"))
        assert dec.shape == (batch, n)
        assert (dec == np.array(vals, dtype=object) % t).all()
        cth = x.back(ct)
        if not x.dev:   # BfvParameters.decrypt on host arrays: staged, Python ints out
            s_host = X.keys(fhe, opar, par, seed)[2]
            assert (np.asarray(par.decrypt(s_host[:cth.shape[-2]], cth, level), dtype=object) == dec).all()
        if columns is None:
            for b in range(batch):
                assert dec[b].tolist() == R.decrypt(osk, oracle_ct(opar, cth[b], level)), b
        else:
            b = batch - 1
            assert [int(dec[b][j]) for j in columns] == R.decrypt_columns(osk, cth[b], level, columns)


def _enc_const(x, enc, sk, opar, value, level, batch, wt):
    n = opar.degree()
    vals = [[value] + [0] * (n - 1) for _ in range(batch)]
    return sk.encrypt(enc.encode(big_in(x, vals, wt), "poly", level, True), level)


def case_arithmetic(fhe, dev, opar, par, batch=3, seed=13, decrypts=True, parity_items=None):
    """ct + ct of 10 and t - 50 gives t - 40; ct x ct of 10 and t - 20 gives t - 200 on three parts and after
    relinearisation (decrypts False: only bit-parity of the decryption with bigt_ref is asked -- set D has no room for
    the product); Multiplicator.default(...).multiply equals the oracle's, word for word.  parity_items: the items whose
    decryption is compared with bigt_ref (default: all)."""
    x = Xfer(dev)
    n, t = opar.degree(), opar.plaintext
    wt = R.limbs_of(t)
    sk, osk = keys(fhe, opar, par, seed)
    enc = par.encoder()
    ctx = par.context_at_level(0)

    def dec0(ct):
        return big_out(x, sk.decrypt(ct, 0))

    def parity(ct, d):
        cth = x.back(ct)
        for b in (range(batch) if parity_items is None else parity_items):
            assert d[b].tolist() == R.decrypt(osk, oracle_ct(opar, cth[b], 0)), b

    a, b50 = _enc_const(x, enc, sk, opar, 10, 0, batch, wt), _enc_const(x, enc, sk, opar, t - 50, 0, batch, wt)
    d = dec0(ctx.add(_enc_const(x, enc, sk, opar, 10, 0, batch, wt), b50))   # (in place on device arrays)
    assert all(int(d[b][0]) == t - 40 and not any(d[b][1:]) for b in range(batch))
    b20 = _enc_const(x, enc, sk, opar, t - 20, 0, batch, wt)
    m3 = fhe.Multiplicator.default(par, None, 0).tensor(a, b20)
    assert tuple(m3.shape) == (batch, 3, len(opar.moduli), n)
    d3 = dec0(m3)
    parity(m3, d3)
    rk = fhe.RelinearizationKey.generate(sk, seed=bytes(range(32)))
    mult = fhe.Multiplicator.default(par, rk, 0)
    m2 = mult.multiply(a, b20)
    d2 = dec0(m2)
    parity(m2, d2)
    if decrypts:
        for dd in (d3, d2):
            assert all(int(dd[b][0]) == t - 200 and not any(dd[b][1:]) for b in range(batch))
    # the oracle's Multiplicator on the same words and the same relinearisation key
    from helpers import ct_arr
    c0, c1 = (M.host(fhe, k) for k in rk.ksk.export()[:2])
    import keygen_ref
    ork = obfv.RelinearizationKey(ksk=keygen_ref.oracle_key(opar, c0, c1, 0, 0))
    ah, bh = x.back(a), x.back(b20)
    want = obfv.Multiplicator.default(ork).multiply(oracle_ct(opar, ah[0], 0), oracle_ct(opar, bh[0], 0))
    assert np.array_equal(x.back(m2)[0], ct_arr(want))


def case_noise(fhe, dev, opar, par, batch=2, seed=17):
    """measure_noise with m given and m NULL on fresh, three-part and relinearised ciphertexts against bigt_ref's
    restatement (m NULL: against the ciphertext's own decryption by bigt_ref)."""
    x = Xfer(dev)
    rng = random.Random(seed)
    n, t = opar.degree(), opar.plaintext
    wt = R.limbs_of(t)
    sk, osk = keys(fhe, opar, par, seed)
    enc = par.encoder()
    vals = [[rng.randrange(t) for _ in range(n)] for _ in range(batch)]
    fresh = sk.encrypt(enc.encode(big_in(x, vals, wt), "poly", 0, True), 0)
    three = fhe.Multiplicator.default(par, None, 0).tensor(fresh, fresh)
    rk = fhe.RelinearizationKey.generate(sk, seed=bytes(range(32)))
    relin = fhe.Multiplicator.default(par, rk, 0).multiply(fresh, fresh)
    for name, ct in (("fresh", fresh), ("three", three), ("relin", relin)):
        cth = x.back(ct)
        octs = [oracle_ct(opar, cth[b], 0) for b in range(batch)]
        own = [R.decrypt(osk, c) for c in octs]
        got = [int(v) for v in np.asarray(x.back(sk.measure_noise(ct, 0))).reshape(-1)]
        assert got == [R.measure_noise(osk, octs[b], own[b]) for b in range(batch)], name
        given = vals if name == "fresh" else own
        got = [int(v) for v in np.asarray(x.back(sk.measure_noise(ct, 0, big_in(x, given, wt)))).reshape(-1)]
        assert got == [R.measure_noise(osk, octs[b], given[b]) for b in range(batch)], name


def case_multiparty(fhe, dev, opar, par, parties=3, seed=19):
    """Three parties: collective public key, encryption, one decryption share each, fhe_mbfv_decrypt_big_dev equal to the
    plaintext and to the BigUint tail of the summed phase."""
    x = Xfer(dev)
    rng = random.Random(seed)
    g = np.random.default_rng(seed)
    n, t = opar.degree(), opar.plaintext
    wt = R.limbs_of(t)
    octx0 = opar.ctx[0]
    sk, s, _ = M.secrets_of(fhe, x, opar, par, rng, parties)
    crp = M.uniform(g, octx0.moduli, n)
    pk = fhe.PublicKeyShare.aggregate(fhe.PublicKeyShare(sk, fhe.CommonRandomPoly(par, x.to(crp)),
                                                         x.to_bytes(X.seeds(rng, parties))))
    enc = par.encoder()
    vals = [[rng.randrange(t) for _ in range(n)]]
    ct = pk.encrypt(enc.encode(big_in(x, vals, wt), "poly", 0, True), 0, x.to_bytes(X.seeds(rng, 1)))
    d = fhe.DecryptionShare(sk, ct[0], 0, x.to_bytes(X.seeds(rng, parties)))
    coeffs = big_out(x, fhe.DecryptionShare.aggregate(d))
    assert coeffs.tolist() == vals[0]
    # Plaintext::from_shares: c0 + the shares, inverse transform, scale, BigUint tail
    cth, dh = x.back(ct), x.back(d.h_share)
    ph = Poly(octx0, NTT, [[int(w) for w in r] for r in cth[0][0]])
    for p in range(parties):
        ph = ph.add(Poly(octx0, NTT, [[int(w) for w in r] for r in dh[p]]))
    scaled = ph.into_power_basis().scale(opar.plain_scaler[0])
    assert coeffs.tolist() == [R.tail(opar, v) for v in scaled.to_biguints()]


def case_one_limb(fhe, opar_small):
    """fhe_params_create_big with a one-limb t (leading zero limbs trimmed) gives handles whose results equal
    fhe_params_create's: W_t = 1 and the same words from the u64 encoder and the down-scaler's constants."""
    from fhe_rs_amd import _lib
    L = _lib.lib()
    n, t = opar_small.degree(), opar_small.plaintext
    m = np.array(opar_small.moduli, dtype=np.uint64)
    tl = np.array([t, 0, 0], dtype=np.uint64)
    h = C.c_void_p()
    fhe.check(L.fhe_params_create_big(0, n, len(m), m.ctypes.data_as(_lib.u64p), tl.ctypes.data_as(_lib.u64p), 3, C.byref(h)))
    try:
        assert L.fhe_params_plaintext_limbs(h) == 1
        par = fhe.BfvParameters(n, t, moduli=opar_small.moduli)
        assert par.plaintext_limbs == 1
        twin = fhe.BfvParameters.__new__(fhe.BfvParameters)
        twin.__dict__.update(par.__dict__)
        twin._h = h
        v = np.arange(n, dtype=np.uint64)[None]
        for scaled in (False, True):
            assert np.array_equal(twin.encoder().encode(v, "poly", 0, scaled), par.encoder().encode(v, "poly", 0, scaled))
        for which in range(10):
            assert np.array_equal(twin.down_scaler(0).constants(which), par.down_scaler(0).constants(which)), which
        twin._h = None
    finally:
        L.fhe_params_destroy(h)


def case_statuses(fhe, opar, par, opar_small, par_small):
    """Every status of the big entry points, the u64 entry points refusing a big handle, and an empty batch."""
    from fhe_rs_amd import _lib
    L = _lib.lib()
    n, t = opar.degree(), opar.plaintext
    wt = R.limbs_of(t)
    m = np.array(opar.moduli, dtype=np.uint64)
    mp = m.ctypes.data_as(_lib.u64p)

    def create(tv, nlimbs=None, moduli=(m, mp), device=0):
        tl = np.array([(tv >> (64 * k)) & (2 ** 64 - 1) for k in range(nlimbs or max(1, (tv.bit_length() + 63) // 64))],
                      dtype=np.uint64)
        h = C.c_void_p()
        st = L.fhe_params_create_big(device, n, len(moduli[0]), moduli[1], tl.ctypes.data_as(_lib.u64p), len(tl), C.byref(h))
        if st == 0:
            L.fhe_params_destroy(h)
        return st

    q0 = 1
    for q in opar.moduli:
        q0 *= q
    assert create(t) == 0 and create(t, wt + 2) == 0             # (leading zero limbs are trimmed)
    assert create(1 << 62) == -3 and create((1 << 64) - 1) == -3   # InvalidPlaintextModulus
    assert create(1 << 256) == -3 and create((1 << 320) + 1) == -3  # the engine's limit
    # t >= Q on three 50-bit moduli, where Q has three limbs: t = Q, Q + 2 and the largest four-limb t
    m3 = np.array(E.params(fhe, n, 1153, moduli_sizes=[50, 50, 50])[0].moduli, dtype=np.uint64)
    three = (m3, m3.ctypes.data_as(_lib.u64p))
    q3 = int(m3[0]) * int(m3[1]) * int(m3[2])
    assert create(q3 - 2, moduli=three) == 0
    assert create(q3, moduli=three) == -3 and create(q3 + 2, moduli=three) == -3 and create((1 << 256) - 189, moduli=three) == -3
    if q0.bit_length() <= 256:
        assert create(q0) == -3 and create(q0 + 2) == -3
    mult = opar.moduli[1] * ((1 << 64) // opar.moduli[1] + 1)
    assert mult >> 64 and create(mult) == -3                        # a q_i divides t
    assert L.fhe_params_create_big(0, n, len(m), mp, None, 2, C.byref(C.c_void_p())) == -1
    assert L.fhe_params_create_big(0, n, 0, mp, mp, 2, C.byref(C.c_void_p())) == -14
    assert L.fhe_params_plaintext_limbs(None) == 0

    enc, enc_small = par.encoder(), par_small.encoder()
    p = lambda a: C.c_void_p(a.data_ptr())   # noqa: E731
    Lr, P = len(opar.moduli), len(opar.plaintext_context.moduli)
    vals = fhe.DeviceArray.from_numpy(np.zeros((1, n, wt), dtype=np.uint64))
    more = fhe.DeviceArray.from_numpy(np.zeros((1, n + 1, wt), dtype=np.uint64))
    out = fhe.DeviceArray((1, Lr, n))
    assert L.fhe_bfv_encode_big_dev(enc._h, 0, 1, 0, p(vals), n, p(out), 1, None) == 0
    assert L.fhe_bfv_encode_big_dev(enc._h, 1, 1, 0, p(vals), n, p(out), 1, None) == -22
    assert L.fhe_bfv_encode_big_dev(enc._h, 2, 1, 0, p(vals), n, p(out), 1, None) == -1
    assert L.fhe_bfv_encode_big_dev(enc._h, 0, 1, Lr, p(vals), n, p(out), 1, None) == -12
    assert L.fhe_bfv_encode_big_dev(enc._h, 0, 1, 0, p(more), n + 1, p(out), 1, None) == -23
    assert L.fhe_bfv_encode_big_dev(enc._h, 0, 1, 0, None, n, p(out), 1, None) == -1
    assert L.fhe_bfv_encode_big_dev(None, 0, 1, 0, p(vals), n, p(out), 1, None) == -1
    assert L.fhe_bfv_encode_big_dev(enc._h, 0, 1, 0, None, n, None, 0, None) == 0           # an empty batch
    assert L.fhe_bfv_encode_big_dev(enc_small._h, 0, 1, 0, p(vals), n, p(out), 1, None) == -11
    # the u64 entry points never compute with a truncated t
    assert L.fhe_bfv_encode_dev(enc._h, 0, 1, 0, p(vals), n, p(out), 1, None) == -11
    assert L.fhe_bfv_decode_dev(enc._h, 0, p(vals), p(out), 1, None) == -11

    polys = fhe.DeviceArray.from_numpy(np.zeros((1, P, n), dtype=np.uint64))
    lim = fhe.DeviceArray((1, n, wt))
    assert L.fhe_encoder_plain_rows(enc._h) == P and L.fhe_encoder_plain_rows(None) == 0
    assert L.fhe_encoder_plain_rows(enc_small._h) == len(opar_small.plaintext_context.moduli)
    assert L.fhe_bfv_reduce_big_dev(enc._h, p(polys), P, p(lim), 1, None) == 0
    assert L.fhe_bfv_reduce_big_dev(enc._h, None, P, None, 0, None) == 0
    assert L.fhe_bfv_reduce_big_dev(enc._h, None, P, p(lim), 1, None) == -1
    assert L.fhe_bfv_reduce_big_dev(enc_small._h, p(polys), P, p(lim), 1, None) == -11
    # a buffer laid out with another row count is refused before it is read, by the ABI and by the wrapper
    for rows in (0, P - 1, P + 1):
        assert L.fhe_bfv_reduce_big_dev(enc._h, p(polys), rows, p(lim), 1, None) == -11
    for shape in ((1, P - 1, n), (1, P + 1, n), (1, P, n // 2), (n,)):
        try:
            enc.reduce(np.zeros(shape, dtype=np.uint64))
            raise AssertionError("a polynomial of another shape must be refused")
        except fhe.FheError as e:
            assert e.code == -1

    sc = par.plain_scaler(0)
    down = par.down_scaler(0)                      # a scaler that is no cipher -> plain scaler of the set
    sc_small = par_small.plain_scaler(0)
    s = fhe.DeviceArray.from_numpy(np.zeros((Lr, n), dtype=np.uint64))
    ct = fhe.DeviceArray.from_numpy(np.zeros((1, 2, Lr, n), dtype=np.uint64))
    sh = fhe.DeviceArray.from_numpy(np.zeros((1, 1, Lr, n), dtype=np.uint64))
    bits = fhe.DeviceArray((1,))
    assert L.fhe_bfv_decrypt_big_dev(enc._h, sc._h, p(s), p(ct), 2, p(lim), 1, None) == 0
    # the u64 decryptions refuse the big set's scaler, whatever t they are handed
    one = fhe.DeviceArray((1, n))
    for tv in (t & (2 ** 64 - 1), 1153):
        assert L.fhe_bfv_decrypt_dev(sc._h, tv, p(s), p(ct), 2, p(one), 1, None) == -11
        assert L.fhe_mbfv_decrypt_dev(sc._h, tv, p(ct), p(sh), 1, Lr * n, p(one), 1, None) == -11
    hs, hc, ho = np.zeros((Lr, n), dtype=np.uint64), np.zeros((1, 2, Lr, n), dtype=np.uint64), np.zeros((1, n), dtype=np.uint64)
    assert L.fhe_bfv_decrypt(sc._h, 1153, hs.ctypes.data_as(_lib.u64p), hc.ctypes.data_as(_lib.u64p), 2,
                             ho.ctypes.data_as(_lib.u64p), 1) == -11
    assert L.fhe_bfv_decrypt_dev(sc_small._h, 1153, p(s), p(ct), 2, p(one), 1, None) == 0
    assert L.fhe_bfv_decrypt_big_dev(enc._h, sc._h, p(s), p(ct), 0, p(lim), 1, None) == -1
    assert L.fhe_bfv_decrypt_big_dev(enc._h, sc._h, None, None, 2, None, 0, None) == 0
    assert L.fhe_bfv_decrypt_big_dev(enc._h, down._h, p(s), p(ct), 2, p(lim), 1, None) == -11
    assert L.fhe_bfv_decrypt_big_dev(enc._h, sc_small._h, p(s), p(ct), 2, p(lim), 1, None) == -11
    assert L.fhe_bfv_decrypt_big_dev(enc_small._h, sc._h, p(s), p(ct), 2, p(lim), 1, None) == -11
    assert L.fhe_bfv_decrypt_big_dev(enc._h, None, p(s), p(ct), 2, p(lim), 1, None) == -1
    assert L.fhe_mbfv_decrypt_big_dev(enc._h, sc._h, p(ct), p(sh), 1, Lr * n, p(lim), 1, None) == 0
    assert L.fhe_mbfv_decrypt_big_dev(enc._h, sc._h, p(ct), p(sh), 0, Lr * n, p(lim), 1, None) == -1
    assert L.fhe_mbfv_decrypt_big_dev(enc._h, down._h, p(ct), p(sh), 1, Lr * n, p(lim), 1, None) == -11
    assert L.fhe_mbfv_decrypt_big_dev(enc_small._h, sc._h, p(ct), p(sh), 1, Lr * n, p(lim), 1, None) == -11
    assert L.fhe_bfv_measure_noise_dev(enc._h, sc._h, p(s), p(ct), 2, None, p(bits), 1, None) == 0
    assert L.fhe_bfv_measure_noise_dev(enc._h, sc._h, p(s), p(ct), 2, p(lim), p(bits), 1, None) == 0
    assert L.fhe_bfv_measure_noise_dev(enc._h, sc_small._h, p(s), p(ct), 2, None, p(bits), 1, None) == -11
    # a host-only set: creation works, the encoder needs a device
    h = C.c_void_p()
    tl = np.array([(t >> (64 * k)) & (2 ** 64 - 1) for k in range(wt)], dtype=np.uint64)
    fhe.check(L.fhe_params_create_big(-1, n, len(m), mp, tl.ctypes.data_as(_lib.u64p), wt, C.byref(h)))
    try:
        assert L.fhe_params_plaintext_limbs(h) == wt
        assert L.fhe_encoder_create(h, _lib.NTT_TABLES_FN(), None, C.byref(C.c_void_p())) == -18
    finally:
        L.fhe_params_destroy(h)
    # the Python layer never truncates: a big t takes the big constructor, values beyond the limbs are refused
    try:
        enc.encode([[1 << (64 * wt)]], "poly", 0, False)
        raise AssertionError("a value beyond W_t limbs must be refused")
    except fhe.FheError as e:
        assert e.code == -1
