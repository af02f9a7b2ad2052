"""Cases of the plaintext encoding entry points (fhe_encoder_*, fhe_bfv_encode_dev / decode_dev / add_plain_dev),
shared by tests/test_encode_emu.py (kernel sources under host emulation) and tests/test_encode_gpu.py (the HIP build).
`dev`: as helpers.Xfer -- False (numpy in, numpy out through DeviceArrays), True (torch tensors) or "abi"."""
import random

import numpy as np

import encode_ref as R
from fhe_oracle import bfv as obfv
from fhe_oracle import coracle
from fhe_oracle.rq import Poly, NTT
from helpers import Xfer, arr, ct_arr, ksk_arrays


_opar = {}


def params(fhe, n, t, moduli=None, moduli_sizes=None):
    """(oracle parameters, engine parameters); the oracle's are built once per shape (seconds at n = 16384)."""
    key = (n, t, tuple(moduli or ()), tuple(moduli_sizes or ()))
    if key not in _opar:
        _opar[key] = obfv.BfvParameters(n, t, moduli=moduli, moduli_sizes=moduli_sizes)
    opar = _opar[key]
    return opar, fhe.BfvParameters(n, t, moduli=opar.moduli)


def stock_t(n):
    """default_parameters_128(20)'s plaintext modulus: generate_prime(20, 2n, 2^20 - 1) (parameters.rs:256-260)."""
    from fhe_oracle.zq import generate_prime
    return generate_prime(20, 2 * n, (1 << 20) - 1)


def values(rng, t, batch, nvalues, wide=False):
    """[batch][nvalues] uniform in [0, t) (wide: any u64), drawn from `rng`'s stream."""
    g = np.random.default_rng(rng.getrandbits(64))
    hi = (1 << 64) - 1 if wide else t - 1
    return g.integers(0, hi, size=(batch, nvalues), dtype=np.uint64, endpoint=True)


def case_parity(fhe, dev, opar, par, batches, nvalues_list, levels=None, check_items=None, seed=1, wide=False):
    """encode (Poly / SIMD, unscaled / scaled) and decode against the restatement, every combination of the given
    batches, value counts and levels; check_items(batch) -> item indices compared (default: all).  wide: the inputs of
    both directions are any u64 words (the engine and the restatement reduce them mod t first)."""
    x = Xfer(dev)
    rng = random.Random(seed)
    n, t = opar.degree(), opar.plaintext
    enc = par.encoder()
    levels = (0, opar.max_level()) if levels is None else levels
    cctx = {lv: coracle.CCtx(opar.ctx[lv]) for lv in set(levels)}
    for level in levels:
        for batch in batches:
            for nv in nvalues_list:
                v = values(rng, t, batch, nv, wide)
                items = range(batch) if check_items is None else check_items(batch)
                for encoding in ("poly", "simd"):
                    for scaled in (False, True):
                        got = x.back(enc.encode(x.to(v), encoding, level, scaled))
                        assert got.shape == (batch, len(opar.ctx[level].moduli), n)
                        for b in items:
                            want = R.encode(opar, v[b], encoding, level, scaled, cctx=cctx[level])
                            assert np.array_equal(got[b], want), (encoding, scaled, level, batch, nv, b)
        for batch in batches:
            c = values(rng, t, batch, n, wide)
            for encoding in ("poly", "simd"):
                got = x.back(enc.decode(x.to(c), encoding))
                assert got.shape == (batch, n)
                for b in (range(batch) if check_items is None else check_items(batch)):
                    assert np.array_equal(got[b], R.decode(c[b], t, n, encoding)), (encoding, batch, b)


def _encrypt(sk, opar, pt_rows, level, rng):
    return sk.encrypt_poly(Poly(opar.ctx[level], NTT, [[int(w) for w in r] for r in pt_rows]), rng)


def case_roundtrip_and_rotations(fhe, dev, opar, par, level=0, seed=3):
    """Pins that do not depend on the restatement (evaluation_key.rs:715-731, 764-787; ops/mod.rs:229-257):
    encode -> oracle encrypt -> engine decrypt -> decode is the identity; the engine's Galois rotation by the
    rotates_columns_by(i) exponent rotates each half-row by i, exponent 2N - 1 swaps the halves; mul_plain of two SIMD
    encodings is the slot-wise product."""
    x = Xfer(dev)
    rng = random.Random(seed)
    n, t = opar.degree(), opar.plaintext
    enc = par.encoder()
    sk = obfv.SecretKey.random(opar, rng)
    s_ntt = x.to(arr(sk._s(opar.ctx[level])))
    ctx = par.context_at_level(level)
    v = values(rng, t, 1, n)[0]
    pt = x.back(enc.encode(x.to(v[None]), "simd", level, scaled=True))[0]
    ct = _encrypt(sk, opar, pt, level, rng)

    def dec(ct_rows):
        d = par.decrypt(s_ntt, x.to(np.asarray(ct_rows)[None]), level)
        return x.back(enc.decode(d, "simd"))[0]

    assert dec(ct_arr(ct)).tolist() == v.tolist()
    h = n // 2
    for i in (1, 2, h - 1):
        e = obfv.rot_to_gk_exponent(n, i)
        ogk = obfv.GaloisKey(sk, e, level, level, rng)
        c0, c0s, c1, c1s = ksk_arrays(ogk.ksk)
        gk = fhe.GaloisKey(fhe.KeySwitchingKey(ctx, ctx, c0, c1), e)
        got = dec(x.back(gk.relinearize(x.to(ct_arr(ct)[None])))[0])
        want = list(v[i:h]) + list(v[:i]) + list(v[h + i:]) + list(v[h:h + i])
        assert got.tolist() == [int(w) for w in want], i
    ogk = obfv.GaloisKey(sk, 2 * n - 1, level, level, rng)
    c0, c0s, c1, c1s = ksk_arrays(ogk.ksk)
    gk = fhe.GaloisKey(fhe.KeySwitchingKey(ctx, ctx, c0, c1), 2 * n - 1)
    got = dec(x.back(gk.relinearize(x.to(ct_arr(ct)[None])))[0])
    assert got.tolist() == list(v[h:]) + list(v[:h])
    w = values(rng, t, 1, n)
    pw = x.back(enc.encode(x.to(w), "simd", level))
    prod = x.back(ctx.mul_plain(x.to(ct_arr(ct)[None]), x.to(pw)))[0]
    assert dec(prod).tolist() == [(int(a) * int(b)) % t for a, b in zip(v, w[0])]


def case_add_plain(fhe, dev, opar, par, level=0, batch=3, seed=5):
    """ct +- pt (ops/mod.rs:71-108, 166-203) against the oracle's Ciphertext.add / sub with encode_poly, per-item and
    shared pt, out-of-place and in place (DeviceArray / torch: the result replaces the input buffer's role)."""
    x = Xfer(dev)
    rng = random.Random(seed)
    n, t = opar.degree(), opar.plaintext
    enc = par.encoder()
    sk = obfv.SecretKey.random(opar, rng)
    ctx = par.context_at_level(level)
    cts = [sk.encrypt([rng.randrange(t) for _ in range(n)], rng, level) for _ in range(batch)]
    vals = values(rng, t, batch, n)
    pts = x.back(enc.encode(x.to(vals), "poly", level, scaled=True))
    for b in range(batch):
        assert pts[b].tolist() == sk.encode_poly([int(w) for w in vals[b]], level).coefficients
    cin = np.stack([ct_arr(c) for c in cts])
    for sub in (False, True):
        op = ctx.sub_plain if sub else ctx.add_plain
        got = x.back(op(x.to(cin), x.to(pts)))
        for b in range(batch):
            opt = obfv.Ciphertext(opar, [sk.encode_poly([int(w) for w in vals[b]], level), cts[b].c[1].sub(cts[b].c[1])], level)
            want = cts[b].sub(opt) if sub else cts[b].add(opt)
            assert np.array_equal(got[b], ct_arr(want)), (sub, b)
        got = x.back(op(x.to(cin), x.to(pts[0])))          # one pt shared by the batch
        for b in range(batch):
            opt = obfv.Ciphertext(opar, [sk.encode_poly([int(w) for w in vals[0]], level), cts[b].c[1].sub(cts[b].c[1])], level)
            want = cts[b].sub(opt) if sub else cts[b].add(opt)
            assert np.array_equal(got[b], ct_arr(want)), (sub, b)
    # the decrypted sum is the slot-wise sum (SIMD encodings)
    s_ntt = x.to(arr(sk._s(opar.ctx[level])))
    va, vb = values(rng, t, 1, n), values(rng, t, 1, n)
    ca = _encrypt(sk, opar, x.back(enc.encode(x.to(va), "simd", level, scaled=True))[0], level, rng)
    pb = enc.encode(x.to(vb), "simd", level, scaled=True)
    for sub in (False, True):
        op = ctx.sub_plain if sub else ctx.add_plain
        d = par.decrypt(s_ntt, op(x.to(ct_arr(ca)[None]), pb), level)
        got = x.back(enc.decode(d, "simd"))[0]
        want = [((int(a) - int(b)) if sub else (int(a) + int(b))) % t for a, b in zip(va[0], vb[0])]
        assert got.tolist() == want


def case_add_plain_in_place_abi(fhe, opar, par, level=0, seed=6):
    """fhe_bfv_add_plain_dev with out == ct (the C ABI directly on DeviceArrays)."""
    import ctypes as C
    from fhe_rs_amd import _lib
    rng = random.Random(seed)
    n, t = opar.degree(), opar.plaintext
    sk = obfv.SecretKey.random(opar, rng)
    ctx = par.context_at_level(level)
    ct = sk.encrypt([rng.randrange(t) for _ in range(n)], rng, level)
    v = [rng.randrange(t) for _ in range(n)]
    pt = arr(sk.encode_poly(v, level))
    d_ct, d_pt = fhe.DeviceArray.from_numpy(ct_arr(ct)[None]), fhe.DeviceArray.from_numpy(pt)
    p = C.c_void_p(d_ct.data_ptr())
    fhe.check(_lib.lib().fhe_bfv_add_plain_dev(ctx._h, 0, 2, p, C.c_void_p(d_pt.data_ptr()), 1, p, 1, None))
    opt = obfv.Ciphertext(opar, [sk.encode_poly(v, level), ct.c[1].sub(ct.c[1])], level)
    assert np.array_equal(d_ct.download()[0], ct_arr(ct.add(opt)))
