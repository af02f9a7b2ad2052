"""Cases of the wire entry points of key-switching keys (fhe_ksk_load_wire_dev, fhe_ksk_serialize_dev) and their Python
wrappers, shared by tests/test_keyload_emu.py (kernel sources under host emulation) and tests/test_keyload_gpu.py (the
HIP build).  `dev`: as helpers.Xfer.  Expected values: tests/keyload_ref.py.

The bar is equality, bit for bit: a loaded handle exports the arrays fhe_ksk_create makes from the same words, switches
one random polynomial exactly as that handle does in every mode with the F64 switch on and off (the only view of the
twins and F64 words), and serializes back to the bytes it was loaded from."""
import ctypes as C
import random

import numpy as np
import pytest

import encrypt_ref as ER
import keyload_ref as KR
from fhe_oracle.rq import poly_from_wire
from helpers import Xfer


def host(fhe, a):
    if isinstance(a, np.ndarray):
        return a
    if isinstance(a, fhe.DeviceArray):
        return a.download()
    a = a.cpu().numpy()
    return a if a.dtype == np.uint8 else a.view(np.uint64)


def placed(fhe, dev, a, misalign=False):
    """The uint8 array where the engine call reads it; misalign: one byte past the start of its own allocation."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.uint8))
    if not misalign:
        return Xfer(dev).to_bytes(a)
    flat = np.concatenate([np.zeros(1, dtype=np.uint8), a.reshape(-1)])
    if dev is True:
        import torch
        t = torch.from_numpy(flat).cuda()[1:].reshape(a.shape)
    else:
        base = fhe.DeviceArray.from_numpy(flat)
        t = fhe.DeviceArray(a.shape, base.device, 1, _ptr=base._p + 1, _base=base)
    assert t.data_ptr() % 16 == 1 and t.is_contiguous()
    return t


def exported(fhe, key):
    return [host(fhe, a) for a in key.export()]


def check_arrays(fhe, key, k, what):
    c0, c1, c0s, c1s = exported(fhe, key)
    assert key.ndigits == k["nd"] and key.log_base == k["lb"], what
    assert key.mode()["mode"] == fhe.KeySwitchingKey.AUTO, what
    for got, want in ((c0, "c0"), (c1, "c1"), (c0s, "c0s"), (c1s, "c1s")):
        assert np.array_equal(got, k[want]), (what, want)


def check_to_wire(fhe, key, k, seeded, what):
    b0, second = key.to_wire()
    assert np.array_equal(host(fhe, b0), k["w0"]), what
    if seeded:
        assert key.seed == k["K"] and second == k["K"], what
        b0, b1 = key.to_wire(seeded=False)
        assert np.array_equal(host(fhe, b0), k["w0"]), what
    else:
        assert key.seed is None, what
        b1 = second
        with pytest.raises(fhe.FheError):
            key.to_wire(seeded=True)
    assert np.array_equal(host(fhe, b1), k["w1"]), what


def check_switch(fhe, dev, key, k, ct, kc, seed=7):
    """The loaded handle against fhe_ksk_create of the same words: the exports, and key_switch of one random
    polynomial with the mode forced fused and unfused and the F64 switch on and off."""
    x = Xfer(dev)
    twin = fhe.KeySwitchingKey(ct, kc, k["c0"], k["c1"], log_base=k["lb"])
    for a, b in zip(exported(fhe, key), exported(fhe, twin)):
        assert np.array_equal(a, b)
    rng = random.Random(seed)
    p = np.array([[rng.randrange(q) for _ in range(ct.degree)] for q in ct.moduli], dtype=np.uint64)[None]
    modes = [fhe.KeySwitchingKey.FUSED] + ([] if k["lb"] else [fhe.KeySwitchingKey.UNFUSED])
    try:
        for f64 in (True, False):
            fhe.set_f64(f64)
            for mode in modes:
                outs = [[x.back(v) for v in h.set_mode(mode).key_switch(x.to(p))] for h in (key, twin)]
                for a, b in zip(*outs):
                    assert np.array_equal(a, b), (mode, f64)
    finally:
        fhe.set_f64(True)
        key.set_mode(fhe.KeySwitchingKey.AUTO)


def stacked(ks):
    w0, w1 = np.array([k["w0"] for k in ks]), np.array([k["w1"] for k in ks])
    K = np.frombuffer(b"".join(k["K"] for k in ks), dtype=np.uint8).reshape(len(ks), 32)
    return w0, w1, K


def case_load(fhe, dev, opar, par, cl, kl, key_seeds=(1,), misalign=False, check=None, switch=True,
              forms=("seeded", "explicit")):
    """`len(key_seeds)` keys from level cl to level kl in one load call per form; the keys in `check` (None: all)
    against the restatement, fhe_ksk_create's handle (switch) and their own bytes."""
    x = Xfer(dev)
    ct, kc = par.context_at_level(cl), par.context_at_level(kl)
    ks = [KR.key(opar, cl, kl, s) for s in key_seeds]
    w0, w1, K = stacked(ks)
    lb = ks[0]["lb"]
    assert w0.shape[1:] == (ks[0]["nd"], kc.serialized_size)
    for form in forms:
        seeded = form == "seeded"
        if seeded:
            keys = fhe.KeySwitchingKey.from_wire(ct, kc, placed(fhe, dev, w0, misalign), seeds=x.to_bytes(K), log_base=lb)
        else:
            keys = fhe.KeySwitchingKey.from_wire(ct, kc, placed(fhe, dev, w0, misalign), placed(fhe, dev, w1, misalign),
                                                 log_base=lb)
        assert len(keys) == len(ks)
        for b, (key, k) in enumerate(zip(keys, ks)):
            if check is not None and b not in check:
                continue
            what = (form, b, opar.degree(), cl, kl, misalign)
            check_arrays(fhe, key, k, what)
            check_to_wire(fhe, key, k, seeded, what)
            if switch and b == (min(check) if check else 0):
                check_switch(fhe, dev, key, k, ct, kc)
    return keys


def case_single(fhe, dev, opar, par, cl=0, kl=0, **kw):
    """One key given without the leading key dimension."""
    ct, kc = par.context_at_level(cl), par.context_at_level(kl)
    k = KR.key(opar, cl, kl, 1)
    x = Xfer(dev)
    (key,) = fhe.KeySwitchingKey.from_wire(ct, kc, x.to_bytes(k["w0"]), x.to_bytes(k["w1"]), log_base=k["lb"])
    check_arrays(fhe, key, k, "single")
    (key,) = fhe.KeySwitchingKey.from_wire(ct, kc, x.to_bytes(k["w0"]), seeds=k["K"], log_base=k["lb"])
    check_arrays(fhe, key, k, "single seeded")
    assert key.seed == k["K"]


def case_generated_to_wire(fhe, dev, opar, par):
    """to_wire of a key generated on the device carries its seed, and from_wire of that message is the same key."""
    import keygen_cases as G
    sk, _ = G.secret(fhe, opar, par, 5)
    rk = fhe.RelinearizationKey.generate(sk, bytes(range(32)))
    b0, seed = rk.to_wire()
    assert seed == rk.ksk.seed and len(seed) == 32
    ct = par.context_at_level(0)
    back = fhe.RelinearizationKey.from_wire(ct, ct, b0, seed=seed)
    for a, b in zip(exported(fhe, rk.ksk), exported(fhe, back.ksk)):
        assert np.array_equal(a, b)
    assert np.array_equal(host(fhe, back.to_wire()[0]), host(fhe, b0))
    b0x, b1x = rk.to_wire(seeded=False)
    back = fhe.RelinearizationKey.from_wire(ct, ct, b0x, b1x)
    for a, b in zip(exported(fhe, rk.ksk), exported(fhe, back.ksk)):
        assert np.array_equal(a, b)


def case_types(fhe, dev, opar, par):
    """The thin forms: GaloisKey / EvaluationKey.from_wire rotate as the host-made keys do; RGSWCiphertext.from_wire's
    external product equals that of the two host-made keys."""
    x = Xfer(dev)
    ct = par.context_at_level(0)
    n = opar.degree()
    ks = [KR.key(opar, 0, 0, s) for s in (11, 12)]
    w0, w1, K = stacked(ks)
    rng = random.Random(3)
    c = np.array([[[rng.randrange(q) for _ in range(n)] for q in ct.moduli] for _ in range(2)], dtype=np.uint64)[None]
    twins = [fhe.KeySwitchingKey(ct, ct, k["c0"], k["c1"]) for k in ks]
    rgsw = fhe.RGSWCiphertext.from_wire(ct, ct, x.to_bytes(w0), seeds=x.to_bytes(K))
    want = x.back(fhe.RGSWCiphertext(*twins).external_product(x.to(c)))
    assert np.array_equal(x.back(rgsw.external_product(x.to(c))), want)
    rgsw = fhe.RGSWCiphertext.from_wire(ct, ct, x.to_bytes(w0), x.to_bytes(w1))
    assert np.array_equal(x.back(rgsw.external_product(x.to(c))), want)
    for (a0, a1), k in zip(rgsw.to_wire(), ks):
        assert np.array_equal(host(fhe, a0), k["w0"]) and np.array_equal(host(fhe, a1), k["w1"])
    if opar.max_level() > 0:
        with pytest.raises(fhe.FheError) as err:   # a key context below the ciphertext's level
            fhe.RGSWCiphertext.from_wire(par.context_at_level(1), ct, x.to_bytes(w0), x.to_bytes(w1))
        assert err.value.code == -1
    exps = [3, 2 * n - 1]
    ek = fhe.EvaluationKey.from_wire(exps, ct, ct, x.to_bytes(w0), seeds=x.to_bytes(K))
    assert sorted(ek.gk) == exps
    for e, twin in zip(exps, twins):
        want = x.back(fhe.GaloisKey(twin, e).relinearize(x.to(c)))
        assert np.array_equal(x.back(ek.gk[e].relinearize(x.to(c))), want), e
    got_exps, msgs = ek.to_wire()
    assert got_exps == exps and [m[1] for m in msgs] == [k["K"] for k in ks]
    with pytest.raises(fhe.FheError):
        fhe.GaloisKey.from_wire([4, 3], ct, ct, x.to_bytes(w0), x.to_bytes(w1))
    rk = fhe.RelinearizationKey.from_wire(ct, ct, x.to_bytes(w0[0]), x.to_bytes(w1[0]))
    c3 = np.array([[[rng.randrange(q) for _ in range(n)] for q in ct.moduli] for _ in range(3)], dtype=np.uint64)[None]
    assert np.array_equal(x.back(rk.relinearizes(x.to(c3))),
                          x.back(fhe.RelinearizationKey(twins[0]).relinearizes(x.to(c3))))


# ---- the range check ---------------------------------------------------------------------------------------------------
def poke(poly, kc, r, e, value):
    """poly uint8 [poly_bytes] with coefficient e of row r replaced by `value` (its nbits-bit field)."""
    n = kc.degree
    bit = 8 * sum(n * KR.wire_bits(q) // 8 for q in kc.moduli[:r]) + e * KR.wire_bits(kc.moduli[r])
    nbits = KR.wire_bits(kc.moduli[r])
    assert value < (1 << nbits)
    v = int.from_bytes(poly.tobytes(), "little")
    v = (v & ~(((1 << nbits) - 1) << bit)) | (value << bit)
    return np.frombuffer(v.to_bytes(len(poly), "little"), dtype=np.uint8)


def raw_load(fhe, ct, kc, lb, c0, c1, K, nkeys, hs):
    from fhe_rs_amd import _lib
    p = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None   # noqa: E731
    return _lib.lib().fhe_ksk_load_wire_dev(ct._h, kc._h, lb, p(c0), p(c1), p(K), nkeys, None, hs)


def dev_bytes(fhe, dev, a):
    """A device uint8 array with a data_ptr (the raw ABI calls; numpy is not staged there)."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.uint8))
    if dev is True:
        import torch
        return torch.from_numpy(a.copy()).cuda()
    return fhe.DeviceArray.from_numpy(a)


def case_range(fhe, dev, opar, par, cl=0, kl=0, nkeys=2, rows=None, coeffs=None):
    """A word equal to q_j - 1 is accepted (and transformed as the oracle transforms it), one equal to q_j is refused
    with FHE_E_ARG and out[] all NULL: at the first and last coefficient of the first and last row of the last digit of
    the last key, in c0 and in an explicit c1.  (q_j is odd and below 2^nbits, so q_j itself is representable.)
    `rows` / `coeffs` narrow the positions (the emulated run above one LDS tile)."""
    ct, kc = par.context_at_level(cl), par.context_at_level(kl)
    okc = opar.ctx[kl]
    ks = [KR.key(opar, cl, kl, 20 + b) for b in range(nkeys)]
    w0, w1, K = stacked(ks)
    nd, lb, n = ks[0]["nd"], ks[0]["lb"], okc.degree
    rows = sorted({0, len(okc.moduli) - 1}) if rows is None else rows
    for part in (0, 1):
        for r in rows:
            q = okc.moduli[r]
            assert q <= (1 << KR.wire_bits(q)) - 1
            for e in (0, n - 1) if coeffs is None else coeffs:
                for value in (q - 1, q):
                    w = [w0.copy(), w1.copy()]
                    w[part][nkeys - 1, nd - 1] = poke(w[part][nkeys - 1, nd - 1], okc, r, e, value)
                    hs = (C.c_void_p * nkeys)(*([1] * nkeys))
                    d0, d1 = dev_bytes(fhe, dev, w[0]), dev_bytes(fhe, dev, w[1])
                    st = raw_load(fhe, ct, kc, lb, d0, d1, None, nkeys, hs)
                    what = (part, r, e, value == q)
                    if value == q:
                        assert st == -1 and list(hs) == [None] * nkeys, what
                        with pytest.raises(fhe.FheError) as err:
                            fhe.KeySwitchingKey.from_wire(ct, kc, d0, d1, log_base=lb)
                        assert err.value.code == -1 and "not reduced" in str(err.value), what
                        continue
                    assert st == 0 and all(hs), what
                    keys = [fhe.KeySwitchingKey._adopt(ct, kc, h, None, 0) for h in hs]
                    got = exported(fhe, keys[-1])[part][nd - 1]
                    pb = np.array(poly_from_wire(okc, w[part][nkeys - 1, nd - 1].tobytes()).coefficients, dtype=np.uint64)
                    assert np.array_equal(got, ER.Ring.of(okc).c.poly_ntt_forward(pb)), what
    if lb == 0:   # the seeded form checks c0 alike
        bad = w0.copy()
        bad[0, 0] = poke(bad[0, 0], okc, 0, 0, okc.moduli[0])
        hs = (C.c_void_p * nkeys)(*([1] * nkeys))
        assert raw_load(fhe, ct, kc, lb, dev_bytes(fhe, dev, bad), None, dev_bytes(fhe, dev, K), nkeys, hs) == -1
        assert list(hs) == [None] * nkeys


def case_statuses(fhe, dev, opar, par):
    from fhe_rs_amd import _lib
    L = _lib.lib()
    assert opar.max_level() >= 2
    c0, c1 = par.context_at_level(0), par.context_at_level(1)
    top = par.context_at_level(opar.max_level())
    k = KR.key(opar, 0, 0, 1)
    w0, w1, K = stacked([k, k])
    d0, d1, dK = dev_bytes(fhe, dev, w0), dev_bytes(fhe, dev, w1), dev_bytes(fhe, dev, K)
    hs = (C.c_void_p * 2)(1, 1)
    load = lambda ct, kc, lb, a0, a1, sd, nk, out: raw_load(fhe, ct, kc, lb, a0, a1, sd, nk, out)   # noqa: E731
    assert load(c0, c0, 0, d0, d1, dK, 2, hs) == -1 and list(hs) == [None, None]   # both
    hs = (C.c_void_p * 2)(1, 1)
    assert load(c0, c0, 0, d0, None, None, 2, hs) == -1 and list(hs) == [None, None]   # neither
    assert load(c0, c0, 0, None, d1, None, 2, hs) == -1
    assert load(c0, c0, 0, d0, d1, None, 2, None) == -1
    p = lambda a: C.c_void_p(a.data_ptr())   # noqa: E731
    assert L.fhe_ksk_load_wire_dev(None, c0._h, 0, p(d0), p(d1), None, 2, None, hs) == -1
    assert L.fhe_ksk_load_wire_dev(c0._h, None, 0, p(d0), p(d1), None, 2, None, hs) == -1
    assert load(c0, c0, 0, None, None, None, 0, None) == 0   # nkeys == 0: a no-op
    # the geometry, as fhe_ksk_create: key level above the ciphertext level; log_base on several moduli; one key
    # modulus without log_base; a log_base the digits cannot hold
    assert load(c0, c1, 0, d0, d1, None, 2, hs) == -9
    assert load(c0, c0, 5, d0, d1, None, 2, hs) == -11
    assert load(top, top, 0, d0, d1, None, 2, hs) == -17
    assert load(top, top, 63, d0, d1, None, 2, hs) == -1
    assert load(c0, c0, 0, d0, d1, None, 0, None) == 0
    hostctx = fhe.Context(opar.moduli, opar.degree(), device=-1)
    assert load(hostctx, hostctx, 0, d0, d1, None, 2, hs) == -18
    # serialize
    (key,) = fhe.KeySwitchingKey.from_wire(c0, c0, d0[0], d1[0])
    out = dev_bytes(fhe, dev, np.zeros_like(w0[0]))
    assert L.fhe_ksk_serialize_dev(None, p(out), None, None) == -1
    assert L.fhe_ksk_serialize_dev(key._h, None, None, None) == -1
    assert L.fhe_ksk_serialize_dev(key._h, p(out), None, None) == 0
    assert np.array_equal(host(fhe, out), w0[0])
    # the Python layer
    x = Xfer(dev)
    with pytest.raises(fhe.FheError):
        fhe.KeySwitchingKey.from_wire(c0, c0, x.to_bytes(w0))
    with pytest.raises(fhe.FheError):
        fhe.KeySwitchingKey.from_wire(c0, c0, x.to_bytes(w0), x.to_bytes(w1), seeds=K)
    with pytest.raises(fhe.FheError):
        fhe.KeySwitchingKey.from_wire(c0, c0, x.to_bytes(w0[:, :, :-1]), x.to_bytes(w1[:, :, :-1]))
    with pytest.raises(fhe.FheError):
        fhe.KeySwitchingKey.from_wire(c0, c0, x.to_bytes(w0), seeds=K[:1])
