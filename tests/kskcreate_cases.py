"""Cases of key creation from given words (fhe_ksk_create, fhe_ksk_create_dev, fhe_mbfv_relin_key_aggregate_dev), shared
by tests/test_kskcreate_emu.py (kernel sources under host emulation) and tests/test_kskcreate_gpu.py (the HIP build).
`dev`: as helpers.Xfer -- False takes the host form, True and "abi" the device form.

Every handle's twins and F64 words come from one device pass, so the independent definition sits here: the Python
oracle's `coefficients_shoup` (helpers.ksk_arrays) for the twins, and the oracle's key_switch for the F64 words, which
only a key switch shows."""
import ctypes as C
import random

import numpy as np
import pytest

import keygen_cases as G
import mbfv_cases as M
from fhe_oracle import bfv as obfv
from fhe_oracle.rq import NTT_SHOUP, POWER_BASIS
from helpers import Xfer, arr, ksk_arrays, rand_poly
from keyload_cases import exported

EW_THREADS = 256   # ksk_twin_ew_kernel's workgroup: one thread per pair of words
NOT_REDUCED = "key coefficient not reduced"
NOT_THE_TWIN = "Shoup twin is not floor(c * 2^64 / q)"
_keys = {}


def oracle_key(opar, cl, kl, seed=1):
    """A synthetic oracle key from level cl to level kl (uniform NttShoup polynomials: neither the twins nor the key
    switch care whether the key is real), cached and left unchanged: (the oracle's KeySwitchingKey, c0, c0s, c1, c1s)."""
    ident = (id(opar), cl, kl, seed)
    if ident not in _keys:
        rng = random.Random(seed)
        kc = opar.ctx[kl]
        lb = 0
        nd = len(opar.ctx[cl].moduli)
        if len(kc.moduli) == 1:
            log_modulus = (kc.moduli[0] - 1).bit_length()
            lb = log_modulus // 2
            nd = -(-log_modulus // lb)
        c0 = [obfv.random_poly(kc, NTT_SHOUP, rng) for _ in range(nd)]
        c1 = [obfv.random_poly(kc, NTT_SHOUP, rng) for _ in range(nd)]
        oksk = obfv.KeySwitchingKey.from_parts(opar, c0, c1, cl, kl, lb)
        arrays = ksk_arrays(oksk)
        for a in arrays:
            a.setflags(write=False)
        _keys[ident] = (oksk,) + arrays
    return _keys[ident]


def create(fhe, dev, ct, kc, c0, c1, lb):
    x = Xfer(dev)
    return fhe.KeySwitchingKey(ct, kc, x.to(c0), x.to(c1), log_base=lb)


def case_created_arrays(fhe, dev, opar, par, cl=0, kl=0):
    """A handle created without twins exports the oracle's c0, c1 and both twin arrays, bit for bit: every word, so the
    first and last one and both sides of every workgroup boundary of the element-wise pass."""
    oksk, c0, c0s, c1, c1s = oracle_key(opar, cl, kl)
    key = create(fhe, dev, par.context_at_level(cl), par.context_at_level(kl), c0, c1, oksk.log_base)
    assert key.ndigits == c0.shape[0]
    for got, want, name in zip(exported(fhe, key), (c0, c1, c0s, c1s), ("c0", "c1", "c0s", "c1s")):
        diff = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        assert diff.size == 0, (name, dev, cl, kl, "first differing word", int(diff[0]), "of", want.size)
    return c0.size // 2   # the pass's pairs


def case_f64_words(fhe, dev, opar, par):
    """An F64-eligible key: key_switch of one random polynomial with the mode forced fused and unfused, and the F64
    switch on and off, gives the same words each time, and they are the Python oracle's key_switch."""
    oksk, c0, c0s, c1, c1s = oracle_key(opar, 0, 0)
    assert all(q < (1 << 50) for q in opar.ctx[0].moduli) and oksk.log_base == 0
    ctx = par.context_at_level(0)
    x = Xfer(dev)
    key = create(fhe, dev, ctx, ctx, c0, c1, 0)
    p = rand_poly(opar.ctx[0], POWER_BASIS, random.Random(7))
    want = [arr(w) for w in oksk.key_switch(p)]
    try:
        for f64 in (True, False):
            fhe.set_f64(f64)
            for mode in (fhe.KeySwitchingKey.FUSED, fhe.KeySwitchingKey.UNFUSED):
                got = [x.back(v)[0] for v in key.set_mode(mode).key_switch(x.to(arr(p)[None]))]
                for g, w in zip(got, want):
                    assert np.array_equal(g, w), (dev, mode, f64)
    finally:
        fhe.set_f64(True)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def raw_create(fhe, dev, ct, kc, lb, c0, c1, c0s=None, c1s=None):
    """The raw ABI call with *out preset: (status, *out, fhe_last_error())."""
    from fhe_rs_amd import _lib
    L = _lib.lib()
    h = C.c_void_p(1)
    nd = c0.shape[0]
    if dev:
        assert c0s is None and c1s is None
        x = Xfer(dev)
        d0, d1 = x.to(c0), x.to(c1)
        st = L.fhe_ksk_create_dev(ct._h, kc._h, nd, C.c_void_p(d0.data_ptr()), C.c_void_p(d1.data_ptr()), lb, None,
                                  C.byref(h))
    else:
        p = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.POINTER(C.c_uint64))   # noqa: E731
        st = L.fhe_ksk_create(ct._h, kc._h, nd, p(c0), p(c0s), p(c1), p(c1s), lb, C.byref(h))
    msg = L.fhe_last_error().decode(errors="replace") if st else ""
    if st == 0:
        L.fhe_ksk_destroy(h)
    return st, h.value, msg


def refused(fhe, dev, ct, kc, lb, message, *arrays):
    st, h, msg = raw_create(fhe, dev, ct, kc, lb, *arrays)
    assert st == -1 and h is None and message in msg, (st, h, msg)


def case_refusals(fhe, dev, opar, par):
    """FHE_E_ARG, the message and a NULL *out: an unreduced word (q_j and 2^64 - 1; the first and the last word of c0,
    and c1 alone), a wrong twin (host form: c0_shoup alone, c1_shoup alone, off by one in the last word), both faults
    at once (the range check answers), and a creation after each refusal succeeds (the flag word is per call)."""
    oksk, c0, c0s, c1, c1s = oracle_key(opar, 0, 0)
    ctx = par.context_at_level(0)
    moduli = opar.ctx[0].moduli
    first, last = (0, 0, 0), tuple(d - 1 for d in c0.shape)
    ok = lambda: raw_create(fhe, dev, ctx, ctx, 0, c0, c1)[0] == 0   # noqa: E731
    assert ok()
    for part, at in ((0, first), (0, last), (1, first)):
        for value in (moduli[at[1]], (1 << 64) - 1):
            w = [c0.copy(), c1.copy()]
            w[part][at] = np.uint64(value)
            refused(fhe, dev, ctx, ctx, 0, NOT_REDUCED, *w)
            with pytest.raises(fhe.FheError) as err:
                create(fhe, dev, ctx, ctx, w[0], w[1], 0)
            assert err.value.code == -1 and NOT_REDUCED in str(err.value), (part, at, value)
            assert ok()
    if dev:
        return
    bad0, bad1, wrong = c0.copy(), c1s.copy(), c0s.copy()
    bad0[last] = np.uint64(moduli[-1])
    wrong[last] += np.uint64(1)
    bad1[last] -= np.uint64(1)
    refused(fhe, dev, ctx, ctx, 0, NOT_THE_TWIN, c0, c1, wrong, None)
    assert ok()
    refused(fhe, dev, ctx, ctx, 0, NOT_THE_TWIN, c0, c1, None, bad1)
    assert raw_create(fhe, dev, ctx, ctx, 0, c0, c1, c0s, c1s)[0] == 0   # the twins themselves are accepted
    refused(fhe, dev, ctx, ctx, 0, NOT_REDUCED, bad0, c1, wrong, bad1)
    assert ok()


def case_aggregate_refusal(fhe, dev, opar, par):
    """RelinKeyShare.aggregate with an r1_h1 word equal to q_j: FHE_E_ARG and no handle; the same shares with the word
    reduced make a key."""
    x = Xfer(dev)
    octx = opar.ctx[0]
    n, L = opar.degree(), len(octx.moduli)
    g = np.random.default_rng(4)
    h0, h1, r1 = (M.uniform(g, octx.moduli, n, (L,)) for _ in range(3))

    def aggregate(r1_h1):
        share = fhe.RelinKeyShare(par, x.to(h0), x.to(h1))
        share.last_round = fhe.RelinKeyShare(par, None, x.to(r1_h1))
        return fhe.RelinKeyShare.aggregate(share)

    bad = r1.copy()
    bad[L - 1, L - 1, n - 1] = np.uint64(octx.moduli[L - 1])
    with pytest.raises(fhe.FheError) as err:
        aggregate(bad)
    assert err.value.code == -1 and NOT_REDUCED in str(err.value)
    rk = aggregate(r1)
    e0, e1, _, _ = exported(fhe, rk.ksk)
    assert np.array_equal(e1, r1)
    assert np.array_equal(e0, np.stack([M.MR.add_all(octx, [h0[i], h1[i]]) for i in range(L)]))


def params(fhe, n, sizes, t=None):
    import encode_cases as E
    return G.params(fhe, n, t or E.stock_t(n), moduli_sizes=sizes)
