"""CPU suite (emulated build): every host-pointer entry point fhe_X and its device-pointer twin fhe_X_dev
(include/fhe_hip.h) answer the same invalid call with the same status.  The pairs are read from the header; each
needs a row in ROWS.  Every call here is refused by the argument checks or has an empty batch: nothing is launched,
and the buffers passed as device pointers are never read."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from helpers import ROOT, load_engine

OK, ARG, NO_MORE_CONTEXT, CONTEXT_NOT_REACHABLE = 0, -1, -8, -9
INVALID_LEVEL, MUL_POLY_COUNT, NO_DEVICE, EMPTY_DOT = -12, -13, -18, -19


def declared_pairs():
    text = open(os.path.join(ROOT, "include", "fhe_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(fhe_[a-z0-9_]+)\s*\(", text))
    return sorted(n for n in names if n + "_dev" in names)


def row(args, handles, nbuf, dev=None, empty=(OK, OK), host_only=True, special=()):
    """args(h, b, n): the host form's arguments for handles and scalars h, buffers b, batch n; dev(h, b, n): the
    device form's when they are not args + (stream,).  handles: names in h set to NULL in turn (FHE_E_ARG).  nbuf:
    buffers, each set to NULL in turn at n = 1 (FHE_E_ARG).  empty: (host, device) status with NULL buffers at
    n = 0.  host_only: whether the handles can be host-only (FHE_E_NO_DEVICE).  special: the checks of this
    operation alone, (label, overrides of h, NULL buffers?, status)."""
    return dict(args=args, dev=dev, handles=handles, nbuf=nbuf, empty=empty, host_only=host_only, special=special)


ROWS = {
    "fhe_ntt_forward": row(lambda h, b, n: (h.ctx, b[0], n), ["ctx"], 1),
    "fhe_ntt_backward": row(lambda h, b, n: (h.ctx, b[0], n), ["ctx"], 1),
    "fhe_poly_add": row(lambda h, b, n: (h.ctx, b[0], b[1], n), ["ctx"], 2),
    "fhe_poly_sub": row(lambda h, b, n: (h.ctx, b[0], b[1], n), ["ctx"], 2),
    "fhe_poly_mul": row(lambda h, b, n: (h.ctx, b[0], b[1], n), ["ctx"], 2),
    "fhe_poly_neg": row(lambda h, b, n: (h.ctx, b[0], n), ["ctx"], 1),
    "fhe_poly_mul_shoup": row(lambda h, b, n: (h.ctx, b[0], b[1], b[2], n), ["ctx"], 3),
    # The one exception: the device form refuses in == out (NULL == NULL included) because the kernel does not work
    # in place; the host form stages them into separate blocks.  (test_substitute_in_place_device_form_only)
    "fhe_poly_substitute": row(lambda h, b, n: (h.ctx, 3, b[0], b[1], n, 1), ["ctx"], 2, empty=(OK, ARG)),
    "fhe_poly_serialize": row(lambda h, b, n: (h.ctx, b[0], b[1], n, 0), ["ctx"], 2),
    "fhe_poly_deserialize": row(lambda h, b, n: (h.ctx, b[0], b[1], n, 0), ["ctx"], 2),
    "fhe_poly_switch_down": row(lambda h, b, n: (h.ctx, b[0], b[1], n), ["ctx"], 2, special=[
        ("last level", {"ctx": "last"}, False, NO_MORE_CONTEXT),
        ("last level, NULL buffers", {"ctx": "last"}, True, NO_MORE_CONTEXT)]),
    "fhe_poly_switch_down_to": row(lambda h, b, n: (h.ctx, h.lvl1, b[0], b[1], n), ["ctx", "lvl1"], 2, special=[
        ("target above the source", {"ctx": "lvl1", "lvl1": "ctx"}, False, CONTEXT_NOT_REACHABLE)]),
    "fhe_poly_scale": row(lambda h, b, n: (h.scaler, b[0], b[1], n, 1), ["scaler"], 2),
    "fhe_ksk_create": row(lambda h, b, n: (h.ctx, h.kctx, 3, b[0], None, b[1], None, 0, h.out),
                          ["ctx", "kctx", "out"], 2, empty=None,
                          dev=lambda h, b, n: (h.ctx, h.kctx, 3, b[0], b[1], 0, None, h.out), special=[
        ("key context below the ciphertext's", {"kctx": "lvl1"}, False, CONTEXT_NOT_REACHABLE)]),
    "fhe_key_switch": row(lambda h, b, n: (h.ksk, b[0], b[1], b[2], n), ["ksk"], 3, host_only=False),
    "fhe_bfv_relinearize": row(lambda h, b, n: (h.ksk, b[0], b[1], n), ["ksk"], 2, host_only=False),
    "fhe_bfv_galois": row(lambda h, b, n: (h.ksk, 3, b[0], b[1], n), ["ksk"], 2, host_only=False),
    "fhe_bfv_switch_down": row(lambda h, b, n: (h.ctx, 2, b[0], b[1], n), ["ctx"], 2, special=[
        ("last level", {"ctx": "last"}, False, NO_MORE_CONTEXT),
        ("last level, NULL buffers", {"ctx": "last"}, True, NO_MORE_CONTEXT)]),
    "fhe_bfv_switch_to_level": row(lambda h, b, n: (h.ctx, h.levels, 2, b[0], b[1], n), ["ctx"], 2, special=[
        ("levels beyond the chain", {"levels": "three"}, False, INVALID_LEVEL)]),
    "fhe_bfv_dot_product_scalar": row(lambda h, b, n: (h.ctx, 2, h.count, b[0], 0, b[1], 0, b[2], n), ["ctx"], 3,
                                      special=[("count 0", {"count": "zero"}, False, EMPTY_DOT),
                                               ("count 0, NULL buffers", {"count": "zero"}, True, EMPTY_DOT)]),
    "fhe_bfv_mul_plain": row(lambda h, b, n: (h.ctx, 2, b[0], b[1], 0, b[2], n), ["ctx"], 3),
    "fhe_bfv_rgsw_mul": row(lambda h, b, n: (h.ksk, h.ksk1, b[0], b[1], n), ["ksk", "ksk1"], 2, host_only=False),
    "fhe_bfv_inner_sum": row(lambda h, b, n: (h.gks, h.exps, h.ngk, b[0], b[1], n), ["gks", "exps", "ngk"], 2,
                             host_only=False),
    "fhe_poly_from_seed": row(lambda h, b, n: (h.ctx, b[0], b[1], n), ["ctx"], 2),
    # (s_ntt is needed at any batch)
    "fhe_bfv_decrypt": row(lambda h, b, n: (h.scaler, 65537, b[0], b[1], 2, b[2], n), ["scaler"], 3, empty=(ARG, ARG)),
    "fhe_bfv_expand": row(lambda h, b, n: (h.gks, h.ngk, b[0], b[1], 2, n), ["gks", "ngk"], 2, host_only=False),
    "fhe_bfv_mul": row(lambda h, b, n: (h.mul, b[0], b[1], b[2], n), ["mul"], 3),
    "fhe_bfv_tensor": row(lambda h, b, n: (h.mul, h.parts, 2, b[0], b[1], b[2], n), ["mul"], 3, special=[
        ("lhs without parts", {"parts": "zero"}, False, MUL_POLY_COUNT)]),
}


@pytest.fixture(scope="module")
def env():
    fhe = load_engine("emu")
    from fhe_rs_amd import _lib
    keep = []

    def params(device):
        p = fhe.BfvParameters(16, 65537, moduli_sizes=[50, 50, 50], device=device)
        keep.append(p)
        c = [p.context_at_level(i) for i in range(3)]
        s = p.extender(0)
        m = fhe.Multiplicator(p.extender(0), p.extender(0), p.down_scaler(0))
        keep.extend(c + [s, m])
        return c, s, m

    (ctx, lvl1, last), scaler, mul = params(0)
    (ctx_h, lvl1_h, _), scaler_h, mul_h = params(-1)
    zeros = np.zeros((3, 3, 16), dtype=np.uint64)
    ksk = fhe.KeySwitchingKey(ctx, ctx, zeros, zeros)
    keep.append(ksk)
    out = C.c_void_p()
    gks = (C.c_void_p * 1)(ksk._h.value)
    gks_null = (C.c_void_p * 1)(None)
    exps = (C.c_size_t * 1)(3)
    h = lambda x: x._h.value
    values = dict(ctx=h(ctx), lvl1=h(lvl1), last=h(last), kctx=h(ctx), scaler=h(scaler), mul=h(mul), ksk=h(ksk),
                  ksk1=h(ksk), gks=C.addressof(gks), exps=C.addressof(exps), ngk=1, out=C.addressof(out), levels=1,
                  count=2, parts=2, zero=0, three=3)
    host_only = dict(ctx=h(ctx_h), lvl1=h(lvl1_h), kctx=h(ctx_h), scaler=h(scaler_h), mul=h(mul_h))
    # a NULL handle: the pointer, or for a key list no key / a NULL key
    nulls = dict(ngk=[0], gks=[None, C.addressof(gks_null)])
    bufs = np.zeros((4, 8192), dtype=np.uint64)   # distinct non-NULL buffers, larger than any call here would touch
    keep += [gks, gks_null, exps, out, bufs]
    return types.SimpleNamespace(lib=_lib.lib(), values=values, host_only=host_only, nulls=nulls, keep=keep,
                                 bufs=[bufs[i].ctypes.data for i in range(4)])


def _call(env, fn, args):
    f = getattr(env.lib, fn)
    conv = []
    for a, t in zip(args, f.argtypes):
        if isinstance(a, int) and t is not None and issubclass(t, C._Pointer):
            a = C.cast(C.c_void_p(a), t)
        conv.append(a)
    return f(*conv)


def statuses(env, name, overrides=None, null_bufs=(), n=1):
    """(host status, device status) of one call: handle values overridden, the buffers at null_bufs NULL."""
    r = ROWS[name]
    h = types.SimpleNamespace(**dict(env.values, **(overrides or {})))
    b = [None if i in null_bufs else env.bufs[i] for i in range(r["nbuf"])]
    host = r["args"](h, b, n)
    dev = r["dev"](h, b, n) if r["dev"] else host + (None,)   # (the stream comes last: NULL, the null stream)
    return _call(env, name, host), _call(env, name + "_dev", dev)


PAIRS = declared_pairs()


def test_every_pair_has_a_row():
    assert len(PAIRS) >= 28
    assert set(PAIRS) == set(ROWS), set(PAIRS) ^ set(ROWS)


@pytest.mark.parametrize("name", PAIRS)
def test_null_handle(env, name):
    for attr in ROWS[name]["handles"]:
        for v in env.nulls.get(attr, [None]):
            assert statuses(env, name, {attr: v}) == (ARG, ARG), attr


@pytest.mark.parametrize("name", PAIRS)
def test_null_buffer(env, name):
    for i in range(ROWS[name]["nbuf"]):
        assert statuses(env, name, null_bufs=(i,)) == (ARG, ARG), i


@pytest.mark.parametrize("name", [p for p in PAIRS if ROWS[p]["empty"] is not None])
def test_null_buffers_empty_batch(env, name):
    r = ROWS[name]
    assert statuses(env, name, null_bufs=range(r["nbuf"]), n=0) == r["empty"]


@pytest.mark.parametrize("name", [p for p in PAIRS if ROWS[p]["host_only"]])
def test_host_only_handle(env, name):
    assert statuses(env, name, env.host_only) == (NO_DEVICE, NO_DEVICE)


@pytest.mark.parametrize("name,label", [(p, s[0]) for p in PAIRS for s in ROWS[p]["special"]])
def test_operation_checks(env, name, label):
    _, over, null, want = next(s for s in ROWS[name]["special"] if s[0] == label)
    over = {k: env.values[v] for k, v in over.items()}
    assert statuses(env, name, over, null_bufs=range(ROWS[name]["nbuf"]) if null else ()) == (want, want)


def test_substitute_in_place_device_form_only(env):
    """The device form refuses in == out; the host form is not called here (it would run: it accepts in == out)."""
    b = env.bufs[0]
    assert _call(env, "fhe_poly_substitute_dev", (env.values["ctx"], 3, b, b, 1, 1, None)) == ARG
