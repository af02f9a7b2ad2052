"""Cases of the entry points that build plaintexts from packed bits (fhe_bfv_encode_bytes_dev, fhe_bfv_encode_words_dev,
fhe_transcode_dev) and their Python wrappers, shared by tests/test_transcode_emu.py (kernel sources under host
emulation) and tests/test_transcode_gpu.py (the HIP build).  `dev`: as helpers.Xfer -- False (numpy in, numpy out) or True
(torch tensors); pointers at odd offsets are DeviceArray views under emulation and tensor slices on the GPU.

Expected values: tests/transcode_ref.py (the transcoders) and tests/encode_ref.py (Poly encoding of the values), i.e. the
restatements of encode_database (crates/fhe/examples/util.rs:97-145) and of the SealPIR fold (sealpir.rs:176-200) below.
Every output word is compared."""
import ctypes as C
import random

import numpy as np

import encode_ref as ER
import transcode_ref as T
from fhe_oracle import bfv as obfv
from fhe_oracle import coracle
from fhe_oracle.zq import generate_prime
from helpers import Xfer

ARG, PARAMETER_MISMATCH, INVALID_LEVEL, TOO_MANY_VALUES = -1, -11, -12, -23
WIDTHS = (1, 7, 8, 13, 20, 36, 61, 62, 63, 64)
NINS = (1, 2, 9, 64, 257)


# ---- the restatements --------------------------------------------------------------------------------------------------
def database_values(data, item_bytes, nbits, batch):
    """encode_database: the values of item b, transcode_from_bytes of bytes [b item_bytes, (b + 1) item_bytes) of `data`
    cut at its end (what lies beyond is zero, and trailing zero values are the zero padding of the plaintext)."""
    data = bytes(data)
    return [T.transcode(data[b * item_bytes:(b + 1) * item_bytes], 8, nbits) for b in range(batch)]


def fold_values(segments, in_bits, nbits, n):
    """The fold: every segment through transcode_bidirectional, the lists appended, cut into chunks of n values."""
    v = []
    for s in segments:
        v += T.transcode([int(w) for w in s], in_bits, nbits)
    return [v[i:i + n] for i in range(0, len(v), n)]


def plaintext_rows(opar, values, level, scaled, cctx=None):
    """Plaintext::try_encode(values, Encoding::poly_at_level(level)).poly_ntt (scaled: to_poly) as [L][N] uint64."""
    return ER.encode(opar, values, "poly", level, scaled, cctx=cctx)


# ---- helpers -----------------------------------------------------------------------------------------------------------
_opar = {}


def params(fhe, n, t, sizes):
    key = (n, t, tuple(sizes))
    if key not in _opar:
        _opar[key] = obfv.BfvParameters(n, t, moduli_sizes=sizes)
    opar = _opar[key]
    return opar, fhe.BfvParameters(n, t, moduli=opar.moduli)


def plaintext_modulus(bits, n, sizes):
    """devop_shapes.plaintext_prime; where no prime of `bits` bits is 1 mod 2n (Poly encoding does not need one), the
    largest prime of that width."""
    import devop_shapes as S
    q = obfv.generate_moduli(sizes, n)
    t = S.plaintext_prime(bits, n, q)
    if t is None:
        t = 3 if bits == 2 else generate_prime(bits, 2, 1 << bits)
    assert t is not None and t.bit_length() == bits and t not in q
    return t


def ilog2(t):
    return t.bit_length() - 1


def host(fhe, a):
    if isinstance(a, np.ndarray):
        return a
    if isinstance(a, fhe.DeviceArray):
        return a.download()
    a = a.cpu().numpy()
    return a if a.dtype == np.uint8 else a.view(np.uint64)


def placed(fhe, dev, a, off=0, fill=0xFF, tail=24):
    """The uint8 array `a` on the device as an interior view: `off` bytes past the start of an allocation whose other
    bytes (the `off` in front, `tail` behind) are `fill`."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.uint8)).reshape(-1)
    flat = np.concatenate([np.full(off, fill, dtype=np.uint8), a, np.full(tail, fill, dtype=np.uint8)])
    if dev is True:
        import torch
        return torch.from_numpy(flat).cuda()[off:off + a.size]
    base = fhe.DeviceArray.from_numpy(flat)
    return fhe.DeviceArray((a.size,), base.device, 1, _ptr=base._p + off, _base=base)


def rand_bytes(rng, n):
    return np.frombuffer(rng.randbytes(n), dtype=np.uint8) if n else np.zeros(0, dtype=np.uint8)


# ---- fhe_transcode_dev -------------------------------------------------------------------------------------------------
def case_transcode(fhe, dev, in_widths=WIDTHS, out_widths=WIDTHS, nins=NINS, batch=3, seed=1):
    """Every (in_bits, out_bits) pair, u64 on both sides and bytes on a side of 8 bits (and of 7 and 1: a byte may carry
    fewer); input words with random bits above in_bits, which the mask removes; every output word."""
    x = Xfer(dev)
    rng = random.Random(seed)
    for ib in in_widths:
        for ob in out_widths:
            for nin in nins:
                a = np.array([[rng.getrandbits(64) for _ in range(nin)] for _ in range(batch)], dtype=np.uint64)
                want = np.array([T.transcode(r, ib, ob) for r in a.tolist()], dtype=np.uint64)
                assert want.shape == (batch, T.count(nin, ib, ob))
                got = x.back(fhe.transcode(x.to(a), ib, ob))
                assert got.dtype == np.uint64 and np.array_equal(got, want), (ib, ob, nin)
                if ob <= 8:
                    got = x.back_bytes(fhe.transcode(x.to(a), ib, ob, out_bytes=True))
                    assert got.dtype == np.uint8 and np.array_equal(got, want.astype(np.uint8)), (ib, ob, nin, "to bytes")
                if ib <= 8:
                    a8 = (a & np.uint64(0xFF)).astype(np.uint8)   # (for ib < 8 the high bits of each byte are set too)
                    got = x.back(fhe.transcode(x.to_bytes(a8), ib, ob))
                    assert np.array_equal(got, want), (ib, ob, nin, "from bytes")
                    if ob <= 8:
                        got = x.back_bytes(fhe.transcode(x.to_bytes(a8), ib, ob, out_bytes=True))
                        assert np.array_equal(got, want.astype(np.uint8)), (ib, ob, nin, "bytes to bytes")


def case_transcode_misc(fhe, dev):
    """Leading dimensions, `bytes` input, an empty row, and the counts."""
    from fhe_rs_amd import _lib
    L = _lib.lib()
    x = Xfer(dev)
    rng = random.Random(2)
    a = np.array([[[rng.getrandbits(36) for _ in range(9)] for _ in range(3)] for _ in range(2)], dtype=np.uint64)
    got = x.back(fhe.transcode(x.to(a), 36, 20))
    assert got.shape == (2, 3, 17)
    assert got.tolist() == [[T.transcode(r, 36, 20) for r in m] for m in a.tolist()]
    raw = rng.randbytes(13)
    assert fhe.transcode(raw, 8, 20).tolist() == T.transcode(raw, 8, 20)
    assert fhe.transcode(np.zeros((2, 0), dtype=np.uint64), 20, 36).shape == (2, 0)
    for ib, nin, ob in ((36, 4096, 20), (8, 10080, 20), (1, 1, 64), (64, 3, 1)):
        assert L.fhe_transcode_count(ib, nin, ob) == T.count(nin, ib, ob)
    assert L.fhe_transcode_count(36, 4096, 20) == 7373
    assert fhe.number_elements_per_plaintext(4096, 20, 288) == 35


# ---- fhe_bfv_encode_bytes_dev ------------------------------------------------------------------------------------------
def check_bytes(fhe, dev, opar, enc, cctx, data, item_bytes, nbits, batch, level, scaled, off=None, what=()):
    """One encode_bytes call against the restatement.  off = None: `data` as Xfer places it; an int: an interior view
    `off` bytes into an allocation, run once with the surroundings 0xFF and once 0x00 -- the same output."""
    n = opar.degree()
    if off is None:
        got = host(fhe, enc.encode_bytes(Xfer(dev).to_bytes(data), item_bytes, nbits, level, scaled, batch=batch))
    else:
        got = host(fhe, enc.encode_bytes(placed(fhe, dev, data, off, 0xFF), item_bytes, nbits, level, scaled, batch=batch))
        again = host(fhe, enc.encode_bytes(placed(fhe, dev, data, off, 0x00), item_bytes, nbits, level, scaled, batch=batch))
        assert np.array_equal(got, again), ("the surroundings were read", what, off)
    assert got.shape == (batch, len(opar.ctx[level].moduli), n), what
    for b, v in enumerate(database_values(data, item_bytes, nbits, batch)):
        assert len(v) <= n
        assert np.array_equal(got[b], plaintext_rows(opar, v, level, scaled, cctx)), (what, b, off)
    return got


def case_encode_bytes(fhe, dev, opar, par, seed=3, full=True):
    """nbits = ilog2(t), level 0 and the deepest, unscaled and scaled.  Per form: item sizes 5 and 13 (odd; where the
    plaintext holds that many bits) and the largest that fits, each with three full items, a short fourth and two items
    wholly past the end of the data; then (full) on the first and last form the source at byte offsets 1 and 7 inside a
    guarded allocation, an empty source, and a source of 0xFF bytes."""
    rng = random.Random(seed)
    n, t = opar.degree(), opar.plaintext
    nbits = ilog2(t)
    enc = par.encoder()
    cap = n * nbits // 8
    assert cap >= 1
    sizes = sorted({s for s in (5, 13, cap) if s <= cap})
    levels = sorted({0, opar.max_level()})
    forms = [(lv, sc) for lv in levels for sc in (False, True)]
    partial = False
    for level, scaled in forms:
        cctx = coracle.CCtx(opar.ctx[level])
        for ib in sizes:
            partial |= (ib * 8) % nbits != 0
            data = rand_bytes(rng, 3 * ib + ib // 2)
            check_bytes(fhe, dev, opar, enc, cctx, data, ib, nbits, 6, level, scaled, what=(n, t, level, scaled, ib))
        if not full or (level, scaled) not in (forms[0], forms[-1]):
            continue
        ib = sizes[-1]
        data = rand_bytes(rng, 2 * ib + max(ib - 1, 0))
        for off in (1, 7):
            check_bytes(fhe, dev, opar, enc, cctx, data, ib, nbits, 3, level, scaled, off=off, what=(n, t, "offset"))
        check_bytes(fhe, dev, opar, enc, cctx, np.zeros(0, dtype=np.uint8), ib, nbits, 2, level, scaled, what=(n, t, "empty"))
        ones = np.full(2 * ib, 0xFF, dtype=np.uint8)
        check_bytes(fhe, dev, opar, enc, cctx, ones, ib, nbits, 2, level, scaled, what=(n, t, "0xFF"))
        check_bytes(fhe, dev, opar, enc, cctx, ones, ib, nbits, 2, level, scaled, off=1, what=(n, t, "0xFF offset"))
    return partial


def case_encode_bytes_defaults(fhe, dev, opar, par):
    """`bytes` input, the default nbits and batch (ceil(len / item_bytes): the short last item)."""
    rng = random.Random(4)
    n, t = opar.degree(), opar.plaintext
    ib = min(13, n * ilog2(t) // 8)
    raw = rng.randbytes(2 * ib + 1)
    got = par.encoder().encode_bytes(raw, ib)
    assert got.shape == (3, len(opar.moduli), n)
    for b, v in enumerate(database_values(raw, ib, ilog2(t), 3)):
        assert np.array_equal(got[b], plaintext_rows(opar, v, 0, False))


# ---- fhe_bfv_encode_words_dev ------------------------------------------------------------------------------------------
def check_words(fhe, dev, opar, enc, cctx, words, in_bits, nbits, level, scaled, what=()):
    x = Xfer(dev)
    n = opar.degree()
    words = np.asarray(words, dtype=np.uint64)
    got = x.back(enc.encode_words(x.to(words), in_bits, nbits, level, scaled))
    lead = words.shape[:-2]
    nseg, seg_len = words.shape[-2:]
    nplain = -(-nseg * T.count(seg_len, in_bits, nbits) // n)
    assert got.shape == lead + (nplain, len(opar.ctx[level].moduli), n), what
    flat_w, flat_g = words.reshape((-1, nseg, seg_len)), got.reshape((-1,) + got.shape[len(lead):])
    for b in range(flat_w.shape[0]):
        chunks = fold_values(flat_w[b], in_bits, nbits, n)
        assert len(chunks) == nplain
        for p, v in enumerate(chunks):
            assert np.array_equal(flat_g[b, p], plaintext_rows(opar, v, level, scaled, cctx)), (what, b, p)
    return nplain


def case_encode_words(fhe, dev, opar, par, pairs=((36, 20), (20, 20), (13, 34)), nsegs=(1, 2), seg_lens=None, batch=3,
                      seed=5, forms=None):
    """Words with random bits above in_bits; seg_len = N and the given other lengths; level 0 / deepest, both scalings."""
    rng = random.Random(seed)
    n = opar.degree()
    enc = par.encoder()
    levels = sorted({0, opar.max_level()})
    forms = forms or [(levels[0], False), (levels[-1], True)]
    seen = {}
    for level, scaled in forms:
        cctx = coracle.CCtx(opar.ctx[level])
        for in_bits, nbits in pairs:
            for nseg in nsegs:
                for seg_len in (n,) + tuple(seg_lens or ()):
                    w = np.array([[[rng.getrandbits(64) for _ in range(seg_len)] for _ in range(nseg)]
                                  for _ in range(batch)], dtype=np.uint64)
                    seen[(in_bits, nbits, nseg, seg_len)] = check_words(
                        fhe, dev, opar, enc, cctx, w, in_bits, nbits, level, scaled, (n, in_bits, nbits, nseg, seg_len))
    return seen


# ---- refusals ----------------------------------------------------------------------------------------------------------
def case_statuses(fhe, dev, opar, par, par_big):
    """Every refusal with its status, through the C ABI itself."""
    from fhe_rs_amd import _lib
    L = _lib.lib()
    n, t = opar.degree(), opar.plaintext
    nbits = ilog2(t)
    enc, big = par.encoder(), par_big.encoder()
    nl = len(opar.moduli)
    p = lambda a: C.c_void_p(a.data_ptr())   # noqa: E731
    cap = n * nbits // 8
    src = placed(fhe, dev, np.zeros(cap + 8, dtype=np.uint8), 0)
    words = fhe.DeviceArray.from_numpy(np.zeros((2, n), dtype=np.uint64)) if dev is not True else Xfer(dev).to(np.zeros((2, n), dtype=np.uint64))
    out = fhe.DeviceArray((8, nl, n)) if dev is not True else Xfer(dev).to(np.zeros((8, nl, n), dtype=np.uint64))
    eb, ew, tr = L.fhe_bfv_encode_bytes_dev, L.fhe_bfv_encode_words_dev, L.fhe_transcode_dev
    assert eb(enc._h, 0, 0, p(src), cap, cap, nbits, p(out), 1, None) == 0
    assert eb(enc._h, 0, 0, p(src), cap + 1, cap + 1, nbits, p(out), 1, None) == TOO_MANY_VALUES
    assert eb(enc._h, 0, 0, p(src), 8, 8, 0, p(out), 1, None) == ARG
    assert eb(enc._h, 0, 0, p(src), 8, 8, 65, p(out), 1, None) == ARG
    assert eb(big._h, 0, 0, p(src), 8, 8, nbits, p(out), 1, None) == PARAMETER_MISMATCH
    assert eb(enc._h, 0, nl, p(src), 8, 8, nbits, p(out), 1, None) == INVALID_LEVEL
    assert eb(None, 0, 0, p(src), 8, 8, nbits, p(out), 1, None) == ARG
    assert eb(enc._h, 0, 0, None, 8, 1, nbits, p(out), 1, None) == ARG
    assert eb(enc._h, 0, 0, p(src), 8, 1, nbits, None, 1, None) == ARG
    assert eb(enc._h, 0, 0, None, 0, 1, nbits, p(out), 1, None) == 0          # an empty source: zero plaintexts
    assert eb(enc._h, 0, 0, None, 8, 1, nbits, None, 0, None) == 0            # an empty batch
    assert ew(enc._h, 0, 0, p(words), 36, 2, n, nbits, p(out), 1, None) == 0
    assert ew(enc._h, 0, 0, p(words), 0, 2, n, nbits, p(out), 1, None) == ARG
    assert ew(enc._h, 0, 0, p(words), 65, 2, n, nbits, p(out), 1, None) == ARG
    assert ew(enc._h, 0, 0, p(words), 36, 2, n, 0, p(out), 1, None) == ARG
    assert ew(enc._h, 0, 0, p(words), 36, 2, n, 65, p(out), 1, None) == ARG
    assert ew(big._h, 0, 0, p(words), 36, 2, n, nbits, p(out), 1, None) == PARAMETER_MISMATCH
    assert ew(enc._h, 0, nl, p(words), 36, 2, n, nbits, p(out), 1, None) == INVALID_LEVEL
    assert ew(None, 0, 0, p(words), 36, 2, n, nbits, p(out), 1, None) == ARG
    assert ew(enc._h, 0, 0, None, 36, 2, n, nbits, p(out), 1, None) == ARG
    assert ew(enc._h, 0, 0, p(words), 36, 2, n, nbits, None, 1, None) == ARG
    assert ew(enc._h, 0, 0, None, 36, 2, n, nbits, None, 0, None) == 0
    assert ew(enc._h, 0, 0, None, 36, 0, n, nbits, None, 1, None) == 0        # no segments: no plaintexts
    assert L.fhe_bfv_encode_words_count(enc._h, 36, 2, n, 20) == -(-2 * T.count(n, 36, 20) // n)
    assert L.fhe_bfv_encode_words_count(None, 36, 2, n, 20) == 0
    assert L.fhe_bfv_encode_words_count(enc._h, 65, 2, n, 20) == 0
    assert tr(p(words), 0, 36, n, p(out), 0, 20, 1, None) == 0
    assert tr(p(words), 0, 0, n, p(out), 0, 20, 1, None) == ARG
    assert tr(p(words), 0, 65, n, p(out), 0, 20, 1, None) == ARG
    assert tr(p(words), 0, 36, n, p(out), 0, 0, 1, None) == ARG
    assert tr(p(words), 0, 36, n, p(out), 1, 9, 1, None) == ARG               # a byte side carries at most 8 bits
    assert tr(p(words), 1, 9, n, p(out), 0, 20, 1, None) == ARG
    assert tr(None, 0, 36, n, p(out), 0, 20, 1, None) == ARG
    assert tr(p(words), 0, 36, n, None, 0, 20, 1, None) == ARG
    assert tr(None, 0, 36, n, None, 0, 20, 0, None) == 0
    assert L.fhe_transcode_count(0, n, 20) == 0 and L.fhe_transcode_count(36, n, 65) == 0
    # the Python layer
    with_err = []
    for call in (lambda: enc.encode_bytes(bytes(cap + 1), cap + 1), lambda: fhe.transcode(np.zeros(4, dtype=np.uint64), 65, 8),
                 lambda: fhe.transcode(np.zeros(4, dtype=np.uint64), 20, 9, out_bytes=True)):
        try:
            call()
        except fhe.FheError as e:
            with_err.append(e.code)
    assert with_err == [TOO_MANY_VALUES, ARG, ARG]


# ---- one SealPIR round -------------------------------------------------------------------------------------------------
def case_sealpir_round(fhe, dev, n, t=2056193, sizes=(36, 36, 37), dim=2, element_size=7, index=None, seed=9):
    """crates/fhe/examples/sealpir.rs with directly encrypted selection ciphertexts (no expansion): the database through
    encode_bytes, the first dot product and the switch to the last level, the fold through encode_words, the second dot
    product and switch; the client decrypts, transcodes back to ciphertext words, decrypts, transcodes to bytes -- the
    chosen element."""
    x = Xfer(dev)
    rng = random.Random(seed)
    par = fhe.BfvParameters(n, t, moduli_sizes=list(sizes))
    enc = par.encoder()
    nbits = ilog2(t)
    qbits = int(par.moduli[0]).bit_length()
    per = fhe.number_elements_per_plaintext(n, nbits, element_size)
    item_bytes = per * element_size
    nelem = dim * dim * per - per // 2                       # (the last plaintext is short)
    db = rng.randbytes(nelem * element_size)
    index = rng.randrange(nelem) if index is None else index
    pts = enc.encode_bytes(x.to_bytes(np.frombuffer(db, dtype=np.uint8)), item_bytes, level=1, batch=dim * dim)
    pts = host(fhe, pts)
    assert pts.shape == (dim * dim, 2, n)
    sk = fhe.SecretKey.random(par, bytes(range(32)))
    row = index // per
    sel = np.zeros((2 * dim, 1), dtype=np.uint64)
    sel[row // dim, 0] = sel[dim + row % dim, 0] = 1
    query = host(fhe, sk.encrypt(enc.encode(x.to(sel), "poly", 1, scaled=True), level=1))
    assert query.shape == (2 * dim, 2, 2, n)
    ctx1 = par.context_at_level(1)
    cols = np.ascontiguousarray(pts.reshape(dim, dim, 2, n).transpose(1, 0, 2, 3))     # column c: rows c, c + dim, ...
    d = ctx1.ciphertext_switch_to_level(ctx1.dot_product_scalar(x.to(query[:dim]), x.to(cols)), 1)
    words = host(fhe, d).reshape(dim, 2, n)
    assert int(words.max()).bit_length() <= qbits
    fold = host(fhe, enc.encode_words(x.to(words), qbits, level=1))
    m = T.count(n, qbits, nbits)
    nplain = -(-2 * m // n)
    assert fold.shape == (dim, nplain, 2, n)
    fp = np.ascontiguousarray(fold.transpose(1, 0, 2, 3))
    o = ctx1.ciphertext_switch_to_level(ctx1.dot_product_scalar(x.to(query[dim:]), x.to(fp)), 1)
    # the client
    dec = host(fhe, sk.decrypt(o, level=2)).reshape(-1)
    assert dec.size >= 2 * m
    halves = np.stack([dec[:m], dec[m:2 * m]])
    back = host(fhe, fhe.transcode(x.to(halves), nbits, qbits))
    assert back.shape[1] >= n
    ct = np.ascontiguousarray(back[:, :n]).reshape(2, 1, n)
    assert np.array_equal(ct, words[row % dim].reshape(2, 1, n))
    pt = host(fhe, sk.decrypt(x.to(ct), level=2))
    plain = host(fhe, fhe.transcode(x.to(pt), nbits, 8, out_bytes=True)).tobytes()
    off = index % per
    assert plain[off * element_size:(off + 1) * element_size] == db[index * element_size:(index + 1) * element_size]
    return nplain
