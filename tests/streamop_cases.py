"""Cases of the streaming kernels (fhe.rs_amd/csrc/kernels_misc.hpp: dot_kernel<1|2>, mul_plain_kernel, switch_down_kernel,
substitute_kernel, wire_pack_kernel / wire_unpack_kernel and their word forms) at the edges random words at one small
shape never reach, and of stage B of the key switch with seventeen digits at the top.  Shared by
tests/test_streamop_emu.py (kernel sources under host emulation) and tests/test_streamop_gpu.py (the HIP build).
`dev`: as helpers.Xfer -- False hands numpy arrays over, True torch tensors, "abi" DeviceArrays.

Every comparison is word for word with the restatements of tests/streamop_ref.py (Python ints); one case per operation
also compares the restatement with oracle/fhe_oracle.  Inputs and expected words are built once per process and shared
(functools.lru_cache); nothing writes into them.

What the shapes are for:
* dot product -- the accumulator's third limb: with every word at q - 1 the exact sum reaches 2^128 at
  c* = ceil(2^128 / (q - 1)^2) terms (computed and asserted per modulus); counts c* - 1, c*, c* + 1 and 4096 at the top, 1 ... 4096
  random, maxima in one of a lane's two coefficients only and in the last part only, part counts 1 ... 5 (1: dot_kernel<1>;
  3 and 5: a dead second part in the last grid row), the three private / shared stride pairs at batch 3;
* modulus switching -- the rounding: last-row words on both sides of h = q_L >> 1 and at both ends of [0, q_L), against
  other-row words at both ends and in the middle of [0, q_i), over moduli sets whose dropped modulus is wider than, as wide
  as and narrower than those that stay, from every level of the chain, one level and every reachable number of levels;
* substitution -- every odd exponent at N = 8 and 16, zeros and q - 1 where the exponent negates;
* wire format -- every class of coefficient width (below, at and above 32 bits; 62), rows of 8, 128 and 2048
  coefficients, buffers on and off a 16-byte boundary."""
import collections
import functools
import zlib

import numpy as np

import hoist_cases as H
import keyed_cases as K
import streamop_ref as R
from cases import MODULI5
from fhe_oracle import bfv as obfv
from fhe_oracle import coracle
from fhe_oracle.rq import NTT, POWER_BASIS, Context as OCtx, Poly, SubstitutionExponent, poly_from_wire, poly_to_wire
from fhe_oracle.zq import generate_prime
from helpers import Xfer, arr
from keyed_cases import same

TWO128 = 1 << 128


@functools.lru_cache(maxsize=None)
def moduli(sizes, n):
    return tuple(obfv.generate_moduli(list(sizes), n))


@functools.lru_cache(maxsize=None)
def c_context(q, n):
    """The C oracle's context (its transforms: the Python oracle's words, tests/test_oracle_c.py)."""
    return coracle.CCtx(OCtx(list(q), n))


def top_row(q):
    return np.array(q, dtype=np.uint64)[:, None] - np.uint64(1)


def alternating(q, n):
    """q - 1 in the even coefficients, 0 in the odd ones."""
    return np.where(np.arange(n)[None, :] % 2 == 0, top_row(q), np.uint64(0)).astype(np.uint64)


# ---- dot product ---------------------------------------------------------------------------------------------------------
DOT_CONTEXTS = collections.OrderedDict([
    ("n8-62-61-60", (8, (62, 61, 60))),        # pl / 2 = 12 lanes of a 256-lane block
    ("n256-62-61-60", (256, (62, 61, 60))),    # two blocks, the second part-filled; a row boundary inside a block
    ("n8-62-62", (8, (62, 62))),
    ("n8-50-40-20", (8, (50, 40, 20))),        # the third limb stays 0: the other branch of the fold
])
DOT_GROUPS = ("thresholds", "random", "mixed", "parts", "strides")
# pattern: "max" (every word at q - 1), "random", "even" (q - 1 in even coefficients, 0 in odd ones: a lane's two
# accumulators are independent), "last" (plaintexts at q - 1; the last part at q - 1, the parts before it random).
# form: None (no batch), or at batch 3 "cts" (cts shared, pts private), "pts" (pts shared), "both" (both private).
# top: whether some exact sum must reach 2^128 (None: not asserted).
Dot = collections.namedtuple("Dot", "ctx pattern count parts form top oracle")
BATCH = 3


def dot_thresholds(name):
    n, sizes = DOT_CONTEXTS[name]
    return [R.dot_threshold(m) for m in moduli(sizes, n)]


def dot_cases(name, group):
    n, sizes = DOT_CONTEXTS[name]
    th = dot_thresholds(name)
    reach = sorted({c for c in th if c <= 4096})
    wide = min(th) <= 75          # a 62- or 61-bit modulus: 300 random terms (about 75 (q - 1)^2) pass 2^128
    big = n > 8                   # the exact reference costs count * parts * L * N Python products: fewer parts there
    mk = lambda pattern, count, parts, form=None, top=None, oracle=False: Dot(name, pattern, count, parts, form, top, oracle)  # noqa: E731
    if group == "thresholds":
        counts = sorted({k for c in reach for k in (c - 1, c, c + 1)}) or [17]
        out = [mk("max", k, 2, top=k >= min(th), oracle=(k == min(th))) for k in counts]
        return out + [mk("max", 4096, 1 if big else 2, top=4096 >= min(th))]
    if group == "random":
        return ([mk("random", k, 2, oracle=(k == 7)) for k in (1, 2, 7)]
                + [mk("random", 300, 2, top=True if wide else None), mk("random", 4096, 1 if big else 2, top=True if wide else None)])
    if group == "mixed":
        return [mk("even", 300, 3, top=300 >= min(th)), mk("last", 300, 3, top=300 >= min(th))]
    if group == "parts":
        return [mk("last", 300, p, top=300 >= min(th)) for p in ((1, 3) if big else (1, 2, 3, 4, 5))]
    assert group == "strides"
    return [mk("random", 300, 3, form, top=True if wide else None) for form in (("both",) if big else ("cts", "pts", "both"))]


def dot_all_cases(name):
    return [c for g in DOT_GROUPS for c in dot_cases(name, g)]


@functools.lru_cache(maxsize=None)
def dot_data(case):
    """(cts, pts, want): the inputs with their leading batch dimensions, the restatement's words [batch..., parts, L, N]."""
    n, sizes = DOT_CONTEXTS[case.ctx]
    q = moduli(sizes, n)
    L = len(q)
    rng = np.random.default_rng(zlib.crc32(repr(case).encode()))
    top = top_row(q)

    def make(lead_c, lead_p):
        cs, ps = lead_c + (case.count, case.parts, L, n), lead_p + (case.count, L, n)
        if case.pattern == "max":
            return np.broadcast_to(top, cs).copy(), np.broadcast_to(top, ps).copy()
        if case.pattern == "even":
            return np.broadcast_to(alternating(q, n), cs).copy(), np.broadcast_to(alternating(q, n), ps).copy()
        cts = K.uniform(rng, q, n, cs[:-2])
        if case.pattern == "last":
            cts[..., -1, :, :] = top
            return cts, np.broadcast_to(top, ps).copy()
        return cts, K.uniform(rng, q, n, ps[:-2])

    if case.form is None:
        cts, pts = make((), ())
        want, peak = R.dot_product(cts, pts, q)
    else:
        cts, pts = make(() if case.form == "cts" else (BATCH,), () if case.form == "pts" else (BATCH,))
        per = [R.dot_product(cts if case.form == "cts" else cts[b], pts if case.form == "pts" else pts[b], q) for b in range(BATCH)]
        want, peak = np.stack([w for w, _ in per]), max(p for _, p in per)
        assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])   # (a wrong stride shows)
    if case.top is not None:
        assert (peak >= TWO128) == case.top, (case, peak.bit_length())
    if case.oracle:     # the restatement against rq::dot_product of the Python oracle
        octx = OCtx(list(q), n)
        for p in range(case.parts):
            o = obfv.poly_dot_product([Poly(octx, NTT, c[p].tolist()) for c in cts], [Poly(octx, NTT, v.tolist()) for v in pts])
            same(want[p], arr(o), ("restatement against the oracle", case))
    for a in (cts, pts, want):
        a.setflags(write=False)
    return cts, pts, want


def case_dot_thresholds_are_what_they_are(name):
    """c* per modulus, in Python ints: (c* - 1) (q - 1)^2 < 2^128 <= c* (q - 1)^2 (asserted by dot_threshold), the least
    over the set -- the first count at which any word's third limb is non-zero -- and whether 4096 terms get there."""
    n, sizes = DOT_CONTEXTS[name]
    q = moduli(sizes, n)
    th = dot_thresholds(name)
    for m, c in zip(q, th):
        assert (c - 1) * (m - 1) ** 2 < TWO128 <= c * (m - 1) ** 2
    return dict(zip(sizes, th))


def run_dot(fhe, dev, case):
    x = Xfer(dev)
    n, sizes = DOT_CONTEXTS[case.ctx]
    cts, pts, want = dot_data(case)
    ctx = fhe.Context(list(moduli(sizes, n)), n)
    got = x.back(ctx.dot_product_scalar(x.to(cts.copy()), x.to(pts.copy())))   # (the shared inputs are read-only)
    same(got, want, case)


# ---- ct x pt -------------------------------------------------------------------------------------------------------------
MUL_PLAIN_N = (8, 256)


@functools.lru_cache(maxsize=None)
def mul_plain_data(n):
    """[(parts, shared, pattern, ct, pt, want)] over [62, 61, 60] at batch 3."""
    q = moduli((62, 61, 60), n)
    rng = np.random.default_rng(4100 + n)
    out = []
    for parts in (1, 2, 3):
        for shared in (True, False):
            for pattern in ("random", "max"):
                lead = () if shared else (BATCH,)
                if pattern == "max":
                    ct = np.broadcast_to(top_row(q), (BATCH, parts, len(q), n)).copy()
                    pt = np.broadcast_to(top_row(q), lead + (len(q), n)).copy()
                else:
                    ct, pt = K.uniform(rng, q, n, (BATCH, parts)), K.uniform(rng, q, n, lead)
                want = np.stack([R.mul_plain(ct[b], pt if shared else pt[b], q) for b in range(BATCH)])
                out.append((parts, shared, pattern, ct, pt, want))
    # the restatement against the oracle's Poly.mul
    parts, shared, pattern, ct, pt, want = out[-2]
    assert (parts, shared, pattern) == (3, False, "random")
    octx = OCtx(list(q), n)
    for p in range(parts):
        same(want[1][p], arr(Poly(octx, NTT, ct[1][p].tolist()).mul(Poly(octx, NTT, pt[1].tolist()))), "mul_plain restatement")
    return out


def case_mul_plain(fhe, dev, n):
    x = Xfer(dev)
    ctx = fhe.Context(list(moduli((62, 61, 60), n)), n)
    for parts, shared, pattern, ct, pt, want in mul_plain_data(n):
        same(x.back(ctx.mul_plain(x.to(ct), x.to(pt))), want, ("mul_plain", n, parts, shared, pattern))


# ---- modulus switching ---------------------------------------------------------------------------------------------------
SD_N = 64
SD_SETS = collections.OrderedDict([
    ("62-62-20", (62, 62, 20)),      # drops a modulus narrower than those that stay, then one as wide
    ("20-40-62", (20, 40, 62)),      # drops the widest: the sum x_L + h is reduced for good under every q_i
    ("62-61-60", (62, 61, 60)),
    ("50-62", (50, 62)),
    ("moduli5", None),               # tests/cases.py's MODULI5: 1153 and four 62-bit primes
])


def sd_moduli(name):
    return tuple(MODULI5) if SD_SETS[name] is None else moduli(SD_SETS[name], SD_N)


def sd_planted(q, rng, npolys):
    """[npolys, L, N] PowerBasis words over q (L >= 2): per polynomial, in columns of its own choosing, the product of
    the last row in {0, 1, h - 1, h, h + 1, h + 2, q_L - 2, q_L - 1} with every other row at {0, 1, q_i - 1, q_i >> 1};
    the remaining columns random."""
    q = list(q)
    ql, h = q[-1], q[-1] >> 1
    lasts = [0, 1, h - 1, h, h + 1, h + 2, ql - 2, ql - 1]
    assert all(0 <= v < ql for v in lasts) and len(set(lasts)) == 8
    others = [lambda m: 0, lambda m: 1, lambda m: m - 1, lambda m: m >> 1]
    assert len(lasts) * len(others) <= SD_N
    out = K.uniform(rng, q, SD_N, (npolys,))
    for b in range(npolys):
        cols = rng.permutation(SD_N)[:len(lasts) * len(others)]
        for k, col in enumerate(cols):
            out[b, -1, col] = lasts[k % 8]
            for r, m in enumerate(q[:-1]):
                out[b, r, col] = others[k // 8](m)
    return out


@functools.lru_cache(maxsize=None)
def sd_data(name):
    """Per start level k (at least two moduli left): planted polynomials [3, L - k, N] and the restatement's words after
    1 ... L - k - 1 levels; and for the ciphertext forms from level 0: planted [3, 2, L, N] in PowerBasis, the same in Ntt
    form, and the Ntt words after 0 ... L - 1 levels."""
    q = sd_moduli(name)
    rng = np.random.default_rng(5200 + len(name) + sum(SD_SETS[name] or (5,)))
    polys = {}
    for k in range(len(q) - 1):
        qk = q[:len(q) - k]
        x = sd_planted(qk, rng, BATCH)
        polys[k] = (x, [R.switch_down_levels(x, qk, lv) for lv in range(len(qk))])
    x, wants = polys[0]
    octx = OCtx(list(q), SD_N)
    if name == "62-62-20":   # the restatement against Poly::switch_down of the Python oracle, planted columns included
        for b in range(BATCH):
            same(wants[1][b], arr(Poly(octx, POWER_BASIS, x[b].tolist()).switch_down()), "switch_down restatement")
            same(wants[len(q) - 1][b], arr(Poly(octx, POWER_BASIS, x[b].tolist()).switch_down_to(octx.context_at_level(len(q) - 1))),
                 "switch_down_to restatement")
    pb = sd_planted(q, rng, BATCH * 2).reshape(BATCH, 2, len(q), SD_N)
    fwd = lambda a, lv: np.stack([c_context(q[:len(q) - lv], SD_N).poly_ntt_forward(p) for p in a.reshape((-1,) + a.shape[-2:])]  # noqa: E731
                                 ).reshape(a.shape)
    ct = fwd(pb, 0)
    ct_wants = [fwd(R.switch_down_levels(pb, q, lv), lv) for lv in range(len(q))]
    return polys, ct, ct_wants


def case_switch_down(fhe, dev, name):
    """switch_down and switch_down_to from every level of the chain; ciphertext_switch_down and
    ciphertext_switch_to_level from level 0; every reachable number of levels in one call each."""
    x = Xfer(dev)
    q = sd_moduli(name)
    polys, ct, ct_wants = sd_data(name)
    c = fhe.Context(list(q), SD_N)
    for k, (inp, wants) in polys.items():
        frm = c.at_level(k)
        same(x.back(frm.switch_down(x.to(inp))), wants[1], ("switch_down", name, k))
        same(x.back(frm.switch_down(x.to(inp[0]))), wants[1][0], ("switch_down, one polynomial", name, k))
        for lv in range(len(wants)):
            same(x.back(frm.switch_down_to(x.to(inp), c.at_level(k + lv))), wants[lv], ("switch_down_to", name, k, lv))
    same(x.back(c.ciphertext_switch_down(x.to(ct))), ct_wants[1], ("ciphertext_switch_down", name))
    for lv in range(len(q)):
        same(x.back(c.ciphertext_switch_to_level(x.to(ct), lv)), ct_wants[lv], ("ciphertext_switch_to_level", name, lv))


# ---- substitution --------------------------------------------------------------------------------------------------------
SUB_N = (8, 16, 1024)
SUB_SIZES = (62, 40, 20)


def sub_exponents(n):
    return list(range(1, 2 * n, 2)) + [2 * n + 5] if n <= 16 else [1, 3, n - 1, n + 1, 2 * n - 1]


@functools.lru_cache(maxsize=None)
def sub_data(n):
    """[(e, x PowerBasis [2, L, N], want PowerBasis, x Ntt, want Ntt)]: random rows with 0 and q - 1 at indices the
    exponent negates (asserted to exist unless e = 1 mod 2N, which negates nothing) and at one it does not."""
    q = moduli(SUB_SIZES, n)
    cc = c_context(q, n)
    octx = OCtx(list(q), n)
    rng = np.random.default_rng(6300 + n)
    fwd = lambda a: np.stack([cc.poly_ntt_forward(p) for p in a])   # noqa: E731
    out = []
    for e in sub_exponents(n):
        x = K.uniform(rng, q, n, (2,))
        neg = R.negated_indices(n, e)
        kept = [j for j in range(n) if j not in set(neg)]
        if e % (2 * n) == 1:
            assert not neg
        else:
            assert len(neg) >= 2 and kept, (n, e)
            x[0, :, neg[0]], x[1, :, neg[0]] = 0, top_row(q)[:, 0]
            x[0, :, neg[-1]], x[1, :, neg[-1]] = top_row(q)[:, 0], 0
        x[0, :, kept[-1]], x[1, :, kept[-1]] = 0, top_row(q)[:, 0]
        want = R.substitute(x, q, e)
        for j in neg[:1] + neg[-1:]:    # a negated zero stays zero, a negated q - 1 becomes 1
            for b in range(2):
                for r in range(len(q)):
                    assert int(want[b, r, (j * e) % n]) == (0 if x[b, r, j] == 0 else 1)
        if n == 16:    # the restatement against Poly::substitute of the Python oracle
            for b in range(2):
                same(want[b], arr(Poly(octx, POWER_BASIS, x[b].tolist()).substitute(SubstitutionExponent(octx, e))),
                     ("substitute restatement", e))
        out.append((e, x, want, fwd(x), fwd(want)))
    return out


def case_substitute(fhe, dev, n):
    x = Xfer(dev)
    c = fhe.Context(list(moduli(SUB_SIZES, n)), n)
    for e, pb, want_pb, ntt, want_ntt in sub_data(n):
        same(x.back(c.substitute(e, x.to(pb), ntt=False)), want_pb, ("substitute PowerBasis", n, e))
        same(x.back(c.substitute(e, x.to(ntt), ntt=True)), want_ntt, ("substitute Ntt", n, e))
    pb = sub_data(n)[0][1]
    for bad in (0, 2, 2 * n, 2 * n + 4):
        for form in (False, True):
            try:
                c.substitute(bad, x.to(pb), ntt=form)
                raise AssertionError("even exponent accepted")
            except fhe.FheError as err:
                assert err.code == -10


# ---- wire format ---------------------------------------------------------------------------------------------------------
WIRE_WIDTHS = (20, 31, 32, 33, 47, 58, 62)
WIRE_MIXED = (62, 33, 20, 47, 31)      # five unequal widths: every row starts where the ones before it end
WIRE_CONTEXTS = [(w,) for w in WIRE_WIDTHS] + [WIRE_MIXED]
WIRE_N = (8, 128, 2048)                # byte kernels on 64 lanes | the smallest row of the word kernels | 256 lanes
WIRE_OFFSETS = (0, 8, 1)               # of the byte buffer from a 16-byte boundary


@functools.lru_cache(maxsize=None)
def wire_moduli(widths, n):
    q = tuple(generate_prime(w, 2 * n, 1 << w) for w in widths)
    assert all(R.wire_bits(m) == w for m, w in zip(q, widths)), (q, widths)
    return q


@functools.lru_cache(maxsize=None)
def wire_data(widths, n):
    """(polys PowerBasis [4, L, N]: rows of 0, of q - 1, alternating, random; the same in Ntt form; the restatement's bytes
    uint8 [4, size])."""
    q = wire_moduli(widths, n)
    rng = np.random.default_rng(7400 + n + sum(widths))
    L = len(q)
    pb = np.stack([np.zeros((L, n), dtype=np.uint64), np.broadcast_to(top_row(q), (L, n)).copy(), alternating(q, n),
                   K.uniform(rng, q, n)])
    data = np.stack([np.frombuffer(R.wire_pack(p, q), dtype=np.uint8) for p in pb])
    assert data.shape == (4, R.wire_size(q, n))
    for p, d in zip(pb, data):
        assert np.array_equal(R.wire_unpack(d, q, n), p)
    if n <= 128:   # the restatement against the Python oracle's shift registers
        octx = OCtx(list(q), n)
        assert poly_to_wire(Poly(octx, POWER_BASIS, pb[3].tolist())) == data[3].tobytes()
        junk = rng.integers(0, 256, size=data.shape[1], dtype=np.uint8)
        same(R.wire_unpack(junk, q, n), arr(poly_from_wire(octx, junk.tobytes())), "wire_unpack restatement")
    cc = c_context(q, n)
    ntt = np.stack([cc.poly_ntt_forward(p) for p in pb])
    return pb, ntt, data


def byte_view(fhe, x, data, off):
    """`data` (uint8, any shape) on the device, starting `off` bytes past a 16-byte boundary: (the allocation, the view)."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    whole = np.zeros(data.size + 16, dtype=np.uint8)
    whole[off:off + data.size] = data.reshape(-1)
    base = x.to_bytes(whole)
    assert base.data_ptr() % 16 == 0
    if x.dev == "abi":
        view = fhe.DeviceArray(data.shape, base.device, 1, _ptr=base.data_ptr() + off, _base=base)
    else:
        view = base[off:off + data.size].view(data.shape)
    assert view.data_ptr() % 16 == off % 16 and view.is_contiguous()
    return base, view


def wire_word_kernels(n, off):
    """launch_wire's rule (engine.hpp): the word kernels for rows of 128 coefficients and more between 16-byte aligned
    buffers, the byte kernels otherwise."""
    return n >= 128 and off % 16 == 0


def case_wire(fhe, dev, widths, n, offsets=WIRE_OFFSETS):
    """Engine bytes == the restatement's from PowerBasis and from Ntt sources, unpack inverts pack (to PowerBasis and to
    Ntt), and a buffer off the 16-byte boundary (device forms) holds the same bytes as an aligned one."""
    from fhe_rs_amd import api
    x = Xfer(dev)
    q = wire_moduli(widths, n)
    pb, ntt, data = wire_data(widths, n)
    c = fhe.Context(list(q), n)
    assert c.serialized_size == data.shape[1] == R.wire_size(q, n)
    # the wrappers (buffers of the allocator: aligned)
    same(x.back_bytes(c.serialize(x.to(pb))), data, ("serialize", widths, n))
    same(x.back_bytes(c.serialize(x.to(ntt), from_ntt=True)), data, ("serialize from Ntt", widths, n))
    same(x.back(c.deserialize(x.to_bytes(data))), pb, ("deserialize", widths, n))
    same(x.back(c.deserialize(x.to_bytes(data), to_ntt=True)), ntt, ("deserialize to Ntt", widths, n))
    if not dev:
        return
    results = {}
    for off in offsets:
        for src, from_ntt in ((pb, 0), (ntt, 1)):
            base, view = byte_view(fhe, x, np.full(data.shape, 0xA5, dtype=np.uint8), off)
            polys = x.to(src)     # (held until the bytes are back: the call is asynchronous)
            st, msg = K.raw(fhe, "fhe_poly_serialize_dev", c._h, api._dptr(polys), api._dptr8(view), len(src), from_ntt,
                            api._stream())
            assert st == 0, (st, msg)
            whole = x.back_bytes(base)
            got = whole[off:off + data.size].reshape(data.shape)
            same(got, data, ("serialize", widths, n, "offset", off, "from Ntt", from_ntt))
            assert (whole[:off] == 0).all() and (whole[off + data.size:] == 0).all(), "bytes outside the buffer written"
            results[off, from_ntt] = got
        for want, to_ntt in ((pb, 0), (ntt, 1)):
            base, view = byte_view(fhe, x, data, off)
            out = x.to(np.zeros_like(pb))
            st, msg = K.raw(fhe, "fhe_poly_deserialize_dev", c._h, api._dptr8(view), api._dptr(out), len(pb), to_ntt, api._stream())
            assert st == 0, (st, msg)
            same(x.back(out), want, ("deserialize", widths, n, "offset", off, "to Ntt", to_ntt))
    for key, got in results.items():
        same(got, results[offsets[0], 0], ("aligned and unaligned buffers differ", key))


def case_wire_guarded(fhe, widths, n):
    """HOST EMULATION ONLY (its device pointers are host pointers): the byte buffer ends on the last byte before a page
    without access rights, so a kernel that reads or writes one byte past the payload ends the process.  What no value
    can show: a coefficient that ends exactly on a 64-bit word -- the last one of every row does -- must not make
    wire_unpack_coeff load the word after it, whose bits the mask would drop anyway.  Run in a process of its own
    (tests/test_streamop_emu.py)."""
    import ctypes as C
    import mmap
    x = Xfer("abi")
    q = wire_moduli(widths, n)
    pb, _ntt, data = wire_data(widths, n)
    c = fhe.Context(list(q), n)
    libc = C.CDLL(None, use_errno=True)
    libc.mmap.restype = C.c_void_p
    libc.mmap.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_long]
    libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    page = mmap.PAGESIZE
    pages = -(-data.size // page)
    addr = libc.mmap(None, (pages + 1) * page, mmap.PROT_READ | mmap.PROT_WRITE, mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS, -1, 0)
    assert addr not in (None, C.c_void_p(-1).value), C.get_errno()
    assert libc.mprotect(addr + pages * page, page, 0) == 0, C.get_errno()     # PROT_NONE
    start = addr + pages * page - data.size
    assert wire_word_kernels(n, start % 16) == (n >= 128)     # (a whole number of 16-byte words per row from N = 128 on)
    C.memmove(start, data.ctypes.data, data.size)
    out = x.to(np.zeros_like(pb))
    st, msg = K.raw(fhe, "fhe_poly_deserialize_dev", c._h, C.c_void_p(start), C.c_void_p(out.data_ptr()), len(pb), 0, None)
    assert st == 0, (st, msg)
    same(x.back(out), pb, ("deserialize before a guard page", widths, n))
    C.memset(start, 0, data.size)
    src = x.to(pb)
    st, msg = K.raw(fhe, "fhe_poly_serialize_dev", c._h, C.c_void_p(src.data_ptr()), C.c_void_p(start), len(pb), 0, None)
    assert st == 0, (st, msg)
    x.back(src)     # (waits for the call)
    assert C.string_at(start, data.size) == data.tobytes(), ("serialize before a guard page", widths, n)


def main_wire_guarded():
    from helpers import load_engine
    fhe = load_engine("emu")
    for widths in ((33,), (62,), WIRE_MIXED):
        for n in WIRE_N:
            case_wire_guarded(fhe, widths, n)
    print("guarded wire buffers ok")


# ---- seventeen digits at the top -----------------------------------------------------------------------------------------
TOP17_N = 128


def top17_moduli():
    return moduli((62,) * 17, TOP17_N)


@functools.lru_cache(maxsize=None)
def top17_saturation():
    """In Python ints, before anything runs: with every ciphertext word and every key word at q - 1, in the row of the
    largest key modulus the sixteen first products of stage B plus one canonical word stay below 2^128 and all seventeen
    reach it -- in every column.  (c2 = -1 in every Ntt slot is the constant polynomial -1: digit i is the constant
    q_i - 1, whose transform under q_j >= q_i is q_i - 1 in every slot; the own row i = j is read from c2 itself.)
    Returns (c2 in PowerBasis [L, N], the least of the seventeen digit words)."""
    q = top17_moduli()
    n, L = TOP17_N, len(q)
    cc = c_context(q, n)
    c2 = np.broadcast_to(top_row(q), (L, n)).copy()
    p = cc.poly_ntt_backward(c2)
    jmax = max(range(L), key=lambda j: q[j])
    w = []
    for i in range(L):
        if i == jmax:
            w.append([int(v) for v in c2[jmax]])
        else:
            digit = np.array([[int(v) % m for v in p[i]] for m in q], dtype=np.uint64)
            w.append([int(v) for v in cc.poly_ntt_forward(digit)[jmax]])
    key = q[jmax] - 1
    for col in range(n):
        prods = [w[i][col] * key for i in range(L)]
        assert sum(prods[:16]) + q[jmax] - 1 < TWO128 <= sum(prods), ("the window is not saturated", col)
    least = min(min(row) for row in w)
    assert least > 1 << 61
    return p, least


_top17_wants = []


def top17_plain_wants(sy):
    """The oracle's words for one all-top ciphertext of three parts and for the key switch of its c2 (PowerBasis); the
    same for every all-top key, so computed once."""
    if not _top17_wants:
        _top17_wants.append(top17_plain_wants_of(sy))
    return _top17_wants[0]


def top17_plain_wants_of(sy):
    q, n = top17_moduli(), TOP17_N
    p, _ = top17_saturation()
    ok = sy.oracle_key(0)
    ct3 = np.broadcast_to(top_row(q), (1, 3, len(q), n)).copy()
    c = obfv.Ciphertext(sy.opar, [Poly(sy.octx, NTT, r.tolist()) for r in ct3[0]], 0)
    obfv.RelinearizationKey(ksk=ok).relinearizes(c)
    w0, w1 = ok.key_switch(Poly(sy.octx, POWER_BASIS, p.tolist()))
    return ct3, K.ct_arr(c)[None], p[None].copy(), arr(w0)[None], arr(w1)[None]


def case_top17_keyed(fhe, dev, seed=171):
    """The keyed call (and, inside keyed_cases.case_synthetic, the single-key call in its default mode and the oracle)."""
    top17_saturation()
    return K.case_synthetic(fhe, dev, list(top17_moduli()), TOP17_N, 2, 1, seed=seed, top=True)


def case_top17_plain(fhe, dev, mode, seed=173):
    """The plain key switch under `mode` (KeySwitchingKey.UNFUSED: ks_mac_kernel; FUSED): relinearizes of the all-top
    ciphertext and key_switch of its c2, against the oracle."""
    top17_saturation()
    x = Xfer(dev)
    sy = K.Synthetic(fhe, list(top17_moduli()), TOP17_N, 1, seed, top=True)
    ct3, want_ct, p, w0, w1 = top17_plain_wants(sy)
    key = sy.keys[0].set_mode(mode)
    assert key.mode()["mode"] == mode
    same(x.back(fhe.RelinearizationKey(key).relinearizes(x.to(ct3))), want_ct, ("relinearizes", mode))
    g0, g1 = key.key_switch(x.to(p))
    same(x.back(g0), w0, ("key_switch c0", mode))
    same(x.back(g1), w1, ("key_switch c1", mode))


def case_top17_hoisted(fhe, dev, seed=179):
    """relinearize_hoisted at exponents (3, 255) against tests/hoist_ref.py."""
    top17_saturation()
    return H.case_synthetic(fhe, dev, list(top17_moduli()), TOP17_N, 2, 1, seed=seed, top=True, exps=(3, 255))
