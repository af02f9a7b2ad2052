"""The columns of tests/scaler_edge_inputs.py through the engine's scaler, every output word against the oracle's
RnsScaler::scale (rns/scaler.rs:249-352).  Shared by tests/test_scaler_edges_emu.py (kernel sources under host emulation)
and tests/test_scaler_edges_gpu.py (the HIP build on the MI355X)."""
import random

import numpy as np

import scaler_edge_inputs as I
from fhe_oracle import bfv as obfv
from fhe_oracle.rq import Poly, POWER_BASIS
from helpers import arr, ct_arr, Xfer

WORKGROUP = 256
N256 = ("one_5x62", "w37_6x62", "bfv8192_down")          # these run on rows of 256 columns, the others on 16


def degree_of(sc):
    return 256 if sc.name in N256 else 16


def pack(sc):
    """-> (polys [npolys][nfrom][N] uint64, columns in launch order).  Threshold columns sit at index 0 and N - 1 of a
    row and either side of the workgroup boundaries 256 | 257 from both ends (the kernel hands columns out from the last
    polynomial backwards); rows of 16 columns never fill the last workgroup."""
    n = degree_of(sc)
    cl = I.classes(sc)
    thr = [c for k in I.THRESHOLD_CLASSES for c in cl.get(k, [])]
    flat = thr + [c for k, cols in cl.items() if k not in I.THRESHOLD_CLASSES for c in cols]
    assert len(thr) >= 16
    i = 0
    while len(flat) % n or len(flat) <= 2 * WORKGROUP or (n < WORKGROUP and len(flat) % WORKGROUP == 0):
        flat.append(thr[i % len(thr)])
        i += 1
    total = len(flat)
    special = sorted({n - 1, WORKGROUP - 1, WORKGROUP, total - WORKGROUP - 1, total - WORKGROUP, total - 1})
    for k, pos in enumerate(special):
        if pos >= len(thr):
            flat[pos], flat[1 + k] = flat[1 + k], flat[pos]
    npolys = total // n
    polys = np.array(flat, dtype=np.uint64).reshape(npolys, n, len(sc.frm)).transpose(0, 2, 1)
    return np.ascontiguousarray(polys), flat


_expected = {}


def expected(sc):
    """(polys, want [npolys][nto][N]) by the oracle, computed once per scaler and never modified."""
    if sc.name not in _expected:
        polys, flat = pack(sc)
        n, ncm, nto = degree_of(sc), sc.ncommon, len(sc.to)
        out = [c[:ncm] + sc.rns.scale(c, nto - ncm, ncm) for c in flat]
        want = np.array(out, dtype=np.uint64).reshape(len(flat) // n, n, nto).transpose(0, 2, 1)
        want = np.ascontiguousarray(want)
        polys.setflags(write=False)
        want.setflags(write=False)
        _expected[sc.name] = (polys, want)
    return _expected[sc.name]


def case_scaler(fhe, dev, sc):
    x = Xfer(dev)
    n = degree_of(sc)
    polys, want = expected(sc)
    s = fhe.Scaler(fhe.Context(sc.frm, n), fhe.Context(sc.to, n), sc.num, sc.den)
    assert s.number_common_moduli == sc.ncommon
    got = x.back(s.scale(x.to(polys.copy()), ntt=False))
    if not np.array_equal(got, want):
        p, r, c = (int(v[0]) for v in np.nonzero(got != want))
        raise AssertionError("%s %s: polynomial %d target %d column %d (flat %d): got %d, want %d, residues %s" % (
            sc.name, I.instance_of(sc), p, r, c, p * n + c, got[p, r, c], want[p, r, c], polys[p, :, c].tolist()))


def case_decrypt_on_threshold(fhe, dev, n=4096):
    """A ciphertext of the stock n = 4096 set whose phase puts the decryption scaler's w on its threshold (window and
    lattice-free tie columns of `bfv4096_decrypt`, threshold columns of v, range columns) on every coefficient:
    c0 = phase - c1 s for a random c1; the engine's decrypt against the oracle's SecretKey::decrypt."""
    x = Xfer(dev)
    if n not in _decrypt:
        _decrypt[n] = _decrypt_on_threshold(n)
    opar, sk, ct, want = _decrypt[n]
    par = fhe.BfvParameters(n, opar.plaintext, moduli=opar.moduli)
    s_ntt = x.to(arr(sk._s(opar.ctx[0])))
    got = x.back(par.decrypt(s_ntt, x.to(ct_arr(ct)), 0))
    assert got.tolist() == want


_decrypt = {}


def _decrypt_on_threshold(n):
    rng = random.Random(4096)
    q = I.DEFAULT_128[n]
    t = I.stock_plaintext(n)
    opar = obfv.BfvParameters(n, t, moduli=q)
    sc = next(s for s in I.bfv_scalers() if s.name == "bfv%d_decrypt" % n)
    assert sc.frm == opar.ctx[0].moduli and sc.to == opar.plaintext_context.moduli
    cols = I.w_window(sc, 2048) + I.v_window(sc, 1024) + I.w_zero(sc)
    for k, c in I.range_columns(sc).items():
        cols += c
    assert len(cols) <= n
    dist = sorted(I.w_distance(sc.rns, c) for c in cols[:2048])
    assert dist[1024] <= 1 << 70
    while len(cols) < n:
        cols.append([rng.randrange(m) for m in q])
    rng.shuffle(cols)
    ctx = opar.ctx[0]
    phase = Poly(ctx, POWER_BASIS, [[c[r] for c in cols] for r in range(len(q))]).into_ntt()
    sk = obfv.SecretKey.random(opar, rng)
    c1 = obfv.random_poly(ctx, phase.rep, rng)
    ct = obfv.Ciphertext(opar, [phase.sub(c1.mul(sk._s(ctx))), c1], 0)
    want = sk.decrypt(ct)
    # (the oracle's decrypt IS the scaler on these columns: row 0 of RnsScaler::scale, + t, mod q_0, mod t)
    assert want[:8] == [(sc.rns.scale(c, 1, 0)[0] + t) % q[0] % t for c in cols[:8]]
    return opar, sk, ct, want
