"""Test-side restatement of BFV plaintext encoding (crates/fhe/src/bfv/plaintext_vec.rs:70-102, plaintext.rs:157-196,
parameters.rs:711-725), built from the oracle's NTT operator over t (fhe_oracle.ntt) and its Poly forms
(`plaintext_poly_ntt`, `SecretKey.encode_poly`).  The transforms run on the plain-C oracle so that full-size sets
stay fast; `check_poly_forms` pins that path against the pure-Python oracle at small sizes.

Shared by tests/test_encode_emu.py, tests/test_encode_gpu.py and tests/golden/make_encode_golden.py."""
import functools

import numpy as np

from fhe_oracle import bfv as obfv
from fhe_oracle import coracle
from fhe_oracle.rq import Context as OCtx
from fhe_oracle.ntt import supports_ntt


@functools.lru_cache(maxsize=None)
def _index_map(n):
    return tuple(index_map(n))


def index_map(n):
    """matrix_reps_index_map (parameters.rs:711-725): generator 3, m = 2N, bit-reversed (pos-1)/2 and (m-pos-1)/2."""
    logn = n.bit_length() - 1

    def rev(v):
        return int(format(v, "0%db" % logn)[::-1], 2) if logn else 0

    m, pos, out = 2 * n, 1, [0] * n
    for i in range(n // 2):
        out[i] = rev((pos - 1) >> 1)
        out[n // 2 + i] = rev((m - pos - 1) >> 1)
        pos = (pos * 3) & (m - 1)
    return out


_tctx = {}


def t_context(t, n, psi=None):
    """The plain-C oracle over the single modulus t (NttOperator::new(t, N), parameters.rs:598), psi as given."""
    key = (t, n, psi)
    if key not in _tctx:
        _tctx[key] = coracle.CCtx(OCtx([t], n, None if psi is None else [psi]))
    return _tctx[key]


def simd_available(t, n):
    return supports_ntt(t, n)


def coefficients(values, t, n, encoding, psi=None):
    """encode_u64_chunk's coefficients mod t before the lift: Poly -> the values zero-padded, SIMD -> the values
    placed at map[i], then NttOperator::backward.  Values are reduced mod t first (what the engine does)."""
    c = np.zeros(n, dtype=np.uint64)
    v = np.asarray(values, dtype=np.uint64) % np.uint64(t)
    if encoding == "poly":
        c[: len(v)] = v
        return c
    c[np.asarray(_index_map(n)[: len(v)], dtype=np.int64)] = v
    return t_context(t, n, psi).ntt_backward_row(0, c)


_delta = {}


def _delta_rows(opar, level):
    """delta of one level as [L][N] uint64: a constant polynomial, so every Ntt slot of row i holds delta_i."""
    key = (id(opar), level)
    if key not in _delta:
        _delta[key] = (opar, np.array(opar.delta[level].coefficients, dtype=np.uint64))
    return _delta[key][1]


def lift(opar, coeffs, level, scaled, cctx=None):
    """Poly::try_convert_from + into_ntt (poly_ntt), or Plaintext::to_poly with scaled: coefficients times q_mod_t mod
    t, lift, NTT, times delta (parameters.rs:607-633).  -> [L_level][N] uint64."""
    t = opar.plaintext
    ctx = opar.ctx[level]
    c = np.asarray(coeffs, dtype=np.uint64)
    if scaled:
        c = ((c.astype(object) * opar.q_mod_t[level]) % t).astype(np.uint64)
    rows = np.stack([c % np.uint64(q) for q in ctx.moduli])
    cctx = cctx or coracle.CCtx(ctx)
    out = cctx.poly_ntt_forward(rows)
    if scaled:
        out = cctx.poly_mul(out, _delta_rows(opar, level))
    return out


def encode(opar, values, encoding, level=0, scaled=False, psi=None, cctx=None):
    return lift(opar, coefficients(values, opar.plaintext, opar.degree(), encoding, psi), level, scaled, cctx)


def decode(coeffs, t, n, encoding, psi=None):
    """Vec<u64>::try_decode (plaintext.rs:157-170, 408-431) on coefficients mod t."""
    c = np.asarray(coeffs, dtype=np.uint64) % np.uint64(t)
    if encoding == "poly":
        return c
    v = t_context(t, n, psi).ntt_forward_row(0, c)
    return v[np.asarray(_index_map(n), dtype=np.int64)]


def check_poly_forms(opar, values, level=0):
    """The Poly forms above equal the oracle's own (`plaintext_poly_ntt`, `SecretKey.encode_poly`)."""
    vals = [int(v) for v in values]
    want = obfv.plaintext_poly_ntt(opar, vals, level).coefficients
    assert encode(opar, vals, "poly", level).tolist() == want
    sk = obfv.SecretKey(opar, [0] * opar.degree())
    want = sk.encode_poly(vals, level).coefficients
    assert encode(opar, vals, "poly", level, scaled=True).tolist() == want
