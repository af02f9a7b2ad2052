"""Plain Python-int restatements of the streaming operations (fhe.rs_amd/csrc/kernels_misc.hpp: dot_kernel<1|2>,
mul_plain_kernel, switch_down_kernel, substitute_kernel, the four wire kernels), written from the reference's semantics
and NOT through the oracle's classes: exact integer arithmetic on object arrays, one `%` per result word, no lazy
ranges, no Shoup constants, no shift registers.  tests/streamop_cases.py compares the engine with these word for word
and, once per operation, these with oracle/fhe_oracle, so the two cannot drift apart.

Arrays are numpy uint64 in the engine's layouts ([..., L, N], moduli along the axis before the last); every function
returns uint64."""
import numpy as np


def ints(a):
    """uint64 array -> object array of Python ints (exact arithmetic from here on)."""
    return np.asarray(a, dtype=np.uint64).astype(object)


def words(a):
    return np.asarray(a, dtype=object).astype(np.uint64)


def qcol(q):
    """The moduli as an object column [L, 1], broadcasting over [..., L, N]."""
    return np.array([int(m) for m in q], dtype=object)[:, None]


# ---- dot product and ct x pt ---------------------------------------------------------------------------------------------
def dot_threshold(q):
    """c* = ceil(2^128 / (q - 1)^2): the least count at which `count` products of two words at q - 1 reach 2^128 (the
    third limb of the accumulator)."""
    sq = (q - 1) ** 2
    c = -((-(1 << 128)) // sq)
    assert (c - 1) * sq < (1 << 128) <= c * sq
    return c


def dot_exact(cts, pts):
    """The exact sums: cts [count, parts, L, N], pts [count, L, N] -> object [parts, L, N], sum_k cts[k][p] * pts[k]."""
    return (ints(cts) * ints(pts)[:, None]).sum(axis=0)


def dot_product(cts, pts, q):
    """out[p][r][j] = (sum_k cts[k][p][r][j] * pts[k][r][j]) mod q_r; also the largest exact sum (whether the accumulator's
    third limb was needed)."""
    s = dot_exact(cts, pts)
    return words(s % qcol(q)), int(s.max())


def mul_plain(ct, pt, q):
    """ct [parts, L, N] times pt [L, N], word by word mod q_r."""
    return words(ints(ct) * ints(pt)[None] % qcol(q))


# ---- modulus switching ---------------------------------------------------------------------------------------------------
def switch_down(x, q):
    """Poly::switch_down on PowerBasis rows x [..., L, N] over q (L >= 2) -> [..., L - 1, N]: with h = q_L >> 1,
    out_i = ((x_i - ((x_L + h) mod q_L) + h) * q_L^-1) mod q_i."""
    q = [int(m) for m in q]
    ql, h = q[-1], q[-1] >> 1
    x = ints(x)
    last = (x[..., -1:, :] + h) % ql
    inv = np.array([pow(ql, -1, m) for m in q[:-1]], dtype=object)[:, None]
    return words((x[..., :-1, :] - last + h) * inv % qcol(q[:-1]))


def switch_down_levels(x, q, levels):
    """`levels` applications of switch_down, one modulus at a time (Poly::switch_down_to's loop)."""
    q = list(q)
    for _ in range(levels):
        x = switch_down(x, q)
        q = q[:-1]
    return np.asarray(x, dtype=np.uint64)


# ---- substitution x -> x^e -----------------------------------------------------------------------------------------------
def negated_indices(n, e):
    """The source indices j whose image j * e lands on an odd multiple of N (the coefficient changes sign)."""
    return [j for j in range(n) if (j * e) & n]


def substitute(x, q, e):
    """PowerBasis rows x [..., L, N]: coefficient j goes to index j * e mod N, negated when (j * e) & N."""
    x = ints(x)
    n = x.shape[-1]
    out = np.zeros_like(x)
    qv = np.array([int(m) for m in q], dtype=object)
    for j in range(n):
        v = x[..., j]
        out[..., (j * e) % n] = (-v) % qv if (j * e) & n else v
    return words(out)


# ---- wire format ---------------------------------------------------------------------------------------------------------
def wire_bits(q):
    return (int(q) - 1).bit_length()


def wire_size(q, n):
    return sum(wire_bits(m) * n // 8 for m in q)


def wire_pack(x, q):
    """One polynomial x [L, N] -> bytes: each row is ONE little-endian integer, coefficient j at bits [j * w, (j + 1) * w)
    with w = bitlen(q_r - 1); rows back to back."""
    out = b""
    for row, m in zip(np.asarray(x, dtype=np.uint64), q):
        w = wire_bits(m)
        mask = (1 << w) - 1
        big = 0
        for j, v in enumerate(row):
            big |= (int(v) & mask) << (j * w)
        out += big.to_bytes(len(row) * w // 8, "little")
    return out


def wire_unpack(data, q, n):
    """bytes -> [L, N] (masking only, as the reference: values are not reduced)."""
    data = bytes(data)
    assert len(data) == wire_size(q, n)
    rows, at = [], 0
    for m in q:
        w = wire_bits(m)
        size = n * w // 8
        big = int.from_bytes(data[at:at + size], "little")
        at += size
        rows.append([(big >> (j * w)) & ((1 << w) - 1) for j in range(n)])
    return np.array(rows, dtype=np.uint64)
