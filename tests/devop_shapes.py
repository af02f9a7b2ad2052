"""Parameter shapes for the device encode / encrypt / key-generation families beyond the stock sets: deterministic
tuples (n, moduli_sizes, t, variance, batch), in the style of full_size.random_shape.

The seven whole-row kernels of these families are instantiated once per tile size LOGM = log2 N in 3 ... 14 and per
row kind.  The kind of a launch follows from the widest modulus of the rows it covers:
  general  one modulus >= 2^60                                   (LOGM 3 ... 14)
  narrow   every modulus below 2^60, one of them >= 2^50         (LOGM 3 ... 14; below LOGM 12 also every narrower set)
  F64 class 3 / 4 / 5 at LOGM 12 ... 14: the widest modulus in [2^49, 2^50) / [2^48, 2^49) / below 2^48
That is 2 x 12 + 3 x 3 = 33 instances per kernel.  generate_prime(bits, ...) returns a prime in [2^(bits - 1), 2^bits),
so a "50-bit" modulus is class 3, a "49-bit" one class 4, 48 bits and fewer class 5, 51 ... 60 bits narrow and 61 or
62 bits general.  The rows of the ciphertext moduli take their kind from the moduli of the level they run at (level l
keeps the first L - l moduli); the row mod t (encode_simd_t_kernel, decode_simd_kernel) takes it from t alone.
The multiparty share kernel has the same 33 row kinds in each of its three forms (mbfv_all_cells, mbfv_cells).

Nothing here imports the engine."""
import random

from fhe_oracle.bfv import generate_moduli
from fhe_oracle.zq import generate_prime

KERNELS = ("encode_simd_t_kernel", "encode_lift_kernel", "decode_simd_kernel", "small_ntt_kernel", "encrypt_sk_kernel",
           "encrypt_pk_kernel", "ksk_gen_kernel")
T_KERNELS = ("encode_simd_t_kernel", "decode_simd_kernel")
LOGMS = range(3, 15)
F64_LOGMS = range(12, 15)
KINDS = ("general", "narrow", "f64_3", "f64_4", "f64_5")


def row_kind(moduli, logm):
    """The instance kind of a whole-row launch over `moduli` at 2^logm points (the module docstring's rule)."""
    widest = max(moduli)
    if logm in F64_LOGMS and widest < (1 << 50):
        return "f64_3" if widest >> 49 else "f64_4" if widest >> 48 else "f64_5"
    return "general" if widest >> 60 else "narrow"


def all_cells():
    """Every (kernel, LOGM, kind) instance: 7 x 33."""
    kinds = [(lm, k) for lm in LOGMS for k in KINDS[:2]] + [(lm, k) for lm in F64_LOGMS for k in KINDS[2:]]
    return {(kern, lm, k) for kern in KERNELS for lm, k in kinds}


def plaintext_prime(bits, n, moduli):
    """generate_prime(bits, 2n, 2^bits), stepped to the next prime below while it is one of `moduli` (a plaintext
    modulus equal to a ciphertext modulus is NonInvertible); None when no such prime has `bits` bits."""
    t = generate_prime(bits, 2 * n, 1 << bits)
    while t is not None and t in moduli:
        t = generate_prime(bits, 2 * n, t)
    return t


def shape(n, sizes, t_bits, variance, batch):
    t = plaintext_prime(t_bits, n, generate_moduli(sizes, n))
    assert t is not None, (n, sizes, t_bits)
    return n, list(sizes), t, variance, batch


# ciphertext moduli by kind (the rotation index is LOGM, so neighbouring tile sizes see different lists)
_GENERAL = ([62, 45, 36], [61, 50], [36, 62], [60, 61, 40])     # [36, 62]: the deepest level alone is narrow / class 5
_NARROW = ([60, 52, 30], [58, 40], [54, 59, 27])                # a 60-bit prime is the widest the narrow passes take
_CLASS3 = ([50, 40], [44, 50, 36], [50, 50])
_CLASS4 = ([49, 36], [49, 44, 27], [40, 49])
_CLASS5 = ([48, 27], [44, 40, 30], [48, 48])
# plaintext moduli: a narrow t on the general shapes (51 ... 59 bits exceed their narrower q_i; 20 bits is the stock
# size, narrow below LOGM 12 and class 5 from there on, so LOGM 13 takes the narrowest narrow width in its place), a
# 61-bit t -- wider than every q_i -- on the narrow ones, and at LOGM 12 ... 14 class 4 on the class-3 shapes, class 5
# on the class-4 shapes and class 3 (wider than every q_i) on the class-5 shapes
_T_NARROW = (55, 20, 59)
_T_NARROW_F64_LOGMS = (55, 51, 59)
_T_CLASS5 = (48, 20, 33)
_VARIANCES = (10, 3, 17, 1, 16, 32)
_BATCHES = (2, 1, 3)   # (at most 2 from N = 8192 on: the restatements draw every sample in Python)


def matrix_shapes():
    """The fixed list that reaches every instance of all_cells(): per LOGM one general and one narrow shape, and at
    LOGM 12 ... 14 one shape per F64 class; the kind of t rotates against the kind of the q_i."""
    out = []

    def add(n, sizes, t_bits):
        i = len(out)
        batch = _BATCHES[i % len(_BATCHES)]
        out.append(shape(n, sizes, t_bits, _VARIANCES[i % len(_VARIANCES)], min(batch, 2) if n >= 8192 else batch))

    for lm in LOGMS:
        n = 1 << lm
        add(n, _GENERAL[lm % 4], (_T_NARROW_F64_LOGMS if lm in F64_LOGMS else _T_NARROW)[lm % 3])
        add(n, _NARROW[lm % 3], 61)
        if lm in F64_LOGMS:
            add(n, _CLASS3[lm % 3], 49)
            add(n, _CLASS4[lm % 3], _T_CLASS5[lm % 3])
            add(n, _CLASS5[lm % 3], 50)
    return out


def cells(shp):
    """The instances the cases of tests/test_devop_shapes_gpu.py launch for one shape: the lift, the samplers and both
    encryptions at level 0 and at the deepest level, key generation over the level-0 key context, the row mod t."""
    n, sizes, t, _v, _b = shp
    lm = n.bit_length() - 1
    q = generate_moduli(sizes, n)
    out = {(k, lm, row_kind([t], lm)) for k in T_KERNELS}
    for rows in (q, q[:1]):
        out |= {(k, lm, row_kind(rows, lm)) for k in KERNELS if k not in T_KERNELS and k != "ksk_gen_kernel"}
    out.add(("ksk_gen_kernel", lm, row_kind(q, lm)))
    return out


# The multiparty share kernel, mbfv_share_kernel<LOGM, NARROW, F64, FORM>, goes through the same dispatcher: the same 33
# row kinds, times its three forms (kernels_mbfv.hpp: MBFV_AX = 0, MBFV_AXX = 1, MBFV_AX_WY = 2).
MBFV_KERNEL = "mbfv_share_kernel"
MBFV_FORMS = (0, 1, 2)


def mbfv_all_cells():
    """Every (mbfv_share_kernel, LOGM, kind, form) instance: 33 x 3."""
    return {(MBFV_KERNEL, lm, k, f) for kern, lm, k in all_cells() if kern == KERNELS[0] for f in MBFV_FORMS}


def mbfv_cells(shp):
    """The instances mbfv_shape_cases.case_shape launches for one shape: MBFV_AX (the public-key share at level 0, the
    decryption share, round-1 h1, round-2 h0) and MBFV_AXX (the secret-key-switch share, round-2 h1) at the kind of
    level 0 and at the kind of the deepest level; MBFV_AX_WY (round-1 h0) at the kind of level 0 alone, and only when
    the relin rounds run (two moduli or more: they run over the level-0 context)."""
    n, sizes, _t, _v, _b = shp
    lm = n.bit_length() - 1
    q = generate_moduli(sizes, n)
    out = {(MBFV_KERNEL, lm, row_kind(rows, lm), f) for rows in (q, q[:1]) for f in MBFV_FORMS[:2]}
    if len(q) >= 2:
        out.add((MBFV_KERNEL, lm, row_kind(q, lm), MBFV_FORMS[2]))
    return out


# the round-trip pins (encode -> encrypt -> decrypt -> decode, the oracle's decrypt, the noise bound): a general
# shape, a class-3 shape and one whose 61-bit t sends decryption through a plaintext context of two moduli (61 + 60
# bits need [62, 59]).  SecretKey::try_decrypt reads the scaled phase d in (-t/2, t/2) from its residue mod q_0 alone, as
# (d + t) mod q_0 (secret_key.rs:232-238), so it -- and the engine, which follows it -- decrypts only when
# 3t/2 < q_0: a 61-bit t needs a 62-bit q_0.  log q - log t at level 0: 143 - 55, 140 - 49, 151 - 61 bits, each >= 40.
def roundtrip_shapes():
    return [shape(4096, [62, 45, 36], 55, 10, 2), shape(4096, [50, 50, 40], 49, 10, 2), shape(1024, [62, 59, 30], 61, 10, 2)]


_N_LOGS = range(3, 15)
_Q_BITS = (27, 36, 44, 48, 49, 50, 54, 58, 60, 61, 62)
_T_BITS = (13, 20, 33, 48, 49, 50, 55, 61)


def random_shape(idx):
    """A deterministic 'random' shape from the same axes: N from 8 to 16384, up to 4 moduli, the kind of t independent
    of theirs, every variance class of the sampler (<= 16 packed, > 16 two words per sample), batch 1 ... 5.  A width of
    t that has no prime = 1 mod 2N (13 bits from N = 2048 on) steps to the next wider one of the list."""
    rng = random.Random(0xDE70 + idx)
    n = 1 << rng.choice(_N_LOGS)
    sizes = [rng.choice(_Q_BITS) for _ in range(rng.randrange(1, 5))]
    ti = rng.randrange(len(_T_BITS))
    variance = rng.choice((1, 3, 10, 16, 17, 32))
    batch = rng.randrange(1, 6)
    q = generate_moduli(sizes, n)
    t = None
    while t is None:
        t = plaintext_prime(_T_BITS[ti], n, q)
        ti += 1
    return n, sizes, t, variance, batch
