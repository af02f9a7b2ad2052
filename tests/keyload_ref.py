"""Test-side expectation for key-switching keys on the wire (crates/fhe/src/bfv/keys/key_switching_key.rs:365-482,
`From<&KeySwitchingKey> for KeySwitchingKeyProto` and `try_convert_from`), built from restatements that exist:
tests/keygen_ref.py makes the key (`ksk`: K by `derive`, c1 by `digit_seeds` + `seeded.random_from_seed`, the twins by
`shoup`), the plain-C oracle takes c0 / c1 to PowerBasis and `fhe_oracle.rq.poly_to_wire` packs them.

Shared by tests/keyload_cases.py, tests/test_keyload_emu.py and tests/test_keyload_gpu.py."""
import random

import numpy as np

import encrypt_ref as ER
import keygen_ref as R
from fhe_oracle import seeded
from fhe_oracle.rq import POWER_BASIS, Poly, poly_to_wire

_keys = {}


def wire_bits(q):
    return (q - 1).bit_length()


def poly_bytes(kc):
    return sum(kc.degree * wire_bits(q) // 8 for q in kc.moduli)


def to_wire(kc, words):
    """Ntt words [nd][Lk][N] -> uint8 [nd][poly_bytes]: each digit's `coefficients` payload."""
    r = ER.Ring.of(kc).c
    out = []
    for p in np.asarray(words):
        pb = r.poly_ntt_backward(np.ascontiguousarray(p))
        out.append(np.frombuffer(poly_to_wire(Poly(kc, POWER_BASIS, [[int(w) for w in row] for row in pb])), dtype=np.uint8))
    return np.array(out)


def seeded_c1(kc, K, nd):
    """generate_c1(ctx_ksk, K, nd) as Ntt words."""
    return np.array([seeded.random_from_seed(kc.moduli, kc.degree, sd) for sd in R.digit_seeds(K, nd)], dtype=np.uint64)


def key(opar, cl, kl, seed):
    """One restated key from level cl to level kl, cached and left unchanged: dict(c0, c1 [nd][Lk][N] Ntt words, K,
    c0s, c1s the twins, w0, w1 the wire bytes [nd][poly_bytes], nd, lb)."""
    ident = (id(opar), cl, kl, seed)
    if ident not in _keys:
        ct, kc = opar.ctx[cl], opar.ctx[kl]
        rng = random.Random(seed)
        sd = bytes(rng.getrandbits(8) for _ in range(32))
        s = ER.samples(bytes(rng.getrandbits(8) for _ in range(32)), kc.degree, opar.variance)[0]
        frm = np.array([[rng.randrange(q) for _ in range(kc.degree)] for q in kc.moduli], dtype=np.uint64)
        c0, c1, K = R.ksk(ct, kc, opar.variance, s, frm, sd)
        nd, lb = R.digits(ct, kc)
        k = dict(c0=c0, c1=c1, K=K, c0s=np.array([R.shoup(p, kc) for p in c0]), c1s=np.array([R.shoup(p, kc) for p in c1]),
                 w0=to_wire(kc, c0), w1=to_wire(kc, c1), nd=nd, lb=lb)
        for v in k.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _keys[ident] = k
    return _keys[ident]
