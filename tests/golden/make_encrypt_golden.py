#!/usr/bin/env python3
"""Generates tests/golden/encrypt_default128_digest.json: SHA-256 digests of SecretKey::random, PublicKey::new and
secret-key / public-key encryptions of the Delta-scaled SIMD encodings of fixed values, at level 0 of the reference's
stock set n = 8192 (default_parameters_128(20), parameters.rs:218-260), with fixed seeds, computed by the test-side
restatement (tests/encrypt_ref.py).  tests/test_encrypt_gpu.py compares the engine's outputs with them.

    python tests/golden/make_encrypt_golden.py        # rewrites the fixture in place"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))

import numpy as np  # noqa: E402

import encode_ref as ER  # noqa: E402
import encrypt_ref as R  # noqa: E402
import make_encode_golden as G  # noqa: E402
import ref_params  # noqa: E402
from fhe_oracle import bfv as obfv  # noqa: E402

N = 8192


def seed(tag, i=0):
    """32 fixed seed bytes: tag, item index, then counting bytes."""
    return bytes([tag, i] + list(range(30)))


SK, PK_A, PK_E, A, E, U = 1, 2, 3, 4, 5, 6


def compute():
    t = ref_params.plaintext_modulus(N)
    opar = obfv.BfvParameters(N, t, moduli=ref_params.DEFAULT_128[N])
    ctx = opar.ctx[0]
    v = opar.variance
    pts = np.stack([ER.encode(opar, x, "simd", 0, True) for x in G.golden_values(t)])
    s = R.small(ctx, v, seed(SK))
    pk = R.encrypt_sk(ctx, v, s, seed(PK_A), seed(PK_E))
    sk_ct = np.stack([R.encrypt_sk(ctx, v, s, seed(A, b), seed(E, b), pts[b]) for b in range(2)])
    pk_ct = np.stack([R.encrypt_pk(ctx, v, pk, seed(U, b), pts[b]) for b in range(2)])
    return {"n": N, "t": t, "moduli": ref_params.DEFAULT_128[N], "variance": v, "s_ntt": G.sha(s), "pk": G.sha(pk),
            "sk_ct": G.sha(sk_ct), "pk_ct": G.sha(pk_ct)}


if __name__ == "__main__":
    d = compute()
    with open(os.path.join(HERE, "encrypt_default128_digest.json"), "w") as f:
        json.dump(d, f, indent=1)
        f.write("\n")
    print(d)
