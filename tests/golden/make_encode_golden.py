#!/usr/bin/env python3
"""Generates tests/golden/encode_default128_digest.json: SHA-256 digests of the level-0 SIMD encodings, unscaled
(`Plaintext::poly_ntt`) and Delta-scaled (`Plaintext::to_poly`), of fixed values under the reference's stock set
n = 8192 (default_parameters_128(20), parameters.rs:218-260), computed by the test-side restatement
(tests/encode_ref.py: the oracle's NTT over t and its Poly forms, on the plain-C oracle).  tests/test_encode_gpu.py
compares the engine's encodings with them.

    python tests/golden/make_encode_golden.py        # rewrites the fixture in place"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))

import numpy as np  # noqa: E402

import encode_ref as R  # noqa: E402
import ref_params  # noqa: E402
from fhe_oracle import bfv as obfv  # noqa: E402

N = 8192
SEED = 0x5EED8192


def golden_values(t, n=N, seed=SEED):
    """Two items of n values in [0, t): a splitmix64 stream, so that any host regenerates them without numpy's RNG."""
    out, x = [], seed
    for _ in range(2 * n):
        x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        out.append((z ^ (z >> 31)) % t)
    return np.array(out, dtype=np.uint64).reshape(2, n)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a, dtype=np.uint64)).tobytes()).hexdigest()


def compute():
    t = ref_params.plaintext_modulus(N)
    opar = obfv.BfvParameters(N, t, moduli=ref_params.DEFAULT_128[N])
    v = golden_values(t)
    out = {"n": N, "t": t, "moduli": ref_params.DEFAULT_128[N], "seed": SEED}
    for scaled in (False, True):
        enc = np.stack([R.encode(opar, v[b], "simd", 0, scaled) for b in range(2)])
        out["simd_scaled" if scaled else "simd"] = sha(enc)
    return out


if __name__ == "__main__":
    d = compute()
    with open(os.path.join(HERE, "encode_default128_digest.json"), "w") as f:
        json.dump(d, f, indent=1)
        f.write("\n")
    print(d)
