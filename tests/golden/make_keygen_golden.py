#!/usr/bin/env python3
"""Generates tests/golden/keygen_default128_digest.json: SHA-256 digests of a relinearization key and a Galois key
(exponent 3, a column rotation by one) generated from a fixed secret and fixed seeds at level 0 of the reference's stock
set n = 8192 (default_parameters_128(20), parameters.rs:218-260), computed by the test-side restatement
(tests/keygen_ref.py).  tests/test_keygen_gpu.py compares the engine's keys with them.

    python tests/golden/make_keygen_golden.py        # rewrites the fixture in place"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))

import encrypt_ref as ER  # noqa: E402
import keygen_ref as R  # noqa: E402
import make_encode_golden as G  # noqa: E402
import ref_params  # noqa: E402
from fhe_oracle import bfv as obfv  # noqa: E402

N = 8192
EXPONENT = 3


def seed(tag):
    """32 fixed seed bytes: tag, then counting bytes."""
    return bytes([tag] + list(range(31)))


SK, RK, GK = 11, 12, 13


def compute():
    t = ref_params.plaintext_modulus(N)
    opar = obfv.BfvParameters(N, t, moduli=ref_params.DEFAULT_128[N])
    ctx = opar.ctx[0]
    s = ER.samples(seed(SK), N, opar.variance)[0]
    out = {"n": N, "t": t, "moduli": ref_params.DEFAULT_128[N], "variance": opar.variance, "exponent": EXPONENT}
    for name, tag, frm in (("rk", RK, R.relin_from(opar, s, 0, 0)), ("gk", GK, R.galois_from(opar, s, EXPONENT, 0, 0))):
        c0, c1, K = R.ksk(ctx, ctx, opar.variance, s, frm, seed(tag))
        out[name] = {"c0": G.sha(c0), "c1": G.sha(c1), "seed": K.hex()}
    return out


if __name__ == "__main__":
    d = compute()
    with open(os.path.join(HERE, "keygen_default128_digest.json"), "w") as f:
        json.dump(d, f, indent=1)
        f.write("\n")
    print(d)
