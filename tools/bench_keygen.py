#!/usr/bin/env python3
"""Key generation on the device against creation from host arrays, on the reference's stock sets n = 4096 / 8192 / 16384
(tests/ref_params.py), the FP64 kernels on and off:
  relin_key       one RelinearizationKey.generate (fhe_bfv_relin_key_generate_dev), ms per key
  ek_pir          one EvaluationKey.generate of the PIR set (expansion level log2 N, inner sum, row rotation: one batched
                  fhe_bfv_galois_keys_generate_dev), ms per call and keys in it
  galois_batch    GaloisKey.generate of --batch keys in one call, keys per second
Two yardsticks from the same process ride on every record:
  sk_encrypt_per_s_over_ndigits   secret-key encryptions of a batch of 1,024 per second divided by ndigits (a key is
                                  ndigits encryptions over the key context)
  ksk_create_host_ms              fhe_ksk_create of the same relinearization key from host arrays (what a host that
                                  generates keys itself pays: two uploads, then the device's range check, Shoup twins
                                  and F64 words), ms per key
Timing: wall clock around `--reps` calls after one warm-up call, the stream synchronised before and after, median of
three windows (key generation allocates each key's buffers on the host side, so device-event timing would miss it).
One JSON line per record on stdout (and to --out).  Kernel times: run it under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fhe_rs_amd as fhe  # noqa: E402
import ref_params  # noqa: E402


def wall_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / reps)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="4096,8192,16384")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for n in (int(x) for x in a.sets.split(",")):
        t = ref_params.plaintext_modulus(n)
        moduli = ref_params.DEFAULT_128[n]
        L = len(moduli)
        par = fhe.BfvParameters(n, t, moduli=moduli)
        ctx = par.context_at_level(0)
        sk = fhe.SecretKey.random(par, bytes(range(32)))
        rng = np.random.default_rng(n)
        dev = lambda *shape: torch.from_numpy(rng.integers(0, 256, size=shape, dtype=np.uint8)).cuda()   # noqa: E731
        s1, sb = dev(1, 32), dev(a.batch, 32)
        exps = fhe.EvaluationKey.exponents(n, row_rotation=True, inner_sum=True, expansion_level=n.bit_length() - 1)
        se = dev(len(exps), 32)
        enc = par.encoder()
        pts = enc.encode(torch.from_numpy(rng.integers(0, t, size=(1024, n), dtype=np.uint64).view(np.int64)).cuda(),
                         "simd", 0, True)
        ea, ee = dev(1024, 32), dev(1024, 32)
        # the host-array yardstick: the same key's arrays on the host, made into a handle by fhe_ksk_create
        host = [x.cpu().numpy().view(np.uint64) for x in fhe.RelinearizationKey.generate(sk, s1).ksk.export()[:2]]
        for f64 in (True, False):
            fhe.set_f64(f64)
            enc_ms = wall_ms(lambda: sk.encrypt(pts, 0, ea, ee), a.reps)
            create_ms = wall_ms(lambda: fhe.KeySwitchingKey(ctx, ctx, host[0], host[1]), a.reps)
            yard = dict(sk_encrypt_per_s_over_ndigits=round(1024 / enc_ms * 1e3 / L, 1),
                        ksk_create_host_ms=round(create_ms, 4))
            cases = (("relin_key", 1, lambda: fhe.RelinearizationKey.generate(sk, s1)),
                     ("ek_pir", len(exps), lambda: fhe.EvaluationKey.generate(
                         sk, row_rotation=True, inner_sum=True, expansion_level=n.bit_length() - 1, seeds=se)),
                     ("galois_batch", a.batch, lambda: fhe.GaloisKey.generate(sk, [3] * a.batch, sb)))
            for name, keys, fn in cases:
                ms = wall_ms(fn, a.reps if keys < 64 else 1)
                row = dict(n=n, moduli=L, ndigits=L, f64=f64, op=name, keys=keys, ms=round(ms, 4),
                           keys_per_s=round(keys / ms * 1e3, 1), **yard)
                print(json.dumps(row), flush=True)
                lines.append(row)
        fhe.set_f64(True)
        fhe.workspace_trim()
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
