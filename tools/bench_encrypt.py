#!/usr/bin/env python3
"""Encryption throughput on the device: secret-key and public-key encryptions per second (fhe_bfv_encrypt_sk_dev /
fhe_bfv_encrypt_pk_dev, fresh seeds per call) and Poly::small (fhe_bfv_sample_small_dev, Ntt form) on the reference's
stock sets n = 4096 / 8192 / 16384 (tests/ref_params.py), batches 1 and 1024, the FP64 kernels on and off; the
single-call latency is the batch-1 `ms`.  Yardsticks from the same process: the batch row-NTT rate (forward NTT of
[1024][L][N]) divided by L (an sk encryption is one forward transform of L rows) and by 3L (pk: three), and the Poly
encode rate (one forward transform of L rows).  Timing: torch events on the current stream around `REPS` calls after
one warm-up call, median of three windows.  One JSON line per case on stdout (and to --out).  Kernel times: run it
under `rocprofv3 --kernel-trace --stats -- python tools/bench_encrypt.py`."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import fhe_rs_amd as fhe  # noqa: E402
import ref_params  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="4096,8192,16384")
    ap.add_argument("--batches", default="1,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    timeit = bench.make_timeit(torch, a.reps)
    lines = []
    for n in (int(x) for x in a.sets.split(",")):
        t = ref_params.plaintext_modulus(n)
        moduli = ref_params.DEFAULT_128[n]
        L = len(moduli)
        par = fhe.BfvParameters(n, t, moduli=moduli)
        enc = par.encoder()
        ctx = par.context_at_level(0)
        sk = fhe.SecretKey.random(par, bytes(range(32)))
        pk = fhe.PublicKey(sk, bytes(range(1, 33)), bytes(range(2, 34)))
        for batch in (int(x) for x in a.batches.split(",")):
            rng = np.random.default_rng(n + batch)
            v = torch.from_numpy(rng.integers(0, t, size=(batch, n), dtype=np.uint64).view(np.int64)).cuda()
            pts = enc.encode(v, "simd", 0, True)
            seeds = [torch.from_numpy(rng.integers(0, 256, size=(batch, 32), dtype=np.uint8)).cuda() for _ in range(2)]
            polys = ctx.synth_uniform(7, 0, 0, 1, batch).view(batch, L, n)
            cases = (("encrypt_sk", lambda: sk.encrypt(pts, 0, seeds[0], seeds[1])),
                     ("encrypt_pk", lambda: pk.encrypt(pts, 0, seeds[0])),
                     ("sample_small_ntt", lambda: ctx.sample_small(seeds[0], par.variance, True)),
                     ("encode_poly", lambda: enc.encode(v, "poly")),
                     ("row_ntt_forward", lambda: ctx.ntt_forward(polys)))
            for f64 in (True, False):
                fhe.set_f64(f64)
                for name, fn in cases:
                    ms = statistics.median(timeit(fn) for _ in range(3))
                    row = dict(n=n, t=t, moduli=L, batch=batch, f64=f64, op=name, ms=round(ms, 5),
                               items_per_s=round(batch / ms * 1e3, 1))
                    if name == "row_ntt_forward":
                        rows_per_s = batch * L / ms * 1e3
                        row.update(row_ntt_per_s=round(rows_per_s, 1), sk_yardstick_per_s=round(rows_per_s / L, 1),
                                   pk_yardstick_per_s=round(rows_per_s / (3 * L), 1))
                    print(json.dumps(row), flush=True)
                    lines.append(row)
            fhe.set_f64(True)
            del v, pts, polys, seeds
            fhe.workspace_trim()
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
