#!/usr/bin/env python3
"""Noise measurement throughput on the device: measure_noise per second with the expected plaintext given and with
m NULL (fhe_bfv_measure_noise_dev), centered_bits and lift polynomials per second (fhe_poly_centered_bits_dev,
fhe_poly_lift_dev) on the reference's stock sets n = 4096 / 8192 / 16384 (tests/ref_params.py), batches 1 and 1024; the
single-call latency is the batch-1 `ms`.  Yardsticks from the same process: the fhe_bfv_decrypt_dev rate of the same
ciphertexts (it shares the phase and the inverse transform) and fhe_ubench_copy's streaming rate over the bytes
centered_bits must read (L N 8 per polynomial).  Timing: torch events
on the current stream around `REPS` calls after one warm-up call, median of three windows.  One JSON line per case on
stdout (and to --out).  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_noise.py`."""
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
    ap.add_argument("--batches", default="1024,1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    timeit = bench.make_timeit(torch, a.reps)
    copy_bytes_per_s = fhe.ubench_copy(1 << 30, 0.2)
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
            m = torch.from_numpy(rng.integers(0, t, size=(batch, n), dtype=np.uint64).view(np.int64)).cuda()
            seeds = torch.from_numpy(rng.integers(0, 256, size=(batch, 32), dtype=np.uint8)).cuda()
            cts = pk.encrypt(enc.encode(m, "poly", 0, True), 0, seeds)
            polys = ctx.synth_uniform(7, 0, 0, 1, batch).view(batch, L, n)
            assert torch.equal(sk.decrypt(cts, 0), m)
            noise = sk.measure_noise(cts, 0, plaintext=m)
            assert torch.equal(noise, sk.measure_noise(cts, 0))
            cases = (("measure_noise_m_given", lambda: sk.measure_noise(cts, 0, plaintext=m)),
                     ("measure_noise_m_null", lambda: sk.measure_noise(cts, 0)),
                     ("decrypt", lambda: sk.decrypt(cts, 0)),
                     ("centered_bits", lambda: ctx.centered_bits(polys)),
                     ("lift", lambda: ctx.lift(polys)))
            for name, fn in cases:
                ms = statistics.median(timeit(fn) for _ in range(3))
                row = dict(n=n, t=t, moduli=L, limbs=ctx.lift_limbs, batch=batch, op=name, ms=round(ms, 5),
                           items_per_s=round(batch / ms * 1e3, 1))
                if name.startswith("measure_noise"):
                    row.update(noise_bits_max=int(noise.max().item()))
                if name == "centered_bits":
                    row.update(copy_bytes_per_s=round(copy_bytes_per_s, 1),
                               copy_yardstick_per_s=round(copy_bytes_per_s / (L * n * 8), 1))
                print(json.dumps(row), flush=True)
                lines.append(row)
            del m, cts, polys, seeds, noise
            fhe.workspace_trim()
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
