#!/usr/bin/env python3
"""Plaintext moduli above 64 bits on the device: scaled encodes per second (fhe_bfv_encode_big_dev) and decryptions per
second (fhe_bfv_decrypt_big_dev) at N = 8192 with five 60-bit moduli, batch 1024, t = 2^127 - 1; in the same process
and on the same moduli with a 20-bit t, the u64 Poly encode (fhe_bfv_encode_dev) and fhe_bfv_decrypt_dev.  A second
pass with the engine's per-launch profiler on (its symbols are the ones rocprofv3 prints; for the trace itself run
`rocprofv3 --kernel-trace --stats -- python tools/bench_bigt.py`) records the share of each call's summed kernel time
(not of the timed call) spent in bigt_project_kernel / bigt_tail_kernel and both kernels' bytes over time as a fraction
of fhe_ubench_copy.
Timing: torch events on the current stream around `REPS` calls after one warm-up call, median of three windows.  One
JSON line per case on stdout (and to --out, default profiles/bigt_bench.jsonl)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import fhe_rs_amd as fhe  # noqa: E402

BIG_T = (1 << 127) - 1


def kernel_ms(fn, pattern):
    """(ms in kernels whose symbol contains `pattern`, ms in all kernels) of one call of fn() under the engine's profiler."""
    fn()
    fhe.prof_reset()
    fhe.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        entries = fhe.prof_entries()
    finally:
        fhe.prof_enable(False)
        fhe.prof_reset()
    return sum(ms for _l, sym, _n, ms in entries if pattern in sym), sum(ms for _l, _s, _n, ms in entries)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bigt_bench.jsonl"))
    a = ap.parse_args()
    n, batch = a.n, a.batch
    timeit = bench.make_timeit(torch, a.reps)
    copy_bytes_per_s = fhe.ubench_copy(1 << 30, 0.2)
    moduli = fhe.generate_moduli([60] * 5, n)
    L = len(moduli)
    rng = np.random.default_rng(n + batch)
    lines = []

    def record(**row):
        print(json.dumps(row), flush=True)
        lines.append(row)

    # the big set: t = 2^127 - 1 (W_t = 2, four plaintext-context rows)
    par = fhe.BfvParameters(n, BIG_T, moduli=moduli)
    enc = par.encoder()
    wt, P = par.plaintext_limbs, par.plaintext_context().nmoduli
    sk = fhe.SecretKey.random(par, bytes(range(32)))
    limbs = rng.integers(0, 1 << 63, size=(batch, n, wt), dtype=np.uint64)
    m = torch.from_numpy(limbs.view(np.int64)).cuda()
    seeds = torch.from_numpy(rng.integers(0, 256, size=(2, batch, 32), dtype=np.uint8)).cuda()
    cts = sk.encrypt(enc.encode(m, "poly", 0, True), 0, seeds[0], seeds[1])
    assert torch.equal(sk.decrypt(cts, 0), m), "the big set does not round-trip"
    big = (("encode_big_scaled", lambda: enc.encode(m, "poly", 0, True), "bigt_project_kernel", (wt + L) * n * 8),
           ("decrypt_big", lambda: sk.decrypt(cts, 0), "bigt_tail_kernel", (P + wt) * n * 8))
    for name, fn, kernel, bytes_per_item in big:
        ms = statistics.median(timeit(fn) for _ in range(3))
        k_ms, all_ms = kernel_ms(fn, kernel)
        record(n=n, t_bits=BIG_T.bit_length(), limbs=wt, plain_rows=P, moduli=L, batch=batch, op=name, ms=round(ms, 5),
               items_per_s=round(batch / ms * 1e3, 1), kernel=kernel, kernel_ms=round(k_ms, 5),
               kernel_share_of_kernel_time=round(k_ms / all_ms, 4) if all_ms else None,
               kernel_bytes_per_s=round(batch * bytes_per_item / (k_ms * 1e-3), 1) if k_ms else None,
               copy_bytes_per_s=round(copy_bytes_per_s, 1),
               kernel_fraction_of_copy=round(batch * bytes_per_item / (k_ms * 1e-3) / copy_bytes_per_s, 4) if k_ms else None)
    del m, cts
    fhe.workspace_trim()
    torch.cuda.empty_cache()

    # the yardstick: the same moduli under a 20-bit t, the u64 entry points
    t20 = fhe.generate_prime(20, 2 * n, (1 << 20) - 1)
    par = fhe.BfvParameters(n, t20, moduli=moduli)
    enc = par.encoder()
    sk = fhe.SecretKey.random(par, bytes(range(32)))
    m = torch.from_numpy(rng.integers(0, t20, size=(batch, n), dtype=np.uint64).view(np.int64)).cuda()
    cts = sk.encrypt(enc.encode(m, "poly", 0, True), 0, seeds[0], seeds[1])
    assert torch.equal(sk.decrypt(cts, 0), m)
    for name, fn in (("encode_u64_scaled", lambda: enc.encode(m, "poly", 0, True)), ("decrypt_u64", lambda: sk.decrypt(cts, 0))):
        ms = statistics.median(timeit(fn) for _ in range(3))
        record(n=n, t_bits=t20.bit_length(), limbs=1, moduli=L, batch=batch, op=name, ms=round(ms, 5),
               items_per_s=round(batch / ms * 1e3, 1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
