#!/usr/bin/env python3
"""Multiparty BFV throughput on the device.  Shares: public-key shares, decryption shares and relin round-1 shares per
second (fhe_mbfv_pk_share_dev / fhe_mbfv_sks_share_dev / fhe_mbfv_rlk_round1_dev, one secret shared by the batch, fresh
outputs per call) on the reference's stock sets n = 4096 / 8192 / 16384 (tests/ref_params.py), batch 1,024 (the relin
round: --rlk-batch, L x L rows per item), the FP64 kernels on and off, next to the fhe_bfv_encrypt_sk_dev rate and the
Poly::small (to_ntt = 1) rate of the same process: a single-draw share does a subset of a secret-key encryption's work
(no seed expansion, no copy of `a`) and more than the bare sample + transform.  Aggregator: fhe_mbfv_aggregate_dev over
2, 8 and 32 shares of 1,024 polynomials at n = 8192, bytes moved (shares read + result written) over time as a fraction
of fhe_ubench_copy on the same byte count.  Timing: torch events on the current stream around `REPS` calls after one
warm-up call, median of three windows.  One JSON line per case on stdout (and to --out, by default
profiles/mbfv_bench.jsonl).  Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/bench_mbfv.py`."""
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
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rlk-batch", type=int, default=64)
    ap.add_argument("--shares", default="2,8,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mbfv_bench.jsonl"))
    a = ap.parse_args()
    timeit = bench.make_timeit(torch, a.reps)
    lines = []

    def emit(row):
        print(json.dumps(row), flush=True)
        lines.append(row)

    for n in (int(x) for x in a.sets.split(",")):
        t = ref_params.plaintext_modulus(n)
        moduli = ref_params.DEFAULT_128[n]
        L = len(moduli)
        par = fhe.BfvParameters(n, t, moduli=moduli)
        ctx = par.context_at_level(0)
        sk = fhe.SecretKey.random(par, bytes(range(32)))
        rng = np.random.default_rng(n)
        batch, rb = a.batch, a.rlk_batch
        seeds = [torch.from_numpy(rng.integers(0, 256, size=(batch, 32), dtype=np.uint8)).cuda() for _ in range(2)]
        ct = ctx.synth_uniform(7, 0, 0, 2, batch)
        crp = fhe.CommonRandomPoly(par, ctx.synth_uniform(8, 0, 0, 1, 1)[0][0])
        crpv = fhe.CommonRandomPoly(par, ctx.synth_uniform(9, 0, 0, L, 1)[0])
        # one party's shares for a batch: the ABI directly, its secret shared
        L_ = fhe._lib.lib()
        import ctypes as C
        p = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
        out = torch.empty((batch, L, n), dtype=torch.int64, device="cuda")
        h0 = torch.empty((rb, L, L, n), dtype=torch.int64, device="cuda")
        h1 = torch.empty_like(h0)
        gen = fhe.RelinKeyGenerator(sk, crpv, bytes(range(3, 35))) if L > 1 else None
        st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731

        def chk(code):
            assert code == 0, code

        cases = [("mbfv_pk_share", batch, lambda: chk(L_.fhe_mbfv_pk_share_dev(
                      ctx._h, par.variance, p(crp.poly), p(sk.s_ntt), 1, p(seeds[0]), p(out), batch, st()))),
                 ("mbfv_decryption_share", batch, lambda: chk(L_.fhe_mbfv_sks_share_dev(
                      ctx._h, par.variance, p(sk.s_ntt), None, 1, C.c_void_p(ct.data_ptr() + 8 * L * n), 2 * L * n,
                      p(seeds[0]), p(out), batch, st()))),
                 ("encrypt_sk", batch, lambda: sk.encrypt(None, 0, seeds[0], seeds[1])),
                 ("sample_small_ntt", batch, lambda: ctx.sample_small(seeds[0], par.variance, True))]
        if gen is not None:
            cases.insert(2, ("mbfv_rlk_round1", rb, lambda: chk(L_.fhe_mbfv_rlk_round1_dev(
                ctx._h, par.variance, p(sk.s_ntt), p(gen.u), 1, p(crpv.poly), p(seeds[1]), p(h0), p(h1), rb, st()))))
        for f64 in (True, False):
            fhe.set_f64(f64)
            for name, items, fn in cases:
                ms = statistics.median(timeit(fn) for _ in range(3))
                emit(dict(n=n, t=t, moduli=L, batch=items, f64=f64, op=name, ms=round(ms, 5),
                          items_per_s=round(items / ms * 1e3, 1)))
        fhe.set_f64(True)
        if n == 8192:
            npolys = 1024
            words = npolys * L * n
            for k in (int(x) for x in a.shares.split(",")):
                sh = ctx.synth_uniform(11, 0, 0, 1, k * npolys)
                res = torch.empty((npolys, L, n), dtype=torch.int64, device="cuda")
                ms = statistics.median(timeit(lambda: chk(L_.fhe_mbfv_aggregate_dev(
                    ctx._h, p(sh), k, words, npolys, None, p(res), st()))) for _ in range(3))
                moved = (k + 1) * words * 8
                copy = fhe.ubench_copy(moved // 2)   # (a copy of half the bytes reads and writes as many)
                emit(dict(n=n, moduli=L, op="mbfv_aggregate", nshares=k, npolys=npolys, ms=round(ms, 5),
                          bytes_moved=moved, gb_per_s=round(moved / ms / 1e6, 1), copy_gb_per_s=round(copy / 1e9, 1),
                          fraction_of_copy=round(moved / ms * 1e3 / copy, 3)))
                del sh, res
        del ct, out, h0, h1, seeds
        fhe.workspace_trim()
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
