#!/usr/bin/env python3
"""Loading key-switching keys from their wire bytes on the device against the piecewise route, on the reference's stock sets
n = 4096 / 8192 / 16384 (tests/ref_params.py), for one relinearization key and for a 22-key evaluation key, seeded (c0
bytes + the 32-byte seed) and unseeded (c0 and c1 bytes):
  load_wire       KeySwitchingKey.from_wire (one fhe_ksk_load_wire_dev for all keys), keys per second
  today           the piecewise route (the record keeps its name, so that runs stay comparable), per key:
                  Context.deserialize(to_ntt=True) of c0 (fhe_poly_deserialize_dev), Context.random_from_seed of the
                  digit seeds (fhe_poly_from_seed_dev; the digit seeds themselves, a host ChaCha8 restatement in this
                  route, are prepared OUTSIDE the timed window, which flatters it) or deserialize of c1, then
                  KeySwitchingKey(c0, c1) (fhe_ksk_create_dev: device copies, range check and twins), keys per second
Both routes are timed in the same process, their windows alternating.  Two more figures ride on every record:
  ntt_rows_yardstick_keys_per_s   rows per second of one batched forward transform of 1,024 polynomials, divided by the
                                  rows a key transforms (ndigits x Lk, twice that with an explicit c1): what the transform
                                  alone would allow
  alloc6_ms_per_key               hipMalloc + hipFree of one key's buffers (four arrays, six when the key carries F64
                                  words) through the ABI's synchronous allocator, and `alloc_share` = that over the
                                  load route's time per key: whether the allocator or the kernels bound a batch
Timing: wall clock around enough calls to fill `--window` seconds after one warm-up call per shape, the device
synchronised before and after (both routes allocate on the host side, which device events would miss); median of
three windows, with the lowest and highest next to it.  One JSON line per record on stdout and in --out (default
profiles/keyload_bench.jsonl).  Kernel times: run it under `rocprofv3 --kernel-trace --stats`, in a run of its own."""
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
import keygen_ref  # noqa: E402
import ref_params  # noqa: E402

EK_KEYS = 22


def alternating_ms(fns, window_s):
    """{name: (median, low, high) ms per call} of the callables, their windows alternating; each window holds enough
    calls to last `window_s`."""
    reps = {}
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        reps[name] = max(1, int(window_s / max(time.perf_counter() - t0, 1e-6)))
    out = {name: [] for name in fns}
    for _ in range(3):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps[name]):
                fn()
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) * 1e3 / reps[name])
    return {name: (statistics.median(v), min(v), max(v)) for name, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="4096,8192,16384")
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyload_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_keyload needs a GPU")
    lines = []
    for n in (int(x) for x in a.sets.split(",")):
        t = ref_params.plaintext_modulus(n)
        moduli = ref_params.DEFAULT_128[n]
        L = len(moduli)
        par = fhe.BfvParameters(n, t, moduli=moduli)
        ctx = par.context_at_level(0)
        sk = fhe.SecretKey.random(par, bytes(range(32)))
        rng = np.random.default_rng(n)
        seeds = torch.from_numpy(rng.integers(0, 256, size=(EK_KEYS, 32), dtype=np.uint8)).cuda()
        exps = [pow(3, i, 2 * n) for i in range(1, EK_KEYS + 1)]
        gen = [g.ksk for g in fhe.GaloisKey.generate(sk, exps, seeds)]
        wire = [k.to_wire(seeded=False) for k in gen]
        c0b, c1b = torch.stack([w[0] for w in wire]), torch.stack([w[1] for w in wire])   # [keys, ndigits, size]
        K = [k.seed for k in gen]
        Kd = torch.from_numpy(np.frombuffer(b"".join(K), dtype=np.uint8).reshape(EK_KEYS, 32).copy()).cuda()
        # the piecewise route restates generate_c1 on the host: the digit seeds, prepared once, outside the timed windows
        dseeds = [torch.from_numpy(np.frombuffer(b"".join(keygen_ref.digit_seeds(k, L)), dtype=np.uint8)
                                   .reshape(L, 32).copy()).cuda() for k in K]
        # the loaded keys are the generated ones (results must not change): checked once per set
        for key, ref in zip(fhe.KeySwitchingKey.from_wire(ctx, ctx, c0b, seeds=Kd), gen):
            for x, y in zip(key.export(), ref.export()):
                assert torch.equal(x, y)
        polys = torch.zeros((1024, L, n), dtype=torch.int64, device="cuda")
        ntt_ms = alternating_ms({"ntt": lambda: ctx.ntt_forward(polys)}, a.window)["ntt"][0]
        rows_per_s = 1024 * L / ntt_ms * 1e3
        f64_words = all(q < (1 << 50) for q in moduli)

        def alloc6():
            for b in [fhe.DeviceArray((L, L, n)) for _ in range(6 if f64_words else 4)]:
                b.free()
        alloc_ms = alternating_ms({"alloc": alloc6}, a.window)["alloc"][0]
        for keys in (1, EK_KEYS):
            for seeded in (True, False):
                b0, b1 = c0b[:keys].contiguous(), c1b[:keys].contiguous()

                def load():
                    if seeded:
                        return fhe.KeySwitchingKey.from_wire(ctx, ctx, b0, seeds=Kd[:keys])
                    return fhe.KeySwitchingKey.from_wire(ctx, ctx, b0, b1)

                def today():
                    out = []
                    for b in range(keys):
                        c0 = ctx.deserialize(b0[b], to_ntt=True)
                        c1 = ctx.random_from_seed(dseeds[b]) if seeded else ctx.deserialize(b1[b], to_ntt=True)
                        out.append(fhe.KeySwitchingKey(ctx, ctx, c0, c1))
                    return out
                ms = alternating_ms({"load_wire": load, "today": today}, a.window)
                rows_per_key = L * L * (1 if seeded else 2)
                for route in ("load_wire", "today"):
                    med, lo, hi = ms[route]
                    row = dict(n=n, moduli=L, ndigits=L, keys=keys, seeded=seeded, route=route, ms=round(med, 4),
                               ms_low=round(lo, 4), ms_high=round(hi, 4), keys_per_s=round(keys / med * 1e3, 1),
                               ntt_rows_yardstick_keys_per_s=round(rows_per_s / rows_per_key, 1),
                               alloc6_ms_per_key=round(alloc_ms, 4), alloc_share=round(alloc_ms * keys / med, 3))
                    print(json.dumps(row), flush=True)
                    lines.append(row)
        fhe.workspace_trim()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
