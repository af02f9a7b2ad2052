#!/usr/bin/env python3
"""Plaintexts from packed bits on the device against the resident-values encode and against the host route, on the
reference's stock sets n = 4096 / 8192 (tests/ref_params.py) and on the PIR examples' set (n = 4096, t = 2056193, moduli
of 36, 36 and 37 bits), 1,024 plaintexts per call at level 0, unscaled:
  encode_bytes    Encoder.encode_bytes (fhe_bfv_encode_bytes_dev) of resident bytes, items of floor(N nbits / 8) bytes
  encode_words    Encoder.encode_words (fhe_bfv_encode_words_dev) of resident words [batch][2][N] carrying bits(q_0) each
                  (the fold: c0 and c1 of a ciphertext at its last level), batch = 1,024 / nplain
  encode_values   the yardstick: Encoder.encode (fhe_bfv_encode_dev, Poly) of resident u64 values [1024][N] -- the same
                  transform behind a loader that reads 8 bytes per coefficient
  today           the host route for the same bytes as encode_bytes: numpy unpack to u64, upload, fhe_bfv_encode_dev
Plaintexts per second from wall-clock windows that alternate in one process (after one warm-up call per route, the device
synchronised before and after), median of three with the lowest and highest next to it.  On every device record also the
profiled time of its transform kernel (the engine's launch events, one profiled call) and `copy_fraction`: the bytes that
kernel must move (source + output) over that time, as a fraction of fhe_ubench_copy of the same byte count in this
process.  One JSON line per record on stdout and in --out (default profiles/transcode_bench.jsonl)."""
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

PLAINTEXTS = 1024


def alternating_ms(fns, window_s):
    """{name: (median, low, high) ms per call} of the callables, their windows alternating."""
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


def numpy_unpack(raw, item_bytes, nbits):
    """transcode_from_bytes of every item with numpy: uint8 [batch * item_bytes] -> uint64 [batch][M]."""
    m = item_bytes * 8 // nbits
    items = raw.reshape(-1, item_bytes)
    w = np.uint64(1) << np.arange(nbits, dtype=np.uint64)
    out = np.empty((items.shape[0], m), dtype=np.uint64)
    for i in range(0, items.shape[0], 64):     # (64 items at a time: the unpacked bits are 64 times the bytes)
        bits = np.unpackbits(items[i:i + 64], axis=1, bitorder="little")[:, :m * nbits]
        out[i:i + 64] = (bits.reshape(-1, m, nbits).astype(np.uint64) * w).sum(axis=2, dtype=np.uint64)
    return out


def profiled_ms(fn, labels):
    fhe.prof_reset()
    fhe.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        rep = fhe.prof_report()
    finally:
        fhe.prof_enable(False)
        fhe.prof_reset()
    return sum(ms for label, (_n, ms) in rep.items() if label in labels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="4096,8192,pir")
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transcode_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_transcode needs a GPU")
    lines = []
    for name in a.sets.split(","):
        if name == "pir":
            n, t = 4096, 2056193
            par = fhe.BfvParameters(n, t, moduli_sizes=[36, 36, 37])
        else:
            n = int(name)
            t = ref_params.plaintext_modulus(n)
            par = fhe.BfvParameters(n, t, moduli=ref_params.DEFAULT_128[n])
        L = len(par.moduli)
        nbits = t.bit_length() - 1
        qbits = int(par.moduli[0]).bit_length()
        enc = par.encoder()
        rng = np.random.default_rng(n)
        item_bytes = n * nbits // 8
        m = item_bytes * 8 // nbits
        raw = rng.integers(0, 256, size=PLAINTEXTS * item_bytes, dtype=np.uint8)
        d_raw = torch.from_numpy(raw).cuda()
        vals = numpy_unpack(raw, item_bytes, nbits)
        d_vals = torch.from_numpy(vals.view(np.int64)).cuda()
        nplain = -(-2 * -(-n * qbits // nbits) // n)
        wb = PLAINTEXTS // nplain
        d_words = torch.from_numpy(rng.integers(0, 1 << qbits, size=(wb, 2, n), dtype=np.uint64).view(np.int64)).cuda()
        # the three device routes agree where they overlap (results must not differ): checked once per set
        assert torch.equal(enc.encode_bytes(d_raw, item_bytes), enc.encode(d_vals, "poly"))

        def today():
            v = numpy_unpack(raw, item_bytes, nbits)
            return enc.encode(torch.from_numpy(v.view(np.int64)).cuda(), "poly")
        fns = {"encode_bytes": lambda: enc.encode_bytes(d_raw, item_bytes),
               "encode_words": lambda: enc.encode_words(d_words, qbits),
               "encode_values": lambda: enc.encode(d_vals, "poly"),
               "today": today}
        ms = alternating_ms(fns, a.window)
        src_bytes = {"encode_bytes": raw.nbytes, "encode_words": wb * 2 * n * 8, "encode_values": PLAINTEXTS * m * 8}
        plaintexts = {"encode_words": wb * nplain}
        for route in fns:
            med, lo, hi = ms[route]
            np_ = plaintexts.get(route, PLAINTEXTS)
            row = dict(set=name, n=n, moduli=L, nbits=nbits, route=route, plaintexts=np_, ms=round(med, 4),
                       ms_low=round(lo, 4), ms_high=round(hi, 4), plaintexts_per_s=round(np_ / med * 1e3, 1))
            if route in src_bytes:
                kms = profiled_ms(fns[route], ("encode_stream", "encode_lift"))
                moved = src_bytes[route] + np_ * L * n * 8
                copy = fhe.ubench_copy(moved // 2)    # (it reads and writes nbytes: the same total)
                row.update(kernel_ms=round(kms, 4), kernel_bytes=moved,
                           copy_fraction=round(moved / (kms * 1e-3) / copy, 3) if kms else None)
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
