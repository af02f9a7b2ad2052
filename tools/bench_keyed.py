#!/usr/bin/env python3
"""Keyed batches (one key per client, fhe_*_keyed_dev) against what a server does without them, on two shapes -- N = 8192
over 4 x 60-bit moduli and the reference's stock n = 8192 set (tests/ref_params.py) -- with the F64 option on and off:
`relinearize` and `rotate_columns` (exponent 3) over 1,024 ciphertexts in total, split as nkeys in {1, 16, 64, 256, 1024}
clients.  Three routes per row, timed in one process, their windows alternating:
  keyed    one keyed call over the whole batch (fhe_bfv_relinearize_keyed_dev / fhe_bfv_galois_keyed_dev)
  loop     nkeys single-key calls of batch / nkeys on one stream: what a server does today
  single   ONE single-key call over all 1,024 under the first key: a floor no keyed call can beat (other values: it is
           not a route a server with many clients could take)
All three go through the raw ABI on preallocated buffers, so the loop pays one foreign call per client and nothing else.
Timing: wall clock around enough calls to fill `--window` seconds after a warm-up call per route, the device synchronised
before and after; the median of `--windows` (at least three) windows with the lowest and highest next to it.
Stage B alone: one more keyed call per row under the engine's profiler (outside the timed windows) gives the kernel time
of ks_mac_keyed_kernel; with the bytes it has to move -- every key's c0 and c1 words once, W, the own Ntt rows, the
addends and both outputs, computed from the shapes below -- that is a rate, reported as a fraction of fhe_ubench_copy's
streaming rate in the same process.  One JSON line per row on stdout and in --out (default profiles/keyed_bench.jsonl)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import fhe_rs_amd as fhe  # noqa: E402
from fhe_rs_amd import _lib  # noqa: E402
from fhe_rs_amd.api import _stream  # noqa: E402

NKEYS = (1, 16, 64, 256, 1024)
EXPONENT = 3


def sync():
    _lib.check(_lib.lib().fhe_device_sync(0))


def alternating_ms(fns, window_s, windows):
    """{name: (median, low, high) ms per call} of the callables, their windows alternating; each window holds enough
    calls to last `window_s`."""
    reps = {}
    for name, fn in fns.items():
        fn()
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        reps[name] = max(1, int(window_s / max(time.perf_counter() - t0, 1e-6)))
    out = {name: [] for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            sync()
            t0 = time.perf_counter()
            for _ in range(reps[name]):
                fn()
            sync()
            out[name].append((time.perf_counter() - t0) * 1e3 / reps[name])
    return {name: (statistics.median(v), min(v), max(v)) for name, v in out.items()}


def stage_b_bytes(op, total, nkeys, L, n):
    """Bytes ks_mac_keyed_kernel moves for `total` polynomials under `nkeys` keys at the ciphertext's level (L digits,
    L key moduli): every key's c0 and c1 once, the W rows (all but the own rows, which are read from the caller's Ntt
    polynomial), the addends (c0 and c1 for a relinearization, c0 for a rotation) and both outputs."""
    row = n * 8
    keys = nkeys * 2 * L * L * row
    w = total * (L * L - L) * row
    own = total * L * row
    addends = total * (2 if op == "relinearize" else 1) * L * row
    outputs = total * 2 * L * row
    return keys + w + own + addends + outputs


def stage_b_ms(call):
    """Kernel time of the ks_mac_keyed launches inside call(), from the engine's profiler."""
    fhe.prof_reset()
    fhe.prof_enable(True)
    try:
        call()
        sync()
    finally:
        fhe.prof_enable(False)
    ms = sum(t for label, _, launches, t in fhe.prof_entries() if label == "ks_mac_keyed" and launches)
    fhe.prof_reset()
    return ms


def run(shapes, total, nkeys_list, window_s, windows, copy_bytes=1 << 30, emit=print):
    """The rows of the module docstring for shapes = [(name, moduli, n)]."""
    L_ = _lib.lib()
    rows = []
    copy_rate = fhe.ubench_copy(copy_bytes, 0.2)
    for name, moduli, n in shapes:
        ctx = fhe.Context(list(moduli), n)
        L = len(moduli)
        pl = L * n * 8                                   # bytes of one polynomial
        kw = ctx.synth_uniform(0x4B455944, 0, 0, 2 * L, max(nkeys_list))    # [keys, 2 * L, L, N]: c0 and c1 digit rows
        keys = []
        for c in range(max(nkeys_list)):
            k = kw[c].reshape(2, L, L, n)
            keys.append(fhe.KeySwitchingKey(ctx, ctx, k[0], k[1]))
        del kw
        ct3 = ctx.synth_uniform(0x4B455945, 0, 0, 3, total)
        ct2 = ctx.synth_uniform(0x4B455946, 0, 0, 2, total)
        out = ctx.synth_uniform(0x4B455947, 0, 0, 2, total)
        p3, p2, po = ct3.data_ptr(), ct2.data_ptr(), out.data_ptr()
        vp = C.c_void_p
        for f64 in (True, False):
            fhe.set_f64(f64)
            try:
                for op in ("relinearize", "rotate_columns"):
                    for nkeys in nkeys_list:
                        m = total // nkeys
                        ks = fhe.KeySet(keys[:nkeys])
                        hs = [k._h for k in keys[:nkeys]]
                        st = _stream()
                        if op == "relinearize":
                            keyed = lambda: L_.fhe_bfv_relinearize_keyed_dev(ks._h, vp(p3), vp(po), total, st)   # noqa: E731
                            single = lambda: L_.fhe_bfv_relinearize_dev(hs[0], vp(p3), vp(po), total, st)       # noqa: E731

                            def loop():
                                r = 0
                                for c in range(nkeys):
                                    r |= L_.fhe_bfv_relinearize_dev(hs[c], vp(p3 + c * m * 3 * pl), vp(po + c * m * 2 * pl), m, st)
                                return r
                        else:
                            keyed = lambda: L_.fhe_bfv_galois_keyed_dev(ks._h, EXPONENT, vp(p2), vp(po), total, st)   # noqa: E731
                            single = lambda: L_.fhe_bfv_galois_dev(hs[0], EXPONENT, vp(p2), vp(po), total, st)       # noqa: E731

                            def loop():
                                r = 0
                                for c in range(nkeys):
                                    r |= L_.fhe_bfv_galois_dev(hs[c], EXPONENT, vp(p2 + c * m * 2 * pl), vp(po + c * m * 2 * pl), m, st)
                                return r
                        for fn in (keyed, loop, single):
                            _lib.check(fn())
                        ms = alternating_ms({"keyed": keyed, "loop": loop, "single": single}, window_s, windows)
                        b_ms = stage_b_ms(keyed)
                        b_bytes = stage_b_bytes(op, total, nkeys, L, n)
                        rate = b_bytes / (b_ms * 1e-3) if b_ms > 0 else 0.0
                        row = dict(shape=name, n=n, moduli=L, f64=f64, op=op, total=total, nkeys=nkeys, per_key=m)
                        for route in ("keyed", "loop", "single"):
                            med, lo, hi = ms[route]
                            row[route + "_ms"] = round(med, 4)
                            row[route + "_ms_low"] = round(lo, 4)
                            row[route + "_ms_high"] = round(hi, 4)
                        row.update(loop_over_keyed=round(ms["loop"][0] / ms["keyed"][0], 2),
                                   keyed_over_single=round(ms["keyed"][0] / ms["single"][0], 2),
                                   stage_b_ms=round(b_ms, 4), stage_b_bytes=b_bytes, stage_b_gb_per_s=round(rate / 1e9, 1),
                                   copy_gb_per_s=round(copy_rate / 1e9, 1),
                                   stage_b_fraction_of_copy=round(rate / copy_rate, 3) if copy_rate else None)
                        emit(json.dumps(row))
                        rows.append(row)
                        del ks
            finally:
                fhe.set_f64(True)
        del keys, ct3, ct2, out
        fhe.workspace_trim()
    return rows


def main():
    import ref_params
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.15)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--total", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyed_bench.jsonl"))
    a = ap.parse_args()
    if a.windows < 3:
        sys.exit("at least three windows")
    _lib.lib()
    if not _lib.loaded_path().endswith("libfhe_hip.so") or fhe.device_count() < 1:
        sys.exit("bench_keyed needs the HIP build and a GPU")
    shapes = [("n8192_4x60", fhe.generate_moduli([60] * 4, 8192), 8192), ("stock_n8192", ref_params.DEFAULT_128[8192], 8192)]
    rows = run(shapes, a.total, [k for k in NKEYS if k <= a.total], a.window, a.windows, emit=lambda s: print(s, flush=True))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
