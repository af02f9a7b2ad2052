#!/usr/bin/env python3
"""Hoisted rotations (fhe_bfv_galois_hoisted_dev: R Galois elements of each ciphertext on one digit decomposition) against
what a caller does without them, a loop of R fhe_bfv_galois_dev calls on the same keys, on four shapes -- N = 8192 over
4 x 60-bit moduli, the reference's stock n = 8192 set with the F64 option on and off, and its stock n = 16384 set
(tests/ref_params.py) -- for R in {1, 4, 16, 64} rotations of batch in {1, 16, 256} ciphertexts (rows whose output would
not fit --max-out-gib are left out).  Both routes go through the raw ABI on preallocated buffers (the single call has no
strided output: with batch > 1 the loop writes each rotation's [batch] block to one scratch block, as a caller that
consumes it at once would); they are timed in one process, their windows alternating (tools/bench_keyed.py's method): wall clock
around enough calls to fill `--window` seconds after a warm-up call per route, the device synchronised before and after;
the median of `--windows` (at least three) windows with the lowest and highest next to it.
Stage B alone: one more hoisted call per row under the engine's profiler (outside the timed windows) gives the kernel time
of hoist_mac_kernel and of its stage A; with the bytes stage B has to move -- every key's c0 and c1 words once, R times W
and the own Ntt rows, the addends and both outputs per rotation, computed from the shapes below -- that is a rate, reported
as a fraction of fhe_ubench_copy's streaming rate in the same process.  One JSON line per row on stdout and in --out
(default profiles/hoisted_bench.jsonl)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import fhe_rs_amd as fhe  # noqa: E402
from fhe_rs_amd import _lib  # noqa: E402
from fhe_rs_amd.api import _stream  # noqa: E402
from bench_keyed import alternating_ms, sync  # noqa: E402

ROTATIONS = (1, 4, 16, 64)
BATCHES = (1, 16, 256)


def stage_b_bytes(batch, nrot, L, n):
    """Bytes hoist_mac_kernel moves for `batch` ciphertexts x `nrot` rotations at the ciphertext's level (L digits, L key
    moduli): every key's c0 and c1 once, and per rotation the W rows (all but the own rows), the own Ntt rows, the addend
    c0 and both outputs."""
    row = n * 8
    keys = nrot * 2 * L * L * row
    w = batch * nrot * (L * L - L) * row
    own = batch * nrot * L * row
    addends = batch * nrot * L * row
    outputs = batch * nrot * 2 * L * row
    return keys + w + own + addends + outputs


def profiled_ms(call):
    """(stage B, stage A, inverse transform) kernel ms inside call(), from the engine's profiler (the second of two
    profiled calls: a kernel's first profiled launch carries one-time costs)."""
    fhe.prof_enable(True)
    try:
        call()
        sync()
        fhe.prof_reset()
        call()
        sync()
    finally:
        fhe.prof_enable(False)
    b = a = other = 0.0
    for label, _, launches, t in fhe.prof_entries():
        if not launches:
            continue
        if label == "hoist_mac":
            b += t
        elif label.startswith("ks_digit_ntt"):
            a += t
        else:
            other += t
    fhe.prof_reset()
    return b, a, other


def run(shapes, rotations, batches, window_s, windows, max_out_bytes, copy_bytes=1 << 30, emit=print):
    """The rows of the module docstring for shapes = [(name, moduli, n, f64)]."""
    L_ = _lib.lib()
    vp = C.c_void_p
    rows = []
    copy_rate = fhe.ubench_copy(copy_bytes, 0.2)
    for name, moduli, n, f64 in shapes:
        fhe.set_f64(f64)
        try:
            ctx = fhe.Context(list(moduli), n)
            L = len(moduli)
            pl = L * n * 8                                   # bytes of one polynomial
            rmax = max(rotations)
            keys = []
            for c in range(rmax):                            # (one key at a time: the key words are the large operand)
                k = ctx.synth_uniform(0x484F4953 + c, 0, 0, 2 * L, 1).reshape(2, L, L, n)
                keys.append(fhe.KeySwitchingKey(ctx, ctx, k[0], k[1]))
                del k
            exps = [pow(3, r + 1, 2 * n) for r in range(rmax)]
            for batch in batches:
                fit = [r for r in rotations if batch * r * 2 * pl <= max_out_bytes]
                if not fit:
                    continue
                ct = ctx.synth_uniform(0x484F4954, 0, 0, 2, batch)
                out = ctx.synth_uniform(0x484F4955, 0, 0, 2, batch * max(fit))
                pc, po = ct.data_ptr(), out.data_ptr()
                for nrot in fit:
                    ks = fhe.KeySet(keys[:nrot])
                    hs = [k._h for k in keys[:nrot]]
                    ex = (C.c_size_t * nrot)(*exps[:nrot])
                    st = _stream()
                    hoisted = lambda: L_.fhe_bfv_galois_hoisted_dev(ks._h, ex, nrot, vp(pc), vp(po), batch, st)   # noqa: E731
                    tmp = ctx.synth_uniform(0x484F4956, 0, 0, 2, batch) if nrot > 1 else out
                    pt = tmp.data_ptr()

                    def loop():
                        # (the single call writes [batch] ciphertexts per rotation: rotation r of every ciphertext lands in
                        # its own block; with batch == 1 that IS the hoisted layout)
                        r_ = 0
                        for r in range(nrot):
                            dst = po + r * 2 * pl if batch == 1 else pt
                            r_ |= L_.fhe_bfv_galois_dev(hs[r], exps[r], vp(pc), vp(dst), batch, st)
                        return r_
                    for fn in (hoisted, loop):
                        _lib.check(fn())
                    ms = alternating_ms({"hoisted": hoisted, "loop": loop}, window_s, windows)
                    b_ms, a_ms, other_ms = profiled_ms(hoisted)
                    b_bytes = stage_b_bytes(batch, nrot, L, n)
                    rate = b_bytes / (b_ms * 1e-3) if b_ms > 0 else 0.0
                    row = dict(shape=name, n=n, moduli=L, f64=f64, batch=batch, rotations=nrot)
                    for route in ("hoisted", "loop"):
                        med, lo, hi = ms[route]
                        row[route + "_ms"] = round(med, 4)
                        row[route + "_ms_low"] = round(lo, 4)
                        row[route + "_ms_high"] = round(hi, 4)
                    row.update(loop_over_hoisted=round(ms["loop"][0] / ms["hoisted"][0], 2),
                               stage_b_ms=round(b_ms, 4), stage_a_ms=round(a_ms, 4), inverse_ntt_ms=round(other_ms, 4),
                               stage_b_bytes=b_bytes, stage_b_gb_per_s=round(rate / 1e9, 1), copy_gb_per_s=round(copy_rate / 1e9, 1),
                               stage_b_fraction_of_copy=round(rate / copy_rate, 3) if copy_rate else None)
                    emit(json.dumps(row))
                    rows.append(row)
                    del ks, tmp
                del ct, out
                fhe.workspace_trim()
            del keys
        finally:
            fhe.set_f64(True)
    return rows


def main():
    import ref_params
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.15)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--max-out-gib", type=float, default=16.0)
    ap.add_argument("--rotations", type=int, nargs="+", default=list(ROTATIONS))
    ap.add_argument("--batches", type=int, nargs="+", default=list(BATCHES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hoisted_bench.jsonl"))
    a = ap.parse_args()
    if a.windows < 3:
        sys.exit("at least three windows")
    _lib.lib()
    if not _lib.loaded_path().endswith("libfhe_hip.so") or fhe.device_count() < 1:
        sys.exit("bench_hoisted needs the HIP build and a GPU")
    shapes = [("n8192_4x60", fhe.generate_moduli([60] * 4, 8192), 8192, True),
              ("stock_n8192", ref_params.DEFAULT_128[8192], 8192, True),
              ("stock_n8192", ref_params.DEFAULT_128[8192], 8192, False),
              ("stock_n16384", ref_params.DEFAULT_128[16384], 16384, True)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def emit(s):
            print(s, flush=True)
            f.write(s + "\n")
            f.flush()
        run(shapes, tuple(a.rotations), tuple(a.batches), a.window, a.windows, int(a.max_out_gib * (1 << 30)), emit=emit)


if __name__ == "__main__":
    main()
