#!/usr/bin/env python3
"""Hoisted rotations and the hoisted matrix-vector product with one Galois key set per client
(fhe_bfv_galois_hoisted_keyed_dev, fhe_bfv_matvec_hoisted_keyed_dev) against what a server does without them, on N = 8192
over 4 x 60-bit moduli and the reference's stock n = 8192 set with the F64 option on and off: a fixed total of 256
ciphertexts split over nclients in {1, 16, 64} clients (synthetic keys through fhe_ksk_create_dev), R in {4, 16}
rotations, `rotate` and `matvec` with diagonals shared by the batch.  Three routes per cell, through the raw ABI on
preallocated buffers, timed in one process, their windows alternating (tools/bench_keyed.py's method), the median of
`--windows` (at least three) with the lowest and highest next to it:
  keyed    (a) one keyed call over the whole batch
  loop     (b) nclients single-client calls of 256 / nclients ciphertexts on one stream: what a server does today
  single   (c) ONE unkeyed call over all 256 ciphertexts under the first client's keys: the floor (other values: not a
           route a server with many clients could take); at nclients = 1 it is the same work as (a) in the other block
           order of hoist_mac_kernel (ciphertext fastest) -- the measurement of hoist_mac_keyed_kernel's rotation-fastest grid.
Stage B alone: one more keyed call per cell under the engine's profiler (outside the timed windows) gives the kernel time
of hoist_mac_keyed_kernel / hoist_matvec_keyed_kernel (+ the summing kernel); with the bytes it has to move -- every key's
c0 and c1 words once, R times W, the own Ntt rows and the addends, the diagonals once per ciphertext, the outputs -- that is
a rate, reported as a fraction of fhe_ubench_copy's streaming rate in the same process.
One JSON line per cell on stdout and in --out (default profiles/hoisted_keyed_bench.jsonl)."""
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

TOTAL = 256
NCLIENTS = (1, 16, 64)
ROTATIONS = (4, 16)


def stage_b_bytes(op, total, nclients, nrot, L, n):
    """Bytes the keyed stage B moves for `total` ciphertexts of `nclients` clients at the ciphertext's level (L digits, L
    key moduli), one rotation group."""
    row = n * 8
    keys = nclients * nrot * 2 * L * L * row
    w = total * nrot * (L * L - L) * row
    own = total * nrot * L * row
    addends = total * nrot * L * row
    if op == "rotate":
        return keys + w + own + addends + total * nrot * 2 * L * row
    return keys + w + own + addends + total * nrot * L * row + total * 2 * L * row


def stage_b_ms(call):
    """(stage B ms incl. the summing kernel, whether it ran) of the second of two profiled calls."""
    fhe.prof_enable(True)
    try:
        _lib.check(call())
        sync()
        fhe.prof_reset()
        _lib.check(call())
        sync()
    finally:
        fhe.prof_enable(False)
    ms, summed = 0.0, False
    for label, _, launches, t in fhe.prof_entries():
        if launches and label in ("hoist_mac_keyed", "hoist_matvec_keyed", "mbfv_sum"):
            ms += t
            summed = summed or label == "mbfv_sum"
    fhe.prof_reset()
    return ms, summed


def run(shapes, nclients_list, rotations, total, window_s, windows, copy_bytes=1 << 30, emit=print):
    L_ = _lib.lib()
    vp = C.c_void_p
    rows = []
    copy_rate = fhe.ubench_copy(copy_bytes, 0.2)
    cmax, rmax = max(nclients_list), max(rotations)
    for name, moduli, n, f64 in shapes:
        fhe.set_f64(f64)
        try:
            ctx = fhe.Context(list(moduli), n)
            L = len(moduli)
            pl = L * n * 8                                   # bytes of one polynomial
            keys = []                                        # client c's key for rotation r at c * rmax + r
            for i in range(cmax * rmax):
                k = ctx.synth_uniform(0x484B0000 + i, 0, 0, 2 * L, 1).reshape(2, L, L, n)
                keys.append(fhe.KeySwitchingKey(ctx, ctx, k[0], k[1]))
                del k
            exps = [pow(3, r + 1, 2 * n) for r in range(rmax)]
            pts = ctx.synth_uniform(0x484B4957, 0, 0, 1, rmax)
            ct = ctx.synth_uniform(0x484B4954, 0, 0, 2, total)
            out = ctx.synth_uniform(0x484B4955, 0, 0, 2, total * rmax)
            pp, pc, po = pts.data_ptr(), ct.data_ptr(), out.data_ptr()
            st = _stream()
            for nclients in nclients_list:
                m = total // nclients
                for nrot in rotations:
                    ex = (C.c_size_t * nrot)(*exps[:nrot])
                    singles = [fhe.KeySet(keys[c * rmax:c * rmax + nrot]) for c in range(nclients)]
                    keyed = fhe.KeySet([keys[c * rmax + r] for c in range(nclients) for r in range(nrot)])
                    for op in ("rotate", "matvec"):
                        oitem = (nrot if op == "rotate" else 1) * 2 * pl      # bytes of one item's output

                        def one(ks, c0, count):
                            if op == "rotate":
                                return L_.fhe_bfv_galois_hoisted_dev(ks._h, ex, nrot, vp(pc + c0 * 2 * pl), vp(po + c0 * oitem), count, st)
                            return L_.fhe_bfv_matvec_hoisted_dev(ks._h, ex, nrot, vp(pc + c0 * 2 * pl), vp(pp), 1, None,
                                                                 vp(po + c0 * oitem), count, st)

                        def call_keyed():
                            if op == "rotate":
                                return L_.fhe_bfv_galois_hoisted_keyed_dev(keyed._h, nclients, ex, nrot, vp(pc), vp(po), total, st)
                            return L_.fhe_bfv_matvec_hoisted_keyed_dev(keyed._h, nclients, ex, nrot, vp(pc), vp(pp), 1, None, vp(po),
                                                                       total, st)

                        def call_loop():
                            r_ = 0
                            for c in range(nclients):
                                r_ |= one(singles[c], c * m, m)
                            return r_

                        def call_single():
                            return one(singles[0], 0, total)
                        routes = {"keyed": call_keyed, "loop": call_loop, "single": call_single}
                        for fn in routes.values():
                            _lib.check(fn())
                        ms = alternating_ms(routes, window_s, windows)
                        row = dict(shape=name, n=n, moduli=L, f64=f64, op=op, total=total, nclients=nclients, per_client=m,
                                   rotations=nrot)
                        for route in routes:
                            med, lo, hi = ms[route]
                            row[route + "_ms"] = round(med, 4)
                            row[route + "_ms_low"] = round(lo, 4)
                            row[route + "_ms_high"] = round(hi, 4)
                        row["loop_over_keyed"] = round(ms["loop"][0] / ms["keyed"][0], 2)
                        row["keyed_over_single"] = round(ms["keyed"][0] / ms["single"][0], 2)
                        b_ms, summed = stage_b_ms(call_keyed)
                        b_bytes = stage_b_bytes(op, total, nclients, nrot, L, n)
                        rate = b_bytes / (b_ms * 1e-3) if b_ms > 0 else 0.0
                        row.update(keyed_stage_b_ms=round(b_ms, 4), keyed_partial_sums=summed, keyed_stage_b_bytes=b_bytes,
                                   keyed_stage_b_gb_per_s=round(rate / 1e9, 1),
                                   keyed_stage_b_fraction_of_copy=round(rate / copy_rate, 3) if copy_rate else None,
                                   copy_gb_per_s=round(copy_rate / 1e9, 1))
                        emit(json.dumps(row))
                        rows.append(row)
                    del singles, keyed
                    fhe.workspace_trim()
            del keys, pts, ct, out
        finally:
            fhe.set_f64(True)
    return rows


def main():
    import ref_params
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.15)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--nclients", type=int, nargs="+", default=list(NCLIENTS))
    ap.add_argument("--rotations", type=int, nargs="+", default=list(ROTATIONS))
    ap.add_argument("--total", type=int, default=TOTAL)
    ap.add_argument("--shapes", nargs="+", default=None, help="names of the shapes to run (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hoisted_keyed_bench.jsonl"))
    a = ap.parse_args()
    if a.windows < 3:
        sys.exit("at least three windows")
    if any(c < 1 or a.total % c for c in a.nclients):
        sys.exit("every client count divides the total")
    _lib.lib()
    if not _lib.loaded_path().endswith("libfhe_hip.so") or fhe.device_count() < 1:
        sys.exit("bench_hoisted_keyed needs the HIP build and a GPU")
    shapes = [("n8192_4x60", fhe.generate_moduli([60] * 4, 8192), 8192, True),
              ("stock_n8192", ref_params.DEFAULT_128[8192], 8192, True),
              ("stock_n8192", ref_params.DEFAULT_128[8192], 8192, False)]
    if a.shapes:
        shapes = [s for s in shapes if s[0] in a.shapes]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def emit(s):
            print(s, flush=True)
            f.write(s + "\n")
            f.flush()
        run(shapes, tuple(a.nclients), tuple(a.rotations), a.total, a.window, a.windows, emit=emit)


if __name__ == "__main__":
    main()
