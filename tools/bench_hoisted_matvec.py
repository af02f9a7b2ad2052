#!/usr/bin/env python3
"""Hoisted matrix-vector product (fhe_bfv_matvec_hoisted_dev: the rotations, the products with the diagonals and their sum
in one stage B) against the composition it replaces -- fhe_bfv_galois_hoisted_dev into a [batch][R] block of rotated
ciphertexts, then fhe_bfv_dot_product_scalar_dev over that block (the yardstick) -- on tools/bench_hoisted.py's shapes and
batches for R in {4, 16, 64} diagonals shared by the batch.  Three routes per cell, through the raw ABI on preallocated
buffers: the fused call at the engine's rotation-group rule, the fused call with rot_split = 1, and the composition (left
out, and said so, where its intermediate block exceeds --max-out-gib).  They are timed in one process, their windows
alternating (tools/bench_keyed.py's method), the median of `--windows` (at least three) with the lowest and highest next
to it.
Stage B alone: one more fused call per route under the engine's profiler (outside the timed windows) gives the kernel
time of hoist_matvec_kernel (+ the summing kernel); with the bytes it has to move -- every key's c0 and c1 words once, R
times W, the own Ntt rows and the addends, the diagonals once per ciphertext, one output, and the partial sums written
and read where the rotations are cut into groups -- that is a rate, reported as a fraction of fhe_ubench_copy's streaming
rate in the same process.
Memory of a route: the caller's buffers it needs (inputs, diagonals, output, and the composition's intermediate block) plus
the scratch the engine holds after one call from a trimmed workspace.
One JSON line per cell on stdout and in --out (default profiles/hoisted_matvec_bench.jsonl)."""
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

ROTATIONS = (4, 16, 64)
BATCHES = (1, 16, 256)


def stage_b_bytes(batch, nrot, L, n, groups):
    """Bytes the fused stage B moves at the ciphertext's level (L digits, L key moduli) with `groups` partial sums per
    ciphertext (1: the result itself)."""
    row = n * 8
    keys = nrot * 2 * L * L * row
    w = batch * nrot * (L * L - L) * row
    own = batch * nrot * L * row
    addends = batch * nrot * L * row
    diagonals = batch * nrot * L * row
    outputs = batch * 2 * L * row
    partial = 2 * groups * outputs if groups > 1 else 0      # written by the groups, read by the summing kernel
    return keys + w + own + addends + diagonals + outputs + partial


def profiled(call):
    """(stage B ms incl. the summing kernel, stage A ms, other ms, partial sums) inside call(): the second of two profiled
    calls."""
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
    summed = False
    for label, _, launches, t in fhe.prof_entries():
        if not launches:
            continue
        if label in ("hoist_matvec", "mbfv_sum"):
            b += t
            summed = summed or label == "mbfv_sum"
        elif label.startswith("ks_digit_ntt"):
            a += t
        else:
            other += t
    fhe.prof_reset()
    return b, a, other, summed


def scratch_after(call):
    fhe.workspace_trim()
    _lib.check(call())
    sync()
    held = fhe.workspace_stats()["held_bytes"]
    return held


def device_cus():
    try:
        import torch
        return int(torch.cuda.get_device_properties(0).multi_processor_count)
    except Exception:
        return None


def rule_groups(cus, batch, L, n, nrot):
    """The engine's rule (engine.hpp: hoist_rot_group), restated for the record: groups of one launch at the default W
    budget (one chunk, one key-modulus group).  None when the compute units are unknown."""
    if not cus:
        return None
    blocks = batch * L * max(n // 512, 1)
    nr = min(nrot, 64)
    groups = 1 if blocks >= 2 * cus else min(-(-2 * cus // blocks), nr)
    return -(-nr // -(-nr // groups))


def run(shapes, rotations, batches, window_s, windows, max_out_bytes, copy_bytes=1 << 30, emit=print):
    L_ = _lib.lib()
    vp = C.c_void_p
    rows = []
    copy_rate = fhe.ubench_copy(copy_bytes, 0.2)
    cus = device_cus()
    for name, moduli, n, f64 in shapes:
        fhe.set_f64(f64)
        try:
            ctx = fhe.Context(list(moduli), n)
            L = len(moduli)
            pl = L * n * 8                                   # bytes of one polynomial
            rmax = max(rotations)
            keys = []
            for c in range(rmax):
                k = ctx.synth_uniform(0x484F4953 + c, 0, 0, 2 * L, 1).reshape(2, L, L, n)
                keys.append(fhe.KeySwitchingKey(ctx, ctx, k[0], k[1]))
                del k
            exps = [pow(3, r + 1, 2 * n) for r in range(rmax)]
            pts = ctx.synth_uniform(0x484F4957, 0, 0, 1, rmax)
            pp = pts.data_ptr()
            for batch in batches:
                ct = ctx.synth_uniform(0x484F4954, 0, 0, 2, batch)
                out = ctx.synth_uniform(0x484F4955, 0, 0, 2, batch)
                pc, po = ct.data_ptr(), out.data_ptr()
                for nrot in rotations:
                    ks = fhe.KeySet(keys[:nrot])
                    ex = (C.c_size_t * nrot)(*exps[:nrot])
                    st = _stream()
                    mid_bytes = batch * nrot * 2 * pl
                    composed_fits = mid_bytes <= max_out_bytes
                    mid = ctx.synth_uniform(0x484F4956, 0, 0, 2, batch * nrot) if composed_fits else None
                    pm = mid.data_ptr() if composed_fits else None

                    def fused(split):
                        def call():
                            L_.fhe_kskset_set_rot_split(ks._h, split)
                            return L_.fhe_bfv_matvec_hoisted_dev(ks._h, ex, nrot, vp(pc), vp(pp), 1, None, vp(po), batch, st)
                        return call

                    def composed():
                        r_ = L_.fhe_bfv_galois_hoisted_dev(ks._h, ex, nrot, vp(pc), vp(pm), batch, st)
                        return r_ | L_.fhe_bfv_dot_product_scalar_dev(ctx._h, 2, nrot, vp(pm), 0, vp(pp), 1, vp(po), batch, st)
                    routes = {"fused_rule": fused(0), "fused_one_group": fused(1)}
                    if composed_fits:
                        routes["composed"] = composed
                    for fn in routes.values():
                        _lib.check(fn())
                    ms = alternating_ms(routes, window_s, windows)
                    row = dict(shape=name, n=n, moduli=L, f64=f64, batch=batch, rotations=nrot,
                               rule_groups=rule_groups(cus, batch, L, n, nrot), composed_run=composed_fits)
                    for route in routes:
                        med, lo, hi = ms[route]
                        row[route + "_ms"] = round(med, 4)
                        row[route + "_ms_low"] = round(lo, 4)
                        row[route + "_ms_high"] = round(hi, 4)
                    if composed_fits:
                        row["composed_over_fused_rule"] = round(ms["composed"][0] / ms["fused_rule"][0], 2)
                        row["composed_over_fused_one_group"] = round(ms["composed"][0] / ms["fused_one_group"][0], 2)
                    row["one_group_over_rule"] = round(ms["fused_one_group"][0] / ms["fused_rule"][0], 2)
                    base = (2 * batch + nrot + 2 * batch) * pl        # ct, diagonals, out
                    for route, split in (("fused_rule", 0), ("fused_one_group", 1)):
                        b_ms, a_ms, other_ms, summed = profiled(routes[route])
                        groups = (row["rule_groups"] or 2) if (summed and split == 0) else 1
                        b_bytes = stage_b_bytes(batch, nrot, L, n, groups)
                        rate = b_bytes / (b_ms * 1e-3) if b_ms > 0 else 0.0
                        row.update({route + "_stage_b_ms": round(b_ms, 4), route + "_stage_a_ms": round(a_ms, 4),
                                    route + "_other_ms": round(other_ms, 4), route + "_partial_sums": summed,
                                    route + "_stage_b_bytes": b_bytes, route + "_stage_b_gb_per_s": round(rate / 1e9, 1),
                                    route + "_stage_b_fraction_of_copy": round(rate / copy_rate, 3) if copy_rate else None,
                                    route + "_buffer_bytes": base, route + "_scratch_bytes": scratch_after(routes[route])})
                    if composed_fits:
                        row.update(composed_buffer_bytes=base + mid_bytes, composed_scratch_bytes=scratch_after(composed))
                    else:
                        row.update(composed_buffer_bytes=base + mid_bytes, composed_scratch_bytes=None)
                    row["copy_gb_per_s"] = round(copy_rate / 1e9, 1)
                    emit(json.dumps(row))
                    rows.append(row)
                    del ks, mid
                    fhe.workspace_trim()
                del ct, out
            del keys, pts
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
    ap.add_argument("--shapes", nargs="+", default=None, help="names of the shapes to run (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hoisted_matvec_bench.jsonl"))
    a = ap.parse_args()
    if a.windows < 3:
        sys.exit("at least three windows")
    _lib.lib()
    if not _lib.loaded_path().endswith("libfhe_hip.so") or fhe.device_count() < 1:
        sys.exit("bench_hoisted_matvec needs the HIP build and a GPU")
    shapes = [("n8192_4x60", fhe.generate_moduli([60] * 4, 8192), 8192, True),
              ("stock_n8192", ref_params.DEFAULT_128[8192], 8192, True),
              ("stock_n8192", ref_params.DEFAULT_128[8192], 8192, False),
              ("stock_n16384", ref_params.DEFAULT_128[16384], 16384, True)]
    if a.shapes:
        shapes = [s for s in shapes if s[0] in a.shapes]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def emit(s):
            print(s, flush=True)
            f.write(s + "\n")
            f.flush()
        run(shapes, tuple(a.rotations), tuple(a.batches), a.window, a.windows, int(a.max_out_gib * (1 << 30)), emit=emit)


if __name__ == "__main__":
    main()
