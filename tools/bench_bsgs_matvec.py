#!/usr/bin/env python3
"""Baby-step/giant-step hoisted matrix-vector product (fhe_bfv_matvec_bsgs_dev) against the two routes it competes with, on
tools/bench_hoisted_matvec.py's shapes and batches for G x B in {4 x 4, 8 x 8, 16 x 16} diagonals shared by the batch.
Routes per cell, through the raw ABI on preallocated buffers:
  bsgs_rule          the new call at the engine's two shape rules (bsgs_group_tile, hoist_rot_group)
  bsgs_tile_1        the new call with the baby tile forced to 1
  bsgs_one_group     the new call with the giant set's rot_split forced to 1
  composed           its specification: G fhe_bfv_matvec_hoisted_dev calls, G - 1 one-key fhe_bfv_galois_hoisted_dev calls
                     and G - 1 additions (fhe_poly_add_dev)
  flat               fhe_bfv_matvec_hoisted_dev over R = G B - 1 keys and the identity diagonal: a different answer word
                     for word, the same plaintext.  Skipped, and said so, where its keys exceed --max-key-gib.
They are timed in one process, their windows alternating (tools/bench_keyed.py's method), the median of `--windows` (at
least three) with the lowest and highest next to it.
The new kernels alone: one more call of bsgs_rule under the engine's profiler (outside the timed windows) gives the time of
bsgs_baby_kernel and of bsgs_giant_kernel (+ the summing kernel); with the bytes each has to move that is a rate, reported
as a fraction of fhe_ubench_copy's streaming rate in the same process.
One JSON line per cell on stdout and in --out (default profiles/bsgs_matvec_bench.jsonl)."""
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
from bench_hoisted_matvec import device_cus  # noqa: E402

GRIDS = ((4, 4), (8, 8), (16, 16))   # (G, B)
BATCHES = (1, 16, 256)


def baby_bytes(batch, nbaby, G, L, n, gt):
    """Bytes bsgs_baby_kernel moves: per tile of gt groups every baby key and, per ciphertext, every rotation's rows of W,
    own row and addend; per group its diagonals (identity included) and one inner sum; the ciphertext's own words."""
    row = n * 8
    tiles = -(-G // gt)
    keys = tiles * nbaby * 2 * L * L * row
    gathered = tiles * batch * nbaby * (L * L + L) * row
    diagonals = batch * G * (nbaby + 1) * L * row
    own = tiles * batch * 2 * L * row
    return keys + gathered + diagonals + own + batch * G * 2 * L * row


def giant_bytes(batch, ngiant, L, n, groups):
    """Bytes bsgs_giant_kernel (+ the summing kernel) moves: every giant key once, per ciphertext and giant W, own row and
    addend, inner sum 0, one output, and the partial sums written and read where the giants are cut into groups."""
    row = n * 8
    keys = ngiant * 2 * L * L * row
    gathered = batch * ngiant * (L * L + L) * row
    outputs = batch * 2 * L * row
    partial = 2 * groups * outputs if groups > 1 else 0
    return keys + gathered + 2 * outputs + partial


def rule_tile(cus, batch, L, n, G):
    """engine.hpp: bsgs_group_tile, restated for the record (default W budget: one chunk, one key-modulus group)."""
    if not cus:
        return None
    for gt in (4, 2):
        if gt <= G and batch * L * max(n // 512, 1) * -(-G // gt) >= 2 * cus:
            return gt
    return 1


def rule_groups(cus, batch, L, n, ngiant):
    """engine.hpp: hoist_rot_group on the giants, restated for the record: the groups the giants are cut into."""
    if not cus:
        return None
    blocks = batch * L * max(n // 512, 1)
    groups = 1 if blocks >= 2 * cus else min(-(-2 * cus // blocks), ngiant)
    return -(-ngiant // -(-ngiant // groups))


def profiled(call):
    """{label: ms} inside call(): the second of two profiled calls."""
    fhe.prof_enable(True)
    try:
        call()
        sync()
        fhe.prof_reset()
        call()
        sync()
    finally:
        fhe.prof_enable(False)
    t = {}
    for label, _, launches, ms in fhe.prof_entries():
        if launches:
            key = label if label in ("bsgs_baby", "bsgs_giant", "mbfv_sum") else "stage_a" if label.startswith("ks_digit_ntt") else "other"
            t[key] = t.get(key, 0.0) + ms
    fhe.prof_reset()
    return t


def run(shapes, grids, batches, window_s, windows, max_key_bytes, copy_bytes=1 << 30, emit=print):
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
            key_bytes = 2 * L * L * n * 8                    # the c0 / c1 words of one key
            gmax, bmax = max(g for g, _ in grids), max(b for _, b in grids)
            flat_max = max((g * b - 1 for g, b in grids if (g * b - 1) * key_bytes * 3 <= max_key_bytes), default=0)
            keys = []
            for c in range(max(flat_max, gmax + bmax - 2)):
                k = ctx.synth_uniform(0x42534753 + c, 0, 0, 2 * L, 1).reshape(2, L, L, n)
                keys.append(fhe.KeySwitchingKey(ctx, ctx, k[0], k[1]))
                del k
            ones = [fhe.KeySet([k]) for k in keys[bmax - 1:bmax - 1 + gmax - 1]]   # the composition's one-key giant sets
            pts = ctx.synth_uniform(0x42534757, 0, 0, 1, gmax * bmax)
            pp = pts.data_ptr()
            for batch in batches:
                ct = ctx.synth_uniform(0x42534754, 0, 0, 2, batch)
                out = ctx.synth_uniform(0x42534755, 0, 0, 2, batch)
                inner = ctx.synth_uniform(0x42534756, 0, 0, 2, batch * (gmax + 1))
                pc, po, pi = ct.data_ptr(), out.data_ptr(), inner.data_ptr()
                ctb = batch * 2 * pl                          # bytes of the batch's ciphertexts
                for G, B in grids:
                    nbaby, ngiant = B - 1, G - 1
                    baby = fhe.KeySet(keys[:nbaby])
                    giant = fhe.KeySet(keys[bmax - 1:bmax - 1 + ngiant])
                    bex = (C.c_size_t * nbaby)(*[pow(3, r + 1, 2 * n) for r in range(nbaby)])
                    gex = (C.c_size_t * ngiant)(*[pow(3, (g + 1) * B, 2 * n) for g in range(ngiant)])
                    st = _stream()
                    nflat = G * B - 1
                    flat_fits = nflat <= flat_max
                    fset = fhe.KeySet(keys[:nflat]) if flat_fits else None
                    fex = (C.c_size_t * nflat)(*[pow(3, r + 1, 2 * n) for r in range(nflat)])

                    def bsgs(tile, split):
                        def call():
                            L_.fhe_kskset_set_bsgs_tile(baby._h, tile)
                            L_.fhe_kskset_set_rot_split(giant._h, split)
                            return L_.fhe_bfv_matvec_bsgs_dev(baby._h, bex, nbaby, giant._h, gex, ngiant, vp(pc), vp(pp), 1, vp(po),
                                                              batch, st)
                        return call

                    def composed():
                        r_ = 0
                        for g in range(G):
                            row0 = pp + g * B * pl
                            r_ |= L_.fhe_bfv_matvec_hoisted_dev(baby._h, bex, nbaby, vp(pc), vp(row0 + pl), 1, vp(row0),
                                                                vp(po if g == 0 else pi + g * ctb), batch, st)
                        for g in range(1, G):
                            one = (C.c_size_t * 1)(gex[g - 1])
                            r_ |= L_.fhe_bfv_galois_hoisted_dev(ones[g - 1]._h, one, 1, vp(pi + g * ctb), vp(pi), batch, st)
                            r_ |= L_.fhe_poly_add_dev(ctx._h, vp(po), vp(pi), batch * 2, st)
                        return r_

                    def flat():
                        return L_.fhe_bfv_matvec_hoisted_dev(fset._h, fex, nflat, vp(pc), vp(pp + pl), 1, vp(pp), vp(po), batch, st)
                    routes = {"bsgs_rule": bsgs(0, 0), "bsgs_tile_1": bsgs(1, 0), "bsgs_one_group": bsgs(0, 1), "composed": composed}
                    if flat_fits:
                        routes["flat"] = flat
                    for fn in routes.values():
                        _lib.check(fn())
                    ms = alternating_ms(routes, window_s, windows)
                    gt, groups = rule_tile(cus, batch, L, n, G), rule_groups(cus, batch, L, n, ngiant)
                    row = dict(shape=name, n=n, moduli=L, f64=f64, batch=batch, G=G, B=B, rule_tile=gt,
                               rule_giant_groups=groups, bsgs_keys=nbaby + ngiant, bsgs_key_bytes=(nbaby + ngiant) * key_bytes,
                               flat_keys=nflat, flat_key_bytes=nflat * key_bytes, flat_run=flat_fits)
                    if not flat_fits:
                        row["flat_skipped"] = "the flat route's %d keys (three word arrays a handle) exceed --max-key-gib" % nflat
                    for route in routes:
                        med, lo, hi = ms[route]
                        row[route + "_ms"] = round(med, 4)
                        row[route + "_ms_low"] = round(lo, 4)
                        row[route + "_ms_high"] = round(hi, 4)
                    for other in ("bsgs_tile_1", "bsgs_one_group", "composed", "flat"):
                        if other in ms:
                            row[other + "_over_bsgs_rule"] = round(ms[other][0] / ms["bsgs_rule"][0], 2)
                    t = profiled(routes["bsgs_rule"])
                    ngroups = groups or 1
                    bb, gb = baby_bytes(batch, nbaby, G, L, n, gt or 1), giant_bytes(batch, ngiant, L, n, ngroups if "mbfv_sum" in t else 1)
                    b_ms, g_ms = t.get("bsgs_baby", 0.0), t.get("bsgs_giant", 0.0) + t.get("mbfv_sum", 0.0)
                    for what, ms_, by in (("baby", b_ms, bb), ("giant", g_ms, gb)):
                        rate = by / (ms_ * 1e-3) if ms_ > 0 else 0.0
                        row.update({what + "_kernel_ms": round(ms_, 4), what + "_bytes": by, what + "_gb_per_s": round(rate / 1e9, 1),
                                    what + "_fraction_of_copy": round(rate / copy_rate, 3) if copy_rate else None})
                    row.update(stage_a_ms=round(t.get("stage_a", 0.0), 4), other_ms=round(t.get("other", 0.0), 4),
                               partial_sums="mbfv_sum" in t, copy_gb_per_s=round(copy_rate / 1e9, 1))
                    emit(json.dumps(row))
                    rows.append(row)
                    del baby, giant, fset
                    fhe.workspace_trim()
                del ct, out, inner
            del keys, ones, pts
        finally:
            fhe.set_f64(True)
    return rows


def main():
    import ref_params
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.15)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--max-key-gib", type=float, default=24.0)
    ap.add_argument("--grids", nargs="+", default=["%dx%d" % g for g in GRIDS], help="G x B, e.g. 4x4 8x8")
    ap.add_argument("--batches", type=int, nargs="+", default=list(BATCHES))
    ap.add_argument("--shapes", nargs="+", default=None, help="names of the shapes to run (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bsgs_matvec_bench.jsonl"))
    a = ap.parse_args()
    if a.windows < 3:
        sys.exit("at least three windows")
    _lib.lib()
    if not _lib.loaded_path().endswith("libfhe_hip.so") or fhe.device_count() < 1:
        sys.exit("bench_bsgs_matvec needs the HIP build and a GPU")
    shapes = [("n8192_4x60", fhe.generate_moduli([60] * 4, 8192), 8192, True),
              ("stock_n8192", ref_params.DEFAULT_128[8192], 8192, True),
              ("stock_n8192", ref_params.DEFAULT_128[8192], 8192, False),
              ("stock_n16384", ref_params.DEFAULT_128[16384], 16384, True)]
    if a.shapes:
        shapes = [s for s in shapes if s[0] in a.shapes]
    grids = tuple(tuple(int(v) for v in g.split("x")) for g in a.grids)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def emit(s):
            print(s, flush=True)
            f.write(s + "\n")
            f.flush()
        run(shapes, grids, tuple(a.batches), a.window, a.windows, int(a.max_key_gib * (1 << 30)), emit=emit)


if __name__ == "__main__":
    main()
