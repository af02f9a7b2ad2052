// kernels_kskeyed.hpp -- stage B of the unfused key switch with ONE KEY PER GROUP OF POLYNOMIALS (keyed batches).
// A server holds a few ciphertexts from each of many clients, each under the client's own relinearization / Galois
// keys; stage A of the unfused form (ks_ntt_kernel, kernels_ks.hpp) never reads a key, so one launch transforms every
// client's digit rows, and only the multiply-accumulate below has to know whose polynomial it is working on.
#pragma once
#include "kernels_ks.hpp"

namespace fhe {
namespace k {

// One entry per key of a set: the key's c0 and c1 words, [ndigits][Lk][N] each (engine.hpp: KskSet::table).
struct KsKeyPtr {
    const u64 *k0, *k1;
};

// ks_mac_keyed_kernel: ks_mac_kernel's sum (F/bfv/keys/key_switching_key.rs:241-320, the lazy accumulation of
// F/bfv/ops/dot_product.rs:54-180), written a second time so that the kernel every single-key launch runs stays as it
// is.  Kept from it: one lane per 16-byte chunk of an output row (b, j), lazy 128-bit accumulators folded every sixteen
// digits, the own-row read from `xhat`, the `gal` gathers on `xhat` and `addend0`, canonical outputs.
// The one difference: (k0, k1) of polynomial b are entry ((poly0 + b) / per_key) % nkeys of `keys`, a table in device
// memory (a set may hold more keys than kernel arguments could); poly0 is the index, within the CALL, of this launch's
// first polynomial, so a chunk of polynomials need not end on a key boundary.  The index is block-uniform and goes
// through to_sgpr (as ksk_gen_kernel's out.k[key]): the entry is read with scalar loads and both pointers are scalars.
// Grid: the block order of ks_mac_kernel is kept -- ids 8 apart share a key range, polynomial fastest within a group
// of eight ranges -- although its purpose there (re-reading ONE key from an XCD's L2) holds here only among the
// per_key polynomials of a client: neighbouring blocks of one XCD still walk neighbouring polynomials, which are the
// ones that share a key, and the host computes one grid for both kernels.
__global__ void __launch_bounds__(256)
    ks_mac_keyed_kernel(const u64 *__restrict__ w, u64 *__restrict__ out0, u64 *__restrict__ out1, u64 out_poly_stride,
                        const u64 *__restrict__ addend0, const u64 *__restrict__ addend1, u64 addend_poly_stride,
                        const KsKeyPtr *__restrict__ keys, uint32_t nkeys, uint32_t per_key, uint32_t poly0,
                        const DevMod *__restrict__ mods, uint32_t ndigits, uint32_t lk, uint32_t j0, uint32_t jg,
                        uint32_t logn, const u64 *__restrict__ xhat, u64 xhat_poly_stride, uint32_t npolys, uint32_t gal) {
    const uint32_t n = 1u << logn;
    const uint32_t cpr = n >= 512 ? n / 512 : 1;          // 256-lane chunks per row
    const uint32_t nkr = jg * cpr;                        // key ranges of this launch
    const uint32_t grp = blockIdx.x >> 3, x8 = blockIdx.x & 7;
    const uint32_t krhi = grp / npolys, b = grp - krhi * npolys;
    const uint32_t kr = krhi * 8 + x8;
    if (kr >= nkr) return;                                // (block-uniform) tail of the rounded-up grid
    const uint32_t key = to_sgpr(((poly0 + b) / per_key) % nkeys);   // (block-uniform) whose polynomial this is
    const uint32_t jj = kr / cpr, cb = kr - jj * cpr, j = j0 + jj;
    const uint32_t ci = cb * 256 + threadIdx.x;           // 16-byte chunk inside the row
    if (2 * ci >= n) return;
    const KsKeyPtr kp = keys[key];
    const DevMod md = mods[j];
    const u64 roff = 2 * (u64)ci;
    const u64 *wp = w + (((u64)b * ndigits) * jg + jj) * n + roff;      // + i * jg * n per digit
    const u64 *kp0 = kp.k0 + (u64)j * n + roff, *kp1 = kp.k1 + (u64)j * n + roff;   // + i * lk * n per digit
    const bool own = xhat != nullptr && j < ndigits;      // (block-uniform)
    u128_t a0x = 0, a0y = 0, a1x = 0, a1y = 0;
    auto mac = [&](u128_t &acc, u64 x, u64 k) {
        u64 hi, lo;
        mul_wide62(x, k, hi, lo);
        acc += ((u128_t)hi << 64) | lo;
    };
    auto fold = [&](u128_t &acc) { acc = reduce_u128((u64)(acc >> 64), (u64)acc, md); };
    for (uint32_t i0 = 0; i0 < ndigits; i0 += 16) {
        const uint32_t i1 = i0 + 16 < ndigits ? i0 + 16 : ndigits;
        if (i0) fold(a0x), fold(a0y), fold(a1x), fold(a1y);
#pragma unroll 4
        for (uint32_t i = i0; i < i1; i++) {
            // (W is read exactly once, by this lane: a streaming load; the key words are the client's other polynomials': cached)
            u64x2 xv;
            if (own && i == j) {
                const u64 *xrow = xhat + (u64)b * xhat_poly_stride + (u64)j * n;
                if (gal) {
                    xv.x = xrow[galois_src_index((uint32_t)roff, gal, logn)];
                    xv.y = xrow[galois_src_index((uint32_t)roff + 1, gal, logn)];
                } else {
                    xv = *reinterpret_cast<const u64x2 *>(xrow + roff);
                }
            } else {
                xv = load_stream(reinterpret_cast<const u64x2 *>(wp + (u64)i * jg * n));
            }
            const u64x2 q0 = *reinterpret_cast<const u64x2 *>(kp0 + (u64)i * lk * n);
            const u64x2 q1 = *reinterpret_cast<const u64x2 *>(kp1 + (u64)i * lk * n);
            mac(a0x, xv.x, q0.x);
            mac(a0y, xv.y, q0.y);
            mac(a1x, xv.x, q1.x);
            mac(a1y, xv.y, q1.y);
        }
    }
    u64x2 r0, r1;
    r0.x = reduce_u128((u64)(a0x >> 64), (u64)a0x, md);
    r0.y = reduce_u128((u64)(a0y >> 64), (u64)a0y, md);
    r1.x = reduce_u128((u64)(a1x >> 64), (u64)a1x, md);
    r1.y = reduce_u128((u64)(a1y >> 64), (u64)a1y, md);
    const u64 ooff = (u64)b * out_poly_stride + (u64)j * n + roff;
    const u64 aoff = (u64)b * addend_poly_stride + (u64)j * n + roff;
    if (addend0) {
        u64x2 a;
        if (gal) {
            const u64 *arow = addend0 + aoff - roff;
            a.x = arow[galois_src_index((uint32_t)roff, gal, logn)];
            a.y = arow[galois_src_index((uint32_t)roff + 1, gal, logn)];
        } else {
            a = *reinterpret_cast<const u64x2 *>(addend0 + aoff);
        }
        r0.x = add_mod(r0.x, a.x, md.p);
        r0.y = add_mod(r0.y, a.y, md.p);
    }
    if (addend1) {
        const u64x2 a = *reinterpret_cast<const u64x2 *>(addend1 + aoff);
        r1.x = add_mod(r1.x, a.x, md.p);
        r1.y = add_mod(r1.y, a.y, md.p);
    }
    *reinterpret_cast<u64x2 *>(out0 + ooff) = r0;
    *reinterpret_cast<u64x2 *>(out1 + ooff) = r1;
}

}  // namespace k
}  // namespace fhe
