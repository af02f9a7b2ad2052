// kernels_bsgs.hpp -- the two stage B kernels of the BABY-STEP/GIANT-STEP hoisted matrix-vector product (Halevi-Shoup,
// CRYPTO 2018 section 4.3): with rotation r = g B + b,
//   sum_r d_r rot_r(x) = sum_g rot_{gB}( sum_b d'_{g,b} rot_b(x) ),   d'_{g,b} = rot_{-gB}(d_{gB+b})  (the caller's part),
// so that (B - 1) + (G - 1) Galois keys and digit loops serve G B diagonals.
//
// NOT the reference's words, in the terms of kernels_kshoist.hpp: every rotation inside substitutes the lifted digits of
// c1 where GaloisKey::relinearize lifts the digits of substitute(c1).  The specification is the composition of the two
// calls these kernels start from (restated on Python ints in tests/bsgs_ref.py):
//   inner_g = hoist_matvec_kernel's sum over the baby keys with the diagonals pts[g][1..B) and pt0 = pts[g][0]
//   out     = inner_0 + sum_{g >= 1} hoist_mac_kernel's rotation of inner_g under giant key g - 1
// canonical mod q_j, word for word, whatever tile or split a launch runs under.
#pragma once
#include "kernels_kshoist.hpp"

namespace fhe {
namespace k {

// bsgs_baby_kernel<GT>: G inner sums from ONE digit loop per baby rotation.  One block per (ciphertext b, key range
// (j, 256-lane chunk), tile of GT giant groups); it loops over the nr baby rotations of the launch with
// hoist_matvec_kernel's digit loop unchanged -- gather, own row from `ct1`, fold every sixteen digits, reduce, add the
// gathered c0 -- and each rotation's canonical words go into GT sets of four 128-bit accumulators, one set per group of
// the tile, each multiplied by THAT group's diagonal words (pts[g][r + 1]) and folded every sixteen rotations: both
// factors are below 2^62, so sixteen products and a folded word stay below 2^128.  After the last fold each group adds
// its identity diagonal pts[g][0] times the lane's own words of c0 / c1 (no gather, no key).  A tile cut by `ngroups`
// handles fewer groups under a block-uniform test.  Group 0 of ciphertext b -- the one no giant rotates -- is written to
// first0 / first1 + b * first_poly_stride, group g >= 1 to out0 / out1 + b * out_poly_stride + (g - 1) * out_group_stride:
// the inner sums the giant stage transforms form one array of their own.
// Grid: the siblings' order.  Ids 8 apart share a key range; within eight ranges the ciphertext runs fastest, then the
// giant tile, so the neighbours of a block on its XCD walk the same baby keys in step.
template <int GT>
__global__ void __launch_bounds__(256)
    bsgs_baby_kernel(const u64 *__restrict__ w, u64 *__restrict__ first0, u64 *__restrict__ first1, u64 first_poly_stride,
                     u64 *__restrict__ out0, u64 *__restrict__ out1, u64 out_poly_stride, u64 out_group_stride,
                     const u64 *__restrict__ ct0, const u64 *__restrict__ ct1, u64 ct_poly_stride,
                     const KsKeyPtr *__restrict__ keys, HoistExps exps, const u64 *__restrict__ pts, u64 pts_batch_stride,
                     u64 pts_group_stride, u64 pts_rot_stride, const DevMod *__restrict__ mods, uint32_t ndigits, uint32_t lk,
                     uint32_t j0, uint32_t jg, uint32_t logn, uint32_t nb, uint32_t nr, uint32_t ngroups, uint32_t ntiles) {
    const uint32_t n = 1u << logn;
    const uint32_t cpr = n >= 512 ? n / 512 : 1;          // 256-lane chunks per row
    const uint32_t nkr = jg * cpr;                        // key ranges of this launch
    const uint32_t grp = blockIdx.x >> 3, x8 = blockIdx.x & 7;
    const uint32_t per = nb * ntiles;
    const uint32_t krhi = grp / per, bt = grp - krhi * per;
    const uint32_t kr = krhi * 8 + x8;
    if (kr >= nkr) return;                                // (block-uniform) tail of the rounded-up grid
    const uint32_t tile = to_sgpr(bt / nb), b = bt - tile * nb;   // (block-uniform) which giant tile of which ciphertext
    const uint32_t g0 = tile * GT;
    const uint32_t ng = ngroups - g0 < (uint32_t)GT ? ngroups - g0 : (uint32_t)GT;   // (block-uniform) groups of a cut tile
    const uint32_t jj = kr / cpr, cb = kr - jj * cpr, j = j0 + jj;
    const uint32_t ci = cb * 256 + threadIdx.x;           // 16-byte chunk inside the row
    if (2 * ci >= n) return;
    const DevMod md = mods[j];
    const u64 roff = 2 * (u64)ci;
    const u64 *wp = w + (((u64)b * ndigits) * jg + jj) * n;             // + i * jg * n per digit
    const u64 *c0row = ct0 + (u64)b * ct_poly_stride + (u64)j * n;
    const u64 *c1row = ct1 + (u64)b * ct_poly_stride + (u64)j * n;      // (stage A skips the own row: W[j][j] = c1 row j)
    // + t * pts_group_stride per group of the tile, + (r + 1) * pts_rot_stride per baby rotation (column 0: the identity)
    const u64 *prow = pts + (u64)b * pts_batch_stride + (u64)g0 * pts_group_stride + (u64)j * n + roff;
    auto mac = [&](u128_t &acc, u64 x, u64 k) {
        u64 hi, lo;
        mul_wide62(x, k, hi, lo);
        acc += ((u128_t)hi << 64) | lo;
    };
    auto fold = [&](u128_t &acc) { acc = reduce_u128((u64)(acc >> 64), (u64)acc, md); };
    u128_t s0x[GT], s0y[GT], s1x[GT], s1y[GT];
#pragma unroll
    for (int t = 0; t < GT; t++) s0x[t] = 0, s0y[t] = 0, s1x[t] = 0, s1y[t] = 0;
    for (uint32_t rr = 0; rr < nr; rr++) {
        const uint32_t r = to_sgpr(rr);
        const uint32_t gal = exps.e[r];
        const KsKeyPtr kp = keys[r];
        const uint32_t src = galois_src_index((uint32_t)roff, gal, logn);   // (the source of roff + 1 is src ^ 1)
        const u64 soff = src & ~1u;
        const bool swap = (src & 1u) != 0;
        auto gather = [&](const u64 *row) {
            const u64x2 v = *reinterpret_cast<const u64x2 *>(row + soff);
            return swap ? u64x2{v.y, v.x} : v;
        };
        const u64 *kp0 = kp.k0 + (u64)j * n + roff, *kp1 = kp.k1 + (u64)j * n + roff;   // + i * lk * n per digit
        u128_t a0x = 0, a0y = 0, a1x = 0, a1y = 0;
        for (uint32_t i0 = 0; i0 < ndigits; i0 += 16) {
            const uint32_t i1 = i0 + 16 < ndigits ? i0 + 16 : ndigits;
            if (i0) fold(a0x), fold(a0y), fold(a1x), fold(a1y);
#pragma unroll 4
            for (uint32_t i = i0; i < i1; i++) {
                const u64x2 xv = gather(i == j ? c1row : wp + (u64)i * jg * n);
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
        const u64x2 a = gather(c0row);
        r0.x = add_mod(r0.x, a.x, md.p);
        r0.y = add_mod(r0.y, a.y, md.p);
        const bool refold = rr != 0 && (rr & 15) == 0;
        const u64 *pr = prow + (u64)(r + 1) * pts_rot_stride;
#pragma unroll
        for (int t = 0; t < GT; t++) {
            if ((uint32_t)t < ng) {
                const u64x2 pv = *reinterpret_cast<const u64x2 *>(pr + (u64)t * pts_group_stride);
                if (refold) fold(s0x[t]), fold(s0y[t]), fold(s1x[t]), fold(s1y[t]);
                mac(s0x[t], r0.x, pv.x);
                mac(s0y[t], r0.y, pv.y);
                mac(s1x[t], r1.x, pv.x);
                mac(s1y[t], r1.y, pv.y);
            }
        }
    }
    const u64x2 x0 = *reinterpret_cast<const u64x2 *>(c0row + roff);
    const u64x2 x1 = *reinterpret_cast<const u64x2 *>(c1row + roff);
#pragma unroll
    for (int t = 0; t < GT; t++) {
        if ((uint32_t)t < ng) {
            u64x2 o0, o1;
            o0.x = reduce_u128((u64)(s0x[t] >> 64), (u64)s0x[t], md);
            o0.y = reduce_u128((u64)(s0y[t] >> 64), (u64)s0y[t], md);
            o1.x = reduce_u128((u64)(s1x[t] >> 64), (u64)s1x[t], md);
            o1.y = reduce_u128((u64)(s1y[t] >> 64), (u64)s1y[t], md);
            const u64x2 pv = *reinterpret_cast<const u64x2 *>(prow + (u64)t * pts_group_stride);
            o0.x = add_mod(o0.x, mul_mod(x0.x, pv.x, md), md.p);
            o0.y = add_mod(o0.y, mul_mod(x0.y, pv.y, md), md.p);
            o1.x = add_mod(o1.x, mul_mod(x1.x, pv.x, md), md.p);
            o1.y = add_mod(o1.y, mul_mod(x1.y, pv.y, md), md.p);
            const bool is_first = t == 0 && g0 == 0;      // (block-uniform; false at compile time for t > 0)
            const u64 ooff = (is_first ? (u64)b * first_poly_stride : (u64)b * out_poly_stride + (u64)(g0 + t - 1) * out_group_stride) +
                             (u64)j * n + roff;
            *reinterpret_cast<u64x2 *>((is_first ? first0 : out0) + ooff) = o0;
            *reinterpret_cast<u64x2 *>((is_first ? first1 : out1) + ooff) = o1;
        }
    }
}

// bsgs_giant_kernel: the key switches of the giants -- DIFFERENT ciphertexts, each with its own key and exponent -- summed
// into one output in registers.  One block per (ciphertext b, key range, giant group), "group" in hoist_rot_group's sense
// with giants in place of rotations; it loops over the giants [grp gpg, min(ngiant, (grp + 1) gpg)) of the call.  For
// giant gi (giant group g = gi + 1 of the grid of diagonals) it runs hoist_mac_kernel's digit loop on the W of item
// (b, gi) -- `w` holds nb x ngiant items, ciphertext-major -- with the own row inner[b][g].c1, key gi of `keys` and exponent
// exps.e[gi], both through to_sgpr.  inner[b][g], g >= 1, is in0 / in1 + b * in_poly_stride + (g - 1) * in_group_stride,
// inner[b][0] is first0 / first1 + b * first_poly_stride (bsgs_baby_kernel's two outputs).
// The four accumulators are CARRIED ACROSS THE GIANTS: before a giant's first digit they are folded (not before the
// group's first giant) and the giant's gathered c0 words of inner[b][g] are added to the c0 pair INSIDE the window.  The
// bound: a window between two folds holds one folded word and one addend, both below 2^62, and at most sixteen products
// below (2^62 - 1)^2 -- 2^128 - 2^67 + 16 + 2^63 < 2^128.
// The group that holds giant 1 (grp 0) also adds inner[b][0]: the lane's own words, no gather.
// Group grp writes polynomial pair b of out0 / out1 + grp * out_group_stride: the result itself when the call is one
// group, else a partial sum that mbfv_sum_kernel adds up.
// Grid: hoist_matvec_kernel's order with the giant group in the rotation group's place.
__global__ void __launch_bounds__(256)
    bsgs_giant_kernel(const u64 *__restrict__ w, u64 *__restrict__ out0, u64 *__restrict__ out1, u64 out_poly_stride,
                      u64 out_group_stride, const u64 *__restrict__ first0, const u64 *__restrict__ first1,
                      u64 first_poly_stride, const u64 *__restrict__ in0, const u64 *__restrict__ in1, u64 in_poly_stride,
                      u64 in_group_stride, const KsKeyPtr *__restrict__ keys, HoistExps exps, const DevMod *__restrict__ mods,
                      uint32_t ndigits, uint32_t lk, uint32_t j0, uint32_t jg, uint32_t logn, uint32_t nb, uint32_t ngiant,
                      uint32_t gpg, uint32_t ngroups) {
    const uint32_t n = 1u << logn;
    const uint32_t cpr = n >= 512 ? n / 512 : 1;          // 256-lane chunks per row
    const uint32_t nkr = jg * cpr;                        // key ranges of this launch
    const uint32_t grp = blockIdx.x >> 3, x8 = blockIdx.x & 7;
    const uint32_t per = nb * ngroups;
    const uint32_t krhi = grp / per, bg = grp - krhi * per;
    const uint32_t kr = krhi * 8 + x8;
    if (kr >= nkr) return;                                // (block-uniform) tail of the rounded-up grid
    const uint32_t gg = to_sgpr(bg / nb), b = bg - gg * nb;   // (block-uniform) which giant group of which ciphertext
    const uint32_t jj = kr / cpr, cb = kr - jj * cpr, j = j0 + jj;
    const uint32_t ci = cb * 256 + threadIdx.x;           // 16-byte chunk inside the row
    if (2 * ci >= n) return;
    const DevMod md = mods[j];
    const u64 roff = 2 * (u64)ci;
    const u64 *i0row = in0 + (u64)b * in_poly_stride + (u64)j * n;      // + gi * in_group_stride per giant
    const u64 *i1row = in1 + (u64)b * in_poly_stride + (u64)j * n;
    auto mac = [&](u128_t &acc, u64 x, u64 k) {
        u64 hi, lo;
        mul_wide62(x, k, hi, lo);
        acc += ((u128_t)hi << 64) | lo;
    };
    auto fold = [&](u128_t &acc) { acc = reduce_u128((u64)(acc >> 64), (u64)acc, md); };
    u128_t a0x = 0, a0y = 0, a1x = 0, a1y = 0;
    const uint32_t glo = gg * gpg, ghi = glo + gpg < ngiant ? glo + gpg : ngiant;
    for (uint32_t gv = glo; gv < ghi; gv++) {
        const uint32_t gi = to_sgpr(gv);
        const uint32_t gal = to_sgpr(exps.e[gi]);
        const KsKeyPtr kp = keys[gi];
        const uint32_t src = galois_src_index((uint32_t)roff, gal, logn);   // (the source of roff + 1 is src ^ 1)
        const u64 soff = src & ~1u;
        const bool swap = (src & 1u) != 0;
        auto gather = [&](const u64 *row) {
            const u64x2 v = *reinterpret_cast<const u64x2 *>(row + soff);
            return swap ? u64x2{v.y, v.x} : v;
        };
        const u64 *wp = w + ((((u64)b * ngiant + gi) * ndigits) * jg + jj) * n;         // + i * jg * n per digit
        const u64 *xrow = i1row + (u64)gi * in_group_stride;      // (stage A skips the own row: W[j][j] = c1 row j)
        const u64 *kp0 = kp.k0 + (u64)j * n + roff, *kp1 = kp.k1 + (u64)j * n + roff;   // + i * lk * n per digit
        if (gv != glo) fold(a0x), fold(a0y), fold(a1x), fold(a1y);
        const u64x2 a = gather(i0row + (u64)gi * in_group_stride);
        a0x += a.x;                                       // (inside the window: the bound above)
        a0y += a.y;
        for (uint32_t i0 = 0; i0 < ndigits; i0 += 16) {
            const uint32_t i1 = i0 + 16 < ndigits ? i0 + 16 : ndigits;
            if (i0) fold(a0x), fold(a0y), fold(a1x), fold(a1y);
#pragma unroll 4
            for (uint32_t i = i0; i < i1; i++) {
                const u64x2 xv = gather(i == j ? xrow : wp + (u64)i * jg * n);
                const u64x2 q0 = *reinterpret_cast<const u64x2 *>(kp0 + (u64)i * lk * n);
                const u64x2 q1 = *reinterpret_cast<const u64x2 *>(kp1 + (u64)i * lk * n);
                mac(a0x, xv.x, q0.x);
                mac(a0y, xv.y, q0.y);
                mac(a1x, xv.x, q1.x);
                mac(a1y, xv.y, q1.y);
            }
        }
    }
    u64x2 r0, r1;
    r0.x = reduce_u128((u64)(a0x >> 64), (u64)a0x, md);
    r0.y = reduce_u128((u64)(a0y >> 64), (u64)a0y, md);
    r1.x = reduce_u128((u64)(a1x >> 64), (u64)a1x, md);
    r1.y = reduce_u128((u64)(a1y >> 64), (u64)a1y, md);
    if (gg == 0) {
        const u64 foff = (u64)b * first_poly_stride + (u64)j * n + roff;
        const u64x2 x0 = *reinterpret_cast<const u64x2 *>(first0 + foff);
        const u64x2 x1 = *reinterpret_cast<const u64x2 *>(first1 + foff);
        r0.x = add_mod(r0.x, x0.x, md.p);
        r0.y = add_mod(r0.y, x0.y, md.p);
        r1.x = add_mod(r1.x, x1.x, md.p);
        r1.y = add_mod(r1.y, x1.y, md.p);
    }
    const u64 ooff = (u64)gg * out_group_stride + (u64)b * out_poly_stride + (u64)j * n + roff;
    *reinterpret_cast<u64x2 *>(out0 + ooff) = r0;
    *reinterpret_cast<u64x2 *>(out1 + ooff) = r1;
}

}  // namespace k
}  // namespace fhe
