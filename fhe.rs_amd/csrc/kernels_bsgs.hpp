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
// hoist_matvec_kernel's steps -- gather, own row from `ct1`, the digit loop, reduce, add the gathered c0 -- and each
// rotation's canonical words go into GT sets of four 128-bit accumulators, one set per group of the tile, each
// multiplied by THAT group's diagonal words (pts[g][r + 1]) and folded every sixteen rotations (KsMacQuad's bound).
// The GT sets are four arrays on KsMacQuad's single-accumulator steps, not KsMacQuad[GT]: as an array of quads the
// wider tiles compile to other code than they had.  After the last fold each group adds its identity diagonal
// pts[g][0] (FHE_KS_IDENTITY_DIAG).  A tile cut by `ngroups` handles fewer groups under a block-uniform test.
// Group 0 of ciphertext b -- the one no giant rotates -- is written to
// first0 / first1 + b * first_poly_stride, group g >= 1 to out0 / out1 + b * out_poly_stride + (g - 1) * out_group_stride:
// the inner sums the giant stage transforms form one array of their own.
// Grid: within eight ranges the ciphertext runs fastest, then the giant tile, so the neighbours of a block on its XCD
// walk the same baby keys in step.
template <int GT>
__global__ void __launch_bounds__(256)
    bsgs_baby_kernel(const u64 *__restrict__ w, u64 *__restrict__ first0, u64 *__restrict__ first1, u64 first_poly_stride,
                     u64 *__restrict__ out0, u64 *__restrict__ out1, u64 out_poly_stride, u64 out_group_stride,
                     const u64 *__restrict__ ct0, const u64 *__restrict__ ct1, u64 ct_poly_stride,
                     const KsKeyPtr *__restrict__ keys, HoistExps exps, const u64 *__restrict__ pts, u64 pts_batch_stride,
                     u64 pts_group_stride, u64 pts_rot_stride, const DevMod *__restrict__ mods, uint32_t ndigits, uint32_t lk,
                     uint32_t j0, uint32_t jg, uint32_t logn, uint32_t nb, uint32_t nr, uint32_t ngroups, uint32_t ntiles) {
    KsMacAt at(logn, jg, nb, ntiles);
    if (at.kr >= at.nkr) return;                          // (block-uniform) tail of the rounded-up grid
    const uint32_t tile = to_sgpr(at.item / nb), b = at.item - tile * nb;   // (block-uniform) which giant tile of which ciphertext
    const uint32_t g0 = tile * GT;
    const uint32_t ng = ngroups - g0 < (uint32_t)GT ? ngroups - g0 : (uint32_t)GT;   // (block-uniform) groups of a cut tile
    at.lane(j0);
    if (2 * at.ci >= at.n) return;
    const uint32_t n = at.n, j = at.j;
    const DevMod md = mods[j];
    const u64 roff = at.roff();
    const u64 *wp = w + (((u64)b * ndigits) * jg + at.jj) * n;          // + i * jg * n per digit
    const u64 *c0row = ct0 + (u64)b * ct_poly_stride + (u64)j * n;
    const u64 *c1row = ct1 + (u64)b * ct_poly_stride + (u64)j * n;      // (stage A skips the own row: W[j][j] = c1 row j)
    // + t * pts_group_stride per group of the tile, + (r + 1) * pts_rot_stride per baby rotation (column 0: the identity)
    const u64 *prow = pts + (u64)b * pts_batch_stride + (u64)g0 * pts_group_stride + (u64)j * n + roff;
    u128_t s0x[GT], s0y[GT], s1x[GT], s1y[GT];
#pragma unroll
    for (int t = 0; t < GT; t++) s0x[t] = 0, s0y[t] = 0, s1x[t] = 0, s1y[t] = 0;
    for (uint32_t rr = 0; rr < nr; rr++) {
        const uint32_t r = to_sgpr(rr);
        const uint32_t gal = exps.e[r];
        const KsKeyPtr kp = keys[r];
        const KsMacGather gather(roff, gal, logn);
        const u64 *kp0 = kp.k0 + (u64)j * n + roff, *kp1 = kp.k1 + (u64)j * n + roff;   // + i * lk * n per digit
        KsMacQuad acc;
        FHE_KS_DIGIT_LOOP(acc, ndigits, md, kp0, kp1, lk, n, xv = gather(i == j ? c1row : wp + (u64)i * jg * n))
        u64x2 r0, r1;
        acc.reduce(md, r0, r1);
        const u64x2 a = gather(c0row);
        r0.x = add_mod(r0.x, a.x, md.p);
        r0.y = add_mod(r0.y, a.y, md.p);
        const bool refold = rr != 0 && (rr & 15) == 0;
        const u64 *pr = prow + (u64)(r + 1) * pts_rot_stride;
#pragma unroll
        for (int t = 0; t < GT; t++) {
            if ((uint32_t)t < ng) {
                const u64x2 pv = *reinterpret_cast<const u64x2 *>(pr + (u64)t * pts_group_stride);
                if (refold)
                    s0x[t] = KsMacQuad::red1(s0x[t], md), s0y[t] = KsMacQuad::red1(s0y[t], md), s1x[t] = KsMacQuad::red1(s1x[t], md),
                    s1y[t] = KsMacQuad::red1(s1y[t], md);
                KsMacQuad::mac1(s0x[t], r0.x, pv.x);
                KsMacQuad::mac1(s0y[t], r0.y, pv.y);
                KsMacQuad::mac1(s1x[t], r1.x, pv.x);
                KsMacQuad::mac1(s1y[t], r1.y, pv.y);
            }
        }
    }
    const u64x2 x0 = *reinterpret_cast<const u64x2 *>(c0row + roff);
    const u64x2 x1 = *reinterpret_cast<const u64x2 *>(c1row + roff);
#pragma unroll
    for (int t = 0; t < GT; t++) {
        if ((uint32_t)t < ng) {
            u64x2 o0, o1;
            o0.x = KsMacQuad::red1(s0x[t], md);
            o0.y = KsMacQuad::red1(s0y[t], md);
            o1.x = KsMacQuad::red1(s1x[t], md);
            o1.y = KsMacQuad::red1(s1y[t], md);
            const u64x2 pv = *reinterpret_cast<const u64x2 *>(prow + (u64)t * pts_group_stride);
            FHE_KS_IDENTITY_DIAG(o0, o1, x0, x1, pv, md)
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
// The accumulator quad is CARRIED ACROSS THE GIANTS: before a giant's first digit it is folded (not before the
// group's first giant) and the giant's gathered c0 words of inner[b][g] are added to the c0 pair INSIDE the window.  The
// bound is KsMacQuad's with one more word below 2^62 in the window: 2^128 - 2^67 + 16 + 2^63 < 2^128.
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
    KsMacAt at(logn, jg, nb, ngroups);
    if (at.kr >= at.nkr) return;                          // (block-uniform) tail of the rounded-up grid
    const uint32_t gg = to_sgpr(at.item / nb), b = at.item - gg * nb;   // (block-uniform) which giant group of which ciphertext
    at.lane(j0);
    if (2 * at.ci >= at.n) return;
    const uint32_t n = at.n, j = at.j;
    const DevMod md = mods[j];
    const u64 roff = at.roff();
    const u64 *i0row = in0 + (u64)b * in_poly_stride + (u64)j * n;      // + gi * in_group_stride per giant
    const u64 *i1row = in1 + (u64)b * in_poly_stride + (u64)j * n;
    KsMacQuad acc;
    const uint32_t glo = gg * gpg, ghi = glo + gpg < ngiant ? glo + gpg : ngiant;
    for (uint32_t gv = glo; gv < ghi; gv++) {
        const uint32_t gi = to_sgpr(gv);
        const uint32_t gal = to_sgpr(exps.e[gi]);
        const KsKeyPtr kp = keys[gi];
        const KsMacGather gather(roff, gal, logn);
        const u64 *wp = w + ((((u64)b * ngiant + gi) * ndigits) * jg + at.jj) * n;      // + i * jg * n per digit
        const u64 *xrow = i1row + (u64)gi * in_group_stride;      // (stage A skips the own row: W[j][j] = c1 row j)
        const u64 *kp0 = kp.k0 + (u64)j * n + roff, *kp1 = kp.k1 + (u64)j * n + roff;   // + i * lk * n per digit
        if (gv != glo) acc.fold(md);
        const u64x2 a = gather(i0row + (u64)gi * in_group_stride);
        acc.a0x += a.x;                                   // (inside the window: the bound above)
        acc.a0y += a.y;
        FHE_KS_DIGIT_LOOP(acc, ndigits, md, kp0, kp1, lk, n, xv = gather(i == j ? xrow : wp + (u64)i * jg * n))
    }
    u64x2 r0, r1;
    acc.reduce(md, r0, r1);
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
