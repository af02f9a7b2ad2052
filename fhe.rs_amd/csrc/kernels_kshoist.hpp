// kernels_kshoist.hpp -- stage B of the unfused key switch for MANY GALOIS ELEMENTS OF ONE CIPHERTEXT (hoisted
// rotations, Halevi-Shoup CRYPTO 2018 section 4).  Stage A (ks_ntt_kernel, kernels_ks.hpp) reads neither a key nor an
// exponent, and in Ntt form the substitution x -> x^e is a gather (galois_src_index): one set of transformed digit rows
// W serves every rotation of the ciphertext, and only the multiply-accumulate below knows which rotation it forms.
//
// NOT the reference's words.  GaloisKey::relinearize (F/bfv/keys/galois_key.rs:63-86) lifts the digits of
// substitute(c1); this kernel substitutes the lifted digits of c1.  Where the power-basis substitution negates a
// coefficient x of row i the reference lifts q_i - x into q_j, and W holds -x mod q_j.  Both digit sets are = sigma(c1)
// mod q_i with magnitude below q_i, so the two results decrypt to the same plaintext under the same noise bound, and
// they are word-equal only at exponent 1.  The specification is the restatement of tests/hoist_ref.py:
//   W[i][j] = NTT_j(PowerBasis(c1)_i mod q_j) (i != j),  W[i][i] = c1 row i,
//   out_r.c0[j] = sigma_r(c0[j]) + sum_i sigma_r(W[i][j]) * gk_r.c0[i][j],   out_r.c1[j] = sum_i sigma_r(W[i][j]) * gk_r.c1[i][j]
// with sigma_r the Ntt branch of Poly::substitute (M/rq/mod.rs:368-388) for exponent e_r, canonical outputs.
#pragma once
#include "kernels_kskeyed.hpp"

namespace fhe {
namespace k {

// The exponents of one launch's rotations (mod 2N, odd), a kernel argument: a call with more rotations than the table
// holds takes several launches on the same W, and nothing is uploaded.
constexpr uint32_t HOIST_ROTS = 64;
struct HoistExps {
    uint32_t e[HOIST_ROTS];
};

// hoist_mac_kernel: ks_mac_keyed_kernel's sum for nb ciphertexts x nr rotations.  Kept from it: one lane per 16-byte
// chunk of an output row, lazy 128-bit accumulators folded every sixteen digits, mul_wide62 / reduce_u128, the own row
// read from `xhat` (the caller's unpermuted c1) and the addend from `addend0` (c0), canonical outputs.
// What differs: output (b, r) reads W of ciphertext b and key rot0 + r of `keys` (block-uniform, through to_sgpr: both
// key pointers and the exponent are scalars), and EVERY operand but the key is read through the gather of exponent
// exps.e[r].  The two words of a chunk stay neighbours under it: e is odd, so destination roff + 1 (roff even) adds
// N/2 to the index before the last bit reversal, which flips bit 0 of the source -- one 16-byte load at the even source
// and a swap.  For destinations that differ only in their low k bits the sources are a permutation of one aligned block
// of 2^k words, so a wave's 128 destination words read one aligned 1 KiB block of the source row.
// W is read once per rotation: cached loads (ks_mac_keyed_kernel streams it).  The key words are read once per ciphertext.
// Grid: ids 8 apart share a key range (j, chunk) as in ks_mac_kernel, so an XCD keeps to one eighth of the ranges.
// Within a group of eight ranges the ciphertext runs fastest, then the rotation: the neighbours of a block on its XCD
// are the other ciphertexts under the SAME key slice (read from HBM once, then from L2), and the rotations in flight
// on an XCD at a time walk the same nb x ndigits rows of W (nb x 256 KiB at N = 8192 x 4 moduli: within the 4 MiB L2 up
// to 16 ciphertexts, from the Infinity Cache above).  The other order (rotation fastest) would keep W hot and re-read
// every key slice once per ciphertext; the keys are the larger operand from nr > nb / 2 on.
__global__ void __launch_bounds__(256)
    hoist_mac_kernel(const u64 *__restrict__ w, u64 *__restrict__ out0, u64 *__restrict__ out1, u64 out_poly_stride,
                     u64 out_rot_stride, const u64 *__restrict__ addend0, u64 addend_poly_stride,
                     const KsKeyPtr *__restrict__ keys, uint32_t rot0, HoistExps exps, const DevMod *__restrict__ mods,
                     uint32_t ndigits, uint32_t lk, uint32_t j0, uint32_t jg, uint32_t logn, const u64 *__restrict__ xhat,
                     u64 xhat_poly_stride, uint32_t nb, uint32_t nr) {
    const uint32_t n = 1u << logn;
    const uint32_t cpr = n >= 512 ? n / 512 : 1;          // 256-lane chunks per row
    const uint32_t nkr = jg * cpr;                        // key ranges of this launch
    const uint32_t grp = blockIdx.x >> 3, x8 = blockIdx.x & 7;
    const uint32_t per = nb * nr;
    const uint32_t krhi = grp / per, br = grp - krhi * per;
    const uint32_t kr = krhi * 8 + x8;
    if (kr >= nkr) return;                                // (block-uniform) tail of the rounded-up grid
    const uint32_t r = to_sgpr(br / nb), b = br - r * nb; // (block-uniform) which rotation of which ciphertext
    const uint32_t jj = kr / cpr, cb = kr - jj * cpr, j = j0 + jj;
    const uint32_t ci = cb * 256 + threadIdx.x;           // 16-byte chunk inside the row
    if (2 * ci >= n) return;
    const uint32_t gal = exps.e[r];
    const KsKeyPtr kp = keys[rot0 + r];
    const DevMod md = mods[j];
    const u64 roff = 2 * (u64)ci;
    const uint32_t src = galois_src_index((uint32_t)roff, gal, logn);   // (the source of roff + 1 is src ^ 1)
    const u64 soff = src & ~1u;
    const bool swap = (src & 1u) != 0;
    auto gather = [&](const u64 *row) {
        const u64x2 v = *reinterpret_cast<const u64x2 *>(row + soff);
        return swap ? u64x2{v.y, v.x} : v;
    };
    const u64 *wp = w + (((u64)b * ndigits) * jg + jj) * n;             // + i * jg * n per digit
    const u64 *kp0 = kp.k0 + (u64)j * n + roff, *kp1 = kp.k1 + (u64)j * n + roff;   // + i * lk * n per digit
    const u64 *xrow = xhat + (u64)b * xhat_poly_stride + (u64)j * n;
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
            const u64x2 xv = gather(i == j ? xrow : wp + (u64)i * jg * n);   // (stage A skips the own row: W[j][j] = c1 row j)
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
    const u64x2 a = gather(addend0 + (u64)b * addend_poly_stride + (u64)j * n);
    r0.x = add_mod(r0.x, a.x, md.p);
    r0.y = add_mod(r0.y, a.y, md.p);
    const u64 ooff = (u64)b * out_poly_stride + (u64)r * out_rot_stride + (u64)j * n + roff;
    *reinterpret_cast<u64x2 *>(out0 + ooff) = r0;
    *reinterpret_cast<u64x2 *>(out1 + ooff) = r1;
}

// hoist_matvec_kernel: the diagonal form of a plaintext matrix times an encrypted vector in ONE stage B -- hoist_mac_kernel's
// sum for every rotation of a group, each multiplied by its diagonal and summed in registers, so that no rotated
// ciphertext reaches memory:
//   out.c0[j] = pt0[j] c0[j] + sum_r pts_r[j] (sigma_r(c0[j]) + sum_i sigma_r(W[i][j]) gk_r.c0[i][j])
//   out.c1[j] = pt0[j] c1[j] + sum_r pts_r[j]                   sum_i sigma_r(W[i][j]) gk_r.c1[i][j]
// (mod q_j, canonical): word for word hoist_mac_kernel's outputs through dot_kernel, and like them not the reference's words.
// One block per (ciphertext b, key range (j, 256-lane chunk), rotation group g); it loops over the rotations
// [g rpg, min(nr, (g + 1) rpg)) of the launch.  Per rotation the digit loop is hoist_mac_kernel's unchanged; its canonical
// words (c0's with the gathered addend) times the lane's two words of pts_r go into a SECOND set of four 128-bit
// accumulators, folded every sixteen rotations: both factors are below 2^62, so sixteen products and a folded word
// stay below 2^128 -- the bound the digit loop rests on.  Group 0 of the call's first launch adds the identity diagonal
// pt0 (NULL: none) after the last fold: the destination lane's own words of c0 and c1, no gather.
// Group g writes polynomial pair b of `out0` / `out1` + g * out_group_stride: the result itself when the call has one
// group, else a partial sum that mbfv_sum_kernel adds up.
// Grid: hoist_mac_kernel's order with the rotation group in the rotation's place.  Ids 8 apart share a key range, so an XCD
// keeps to one eighth of the ranges; within a group of eight ranges the ciphertext runs fastest, then the rotation
// group.  The neighbours of a block on its XCD are the other ciphertexts under the SAME key range, and they walk the
// group's keys in step: a key slice comes from HBM once and from L2 for the other ciphertexts, while the nb x ndigits
// rows of W they gather from stay hot across all rotations.
__global__ void __launch_bounds__(256)
    hoist_matvec_kernel(const u64 *__restrict__ w, u64 *__restrict__ out0, u64 *__restrict__ out1, u64 out_poly_stride,
                        u64 out_group_stride, const u64 *__restrict__ ct0, const u64 *__restrict__ ct1, u64 ct_poly_stride,
                        const KsKeyPtr *__restrict__ keys, uint32_t rot0, HoistExps exps, const u64 *__restrict__ pts,
                        u64 pts_batch_stride, u64 pts_rot_stride, const u64 *__restrict__ pt0, u64 pt0_batch_stride,
                        const DevMod *__restrict__ mods, uint32_t ndigits, uint32_t lk, uint32_t j0, uint32_t jg,
                        uint32_t logn, uint32_t nb, uint32_t nr, uint32_t rpg, uint32_t ngroups) {
    const uint32_t n = 1u << logn;
    const uint32_t cpr = n >= 512 ? n / 512 : 1;          // 256-lane chunks per row
    const uint32_t nkr = jg * cpr;                        // key ranges of this launch
    const uint32_t grp = blockIdx.x >> 3, x8 = blockIdx.x & 7;
    const uint32_t per = nb * ngroups;
    const uint32_t krhi = grp / per, bg = grp - krhi * per;
    const uint32_t kr = krhi * 8 + x8;
    if (kr >= nkr) return;                                // (block-uniform) tail of the rounded-up grid
    const uint32_t g = bg / nb, b = bg - g * nb;          // (block-uniform) which rotation group of which ciphertext
    const uint32_t jj = kr / cpr, cb = kr - jj * cpr, j = j0 + jj;
    const uint32_t ci = cb * 256 + threadIdx.x;           // 16-byte chunk inside the row
    if (2 * ci >= n) return;
    const DevMod md = mods[j];
    const u64 roff = 2 * (u64)ci;
    const u64 *wp = w + (((u64)b * ndigits) * jg + jj) * n;             // + i * jg * n per digit
    const u64 *c0row = ct0 + (u64)b * ct_poly_stride + (u64)j * n;
    const u64 *c1row = ct1 + (u64)b * ct_poly_stride + (u64)j * n;      // (stage A skips the own row: W[j][j] = c1 row j)
    const u64 *prow = pts + (u64)b * pts_batch_stride + (u64)j * n + roff;   // + r * pts_rot_stride per rotation
    auto mac = [&](u128_t &acc, u64 x, u64 k) {
        u64 hi, lo;
        mul_wide62(x, k, hi, lo);
        acc += ((u128_t)hi << 64) | lo;
    };
    auto fold = [&](u128_t &acc) { acc = reduce_u128((u64)(acc >> 64), (u64)acc, md); };
    u128_t s0x = 0, s0y = 0, s1x = 0, s1y = 0;
    const uint32_t rlo = g * rpg, rhi = rlo + rpg < nr ? rlo + rpg : nr;
    for (uint32_t rr = rlo; rr < rhi; rr++) {
        const uint32_t r = to_sgpr(rr);
        const uint32_t gal = exps.e[r];
        const KsKeyPtr kp = keys[rot0 + r];
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
        const u64x2 pv = *reinterpret_cast<const u64x2 *>(prow + (u64)r * pts_rot_stride);
        if (rr != rlo && ((rr - rlo) & 15) == 0) fold(s0x), fold(s0y), fold(s1x), fold(s1y);
        mac(s0x, r0.x, pv.x);
        mac(s0y, r0.y, pv.y);
        mac(s1x, r1.x, pv.x);
        mac(s1y, r1.y, pv.y);
    }
    u64x2 o0, o1;
    o0.x = reduce_u128((u64)(s0x >> 64), (u64)s0x, md);
    o0.y = reduce_u128((u64)(s0y >> 64), (u64)s0y, md);
    o1.x = reduce_u128((u64)(s1x >> 64), (u64)s1x, md);
    o1.y = reduce_u128((u64)(s1y >> 64), (u64)s1y, md);
    if (pt0 != nullptr && g == 0) {
        const u64x2 pv = *reinterpret_cast<const u64x2 *>(pt0 + (u64)b * pt0_batch_stride + (u64)j * n + roff);
        const u64x2 x0 = *reinterpret_cast<const u64x2 *>(c0row + roff);
        const u64x2 x1 = *reinterpret_cast<const u64x2 *>(c1row + roff);
        o0.x = add_mod(o0.x, mul_mod(x0.x, pv.x, md), md.p);
        o0.y = add_mod(o0.y, mul_mod(x0.y, pv.y, md), md.p);
        o1.x = add_mod(o1.x, mul_mod(x1.x, pv.x, md), md.p);
        o1.y = add_mod(o1.y, mul_mod(x1.y, pv.y, md), md.p);
    }
    const u64 ooff = (u64)g * out_group_stride + (u64)b * out_poly_stride + (u64)j * n + roff;
    *reinterpret_cast<u64x2 *>(out0 + ooff) = o0;
    *reinterpret_cast<u64x2 *>(out1 + ooff) = o1;
}

}  // namespace k
}  // namespace fhe
