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

// hoist_mac_kernel: ks_mac_keyed_kernel's sum for nb ciphertexts x nr rotations, on the shared pieces of
// kernels_ksmac.hpp (coordinates, accumulator quad, digit loop, gather); canonical outputs.
// What differs: output (b, r) reads W of ciphertext b and key rot0 + r of `keys` (block-uniform, through to_sgpr: both
// key pointers and the exponent are scalars), and EVERY operand but the key is read through the gather of exponent
// exps.e[r] (KsMacGather) -- the own row from `xhat` (the caller's unpermuted c1), the addend from `addend0` (c0).
// W is read once per rotation: cached loads (ks_mac_keyed_kernel streams it).  The key words are read once per ciphertext.
// Grid: within a group of eight ranges the ciphertext runs fastest, then the rotation: the neighbours of a block on its XCD
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
    KsMacAt at(logn, jg, nb, nr);
    if (at.kr >= at.nkr) return;                          // (block-uniform) tail of the rounded-up grid
    const uint32_t r = to_sgpr(at.item / nb), b = at.item - r * nb;   // (block-uniform) which rotation of which ciphertext
    at.lane(j0);
    if (2 * at.ci >= at.n) return;
    const uint32_t n = at.n, j = at.j;
    const uint32_t gal = exps.e[r];
    const KsKeyPtr kp = keys[rot0 + r];
    const DevMod md = mods[j];
    const u64 roff = at.roff();
    const KsMacGather gather(roff, gal, logn);
    const u64 *wp = w + (((u64)b * ndigits) * jg + at.jj) * n;          // + i * jg * n per digit
    const u64 *kp0 = kp.k0 + (u64)j * n + roff, *kp1 = kp.k1 + (u64)j * n + roff;   // + i * lk * n per digit
    const u64 *xrow = xhat + (u64)b * xhat_poly_stride + (u64)j * n;    // (stage A skips the own row: W[j][j] = c1 row j)
    KsMacQuad acc;
    FHE_KS_DIGIT_LOOP(acc, ndigits, md, kp0, kp1, lk, n, xv = gather(i == j ? xrow : wp + (u64)i * jg * n))
    u64x2 r0, r1;
    acc.reduce(md, r0, r1);
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
// [g rpg, min(nr, (g + 1) rpg)) of the launch.  Per rotation the digit loop is hoist_mac_kernel's; its canonical words
// (c0's with the gathered addend) times the lane's two words of pts_r go into a SECOND accumulator quad, folded every
// sixteen rotations (KsMacQuad's bound: both factors are below 2^62).  Group 0 of the call's first launch adds the
// identity diagonal pt0 (NULL: none) after the last fold (FHE_KS_IDENTITY_DIAG).
// Group g writes polynomial pair b of `out0` / `out1` + g * out_group_stride: the result itself when the call has one
// group, else a partial sum that mbfv_sum_kernel adds up.
// Grid: hoist_mac_kernel's order with the rotation group in the rotation's place: the neighbours of a block on its XCD
// are the other ciphertexts under the SAME key range, and they walk the group's keys in step: a key slice comes from
// HBM once and from L2 for the other ciphertexts, while the nb x ndigits rows of W they gather from stay hot across
// all rotations.
__global__ void __launch_bounds__(256)
    hoist_matvec_kernel(const u64 *__restrict__ w, u64 *__restrict__ out0, u64 *__restrict__ out1, u64 out_poly_stride,
                        u64 out_group_stride, const u64 *__restrict__ ct0, const u64 *__restrict__ ct1, u64 ct_poly_stride,
                        const KsKeyPtr *__restrict__ keys, uint32_t rot0, HoistExps exps, const u64 *__restrict__ pts,
                        u64 pts_batch_stride, u64 pts_rot_stride, const u64 *__restrict__ pt0, u64 pt0_batch_stride,
                        const DevMod *__restrict__ mods, uint32_t ndigits, uint32_t lk, uint32_t j0, uint32_t jg,
                        uint32_t logn, uint32_t nb, uint32_t nr, uint32_t rpg, uint32_t ngroups) {
    KsMacAt at(logn, jg, nb, ngroups);
    if (at.kr >= at.nkr) return;                          // (block-uniform) tail of the rounded-up grid
    const uint32_t g = at.item / nb, b = at.item - g * nb;   // (block-uniform) which rotation group of which ciphertext
    at.lane(j0);
    if (2 * at.ci >= at.n) return;
    const uint32_t n = at.n, j = at.j;
    const DevMod md = mods[j];
    const u64 roff = at.roff();
    const u64 *wp = w + (((u64)b * ndigits) * jg + at.jj) * n;          // + i * jg * n per digit
    const u64 *c0row = ct0 + (u64)b * ct_poly_stride + (u64)j * n;
    const u64 *c1row = ct1 + (u64)b * ct_poly_stride + (u64)j * n;      // (stage A skips the own row: W[j][j] = c1 row j)
    const u64 *prow = pts + (u64)b * pts_batch_stride + (u64)j * n + roff;   // + r * pts_rot_stride per rotation
    KsMacQuad sum;
    const uint32_t rlo = g * rpg, rhi = rlo + rpg < nr ? rlo + rpg : nr;
    for (uint32_t rr = rlo; rr < rhi; rr++) {
        const uint32_t r = to_sgpr(rr);
        const uint32_t gal = exps.e[r];
        const KsKeyPtr kp = keys[rot0 + r];
        const KsMacGather gather(roff, gal, logn);
        const u64 *kp0 = kp.k0 + (u64)j * n + roff, *kp1 = kp.k1 + (u64)j * n + roff;   // + i * lk * n per digit
        KsMacQuad acc;
        FHE_KS_DIGIT_LOOP(acc, ndigits, md, kp0, kp1, lk, n, xv = gather(i == j ? c1row : wp + (u64)i * jg * n))
        u64x2 r0, r1;
        acc.reduce(md, r0, r1);
        const u64x2 a = gather(c0row);
        r0.x = add_mod(r0.x, a.x, md.p);
        r0.y = add_mod(r0.y, a.y, md.p);
        const u64x2 pv = *reinterpret_cast<const u64x2 *>(prow + (u64)r * pts_rot_stride);
        if (rr != rlo && ((rr - rlo) & 15) == 0) sum.fold(md);
        sum.mac(r0, pv, r1, pv);
    }
    u64x2 o0, o1;
    sum.reduce(md, o0, o1);
    if (pt0 != nullptr && g == 0) {
        const u64x2 pv = *reinterpret_cast<const u64x2 *>(pt0 + (u64)b * pt0_batch_stride + (u64)j * n + roff);
        const u64x2 x0 = *reinterpret_cast<const u64x2 *>(c0row + roff);
        const u64x2 x1 = *reinterpret_cast<const u64x2 *>(c1row + roff);
        FHE_KS_IDENTITY_DIAG(o0, o1, x0, x1, pv, md)
    }
    const u64 ooff = (u64)g * out_group_stride + (u64)b * out_poly_stride + (u64)j * n + roff;
    *reinterpret_cast<u64x2 *>(out0 + ooff) = o0;
    *reinterpret_cast<u64x2 *>(out1 + ooff) = o1;
}

}  // namespace k
}  // namespace fhe
