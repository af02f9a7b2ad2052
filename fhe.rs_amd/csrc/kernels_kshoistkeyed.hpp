// kernels_kshoistkeyed.hpp -- stage B of the hoisted rotations and of the hoisted matrix-vector product with ONE GALOIS KEY
// SET PER CLIENT (keyed batches x hoisting).  A server multiplies its plaintext matrix by each client's encrypted
// vector, every client under their own keys: stage A (ks_ntt_kernel, kernels_ks.hpp) reads no key, so one launch
// transforms every client's digit rows as it does for the single-client calls, and only the multiply-accumulates below
// have to know whose ciphertext they are working on.
//
// The key table is CLIENT-MAJOR: entry c * nrot + r is client c's key for rotation r of the call.  Ciphertext b of a
// launch whose first ciphertext has index item0 within the CALL belongs to client ((item0 + b) / per_client) % nclients
// (ks_mac_keyed_kernel's rule with poly0), so a chunk cut by the W budget need not end on a client boundary.  The index
// is block-uniform and goes through to_sgpr: the entry is read with scalar loads, both key pointers are scalars.
//
// The specification is one single-client call (hoist_mac_kernel / hoist_matvec_kernel, kernels_kshoist.hpp) per client
// on that client's keys and slice of the batch, word for word; the caveat NOT the reference's words is inherited.
// These are the last users of the shared macro bodies of kernels_ksmac.hpp, which are undefined at the end.
#pragma once
#include "kernels_bsgs.hpp"

namespace fhe {
namespace k {

// (block-uniform) entry of the client-major key table for ciphertext `item` of the call and rotation `rot` of the set
__device__ __forceinline__ uint32_t hoist_keyed_entry(uint32_t item, uint32_t per_client, uint32_t nclients, uint32_t nrot,
                                                      uint32_t rot) {
    return ((item / per_client) % nclients) * nrot + rot;
}

// hoist_mac_keyed_kernel: hoist_mac_kernel's sum -- the same coordinates, accumulator quad, digit loop and gather -- with
// the key of output (b, r) taken from entry (((item0 + b) / per_client) % nclients) * nrot + rot0 + r of `keys`.
// Grid: within a group of eight key ranges the ROTATION runs fastest, then the ciphertext (hoist_mac_kernel: the other
// way round).  The unkeyed order puts the ciphertext fastest because neighbouring ciphertexts share a key slice; under
// one key set per client they share nothing at one ciphertext per client.  Argued from the cache sizes, NOT measured
// here (tools/bench_hoisted_keyed.py times this order against the unkeyed one at nclients = 1; STATE.md has the table):
//  * the neighbours of a block on its XCD are the rotations of ONE ciphertext, which gather from the same ndigits rows of
//    W: 256 KiB per key modulus at N = 8192 x 4 moduli, inside the 4 MiB L2;
//  * every key slice is read once either way;
//  * with several ciphertexts per client a key slice is read again nr blocks later: nr x 32 KiB per range at four
//    digits (2 MiB at 64 rotations), still within L2.
__global__ void __launch_bounds__(256)
    hoist_mac_keyed_kernel(const u64 *__restrict__ w, u64 *__restrict__ out0, u64 *__restrict__ out1, u64 out_poly_stride,
                           u64 out_rot_stride, const u64 *__restrict__ addend0, u64 addend_poly_stride,
                           const KsKeyPtr *__restrict__ keys, uint32_t item0, uint32_t per_client, uint32_t nclients,
                           uint32_t nrot, uint32_t rot0, HoistExps exps, const DevMod *__restrict__ mods, uint32_t ndigits,
                           uint32_t lk, uint32_t j0, uint32_t jg, uint32_t logn, const u64 *__restrict__ xhat,
                           u64 xhat_poly_stride, uint32_t nb, uint32_t nr) {
    KsMacAt at(logn, jg, nr, nb);                         // (nr x nb items: the rotation fastest)
    if (at.kr >= at.nkr) return;                          // (block-uniform) tail of the rounded-up grid
    const uint32_t b = to_sgpr(at.item / nr), r = to_sgpr(at.item - b * nr);   // (block-uniform) which rotation of which ciphertext
    const uint32_t key = to_sgpr(hoist_keyed_entry(item0 + b, per_client, nclients, nrot, rot0 + r));   // whose ciphertext this is
    at.lane(j0);
    if (2 * at.ci >= at.n) return;
    const uint32_t n = at.n, j = at.j;
    const uint32_t gal = exps.e[r];
    const KsKeyPtr kp = keys[key];
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

// hoist_matvec_keyed_kernel: hoist_matvec_kernel with that key lookup -- the same grid order (ciphertext fastest, then the
// rotation group: a block walks every rotation of its group, so there is no rotation to put first), the same second
// accumulator quad folded every sixteen rotations, the same identity diagonal in group 0 of the call's first launch.
// The client's first entry is found once per block; rotation r of the launch reads entry base + r.
__global__ void __launch_bounds__(256)
    hoist_matvec_keyed_kernel(const u64 *__restrict__ w, u64 *__restrict__ out0, u64 *__restrict__ out1, u64 out_poly_stride,
                              u64 out_group_stride, const u64 *__restrict__ ct0, const u64 *__restrict__ ct1,
                              u64 ct_poly_stride, const KsKeyPtr *__restrict__ keys, uint32_t item0, uint32_t per_client,
                              uint32_t nclients, uint32_t nrot, uint32_t rot0, HoistExps exps, const u64 *__restrict__ pts,
                              u64 pts_batch_stride, u64 pts_rot_stride, const u64 *__restrict__ pt0, u64 pt0_batch_stride,
                              const DevMod *__restrict__ mods, uint32_t ndigits, uint32_t lk, uint32_t j0, uint32_t jg,
                              uint32_t logn, uint32_t nb, uint32_t nr, uint32_t rpg, uint32_t ngroups) {
    KsMacAt at(logn, jg, nb, ngroups);
    if (at.kr >= at.nkr) return;                          // (block-uniform) tail of the rounded-up grid
    const uint32_t g = at.item / nb, b = at.item - g * nb;   // (block-uniform) which rotation group of which ciphertext
    const uint32_t base = to_sgpr(hoist_keyed_entry(item0 + b, per_client, nclients, nrot, rot0));   // whose ciphertext this is
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
        const KsKeyPtr kp = keys[base + r];
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

#undef FHE_KS_DIGIT_LOOP
#undef FHE_KS_IDENTITY_DIAG

}  // namespace k
}  // namespace fhe
