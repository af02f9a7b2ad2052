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
// F/bfv/ops/dot_product.rs:54-180) -- the same body, FHE_KS_MAC_SUM (kernels_ks.hpp).
// The one difference: (k0, k1) of polynomial b are entry ((poly0 + b) / per_key) % nkeys of `keys`, a table in device
// memory (a set may hold more keys than kernel arguments could); poly0 is the index, within the CALL, of this launch's
// first polynomial, so a chunk of polynomials need not end on a key boundary.  The index is block-uniform and goes
// through to_sgpr (as ksk_gen_kernel's out.k[key]): the entry is read with scalar loads and both pointers are scalars.
// Grid: ks_mac_kernel's -- polynomial fastest within a group of eight ranges -- although its purpose there (re-reading
// ONE key from an XCD's L2) holds here only among the per_key polynomials of a client: neighbouring blocks of one XCD
// still walk neighbouring polynomials, which are the ones that share a key, and the host computes one grid for both
// kernels.
__global__ void __launch_bounds__(256)
    ks_mac_keyed_kernel(const u64 *__restrict__ w, u64 *__restrict__ out0, u64 *__restrict__ out1, u64 out_poly_stride,
                        const u64 *__restrict__ addend0, const u64 *__restrict__ addend1, u64 addend_poly_stride,
                        const KsKeyPtr *__restrict__ keys, uint32_t nkeys, uint32_t per_key, uint32_t poly0,
                        const DevMod *__restrict__ mods, uint32_t ndigits, uint32_t lk, uint32_t j0, uint32_t jg,
                        uint32_t logn, const u64 *__restrict__ xhat, u64 xhat_poly_stride, uint32_t npolys, uint32_t gal) {
    KsMacAt at(logn, jg, npolys);
    if (at.kr >= at.nkr) return;                          // (block-uniform) tail of the rounded-up grid
    const uint32_t b = at.item;
    const uint32_t key = to_sgpr(((poly0 + b) / per_key) % nkeys);   // (block-uniform) whose polynomial this is
    at.lane(j0);
    if (2 * at.ci >= at.n) return;
    const KsKeyPtr kp = keys[key];
    FHE_KS_MAC_SUM(b, kp.k0, kp.k1)
}
#undef FHE_KS_MAC_SUM

}  // namespace k
}  // namespace fhe
