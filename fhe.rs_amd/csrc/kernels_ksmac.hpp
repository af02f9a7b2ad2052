// kernels_ksmac.hpp -- what the stage B kernels of the unfused key switch share, each piece stated once: ks_mac_kernel
// (kernels_ks.hpp), ks_mac_keyed_kernel (kernels_kskeyed.hpp), hoist_mac_kernel and hoist_matvec_kernel
// (kernels_kshoist.hpp), bsgs_baby_kernel<GT> and bsgs_giant_kernel (kernels_bsgs.hpp), hoist_mac_keyed_kernel and
// hoist_matvec_keyed_kernel (kernels_kshoistkeyed.hpp).  All of them form
//   sum_i x_i[j] (.) (k0, k1)[i][j]   (x_i: row (i, j) of W, or the caller's Ntt row where i == j)
// with one lane per 16-byte chunk of an output row under key modulus j; they differ in where the key, the digit words
// and the result come from and go to.  Included from kernels_ks.hpp.
#pragma once
#include "kernels_passes.hpp"

namespace fhe {
namespace k {

// 256-lane chunks per row of n words (host and device: the grid, the group rules and the kernels agree on it).
FHE_HD uint32_t ks_mac_chunks_per_row(u64 n) { return n >= 512 ? (uint32_t)(n / 512) : 1u; }

// Where a block and a lane of a stage B grid stand.  The grid is (key range, item) in an XCD-aware order: a key range
// is (key modulus jj of the launch's jg, 256-lane chunk of its row); the lanes of a block read ndigits * 2 * 4 KiB of
// key words that other items of the launch need again, so the blocks of one key range get ids 8 apart (same XCD,
// dispatched back to back: the re-reads hit that L2, and an XCD keeps to one eighth of the ranges).  Within a group of
// eight ranges the `per` items of the launch follow each other; `item` is that index, which each kernel splits its own
// way (polynomial; ciphertext fastest, then rotation, rotation group, giant tile or giant group).
// The grid is rounded up to eights of ranges.  A kernel takes its coordinates in two steps, in this order, because the
// order of the statements is what the compiler schedules: the constructor gives the block's part and the kernel
// returns on `kr >= nkr` (block-uniform), splits `item`, then lane(j0) gives the rest and the kernel returns on
// `2 * ci >= n` (lanes past a row shorter than 512 words).  Two returns: as one test they cost registers.
struct KsMacAt {
    uint32_t n, cpr, nkr, kr, item;   // row length, chunks per row, key ranges of this launch, this block's range and item
    uint32_t jj, j, ci;               // key modulus within the launch and in the key, 16-byte chunk inside the row
    // (nb x m items: nb polynomials or ciphertexts, fastest, times m of whatever else the kernel's grid runs over)
    __device__ __forceinline__ KsMacAt(uint32_t logn, uint32_t jg, uint32_t nb, uint32_t m = 1) {
        n = 1u << logn;
        cpr = ks_mac_chunks_per_row(n);
        nkr = jg * cpr;
        const uint32_t grp = blockIdx.x >> 3, x8 = blockIdx.x & 7;
        const uint32_t per = nb * m;
        const uint32_t krhi = grp / per;
        item = grp - krhi * per;
        kr = krhi * 8 + x8;
    }
    __device__ __forceinline__ void lane(uint32_t j0) {
        jj = kr / cpr;
        const uint32_t cb = kr - jj * cpr;
        j = j0 + jj;
        ci = cb * 256 + threadIdx.x;
    }
    __device__ __forceinline__ u64 roff() const { return 2 * (u64)ci; }   // the lane's first word inside the row
};

// The four lazy 128-bit accumulators of a lane: parts 0 and 1 of the lane's two words.  mac adds x0 (.) k0 to part 0
// and x1 (.) k1 to part 1 (mul_wide62: factors below 2^62, products below 2^124); fold reduces each accumulator to a
// canonical word.  THE BOUND: a window between two folds holds one folded word (below 2^62) and at most sixteen
// products below (2^62 - 1)^2 -- 2^128 - 2^67 + 16 + 2^62 < 2^128 -- so whoever accumulates folds before every
// seventeenth product.
struct KsMacQuad {
    u128_t a0x = 0, a0y = 0, a1x = 0, a1y = 0;
    static __device__ __forceinline__ void mac1(u128_t &acc, u64 x, u64 k) {
        u64 hi, lo;
        mul_wide62(x, k, hi, lo);
        acc += ((u128_t)hi << 64) | lo;
    }
    static __device__ __forceinline__ u64 red1(u128_t acc, const DevMod &md) { return reduce_u128((u64)(acc >> 64), (u64)acc, md); }
    __device__ __forceinline__ void mac(u64x2 x0, u64x2 k0, u64x2 x1, u64x2 k1) {
        mac1(a0x, x0.x, k0.x);
        mac1(a0y, x0.y, k0.y);
        mac1(a1x, x1.x, k1.x);
        mac1(a1y, x1.y, k1.y);
    }
    __device__ __forceinline__ void fold(const DevMod &md) {
        a0x = red1(a0x, md), a0y = red1(a0y, md), a1x = red1(a1x, md), a1y = red1(a1y, md);
    }
    __device__ __forceinline__ void reduce(const DevMod &md, u64x2 &r0, u64x2 &r1) const {
        r0.x = red1(a0x, md);
        r0.y = red1(a0y, md);
        r1.x = red1(a1x, md);
        r1.y = red1(a1y, md);
    }
};

// The digit loop: acc += sum_{i < ndigits} xv(i) (.) (kp0, kp1)[i * lk * n], in windows of sixteen digits with a fold
// between them (the bound above; an accumulator that enters with more than a folded word states its own).  X is a
// statement that assigns the lane's two words of digit `i` to `xv`: a streaming load of W or the own row (ks_mac_kernel,
// ks_mac_keyed_kernel), or a cached gathered load with the own row from c1 (the other four).  A macro body, as
// FHE_GARNER_HORNER is: as a function template over the loader the loop costs instructions and registers (hoist_mac_kernel:
// 1160 against 1145 instructions, 86 against 79 VGPRs), and even a lambda for X moves ks_mac_kernel's code.  Undefined
// after its last use (kernels_kshoistkeyed.hpp).
#define FHE_KS_DIGIT_LOOP(acc, ndigits, md, kp0, kp1, lk, n, X)                                            \
    for (uint32_t i0 = 0; i0 < (ndigits); i0 += 16) {                                                      \
        const uint32_t i1 = i0 + 16 < (ndigits) ? i0 + 16 : (ndigits);                                     \
        if (i0) (acc).fold(md);                                                                            \
        _Pragma("unroll 4") for (uint32_t i = i0; i < i1; i++) {                                           \
            u64x2 xv;                                                                                      \
            X;                                                                                             \
            const u64x2 q0 = *reinterpret_cast<const u64x2 *>((kp0) + (u64)i * (lk) * (n));                 \
            const u64x2 q1 = *reinterpret_cast<const u64x2 *>((kp1) + (u64)i * (lk) * (n));                 \
            (acc).mac(xv, q0, xv, q1);                                                                     \
        }                                                                                                  \
    }

// The Ntt-domain substitution x -> x^e read as a gather of a lane's two words (destination words roff, roff + 1 of a
// row; roff even).  The two stay neighbours under it: e is odd, so destination roff + 1 adds N/2 to the index before
// the last bit reversal, which flips bit 0 of the source -- one 16-byte load at the even source and a swap.  For
// destinations that differ only in their low k bits the sources are a permutation of one aligned block of 2^k words,
// so a wave's 128 destination words read one aligned 1 KiB block of the source row.
struct KsMacGather {
    u64 soff;
    bool swap;
    __device__ __forceinline__ KsMacGather(u64 roff, uint32_t e, uint32_t logn) {
        const uint32_t src = galois_src_index((uint32_t)roff, e, logn);   // (the source of roff + 1 is src ^ 1)
        soff = src & ~1u;
        swap = (src & 1u) != 0;
    }
    __device__ __forceinline__ u64x2 operator()(const u64 *row) const {
        const u64x2 v = *reinterpret_cast<const u64x2 *>(row + soff);
        return swap ? u64x2{v.y, v.x} : v;
    }
};

// The identity diagonal of a matrix-vector product: (o0, o1) += (x0, x1) (.) pv, the lane's own words of c0 / c1 times
// its diagonal words (no gather, no key), canonical.  A macro body like the digit loop, and undefined with it: as a
// function (by reference or by value) it changes the code of bsgs_baby_kernel<2> and <4>.
#define FHE_KS_IDENTITY_DIAG(o0, o1, x0, x1, pv, md)                                                       \
    (o0).x = add_mod((o0).x, mul_mod((x0).x, (pv).x, md), (md).p);                                         \
    (o0).y = add_mod((o0).y, mul_mod((x0).y, (pv).y, md), (md).p);                                         \
    (o1).x = add_mod((o1).x, mul_mod((x1).x, (pv).x, md), (md).p);                                         \
    (o1).y = add_mod((o1).y, mul_mod((x1).y, (pv).y, md), (md).p);

}  // namespace k
}  // namespace fhe
