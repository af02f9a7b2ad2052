// kernels_mbfv.hpp -- the shares of the multiparty BFV protocols (eprint 2020/304; F/mbfv/) and their aggregation.
// Every share is one Poly::small draw, its forward transform and one or two pointwise products with a secret: the
// encryption kernels' pieces (kernels_encrypt.hpp) behind another epilogue.
//   mbfv_share_kernel       NTT(e) +- A (.) (X - X2) + w Y: PublicKeyShare::new          F/mbfv/public_key_gen.rs:32-57
//                           SecretKeySwitchShare / DecryptionShare::new                 F/mbfv/secret_key_switch.rs:38-95, 133-142
//                           RelinKeyShare<R1> / <R2>::new                                F/mbfv/relin_key_gen.rs:141-197, 243-296
//   mbfv_share_ew_kernel    the same epilogue as an element-wise pass, for rows larger than one LDS tile (N >= 32768)
//   mbfv_mul_ew_kernel      s (.) c1, the addend of PublicKeySwitchShare::new            F/mbfv/public_key_switch.rs:70-75
//   mbfv_sum_kernel         base + the sum of P parties' shares (every Aggregate::from_shares of F/mbfv/)
// The samples and X, X2, Y are secrets: no branch or address below depends on them, only on indices, the form and the
// moduli (the sign is a launch argument; the sums and differences are the branch-free add_mod / sub_mod).
#pragma once
#include "kernels_keygen.hpp"

namespace fhe {
namespace k {

// What a share adds to its transformed error, beyond sign A (.) X
enum : int {
    MBFV_AX = 0,     // e +- A (.) X                   (public-key, decryption, round-1 h1, round-2 h0 shares)
    MBFV_AXX = 1,    // e +- A (.) (X - X2)            (secret-key switch, round-2 h1)
    MBFV_AX_WY = 2,  // e +- A (.) X + w[k][r] Y       (round-1 h0: w = the Garner scalars of ksk_consts_kernel)
};

// The operands of one launch.  Draw kk of item b is e[(b edraws + e0 + kk) N]: a call's 2L relin draws serve two
// launches (e0 = 0 and e0 = L).  A is public, [k][rows][N] per item at a_stride words (0: one for the batch); X, X2, Y
// are [rows][N] per item at s_stride words (0: one party serves the batch).
struct MbfvArgs {
    const int8_t *e;
    const u64 *A, *X, *X2, *Y, *w;
    u64 a_stride, s_stride;
    uint32_t edraws, e0, k, rows, neg;
};

template <int FORM>
__device__ __forceinline__ u64 mbfv_combine(u64 x, u64 a, u64 s, u64 s2, u64 y, u64 w, uint32_t neg, const DevMod &md) {
    if constexpr (FORM == MBFV_AXX) s = sub_mod(s, s2, md.p);
    const u64 t = mul_mod(a, s, md);
    u64 c = neg ? sub_mod(x, t, md.p) : add_mod(x, t, md.p);   // (neg: a launch argument, uniform)
    if constexpr (FORM == MBFV_AX_WY) c = add_mod(c, mul_mod(w, y, md), md.p);
    return c;
}

// One workgroup per (item, draw kk, row r): out[b][kk][r] = NTT(e_{b,kk})[r] +- A[b][kk][r] (.) (X[b][r] - X2[b][r])
// + w[kk][r] Y[b][r].  The transformed error row stays in the LDS tile; X2 and the w Y term are compile-time (FORM), so
// the two-operand form loads and multiplies nothing more than encrypt_sk_kernel does.  (All three forms hold at most
// four 16-byte operands a pair beside the tile and compile without scratch at every tile size, 16384 points included.)
template <int LOGM, bool NARROW = false, int F64 = 0, int FORM = MBFV_AX>
__global__ void __launch_bounds__(ntt_threads_c(LOGM), 4)
    mbfv_share_kernel(MbfvArgs g, u64 *__restrict__ out, const DevMod *__restrict__ mods, const u64x2 *__restrict__ tw) {
    FHE_DYN_SMEM(u64, lds);
    constexpr int T = ntt_threads_c(LOGM);
    constexpr int M = 1 << LOGM;
    const uint32_t tid = threadIdx.x;
    const uint32_t bk = to_sgpr(blockIdx.x / g.rows);   // item * k + draw
    const uint32_t r = blockIdx.x - bk * g.rows;
    const uint32_t b = to_sgpr(bk / g.k), kk = bk - b * g.k;
    const DevMod md = mods[r];
    const u64 ro = (u64)r * M;
    const u64x2 *ar = reinterpret_cast<const u64x2 *>(g.A + (u64)b * g.a_stride + ((u64)kk * g.rows + r) * M);
    const u64x2 *xr = reinterpret_cast<const u64x2 *>(g.X + (u64)b * g.s_stride + ro);
    const u64x2 *x2r = FORM == MBFV_AXX ? reinterpret_cast<const u64x2 *>(g.X2 + (u64)b * g.s_stride + ro) : nullptr;
    const u64x2 *yr = FORM == MBFV_AX_WY ? reinterpret_cast<const u64x2 *>(g.Y + (u64)b * g.s_stride + ro) : nullptr;
    const u64 w = FORM == MBFV_AX_WY ? g.w[kk * g.rows + r] : 0;
    const uint32_t neg = g.neg;
    u64x2 *o = reinterpret_cast<u64x2 *>(out + ((u64)bk * g.rows + r) * M);
    const int8_t *src = g.e + ((u64)b * g.edraws + g.e0 + kk) * M;
    small_row_ntt<LOGM, T, NARROW, F64>(lds, tw + ro, md, tid, src, [&](uint32_t i, u64 x, u64 y) {
        const u64x2 av = ar[i >> 1], sv = xr[i >> 1];
        u64x2 s2{0, 0}, yv{0, 0};
        if constexpr (FORM == MBFV_AXX) s2 = x2r[i >> 1];
        if constexpr (FORM == MBFV_AX_WY) yv = yr[i >> 1];
        o[i >> 1] = u64x2{mbfv_combine<FORM>(x, av.x, sv.x, s2.x, yv.x, w, neg, md),
                          mbfv_combine<FORM>(y, av.y, sv.y, s2.y, yv.y, w, neg, md)};
    });
}

// mbfv_share_kernel's epilogue as an element-wise pass over the transformed draws x [batch][edraws][rows][N] (rows
// larger than one LDS tile; g.e is not read: the caller lifted and transformed every draw).  `form` is uniform.
// total = batch * k * rows * 2^logn.
__global__ void mbfv_share_ew_kernel(const u64 *__restrict__ x, MbfvArgs g, uint32_t form, u64 *__restrict__ out,
                                     const DevMod *__restrict__ mods, uint32_t logn, u64 total) {
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const u64 row = gid >> logn, j = gid & ((1ull << logn) - 1);
    const u64 bk = row / g.rows;
    const uint32_t r = (uint32_t)(row - bk * g.rows);
    const u64 b = bk / g.k;
    const uint32_t kk = (uint32_t)(bk - b * g.k);
    const DevMod md = mods[r];
    const u64 so = b * g.s_stride + ((u64)r << logn) + j;
    const u64 a = g.A[b * g.a_stride + ((((u64)kk * g.rows + r)) << logn) + j];
    const u64 s = g.X[so];
    const u64 xv = x[((((b * g.edraws + g.e0 + kk) * g.rows) + r) << logn) + j];
    if (form == MBFV_AXX) out[gid] = mbfv_combine<MBFV_AXX>(xv, a, s, g.X2[so], 0, 0, g.neg, md);
    else if (form == MBFV_AX_WY) out[gid] = mbfv_combine<MBFV_AX_WY>(xv, a, s, 0, g.Y[so], g.w[kk * g.rows + r], g.neg, md);
    else out[gid] = mbfv_combine<MBFV_AX>(xv, a, s, 0, 0, 0, g.neg, md);
}

// out[b][r] = s[b][r] (.) c1[b][r]: s at s_stride, c1 at c_stride words per item (0: shared); out [batch][rows][N].
// total = batch * rows * 2^logn.
__global__ void mbfv_mul_ew_kernel(const u64 *__restrict__ s, u64 s_stride, const u64 *__restrict__ c1, u64 c_stride,
                                   u64 *__restrict__ out, uint32_t rows, const DevMod *__restrict__ mods, uint32_t logn,
                                   u64 total) {
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const u64 pl = (u64)rows << logn;
    const u64 b = gid / pl, off = gid - b * pl;
    out[gid] = mul_mod(s[b * s_stride + off], c1[b * c_stride + off], mods[off >> logn]);
}

// The aggregator: out[j][i] = (base ? base[j][i] : 0) + sum_{p < nshares} shares[p share_stride + j rows N + i] mod
// q_row(i) over npolys polynomials of [rows][N] words.  grid = (ceil(rows N / 2 / block), npolys): blockIdx.y is the
// polynomial j, a thread owns two words (16 bytes) of it, so no index needs a division.  Polynomial j of base starts
// at word j base_stride (a ciphertext's c0 parts: 2 rows N), polynomial j of a share and of out at j rows N.  Inputs
// are canonical residues of moduli below 2^62, so a canonical accumulator takes three addends before it is reduced:
// acc < q + 3 (q - 1) < 4 q < 2^64, and two conditional subtractions (2q, q) make it canonical again.  out == base is
// allowed (a thread reads its own two words before it writes them).  pairs = rows * N / 2.
constexpr int MBFV_SUM_LAZY = 3;
__global__ void mbfv_sum_kernel(const u64 *shares, uint32_t nshares, u64 share_stride, const u64 *base, u64 base_stride,
                                u64 *out, const DevMod *__restrict__ mods, uint32_t logn, uint32_t pairs) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= pairs) return;
    const u64 off = 2ull * gid, po = (u64)blockIdx.y * 2 * pairs + off;
    const u64 q = mods[off >> logn].p, q2 = q << 1;
    u64x2 acc{0, 0};
    if (base) acc = *reinterpret_cast<const u64x2 *>(base + (u64)blockIdx.y * base_stride + off);
    const u64 *sp = shares + po;
    for (uint32_t p0 = 0; p0 < nshares; p0 += MBFV_SUM_LAZY) {
        const uint32_t p1 = p0 + MBFV_SUM_LAZY < nshares ? p0 + MBFV_SUM_LAZY : nshares;
        for (uint32_t p = p0; p < p1; p++) {
            const u64x2 v = *reinterpret_cast<const u64x2 *>(sp + (u64)p * share_stride);
            acc.x += v.x;
            acc.y += v.y;
        }
        acc.x = csub(csub(acc.x, q2), q);
        acc.y = csub(csub(acc.y, q2), q);
    }
    *reinterpret_cast<u64x2 *>(out + po) = acc;
}

}  // namespace k
}  // namespace fhe
