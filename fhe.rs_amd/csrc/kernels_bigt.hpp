// kernels_bigt.hpp -- plaintext moduli of more than 64 bits (PlaintextModulus::Large: BfvParametersBuilder::
// set_plaintext_modulus_biguint, F/bfv/parameters.rs:560-738).  t has WT = ceil(bits(t) / 64) limbs, WT = 2, 3 or 4
// (t below 2^256); every value modulo t lives in WT registers of the thread that owns its coefficient:
//   bigt_project_kernel<WT>   Vec<BigUint> -> Plaintext::poly_ntt / to_poly before the transform: the value reduced
//                             modulo t, times q_mod_t modulo t when scaled, then its residue modulo every q_i (times
//                             delta_i when scaled)          F/bfv/plaintext_vec.rs:105-132, plaintext.rs:172-197
//   bigt_tail_kernel<P, WT>   the Large branch of SecretKey::try_decrypt and Plaintext::from_shares: the CRT lift x of
//                             the P plaintext-context residues, then ((x + t) mod Q_p) mod t   F/bfv/keys/secret_key.rs:238-250
// The encoder takes v reduced modulo t first, as the u64 encoder does; the result equals the reference's bit for bit
// whenever v < t (the reference does not reduce: a value of t or more gives it residues of v itself).
// delta_i is a constant of the row, so NTT(m' mod q_i) delta_i = NTT((m' mod q_i) delta_i): the projection applies it
// and the rows then go through the plain forward transform.
// Reduction modulo t is Barrett's multi-word method (HAC 14.42, base b = 2^64, k = WT, mu = floor(b^2k / t)): for
// x < b^2k, q3 = floor(floor(x / b^(k-1)) mu / b^(k+1)) is floor(x / t) or up to two less, so
// (x - q3 t) mod b^(k+1) < 3t and two conditional subtractions finish.  mu has k + 2 limbs: the top one is 1 only for
// t = b^(k-1) itself.  The values are plaintext coefficients: selects only, no branch or address depends on them.
#pragma once
#include "kernels_noise.hpp"

namespace fhe {
namespace k {

constexpr int BIGT_THREADS = 256;
constexpr int BIGT_WMAX = 4;

template <int WT>
struct BigT {
    u64 t[WT];
    u64 mu[WT + 2];
};
template <int WT>
struct BigVal {
    u64 w[WT];
};

// acc + a b + carry -> {acc, carry}; the sum is below 2^128
FHE_HD void bigt_mac(u64 &acc, u64 a, u64 b, u64 &carry) {
    const u64 hi = mulhi64(a, b), lo = a * b;
    const u64 s = acc + lo;
    const u64 s2 = s + carry;
    carry = hi + (s < lo ? 1 : 0) + (s2 < carry ? 1 : 0);
    acc = s2;
}

// r = x mod t for x[2 WT] below 2^(128 WT)
template <int WT>
FHE_HD void bigt_reduce(const u64 *x, const BigT<WT> &bt, u64 *r) {
    constexpr int K = WT;
    u64 q2[2 * K + 3];
#pragma unroll
    for (int i = 0; i < 2 * K + 3; i++) q2[i] = 0;
    // q2 = floor(x / b^(K-1)) mu: (K + 1) x (K + 2) limbs
#pragma unroll
    for (int i = 0; i <= K; i++) {
        u64 carry = 0;
#pragma unroll
        for (int j = 0; j < K + 2; j++) bigt_mac(q2[i + j], x[K - 1 + i], bt.mu[j], carry);
        q2[i + K + 2] = carry;
    }
    // rr = (x - q3 t) mod b^(K+1), q3 = q2 / b^(K+1) (below b^(K+1): x / t < b^(K+1))
    u64 p[K + 1];
#pragma unroll
    for (int i = 0; i <= K; i++) p[i] = 0;
#pragma unroll
    for (int i = 0; i <= K; i++) {
        u64 carry = 0;
#pragma unroll
        for (int j = 0; j < K; j++)
            if (i + j <= K) bigt_mac(p[i + j], q2[K + 1 + i], bt.t[j], carry);
        if (i + K <= K) p[i + K] += carry;
    }
    u64 rr[K + 1];
    u64 borrow = 0;
#pragma unroll
    for (int i = 0; i <= K; i++) {
        const u64 d = x[i] - p[i], e = d - borrow;
        borrow = (x[i] < p[i] ? 1 : 0) | (d < borrow ? 1 : 0);
        rr[i] = e;
    }
    // rr < 3t: twice rr -= t where rr >= t
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        u64 s[K + 1];
        borrow = 0;
#pragma unroll
        for (int i = 0; i <= K; i++) {
            const u64 ti = i < K ? bt.t[i] : 0;
            const u64 d = rr[i] - ti, e = d - borrow;
            borrow = (rr[i] < ti ? 1 : 0) | (d < borrow ? 1 : 0);
            s[i] = e;
        }
#pragma unroll
        for (int i = 0; i <= K; i++) rr[i] = borrow ? rr[i] : s[i];
    }
#pragma unroll
    for (int i = 0; i < K; i++) r[i] = rr[i];
}

// r = a c mod t for a, c below t
template <int WT>
FHE_HD void bigt_mul(const u64 *a, const u64 *c, const BigT<WT> &bt, u64 *r) {
    u64 x[2 * WT];
#pragma unroll
    for (int i = 0; i < 2 * WT; i++) x[i] = 0;
#pragma unroll
    for (int i = 0; i < WT; i++) {
        u64 carry = 0;
#pragma unroll
        for (int j = 0; j < WT; j++) bigt_mac(x[i + j], a[i], c[j], carry);
        x[i + WT] = carry;
    }
    bigt_reduce<WT>(x, bt, r);
}

// One lane per coefficient (b, j): values [batch][nvalues][WT] limbs (zero from nvalues on) -> out[b][i][j] for the
// `rows` moduli of the level.  qmt = q_mod_t, applied when `scaled`, as is delta [rows] {delta_i, shoup}.
// total = batch * 2^logn.
template <int WT>
__global__ void __launch_bounds__(BIGT_THREADS)
    bigt_project_kernel(const u64 *__restrict__ values, u64 nvalues, u64 *__restrict__ out, uint32_t rows,
                        const DevMod *__restrict__ mods, const u64x2 *__restrict__ delta, BigT<WT> bt, BigVal<WT> qmt,
                        uint32_t scaled, uint32_t logn, u64 total) {
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const u64 b = gid >> logn, j = gid & ((1ull << logn) - 1);
    const bool have = j < nvalues;
    const u64 *src = values + (b * nvalues + (have ? j : 0)) * WT;
    u64 x[2 * WT], m[WT];
#pragma unroll
    for (int k = 0; k < WT; k++) {
        x[k] = have ? src[k] : 0;
        x[WT + k] = 0;
    }
    bigt_reduce<WT>(x, bt, m);
    if (scaled) bigt_mul<WT>(m, qmt.w, bt, m);
    u64 *dst = out + ((b * rows) << logn) + j;
    for (uint32_t i = 0; i < rows; i++) {
        const DevMod md = mods[i];
        u64 r = reduce_u64(m[WT - 1], md);
#pragma unroll
        for (int k = WT - 2; k >= 0; k--) r = reduce_u128(r, m[k], md);
        if (scaled) {
            const u64x2 d = delta[i];
            r = mul_shoup(r, d.x, d.y, md.p);
        }
        dst[(u64)i << logn] = r;
    }
}

// One thread per coefficient: polys [batch][P][N] PowerBasis over the plaintext context (tab: its lift table) ->
// out [batch][N][WT], ((x + t) mod Q_p) mod t.  Q_p has at most WT + 2 <= 2 WT limbs (bits(Q_p) < bits(t) + 122), so the
// sum is within bigt_reduce's range.  PC = 0: run-time P up to LIFT_LMAX, arrays in scratch.
// grid = batch * nblk workgroups, nblk = ceil(N / BIGT_THREADS).
template <int PC, int WT>
__global__ void __launch_bounds__(BIGT_THREADS)
    bigt_tail_kernel(const u64 *__restrict__ polys, const u64 *__restrict__ tab, BigT<WT> bt, u64 *__restrict__ out,
                     uint32_t p_rt, uint32_t logn, uint32_t nblk) {
    constexpr int LA = PC > 0 ? PC : LIFT_LMAX;
    constexpr int UF = PC > 0 ? PC : 1;
    const int P = PC > 0 ? PC : (int)p_rt;
    const uint32_t b = blockIdx.x / nblk, kb = blockIdx.x - b * nblk;
    const uint32_t n = 1u << logn;
    const uint32_t c = kb * BIGT_THREADS + threadIdx.x;
    const bool live = c < n;
    const uint32_t cc = live ? c : 0;
    const u64 *src = polys + (((u64)b * P) << logn) + cc;

    u64 d[LA], x[LA];
#pragma unroll UF
    for (int i = 0; i < P; i++) d[i] = src[(u64)i << logn];
    garner_horner<LA, UF>(d, x, tab, P);   // (kernels_noise.hpp)

    // s = x + t (carry cs), df = s - Q_p (borrow); w = s >= Q_p ? df : s, kept in d
    const u64 *ql = tab + lift_q_at(P);
    u64 cs = 0, borrow = 0;
#pragma unroll UF
    for (int k = 0; k < P; k++) {
        const u64 tk = k < WT ? bt.t[k < WT ? k : 0] : 0;   // (the index stays inside t[] for the unrolled k >= WT)
        const u64 a = x[k] + tk, s = a + cs;
        cs = (a < tk ? 1 : 0) | (s < cs ? 1 : 0);
        const u64 qk = ql[k], e = s - qk, f = e - borrow;
        borrow = (s < qk ? 1 : 0) | (e < borrow ? 1 : 0);
        x[k] = s;
        d[k] = f;
    }
    const bool ge = cs != 0 || borrow == 0;
    u64 z[2 * WT], w[WT];
#pragma unroll
    for (int k = 0; k < 2 * WT; k++) {
        const int kk = k < LA ? k : 0;   // (limbs from P on are zero: Q_p has at most 2 WT)
        z[k] = k < P ? (ge ? d[kk] : x[kk]) : 0;
    }
    bigt_reduce<WT>(z, bt, w);
    u64 *o = out + (((u64)b << logn) + cc) * WT;
#pragma unroll
    for (int k = 0; k < WT; k++)
        if (live) o[k] = w[k];
}

}  // namespace k
}  // namespace fhe
