// kernels_noise.hpp -- residues to integers, and the noise of a ciphertext (RnsContext::lift, M/rns/mod.rs:138-143,
// reached through Vec<BigUint>::from(&Poly), M/rq/convert.rs:507-529; SecretKey::measure_noise,
// F/bfv/keys/secret_key.rs:55-98).  One thread owns one coefficient: its L residues are read at stride N (coalesced
// along N), and the integer x in [0, q) with x = r_i mod q_i is built in registers:
//   lift_kernel<L, false>   x as W little-endian u64 limbs per coefficient                     rns/mod.rs:138-143
//   lift_kernel<L, true>    max over a polynomial of min(bits(x), bits(q - x)), per workgroup   secret_key.rs:88-95
//   noise_max_kernel        the maximum over a polynomial's workgroups
// The reference sums garner_i r_i and reduces mod q; here Garner's mixed-radix digits d_i (x = d_0 + d_1 q_0 +
// d_2 q_0 q_1 + ...) are evaluated by Horner's rule, which never leaves [0, q): the same integer, so the same limbs.
// L is a template argument so that the digit and limb arrays are indexed by constants and stay in VGPRs; L = 0 is the
// generic instance (run-time L up to LIFT_LMAX, arrays in scratch) for chains longer than the instantiated ones.
// The loader can subtract the Delta-scaled plaintext of Plaintext::to_poly (F/bfv/plaintext.rs:172-196) on the way in:
// in PowerBasis that polynomial is delta_i ((m q_mod_t) mod t) mod q_i per coefficient, no transform.
// The values are secret-dependent (the reference marks measure_noise variable-time): no branch or address below depends
// on them -- selects only.
#pragma once
#include "kernels_common.hpp"

namespace fhe {
namespace k {

constexpr int LIFT_THREADS = 256;
constexpr int LIFT_LMAX = 64;   // the generic instance's arrays
constexpr size_t LIFT_SMEM_BYTES = LIFT_THREADS * sizeof(uint32_t);

// The public constants of a context's lift, [lift_table_words(L)] u64 (engine.hpp lift_consts):
//   [0, L)              q_i
//   [L, 2L)             M_i, the multiple of q_i in [2^62, 2^63): t + M_i - d_j is non-negative and = t - d_j mod q_i
//   [2L, 2L + L(L-1))   {c, floor(c 2^64 / q_i)}, c = q_j^-1 mod q_i, for i = 1 .. L-1, j < i at pair i(i-1)/2 + j
//   then L words        the limbs of q (zero above the W-th)
FHE_HD uint32_t lift_pairs_at(uint32_t l) { return 2 * l; }
FHE_HD uint32_t lift_q_at(uint32_t l) { return 2 * l + l * (l - 1); }
FHE_HD uint32_t lift_table_words(uint32_t l) { return lift_q_at(l) + l; }

// Plaintext::to_poly in PowerBasis, subtracted by the loader: m [batch][N] in [0, t) (null: nothing is subtracted),
// delta [L] {delta_i, shoup}, qmt {q_mod_t, shoup mod t}.
struct LiftSub {
    const u64 *m;
    const u64x2 *delta;
    u64 t;
    u64x2 qmt;
};
inline LiftSub lift_sub_none() { return LiftSub{}; }   // m null: nothing is subtracted

FHE_HD uint32_t bits64(u64 v) { return v ? 64u - (uint32_t)__builtin_clzll(v) : 0u; }

// Garner's digits of the residues d[0 .. L) in place, d_i = (..((r_i - d_0) q_0^-1 - d_1) q_1^-1 ...) mod q_i (lazily
// below 2 q_i inside the chain), then Horner's limbs x[0 .. L): x = (..(d_{L-1} q_{L-2} + d_{L-2}) q_{L-3} + ...) q_0 +
// d_0, one limb longer per step.  tab: the table above; UF (in scope): the unroll factor, L for a compile-time L and 1
// for the generic instances.  Stated once, as a macro (undefined after lift_kernel): lift_kernel expands it in its body
// and bigt_tail_kernel (kernels_bigt.hpp) calls garner_horner below, the forms in which each of them compiles to the
// code it had with a body of its own (lift_kernel through the function: up to 4.7 % more instructions).  The
// expansion declares i, j, k, q, mq, pr, t, len, carry, hi, lo in loop scopes of its own.
#define FHE_GARNER_HORNER(d, x, tab, L)                                                                     \
    _Pragma("unroll UF") for (int i = 1; i < L; i++) {                                                     \
        const u64 q = tab[i], mq = tab[L + i];                                                             \
        const u64 *pr = tab + lift_pairs_at(L) + (uint32_t)(i * (i - 1));                                  \
        u64 t = d[i];                                                                                      \
        _Pragma("unroll UF") for (int j = 0; j < i; j++)                                                   \
            t = mul_shoup_lazy(t + mq - d[j], pr[2 * j], pr[2 * j + 1], q);                                \
        d[i] = csub(t, q);                                                                                 \
    }                                                                                                      \
    x[0] = d[L - 1];                                                                                       \
    _Pragma("unroll UF") for (int i = L - 2; i >= 0; i--) {                                                \
        const u64 q = tab[i];                                                                              \
        const int len = L - 1 - i;                                                                         \
        u64 carry = d[i];                                                                                  \
        _Pragma("unroll UF") for (int k = 0; k < len; k++) {                                               \
            const u64 hi = mulhi64(x[k], q);                                                               \
            const u64 lo = x[k] * q + carry;                                                               \
            carry = hi + (lo < carry ? 1 : 0);                                                             \
            x[k] = lo;                                                                                     \
        }                                                                                                  \
        x[len] = carry;                                                                                    \
    }
template <int LA, int UF>
__device__ __forceinline__ void garner_horner(u64 (&d)[LA], u64 (&x)[LA], const u64 *__restrict__ tab, const int L) {
    FHE_GARNER_HORNER(d, x, tab, L)
}

// grid = batch * nblk workgroups, nblk = ceil(N / LIFT_THREADS); polys [batch][L][N]; BITS: partial [nblk][batch],
// else out [batch][N][W].
template <int LC, bool BITS>
__global__ void __launch_bounds__(LIFT_THREADS)
    lift_kernel(const u64 *__restrict__ polys, const u64 *__restrict__ tab, LiftSub sub, u64 *__restrict__ out,
                uint32_t *__restrict__ partial, uint32_t l_rt, uint32_t w, uint32_t logn, uint32_t nblk, uint32_t batch) {
    constexpr int LA = LC > 0 ? LC : LIFT_LMAX;
    constexpr int UF = LC > 0 ? LC : 1;   // full unrolling for a compile-time L, none for the generic instance
    const int L = LC > 0 ? LC : (int)l_rt;
    const uint32_t tid = threadIdx.x;
    const uint32_t b = blockIdx.x / nblk, kb = blockIdx.x - b * nblk;
    const uint32_t n = 1u << logn;
    const uint32_t c = kb * LIFT_THREADS + tid;
    const bool live = c < n;
    const uint32_t cc = live ? c : 0;   // (idle lanes of a short row recompute coefficient 0 and write nothing)
    const u64 *src = polys + (((u64)b * L) << logn) + cc;

    u64 d[LA], x[LA];
#pragma unroll UF
    for (int i = 0; i < L; i++) d[i] = src[(u64)i << logn];
    if (sub.m != nullptr) {
        const u64 mm = mul_shoup(sub.m[((u64)b << logn) + cc], sub.qmt.x, sub.qmt.y, sub.t);
#pragma unroll UF
        for (int i = 0; i < L; i++) {
            const u64 q = tab[i];
            const u64x2 dl = sub.delta[i];
            d[i] = sub_mod(d[i], mul_shoup(mm, dl.x, dl.y, q), q);
        }
    }
    FHE_GARNER_HORNER(d, x, tab, L)

    if constexpr (!BITS) {
        u64 *o = out + (((u64)b << logn) + cc) * w;
#pragma unroll UF
        for (int k = 0; k < L; k++)
            if (live && (uint32_t)k < w) o[k] = x[k];
    } else {
        FHE_DYN_SMEM(uint32_t, red);   // LIFT_SMEM_BYTES
        const u64 *ql = tab + lift_q_at(L);
        uint32_t bx = 0, by = 0;
        u64 borrow = 0;
#pragma unroll UF
        for (int k = 0; k < L; k++) {
            const u64 qk = ql[k], df = qk - x[k], y = df - borrow;
            borrow = (qk < x[k] ? 1 : 0) | (df < borrow ? 1 : 0);
            bx = x[k] ? 64u * k + bits64(x[k]) : bx;
            by = y ? 64u * k + bits64(y) : by;
        }
        red[tid] = live ? (bx < by ? bx : by) : 0u;
        __syncthreads();
        for (uint32_t s = LIFT_THREADS / 2; s > 0; s >>= 1) {
            if (tid < s) {
                const uint32_t a = red[tid], o = red[tid + s];
                red[tid] = a > o ? a : o;
            }
            __syncthreads();
        }
        if (tid == 0) partial[(u64)kb * batch + b] = red[0];
    }
}

#undef FHE_GARNER_HORNER

// partial [nblk][batch] -> out [batch]: one thread per polynomial, never across polynomials
__global__ void noise_max_kernel(const uint32_t *__restrict__ partial, uint32_t nblk, uint32_t batch, u64 *__restrict__ out) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    uint32_t mx = 0;
    for (uint32_t k = 0; k < nblk; k++) {
        const uint32_t v = partial[(u64)k * batch + b];
        mx = v > mx ? v : mx;
    }
    out[b] = mx;
}

}  // namespace k
}  // namespace fhe
