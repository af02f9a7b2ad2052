// kernels_keygen.hpp -- key-switching-key generation on the device (KeySwitchingKey::new, F/bfv/keys/
// key_switching_key.rs:71-236, and the `from` polynomials of RelinearizationKey / GaloisKey).  A key is `ndigits`
// secret-key encryptions over the key context whose digit i carries g_i (.) from; the pieces are the encryption
// kernels' (kernels_encrypt.hpp):
//   ksk_seeds_kernel        the key's public seed K and the per-digit seeds of ChaCha8Rng::from_seed(K)   :90-93, 126-141
//   cbd_sample_at_kernel    the errors: cbd_sample_kernel's draws, starting after K (u64 word 4 of the stream of S)
//   ksk_consts_kernel       g_i mod q_j (RnsContext::get_garner, or 2^(i log_base) for one modulus), 2^64 mod q_j, q_j^-1
//   ksk_gen_kernel          NTT(lift(e_i)) - c1[i] (.) s + g_i (.) from, with both Shoup twins and the F64 words
//                           written in the epilogue                                                       :149-236
//   ksk_combine_ew_kernel   the same epilogue as an element-wise pass, for rows larger than one LDS tile (N >= 32768)
//   galois_from_kernel      the Ntt-form substitution of s for a batch of exponents (GaloisKey::new)   galois_key.rs:26-58
// c1[i] = Poly::random_from_seed(ctx_ksk, seed_i) is seed_expand_kernel's output, taken as Ntt values as the reference
// takes them.  c0 = NTT(e - INTT(c1 (.) s) + g from) is computed as NTT(e) - c1 (.) s + g (.) NTT(from): the transform is
// linear mod q_j, so the two are bit-identical, and this form needs no inverse transform per digit.
// No branch or address below depends on a sample, on s or on `from`: only on indices, exponents and moduli.
#pragma once
#include "kernels_encrypt.hpp"

namespace fhe {
namespace k {

// Keys per launch group: every key's output buffers travel in the kernel arguments (a table of 6 x 32 pointers).
constexpr int KG_KEYS = 32;
struct KskOut {
    u64 *c0, *c0s, *c1, *c1s, *c0f, *c1f;   // [ndigits][Lk][N] each; c0f / c1f null when the key is not F64-eligible
};
struct KskOutTable {
    KskOut k[KG_KEYS];
};
struct KgExps {
    uint32_t e[KG_KEYS];   // substitution exponents mod 2N (odd)
};

__device__ __forceinline__ void seed_key(const uint8_t *sd, uint32_t key[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++)
        key[i] = (uint32_t)sd[4 * i] | ((uint32_t)sd[4 * i + 1] << 8) | ((uint32_t)sd[4 * i + 2] << 16) |
                 ((uint32_t)sd[4 * i + 3] << 24);
}
__device__ __forceinline__ void put_words(uint8_t *dst, const uint32_t *w) {
    for (int i = 0; i < 32; i++) dst[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

// One thread per (key, digit): K = bytes [0, 32) of ChaCha8Rng::from_seed(S[key]) (rng.fill(&mut seed), the first
// eight keystream words), seed_i = bytes [32 i, 32 i + 32) of ChaCha8Rng::from_seed(K) (generate_c1).
// S [nkeys][32] -> K_out [nkeys][32] (digit 0's thread; may be null), dseeds [nkeys][ndigits][32].
__global__ void ksk_seeds_kernel(const uint8_t *__restrict__ S, uint8_t *__restrict__ K_out, uint8_t *__restrict__ dseeds,
                                 uint32_t ndigits, uint32_t total) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const uint32_t key = gid / ndigits, i = gid - key * ndigits;
    uint32_t sk[8], w[16], kk[8];
    seed_key(S + (u64)key * 32, sk);
    chacha8_block(sk, 0, w);
#pragma unroll
    for (int j = 0; j < 8; j++) kk[j] = w[j];
    if (i == 0 && K_out) put_words(K_out + (u64)key * 32, kk);
    chacha8_block(kk, i >> 1, w);
    put_words(dseeds + (u64)gid * 32, w + 8 * (i & 1));
}

// cbd_sample_kernel with the draws starting at next_u64 word `word0` of each stream (KeySwitchingKey::new draws its
// errors after the 32 bytes of K: word0 = 4).  The same body (FHE_CBD_SAMPLE_BODY, kernels_encrypt.hpp); one more
// keystream block in LDS, as word0 need not be block-aligned.
__global__ void __launch_bounds__(CBD_THREADS)
    cbd_sample_at_kernel(const uint8_t *__restrict__ seeds, int8_t *__restrict__ out, uint32_t variance, u64 nsamples,
                         uint32_t logn, u64 wpd, u64 word0) {
    FHE_DYN_SMEM(uint32_t, words);   // CBD_AT_SMEM_BYTES: [nblk][16] keystream words
#define FHE_CBD_BIT_AT(g) (word0 * 64 + cbd_bit_offset(g, variance, logn, wpd))
    FHE_CBD_SAMPLE_BODY(FHE_CBD_BIT_AT);
#undef FHE_CBD_BIT_AT
}
#undef FHE_CBD_SAMPLE_BODY
constexpr size_t CBD_AT_SMEM_BYTES = (CBD_MAX_BLOCKS + 1) * 16 * sizeof(uint32_t);

// The public constants of one generation call, one thread per (digit i, key row j) -- nothing comes from the host:
//   g [ndigits][Lk] = g_i mod q_j: log_base == 0: the Garner coefficient q*_i (q*_i^-1 mod q_i) of the first `ndigits`
//                     moduli (RnsContext::get_garner, not reduced mod Q); otherwise 2^(i log_base) mod q_j
//   rq [Lk]         = {2^64 mod q_j, q_j^-1 mod 2^64} (the Shoup twins of the epilogue)
__global__ void ksk_consts_kernel(const DevMod *__restrict__ mods, uint32_t ndigits, uint32_t lk, uint32_t log_base,
                                  u64 *__restrict__ g, u64x2 *__restrict__ rq) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= ndigits * lk) return;
    const uint32_t i = gid / lk, j = gid - i * lk;
    const DevMod md = mods[j];
    const u64 q = md.p;
    u64 gij;
    if (log_base) {
        gij = (1ull << (i * log_base)) % q;
    } else {
        const DevMod mi = mods[i];
        u64 star_j = 1 % q, star_i = 1;
        for (uint32_t k = 0; k < ndigits; k++) {
            if (k == i) continue;
            star_j = mul_mod(star_j, mods[k].p % q, md);
            star_i = mul_mod(star_i, mods[k].p % mi.p, mi);
        }
        u64 tilde = 1, base = star_i, e = mi.p - 2;   // Fermat: star_i^(q_i - 2) = star_i^-1 mod q_i
        while (e) {
            if (e & 1) tilde = mul_mod(tilde, base, mi);
            base = mul_mod(base, base, mi);
            e >>= 1;
        }
        gij = mul_mod(star_j, tilde % q, md);
    }
    g[gid] = gij;
    if (i == 0) {
        u64 inv = q;   // Newton over 2^64: q q = 1 mod 8, each step doubles the bits
        for (int it = 0; it < 5; it++) inv *= 2 - q * inv;
        rq[j] = u64x2{(~0ull % q + 1) % q, inv};
    }
}

// floor(c 2^64 / q) for c < q, q odd: c 2^64 = floor(.) q + r with r = c (2^64 mod q) mod q, so floor(.) = -r q^-1 mod 2^64
__device__ __forceinline__ u64 shoup_twin(u64 c, u64 r64, u64 qinv, const DevMod &md) {
    return (0ull - mul_mod(c, r64, md)) * qinv;
}
__device__ __forceinline__ u64 f64_word(u64 c) {   // (exact: c < 2^50 on F64-eligible keys)
    const double d = (double)c;
    u64 b;
    __builtin_memcpy(&b, &d, 8);
    return b;
}

// One workgroup per (key, digit, key row).  e [nkeys][ndigits][N] int8 (ChaCha8Rng::from_seed(S[key]) draws);
// c1 [nkeys][ndigits][rows][N] (seed_expand_kernel); s_ntt [rows][N]; from_ntt [nkeys][rows][N]; g, rq from
// ksk_consts_kernel; out: the keys' buffers (wf: write the F64 words).
template <int LOGM, bool NARROW = false, int F64 = 0>
__global__ void __launch_bounds__(ntt_threads_c(LOGM), 4)
    ksk_gen_kernel(const int8_t *__restrict__ e, const u64 *__restrict__ c1, const u64 *__restrict__ s_ntt,
                   const u64 *__restrict__ from_ntt, const u64 *__restrict__ g, const u64x2 *__restrict__ rq,
                   KskOutTable out, uint32_t ndigits, uint32_t rows, uint32_t wf, const DevMod *__restrict__ mods,
                   const u64x2 *__restrict__ tw) {
    FHE_DYN_SMEM(u64, lds);
    constexpr int T = ntt_threads_c(LOGM);
    constexpr int M = 1 << LOGM;
    const uint32_t tid = threadIdx.x;
    const uint32_t kd = to_sgpr(blockIdx.x / rows);   // key * ndigits + digit
    const uint32_t r = blockIdx.x - kd * rows;
    const uint32_t key = to_sgpr(kd / ndigits), i = kd - key * ndigits;
    const DevMod md = mods[r];
    const u64 gi = g[i * rows + r];
    const u64x2 rc = rq[r];
    const u64x2 *ar = reinterpret_cast<const u64x2 *>(c1 + ((u64)kd * rows + r) * M);
    const u64x2 *sr = reinterpret_cast<const u64x2 *>(s_ntt + (u64)r * M);
    const u64x2 *fr = reinterpret_cast<const u64x2 *>(from_ntt + ((u64)key * rows + r) * M);
    const KskOut o = out.k[key];
    const u64 off = ((u64)i * rows + r) * M;
    u64x2 *o0 = reinterpret_cast<u64x2 *>(o.c0 + off), *o0s = reinterpret_cast<u64x2 *>(o.c0s + off);
    u64x2 *o1 = reinterpret_cast<u64x2 *>(o.c1 + off), *o1s = reinterpret_cast<u64x2 *>(o.c1s + off);
    small_row_ntt<LOGM, T, NARROW, F64>(lds, tw + (u64)r * M, md, tid, e + (u64)kd * M, [&](uint32_t x_i, u64 x, u64 y) {
        const u64x2 av = ar[x_i >> 1], sv = sr[x_i >> 1], fv = fr[x_i >> 1];
        const u64x2 c{add_mod(sub_mod(x, mul_mod(av.x, sv.x, md), md.p), mul_mod(gi, fv.x, md), md.p),
                      add_mod(sub_mod(y, mul_mod(av.y, sv.y, md), md.p), mul_mod(gi, fv.y, md), md.p)};
        o0[x_i >> 1] = c;
        o1[x_i >> 1] = av;
        o0s[x_i >> 1] = u64x2{shoup_twin(c.x, rc.x, rc.y, md), shoup_twin(c.y, rc.x, rc.y, md)};
        o1s[x_i >> 1] = u64x2{shoup_twin(av.x, rc.x, rc.y, md), shoup_twin(av.y, rc.x, rc.y, md)};
        if (wf) {
            reinterpret_cast<u64x2 *>(o.c0f + off)[x_i >> 1] = u64x2{f64_word(c.x), f64_word(c.y)};
            reinterpret_cast<u64x2 *>(o.c1f + off)[x_i >> 1] = u64x2{f64_word(av.x), f64_word(av.y)};
        }
    });
}

// ksk_gen_kernel's epilogue as an element-wise pass over the transformed errors x [nkeys][ndigits][rows][N] (rows
// larger than one LDS tile); total = nkeys * ndigits * rows * 2^logn.
__global__ void ksk_combine_ew_kernel(const u64 *__restrict__ x, const u64 *__restrict__ c1, const u64 *__restrict__ s_ntt,
                                      const u64 *__restrict__ from_ntt, const u64 *__restrict__ g,
                                      const u64x2 *__restrict__ rq, KskOutTable out,
                                      uint32_t ndigits, uint32_t rows, uint32_t wf, const DevMod *__restrict__ mods,
                                      uint32_t logn, u64 total) {
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const u64 row = gid >> logn, j = gid & ((1ull << logn) - 1);
    const uint32_t kd = (uint32_t)(row / rows), r = (uint32_t)(row - (u64)kd * rows);
    const uint32_t key = kd / ndigits, i = kd - key * ndigits;
    const DevMod md = mods[r];
    const u64 av = c1[gid], sv = s_ntt[((u64)r << logn) + j], fv = from_ntt[(((u64)key * rows + r) << logn) + j];
    const u64 c = add_mod(sub_mod(x[gid], mul_mod(av, sv, md), md.p), mul_mod(g[i * rows + r], fv, md), md.p);
    const u64x2 rc = rq[r];
    const KskOut o = out.k[key];
    const u64 off = (((u64)i * rows + r) << logn) + j;
    o.c0[off] = c;
    o.c1[off] = av;
    o.c0s[off] = shoup_twin(c, rc.x, rc.y, md);
    o.c1s[off] = shoup_twin(av, rc.x, rc.y, md);
    if (wf) {
        o.c0f[off] = f64_word(c);
        o.c1f[off] = f64_word(av);
    }
}

// GaloisKey::new's s_sub in Ntt form for a batch of exponents: s [rows][N] Ntt -> out [nkeys][rows][N], key b
// substituted by exps.e[b] (substitute_kernel's Ntt-form gather); total = nkeys * rows * 2^logn.
__global__ void galois_from_kernel(const u64 *__restrict__ s, u64 *__restrict__ out, KgExps exps, uint32_t rows,
                                   uint32_t logn, u64 total) {
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const uint32_t j = (uint32_t)(gid & ((1ull << logn) - 1));
    const u64 row = gid >> logn;
    const uint32_t key = (uint32_t)(row / rows), r = (uint32_t)(row - (u64)key * rows);
    out[gid] = s[((u64)r << logn) + galois_src_index(j, exps.e[key], logn)];
}

}  // namespace k
}  // namespace fhe
