// kernels_encrypt.hpp -- BFV encryption on the device: the centered binomial sampler (Poly::small), secret-key and
// public-key encryption.  The transforms are the ntt_kernel passes (kernels_passes.hpp) behind loaders / stores of
// their own:
//   cbd_sample_kernel       sample_vec_cbd over ChaCha8Rng::from_seed (no hashing)     fhe-util/src/lib.rs:22-66
//   small_ntt_kernel        lift into every q_i + NttOperator::forward (Poly::small)   M/rq/mod.rs:298-330
//   encrypt_sk_kernel       e_ntt - a (.) s + m, with a copied into c1                 F/bfv/keys/secret_key.rs:100-134
//   encrypt_pk_kernel       u (.) pk0 + e1 + m, u (.) pk1 + e2 (three stages)          F/bfv/keys/public_key.rs:47-97
//   small_lift_ew_kernel / encrypt_combine_ew_kernel   the element-wise forms, for rows larger than one LDS tile
//                           (N >= 32768) and for PowerBasis samples, around launch_ntt
//                           (both forms of an epilogue take their steps from encrypt_sk_combine / encrypt_pk_combine /
//                           encrypt_plus)
// The samples are secrets: every address and branch below depends on indices and parameters only, never on a sample,
// a key or a plaintext word (the lift of a negative sample is a select, the products are the branch-free mul_mod).
#pragma once
#include "kernels_passes.hpp"

namespace fhe {
namespace k {

// ---------------------------------------------------------------------- sampler ----
// sample_vec_cbd (fhe-util/src/lib.rs:22-66) is counter-addressable.  Within one draw of N samples, for v <= 16 sample
// i is popcount(bits [4vi, 4vi + 2v)) - popcount(bits [4vi + 2v, 4v(i + 1))) of the draw's next_u64 words (least
// significant bit first), and for 17 <= v <= 32 it takes the draw's words 2i and 2i + 1.  Every draw starts a fresh
// pool at a word boundary and drops the bits left in its last word, so a draw consumes wpd = ceil(N 4v / 64) words
// (v <= 16; 2N for v > 16) and draw j of one generator (u, e1, e2: j = 0, 1, 2) starts at word j wpd.  (For N >= 16
// every draw ends on a word boundary; at N = 8 with odd v it does not.)  ChaCha8Rng::from_seed(seed): key = the 32
// seed bytes as little-endian words; 64-bit block counter from 0, stream id 0; next_u64 = two consecutive
// little-endian words, low word first -- the layout of seed_expand_kernel, PARITY UNPINNED like it.
// grid = (ceil(kN / CBD_THREADS), batch): a workgroup computes the ChaCha blocks its CBD_THREADS samples read once,
// into LDS, then one thread per sample extracts its bits.  out [batch][kN] int8 (|x| <= 2v <= 64), draw after draw.
constexpr int CBD_THREADS = 256;
// v > 16: 2 words a sample (64 blocks + one partial); v <= 16: <= 16v + 1 words plus <= 32 skipped bits per draw
// boundary (only at N = 8: 32 boundaries, 16 words) in one workgroup's range
constexpr int CBD_MAX_BLOCKS = 2 * CBD_THREADS / 8 + 2;
constexpr size_t CBD_SMEM_BYTES = CBD_MAX_BLOCKS * 16 * sizeof(uint32_t);
// first stream bit of sample g (draw g >> logn, index g mod N); wpd = words per draw
__device__ __forceinline__ u64 cbd_bit_offset(u64 g, uint32_t v, uint32_t logn, u64 wpd) {
    const u64 i = g & ((1ull << logn) - 1);
    return (g >> logn) * wpd * 64 + (v <= 16 ? 4ull * v * i : 128ull * i);
}
// The body of both samplers, written once: BIT(g) is the first stream bit of sample g (cbd_sample_kernel: draws from
// word 0; cbd_sample_at_kernel, kernels_keygen.hpp: from a word offset).  A macro and not an inline function: inlining a
// shared function reorders cbd_sample_kernel's instructions, and its ISA stays as it was.
#define FHE_CBD_SAMPLE_BODY(BIT)                                                                                   \
    const uint32_t tid = threadIdx.x;                                                                              \
    const uint32_t b = blockIdx.y;                                                                                 \
    const u64 g0 = (u64)blockIdx.x * CBD_THREADS;                                                                  \
    const u64 glast = (g0 + CBD_THREADS <= nsamples ? g0 + CBD_THREADS : nsamples) - 1;                            \
    const u64 blk0 = (BIT(g0) >> 6) >> 3;                                                                          \
    const u64 wlast = (BIT(glast) >> 6) + 1;   /* (the word after a sample's first is always read) */              \
    const uint32_t nblk = (uint32_t)((wlast >> 3) - blk0 + 1);                                                     \
    if (tid < nblk) {                                                                                              \
        const uint8_t *sd = seeds + (u64)b * 32;                                                                   \
        uint32_t key[8];                                                                                           \
        _Pragma("unroll") for (int i = 0; i < 8; i++)                                                              \
            key[i] = (uint32_t)sd[4 * i] | ((uint32_t)sd[4 * i + 1] << 8) | ((uint32_t)sd[4 * i + 2] << 16) |     \
                     ((uint32_t)sd[4 * i + 3] << 24);                                                              \
        uint32_t w[16];                                                                                            \
        chacha8_block(key, blk0 + tid, w);                                                                         \
        _Pragma("unroll") for (int i = 0; i < 16; i++) words[16 * tid + i] = w[i];                                 \
    }                                                                                                              \
    __syncthreads();                                                                                               \
    const u64 g = g0 + tid;                                                                                        \
    if (g >= nsamples) return;                                                                                     \
    const u64 bo = BIT(g);                                                                                         \
    const uint32_t wi = (uint32_t)((bo >> 6) - 8 * blk0), sh = (uint32_t)(bo & 63);                                \
    const u64 lo = (u64)words[2 * wi] | ((u64)words[2 * wi + 1] << 32);                                            \
    const u64 hi = (u64)words[2 * wi + 2] | ((u64)words[2 * wi + 3] << 32);                                        \
    const u128_t pool = (((u128_t)hi << 64) | lo) >> sh;                                                           \
    const uint32_t v2 = 2 * variance; /* 2 ... 64 */                                                               \
    const u64 mask = v2 == 64 ? ~0ull : (1ull << v2) - 1;                                                          \
    const int add = __builtin_popcountll((u64)pool & mask), sub = __builtin_popcountll((u64)(pool >> v2) & mask);  \
    out[(u64)b * nsamples + g] = (int8_t)(add - sub)
#define FHE_CBD_BIT(g) cbd_bit_offset(g, variance, logn, wpd)
__global__ void __launch_bounds__(CBD_THREADS)
    cbd_sample_kernel(const uint8_t *__restrict__ seeds, int8_t *__restrict__ out, uint32_t variance, u64 nsamples,
                      uint32_t logn, u64 wpd) {
    FHE_DYN_SMEM(uint32_t, words);   // CBD_SMEM_BYTES: [nblk][16] keystream words
    FHE_CBD_SAMPLE_BODY(FHE_CBD_BIT);
}
#undef FHE_CBD_BIT

// x in [-64, 64] -> x mod p (try_convert_from(&[i64], ctx, false)): p + x selected for negative x, no branch
__device__ __forceinline__ u64 lift_small(int8_t x, u64 p) {
    const int64_t s = x;
    return (u64)s + (p & (0ull - (u64)(s < 0)));
}

// The index-aware sibling of lds_to_tile: the same chunk ownership (thread t owns the element pairs {c*T + t}), but
// f(i, x_i, x_{i+1}) does its own loads and stores, so an epilogue can combine the tile with other rows.
template <int CH, int M, int T, class F>
__device__ __forceinline__ void lds_pairs(const u64 *lds, uint32_t tid, F f) {
    if constexpr (CH > 0) {
#pragma unroll
        for (int c = 0; c < CH; c++) {
            const uint32_t i = 2 * (c * T + tid);
            f(i, lds[padi(i)], lds[padi(i + 1)]);
        }
    } else {
        for (uint32_t i = 2 * tid; i < (uint32_t)M; i += 2 * T) f(i, lds[padi(i)], lds[padi(i + 1)]);
    }
}

// The forward transform of one lifted sample row src[N] (int8) mod md in the LDS tile, then epi(i, X_i, X_{i+1}) with
// canonical values.  NARROW / F64 as encode_lift_kernel.  Ends without a barrier: a second transform in the same
// workgroup puts one before its loads.
template <int LOGM, int T, bool NARROW, int F64, class F>
__device__ __forceinline__ void small_row_ntt(u64 *lds, const u64x2 *__restrict__ twr, const DevMod &md, uint32_t tid,
                                              const int8_t *__restrict__ src, F epi) {
    constexpr int M = 1 << LOGM;
    constexpr int CH = tile_chunks_c(LOGM, T);
    if constexpr (F64 > 0) {
        const PM pmf = make_pm_f64(md);
        const PF pf = pf_of(pmf);
        auto ld = [&](uint32_t i, uint32_t) { return bits_of_f64(f64_from_u64(lift_small(src[i], md.p))); };
        ntt_fwd_lds<LOGM, T, GMAX, true, true, -F64>(lds, twr, 1, pmf, tid, ld);
        lds_pairs<CH, M, T>(lds, tid, [&](uint32_t i, u64 x, u64 y) {
            epi(i, to_u64_canonical(f64_of_bits(x), pf), to_u64_canonical(f64_of_bits(y), pf));
        });
    } else {
        const PM pm = make_pm(md);
        if constexpr (LOGM <= 12) {
            // (the lift staged through the tile, and no twiddle prefetch on the general passes: the loader form spills
            // at LOGM = 12, as decode_simd_kernel's does)
            for (uint32_t i = tid; i < (uint32_t)M; i += T) lds[padi(i)] = lift_small(src[i], md.p);
            FHE_BARRIER();
            ntt_fwd_lds<LOGM, T, GMAX, NARROW, true, (NARROW ? 1 : 0)>(lds, twr, 1, pm, tid);
        } else {
            auto ld = [&](uint32_t i, uint32_t) { return lift_small(src[i], md.p); };
            ntt_fwd_lds<LOGM, T, GMAX, true, true, (NARROW ? 1 : 0)>(lds, twr, 1, pm, tid, ld);
        }
        const u64 p = md.p, p2 = md.p2, p4 = p2 << 1, p8 = p2 << 2, np4 = pm.np2 << 1, np8 = pm.np2 << 2;
        auto canon = [&](u64 v) {
            if constexpr (NARROW) v = csub_n(csub_n(v, p8, np8), p4, np4);   // < 16p -> < 4p
            return csub_n(csub_n(v, p2, pm.np2), p, pm.np);
        };
        lds_pairs<CH, M, T>(lds, tid, [&](uint32_t i, u64 x, u64 y) { epi(i, canon(x), canon(y)); });
    }
}

// Poly::<Ntt>::small: one workgroup per (item, row); samples [batch][N] int8 -> out [batch][rows][N].
template <int LOGM, bool NARROW = false, int F64 = 0>
__global__ void __launch_bounds__(ntt_threads_c(LOGM), 4)
    small_ntt_kernel(const int8_t *__restrict__ smp, u64 *__restrict__ out, uint32_t rows, const DevMod *__restrict__ mods,
                     const u64x2 *__restrict__ tw) {
    FHE_DYN_SMEM(u64, lds);
    constexpr int T = ntt_threads_c(LOGM);
    constexpr int M = 1 << LOGM;
    const uint32_t tid = threadIdx.x;
    const uint32_t b = to_sgpr(blockIdx.x / rows);
    const uint32_t r = blockIdx.x - b * rows;
    const DevMod md = mods[r];
    u64x2 *dst = reinterpret_cast<u64x2 *>(out + ((u64)b * rows + r) * M);
    small_row_ntt<LOGM, T, NARROW, F64>(lds, tw + (u64)r * M, md, tid, smp + (u64)b * M,
                                        [&](uint32_t i, u64 x, u64 y) { dst[i >> 1] = u64x2{x, y}; });
}

// The per-coefficient steps of the encryptions: the whole-row kernels call these on the .x and .y of a pair (the
// plaintext addend under their uniform branch on its pointer), encrypt_combine_ew_kernel once per word.  For secret-key
// encryption that is the epilogue but for the plaintext addend.  For public-key encryption only the single steps are
// shared, not the epilogue: its composition c0 = u pk0 + e1 + m, c1 = u pk1 + e2 is spread over encrypt_pk_kernel's three
// stages and written out in encrypt_combine_ew_kernel (one combine returning {c0, c1} cost that kernel a VGPR).
// SecretKey::encrypt_poly: c0 = e - a s, before the plaintext
__device__ __forceinline__ u64 encrypt_sk_combine(u64 e, u64 a, u64 s, const DevMod &md) {
    return sub_mod(e, mul_mod(a, s, md), md.p);
}
// PublicKey::try_encrypt, stage 0: the partial u pk_j, before its error (and the plaintext)
__device__ __forceinline__ u64 encrypt_pk_combine(u64 u, u64 key, const DevMod &md) { return mul_mod(u, key, md); }
// a further addend of a ciphertext part: the plaintext word, or stage 1 / 2's error on the partial
__device__ __forceinline__ u64 encrypt_plus(u64 c, u64 v, const DevMod &md) { return add_mod(c, v, md.p); }

// SecretKey::encrypt_poly: one workgroup per (item, row).  e [batch][N] int8; a [batch][rows][N] (seed_expand_kernel's
// rows); s_ntt [rows][N]; pt [batch][rows][N] (pt_stride 0: one for the batch; null: the zero plaintext).
// out[b][0][r] = NTT(e) - a (.) s + pt, out[b][1][r] = a.
template <int LOGM, bool NARROW = false, int F64 = 0>
__global__ void __launch_bounds__(ntt_threads_c(LOGM), 4)
    encrypt_sk_kernel(const int8_t *__restrict__ e, const u64 *__restrict__ a, const u64 *__restrict__ s_ntt,
                      const u64 *__restrict__ pt, u64 pt_stride, u64 *__restrict__ out, uint32_t rows,
                      const DevMod *__restrict__ mods, const u64x2 *__restrict__ tw) {
    FHE_DYN_SMEM(u64, lds);
    constexpr int T = ntt_threads_c(LOGM);
    constexpr int M = 1 << LOGM;
    const uint32_t tid = threadIdx.x;
    const uint32_t b = to_sgpr(blockIdx.x / rows);
    const uint32_t r = blockIdx.x - b * rows;
    const DevMod md = mods[r];
    const u64x2 *ar = reinterpret_cast<const u64x2 *>(a + ((u64)b * rows + r) * M);
    const u64x2 *sr = reinterpret_cast<const u64x2 *>(s_ntt + (u64)r * M);
    const u64x2 *pr = pt ? reinterpret_cast<const u64x2 *>(pt + (u64)b * pt_stride + (u64)r * M) : nullptr;
    u64x2 *o0 = reinterpret_cast<u64x2 *>(out + ((u64)b * 2 * rows + r) * M);
    u64x2 *o1 = o0 + (u64)rows * M / 2;
    small_row_ntt<LOGM, T, NARROW, F64>(lds, tw + (u64)r * M, md, tid, e + (u64)b * M, [&](uint32_t i, u64 x, u64 y) {
        const u64x2 av = ar[i >> 1], sv = sr[i >> 1];
        u64x2 c{encrypt_sk_combine(x, av.x, sv.x, md), encrypt_sk_combine(y, av.y, sv.y, md)};
        if (pr) {
            const u64x2 m = pr[i >> 1];
            c = u64x2{encrypt_plus(c.x, m.x, md), encrypt_plus(c.y, m.y, md)};
        }
        o0[i >> 1] = c;
        o1[i >> 1] = av;
    });
}

// PublicKey::try_encrypt: one workgroup per (item, row), one transform per launch, launched for stage = 0, 1, 2 in
// turn on one stream.  smp [batch][3][N] int8 = u, e1, e2; pk [2][rows][N].  Stage 0 transforms u and stores the
// partials u (.) pk0, u (.) pk1 into out; stage 1 adds NTT(e1) (+ pt) to c0, stage 2 adds NTT(e2) to c1.  (One
// workgroup holds one LDS tile; the three transforms in one kernel -- unrolled or in a rolled loop -- overlap in
// registers and spill at every tile size, so the partials go through `out` between launches instead.)
template <int LOGM, bool NARROW = false, int F64 = 0>
__global__ void __launch_bounds__(ntt_threads_c(LOGM), 4)
    encrypt_pk_kernel(const int8_t *__restrict__ smp, const u64 *__restrict__ pk, const u64 *__restrict__ pt,
                      u64 pt_stride, u64 *__restrict__ out, uint32_t rows, const DevMod *__restrict__ mods,
                      const u64x2 *__restrict__ tw, uint32_t stage) {
    FHE_DYN_SMEM(u64, lds);
    constexpr int T = ntt_threads_c(LOGM);
    constexpr int M = 1 << LOGM;
    const uint32_t tid = threadIdx.x;
    const uint32_t b = to_sgpr(blockIdx.x / rows);
    const uint32_t r = blockIdx.x - b * rows;
    const DevMod md = mods[r];
    u64x2 *o0 = reinterpret_cast<u64x2 *>(out + ((u64)b * 2 * rows + r) * M);
    u64x2 *o1 = o0 + (u64)rows * M / 2;
    const int8_t *src = smp + ((u64)b * 3 + stage) * M;
    if (stage == 0) {
        const u64x2 *k0 = reinterpret_cast<const u64x2 *>(pk + (u64)r * M);
        const u64x2 *k1 = k0 + (u64)rows * M / 2;
        small_row_ntt<LOGM, T, NARROW, F64>(lds, tw + (u64)r * M, md, tid, src, [&](uint32_t i, u64 x, u64 y) {
            const u64x2 p0 = k0[i >> 1], p1 = k1[i >> 1];
            o0[i >> 1] = u64x2{encrypt_pk_combine(x, p0.x, md), encrypt_pk_combine(y, p0.y, md)};
            o1[i >> 1] = u64x2{encrypt_pk_combine(x, p1.x, md), encrypt_pk_combine(y, p1.y, md)};
        });
        return;
    }
    u64x2 *o = stage == 1 ? o0 : o1;
    const u64x2 *pr = stage == 1 && pt ? reinterpret_cast<const u64x2 *>(pt + (u64)b * pt_stride + (u64)r * M) : nullptr;
    small_row_ntt<LOGM, T, NARROW, F64>(lds, tw + (u64)r * M, md, tid, src, [&](uint32_t i, u64 x, u64 y) {
        u64x2 c = o[i >> 1];
        c = u64x2{encrypt_plus(c.x, x, md), encrypt_plus(c.y, y, md)};
        if (pr) {   // (stage 1 with a plaintext: the addend of c0)
            const u64x2 m = pr[i >> 1];
            c = u64x2{encrypt_plus(c.x, m.x, md), encrypt_plus(c.y, m.y, md)};
        }
        o[i >> 1] = c;
    });
}

// The sample lift as an element-wise pass: smp [npolys][N] int8 -> out [npolys][rows][N] mod q_r;
// total = npolys * rows * 2^logn.
__global__ void small_lift_ew_kernel(const int8_t *__restrict__ smp, u64 *__restrict__ out, uint32_t rows,
                                     const DevMod *__restrict__ mods, uint32_t logn, u64 total) {
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const u64 row = gid >> logn, j = gid & ((1ull << logn) - 1);
    const u64 poly = row / rows;
    out[gid] = lift_small(smp[(poly << logn) + j], mods[row % rows].p);
}

// The epilogues of encrypt_sk_kernel (pk == 0) and encrypt_pk_kernel (pk == 1) as an element-wise pass over the
// transformed samples x [batch][k][rows][N] (k = 1: e; k = 3: u, e1, e2).  key: s_ntt [rows][N] (sk) or pk [2][rows][N];
// a [batch][rows][N] (sk only).  total = batch * rows * 2^logn.
__global__ void encrypt_combine_ew_kernel(const u64 *__restrict__ x, const u64 *__restrict__ a, const u64 *__restrict__ key,
                                          const u64 *__restrict__ pt, u64 pt_stride, u64 *__restrict__ out, uint32_t rows,
                                          const DevMod *__restrict__ mods, uint32_t logn, uint32_t pk, u64 total) {
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const u64 pl = (u64)rows << logn;
    const u64 b = gid / pl, off = gid - b * pl;
    const DevMod md = mods[off >> logn];
    u64 *o = out + 2 * b * pl + off;
    const u64 m = pt ? pt[b * pt_stride + off] : 0;
    if (pk) {
        const u64 *xb = x + 3 * b * pl + off;
        const u64 u = xb[0];
        o[0] = encrypt_plus(encrypt_plus(encrypt_pk_combine(u, key[off], md), xb[pl], md), m, md);
        o[pl] = encrypt_plus(encrypt_pk_combine(u, key[pl + off], md), xb[2 * pl], md);
    } else {
        const u64 av = a[gid];
        o[0] = encrypt_plus(encrypt_sk_combine(x[gid], av, key[off], md), m, md);
        o[pl] = av;
    }
}

}  // namespace k
}  // namespace fhe
