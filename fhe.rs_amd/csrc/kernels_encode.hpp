// kernels_encode.hpp -- BFV plaintext encoding and decoding (PlaintextVec::try_encode, Plaintext::to_poly, the
// decoders) and ct +- pt.  The transforms are the ntt_kernel passes (kernels_passes.hpp) behind loaders / stores of
// their own:
//   encode_simd_t_kernel   SIMD index map (gather) + NttOperator::backward mod t     F/bfv/plaintext_vec.rs:70-102
//   encode_lift_kernel     lift into every q_i (x delta_i) + NttOperator::forward    F/bfv/plaintext.rs:172-196
//   decode_simd_kernel     NttOperator::forward mod t + index map (scatter via LDS)  F/bfv/plaintext.rs:157-170
//   perm_reduce_kernel / encode_lift_ew_kernel   the element-wise forms of those loaders, for rows larger than one
//                          LDS tile (N >= 32768), around launch_ntt
//   add_plain_kernel       ct +- pt                                                 F/bfv/ops/mod.rs:71-108, 166-203
// Every input word is reduced mod t on load (reduce_u64 accepts any u64), so the transforms only see canonical residues.
#pragma once
#include "kernels_passes.hpp"

namespace fhe {
namespace k {

// One workgroup per item (whole rows only, N = 2^LOGM <= 16384): tile[j] = values[b][inv_map[j]] mod t (zero when
// inv_map[j] >= nvalues), the inverse transform mod t with `nscale` = {c, shoup} in place of {N^-1, shoup} and
// `zscale` = {z_last c, shoup} (F64: the double pairs of the same constants), canonical out[b][N].
template <int LOGM, bool NARROW = false, int F64 = 0>
__global__ void __launch_bounds__(ntt_threads_c(LOGM), 4)
    encode_simd_t_kernel(const u64 *__restrict__ values, u64 nvalues, const uint32_t *__restrict__ inv_map,
                         u64 *__restrict__ out, const DevMod *__restrict__ tmod, const u64x2 *__restrict__ itw,
                         u64x2 nscale, u64x2 zscale) {
    FHE_DYN_SMEM(u64, lds);
    constexpr int T = ntt_threads_c(LOGM);
    constexpr int M = 1 << LOGM;
    constexpr int CH = tile_chunks_c(LOGM, T);
    const uint32_t tid = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const DevMod md = tmod[0];
    const u64 *src = values + (u64)b * nvalues;
    u64 *dst = out + (u64)b * M;
    InvTwFirst<LOGM, T> tw0;
    auto at = [&](uint32_t j) -> u64 {
        const uint32_t s = inv_map[j];
        return s < nvalues ? reduce_u64(src[s], md) : 0;
    };
    if constexpr (F64 > 0) {
        const PM pmf = make_pm_f64(md);
        const PF pf = pf_of(pmf);
        for (uint32_t j = tid; j < (uint32_t)M; j += T) lds[padi(j)] = bits_of_f64(f64_from_u64(at(j)));
        inv_tw_load(tw0, itw, LOGM, 0, tid);   // (after the gather: its registers are free again)
        FHE_BARRIER();
        ntt_inv_lds<LOGM, T, 0, 0, false, F64>(lds, itw, LOGM, 0, pmf, tid, true, nscale, zscale, tw0);
        lds_to_tile<CH, M, T>(lds, dst, tid, [&](u64 v) { return to_u64_canonical(f64_of_bits(v), pf); });
    } else {
        const PM pm = make_pm(md);
        for (uint32_t j = tid; j < (uint32_t)M; j += T) lds[padi(j)] = at(j);
        inv_tw_load(tw0, itw, LOGM, 0, tid);
        FHE_BARRIER();
        ntt_inv_lds<LOGM, T, 0, 0, NARROW>(lds, itw, LOGM, 0, pm, tid, true, nscale, zscale, tw0);
        lds_to_tile<CH, M, T>(lds, dst, tid, [&](u64 v) { return csub_n(v, md.p, pm.np); });
    }
}

// The loader shared by both lift forms: coefficient j of item b's mod-t row (zero from nvalues on), reduced mod t,
// times q_mod_t mod t when `mul_t` (Poly to_poly: the SIMD path has folded that factor into its inverse transform),
// reduced into q_i and times delta_i when `delta` is given.
struct LiftSrc {
    const u64 *src;
    u64 stride, nvalues;
    DevMod tm;
    u64x2 qmt;             // {q_mod_t, shoup} mod t, applied when mul_t != 0
    uint32_t mul_t;
    const u64x2 *delta;    // [rows] {delta_i, shoup} mod q_i, or null
};
// (the steps on one source word `w`, shared with the bit-stream loader of kernels_transcode.hpp)
__device__ __forceinline__ u64 lift_steps(u64 w, const DevMod &tm, const u64x2 &qmt, uint32_t mul_t,
                                          const u64x2 *__restrict__ delta, uint32_t r, const DevMod &md) {
    u64 v = reduce_u64(w, tm);
    if (mul_t) v = mul_shoup(v, qmt.x, qmt.y, tm.p);
    v = reduce_u64(v, md);
    if (delta) {
        const u64x2 d = delta[r];
        v = mul_shoup(v, d.x, d.y, md.p);
    }
    return v;
}
__device__ __forceinline__ u64 lift_load(const LiftSrc &ls, uint32_t b, uint32_t j, uint32_t r, const DevMod &md) {
    if (j >= ls.nvalues) return 0;
    return lift_steps(ls.src[(u64)b * ls.stride + j], ls.tm, ls.qmt, ls.mul_t, ls.delta, r, md);
}

// One workgroup per (item, row): the lifted row in Ntt form, out[b][r][N] (N = 2^LOGM <= 16384).  NARROW: every modulus
// of the launch below 2^60 (the bound-tracked forward passes, as ntt_kernel); F64: every modulus below 2^(53 - F64).
template <int LOGM, bool NARROW = false, int F64 = 0>
__global__ void __launch_bounds__(ntt_threads_c(LOGM), 4)
    encode_lift_kernel(LiftSrc ls, u64 *__restrict__ out, uint32_t rows, const DevMod *__restrict__ mods,
                       const u64x2 *__restrict__ tw) {
    FHE_DYN_SMEM(u64, lds);
    constexpr int T = ntt_threads_c(LOGM);
    constexpr int M = 1 << LOGM;
    constexpr int CH = tile_chunks_c(LOGM, T);
    const uint32_t tid = threadIdx.x;
    const uint32_t b = to_sgpr(blockIdx.x / rows);
    const uint32_t r = blockIdx.x - b * rows;
    const DevMod md = mods[r];
    u64 *dst = out + ((u64)b * rows + r) * M;
    const u64x2 *twr = tw + (u64)r * M;
    if constexpr (F64 > 0) {
        const PM pmf = make_pm_f64(md);
        const PF pf = pf_of(pmf);
        auto ld = [&](uint32_t i, uint32_t) { return bits_of_f64(f64_from_u64(lift_load(ls, b, i, r, md))); };
        ntt_fwd_lds<LOGM, T, GMAX, true, true, -F64>(lds, twr, 1, pmf, tid, ld);
        lds_to_tile<CH, M, T>(lds, dst, tid, [&](u64 v) { return to_u64_canonical(f64_of_bits(v), pf); });
    } else {
        const PM pm = make_pm(md);
        auto ld = [&](uint32_t i, uint32_t) { return lift_load(ls, b, i, r, md); };
        ntt_fwd_lds<LOGM, T, GMAX, true, true, (NARROW ? 1 : 0)>(lds, twr, 1, pm, tid, ld);
        const u64 p = md.p, p2 = md.p2, p4 = p2 << 1, p8 = p2 << 2, np4 = pm.np2 << 1, np8 = pm.np2 << 2;
        lds_to_tile<CH, M, T>(lds, dst, tid, [&](u64 v) {
            if constexpr (NARROW) v = csub_n(csub_n(v, p8, np8), p4, np4);   // < 16p -> < 4p
            return csub_n(csub_n(v, p2, pm.np2), p, pm.np);
        });
    }
}

// One workgroup per item (whole rows): the forward transform mod t of coeffs[b] (reduced mod t on load), then
// out[b][i] = X[map[i]] read from the LDS tile, so the global stores stay coalesced.
template <int LOGM, bool NARROW = false, int F64 = 0>
__global__ void __launch_bounds__(ntt_threads_c(LOGM), 4)
    decode_simd_kernel(const u64 *__restrict__ coeffs, const uint32_t *__restrict__ map, u64 *__restrict__ out,
                       const DevMod *__restrict__ tmod, const u64x2 *__restrict__ tw) {
    FHE_DYN_SMEM(u64, lds);
    constexpr int T = ntt_threads_c(LOGM);
    constexpr int M = 1 << LOGM;
    const uint32_t tid = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const DevMod md = tmod[0];
    const u64 *src = coeffs + (u64)b * M;
    u64 *dst = out + (u64)b * M;
    if constexpr (F64 > 0) {
        const PM pmf = make_pm_f64(md);
        const PF pf = pf_of(pmf);
        auto ld = [&](uint32_t i, uint32_t) { return bits_of_f64(f64_from_u64(reduce_u64(src[i], md))); };
        ntt_fwd_lds<LOGM, T, GMAX, true, true, -F64>(lds, tw, 1, pmf, tid, ld);
        for (uint32_t i = tid; i < (uint32_t)M; i += T) dst[i] = to_u64_canonical(f64_of_bits(lds[padi(map[i])]), pf);
    } else {
        const PM pm = make_pm(md);
        // (the reduction staged through the tile, and no twiddle prefetch on the general passes: either one in the
        // first pass spills at LOGM = 12)
        tile_to_lds<tile_chunks_c(LOGM, T), M, T>(lds, src, tid, [&](u64 v) { return reduce_u64(v, md); });
        FHE_BARRIER();
        ntt_fwd_lds<LOGM, T, GMAX, NARROW, true, (NARROW ? 1 : 0)>(lds, tw, 1, pm, tid);
        const u64 p = md.p, p2 = md.p2, p4 = p2 << 1, p8 = p2 << 2, np4 = pm.np2 << 1, np8 = pm.np2 << 2;
#pragma unroll 4
        for (uint32_t i = tid; i < (uint32_t)M; i += T) {
            u64 v = lds[padi(map[i])];
            if constexpr (NARROW) v = csub_n(csub_n(v, p8, np8), p4, np4);
            dst[i] = csub_n(csub_n(v, p2, pm.np2), p, pm.np);
        }
    }
}

// out[b][j] = in[b][map[j]] mod t (map == null: the identity), zero where the source index is >= nvalid; `stride` is
// the item stride of `in`.  One lane per output word; total = batch * 2^logn.
__global__ void perm_reduce_kernel(const u64 *__restrict__ in, u64 stride, u64 nvalid, const uint32_t *__restrict__ map,
                                   u64 *__restrict__ out, DevMod tm, uint32_t logn, u64 total) {
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const u64 b = gid >> logn, j = gid & ((1ull << logn) - 1);
    const u64 s = map ? (u64)map[j] : j;
    out[gid] = s < nvalid ? reduce_u64(in[b * stride + s], tm) : 0;
}

// The lift loader as an element-wise pass: out[b][r][j] over `rows` moduli; total = batch * rows * 2^logn.
__global__ void encode_lift_ew_kernel(LiftSrc ls, u64 *__restrict__ out, uint32_t rows, const DevMod *__restrict__ mods,
                                      uint32_t logn, u64 total) {
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const u64 row = gid >> logn;
    const uint32_t b = (uint32_t)(row / rows), r = (uint32_t)(row % rows);
    out[gid] = lift_load(ls, b, (uint32_t)(gid & ((1ull << logn) - 1)), r, mods[r]);
}

// out[b][0] = ct[b][0] +- pt[b] (pt_stride 0: one pt for the batch); parts 1.. copied when `copy` (out != ct).
// grid = (ceil(L N / block), batch); pl = L N.
__global__ void add_plain_kernel(const u64 *ct, const u64 *__restrict__ pt, u64 pt_stride, u64 *out,
                                 const DevMod *__restrict__ mods, uint32_t nparts, uint32_t logn, u64 pl, uint32_t subtract,
                                 uint32_t copy) {
    const u64 off = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (off >= pl) return;
    const u64 b = blockIdx.y;
    const u64 p = mods[off >> logn].p;
    const u64 *c = ct + b * nparts * pl + off;
    u64 *o = out + b * nparts * pl + off;
    const u64 x = c[0], y = pt[b * pt_stride + off];
    o[0] = subtract ? sub_mod(x, y, p) : add_mod(x, y, p);
    if (copy)
        for (uint32_t i = 1; i < nparts; i++) o[(u64)i * pl] = c[(u64)i * pl];
}

}  // namespace k
}  // namespace fhe
