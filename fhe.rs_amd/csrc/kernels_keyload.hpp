// kernels_keyload.hpp -- key-switching keys from their wire bytes (KeySwitchingKey::try_convert_from(&KeySwitchingKeyProto),
// F/bfv/keys/key_switching_key.rs:387-482).  A message holds c0 as `ndigits` bit-packed PowerBasis polynomials over the
// key context and either the c1 polynomials in the same form or the 32-byte seed K they expand from (generate_c1):
//   ksk_dseeds_kernel       the per-digit seeds of ChaCha8Rng::from_seed(K) (the second half of ksk_seeds_kernel)
//   ksk_load_kernel         one row of c0 / c1: unpack (the loader of the transform), NttOperator::forward, and the
//                           canonical word, its Shoup twin and the F64 word written into the handle in the epilogue
//   ksk_twin_ew_kernel      the twins and F64 words of Ntt words already in a handle, element-wise: the seeded c1
//                           (seed_expand_kernel writes it there) and rows larger than one LDS tile (N >= 32768:
//                           wire_unpack*_kernel into the handle, this kernel's compare alone, launch_ntt, this kernel)
// Every unpacked word is compared with its modulus; a word >= q_j raises one flag word per call, which the engine
// reads back once.  Key material on the wire is public: the compare is on public data, and still no address depends on it.
#pragma once
#include "kernels_keygen.hpp"

namespace fhe {
namespace k {

// One thread per (key, digit): seed_i = bytes [32 i, 32 i + 32) of ChaCha8Rng::from_seed(K[key]) (generate_c1).
// K [nkeys][32] -> dseeds [nkeys][ndigits][32].
__global__ void ksk_dseeds_kernel(const uint8_t *__restrict__ K, uint8_t *__restrict__ dseeds, uint32_t ndigits,
                                  uint32_t total) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const uint32_t key = gid / ndigits, i = gid - key * ndigits;
    uint32_t kk[8], w[16];
    seed_key(K + (u64)key * 32, kk);
    chacha8_block(kk, i >> 1, w);
    put_words(dseeds + (u64)gid * 32, w + 8 * (i & 1));
}

// Coefficient e of a packed row at byte granularity: stream bits [e nbits, (e + 1) nbits) of `row`.
// No over-read: the bytes touched are floor(e nbits / 8) ... floor(((e + 1) nbits - 1) / 8), and for e <= N - 1 the
// last of them is below N nbits / 8, the row's length -- so the last coefficient of the last row of a buffer ends
// inside it.  No alignment is assumed: single-byte loads.
__device__ __forceinline__ u64 wire_unpack_coeff_bytes(const uint8_t *__restrict__ row, uint32_t e, uint32_t nbits, u64 mask) {
    const u64 bit = (u64)e * nbits;
    const uint8_t *b = row + (bit >> 3);
    const uint32_t off = (uint32_t)(bit & 7), nb = (off + nbits + 7) >> 3;   // 1 ... 9 bytes
    u64 lo = 0;
    for (uint32_t k_ = 0; k_ < 8; k_++)
        if (k_ < nb) lo |= (u64)b[k_] << (8 * k_);
    u64 v = lo >> off;
    if (nb == 9) v |= (u64)b[8] << (64 - off);   // (nbits <= 62: a ninth byte means off >= 3)
    return v & mask;
}

// One workgroup per (part, key, digit, key row): blockIdx.x = (part * nkd + key * ndigits + digit) * rows + r with
// part 0 = c0, 1 = c1 (the grid has the second half only with an explicit c1).  c0b, c1b [nkeys][ndigits][poly_bytes]
// packed PowerBasis polynomials; rq from ksk_consts_kernel; out: the keys' buffers (wf: write the F64 words).
//
// Alignment.  words != 0 is the engine's statement that N >= 128 and both byte pointers are 16-byte aligned
// (ksk_load_wire checks it, as wire_deserialize does).  A row is N nbits / 8 bytes, a multiple of 16 from N = 128 on,
// so poly_bytes and every row offset are multiples of 16 too and each row starts on a 16-byte boundary: the 8-byte
// loads of wire_unpack_coeff are aligned.  Otherwise (N < 128, where a row of N = 8 is nbits bytes and starts at any
// byte, or a caller's pointer at any address) the row is read with single-byte loads.
// No over-read.  Word path: coefficient e reads word w = floor(e nbits / 64), and word w + 1 only when the
// coefficient reaches into it (off + nbits > 64); then bit 64 (w + 1) <= (e + 1) nbits - 1 < N nbits, so w + 1 is below
// N nbits / 64, the row's word count -- the second word of a straddling coefficient at the end of the last row exists.
// Byte path: see wire_unpack_coeff_bytes.  Both read inside [row, row + N nbits / 8) only.
template <int LOGM, bool NARROW = false, int F64 = 0>
__global__ void __launch_bounds__(ntt_threads_c(LOGM), 4)
    ksk_load_kernel(const uint8_t *__restrict__ c0b, const uint8_t *__restrict__ c1b, u64 poly_bytes, uint32_t words,
                    const u64x2 *__restrict__ rq, KskOutTable out, uint32_t ndigits, uint32_t rows, uint32_t nkd,
                    uint32_t wf, const DevMod *__restrict__ mods, const u64x2 *__restrict__ tw, uint32_t *__restrict__ flag) {
    FHE_DYN_SMEM(u64, lds);
    constexpr int T = ntt_threads_c(LOGM);
    constexpr int M = 1 << LOGM;
    constexpr int CH = tile_chunks_c(LOGM, T);
    const uint32_t tid = threadIdx.x;
    const uint32_t pkd = to_sgpr(blockIdx.x / rows);   // part * nkd + key * ndigits + digit
    const uint32_t r = blockIdx.x - pkd * rows;
    const uint32_t part = to_sgpr(pkd / nkd), kd = pkd - part * nkd;
    const uint32_t key = to_sgpr(kd / ndigits), i = kd - key * ndigits;
    const DevMod md = mods[r];
    const u64x2 rc = rq[r];
    const uint32_t nbits = wire_bits(md.p);
    const u64 mask = ~0ull >> (64 - nbits);
    const uint8_t *row = (part ? c1b : c0b) + (u64)kd * poly_bytes + wire_row_offset(mods, r, LOGM);
    const u64 *roww = reinterpret_cast<const u64 *>(row);   // (dereferenced under `words` only)
    const u64x2 *twr = tw + (u64)r * M;
    const KskOut o = out.k[key];
    const u64 off = ((u64)i * rows + r) * M;
    u64x2 *oc = reinterpret_cast<u64x2 *>((part ? o.c1 : o.c0) + off);
    u64x2 *os = reinterpret_cast<u64x2 *>((part ? o.c1s : o.c0s) + off);
    u64x2 *of = wf ? reinterpret_cast<u64x2 *>((part ? o.c1f : o.c0f) + off) : nullptr;
    uint32_t bad = 0;
    auto checked = [&](u64 v) {
        bad |= (uint32_t)(v >= md.p);
        return v;
    };
    auto epi = [&](uint32_t x_i, u64 x, u64 y) {
        oc[x_i >> 1] = u64x2{x, y};
        os[x_i >> 1] = u64x2{shoup_twin(x, rc.x, rc.y, md), shoup_twin(y, rc.x, rc.y, md)};
        if (of) of[x_i >> 1] = u64x2{f64_word(x), f64_word(y)};
    };
    // The transform as small_row_ntt runs it (kernels_encrypt.hpp), behind a loader that unpacks: on the word path the
    // first pass reads its coefficients straight from the packed row from LOGM = 13 on (staged through the tile below
    // that: the loader form spills at LOGM = 12, as small_row_ntt's does); the byte path always stages, in a rolled loop.
    if constexpr (F64 > 0) {
        const PM pmf = make_pm_f64(md);
        const PF pf = pf_of(pmf);
        auto staged = [&] {
            if (words)
                for (uint32_t e = tid; e < (uint32_t)M; e += T)
                    lds[padi(e)] = bits_of_f64(f64_from_u64(checked(wire_unpack_coeff(roww, e, nbits, mask))));
            else
                for (uint32_t e = tid; e < (uint32_t)M; e += T)
                    lds[padi(e)] = bits_of_f64(f64_from_u64(checked(wire_unpack_coeff_bytes(row, e, nbits, mask))));
            FHE_BARRIER();
            ntt_fwd_lds<LOGM, T, GMAX, true, true, -F64>(lds, twr, 1, pmf, tid);
        };
        if constexpr (LOGM > 12) {
            if (words) {
                auto ld = [&](uint32_t e, uint32_t) {
                    return bits_of_f64(f64_from_u64(checked(wire_unpack_coeff(roww, e, nbits, mask))));
                };
                ntt_fwd_lds<LOGM, T, GMAX, true, true, -F64>(lds, twr, 1, pmf, tid, ld);
            } else {
                staged();
            }
        } else {
            staged();
        }
        lds_pairs<CH, M, T>(lds, tid, [&](uint32_t e, u64 x, u64 y) {
            epi(e, to_u64_canonical(f64_of_bits(x), pf), to_u64_canonical(f64_of_bits(y), pf));
        });
    } else {
        const PM pm = make_pm(md);
        auto staged = [&] {
            if (words)
                for (uint32_t e = tid; e < (uint32_t)M; e += T) lds[padi(e)] = checked(wire_unpack_coeff(roww, e, nbits, mask));
            else
                for (uint32_t e = tid; e < (uint32_t)M; e += T)
                    lds[padi(e)] = checked(wire_unpack_coeff_bytes(row, e, nbits, mask));
            FHE_BARRIER();
            ntt_fwd_lds<LOGM, T, GMAX, NARROW, true, (NARROW ? 1 : 0)>(lds, twr, 1, pm, tid);
        };
        if constexpr (LOGM > 12) {
            if (words) {
                auto ld = [&](uint32_t e, uint32_t) { return checked(wire_unpack_coeff(roww, e, nbits, mask)); };
                ntt_fwd_lds<LOGM, T, GMAX, true, true, (NARROW ? 1 : 0)>(lds, twr, 1, pm, tid, ld);
            } else {
                staged();
            }
        } else {
            staged();
        }
        const u64 p = md.p, p2 = md.p2, p4 = p2 << 1, p8 = p2 << 2, np4 = pm.np2 << 1, np8 = pm.np2 << 2;
        auto canon = [&](u64 v) {
            if constexpr (NARROW) v = csub_n(csub_n(v, p8, np8), p4, np4);   // < 16p -> < 4p
            return csub_n(csub_n(v, p2, pm.np2), p, pm.np);
        };
        lds_pairs<CH, M, T>(lds, tid, [&](uint32_t e, u64 x, u64 y) { epi(e, canon(x), canon(y)); });
    }
    if (bad) *flag = 1u;   // (every writer stores the same word)
}

// The Shoup twins and F64 words of the Ntt words already in the handles' c0 (parts & 1) and c1 (parts & 2), one thread
// per 16 bytes of each; the same range check into the same flag.  check_only != 0: the compare alone -- the pass over the
// unpacked PowerBasis words of rows larger than one LDS tile, before their transform (after it every word is reduced).
// pairs = nkeys * ndigits * rows * N / 2.
__global__ void ksk_twin_ew_kernel(KskOutTable out, uint32_t parts, uint32_t check_only, const u64x2 *__restrict__ rq,
                                   uint32_t ndigits, uint32_t rows, uint32_t wf, const DevMod *__restrict__ mods,
                                   uint32_t logn, u64 pairs, uint32_t *__restrict__ flag) {
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= pairs) return;
    const u64 per_key = ((u64)ndigits * rows << logn) >> 1;   // pairs of one key array
    const uint32_t key = (uint32_t)(gid / per_key);
    const u64 pr = gid - (u64)key * per_key;   // pair index within the key array
    const uint32_t r = (uint32_t)(((pr << 1) >> logn) % rows);
    const DevMod md = mods[r];
    const u64x2 rc = rq[r];
    const KskOut o = out.k[key];
    uint32_t bad = 0;
    for (uint32_t part = 0; part < 2; part++) {
        if (!(parts & (1u << part))) continue;
        const u64x2 c = reinterpret_cast<const u64x2 *>(part ? o.c1 : o.c0)[pr];
        bad |= (uint32_t)(c.x >= md.p) | (uint32_t)(c.y >= md.p);
        if (check_only) continue;
        reinterpret_cast<u64x2 *>(part ? o.c1s : o.c0s)[pr] =
            u64x2{shoup_twin(c.x, rc.x, rc.y, md), shoup_twin(c.y, rc.x, rc.y, md)};
        if (wf) reinterpret_cast<u64x2 *>(part ? o.c1f : o.c0f)[pr] = u64x2{f64_word(c.x), f64_word(c.y)};
    }
    if (bad) *flag = 1u;
}

}  // namespace k
}  // namespace fhe
