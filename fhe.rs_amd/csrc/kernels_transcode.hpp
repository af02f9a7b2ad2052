// kernels_transcode.hpp -- plaintexts from packed bits (fhe-util's transcode_from_bytes / transcode_to_bytes /
// transcode_bidirectional, crates/fhe-util/src/lib.rs:71-190, as the PIR examples use them:
// crates/fhe/examples/util.rs:97-145 encode_database, sealpir.rs:176-200 the fold, sealpir.rs:231-273 and mulpir.rs:195 the
// client's way back).  All three are one operation on a bit stream: the low in_bits of every input element laid end to
// end, least significant bit first; output element k is stream bits [k out_bits, (k + 1) out_bits), bits past the end of
// the stream read as zero.
//   transcode_load         element k of that stream, from uint8_t or u64 elements bounded by an element count
//   encode_stream_kernel   encode_lift_kernel (kernels_encode.hpp) with the source word of each coefficient taken from
//                          the loader instead of a u64 array: Plaintext::try_encode(Encoding::poly_at_level) of the
//                          transcoded values without an unpacked copy in HBM
//   transcode_ew_kernel    the loader element-wise, into uint8_t or u64 elements: the public transcode call, and the
//                          values of rows larger than one LDS tile (N >= 32768) ahead of encode_lift_ew_kernel
// No packed bit decides an address: the positions read follow from the geometry alone.
#pragma once
#include "kernels_encode.hpp"

namespace fhe {
namespace k {

// Element k (out_bits bits) of the stream made of the low in_bits of src[0 .. count).  E = u64: in_bits in 1 ... 64;
// E = uint8_t: in_bits in 1 ... 8.  out_bits in 1 ... 64.  The caller keeps count * in_bits below 2^64; every offset is
// formed in 64 bits.
//
// No read falls outside [src, src + count), at any alignment of src.
//   General path (u64 elements; bytes that carry fewer than 8 bits): the elements touched are e0 = floor(k out_bits /
//   in_bits) and its successors while the value is incomplete, each compared with `count` before it is read.
//   Bytes of 8 bits: the value lies in the nb = ceil((off + out_bits) / 8) <= 9 bytes from b0 = floor(k out_bits / 8),
//   cut to the n <= nb of them below `count`.  Interior path: the one or two ALIGNED 8-byte words that cover those n
//   bytes are read with 8-byte loads only when both lie wholly inside [src, src + count) -- compared as addresses, so
//   the over-read is zero bytes, before src and after src + count alike, whatever src's alignment.  Otherwise (the first
//   and last up to 15 bytes of a source, and every source shorter than that) single-byte loads of exactly those n bytes.
//   Both paths give the same value: the word path only fetches the same bytes wider.
template <class E>
__device__ __forceinline__ u64 transcode_load(const E *__restrict__ src, u64 count, uint32_t in_bits, uint32_t out_bits,
                                              u64 k_) {
    const u64 bit = k_ * out_bits;
    const u64 omask = ~0ull >> (64 - out_bits);
    if constexpr (sizeof(E) == 1) {
        if (in_bits == 8) {
            const u64 b0 = bit >> 3;
            if (b0 >= count) return 0;
            const uint32_t off = (uint32_t)(bit & 7), nb = (off + out_bits + 7) >> 3;   // 1 ... 9 bytes
            const u64 avail = count - b0;
            const uint32_t n = avail < nb ? (uint32_t)avail : nb;
            const uint8_t *p = reinterpret_cast<const uint8_t *>(src) + b0;
            const u64 a = (u64)reinterpret_cast<uintptr_t>(p), wa = a & ~7ull;
            const u64 lo_addr = (u64)reinterpret_cast<uintptr_t>(src), hi_addr = lo_addr + count;
            const bool two = a + n > wa + 8;
            u64 lo, hi;
            if (wa >= lo_addr && wa + (two ? 16 : 8) <= hi_addr) {
                const u64 *w = reinterpret_cast<const u64 *>(p - (a - wa));
                const u64 w0 = w[0], w1 = two ? w[1] : 0;
                const uint32_t sh = (uint32_t)(a - wa) * 8;
                lo = sh ? (w0 >> sh) | (w1 << (64 - sh)) : w0;
                hi = sh ? w1 >> sh : w1;
            } else {
                lo = 0;
                for (uint32_t i = 0; i < 8; i++)
                    if (i < n) lo |= (u64)p[i] << (8 * i);
                hi = n == 9 ? (u64)p[8] : 0;
            }
            u64 v = lo >> off;
            if (off) v |= hi << (64 - off);   // (a ninth byte means off > 0; only its low `off` bits are below bit 64)
            return v & omask;
        }
    }
    u64 e = in_bits == 64 ? bit >> 6 : (bit >> 32) ? bit / in_bits : (u64)((uint32_t)bit / in_bits);
    if (e >= count) return 0;
    const uint32_t off = (uint32_t)(bit - e * in_bits);
    const u64 imask = ~0ull >> (64 - in_bits);
    u64 v = ((u64)src[e] & imask) >> off;
    uint32_t have = in_bits - off;
    while (have < out_bits && ++e < count) {
        v |= ((u64)src[e] & imask) << have;   // (have < 64 here; bits beyond 64 belong to the next value)
        have += in_bits;
    }
    return v & omask;
}

// The source of encode_stream_kernel: per item `nseg` segments of `seg_len` elements (in_bits each), segment s of item b
// `(b nseg + s) seg_stride` elements into `src`; a segment gives M = ceil(seg_len in_bits / nbits) values of nbits bits.
// The item's value stream is the segments' values appended; coefficient j of plaintext p is value v = p N + j: segment
// v / M at position v % M, zero from nseg M on.  Nothing is read from element `total` on (those read as zero): a short
// last item and items wholly past the end of the source.  Then the steps of lift_load.
struct StreamSrc {
    const void *src;
    u64 total, nseg, seg_len, seg_stride, M;   // (M >= 1: an empty stream is nseg == 0)
    uint32_t is_bytes, in_bits, nbits, nplain;
    DevMod tm;
    u64x2 qmt;
    uint32_t mul_t;
    const u64x2 *delta;
};
__device__ __forceinline__ u64 stream_value(const StreamSrc &ss, u64 b, u64 seg, u64 pos) {
    if (seg >= ss.nseg) return 0;
    const u64 start = (b * ss.nseg + seg) * ss.seg_stride;
    if (start >= ss.total) return 0;
    const u64 left = ss.total - start, cnt = left < ss.seg_len ? left : ss.seg_len;
    if (ss.is_bytes) return transcode_load(static_cast<const uint8_t *>(ss.src) + start, cnt, ss.in_bits, ss.nbits, pos);
    return transcode_load(static_cast<const u64 *>(ss.src) + start, cnt, ss.in_bits, ss.nbits, pos);
}
// (s0, r0) = (v0 / M, v0 % M) of the plaintext's first value, j < N: no 64-bit division per lane
__device__ __forceinline__ u64 stream_coeff(const StreamSrc &ss, u64 b, u64 s0, u64 r0, uint32_t j) {
    u64 seg = s0, pos = r0 + j;
    if (pos >= ss.M) {
        pos -= ss.M;
        seg++;
        if (pos >= ss.M) {   // (then M <= pos < N: both fit 32 bits)
            const uint32_t q = (uint32_t)pos / (uint32_t)ss.M;
            seg += q;
            pos -= (u64)q * ss.M;
        }
    }
    return stream_value(ss, b, seg, pos);
}

// One workgroup per (item, plaintext, row): blockIdx.x = ((b nplain + p) rows + r); out [batch][nplain][rows][N] in Ntt
// form (N = 2^LOGM <= 16384).  NARROW / F64 as encode_lift_kernel.  The loader feeds the first pass directly from
// LOGM = 13 on; below that it is staged through the tile in a rolled loop (the loader form spills at LOGM = 12, as
// ksk_load_kernel's does).
template <int LOGM, bool NARROW = false, int F64 = 0>
__global__ void __launch_bounds__(ntt_threads_c(LOGM), 4)
    encode_stream_kernel(StreamSrc ss, u64 *__restrict__ out, uint32_t rows, const DevMod *__restrict__ mods,
                         const u64x2 *__restrict__ tw) {
    FHE_DYN_SMEM(u64, lds);
    constexpr int T = ntt_threads_c(LOGM);
    constexpr int M = 1 << LOGM;
    constexpr int CH = tile_chunks_c(LOGM, T);
    const uint32_t tid = threadIdx.x;
    const uint32_t item = to_sgpr(blockIdx.x / rows);   // b * nplain + p
    const uint32_t r = blockIdx.x - item * rows;
    const uint32_t b = to_sgpr(item / ss.nplain), p = item - b * ss.nplain;
    const u64 v0 = (u64)p << LOGM, s0 = v0 / ss.M, r0 = v0 - s0 * ss.M;
    const DevMod md = mods[r];
    u64 *dst = out + ((u64)item * rows + r) * M;
    const u64x2 *twr = tw + (u64)r * M;
    auto word = [&](uint32_t j) {
        return lift_steps(stream_coeff(ss, b, s0, r0, j), ss.tm, ss.qmt, ss.mul_t, ss.delta, r, md);
    };
    if constexpr (F64 > 0) {
        const PM pmf = make_pm_f64(md);
        const PF pf = pf_of(pmf);
        if constexpr (LOGM > 12) {
            auto ld = [&](uint32_t j, uint32_t) { return bits_of_f64(f64_from_u64(word(j))); };
            ntt_fwd_lds<LOGM, T, GMAX, true, true, -F64>(lds, twr, 1, pmf, tid, ld);
        } else {
            for (uint32_t j = tid; j < (uint32_t)M; j += T) lds[padi(j)] = bits_of_f64(f64_from_u64(word(j)));
            FHE_BARRIER();
            ntt_fwd_lds<LOGM, T, GMAX, true, true, -F64>(lds, twr, 1, pmf, tid);
        }
        lds_to_tile<CH, M, T>(lds, dst, tid, [&](u64 v) { return to_u64_canonical(f64_of_bits(v), pf); });
    } else {
        const PM pm = make_pm(md);
        if constexpr (LOGM > 12) {
            auto ld = [&](uint32_t j, uint32_t) { return word(j); };
            ntt_fwd_lds<LOGM, T, GMAX, true, true, (NARROW ? 1 : 0)>(lds, twr, 1, pm, tid, ld);
        } else {
            for (uint32_t j = tid; j < (uint32_t)M; j += T) lds[padi(j)] = word(j);
            FHE_BARRIER();
            ntt_fwd_lds<LOGM, T, GMAX, NARROW, true, (NARROW ? 1 : 0)>(lds, twr, 1, pm, tid);
        }
        const u64 q = md.p, p2 = md.p2, p4 = p2 << 1, p8 = p2 << 2, np4 = pm.np2 << 1, np8 = pm.np2 << 2;
        lds_to_tile<CH, M, T>(lds, dst, tid, [&](u64 v) {
            if constexpr (NARROW) v = csub_n(csub_n(v, p8, np8), p4, np4);   // < 16p -> < 4p
            return csub_n(csub_n(v, p2, pm.np2), q, pm.np);
        });
    }
}

// Rows of `nin` elements -> rows of `nout` elements, one lane per output element: row i starts i in_stride elements
// into `in` (nothing is read from element total_in on) and is written at (i / grp) out_stride + (i % grp) nout of `out`
// (grp rows appended per output item: the segments of an item).  Bytes on either side by is_bytes flags.
// grid.x = rows * bpr, bpr = ceil(nout / blockDim.x): the row is uniform per workgroup.
struct TranscodeIo {
    const void *in;
    void *out;
    u64 total_in, in_stride, nin, nout, grp, out_stride;
    uint32_t in_bytes, in_bits, out_bytes, out_bits, bpr;
};
__global__ void __launch_bounds__(256) transcode_ew_kernel(TranscodeIo io) {
    const uint32_t row = to_sgpr(blockIdx.x / io.bpr);
    const u64 k_ = (u64)(blockIdx.x - row * io.bpr) * blockDim.x + threadIdx.x;
    if (k_ >= io.nout) return;
    const u64 start = (u64)row * io.in_stride;
    u64 v = 0;
    if (start < io.total_in) {
        const u64 left = io.total_in - start, cnt = left < io.nin ? left : io.nin;
        v = io.in_bytes ? transcode_load(static_cast<const uint8_t *>(io.in) + start, cnt, io.in_bits, io.out_bits, k_)
                        : transcode_load(static_cast<const u64 *>(io.in) + start, cnt, io.in_bits, io.out_bits, k_);
    }
    const u64 item = (u64)row / io.grp, o = item * io.out_stride + ((u64)row - item * io.grp) * io.nout + k_;
    if (io.out_bytes) static_cast<uint8_t *>(io.out)[o] = (uint8_t)v;
    else static_cast<u64 *>(io.out)[o] = v;
}

}  // namespace k
}  // namespace fhe
