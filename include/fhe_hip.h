/* fhe_hip.h -- C ABI of the MI355X-native RNS polynomial engine for fhe.rs' BFV hot path.
 *
 * This is the drop-in boundary: the entry points a `hip` cargo feature of fhe-math / fhe
 * would bind (see INTEGRATION.md for the Rust `extern "C"` block and the call-site patches).
 * fhe.rs has no FFI of its own; each entry point cites the Rust item it replaces
 * (paths relative to the reference repo: M/ = crates/fhe-math/src, F/ = crates/fhe/src).
 *
 * Conventions
 *  - All coefficient buffers are caller-owned, contiguous row-major u64 `[batch][...][L][N]`,
 *    exactly `fhe_math::rq::Poly`'s `Array2<u64>` layout (M/rq/mod.rs:126-133, 189-204) with
 *    outer batch dimensions.  Inputs and outputs are canonical residues in [0, q_i).
 *  - Plain entry points take HOST pointers and are synchronous.  `_dev` twins take DEVICE
 *    pointers plus a `hipStream_t` (passed as `void*`) and are stream-ordered.  Device buffers and
 *    streams come from the "device memory and streams" block below (or from any other HIP
 *    allocator in the process: the engine only sees pointers), so a host written in C, Rust, Go ...
 *    keeps polynomials resident on the GPU between calls without linking HIP itself.
 *  - Handles are opaque, immutable after creation and may be shared by concurrent callers
 *    working on different buffers (matches `Arc<Context>`, M/rq/context.rs:8-19).
 *  - Every function returns 0 (FHE_OK) or a negative `fhe_status`; nothing throws or aborts
 *    across the boundary.  `fhe_last_error()` gives a thread-local message.
 *  - Results are bit-identical to the reference CPU path on the same inputs and tables.
 */
#ifndef FHE_HIP_H
#define FHE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t fhe_status;

/* Status codes: 1:1 with the `Result` variants used on the path
 * (M/errors.rs:12-118, F/errors.rs:18-70) plus runtime/argument errors. */
enum {
    FHE_OK = 0,
    FHE_E_ARG = -1,                           /* null pointer, zero size, bad flag               */
    FHE_E_HIP = -2,                           /* HIP runtime error (message in fhe_last_error)   */
    FHE_E_INVALID_MODULUS = -3,               /* Error::InvalidModulus                            */
    FHE_E_INVALID_DEGREE = -4,                /* Error::InvalidPolynomialDegree                   */
    FHE_E_NTT_UNAVAILABLE = -5,               /* Error::NttOperatorUnavailable                    */
    FHE_E_CONTEXT_MISMATCH = -6,              /* Error::PolynomialContextMismatch                 */
    FHE_E_DEGREE_MISMATCH = -7,               /* Error::DegreeMismatch                            */
    FHE_E_NO_MORE_CONTEXT = -8,               /* Error::NoMoreContext                             */
    FHE_E_CONTEXT_NOT_REACHABLE = -9,         /* Error::ContextNotReachable                       */
    FHE_E_INVALID_SUBSTITUTION_EXPONENT = -10,/* Error::InvalidSubstitutionExponent               */
    FHE_E_PARAMETER_MISMATCH = -11,           /* fhe::Error::ParameterMismatch                    */
    FHE_E_INVALID_LEVEL = -12,                /* fhe::Error::InvalidLevel / InvalidContextLevel   */
    FHE_E_MUL_POLY_COUNT = -13,               /* CiphertextError::MultiplicationPolynomialCount   */
    FHE_E_EMPTY_MODULI = -14,                 /* Error::EmptyModuli                               */
    FHE_E_NON_COPRIME = -15,                  /* Error::NonCoprimeModuli                          */
    FHE_E_NOT_ENOUGH_PRIMES = -16,            /* ParametersError::NotEnoughPrimes                 */
    FHE_E_KEYSWITCH_UNSUPPORTED = -17,        /* EvaluationKeyError::KeySwitchingNotSupported     */
    FHE_E_NO_DEVICE = -18,                    /* compute call on a host-only (device = -1) handle */
    FHE_E_EMPTY_DOT_PRODUCT = -19,            /* Error::EmptyDotProduct / DotProductError::EmptyInput */
    FHE_E_INVALID_EXPANSION_SIZE = -20,       /* EvaluationKeyError::InvalidExpansionSize          */
    FHE_E_EXPANSION_UNSUPPORTED = -21,        /* EvaluationKeyError::Unsupported{Expansion} / Missing{GaloisKey} */
    FHE_E_SIMD_UNAVAILABLE = -22,             /* EncodingError::SimdUnavailable (F/bfv/plaintext.rs:157-170)     */
    FHE_E_TOO_MANY_VALUES = -23,              /* PlaintextError::TooManyValues (F/bfv/plaintext.rs:313-325)      */
    FHE_E_INVALID_VARIANCE = -24              /* Error::InvalidVariance (M/rq/mod.rs:303-309)                    */
};

typedef struct fhe_ctx fhe_ctx;       /* == rq::Context on one device   (M/rq/context.rs:9-19)        */
typedef struct fhe_scaler fhe_scaler; /* == rq::scaler::Scaler          (M/rq/scaler.rs:18-23)        */
typedef struct fhe_ksk fhe_ksk;       /* == bfv::KeySwitchingKey        (F/bfv/keys/key_switching_key.rs:22-46) */
typedef struct fhe_kskset fhe_kskset; /* the KeySwitchingKeys of many clients for one operation (keyed batches) */
typedef struct fhe_mul fhe_mul;       /* == bfv::Multiplicator          (F/bfv/ops/mul.rs:21-32)      */
typedef struct fhe_params fhe_params; /* == bfv::BfvParameters' level tables (F/bfv/parameters.rs:83-117) */
typedef struct fhe_encoder fhe_encoder; /* == BfvParameters' encoding tables (F/bfv/parameters.rs:598, 607-633, 711-725) */

const char *fhe_last_error(void);
const char *fhe_version(void);
/* Number of visible HIP devices (0 without a GPU).  Never fails. */
int fhe_device_count(void);

/* -------------------------------------------------- device memory and streams ---- */
/* What a non-HIP host needs to use the `_dev` entry points: `rq::Poly`'s `coefficients: Array2<u64>`
 * (M/rq/mod.rs:126-133) gets a device-resident shadow that lives across calls -- upload once,
 * chain multiply -> relinearise -> rotate -> switch_down on the device, download lazily (the Rust side of
 * this is `DevicePoly` / `DeviceCiphertext` in rust/fhe-math-hip).
 *  - A stream is a plain `hipStream_t` handed out as `void *` (non-blocking with respect to the null
 *    stream); NULL everywhere means the device's null stream.  Work on one stream runs in order.
 *  - `*_async` calls only enqueue: with pageable host memory HIP stages the bytes itself, with pinned
 *    host memory (fhe_host_alloc) the caller must keep the host buffer untouched until the stream
 *    reaches that point (fhe_stream_sync).  The plain twins additionally wait for the stream.
 *  - fhe_stream_destroy waits for the stream, then frees what the engine kept for it (its internal
 *    second stream and idle scratch blocks).  Handles (contexts, keys ...) are not tied to a stream. */
fhe_status fhe_buf_alloc(int device, size_t bytes, void **out);      /* hipMalloc on `device`           */
fhe_status fhe_buf_free(void *buf);                                   /* NULL is a no-op                  */
/* Stream-ordered twins (hipMallocFromPoolAsync / hipFreeAsync on a memory pool PRIVATE to this library, one per device,
 * told to keep freed blocks -- the device's default pool is left alone): the block may be used by work enqueued on `stream` after the call, and a free takes effect
 * behind the work already enqueued on `stream` -- no device synchronisation, unlike hipMalloc / hipFree.  Using the
 * block on another stream needs the caller's own ordering (events).  fhe_buf_free also accepts such a block (and waits);
 * fhe_buf_free_async is for blocks from fhe_buf_alloc_async only.  fhe_workspace_trim returns the pool's idle blocks. */
fhe_status fhe_buf_alloc_async(int device, size_t bytes, void *stream, void **out);
fhe_status fhe_buf_free_async(void *buf, void *stream);              /* NULL is a no-op                  */
fhe_status fhe_buf_upload(void *dst_dev, const void *src_host, size_t bytes, void *stream);
fhe_status fhe_buf_upload_async(void *dst_dev, const void *src_host, size_t bytes, void *stream);
fhe_status fhe_buf_download(void *dst_host, const void *src_dev, size_t bytes, void *stream);
fhe_status fhe_buf_download_async(void *dst_host, const void *src_dev, size_t bytes, void *stream);
fhe_status fhe_buf_copy_async(void *dst_dev, const void *src_dev, size_t bytes, void *stream);
fhe_status fhe_buf_zero_async(void *buf, size_t bytes, void *stream);  /* e.g. wiping a secret-dependent buffer */
fhe_status fhe_host_alloc(size_t bytes, void **out);                 /* pinned host memory (true async copies) */
fhe_status fhe_host_free(void *p);
fhe_status fhe_stream_create(int device, void **stream_out);
fhe_status fhe_stream_sync(void *stream);
fhe_status fhe_stream_destroy(void *stream);
fhe_status fhe_device_sync(int device);
fhe_status fhe_device_mem_info(int device, size_t *free_bytes, size_t *total_bytes);  /* either may be NULL */

/* ------------------------------------------------------------------ rq::Context ---- */
/* Context::new (M/rq/context.rs:42-92).  `device` >= 0 uploads tables to that GPU; -1 builds
 * a host-only handle (setup / introspection, no compute).  Tables (M/ntt/native.rs:16-26,
 * each `[nmoduli][degree]`, size_inv* `[nmoduli]`) are what the Rust host already holds in
 * its NttOperators; pass all NULL to let the engine derive its own primitive roots
 * (psi = g^((p-1)/2N) for the smallest g >= 2 that is a primitive 2N-th root).
 * The whole `next_context` chain (moduli prefixes) is built eagerly. */
fhe_status fhe_ctx_create(int device, size_t degree, size_t nmoduli, const uint64_t *moduli,
                          const uint64_t *omegas, const uint64_t *omegas_shoup,
                          const uint64_t *zetas_inv, const uint64_t *zetas_inv_shoup,
                          const uint64_t *size_inv, const uint64_t *size_inv_shoup, fhe_ctx **out);
void fhe_ctx_destroy(fhe_ctx *ctx);
/* Context::context_at_level (M/rq/context.rs:143-156): borrowed handle owned by `ctx`. */
fhe_status fhe_ctx_at_level(const fhe_ctx *ctx, size_t level, const fhe_ctx **out);
/* Context::niterations_to (M/rq/context.rs:117-141). */
fhe_status fhe_ctx_niterations_to(const fhe_ctx *from, const fhe_ctx *to, size_t *out);
size_t fhe_ctx_degree(const fhe_ctx *ctx);
size_t fhe_ctx_nmoduli(const fhe_ctx *ctx);
int fhe_ctx_device(const fhe_ctx *ctx);
fhe_status fhe_ctx_moduli(const fhe_ctx *ctx, uint64_t *out /* [nmoduli] */);
/* Introspection (tests / Rust host cross-check): which: 0 omegas, 1 omegas_shoup, 2 zetas_inv,
 * 3 zetas_inv_shoup (each [nmoduli][degree]); 4 size_inv, 5 size_inv_shoup (each [nmoduli]);
 * 6 inv_last_qi_mod_qj, 7 its Shoup twin (each [nmoduli-1], M/rq/context.rs:66-73). */
fhe_status fhe_ctx_get_table(const fhe_ctx *ctx, int which, uint64_t *out);

/* NttOperator::{forward,backward} via Poly::{ntt_forward,ntt_backward} (M/rq/mod.rs:335-354):
 * `polys` is [batch][L][N], transformed in place, canonical outputs.
 * The reference also has a lazy forward transform, NttOperator::forward_vt_lazy (M/ntt/native.rs:142-175, outputs in
 * [0, 2p)); its only caller on the path is the key switch's lift-and-transform (M/rq/mod.rs:563-586), which the
 * engine performs inside fhe_key_switch and its relatives.  No `lazy` flag is exported on purpose (SURVEY 8b's draft
 * signature had one): only canonical residues cross this ABI -- a value in [0, 2p) is not a function of the inputs
 * alone, and bit-exact parity is stated on canonical values. */
fhe_status fhe_ntt_forward(const fhe_ctx *ctx, uint64_t *polys, size_t batch);
fhe_status fhe_ntt_backward(const fhe_ctx *ctx, uint64_t *polys, size_t batch);
fhe_status fhe_ntt_forward_dev(const fhe_ctx *ctx, uint64_t *polys, size_t batch, void *stream);
fhe_status fhe_ntt_backward_dev(const fhe_ctx *ctx, uint64_t *polys, size_t batch, void *stream);

/* AddAssign / SubAssign / MulAssign<&Poly<Ntt>> / Neg (M/rq/ops.rs:10-206, 354-418): a op= b. */
fhe_status fhe_poly_add(const fhe_ctx *ctx, uint64_t *a, const uint64_t *b, size_t batch);
fhe_status fhe_poly_sub(const fhe_ctx *ctx, uint64_t *a, const uint64_t *b, size_t batch);
fhe_status fhe_poly_mul(const fhe_ctx *ctx, uint64_t *a, const uint64_t *b, size_t batch);
fhe_status fhe_poly_neg(const fhe_ctx *ctx, uint64_t *a, size_t batch);
/* MulAssign<&Poly<NttShoup>> (M/rq/ops.rs:208-245); Poly::compute_coefficients_shoup (M/rq/mod.rs:244-258). */
fhe_status fhe_poly_mul_shoup(const fhe_ctx *ctx, uint64_t *a, const uint64_t *b, const uint64_t *b_shoup,
                              size_t batch);
fhe_status fhe_poly_shoup(const fhe_ctx *ctx, const uint64_t *a, uint64_t *a_shoup, size_t batch);
fhe_status fhe_poly_add_dev(const fhe_ctx *ctx, uint64_t *a, const uint64_t *b, size_t batch, void *stream);
fhe_status fhe_poly_sub_dev(const fhe_ctx *ctx, uint64_t *a, const uint64_t *b, size_t batch, void *stream);
fhe_status fhe_poly_mul_dev(const fhe_ctx *ctx, uint64_t *a, const uint64_t *b, size_t batch, void *stream);
fhe_status fhe_poly_neg_dev(const fhe_ctx *ctx, uint64_t *a, size_t batch, void *stream);
fhe_status fhe_poly_mul_shoup_dev(const fhe_ctx *ctx, uint64_t *a, const uint64_t *b, const uint64_t *b_shoup,
                                  size_t batch, void *stream);

/* Poly::substitute (M/rq/mod.rs:360-412) with SubstitutionExponent::new (M/rq/mod.rs:99-121).
 * repr_is_ntt != 0: Ntt-domain permutation; 0: PowerBasis signed scatter.  in != out. */
fhe_status fhe_poly_substitute(const fhe_ctx *ctx, size_t exponent, const uint64_t *in, uint64_t *out,
                               size_t batch, int repr_is_ntt);
fhe_status fhe_poly_substitute_dev(const fhe_ctx *ctx, size_t exponent, const uint64_t *in, uint64_t *out,
                                   size_t batch, int repr_is_ntt, void *stream);

/* Poly::<PowerBasis>::switch_down (M/rq/mod.rs:433-492): in [batch][L][N] -> out [batch][L-1][N]. */
fhe_status fhe_poly_switch_down(const fhe_ctx *ctx, const uint64_t *in, uint64_t *out, size_t batch);
fhe_status fhe_poly_switch_down_dev(const fhe_ctx *ctx, const uint64_t *in, uint64_t *out, size_t batch,
                                    void *stream);

/* Poly::<PowerBasis>::switch_down_to (M/rq/mod.rs:498-507): niterations_to(to) applications of switch_down in one
 * call; in [batch][from.L][N] -> out [batch][to.L][N], PowerBasis.  `to` not on `from`'s chain ->
 * FHE_E_CONTEXT_NOT_REACHABLE; from == to copies. */
fhe_status fhe_poly_switch_down_to(const fhe_ctx *from, const fhe_ctx *to, const uint64_t *in, uint64_t *out,
                                   size_t batch);
fhe_status fhe_poly_switch_down_to_dev(const fhe_ctx *from, const fhe_ctx *to, const uint64_t *in, uint64_t *out,
                                       size_t batch, void *stream);

/* Rq wire format (`impl From<&Poly> for Rq` / parse_proto, M/rq/convert.rs:17-44, 46-99; Modulus::
 * serialize_vec / deserialize_vec, M/zq/mod.rs:783-793; fhe-util transcode_{to,from}_bytes,
 * crates/fhe-util/src/lib.rs:71-148): the `coefficients` bytes of the Rq message hold, per residue
 * row i, the N PowerBasis coefficients as bitlen(q_i - 1)-bit little-endian bit-packed integers, rows
 * concatenated (N % 8 == 0, so every row is byte aligned).  The protobuf envelope (representation tag,
 * degree) stays on the host; these calls move its payload.
 *   fhe_poly_serialized_size: bytes per polynomial = sum_i N * bitlen(q_i - 1) / 8.
 *   fhe_poly_serialize:   polys [batch][L][N] -> bytes [batch][size]; from_ntt != 0: the input is in Ntt
 *                         form and is taken to PowerBasis first (the wire is always PowerBasis).
 *   fhe_poly_deserialize: bytes [batch][size] -> polys [batch][L][N], coefficients taken verbatim
 *                         (TryConvertFrom<Vec<u64>>, convert.rs:148-160); to_ntt != 0: followed by
 *                         into_ntt (representation tag Ntt / NttShoup). */
size_t fhe_poly_serialized_size(const fhe_ctx *ctx);
fhe_status fhe_poly_serialize(const fhe_ctx *ctx, const uint64_t *polys, uint8_t *bytes, size_t batch, int from_ntt);
fhe_status fhe_poly_serialize_dev(const fhe_ctx *ctx, const uint64_t *polys, uint8_t *bytes, size_t batch,
                                  int from_ntt, void *stream);
fhe_status fhe_poly_deserialize(const fhe_ctx *ctx, const uint8_t *bytes, uint64_t *polys, size_t batch, int to_ntt);
fhe_status fhe_poly_deserialize_dev(const fhe_ctx *ctx, const uint8_t *bytes, uint64_t *polys, size_t batch,
                                    int to_ntt, void *stream);

/* ------------------------------------------------------------------ rq::Scaler ---- */
/* Scaler::new (M/rq/scaler.rs:27-52) + RnsScaler::new (M/rns/scaler.rs:79-175): the engine
 * derives gamma/omega/theta with its own big-integer code from the ScalingFactor
 * numerator/denominator, given as little-endian u64 limbs (ScalingFactor::new,
 * M/rns/scaler.rs:26-36; numerator == denominator <=> is_one). */
fhe_status fhe_scaler_create(const fhe_ctx *from, const fhe_ctx *to, const uint64_t *numerator,
                             size_t numerator_limbs, const uint64_t *denominator, size_t denominator_limbs,
                             fhe_scaler **out);
/* Same, but every RnsScaler field (M/rns/scaler.rs:52-72) is supplied by the Rust host. */
fhe_status fhe_scaler_create_from_constants(
    const fhe_ctx *from, const fhe_ctx *to, size_t number_common_moduli, int is_one,
    const uint64_t *gamma, const uint64_t *gamma_shoup,   /* [to]       */
    const uint64_t *omega, const uint64_t *omega_shoup,   /* [to][from] */
    uint64_t theta_gamma_lo, uint64_t theta_gamma_hi, int theta_gamma_sign,
    const uint64_t *theta_omega_lo, const uint64_t *theta_omega_hi, const uint8_t *theta_omega_sign, /* [from] */
    const uint64_t *theta_garner_lo, const uint64_t *theta_garner_hi, size_t theta_garner_shift,     /* [from] */
    fhe_scaler **out);
/* Switcher::new (M/rq/switcher.rs:17-22): factor to.modulus / from.modulus. */
fhe_status fhe_switcher_create(const fhe_ctx *from, const fhe_ctx *to, fhe_scaler **out);
void fhe_scaler_destroy(fhe_scaler *s);
size_t fhe_scaler_number_common_moduli(const fhe_scaler *s);
/* Introspection: which: 0 gamma, 1 gamma_shoup ([to]); 2 omega, 3 omega_shoup ([to][from]);
 * 4 theta_omega_lo, 5 theta_omega_hi, 6 theta_omega_sign, 7 theta_garner_lo, 8 theta_garner_hi ([from]);
 * 9 {theta_gamma_lo, theta_gamma_hi, theta_gamma_sign, theta_garner_shift, is_one} ([5]). */
fhe_status fhe_scaler_get_constants(const fhe_scaler *s, int which, uint64_t *out);
/* Scaler::scale (M/rq/scaler.rs:55-127) == Poly::scale / Poly::switch (M/rq/mod.rs:660-680):
 * in [batch][from.L][N] -> out [batch][to.L][N]; repr_is_ntt selects Ntt vs PowerBasis. */
fhe_status fhe_poly_scale(const fhe_scaler *s, const uint64_t *in, uint64_t *out, size_t batch, int repr_is_ntt);
fhe_status fhe_poly_scale_dev(const fhe_scaler *s, const uint64_t *in, uint64_t *out, size_t batch,
                              int repr_is_ntt, void *stream);

/* ------------------------------------------------------------ KeySwitchingKey ---- */
/* KeySwitchingKey{c0,c1: Box<[Poly<NttShoup>]>, ctx_ciphertext, ctx_ksk, log_base}
 * (F/bfv/keys/key_switching_key.rs:22-46).  c0/c1: [ndigits][Lk][N]; Shoup twins may be NULL
 * (then computed as floor(c * 2^64 / q), M/zq/mod.rs:195-199).  log_base != 0 selects the
 * single-modulus decomposition path (:323-362); otherwise ndigits must equal ct_ctx's L. */
fhe_status fhe_ksk_create(const fhe_ctx *ct_ctx, const fhe_ctx *ksk_ctx, size_t ndigits, const uint64_t *c0,
                          const uint64_t *c0_shoup, const uint64_t *c1, const uint64_t *c1_shoup,
                          size_t log_base, fhe_ksk **out);
/* Same with key polynomials already resident on the device: copied device-to-device on `stream`, checked and twinned
 * there by the pass every other route uses (no key word passes through host memory).  The words are untrusted input:
 * the call waits for `stream` to read the range check's flag word and once more before it returns, so the key is
 * usable from any stream afterwards.  fhe_ksk_create is the host form of this call: its arrays are uploaded and finished
 * the same way, and a supplied twin array is compared with the twins the device wrote. */
fhe_status fhe_ksk_create_dev(const fhe_ctx *ct_ctx, const fhe_ctx *ksk_ctx, size_t ndigits, const uint64_t *c0,
                              const uint64_t *c1, size_t log_base, void *stream, fhe_ksk **out);
void fhe_ksk_destroy(fhe_ksk *k);
/* Execution options of every key switch through this handle (key_switch, relinearise, Galois, RGSW, the relinearise
 * step of fhe_bfv_mul), kept on the handle like fhe_mul's: atomics read once per call; they only choose how the sum
 * of KeySwitchingKey::key_switch (F/bfv/keys/key_switching_key.rs:241-320) is evaluated, never its value.
 *   mode     FHE_KS_AUTO (default): the engine picks per shape and launch size; FHE_KS_FUSED: one kernel per
 *            (ciphertext, key modulus) that transforms the digits in LDS and multiplies them into register
 *            accumulators (Shoup twins) -- rows larger than LDS (N >= 32768) as 16384-point parts with the first one /
 *            two stages folded into the loader; FHE_KS_FUSED_SUB: the same on 8192-point sub-blocks for N >= 32768
 *            (twice the workgroups, each 1.7 x shorter: ahead only while a launch does not fill the device);
 *            FHE_KS_UNFUSED: the digit transforms of a launch as one batched NTT into scratch, then a streaming
 *            multiply-accumulate with lazy 128-bit sums (the pattern of F/bfv/ops/dot_product.rs:54-180) that reads
 *            the key without its twins; FHE_KS_UNFUSED_SUB: the same on 8192-point sub-block tiles at N = 16384 too.
 *            Decomposition keys (log_base != 0) always take the fused kernel.
 *   w_budget bytes of transformed digit rows one launch pair may have in flight (0 = default, 4 GiB).
 * What FHE_KS_AUTO does, from measurements on the MI355X (profiles/r04_ks_unfused_ab.txt, r04_ks_half15_ab.txt,
 * r04_final3_ks_modes_ab_c5.jsonl, r04_ks_small_launch_ab.txt, r04_ks_small_batches_all_modes.txt):
 *   - a launch that fills the device takes FHE_KS_FUSED at every size (N = 32768, 16 moduli, 16 polynomials: 1.08 vs
 *     1.23 ms unfused; N = 16384, 8 moduli, 512: 3.5 vs 4.3 ms; N = 8192, 4 moduli, 1024: 0.83 vs 0.97 ms);
 *   - a launch with few fused workgroups (2 x batch x key moduli [x N / 16384] <= compute units; RNS-digit keys with at
 *     least three digits, N >= 4096) takes FHE_KS_UNFUSED, whose first stage has digits x more tiles: one ciphertext at
 *     N = 16384, 8 moduli 0.220 -> 0.055 ms, at N = 32768, 16 moduli 0.32 -> 0.12 ms, at N = 8192, 4 moduli 0.054 -> 0.030;
 *   - other launches at N >= 32768 whose 8192-point sub-blocks fit the device at once (decomposition keys, fewer than
 *     three digits) take FHE_KS_FUSED_SUB. */
enum { FHE_KS_AUTO = 0, FHE_KS_FUSED = 1, FHE_KS_UNFUSED = 2, FHE_KS_UNFUSED_SUB = 3, FHE_KS_FUSED_SUB = 4 };
fhe_status fhe_ksk_set_mode(fhe_ksk *k, int mode, size_t w_budget);
fhe_status fhe_ksk_get_mode(const fhe_ksk *k, int *mode, size_t *w_budget);
/* KeySwitchingKey::key_switch / key_switch_assign (:241-320): p [batch][L][N] PowerBasis over
 * ct_ctx -> c0_out, c1_out [batch][Lk][N] Ntt over ksk_ctx. */
fhe_status fhe_key_switch(const fhe_ksk *k, const uint64_t *p, uint64_t *c0_out, uint64_t *c1_out, size_t batch);
fhe_status fhe_key_switch_dev(const fhe_ksk *k, const uint64_t *p, uint64_t *c0_out, uint64_t *c1_out,
                              size_t batch, void *stream);
/* RelinearizationKey::relinearizes (F/bfv/keys/relinearization_key.rs:69-102):
 * ct3 [batch][3][L][N] Ntt -> out [batch][2][L][N] Ntt (switch_down_to when the key level is higher). */
fhe_status fhe_bfv_relinearize(const fhe_ksk *rk, const uint64_t *ct3, uint64_t *out, size_t batch);
fhe_status fhe_bfv_relinearize_dev(const fhe_ksk *rk, const uint64_t *ct3, uint64_t *out, size_t batch,
                                   void *stream);
/* GaloisKey::relinearize / relinearize_into (F/bfv/keys/galois_key.rs:63-123), i.e.
 * EvaluationKey::rotates_columns_by (exponent 3^i mod 2N) / rotates_rows (exponent 2N-1)
 * (F/bfv/keys/evaluation_key.rs:110-170, 278-286): ct, out [batch][2][L][N] Ntt.
 * From N = 4096 on (key at the ciphertext's level) there is no separate permutation pass: the Ntt-domain substitution is
 * read as a gather inside the inverse transform and the key switch.  `out` may be `ct` itself (the reference's
 * `c1 = ek.rotates_rows(&c1)`): any overlap of `ct` and `out` takes the copying path (every read of `ct` precedes the first write of `out`). */
fhe_status fhe_bfv_galois(const fhe_ksk *gk, size_t exponent, const uint64_t *ct, uint64_t *out, size_t batch);
fhe_status fhe_bfv_galois_dev(const fhe_ksk *gk, size_t exponent, const uint64_t *ct, uint64_t *out,
                              size_t batch, void *stream);
/* Ciphertext::switch_down (F/bfv/ciphertext.rs:148-161): ct [batch][nparts][L][N] Ntt ->
 * out [batch][nparts][L-1][N] Ntt. */
fhe_status fhe_bfv_switch_down(const fhe_ctx *ctx, size_t nparts, const uint64_t *ct, uint64_t *out, size_t batch);
fhe_status fhe_bfv_switch_down_dev(const fhe_ctx *ctx, size_t nparts, const uint64_t *ct, uint64_t *out,
                                   size_t batch, void *stream);

/* Ciphertext::switch_to_level (F/bfv/ciphertext.rs:164-183) with levels = target_level - level >= 0:
 * ct [batch][nparts][L][N] Ntt -> out [batch][nparts][L-levels][N] Ntt.  The reference loops
 * switch_down (PowerBasis -> divide-and-round -> Ntt per level); here one inverse transform, `levels` divide-and-round
 * passes and one forward transform give the same values (the Ntt round trips in between are the identity).
 * levels beyond the chain -> FHE_E_INVALID_LEVEL; levels == 0 copies. */
fhe_status fhe_bfv_switch_to_level(const fhe_ctx *ctx, size_t levels, size_t nparts, const uint64_t *ct, uint64_t *out,
                                   size_t batch);
fhe_status fhe_bfv_switch_to_level_dev(const fhe_ctx *ctx, size_t levels, size_t nparts, const uint64_t *ct,
                                       uint64_t *out, size_t batch, void *stream);

/* ------------------------------------ PIR / RGSW / inner sum ("next" rows) ---- */
/* fhe_math::rq::dot_product (M/rq/ops.rs:449-570) and bfv::dot_product_scalar
 * (F/bfv/ops/dot_product.rs:54-180): out[b][part] = sum_k cts[b][k][part] (.) pts[b][k], all Ntt.
 * cts: [batch][count][nparts][L][N] (or [count][nparts][L][N] shared by the batch when cts_shared != 0);
 * pts: [batch][count][L][N] (`Plaintext::poly_ntt`; shared when pts_shared != 0); out: [batch][nparts][L][N].
 * nparts = 1 is the polynomial dot product.  count == 0 -> FHE_E_EMPTY_DOT_PRODUCT. */
fhe_status fhe_bfv_dot_product_scalar(const fhe_ctx *ctx, size_t nparts, size_t count, const uint64_t *cts,
                                      int cts_shared, const uint64_t *pts, int pts_shared, uint64_t *out,
                                      size_t batch);
fhe_status fhe_bfv_dot_product_scalar_dev(const fhe_ctx *ctx, size_t nparts, size_t count, const uint64_t *cts,
                                          int cts_shared, const uint64_t *pts, int pts_shared, uint64_t *out,
                                          size_t batch, void *stream);
/* `Ciphertext * Plaintext` (F/bfv/ops/mod.rs:229-257): out[b][part] = ct[b][part] (.) pt[b] (pt shared if pt_shared). */
fhe_status fhe_bfv_mul_plain(const fhe_ctx *ctx, size_t nparts, const uint64_t *ct, const uint64_t *pt, int pt_shared,
                             uint64_t *out, size_t batch);
fhe_status fhe_bfv_mul_plain_dev(const fhe_ctx *ctx, size_t nparts, const uint64_t *ct, const uint64_t *pt,
                                 int pt_shared, uint64_t *out, size_t batch, void *stream);
/* Poly::<Ntt>::random_from_seed (M/rq/mod.rs:276-292) as a received ciphertext applies it (F/bfv/ciphertext.rs:
 * 287-302): seeds [batch][32] bytes -> out [batch][L][N], the polynomial c1 of a seeded ciphertext, taken as Ntt form.
 * key = SHA-256(seed); one ChaCha8 stream per polynomial; every residue row draws `degree` values from
 * Uniform[0, q_i).  SHA-256 and the ChaCha block function are public algorithms (known-answer tested); the
 * generator's word layout and the rejection sampler restate rand_chacha 0.10 / rand 0.10, third-party crates the
 * reference does not vendor: PARITY UNPINNED against a real fhe.rs run, exactly like the NTT's psi -- a host that
 * needs certainty expands c1 itself and uploads it. */
fhe_status fhe_poly_from_seed(const fhe_ctx *ctx, const uint8_t *seeds, uint64_t *out, size_t batch);
fhe_status fhe_poly_from_seed_dev(const fhe_ctx *ctx, const uint8_t *seeds, uint64_t *out, size_t batch, void *stream);
/* SecretKey::try_decrypt, small-plaintext branch (F/bfv/keys/secret_key.rs:198-247): phase
 * c0 + c1 s + c2 s^2 + ... over the ciphertext context, PowerBasis, Scaler::scale with the level's
 * cipher-to-plaintext scaler (factor t / q, F/bfv/parameters.rs:636-643), then per coefficient
 * ((d_0 + t) mod q_0) mod t.  `cipher_plain_scaler`: from = the ciphertext context, to = the plaintext
 * context (a prefix of the moduli).  s_ntt [L][N]: the secret key polynomial over the ciphertext
 * context in Ntt form (the host builds it from its ternary coefficients, secret_key.rs:200-203).
 * ct [batch][nparts][L][N] Ntt -> out [batch][N], the plaintext polynomial's coefficients in [0, t).
 * Secret hygiene (the reference wraps s, the phase and the scaled plaintext in Zeroizing, secret_key.rs:198-226):
 * the engine's intermediates (phase, scaled plaintext) are cleared on the stream before their scratch blocks
 * are reused; the host-pointer variant also clears its staged copies of s_ntt and of the result.  The `_dev`
 * variant's s_ntt and out are caller-owned device buffers: clearing them is the caller's job. */
fhe_status fhe_bfv_decrypt(const fhe_scaler *cipher_plain_scaler, uint64_t plaintext_modulus, const uint64_t *s_ntt,
                           const uint64_t *ct, size_t nparts, uint64_t *out, size_t batch);
fhe_status fhe_bfv_decrypt_dev(const fhe_scaler *cipher_plain_scaler, uint64_t plaintext_modulus,
                               const uint64_t *s_ntt, const uint64_t *ct, size_t nparts, uint64_t *out, size_t batch,
                               void *stream);
/* `&Ciphertext * &RGSWCiphertext` (F/bfv/rgsw_ciphertext.rs:122-156), RGSWCiphertext{ksk0, ksk1}:
 * ct, out [batch][2][L][N] Ntt; both keys at the ciphertext level. */
fhe_status fhe_bfv_rgsw_mul(const fhe_ksk *ksk0, const fhe_ksk *ksk1, const uint64_t *ct, uint64_t *out, size_t batch);
fhe_status fhe_bfv_rgsw_mul_dev(const fhe_ksk *ksk0, const fhe_ksk *ksk1, const uint64_t *ct, uint64_t *out,
                                size_t batch, void *stream);
/* EvaluationKey::computes_inner_sum (F/bfv/keys/evaluation_key.rs:56-100): out = ct; for every
 * (gks[i], exponents[i]) in order: out += GaloisKey::relinearize(out).  The caller passes the keys for
 * 3^(2^j) mod 2N, j = 0 .. log2(N/2)-1, then 2N-1 (exactly the reference's sequence). */
fhe_status fhe_bfv_inner_sum(const fhe_ksk *const *gks, const size_t *exponents, size_t ngk, const uint64_t *ct,
                             uint64_t *out, size_t batch);
fhe_status fhe_bfv_inner_sum_dev(const fhe_ksk *const *gks, const size_t *exponents, size_t ngk, const uint64_t *ct,
                                 uint64_t *out, size_t batch, void *stream);
/* EvaluationKey::expands (F/bfv/keys/evaluation_key.rs:192-256), the oblivious expansion of
 * eprint 2019/1483: gks[l] is the Galois key of element (N >> l) + 1, l < nlevels; expanding to
 * `size` outputs needs ceil(log2(size)) of them (fewer -> FHE_E_EXPANSION_UNSUPPORTED; size == 0 or
 * size > N -> FHE_E_INVALID_EXPANSION_SIZE).  The monomials -x^(N - 2^l) of the reference's
 * EvaluationKey are derived by the engine from the context's NTT tables.
 * ct [batch][2][L][N] Ntt -> out [size][batch][2][L][N] Ntt (batch = 1: the reference's Vec<Ciphertext>). */
fhe_status fhe_bfv_expand(const fhe_ksk *const *gks, size_t nlevels, const uint64_t *ct, uint64_t *out, size_t size,
                          size_t batch);
fhe_status fhe_bfv_expand_dev(const fhe_ksk *const *gks, size_t nlevels, const uint64_t *ct, uint64_t *out, size_t size,
                              size_t batch, void *stream);

/* ------------------------------------------------- keyed batches: one key per client ---- */
/* A server holds one ciphertext, or a few, from each of many clients, and every client has its own relinearization and
 * Galois keys.  The calls above take one key for the whole batch; the calls below take a SET of keys and a batch in which
 * items [c * m, (c + 1) * m), m = batch / nkeys, belong to key c -- the same values as one single-key call per client
 * (KeySwitchingKey::key_switch, F/bfv/keys/key_switching_key.rs:241-320, client by client), in the launches of one batch.
 * They rest on the unfused key switch: its digit transforms read no key, so one launch serves every client, and the
 * multiply-accumulate takes each polynomial's key words from a table on the device (ks_mac_keyed_kernel).
 * Device-pointer forms only.  For every keyed call: `batch` must be a multiple of the set's size (else FHE_E_ARG);
 * batch == 0 is a no-op (NULL buffers allowed); a NULL buffer with batch > 0 -> FHE_E_ARG; the layouts are those of
 * the single-key calls.
 * fhe_kskset_create: `keys` [nkeys] are BORROWED -- they outlive the set -- and must be RNS-digit keys (log_base == 0)
 * of one parameter set, one (ciphertext level, key level) pair and one digit count.  The set's device table is built
 * here (one upload, one wait).  An empty list or a NULL key -> FHE_E_ARG; a decomposition key -> FHE_E_ARG ("keyed
 * batches take RNS-digit keys"); keys that differ in contexts, levels or digits -> FHE_E_PARAMETER_MISMATCH; a
 * host-only context -> FHE_E_NO_DEVICE.  The keys' own modes (fhe_ksk_set_mode) do not apply to keyed calls.
 * fhe_kskset_set_w_budget: bytes of transformed digit rows one launch pair may have in flight (0 = default), as
 * fhe_ksk_set_mode's; launches cut by it need not end on a client boundary.
 * Not offered: an automatic choice between a keyed call and a loop of single-key calls (with many ciphertexts per client
 * the fused kernels of the single-key calls fill the device; tools/bench_keyed.py measures both), per-item exponents,
 * one RGSW ciphertext per item, and a Multiplicator with a key set.  To multiply and relinearize with one key per
 * client, in the order of Multiplicator::multiply (F/bfv/ops/mul.rs:165-243): fhe_bfv_mul_dev on a fhe_mul created
 * WITHOUT a relinearization key and without mod_switch (three parts out), then fhe_bfv_relinearize_keyed_dev, then
 * fhe_bfv_switch_down_dev (nparts = 2) where the modulus switch is wanted. */
fhe_status fhe_kskset_create(const fhe_ksk *const *keys, size_t nkeys, fhe_kskset **out);
void fhe_kskset_destroy(fhe_kskset *s);
size_t fhe_kskset_size(const fhe_kskset *s);
fhe_status fhe_kskset_set_w_budget(fhe_kskset *s, size_t bytes);
fhe_status fhe_kskset_get_w_budget(const fhe_kskset *s, size_t *bytes);
/* Rotation groups of one launch of fhe_bfv_matvec_hoisted_dev (below): 0 = the engine's rule, k = k groups, clamped to
 * the rotations of the launch.  It changes how the work is cut, never a word of the result. */
fhe_status fhe_kskset_set_rot_split(fhe_kskset *s, size_t groups);
fhe_status fhe_kskset_get_rot_split(const fhe_kskset *s, size_t *groups);
/* Giant groups served by one block of the baby stage of fhe_bfv_matvec_bsgs_dev (below), read from the BABY set: 0 = the
 * engine's rule on the shape and the device's compute units, 1, 2 or 4 = that kernel instance; anything else ->
 * FHE_E_ARG.  It changes how the work is cut, never a word of the result. */
fhe_status fhe_kskset_set_bsgs_tile(fhe_kskset *s, size_t gt);
fhe_status fhe_kskset_get_bsgs_tile(const fhe_kskset *s, size_t *gt);
/* KeySwitchingKey::key_switch (:241-320) per client: p [batch][L][N] PowerBasis -> c0_out, c1_out [batch][Lk][N] Ntt. */
fhe_status fhe_key_switch_keyed_dev(const fhe_kskset *s, const uint64_t *p, uint64_t *c0_out, uint64_t *c1_out,
                                    size_t batch, void *stream);
/* RelinearizationKey::relinearizes (F/bfv/keys/relinearization_key.rs:69-102) per client:
 * ct3 [batch][3][L][N] Ntt -> out [batch][2][L][N] Ntt. */
fhe_status fhe_bfv_relinearize_keyed_dev(const fhe_kskset *rks, const uint64_t *ct3, uint64_t *out, size_t batch,
                                         void *stream);
/* GaloisKey::relinearize (F/bfv/keys/galois_key.rs:63-123) per client, one exponent for the batch: the set holds every
 * client's key of that exponent.  ct, out [batch][2][L][N] Ntt; `out` may be `ct` (the copying path, as fhe_bfv_galois_dev). */
fhe_status fhe_bfv_galois_keyed_dev(const fhe_kskset *gks, size_t exponent, const uint64_t *ct, uint64_t *out,
                                    size_t batch, void *stream);
/* EvaluationKey::computes_inner_sum (F/bfv/keys/evaluation_key.rs:56-100) per client: one set per rotation, in the
 * order of fhe_bfv_inner_sum_dev.  Sets of different sizes -> FHE_E_PARAMETER_MISMATCH. */
fhe_status fhe_bfv_inner_sum_keyed_dev(const fhe_kskset *const *gks, const size_t *exponents, size_t ngk,
                                       const uint64_t *ct, uint64_t *out, size_t batch, void *stream);
/* EvaluationKey::expands (F/bfv/keys/evaluation_key.rs:192-256) per client: gks[l] holds every client's key of element
 * (N >> l) + 1.  ct [batch][2][L][N] -> out [size][batch][2][L][N].  Sets of different sizes -> FHE_E_PARAMETER_MISMATCH. */
fhe_status fhe_bfv_expand_keyed_dev(const fhe_kskset *const *gks, size_t nlevels, const uint64_t *ct, uint64_t *out,
                                    size_t size, size_t batch, void *stream);
/* Many Galois elements of each ciphertext from ONE digit decomposition (hoisting, Halevi-Shoup CRYPTO 2018 section 4; not
 * in the reference).  A loop of fhe_bfv_galois_dev pays the digit transforms once per rotation; here R rotations cost
 * one set of transforms and R multiply-accumulates (hoist_mac_kernel).
 * THE OUTPUT IS NOT THE REFERENCE'S WORDS.  GaloisKey::relinearize lifts the digits of substitute(c1); this call
 * substitutes the lifted digits of c1: with p = PowerBasis(c1), W[i][j] = NTT_j(p_i mod q_j) for i != j, W[i][i] = c1 row i,
 * and sigma_r the Ntt branch of Poly::substitute (M/rq/mod.rs:368-388) for exponents[r],
 *   out_r.c0[j] = sigma_r(c0[j]) + sum_i sigma_r(W[i][j]) * gk_r.c0[i][j],  out_r.c1[j] = sum_i sigma_r(W[i][j]) * gk_r.c1[i][j]
 * (mod q_j, canonical; tests/hoist_ref.py).  Both digit sets are = sigma(c1) mod q_i with magnitude below q_i, so the result
 * decrypts to what fhe_bfv_galois_dev's does under the same noise bound, but its words differ from that call's at every
 * exponent except 1.
 * gks: a set of nrot RNS-digit Galois keys at the ciphertext's level, key r for exponents[r] (host array, mod 2N); a
 * repeated exponent is allowed.  ct [batch][2][L][N] Ntt -> out [batch][nrot][2][L][N] Ntt (the layout
 * fhe_bfv_dot_product_scalar_dev reads as `count = nrot` ciphertexts per item).  The exponents travel as kernel arguments
 * (64 per launch): the call only enqueues.  Device-pointer form only.
 * NULL set or exponents, nrot != fhe_kskset_size, keys above the ciphertext's level, `out` overlapping `ct`, a NULL buffer
 * with batch > 0 -> FHE_E_ARG; an even exponent -> FHE_E_INVALID_SUBSTITUTION_EXPONENT; batch == 0 is a no-op.
 * No automatic choice between this call and a loop of single rotations is made: one rotation is faster through
 * fhe_bfv_galois_dev, two or more through this call (tools/bench_hoisted.py measures both; STATE.md). */
fhe_status fhe_bfv_galois_hoisted_dev(const fhe_kskset *gks, const size_t *exponents, size_t nrot, const uint64_t *ct,
                                      uint64_t *out, size_t batch, void *stream);
/* Hoisted matrix-vector product: the diagonal form of a plaintext matrix times an encrypted vector in ONE call whose only
 * output is the result ciphertext (hoist_matvec_kernel; not in the reference).  With W and sigma_r as above,
 *   out.c0[j] = pt0[j] c0[j] + sum_r pts_r[j] (sigma_r(c0[j]) + sum_i sigma_r(W[i][j]) gk_r.c0[i][j])
 *   out.c1[j] = pt0[j] c1[j] + sum_r pts_r[j]                   sum_i sigma_r(W[i][j]) gk_r.c1[i][j]
 * (mod q_j, canonical; tests/hoistmv_ref.py).  This equals, word for word, fhe_bfv_galois_hoisted_dev followed by
 * fhe_bfv_dot_product_scalar_dev(ctx, 2, nrot or nrot + 1, ...) with the unrotated ciphertext and pt0 first when pt0 is
 * given -- that composition is the specification -- without writing and re-reading the [batch][nrot] rotated ciphertexts.
 * LIKE THAT CALL'S, THE OUTPUT IS NOT THE REFERENCE'S WORDS: the rotations inside it substitute the lifted digits of c1
 * where GaloisKey::relinearize lifts the digits of substitute(c1), so the result decrypts to what a loop of
 * fhe_bfv_galois_dev and a dot product gives, under the same noise bound, but differs from it word for word unless
 * every exponent is 1.
 * gks, exponents, nrot: as fhe_bfv_galois_hoisted_dev (a repeated exponent is allowed).  ct [batch][2][L][N] Ntt.  pts:
 * Plaintext::poly_ntt rows over the ciphertext's context, [nrot][L][N] shared by the batch when pts_shared != 0, else
 * [batch][nrot][L][N].  pt0: the identity diagonal (the term of the unrotated ciphertext: no Galois key of exponent 1 is
 * needed, and no key switch adds its noise), [L][N] or [batch][L][N] by the same flag, NULL for none.
 * out [batch][2][L][N] Ntt.  16-byte aligned buffers.  Device-pointer form only; the call only enqueues.
 * A launch covers 64 rotations; its rotations may be cut into groups whose blocks run side by side
 * (fhe_kskset_set_rot_split: 0 = a rule on the shape and the device's compute units, k = k groups, clamped to the
 * rotations of a launch).  A call that is one group writes `out` directly; otherwise the groups write partial sums into
 * wiped workspace and one more launch adds them.  The result does not depend on the split.
 * NULL set, exponents, or ct / pts / out with batch > 0, nrot != fhe_kskset_size, keys above the ciphertext's level, `out`
 * overlapping ct, pts or pt0 -> FHE_E_ARG; an even exponent -> FHE_E_INVALID_SUBSTITUTION_EXPONENT; batch == 0 is a no-op
 * (NULL buffers allowed).  A refused call leaves `out` untouched.
 * No automatic choice between this call and the composition is made (tools/bench_hoisted_matvec.py measures both). */
fhe_status fhe_bfv_matvec_hoisted_dev(const fhe_kskset *gks, const size_t *exponents, size_t nrot, const uint64_t *ct,
                                      const uint64_t *pts, int pts_shared, const uint64_t *pt0, uint64_t *out, size_t batch,
                                      void *stream);
/* Baby-step/giant-step hoisted matrix-vector product (Halevi-Shoup, CRYPTO 2018, section 4.3; bsgs_baby_kernel and
 * bsgs_giant_kernel; not in the reference): with G = ngiant + 1 groups of B = nbaby + 1 diagonals,
 *   out = sum_g rot_giant_g( sum_b pts[g][b] * rot_baby_b(ct) ),
 * from nbaby + ngiant Galois keys and digit loops where the flat call above needs G * B - 1.  A caller who wants
 * sum_r d_r * rot_r(ct) with r = g B + b owes the pre-rotation pts[g][b] = rot_{-gB}(d_{gB+b}) of the plaintext diagonals.
 * The specification is a composition of the two calls above:
 *   inner_g = fhe_bfv_matvec_hoisted_dev(baby, baby_exps, nbaby, ct, pts[g][1..B), pts_shared, pt0 = pts[g][0])   g = 0 .. ngiant
 *   out     = inner_0 + sum_{g=1..ngiant} fhe_bfv_galois_hoisted_dev({giant key g-1}, {giant_exps[g-1]}, 1, inner_g)
 * with canonical sums mod q_j (tests/bsgs_ref.py); the call equals it word for word, whatever tile, split or W budget it
 * runs under.  LIKE THOSE CALLS', THE OUTPUT IS NOT THE REFERENCE'S WORDS: the rotations inside it substitute the lifted
 * digits of c1 where GaloisKey::relinearize lifts the digits of substitute(c1), so the result decrypts to what the flat
 * product on the un-pre-rotated diagonals decrypts to, but differs from a loop of fhe_bfv_galois_dev word for word.
 * baby, giant: two key sets of ONE client, key r of a set for exponent r of its list (odd, reduced mod 2N; a repeated
 * exponent is allowed).  ct, out [batch][2][L][N] Ntt.  pts: Plaintext::poly_ntt rows over the ciphertext's context,
 * [G][B][L][N] shared by the batch when pts_shared != 0, else [batch][G][B][L][N]; column b = 0 of every group is that
 * group's identity diagonal (no baby key, no key switch), row g = 0 the group that takes no giant rotation.  16-byte
 * aligned buffers.  Device-pointer form only; the call only enqueues.
 * LIMIT: a key table holds 64 rotations, so nbaby, ngiant <= 64 -- 65 x 65 diagonals per call; a caller with more splits
 * the giants over calls and adds the results.
 * The baby stage computes all G inner sums from one digit loop per baby rotation, a block serving a tile of 1, 2 or 4
 * groups (fhe_kskset_set_bsgs_tile on `baby`); the giant stage key-switches the G - 1 inner sums under their own keys
 * and sums them in registers, the giants cut into groups by the rule of fhe_kskset_set_rot_split (read from `giant`).
 * NULL set or exponent list, nbaby != fhe_kskset_size(baby), ngiant != fhe_kskset_size(giant), nbaby or ngiant above 64,
 * NULL ct / pts / out with batch > 0, `out` overlapping ct or pts, a buffer not 16-byte aligned, either set's keys
 * above the ciphertext's level -> FHE_E_ARG; an even exponent in either list -> FHE_E_INVALID_SUBSTITUTION_EXPONENT;
 * the two sets differing in ring, levels, device or digit count -> FHE_E_PARAMETER_MISMATCH; batch == 0 is a no-op (NULL
 * buffers allowed).  A refused call leaves `out` untouched.
 * No automatic choice of B and G, or between this call and the flat one, is made (tools/bench_bsgs_matvec.py measures). */
fhe_status fhe_bfv_matvec_bsgs_dev(const fhe_kskset *baby, const size_t *baby_exps, size_t nbaby, const fhe_kskset *giant,
                                   const size_t *giant_exps, size_t ngiant, const uint64_t *ct, const uint64_t *pts,
                                   int pts_shared, uint64_t *out, size_t batch, void *stream);
/* Hoisted rotations and the hoisted matrix-vector product with ONE GALOIS KEY SET PER CLIENT (keyed batches x hoisting;
 * hoist_mac_keyed_kernel and hoist_matvec_keyed_kernel): a server that multiplies its plaintext matrix by each client's
 * encrypted vector, every client under their own keys, in the launches of one batch.
 * gks: a set of nclients * nrot RNS-digit Galois keys at the ciphertext's level in CLIENT-MAJOR order: entry c * nrot + r is
 * client c's key for exponents[r].  `batch` is a multiple of nclients; with m = batch / nclients, items [c * m, (c + 1) * m)
 * belong to client c (the rule of the keyed calls above).
 * THE SPECIFICATION IS A COMPOSITION: the result equals, word for word, one call of fhe_bfv_galois_hoisted_dev /
 * fhe_bfv_matvec_hoisted_dev per client, on a set of that client's nrot keys and the client's slice of ct -- and, for the
 * matvec, of pts (when not shared) and pt0.  LIKE THOSE CALLS', THE OUTPUT IS NOT THE REFERENCE'S WORDS (tests/hoist_ref.py,
 * tests/hoistmv_ref.py restate it).  The words do not depend on the W budget, the rotation split or the chunking: a
 * launch cut by fhe_kskset_set_w_budget need not end on a client boundary.
 * Layouts, alignment, overlap rules and the pts_shared / pt0 conventions are those of the unkeyed calls: ct
 * [batch][2][L][N] Ntt; pts [nrot][L][N] shared by the WHOLE batch (every client's), or [batch][nrot][L][N]; pt0 NULL,
 * [L][N] or [batch][L][N] by the same flag; out [batch][nrot][2][L][N] for the rotations, [batch][2][L][N] for the matvec.
 * fhe_kskset_set_w_budget and fhe_kskset_set_rot_split apply as they do to the unkeyed calls.  One stage-A launch per
 * chunk and key-modulus group and one stage-B launch per 64 rotations of it, however many clients there are.
 * Device-pointer forms only; the calls only enqueue: nothing is uploaded.
 * Refused: everything the unkeyed calls refuse, with their texts; nclients == 0, nclients * nrot != fhe_kskset_size(gks),
 * batch % nclients != 0 -> FHE_E_ARG, each with a text that names both numbers.  batch == 0 is a no-op (NULL buffers
 * allowed).  A refused call leaves `out` untouched.
 * Not offered: keyed x BSGS (fhe_bfv_matvec_bsgs_dev takes the two key sets of one client); per-client diagonals as a
 * third `pts` form (one set of diagonals per client: pass them per item); any automatic choice between the keyed call
 * and a loop of single-client calls (tools/bench_hoisted_keyed.py measures both; STATE.md). */
fhe_status fhe_bfv_galois_hoisted_keyed_dev(const fhe_kskset *gks, size_t nclients, const size_t *exponents, size_t nrot,
                                            const uint64_t *ct, uint64_t *out, size_t batch, void *stream);
fhe_status fhe_bfv_matvec_hoisted_keyed_dev(const fhe_kskset *gks, size_t nclients, const size_t *exponents, size_t nrot,
                                            const uint64_t *ct, const uint64_t *pts, int pts_shared, const uint64_t *pt0,
                                            uint64_t *out, size_t batch, void *stream);

/* ------------------------------------------------------------- Multiplicator ---- */
/* Multiplicator::new_leveled_internal + enable_relinearization + enable_mod_switching
 * (F/bfv/ops/mul.rs:74-163).  rk may be NULL (3-part output). */
fhe_status fhe_mul_create(const fhe_scaler *extender_lhs, const fhe_scaler *extender_rhs,
                          const fhe_scaler *down_scaler, const fhe_ksk *rk_or_null, int mod_switch,
                          fhe_mul **out);
void fhe_mul_destroy(fhe_mul *m);
/* Output geometry: parts (2 with rk, else 3) and rows per part (L, or L-1 with mod switch). */
fhe_status fhe_mul_out_shape(const fhe_mul *m, size_t *parts, size_t *rows);
/* The multiplication basis (Multiplicator::mul_ctx moduli, mul.rs:84): *count = its length; moduli may be NULL. */
fhe_status fhe_mul_basis(const fhe_mul *m, size_t *count, uint64_t *moduli);
/* Execution options of fhe_bfv_mul(_dev), kept on the handle (there are no process-wide knobs): atomics, read
 * once on entry of every call, so they may be set while other threads use the handle -- calls already running
 * keep the values they started with.  (The reference's Multiplicator has no such state; these only choose how
 * the same values are computed.)
 *   chunk   ciphertext pairs per pipeline pass; 0 (default) = equal chunks under a workspace budget
 *           (3 GiB with one stream: 512 pairs at N = 8192, 4 moduli; 384 MiB but at least 8 pairs with two: 64
 *           pairs -- used when the batch gives four or more such chunks, else the one-stream cut)
 *   streams 2 (default) = the chunks of a batch alternate between the caller's stream and an internal one,
 *           forked from and joined back into the caller's stream with events: stream-ordered for the caller
 *           exactly as with 1, capturable into a hipGraph, bit-identical results, +4.5 % at C2;
 *           1 = the caller's stream only (per-kernel durations do not overlap: what profilers want). */
fhe_status fhe_mul_set_chunk(fhe_mul *m, size_t chunk);
fhe_status fhe_mul_set_streams(fhe_mul *m, size_t streams);
fhe_status fhe_mul_get_options(const fhe_mul *m, size_t *chunk, size_t *streams);
/* Multiplicator::multiply (F/bfv/ops/mul.rs:165-243), the metric's unit of work:
 * lhs, rhs [batch][2][L][N] Ntt -> out [batch][parts][rows][N] Ntt.  lhs == rhs (the same buffer: squaring, the
 * reference's `&c1 * &c1`) extends the operand once; the values are those of the general call.
 * The host-pointer form sends a large batch (>= 3 slices of >= 32 MiB per operand) through in slices whose upload,
 * pipeline and download overlap on internal streams (so do fhe_bfv_relinearize and fhe_bfv_galois); it returns when
 * `out` is complete, like every host-pointer call. */
fhe_status fhe_bfv_mul(const fhe_mul *m, const uint64_t *lhs, const uint64_t *rhs, uint64_t *out, size_t batch);
fhe_status fhe_bfv_mul_dev(const fhe_mul *m, const uint64_t *lhs, const uint64_t *rhs, uint64_t *out,
                           size_t batch, void *stream);
/* `Mul<&Ciphertext> for &Ciphertext` with any number of parts (F/bfv/ops/mod.rs:259-358; the squaring branch
 * computes the same values): extend every part, c[k] = sum_{i+j=k} lhs[i] (.) rhs[j] over the multiplication
 * basis, scale every c[k] down; never relinearises (the handle's key and mod-switch flag are ignored).
 * lhs [batch][lhs_parts][L][N], rhs [batch][rhs_parts][L][N] Ntt -> out [batch][lhs_parts+rhs_parts-1][L][N] Ntt.
 * (fhe_bfv_mul is the 2 x 2 case on its fused pipeline and is what Multiplicator::multiply accepts.) */
fhe_status fhe_bfv_tensor(const fhe_mul *m, size_t lhs_parts, size_t rhs_parts, const uint64_t *lhs, const uint64_t *rhs,
                          uint64_t *out, size_t batch);
fhe_status fhe_bfv_tensor_dev(const fhe_mul *m, size_t lhs_parts, size_t rhs_parts, const uint64_t *lhs,
                              const uint64_t *rhs, uint64_t *out, size_t batch, void *stream);

/* ------------------------------------------------------------- BfvParameters ---- */
/* BfvParametersBuilder::build (F/bfv/parameters.rs:560-738), the part that defines device
 * tables: per-level contexts, the extended multiplication basis (:660-676) and per-level
 * MultiplicationParameters{extender, down_scaler} (:686-700, 793-814).
 * moduli may be generated first with fhe_generate_moduli. */
fhe_status fhe_params_create(int device, size_t degree, size_t nmoduli, const uint64_t *moduli,
                             uint64_t plaintext_modulus, fhe_params **out);
/* NTT tables of the host.  fhe_params_create derives its own primitive root psi per modulus (the smallest
 * generator), so its handles agree only with Ntt-form data produced through THIS engine.  The reference draws
 * psi from ChaCha8Rng::seed_from_u64(0) (M/ntt/native.rs:320-336; third-party RNG, not reproducible here), and
 * every Ntt-form ciphertext or key made by the Rust host is in that evaluation order: a host that brings its own
 * Ntt-form data MUST create the parameter set with fhe_params_create_with_tables.  The engine calls `tables`
 * once for every modulus it builds a context over -- the ciphertext moduli and the 62-bit extension primes of
 * parameters.rs:660-676 -- and the host fills the four [degree] tables and the two scalars of
 * NttOperator::new(modulus, degree) (M/ntt/native.rs:16-26, same meaning as in fhe_ctx_create).  A non-zero
 * return aborts creation with FHE_E_NTT_UNAVAILABLE.  The callback is invoked only while this call runs (the
 * tables are cached per modulus for handles made later, e.g. fhe_mul_create_default's level-specific basis).
 * tables == NULL behaves like fhe_params_create. */
typedef int (*fhe_ntt_tables_fn)(void *user, uint64_t modulus, size_t degree, uint64_t *omegas,
                                 uint64_t *omegas_shoup, uint64_t *zetas_inv, uint64_t *zetas_inv_shoup,
                                 uint64_t *size_inv, uint64_t *size_inv_shoup);
fhe_status fhe_params_create_with_tables(int device, size_t degree, size_t nmoduli, const uint64_t *moduli,
                                         uint64_t plaintext_modulus, fhe_ntt_tables_fn tables, void *user,
                                         fhe_params **out);
void fhe_params_destroy(fhe_params *p);
size_t fhe_params_max_level(const fhe_params *p);
fhe_status fhe_params_ctx(const fhe_params *p, size_t level, const fhe_ctx **out);      /* context_at_level */
fhe_status fhe_params_mul_ctx(const fhe_params *p, size_t level, const fhe_ctx **out);  /* mul_params.to    */
fhe_status fhe_params_extender(const fhe_params *p, size_t level, const fhe_scaler **out);
fhe_status fhe_params_down_scaler(const fhe_params *p, size_t level, const fhe_scaler **out);
/* Multiplicator::default(rk) (F/bfv/ops/mul.rs:101-138) at rk's ciphertext level: the extension primes are
 * the first 62-bit NTT primes that are not moduli OF THAT LEVEL (mul.rs:110-126) -- at level > 0 this can differ
 * from the level's mul_params basis, which skips every top-level modulus (parameters.rs:660-676); the handle then
 * owns its own multiplication context and scalers.  rk == NULL gives the `&ct * &ct` strategy without
 * relinearisation (F/bfv/ops/mod.rs:259-358), which uses the level's mul_params as the reference does. */
fhe_status fhe_mul_create_default(const fhe_params *p, size_t level, const fhe_ksk *rk_or_null, int mod_switch,
                                  fhe_mul **out);

/* ------------------------------------------------------- plaintext encoding ---- */
/* Encoding and decoding of BFV plaintexts and ct +- pt.  Device-pointer forms only, with no host-pointer twin (like
 * fhe_synth_uniform_dev): a host without PyTorch stages through fhe_buf_*.
 * Every value and coefficient is reduced mod t on load.  For inputs in [0, t) -- what the reference accepts -- the
 * results are the reference's, bit for bit.  The reference itself does not reduce: for inputs >= t its SIMD transform
 * gets out-of-range words and Poly encoding keeps v mod q_i, so there the two differ. */
enum { FHE_ENCODING_POLY = 0, FHE_ENCODING_SIMD = 1 };
/* The encoding tables of a parameter set (BfvParametersBuilder::build, F/bfv/parameters.rs:598, 607-633, 711-725):
 * t's NttOperator::new(t, N) when t admits a degree-N NTT (parameters.rs:71-75; otherwise SIMD calls return
 * FHE_E_SIMD_UNAVAILABLE and Poly encoding still works), SEAL's index map (generator 3, m = 2N), and per level
 * q_mod_t and delta_i = (-t)^-1 mod q_i.  `tables` (same typedef as fhe_params_create_with_tables) is called once, for
 * t, when t admits the NTT, and only while this call runs; a non-zero return -> FHE_E_NTT_UNAVAILABLE.  NULL -> the
 * engine's own psi (as fhe_params_create).  A host-only parameter set -> FHE_E_NO_DEVICE.  `par` must outlive the
 * encoder. */
fhe_status fhe_encoder_create(const fhe_params *par, fhe_ntt_tables_fn tables, void *user, fhe_encoder **out);
void fhe_encoder_destroy(fhe_encoder *enc);
/* PlaintextVec::try_encode (F/bfv/plaintext_vec.rs:70-102) with Encoding::{poly,simd}_at_level: values
 * [batch][nvalues] (nvalues <= N, zero-padded; more -> FHE_E_TOO_MANY_VALUES) -> out [batch][L_level][N] Ntt, the
 * plaintexts' `poly_ntt` (scaled = 0) or their Delta-scaled Plaintext::to_poly (F/bfv/plaintext.rs:172-196;
 * scaled = 1), the operand of fhe_bfv_add_plain_dev.  Poly: coefficients = values; SIMD: coefficients[map[i]] =
 * values[i], then NttOperator::backward mod t.  level > max -> FHE_E_INVALID_LEVEL.  The engine's scratch rows of
 * coefficients mod t are cleared before they are reused (the reference zeroizes them, plaintext.rs:104, 178). */
fhe_status fhe_bfv_encode_dev(const fhe_encoder *enc, int encoding, int scaled, size_t level, const uint64_t *values,
                              size_t nvalues, uint64_t *out, size_t batch, void *stream);
/* Vec<u64>::try_decode (F/bfv/plaintext.rs:157-170, 408-431): coefficients mod t [batch][N] (what fhe_bfv_decrypt_dev
 * writes) -> values [batch][N].  Poly: the coefficients; SIMD: NttOperator::forward mod t, then out[i] = v[map[i]]. */
fhe_status fhe_bfv_decode_dev(const fhe_encoder *enc, int encoding, const uint64_t *coeffs, uint64_t *out, size_t batch,
                              void *stream);
/* Plaintexts from packed bits: fhe_util::transcode_from_bytes / transcode_to_bytes / transcode_bidirectional
 * (crates/fhe-util/src/lib.rs:71-190) followed by Plaintext::try_encode(Encoding::poly_at_level), without an unpacked
 * copy of the values in device memory.  The three transcoders are one operation on a bit stream: the low in_bits of each
 * input element laid end to end, least significant bit first (a byte string is in_bits = 8); output element k is stream
 * bits [k out_bits, (k + 1) out_bits), bits past the end read as zero; ceil(nin in_bits / out_bits) output elements, the
 * last one possibly partial.  As everywhere in this section the values are reduced mod t on load: with
 * nbits = ilog2(t), what the examples use, every value is below t and the result is the reference's bit for bit.
 *
 * fhe_bfv_encode_bytes_dev: encode_database (crates/fhe/examples/util.rs:97-145; both PIR servers): item b is bytes
 * [b item_bytes, min((b + 1) item_bytes, nbytes)) of `bytes`, and everything from nbytes on reads as zero -- a short last
 * item and the all-zero padding rows up to dim1 * dim2 come out of the same call.  Each item gives the
 * ceil(item_bytes 8 / nbits) values of transcode_from_bytes(item, nbits), the coefficients of one plaintext -> out
 * [batch][L_level][N] Ntt, its poly_ntt (scaled = 0) or Delta-scaled to_poly (scaled = 1), as fhe_bfv_encode_dev.
 * item_bytes * 8 > N * nbits -> FHE_E_TOO_MANY_VALUES; nbits outside 1 ... 64 -> FHE_E_ARG; an encoder of a plaintext
 * modulus above 64 bits -> FHE_E_PARAMETER_MISMATCH; level > max -> FHE_E_INVALID_LEVEL.  `bytes` may have any alignment. */
fhe_status fhe_bfv_encode_bytes_dev(const fhe_encoder *enc, int scaled, size_t level, const uint8_t *bytes, size_t nbytes,
                                    size_t item_bytes, size_t nbits, uint64_t *out, size_t batch, void *stream);
/* The SealPIR fold (crates/fhe/examples/sealpir.rs:176-200): words [batch][nseg][seg_len], each word carrying in_bits
 * (higher bits are masked off).  Every segment goes through transcode_bidirectional(segment, in_bits, nbits) on its own
 * -- M = ceil(seg_len in_bits / nbits) values --, the segments' value lists of an item are appended, and
 * PlaintextVec::try_encode(Encoding::poly_at_level) cuts them into nplain = ceil(nseg M / N) plaintexts of N values,
 * the last one zero-padded -> out [batch][nplain][L_level][N] Ntt.  For the fold a segment is c0 or c1 of a ciphertext
 * at its last level (nseg = 2, seg_len = N, in_bits = bits(q_0)).  fhe_bfv_encode_words_count returns nplain (0 for
 * widths outside 1 ... 64 or a NULL encoder).  Refusals as fhe_bfv_encode_bytes_dev; in_bits outside 1 ... 64 ->
 * FHE_E_ARG. */
size_t fhe_bfv_encode_words_count(const fhe_encoder *enc, size_t in_bits, size_t nseg, size_t seg_len, size_t nbits);
fhe_status fhe_bfv_encode_words_dev(const fhe_encoder *enc, int scaled, size_t level, const uint64_t *words, size_t in_bits,
                                    size_t nseg, size_t seg_len, size_t nbits, uint64_t *out, size_t batch, void *stream);
/* The transcoders on their own -- the client's way back (crates/fhe/examples/sealpir.rs:231-252, 273; mulpir.rs:195):
 * transcode_bidirectional (u64 -> u64), transcode_to_bytes (u64 -> bytes, out_bits = 8) and transcode_from_bytes
 * (bytes -> u64, in_bits = 8).  Rows [batch][nin] -> [batch][nout], nout = fhe_transcode_count(in_bits, nin, out_bits)
 * = ceil(nin in_bits / out_bits) (0 for widths outside 1 ... 64).  A side given as bytes (in_is_bytes / out_is_bytes
 * != 0) is an array of uint8_t whose elements carry at most 8 bits; otherwise of uint64_t.  Input bits above in_bits are
 * masked off.  Widths outside 1 ... 64 (1 ... 8 for a byte side) -> FHE_E_ARG.  The call takes no handle: it runs on the
 * calling thread's current device, which `stream` belongs to (as fhe_buf_zero_async). */
size_t fhe_transcode_count(size_t in_bits, size_t nin, size_t out_bits);
fhe_status fhe_transcode_dev(const void *in, int in_is_bytes, size_t in_bits, size_t nin, void *out, int out_is_bytes,
                             size_t out_bits, size_t batch, void *stream);
/* `&Ciphertext + &Plaintext` / `-` (F/bfv/ops/mod.rs:71-108, 166-203): out = ct with c0 +- pt, pt the Delta-scaled
 * form (fhe_bfv_encode_dev with scaled = 1) at the ciphertext's level.  ct, out [batch][nparts][L][N] Ntt; pt
 * [batch][L][N] (or [L][N] shared by the batch when pt_shared != 0); out == ct allowed. */
fhe_status fhe_bfv_add_plain_dev(const fhe_ctx *ctx, int subtract, size_t nparts, const uint64_t *ct, const uint64_t *pt,
                                 int pt_shared, uint64_t *out, size_t batch, void *stream);

/* ------------------------------------------------------------- encryption ---- */
/* Sampling and encryption of BFV ciphertexts.  Device-pointer forms only, with no host-pointer twin: secrets and
 * errors are never staged through host memory by the engine (a host without PyTorch stages through fhe_buf_*).
 *
 * ChaCha8Rng::from_seed(seed) below is the generator whose key is the 32 seed bytes read as little-endian words, with
 * no hashing (Poly::random_from_seed hashes its seed with SHA-256 first).  Its word layout -- 64-bit block counter from
 * 0, stream id 0, next_u64 = two consecutive little-endian words, low word first -- restates rand_chacha, which the
 * reference does not vendor: PARITY UNPINNED against a real fhe.rs run, exactly like fhe_poly_from_seed.
 * sample_vec_cbd (fhe-util/src/lib.rs:22-66) is taken as counter-addressable: within one draw, for v <= 16 sample i is
 * popcount(bits [4v i, 4v i + 2v)) - popcount(bits [4v i + 2v, 4v (i + 1))) of the draw's next_u64 words, least
 * significant bit first; for 17 <= v <= 32 sample i takes the draw's words 2i and 2i + 1.  Each draw starts a fresh
 * pool and drops the bits left in its last word: a draw of N samples consumes ceil(N 4v / 64) words (2N for v > 16),
 * and consecutive draws of one generator start at the next word.  variance outside [1, 32] -> FHE_E_INVALID_VARIANCE.
 *
 * Secret hygiene: the engine's scratch that holds samples (secret key, u, errors) or their transforms is cleared on
 * the stream before it returns to the pool.  The caller's buffers -- s_ntt, and `out` of fhe_bfv_sample_small_dev --
 * are the caller's to clear.  No branch or address of the kernels depends on a sample, a key or a plaintext word.
 * Outputs are canonical words in the usual [batch][parts][L][N] layout; batch == 0 is a no-op (NULL buffers allowed). */
/* Poly::small(ctx, variance, &mut ChaCha8Rng::from_seed(seeds[b])) (M/rq/mod.rs:298-330): seeds [batch][32] ->
 * out [batch][L][N], PowerBasis (to_ntt = 0) or Ntt (to_ntt = 1); negative samples lift to q_i - |x|
 * (try_convert_from(&[i64], ctx, false)).  With to_ntt = 1 over the top-level context this is SecretKey::random
 * (F/bfv/keys/secret_key.rs:41-46) in the s_ntt form fhe_bfv_decrypt_dev takes. */
fhe_status fhe_bfv_sample_small_dev(const fhe_ctx *ctx, size_t variance, const uint8_t *seeds, int to_ntt, uint64_t *out,
                                    size_t batch, void *stream);
/* SecretKey::encrypt_poly (F/bfv/keys/secret_key.rs:100-134): out[b][1] = Poly::random_from_seed(ctx, a_seeds[b])
 * (bit-identical to fhe_poly_from_seed_dev: the wire format's seeded c1), out[b][0] = small(ctx, variance,
 * ChaCha8Rng::from_seed(e_seeds[b]))_ntt - out[b][1] (.) s_ntt + pt[b].  s_ntt [L][N] over ctx; pt [batch][L][N] the
 * Delta-scaled Ntt form fhe_bfv_encode_dev(scaled = 1) writes at ctx's level ([L][N] shared when pt_shared != 0; NULL:
 * the zero plaintext, which is PublicKey::new, F/bfv/keys/public_key.rs:26-30); out [batch][2][L][N] Ntt. */
fhe_status fhe_bfv_encrypt_sk_dev(const fhe_ctx *ctx, size_t variance, const uint64_t *s_ntt, const uint8_t *a_seeds,
                                  const uint8_t *e_seeds, const uint64_t *pt, int pt_shared, uint64_t *out, size_t batch,
                                  void *stream);
/* PublicKey::try_encrypt (F/bfv/keys/public_key.rs:47-97): u, e1, e2 are three consecutive Poly::small draws of one
 * ChaCha8Rng::from_seed(seeds[b]); out[b][0] = u (.) pk[0] + e1 + pt[b], out[b][1] = u (.) pk[1] + e2, all Ntt.  pk
 * [2][L][N] must already be over ctx (the reference switches a copy of the key down to the plaintext's level:
 * fhe_bfv_switch_to_level_dev does that once per level).  pt as fhe_bfv_encrypt_sk_dev. */
fhe_status fhe_bfv_encrypt_pk_dev(const fhe_ctx *ctx, size_t variance, const uint64_t *pk, const uint8_t *seeds,
                                  const uint64_t *pt, int pt_shared, uint64_t *out, size_t batch, void *stream);

/* --------------------------------------------------------- key generation ---- */
/* Key-switching, relinearization and Galois keys made on the device from a device-resident secret.  Device-pointer
 * forms only, with no host-pointer twin: the secret, the errors and s^2 / s_sub never pass through host memory.
 *
 * KeySwitchingKey::new(sk, from, ciphertext_level, ksk_level, rng) (F/bfv/keys/key_switching_key.rs:71-236) with
 * rng = ChaCha8Rng::from_seed(seeds[b]) (the layout of fhe_bfv_sample_small_dev, PARITY UNPINNED like it):
 *   K      = the rng's first 32 bytes (u64 words 0 ... 3): the key's public seed, written to seeds_out[b] when given;
 *   c1[i]  = Poly::random_from_seed(ksk_ctx, bytes [32 i, 32 i + 32) of ChaCha8Rng::from_seed(K)), as Ntt values;
 *   e_i    = the rng's i-th Poly::small(variance) draw, starting at u64 word 4 + i wpd (draws start on word boundaries);
 *   c0[i]  = NTT(e_i) - c1[i] (.) s + g_i (.) from, bit-identical to the reference's NTT(e_i - INTT(c1[i] s) + g_i from).
 * Digits: ndigits = the ciphertext context's moduli count and g_i = RnsContext(moduli[..ndigits]).get_garner(i) mod q_j;
 * for a single-modulus key context the decomposition (:197-236): log_base = log_modulus / 2 with
 * log_modulus = q.next_power_of_two().ilog2(), ndigits = ceil(log_modulus / log_base), g_i = 2^(i log_base) mod q.
 * s_ntt is the level-0 secret in Ntt form (fhe_bfv_sample_small_dev's SecretKey::random); the first Lk rows are read.
 * The handles hold the Shoup twins and, when eligible, the F64 words, as fhe_ksk_create would make them from the
 * exported arrays.  They are ready to use on `stream`; on another stream, synchronise first.  Statuses:
 * FHE_E_INVALID_VARIANCE (variance outside [1, 32]), FHE_E_CONTEXT_NOT_REACHABLE (key level above the ciphertext
 * level), FHE_E_ARG (NULL handle or buffer).  nkeys == 0 is a no-op.  On an error no handle is returned (out[] NULL).
 * Engine scratch holding samples, s^2 or s_sub is cleared before it returns to the pool. */
/* KeySwitchingKey::new for nkeys keys: from_ntt [nkeys][Lk][N] Ntt over ksk_ctx (the reference's `from` after the
 * forward transform), seeds [nkeys][32] -> out[nkeys] handles, seeds_out [nkeys][32] (may be NULL).  from_ntt must
 * hold canonical residues (row j below q_j), as every Ntt-form output of this library does: the words are not checked
 * (fhe_ksk_create_dev's range check waits for the stream; generation never does), and a word >= q_j gives a key whose
 * c0 words and Shoup twins are not canonical. */
fhe_status fhe_ksk_generate_dev(const fhe_ctx *ct_ctx, const fhe_ctx *ksk_ctx, size_t variance, const uint64_t *s_ntt,
                                const uint64_t *from_ntt, const uint8_t *seeds, size_t nkeys, uint8_t *seeds_out,
                                void *stream, fhe_ksk **out);
/* RelinearizationKey::new_leveled (F/bfv/keys/relinearization_key.rs:43-64): from = Switcher(ct_ctx -> key_ctx) of
 * s_ct (.) s_ct (the identity when the two contexts are one).  One key from seed [32]; seed_out [32] may be NULL.  A
 * single-modulus key_ctx -> FHE_E_KEYSWITCH_UNSUPPORTED.  (A switch-up builds the switcher's public tables on the host
 * and waits for the stream before freeing them.) */
fhe_status fhe_bfv_relin_key_generate_dev(const fhe_ctx *ct_ctx, const fhe_ctx *key_ctx, size_t variance,
                                          const uint64_t *s_ntt, const uint8_t *seed, uint8_t *seed_out, void *stream,
                                          fhe_ksk **out);
/* GaloisKey::new (F/bfv/keys/galois_key.rs:26-58) for nkeys exponents (host array) in one batched call: from =
 * Switcher(ct_ctx -> key_ctx) of substitute(s_ct, exponents[b]); key b from seeds[b].  An even exponent (mod 2N) ->
 * FHE_E_INVALID_SUBSTITUTION_EXPONENT.  Use the handles with fhe_bfv_galois_dev(exponent mod 2N). */
fhe_status fhe_bfv_galois_keys_generate_dev(const fhe_ctx *ct_ctx, const fhe_ctx *key_ctx, size_t variance,
                                            const uint64_t *s_ntt, const size_t *exponents, const uint8_t *seeds,
                                            size_t nkeys, uint8_t *seeds_out, void *stream, fhe_ksk **out);
/* A key's arrays as a client sends them: c0, c1 [ndigits][Lk][N] (NttShoup values) and, when not NULL, their Shoup
 * twins floor(c 2^64 / q); device-to-device copies on `stream`.  fhe_ksk_create of the copies makes an equal handle. */
fhe_status fhe_ksk_export_dev(const fhe_ksk *ksk, uint64_t *c0, uint64_t *c1, uint64_t *c0_shoup, uint64_t *c1_shoup,
                              void *stream);
/* A key's digit count: each of fhe_ksk_export_dev's arrays holds ndigits * Lk * N words (0 for NULL). */
size_t fhe_ksk_ndigits(const fhe_ksk *ksk);

/* --------------------------------------------------------- keys on the wire ---- */
/* Key-switching keys to and from the payloads of their KeySwitchingKeyProto messages, on the device.  Device-pointer
 * forms only, with no host-pointer twin.  RelinearizationKey, GaloisKey, EvaluationKey and RGSWCiphertext are one or
 * more such messages.  The envelope checks (representation tag, degree, polynomial counts, seed length) stay with the
 * host that parses the protobuf; these calls move the `coefficients` payloads and the seed.
 *
 * KeySwitchingKey::try_convert_from(&KeySwitchingKeyProto) (F/bfv/keys/key_switching_key.rs:387-482) for nkeys
 * keys of one geometry: c0_bytes [nkeys][ndigits][fhe_poly_serialized_size(ksk_ctx)], the `coefficients` payloads
 * of the c0 Rq messages; exactly one of c1_bytes (same shape) and seeds [nkeys][32] (the message's `seed`) non-NULL.
 * ndigits follows from the contexts and log_base as in the reference (:394-412): ceil(log_modulus / log_base) with
 * log_modulus = q.next_power_of_two().ilog2() for a decomposition key, else the ciphertext context's moduli count.
 * With a seed, c1[i] = Poly::random_from_seed(ksk_ctx, bytes [32 i, 32 i + 32) of ChaCha8Rng::from_seed(seed))
 * (generate_c1; the layout of fhe_ksk_generate_dev, PARITY UNPINNED like it).  The byte pointers need no alignment
 * (16-byte aligned ones take a faster loader from N = 128 on).
 * A handle made here is indistinguishable from fhe_ksk_create of the same words: c0, c1, both Shoup twin arrays, the
 * F64 words when the key is eligible, mode FHE_KS_AUTO.
 * Range check: a coefficient >= q_j anywhere in c0 or an explicit c1 -> FHE_E_ARG ("key coefficient not reduced"),
 * no handle is returned (out[] all NULL) and every buffer is freed, exactly as fhe_ksk_create refuses such a word.
 * The reference takes such words verbatim (Poly::from_bytes does not reduce them, convert.rs:148-160) and would compute
 * with a non-canonical key; here the Shoup quotient of an unreduced word does not fit 64 bits, so the key is refused.
 * Stream: the bytes are untrusted input, so the call waits for `stream` once, after its last launch, to read the
 * check's flag word (fhe_ksk_create_dev waits too: for the same flag word before its twin pass, and before it returns).
 * Keys it returns are therefore ready on any stream.
 * Statuses: the geometry as fhe_ksk_create (FHE_E_DEGREE_MISMATCH, FHE_E_CONTEXT_NOT_REACHABLE,
 * FHE_E_PARAMETER_MISMATCH, FHE_E_KEYSWITCH_UNSUPPORTED, FHE_E_ARG for a bad log_base); both or neither of c1_bytes /
 * seeds, or a NULL handle or buffer with nkeys > 0 -> FHE_E_ARG; nkeys == 0 is a no-op. */
fhe_status fhe_ksk_load_wire_dev(const fhe_ctx *ct_ctx, const fhe_ctx *ksk_ctx, size_t log_base,
                                 const uint8_t *c0_bytes, const uint8_t *c1_bytes, const uint8_t *seeds,
                                 size_t nkeys, void *stream, fhe_ksk **out);
/* The reverse (:365-385): c0 (and c1 when c1_bytes != NULL) taken to PowerBasis and packed, straight from the
 * handle's arrays (no export copy): c0_bytes, c1_bytes [ndigits][fhe_poly_serialized_size(ksk_ctx)].  A seeded message
 * carries c0_bytes and the key's seed instead of c1_bytes.  Asynchronous on `stream`. */
fhe_status fhe_ksk_serialize_dev(const fhe_ksk *ksk, uint8_t *c0_bytes, uint8_t *c1_bytes, void *stream);

/* ------------------------------------------------------------ lift and noise ---- */
/* Residues to integers, and the noise of a ciphertext.  Device-pointer forms only, with no host-pointer twin: the phase
 * and the error polynomial are secret-dependent and are never staged through host memory by the engine.  batch == 0 is
 * a no-op (NULL buffers allowed).  The lift's public constants (q_j^-1 mod q_i, the limbs of q) are built per context
 * by the first call that needs them, with a synchronous allocation and copy: concurrent first calls on a shared handle
 * are safe, but that first call blocks the host and must not be made while its stream is being captured into a graph
 * -- make one call per context (batch 1 will do) before capturing. */
/* W = ceil(bitlen(q) / 64) for q the product of ctx's moduli: the limbs per coefficient fhe_poly_lift_dev writes
 * (0 for a NULL handle; works on host-only handles). */
size_t fhe_ctx_lift_limbs(const fhe_ctx *ctx);
/* RnsContext::lift (M/rns/mod.rs:138-143) per coefficient, as Vec<BigUint>::from(&Poly) applies it
 * (M/rq/convert.rs:507-529): polys [batch][L][N] canonical residues (any representation: the lift is per coefficient;
 * not modified) -> out [batch][N][W] little-endian u64 limbs of the unique x in [0, q) with x = r_i mod q_i. */
fhe_status fhe_poly_lift_dev(const fhe_ctx *ctx, const uint64_t *polys, uint64_t *out, size_t batch, void *stream);
/* The loop of SecretKey::measure_noise (F/bfv/keys/secret_key.rs:88-95) on its own: out_bits[b] = max over the N
 * coefficients of polys[b] of min(bits(x), bits(q - x)), x as in fhe_poly_lift_dev, bits(0) = 0.  No limbs are written;
 * the maximum is per polynomial. */
fhe_status fhe_poly_centered_bits_dev(const fhe_ctx *ctx, const uint64_t *polys, uint64_t *out_bits, size_t batch,
                                      void *stream);
/* SecretKey::measure_noise (F/bfv/keys/secret_key.rs:55-98): noise_bits[b] = the centered bit length of
 * phase(ct[b]) - Plaintext::to_poly(m[b]) (F/bfv/plaintext.rs:172-196), in PowerBasis.  ct [batch][nparts][L][N] Ntt and
 * s_ntt as fhe_bfv_decrypt_dev takes them; the ciphertext context is cipher_plain_scaler's `from`, which must be a
 * level of enc's parameter set (else FHE_E_PARAMETER_MISMATCH) and selects enc's q_mod_t and delta.
 * m_or_null == NULL: m is the ciphertext's own decryption (fhe_bfv_decrypt_dev's value), exactly the reference.
 * m_or_null [batch][N] coefficients in [0, t): the noise against the plaintext the caller expects -- it keeps growing
 * past the point where the ciphertext stops decrypting to m.  nparts == 0 -> FHE_E_ARG.
 * Phase, scaled plaintext, decrypted coefficients and partial maxima live in engine scratch that is cleared before it
 * is reused; m_or_null and noise_bits are the caller's to clear. */
fhe_status fhe_bfv_measure_noise_dev(const fhe_encoder *enc, const fhe_scaler *cipher_plain_scaler, const uint64_t *s_ntt,
                                     const uint64_t *ct, size_t nparts, const uint64_t *m_or_null, uint64_t *noise_bits,
                                     size_t batch, void *stream);

/* --------------------------------------------------------- multiparty BFV ---- */
/* The threshold protocols of eprint 2020/304 (crates/fhe/src/mbfv/): a party's shares and the aggregator's sums.
 * Device-pointer forms only, with no host-pointer twin: secret shares and errors are never staged through host memory
 * by the engine.  The common random polynomial (CRP) is an input, as Ntt words (the reference draws it with
 * Poly::random; fhe_poly_from_seed_dev makes one from a seed).
 *
 * Draws: every share takes its errors from ChaCha8Rng::from_seed(seeds[b]) as consecutive Poly::small draws, draw j
 * starting at u64 word j wpd -- the layout of fhe_bfv_sample_small_dev, PARITY UNPINNED like it.  Each entry point
 * states its draw order.  variance outside [1, 32] -> FHE_E_INVALID_VARIANCE; batch == 0 is a no-op (NULL buffers
 * allowed); a NULL handle or buffer -> FHE_E_ARG; a host-only context -> FHE_E_NO_DEVICE.
 *
 * Secrets: s_ntt (and u_ntt) are a party's secret in Ntt form, as fhe_bfv_sample_small_dev(to_ntt = 1) writes it over
 * the level-0 context; over a deeper ctx its first L rows are read.  s_shared != 0: one secret [L][N] serves the whole
 * batch; s_shared == 0: one party per item, [batch][L0][N] level-0 secrets (L0 rows each, the moduli count of level 0).
 * Secret hygiene: the engine's scratch that holds samples, their transforms or a product with a secret is cleared on the
 * stream before it returns to the pool; the caller's buffers are the caller's to clear.  No branch or address of the
 * kernels depends on a sample or a secret word.  Outputs are canonical Ntt words. */
/* PublicKeyShare::new (mbfv/public_key_gen.rs:32-57): out[b] = e - crp (.) s.  Draws: e.  crp [L][N] over ctx (level
 * 0); out [batch][L][N]. */
fhe_status fhe_mbfv_pk_share_dev(const fhe_ctx *ctx, size_t variance, const uint64_t *crp, const uint64_t *s_ntt,
                                 int s_shared, const uint8_t *seeds, uint64_t *out, size_t batch, void *stream);
/* SecretKeySwitchShare::new (mbfv/secret_key_switch.rs:38-95): out[b] = e + c1[b] (.) (s_in - s_out).  Draws: e.
 * s_out_ntt_or_null == NULL is DecryptionShare::new (:133-142): the zero output key, e + c1 (.) s_in, with no zero key
 * built.  ctx is the ciphertext's level.  c1: the ciphertexts' second parts, item b at c1 + b c1_stride words (2 L N
 * for a [batch][2][L][N] buffer passed at its part 1; 0: one ciphertext for the batch); out [batch][L][N]. */
fhe_status fhe_mbfv_sks_share_dev(const fhe_ctx *ctx, size_t variance, const uint64_t *s_in_ntt,
                                  const uint64_t *s_out_ntt_or_null, int s_shared, const uint64_t *c1, size_t c1_stride,
                                  const uint8_t *seeds, uint64_t *out, size_t batch, void *stream);
/* PublicKeySwitchShare::new (mbfv/public_key_switch.rs:33-92): out[b][0] = pk[0] (.) u + s (.) ct[b][1] + e0,
 * out[b][1] = pk[1] (.) u + e1.  Draws: u, e0, e1 -- fhe_bfv_encrypt_pk_dev with the addend s (.) c1, which lives in
 * engine scratch that is cleared before reuse.  pk [2][L][N] must already be at the ciphertext's level (ctx), as for
 * fhe_bfv_encrypt_pk_dev; ct [batch][2][L][N] ([2][L][N] when ct_shared != 0); out [batch][2][L][N]. */
fhe_status fhe_mbfv_pks_share_dev(const fhe_ctx *ctx, size_t variance, const uint64_t *s_ntt, int s_shared,
                                  const uint64_t *pk, const uint64_t *ct, int ct_shared, const uint8_t *seeds,
                                  uint64_t *out, size_t batch, void *stream);
/* RelinKeyShare<R1>::new (mbfv/relin_key_gen.rs:141-197) over the level-0 context: out_h0[b][i] = e_i - crp[i] (.) u +
 * g_i s, out_h1[b][i] = e'_i + crp[i] (.) s, g_i = RnsContext(moduli).get_garner(i) mod q_r.  Draws: e_0 ... e_{L-1},
 * then e'_0 ... e'_{L-1}.  u_ntt is the party's RelinKeyGenerator::new draw (:92), a fhe_bfv_sample_small_dev(to_ntt =
 * 1) output laid out like s_ntt.  crp [L][L][N]; out_h0, out_h1 [batch][L][L][N].  A single-modulus context ->
 * FHE_E_KEYSWITCH_UNSUPPORTED. */
fhe_status fhe_mbfv_rlk_round1_dev(const fhe_ctx *ctx, size_t variance, const uint64_t *s_ntt, const uint64_t *u_ntt,
                                   int s_shared, const uint64_t *crp, const uint8_t *seeds, uint64_t *out_h0,
                                   uint64_t *out_h1, size_t batch, void *stream);
/* RelinKeyShare<R2>::new (mbfv/relin_key_gen.rs:243-296): out_h0[b][i] = e_i + r1_h0[i] (.) s, out_h1[b][i] = e'_i +
 * r1_h1[i] (.) (u - s).  Draws: as round 1.  r1_h0, r1_h1 [L][L][N]: the aggregated round-1 shares
 * (fhe_mbfv_aggregate_dev of every party's out_h0 / out_h1).  A single-modulus context -> FHE_E_KEYSWITCH_UNSUPPORTED. */
fhe_status fhe_mbfv_rlk_round2_dev(const fhe_ctx *ctx, size_t variance, const uint64_t *s_ntt, const uint64_t *u_ntt,
                                   int s_shared, const uint64_t *r1_h0, const uint64_t *r1_h1, const uint8_t *seeds,
                                   uint64_t *out_h0, uint64_t *out_h1, size_t batch, void *stream);
/* Aggregate::from_shares: out[j] = (base_or_null ? base[j] : 0) + sum_{p < nshares} shares[p share_stride + j] over
 * npolys polynomials [L][N] of canonical words (moduli below 2^62); share_stride in words.  nshares == 0 -> FHE_E_ARG (the
 * reference's NoShares).  out == base_or_null is allowed.  Buffers are 16-byte aligned and share_stride is even.  No
 * draws, no secrets.  With npolys = 1 and no base this is PublicKey::from_shares' part 0 (public_key_gen.rs:60-77; part 1
 * is the CRP, copied by the caller); with base = the ciphertexts' c0 it is Ciphertext::from_shares of both switch
 * protocols (secret_key_switch.rs:98-115, public_key_switch.rs:95-113); with npolys = L it is
 * RelinKeyShare<R1Aggregated>::from_shares (relin_key_gen.rs:200-222). */
fhe_status fhe_mbfv_aggregate_dev(const fhe_ctx *ctx, const uint64_t *shares, size_t nshares, size_t share_stride,
                                  size_t npolys, const uint64_t *base_or_null, uint64_t *out, void *stream);
/* RelinearizationKey::from_shares (mbfv/relin_key_gen.rs:299-351): c0[i] = sum_p r2_h0[p][i] + sum_p r2_h1[p][i],
 * c1[i] = r1_h1[i] (the aggregated round-1 h1), log_base 0, ciphertext and key level 0 (ctx).  r2_h0, r2_h1: nshares
 * arrays [L][L][N] at share_stride words; r1_h1 [L][L][N].  The sums are written straight into the new handle's c0,
 * r1_h1 is copied into its c1, and the handle is finished as fhe_ksk_create_dev finishes it (range check, Shoup twins
 * and F64 words on the device; a word >= q_j -> FHE_E_ARG; the call waits for `stream`).  nshares == 0 -> FHE_E_ARG; a
 * single-modulus context -> FHE_E_KEYSWITCH_UNSUPPORTED.  No draws, no secrets. */
fhe_status fhe_mbfv_relin_key_aggregate_dev(const fhe_ctx *ctx, const uint64_t *r2_h0, const uint64_t *r2_h1,
                                            size_t nshares, size_t share_stride, const uint64_t *r1_h1, void *stream,
                                            fhe_ksk **out);
/* Plaintext::from_shares (mbfv/secret_key_switch.rs:145-186): ct[b][0] + the sum of the decryption shares, then the
 * inverse transform, Scaler::scale and ((d_0 + t) mod q_0) mod t exactly as fhe_bfv_decrypt_dev after its phase.
 * cipher_plain_scaler as fhe_bfv_decrypt_dev; ct [batch][2][L][N] Ntt; shares: nshares arrays [batch][L][N] at
 * share_stride words; out [batch][N] coefficients in [0, t).  nshares == 0 -> FHE_E_ARG.  No draws.  The summed phase
 * and the scaled plaintext live in engine scratch that is cleared before reuse; `out` is the caller's to clear. */
fhe_status fhe_mbfv_decrypt_dev(const fhe_scaler *cipher_plain_scaler, uint64_t plaintext_modulus, const uint64_t *ct,
                                const uint64_t *shares, size_t nshares, size_t share_stride, uint64_t *out, size_t batch,
                                void *stream);

/* ------------------------------------------- plaintext moduli above 64 bits ---- */
/* PlaintextModulus::Large (BfvParametersBuilder::set_plaintext_modulus_biguint, F/bfv/parameters.rs:560-738): t as
 * t_nlimbs little-endian limbs, leading zero limbs trimmed.  W_t = ceil(bits(t) / 64).  A t that fits one limb behaves
 * exactly as fhe_params_create.  Otherwise t < 2^256 (W_t <= 4: the limit of this engine; more ->
 * FHE_E_INVALID_MODULUS), t < Q at level 0 and no q_i divides t (else FHE_E_INVALID_MODULUS); t in [2^62, 2^64) ->
 * FHE_E_INVALID_MODULUS (the reference's InvalidPlaintextModulus).  The down-scalers have the factor t / Q_level; the
 * plaintext context is the shortest prefix of the moduli with at least bits(t) + 60 bits, capped at all of them.
 * Every other handle of the set (contexts, extenders, Multiplicator) is made and used as for a u64 t.  The u64-t entry
 * points return FHE_E_PARAMETER_MISMATCH: fhe_bfv_encode_dev and fhe_bfv_decode_dev given such a set's encoder,
 * fhe_bfv_decrypt(_dev) and fhe_mbfv_decrypt_dev given a scaler whose numerator exceeds 64 bits (fhe_scaler_create
 * remembers that; a scaler made by fhe_scaler_create_from_constants cannot tell).  Nothing computes with a truncated t.  Device-pointer forms only, with no host-pointer twin. */
fhe_status fhe_params_create_big(int device, size_t degree, size_t nmoduli, const uint64_t *moduli,
                                 const uint64_t *t_limbs, size_t t_nlimbs, fhe_params **out);
fhe_status fhe_params_create_big_with_tables(int device, size_t degree, size_t nmoduli, const uint64_t *moduli,
                                             const uint64_t *t_limbs, size_t t_nlimbs, fhe_ntt_tables_fn tables,
                                             void *user, fhe_params **out);
/* W_t, or 1 for a parameter set whose t fits 64 bits (0 for NULL). */
size_t fhe_params_plaintext_limbs(const fhe_params *p);
/* PlaintextVec::try_encode for Vec<BigUint> with Encoding::poly_at_level (F/bfv/plaintext_vec.rs:105-132), or with
 * scaled = 1 the Large branch of Plaintext::to_poly (F/bfv/plaintext.rs:172-197): values [batch][nvalues][W_t] limbs
 * (nvalues <= N, zero-padded; more -> FHE_E_TOO_MANY_VALUES) -> out [batch][L_level][N] Ntt.  Every value is reduced
 * modulo t first, as the u64 encoder does; the result is the reference's bit for bit whenever the value is below t.
 * enc is fhe_encoder_create of a big set (a u64 set's -> FHE_E_PARAMETER_MISMATCH).  FHE_ENCODING_SIMD ->
 * FHE_E_SIMD_UNAVAILABLE (the reference has no NttOperator for a Large t).  level > max -> FHE_E_INVALID_LEVEL. */
fhe_status fhe_bfv_encode_big_dev(const fhe_encoder *enc, int encoding, int scaled, size_t level, const uint64_t *values,
                                  size_t nvalues, uint64_t *out, size_t batch, void *stream);
/* The tail of the Large branch of SecretKey::try_decrypt (F/bfv/keys/secret_key.rs:238-250) alone: polys [batch][P][N],
 * PowerBasis residues over the plaintext context (P rows, product Q_p) -> out [batch][N][W_t] limbs of
 * ((x + t) mod Q_p) mod t, x the CRT lift of the column in [0, Q_p).  `rows` is the row count of the caller's
 * polynomials: anything but P (fhe_encoder_plain_rows) -> FHE_E_PARAMETER_MISMATCH, so that a buffer laid out for
 * another context is never read.  The first call on an encoder uploads the context's lift table (as
 * fhe_poly_lift_dev: it blocks the host and cannot be part of a stream capture). */
fhe_status fhe_bfv_reduce_big_dev(const fhe_encoder *enc, const uint64_t *polys, size_t rows, uint64_t *out, size_t batch,
                                  void *stream);
/* P: the moduli of the encoder's plaintext context (F/bfv/parameters.rs:578-595), for any encoder; 0 for NULL. */
size_t fhe_encoder_plain_rows(const fhe_encoder *enc);
/* SecretKey::try_decrypt, Large branch (F/bfv/keys/secret_key.rs:198-250): as fhe_bfv_decrypt_dev with out
 * [batch][N][W_t] limbs in [0, t).  cipher_plain_scaler: from a level of enc's set to its plaintext context with the
 * factor t / Q_level (any other pair of contexts -> FHE_E_PARAMETER_MISMATCH).  Phase and scaled plaintext live in
 * engine scratch that is cleared before it is reused. */
fhe_status fhe_bfv_decrypt_big_dev(const fhe_encoder *enc, const fhe_scaler *cipher_plain_scaler, const uint64_t *s_ntt,
                                   const uint64_t *ct, size_t nparts, uint64_t *out, size_t batch, void *stream);
/* Plaintext::from_shares (mbfv/secret_key_switch.rs:145-186) with the Large tail: as fhe_mbfv_decrypt_dev with out
 * [batch][N][W_t] limbs. */
fhe_status fhe_mbfv_decrypt_big_dev(const fhe_encoder *enc, const fhe_scaler *cipher_plain_scaler, const uint64_t *ct,
                                    const uint64_t *shares, size_t nshares, size_t share_stride, uint64_t *out,
                                    size_t batch, void *stream);
/* fhe_bfv_measure_noise_dev given the encoder of a big set reads m_or_null as [batch][N][W_t] limbs. */

/* ------------------------------------------------- zq::primes (host, no GPU) ---- */
/* generate_prime (M/zq/primes.rs:30-59): returns 0 when none exists. */
uint64_t fhe_generate_prime(size_t num_bits, uint64_t modulo, uint64_t upper_bound);
int fhe_supports_opt(uint64_t p);                                      /* M/zq/primes.rs:10-24 */
int fhe_is_prime(uint64_t p);                                          /* fhe-util/src/lib.rs:16-18 */
/* BfvParametersBuilder::generate_moduli (F/bfv/parameters.rs:391-431). */
fhe_status fhe_generate_moduli(const size_t *sizes, size_t count, size_t degree, uint64_t *out);

/* ---------------------------------------------------------- bench / test aids ---- */
/* Counter-based synthetic residues written on the device:
 * x = splitmix64(seed ^ (ct<<40) ^ (part<<36) ^ (row<<28) ^ coeff) mod q_row for
 * out[b][part_local][row][coeff], ct = ct0 + b, part = part0 + part_local. */
fhe_status fhe_synth_uniform_dev(const fhe_ctx *ctx, uint64_t seed, uint64_t ct0, uint64_t part0, size_t nparts,
                                 uint64_t *out, size_t batch, void *stream);
/* The engine keeps its scratch buffers (grow-only, reused in stream order per device), its internal second
 * streams and a few pooled events between calls; this frees every idle one (call it while no engine call is
 * running) and returns the number of scratch bytes released.  (Up to eight idle internal stream HANDLES stay parked
 * for reuse -- a stream holds no device memory, and the runtime assigns a stream's hardware queue once, at creation:
 * a re-created stream can land on the caller's queue and serialise the two lanes of a multiply.) */
size_t fhe_workspace_trim(void);
/* Bounds on what the engine RETAINS between calls: `per_stream_bytes` for the scratch blocks keyed to one
 * (device, stream), `total_bytes` over all of them; 0 = no bound.  Defaults: no per-stream bound, total = a quarter of
 * the device's memory (at least 8 GiB) -- pass FHE_WORKSPACE_DEFAULT to ask for it again.  Idle blocks beyond a bound are
 * evicted least-recently-used first, when a block is released and before a stream's block grows; blocks in use are
 * never refused (a call that needs more than the bound runs, its blocks are not kept afterwards).
 * Hosts that create and destroy their OWN HIP streams (torch, hip-rs): the engine is never told that such a stream is
 * gone and has no safe way to ask (hipStreamQuery on a destroyed handle crashes in this runtime), so what it kept for
 * it -- scratch blocks, an internal second stream -- stays until it is the least recently used: blocks under the
 * `total_bytes` bound, internal streams beyond 32 live user streams.  Such a host sets `total_bytes` to a few times
 * one stream's footprint (tests: 1,000 short-lived streams stay within 2x of one), or calls fhe_workspace_trim.
 * Scratch blocks come from the library's private stream-ordered SCRATCH pool; a stream's own blocks return to it in
 * stream order (growing does not synchronise the device), other streams' blocks are evicted with hipFree (which waits).
 * `total_bytes` is PER DEVICE (the default a quarter of that device's memory), and it bounds DEVICE MEMORY, not only the
 * engine's bookkeeping: the scratch pool's release threshold is the bound and evictions trim the pool, so another
 * allocator in the process (torch, the host's own hipMalloc) gets the memory back.  fhe_buf_alloc_async has its own pool
 * (BUFFERS), which keeps what is freed into it until fhe_workspace_trim.
 * fhe_workspace_stats: bytes held (idle + in use), bytes in use, blocks, distinct (device, stream) owners, internal
 * second streams alive.  fhe_workspace_pool_stats: what the DRIVER says the two pools of `device` hold -- reserved
 * (backed by device memory) and used (handed out) bytes of each (hipMemPoolAttrReservedMemCurrent / UsedMemCurrent). */
#define FHE_WORKSPACE_DEFAULT ((size_t)-1)
fhe_status fhe_workspace_set_limit(size_t per_stream_bytes, size_t total_bytes);
fhe_status fhe_workspace_get_limit(size_t *per_stream_bytes, size_t *total_bytes);
fhe_status fhe_workspace_stats(size_t *held_bytes, size_t *in_use_bytes, size_t *blocks, size_t *owners,
                               size_t *internal_streams);
fhe_status fhe_workspace_pool_stats(int device, size_t *scratch_reserved_bytes, size_t *scratch_used_bytes,
                                    size_t *buffers_reserved_bytes, size_t *buffers_used_bytes);
/* Integer-issue ceiling ("report both ceilings"): register-resident loops of the instructions /
 * butterflies the NTT-type kernels are made of, chip-wide, no memory traffic, run for at least min_seconds
 * (0 < min_seconds <= 10).  which: 0 v_mad_u64_u32, 1 v_mul_lo_u32, 2 v_mul_hi_u32, 3 lazy Shoup product,
 * 4 forward butterfly (any modulus < 2^62), 5 forward butterfly for moduli < 2^60, 6 inverse butterfly,
 * 7 the key switch's Shoup multiply-accumulate, 8 the tensor product of slots 0 / 2 (one product + single-word Barrett),
 * 9 the tensor product of slot 1 (two products, one 128-bit sum, one Barrett); 10-15 (round 6) the FP64 forms for
 * moduli below 2^50 (csrc/zq_f64.hpp): 10 v_fma_f64, 11 v_rndne_f64, 12 exact lazy modular product, 13 forward and
 * 14 inverse butterfly with their amortised reductions, 15 the key switch's multiply-accumulate;
 * *ops_per_s = lane-operations (multiplies / products / butterflies) per second.  Measurement aid, not on the path.
 * fhe_ubench_scaler: RnsScaler::scale's ceiling -- the scale_kernel instance that serves `scaler`, run over coefficient
 * columns that all alias ONE polynomial (L2 resident: the instruction stream without HBM traffic); *columns_per_s
 * chip-wide.  With these, bench.py prices every kernel family of ct x ct + relinearise against an integer ceiling. */
fhe_status fhe_ubench_int(int device, int which, double min_seconds, double *ops_per_s);
fhe_status fhe_ubench_scaler(const fhe_scaler *scaler, double min_seconds, double *columns_per_s);
/* The box's own streaming rate: a 16-byte-per-lane copy of `bytes` bytes with streaming loads / stores (the path's
 * element-wise kernels are made of the same accesses); *bytes_per_s = read + write bytes per second. */
fhe_status fhe_ubench_copy(int device, size_t bytes, double min_seconds, double *bytes_per_s);
/* Execution option (round 6): rows whose moduli are all below 2^50 -- every modulus of the reference's stock parameter sets,
 * F/bfv/parameters.rs:222-251 -- run their transforms and key-switch accumulations on the FP64 FMA pipe (exact arithmetic on
 * doubles holding integers, csrc/zq_f64.hpp); on = 0 sends them to the integer kernels like every wider modulus.  Results
 * are bit-identical either way (canonical residues are a function of the inputs); default on; process-wide, read per launch. */
void fhe_engine_set_f64(int on);
int fhe_engine_get_f64(void);
/* Per-kernel HIP-event timing (events carried by the launches, on the launching stream).  One entry per (launch label,
 * kernel symbol): fhe_prof_get gives the entry's label -- several entries share a label when several instantiations of a
 * kernel template run under it; sum them for the family -- and fhe_prof_get_symbol the kernel's demangled symbol, the
 * name rocprofv3 lists it under.  (No reference counterpart: fhe.rs times with Criterion on the host.) */
void fhe_prof_enable(int on);
void fhe_prof_reset(void);
size_t fhe_prof_count(void);
fhe_status fhe_prof_get(size_t index, char *name, size_t name_cap, uint64_t *launches, double *total_ms);
fhe_status fhe_prof_get_symbol(size_t index, char *symbol, size_t symbol_cap);

#ifdef __cplusplus
}
#endif
#endif /* FHE_HIP_H */
