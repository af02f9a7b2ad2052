// kernels.hpp -- hand-written HIP kernels (gfx950 / CDNA4) for the fhe.rs BFV hot path.
//
// Layout in HBM: every polynomial is `[rows][N]` u64 row-major exactly as rq::Poly
// (M/rq/mod.rs:126-133); batches add outer dimensions.  Row-wise phases (NTT, key-switch) use
// one workgroup per residue row with the row staged in LDS; column-wise phases (RNS scaler,
// modulus switch) use one lane per coefficient so that all row reads/writes are coalesced
// along N -- no transposes anywhere.  No MFMA: this is 64-bit modular integer arithmetic.
//
// Kernel inventory (reference loop each one replaces):
//   ntt_kernel<false/true>  NttOperator::forward / backward        M/ntt/native.rs:77-233
//   ntt_global_kernel<..>   first/last radix stages for N > 16384   (row does not fit LDS)
//   ks_fused_kernel         KeySwitchingKey::key_switch             F/bfv/keys/key_switching_key.rs:241-320
//                           (+ lazy lift M/rq/mod.rs:563-586 + Shoup MAC M/rq/ops.rs:208-245)
//   ks_fused_split_kernel   the same for N >= 32768: per 8192-point sub-block, first stages in the loader
//   ks_mac_keyed_kernel     stage B of the unfused key switch with one key per group of polynomials (keyed batches:
//                           KeySwitchingKey::key_switch client by client)   F/bfv/keys/key_switching_key.rs:241-320
//   hoist_mac_kernel        stage B for many Galois elements of one ciphertext on ONE digit decomposition (hoisted
//                           rotations; a restatement, not the reference's words: kernels_kshoist.hpp)
//   hoist_matvec_kernel     the same with each rotation multiplied by its plaintext diagonal and the products summed in
//                           registers (a plaintext matrix times an encrypted vector; hoist_mac_kernel + dot_kernel's words)
//   bsgs_baby_kernel<GT>, bsgs_giant_kernel   the baby-step/giant-step form of that product: G inner sums from one digit
//                           loop per baby rotation, then the giants' key switches summed in registers (kernels_bsgs.hpp)
//   hoist_mac_keyed_kernel, hoist_matvec_keyed_kernel   hoist_mac_kernel / hoist_matvec_kernel with one Galois key set per
//                           client: the key of (ciphertext, rotation) from a client-major table (kernels_kshoistkeyed.hpp)
//   scale_kernel            RnsScaler::scale per column             M/rns/scaler.rs:249-352, M/rq/scaler.rs:85-94
//   switch_down_kernel      Poly::switch_down                       M/rq/mod.rs:433-492
//   substitute_kernel       Poly::substitute                        M/rq/mod.rs:360-412
//   tensor_intt_kernel      tensor step fused with the following inverse NTT   F/bfv/ops/mul.rs:198-205
//   ew_kernel / tensor_kernel / tensor_general_kernel / mul_shoup_kernel   M/rq/ops.rs:10-245, F/bfv/ops/mul.rs:198-201,
//                                                                   F/bfv/ops/mod.rs:300-327
//   dot_kernel, mul_plain_kernel        dot_product_scalar, ct x pt F/bfv/ops/dot_product.rs:54-180, ops/mod.rs:229-257
//   expand_step_kernel, monomial_kernel EvaluationKey::expands      F/bfv/keys/evaluation_key.rs:192-256
//   phase_kernel, decrypt_tail_kernel   SecretKey::try_decrypt      F/bfv/keys/secret_key.rs:198-247
//   wire_pack_kernel, wire_unpack_kernel  Rq payload bit packing    M/rq/convert.rs:17-99, fhe-util lib.rs:71-148
//   synth_kernel            synthetic uniform residues (bench/test inputs)
//   encode_simd_t_kernel, encode_lift_kernel, decode_simd_kernel   PlaintextVec::try_encode, Plaintext::to_poly, decoders
//                                                                   F/bfv/plaintext_vec.rs:70-102, plaintext.rs:157-196
//   add_plain_kernel        ct +- pt                                 F/bfv/ops/mod.rs:71-108, 166-203
//   cbd_sample_kernel, small_ntt_kernel, encrypt_sk_kernel, encrypt_pk_kernel   Poly::small, SecretKey::encrypt_poly,
//                           PublicKey::try_encrypt   M/rq/mod.rs:298-330, F/bfv/keys/secret_key.rs:100-134, public_key.rs:47-97
//   ksk_seeds_kernel, cbd_sample_at_kernel, ksk_consts_kernel, ksk_gen_kernel, galois_from_kernel   KeySwitchingKey::new,
//                           RelinearizationKey / GaloisKey::new   F/bfv/keys/key_switching_key.rs:71-236, galois_key.rs:26-58
//   ksk_dseeds_kernel, ksk_load_kernel, ksk_twin_ew_kernel   KeySwitchingKey::try_convert_from(&KeySwitchingKeyProto): the
//                           wire bytes to a handle's arrays, twins and F64 words   F/bfv/keys/key_switching_key.rs:387-482
//   lift_kernel, noise_max_kernel       RnsContext::lift, SecretKey::measure_noise   M/rns/mod.rs:138-143, F/bfv/keys/secret_key.rs:55-98
//   mbfv_share_kernel, mbfv_sum_kernel  the shares of the multiparty protocols and their aggregation   F/mbfv/*.rs
//   bigt_project_kernel, bigt_tail_kernel   plaintext moduli above 64 bits: Vec<BigUint> encoding and the Large branch of
//                           SecretKey::try_decrypt   F/bfv/plaintext_vec.rs:105-132, plaintext.rs:172-197, secret_key.rs:238-250
//   encode_stream_kernel, transcode_ew_kernel   plaintexts from packed bits: fhe_util::transcode_* + Plaintext::try_encode
//                           (encode_database, the SealPIR fold)   fhe-util lib.rs:71-190, examples/util.rs:97-145, sealpir.rs:176-200
// There are no build variants: measured-and-rejected alternatives are listed in docs/HISTORY.md, their code is in git.
#pragma once
#include "kernels_common.hpp"
#include "kernels_passes.hpp"
#include "kernels_ntt.hpp"
#include "kernels_ks.hpp"
#include "kernels_kskeyed.hpp"
#include "kernels_kshoist.hpp"
#include "kernels_bsgs.hpp"
#include "kernels_kshoistkeyed.hpp"
#include "kernels_scaler.hpp"
#include "kernels_misc.hpp"
#include "kernels_encode.hpp"
#include "kernels_encrypt.hpp"
#include "kernels_keygen.hpp"
#include "kernels_keyload.hpp"
#include "kernels_noise.hpp"
#include "kernels_mbfv.hpp"
#include "kernels_bigt.hpp"
#include "kernels_transcode.hpp"
