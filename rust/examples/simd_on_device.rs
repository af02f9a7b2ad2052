//! A host that drives the engine without the patched crates: SIMD-encode a batch of plaintexts on the GPU, multiply
//! resident ciphertexts by them, rotate the columns, add a Delta-scaled plaintext, decrypt and decode -- one upload of the
//! values, one download of the result.  (The handles are built once by the host: the parameter set with its NTT tables,
//! a Galois key for exponent 3, the cipher-to-plaintext scaler from the parameter set's `CipherPlainContext`, and the
//! secret key in Ntt form.)  (No Rust toolchain exists in the build image: reviewed source, not compiled there.)
use std::sync::Arc;

use fhe_math_hip::{DeviceBuffer, DeviceCiphertexts, Encoding, HipError, HipKsk, HipParams, HipScaler, Stream};

/// slots of (ct * values) rotated by one column, plus `offset` -- then minus `offset` again: the rotated product
#[allow(clippy::too_many_arguments)]
pub fn rotated_product_slots(
    params: &Arc<HipParams>,
    galois_key_3: &HipKsk,          // rotates_columns_by(1): exponent 3
    decrypt_scaler: &HipScaler,     // CipherPlainContext::scaler at level 0
    plaintext_modulus: u64,
    s_ntt: &DeviceBuffer,           // the secret key over the level-0 context, Ntt form
    cts: &DeviceCiphertexts,        // level 0, two parts each
    values: &[u64],                 // one row of N slot values per ciphertext
    offset: &[u64],                 // N slot values added and taken away again
) -> Result<Vec<u64>, HipError> {
    let s = Stream::new(fhe_math_hip::default_device())?;
    let enc = params.encoder(None)?;
    let ctx = params.context_at_level(0)?;
    let n = ctx.degree();
    let dv = DeviceBuffer::alloc_on(ctx.device(), values.len(), &s)?;
    dv.upload(values, &s)?;
    let doff = DeviceBuffer::alloc_on(ctx.device(), offset.len(), &s)?;
    doff.upload(offset, &s)?;
    let pts = enc.encode_dev(Encoding::Simd, false, 0, &dv, n, &s)?;          // poly_ntt, [batch][L][N]
    let off = enc.encode_dev(Encoding::Simd, true, 0, &doff, n, &s)?;         // to_poly(), shared by the batch
    let prod = ctx.mul_plain_dev(cts, &pts, &s)?;
    let rot = galois_key_3.galois_dev(3, &prod, &s)?;
    let shifted = rot.add_plain_dev(&ctx, &off, &s)?;
    let back = shifted.sub_plain_dev(&ctx, &off, &s)?;
    let coeffs = decrypt_scaler.decrypt_dev(plaintext_modulus, s_ntt, &back, &s)?;
    let slots = enc.decode_dev(Encoding::Simd, &coeffs, &s)?;
    let mut out = vec![0u64; slots.len()];
    slots.download(&mut out, &s)?;                                            // the only wait
    for d in [prod, rot, shifted, back] {
        d.release_on(&s)?;
    }
    for b in [dv, doff, pts, off, coeffs, slots] {
        b.release_on(&s)?;
    }
    Ok(out)
}
