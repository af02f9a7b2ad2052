//! A client that encrypts on the GPU: a secret key drawn on the device, its public key, then a batch of SIMD-encoded
//! plaintexts encrypted under both keys and decrypted again -- the values are uploaded once, the secret never leaves
//! the device.  (The handles are built once by the host: the parameter set and the cipher-to-plaintext scaler from
//! its `CipherPlainContext`.)  (No Rust toolchain exists in the build image: reviewed source, not compiled there.)
use std::sync::Arc;

use fhe_math_hip::{DeviceBuffer, DeviceCiphertexts, DeviceSeeds, Encoding, HipEncoder, HipError, HipParams, HipScaler,
                   Stream};

fn decrypt_slots(enc: &HipEncoder, scaler: &HipScaler, t: u64, s_ntt: &DeviceBuffer, ct: &DeviceCiphertexts, s: &Stream)
                 -> Result<Vec<u64>, HipError> {
    let coeffs = scaler.decrypt_dev(t, s_ntt, ct, s)?;
    let slots = enc.decode_dev(Encoding::Simd, &coeffs, s)?;
    let mut v = vec![0u64; slots.len()];
    slots.download(&mut v, s)?;
    coeffs.release_on(s)?;
    slots.release_on(s)?;
    Ok(v)
}

/// Encrypts `values` (one row of N slot values per plaintext) under a fresh secret key and under its public key,
/// decrypts both batches and returns the decoded slots `(sk, pk)`.  The 32-byte seeds come from the caller's CSPRNG:
/// `key_seeds` = the secret key's and the public key's two; `a`, `e` (secret-key form) and `u` (public-key form) one per
/// plaintext.
pub fn encrypt_roundtrip(
    params: &Arc<HipParams>,
    decrypt_scaler: &HipScaler,     // CipherPlainContext::scaler at level 0
    plaintext_modulus: u64,
    variance: usize,                // BfvParameters::variance (10 by default)
    values: &[u64],
    key_seeds: [[u8; 32]; 3],
    a_seeds: &[[u8; 32]],
    e_seeds: &[[u8; 32]],
    u_seeds: &[[u8; 32]],
) -> Result<(Vec<u64>, Vec<u64>), HipError> {
    let s = Stream::new(fhe_math_hip::default_device())?;
    let enc = params.encoder(None)?;
    let ctx = params.context_at_level(0)?;
    let n = ctx.degree();
    let dev = ctx.device();
    let sk_seed = DeviceSeeds::upload(dev, &key_seeds[0..1], &s)?;
    let s_ntt = ctx.sample_small_dev(variance, &sk_seed, true, &s)?;          // SecretKey::random, Ntt form
    let pk_a = DeviceSeeds::upload(dev, &key_seeds[1..2], &s)?;
    let pk_e = DeviceSeeds::upload(dev, &key_seeds[2..3], &s)?;
    let pk = ctx.encrypt_sk_dev(0, variance, &s_ntt, &pk_a, &pk_e, None, &s)?; // PublicKey::new
    let dv = DeviceBuffer::alloc_on(dev, values.len(), &s)?;
    dv.upload(values, &s)?;
    let pts = enc.encode_dev(Encoding::Simd, true, 0, &dv, n, &s)?;          // to_poly(), [batch][L][N]
    let a = DeviceSeeds::upload(dev, a_seeds, &s)?;
    let e = DeviceSeeds::upload(dev, e_seeds, &s)?;
    let u = DeviceSeeds::upload(dev, u_seeds, &s)?;
    let ct_sk = ctx.encrypt_sk_dev(0, variance, &s_ntt, &a, &e, Some(&pts), &s)?;
    let ct_pk = ctx.encrypt_pk_dev(variance, &pk, &u, Some(&pts), &s)?;
    let got_sk = decrypt_slots(&enc, decrypt_scaler, plaintext_modulus, &s_ntt, &ct_sk, &s)?;
    let got_pk = decrypt_slots(&enc, decrypt_scaler, plaintext_modulus, &s_ntt, &ct_pk, &s)?;
    // the secret key is the caller's to clear: zeroed before its memory returns to the allocator
    s_ntt.upload(&vec![0u64; s_ntt.len()], &s)?;
    for d in [ct_sk, ct_pk, pk] {
        d.release_on(&s)?;
    }
    for b in [dv, pts, s_ntt] {
        b.release_on(&s)?;
    }
    for sd in [sk_seed, pk_a, pk_e, a, e, u] {
        sd.release_on(&s)?;
    }
    Ok((got_sk, got_pk))
}
