//! Noise budgeting on the GPU: how many bits of noise a batch of ciphertexts carries, measured against the plaintexts
//! the caller expects and against the ciphertexts' own decryption, without the phase or the secret key leaving the
//! device; and `RnsContext::lift` of a batch of polynomials (the integers in [0, q) as u64 limbs), with the centered
//! bit length of each.  (No Rust toolchain exists in the build image: reviewed source, not compiled there.)
use fhe_math_hip::{DeviceBuffer, DeviceCiphertexts, HipEncoder, HipError, HipParams, HipScaler, Stream};

/// `(noise against expected, noise against the own decryption)`, one value per ciphertext.  `expected`: the
/// plaintexts' coefficients mod t, `[batch][N]` on the device (what `HipScaler::decrypt_dev` writes).
pub fn noise_of(enc: &HipEncoder, scaler: &HipScaler, s_ntt: &DeviceBuffer, ct: &DeviceCiphertexts, expected: &DeviceBuffer,
                s: &Stream) -> Result<(Vec<u64>, Vec<u64>), HipError> {
    let given = enc.measure_noise_dev(scaler, s_ntt, ct, Some(expected), s)?;
    let own = enc.measure_noise_dev(scaler, s_ntt, ct, None, s)?;      // SecretKey::measure_noise as the reference has it
    let mut a = vec![0u64; given.len()];
    let mut b = vec![0u64; own.len()];
    given.download(&mut a, s)?;
    own.download(&mut b, s)?;
    given.release_on(s)?;
    own.release_on(s)?;
    Ok((a, b))
}

/// The coefficients of `polys` (`[batch][L][N]` residues over level `level`) as W-limb integers `[batch][N][W]`, and
/// each polynomial's centered bit length.
pub fn integers_of(params: &HipParams, level: usize, polys: &DeviceBuffer, s: &Stream)
                   -> Result<(usize, Vec<u64>, Vec<u64>), HipError> {
    let ctx = params.context_at_level(level)?;
    let w = ctx.lift_limbs();
    let limbs = ctx.lift_dev(polys, s)?;
    let bits = ctx.centered_bits_dev(polys, s)?;
    let mut x = vec![0u64; limbs.len()];
    let mut b = vec![0u64; bits.len()];
    limbs.download(&mut x, s)?;
    bits.download(&mut b, s)?;
    limbs.release_on(s)?;
    bits.release_on(s)?;
    Ok((w, x, b))
}
