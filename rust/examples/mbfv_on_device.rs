//! Three parties run the threshold protocols of `fhe::mbfv` (eprint 2020/304) on one GPU: a collective public key, an
//! encryption under it, a collective relinearization key, a public-key switch to a receiver and a threshold
//! decryption.  Every party's secret is drawn on the device and never leaves it; in a real deployment each party runs
//! its own share calls on its own device and only the shares travel.  The common random polynomials are public inputs
//! (`crp`: `[L][N]`, `crp_vec`: `[L][L][N]` Ntt words, e.g. from `fhe_poly_from_seed`).  (No Rust toolchain exists in
//! the build image: reviewed source, not compiled there.)
use std::sync::Arc;

use fhe_math_hip::{DeviceBuffer, DeviceCiphertexts, DeviceSeeds, Encoding, HipCtx, HipError, HipKsk, HipParams, HipScaler,
                   PartySecrets, Stream};

/// Returns the decoded slots of the threshold decryption, the collective relinearization key and the ciphertext
/// switched to the receiver.  Seeds come from the parties' CSPRNGs, one per party in each array: `secret_seeds`
/// (SecretKey::random), `ephemeral_seeds` (RelinKeyGenerator::new's u) and `share_seeds` for the five protocols in the
/// order public key, relin round 1, relin round 2, public-key switch, decryption.
#[allow(clippy::too_many_arguments)]
pub fn threshold_session(
    params: &Arc<HipParams>,
    ctx0: &Arc<HipCtx>,               // the level-0 context the collective key lives over
    decrypt_scaler: &HipScaler,       // CipherPlainContext::scaler at level 0
    plaintext_modulus: u64,
    variance: usize,
    crp: &[u64],
    crp_vec: &[u64],
    receiver_pk: &DeviceCiphertexts,  // the public key the ciphertext is switched to
    values: &[u64],
    secret_seeds: &[[u8; 32]],
    ephemeral_seeds: &[[u8; 32]],
    share_seeds: [&[[u8; 32]]; 5],
    encrypt_seed: [u8; 32],
) -> Result<(Vec<u64>, HipKsk, DeviceCiphertexts), HipError> {
    let s = Stream::new(fhe_math_hip::default_device())?;
    let enc = params.encoder(None)?;
    let ctx = params.context_at_level(0)?;
    let (n, rows, dev) = (ctx.degree(), ctx.nmoduli(), ctx.device());
    let parties = secret_seeds.len();
    let up = |sd: &[[u8; 32]]| DeviceSeeds::upload(dev, sd, &s);
    // every party's secret and ephemeral secret in one call each: [parties][L][N], Ntt
    let sk = ctx.sample_small_dev(variance, &up(secret_seeds)?, true, &s)?;
    let u = ctx.sample_small_dev(variance, &up(ephemeral_seeds)?, true, &s)?;
    let each = PartySecrets::PerItem { secrets: &sk, level0_rows: rows };
    let d_crp = DeviceBuffer::alloc_on(dev, crp.len(), &s)?;
    d_crp.upload(crp, &s)?;
    let d_crpv = DeviceBuffer::alloc_on(dev, crp_vec.len(), &s)?;
    d_crpv.upload(crp_vec, &s)?;
    // PublicKey::from_shares: [sum of the shares, crp]
    let p0 = ctx.mbfv_pk_share_dev(variance, &d_crp, &each, &up(share_seeds[0])?, &s)?;
    let pk0 = ctx.mbfv_aggregate_dev(&p0, parties, None, &s)?;
    let mut pk_words = vec![0u64; pk0.len()];
    pk0.download(&mut pk_words, &s)?;
    pk_words.extend_from_slice(crp);
    let pk = DeviceCiphertexts::upload(dev, &pk_words, 2, rows, n, 0, &s)?;
    // the two rounds of the relinearization-key protocol
    let (r1_h0, r1_h1) = ctx.mbfv_rlk_round_dev(variance, &each, &u, &d_crpv, None, &up(share_seeds[1])?, &s)?;
    let (a_h0, a_h1) = (ctx.mbfv_aggregate_dev(&r1_h0, parties, None, &s)?, ctx.mbfv_aggregate_dev(&r1_h1, parties, None, &s)?);
    let (r2_h0, r2_h1) = ctx.mbfv_rlk_round_dev(variance, &each, &u, &d_crpv, Some((&a_h0, &a_h1)), &up(share_seeds[2])?, &s)?;
    let rk = HipKsk::from_relin_shares_dev(ctx0, &r2_h0, &r2_h1, parties, &a_h1, &s)?;
    // encrypt under the collective key
    let dv = DeviceBuffer::alloc_on(dev, values.len(), &s)?;
    dv.upload(values, &s)?;
    let pts = enc.encode_dev(Encoding::Simd, true, 0, &dv, n, &s)?;
    let ct = ctx.encrypt_pk_dev(variance, &pk, &up(&[encrypt_seed])?, Some(&pts), &s)?;
    // PublicKeySwitchShare: hand the ciphertext to the receiver -- [c0 + sum h0, sum h1]
    let h = ctx.mbfv_pks_share_dev(variance, &each, receiver_pk, &ct, &up(share_seeds[3])?, &s)?;
    let mut base = ct.download(&s)?;
    for w in &mut base[rows * n..] {
        *w = 0;
    }
    let d_base = DeviceBuffer::alloc_on(dev, base.len(), &s)?;
    d_base.upload(&base, &s)?;
    let switched_words = ctx.mbfv_aggregate_dev(h.buffer(), parties, Some(&d_base), &s)?;
    let mut sw = vec![0u64; switched_words.len()];
    switched_words.download(&mut sw, &s)?;
    let switched = DeviceCiphertexts::upload(dev, &sw, 2, rows, n, 0, &s)?;
    // the secret-key switch to the zero key is the decryption protocol: one share per party, then Plaintext::from_shares
    let d = ctx.mbfv_sks_share_dev(variance, &each, None, &ct, &up(share_seeds[4])?, &s)?;
    let coeffs = decrypt_scaler.mbfv_decrypt_dev(plaintext_modulus, &ct, &d, parties, &s)?;
    let slots = enc.decode_dev(Encoding::Simd, &coeffs, &s)?;
    let mut got = vec![0u64; slots.len()];
    slots.download(&mut got, &s)?;
    // the secrets are the caller's to clear: zeroed before their memory returns to the allocator
    for b in [&sk, &u] {
        b.upload(&vec![0u64; b.len()], &s)?;
    }
    for b in [sk, u, d_crp, d_crpv, p0, pk0, r1_h0, r1_h1, a_h0, a_h1, r2_h0, r2_h1, dv, pts, d_base, switched_words, d, coeffs, slots] {
        b.release_on(&s)?;
    }
    for c in [pk, ct, h] {
        c.release_on(&s)?;
    }
    Ok((got, rk, switched))
}
