//! A server that receives a client's evaluation key as serialized messages and rotates with it: the `coefficients`
//! payloads of every Galois key's `c0` polynomials go to the device as they are, the keys are loaded there in one call
//! (unpacked, transformed, range-checked, with their Shoup twins), and a ciphertext is rotated with one of them.
//! (No Rust toolchain exists in the build image: reviewed source, not compiled there.)
use std::sync::Arc;

use fhe_math_hip::{DeviceBuffer, DeviceCiphertexts, DeviceSeeds, HipCtx, HipError, HipKsk, Stream, WireC1};

/// `c0_payloads[b]` is `proto.c0[0].coefficients ++ proto.c0[1].coefficients ++ ...` of key b and `seeds[b]` its
/// `proto.seed`; `exponents[b]` the Galois exponent it serves.  Rotates `ct` by `exponents[which]` and hands key
/// `which` back as the message a peer would receive.
pub fn load_and_rotate(ctx: &Arc<HipCtx>, exponents: &[usize], c0_payloads: &[Vec<u8>], seeds: &[[u8; 32]], which: usize,
                       ct: &DeviceCiphertexts) -> Result<(DeviceCiphertexts, Vec<u64>), HipError> {
    let s = Stream::new(ctx.device())?;
    let nkeys = exponents.len();
    let ndigits = ctx.nmoduli();
    assert_eq!(c0_payloads.len(), nkeys);
    let per_key = ndigits * ctx.serialized_size();
    let bytes: Vec<u8> = c0_payloads.iter().flat_map(|p| {
        assert_eq!(p.len(), per_key);
        p.iter().copied()
    }).collect();
    let c0 = DeviceBuffer::upload_bytes(ctx.device(), &bytes, &s)?;
    let sd = DeviceSeeds::upload(ctx.device(), seeds, &s)?;
    let keys = HipKsk::from_wire_dev(ctx, ctx, 0, ndigits, &c0, WireC1::Seeds(&sd), nkeys, &s)?;
    let rotated = keys[which].galois_dev(exponents[which], ct, &s)?;
    // the reverse: the key's c0 payloads again (a seeded message carries the seed, not c1)
    let (back, none) = keys[which].to_wire_dev(false, &s)?;
    assert!(none.is_none());
    let mut out = vec![0u64; back.len()];
    back.download(&mut out, &s)?;
    back.release_on(&s)?;
    c0.release_on(&s)?;
    sd.release_on(&s)?;
    Ok((rotated, out))
}
