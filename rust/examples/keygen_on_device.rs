//! A client that makes its evaluation keys on the GPU: a secret key drawn on the device, then its relinearization key,
//! the Galois keys of a PIR query expansion and a generic key-switching key, all generated from the device-resident
//! secret -- the secret never leaves the device, and what goes to the server is each key's exported arrays.
//! (No Rust toolchain exists in the build image: reviewed source, not compiled there.)
use std::sync::Arc;

use fhe_math_hip::{DeviceBuffer, DeviceSeeds, HipCtx, HipError, HipKsk, Stream};

/// The keys a PIR client sends: one relinearization key and the Galois keys (N >> l) + 1, l < `levels`, each as
/// (c0, c1) downloaded from the device, plus the keys' public seeds.  `ctx` is the level-0 context; the 32-byte seeds
/// come from the caller's CSPRNG (`seeds[0]`: the secret key's, then one per key, then the second secret's).
pub fn pir_client_keys(ctx: &Arc<HipCtx>, variance: usize, levels: usize, seeds: &[[u8; 32]])
                       -> Result<Vec<(Vec<u64>, Vec<u64>)>, HipError> {
    let s = Stream::new(ctx.device())?;
    let n = ctx.degree();
    let sk_seed = DeviceSeeds::upload(ctx.device(), &seeds[0..1], &s)?;
    let s_ntt = ctx.sample_small_dev(variance, &sk_seed, true, &s)?;                  // SecretKey::random
    let rk_seed = DeviceSeeds::upload(ctx.device(), &seeds[1..2], &s)?;
    let (rk, rk_k) = HipKsk::generate_relin(ctx, ctx, variance, &s_ntt, &rk_seed, &s)?;
    let exps: Vec<usize> = (0..levels).map(|l| (n >> l) + 1).collect();
    let gk_seeds = DeviceSeeds::upload(ctx.device(), &seeds[2..2 + levels], &s)?;
    let (gks, gk_k) = HipKsk::generate_galois(ctx, ctx, variance, &s_ntt, &exps, &gk_seeds, &s)?;
    // a generic key: switching from a second secret s' (drawn on the device) to s -- what a key rotation hands out
    let other_seed = DeviceSeeds::upload(ctx.device(), &seeds[3 + levels..4 + levels], &s)?;
    let from: DeviceBuffer = ctx.sample_small_dev(variance, &other_seed, true, &s)?;
    let id_seed = DeviceSeeds::upload(ctx.device(), &seeds[2 + levels..3 + levels], &s)?;
    let (ids, id_k) = HipKsk::generate(ctx, ctx, variance, &s_ntt, &from, &id_seed, &s)?;
    let mut out = Vec::new();
    let mut keys = vec![&rk];
    for k in gks.iter() {
        keys.push(k);
    }
    for k in ids.iter() {
        keys.push(k);
    }
    for k in keys {
        let [c0, c1, c0s, c1s] = k.export_dev(&s)?;
        assert_eq!(c0.len(), k.ndigits() * n * ctx.nmoduli());
        let mut h0 = vec![0u64; c0.len()];
        let mut h1 = vec![0u64; c1.len()];
        c0.download(&mut h0, &s)?;
        c1.download(&mut h1, &s)?;
        out.push((h0, h1));
        for b in [c0, c1, c0s, c1s] {
            b.release_on(&s)?;
        }
    }
    // the two secrets are the caller's to clear
    s_ntt.upload(&vec![0u64; s_ntt.len()], &s)?;
    from.upload(&vec![0u64; from.len()], &s)?;
    for b in [s_ntt, from] {
        b.release_on(&s)?;
    }
    for sd in [sk_seed, rk_seed, gk_seeds, id_seed, other_seed, rk_k, gk_k, id_k] {
        sd.release_on(&s)?;
    }
    Ok(out)
}
