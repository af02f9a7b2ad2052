//! The two places where a SealPIR server (crates/fhe/examples/sealpir.rs) builds plaintexts from raw bits, without
//! leaving the device: the database preprocessing (`encode_database`, util.rs:97-145) from the database's own bytes,
//! and the fold of every query (sealpir.rs:176-200) from the first-dimension results as they lie in device memory after
//! the switch to the last level.  The client's way back (sealpir.rs:239-248) is the same transcoder the other way.
//! (No Rust toolchain exists in the build image: reviewed source, not compiled there.)
use std::sync::Arc;

use fhe_math_hip::{DeviceBuffer, HipError, HipParams, Stream};

/// `database`: the elements back to back, `per_plaintext` of them (`number_elements_per_plaintext`) of `element_size`
/// bytes per plaintext; `rows` = dim1 * dim2 plaintexts at `level`, the ones past the end of the database all zero.
pub fn preprocess_database(params: &Arc<HipParams>, database: &[u8], element_size: usize, per_plaintext: usize,
                           plaintext_nbits: usize, rows: usize, level: usize) -> Result<DeviceBuffer, HipError> {
    let s = Stream::new(fhe_math_hip::default_device())?;
    let enc = params.encoder(None)?;
    let ctx = params.context_at_level(level)?;
    let bytes = DeviceBuffer::upload_bytes(ctx.device(), database, &s)?;
    let pts = enc.encode_bytes_dev(false, level, &bytes, database.len(), per_plaintext * element_size, plaintext_nbits, rows, &s)?;
    bytes.release_on(&s)?;
    s.synchronize()?;
    Ok(pts)   // [rows][L_level][N] poly_ntt: the operand of dot_product_scalar
}

/// `switched`: the dim2 first-dimension results at the last level, `[dim2][2][N]` words below q_0 (`q0_bits` bits).
/// Returns the fold `[dim2][nplain][L_level][N]` with nplain, and -- what a client does with the decrypted values of
/// one of them -- the words of that ciphertext again, `[2][M' >= N]`.
pub fn fold(params: &Arc<HipParams>, switched: &DeviceBuffer, q0_bits: usize, plaintext_nbits: usize, level: usize)
            -> Result<(DeviceBuffer, usize, Vec<u64>), HipError> {
    let s = Stream::new(fhe_math_hip::default_device())?;
    let enc = params.encoder(None)?;
    let ctx = params.context_at_level(level)?;
    let n = ctx.degree();
    let (pts, nplain) = enc.encode_words_dev(false, level, switched, q0_bits, 2, n, plaintext_nbits, &s)?;
    // the values themselves, per segment, and back: transcode(transcode(c, q0_bits, nbits), nbits, q0_bits)[..N] == c
    let values = fhe_math_hip::transcode_dev(ctx.device(), switched, q0_bits, n, plaintext_nbits, &s)?;
    let per_segment = values.len() / (switched.len() / n);
    let words = fhe_math_hip::transcode_dev(ctx.device(), &values, plaintext_nbits, per_segment, q0_bits, &s)?;
    let mut back = vec![0u64; words.len()];
    words.download(&mut back, &s)?;
    values.release_on(&s)?;
    words.release_on(&s)?;
    Ok((pts, nplain, back))
}
