//! A plaintext matrix times an encrypted SIMD vector by the diagonal method: every column rotation of the ciphertext
//! from ONE digit decomposition (`HipKskSet::galois_hoisted_dev`), then the products with the diagonals and their sum in
//! one `dot_product_scalar_dev`.  The rotations are not the reference's words (include/fhe_hip.h); they decrypt to the
//! same plaintexts.  The last function runs the product for many clients at once, each under their own keys.
//! (No Rust toolchain exists in the build image: reviewed source, not compiled there.)
use std::sync::Arc;

use fhe_math_hip::{DeviceBuffer, DeviceCiphertexts, HipCtx, HipError, HipKsk, HipKskSet, Stream};

/// `galois_keys[r]` is the client's Galois key of element `exponents[r]` (3^(r + 1) mod 2N for the column rotations by
/// 1, 2, ...), `diagonals` the `poly_ntt` rows of the matrix's diagonals 1 ... R, `[R][L][N]`.  Returns, per ciphertext,
/// the sum over r of rotation r times diagonal r (diagonal 0 times the ciphertext itself is one `mul_plain_dev` more).
pub fn rotated_products(ctx: &Arc<HipCtx>, galois_keys: &[&HipKsk], exponents: &[usize], ct: &DeviceCiphertexts,
                        diagonals: &DeviceBuffer) -> Result<DeviceCiphertexts, HipError> {
    let s = Stream::new(ctx.device())?;
    let set = HipKskSet::new(galois_keys)?;                                   // built once per client, reused per query
    let rotations = set.galois_hoisted_dev(exponents, ct, &s)?;               // [batch][R] ciphertexts, one stage A
    let sum = ctx.dot_product_scalar_dev(exponents.len(), &rotations, diagonals, &s)?;
    rotations.release_on(&s)?;
    Ok(sum)
}

/// The same product in ONE call (`HipKskSet::matvec_hoisted_dev`): the rotations never reach memory, and `diagonal0`
/// (`[L][N]`) multiplies the ciphertext itself, so the whole matrix-vector product is the result.  `groups`: rotation
/// groups per launch for a host that has measured its shape (0 keeps the engine's rule).
pub fn matrix_times_vector(galois_keys: &[&HipKsk], exponents: &[usize], ct: &DeviceCiphertexts, diagonals: &DeviceBuffer,
                           diagonal0: &DeviceBuffer, groups: usize, s: &Stream) -> Result<DeviceCiphertexts, HipError> {
    let set = HipKskSet::new(galois_keys)?;
    if set.rot_split()? != groups {
        set.set_rot_split(groups)?;
    }
    set.matvec_hoisted_dev(exponents, ct, diagonals, Some(diagonal0), s)
}

/// The baby-step/giant-step form (`HipKskSet::matvec_bsgs_dev`): `baby_keys` rotate by 1 ... B - 1, `giant_keys` by B, 2B ...
/// (G - 1)B, and `grid` holds the `[G][B][L][N]` diagonals the caller has pre-rotated (`grid[g][b] = rot_{-gB}(d_{gB+b})`),
/// so `B + G - 2` keys serve `G * B` diagonals.  `tile`: giant groups per block of the baby stage for a host that has
/// measured its shape (0 keeps the engine's rule; 1, 2 or 4).
pub fn matrix_times_vector_bsgs(baby_keys: &[&HipKsk], baby_exps: &[usize], giant_keys: &[&HipKsk], giant_exps: &[usize],
                                ct: &DeviceCiphertexts, grid: &DeviceBuffer, tile: usize, s: &Stream)
                                -> Result<DeviceCiphertexts, HipError> {
    let baby = HipKskSet::new(baby_keys)?;
    let giant = HipKskSet::new(giant_keys)?;
    if baby.bsgs_tile()? != tile {
        baby.set_bsgs_tile(tile)?;
    }
    baby.matvec_bsgs_dev(baby_exps, &giant, giant_exps, ct, grid, s)
}

/// The same two calls for MANY CLIENTS at once, each under their own Galois keys (`HipKskSet::galois_hoisted_keyed_dev`,
/// `HipKskSet::matvec_hoisted_keyed_dev`): `client_keys[c][r]` is client c's key of element `exponents[r]`, `ct` holds
/// `ct.batch / clients` ciphertexts per client, client by client, and `diagonals` / `diagonal0` serve the whole batch.
/// The set is client-major; the results are those of one `matrix_times_vector` per client, word for word.
pub fn matrix_times_vectors_of_many_clients(client_keys: &[Vec<&HipKsk>], exponents: &[usize], ct: &DeviceCiphertexts,
                                            diagonals: &DeviceBuffer, diagonal0: &DeviceBuffer, keep_rotations: bool, s: &Stream)
                                            -> Result<(DeviceCiphertexts, Option<DeviceCiphertexts>), HipError> {
    let flat: Vec<&HipKsk> = client_keys.iter().flat_map(|keys| keys.iter().copied()).collect();
    let set = HipKskSet::new(&flat)?;                                         // built once per group of clients
    let clients = client_keys.len();
    let rotations = if keep_rotations { Some(set.galois_hoisted_keyed_dev(clients, exponents, ct, s)?) } else { None };
    let product = set.matvec_hoisted_keyed_dev(clients, exponents, ct, diagonals, Some(diagonal0), s)?;
    Ok((product, rotations))
}
