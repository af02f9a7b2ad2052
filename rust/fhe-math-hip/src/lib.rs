//! Safe handles over the C ABI of the MI355X engine (`include/fhe_hip.h`, `libfhe_hip.so`).
//!
//! One RAII type per opaque C handle, named after the reference type it shadows:
//!
//! | here               | C handle / object        | reference type (fhe.rs)                                   |
//! |--------------------|--------------------------|-----------------------------------------------------------|
//! | [`HipCtx`]         | `fhe_ctx`                | `fhe_math::rq::Context`            (rq/context.rs:9-19)    |
//! | [`HipScaler`]      | `fhe_scaler`             | `fhe_math::rq::scaler::Scaler`     (rq/scaler.rs:18-23)    |
//! | [`HipKsk`]         | `fhe_ksk`                | `fhe::bfv::KeySwitchingKey`        (keys/key_switching_key.rs:22-46) |
//! | [`HipKskSet`]      | `fhe_kskset`             | the `KeySwitchingKey`s of many clients for one operation (keyed batches) |
//! | [`HipMul`]         | `fhe_mul`                | `fhe::bfv::Multiplicator`          (ops/mul.rs:21-32)      |
//! | [`HipParams`]      | `fhe_params`             | level tables of `BfvParameters`    (parameters.rs:83-117)  |
//! | [`HipEncoder`]     | `fhe_encoder`            | encoding tables of `BfvParameters` (parameters.rs:598, 711-725) |
//! | [`DeviceSeeds`]    | `[batch][32]` bytes      | the seeds of `Poly::small` / `random_from_seed` (encryption)   |
//! | [`Stream`]         | `hipStream_t` (ABI-made) | --                                                         |
//! | [`DeviceBuffer`]   | `fhe_buf_alloc` memory   | the device shadow of `Poly.coefficients: Array2<u64>`      |
//! | [`DeviceCiphertexts`] | a `DeviceBuffer` + shape | a batch of `bfv::Ciphertext` kept on the GPU between calls |
//!
//! Two ways to call the engine:
//! * **host slices** -- `Poly`'s own `[L][N]` row-major `u64` slices (`coefficients.as_slice()`), batches are
//!   concatenations; synchronous, H2D + compute + D2H inside every call (the drop-in path of the call-site patches);
//! * **device resident** -- [`DeviceCiphertexts`] on a [`Stream`]: upload once, chain `multiply` -> `relinearize` ->
//!   `rotate` -> `switch_to_level` without leaving the GPU, download lazily.  This is the path the throughput numbers
//!   are quoted on.
//!
//! Safety contract of the safe API: every slice length is checked against the handle's own geometry before the
//! call (the C side trusts `batch`); borrowed level contexts carry a lifetime ([`CtxView`]); handles that the C side
//! keeps pointers to (`fhe_scaler` -> its two contexts, `fhe_ksk` -> its two contexts, `fhe_mul` -> scalers and key)
//! are kept alive by `Arc`s inside the dependent wrapper.  Handles are immutable after creation: `Send + Sync`.
//! `ffi.rs` is generated from the header (`tools/gen_rust_ffi.py`); `tests/test_rust_shim.py` keeps the two equal and
//! checks that every identifier the call-site patches use is defined here or by another patch.
//! (No Rust toolchain exists in the build image: this crate is reviewed source, not compiled there.)
pub mod ffi;

use std::ffi::CStr;
use std::marker::PhantomData;
use std::ops::Deref;
use std::os::raw::{c_int, c_void};
use std::ptr;
use std::sync::{Arc, OnceLock};

/// Non-zero `fhe_status` with the engine's thread-local message.  The codes map 1:1 onto the `Result` variants
/// of the path (table in `fhe_hip.h`); `fhe-math` / `fhe` translate them back (`hip_error` in each crate,
/// rust/patches/10-*.patch and 13-*.patch).
#[derive(Debug, Clone, PartialEq, Eq)]
pub struct HipError {
    pub status: i32,
    pub message: String,
}
impl std::fmt::Display for HipError {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "fhe_hip status {}: {}", self.status, self.message)
    }
}
impl std::error::Error for HipError {}
pub type Result<T> = std::result::Result<T, HipError>;

pub mod status {
    pub const ARG: i32 = -1;
    pub const HIP: i32 = -2;
    pub const INVALID_MODULUS: i32 = -3;
    pub const INVALID_DEGREE: i32 = -4;
    pub const NTT_UNAVAILABLE: i32 = -5;
    pub const CONTEXT_MISMATCH: i32 = -6;
    pub const DEGREE_MISMATCH: i32 = -7;
    pub const NO_MORE_CONTEXT: i32 = -8;
    pub const CONTEXT_NOT_REACHABLE: i32 = -9;
    pub const INVALID_SUBSTITUTION_EXPONENT: i32 = -10;
    pub const PARAMETER_MISMATCH: i32 = -11;
    pub const INVALID_LEVEL: i32 = -12;
    pub const MUL_POLY_COUNT: i32 = -13;
    pub const EMPTY_MODULI: i32 = -14;
    pub const NON_COPRIME: i32 = -15;
    pub const NOT_ENOUGH_PRIMES: i32 = -16;
    pub const KEYSWITCH_UNSUPPORTED: i32 = -17;
    pub const NO_DEVICE: i32 = -18;
    pub const EMPTY_DOT_PRODUCT: i32 = -19;
    pub const INVALID_EXPANSION_SIZE: i32 = -20;
    pub const EXPANSION_UNSUPPORTED: i32 = -21;
    pub const SIMD_UNAVAILABLE: i32 = -22;
    pub const TOO_MANY_VALUES: i32 = -23;
    pub const INVALID_VARIANCE: i32 = -24;
}

pub fn check(status: ffi::FheStatus) -> Result<()> {
    if status == 0 {
        return Ok(());
    }
    let message = unsafe { CStr::from_ptr(ffi::fhe_last_error()) }.to_string_lossy().into_owned();
    Err(HipError { status, message })
}
/// A shape the caller got wrong on the Rust side (never reaches the C ABI).
fn shape_error(what: &str) -> HipError {
    HipError { status: status::ARG, message: format!("fhe-math-hip: {what}") }
}
fn expect_len(what: &str, got: usize, want: usize) -> Result<()> {
    if got == want { Ok(()) } else { Err(shape_error(&format!("{what}: {got} u64 words, expected {want}"))) }
}
/// `len / per` when `len` is a whole number of `per`-word items.
fn whole_batch(what: &str, len: usize, per: usize) -> Result<usize> {
    if per == 0 || len % per != 0 {
        return Err(shape_error(&format!("{what}: {len} u64 words is not a whole number of {per}-word items")));
    }
    Ok(len / per)
}
/// Checks a plaintext operand against a device-resident batch over `ctx`: true when one `[rows][N]` plaintext is
/// shared by the batch, false for one per ciphertext.
fn plain_operand(what: &str, ctx: &CtxView<'_>, ct: &DeviceCiphertexts, pt: &DeviceBuffer) -> Result<bool> {
    if ct.rows != ctx.nmoduli() || ct.degree != ctx.degree() {
        return Err(shape_error(&format!("{what}: the ciphertexts are not over this context")));
    }
    let pw = ct.rows * ct.degree;
    if pt.len() == pw {
        return Ok(true);
    }
    expect_len(what, pt.len(), ct.batch * pw)?;
    Ok(false)
}
/// The device the patched crates put their handles on: `FHE_HIP_DEVICE` (one process per GPU when a batch is
/// sharded across the GPUs of a node), default 0.
pub fn default_device() -> i32 {
    std::env::var("FHE_HIP_DEVICE").ok().and_then(|s| s.parse().ok()).unwrap_or(0)
}

thread_local! {
    /// Depth of `with_native` scopes on this thread (see `enabled`).
    static FORCE_NATIVE: std::cell::Cell<u32> = const { std::cell::Cell::new(0) };
}

/// Runs `f` with the patched crates on their NATIVE (CPU) path on the calling thread, whatever the process-wide
/// switch says, and restores the previous state afterwards (also when `f` panics).  This is what lets ONE test
/// process compute a value twice -- once through fhe.rs's own code, once through the engine -- and compare the two
/// bit for bit (`crates/*/tests/hip_parity.rs`, patches 17 / 18): the only way psi, the seeded sampler and every
/// composite operation can be pinned against the reference itself.  Nests; affects this thread only.
pub fn with_native<R>(f: impl FnOnce() -> R) -> R {
    struct Restore;
    impl Drop for Restore {
        fn drop(&mut self) { FORCE_NATIVE.with(|c| c.set(c.get() - 1)); }
    }
    FORCE_NATIVE.with(|c| c.set(c.get() + 1));
    let _restore = Restore;
    f()
}

/// Is the calling thread inside a `with_native` scope?
pub fn native_forced() -> bool { FORCE_NATIVE.with(|c| c.get() > 0) }

/// Whether the patched crates forward to the engine at all: the `hip` cargo feature compiles the forwarding in, this
/// decides at run time.  False when `FHE_HIP_DISABLE` is set or no HIP device is visible (both read once per process),
/// so a binary built with the feature still runs -- on the native CPU path -- on a machine without a GPU; and false
/// inside `with_native` on the calling thread.
pub fn enabled() -> bool {
    static ON: OnceLock<bool> = OnceLock::new();
    !native_forced() && *ON.get_or_init(|| std::env::var_os("FHE_HIP_DISABLE").is_none() && unsafe { ffi::fhe_device_count() } > 0)
}

/// Execution option of the engine (`fhe_engine_set_f64`): rows whose moduli are all below 2^50 -- every modulus of
/// `BfvParameters::default_parameters_128` -- run on the FP64-FMA kernels (default) or on the integer kernels.  Results are
/// bit-identical either way; the parity tests run both.
pub fn set_f64_kernels(on: bool) { unsafe { ffi::fhe_engine_set_f64(on as std::os::raw::c_int) } }
pub fn f64_kernels() -> bool { unsafe { ffi::fhe_engine_get_f64() != 0 } }

/// The six tables of one `NttOperator` per modulus (ntt/native.rs:16-26), flattened `[nmoduli][degree]`.
/// The host passes its own so that psi -- drawn from ChaCha8 in the reference -- is the same on both sides.
pub struct NttTables<'a> {
    pub omegas: &'a [u64],
    pub omegas_shoup: &'a [u64],
    pub zetas_inv: &'a [u64],
    pub zetas_inv_shoup: &'a [u64],
    pub size_inv: &'a [u64],
    pub size_inv_shoup: &'a [u64],
}

/// How the reference's structs carry a device twin: `Context`, `Scaler`, `KeySwitchingKey`, `Multiplicator` derive
/// `Clone + PartialEq + Eq` (some `Default`), and a device handle must not take part in equality (two equal contexts
/// are equal whichever device object backs them).  The twin is built on FIRST USE (`get_or_try_init`), so
/// constructors and deserialisers only add `hip: Default::default()`, objects that never compute never touch the GPU,
/// and a clone made after the first use shares the same device object.
pub struct LazyHandle<T>(OnceLock<Arc<T>>);
impl<T> LazyHandle<T> {
    pub fn get(&self) -> Option<&Arc<T>> { self.0.get() }
    /// The device twin, built by `init` the first time (concurrent first users may both build; one result is kept).
    pub fn get_or_try_init<E>(&self, init: impl FnOnce() -> std::result::Result<T, E>) -> std::result::Result<&Arc<T>, E> {
        if let Some(v) = self.0.get() {
            return Ok(v);
        }
        let built = Arc::new(init()?);
        Ok(self.0.get_or_init(|| built))
    }
    /// Forgets the twin (the owner changed something the twin was built from); the next use rebuilds it.
    pub fn reset(&mut self) { self.0 = OnceLock::new(); }
}
impl<T> Default for LazyHandle<T> {
    fn default() -> Self { Self(OnceLock::new()) }
}
impl<T> Clone for LazyHandle<T> {
    fn clone(&self) -> Self {
        let c = OnceLock::new();
        if let Some(v) = self.0.get() {
            let _ = c.set(v.clone());
        }
        Self(c)
    }
}
impl<T> PartialEq for LazyHandle<T> {
    fn eq(&self, _: &Self) -> bool { true }
}
impl<T> Eq for LazyHandle<T> {}
impl<T> std::fmt::Debug for LazyHandle<T> {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        f.write_str(if self.0.get().is_some() { "LazyHandle(device)" } else { "LazyHandle(unset)" })
    }
}

// ------------------------------------------------------------------------------------------ rq::Context
/// A context handle that does not own the C object: either the view inside a [`HipCtx`] or a level handle borrowed
/// from one (`'a` ties it to its root, which frees the whole chain).  Deliberately not `Clone`.
pub struct CtxView<'a> {
    ptr: *const ffi::FheCtx,
    _root: PhantomData<&'a ()>,
}
unsafe impl Send for CtxView<'_> {}
unsafe impl Sync for CtxView<'_> {}
impl CtxView<'_> {
    pub fn as_ptr(&self) -> *const ffi::FheCtx { self.ptr }
    pub fn degree(&self) -> usize { unsafe { ffi::fhe_ctx_degree(self.ptr) } }
    pub fn nmoduli(&self) -> usize { unsafe { ffi::fhe_ctx_nmoduli(self.ptr) } }
    pub fn device(&self) -> i32 { unsafe { ffi::fhe_ctx_device(self.ptr) as i32 } }
    /// u64 words of one polynomial, `L * N`.
    pub fn poly_words(&self) -> usize { self.nmoduli() * self.degree() }
    /// Bytes of one polynomial's `coefficients` payload on the wire (`fhe_poly_serialized_size`).
    pub fn serialized_size(&self) -> usize { unsafe { ffi::fhe_poly_serialized_size(self.ptr) } }
    /// `Poly::ntt_forward` (rq/mod.rs:335-343) on `polys.len() / (L*N)` polynomials, in place.
    pub fn ntt_forward(&self, polys: &mut [u64]) -> Result<()> {
        let b = whole_batch("ntt_forward", polys.len(), self.poly_words())?;
        check(unsafe { ffi::fhe_ntt_forward(self.ptr, polys.as_mut_ptr(), b) })
    }
    /// `Poly::ntt_backward` (rq/mod.rs:346-354).
    pub fn ntt_backward(&self, polys: &mut [u64]) -> Result<()> {
        let b = whole_batch("ntt_backward", polys.len(), self.poly_words())?;
        check(unsafe { ffi::fhe_ntt_backward(self.ptr, polys.as_mut_ptr(), b) })
    }
    /// `AddAssign` / `SubAssign` / `MulAssign<&Poly<Ntt>>` (rq/ops.rs:10-206): `a op= b`.
    pub fn add_assign(&self, a: &mut [u64], b: &[u64]) -> Result<()> {
        expect_len("add_assign rhs", b.len(), a.len())?;
        let n = whole_batch("add_assign", a.len(), self.poly_words())?;
        check(unsafe { ffi::fhe_poly_add(self.ptr, a.as_mut_ptr(), b.as_ptr(), n) })
    }
    pub fn sub_assign(&self, a: &mut [u64], b: &[u64]) -> Result<()> {
        expect_len("sub_assign rhs", b.len(), a.len())?;
        let n = whole_batch("sub_assign", a.len(), self.poly_words())?;
        check(unsafe { ffi::fhe_poly_sub(self.ptr, a.as_mut_ptr(), b.as_ptr(), n) })
    }
    pub fn mul_assign(&self, a: &mut [u64], b: &[u64]) -> Result<()> {
        expect_len("mul_assign rhs", b.len(), a.len())?;
        let n = whole_batch("mul_assign", a.len(), self.poly_words())?;
        check(unsafe { ffi::fhe_poly_mul(self.ptr, a.as_mut_ptr(), b.as_ptr(), n) })
    }
    /// `MulAssign<&Poly<NttShoup>>` (rq/ops.rs:208-245).
    pub fn mul_shoup_assign(&self, a: &mut [u64], b: &[u64], b_shoup: &[u64]) -> Result<()> {
        expect_len("mul_shoup_assign rhs", b.len(), a.len())?;
        expect_len("mul_shoup_assign rhs twins", b_shoup.len(), a.len())?;
        let n = whole_batch("mul_shoup_assign", a.len(), self.poly_words())?;
        check(unsafe { ffi::fhe_poly_mul_shoup(self.ptr, a.as_mut_ptr(), b.as_ptr(), b_shoup.as_ptr(), n) })
    }
    pub fn neg_assign(&self, a: &mut [u64]) -> Result<()> {
        let n = whole_batch("neg_assign", a.len(), self.poly_words())?;
        check(unsafe { ffi::fhe_poly_neg(self.ptr, a.as_mut_ptr(), n) })
    }
    /// `Poly::substitute` (rq/mod.rs:360-412); `exponent` as in `SubstitutionExponent::new`.
    pub fn substitute(&self, exponent: usize, input: &[u64], out: &mut [u64], repr_is_ntt: bool) -> Result<()> {
        expect_len("substitute output", out.len(), input.len())?;
        let n = whole_batch("substitute", input.len(), self.poly_words())?;
        check(unsafe {
            ffi::fhe_poly_substitute(self.ptr, exponent, input.as_ptr(), out.as_mut_ptr(), n, repr_is_ntt as c_int)
        })
    }
    /// `Poly::<PowerBasis>::switch_down` (rq/mod.rs:433-492): `[batch][L][N]` -> `[batch][L-1][N]`.
    pub fn switch_down(&self, input: &[u64], out: &mut [u64]) -> Result<()> {
        let b = whole_batch("switch_down", input.len(), self.poly_words())?;
        expect_len("switch_down output", out.len(), b * (self.nmoduli().saturating_sub(1)) * self.degree())?;
        check(unsafe { ffi::fhe_poly_switch_down(self.ptr, input.as_ptr(), out.as_mut_ptr(), b) })
    }
    /// `Poly::<PowerBasis>::switch_down_to` (rq/mod.rs:498-507) in one call: `[batch][L][N]` -> `[batch][to.L][N]`.
    pub fn switch_down_to(&self, to: &CtxView<'_>, input: &[u64], out: &mut [u64]) -> Result<()> {
        let b = whole_batch("switch_down_to", input.len(), self.poly_words())?;
        expect_len("switch_down_to output", out.len(), b * to.poly_words())?;
        check(unsafe { ffi::fhe_poly_switch_down_to(self.ptr, to.ptr, input.as_ptr(), out.as_mut_ptr(), b) })
    }
    /// `Ciphertext::switch_down` (bfv/ciphertext.rs:148-161) on `nparts`-part ciphertexts in Ntt form.
    pub fn ciphertext_switch_down(&self, nparts: usize, ct: &[u64], out: &mut [u64]) -> Result<()> {
        self.ciphertext_switch_to_level(1, nparts, ct, out)
    }
    /// `Ciphertext::switch_to_level` (bfv/ciphertext.rs:164-183), `levels` = target level - current level.
    pub fn ciphertext_switch_to_level(&self, levels: usize, nparts: usize, ct: &[u64], out: &mut [u64]) -> Result<()> {
        if nparts == 0 || levels >= self.nmoduli() {
            return Err(shape_error("switch_to_level: no parts, or more levels than the context chain has"));
        }
        let b = whole_batch("switch_to_level", ct.len(), nparts * self.poly_words())?;
        expect_len("switch_to_level output", out.len(), b * nparts * (self.nmoduli() - levels) * self.degree())?;
        check(unsafe { ffi::fhe_bfv_switch_to_level(self.ptr, levels, nparts, ct.as_ptr(), out.as_mut_ptr(), b) })
    }
    /// The same on a device-resident batch (`fhe_bfv_switch_to_level_dev`), stream-ordered.
    pub fn ciphertexts_switch_to_level_dev(&self, levels: usize, ct: &DeviceCiphertexts, stream: &Stream) -> Result<DeviceCiphertexts> {
        if ct.rows != self.nmoduli() || ct.degree != self.degree() || levels >= ct.rows {
            return Err(shape_error("switch_to_level_dev: ciphertexts do not live over this context"));
        }
        let out = DeviceCiphertexts::alloc_on(self.device(), ct.batch, ct.parts, ct.rows - levels, ct.degree, ct.level + levels, stream)?;
        check(unsafe {
            ffi::fhe_bfv_switch_to_level_dev(self.ptr, levels, ct.parts, ct.buf.as_ptr(), out.buf.as_mut_ptr(), ct.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
    /// `&Ciphertext * &Plaintext` (ops/mod.rs:229-257) on a device-resident batch: every part times `pt`, the
    /// plaintext's `poly_ntt` (`[rows][N]` shared by the batch, or `[batch][rows][N]`) -- `fhe_bfv_mul_plain_dev`.
    pub fn mul_plain_dev(&self, ct: &DeviceCiphertexts, pt: &DeviceBuffer, stream: &Stream) -> Result<DeviceCiphertexts> {
        let shared = plain_operand("mul_plain_dev", self, ct, pt)?;
        let out = DeviceCiphertexts::alloc_on(self.device(), ct.batch, ct.parts, ct.rows, ct.degree, ct.level, stream)?;
        check(unsafe {
            ffi::fhe_bfv_mul_plain_dev(self.ptr, ct.parts, ct.buf.as_ptr(), pt.as_ptr(), shared as c_int, out.buf.as_mut_ptr(),
                                       ct.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
    /// `bfv::dot_product_scalar` (ops/dot_product.rs:54-180) on device-resident operands (`fhe_bfv_dot_product_scalar_dev`):
    /// `cts` holds `count` ciphertexts per item (`cts.batch` a multiple of `count`: the layout `galois_hoisted_dev` writes),
    /// `pts` the `count` `poly_ntt` rows every item shares -> one ciphertext per item.
    pub fn dot_product_scalar_dev(&self, count: usize, cts: &DeviceCiphertexts, pts: &DeviceBuffer, stream: &Stream) -> Result<DeviceCiphertexts> {
        if count == 0 {
            return Err(HipError { status: status::EMPTY_DOT_PRODUCT, message: "dot_product_scalar_dev: no operands".into() });
        }
        if cts.rows != self.nmoduli() || cts.degree != self.degree() {
            return Err(shape_error("dot_product_scalar_dev: the ciphertexts do not live over this context"));
        }
        let items = whole_batch("dot_product_scalar_dev ciphertexts", cts.batch, count)?;
        expect_len("dot_product_scalar_dev plaintexts", pts.len(), count * self.poly_words())?;
        let out = DeviceCiphertexts::alloc_on(self.device(), items, cts.parts, cts.rows, cts.degree, cts.level, stream)?;
        check(unsafe {
            ffi::fhe_bfv_dot_product_scalar_dev(self.ptr, cts.parts, count, cts.buf.as_ptr(), 0, pts.as_ptr(), 1, out.buf.as_mut_ptr(),
                                                items, stream.as_ptr())
        })?;
        Ok(out)
    }
}

pub struct HipCtx {
    view: CtxView<'static>, // (never handed out with the 'static lifetime: only through `Deref`, i.e. bounded by `&self`)
}
impl HipCtx {
    /// `Context::new` (rq/context.rs:42-92) on `device` (-1: host-only handle).
    pub fn new(device: i32, degree: usize, moduli: &[u64], tables: Option<&NttTables<'_>>) -> Result<Self> {
        let mut out: *mut ffi::FheCtx = ptr::null_mut();
        // (all six table pointers, or all NULL: the engine then derives its own primitive roots)
        let null = ptr::null::<u64>();
        let (om, oms, zi, zis, si, sis) = match tables {
            Some(t) => (t.omegas.as_ptr(), t.omegas_shoup.as_ptr(), t.zetas_inv.as_ptr(), t.zetas_inv_shoup.as_ptr(),
                        t.size_inv.as_ptr(), t.size_inv_shoup.as_ptr()),
            None => (null, null, null, null, null, null),
        };
        if let Some(t) = tables {
            let full = moduli.len() * degree;
            expect_len("NttTables.omegas", t.omegas.len(), full)?;
            expect_len("NttTables.omegas_shoup", t.omegas_shoup.len(), full)?;
            expect_len("NttTables.zetas_inv", t.zetas_inv.len(), full)?;
            expect_len("NttTables.zetas_inv_shoup", t.zetas_inv_shoup.len(), full)?;
            expect_len("NttTables.size_inv", t.size_inv.len(), moduli.len())?;
            expect_len("NttTables.size_inv_shoup", t.size_inv_shoup.len(), moduli.len())?;
        }
        check(unsafe {
            ffi::fhe_ctx_create(device as c_int, degree, moduli.len(), moduli.as_ptr(), om, oms, zi, zis, si, sis, &mut out)
        })?;
        Ok(Self { view: CtxView { ptr: out, _root: PhantomData } })
    }
    /// `Context::context_at_level`: a handle that lives as long as `self` (the root frees the chain).
    pub fn at_level(&self, level: usize) -> Result<CtxView<'_>> {
        let mut out: *const ffi::FheCtx = ptr::null();
        check(unsafe { ffi::fhe_ctx_at_level(self.view.ptr, level, &mut out) })?;
        Ok(CtxView { ptr: out, _root: PhantomData })
    }
}
impl Deref for HipCtx {
    type Target = CtxView<'static>;
    fn deref(&self) -> &CtxView<'static> { &self.view }
}
impl Drop for HipCtx {
    fn drop(&mut self) { unsafe { ffi::fhe_ctx_destroy(self.view.ptr as *mut ffi::FheCtx) } }
}

// ------------------------------------------------------------------------------------------ rq::Scaler
/// Every field of `RnsScaler` (rns/scaler.rs:52-72), `omega*` flattened `[to][from]`.
pub struct RnsScalerConstants<'a> {
    pub gamma: &'a [u64],
    pub gamma_shoup: &'a [u64],
    pub omega: &'a [u64],
    pub omega_shoup: &'a [u64],
    pub theta_gamma_lo: u64,
    pub theta_gamma_hi: u64,
    pub theta_gamma_sign: bool,
    pub theta_omega_lo: &'a [u64],
    pub theta_omega_hi: &'a [u64],
    pub theta_omega_sign: &'a [u8],
    pub theta_garner_lo: &'a [u64],
    pub theta_garner_hi: &'a [u64],
    pub theta_garner_shift: usize,
}
/// The same, owned (what `RnsScaler::hip_constants` of rust/patches/11-*.patch returns), plus `is_one`.
pub struct RnsScalerConstantsBuf {
    pub is_one: bool,
    pub gamma: Vec<u64>,
    pub gamma_shoup: Vec<u64>,
    pub omega: Vec<u64>,
    pub omega_shoup: Vec<u64>,
    pub theta_gamma_lo: u64,
    pub theta_gamma_hi: u64,
    pub theta_gamma_sign: bool,
    pub theta_omega_lo: Vec<u64>,
    pub theta_omega_hi: Vec<u64>,
    pub theta_omega_sign: Vec<u8>,
    pub theta_garner_lo: Vec<u64>,
    pub theta_garner_hi: Vec<u64>,
    pub theta_garner_shift: usize,
}
impl RnsScalerConstantsBuf {
    pub fn view(&self) -> RnsScalerConstants<'_> {
        RnsScalerConstants {
            gamma: &self.gamma, gamma_shoup: &self.gamma_shoup, omega: &self.omega, omega_shoup: &self.omega_shoup,
            theta_gamma_lo: self.theta_gamma_lo, theta_gamma_hi: self.theta_gamma_hi, theta_gamma_sign: self.theta_gamma_sign,
            theta_omega_lo: &self.theta_omega_lo, theta_omega_hi: &self.theta_omega_hi, theta_omega_sign: &self.theta_omega_sign,
            theta_garner_lo: &self.theta_garner_lo, theta_garner_hi: &self.theta_garner_hi,
            theta_garner_shift: self.theta_garner_shift,
        }
    }
}
pub struct HipScaler {
    ptr: *mut ffi::FheScaler,
    from: Arc<HipCtx>, // the C object points at both contexts
    to: Arc<HipCtx>,
}
unsafe impl Send for HipScaler {}
unsafe impl Sync for HipScaler {}
impl HipScaler {
    /// `Scaler::new` (rq/scaler.rs:27-52) with the constants the host's `RnsScaler::new` already computed.
    pub fn from_constants(from: &Arc<HipCtx>, to: &Arc<HipCtx>, number_common_moduli: usize, is_one: bool,
                          k: &RnsScalerConstants<'_>) -> Result<Self> {
        let (nf, nt) = (from.nmoduli(), to.nmoduli());
        expect_len("gamma", k.gamma.len(), nt)?;
        expect_len("gamma_shoup", k.gamma_shoup.len(), nt)?;
        expect_len("omega", k.omega.len(), nt * nf)?;
        expect_len("omega_shoup", k.omega_shoup.len(), nt * nf)?;
        expect_len("theta_omega_lo", k.theta_omega_lo.len(), nf)?;
        expect_len("theta_omega_hi", k.theta_omega_hi.len(), nf)?;
        expect_len("theta_omega_sign", k.theta_omega_sign.len(), nf)?;
        expect_len("theta_garner_lo", k.theta_garner_lo.len(), nf)?;
        expect_len("theta_garner_hi", k.theta_garner_hi.len(), nf)?;
        let mut out: *mut ffi::FheScaler = ptr::null_mut();
        check(unsafe {
            ffi::fhe_scaler_create_from_constants(from.as_ptr(), to.as_ptr(), number_common_moduli, is_one as c_int,
                k.gamma.as_ptr(), k.gamma_shoup.as_ptr(), k.omega.as_ptr(), k.omega_shoup.as_ptr(), k.theta_gamma_lo,
                k.theta_gamma_hi, k.theta_gamma_sign as c_int, k.theta_omega_lo.as_ptr(), k.theta_omega_hi.as_ptr(),
                k.theta_omega_sign.as_ptr(), k.theta_garner_lo.as_ptr(), k.theta_garner_hi.as_ptr(),
                k.theta_garner_shift, &mut out)
        })?;
        Ok(Self { ptr: out, from: from.clone(), to: to.clone() })
    }
    pub fn as_ptr(&self) -> *const ffi::FheScaler { self.ptr }
    pub fn from_ctx(&self) -> &Arc<HipCtx> { &self.from }
    pub fn to_ctx(&self) -> &Arc<HipCtx> { &self.to }
    /// `SecretKey::try_decrypt` (keys/secret_key.rs:198-247) on a device-resident batch with this cipher-to-plaintext
    /// scaler (`CipherPlainContext::scaler`): `s_ntt` `[from.L][N]` -> the plaintexts' coefficients mod t, `[batch][N]`
    /// (`fhe_bfv_decrypt_dev`; clearing `s_ntt` and the result is the caller's job).
    pub fn decrypt_dev(&self, plaintext_modulus: u64, s_ntt: &DeviceBuffer, ct: &DeviceCiphertexts, stream: &Stream) -> Result<DeviceBuffer> {
        expect_len("decrypt_dev secret key", s_ntt.len(), self.from.poly_words())?;
        if ct.rows != self.from.nmoduli() || ct.degree != self.from.degree() {
            return Err(shape_error("decrypt_dev: the ciphertexts are not over the scaler's source context"));
        }
        let out = DeviceBuffer::alloc_on(self.from.device(), ct.batch * ct.degree, stream)?;
        check(unsafe {
            ffi::fhe_bfv_decrypt_dev(self.ptr, plaintext_modulus, s_ntt.as_ptr(), ct.buf.as_ptr(), ct.parts, out.as_mut_ptr(),
                                     ct.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
    /// `Scaler::scale` (rq/scaler.rs:55-127): `[batch][from.L][N]` -> `[batch][to.L][N]`.
    pub fn scale(&self, input: &[u64], out: &mut [u64], repr_is_ntt: bool) -> Result<()> {
        let b = whole_batch("scale", input.len(), self.from.poly_words())?;
        expect_len("scale output", out.len(), b * self.to.poly_words())?;
        check(unsafe { ffi::fhe_poly_scale(self.ptr, input.as_ptr(), out.as_mut_ptr(), b, repr_is_ntt as c_int) })
    }
}
impl Drop for HipScaler {
    fn drop(&mut self) { unsafe { ffi::fhe_scaler_destroy(self.ptr) } }
}

// ------------------------------------------------------------------------------------- KeySwitchingKey
pub struct HipKsk {
    ptr: *mut ffi::FheKsk,
    ct_ctx: Arc<HipCtx>, // the C object points at both contexts
    ksk_ctx: Arc<HipCtx>,
}
unsafe impl Send for HipKsk {}
unsafe impl Sync for HipKsk {}
impl HipKsk {
    /// Uploads `c0`, `c1` (`[ndigits][Lk][N]`, the `Poly<NttShoup>`s' coefficients).  The Shoup twins are optional:
    /// `None` lets the engine compute floor(c * 2^64 / q) itself -- the very definition `Poly<NttShoup>` uses
    /// (zq/mod.rs:195-199), and `Poly` has no public accessor for its twins.
    pub fn new(ct_ctx: &Arc<HipCtx>, ksk_ctx: &Arc<HipCtx>, ndigits: usize, c0: &[u64], c0_shoup: Option<&[u64]>,
               c1: &[u64], c1_shoup: Option<&[u64]>, log_base: usize) -> Result<Self> {
        let n = ndigits * ksk_ctx.poly_words();
        expect_len("ksk c0", c0.len(), n)?;
        expect_len("ksk c1", c1.len(), n)?;
        if let Some(t) = c0_shoup { expect_len("ksk c0 twins", t.len(), n)?; }
        if let Some(t) = c1_shoup { expect_len("ksk c1 twins", t.len(), n)?; }
        let mut out: *mut ffi::FheKsk = ptr::null_mut();
        check(unsafe {
            ffi::fhe_ksk_create(ct_ctx.as_ptr(), ksk_ctx.as_ptr(), ndigits, c0.as_ptr(),
                c0_shoup.map_or(ptr::null(), |t| t.as_ptr()), c1.as_ptr(), c1_shoup.map_or(ptr::null(), |t| t.as_ptr()),
                log_base, &mut out)
        })?;
        Ok(Self { ptr: out, ct_ctx: ct_ctx.clone(), ksk_ctx: ksk_ctx.clone() })
    }
    pub fn as_ptr(&self) -> *const ffi::FheKsk { self.ptr }
    pub fn ct_ctx(&self) -> &Arc<HipCtx> { &self.ct_ctx }
    pub fn ksk_ctx(&self) -> &Arc<HipCtx> { &self.ksk_ctx }
    /// `KeySwitchingKey::key_switch` (keys/key_switching_key.rs:241-270): `p` `[batch][L][N]` PowerBasis over the
    /// ciphertext context -> `c0`, `c1` `[batch][Lk][N]` Ntt over the key context.
    pub fn key_switch(&self, p: &[u64], c0: &mut [u64], c1: &mut [u64]) -> Result<()> {
        let b = whole_batch("key_switch input", p.len(), self.ct_ctx.poly_words())?;
        expect_len("key_switch c0", c0.len(), b * self.ksk_ctx.poly_words())?;
        expect_len("key_switch c1", c1.len(), b * self.ksk_ctx.poly_words())?;
        check(unsafe { ffi::fhe_key_switch(self.ptr, p.as_ptr(), c0.as_mut_ptr(), c1.as_mut_ptr(), b) })
    }
    /// `RelinearizationKey::relinearizes` (keys/relinearization_key.rs:69-102): `[batch][3][L][N]` -> `[batch][2][L][N]`.
    pub fn relinearize(&self, ct3: &[u64], out: &mut [u64]) -> Result<()> {
        let b = whole_batch("relinearize input", ct3.len(), 3 * self.ct_ctx.poly_words())?;
        expect_len("relinearize output", out.len(), b * 2 * self.ct_ctx.poly_words())?;
        check(unsafe { ffi::fhe_bfv_relinearize(self.ptr, ct3.as_ptr(), out.as_mut_ptr(), b) })
    }
    /// `GaloisKey::relinearize` (keys/galois_key.rs:63-86): `[batch][2][L][N]` -> the same shape.
    pub fn galois(&self, exponent: usize, ct: &[u64], out: &mut [u64]) -> Result<()> {
        let b = whole_batch("galois input", ct.len(), 2 * self.ct_ctx.poly_words())?;
        expect_len("galois output", out.len(), ct.len())?;
        check(unsafe { ffi::fhe_bfv_galois(self.ptr, exponent, ct.as_ptr(), out.as_mut_ptr(), b) })
    }
    fn check_resident(&self, what: &str, ct: &DeviceCiphertexts, parts: usize) -> Result<()> {
        if ct.parts != parts || ct.rows != self.ct_ctx.nmoduli() || ct.degree != self.ct_ctx.degree() {
            return Err(shape_error(&format!("{what}: expected {parts}-part ciphertexts over the key's ciphertext context")));
        }
        Ok(())
    }
    /// `relinearizes` on a device-resident batch, stream-ordered (`fhe_bfv_relinearize_dev`).
    pub fn relinearize_dev(&self, ct3: &DeviceCiphertexts, stream: &Stream) -> Result<DeviceCiphertexts> {
        self.check_resident("relinearize_dev", ct3, 3)?;
        let out = DeviceCiphertexts::alloc_on(self.ct_ctx.device(), ct3.batch, 2, ct3.rows, ct3.degree, ct3.level, stream)?;
        check(unsafe { ffi::fhe_bfv_relinearize_dev(self.ptr, ct3.buf.as_ptr(), out.buf.as_mut_ptr(), ct3.batch, stream.as_ptr()) })?;
        Ok(out)
    }
    /// `EvaluationKey::rotates_columns_by` / `rotates_rows` on a device-resident batch (`fhe_bfv_galois_dev`).
    pub fn galois_dev(&self, exponent: usize, ct: &DeviceCiphertexts, stream: &Stream) -> Result<DeviceCiphertexts> {
        self.check_resident("galois_dev", ct, 2)?;
        let out = DeviceCiphertexts::alloc_on(self.ct_ctx.device(), ct.batch, 2, ct.rows, ct.degree, ct.level, stream)?;
        check(unsafe {
            ffi::fhe_bfv_galois_dev(self.ptr, exponent, ct.buf.as_ptr(), out.buf.as_mut_ptr(), ct.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
    /// `EvaluationKey::computes_inner_sum` on a device-resident batch (`fhe_bfv_inner_sum_dev`): `keys[i]` is the
    /// Galois key of element `exponents[i]`, in the reference's order (evaluation_key.rs:56-100).
    pub fn inner_sum_dev(keys: &[Arc<HipKsk>], exponents: &[usize], ct: &DeviceCiphertexts, stream: &Stream) -> Result<DeviceCiphertexts> {
        let first = keys.first().ok_or_else(|| shape_error("inner_sum_dev: no Galois keys"))?;
        if keys.len() != exponents.len() {
            return Err(shape_error("inner_sum_dev: one exponent per Galois key"));
        }
        first.check_resident("inner_sum_dev", ct, 2)?;
        let ptrs: Vec<*const ffi::FheKsk> = keys.iter().map(|k| k.as_ptr()).collect();
        let out = DeviceCiphertexts::alloc_on(first.ct_ctx.device(), ct.batch, 2, ct.rows, ct.degree, ct.level, stream)?;
        check(unsafe {
            ffi::fhe_bfv_inner_sum_dev(ptrs.as_ptr(), exponents.as_ptr(), keys.len(), ct.buf.as_ptr(), out.buf.as_mut_ptr(),
                                       ct.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
    /// `EvaluationKey::expands` on a device-resident batch (`fhe_bfv_expand_dev`): `keys[l]` is the Galois key of
    /// element `(N >> l) + 1`.  The result has `size * ct.batch` ciphertexts laid out `[size][batch]`.
    pub fn expand_dev(keys: &[Arc<HipKsk>], size: usize, ct: &DeviceCiphertexts, stream: &Stream) -> Result<DeviceCiphertexts> {
        if size == 0 || size > ct.degree {
            return Err(HipError { status: status::INVALID_EXPANSION_SIZE, message: format!("expand_dev: size {size}, degree {}", ct.degree) });
        }
        let device = match keys.first() {
            Some(k) => {
                k.check_resident("expand_dev", ct, 2)?;
                k.ct_ctx.device()
            }
            None if size == 1 => default_device(),
            None => return Err(HipError { status: status::EXPANSION_UNSUPPORTED, message: "expand_dev: no Galois keys".into() }),
        };
        let out = DeviceCiphertexts::alloc_on(device, size * ct.batch, 2, ct.rows, ct.degree, ct.level, stream)?;
        if keys.is_empty() {   // size 1: the expansion is the ciphertext itself
            check(unsafe {
                ffi::fhe_buf_copy_async(out.buf.as_mut_ptr() as *mut c_void, ct.buf.as_ptr() as *const c_void, ct.buf.len() * 8, stream.as_ptr())
            })?;
            return Ok(out);
        }
        let ptrs: Vec<*const ffi::FheKsk> = keys.iter().map(|k| k.as_ptr()).collect();
        check(unsafe {
            ffi::fhe_bfv_expand_dev(ptrs.as_ptr(), keys.len(), ct.buf.as_ptr(), out.buf.as_mut_ptr(), size, ct.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
    /// How the engine evaluates every key switch through this key (`fhe_ksk_set_mode`): [`KsMode`]; `w_budget` bytes of
    /// transformed digit rows per launch pair of the unfused strategy (0 = default).  Values never change, only speed.
    pub fn set_mode(&self, mode: KsMode, w_budget: usize) -> Result<()> {
        check(unsafe { ffi::fhe_ksk_set_mode(self.ptr, mode as c_int, w_budget) })
    }
}
/// Key-switch evaluation strategies (`FHE_KS_*` of the header).
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
#[repr(i32)]
pub enum KsMode {
    Auto = 0,
    Fused = 1,
    Unfused = 2,
    UnfusedSub = 3,
    /// rows larger than LDS (N >= 32768) on 8192-point sub-blocks instead of 16384-point parts
    FusedSub = 4,
}
impl Drop for HipKsk {
    fn drop(&mut self) { unsafe { ffi::fhe_ksk_destroy(self.ptr) } }
}

// ------------------------------------------------------------------------------------------ keyed batches
/// The keys of many clients for ONE operation (`fhe_kskset`): every client's relinearization key, or every client's
/// Galois key of one exponent.  A keyed call takes a batch whose size is a multiple of `len()`; ciphertexts
/// `[c * m, (c + 1) * m)` belong to key `c`, and the result is what one single-key call per client gives
/// (`KeySwitchingKey::key_switch`, keys/key_switching_key.rs:241-320, client by client) in the launches of one batch.
/// The C object borrows the keys: the lifetime `'k` keeps them alive for as long as the set exists.
pub struct HipKskSet<'k> {
    ptr: *mut ffi::FheKskSet,
    first: &'k HipKsk,
    len: usize,
    _keys: PhantomData<&'k [HipKsk]>,
}
unsafe impl Send for HipKskSet<'_> {}
unsafe impl Sync for HipKskSet<'_> {}
impl<'k> HipKskSet<'k> {
    /// RNS-digit keys (`log_base == 0`) of one parameter set, one level pair and one digit count; builds the set's device
    /// table (one upload, one wait).
    pub fn new(keys: &[&'k HipKsk]) -> Result<Self> {
        let first = *keys.first().ok_or_else(|| shape_error("HipKskSet::new: no keys"))?;
        let ptrs: Vec<*const ffi::FheKsk> = keys.iter().map(|k| k.as_ptr()).collect();
        let mut out: *mut ffi::FheKskSet = ptr::null_mut();
        check(unsafe { ffi::fhe_kskset_create(ptrs.as_ptr(), ptrs.len(), &mut out) })?;
        Ok(Self { ptr: out, first, len: keys.len(), _keys: PhantomData })
    }
    pub fn as_ptr(&self) -> *const ffi::FheKskSet { self.ptr }
    pub fn len(&self) -> usize { self.len }
    pub fn is_empty(&self) -> bool { self.len == 0 }
    /// Bytes of transformed digit rows one launch pair may have in flight (`fhe_kskset_set_w_budget`; 0 = default).
    pub fn set_w_budget(&self, bytes: usize) -> Result<()> {
        check(unsafe { ffi::fhe_kskset_set_w_budget(self.ptr, bytes) })
    }
    pub fn w_budget(&self) -> Result<usize> {
        let mut bytes = 0usize;
        check(unsafe { ffi::fhe_kskset_get_w_budget(self.ptr, &mut bytes) })?;
        Ok(bytes)
    }
    /// Rotation groups of one launch of `matvec_hoisted_dev` (`fhe_kskset_set_rot_split`; 0 = the engine's rule).
    pub fn set_rot_split(&self, groups: usize) -> Result<()> {
        check(unsafe { ffi::fhe_kskset_set_rot_split(self.ptr, groups) })
    }
    pub fn rot_split(&self) -> Result<usize> {
        let mut groups = 0usize;
        check(unsafe { ffi::fhe_kskset_get_rot_split(self.ptr, &mut groups) })?;
        Ok(groups)
    }
    /// Giant groups per block of the baby stage of `matvec_bsgs_dev`, read from the BABY set (`fhe_kskset_set_bsgs_tile`;
    /// 0 = the engine's rule, 1 / 2 / 4 force a kernel instance, anything else is refused).
    pub fn set_bsgs_tile(&self, gt: usize) -> Result<()> {
        check(unsafe { ffi::fhe_kskset_set_bsgs_tile(self.ptr, gt) })
    }
    pub fn bsgs_tile(&self) -> Result<usize> {
        let mut gt = 0usize;
        check(unsafe { ffi::fhe_kskset_get_bsgs_tile(self.ptr, &mut gt) })?;
        Ok(gt)
    }
    fn check_keyed(&self, what: &str, ct: &DeviceCiphertexts, parts: usize) -> Result<()> {
        self.first.check_resident(what, ct, parts)?;
        if ct.batch % self.len != 0 {
            return Err(shape_error(&format!("{what}: the batch must be a multiple of the set's {} keys", self.len)));
        }
        Ok(())
    }
    /// `KeySwitchingKey::key_switch` per client (`fhe_key_switch_keyed_dev`): `p` `[batch][L][N]` PowerBasis ->
    /// `c0`, `c1` `[batch][Lk][N]` Ntt.
    pub fn key_switch_dev(&self, p: &DeviceBuffer, c0: &DeviceBuffer, c1: &DeviceBuffer, stream: &Stream) -> Result<()> {
        let b = whole_batch("key_switch_dev input", p.len(), self.first.ct_ctx().poly_words())?;
        expect_len("key_switch_dev c0", c0.len(), b * self.first.ksk_ctx().poly_words())?;
        expect_len("key_switch_dev c1", c1.len(), b * self.first.ksk_ctx().poly_words())?;
        check(unsafe { ffi::fhe_key_switch_keyed_dev(self.ptr, p.as_ptr(), c0.as_mut_ptr(), c1.as_mut_ptr(), b, stream.as_ptr()) })
    }
    /// `RelinearizationKey::relinearizes` per client (`fhe_bfv_relinearize_keyed_dev`).  After a `HipMul` made without a
    /// relinearization key this is `Multiplicator::multiply` with one key per client (ops/mul.rs:165-243).
    pub fn relinearize_dev(&self, ct3: &DeviceCiphertexts, stream: &Stream) -> Result<DeviceCiphertexts> {
        self.check_keyed("relinearize_dev", ct3, 3)?;
        let out = DeviceCiphertexts::alloc_on(self.first.ct_ctx().device(), ct3.batch, 2, ct3.rows, ct3.degree, ct3.level, stream)?;
        check(unsafe {
            ffi::fhe_bfv_relinearize_keyed_dev(self.ptr, ct3.buf.as_ptr(), out.buf.as_mut_ptr(), ct3.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
    /// `GaloisKey::relinearize` per client with the clients' keys of `exponent` (`fhe_bfv_galois_keyed_dev`).
    pub fn galois_dev(&self, exponent: usize, ct: &DeviceCiphertexts, stream: &Stream) -> Result<DeviceCiphertexts> {
        self.check_keyed("galois_dev", ct, 2)?;
        let out = DeviceCiphertexts::alloc_on(self.first.ct_ctx().device(), ct.batch, 2, ct.rows, ct.degree, ct.level, stream)?;
        check(unsafe {
            ffi::fhe_bfv_galois_keyed_dev(self.ptr, exponent, ct.buf.as_ptr(), out.buf.as_mut_ptr(), ct.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
    /// Hoisted rotations (`fhe_bfv_galois_hoisted_dev`; not in the reference): the set holds ONE client's Galois keys, key
    /// `r` for `exponents[r]`, and every ciphertext is rotated by all of them on one digit decomposition.  The result has
    /// `ct.batch * exponents.len()` ciphertexts laid out `[batch][rotations]`, what `dot_product_scalar_dev` reads as
    /// `count = exponents.len()` ciphertexts per item.  Its words are NOT those of a loop of `HipKsk::galois_dev` except at
    /// exponent 1 (the header states the restatement); both decrypt to the same plaintext under the same noise bound.
    pub fn galois_hoisted_dev(&self, exponents: &[usize], ct: &DeviceCiphertexts, stream: &Stream) -> Result<DeviceCiphertexts> {
        self.first.check_resident("galois_hoisted_dev", ct, 2)?;
        expect_len("galois_hoisted_dev exponents", exponents.len(), self.len)?;
        let out = DeviceCiphertexts::alloc_on(self.first.ct_ctx().device(), ct.batch * self.len, 2, ct.rows, ct.degree, ct.level, stream)?;
        check(unsafe {
            ffi::fhe_bfv_galois_hoisted_dev(self.ptr, exponents.as_ptr(), exponents.len(), ct.buf.as_ptr(), out.buf.as_mut_ptr(),
                                            ct.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
    /// Hoisted matrix-vector product (`fhe_bfv_matvec_hoisted_dev`; not in the reference): `pt0 * ct` plus the sum over `r`
    /// of `diagonals[r]` times rotation `r` of `ct`, in one call whose only output is the result -- what
    /// `galois_hoisted_dev` followed by `dot_product_scalar_dev` gives, word for word, without the `[batch][rotations]`
    /// block between them (and, like it, NOT the reference's words; the header states the restatement).  `diagonals`
    /// holds `poly_ntt` rows, `[R][L][N]` shared by the batch or `[batch][R][L][N]`; `pt0` is the identity diagonal
    /// (`[L][N]` or `[batch][L][N]`, the same way), `None` for none.
    pub fn matvec_hoisted_dev(&self, exponents: &[usize], ct: &DeviceCiphertexts, diagonals: &DeviceBuffer, pt0: Option<&DeviceBuffer>,
                              stream: &Stream) -> Result<DeviceCiphertexts> {
        self.first.check_resident("matvec_hoisted_dev", ct, 2)?;
        expect_len("matvec_hoisted_dev exponents", exponents.len(), self.len)?;
        let poly = ct.rows * ct.degree;
        let shared = diagonals.len() == self.len * poly;
        if !shared {
            expect_len("matvec_hoisted_dev diagonals", diagonals.len(), ct.batch * self.len * poly)?;
        }
        if let Some(p) = pt0 {
            expect_len("matvec_hoisted_dev identity diagonal", p.len(), if shared { poly } else { ct.batch * poly })?;
        }
        let out = DeviceCiphertexts::alloc_on(self.first.ct_ctx().device(), ct.batch, 2, ct.rows, ct.degree, ct.level, stream)?;
        check(unsafe {
            ffi::fhe_bfv_matvec_hoisted_dev(self.ptr, exponents.as_ptr(), exponents.len(), ct.buf.as_ptr(), diagonals.as_ptr(),
                                            shared as c_int, pt0.map_or(ptr::null(), |p| p.as_ptr()), out.buf.as_mut_ptr(), ct.batch,
                                            stream.as_ptr())
        })?;
        Ok(out)
    }
    /// `galois_hoisted_dev` with one Galois key set per client (`fhe_bfv_galois_hoisted_keyed_dev`): the set holds
    /// `nclients * exponents.len()` keys CLIENT-MAJOR -- entry `c * R + r` is client `c`'s key for `exponents[r]` -- and with
    /// `m = ct.batch / nclients` ciphertexts `[c * m, (c + 1) * m)` belong to client `c`.  Word for word one
    /// `galois_hoisted_dev` call per client on the client's keys and slice of the batch; the same layout of the result.
    pub fn galois_hoisted_keyed_dev(&self, nclients: usize, exponents: &[usize], ct: &DeviceCiphertexts, stream: &Stream)
                                    -> Result<DeviceCiphertexts> {
        self.first.check_resident("galois_hoisted_keyed_dev", ct, 2)?;
        expect_len("galois_hoisted_keyed_dev clients x exponents", nclients * exponents.len(), self.len)?;
        let out = DeviceCiphertexts::alloc_on(self.first.ct_ctx().device(), ct.batch * exponents.len(), 2, ct.rows, ct.degree, ct.level,
                                              stream)?;
        check(unsafe {
            ffi::fhe_bfv_galois_hoisted_keyed_dev(self.ptr, nclients, exponents.as_ptr(), exponents.len(), ct.buf.as_ptr(),
                                                  out.buf.as_mut_ptr(), ct.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
    /// `matvec_hoisted_dev` with one Galois key set per client (`fhe_bfv_matvec_hoisted_keyed_dev`): the set and the
    /// ownership rule of `galois_hoisted_keyed_dev`, the diagonals of `matvec_hoisted_dev` -- `[R][L][N]` shared by the
    /// WHOLE batch or `[batch][R][L][N]`, `pt0` the same way.  Word for word one `matvec_hoisted_dev` call per client.
    pub fn matvec_hoisted_keyed_dev(&self, nclients: usize, exponents: &[usize], ct: &DeviceCiphertexts, diagonals: &DeviceBuffer,
                                    pt0: Option<&DeviceBuffer>, stream: &Stream) -> Result<DeviceCiphertexts> {
        self.first.check_resident("matvec_hoisted_keyed_dev", ct, 2)?;
        expect_len("matvec_hoisted_keyed_dev clients x exponents", nclients * exponents.len(), self.len)?;
        let (poly, nrot) = (ct.rows * ct.degree, exponents.len());
        let shared = diagonals.len() == nrot * poly;
        if !shared {
            expect_len("matvec_hoisted_keyed_dev diagonals", diagonals.len(), ct.batch * nrot * poly)?;
        }
        if let Some(p) = pt0 {
            expect_len("matvec_hoisted_keyed_dev identity diagonal", p.len(), if shared { poly } else { ct.batch * poly })?;
        }
        let out = DeviceCiphertexts::alloc_on(self.first.ct_ctx().device(), ct.batch, 2, ct.rows, ct.degree, ct.level, stream)?;
        check(unsafe {
            ffi::fhe_bfv_matvec_hoisted_keyed_dev(self.ptr, nclients, exponents.as_ptr(), exponents.len(), ct.buf.as_ptr(),
                                                  diagonals.as_ptr(), shared as c_int, pt0.map_or(ptr::null(), |p| p.as_ptr()),
                                                  out.buf.as_mut_ptr(), ct.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
    /// Baby-step/giant-step hoisted matrix-vector product (`fhe_bfv_matvec_bsgs_dev`; not in the reference): `self` holds
    /// the baby Galois keys (key `r` for `baby_exps[r]`), `giant` the giant keys; with `G = giant.len() + 1` groups of
    /// `B = self.len() + 1` diagonals the result is the sum over `g` of giant rotation `g` of the sum over `b` of
    /// `diagonals[g][b]` times baby rotation `b` of `ct` -- `B + G - 2` keys and digit loops where `matvec_hoisted_dev`
    /// needs `G * B - 1`.  `diagonals` holds `poly_ntt` rows, `[G][B][L][N]` shared by the batch or `[batch][G][B][L][N]`;
    /// column 0 of a group is its identity diagonal, row 0 the group without a giant rotation, and the caller owes the
    /// pre-rotation `diagonals[g][b] = rot_{-gB}(d_{gB+b})`.  Word for word the composition of `matvec_hoisted_dev` and
    /// one-key `galois_hoisted_dev` calls the header states, and like them NOT the reference's words.  At most 64 keys
    /// per set (65 x 65 diagonals per call).
    pub fn matvec_bsgs_dev(&self, baby_exps: &[usize], giant: &HipKskSet<'_>, giant_exps: &[usize], ct: &DeviceCiphertexts,
                           diagonals: &DeviceBuffer, stream: &Stream) -> Result<DeviceCiphertexts> {
        self.first.check_resident("matvec_bsgs_dev", ct, 2)?;
        expect_len("matvec_bsgs_dev baby exponents", baby_exps.len(), self.len)?;
        expect_len("matvec_bsgs_dev giant exponents", giant_exps.len(), giant.len)?;
        let grid = (giant.len + 1) * (self.len + 1) * ct.rows * ct.degree;
        let shared = diagonals.len() == grid;
        if !shared {
            expect_len("matvec_bsgs_dev diagonals", diagonals.len(), ct.batch * grid)?;
        }
        let out = DeviceCiphertexts::alloc_on(self.first.ct_ctx().device(), ct.batch, 2, ct.rows, ct.degree, ct.level, stream)?;
        check(unsafe {
            ffi::fhe_bfv_matvec_bsgs_dev(self.ptr, baby_exps.as_ptr(), baby_exps.len(), giant.ptr, giant_exps.as_ptr(), giant_exps.len(),
                                         ct.buf.as_ptr(), diagonals.as_ptr(), shared as c_int, out.buf.as_mut_ptr(), ct.batch,
                                         stream.as_ptr())
        })?;
        Ok(out)
    }
    /// `EvaluationKey::computes_inner_sum` per client (`fhe_bfv_inner_sum_keyed_dev`): `sets[i]` holds every client's
    /// Galois key of element `exponents[i]`, in the reference's order (evaluation_key.rs:56-100).
    pub fn inner_sum_dev(sets: &[&HipKskSet<'k>], exponents: &[usize], ct: &DeviceCiphertexts, stream: &Stream) -> Result<DeviceCiphertexts> {
        let first = *sets.first().ok_or_else(|| shape_error("inner_sum_dev: no key sets"))?;
        if sets.len() != exponents.len() {
            return Err(shape_error("inner_sum_dev: one exponent per key set"));
        }
        first.check_keyed("inner_sum_dev", ct, 2)?;
        let ptrs: Vec<*const ffi::FheKskSet> = sets.iter().map(|s| s.as_ptr()).collect();
        let out = DeviceCiphertexts::alloc_on(first.first.ct_ctx().device(), ct.batch, 2, ct.rows, ct.degree, ct.level, stream)?;
        check(unsafe {
            ffi::fhe_bfv_inner_sum_keyed_dev(ptrs.as_ptr(), exponents.as_ptr(), sets.len(), ct.buf.as_ptr(), out.buf.as_mut_ptr(),
                                             ct.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
    /// `EvaluationKey::expands` per client (`fhe_bfv_expand_keyed_dev`): `sets[l]` holds every client's Galois key of
    /// element `(N >> l) + 1`.  The result has `size * ct.batch` ciphertexts laid out `[size][batch]`.
    pub fn expand_dev(sets: &[&HipKskSet<'k>], size: usize, ct: &DeviceCiphertexts, stream: &Stream) -> Result<DeviceCiphertexts> {
        if size == 0 || size > ct.degree {
            return Err(HipError { status: status::INVALID_EXPANSION_SIZE, message: format!("expand_dev: size {size}, degree {}", ct.degree) });
        }
        let first = *sets.first()
            .ok_or_else(|| HipError { status: status::EXPANSION_UNSUPPORTED, message: "expand_dev: no key sets".into() })?;
        first.check_keyed("expand_dev", ct, 2)?;
        let ptrs: Vec<*const ffi::FheKskSet> = sets.iter().map(|s| s.as_ptr()).collect();
        let out = DeviceCiphertexts::alloc_on(first.first.ct_ctx().device(), size * ct.batch, 2, ct.rows, ct.degree, ct.level, stream)?;
        check(unsafe {
            ffi::fhe_bfv_expand_keyed_dev(ptrs.as_ptr(), sets.len(), ct.buf.as_ptr(), out.buf.as_mut_ptr(), size, ct.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
}
impl Drop for HipKskSet<'_> {
    fn drop(&mut self) { unsafe { ffi::fhe_kskset_destroy(self.ptr) } }
}

// ----------------------------------------------------------------------------------------- Multiplicator
/// What a `fhe_mul` points at and therefore has to outlive.
enum MulKeep {
    Parts { _ext_lhs: Arc<HipScaler>, _ext_rhs: Arc<HipScaler>, _down: Arc<HipScaler>, _rk: Option<Arc<HipKsk>> },
    Params { _params: Arc<HipParams>, _rk: Option<Arc<HipKsk>> },
}
pub struct HipMul {
    ptr: *mut ffi::FheMul,
    device: i32,
    in_words: usize,  // one input ciphertext: 2 * L * N
    out_words: usize, // one output ciphertext: parts * rows * N
    out_parts: usize,
    out_rows: usize,
    degree: usize,
    _keep: MulKeep,
}
unsafe impl Send for HipMul {}
unsafe impl Sync for HipMul {}
impl HipMul {
    fn finish(ptr: *mut ffi::FheMul, base: &CtxView<'_>, keep: MulKeep) -> Result<Self> {
        let (mut p, mut r) = (0usize, 0usize);
        let st = unsafe { ffi::fhe_mul_out_shape(ptr, &mut p, &mut r) };
        if st != 0 {
            unsafe { ffi::fhe_mul_destroy(ptr) };
            check(st)?;
        }
        let n = base.degree();
        Ok(Self { ptr, device: base.device(), in_words: 2 * base.poly_words(), out_words: p * r * n, out_parts: p,
                  out_rows: r, degree: n, _keep: keep })
    }
    /// `Multiplicator::new_leveled_internal` (+ `enable_relinearization`, `enable_mod_switching`), ops/mul.rs:74-163.
    pub fn new(extender_lhs: &Arc<HipScaler>, extender_rhs: &Arc<HipScaler>, down_scaler: &Arc<HipScaler>,
               rk: Option<&Arc<HipKsk>>, mod_switch: bool) -> Result<Self> {
        let mut out: *mut ffi::FheMul = ptr::null_mut();
        check(unsafe {
            ffi::fhe_mul_create(extender_lhs.as_ptr(), extender_rhs.as_ptr(), down_scaler.as_ptr(),
                rk.map_or(ptr::null(), |k| k.as_ptr()), mod_switch as c_int, &mut out)
        })?;
        let keep = MulKeep::Parts { _ext_lhs: extender_lhs.clone(), _ext_rhs: extender_rhs.clone(),
                                    _down: down_scaler.clone(), _rk: rk.cloned() };
        Self::finish(out, extender_lhs.from_ctx(), keep)
    }
    /// (parts, rows) of one output ciphertext.
    pub fn out_shape(&self) -> (usize, usize) { (self.out_parts, self.out_rows) }
    /// `Multiplicator::multiply` (ops/mul.rs:165-243) on `lhs.len() / (2*L*N)` ciphertext pairs `[batch][2][L][N]`
    /// in Ntt form -> `out` `[batch][parts][rows][N]`.  One pair is the reference's call; a whole `&[Ciphertext]`
    /// flattened into one slice amortises the PCIe copies.
    pub fn multiply(&self, lhs: &[u64], rhs: &[u64], out: &mut [u64]) -> Result<()> {
        expect_len("multiply rhs", rhs.len(), lhs.len())?;
        let b = whole_batch("multiply lhs", lhs.len(), self.in_words)?;
        expect_len("multiply output", out.len(), b * self.out_words)?;
        check(unsafe { ffi::fhe_bfv_mul(self.ptr, lhs.as_ptr(), rhs.as_ptr(), out.as_mut_ptr(), b) })
    }
    /// The same on device-resident batches (`fhe_bfv_mul_dev`), stream-ordered: the result stays on the GPU.
    pub fn multiply_dev(&self, lhs: &DeviceCiphertexts, rhs: &DeviceCiphertexts, stream: &Stream) -> Result<DeviceCiphertexts> {
        if lhs.parts != 2 || rhs.parts != 2 || lhs.batch != rhs.batch || lhs.words_per_ct() != self.in_words
            || rhs.words_per_ct() != self.in_words || lhs.level != rhs.level {
            return Err(HipError { status: status::MUL_POLY_COUNT,
                                  message: "multiply_dev: operands must be equal batches of 2-part ciphertexts at the multiplicator's level".into() });
        }
        let level = lhs.level + (lhs.rows - self.out_rows); // (one level deeper when the handle switches the modulus)
        let out = DeviceCiphertexts::alloc_on(self.device, lhs.batch, self.out_parts, self.out_rows, self.degree, level, stream)?;
        check(unsafe {
            ffi::fhe_bfv_mul_dev(self.ptr, lhs.buf.as_ptr(), rhs.buf.as_ptr(), out.buf.as_mut_ptr(), lhs.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
    /// 1: caller's stream only; 2 (default): chunks alternate with an internal stream.
    pub fn set_streams(&self, n: usize) -> Result<()> { check(unsafe { ffi::fhe_mul_set_streams(self.ptr, n) }) }
    pub fn set_chunk(&self, pairs: usize) -> Result<()> { check(unsafe { ffi::fhe_mul_set_chunk(self.ptr, pairs) }) }
}
impl Drop for HipMul {
    fn drop(&mut self) { unsafe { ffi::fhe_mul_destroy(self.ptr) } }
}

// ---------------------------------------------------------------------------------------- BfvParameters
/// `FnMut(modulus, degree) -> NttOperator tables` used by [`HipParams::with_tables`]: the engine asks for every
/// modulus it builds a context over (ciphertext moduli and the 62-bit extension primes).
pub type TablesFn<'a> = dyn FnMut(u64, usize, &mut [u64], &mut [u64], &mut [u64], &mut [u64]) -> Option<(u64, u64)> + 'a;

unsafe extern "C" fn tables_trampoline(user: *mut c_void, modulus: u64, degree: usize, omegas: *mut u64,
                                       omegas_shoup: *mut u64, zetas_inv: *mut u64, zetas_inv_shoup: *mut u64,
                                       size_inv: *mut u64, size_inv_shoup: *mut u64) -> c_int {
    let f = unsafe { &mut *(user as *mut &mut TablesFn<'_>) };
    let s = |p: *mut u64| unsafe { std::slice::from_raw_parts_mut(p, degree) };
    match f(modulus, degree, s(omegas), s(omegas_shoup), s(zetas_inv), s(zetas_inv_shoup)) {
        Some((inv, inv_shoup)) => {
            unsafe {
                *size_inv = inv;
                *size_inv_shoup = inv_shoup;
            }
            0
        }
        None => 1,
    }
}

pub struct HipParams {
    ptr: *mut ffi::FheParams,
}
unsafe impl Send for HipParams {}
unsafe impl Sync for HipParams {}
impl HipParams {
    /// `BfvParametersBuilder::build`'s level tables with the HOST's NTT tables (parameters.rs:560-738): `tables`
    /// writes `NttOperator::new(modulus, degree)`'s four arrays and returns `(size_inv, size_inv_shoup)`.
    pub fn with_tables(device: i32, degree: usize, moduli: &[u64], plaintext_modulus: u64,
                       tables: &mut TablesFn<'_>) -> Result<Arc<Self>> {
        let mut out: *mut ffi::FheParams = ptr::null_mut();
        let mut fat: &mut TablesFn<'_> = tables;
        check(unsafe {
            ffi::fhe_params_create_with_tables(device as c_int, degree, moduli.len(), moduli.as_ptr(), plaintext_modulus,
                Some(tables_trampoline), &mut fat as *mut &mut TablesFn<'_> as *mut c_void, &mut out)
        })?;
        Ok(Arc::new(Self { ptr: out }))
    }
    /// The same for `BfvParametersBuilder::set_plaintext_modulus_biguint`: `t_limbs` are t's little-endian limbs
    /// (`fhe_params_create_big_with_tables`; a t that fits one limb behaves as `with_tables`, t >= 2^256 is refused).
    pub fn with_tables_big(device: i32, degree: usize, moduli: &[u64], t_limbs: &[u64],
                           tables: &mut TablesFn<'_>) -> Result<Arc<Self>> {
        let mut out: *mut ffi::FheParams = ptr::null_mut();
        let mut fat: &mut TablesFn<'_> = tables;
        check(unsafe {
            ffi::fhe_params_create_big_with_tables(device as c_int, degree, moduli.len(), moduli.as_ptr(), t_limbs.as_ptr(),
                t_limbs.len(), Some(tables_trampoline), &mut fat as *mut &mut TablesFn<'_> as *mut c_void, &mut out)
        })?;
        Ok(Arc::new(Self { ptr: out }))
    }
    /// W_t = ceil(bits(t) / 64): the limbs per plaintext coefficient of the `_big` calls (1 for a u64 t).
    pub fn plaintext_limbs(&self) -> usize { unsafe { ffi::fhe_params_plaintext_limbs(self.ptr) } }
    /// `Multiplicator::default(rk)` (+ `enable_mod_switching`) at `level`; `rk = None`: `&ct * &ct`.
    /// (The engine cached every table `with_tables` supplied; the closure is not called again.)  The handle keeps
    /// the parameter set (and the key) alive.
    pub fn multiplicator(self: &Arc<Self>, level: usize, rk: Option<&Arc<HipKsk>>, mod_switch: bool) -> Result<HipMul> {
        let mut out: *mut ffi::FheMul = ptr::null_mut();
        check(unsafe {
            ffi::fhe_mul_create_default(self.ptr, level, rk.map_or(ptr::null(), |k| k.as_ptr()), mod_switch as c_int, &mut out)
        })?;
        let base = self.context_at_level(level)?;
        HipMul::finish(out, &base, MulKeep::Params { _params: self.clone(), _rk: rk.cloned() })
    }
    /// The parameter set's plaintext encoding tables (`fhe_encoder_create`): t's NTT operator -- from `tables` (called
    /// once, for t, with the same contract as `with_tables`) or the engine's own psi -- SEAL's index map, and per level
    /// q mod t and delta.  The encoder keeps the parameter set alive.
    pub fn encoder(self: &Arc<Self>, tables: Option<&mut TablesFn<'_>>) -> Result<HipEncoder> {
        let mut out: *mut ffi::FheEncoder = ptr::null_mut();
        match tables {
            Some(f) => {
                let mut fat: &mut TablesFn<'_> = f;
                check(unsafe {
                    ffi::fhe_encoder_create(self.ptr, Some(tables_trampoline), &mut fat as *mut &mut TablesFn<'_> as *mut c_void,
                                            &mut out)
                })?
            }
            None => check(unsafe { ffi::fhe_encoder_create(self.ptr, None, ptr::null_mut(), &mut out) })?,
        }
        let degree = self.context_at_level(0)?.degree();
        Ok(HipEncoder { ptr: out, params: self.clone(), degree })
    }
    /// `BfvParameters::context_at_level`: borrowed from `self`.
    pub fn context_at_level(&self, level: usize) -> Result<CtxView<'_>> {
        let mut out: *const ffi::FheCtx = ptr::null();
        check(unsafe { ffi::fhe_params_ctx(self.ptr, level, &mut out) })?;
        Ok(CtxView { ptr: out, _root: PhantomData })
    }
}
impl Drop for HipParams {
    fn drop(&mut self) { unsafe { ffi::fhe_params_destroy(self.ptr) } }
}

/// `Encoding::poly()` / `Encoding::simd()` (F/bfv/encoding.rs).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Encoding {
    Poly = 0,
    Simd = 1,
}

/// The encoding tables of a `BfvParameters` on the device (`fhe_encoder`): `PlaintextVec::try_encode`,
/// `Plaintext::to_poly` and the decoders without leaving the GPU.  Values are reduced mod t on load.
pub struct HipEncoder {
    ptr: *mut ffi::FheEncoder,
    params: Arc<HipParams>, // the C object borrows the parameter set's contexts
    degree: usize,
}
unsafe impl Send for HipEncoder {}
unsafe impl Sync for HipEncoder {}
impl HipEncoder {
    /// `PlaintextVec::try_encode` (plaintext_vec.rs:70-102) at `level`: `values` `[batch][nvalues]` (nvalues <= N,
    /// zero-padded) -> `[batch][L_level][N]` Ntt, each plaintext's `poly_ntt`, or with `scaled` its `to_poly()`
    /// (plaintext.rs:172-196), the operand of `DeviceCiphertexts::{add,sub}_plain_dev`.
    pub fn encode_dev(&self, encoding: Encoding, scaled: bool, level: usize, values: &DeviceBuffer, nvalues: usize,
                      stream: &Stream) -> Result<DeviceBuffer> {
        if nvalues > self.degree {
            return Err(HipError { status: status::TOO_MANY_VALUES, message: "TooManyValues".into() });
        }
        let batch = whole_batch("encode_dev values", values.len(), nvalues)?;
        let ctx = self.params.context_at_level(level)?;
        let out = DeviceBuffer::alloc_on(ctx.device(), batch * ctx.poly_words(), stream)?;
        check(unsafe {
            ffi::fhe_bfv_encode_dev(self.ptr, encoding as c_int, scaled as c_int, level, values.as_ptr(), nvalues,
                                    out.as_mut_ptr(), batch, stream.as_ptr())
        })?;
        Ok(out)
    }
    /// `Vec::<u64>::try_decode` (plaintext.rs:157-170, 408-431): coefficients mod t `[batch][N]` (what
    /// `HipScaler::decrypt_dev` returns) -> values `[batch][N]`.
    pub fn decode_dev(&self, encoding: Encoding, coeffs: &DeviceBuffer, stream: &Stream) -> Result<DeviceBuffer> {
        let batch = whole_batch("decode_dev coefficients", coeffs.len(), self.degree)?;
        let device = self.params.context_at_level(0)?.device();
        let out = DeviceBuffer::alloc_on(device, coeffs.len(), stream)?;
        check(unsafe {
            ffi::fhe_bfv_decode_dev(self.ptr, encoding as c_int, coeffs.as_ptr(), out.as_mut_ptr(), batch, stream.as_ptr())
        })?;
        Ok(out)
    }
}
impl HipEncoder {
    /// `encode_database` (crates/fhe/examples/util.rs:97-145): item b is bytes `[b item_bytes, (b + 1) item_bytes)` of
    /// the first `nbytes` bytes of `bytes` (`DeviceBuffer::upload_bytes`; what lies from `nbytes` on reads as zero), its
    /// `transcode_from_bytes(item, nbits)` values the coefficients of one plaintext -> `[batch][L_level][N]` Ntt,
    /// `poly_ntt` or with `scaled` `to_poly()`.  `batch` items: beyond `ceil(nbytes / item_bytes)` they are the all-zero
    /// padding plaintexts (`fhe_bfv_encode_bytes_dev`).
    pub fn encode_bytes_dev(&self, scaled: bool, level: usize, bytes: &DeviceBuffer, nbytes: usize, item_bytes: usize,
                            nbits: usize, batch: usize, stream: &Stream) -> Result<DeviceBuffer> {
        if nbytes > bytes.len() * 8 {
            return Err(shape_error("encode_bytes_dev: nbytes exceeds the buffer"));
        }
        let ctx = self.params.context_at_level(level)?;
        let out = DeviceBuffer::alloc_on(ctx.device(), (batch * ctx.poly_words()).max(1), stream)?;
        check(unsafe {
            ffi::fhe_bfv_encode_bytes_dev(self.ptr, scaled as c_int, level, bytes.as_ptr() as *const u8, nbytes, item_bytes,
                                          nbits, out.as_mut_ptr(), batch, stream.as_ptr())
        })?;
        Ok(out)
    }
    /// The SealPIR fold (crates/fhe/examples/sealpir.rs:176-200): `words` `[batch][nseg][seg_len]` carrying `in_bits`
    /// each; every segment through `transcode_bidirectional(segment, in_bits, nbits)`, an item's value lists appended
    /// and cut into plaintexts of N values -> (`[batch][nplain][L_level][N]` Ntt, nplain) (`fhe_bfv_encode_words_dev`).
    pub fn encode_words_dev(&self, scaled: bool, level: usize, words: &DeviceBuffer, in_bits: usize, nseg: usize,
                            seg_len: usize, nbits: usize, stream: &Stream) -> Result<(DeviceBuffer, usize)> {
        let batch = whole_batch("encode_words_dev words", words.len(), nseg * seg_len)?;
        let nplain = unsafe { ffi::fhe_bfv_encode_words_count(self.ptr, in_bits, nseg, seg_len, nbits) };
        let ctx = self.params.context_at_level(level)?;
        let out = DeviceBuffer::alloc_on(ctx.device(), (batch * nplain * ctx.poly_words()).max(1), stream)?;
        check(unsafe {
            ffi::fhe_bfv_encode_words_dev(self.ptr, scaled as c_int, level, words.as_ptr(), in_bits, nseg, seg_len, nbits,
                                          out.as_mut_ptr(), batch, stream.as_ptr())
        })?;
        Ok((out, nplain))
    }
}

/// `fhe_util::transcode_bidirectional` (fhe-util/src/lib.rs:150-187) on device words: rows `[batch][nin]` carrying
/// `in_bits` each -> `[batch][ceil(nin in_bits / out_bits)]` words of `out_bits` bits (`fhe_transcode_dev`; the byte
/// forms `transcode_to_bytes` / `transcode_from_bytes` are the same call with a byte side, through `ffi`).  Runs on the
/// calling thread's current device, which `stream` and `input` belong to.
pub fn transcode_dev(device: i32, input: &DeviceBuffer, in_bits: usize, nin: usize, out_bits: usize, stream: &Stream)
                     -> Result<DeviceBuffer> {
    let batch = whole_batch("transcode_dev input", input.len(), nin)?;
    let nout = unsafe { ffi::fhe_transcode_count(in_bits, nin, out_bits) };
    let out = DeviceBuffer::alloc_on(device, (batch * nout).max(1), stream)?;
    check(unsafe {
        ffi::fhe_transcode_dev(input.as_ptr() as *const c_void, 0, in_bits, nin, out.as_mut_ptr() as *mut c_void, 0, out_bits,
                               batch, stream.as_ptr())
    })?;
    Ok(out)
}

impl HipEncoder {
    /// `SecretKey::measure_noise` (keys/secret_key.rs:55-98) on a device-resident batch: the bits of noise of each
    /// ciphertext, `[batch]`.  `scaler`: the cipher-to-plaintext scaler of the ciphertexts' level (as
    /// `HipScaler::decrypt_dev`), whose source context must be a level of this encoder's parameter set; `s_ntt`
    /// `[L][N]` over it.  `expected`: `None` measures against the ciphertext's own decryption (the reference);
    /// `Some` `[batch][N]` coefficients in [0, t) measures against the plaintext the caller expects
    /// (`fhe_bfv_measure_noise_dev`; the phase and the error stay in engine scratch that is cleared before reuse).
    pub fn measure_noise_dev(&self, scaler: &HipScaler, s_ntt: &DeviceBuffer, ct: &DeviceCiphertexts,
                             expected: Option<&DeviceBuffer>, stream: &Stream) -> Result<DeviceBuffer> {
        let from = scaler.from_ctx();
        expect_len("measure_noise_dev secret key", s_ntt.len(), from.poly_words())?;
        if ct.rows != from.nmoduli() || ct.degree != from.degree() {
            return Err(shape_error("measure_noise_dev: the ciphertexts are not over the scaler's source context"));
        }
        let m = match expected {
            None => ptr::null(),
            Some(p) => {
                expect_len("measure_noise_dev expected plaintexts", p.len(), ct.batch * ct.degree)?;
                p.as_ptr()
            }
        };
        let out = DeviceBuffer::alloc_on(from.device(), ct.batch.max(1), stream)?;
        check(unsafe {
            ffi::fhe_bfv_measure_noise_dev(self.ptr, scaler.as_ptr(), s_ntt.as_ptr(), ct.buf.as_ptr(), ct.parts, m,
                                           out.as_mut_ptr(), ct.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
}
impl HipEncoder {
    /// `PlaintextVec::try_encode` for `Vec<BigUint>` (plaintext_vec.rs:105-132) of a parameter set whose t exceeds 64
    /// bits: `values` `[batch][nvalues][W_t]` limbs -> `[batch][L_level][N]` Ntt, `poly_ntt` or with `scaled` the Large
    /// branch of `to_poly()` (plaintext.rs:172-197).  `Encoding::Simd` is unavailable (`fhe_bfv_encode_big_dev`).
    pub fn encode_big_dev(&self, encoding: Encoding, scaled: bool, level: usize, values: &DeviceBuffer, nvalues: usize,
                          stream: &Stream) -> Result<DeviceBuffer> {
        if nvalues > self.degree {
            return Err(HipError { status: status::TOO_MANY_VALUES, message: "TooManyValues".into() });
        }
        let wt = self.params.plaintext_limbs();
        let batch = whole_batch("encode_big_dev values", values.len(), nvalues * wt)?;
        let ctx = self.params.context_at_level(level)?;
        let out = DeviceBuffer::alloc_on(ctx.device(), batch * ctx.poly_words(), stream)?;
        check(unsafe {
            ffi::fhe_bfv_encode_big_dev(self.ptr, encoding as c_int, scaled as c_int, level, values.as_ptr(), nvalues,
                                        out.as_mut_ptr(), batch, stream.as_ptr())
        })?;
        Ok(out)
    }
    /// The tail of `SecretKey::try_decrypt`'s Large branch alone (keys/secret_key.rs:238-250): PowerBasis residues over
    /// the plaintext context `[batch][P][N]` -> `[batch][N][W_t]` limbs of ((x + t) mod Q_p) mod t
    /// (`fhe_bfv_reduce_big_dev`).  `rows` is the row count the caller laid `polys` out with: anything but
    /// `plain_rows()` is refused before the device reads a word.
    pub fn reduce_big_dev(&self, polys: &DeviceBuffer, rows: usize, stream: &Stream) -> Result<DeviceBuffer> {
        if rows == 0 || rows != self.plain_rows() {
            return Err(shape_error("reduce_big_dev: one row per modulus of the plaintext context"));
        }
        let batch = whole_batch("reduce_big_dev polynomials", polys.len(), rows * self.degree)?;
        let device = self.params.context_at_level(0)?.device();
        let out = DeviceBuffer::alloc_on(device, (batch * self.degree * self.params.plaintext_limbs()).max(1), stream)?;
        check(unsafe {
            ffi::fhe_bfv_reduce_big_dev(self.ptr, polys.as_ptr(), rows, out.as_mut_ptr(), batch, stream.as_ptr())
        })?;
        Ok(out)
    }
    /// P: the moduli of the parameter set's plaintext context (`fhe_encoder_plain_rows`).
    pub fn plain_rows(&self) -> usize { unsafe { ffi::fhe_encoder_plain_rows(self.ptr) } }
    /// `SecretKey::try_decrypt`, Large branch (keys/secret_key.rs:198-250), on a device-resident batch: as
    /// `HipScaler::decrypt_dev` with `[batch][N][W_t]` limbs out (`fhe_bfv_decrypt_big_dev`).
    pub fn decrypt_big_dev(&self, scaler: &HipScaler, s_ntt: &DeviceBuffer, ct: &DeviceCiphertexts, stream: &Stream)
                           -> Result<DeviceBuffer> {
        let from = scaler.from_ctx();
        expect_len("decrypt_big_dev secret key", s_ntt.len(), from.poly_words())?;
        if ct.rows != from.nmoduli() || ct.degree != from.degree() {
            return Err(shape_error("decrypt_big_dev: the ciphertexts are not over the scaler's source context"));
        }
        let out = DeviceBuffer::alloc_on(from.device(), (ct.batch * ct.degree * self.params.plaintext_limbs()).max(1), stream)?;
        check(unsafe {
            ffi::fhe_bfv_decrypt_big_dev(self.ptr, scaler.as_ptr(), s_ntt.as_ptr(), ct.buf.as_ptr(), ct.parts,
                                         out.as_mut_ptr(), ct.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
}
impl Drop for HipEncoder {
    fn drop(&mut self) { unsafe { ffi::fhe_encoder_destroy(self.ptr) } }
}

// ------------------------------------------------------------------------------------ engine-wide state
/// Bounds on the scratch memory the engine retains between calls (`fhe_workspace_set_limit`; 0 = none, `usize::MAX` =
/// the default: a quarter of the device's memory in total): bytes per (device, stream) and in total.  Idle blocks beyond
/// a bound are evicted least-recently-used first; calls that need more still run.  A host that destroys HIP streams of
/// its own (not [`Stream`]s, whose `Drop` tells the engine) sets `total_bytes` to a few streams' footprint.
pub fn workspace_set_limit(per_stream_bytes: usize, total_bytes: usize) -> Result<()> {
    check(unsafe { ffi::fhe_workspace_set_limit(per_stream_bytes, total_bytes) })
}
/// (bytes held, bytes in use, blocks, distinct (device, stream) owners, internal second streams) of the engine's
/// scratch pool.
pub fn workspace_stats() -> Result<(usize, usize, usize, usize, usize)> {
    let (mut h, mut u, mut b, mut o, mut a) = (0usize, 0usize, 0usize, 0usize, 0usize);
    check(unsafe { ffi::fhe_workspace_stats(&mut h, &mut u, &mut b, &mut o, &mut a) })?;
    Ok((h, u, b, o, a))
}
/// What the driver says the library's two private stream-ordered pools on `device` hold: (scratch reserved, scratch used,
/// buffers reserved, buffers used) bytes (`fhe_workspace_pool_stats`).  The scratch pool's reserved bytes respect the
/// `total_bytes` bound of [`workspace_set_limit`] once evicted blocks have retired.
pub fn workspace_pool_stats(device: i32) -> Result<(usize, usize, usize, usize)> {
    let (mut sr, mut su, mut br, mut bu) = (0usize, 0usize, 0usize, 0usize);
    check(unsafe { ffi::fhe_workspace_pool_stats(device as c_int, &mut sr, &mut su, &mut br, &mut bu) })?;
    Ok((sr, su, br, bu))
}
/// Frees every idle scratch block, internal stream and pooled event; returns the bytes released.
pub fn workspace_trim() -> usize { unsafe { ffi::fhe_workspace_trim() } }
/// Number of HIP devices the engine sees (a host that shards a batch over the GPUs of a node makes one set of handles
/// per device and drives each from its own thread -- `tests/c_host/c4_sharded.c` is that host in C).
pub fn device_count() -> i32 { unsafe { ffi::fhe_device_count() as i32 } }

// -------------------------------------------------------------------- device memory, streams, residency
/// A HIP stream made by the C ABI (`fhe_stream_create`); `_dev` calls on one stream run in order.
pub struct Stream {
    ptr: *mut c_void,
}
unsafe impl Send for Stream {}
unsafe impl Sync for Stream {}
impl Stream {
    pub fn new(device: i32) -> Result<Self> {
        let mut out: *mut c_void = ptr::null_mut();
        check(unsafe { ffi::fhe_stream_create(device as c_int, &mut out) })?;
        Ok(Self { ptr: out })
    }
    pub fn as_ptr(&self) -> *mut c_void { self.ptr }
    /// Blocks until everything enqueued on the stream has finished.
    pub fn synchronize(&self) -> Result<()> { check(unsafe { ffi::fhe_stream_sync(self.ptr) }) }
}
impl Drop for Stream {
    fn drop(&mut self) { unsafe { ffi::fhe_stream_destroy(self.ptr); } }
}

/// `len` u64 words of device memory (`fhe_buf_alloc`).  Freed on drop; `hipFree` waits for work that still uses
/// the allocation, so dropping a buffer a stream is reading is slow, not unsound.
pub struct DeviceBuffer {
    ptr: *mut u64,
    len: usize,
}
unsafe impl Send for DeviceBuffer {}
unsafe impl Sync for DeviceBuffer {}
impl DeviceBuffer {
    pub fn alloc(device: i32, len: usize) -> Result<Self> {
        let mut out: *mut c_void = ptr::null_mut();
        check(unsafe { ffi::fhe_buf_alloc(device as c_int, len * 8, &mut out) })?;
        Ok(Self { ptr: out as *mut u64, len })
    }
    /// Stream-ordered allocation (`fhe_buf_alloc_async`): usable by work enqueued on `stream` from here on, and no
    /// device synchronisation -- what the `_dev` operations allocate their results with.
    pub fn alloc_on(device: i32, len: usize, stream: &Stream) -> Result<Self> {
        let mut out: *mut c_void = ptr::null_mut();
        check(unsafe { ffi::fhe_buf_alloc_async(device as c_int, len * 8, stream.as_ptr(), &mut out) })?;
        Ok(Self { ptr: out as *mut u64, len })
    }
    /// Gives the block back behind the work already enqueued on `stream` (`fhe_buf_free_async`) instead of waiting for
    /// the device as `drop` does.  `stream` must be the stream of the buffer's LAST USE (every operation that read or
    /// wrote it was enqueued there, or is ordered before it by the caller's own events): a free that is ordered on
    /// another stream can hand the memory out again while the last reader still runs.  When in doubt,
    /// drop the buffer: `Drop` waits for the device.
    pub fn release_on(self, stream: &Stream) -> Result<()> {
        let p = self.ptr as *mut c_void;
        std::mem::forget(self);
        check(unsafe { ffi::fhe_buf_free_async(p, stream.as_ptr()) })
    }
    pub fn len(&self) -> usize { self.len }
    pub fn is_empty(&self) -> bool { self.len == 0 }
    pub fn as_ptr(&self) -> *const u64 { self.ptr }
    pub fn as_mut_ptr(&self) -> *mut u64 { self.ptr }
    /// Host -> device, stream-ordered; returns when the bytes have left `src` (the copy is waited for).
    pub fn upload(&self, src: &[u64], stream: &Stream) -> Result<()> {
        expect_len("upload", src.len(), self.len)?;
        check(unsafe { ffi::fhe_buf_upload(self.ptr as *mut c_void, src.as_ptr() as *const c_void, self.len * 8, stream.as_ptr()) })
    }
    /// Device -> host after everything enqueued on `stream` so far (waits for the stream).
    /// Host bytes (wire payloads) as a device buffer of little-endian u64 words, the last one zero-padded.
    pub fn upload_bytes(device: i32, bytes: &[u8], stream: &Stream) -> Result<Self> {
        let mut padded = bytes.to_vec();
        padded.resize(((bytes.len() + 7) / 8).max(1) * 8, 0);
        let words: Vec<u64> = padded.chunks_exact(8).map(|c| u64::from_le_bytes(c.try_into().unwrap())).collect();
        let buf = Self::alloc_on(device, words.len(), stream)?;
        buf.upload(&words, stream)?;
        Ok(buf)
    }
    pub fn download(&self, dst: &mut [u64], stream: &Stream) -> Result<()> {
        expect_len("download", dst.len(), self.len)?;
        check(unsafe { ffi::fhe_buf_download(dst.as_mut_ptr() as *mut c_void, self.ptr as *const c_void, self.len * 8, stream.as_ptr()) })
    }
}
impl Drop for DeviceBuffer {
    fn drop(&mut self) { unsafe { ffi::fhe_buf_free(self.ptr as *mut c_void); } }
}

/// 32-byte seeds on the device, `[batch][32]` bytes (four little-endian `u64` words each): the generators of
/// `CtxView::{sample_small_dev, encrypt_sk_dev, encrypt_pk_dev}`.  `ChaCha8Rng::from_seed(seed)` takes the bytes as its
/// key; the word layout is PARITY UNPINNED against a real fhe.rs run, like `fhe_poly_from_seed` (`fhe_hip.h`).
pub struct DeviceSeeds {
    buf: DeviceBuffer,
    pub batch: usize,
}
impl DeviceSeeds {
    pub fn upload(device: i32, seeds: &[[u8; 32]], stream: &Stream) -> Result<Self> {
        let words: Vec<u64> = seeds
            .iter()
            .flat_map(|s| s.chunks_exact(8).map(|c| u64::from_le_bytes(c.try_into().unwrap())).collect::<Vec<_>>())
            .collect();
        let buf = DeviceBuffer::alloc_on(device, words.len().max(1), stream)?;
        if !words.is_empty() {
            buf.upload(&words, stream)?;
        }
        Ok(Self { buf, batch: seeds.len() })
    }
    fn as_ptr(&self) -> *const u8 { self.buf.as_ptr() as *const u8 }
    pub fn release_on(self, stream: &Stream) -> Result<()> { self.buf.release_on(stream) }
}

/// Key generation on the device (F/bfv/keys/key_switching_key.rs:71-236, relinearization_key.rs:43-64,
/// galois_key.rs:26-58): key b with rng = `ChaCha8Rng::from_seed(seeds[b])`; the keys' public seeds K come back as
/// `DeviceSeeds`.  `s_ntt` is the level-0 secret in Ntt form (`CtxView::sample_small_dev`), the caller's to clear; the
/// engine clears its own scratch of errors, s^2 and s_sub.  The handles are ready to use on `stream`.
impl HipKsk {
    fn adopt(ptrs: Vec<*mut ffi::FheKsk>, ct_ctx: &Arc<HipCtx>, ksk_ctx: &Arc<HipCtx>) -> Vec<Self> {
        ptrs.into_iter().map(|p| Self { ptr: p, ct_ctx: ct_ctx.clone(), ksk_ctx: ksk_ctx.clone() }).collect()
    }
    fn seeds_out(ksk_ctx: &Arc<HipCtx>, batch: usize, stream: &Stream) -> Result<DeviceSeeds> {
        DeviceSeeds::upload(ksk_ctx.device(), &vec![[0u8; 32]; batch], stream)
    }
    /// `KeySwitchingKey::new` for `seeds.batch` keys: `from_ntt` `[batch][Lk][N]` is the reference's `from` in Ntt form
    /// over the key context, canonical residues (row j below q_j; not checked on the device).
    pub fn generate(ct_ctx: &Arc<HipCtx>, ksk_ctx: &Arc<HipCtx>, variance: usize, s_ntt: &DeviceBuffer,
                    from_ntt: &DeviceBuffer, seeds: &DeviceSeeds, stream: &Stream) -> Result<(Vec<Self>, DeviceSeeds)> {
        expect_len("generate from_ntt", from_ntt.len(), seeds.batch * ksk_ctx.poly_words())?;
        if s_ntt.len() < ksk_ctx.poly_words() {
            return Err(shape_error("generate: s_ntt is shorter than one polynomial over the key context"));
        }
        let k = Self::seeds_out(ksk_ctx, seeds.batch, stream)?;
        let mut out = vec![ptr::null_mut(); seeds.batch];
        check(unsafe {
            ffi::fhe_ksk_generate_dev(ct_ctx.as_ptr(), ksk_ctx.as_ptr(), variance, s_ntt.as_ptr(), from_ntt.as_ptr(),
                                      seeds.as_ptr(), seeds.batch, k.buf.as_mut_ptr() as *mut u8, stream.as_ptr(),
                                      out.as_mut_ptr())
        })?;
        Ok((Self::adopt(out, ct_ctx, ksk_ctx), k))
    }
    /// `RelinearizationKey::new_leveled` from one seed.
    pub fn generate_relin(ct_ctx: &Arc<HipCtx>, key_ctx: &Arc<HipCtx>, variance: usize, s_ntt: &DeviceBuffer,
                          seed: &DeviceSeeds, stream: &Stream) -> Result<(Self, DeviceSeeds)> {
        expect_len("generate_relin seeds", seed.batch, 1)?;
        if s_ntt.len() < key_ctx.poly_words() {
            return Err(shape_error("generate_relin: s_ntt is shorter than one polynomial over the key context"));
        }
        let k = Self::seeds_out(key_ctx, 1, stream)?;
        let mut out: *mut ffi::FheKsk = ptr::null_mut();
        check(unsafe {
            ffi::fhe_bfv_relin_key_generate_dev(ct_ctx.as_ptr(), key_ctx.as_ptr(), variance, s_ntt.as_ptr(), seed.as_ptr(),
                                                k.buf.as_mut_ptr() as *mut u8, stream.as_ptr(), &mut out)
        })?;
        Ok((Self { ptr: out, ct_ctx: ct_ctx.clone(), ksk_ctx: key_ctx.clone() }, k))
    }
    /// `GaloisKey::new` for every exponent in one call, key b from `seeds[b]`; use key b with exponent b mod 2N.
    pub fn generate_galois(ct_ctx: &Arc<HipCtx>, key_ctx: &Arc<HipCtx>, variance: usize, s_ntt: &DeviceBuffer,
                           exponents: &[usize], seeds: &DeviceSeeds, stream: &Stream) -> Result<(Vec<Self>, DeviceSeeds)> {
        expect_len("generate_galois seeds", seeds.batch, exponents.len())?;
        if s_ntt.len() < key_ctx.poly_words() {
            return Err(shape_error("generate_galois: s_ntt is shorter than one polynomial over the key context"));
        }
        let k = Self::seeds_out(key_ctx, seeds.batch, stream)?;
        let mut out = vec![ptr::null_mut(); seeds.batch];
        check(unsafe {
            ffi::fhe_bfv_galois_keys_generate_dev(ct_ctx.as_ptr(), key_ctx.as_ptr(), variance, s_ntt.as_ptr(),
                                                  exponents.as_ptr(), seeds.as_ptr(), seeds.batch,
                                                  k.buf.as_mut_ptr() as *mut u8, stream.as_ptr(), out.as_mut_ptr())
        })?;
        Ok((Self::adopt(out, ct_ctx, key_ctx), k))
    }
    /// The key's digit count as the engine holds it (`fhe_ksk_ndigits`): `c0`, `c1` and their twins are
    /// `[ndigits][Lk][N]`.
    pub fn ndigits(&self) -> usize { unsafe { ffi::fhe_ksk_ndigits(self.ptr) } }
    /// The key's `c0`, `c1` and their Shoup twins, `[ndigits][Lk][N]` each on the device, sized from the engine's own
    /// digit count of this key: what a client sends to the server (`HipKsk::new` of the downloaded arrays is an equal
    /// key).
    pub fn export_dev(&self, stream: &Stream) -> Result<[DeviceBuffer; 4]> {
        let len = self.ndigits() * self.ksk_ctx.poly_words();
        let dev = self.ksk_ctx.device();
        let out = [DeviceBuffer::alloc_on(dev, len, stream)?, DeviceBuffer::alloc_on(dev, len, stream)?,
                   DeviceBuffer::alloc_on(dev, len, stream)?, DeviceBuffer::alloc_on(dev, len, stream)?];
        check(unsafe {
            ffi::fhe_ksk_export_dev(self.ptr, out[0].as_mut_ptr(), out[1].as_mut_ptr(), out[2].as_mut_ptr(),
                                    out[3].as_mut_ptr(), stream.as_ptr())
        })?;
        Ok(out)
    }
}

/// The `c1` half of a `KeySwitchingKeyProto`: the packed polynomials, or the 32-byte seeds they expand from.
pub enum WireC1<'a> {
    Bytes(&'a DeviceBuffer),
    Seeds(&'a DeviceSeeds),
}

/// Keys to and from the payloads of their `KeySwitchingKeyProto` messages on the device
/// (F/bfv/keys/key_switching_key.rs:365-482).  Wire bytes travel in `DeviceBuffer`s (u64 words, the last one padded).
impl HipKsk {
    /// u64 words that hold `nkeys` keys' `c0` (or `c1`) payloads: `nkeys * ndigits * serialized_size` bytes, rounded up.
    pub fn wire_words(ksk_ctx: &Arc<HipCtx>, ndigits: usize, nkeys: usize) -> usize {
        (nkeys * ndigits * ksk_ctx.serialized_size() + 7) / 8
    }
    /// `KeySwitchingKey::try_convert_from(&KeySwitchingKeyProto)` for `nkeys` keys of one geometry: `c0_bytes` holds
    /// `proto.c0[i].coefficients` concatenated, key after key; `c1` the same for `proto.c1`, or `proto.seed` per key.
    /// `ndigits` is the messages' polynomial count (the engine derives its own from the contexts and `log_base`, and
    /// the lengths are checked against the caller's).  A coefficient >= q_j -> `status::ARG`, no key is made.  The
    /// call waits for `stream` once; the keys are ready on any stream.
    pub fn from_wire_dev(ct_ctx: &Arc<HipCtx>, ksk_ctx: &Arc<HipCtx>, log_base: usize, ndigits: usize,
                         c0_bytes: &DeviceBuffer, c1: WireC1<'_>, nkeys: usize, stream: &Stream) -> Result<Vec<Self>> {
        let words = Self::wire_words(ksk_ctx, ndigits, nkeys);
        expect_len("from_wire_dev c0_bytes", c0_bytes.len(), words.max(1))?;
        let (c1_ptr, seed_ptr) = match c1 {
            WireC1::Bytes(b) => {
                expect_len("from_wire_dev c1_bytes", b.len(), words.max(1))?;
                (b.as_ptr() as *const u8, ptr::null())
            }
            WireC1::Seeds(sd) => {
                expect_len("from_wire_dev seeds", sd.batch, nkeys)?;
                (ptr::null(), sd.as_ptr())
            }
        };
        let mut out = vec![ptr::null_mut(); nkeys];
        check(unsafe {
            ffi::fhe_ksk_load_wire_dev(ct_ctx.as_ptr(), ksk_ctx.as_ptr(), log_base, c0_bytes.as_ptr() as *const u8, c1_ptr,
                                       seed_ptr, nkeys, stream.as_ptr(), out.as_mut_ptr())
        })?;
        let keys = Self::adopt(out, ct_ctx, ksk_ctx);
        for k in keys.iter() {
            expect_len("from_wire_dev ndigits", k.ndigits(), ndigits)?;
        }
        Ok(keys)
    }
    /// `From<&KeySwitchingKey> for KeySwitchingKeyProto`: (`c0` payloads, `c1` payloads when `with_c1`), packed from the
    /// handle's arrays on `stream`; a seeded message sends `c0` and the key's seed.
    pub fn to_wire_dev(&self, with_c1: bool, stream: &Stream) -> Result<(DeviceBuffer, Option<DeviceBuffer>)> {
        let words = Self::wire_words(&self.ksk_ctx, self.ndigits(), 1).max(1);
        let dev = self.ksk_ctx.device();
        let c0 = DeviceBuffer::alloc_on(dev, words, stream)?;
        let c1 = if with_c1 { Some(DeviceBuffer::alloc_on(dev, words, stream)?) } else { None };
        expect_len("to_wire_dev c0_bytes", c0.len(), words)?;
        check(unsafe {
            ffi::fhe_ksk_serialize_dev(self.ptr, c0.as_mut_ptr() as *mut u8,
                                       c1.as_ref().map_or(ptr::null_mut(), |b| b.as_mut_ptr() as *mut u8), stream.as_ptr())
        })?;
        Ok((c0, c1))
    }
}

/// Encryption over one level's context (F/bfv/keys/secret_key.rs, public_key.rs).  The engine clears its own scratch of
/// samples; `s_ntt` and the output of `sample_small_dev` are the caller's to clear.
impl CtxView<'_> {
    /// `Poly::small(ctx, variance, ChaCha8Rng::from_seed(seed))` (rq/mod.rs:298-330) per seed -> `[batch][L][N]`,
    /// Ntt when `to_ntt` (over the level-0 context: `SecretKey::random`'s `s_ntt`, secret_key.rs:41-46).
    pub fn sample_small_dev(&self, variance: usize, seeds: &DeviceSeeds, to_ntt: bool, stream: &Stream) -> Result<DeviceBuffer> {
        let out = DeviceBuffer::alloc_on(self.device(), (seeds.batch * self.poly_words()).max(1), stream)?;
        check(unsafe {
            ffi::fhe_bfv_sample_small_dev(self.ptr, variance, seeds.as_ptr(), to_ntt as c_int, out.as_mut_ptr(), seeds.batch,
                                          stream.as_ptr())
        })?;
        Ok(out)
    }
    /// `SecretKey::encrypt_poly` (secret_key.rs:100-134) at this context's `level`: c1 = `random_from_seed(a_seeds[b])`,
    /// c0 = `small(e_seeds[b])` - c1 s + pt.  `s_ntt`: the level-0 key (its first L rows are used); `pt`: the
    /// Delta-scaled plaintexts (`HipEncoder::encode_dev` with `scaled`), `[rows][N]` shared or `[batch][rows][N]`, or
    /// `None` for the zero plaintext (`PublicKey::new`).
    pub fn encrypt_sk_dev(&self, level: usize, variance: usize, s_ntt: &DeviceBuffer, a_seeds: &DeviceSeeds,
                          e_seeds: &DeviceSeeds, pt: Option<&DeviceBuffer>, stream: &Stream) -> Result<DeviceCiphertexts> {
        if a_seeds.batch != e_seeds.batch {
            return Err(shape_error("encrypt_sk_dev: as many a seeds as e seeds"));
        }
        if s_ntt.len() < self.poly_words() {
            return Err(shape_error("encrypt_sk_dev: s_ntt is shorter than one polynomial over this context"));
        }
        let (pp, shared) = self.plain_for("encrypt_sk_dev", a_seeds.batch, pt)?;
        let out = DeviceCiphertexts::alloc_on(self.device(), a_seeds.batch.max(1), 2, self.nmoduli(), self.degree(), level,
                                              stream)?;
        check(unsafe {
            ffi::fhe_bfv_encrypt_sk_dev(self.ptr, variance, s_ntt.as_ptr(), a_seeds.as_ptr(), e_seeds.as_ptr(), pp,
                                        shared as c_int, out.buf.as_mut_ptr(), a_seeds.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
    /// `PublicKey::try_encrypt` (public_key.rs:47-97): u, e1, e2 three `Poly::small` draws of
    /// `ChaCha8Rng::from_seed(seeds[b])`; c0 = u pk0 + e1 + pt, c1 = u pk1 + e2.  `pk`: one two-part ciphertext over
    /// this context (switched down to it with `ciphertexts_switch_to_level_dev` when the level is not 0).
    pub fn encrypt_pk_dev(&self, variance: usize, pk: &DeviceCiphertexts, seeds: &DeviceSeeds, pt: Option<&DeviceBuffer>,
                          stream: &Stream) -> Result<DeviceCiphertexts> {
        if pk.batch != 1 || pk.parts != 2 || pk.rows != self.nmoduli() || pk.degree != self.degree() {
            return Err(shape_error("encrypt_pk_dev: the public key must be one two-part ciphertext over this context"));
        }
        let (pp, shared) = self.plain_for("encrypt_pk_dev", seeds.batch, pt)?;
        let out = DeviceCiphertexts::alloc_on(self.device(), seeds.batch.max(1), 2, self.nmoduli(), self.degree(), pk.level,
                                              stream)?;
        check(unsafe {
            ffi::fhe_bfv_encrypt_pk_dev(self.ptr, variance, pk.buf.as_ptr(), seeds.as_ptr(), pp, shared as c_int,
                                        out.buf.as_mut_ptr(), seeds.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
    /// W = ceil(bitlen(q) / 64): the limbs per coefficient `lift_dev` writes (`fhe_ctx_lift_limbs`).
    pub fn lift_limbs(&self) -> usize { unsafe { ffi::fhe_ctx_lift_limbs(self.ptr) } }
    /// `RnsContext::lift` per coefficient (rns/mod.rs:138-143, as `Vec<BigUint>::from(&Poly)` applies it): `polys`
    /// `[batch][L][N]` canonical residues in any representation -> `[batch][N][W]` little-endian u64 limbs of the
    /// integers in [0, q).
    pub fn lift_dev(&self, polys: &DeviceBuffer, stream: &Stream) -> Result<DeviceBuffer> {
        let batch = whole_batch("lift_dev polynomials", polys.len(), self.poly_words())?;
        let out = DeviceBuffer::alloc_on(self.device(), (batch * self.degree() * self.lift_limbs()).max(1), stream)?;
        check(unsafe { ffi::fhe_poly_lift_dev(self.ptr, polys.as_ptr(), out.as_mut_ptr(), batch, stream.as_ptr()) })?;
        Ok(out)
    }
    /// The loop of `SecretKey::measure_noise` (secret_key.rs:88-95) on its own: per polynomial of `polys`
    /// `[batch][L][N]`, the maximum over its coefficients of min(bits(x), bits(q - x)) -> `[batch]`.
    pub fn centered_bits_dev(&self, polys: &DeviceBuffer, stream: &Stream) -> Result<DeviceBuffer> {
        let batch = whole_batch("centered_bits_dev polynomials", polys.len(), self.poly_words())?;
        let out = DeviceBuffer::alloc_on(self.device(), batch.max(1), stream)?;
        check(unsafe { ffi::fhe_poly_centered_bits_dev(self.ptr, polys.as_ptr(), out.as_mut_ptr(), batch, stream.as_ptr()) })?;
        Ok(out)
    }
    /// (plaintext pointer, shared) of an encryption's optional plaintext operand for `batch` items.
    fn plain_for(&self, what: &str, batch: usize, pt: Option<&DeviceBuffer>) -> Result<(*const u64, bool)> {
        match pt {
            None => Ok((ptr::null(), false)),
            Some(p) if p.len() == self.poly_words() => Ok((p.as_ptr(), true)),
            Some(p) => {
                expect_len(what, p.len(), batch * self.poly_words())?;
                Ok((p.as_ptr(), false))
            }
        }
    }
}

/// The secret operand of a multiparty share call: one party's level-0 secret serving the whole batch (its first L rows
/// are read), or one level-0 secret of `level0_rows` rows per item -- many parties in one call.
pub enum PartySecrets<'a> {
    Shared(&'a DeviceBuffer),
    PerItem { secrets: &'a DeviceBuffer, level0_rows: usize },
}

/// Multiparty BFV over one level's context (crates/fhe/src/mbfv/): a party's shares and the aggregator's sums.  Errors
/// are `Poly::small` draws of `ChaCha8Rng::from_seed(seeds[b])`; the engine clears its own scratch of samples and of
/// products with a secret, the secrets and the shares are the caller's to clear.
impl CtxView<'_> {
    /// (pointer, shared) of a call's secrets after checking their length for `batch` items.
    fn party_secrets(&self, what: &str, s: &PartySecrets<'_>, batch: usize) -> Result<(*const u64, bool)> {
        match s {
            PartySecrets::Shared(b) => {
                if b.len() < self.poly_words() {
                    return Err(shape_error(&format!("{what}: the secret is shorter than one polynomial over this context")));
                }
                Ok((b.as_ptr(), true))
            }
            PartySecrets::PerItem { secrets, level0_rows } => {
                if *level0_rows < self.nmoduli() {
                    return Err(shape_error(&format!("{what}: a level-0 secret has at least this context's rows")));
                }
                expect_len(what, secrets.len(), batch * level0_rows * self.degree())?;
                Ok((secrets.as_ptr(), false))
            }
        }
    }
    /// `PublicKeyShare::new` (mbfv/public_key_gen.rs:32-57): e - crp s per seed -> `[batch][L][N]`.  `crp` `[L][N]`.
    pub fn mbfv_pk_share_dev(&self, variance: usize, crp: &DeviceBuffer, s: &PartySecrets<'_>, seeds: &DeviceSeeds,
                             stream: &Stream) -> Result<DeviceBuffer> {
        expect_len("mbfv_pk_share_dev crp", crp.len(), self.poly_words())?;
        let (sp, shared) = self.party_secrets("mbfv_pk_share_dev secrets", s, seeds.batch)?;
        let out = DeviceBuffer::alloc_on(self.device(), (seeds.batch * self.poly_words()).max(1), stream)?;
        check(unsafe {
            ffi::fhe_mbfv_pk_share_dev(self.ptr, variance, crp.as_ptr(), sp, shared as c_int, seeds.as_ptr(), out.as_mut_ptr(),
                                       seeds.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
    /// `SecretKeySwitchShare::new` (mbfv/secret_key_switch.rs:38-95): e + c1 (s_in - s_out) for every ciphertext of
    /// `ct` (one: shared by the batch of parties) -> `[batch][L][N]`; `s_out` `None` is `DecryptionShare::new`
    /// (:133-142).  `s_out` takes the form of `s_in`.
    pub fn mbfv_sks_share_dev(&self, variance: usize, s_in: &PartySecrets<'_>, s_out: Option<&DeviceBuffer>,
                              ct: &DeviceCiphertexts, seeds: &DeviceSeeds, stream: &Stream) -> Result<DeviceBuffer> {
        if ct.parts != 2 || ct.rows != self.nmoduli() || ct.degree != self.degree() || (ct.batch != 1 && ct.batch != seeds.batch) {
            return Err(shape_error("mbfv_sks_share_dev: two-part ciphertexts over this context, one or one per seed"));
        }
        let (sp, shared) = self.party_secrets("mbfv_sks_share_dev secrets", s_in, seeds.batch)?;
        let so = match (s_out, s_in) {
            (None, _) => ptr::null(),
            (Some(o), PartySecrets::Shared(i)) => { expect_len("mbfv_sks_share_dev output secret", o.len(), i.len())?; o.as_ptr() }
            (Some(o), PartySecrets::PerItem { secrets, .. }) => {
                expect_len("mbfv_sks_share_dev output secrets", o.len(), secrets.len())?;
                o.as_ptr()
            }
        };
        let stride = if ct.batch == 1 { 0 } else { ct.words_per_ct() };
        let out = DeviceBuffer::alloc_on(self.device(), (seeds.batch * self.poly_words()).max(1), stream)?;
        check(unsafe {
            ffi::fhe_mbfv_sks_share_dev(self.ptr, variance, sp, so, shared as c_int, ct.buf.as_ptr().add(self.poly_words()),
                                        stride, seeds.as_ptr(), out.as_mut_ptr(), seeds.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
    /// `PublicKeySwitchShare::new` (mbfv/public_key_switch.rs:33-92): (pk0 u + s c1 + e0, pk1 u + e1) per seed, as a
    /// batch of two-part ciphertexts.  `pk`: the output key over this context, as for `encrypt_pk_dev`.
    pub fn mbfv_pks_share_dev(&self, variance: usize, s: &PartySecrets<'_>, pk: &DeviceCiphertexts, ct: &DeviceCiphertexts,
                              seeds: &DeviceSeeds, stream: &Stream) -> Result<DeviceCiphertexts> {
        for c in [pk, ct] {
            if c.parts != 2 || c.rows != self.nmoduli() || c.degree != self.degree() {
                return Err(shape_error("mbfv_pks_share_dev: the key and the ciphertexts have two parts over this context"));
            }
        }
        if pk.batch != 1 || (ct.batch != 1 && ct.batch != seeds.batch) {
            return Err(shape_error("mbfv_pks_share_dev: one public key; one ciphertext or one per seed"));
        }
        let (sp, shared) = self.party_secrets("mbfv_pks_share_dev secrets", s, seeds.batch)?;
        let out = DeviceCiphertexts::alloc_on(self.device(), seeds.batch.max(1), 2, self.nmoduli(), self.degree(), ct.level, stream)?;
        check(unsafe {
            ffi::fhe_mbfv_pks_share_dev(self.ptr, variance, sp, shared as c_int, pk.buf.as_ptr(), ct.buf.as_ptr(),
                                        (ct.batch == 1) as c_int, seeds.as_ptr(), out.buf.as_mut_ptr(), seeds.batch,
                                        stream.as_ptr())
        })?;
        Ok(out)
    }
    /// `RelinKeyShare<R1>::new` (round 1, mbfv/relin_key_gen.rs:141-197) or, with the aggregated round-1 shares
    /// `r1 = Some((h0, h1))`, `RelinKeyShare<R2>::new` (:243-296) -> (h0, h1), `[batch][L][L][N]` each.  `crp`
    /// `[L][L][N]` (round 1 only); `u`: the parties' `RelinKeyGenerator::new` draws (`sample_small_dev`, Ntt), in the
    /// form of `s`.
    pub fn mbfv_rlk_round_dev(&self, variance: usize, s: &PartySecrets<'_>, u: &DeviceBuffer, crp: &DeviceBuffer,
                              r1: Option<(&DeviceBuffer, &DeviceBuffer)>, seeds: &DeviceSeeds, stream: &Stream)
                              -> Result<(DeviceBuffer, DeviceBuffer)> {
        let key_words = self.nmoduli() * self.poly_words();
        expect_len("mbfv_rlk_round_dev crp", crp.len(), key_words)?;
        let (sp, shared) = self.party_secrets("mbfv_rlk_round_dev secrets", s, seeds.batch)?;
        match s {
            PartySecrets::Shared(b) => expect_len("mbfv_rlk_round_dev u", u.len(), b.len())?,
            PartySecrets::PerItem { secrets, .. } => expect_len("mbfv_rlk_round_dev u", u.len(), secrets.len())?,
        }
        let len = (seeds.batch * key_words).max(1);
        let (h0, h1) = (DeviceBuffer::alloc_on(self.device(), len, stream)?, DeviceBuffer::alloc_on(self.device(), len, stream)?);
        check(match r1 {
            None => unsafe {
                ffi::fhe_mbfv_rlk_round1_dev(self.ptr, variance, sp, u.as_ptr(), shared as c_int, crp.as_ptr(), seeds.as_ptr(),
                                             h0.as_mut_ptr(), h1.as_mut_ptr(), seeds.batch, stream.as_ptr())
            },
            Some((a0, a1)) => {
                expect_len("mbfv_rlk_round_dev aggregated h0", a0.len(), key_words)?;
                expect_len("mbfv_rlk_round_dev aggregated h1", a1.len(), key_words)?;
                unsafe {
                    ffi::fhe_mbfv_rlk_round2_dev(self.ptr, variance, sp, u.as_ptr(), shared as c_int, a0.as_ptr(), a1.as_ptr(),
                                                 seeds.as_ptr(), h0.as_mut_ptr(), h1.as_mut_ptr(), seeds.batch, stream.as_ptr())
                }
            }
        })?;
        Ok((h0, h1))
    }
    /// `Aggregate::from_shares`: `base` + the sum of `nshares` shares of `npolys` polynomials each, laid out
    /// `[nshares][npolys][L][N]` -> `[npolys][L][N]`.  `base` (`[npolys][L][N]`, e.g. the c0 parts) is optional.
    pub fn mbfv_aggregate_dev(&self, shares: &DeviceBuffer, nshares: usize, base: Option<&DeviceBuffer>, stream: &Stream)
                              -> Result<DeviceBuffer> {
        if nshares == 0 {
            return Err(shape_error("mbfv_aggregate_dev: NoShares"));
        }
        let per = whole_batch("mbfv_aggregate_dev shares", shares.len(), nshares)?;
        let npolys = whole_batch("mbfv_aggregate_dev share", per, self.poly_words())?;
        if let Some(b) = base { expect_len("mbfv_aggregate_dev base", b.len(), per)?; }
        let out = DeviceBuffer::alloc_on(self.device(), per.max(1), stream)?;
        check(unsafe {
            ffi::fhe_mbfv_aggregate_dev(self.ptr, shares.as_ptr(), nshares, per, npolys, base.map_or(ptr::null(), |b| b.as_ptr()),
                                        out.as_mut_ptr(), stream.as_ptr())
        })?;
        Ok(out)
    }
}

impl HipScaler {
    /// `Plaintext::from_shares` (mbfv/secret_key_switch.rs:145-186) with this cipher-to-plaintext scaler: c0 + the sum
    /// of the `nshares` decryption shares (`[nshares][batch][L][N]`), scaled -> the coefficients mod t, `[batch][N]`.
    pub fn mbfv_decrypt_dev(&self, plaintext_modulus: u64, ct: &DeviceCiphertexts, shares: &DeviceBuffer, nshares: usize,
                            stream: &Stream) -> Result<DeviceBuffer> {
        if ct.parts != 2 || ct.rows != self.from.nmoduli() || ct.degree != self.from.degree() {
            return Err(shape_error("mbfv_decrypt_dev: two-part ciphertexts over the scaler's source context"));
        }
        if nshares == 0 {
            return Err(shape_error("mbfv_decrypt_dev: NoShares"));
        }
        let stride = ct.batch * self.from.poly_words();
        expect_len("mbfv_decrypt_dev shares", shares.len(), nshares * stride)?;
        let out = DeviceBuffer::alloc_on(self.from.device(), (ct.batch * ct.degree).max(1), stream)?;
        check(unsafe {
            ffi::fhe_mbfv_decrypt_dev(self.ptr, plaintext_modulus, ct.buf.as_ptr(), shares.as_ptr(), nshares, stride,
                                      out.as_mut_ptr(), ct.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
}

impl HipScaler {
    /// `Plaintext::from_shares` with the Large tail, for `encoder`'s parameter set (t above 64 bits): as
    /// `mbfv_decrypt_dev` with `[batch][N][W_t]` limbs out (`fhe_mbfv_decrypt_big_dev`).
    pub fn mbfv_decrypt_big_dev(&self, encoder: &HipEncoder, ct: &DeviceCiphertexts, shares: &DeviceBuffer, nshares: usize,
                                stream: &Stream) -> Result<DeviceBuffer> {
        if ct.parts != 2 || ct.rows != self.from.nmoduli() || ct.degree != self.from.degree() {
            return Err(shape_error("mbfv_decrypt_big_dev: two-part ciphertexts over the scaler's source context"));
        }
        if nshares == 0 {
            return Err(shape_error("mbfv_decrypt_big_dev: NoShares"));
        }
        let stride = ct.batch * self.from.poly_words();
        expect_len("mbfv_decrypt_big_dev shares", shares.len(), nshares * stride)?;
        let wt = encoder.params.plaintext_limbs();
        let out = DeviceBuffer::alloc_on(self.from.device(), (ct.batch * ct.degree * wt).max(1), stream)?;
        check(unsafe {
            ffi::fhe_mbfv_decrypt_big_dev(encoder.ptr, self.ptr, ct.buf.as_ptr(), shares.as_ptr(), nshares, stride,
                                          out.as_mut_ptr(), ct.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
}

impl HipKsk {
    /// `RelinearizationKey::from_shares` (mbfv/relin_key_gen.rs:299-351): the collective key of `nshares` round-2
    /// shares (`r2_h0`, `r2_h1` `[nshares][L][L][N]`) and the aggregated round-1 `r1_h1` `[L][L][N]`, at level 0.
    pub fn from_relin_shares_dev(ctx: &Arc<HipCtx>, r2_h0: &DeviceBuffer, r2_h1: &DeviceBuffer, nshares: usize,
                                 r1_h1: &DeviceBuffer, stream: &Stream) -> Result<Self> {
        let key_words = ctx.nmoduli() * ctx.poly_words();
        if nshares == 0 {
            return Err(shape_error("from_relin_shares_dev: NoShares"));
        }
        expect_len("from_relin_shares_dev h0 shares", r2_h0.len(), nshares * key_words)?;
        expect_len("from_relin_shares_dev h1 shares", r2_h1.len(), nshares * key_words)?;
        expect_len("from_relin_shares_dev round-1 h1", r1_h1.len(), key_words)?;
        let mut out: *mut ffi::FheKsk = ptr::null_mut();
        check(unsafe {
            ffi::fhe_mbfv_relin_key_aggregate_dev(ctx.as_ptr(), r2_h0.as_ptr(), r2_h1.as_ptr(), nshares, key_words,
                                                  r1_h1.as_ptr(), stream.as_ptr(), &mut out)
        })?;
        Ok(Self { ptr: out, ct_ctx: ctx.clone(), ksk_ctx: ctx.clone() })
    }
}

/// A batch of `bfv::Ciphertext`s that stays on the GPU between operations: `[batch][parts][rows][N]` u64, Ntt form,
/// plus the `level` bookkeeping of `Ciphertext` (ciphertext.rs:18-30).  Made by `upload` (or by an operation), consumed
/// by `HipMul::multiply_dev`, `HipKsk::{relinearize_dev, galois_dev}`, `CtxView::ciphertexts_switch_to_level_dev`;
/// `download` is the only point that waits.  (`seed` is dropped on upload exactly as every evaluation drops it,
/// ops/mod.rs:66.)
pub struct DeviceCiphertexts {
    buf: DeviceBuffer,
    pub batch: usize,
    pub parts: usize,
    pub rows: usize,
    pub degree: usize,
    pub level: usize,
}
impl DeviceCiphertexts {
    pub fn alloc(device: i32, batch: usize, parts: usize, rows: usize, degree: usize, level: usize) -> Result<Self> {
        Ok(Self { buf: DeviceBuffer::alloc(device, batch * parts * rows * degree)?, batch, parts, rows, degree, level })
    }
    /// The same on `stream`'s allocation order (results of the `_dev` operations).
    pub fn alloc_on(device: i32, batch: usize, parts: usize, rows: usize, degree: usize, level: usize, stream: &Stream) -> Result<Self> {
        Ok(Self { buf: DeviceBuffer::alloc_on(device, batch * parts * rows * degree, stream)?, batch, parts, rows, degree, level })
    }
    /// Frees the batch behind the work enqueued on `stream` (no device synchronisation).
    pub fn release_on(self, stream: &Stream) -> Result<()> { self.buf.release_on(stream) }
    pub fn words_per_ct(&self) -> usize { self.parts * self.rows * self.degree }
    pub fn buffer(&self) -> &DeviceBuffer { &self.buf }
    /// `flat`: the ciphertexts' polynomials' coefficients, concatenated `[batch][parts][rows][N]`.
    pub fn upload(device: i32, flat: &[u64], parts: usize, rows: usize, degree: usize, level: usize, stream: &Stream) -> Result<Self> {
        let batch = whole_batch("DeviceCiphertexts::upload", flat.len(), parts * rows * degree)?;
        let d = Self::alloc(device, batch, parts, rows, degree, level)?;
        d.buf.upload(flat, stream)?;
        Ok(d)
    }
    pub fn download(&self, stream: &Stream) -> Result<Vec<u64>> {
        let mut v = vec![0u64; self.buf.len()];
        self.buf.download(&mut v, stream)?;
        Ok(v)
    }
    /// `&Ciphertext + &Plaintext` (ops/mod.rs:71-108) over `ctx` (the ciphertexts' level): c0 + `pt`, `pt` the
    /// Delta-scaled form (`HipEncoder::encode_dev` with `scaled`), `[rows][N]` shared or `[batch][rows][N]`.
    pub fn add_plain_dev(&self, ctx: &CtxView<'_>, pt: &DeviceBuffer, stream: &Stream) -> Result<DeviceCiphertexts> {
        self.plain_dev("add_plain_dev", ctx, pt, false, stream)
    }
    /// `&Ciphertext - &Plaintext` (ops/mod.rs:166-203): c0 - `pt`.
    pub fn sub_plain_dev(&self, ctx: &CtxView<'_>, pt: &DeviceBuffer, stream: &Stream) -> Result<DeviceCiphertexts> {
        self.plain_dev("sub_plain_dev", ctx, pt, true, stream)
    }
    fn plain_dev(&self, what: &str, ctx: &CtxView<'_>, pt: &DeviceBuffer, subtract: bool, stream: &Stream) -> Result<DeviceCiphertexts> {
        let shared = plain_operand(what, ctx, self, pt)?;
        let out = Self::alloc_on(ctx.device(), self.batch, self.parts, self.rows, self.degree, self.level, stream)?;
        check(unsafe {
            ffi::fhe_bfv_add_plain_dev(ctx.as_ptr(), subtract as c_int, self.parts, self.buf.as_ptr(), pt.as_ptr(), shared as c_int,
                                       out.buf.as_mut_ptr(), self.batch, stream.as_ptr())
        })?;
        Ok(out)
    }
}
