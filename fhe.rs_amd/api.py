"""Host-side mirror of the reference types that sit on the hot path, as thin ctypes wrappers
over the C ABI (include/fhe_hip.h).  Names, argument meaning and error behaviour follow fhe.rs:

    Context, Scaler, Switcher                  fhe_math::rq            (crates/fhe-math/src/rq/)
    KeySwitchingKey, RelinearizationKey,
    GaloisKey, EvaluationKey, Multiplicator,
    BfvParameters                              fhe::bfv                (crates/fhe/src/bfv/)

Every compute method accepts either
  * a numpy uint64 array  -> host-pointer entry point (synchronous, returns a new array),
  * a torch CUDA tensor   -> `_dev` entry point on torch's current stream (device pointers;
    torch is used purely as the device allocator / stream provider), or
  * a `DeviceArray`       -> `_dev` entry point on the current `Stream`: buffers and streams that come from the C
    ABI itself (fhe_buf_alloc / fhe_stream_create), i.e. what a host without PyTorch -- the Rust shim, a C program --
    uses; results are DeviceArrays that stay resident until `.download()`.
Polynomials are `[..., L, N]` row-major exactly like `rq::Poly`; leading dims are the batch.
Nothing in this module computes on the CPU: without the HIP library it cannot be imported.
"""
import ctypes as C
import secrets

import numpy as np

from . import _lib
from ._lib import check, FheError  # noqa: F401  (re-exported)

try:  # torch is only the device allocator / stream provider
    import torch
except Exception:  # pragma: no cover
    torch = None


import threading

_tls = threading.local()


class Stream:
    """A HIP stream handed out by the C ABI (fhe_stream_create).  `with Stream(dev) as s:` makes it the stream every
    `_dev` call of this thread runs on (instead of torch's current stream)."""

    def __init__(self, device=0, _foreign=None):
        if _foreign is not None:     # a hipStream_t the host made itself: used, never destroyed here
            self._h, self.device, self._owned = C.c_void_p(_foreign), device, False
            return
        h = C.c_void_p()
        check(_lib.lib().fhe_stream_create(device, C.byref(h)))
        self._h, self.device, self._owned = h, device, True

    @classmethod
    def foreign(cls, handle, device=0):
        """Wraps a HIP stream that the host created (and will destroy) itself -- what a torch / hip-rs host passes."""
        return cls(device, _foreign=int(handle))

    @property
    def handle(self):
        return self._h

    def synchronize(self):
        check(_lib.lib().fhe_stream_sync(self._h))

    def destroy(self):
        if self._h is not None and self._owned:
            check(_lib.lib().fhe_stream_destroy(self._h))
        self._h = None

    def __enter__(self):
        self._prev = getattr(_tls, "stream", None)
        _tls.stream = self
        return self

    def __exit__(self, *exc):
        _tls.stream = self._prev
        return False

    def __del__(self):
        if getattr(self, "_h", None) is not None and getattr(self, "_owned", False) and _lib._lib is not None:
            _lib._lib.fhe_stream_destroy(self._h)


class DeviceArray:
    """A device buffer owned through the C ABI (fhe_buf_alloc, or fhe_buf_alloc_async inside `with Stream`), with a shape: the device-resident shadow of a
    `[..., L, N]` coefficient array (`rq::Poly.coefficients`) for hosts that do not bring their own HIP allocator."""

    def __init__(self, shape, device=0, itemsize=8, _ptr=None, _base=None):
        self.shape = tuple(int(d) for d in shape)
        self.device, self.itemsize = device, itemsize
        self._base = _base
        self._astream = None
        self._other_stream_use = False    # (set by _note_use: some call used this array on another stream)
        if _ptr is None:
            h = C.c_void_p()
            st = getattr(_tls, "stream", None)
            if st is not None and st.device == device and st.handle is not None:
                # inside `with Stream(...)`: stream-ordered allocation (no device synchronisation when results are
                # allocated and dropped per call); the array remembers its stream for the matching free
                check(_lib.lib().fhe_buf_alloc_async(device, max(self.nbytes, 1), st.handle, C.byref(h)))
                self._astream = st
            else:
                check(_lib.lib().fhe_buf_alloc(device, max(self.nbytes, 1), C.byref(h)))
            self._p = h.value
        else:
            self._p = _ptr

    @classmethod
    def from_numpy(cls, a, device=0):
        a = np.ascontiguousarray(a)
        d = cls(a.shape, device, a.dtype.itemsize)
        check(_lib.lib().fhe_buf_upload(C.c_void_p(d._p), a.ctypes.data_as(C.c_void_p), a.nbytes, _stream()))
        return d

    @property
    def nbytes(self):
        n = self.itemsize
        for d in self.shape:
            n *= d
        return n

    # the few members the wrappers below use on torch tensors
    is_cuda = True

    def is_contiguous(self):
        return True

    def contiguous(self):
        return self

    def element_size(self):
        return self.itemsize

    def data_ptr(self):
        return self._p

    def numel(self):
        return self.nbytes // self.itemsize

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, i):
        """View of the i-th slice along the first dimension (no copy; keeps the parent alive)."""
        if not isinstance(i, int) or not self.shape:
            raise TypeError("DeviceArray supports integer indexing of the first dimension only")
        if i < 0:
            i += self.shape[0]
        if not 0 <= i < self.shape[0]:
            raise IndexError(i)
        sub = self.nbytes // self.shape[0]
        return DeviceArray(self.shape[1:], self.device, self.itemsize, _ptr=self._p + i * sub, _base=self if self._base is None else self._base)

    def reshape(self, *shape):
        shape = shape[0] if len(shape) == 1 and isinstance(shape[0], (tuple, list)) else shape
        v = DeviceArray(shape, self.device, self.itemsize, _ptr=self._p, _base=self if self._base is None else self._base)
        if v.nbytes != self.nbytes:
            raise ValueError("reshape changes the size")
        return v

    def download(self):
        """Waits for the current stream and returns the contents as a numpy array (uint64 / uint8)."""
        out = np.empty(self.shape, dtype=np.uint64 if self.itemsize == 8 else np.uint8)
        check(_lib.lib().fhe_buf_download(out.ctypes.data_as(C.c_void_p), C.c_void_p(self._p), self.nbytes, _stream()))
        return out

    def _note_use(self):
        """Called for every engine call that takes this array: remembers whether any of them ran on a stream other
        than the allocating one (an array used inside another `with Stream` block and dropped after
        returning to its own stream must not be freed in the allocating stream's order)."""
        root = self if self._base is None else self._base   # (not `or`: __len__ makes an empty base falsy)
        if root._astream is not None and getattr(_tls, "stream", None) is not root._astream:
            root._other_stream_use = True

    def _release(self, L):
        st = getattr(self, "_astream", None)
        # stream-ordered free only when EVERY use of the array was enqueued on the allocating stream and that stream is
        # still the current one.  Otherwise the synchronous free, which waits for the device (ADVICE r03 / r04:
        # hipFreeAsync on the allocating stream could hand the block back while another stream still read it).
        if (st is not None and st.handle is not None and getattr(_tls, "stream", None) is st
                and not getattr(self, "_other_stream_use", False)):
            return L.fhe_buf_free_async(C.c_void_p(self._p), st.handle)
        return L.fhe_buf_free(C.c_void_p(self._p))                        # (hipFree: waits for the device)

    def free(self):
        if self._base is None and self._p is not None:
            check(self._release(_lib.lib()))
        self._p = None

    def __del__(self):
        if getattr(self, "_base", None) is None and getattr(self, "_p", None) is not None and _lib._lib is not None:
            self._release(_lib._lib)


def _is_dev(x):
    return isinstance(x, DeviceArray) or (torch is not None and isinstance(x, torch.Tensor))


def _empty_dev(ref, shape, itemsize=8, zero=False):
    """An uninitialised (or zeroed) device array of `shape` next to `ref` (same allocator, same device)."""
    if isinstance(ref, DeviceArray):
        d = DeviceArray(shape, ref.device, itemsize)
        if zero:
            check(_lib.lib().fhe_buf_zero_async(C.c_void_p(d._p), d.nbytes, _stream()))
        return d
    dt = torch.int64 if itemsize == 8 else torch.uint8
    return (torch.zeros if zero else torch.empty)(tuple(shape), dtype=dt, device=ref.device)


def _np(x):
    a = np.ascontiguousarray(np.asarray(x, dtype=np.uint64))
    return a


def _ptr(a):
    return a.ctypes.data_as(_lib.u64p)


def _dptr(t):
    if not t.is_cuda or not t.is_contiguous() or t.element_size() != 8:
        raise ValueError("device buffers must be contiguous 8-byte CUDA tensors")
    if isinstance(t, DeviceArray):
        t._note_use()
    return C.c_void_p(t.data_ptr())


def _dptr8(t):
    if not t.is_cuda or not t.is_contiguous() or t.element_size() != 1:
        raise ValueError("wire buffers must be contiguous uint8 CUDA tensors")
    if isinstance(t, DeviceArray):
        t._note_use()
    return C.c_void_p(t.data_ptr())


def _stream():
    s = getattr(_tls, "stream", None)
    if s is not None:
        return s.handle
    if torch is not None and torch.cuda.is_available():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return None   # the device's null stream


def _limbs(x: int):
    out = []
    while True:
        out.append(x & 0xFFFFFFFFFFFFFFFF)
        x >>= 64
        if x == 0:
            break
    return np.array(out, dtype=np.uint64)


def _to_limbs(values, wt):
    """Python ints [...] (a list or an object array) -> uint64 [..., wt] little-endian limbs."""
    v = np.asarray(values, dtype=object)
    flat = [int(x) for x in v.reshape(-1)]
    if any(x < 0 or x >> (64 * wt) for x in flat):
        raise FheError(-1, "values must be in [0, 2^%d)" % (64 * wt))
    out = np.array([[(x >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(wt)] for x in flat], dtype=np.uint64)
    return out.reshape(tuple(v.shape) + (wt,))


def _from_limbs(a):
    """uint64 [..., wt] limbs -> an object array [...] of Python ints."""
    a = np.asarray(a, dtype=np.uint64).astype(object)
    return sum(a[..., k] << (64 * k) for k in range(a.shape[-1]))


class Context:
    """rq::Context (crates/fhe-math/src/rq/context.rs:9-92)."""

    def __init__(self, moduli, degree, device=0, tables=None, _handle=None, _owner=None):
        self._owner = _owner
        if _handle is not None:
            self._h = _handle
        else:
            m = _np(moduli)
            h = C.c_void_p()
            if tables is None:
                args = [None] * 6
                keep = []
            else:
                keep = [_np(tables[k]) for k in ("omegas", "omegas_shoup", "zetas_inv", "zetas_inv_shoup",
                                                 "size_inv", "size_inv_shoup")]
                args = [_ptr(a) for a in keep]
            check(_lib.lib().fhe_ctx_create(device, degree, len(m), _ptr(m), *args, C.byref(h)))
            self._h = h
        L = _lib.lib()
        self.degree = L.fhe_ctx_degree(self._h)
        self.nmoduli = L.fhe_ctx_nmoduli(self._h)
        self.device = L.fhe_ctx_device(self._h)
        mm = np.zeros(self.nmoduli, dtype=np.uint64)
        check(L.fhe_ctx_moduli(self._h, _ptr(mm)))
        self.moduli = [int(x) for x in mm]

    def __del__(self):
        if self._owner is None and getattr(self, "_h", None) is not None and _lib._lib is not None:
            _lib._lib.fhe_ctx_destroy(self._h)

    def at_level(self, level):
        """Context::context_at_level."""
        h = C.c_void_p()
        check(_lib.lib().fhe_ctx_at_level(self._h, level, C.byref(h)))
        return Context(None, None, _handle=h, _owner=self._owner or self)

    def niterations_to(self, other):
        n = C.c_size_t()
        check(_lib.lib().fhe_ctx_niterations_to(self._h, other._h, C.byref(n)))
        return n.value

    def table(self, which):
        shape = (self.nmoduli, self.degree) if which < 4 else ((self.nmoduli,) if which < 6 else (max(self.nmoduli - 1, 0),))
        out = np.zeros(max(int(np.prod(shape)), 1), dtype=np.uint64)
        check(_lib.lib().fhe_ctx_get_table(self._h, which, _ptr(out)))
        return out[: int(np.prod(shape))].reshape(shape)

    # -- helpers ------------------------------------------------------------------
    def _batch(self, x, rows=None):
        rows = self.nmoduli if rows is None else rows
        shp = tuple(x.shape)
        if len(shp) < 2 or shp[-1] != self.degree or shp[-2] != rows:
            raise ValueError(f"expected [..., {rows}, {self.degree}], got {shp}")
        b = 1
        for d in shp[:-2]:
            b *= d
        return b

    def _unary_inplace(self, host_fn, dev_fn, x):
        L = _lib.lib()
        if _is_dev(x):
            check(getattr(L, dev_fn)(self._h, _dptr(x), self._batch(x), _stream()))
            return x
        a = _np(x).copy()
        check(getattr(L, host_fn)(self._h, _ptr(a), self._batch(a)))
        return a

    def _binary_inplace(self, host_fn, dev_fn, x, y):
        L = _lib.lib()
        if _is_dev(x):
            check(getattr(L, dev_fn)(self._h, _dptr(x), _dptr(y), self._batch(x), _stream()))
            return x
        a, b = _np(x).copy(), _np(y)
        if a.shape != b.shape:
            raise ValueError("shape mismatch")
        check(getattr(L, host_fn)(self._h, _ptr(a), _ptr(b), self._batch(a)))
        return a

    # -- NttOperator / Poly representation changes (rq/mod.rs:335-354) ---------------
    def ntt_forward(self, polys):
        return self._unary_inplace("fhe_ntt_forward", "fhe_ntt_forward_dev", polys)

    def ntt_backward(self, polys):
        return self._unary_inplace("fhe_ntt_backward", "fhe_ntt_backward_dev", polys)

    # -- Rq wire format (rq/convert.rs:17-99, zq/mod.rs:783-793) ------------------------------
    @property
    def serialized_size(self):
        return int(_lib.lib().fhe_poly_serialized_size(self._h))

    def serialize(self, polys, from_ntt=False):
        """[..., L, N] -> uint8 [..., serialized_size]: the `coefficients` payload of the Rq message."""
        L = _lib.lib()
        b = self._batch(polys)
        oshape = tuple(polys.shape[:-2]) + (self.serialized_size,)
        if _is_dev(polys):
            out = _empty_dev(polys, oshape, 1)
            check(L.fhe_poly_serialize_dev(self._h, _dptr(polys), _dptr8(out), b, 1 if from_ntt else 0, _stream()))
            return out
        x = _np(polys)
        out = np.zeros(oshape, dtype=np.uint8)
        check(L.fhe_poly_serialize(self._h, _ptr(x), out.ctypes.data_as(_lib.u8p), b, 1 if from_ntt else 0))
        return out

    def deserialize(self, data, to_ntt=False):
        """uint8 [..., serialized_size] -> [..., L, N]."""
        L = _lib.lib()
        if data.shape[-1] != self.serialized_size:
            raise FheError(-1, "InvalidCoefficientCount")
        oshape = tuple(data.shape[:-1]) + (self.nmoduli, self.degree)
        b = 1
        for d in data.shape[:-1]:
            b *= int(d)
        if _is_dev(data):
            out = _empty_dev(data, oshape)
            check(L.fhe_poly_deserialize_dev(self._h, _dptr8(data.contiguous()), _dptr(out), b, 1 if to_ntt else 0, _stream()))
            return out
        x = np.ascontiguousarray(np.asarray(data, dtype=np.uint8))
        out = np.zeros(oshape, dtype=np.uint64)
        check(L.fhe_poly_deserialize(self._h, x.ctypes.data_as(_lib.u8p), _ptr(out), b, 1 if to_ntt else 0))
        return out

    # -- rq/ops.rs ----------------------------------------------------------------------
    def add(self, a, b):
        return self._binary_inplace("fhe_poly_add", "fhe_poly_add_dev", a, b)

    def sub(self, a, b):
        return self._binary_inplace("fhe_poly_sub", "fhe_poly_sub_dev", a, b)

    def mul(self, a, b):
        return self._binary_inplace("fhe_poly_mul", "fhe_poly_mul_dev", a, b)

    def neg(self, a):
        return self._unary_inplace("fhe_poly_neg", "fhe_poly_neg_dev", a)

    def mul_shoup(self, a, b, b_shoup):
        L = _lib.lib()
        if _is_dev(a):
            check(L.fhe_poly_mul_shoup_dev(self._h, _dptr(a), _dptr(b), _dptr(b_shoup), self._batch(a), _stream()))
            return a
        x, y, ys = _np(a).copy(), _np(b), _np(b_shoup)
        check(L.fhe_poly_mul_shoup(self._h, _ptr(x), _ptr(y), _ptr(ys), self._batch(x)))
        return x

    def shoup(self, a):
        """Poly::compute_coefficients_shoup (host, setup-time)."""
        x = _np(a)
        out = np.zeros_like(x)
        check(_lib.lib().fhe_poly_shoup(self._h, _ptr(x), _ptr(out), self._batch(x)))
        return out

    def substitute(self, exponent, polys, ntt=True):
        """Poly::substitute with SubstitutionExponent::new(ctx, exponent)."""
        L = _lib.lib()
        if _is_dev(polys):
            out = _empty_dev(polys, polys.shape)
            check(L.fhe_poly_substitute_dev(self._h, exponent, _dptr(polys), _dptr(out), self._batch(polys),
                                            1 if ntt else 0, _stream()))
            return out
        x = _np(polys)
        out = np.zeros_like(x)
        check(L.fhe_poly_substitute(self._h, exponent, _ptr(x), _ptr(out), self._batch(x), 1 if ntt else 0))
        return out

    def switch_down(self, polys):
        """Poly::<PowerBasis>::switch_down: [..., L, N] -> [..., L-1, N]."""
        L = _lib.lib()
        b = self._batch(polys)
        oshape = tuple(polys.shape[:-2]) + (self.nmoduli - 1, self.degree)
        if _is_dev(polys):
            out = _empty_dev(polys, oshape)
            check(L.fhe_poly_switch_down_dev(self._h, _dptr(polys), _dptr(out), b, _stream()))
            return out
        x = _np(polys)
        out = np.zeros(oshape if self.nmoduli > 1 else (1,), dtype=np.uint64)
        check(L.fhe_poly_switch_down(self._h, _ptr(x), _ptr(out), b))
        return out

    def ciphertext_switch_down(self, ct):
        """Ciphertext::switch_down: [..., parts, L, N] Ntt -> [..., parts, L-1, N] Ntt."""
        L = _lib.lib()
        parts = ct.shape[-3]
        b = self._batch(ct) // parts
        oshape = tuple(ct.shape[:-2]) + (self.nmoduli - 1, self.degree)
        if _is_dev(ct):
            out = _empty_dev(ct, oshape)
            check(L.fhe_bfv_switch_down_dev(self._h, parts, _dptr(ct), _dptr(out), b, _stream()))
            return out
        x = _np(ct)
        out = np.zeros(oshape if self.nmoduli > 1 else (1,), dtype=np.uint64)
        check(L.fhe_bfv_switch_down(self._h, parts, _ptr(x), _ptr(out), b))
        return out

    def switch_down_to(self, polys, to_ctx):
        """Poly::<PowerBasis>::switch_down_to (rq/mod.rs:498-507): [..., L, N] -> [..., to.L, N] in one call."""
        L = _lib.lib()
        b = self._batch(polys)
        oshape = tuple(polys.shape[:-2]) + (to_ctx.nmoduli, self.degree)
        if _is_dev(polys):
            out = _empty_dev(polys, oshape)
            check(L.fhe_poly_switch_down_to_dev(self._h, to_ctx._h, _dptr(polys), _dptr(out), b, _stream()))
            return out
        x = _np(polys)
        out = np.zeros(oshape, dtype=np.uint64)
        check(L.fhe_poly_switch_down_to(self._h, to_ctx._h, _ptr(x), _ptr(out), b))
        return out

    def ciphertext_switch_to_level(self, ct, levels):
        """Ciphertext::switch_to_level (bfv/ciphertext.rs:164-183), `levels` = target_level - level:
        [..., parts, L, N] Ntt -> [..., parts, L-levels, N] Ntt with one inverse / forward transform pair."""
        L = _lib.lib()
        parts = ct.shape[-3]
        b = self._batch(ct) // parts
        oshape = tuple(ct.shape[:-2]) + (max(self.nmoduli - levels, 0), self.degree)
        if _is_dev(ct):
            out = _empty_dev(ct, oshape if self.nmoduli > levels else (1,))
            check(L.fhe_bfv_switch_to_level_dev(self._h, levels, parts, _dptr(ct), _dptr(out), b, _stream()))
            return out
        x = _np(ct)
        out = np.zeros(oshape if self.nmoduli > levels else (1,), dtype=np.uint64)
        check(L.fhe_bfv_switch_to_level(self._h, levels, parts, _ptr(x), _ptr(out), b))
        return out

    def dot_product_scalar(self, cts, pts):
        """bfv::dot_product_scalar (crates/fhe/src/bfv/ops/dot_product.rs:54-180):
        cts [..., count, parts, L, N] and pts [..., count, L, N] (`Plaintext::poly_ntt`), or either
        without the leading batch dims (then shared by the batch) -> [..., parts, L, N].
        With parts == 1 this is fhe_math::rq::dot_product (rq/ops.rs:449-570)."""
        L = _lib.lib()
        cb, pb = tuple(cts.shape[:-4]), tuple(pts.shape[:-3])
        count, parts = cts.shape[-4], cts.shape[-3]
        if pts.shape[-3] != count:
            raise FheError(-1, "DotProductLengthMismatch")
        bshape = cb if len(cb) >= len(pb) else pb
        batch = 1
        for d in bshape:
            batch *= d
        cts_shared = 1 if (cb != bshape) else 0
        pts_shared = 1 if (pb != bshape) else 0
        oshape = bshape + (parts, self.nmoduli, self.degree)
        if _is_dev(cts):
            out = _empty_dev(cts, oshape)
            check(L.fhe_bfv_dot_product_scalar_dev(self._h, parts, count, _dptr(cts), cts_shared, _dptr(pts), pts_shared,
                                                   _dptr(out), batch, _stream()))
            return out
        x, y = _np(cts), _np(pts)
        out = np.zeros(oshape, dtype=np.uint64)
        check(L.fhe_bfv_dot_product_scalar(self._h, parts, count, _ptr(x), cts_shared, _ptr(y), pts_shared, _ptr(out), batch))
        return out

    def mul_plain(self, ct, pt):
        """`&Ciphertext * &Plaintext` (ops/mod.rs:229-257): ct [..., parts, L, N] times pt [..., L, N]
        (or [L, N] shared by the batch)."""
        L = _lib.lib()
        parts = ct.shape[-3]
        batch = self._batch(ct) // parts
        shared = 1 if len(pt.shape) == 2 and len(ct.shape) > 3 else 0
        if _is_dev(ct):
            out = _empty_dev(ct, ct.shape)
            check(L.fhe_bfv_mul_plain_dev(self._h, parts, _dptr(ct), _dptr(pt), shared, _dptr(out), batch, _stream()))
            return out
        x, y = _np(ct), _np(pt)
        out = np.zeros_like(x)
        check(L.fhe_bfv_mul_plain(self._h, parts, _ptr(x), _ptr(y), shared, _ptr(out), batch))
        return out

    def _add_plain(self, ct, pt, subtract):
        L = _lib.lib()
        parts = ct.shape[-3]
        batch = self._batch(ct) // parts
        shared = 1 if len(pt.shape) == 2 and len(ct.shape) > 3 else 0
        if _is_dev(ct):
            out = _empty_dev(ct, ct.shape)
            check(L.fhe_bfv_add_plain_dev(self._h, subtract, parts, _dptr(ct), _dptr(pt), shared, _dptr(out), batch,
                                          _stream()))
            return out
        dev = max(self.device, 0)
        x, y = DeviceArray.from_numpy(_np(ct), dev), DeviceArray.from_numpy(_np(pt), dev)
        check(L.fhe_bfv_add_plain_dev(self._h, subtract, parts, _dptr(x), _dptr(y), shared, _dptr(x), batch, _stream()))
        return x.download()

    def add_plain(self, ct, pt):
        """`&Ciphertext + &Plaintext` (ops/mod.rs:71-108): ct [..., parts, L, N] Ntt plus pt [..., L, N] (or [L, N]
        shared by the batch) in its Delta-scaled form (`Encoder.encode(..., scaled=True)`): c0 + pt, other parts
        unchanged."""
        return self._add_plain(ct, pt, 0)

    def sub_plain(self, ct, pt):
        """`&Ciphertext - &Plaintext` (ops/mod.rs:166-203): c0 - pt, other parts unchanged."""
        return self._add_plain(ct, pt, 1)

    def random_from_seed(self, seeds):
        """Poly::<Ntt>::random_from_seed (rq/mod.rs:276-292) per 32-byte seed: seeds [batch, 32] uint8 ->
        [batch, L, N]; numpy in -> numpy out, torch CUDA uint8 tensor in -> CUDA tensor out.

        PARITY UNPINNED (as include/fhe_hip.h says for fhe_poly_from_seed): SHA-256 and the ChaCha block function are
        known-answer tested, but the generator's word layout and the `Uniform` rejection sampler restate
        rand_chacha 0.10 / rand 0.10 -- crates the reference does not vendor -- and no vector from a real fhe.rs run
        exists here.  The test-side oracle was written from the same reading, so agreement with it does not pin the
        stream either.  A host that must interoperate with seeded ciphertexts made by fhe.rs expands c1 itself and
        uploads it (or first checks one (seed, modulus) pair against its Rust build)."""
        L = _lib.lib()
        if _is_dev(seeds):
            b = int(seeds.numel() // 32)
            out = _empty_dev(seeds, (b, self.nmoduli, self.degree))
            check(L.fhe_poly_from_seed_dev(self._h, _dptr8(seeds), _dptr(out), b, _stream()))
            return out
        sd = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint8)).reshape(-1, 32)
        out = np.zeros((sd.shape[0], self.nmoduli, self.degree), dtype=np.uint64)
        check(L.fhe_poly_from_seed(self._h, sd.ctypes.data_as(_lib.u8p), _ptr(out), sd.shape[0]))
        return out

    def sample_small(self, seeds, variance, ntt=True):
        """Poly::small (rq/mod.rs:298-330) of ChaCha8Rng::from_seed(seed) per 32-byte seed (fhe_bfv_sample_small_dev):
        seeds [batch, 32] uint8 -> [batch, L, N], Ntt (ntt=True) or PowerBasis.  numpy seeds -> numpy out; device seeds
        -> a device array.  The device buffers this wrapper stages host seeds and samples through are cleared before
        they are freed; what it returns, and device seeds the caller passes, are the caller's to clear."""
        staged = []
        try:
            sd, b, own = _seeds(seeds, 1, self.device)
            if own:
                staged.append(sd)
            host = not _is_dev(seeds)
            out = DeviceArray((b, self.nmoduli, self.degree), max(self.device, 0)) if host else _empty_dev(
                seeds, (b, self.nmoduli, self.degree))
            if host:
                staged.append(out)
            check(_lib.lib().fhe_bfv_sample_small_dev(self._h, variance, _dptr8(sd), 1 if ntt else 0, _dptr(out), b,
                                                      _stream()))
            return out.download() if host else out
        finally:
            _wipe(staged)

    # -- RnsContext::lift and the centered bit length (rns/mod.rs:138-143, secret_key.rs:88-95) -----
    @property
    def lift_limbs(self):
        """W = ceil(bitlen(q) / 64): the u64 limbs per coefficient `lift` writes."""
        return _lib.lib().fhe_ctx_lift_limbs(self._h)

    def lift(self, polys):
        """RnsContext::lift per coefficient (fhe_poly_lift_dev), as Vec<BigUint>::from(&Poly) applies it: polys
        [..., L, N] canonical residues in any representation -> the integers in [0, q).  numpy in -> an object array
        [..., N] of Python ints; a device array in -> a device array [..., N, W] of little-endian u64 limbs."""
        b, w = self._batch(polys), self.lift_limbs
        lead = tuple(int(d) for d in polys.shape[:-2])
        if _is_dev(polys):
            out = _empty_dev(polys, lead + (self.degree, w))
            check(_lib.lib().fhe_poly_lift_dev(self._h, _dptr(polys), _dptr(out), b, _stream()))
            return out
        x = DeviceArray.from_numpy(_np(polys), max(self.device, 0))
        out = DeviceArray(lead + (self.degree, w), x.device)
        check(_lib.lib().fhe_poly_lift_dev(self._h, _dptr(x), _dptr(out), b, _stream()))
        limbs = out.download().astype(object)
        ints = limbs[..., 0]
        for k in range(1, w):
            ints = ints + (limbs[..., k] << (64 * k))
        return ints

    def centered_bits(self, polys):
        """max over the coefficients of min(bits(x), bits(q - x)), x the lifted coefficient (fhe_poly_centered_bits_dev;
        the loop of SecretKey::measure_noise): polys [..., L, N] -> [...] uint64, one value per polynomial.  numpy in ->
        numpy out (an int without batch dimensions); a device array in -> a device array."""
        b = self._batch(polys)
        lead = tuple(int(d) for d in polys.shape[:-2])
        if _is_dev(polys):
            out = _empty_dev(polys, lead or (1,))
            check(_lib.lib().fhe_poly_centered_bits_dev(self._h, _dptr(polys), _dptr(out), b, _stream()))
            return out
        x = DeviceArray.from_numpy(_np(polys), max(self.device, 0))
        out = DeviceArray(lead or (1,), x.device)
        check(_lib.lib().fhe_poly_centered_bits_dev(self._h, _dptr(x), _dptr(out), b, _stream()))
        r = out.download()
        return r if lead else int(r[0])

    def synth_uniform(self, seed, ct0, part0, nparts, batch):
        """Device-side synthetic residues [batch, nparts, L, N] (bench / parity inputs)."""
        shape = (batch, nparts, self.nmoduli, self.degree)
        if getattr(_tls, "stream", None) is not None or torch is None or not torch.cuda.is_available():
            out = DeviceArray(shape, max(self.device, 0))   # a Stream is current: stay on the ABI's own allocator
        else:
            out = torch.empty(shape, dtype=torch.int64, device=f"cuda:{self.device}")
        check(_lib.lib().fhe_synth_uniform_dev(self._h, seed, ct0, part0, nparts, _dptr(out), batch, _stream()))
        return out


class Scaler:
    """rq::scaler::Scaler (crates/fhe-math/src/rq/scaler.rs:18-127); the scaling factor is
    ScalingFactor::new(numerator, denominator) given as Python ints."""

    def __init__(self, from_ctx, to_ctx, numerator=1, denominator=1, _handle=None, _owner=None):
        self.from_ctx, self.to_ctx = from_ctx, to_ctx
        self._owner = _owner
        if _handle is not None:
            self._h = _handle
        else:
            n, d = _limbs(numerator), _limbs(denominator)
            h = C.c_void_p()
            check(_lib.lib().fhe_scaler_create(from_ctx._h, to_ctx._h, _ptr(n), len(n), _ptr(d), len(d), C.byref(h)))
            self._h = h
        self.number_common_moduli = _lib.lib().fhe_scaler_number_common_moduli(self._h)

    @classmethod
    def from_constants(cls, from_ctx, to_ctx, number_common_moduli, is_one, k):
        """All RnsScaler fields supplied by the caller (what a Rust host already holds)."""
        keep = {n: _np(k[n]) for n in ("gamma", "gamma_shoup", "omega", "omega_shoup", "theta_omega_lo",
                                        "theta_omega_hi", "theta_garner_lo", "theta_garner_hi")}
        sign = np.ascontiguousarray(np.asarray(k["theta_omega_sign"], dtype=np.uint8))
        h = C.c_void_p()
        check(_lib.lib().fhe_scaler_create_from_constants(
            from_ctx._h, to_ctx._h, number_common_moduli, 1 if is_one else 0,
            _ptr(keep["gamma"]), _ptr(keep["gamma_shoup"]), _ptr(keep["omega"]), _ptr(keep["omega_shoup"]),
            int(k["theta_gamma_lo"]), int(k["theta_gamma_hi"]), 1 if k["theta_gamma_sign"] else 0,
            _ptr(keep["theta_omega_lo"]), _ptr(keep["theta_omega_hi"]), sign.ctypes.data_as(_lib.u8p),
            _ptr(keep["theta_garner_lo"]), _ptr(keep["theta_garner_hi"]), int(k["theta_garner_shift"]), C.byref(h)))
        return cls(from_ctx, to_ctx, _handle=h)

    def __del__(self):
        if self._owner is None and getattr(self, "_h", None) is not None and _lib._lib is not None:
            _lib._lib.fhe_scaler_destroy(self._h)

    def constants(self, which):
        nf, nt = self.from_ctx.nmoduli, self.to_ctx.nmoduli
        size = {0: nt, 1: nt, 2: nt * nf, 3: nt * nf, 4: nf, 5: nf, 6: nf, 7: nf, 8: nf, 9: 5}[which]
        out = np.zeros(size, dtype=np.uint64)
        check(_lib.lib().fhe_scaler_get_constants(self._h, which, _ptr(out)))
        return out

    def scale(self, polys, ntt):
        """Scaler::scale == Poly::scale(&scaler): [..., Lfrom, N] -> [..., Lto, N]."""
        L = _lib.lib()
        b = self.from_ctx._batch(polys)
        oshape = tuple(polys.shape[:-2]) + (self.to_ctx.nmoduli, self.to_ctx.degree)
        if _is_dev(polys):
            out = _empty_dev(polys, oshape, zero=True)
            check(L.fhe_poly_scale_dev(self._h, _dptr(polys), _dptr(out), b, 1 if ntt else 0, _stream()))
            return out
        x = _np(polys)
        out = np.zeros(oshape, dtype=np.uint64)
        check(L.fhe_poly_scale(self._h, _ptr(x), _ptr(out), b, 1 if ntt else 0))
        return out


class Switcher(Scaler):
    """rq::switcher::Switcher (crates/fhe-math/src/rq/switcher.rs:11-26)."""

    def __init__(self, from_ctx, to_ctx):
        h = C.c_void_p()
        check(_lib.lib().fhe_switcher_create(from_ctx._h, to_ctx._h, C.byref(h)))
        super().__init__(from_ctx, to_ctx, _handle=h)

    def switch(self, polys, ntt=False):
        return self.scale(polys, ntt)


class KeySwitchingKey:
    """bfv::KeySwitchingKey (crates/fhe/src/bfv/keys/key_switching_key.rs:22-46): c0, c1 are
    `[ndigits, Lk, N]` NttShoup polynomials over ctx_ksk; Shoup twins are optional."""

    def __init__(self, ctx_ciphertext, ctx_ksk, c0, c1, c0_shoup=None, c1_shoup=None, log_base=0):
        self.ctx_ciphertext, self.ctx_ksk, self.log_base = ctx_ciphertext, ctx_ksk, log_base
        L = _lib.lib()
        h = C.c_void_p()
        if _is_dev(c0):
            nd = c0.shape[0]
            check(L.fhe_ksk_create_dev(ctx_ciphertext._h, ctx_ksk._h, nd, _dptr(c0), _dptr(c1), log_base, _stream(),
                                       C.byref(h)))
        else:
            a0, a1 = _np(c0), _np(c1)
            nd = a0.shape[0]
            s0 = _np(c0_shoup) if c0_shoup is not None else None
            s1 = _np(c1_shoup) if c1_shoup is not None else None
            check(L.fhe_ksk_create(ctx_ciphertext._h, ctx_ksk._h, nd, _ptr(a0), _ptr(s0) if s0 is not None else None,
                                   _ptr(a1), _ptr(s1) if s1 is not None else None, log_base, C.byref(h)))
        self.ndigits = nd
        self._h = h
        forced = getattr(_tls, "ks_forced_mode", (0, 0))   # (tests and A/B tools: keys made inside `forced_mode`)
        if forced != (0, 0):
            self.set_mode(*forced)

    @classmethod
    def forced_mode(cls, mode, w_budget=0):
        """Context manager for TEST code: keys created inside it BY THIS THREAD take `mode` (the parity suites run their
        key-switch cases once per evaluation strategy this way).  Thread-local, restored on exit; the library itself
        has no process-wide switch, and product code sets the mode per key (`set_mode`)."""
        import contextlib

        @contextlib.contextmanager
        def cm():
            old = getattr(_tls, "ks_forced_mode", (0, 0))
            _tls.ks_forced_mode = (int(mode), int(w_budget))
            try:
                yield
            finally:
                _tls.ks_forced_mode = old
        return cm()

    @classmethod
    def _adopt(cls, ctx_ciphertext, ctx_ksk, handle, seeds, index):
        """A handle made by one of the generation entry points; `seeds[index]` is its public seed K (device)."""
        self = cls.__new__(cls)
        self.ctx_ciphertext, self.ctx_ksk = ctx_ciphertext, ctx_ksk
        self._h = C.c_void_p(handle)
        _, self.log_base = _ksk_digits(ctx_ciphertext, ctx_ksk)
        self.ndigits = _lib.lib().fhe_ksk_ndigits(self._h)   # (export sizes its arrays from the engine's count)
        self._seeds, self._seed_index = seeds, index
        forced = getattr(_tls, "ks_forced_mode", (0, 0))
        if forced != (0, 0):
            self.set_mode(*forced)
        return self

    @property
    def seed(self):
        """The key's public seed K (32 bytes) when it was generated on the device (KeySwitchingKey::new's `seed`),
        else None."""
        sd = getattr(self, "_seeds", None)
        if sd is None:
            return None
        row = sd[self._seed_index]
        return bytes(row.download() if isinstance(row, DeviceArray) else row.cpu().numpy())

    @classmethod
    def generate(cls, sk, from_ntt, ciphertext_level=0, ksk_level=0, seed=None):
        """KeySwitchingKey::new (key_switching_key.rs:71-236) on the device with rng = ChaCha8Rng::from_seed(seed):
        from_ntt [Lk, N] (one key) or [nkeys, Lk, N] is the reference's `from` in Ntt form over the key context (a
        device array; numpy is staged and cleared again), canonical residues (row j below q_j: not checked on the
        device, a larger word gives a key that is not canonical); seed: 32 bytes, or one per key (None: from `secrets`).
        Returns one key, or a list for a batch (fhe_ksk_generate_dev)."""
        L = _lib.lib()
        one = len(from_ntt.shape) == 2
        count = 1 if one else int(from_ntt.shape[0])
        staged = []
        try:
            f = from_ntt
            if not _is_dev(f):
                f = DeviceArray.from_numpy(_np(f), max(sk.params.device, 0))
                staged.append(f)
            keys = _keygen(sk, ciphertext_level, ksk_level, count, seed, lambda ct, kc, sd, ko, hs: (
                L.fhe_ksk_generate_dev(ct._h, kc._h, sk.params.variance, _dptr(sk.s_ntt), _dptr(f), _dptr8(sd), count,
                                       _dptr8(ko), _stream(), hs)))
        finally:
            _wipe(staged)
        return keys[0] if one else keys

    @classmethod
    def from_wire(cls, ctx_ciphertext, ctx_ksk, c0_bytes, c1_bytes=None, seeds=None, log_base=0):
        """KeySwitchingKey::try_convert_from(&KeySwitchingKeyProto) (key_switching_key.rs:387-482) on the device
        (fhe_ksk_load_wire_dev): c0_bytes uint8 [ndigits, ctx_ksk.serialized_size] -- `proto.c0[i].coefficients`
        concatenated -- or [nkeys, ndigits, size] for a batch of keys of one geometry; exactly one of c1_bytes (same
        shape) and seeds (`proto.seed`: 32 bytes per key, as `_seeds` takes them).  Device arrays are read in place, numpy
        is staged.  A coefficient >= q_j -> FheError(-1).  Returns a list of keys, ready on any stream."""
        L = _lib.lib()
        if (c1_bytes is None) == (seeds is None):
            raise FheError(-1, "exactly one of c1_bytes and seeds")
        nd = -(-(ctx_ksk.moduli[0] - 1).bit_length() // log_base) if log_base else ctx_ciphertext.nmoduli
        tail = (nd, ctx_ksk.serialized_size)
        dev = max(ctx_ksk.device, 0)

        def wire(b):
            if tuple(b.shape[-2:]) != tail or len(b.shape) > 3:
                raise FheError(-1, "wire bytes must be [ndigits, serialized_size] (%d, %d) per key" % tail)
            if not _is_dev(b):
                b = DeviceArray.from_numpy(np.ascontiguousarray(np.asarray(b, dtype=np.uint8)), dev)
            return b
        c0 = wire(c0_bytes)
        count = 1 if len(c0.shape) == 2 else int(c0.shape[0])
        c1 = sd = None
        if c1_bytes is not None:
            c1 = wire(c1_bytes)
            if tuple(c1.shape) != tuple(c0.shape):
                raise FheError(-1, "c0_bytes and c1_bytes differ in shape")
        else:
            sd, n, _own = _seeds(seeds, count, dev)   # (public seeds: kept with the keys, not wiped)
            if n != count:
                raise FheError(-1, "one seed per key: %d keys, %d seeds" % (count, n))
        hs = (C.c_void_p * count)()
        check(L.fhe_ksk_load_wire_dev(ctx_ciphertext._h, ctx_ksk._h, log_base, _dptr8(c0),
                                      _dptr8(c1) if c1 is not None else None, _dptr8(sd) if sd is not None else None,
                                      count, _stream(), hs))
        keys = []
        for i in range(count):
            k = cls._adopt(ctx_ciphertext, ctx_ksk, hs[i], sd.reshape(count, 32) if sd is not None else None, i)
            k.log_base = log_base
            keys.append(k)
        return keys

    def to_wire(self, seeded=None):
        """From<&KeySwitchingKey> for KeySwitchingKeyProto (key_switching_key.rs:365-385) on the device
        (fhe_ksk_serialize_dev): (c0_bytes, seed) when the key carries its seed (keys from `.generate` and from a
        seeded `from_wire`), else (c0_bytes, c1_bytes); the byte arrays are uint8 [ndigits, serialized_size] on the
        device, one row per `proto.c0[i].coefficients`.  seeded = False forces the explicit c1."""
        if seeded is None:
            seeded = self.seed is not None
        if seeded and self.seed is None:
            raise FheError(-1, "the key carries no seed")
        shape = (self.ndigits, self.ctx_ksk.serialized_size)
        c0 = _alloc(shape, self.ctx_ksk.device, itemsize=1)
        c1 = None if seeded else _alloc(shape, self.ctx_ksk.device, itemsize=1)
        check(_lib.lib().fhe_ksk_serialize_dev(self._h, _dptr8(c0), _dptr8(c1) if c1 is not None else None, _stream()))
        return c0, (self.seed if seeded else c1)

    def export(self):
        """(c0, c1, c0_shoup, c1_shoup), each [ndigits, Lk, N] on the device (fhe_ksk_export_dev): what a client sends
        to the server; `KeySwitchingKey(ctx_ct, ctx_ksk, c0, c1, ...)` of them is an equal key."""
        shape = (self.ndigits, self.ctx_ksk.nmoduli, self.ctx_ksk.degree)
        out = [_alloc(shape, self.ctx_ksk.device) for _ in range(4)]
        check(_lib.lib().fhe_ksk_export_dev(self._h, *[_dptr(x) for x in out], _stream()))
        return tuple(out)

    def __del__(self):
        if getattr(self, "_h", None) is not None and _lib._lib is not None:
            _lib._lib.fhe_ksk_destroy(self._h)

    AUTO, FUSED, UNFUSED, UNFUSED_SUB, FUSED_SUB = 0, 1, 2, 3, 4

    def set_mode(self, mode, w_budget=0):
        """How every key switch through this handle is evaluated (fhe_ksk_set_mode): AUTO, FUSED, UNFUSED (batched
        digit transforms + streaming lazy MAC), UNFUSED_SUB, FUSED_SUB (N >= 32768 on 8192-point sub-blocks);
        `w_budget` bytes of transformed rows per launch pair."""
        check(_lib.lib().fhe_ksk_set_mode(self._h, int(mode), int(w_budget)))
        return self

    def mode(self):
        m, w = C.c_int(), C.c_size_t()
        check(_lib.lib().fhe_ksk_get_mode(self._h, C.byref(m), C.byref(w)))
        return dict(mode=m.value, w_budget=w.value)

    def key_switch(self, p):
        """KeySwitchingKey::key_switch: p [..., L, N] PowerBasis -> (c0, c1) [..., Lk, N] Ntt."""
        L = _lib.lib()
        b = self.ctx_ciphertext._batch(p)
        oshape = tuple(p.shape[:-2]) + (self.ctx_ksk.nmoduli, self.ctx_ksk.degree)
        if _is_dev(p):
            o0, o1 = _empty_dev(p, oshape), _empty_dev(p, oshape)
            check(L.fhe_key_switch_dev(self._h, _dptr(p), _dptr(o0), _dptr(o1), b, _stream()))
            return o0, o1
        x = _np(p)
        o0, o1 = np.zeros(oshape, dtype=np.uint64), np.zeros(oshape, dtype=np.uint64)
        check(L.fhe_key_switch(self._h, _ptr(x), _ptr(o0), _ptr(o1), b))
        return o0, o1


class RelinearizationKey:
    """bfv::RelinearizationKey (crates/fhe/src/bfv/keys/relinearization_key.rs:24-110)."""

    def __init__(self, ksk: KeySwitchingKey):
        if ksk.ctx_ksk.nmoduli == 1:
            raise FheError(-17, "KeySwitchingNotSupported")
        self.ksk = ksk

    @classmethod
    def generate(cls, sk, seed=None, ciphertext_level=0, key_level=0):
        """RelinearizationKey::new_leveled (relinearization_key.rs:43-64) on the device with
        rng = ChaCha8Rng::from_seed(seed) (32 bytes; None: from `secrets`): fhe_bfv_relin_key_generate_dev."""
        L = _lib.lib()
        return cls(_keygen(sk, ciphertext_level, key_level, 1, seed, lambda ct, kc, sd, ko, hs: (
            L.fhe_bfv_relin_key_generate_dev(ct._h, kc._h, sk.params.variance, _dptr(sk.s_ntt), _dptr8(sd), _dptr8(ko),
                                             _stream(), hs)))[0])

    @classmethod
    def from_wire(cls, ctx_ciphertext, ctx_ksk, c0_bytes, c1_bytes=None, seed=None):
        """RelinearizationKeyProto's one KeySwitchingKeyProto (relinearization_key.rs), as KeySwitchingKey.from_wire."""
        return cls(KeySwitchingKey.from_wire(ctx_ciphertext, ctx_ksk, c0_bytes, c1_bytes, seed)[0])

    def to_wire(self, seeded=None):
        return self.ksk.to_wire(seeded)

    def relinearizes(self, ct3):
        """[..., 3, L, N] Ntt -> [..., 2, L, N] Ntt."""
        L = _lib.lib()
        ctx = self.ksk.ctx_ciphertext
        if ct3.shape[-3] != 3:
            raise FheError(-13, "InvalidPolynomialCount: relinearization expects 3 parts")
        b = ctx._batch(ct3) // 3
        oshape = tuple(ct3.shape[:-3]) + (2, ctx.nmoduli, ctx.degree)
        if _is_dev(ct3):
            out = _empty_dev(ct3, oshape)
            check(L.fhe_bfv_relinearize_dev(self.ksk._h, _dptr(ct3), _dptr(out), b, _stream()))
            return out
        x = _np(ct3)
        out = np.zeros(oshape, dtype=np.uint64)
        check(L.fhe_bfv_relinearize(self.ksk._h, _ptr(x), _ptr(out), b))
        return out


class GaloisKey:
    """bfv::GaloisKey (crates/fhe/src/bfv/keys/galois_key.rs:19-123)."""

    def __init__(self, ksk: KeySwitchingKey, exponent: int):
        n = ksk.ctx_ciphertext.degree
        if (exponent % (2 * n)) & 1 == 0:
            raise FheError(-10, "InvalidSubstitutionExponent")
        self.ksk, self.exponent = ksk, exponent % (2 * n)

    @classmethod
    def generate(cls, sk, exponents, seeds=None, ciphertext_level=0, key_level=0):
        """GaloisKey::new (galois_key.rs:26-58) for every exponent in one batched device call
        (fhe_bfv_galois_keys_generate_dev), key b with rng = ChaCha8Rng::from_seed(seeds[b]) (None: from `secrets`).
        Returns a list of keys in the order of `exponents`."""
        exps = [int(e) for e in exponents]
        if not exps:
            return []
        L = _lib.lib()
        arr = (C.c_size_t * len(exps))(*exps)
        keys = _keygen(sk, ciphertext_level, key_level, len(exps), seeds, lambda ct, kc, sd, ko, hs: (
            L.fhe_bfv_galois_keys_generate_dev(ct._h, kc._h, sk.params.variance, _dptr(sk.s_ntt), arr, _dptr8(sd),
                                               len(exps), _dptr8(ko), _stream(), hs)))
        return [cls(k, e) for k, e in zip(keys, exps)]

    @classmethod
    def from_wire(cls, exponents, ctx_ciphertext, ctx_ksk, c0_bytes, c1_bytes=None, seeds=None, log_base=0):
        """One GaloisKeyProto per exponent (galois_key.rs): the keys' bytes batched as KeySwitchingKey.from_wire takes
        them ([nkeys, ndigits, size]), one load call.  Returns a list of keys in the order of `exponents`."""
        exps = [int(e) for e in exponents]
        if not exps:
            return []
        n = ctx_ciphertext.degree
        if any((e % (2 * n)) & 1 == 0 for e in exps):
            raise FheError(-10, "InvalidSubstitutionExponent")
        keys = KeySwitchingKey.from_wire(ctx_ciphertext, ctx_ksk, c0_bytes, c1_bytes, seeds, log_base)
        if len(keys) != len(exps):
            raise FheError(-1, "one key per exponent: %d exponents, %d keys" % (len(exps), len(keys)))
        return [cls(k, e) for k, e in zip(keys, exps)]

    def to_wire(self, seeded=None):
        return self.ksk.to_wire(seeded)

    def relinearize(self, ct):
        """[..., 2, L, N] Ntt -> same shape."""
        L = _lib.lib()
        ctx = self.ksk.ctx_ciphertext
        if ct.shape[-3] != 2:
            raise FheError(-13, "InvalidPolynomialCount: rotation expects 2 parts")
        b = ctx._batch(ct) // 2
        if _is_dev(ct):
            out = _empty_dev(ct, ct.shape)
            check(L.fhe_bfv_galois_dev(self.ksk._h, self.exponent, _dptr(ct), _dptr(out), b, _stream()))
            return out
        x = _np(ct)
        out = np.zeros_like(x)
        check(L.fhe_bfv_galois(self.ksk._h, self.exponent, _ptr(x), _ptr(out), b))
        return out


class EvaluationKey:
    """The rotation part of bfv::EvaluationKey (crates/fhe/src/bfv/keys/evaluation_key.rs:
    rotates_rows :110-131, rotates_columns_by :145-170, exponent map :278-286)."""

    def __init__(self, degree, galois_keys):
        self.degree = degree
        self.gk = {g.exponent: g for g in galois_keys}

    @staticmethod
    def exponents(degree, column_rotations=(), row_rotation=False, inner_sum=False, expansion_level=0):
        """The Galois exponents EvaluationKeyBuilder::build generates keys for (evaluation_key.rs:429-489), sorted."""
        n = degree
        idx = set()
        for i in column_rotations:
            if not 1 <= i < n // 2:
                raise FheError(-1, "InvalidRotationStep: %d not in [1, %d]" % (i, n // 2 - 1))
            idx.add(pow(3, i, 2 * n))
        if row_rotation or inner_sum:
            idx.add(2 * n - 1)
        if inner_sum:
            i = 1
            while i < n // 2:
                idx.add(pow(3, i, 2 * n))
                i *= 2
        if not 0 <= expansion_level <= n.bit_length() - 1:
            raise FheError(-12, "InvalidLevel: the expansion level is at most log2(N)")
        for l in range(expansion_level):
            idx.add((n >> l) + 1)
        return sorted(idx)

    @classmethod
    def generate(cls, sk, column_rotations=(), row_rotation=False, inner_sum=False, expansion_level=0, seeds=None,
                 ciphertext_level=0, key_level=0):
        """EvaluationKeyBuilder (evaluation_key.rs:345-489) on the device: the builder's Galois exponents, sorted, one
        seed per exponent (None: from `secrets`), in one batched call.  (The reference draws its keys from one rng in
        HashSet order; here each key has its own seed.)"""
        exps = cls.exponents(sk.params.degree, column_rotations, row_rotation, inner_sum, expansion_level)
        return cls(sk.params.degree, GaloisKey.generate(sk, exps, seeds, ciphertext_level, key_level))

    @classmethod
    def from_wire(cls, exponents, ctx_ciphertext, ctx_ksk, c0_bytes, c1_bytes=None, seeds=None, log_base=0):
        """EvaluationKeyProto's Galois keys (evaluation_key.rs): `exponents` are the messages' exponents, the bytes
        batched in the same order (GaloisKey.from_wire)."""
        return cls(ctx_ciphertext.degree,
                   GaloisKey.from_wire(exponents, ctx_ciphertext, ctx_ksk, c0_bytes, c1_bytes, seeds, log_base))

    def to_wire(self, seeded=None):
        """(exponents, [KeySwitchingKey.to_wire(seeded) per key]), exponents sorted."""
        exps = sorted(self.gk)
        return exps, [self.gk[e].to_wire(seeded) for e in exps]

    @staticmethod
    def batched(eks):
        """The evaluation keys of many clients as one `EvaluationKeySet` (keyed batches: one set per exponent); refuses
        clients whose exponent lists differ."""
        return EvaluationKeySet(eks)

    def rotates_rows(self, ct):
        e = 2 * self.degree - 1
        if e not in self.gk:
            raise FheError(-11, "EvaluationKeyError::Unsupported(RowRotation)")
        return self.gk[e].relinearize(ct)

    def computes_inner_sum(self, ct):
        """EvaluationKey::computes_inner_sum (evaluation_key.rs:56-100)."""
        n = self.degree
        seq, i = [], 1
        while i < n // 2:
            seq.append(pow(3, i, 2 * n))
            i *= 2
        seq.append(2 * n - 1)
        if any(e not in self.gk for e in seq):
            raise FheError(-11, "EvaluationKeyError::Unsupported(InnerSum)")
        L = _lib.lib()
        handles = (C.c_void_p * len(seq))(*[self.gk[e].ksk._h for e in seq])
        exps = (C.c_size_t * len(seq))(*seq)
        ctx = self.gk[seq[0]].ksk.ctx_ciphertext
        b = ctx._batch(ct) // 2
        if _is_dev(ct):
            out = _empty_dev(ct, ct.shape)
            check(L.fhe_bfv_inner_sum_dev(handles, exps, len(seq), _dptr(ct), _dptr(out), b, _stream()))
            return out
        x = _np(ct)
        out = np.zeros_like(x)
        check(L.fhe_bfv_inner_sum(handles, exps, len(seq), _ptr(x), _ptr(out), b))
        return out

    def supports_expansion(self, level):
        """evaluation_key.rs:174-186: the Galois keys of (N >> l) + 1, l < level, are present."""
        return level <= self.degree.bit_length() - 1 and all((self.degree >> l) + 1 in self.gk for l in range(level))

    def expands(self, ct, size):
        """EvaluationKey::expands (evaluation_key.rs:192-256): ct [2, L, N] (or [batch, 2, L, N])
        -> [size, 2, L, N] (or [size, batch, 2, L, N])."""
        if size == 0 or size > self.degree:
            raise FheError(-20, "InvalidExpansionSize")
        level = (size - 1).bit_length()
        if not self.supports_expansion(level):
            raise FheError(-21, "EvaluationKeyError::Unsupported(Expansion)")
        L = _lib.lib()
        if level == 0:   # the reference returns vec![ct.clone()] without looking at any key
            return (ct.clone() if _is_dev(ct) else _np(ct).copy())[None]
        handles = (C.c_void_p * level)(*[self.gk[(self.degree >> l) + 1].ksk._h for l in range(level)])
        ctx = self.gk[self.degree + 1].ksk.ctx_ciphertext
        b = ctx._batch(ct) // 2
        oshape = (size,) + tuple(ct.shape)
        if _is_dev(ct):
            out = _empty_dev(ct, oshape)
            check(L.fhe_bfv_expand_dev(handles, level, _dptr(ct), _dptr(out), size, b, _stream()))
            return out
        x = _np(ct)
        out = np.zeros(oshape, dtype=np.uint64)
        check(L.fhe_bfv_expand(handles, level, _ptr(x), _ptr(out), size, b))
        return out

    def rotates_columns_by(self, ct, i):
        if not (1 <= i < self.degree // 2):
            raise FheError(-1, "InvalidRotationStep")
        e = pow(3, i, 2 * self.degree)
        if e not in self.gk:
            raise FheError(-11, "EvaluationKeyError::Unsupported(ColumnRotation)")
        return self.gk[e].relinearize(ct)

    def hoisted(self, column_rotations=(), row_rotation=False):
        """The rotations `column_rotations` (steps, in this order) and then the row rotation as ONE hoisted call per
        ciphertext batch: a `HoistedRotations` holding the key set and the exponent list, both built once.  A missing
        key raises what rotates_columns_by / rotates_rows raise."""
        exps = []
        for i in column_rotations:
            if not (1 <= i < self.degree // 2):
                raise FheError(-1, "InvalidRotationStep")
            e = pow(3, i, 2 * self.degree)
            if e not in self.gk:
                raise FheError(-11, "EvaluationKeyError::Unsupported(ColumnRotation)")
            exps.append(e)
        if row_rotation:
            e = 2 * self.degree - 1
            if e not in self.gk:
                raise FheError(-11, "EvaluationKeyError::Unsupported(RowRotation)")
            exps.append(e)
        if not exps:
            raise FheError(-1, "hoisted rotations: no rotation was asked for")
        return HoistedRotations([self.gk[e] for e in exps])

    def bsgs(self, baby_steps, giant_steps):
        """The baby-step/giant-step form of a matrix-vector product over B = baby_steps x G = giant_steps diagonals: a
        `BsgsRotations` holding the column rotations 1 .. B - 1 (the babies) and g * B for g = 1 .. G - 1 (the giants),
        B + G - 2 keys where `hoisted` needs G * B - 1.  A missing key raises what hoisted() raises."""
        B, G = int(baby_steps), int(giant_steps)
        if B < 2 or G < 2:
            raise FheError(-1, "bsgs: at least two baby steps and two giant steps (else use hoisted())")
        keys = []
        for steps in (range(1, B), [g * B for g in range(1, G)]):
            row = []
            for i in steps:
                if not (1 <= i < self.degree // 2):
                    raise FheError(-1, "InvalidRotationStep")
                e = pow(3, i, 2 * self.degree)
                if e not in self.gk:
                    raise FheError(-11, "EvaluationKeyError::Unsupported(ColumnRotation)")
                row.append(self.gk[e])
            keys.append(row)
        return BsgsRotations(keys[0], keys[1])


class HoistedRotations:
    """`EvaluationKey.hoisted(...)`: several rotations of each ciphertext on one digit decomposition (KeySet.
    relinearize_hoisted).  rotate(ct): [batch, 2, L, N] -> [batch, R, 2, L, N], rotation r under galois_keys[r] -- the
    layout Context.dot_product_scalar reads as R ciphertexts per item.  Not the reference's words (include/fhe_hip.h)."""

    def __init__(self, galois_keys):
        self.keys = list(galois_keys)
        self.exponents = [g.exponent for g in self.keys]
        self.set = KeySet([g.ksk for g in self.keys])

    def __len__(self):
        return len(self.exponents)

    def rotate(self, ct):
        return self.set.relinearize_hoisted(self.exponents, ct)

    def matvec(self, ct, pts, pt0=None):
        """The diagonal form of a plaintext matrix times an encrypted vector in one call (KeySet.matvec_hoisted):
        pt0 * ct + sum_r pts[r] * rotation_r(ct) -> [batch, 2, L, N] (or [2, L, N]); no rotated ciphertext is stored."""
        return self.set.matvec_hoisted(self.exponents, ct, pts, pt0)


class BsgsRotations:
    """`EvaluationKey.bsgs(B, G)`: the baby-step/giant-step hoisted matrix-vector product (KeySet.matvec_bsgs) over the
    column rotations 1 .. B - 1 (`baby`, a KeySet, with `baby_exponents`) and B, 2B .. (G - 1)B (`giant`,
    `giant_exponents`).  matvec(ct, pts) computes
        sum_g rot_{gB}( sum_b pts[g][b] * rot_b(ct) ),     pts [G, B, L, N] (or [batch, G, B, L, N]) poly_ntt rows,
    so a caller who wants sum_r d_r * rot_r(ct) over the diagonals d_r, r = g B + b, OWES THE PRE-ROTATION
        pts[g][b] = encode( rot_{-gB}(d_{gB+b}) ):
    the slots of diagonal g B + b turned by g B column steps AGAINST the direction of rotates_columns_by (in both rows
    of the slot matrix) before they are encoded.  Row g = 0 and column b = 0 take no rotation.  Not the reference's
    words (include/fhe_hip.h); it decrypts to what the flat product on the diagonals d_r decrypts to."""

    def __init__(self, baby_keys, giant_keys):
        self.baby_keys, self.giant_keys = list(baby_keys), list(giant_keys)
        self.baby_exponents = [g.exponent for g in self.baby_keys]
        self.giant_exponents = [g.exponent for g in self.giant_keys]
        self.baby = KeySet([g.ksk for g in self.baby_keys])
        self.giant = KeySet([g.ksk for g in self.giant_keys])

    @property
    def shape(self):
        """(G, B): the grid of diagonals matvec expects."""
        return len(self.giant_exponents) + 1, len(self.baby_exponents) + 1

    def matvec(self, ct, pts):
        return self.baby.matvec_bsgs(self.baby_exponents, self.giant, self.giant_exponents, ct, pts)


class KeySet:
    """Keyed batches (fhe_kskset): the keys of many clients for ONE operation -- every client's relinearization key, or
    every client's Galois key of one exponent -- as `KeySwitchingKey`, `RelinearizationKey` or `GaloisKey` objects (kept
    alive here).  A call takes a batch whose leading dimension is a multiple of len(keys): items [c * m, (c + 1) * m)
    belong to keys[c], and the result is what one single-key call per client gives.  numpy in -> numpy out (staged
    through the device); torch tensors and DeviceArrays are read in place."""

    def __init__(self, keys):
        self.keys = list(keys)
        ksks = [getattr(k, "ksk", k) for k in self.keys]
        exps = {getattr(k, "exponent", None) for k in self.keys}
        if len(exps) > 1:
            raise FheError(-1, "a key set holds the clients' keys of one exponent")
        self.exponent = exps.pop() if exps else None
        h = C.c_void_p()
        arr = (C.c_void_p * max(len(ksks), 1))(*[k._h.value if k is not None else None for k in ksks])
        check(_lib.lib().fhe_kskset_create(arr, len(ksks), C.byref(h)))
        self._h = h
        self.ctx_ciphertext, self.ctx_ksk = ksks[0].ctx_ciphertext, ksks[0].ctx_ksk

    def __del__(self):
        if getattr(self, "_h", None) is not None and _lib._lib is not None:
            _lib._lib.fhe_kskset_destroy(self._h)

    def __len__(self):
        return int(_lib.lib().fhe_kskset_size(self._h))

    def set_w_budget(self, nbytes=0):
        """Bytes of transformed digit rows per launch pair (fhe_kskset_set_w_budget; 0 = default)."""
        check(_lib.lib().fhe_kskset_set_w_budget(self._h, int(nbytes)))
        return self

    def set_rot_split(self, groups=0):
        """Rotation groups of one launch of matvec_hoisted (fhe_kskset_set_rot_split; 0 = the engine's rule)."""
        check(_lib.lib().fhe_kskset_set_rot_split(self._h, int(groups)))
        return self

    def rot_split(self):
        g = C.c_size_t()
        check(_lib.lib().fhe_kskset_get_rot_split(self._h, C.byref(g)))
        return g.value

    def set_bsgs_tile(self, gt=0):
        """Giant groups per block of matvec_bsgs's baby stage, read from the BABY set (fhe_kskset_set_bsgs_tile; 0 = the
        engine's rule, 1 / 2 / 4 force an instance)."""
        check(_lib.lib().fhe_kskset_set_bsgs_tile(self._h, int(gt)))
        return self

    def bsgs_tile(self):
        g = C.c_size_t()
        check(_lib.lib().fhe_kskset_get_bsgs_tile(self._h, C.byref(g)))
        return g.value

    def w_budget(self):
        w = C.c_size_t()
        check(_lib.lib().fhe_kskset_get_w_budget(self._h, C.byref(w)))
        return w.value

    def _run(self, x, oshapes, call):
        """Stages `x`, allocates one output per shape, runs call(x, outs) and hands the outputs back in x's kind."""
        host = not _is_dev(x)
        d = DeviceArray.from_numpy(_np(x), max(self.ctx_ksk.device, 0)) if host else x
        outs = [DeviceArray(sh, d.device) if host else _empty_dev(d, sh) for sh in oshapes]
        check(call(d, outs))
        return [o.download() if host else o for o in outs]

    def key_switch(self, p):
        """KeySwitchingKey::key_switch per client: p [batch, L, N] PowerBasis -> (c0, c1) [batch, Lk, N] Ntt."""
        L = _lib.lib()
        b = self.ctx_ciphertext._batch(p)
        oshape = tuple(p.shape[:-2]) + (self.ctx_ksk.nmoduli, self.ctx_ksk.degree)
        o0, o1 = self._run(p, [oshape, oshape], lambda d, o: L.fhe_key_switch_keyed_dev(
            self._h, _dptr(d), _dptr(o[0]), _dptr(o[1]), b, _stream()))
        return o0, o1

    def relinearizes(self, ct3):
        """RelinearizationKey::relinearizes per client: [batch, 3, L, N] Ntt -> [batch, 2, L, N] Ntt."""
        L = _lib.lib()
        ctx = self.ctx_ciphertext
        if ct3.shape[-3] != 3:
            raise FheError(-13, "InvalidPolynomialCount: relinearization expects 3 parts")
        b = ctx._batch(ct3) // 3
        oshape = tuple(ct3.shape[:-3]) + (2, ctx.nmoduli, ctx.degree)
        return self._run(ct3, [oshape], lambda d, o: L.fhe_bfv_relinearize_keyed_dev(
            self._h, _dptr(d), _dptr(o[0]), b, _stream()))[0]

    def relinearize(self, exponent, ct, out=None):
        """GaloisKey::relinearize per client with the clients' keys of `exponent`: [batch, 2, L, N] Ntt -> same shape.
        out (device arrays only): where to write; `out is ct` rotates in place."""
        L = _lib.lib()
        ctx = self.ctx_ciphertext
        if ct.shape[-3] != 2:
            raise FheError(-13, "InvalidPolynomialCount: rotation expects 2 parts")
        e = int(exponent) % (2 * ctx.degree)
        if e & 1 == 0:
            raise FheError(-10, "InvalidSubstitutionExponent")
        if self.exponent is not None and self.exponent != e:
            raise FheError(-1, "the set holds the Galois keys of exponent %d, not %d" % (self.exponent, e))
        b = ctx._batch(ct) // 2
        if out is not None:
            check(L.fhe_bfv_galois_keyed_dev(self._h, e, _dptr(ct), _dptr(out), b, _stream()))
            return out
        return self._run(ct, [tuple(ct.shape)], lambda d, o: L.fhe_bfv_galois_keyed_dev(
            self._h, e, _dptr(d), _dptr(o[0]), b, _stream()))[0]

    def relinearize_hoisted(self, exponents, ct):
        """Hoisted rotations (fhe_bfv_galois_hoisted_dev): the set holds ONE client's Galois keys, key r for exponents[r];
        [batch, 2, L, N] Ntt (or [2, L, N]) -> [batch, R, 2, L, N] (or [R, 2, L, N]), every rotation of a ciphertext on one
        digit decomposition.  Not the reference's words: a restatement (include/fhe_hip.h) that decrypts to what
        GaloisKey.relinearize's result does and equals it word for word only at exponent 1."""
        L = _lib.lib()
        ctx = self.ctx_ciphertext
        if ct.shape[-3] != 2:
            raise FheError(-13, "InvalidPolynomialCount: rotation expects 2 parts")
        exps = [int(e) for e in exponents]
        arr = (C.c_size_t * max(len(exps), 1))(*exps)
        b = ctx._batch(ct) // 2
        oshape = tuple(ct.shape[:-3]) + (len(exps),) + tuple(ct.shape[-3:])
        return self._run(ct, [oshape], lambda d, o: L.fhe_bfv_galois_hoisted_dev(
            self._h, arr, len(exps), _dptr(d), _dptr(o[0]), b, _stream()))[0]

    def matvec_hoisted(self, exponents, ct, pts, pt0=None):
        """Hoisted matrix-vector product (fhe_bfv_matvec_hoisted_dev): pt0 * ct + sum_r pts[r] * rotation_r(ct), the set
        holding ONE client's Galois keys, key r for exponents[r].  ct [batch, 2, L, N] Ntt (or [2, L, N]); pts
        `Plaintext::poly_ntt` rows, [R, L, N] shared by the batch or [batch, R, L, N]; pt0 None, [L, N] or [batch, L, N]
        likewise -> [batch, 2, L, N] (or [2, L, N]), of ct's kind.  Word for word relinearize_hoisted followed by
        Context.dot_product_scalar, and like it not the reference's words (include/fhe_hip.h)."""
        L = _lib.lib()
        ctx = self.ctx_ciphertext
        if ct.shape[-3] != 2:
            raise FheError(-13, "InvalidPolynomialCount: rotation expects 2 parts")
        exps = [int(e) for e in exponents]
        arr = (C.c_size_t * max(len(exps), 1))(*exps)
        lead = tuple(ct.shape[:-3])
        b = ctx._batch(ct) // 2
        shared = len(pts.shape) == 3
        want = ((len(exps),) if shared else lead + (len(exps),)) + (ctx.nmoduli, ctx.degree)
        if tuple(pts.shape) != want:
            raise FheError(-1, "DotProductLengthMismatch: diagonals %s, expected %s" % (tuple(pts.shape), want))
        if pt0 is not None and tuple(pt0.shape) != (() if shared else lead) + (ctx.nmoduli, ctx.degree):
            raise FheError(-1, "DotProductLengthMismatch: the identity diagonal follows the diagonals' batch shape")
        host = not _is_dev(ct)
        dev = max(self.ctx_ksk.device, 0)
        stage = (lambda a: DeviceArray.from_numpy(_np(a), dev)) if host else (lambda a: a)
        d, p, p0 = stage(ct), stage(pts), (None if pt0 is None else stage(pt0))
        out = DeviceArray(tuple(ct.shape), dev) if host else _empty_dev(d, tuple(ct.shape))
        check(L.fhe_bfv_matvec_hoisted_dev(self._h, arr, len(exps), _dptr(d), _dptr(p), 1 if shared else 0,
                                           None if p0 is None else _dptr(p0), _dptr(out), b, _stream()))
        return out.download() if host else out

    def relinearize_hoisted_keyed(self, nclients, exponents, ct):
        """Hoisted rotations with one Galois key set per client (fhe_bfv_galois_hoisted_keyed_dev): the set holds
        nclients * R keys CLIENT-MAJOR, entry c * R + r being client c's key for exponents[r]; items [c * m, (c + 1) * m),
        m = batch / nclients, belong to client c.  [batch, 2, L, N] Ntt -> [batch, R, 2, L, N], word for word one
        relinearize_hoisted call per client on the client's keys and slice of the batch (not the reference's words)."""
        L = _lib.lib()
        ctx = self.ctx_ciphertext
        if ct.shape[-3] != 2:
            raise FheError(-13, "InvalidPolynomialCount: rotation expects 2 parts")
        exps = [int(e) for e in exponents]
        arr = (C.c_size_t * max(len(exps), 1))(*exps)
        b = ctx._batch(ct) // 2
        oshape = tuple(ct.shape[:-3]) + (len(exps),) + tuple(ct.shape[-3:])
        return self._run(ct, [oshape], lambda d, o: L.fhe_bfv_galois_hoisted_keyed_dev(
            self._h, int(nclients), arr, len(exps), _dptr(d), _dptr(o[0]), b, _stream()))[0]

    def matvec_hoisted_keyed(self, nclients, exponents, ct, pts, pt0=None):
        """Hoisted matrix-vector product with one Galois key set per client (fhe_bfv_matvec_hoisted_keyed_dev): the set and
        the ownership rule of relinearize_hoisted_keyed, the shapes of matvec_hoisted -- pts [R, L, N] shared by the WHOLE
        batch or [batch, R, L, N], pt0 None, [L, N] or [batch, L, N] likewise -> [batch, 2, L, N], of ct's kind.  Word for
        word one matvec_hoisted call per client on the client's keys and slices of ct, pts and pt0."""
        L = _lib.lib()
        ctx = self.ctx_ciphertext
        if ct.shape[-3] != 2:
            raise FheError(-13, "InvalidPolynomialCount: rotation expects 2 parts")
        exps = [int(e) for e in exponents]
        arr = (C.c_size_t * max(len(exps), 1))(*exps)
        lead = tuple(ct.shape[:-3])
        b = ctx._batch(ct) // 2
        shared = len(pts.shape) == 3
        want = ((len(exps),) if shared else lead + (len(exps),)) + (ctx.nmoduli, ctx.degree)
        if tuple(pts.shape) != want:
            raise FheError(-1, "DotProductLengthMismatch: diagonals %s, expected %s" % (tuple(pts.shape), want))
        if pt0 is not None and tuple(pt0.shape) != (() if shared else lead) + (ctx.nmoduli, ctx.degree):
            raise FheError(-1, "DotProductLengthMismatch: the identity diagonal follows the diagonals' batch shape")
        host = not _is_dev(ct)
        dev = max(self.ctx_ksk.device, 0)
        stage = (lambda a: DeviceArray.from_numpy(_np(a), dev)) if host else (lambda a: a)
        d, p, p0 = stage(ct), stage(pts), (None if pt0 is None else stage(pt0))
        out = DeviceArray(tuple(ct.shape), dev) if host else _empty_dev(d, tuple(ct.shape))
        check(L.fhe_bfv_matvec_hoisted_keyed_dev(self._h, int(nclients), arr, len(exps), _dptr(d), _dptr(p), 1 if shared else 0,
                                                 None if p0 is None else _dptr(p0), _dptr(out), b, _stream()))
        return out.download() if host else out

    def matvec_bsgs(self, baby_exps, giant_set, giant_exps, ct, pts):
        """Baby-step/giant-step hoisted matrix-vector product (fhe_bfv_matvec_bsgs_dev): this set holds ONE client's baby
        Galois keys (key r for baby_exps[r]), `giant_set` the giant keys.  ct [batch, 2, L, N] Ntt (or [2, L, N]); pts
        `Plaintext::poly_ntt` rows, [G, B, L, N] shared by the batch or [batch, G, B, L, N], G = len(giant_exps) + 1,
        B = len(baby_exps) + 1; column 0 of a group is its identity diagonal, row 0 the group without a giant rotation
        -> sum_g rot_giant_g( sum_b pts[g][b] * rot_baby_b(ct) ), [batch, 2, L, N] (or [2, L, N]), of ct's kind.
        Word for word G matvec_hoisted calls, one-key relinearize_hoisted calls and additions; like them not the
        reference's words (include/fhe_hip.h)."""
        L = _lib.lib()
        ctx = self.ctx_ciphertext
        if ct.shape[-3] != 2:
            raise FheError(-13, "InvalidPolynomialCount: rotation expects 2 parts")
        bex, gex = [int(e) for e in baby_exps], [int(e) for e in giant_exps]
        ba, ga = (C.c_size_t * max(len(bex), 1))(*bex), (C.c_size_t * max(len(gex), 1))(*gex)
        lead = tuple(ct.shape[:-3])
        b = ctx._batch(ct) // 2
        shared = len(pts.shape) == 4
        grid = (len(gex) + 1, len(bex) + 1)
        want = (grid if shared else lead + grid) + (ctx.nmoduli, ctx.degree)
        if tuple(pts.shape) != want:
            raise FheError(-1, "DotProductLengthMismatch: diagonals %s, expected %s" % (tuple(pts.shape), want))
        host = not _is_dev(ct)
        dev = max(self.ctx_ksk.device, 0)
        stage = (lambda a: DeviceArray.from_numpy(_np(a), dev)) if host else (lambda a: a)
        d, p = stage(ct), stage(pts)
        out = DeviceArray(tuple(ct.shape), dev) if host else _empty_dev(d, tuple(ct.shape))
        check(L.fhe_bfv_matvec_bsgs_dev(self._h, ba, len(bex), giant_set._h, ga, len(gex), _dptr(d), _dptr(p),
                                        1 if shared else 0, _dptr(out), b, _stream()))
        return out.download() if host else out


class EvaluationKeySet:
    """`EvaluationKey.batched(eks)`: the rotation keys of many clients, one `KeySet` per Galois exponent.  Each method
    is the `EvaluationKey` method of the same name applied client by client to a batch whose leading dimension is a
    multiple of the client count (items [c * m, (c + 1) * m) belong to client c)."""

    def __init__(self, eks):
        eks = list(eks)
        if not eks:
            raise FheError(-1, "a key set needs at least one key")
        exps = sorted(eks[0].gk)
        if any(sorted(ek.gk) != exps or ek.degree != eks[0].degree for ek in eks):
            raise FheError(-1, "the clients' evaluation keys differ in their Galois exponents")
        self.degree, self.nclients = eks[0].degree, len(eks)
        self.sets = {e: KeySet([ek.gk[e] for ek in eks]) for e in exps}

    def _need(self, exps, what):
        if any(e not in self.sets for e in exps):
            raise FheError(-11, "EvaluationKeyError::Unsupported(%s)" % what)

    def rotates_rows(self, ct):
        e = 2 * self.degree - 1
        self._need([e], "RowRotation")
        return self.sets[e].relinearize(e, ct)

    def rotates_columns_by(self, ct, i):
        if not (1 <= i < self.degree // 2):
            raise FheError(-1, "InvalidRotationStep")
        e = pow(3, i, 2 * self.degree)
        self._need([e], "ColumnRotation")
        return self.sets[e].relinearize(e, ct)

    def hoisted(self, column_rotations=(), row_rotation=False):
        """EvaluationKey.hoisted for every client at once: the rotations `column_rotations` (steps, in this order) and
        then the row rotation as ONE hoisted call per batch, each ciphertext under its owner's keys -- a
        `KeyedHoistedRotations`.  A missing key or a bad step raises what EvaluationKey.hoisted raises."""
        exps = []
        for i in column_rotations:
            if not (1 <= i < self.degree // 2):
                raise FheError(-1, "InvalidRotationStep")
            e = pow(3, i, 2 * self.degree)
            self._need([e], "ColumnRotation")
            exps.append(e)
        if row_rotation:
            e = 2 * self.degree - 1
            self._need([e], "RowRotation")
            exps.append(e)
        if not exps:
            raise FheError(-1, "hoisted rotations: no rotation was asked for")
        return KeyedHoistedRotations(self.nclients, [[self.sets[e].keys[c] for e in exps] for c in range(self.nclients)])

    def computes_inner_sum(self, ct):
        """EvaluationKey::computes_inner_sum (evaluation_key.rs:56-100) per client."""
        n = self.degree
        seq, i = [], 1
        while i < n // 2:
            seq.append(pow(3, i, 2 * n))
            i *= 2
        seq.append(2 * n - 1)
        self._need(seq, "InnerSum")
        L = _lib.lib()
        handles = (C.c_void_p * len(seq))(*[self.sets[e]._h.value for e in seq])
        exps = (C.c_size_t * len(seq))(*seq)
        first = self.sets[seq[0]]
        b = first.ctx_ciphertext._batch(ct) // 2
        return first._run(ct, [tuple(ct.shape)], lambda d, o: L.fhe_bfv_inner_sum_keyed_dev(
            handles, exps, len(seq), _dptr(d), _dptr(o[0]), b, _stream()))[0]

    def supports_expansion(self, level):
        return level <= self.degree.bit_length() - 1 and all((self.degree >> l) + 1 in self.sets for l in range(level))

    def expands(self, ct, size):
        """EvaluationKey::expands (evaluation_key.rs:192-256) per client: ct [batch, 2, L, N] ->
        [size, batch, 2, L, N]."""
        if size == 0 or size > self.degree:
            raise FheError(-20, "InvalidExpansionSize")
        level = (size - 1).bit_length()
        if not self.supports_expansion(level):
            raise FheError(-21, "EvaluationKeyError::Unsupported(Expansion)")
        if level == 0:
            return (ct.clone() if _is_dev(ct) else _np(ct).copy())[None]
        L = _lib.lib()
        handles = (C.c_void_p * level)(*[self.sets[(self.degree >> l) + 1]._h.value for l in range(level)])
        first = self.sets[self.degree + 1]
        b = first.ctx_ciphertext._batch(ct) // 2
        return first._run(ct, [(size,) + tuple(ct.shape)], lambda d, o: L.fhe_bfv_expand_keyed_dev(
            handles, level, _dptr(d), _dptr(o[0]), size, b, _stream()))[0]


class KeyedHoistedRotations:
    """`EvaluationKeySet.hoisted(...)`: HoistedRotations for many clients in one call (KeySet.relinearize_hoisted_keyed,
    KeySet.matvec_hoisted_keyed).  `set` is ONE KeySet over the clients' Galois keys in client-major order (client c's
    key for exponents[r] at c * R + r), built once; items [c * m, (c + 1) * m) of a batch belong to client c.
    rotate(ct): [batch, 2, L, N] -> [batch, R, 2, L, N]; matvec(ct, pts, pt0): pt0 * ct + sum_r pts[r] * rotation_r(ct)
    -> [batch, 2, L, N], the diagonals shared by the whole batch or one set per item.  Word for word HoistedRotations
    client by client, and like it not the reference's words (include/fhe_hip.h)."""

    def __init__(self, nclients, client_keys):
        self.nclients = int(nclients)
        self.keys = [list(row) for row in client_keys]
        self.exponents = [g.exponent for g in self.keys[0]]
        self.set = KeySet([g.ksk for row in self.keys for g in row])

    def __len__(self):
        return len(self.exponents)

    def rotate(self, ct):
        return self.set.relinearize_hoisted_keyed(self.nclients, self.exponents, ct)

    def matvec(self, ct, pts, pt0=None):
        return self.set.matvec_hoisted_keyed(self.nclients, self.exponents, ct, pts, pt0)


class RGSWCiphertext:
    """bfv::RGSWCiphertext{ksk0, ksk1} (crates/fhe/src/bfv/rgsw_ciphertext.rs:19-156)."""

    def __init__(self, ksk0: KeySwitchingKey, ksk1: KeySwitchingKey):
        self.ksk0, self.ksk1 = ksk0, ksk1

    @classmethod
    def from_wire(cls, ctx_ciphertext, ctx_ksk, c0_bytes, c1_bytes=None, seeds=None, log_base=0):
        """RGSWCiphertextProto{ksk0, ksk1} (rgsw_ciphertext.rs): two keys in one load call, bytes [2, ndigits, size].
        Both keys are at the ciphertext's level, else FheError(-1)."""
        if list(ctx_ksk.moduli) != list(ctx_ciphertext.moduli) or len(c0_bytes.shape) != 3 or c0_bytes.shape[0] != 2:
            raise FheError(-1, "an RGSW ciphertext is two keys at the ciphertext level")
        return cls(*KeySwitchingKey.from_wire(ctx_ciphertext, ctx_ksk, c0_bytes, c1_bytes, seeds, log_base))

    def to_wire(self, seeded=None):
        return self.ksk0.to_wire(seeded), self.ksk1.to_wire(seeded)

    def external_product(self, ct):
        """`&Ciphertext * &RGSWCiphertext`: ct, result [..., 2, L, N] Ntt."""
        L = _lib.lib()
        ctx = self.ksk0.ctx_ciphertext
        if ct.shape[-3] != 2:
            raise FheError(-13, "Ciphertext must have two parts")
        b = ctx._batch(ct) // 2
        if _is_dev(ct):
            out = _empty_dev(ct, ct.shape)
            check(L.fhe_bfv_rgsw_mul_dev(self.ksk0._h, self.ksk1._h, _dptr(ct), _dptr(out), b, _stream()))
            return out
        x = _np(ct)
        out = np.zeros_like(x)
        check(L.fhe_bfv_rgsw_mul(self.ksk0._h, self.ksk1._h, _ptr(x), _ptr(out), b))
        return out


_ENCODINGS = {"poly": 0, "simd": 1}


def _encoding(name):
    if name not in _ENCODINGS:
        raise FheError(-1, f"unknown encoding {name!r} (poly / simd)")
    return _ENCODINGS[name]


def _tables_cb(tables_fn):
    """fhe_ntt_tables_fn around a Python tables_fn(modulus, degree) -> dict (see BfvParameters)."""
    def _cb(_user, modulus, deg, om, oms, zi, zis, si, sis):
        try:
            t = tables_fn(int(modulus), int(deg))
            arrs = [_np(t[key]).reshape(-1) for key in ("omegas", "omegas_shoup", "zetas_inv", "zetas_inv_shoup")]
            if any(a.size != deg for a in arrs):
                return 1   # a short table would be read out of bounds: creation fails (NttOperatorUnavailable)
            for dst, a in zip((om, oms, zi, zis), arrs):
                C.memmove(dst, a.ctypes.data, 8 * deg)
            si[0], sis[0] = int(t["size_inv"]), int(t["size_inv_shoup"])
            return 0
        except Exception:
            return 1
    return _lib.NTT_TABLES_FN(_cb)


class Encoder:
    """The encoding tables of bfv::BfvParameters (parameters.rs:598, 607-633, 711-725) on the device: made by
    `BfvParameters.encoder()`.  numpy in -> numpy out (staged through `DeviceArray`s on the ABI's allocator); a device
    array in -> a device array out, on the current stream."""

    def __init__(self, params, tables_fn=None):
        self._params = params   # (the C handle borrows the parameter set's contexts)
        self.degree, self.plaintext = params.degree, params.plaintext
        h = C.c_void_p()
        cb = _tables_cb(tables_fn) if tables_fn is not None else _lib.NTT_TABLES_FN()
        check(_lib.lib().fhe_encoder_create(params._h, cb, None, C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None) is not None and _lib._lib is not None:
            _lib._lib.fhe_encoder_destroy(self._h)

    def encode(self, values, encoding="simd", level=0, scaled=False):
        """PlaintextVec::try_encode (plaintext_vec.rs:70-102): values [..., nvalues] (nvalues <= N) -> the
        plaintexts' poly_ntt [..., L_level, N]; scaled=True gives Plaintext::to_poly (plaintext.rs:172-196), the
        operand of Context.add_plain / sub_plain.  Values are reduced mod t."""
        L = _lib.lib()
        enc = _encoding(encoding)
        nmod = len(self._params.moduli) - level if 0 <= level < len(self._params.moduli) else 1
        wt = self._params.plaintext_limbs
        if wt > 1:
            # PlaintextVec::try_encode for Vec<BigUint> (plaintext_vec.rs:105-132): Python ints [..., nvalues] (a list or
            # an object array), or a device array of limbs [..., nvalues, W_t]
            if not _is_dev(values):
                values = _to_limbs(values, wt)
            if len(values.shape) < 2 or int(values.shape[-1]) != wt:
                raise FheError(-1, "values: expected [..., nvalues, %d] limbs" % wt)
            lead, nvalues = tuple(int(d) for d in values.shape[:-2]), int(values.shape[-2])
            batch = int(np.prod(lead)) if lead else 1
            oshape = lead + (nmod, self.degree)
            host = not _is_dev(values)
            x = DeviceArray.from_numpy(values, max(self._params.device, 0)) if host else values
            try:
                out = DeviceArray(oshape, x.device) if host else _empty_dev(values, oshape)
                check(L.fhe_bfv_encode_big_dev(self._h, enc, 1 if scaled else 0, level, _dptr(x), nvalues, _dptr(out),
                                               batch, _stream()))
                return out.download() if host else out
            finally:
                _wipe([x] if host else [])
        lead, nvalues = tuple(values.shape[:-1]), int(values.shape[-1])
        batch = int(np.prod(lead)) if lead else 1
        oshape = lead + (nmod, self.degree)
        if _is_dev(values):
            out = _empty_dev(values, oshape)
            check(L.fhe_bfv_encode_dev(self._h, enc, 1 if scaled else 0, level, _dptr(values), nvalues, _dptr(out), batch,
                                       _stream()))
            return out
        x = DeviceArray.from_numpy(_np(values), max(self._params.device, 0))
        out = DeviceArray(oshape, x.device)
        check(L.fhe_bfv_encode_dev(self._h, enc, 1 if scaled else 0, level, _dptr(x), nvalues, _dptr(out), batch,
                                   _stream()))
        return out.download()

    def _stream_args(self, nbits, level):
        nbits = (int(self.plaintext).bit_length() - 1) if nbits is None else int(nbits)
        nmod = len(self._params.moduli) - level if 0 <= level < len(self._params.moduli) else 1
        return nbits, nmod

    def encode_bytes(self, data, item_bytes, nbits=None, level=0, scaled=False, batch=None):
        """encode_database (crates/fhe/examples/util.rs:97-145): item b is bytes [b item_bytes, (b + 1) item_bytes) of
        `data` (`bytes`, a numpy uint8 array or a device uint8 array; what lies past its end reads as zero), its
        transcode_from_bytes(item, nbits) values the coefficients of one plaintext -> poly_ntt [batch, L_level, N]
        (scaled=True: Plaintext::to_poly).  nbits defaults to ilog2(t); batch to ceil(len(data) / item_bytes) -- a larger
        one appends all-zero plaintexts, the padding rows up to dim1 * dim2."""
        L = _lib.lib()
        nbits, nmod = self._stream_args(nbits, level)
        item_bytes = int(item_bytes)
        host = not _is_dev(data)
        if host:
            a = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) \
                else np.ascontiguousarray(np.asarray(data, dtype=np.uint8)).reshape(-1)
            nbytes = int(a.size)
            x = DeviceArray.from_numpy(a, max(self._params.device, 0)) if nbytes else None
        else:
            x, nbytes = data, int(data.numel())
        if batch is None:
            batch = -(-nbytes // item_bytes) if item_bytes else 0
        oshape = (int(batch), nmod, self.degree)
        out = DeviceArray(oshape, max(self._params.device, 0)) if host else _empty_dev(data, oshape)
        check(L.fhe_bfv_encode_bytes_dev(self._h, 1 if scaled else 0, level, _dptr8(x) if nbytes else None, nbytes,
                                         item_bytes, nbits, _dptr(out), batch, _stream()))
        return out.download() if host else out

    def encode_words(self, words, in_bits, nbits=None, level=0, scaled=False):
        """The SealPIR fold (crates/fhe/examples/sealpir.rs:176-200): words [..., nseg, seg_len] carrying in_bits each;
        every segment through transcode_bidirectional(segment, in_bits, nbits), an item's value lists appended and cut
        into plaintexts of N values -> poly_ntt [..., nplain, L_level, N].  nbits defaults to ilog2(t)."""
        L = _lib.lib()
        nbits, nmod = self._stream_args(nbits, level)
        if len(words.shape) < 2:
            raise FheError(-1, "words: expected [..., nseg, seg_len]")
        lead, nseg, seg_len = tuple(int(d) for d in words.shape[:-2]), int(words.shape[-2]), int(words.shape[-1])
        batch = int(np.prod(lead)) if lead else 1
        nplain = int(L.fhe_bfv_encode_words_count(self._h, int(in_bits), nseg, seg_len, nbits))
        oshape = lead + (nplain, nmod, self.degree)
        host = not _is_dev(words)
        x = DeviceArray.from_numpy(_np(words), max(self._params.device, 0)) if host else words
        out = DeviceArray(oshape, x.device) if host else _empty_dev(words, oshape)
        try:
            check(L.fhe_bfv_encode_words_dev(self._h, 1 if scaled else 0, level, _dptr(x), int(in_bits), nseg, seg_len,
                                             nbits, _dptr(out), batch, _stream()))
            return out.download() if host else out
        finally:
            _wipe([x] if host else [])

    def reduce(self, polys):
        """The tail of SecretKey::try_decrypt's Large branch alone (secret_key.rs:238-250, fhe_bfv_reduce_big_dev):
        PowerBasis residues over the plaintext context [..., P, N] -> ((x + t) mod Q_p) mod t of each lifted column,
        Python ints [..., N] for numpy input and limbs [..., N, W_t] for a device array."""
        wt = self._params.plaintext_limbs
        rows = int(_lib.lib().fhe_encoder_plain_rows(self._h))
        if len(polys.shape) < 2 or (int(polys.shape[-2]), int(polys.shape[-1])) != (rows, self.degree):
            raise FheError(-1, "polys: expected [..., %d, %d] over the plaintext context" % (rows, self.degree))
        lead = tuple(int(d) for d in polys.shape[:-2])
        batch = int(np.prod(lead)) if lead else 1
        host = not _is_dev(polys)
        x = DeviceArray.from_numpy(_np(polys), max(self._params.device, 0)) if host else polys
        oshape = lead + (self.degree, wt)
        out = DeviceArray(oshape, x.device) if host else _empty_dev(polys, oshape)
        try:
            check(_lib.lib().fhe_bfv_reduce_big_dev(self._h, _dptr(x), rows, _dptr(out), batch, _stream()))
            return _from_limbs(out.download()) if host else out
        finally:
            _wipe([x, out] if host else [])

    def decode(self, coeffs, encoding="simd"):
        """Vec<u64>::try_decode (plaintext.rs:157-170, 408-431): coefficients mod t [..., N] (what decrypt returns)
        -> values [..., N]."""
        L = _lib.lib()
        enc = _encoding(encoding)
        if self._params.plaintext_limbs > 1:
            # (a plaintext modulus above 64 bits has no NTT operator: Poly only, and its values are the coefficients)
            if enc != 0:
                raise FheError(-22, "SimdUnavailable: no NTT modulo a plaintext modulus above 64 bits")
            return coeffs
        if int(coeffs.shape[-1]) != self.degree:
            raise FheError(-1, "coefficients: the last dimension must be the degree")
        batch = int(np.prod(coeffs.shape[:-1])) if len(coeffs.shape) > 1 else 1
        if _is_dev(coeffs):
            out = _empty_dev(coeffs, tuple(coeffs.shape))
            check(L.fhe_bfv_decode_dev(self._h, enc, _dptr(coeffs), _dptr(out), batch, _stream()))
            return out
        x = DeviceArray.from_numpy(_np(coeffs), max(self._params.device, 0))
        out = DeviceArray(x.shape, x.device)
        check(L.fhe_bfv_decode_dev(self._h, enc, _dptr(x), _dptr(out), batch, _stream()))
        return out.download()


def number_elements_per_plaintext(degree, nbits, element_size):
    """crates/fhe/examples/util.rs:86-92: database elements of element_size bytes per plaintext of `degree` values of
    `nbits` bits."""
    return (nbits * degree) // (element_size * 8)


def transcode(a, in_bits, out_bits, out_bytes=False, device=0):
    """fhe_util::transcode_bidirectional / transcode_to_bytes / transcode_from_bytes (fhe-util/src/lib.rs:71-190) on the
    device: rows [..., nin] of elements carrying in_bits each -> [..., ceil(nin in_bits / out_bits)] elements of out_bits
    bits.  `a` is uint64 or -- `bytes`, a numpy uint8 array, a device uint8 array -- bytes; the result is uint8 when
    out_bytes, else uint64.  numpy / bytes in -> numpy out (staged on `device`); a device array in -> a device array out,
    on the current stream."""
    L = _lib.lib()
    host = not _is_dev(a)
    if host:
        if isinstance(a, (bytes, bytearray, memoryview)):
            a = np.frombuffer(bytes(a), dtype=np.uint8)
        a = np.asarray(a)
        a = np.ascontiguousarray(a if a.dtype == np.uint8 else np.asarray(a, dtype=np.uint64))
        in_bytes = a.dtype == np.uint8
    else:
        in_bytes = a.element_size() == 1
    if len(a.shape) < 1:
        raise FheError(-1, "transcode: expected [..., nin]")
    lead, nin = tuple(int(d) for d in a.shape[:-1]), int(a.shape[-1])
    batch = int(np.prod(lead)) if lead else 1
    in_bits, out_bits = int(in_bits), int(out_bits)
    if not (1 <= in_bits <= (8 if in_bytes else 64) and 1 <= out_bits <= (8 if out_bytes else 64)):
        raise FheError(-1, "transcode: widths must be in [1, 64] ([1, 8] on a byte side)")
    nout = int(L.fhe_transcode_count(in_bits, nin, out_bits))
    oshape, osize = lead + (nout,), 1 if out_bytes else 8
    x = DeviceArray.from_numpy(a, device) if host else a
    out = DeviceArray(oshape, x.device, osize) if host else _empty_dev(a, oshape, osize)
    try:
        check(L.fhe_transcode_dev((_dptr8 if in_bytes else _dptr)(x), 1 if in_bytes else 0, in_bits, nin,
                                  (_dptr8 if out_bytes else _dptr)(out), 1 if out_bytes else 0, out_bits, batch, _stream()))
        return out.download() if host else out
    finally:
        _wipe([x, out] if host else [])


def _alloc(shape, device, itemsize=8):
    """A new device array: a torch CUDA tensor when torch drives the device and no `Stream` is current, else a
    DeviceArray on the ABI's own allocator."""
    if getattr(_tls, "stream", None) is not None or torch is None or not torch.cuda.is_available():
        return DeviceArray(shape, max(device, 0), itemsize)
    return torch.empty(tuple(shape), dtype=torch.int64 if itemsize == 8 else torch.uint8, device=f"cuda:{max(device, 0)}")


def _seeds(seeds, count, device):
    """(device uint8 buffer [n, 32], n, owned): None -> `count` fresh seeds from `secrets`; bytes -> one seed; a list
    of bytes, a numpy uint8 [n, 32] array or a device uint8 [n, 32] array as given.  `owned`: the buffer was staged
    here (the caller of _seeds clears it with _wipe once the engine call is enqueued)."""
    if seeds is not None and _is_dev(seeds):
        if seeds.element_size() != 1 or seeds.numel() % 32:
            raise ValueError("device seeds must be a contiguous uint8 [count, 32] array")
        return seeds, int(seeds.numel() // 32), False
    if seeds is None:
        a = np.frombuffer(b"".join(secrets.token_bytes(32) for _ in range(count)), dtype=np.uint8)
    elif isinstance(seeds, (bytes, bytearray)):
        a = np.frombuffer(bytes(seeds), dtype=np.uint8)
    elif isinstance(seeds, (list, tuple)):
        a = np.frombuffer(b"".join(bytes(x) for x in seeds), dtype=np.uint8)
    else:
        a = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint8)).reshape(-1)
    if a.size == 0 or a.size % 32:
        raise ValueError("seeds are 32 bytes each")
    return DeviceArray.from_numpy(a.reshape(-1, 32), max(device, 0)), a.size // 32, True


def _wipe(staged):
    """Clears the device buffers staged from host secrets (seeds, samples, plaintexts) on the current stream, ahead of
    their release (the engine clears its own scratch the same way)."""
    for d in staged:
        check(_lib.lib().fhe_buf_zero_async(C.c_void_p(d.data_ptr()), d.nbytes, _stream()))


def _seed_count(seeds):
    if _is_dev(seeds):
        return int(seeds.numel() // 32)
    if isinstance(seeds, (bytes, bytearray)):
        return len(seeds) // 32
    if isinstance(seeds, (list, tuple)):
        return len(seeds)
    return int(np.asarray(seeds).size // 32)


def _batch_of(pt, count):
    """(leading dims, batch, pt_shared) of a plaintext [..., L, N] (or None) encrypted with `count` seeds."""
    if pt is None or len(pt.shape) == 2:
        return ((count,) if count != 1 or pt is None else ()), count, 1
    lead = tuple(int(d) for d in pt.shape[:-2])
    return lead, int(np.prod(lead)), 0


def _ksk_digits(ct, kc):
    """(ndigits, log_base) of a key from `ct`'s level to `kc`'s (key_switching_key.rs:97-136)."""
    if kc.nmoduli == 1:
        lm = (kc.moduli[0] - 1).bit_length()
        return -(-lm // (lm // 2)), lm // 2
    return ct.nmoduli, 0


def _keygen(sk, ciphertext_level, key_level, count, seeds, call):
    """The shared body of the key-generation wrappers: the two contexts, one seed per key (host seeds are staged and
    cleared again), a device array for the public seeds and call(ct, kc, seeds, seeds_out, handles) -> status."""
    par = sk.params
    for lvl in (ciphertext_level, key_level):
        if not 0 <= lvl <= par.max_level:
            raise FheError(-12, "InvalidLevel")
    ct, kc = par.context_at_level(ciphertext_level), par.context_at_level(key_level)
    staged = []
    try:
        sd, n, own = _seeds(seeds, count, par.device)
        if own:
            staged.append(sd)
        if n != count:
            raise FheError(-1, "one seed per key: %d keys, %d seeds" % (count, n))
        kout = _alloc((count, 32), par.device, itemsize=1)
        hs = (C.c_void_p * count)()
        check(call(ct, kc, sd, kout, hs))
    finally:
        _wipe(staged)
    return [KeySwitchingKey._adopt(ct, kc, hs[i], kout, i) for i in range(count)]


class SecretKey:
    """bfv::SecretKey (F/bfv/keys/secret_key.rs) kept on the device: `s_ntt` is the level-0 key in Ntt form [L, N]
    (level l uses its first L - l rows).  Made by `SecretKey.random`; nothing here copies it to the host.  Device buffers
    the encryption wrappers stage host seeds and plaintexts through are cleared before they are freed; `s_ntt` itself
    and device arrays the caller passes are the caller's to clear."""

    def __init__(self, params, s_ntt):
        self.params, self.s_ntt = params, s_ntt
        self._encoder = None   # (measure_noise's q_mod_t and delta per level: made on first use)

    @classmethod
    def random(cls, params, seed=None):
        """SecretKey::random (secret_key.rs:41-46): Poly::small(variance) of ChaCha8Rng::from_seed(seed) (32 bytes;
        None: from `secrets`), in Ntt form over the level-0 context (fhe_bfv_sample_small_dev)."""
        ctx = params.context_at_level(0)
        sd, _, own = _seeds(seed, 1, params.device)
        try:
            out = _alloc((ctx.nmoduli, params.degree), params.device)
            check(_lib.lib().fhe_bfv_sample_small_dev(ctx._h, params.variance, _dptr8(sd), 1, _dptr(out), 1,
                                                      _stream()))
        finally:
            _wipe([sd] if own else [])
        return cls(params, out)

    def encrypt(self, pt, level=0, a_seeds=None, e_seeds=None):
        """SecretKey::try_encrypt (secret_key.rs:100-134) of Delta-scaled plaintexts pt [..., L - level, N]
        (`Encoder.encode(..., scaled=True)`; [L - level, N] with several seeds: shared; None: the zero plaintext) ->
        [..., 2, L - level, N] Ntt.  c1 = Poly::random_from_seed(a_seeds[b]) (the wire format's seeded c1), the error
        is Poly::small of ChaCha8Rng::from_seed(e_seeds[b]); one a seed and one e seed per plaintext, seeds not given
        come from `secrets`.  numpy in -> numpy out; a device array in -> a device array out."""
        L = _lib.lib()
        return _encrypt(self.params, level, pt, a_seeds, e_seeds, True, lambda ctx, a, e, ptp, shared, out, b: (
            L.fhe_bfv_encrypt_sk_dev(ctx._h, self.params.variance, _dptr(self.s_ntt), _dptr8(a), _dptr8(e), ptp, shared,
                                     _dptr(out), b, _stream())))

    def decrypt(self, ct, level=0):
        """SecretKey::try_decrypt (secret_key.rs:198-247): ct [..., nparts, L - level, N] -> coefficients mod t
        [..., N] (Encoder.decode turns them into values).  The key stays on the device: numpy ciphertexts are
        uploaded."""
        if _is_dev(ct):
            return self.params.decrypt(self.s_ntt, ct, level)
        x = DeviceArray.from_numpy(_np(ct), max(self.params.device, 0))
        d = self.params.decrypt(self.s_ntt, x, level)
        try:
            return _from_limbs(_download(d)) if self.params.plaintext_limbs > 1 else _download(d)
        finally:
            _wipe([d])   # (the plaintext coefficients)

    def measure_noise(self, ct, level=0, plaintext=None):
        """SecretKey::measure_noise (secret_key.rs:55-98, fhe_bfv_measure_noise_dev): ct [..., nparts, L - level, N] ->
        [...] uint64, the bits of noise of each ciphertext.  plaintext=None measures against the ciphertext's own
        decryption (the reference); plaintext [..., N] coefficients in [0, t) (what `decrypt` returns, or
        `Encoder.decode`'s inverse) measures against the plaintext the caller expects, which keeps growing after the
        ciphertext has stopped decrypting to it.  The key, the phase and the error stay on the device: numpy inputs
        are uploaded (and the staged plaintext is cleared); numpy in -> numpy out (an int without batch dimensions), a
        device array in -> a device array."""
        par = self.params
        if not 0 <= level <= par.max_level:
            raise FheError(-12, "InvalidLevel")
        sc = par.plain_scaler(level)
        nparts = int(ct.shape[-3])
        b = sc.from_ctx._batch(ct) // nparts
        lead = tuple(int(d) for d in ct.shape[:-3])
        if self._encoder is None:
            self._encoder = par.encoder()
        enc = self._encoder
        wt = par.plaintext_limbs
        if wt > 1 and plaintext is not None and not _is_dev(plaintext):
            plaintext = _to_limbs(plaintext, wt)   # (Python ints [..., N] -> limbs [..., N, W_t])
        want = lead + ((par.degree,) if wt == 1 else (par.degree, wt))
        if plaintext is not None and (tuple(int(d) for d in plaintext.shape) != want):
            raise FheError(-1, "plaintext: expected one [N] row of coefficients per ciphertext")
        host = not _is_dev(ct)
        staged = []
        try:
            x = DeviceArray.from_numpy(_np(ct), max(par.device, 0)) if host else ct
            m = None
            if plaintext is not None:
                m = plaintext
                if not _is_dev(plaintext):
                    m = DeviceArray.from_numpy(_np(plaintext), max(par.device, 0))
                    staged.append(m)
            out = DeviceArray(lead or (1,), x.device) if host else _empty_dev(ct, lead or (1,))
            check(_lib.lib().fhe_bfv_measure_noise_dev(enc._h, sc._h, _dptr(self.s_ntt), _dptr(x), nparts,
                                                       _dptr(m) if m is not None else None, _dptr(out), b, _stream()))
            if not host:
                return out
            r = out.download()
            return r if lead else int(r[0])
        finally:
            _wipe(staged)


class PublicKey:
    """bfv::PublicKey (F/bfv/keys/public_key.rs) on the device: the encryption of zero under `sk` (PublicKey::new,
    :26-30), [2, L, N] Ntt, plus its copies switched down to each level used (made once, then cached)."""

    def __init__(self, sk, a_seed=None, e_seed=None):
        self.params = sk.params
        dev = self.params.device
        a, _, own_a = _seeds(a_seed, 1, dev)
        e, _, own_e = _seeds(e_seed, 1, dev)
        try:   # (device seeds in: the key stays on the device)
            c = sk.encrypt(None, 0, a_seeds=a, e_seeds=e)
        finally:
            _wipe([x for x, own in ((a, own_a), (e, own_e)) if own])
        self.c = c.reshape(2, c.shape[-2], c.shape[-1])
        self._levels = {0: self.c}

    @classmethod
    def from_ciphertext(cls, params, c):
        """A key whose ciphertext c [2, L, N] (Ntt, level 0, on the device) was made elsewhere: the collective key of the
        multiparty protocol (`PublicKeyShare.aggregate`)."""
        self = cls.__new__(cls)
        self.params, self.c = params, c
        self._levels = {0: c}
        return self

    def at_level(self, level):
        """The key over the context of `level` (Ciphertext::switch_down until the level matches, public_key.rs:66-74)."""
        if level not in self._levels:
            if not 0 <= level <= self.params.max_level:
                raise FheError(-12, "InvalidLevel")
            ctx = self.params.context_at_level(0)
            self._levels[level] = ctx.ciphertext_switch_to_level(self.c, level)
        return self._levels[level]

    def encrypt(self, pt, level=0, seeds=None):
        """PublicKey::try_encrypt (public_key.rs:47-97) of Delta-scaled plaintexts pt [..., L - level, N] (as
        SecretKey.encrypt) -> [..., 2, L - level, N] Ntt; u, e1, e2 are three consecutive Poly::small draws of
        ChaCha8Rng::from_seed(seeds[b]), one seed per plaintext; seeds not given come from `secrets`."""
        pk = self.at_level(level)
        L = _lib.lib()
        return _encrypt(self.params, level, pt, seeds, None, False, lambda ctx, sd, _e, ptp, shared, out, b: (
            L.fhe_bfv_encrypt_pk_dev(ctx._h, self.params.variance, _dptr(pk), _dptr8(sd), ptp, shared, _dptr(out), b,
                                     _stream())))


def _download(x):
    return x.download() if isinstance(x, DeviceArray) else x.cpu().numpy().view(np.uint64)


def _encrypt(params, level, pt, seeds, seeds2, two, call):
    """The shared body of SecretKey.encrypt (two seed sets: a, e) and PublicKey.encrypt (one): checks that there is one
    seed of each set per plaintext, stages numpy plaintexts and host seeds (cleared again after the call), sizes the
    output and runs call(ctx, seeds, seeds2, pt_ptr, pt_shared, out, batch)."""
    if not 0 <= level <= params.max_level:
        raise FheError(-12, "InvalidLevel")
    ctx = params.context_at_level(level)
    if pt is not None and len(pt.shape) > 2:
        count = int(np.prod(pt.shape[:-2]))
    elif seeds is not None:
        count = _seed_count(seeds)
    elif two and seeds2 is not None:
        count = _seed_count(seeds2)
    else:
        count = 1
    if pt is not None and (int(pt.shape[-2]), int(pt.shape[-1])) != (ctx.nmoduli, params.degree):
        raise FheError(-1, "the plaintext must be [..., L - level, N] at the encryption level")
    staged = []
    try:
        sd, n, own = _seeds(seeds, count, params.device)
        if own:
            staged.append(sd)
        sd2 = None
        if two:
            sd2, n2, own2 = _seeds(seeds2, n, params.device)
            if own2:
                staged.append(sd2)
            if n2 != n:
                raise FheError(-1, "one e seed per a seed: %d a seeds, %d e seeds" % (n, n2))
        lead, batch, shared = _batch_of(pt, n)
        if batch != n:
            raise FheError(-1, "one seed per plaintext: %d plaintexts, %d seeds" % (batch, n))
        host = not _is_dev(pt if pt is not None else seeds)   # numpy (or host seeds, for pt None) in -> numpy out
        if host and pt is not None:
            pt = DeviceArray.from_numpy(_np(pt), max(params.device, 0))
            staged.append(pt)
        oshape = lead + (2, ctx.nmoduli, params.degree)
        out = DeviceArray(oshape, max(params.device, 0)) if host else _empty_dev(pt if pt is not None else seeds,
                                                                                 oshape)
        check(call(ctx, sd, sd2, _dptr(pt) if pt is not None else None, shared, out, batch))
        return out.download() if host else out
    finally:
        _wipe(staged)


class BfvParameters:
    """The device-table part of bfv::BfvParameters (crates/fhe/src/bfv/parameters.rs:560-738):
    per-level contexts, the extended multiplication basis and per-level mul parameters."""

    def __init__(self, degree, plaintext_modulus, moduli=None, moduli_sizes=None, device=0, tables_fn=None, variance=10):
        """tables_fn(modulus, degree) -> dict(omegas, omegas_shoup, zetas_inv, zetas_inv_shoup, size_inv,
        size_inv_shoup): the host's NttOperator tables for every modulus the parameter set builds a context over
        (fhe_params_create_with_tables); None: the engine's own psi (fhe_params_create).  variance: the centered
        binomial variance of the secret key and the errors (BfvParametersBuilder::set_variance, default 10); the
        encryption calls return FheError -24 (InvalidVariance) outside [1, 32]."""
        L = _lib.lib()
        if moduli_sizes:
            sizes = (C.c_size_t * len(moduli_sizes))(*moduli_sizes)
            out = np.zeros(len(moduli_sizes), dtype=np.uint64)
            check(L.fhe_generate_moduli(sizes, len(moduli_sizes), degree, _ptr(out)))
            moduli = [int(x) for x in out]
        m = _np(moduli)
        h = C.c_void_p()
        plaintext_modulus = int(plaintext_modulus)
        big = plaintext_modulus >> 64 != 0   # PlaintextModulus::Large: the limbs go through the _big constructors
        tl = _limbs(plaintext_modulus)
        if tables_fn is None and big:
            check(L.fhe_params_create_big(device, degree, len(m), _ptr(m), _ptr(tl), len(tl), C.byref(h)))
        elif tables_fn is None:
            check(L.fhe_params_create(device, degree, len(m), _ptr(m), plaintext_modulus, C.byref(h)))
        elif big:
            cb = _tables_cb(tables_fn)
            check(L.fhe_params_create_big_with_tables(device, degree, len(m), _ptr(m), _ptr(tl), len(tl), cb, None,
                                                      C.byref(h)))
        else:
            cb = _tables_cb(tables_fn)
            check(L.fhe_params_create_with_tables(device, degree, len(m), _ptr(m), plaintext_modulus, cb, None,
                                                  C.byref(h)))
            # (the C side calls `cb` only while fhe_params_create_with_tables runs and caches every table per modulus:
            # nothing has to keep the callback alive afterwards)
        self._h = h
        self.degree, self.plaintext, self.moduli, self.device = degree, plaintext_modulus, [int(x) for x in m], device
        self.variance = variance
        self.max_level = L.fhe_params_max_level(h)
        self.plaintext_limbs = int(L.fhe_params_plaintext_limbs(h))   # W_t: 1 unless t exceeds 64 bits

    def __del__(self):
        if getattr(self, "_h", None) is not None and _lib._lib is not None:
            _lib._lib.fhe_params_destroy(self._h)

    def _get(self, fn, level):
        h = C.c_void_p()
        check(getattr(_lib.lib(), fn)(self._h, level, C.byref(h)))
        return h

    def context_at_level(self, level):
        return Context(None, None, _handle=self._get("fhe_params_ctx", level), _owner=self)

    def mul_context_at_level(self, level):
        return Context(None, None, _handle=self._get("fhe_params_mul_ctx", level), _owner=self)

    def extender(self, level):
        return Scaler(self.context_at_level(level), self.mul_context_at_level(level),
                      _handle=self._get("fhe_params_extender", level), _owner=self)

    def down_scaler(self, level):
        return Scaler(self.mul_context_at_level(level), self.context_at_level(level),
                      _handle=self._get("fhe_params_down_scaler", level), _owner=self)

    def encoder(self, tables_fn=None):
        """The parameter set's `Encoder` (fhe_encoder_create).  tables_fn(t, degree) -> the host's NttOperator tables
        for t (same dict as the constructor's); None: the engine's own psi."""
        return Encoder(self, tables_fn)

    def plaintext_context(self):
        """parameters.rs:578-595: the shortest prefix of the moduli with >= bits(t) + 60 bits."""
        if getattr(self, "_plain_ctx", None) is None:
            acc, count = 0, 0
            for m in self.moduli:
                acc += int(m).bit_length()
                count += 1
                if acc >= int(self.plaintext).bit_length() + 60:
                    break
            self._plain_ctx = Context(self.moduli[:max(1, count)], self.degree, device=self.device)
        return self._plain_ctx

    def plain_scaler(self, level):
        """CipherPlainContext::scaler (parameters.rs:636-643): ciphertext level -> plaintext context, t / q."""
        cache = self.__dict__.setdefault("_plain_scalers", {})
        if level not in cache:
            ctx = self.context_at_level(level)
            q = 1
            for m in ctx.moduli:
                q *= int(m)
            cache[level] = Scaler(ctx, self.plaintext_context(), int(self.plaintext), q)
        return cache[level]

    def decrypt(self, s_ntt, ct, level=0):
        """SecretKey::try_decrypt (secret_key.rs:198-247, small plaintext modulus): s_ntt [L, N] is the
        secret key over the ciphertext context in Ntt form; ct [..., nparts, L, N] -> [..., N] in [0, t)."""
        L = _lib.lib()
        sc = self.plain_scaler(level)
        nparts = int(ct.shape[-3])
        b = sc.from_ctx._batch(ct) // nparts
        oshape = tuple(ct.shape[:-3]) + (self.degree,)
        if self.plaintext_limbs > 1:
            # the Large branch (secret_key.rs:238-250, fhe_bfv_decrypt_big_dev): device in -> limbs [..., N, W_t];
            # numpy in -> Python ints [..., N] (staged: the big forms have no host-pointer twin)
            if getattr(self, "_big_encoder", None) is None:
                self._big_encoder = self.encoder()
            host = not _is_dev(ct)
            staged = [DeviceArray.from_numpy(_np(a), max(self.device, 0)) for a in (ct, s_ntt)] if host else []
            x, sk = staged if host else (ct, s_ntt)
            out = (DeviceArray(oshape + (self.plaintext_limbs,), x.device) if host
                   else _empty_dev(ct, oshape + (self.plaintext_limbs,)))
            try:
                check(L.fhe_bfv_decrypt_big_dev(self._big_encoder._h, sc._h, _dptr(sk), _dptr(x), nparts, _dptr(out), b,
                                                _stream()))
                return _from_limbs(out.download()) if host else out
            finally:
                _wipe(staged[1:] + ([out] if host else []))
        if _is_dev(ct):
            out = _empty_dev(ct, oshape)
            check(L.fhe_bfv_decrypt_dev(sc._h, int(self.plaintext), _dptr(s_ntt), _dptr(ct), nparts, _dptr(out), b,
                                        _stream()))
            return out
        x, sk = _np(ct), _np(s_ntt)
        out = np.zeros(oshape, dtype=np.uint64)
        check(L.fhe_bfv_decrypt(sc._h, int(self.plaintext), _ptr(sk), _ptr(x), nparts, _ptr(out), b))
        return out


class Multiplicator:
    """bfv::Multiplicator (crates/fhe/src/bfv/ops/mul.rs:21-243)."""

    def __init__(self, extender_lhs, extender_rhs, down_scaler, rk=None, mod_switch=False, _handle=None, _keep=()):
        self._keep = (extender_lhs, extender_rhs, down_scaler, rk) + tuple(_keep)
        if _handle is None:
            h = C.c_void_p()
            check(_lib.lib().fhe_mul_create(extender_lhs._h, extender_rhs._h, down_scaler._h,
                                            rk.ksk._h if rk is not None else None, 1 if mod_switch else 0, C.byref(h)))
            _handle = h
        self._h = _handle
        p, r = C.c_size_t(), C.c_size_t()
        check(_lib.lib().fhe_mul_out_shape(self._h, C.byref(p), C.byref(r)))
        self.out_parts, self.out_rows = p.value, r.value

    @classmethod
    def default(cls, params: BfvParameters, rk: RelinearizationKey = None, level=0, mod_switch=False):
        """Multiplicator::default(rk) (+ enable_mod_switching); rk=None gives `&ct * &ct`."""
        h = C.c_void_p()
        check(_lib.lib().fhe_mul_create_default(params._h, level, rk.ksk._h if rk is not None else None,
                                                1 if mod_switch else 0, C.byref(h)))
        m = cls(None, None, None, rk, mod_switch, _handle=h, _keep=(params,))
        m.base_ctx = params.context_at_level(level)
        return m

    def __del__(self):
        if getattr(self, "_h", None) is not None and _lib._lib is not None:
            _lib._lib.fhe_mul_destroy(self._h)

    def basis(self):
        """Moduli of the multiplication context (Multiplicator::mul_ctx)."""
        n = C.c_size_t()
        check(_lib.lib().fhe_mul_basis(self._h, C.byref(n), None))
        out = np.zeros(n.value, dtype=np.uint64)
        check(_lib.lib().fhe_mul_basis(self._h, C.byref(n), _ptr(out)))
        return [int(x) for x in out]

    def set_chunk(self, chunk):
        """Ciphertext pairs per pipeline pass (0 = default); an option of this handle (fhe_mul_set_chunk)."""
        check(_lib.lib().fhe_mul_set_chunk(self._h, chunk))
        return self

    def set_streams(self, n):
        """2 (default): chunks alternate between the caller's stream and an internal one; 1: caller's stream only."""
        check(_lib.lib().fhe_mul_set_streams(self._h, n))
        return self

    def options(self):
        c, s = C.c_size_t(), C.c_size_t()
        check(_lib.lib().fhe_mul_get_options(self._h, C.byref(c), C.byref(s)))
        return dict(chunk=c.value, streams=s.value)

    def multiply(self, lhs, rhs):
        """Multiplicator::multiply: lhs, rhs [..., 2, L, N] Ntt -> [..., parts, rows, N] Ntt."""
        L = _lib.lib()
        if tuple(lhs.shape) != tuple(rhs.shape) or lhs.shape[-3] != 2:
            raise FheError(-13, "MultiplicationPolynomialCount: expected 2-part ciphertexts of equal shape")
        b = 1
        for d in lhs.shape[:-3]:
            b *= d
        oshape = tuple(lhs.shape[:-3]) + (self.out_parts, self.out_rows, lhs.shape[-1])
        if _is_dev(lhs):
            out = _empty_dev(lhs, oshape)
            check(L.fhe_bfv_mul_dev(self._h, _dptr(lhs), _dptr(rhs), _dptr(out), b, _stream()))
            return out
        x, y = _np(lhs), _np(rhs)
        out = np.zeros(oshape, dtype=np.uint64)
        check(L.fhe_bfv_mul(self._h, _ptr(x), _ptr(y), _ptr(out), b))
        return out

    def tensor(self, lhs, rhs):
        """`&ct * &ct` (ops/mod.rs:259-358) for any number of parts: lhs [..., la, L, N], rhs [..., lb, L, N]
        -> [..., la + lb - 1, L, N]; no relinearisation."""
        L = _lib.lib()
        if tuple(lhs.shape[:-3]) != tuple(rhs.shape[:-3]) or tuple(lhs.shape[-2:]) != tuple(rhs.shape[-2:]):
            raise FheError(-11, "ParameterMismatch: operands of different batch shape or level")
        la, lb = int(lhs.shape[-3]), int(rhs.shape[-3])
        b = 1
        for d in lhs.shape[:-3]:
            b *= d
        oshape = tuple(lhs.shape[:-3]) + (la + lb - 1,) + tuple(lhs.shape[-2:])
        if _is_dev(lhs):
            out = _empty_dev(lhs, oshape)
            check(L.fhe_bfv_tensor_dev(self._h, la, lb, _dptr(lhs), _dptr(rhs), _dptr(out), b, _stream()))
            return out
        x, y = _np(lhs), _np(rhs)
        out = np.zeros(oshape, dtype=np.uint64)
        check(L.fhe_bfv_tensor(self._h, la, lb, _ptr(x), _ptr(y), _ptr(out), b))
        return out


# ---- zq::primes (host) ---------------------------------------------------------------------
def generate_prime(num_bits, modulo, upper_bound):
    p = _lib.lib().fhe_generate_prime(num_bits, modulo, upper_bound)
    return p or None


def supports_opt(p):
    return bool(_lib.lib().fhe_supports_opt(p))


def is_prime(p):
    return bool(_lib.lib().fhe_is_prime(p))


def generate_moduli(sizes, degree):
    arr = (C.c_size_t * len(sizes))(*sizes)
    out = np.zeros(len(sizes), dtype=np.uint64)
    check(_lib.lib().fhe_generate_moduli(arr, len(sizes), degree, _ptr(out)))
    return [int(x) for x in out]


def device_count():
    return _lib.lib().fhe_device_count()


# ---- execution options ------------------------------------------------------------------------------
def set_f64(on=True):
    """fhe_engine_set_f64: rows whose moduli are all below 2^50 take the FP64-FMA kernels (default) or the integer ones."""
    _lib.lib().fhe_engine_set_f64(1 if on else 0)


def get_f64():
    return bool(_lib.lib().fhe_engine_get_f64())


# ---- profiling ---------------------------------------------------------------------------------
def prof_enable(on=True):
    _lib.lib().fhe_prof_enable(1 if on else 0)


def prof_reset():
    _lib.lib().fhe_prof_reset()


def prof_report():
    """{launch label: (launches, total_ms)} from the HIP events the launches carried (entries of one label summed)."""
    out = {}
    for label, _sym, n, ms in prof_entries():
        a = out.get(label, (0, 0.0))
        out[label] = (a[0] + n, a[1] + ms)
    return out


def prof_entries():
    """[(launch label, kernel symbol, launches, total_ms)]: one entry per kernel instantiation, named as rocprofv3 names
    it (fhe_prof_get + fhe_prof_get_symbol)."""
    L = _lib.lib()
    out = []
    for i in range(L.fhe_prof_count()):
        name, sym = C.create_string_buffer(64), C.create_string_buffer(512)
        n, ms = C.c_uint64(), C.c_double()
        check(L.fhe_prof_get(i, name, 64, C.byref(n), C.byref(ms)))
        check(L.fhe_prof_get_symbol(i, sym, 512))
        out.append((name.value.decode(), sym.value.decode(), n.value, ms.value))
    return out


def workspace_trim():
    """Frees the engine's idle scratch buffers; returns the bytes released."""
    return int(_lib.lib().fhe_workspace_trim())


WORKSPACE_DEFAULT = (1 << 64) - 1


def workspace_set_limit(per_stream_bytes=0, total_bytes=WORKSPACE_DEFAULT):
    """Bounds on the scratch the engine retains between calls (fhe_workspace_set_limit; 0 = none; the default total
    is a quarter of the device's memory)."""
    check(_lib.lib().fhe_workspace_set_limit(int(per_stream_bytes), int(total_bytes)))


def workspace_stats():
    h, u, b, o, a = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    check(_lib.lib().fhe_workspace_stats(C.byref(h), C.byref(u), C.byref(b), C.byref(o), C.byref(a)))
    return dict(held_bytes=h.value, in_use_bytes=u.value, blocks=b.value, owners=o.value, internal_streams=a.value)


def workspace_pool_stats(device=0):
    """What the driver says the library's two private pools on `device` hold (fhe_workspace_pool_stats)."""
    v = [C.c_size_t() for _ in range(4)]
    check(_lib.lib().fhe_workspace_pool_stats(int(device), *[C.byref(x) for x in v]))
    return dict(scratch_reserved_bytes=v[0].value, scratch_used_bytes=v[1].value,
                buffers_reserved_bytes=v[2].value, buffers_used_bytes=v[3].value)


UBENCH_KINDS = {"mad_u64_u32": 0, "mul_lo_u32": 1, "mul_hi_u32": 2, "shoup_lazy": 3, "fwd_butterfly": 4,
                "fwd_butterfly_narrow": 5, "inv_butterfly": 6, "shoup_mac": 7, "tensor_mul": 8, "tensor_mac2": 9,
                # round 6: the FP64-FMA forms for moduli below 2^50 (csrc/zq_f64.hpp)
                "f64_fma": 10, "f64_rndne": 11, "f64_mulmod": 12, "f64_fwd_butterfly": 13, "f64_inv_butterfly": 14,
                "f64_mac": 15}


def ubench_int(kind, min_seconds=0.05, device=0):
    """Register-resident integer-issue microbenchmark (fhe_ubench_int): lane-operations per second chip-wide."""
    v = C.c_double()
    check(_lib.lib().fhe_ubench_int(device, UBENCH_KINDS[kind] if isinstance(kind, str) else int(kind),
                                    float(min_seconds), C.byref(v)))
    return v.value


def ubench_scaler(scaler, min_seconds=0.05):
    """RnsScaler::scale's no-HBM ceiling for this scaler's kernel instance (fhe_ubench_scaler): columns per second."""
    v = C.c_double()
    check(_lib.lib().fhe_ubench_scaler(scaler._h, float(min_seconds), C.byref(v)))
    return v.value


def ubench_copy(nbytes, min_seconds=0.05, device=0):
    """The box's streaming rate (fhe_ubench_copy): read + write bytes per second of a 16-byte-per-lane copy."""
    v = C.c_double()
    check(_lib.lib().fhe_ubench_copy(int(device), int(nbytes), float(min_seconds), C.byref(v)))
    return v.value


def device_mem_info(device=0):
    f, t = C.c_size_t(), C.c_size_t()
    check(_lib.lib().fhe_device_mem_info(device, C.byref(f), C.byref(t)))
    return f.value, t.value


# ---- multiparty BFV (crates/fhe/src/mbfv/): shares and their aggregation on the device -------------------------
# A party's secret is a `SecretKey` (s_ntt [L, N] on the device); `SecretKey(params, s)` with s [P, L, N] holds P
# parties, and every share made from it carries that leading party dimension: one call makes all P shares.  Public
# inputs (the CRP, ciphertexts, a public key) are numpy arrays, torch tensors or DeviceArrays; numpy in -> numpy out.

def _dev_copy(dst, src, nbytes):
    check(_lib.lib().fhe_buf_copy_async(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), nbytes, _stream()))


def _nbytes(x):
    return int(x.numel()) * int(x.element_size())


class _Staging:
    """Device copies of the host inputs of one call (cleared again when `secret`), and the kind of its result."""

    def __init__(self, params, ref):
        self.device = max(params.device, 0)
        self.host = not _is_dev(ref)
        self.ref = ref
        self.secret = []
        self.keep = []    # (staged copies stay alive until the object goes: the calls that read them are enqueued by then)

    def dev(self, x):
        if _is_dev(x):
            return x
        d = DeviceArray.from_numpy(_np(x), self.device)
        self.keep.append(d)
        return d

    def seeds(self, seeds, count):
        sd, n, own = _seeds(seeds, count, self.device)
        if own:
            self.secret.append(sd)
        if n != count:
            raise FheError(-1, "one seed per share: %d shares, %d seeds" % (count, n))
        return sd

    def out(self, shape):
        return DeviceArray(shape, self.device) if self.host else _empty_dev(self.ref, shape)

    def give(self, x):
        return x.download() if self.host else x

    def done(self):
        _wipe(self.secret)


def _parties(sk, params):
    """(party count or None, s_shared) of a SecretKey whose s_ntt is [L, N] or [P, L, N] over level 0."""
    sh = tuple(int(d) for d in sk.s_ntt.shape)
    if sh[-2:] != (len(params.moduli), params.degree) or len(sh) not in (2, 3):
        raise FheError(-1, "the secret must be [L, N] or [parties, L, N] over the level-0 context")
    return (None, 1) if len(sh) == 2 else (sh[0], 0)


def _level_ctx(params, level):
    if not 0 <= level <= params.max_level:
        raise FheError(-12, "InvalidLevel")
    return params.context_at_level(level)


def _mbfv_sum(ctx, shares, nshares, stride, npolys, base, out):
    check(_lib.lib().fhe_mbfv_aggregate_dev(ctx._h, _dptr(shares), nshares, stride, npolys,
                                            _dptr(base) if base is not None else None, _dptr(out), _stream()))


def _first_share(shares):
    """One party-batched share, or the first of a list (an empty list is the reference's NoShares)."""
    if not isinstance(shares, (list, tuple)):
        return shares
    if not shares:
        raise FheError(-1, "NoShares: an aggregation needs at least one share")
    return shares[0]


def _stack_shares(st, shares, attr):
    """The share arrays of one party-batched share (leading party dimension) or of a list of single-party shares, as
    one device array [P, ...] (a list is copied into one; numpy arrays are uploaded)."""
    if not isinstance(shares, (list, tuple)):
        a = getattr(shares, attr)
        if not shares.parties:
            a = a.reshape((1,) + tuple(int(d) for d in a.shape))
        return st.dev(a)
    if not shares:
        raise FheError(-1, "NoShares")
    parts = [getattr(s, attr) for s in shares]
    if any(s.parties for s in shares):
        raise FheError(-1, "a list holds single-party shares; a share with a party dimension aggregates on its own")
    if not _is_dev(parts[0]):
        return st.dev(np.stack([_np(p) for p in parts]))
    out = _empty_dev(parts[0], (len(parts),) + tuple(int(d) for d in parts[0].shape))
    for i, p in enumerate(parts):
        _dev_copy(out[i], p, _nbytes(p))
    return out


class CommonRandomPoly:
    """mbfv::CommonRandomPoly (mbfv/crp.rs): `poly` [L, N] Ntt over the level-0 context, or [count, L, N] for a vector
    (CommonRandomPoly::new_vec: one per ciphertext modulus for the relinearization-key protocol)."""

    def __init__(self, params, poly):
        sh = tuple(int(d) for d in poly.shape)
        if sh[-2:] != (len(params.moduli), params.degree) or len(sh) not in (2, 3):
            raise FheError(-1, "a common random polynomial is [L, N] (a vector: [count, L, N]) over the level-0 context")
        self.params, self.poly = params, poly

    @classmethod
    def from_seed(cls, params, seeds):
        """The CRP every party derives from a public seed: Poly::random_from_seed per 32-byte seed
        (fhe_poly_from_seed_dev).  One seed -> [L, N]; a list or a [count, 32] array -> the vector [count, L, N]."""
        one = isinstance(seeds, (bytes, bytearray))
        ctx = params.context_at_level(0)
        if not _is_dev(seeds):   # host seeds -> a numpy polynomial (numpy in -> numpy out, as everywhere)
            if isinstance(seeds, (list, tuple)):
                seeds = b"".join(bytes(x) for x in seeds)
            if isinstance(seeds, (bytes, bytearray)):
                seeds = np.frombuffer(bytes(seeds), dtype=np.uint8)
        p = ctx.random_from_seed(seeds)
        return cls(params, p[0] if one else p)


class PublicKeyShare:
    """mbfv::PublicKeyShare (mbfv/public_key_gen.rs:32-57): p0_share = e - crp (.) s, [L, N] ([P, L, N] for P parties);
    one Poly::small draw of ChaCha8Rng::from_seed(seeds[party]) each."""

    def __init__(self, sk, crp, seeds=None):
        par = self.params = sk.params
        self.crp = crp
        if len(crp.poly.shape) != 2:
            raise FheError(-1, "the public-key protocol takes one common random polynomial")
        P, shared = _parties(sk, par)
        self.parties = P is not None
        ctx = par.context_at_level(0)
        st = _Staging(par, crp.poly)
        try:
            sd = st.seeds(seeds, P or 1)
            out = st.out(((P,) if self.parties else ()) + (ctx.nmoduli, par.degree))
            check(_lib.lib().fhe_mbfv_pk_share_dev(ctx._h, par.variance, _dptr(st.dev(crp.poly)), _dptr(sk.s_ntt), shared,
                                                   _dptr8(sd), _dptr(out), P or 1, _stream()))
            self.p0_share = st.give(out)
        finally:
            st.done()

    @staticmethod
    def aggregate(shares):
        """PublicKey::from_shares (public_key_gen.rs:60-77): [sum of the p0 shares, crp] as a `PublicKey`."""
        first = _first_share(shares)
        par, crp = first.params, first.crp
        ctx = par.context_at_level(0)
        st = _Staging(par, first.p0_share)
        h = _stack_shares(st, shares, "p0_share")
        PL = ctx.nmoduli * par.degree
        c = _alloc((2, ctx.nmoduli, par.degree), par.device)
        _mbfv_sum(ctx, h, int(h.shape[0]), PL, 1, None, c[0])
        _dev_copy(c[1], st.dev(crp.poly), PL * 8)
        return PublicKey.from_ciphertext(par, c)


class SecretKeySwitchShare:
    """mbfv::SecretKeySwitchShare (mbfv/secret_key_switch.rs:38-95): h = e + c1 (.) (s_in - s_out) for every ciphertext
    of ct [..., 2, L - level, N]: h_share [..., L - level, N], with a leading party dimension when the keys hold P
    parties.  One Poly::small draw per (party, ciphertext), seeds in that order."""

    def __init__(self, sk_in, sk_out, ct, level=0, seeds=None):
        par = self.params = sk_in.params
        self.level, self.ct = level, ct
        ctx = _level_ctx(par, level)
        P, shared = _parties(sk_in, par)
        if sk_out is not None and _parties(sk_out, par) != (P, shared):
            raise FheError(-3, "ParameterMismatch: the input and output secrets hold different parties")
        self.parties = P is not None
        if tuple(int(d) for d in ct.shape[-3:]) != (2, ctx.nmoduli, par.degree):
            raise FheError(-13, "InvalidPolynomialCount: the multiparty switches take ciphertexts of 2 parts at `level`")
        lead = tuple(int(d) for d in ct.shape[:-3])
        B = int(np.prod(lead)) if lead else 1
        PL = ctx.nmoduli * par.degree
        L = _lib.lib()
        st = _Staging(par, ct)
        try:
            sd = st.seeds(seeds, (P or 1) * B)
            x = st.dev(ct).reshape((B, 2, ctx.nmoduli, par.degree))
            out = st.out(((P,) if self.parties else ()) + lead + (ctx.nmoduli, par.degree))
            c1 = C.c_void_p(_dptr(x).value + PL * 8)
            s_out = lambda p: None if sk_out is None else _dptr(sk_out.s_ntt if p is None else sk_out.s_ntt[p])   # noqa: E731
            if not self.parties:
                check(L.fhe_mbfv_sks_share_dev(ctx._h, par.variance, _dptr(sk_in.s_ntt), s_out(None), 1, c1, 2 * PL,
                                               _dptr8(sd), _dptr(out), B, _stream()))
            elif B == 1:   # P parties, one ciphertext: one call, a secret per item
                check(L.fhe_mbfv_sks_share_dev(ctx._h, par.variance, _dptr(sk_in.s_ntt), s_out(None), 0, c1, 0, _dptr8(sd),
                                               _dptr(out), P, _stream()))
            else:          # P parties, B ciphertexts: one call per party, its secret shared by the batch
                for p in range(P):
                    check(L.fhe_mbfv_sks_share_dev(ctx._h, par.variance, _dptr(sk_in.s_ntt[p]), s_out(p), 1, c1, 2 * PL,
                                                   C.c_void_p(_dptr8(sd).value + 32 * B * p), _dptr(out[p]), B, _stream()))
            self.h_share = st.give(out)
        finally:
            st.done()

    @staticmethod
    def _summed(shares):
        """(params, level, ctx, staging, c0 + sum of the shares [B, L, N] on the device, the ciphertexts [B, 2, L, N])"""
        first = _first_share(shares)
        par, level = first.params, first.level
        ctx = _level_ctx(par, level)
        st = _Staging(par, first.h_share)
        h = _stack_shares(st, shares, "h_share")
        PL = ctx.nmoduli * par.degree
        B = int(np.prod(h.shape[1:-2])) if len(h.shape) > 3 else 1
        x = st.dev(first.ct).reshape((B, 2, ctx.nmoduli, par.degree))
        return par, ctx, st, h, x, B, PL

    @staticmethod
    def aggregate(shares):
        """Ciphertext::from_shares (secret_key_switch.rs:98-115): [c0 + sum of the shares, c1], shaped like the input
        ciphertexts."""
        first = _first_share(shares)
        par, ctx, st, h, x, B, PL = SecretKeySwitchShare._summed(shares)
        out = st.out(tuple(int(d) for d in first.ct.shape))
        _dev_copy(out, x, B * 2 * PL * 8)
        # (c0 of ciphertext b sits at b 2 L N: one launch per ciphertext keeps the aggregator's contiguous layout)
        o = out.reshape((B, 2, ctx.nmoduli, par.degree))
        for b in range(B):
            check(_lib.lib().fhe_mbfv_aggregate_dev(ctx._h, C.c_void_p(_dptr(h).value + b * PL * 8), int(h.shape[0]), B * PL,
                                                    1, _dptr(o[b][0]), _dptr(o[b][0]), _stream()))
        return st.give(out)


class DecryptionShare(SecretKeySwitchShare):
    """mbfv::DecryptionShare (mbfv/secret_key_switch.rs:133-142): the key switch to the zero key, h = e + c1 (.) s."""

    def __init__(self, sk, ct, level=0, seeds=None):
        super().__init__(sk, None, ct, level, seeds)

    @staticmethod
    def aggregate(shares):
        """Plaintext::from_shares (secret_key_switch.rs:145-186, fhe_mbfv_decrypt_dev): the plaintext coefficients
        [..., N] in [0, t) (`Encoder.decode` turns them into values)."""
        first = _first_share(shares)
        par, ctx, st, h, x, B, PL = SecretKeySwitchShare._summed(shares)
        sc = par.plain_scaler(first.level)
        wt = par.plaintext_limbs
        out = st.out(tuple(int(d) for d in first.ct.shape[:-3]) + ((par.degree,) if wt == 1 else (par.degree, wt)))
        if wt > 1:   # the Large tail (fhe_mbfv_decrypt_big_dev): limbs [..., N, W_t], Python ints for host input
            if getattr(par, "_big_encoder", None) is None:
                par._big_encoder = par.encoder()
            check(_lib.lib().fhe_mbfv_decrypt_big_dev(par._big_encoder._h, sc._h, _dptr(x), _dptr(h), int(h.shape[0]),
                                                      B * PL, _dptr(out), B, _stream()))
        else:
            check(_lib.lib().fhe_mbfv_decrypt_dev(sc._h, int(par.plaintext), _dptr(x), _dptr(h), int(h.shape[0]), B * PL,
                                                  _dptr(out), B, _stream()))
        if not st.host:
            return out
        try:
            return _from_limbs(out.download()) if wt > 1 else out.download()
        finally:
            _wipe([out])   # (the plaintext coefficients)


class PublicKeySwitchShare:
    """mbfv::PublicKeySwitchShare (mbfv/public_key_switch.rs:33-92): h0 = pk0 (.) u + s (.) c1 + e0, h1 = pk1 (.) u + e1
    for every ciphertext of ct [..., 2, L - level, N]: `h` [..., 2, L - level, N], with a leading party dimension when
    the key holds P parties.  Three draws (u, e0, e1) of one seed per (party, ciphertext)."""

    def __init__(self, sk, pk, ct, level=0, seeds=None):
        par = self.params = sk.params
        self.level, self.ct = level, ct
        ctx = _level_ctx(par, level)
        P, shared = _parties(sk, par)
        self.parties = P is not None
        if tuple(int(d) for d in ct.shape[-3:]) != (2, ctx.nmoduli, par.degree):
            raise FheError(-13, "InvalidPolynomialCount: the multiparty switches take ciphertexts of 2 parts at `level`")
        lead = tuple(int(d) for d in ct.shape[:-3])
        B = int(np.prod(lead)) if lead else 1
        L = _lib.lib()
        st = _Staging(par, ct)
        try:
            sd = st.seeds(seeds, (P or 1) * B)
            x = st.dev(ct)
            pkl = st.dev(pk.at_level(level))
            out = st.out(((P,) if self.parties else ()) + lead + (2, ctx.nmoduli, par.degree))
            if not self.parties:
                check(L.fhe_mbfv_pks_share_dev(ctx._h, par.variance, _dptr(sk.s_ntt), 1, _dptr(pkl), _dptr(x), 0,
                                               _dptr8(sd), _dptr(out), B, _stream()))
            elif B == 1:
                check(L.fhe_mbfv_pks_share_dev(ctx._h, par.variance, _dptr(sk.s_ntt), 0, _dptr(pkl), _dptr(x), 1,
                                               _dptr8(sd), _dptr(out), P, _stream()))
            else:
                for p in range(P):
                    check(L.fhe_mbfv_pks_share_dev(ctx._h, par.variance, _dptr(sk.s_ntt[p]), 1, _dptr(pkl), _dptr(x), 0,
                                                   C.c_void_p(_dptr8(sd).value + 32 * B * p), _dptr(out[p]), B, _stream()))
            self.h = st.give(out)
        finally:
            st.done()

    @staticmethod
    def aggregate(shares):
        """Ciphertext::from_shares (public_key_switch.rs:95-113): [c0 + sum of the h0 shares, sum of the h1 shares]."""
        first = _first_share(shares)
        par = first.params
        ctx = _level_ctx(par, first.level)
        st = _Staging(par, first.h)
        h = _stack_shares(st, shares, "h")
        PL = ctx.nmoduli * par.degree
        B = int(np.prod(h.shape[1:-3])) if len(h.shape) > 4 else 1
        x = st.dev(first.ct)
        out = st.out(tuple(int(d) for d in first.ct.shape))
        # base: the ciphertexts' c0 with zero second parts
        check(_lib.lib().fhe_buf_zero_async(C.c_void_p(out.data_ptr()), B * 2 * PL * 8, _stream()))
        o, xi = out.reshape((B, 2, ctx.nmoduli, par.degree)), x.reshape((B, 2, ctx.nmoduli, par.degree))
        for b in range(B):
            _dev_copy(o[b][0], xi[b][0], PL * 8)
        _mbfv_sum(ctx, h, int(h.shape[0]), B * 2 * PL, 2 * B, out, out)
        return st.give(out)


class RelinKeyGenerator:
    """mbfv::RelinKeyGenerator (mbfv/relin_key_gen.rs:65-110): the two rounds of the relinearization-key protocol for
    one party, or for P parties when `sk` holds P secrets.  `u` is the party's ephemeral secret (RelinKeyGenerator::new's
    Poly::small draw of ChaCha8Rng::from_seed(u_seeds[party])); it stays on the device."""

    def __init__(self, sk, crp, u_seeds=None):
        par = self.params = sk.params
        ctx = par.context_at_level(0)
        if ctx.nmoduli == 1:
            raise FheError(-17, "KeySwitchingNotSupported")
        if len(crp.poly.shape) != 3 or int(crp.poly.shape[0]) != ctx.nmoduli:
            raise FheError(-1, "InvalidCommonRandomPolynomialCount: one common random polynomial per ciphertext modulus")
        self.sk, self.crp = sk, crp
        self.P, self.shared = _parties(sk, par)
        count = self.P or 1
        sd, n, own = _seeds(u_seeds, count, par.device)
        try:
            if n != count:
                raise FheError(-1, "one seed per party")
            u = _alloc((count, ctx.nmoduli, par.degree), par.device)
            check(_lib.lib().fhe_bfv_sample_small_dev(ctx._h, par.variance, _dptr8(sd), 1, _dptr(u), count, _stream()))
        finally:
            _wipe([sd] if own else [])
        self.u = u if self.P else u[0]

    def _round(self, fn, a0, a1, seeds, ref):
        par = self.params
        ctx = par.context_at_level(0)
        Lm = ctx.nmoduli
        st = _Staging(par, ref)
        try:
            sd = st.seeds(seeds, self.P or 1)
            shape = ((self.P,) if self.P else ()) + (Lm, Lm, par.degree)
            h0, h1 = st.out(shape), st.out(shape)
            ins = [_dptr(st.dev(a)) for a in ((a0,) if a1 is None else (a0, a1))]
            check(fn(ctx._h, par.variance, _dptr(self.sk.s_ntt), _dptr(self.u), self.shared, *ins, _dptr8(sd), _dptr(h0),
                     _dptr(h1), self.P or 1, _stream()))
            return RelinKeyShare(par, st.give(h0), st.give(h1), self.P is not None)
        finally:
            st.done()

    def round_1(self, seeds=None):
        """RelinKeyShare<R1>::new (relin_key_gen.rs:141-197): 2L draws of one seed per party."""
        return self._round(_lib.lib().fhe_mbfv_rlk_round1_dev, self.crp.poly, None, seeds, self.crp.poly)

    def round_2(self, r1, seeds=None):
        """RelinKeyShare<R2>::new (relin_key_gen.rs:243-296) from the aggregated round-1 share."""
        if r1.parties:
            raise FheError(-1, "round 2 takes the AGGREGATED round-1 share (RelinKeyShare.aggregate_round_1)")
        s = self._round(_lib.lib().fhe_mbfv_rlk_round2_dev, r1.h0, r1.h1, seeds, r1.h0)
        s.last_round = r1
        return s


class RelinKeyShare:
    """mbfv::RelinKeyShare (mbfv/relin_key_gen.rs:17-24): h0, h1 [L, L, N] ([P, L, L, N] for P parties)."""

    def __init__(self, params, h0, h1, parties=False):
        self.params, self.h0, self.h1, self.parties = params, h0, h1, parties
        self.last_round = None

    @staticmethod
    def aggregate_round_1(shares):
        """RelinKeyShare<R1Aggregated>::from_shares (relin_key_gen.rs:200-222)."""
        first = _first_share(shares)
        par = first.params
        ctx = par.context_at_level(0)
        Lm = ctx.nmoduli
        st = _Staging(par, first.h0)
        outs = []
        for attr in ("h0", "h1"):
            h = _stack_shares(st, shares, attr)
            o = st.out((Lm, Lm, par.degree))
            _mbfv_sum(ctx, h, int(h.shape[0]), Lm * Lm * par.degree, Lm, None, o)
            outs.append(st.give(o))
        return RelinKeyShare(par, outs[0], outs[1])

    @staticmethod
    def aggregate(shares):
        """RelinearizationKey::from_shares (relin_key_gen.rs:299-351) of round-2 shares: the collective
        `RelinearizationKey` at level 0 (fhe_mbfv_relin_key_aggregate_dev)."""
        first = _first_share(shares)
        if first.last_round is None:
            raise FheError(-1, "MissingRelinearizationRoundOneShare")
        par = first.params
        ctx = par.context_at_level(0)
        Lm = ctx.nmoduli
        st = _Staging(par, first.h0)
        h0, h1 = _stack_shares(st, shares, "h0"), _stack_shares(st, shares, "h1")
        r1 = st.dev(first.last_round.h1)
        h = C.c_void_p()
        check(_lib.lib().fhe_mbfv_relin_key_aggregate_dev(ctx._h, _dptr(h0), _dptr(h1), int(h0.shape[0]),
                                                          Lm * Lm * par.degree, _dptr(r1), _stream(), C.byref(h)))
        return RelinearizationKey(KeySwitchingKey._adopt(ctx, ctx, h.value, None, 0))
