// fhe_hip.cpp -- the extern "C" boundary declared in include/fhe_hip.h.
// Compiled as HIP for gfx950 (`hipcc -x hip --offload-arch=gfx950`, see __graft_entry__.build()).
// Every entry point: validate -> run engine code -> translate exceptions to status codes;
// nothing throws across the boundary.
#include "../../include/fhe_hip.h"

#include <array>
#include <cstdio>
#include <map>

#include <cxxabi.h>

#include "engine.hpp"
#include "ubench.hpp"

using namespace fhe;

struct fhe_ctx {
    std::unique_ptr<Ctx> owned;  // set on handles returned by fhe_ctx_create
    const Ctx *c = nullptr;
    std::vector<std::unique_ptr<fhe_ctx>> level_handles;  // borrowed-handle storage for fhe_ctx_at_level
    const fhe_ctx *root_handle = nullptr;                 // set on borrowed handles
    size_t level_in_root = 0;
};
struct fhe_scaler {
    std::unique_ptr<Scaler> s;
};
struct fhe_ksk {
    std::unique_ptr<Ksk> k;
};
struct fhe_kskset {
    std::unique_ptr<KskSet> s;
};
struct fhe_mul {
    std::unique_ptr<Mul> m;
    // scalers created by fhe_mul_create_default are owned here
    std::vector<std::unique_ptr<fhe_ctx>> ctxs;
    std::vector<std::unique_ptr<fhe_scaler>> scalers;
};
struct HostTables {  // one NttOperator's tables as the host's callback filled them
    std::vector<u64> om, oms, zi, zis;
    u64 si = 0, sis = 0;
};
struct fhe_params {
    int device = -1;
    bool host_tables = false;               // created with the host's NTT tables (callback)
    std::map<u64, HostTables> table_cache;  // modulus -> tables, filled while the callback was alive
    size_t degree = 0;
    u64 plaintext = 0;                      // t when it fits 64 bits, else 0
    BigUint plaintext_big;                  // t, of any size (PlaintextModulus::Large above 64 bits)
    std::vector<u64> moduli;
    std::vector<size_t> moduli_sizes;
    std::unique_ptr<fhe_ctx> top;                       // level-0 context (+ chain)
    std::vector<std::unique_ptr<fhe_ctx>> mul_ctx;      // per level
    std::vector<std::unique_ptr<fhe_scaler>> extender;  // per level
    std::vector<std::unique_ptr<fhe_scaler>> down;      // per level
};
struct fhe_encoder {
    std::unique_ptr<Encoder> e;
};

namespace {
thread_local std::string g_last_error;

template <class F>
fhe_status guard(F &&f) {
    try {
        f();
        return FHE_OK;
    } catch (const StatusError &e) {
        g_last_error = e.what();
        return e.code;
    } catch (const std::bad_alloc &) {
        g_last_error = "out of host memory";
        return FHE_E_ARG;
    } catch (const std::exception &e) {
        g_last_error = e.what();
        return FHE_E_ARG;
    }
}
void need(const void *p, const char *what) {
    if (!p) throw StatusError(FHE_E_ARG, std::string("null argument: ") + what);
}
std::unique_ptr<fhe_ctx> wrap_ctx(std::unique_ptr<Ctx> c) {
    auto h = std::make_unique<fhe_ctx>();
    h->c = c.get();
    h->owned = std::move(c);
    // one borrowed handle per level of the chain
    for (const Ctx *l = h->c->next.get(); l; l = l->next.get()) {
        auto b = std::make_unique<fhe_ctx>();
        b->c = l;
        b->root_handle = h.get();
        b->level_in_root = h->level_handles.size() + 1;
        h->level_handles.push_back(std::move(b));
    }
    return h;
}
const fhe_ctx *ctx_level_handle(const fhe_ctx *h, size_t level) {
    if (level == 0) return h;
    if (h->root_handle) return ctx_level_handle(h->root_handle, h->level_in_root + level);
    if (level - 1 < h->level_handles.size()) return h->level_handles[level - 1].get();
    return nullptr;
}
void set_device(const Ctx &c) {
    if (c.device >= 0) FHE_HIP_CHECK(hipSetDevice(c.device));
}

// Paired entry points.  Every operation exported as a host-pointer form fhe_X and a device-pointer form fhe_X_dev is
// one struct derived from Paired:
//  - its constructor makes every argument check, in one order: handles, then device / level / context, then buffers.
//    Checks the engine repeats stay here when staging depends on them: the device check (a host-only handle is refused
//    before the host form takes workspace for it), checks whose values size a staged array or decide whether the
//    buffers are needed (NoMoreContext, InvalidLevel, ContextNotReachable, EmptyDotProduct, MulPolyCount), and the
//    buffer checks themselves.  The rest (key levels, moduli agreement, expansion size) is left to the engine;
//  - `io` lists the arrays it reads and writes with their sizes;
//  - run(d, batch, stream) is the device body on the arrays of `io`, in that order.
// run_dev() calls the body on the caller's pointers and stream, run_host() stages `io` through the workspace.
struct Io {
    enum { IN = 1, OUT = 2, INOUT = IN | OUT, ZEROED = 4, SECRET = 8 };
    const void *p;   // the caller's array; NULL (no array, or an empty batch) is passed through and never staged
    size_t items;    // the batch, or 1 for an array the batch shares
    size_t bytes;    // per item
    int kind;        // ZEROED: an output cleared before the body; SECRET: cleared before its staging block is released
    // arrays of u64 words
    static Io in(const void *p, size_t items, size_t words, int flags = 0) { return {p, items, words * sizeof(u64), IN | flags}; }
    static Io out(void *p, size_t items, size_t words, int flags = 0) { return {p, items, words * sizeof(u64), OUT | flags}; }
    static Io inout(void *p, size_t items, size_t words) { return {p, items, words * sizeof(u64), INOUT}; }
};
// (an input with the same host array and size as an earlier one is staged once: fhe_bfv_mul's lhs == rhs squaring)
static bool shares(const Io &a, const Io &b) {
    return a.kind == Io::IN && b.kind == Io::IN && a.p == b.p && a.items == b.items && a.bytes == b.bytes;
}
struct Paired {
    static constexpr bool sliced = false;   // true: a large host-form batch goes through host_sliced
    const Ctx *dev = nullptr;               // the context whose device runs the body
    size_t batch = 0;
    void on(const Ctx &c, size_t b) {       // the device check
        c.need_device();
        dev = &c;
        batch = b;
    }
};
template <size_t K> using Ptrs = std::array<u64 *, K>;

// Staging blocks come from the engine's workspace pool (null stream), not from hipMalloc / hipFree per call: a host
// call is synchronous, so a block released here is idle by the time the next call takes it.
struct HostIO {
    std::vector<void *> bufs;
    std::vector<std::pair<void *, size_t>> secrets;  // staging copies cleared before they are released
    ~HostIO() {
        for (auto &s : secrets) (void)hipMemset(s.first, 0, s.second);
        if (!secrets.empty()) (void)hipStreamSynchronize(nullptr);
        for (void *p : bufs) Workspace::get().release(p);
    }
    u64 *take(size_t bytes) {   // at least one word
        void *d = Workspace::get().acquire(std::max<size_t>((bytes + 7) / 8, 1) * sizeof(u64), nullptr);
        bufs.push_back(d);
        return (u64 *)d;
    }
    u64 *stage(const Io &a) {
        const size_t bytes = a.items * a.bytes;
        u64 *d = take(bytes);
        if (a.kind & Io::SECRET) secrets.emplace_back(d, std::max<size_t>((bytes + 7) / 8, 1) * sizeof(u64));
        if ((a.kind & Io::IN) && bytes) FHE_HIP_CHECK(hipMemcpy(d, a.p, bytes, hipMemcpyHostToDevice));
        if (a.kind & Io::ZEROED)
            FHE_HIP_CHECK(hipMemsetAsync(d, 0, std::max<size_t>((bytes + 7) / 8, 1) * sizeof(u64), nullptr));
        return d;
    }
};

// Host-pointer calls on a large batch of independent items: the batch goes through in slices whose upload, kernels and
// download overlap (three internal streams: the link is full duplex and the GPU works on slice i while slice i + 1
// arrives and slice i - 1 leaves).  Values are those of the one-shot path.  Every array of `io` holds `batch` items;
// body(device arrays of the slice, items, stream).  Returns false -- nothing done -- when the batch is smaller than three
// slices of >= 32 MiB.
template <size_t K, class Body>
static bool host_sliced(int dev, size_t batch, const std::array<Io, K> &io, Body body) {
    size_t widest = 0;
    for (const Io &a : io) widest = std::max(widest, a.bytes / sizeof(u64));
    if (!widest) return false;
#if defined(FHE_HOST_EMULATION)
    const size_t slice = 2;   // (so that the emulated suite walks the sliced path: batches of 6 and more)
#else
    const size_t slice = std::max<size_t>(8, (((size_t)32 << 20) / (widest * sizeof(u64)) + 7) / 8 * 8);
#endif
    if (batch < 3 * slice) return false;
    static char tag_up, tag_comp, tag_down;   // keys of the three internal streams (no user stream has these addresses)
    AuxStreams &ax = AuxStreams::get();
    hipStream_t s_up = ax.stream_for(dev, (hipStream_t)&tag_up, true), s_comp = ax.stream_for(dev, (hipStream_t)&tag_comp, true),
                s_down = ax.stream_for(dev, (hipStream_t)&tag_down, true);
    // The staging blocks below come from the pool's NULL-stream blocks, which count as idle as soon as the call that
    // used them has returned -- but an asynchronous `_dev` call on the null stream may still be running in them, and
    // the three internal streams are non-blocking: they do not order against the null stream by themselves.
    FHE_HIP_CHECK(hipStreamSynchronize(nullptr));
    HostIO h;
    Ptrs<K> din{};
    std::array<bool, K> upload{};
    for (size_t k = 0; k < K; k++) {
        for (size_t j = 0; j < k; j++)
            if (shares(io[j], io[k])) din[k] = din[j];
        upload[k] = (io[k].kind & Io::IN) && !din[k];
        if (!din[k]) din[k] = h.take(batch * io[k].bytes);
    }
    const size_t nsl = (batch + slice - 1) / slice;
    std::vector<hipEvent_t> up(nsl, nullptr), done(nsl, nullptr);
    auto finish = [&] {   // nothing may still use the buffers when HostIO gives them back
        (void)hipStreamSynchronize(s_up);
        (void)hipStreamSynchronize(s_comp);
        (void)hipStreamSynchronize(s_down);
        for (auto *v : {&up, &done})
            for (hipEvent_t &e : *v)
                if (e) ax.give_event(e), e = nullptr;
    };
    try {
        for (size_t i = 0; i < nsl + 2; i++) {
            if (i < nsl) {
                const size_t o = i * slice, n = std::min(slice, batch - o);
                for (size_t k = 0; k < K; k++)
                    if (upload[k])
                        FHE_HIP_CHECK(hipMemcpyAsync((char *)din[k] + o * io[k].bytes, (const char *)io[k].p + o * io[k].bytes,
                                                     n * io[k].bytes, hipMemcpyHostToDevice, s_up));
                up[i] = ax.take_event();
                FHE_HIP_CHECK(hipEventRecord(up[i], s_up));
            }
            if (i >= 1 && i - 1 < nsl) {
                const size_t c = i - 1, o = c * slice, n = std::min(slice, batch - o);
                FHE_HIP_CHECK(hipStreamWaitEvent(s_comp, up[c], 0));
                Ptrs<K> ds;
                for (size_t k = 0; k < K; k++) ds[k] = din[k] + o * (io[k].bytes / sizeof(u64));
                body(ds, n, s_comp);
                done[c] = ax.take_event();
                FHE_HIP_CHECK(hipEventRecord(done[c], s_comp));
            }
            if (i >= 2) {
                const size_t c = i - 2, o = c * slice, n = std::min(slice, batch - o);
                FHE_HIP_CHECK(hipStreamWaitEvent(s_down, done[c], 0));
                for (size_t k = 0; k < K; k++)
                    if (io[k].kind & Io::OUT)
                        FHE_HIP_CHECK(hipMemcpyAsync((char *)io[k].p + o * io[k].bytes, (char *)din[k] + o * io[k].bytes,
                                                     n * io[k].bytes, hipMemcpyDeviceToHost, s_down));
            }
        }
    } catch (...) {
        finish();
        throw;
    }
    finish();
    return true;
}

template <class Op>
void run_dev(const Op &op, void *stream) {
    set_device(*op.dev);
    Ptrs<std::tuple_size<decltype(op.io)>::value> d;
    for (size_t k = 0; k < d.size(); k++) d[k] = (u64 *)op.io[k].p;
    op.run(d, op.batch, as_stream(stream));
}
// The host form: copy in, run the body on the null stream, copy out.
template <class Op>
void run_host(const Op &op) {
    set_device(*op.dev);
    constexpr size_t K = std::tuple_size<decltype(op.io)>::value;
    const std::array<Io, K> &io = op.io;
    if (Op::sliced && host_sliced(op.dev->device, op.batch, io,
                                  [&](const Ptrs<K> &d, size_t n, hipStream_t s) { op.run(d, n, s); }))
        return;
    HostIO h;
    Ptrs<K> d{};
    for (size_t k = 0; k < K; k++) {
        if (!io[k].p) continue;
        for (size_t j = 0; j < k; j++)
            if (shares(io[j], io[k])) d[k] = d[j];
        if (!d[k]) d[k] = h.stage(io[k]);
    }
    op.run(d, op.batch, nullptr);
    FHE_HIP_CHECK(hipStreamSynchronize(nullptr));
    for (size_t k = 0; k < K; k++) {
        const size_t bytes = io[k].items * io[k].bytes;
        if ((io[k].kind & Io::OUT) && io[k].p && bytes) FHE_HIP_CHECK(hipMemcpy((void *)io[k].p, d[k], bytes, hipMemcpyDeviceToHost));
    }
}
template <class Op, class... A>
fhe_status dev_call(void *stream, A... a) {
    return guard([&] { run_dev(Op(a...), stream); });
}
template <class Op, class... A>
fhe_status host_call(A... a) {
    return guard([&] { run_host(Op(a...)); });
}

// Context over `moduli` whose NTT tables come from the host's callback (NULL: the engine's own psi).  Every table
// is cached per modulus, so handles made later from the parameter set (a level-specific multiplication basis) never
// call back into the host: `fn` is only invoked while fhe_params_create_with_tables runs.
std::unique_ptr<Ctx> ctx_create_cb(int device, size_t degree, const std::vector<u64> &moduli, fhe_ntt_tables_fn fn,
                                   void *user, bool host_tables, std::map<u64, HostTables> &cache) {
    if (!host_tables) return ctx_create(device, degree, moduli, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    const size_t L = moduli.size();
    std::vector<u64> om(L * degree), oms(L * degree), zi(L * degree), zis(L * degree), si(L), sis(L);
    for (size_t i = 0; i < L; i++) {
        auto it = cache.find(moduli[i]);
        if (it == cache.end()) {
            if (!fn) throw StatusError(FHE_E_NTT_UNAVAILABLE, "NttOperatorUnavailable: no host table cached for this modulus");
            HostTables t;
            t.om.resize(degree), t.oms.resize(degree), t.zi.resize(degree), t.zis.resize(degree);
            if (fn(user, moduli[i], degree, t.om.data(), t.oms.data(), t.zi.data(), t.zis.data(), &t.si, &t.sis) != 0)
                throw StatusError(FHE_E_NTT_UNAVAILABLE, "NttOperatorUnavailable: the host's table callback failed");
            it = cache.emplace(moduli[i], std::move(t)).first;
        }
        const HostTables &t = it->second;
        std::copy(t.om.begin(), t.om.end(), om.begin() + i * degree);
        std::copy(t.oms.begin(), t.oms.end(), oms.begin() + i * degree);
        std::copy(t.zi.begin(), t.zi.end(), zi.begin() + i * degree);
        std::copy(t.zis.begin(), t.zis.end(), zis.begin() + i * degree);
        si[i] = t.si, sis[i] = t.sis;
    }
    return ctx_create(device, degree, moduli, om.data(), oms.data(), zi.data(), zis.data(), si.data(), sis.data());
}
}  // namespace

extern "C" {

const char *fhe_last_error(void) { return g_last_error.c_str(); }
const char *fhe_version(void) { return "fhe.rs_amd 0.1 (gfx950)"; }
int fhe_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ------------------------------------------------ device memory and streams ----
fhe_status fhe_buf_alloc(int device, size_t bytes, void **out) {
    return guard([&] {
        need(out, "out");
        *out = nullptr;
        int ndev = 0;
        FHE_HIP_CHECK(hipGetDeviceCount(&ndev));
        require(device >= 0 && device < ndev, E_NO_DEVICE, "no such HIP device");
        FHE_HIP_CHECK(hipSetDevice(device));
        FHE_HIP_CHECK(hipMalloc(out, std::max<size_t>(bytes, 1)));
    });
}
fhe_status fhe_buf_free(void *buf) {
    return guard([&] {
        if (buf) FHE_HIP_CHECK(hipFree(buf));
    });
}
// fhe_buf_alloc_async takes its memory from the device's PRIVATE stream-ordered pool (DevPools, engine.hpp), which is
// told to keep what is freed into it -- a host that allocates its results per call does not go back to the driver
// each time, and no other hipMallocAsync user of the process sees a changed default pool.
fhe_status fhe_buf_alloc_async(int device, size_t bytes, void *stream, void **out) {
    return guard([&] {
        need(out, "out");
        *out = nullptr;
        int ndev = 0;
        FHE_HIP_CHECK(hipGetDeviceCount(&ndev));
        require(device >= 0 && device < ndev, E_NO_DEVICE, "no such HIP device");
        FHE_HIP_CHECK(hipSetDevice(device));
        *out = DevPools::get().alloc(device, std::max<size_t>(bytes, 1), as_stream(stream), DevPools::BUFFERS);
    });
}
fhe_status fhe_buf_free_async(void *buf, void *stream) {
    return guard([&] {
        if (buf) FHE_HIP_CHECK(hipFreeAsync(buf, as_stream(stream)));
    });
}
static void copy_async(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, void *stream, bool wait) {
    if (bytes) {
        need(dst, "dst");
        need(src, "src");
        FHE_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, kind, as_stream(stream)));
    }
    if (wait) FHE_HIP_CHECK(hipStreamSynchronize(as_stream(stream)));
}
fhe_status fhe_buf_upload_async(void *dst_dev, const void *src_host, size_t bytes, void *stream) {
    return guard([&] { copy_async(dst_dev, src_host, bytes, hipMemcpyHostToDevice, stream, false); });
}
fhe_status fhe_buf_upload(void *dst_dev, const void *src_host, size_t bytes, void *stream) {
    return guard([&] { copy_async(dst_dev, src_host, bytes, hipMemcpyHostToDevice, stream, true); });
}
fhe_status fhe_buf_download_async(void *dst_host, const void *src_dev, size_t bytes, void *stream) {
    return guard([&] { copy_async(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, stream, false); });
}
fhe_status fhe_buf_download(void *dst_host, const void *src_dev, size_t bytes, void *stream) {
    return guard([&] { copy_async(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, stream, true); });
}
fhe_status fhe_buf_copy_async(void *dst_dev, const void *src_dev, size_t bytes, void *stream) {
    return guard([&] { copy_async(dst_dev, src_dev, bytes, hipMemcpyDeviceToDevice, stream, false); });
}
fhe_status fhe_buf_zero_async(void *buf, size_t bytes, void *stream) {
    return guard([&] {
        if (!bytes) return;
        need(buf, "buf");
        FHE_HIP_CHECK(hipMemsetAsync(buf, 0, bytes, as_stream(stream)));
    });
}
fhe_status fhe_host_alloc(size_t bytes, void **out) {
    return guard([&] {
        need(out, "out");
        *out = nullptr;
        FHE_HIP_CHECK(hipHostMalloc(out, std::max<size_t>(bytes, 1), 0));
    });
}
fhe_status fhe_host_free(void *p) {
    return guard([&] {
        if (p) FHE_HIP_CHECK(hipHostFree(p));
    });
}
fhe_status fhe_stream_create(int device, void **out) {
    return guard([&] {
        need(out, "out");
        *out = nullptr;
        int ndev = 0;
        FHE_HIP_CHECK(hipGetDeviceCount(&ndev));
        require(device >= 0 && device < ndev, E_NO_DEVICE, "no such HIP device");
        FHE_HIP_CHECK(hipSetDevice(device));
        hipStream_t s = nullptr;
        FHE_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        *out = (void *)s;
    });
}
fhe_status fhe_stream_sync(void *stream) {
    return guard([&] { FHE_HIP_CHECK(hipStreamSynchronize(as_stream(stream))); });
}
fhe_status fhe_stream_destroy(void *stream) {
    return guard([&] {
        if (!stream) return;   // the null stream is not ours to destroy
        FHE_HIP_CHECK(hipStreamSynchronize(as_stream(stream)));
        // what the engine keeps per caller stream: its internal second stream and its idle scratch blocks
        // (the internal stream's own blocks too -- a ChunkWs and the split-extension scratch are keyed to it: ADVICE r03)
        AuxStreams::get().drop(-1, as_stream(stream), false);
        Workspace::get().drop_stream(as_stream(stream));
        FHE_HIP_CHECK(hipStreamDestroy(as_stream(stream)));
    });
}
fhe_status fhe_device_sync(int device) {
    return guard([&] {
        int ndev = 0;
        FHE_HIP_CHECK(hipGetDeviceCount(&ndev));
        require(device >= 0 && device < ndev, E_NO_DEVICE, "no such HIP device");
        FHE_HIP_CHECK(hipSetDevice(device));
        FHE_HIP_CHECK(hipDeviceSynchronize());
    });
}
fhe_status fhe_device_mem_info(int device, size_t *free_bytes, size_t *total_bytes) {
    return guard([&] {
        int ndev = 0;
        FHE_HIP_CHECK(hipGetDeviceCount(&ndev));
        require(device >= 0 && device < ndev, E_NO_DEVICE, "no such HIP device");
        FHE_HIP_CHECK(hipSetDevice(device));
        size_t f = 0, t = 0;
        FHE_HIP_CHECK(hipMemGetInfo(&f, &t));
        if (free_bytes) *free_bytes = f;
        if (total_bytes) *total_bytes = t;
    });
}

// ----------------------------------------------------------------------------- ctx ----
fhe_status fhe_ctx_create(int device, size_t degree, size_t nmoduli, const uint64_t *moduli, const uint64_t *omegas,
                          const uint64_t *omegas_shoup, const uint64_t *zetas_inv, const uint64_t *zetas_inv_shoup,
                          const uint64_t *size_inv, const uint64_t *size_inv_shoup, fhe_ctx **out) {
    return guard([&] {
        need(out, "out");
        *out = nullptr;
        if (nmoduli == 0) throw StatusError(FHE_E_EMPTY_MODULI, "EmptyModuli");
        need(moduli, "moduli");
        std::vector<u64> m(moduli, moduli + nmoduli);
        *out = wrap_ctx(ctx_create(device, degree, m, omegas, omegas_shoup, zetas_inv, zetas_inv_shoup, size_inv,
                                   size_inv_shoup))
                   .release();
    });
}
void fhe_ctx_destroy(fhe_ctx *ctx) {
    if (ctx && ctx->owned) delete ctx;
}
fhe_status fhe_ctx_at_level(const fhe_ctx *ctx, size_t level, const fhe_ctx **out) {
    return guard([&] {
        need(ctx, "ctx");
        need(out, "out");
        // a borrowed level handle can itself be asked for deeper levels: resolve on the Ctx chain
        const Ctx *target = ctx->c->at_level(level);
        if (!target) throw StatusError(FHE_E_INVALID_LEVEL, "InvalidContextLevel");
        if (level == 0) {
            *out = ctx;
            return;
        }
        const fhe_ctx *h = ctx_level_handle(ctx, level);
        if (!h) throw StatusError(FHE_E_ARG, "fhe_ctx_at_level must be called on a handle from fhe_ctx_create");
        *out = h;
    });
}
fhe_status fhe_ctx_niterations_to(const fhe_ctx *from, const fhe_ctx *to, size_t *out) {
    return guard([&] {
        need(from, "from");
        need(to, "to");
        need(out, "out");
        long it = from->c->niterations_to(*to->c);
        if (it < 0) throw StatusError(FHE_E_CONTEXT_NOT_REACHABLE, "ContextNotReachable");
        *out = (size_t)it;
    });
}
size_t fhe_ctx_degree(const fhe_ctx *ctx) { return ctx ? ctx->c->n : 0; }
size_t fhe_ctx_nmoduli(const fhe_ctx *ctx) { return ctx ? ctx->c->L : 0; }
int fhe_ctx_device(const fhe_ctx *ctx) { return ctx ? ctx->c->device : -1; }
fhe_status fhe_ctx_moduli(const fhe_ctx *ctx, uint64_t *out) {
    return guard([&] {
        need(ctx, "ctx");
        need(out, "out");
        std::copy(ctx->c->moduli.begin(), ctx->c->moduli.end(), out);
    });
}
fhe_status fhe_ctx_get_table(const fhe_ctx *ctx, int which, uint64_t *out) {
    return guard([&] {
        need(ctx, "ctx");
        need(out, "out");
        const Ctx &c = *ctx->c;
        for (size_t i = 0; i < c.L; i++) {
            const NttTables &t = c.tab(i);
            switch (which) {
                case 0: std::copy(t.omegas.begin(), t.omegas.end(), out + i * c.n); break;
                case 1: std::copy(t.omegas_shoup.begin(), t.omegas_shoup.end(), out + i * c.n); break;
                case 2: std::copy(t.zetas_inv.begin(), t.zetas_inv.end(), out + i * c.n); break;
                case 3: std::copy(t.zetas_inv_shoup.begin(), t.zetas_inv_shoup.end(), out + i * c.n); break;
                case 4: out[i] = t.size_inv; break;
                case 5: out[i] = t.size_inv_shoup; break;
                case 6: if (i + 1 < c.L) out[i] = c.inv_last[i]; break;
                case 7: if (i + 1 < c.L) out[i] = c.inv_last_shoup[i]; break;
                default: throw StatusError(FHE_E_ARG, "unknown table selector");
            }
        }
    });
}

struct Ntt : Paired {   // NttOperator::{forward,backward}, in place
    bool inverse;
    std::array<Io, 1> io;
    Ntt(const fhe_ctx *ctx, uint64_t *polys, size_t batch, bool inverse) : inverse(inverse) {
        need(ctx, "ctx");
        on(*ctx->c, batch);
        if (batch) need(polys, "polys");
        io = {Io::inout(polys, batch, dev->L * dev->n)};
    }
    void run(const Ptrs<1> &d, size_t n, hipStream_t s) const { ntt_polys(*dev, inverse, d[0], d[0], n, s); }
};
fhe_status fhe_ntt_forward(const fhe_ctx *ctx, uint64_t *polys, size_t batch) { return host_call<Ntt>(ctx, polys, batch, false); }
fhe_status fhe_ntt_backward(const fhe_ctx *ctx, uint64_t *polys, size_t batch) { return host_call<Ntt>(ctx, polys, batch, true); }
fhe_status fhe_ntt_forward_dev(const fhe_ctx *ctx, uint64_t *polys, size_t batch, void *stream) {
    return dev_call<Ntt>(stream, ctx, polys, batch, false);
}
fhe_status fhe_ntt_backward_dev(const fhe_ctx *ctx, uint64_t *polys, size_t batch, void *stream) {
    return dev_call<Ntt>(stream, ctx, polys, batch, true);
}

struct Ew : Paired {   // a op= b (b absent for neg)
    uint32_t op;
    std::array<Io, 2> io;
    Ew(const fhe_ctx *ctx, uint64_t *a, const uint64_t *b, size_t batch, uint32_t op) : op(op) {
        need(ctx, "ctx");
        on(*ctx->c, batch);
        if (batch) {
            need(a, "a");
            if (op != k::EW_NEG) need(b, "b");
        }
        const size_t pe = dev->L * dev->n;
        io = {Io::inout(a, batch, pe), Io::in(b, batch, pe)};
    }
    void run(const Ptrs<2> &d, size_t n, hipStream_t s) const { ew_op(*dev, d[0], d[1], n, op, s); }
};
fhe_status fhe_poly_add(const fhe_ctx *c, uint64_t *a, const uint64_t *b, size_t n) { return host_call<Ew>(c, a, b, n, k::EW_ADD); }
fhe_status fhe_poly_sub(const fhe_ctx *c, uint64_t *a, const uint64_t *b, size_t n) { return host_call<Ew>(c, a, b, n, k::EW_SUB); }
fhe_status fhe_poly_mul(const fhe_ctx *c, uint64_t *a, const uint64_t *b, size_t n) { return host_call<Ew>(c, a, b, n, k::EW_MUL); }
fhe_status fhe_poly_neg(const fhe_ctx *c, uint64_t *a, size_t n) { return host_call<Ew>(c, a, nullptr, n, k::EW_NEG); }
fhe_status fhe_poly_add_dev(const fhe_ctx *c, uint64_t *a, const uint64_t *b, size_t n, void *s) { return dev_call<Ew>(s, c, a, b, n, k::EW_ADD); }
fhe_status fhe_poly_sub_dev(const fhe_ctx *c, uint64_t *a, const uint64_t *b, size_t n, void *s) { return dev_call<Ew>(s, c, a, b, n, k::EW_SUB); }
fhe_status fhe_poly_mul_dev(const fhe_ctx *c, uint64_t *a, const uint64_t *b, size_t n, void *s) { return dev_call<Ew>(s, c, a, b, n, k::EW_MUL); }
fhe_status fhe_poly_neg_dev(const fhe_ctx *c, uint64_t *a, size_t n, void *s) { return dev_call<Ew>(s, c, a, nullptr, n, k::EW_NEG); }

struct MulShoup : Paired {   // MulAssign<&Poly<NttShoup>>
    std::array<Io, 3> io;
    MulShoup(const fhe_ctx *ctx, uint64_t *a, const uint64_t *b, const uint64_t *b_shoup, size_t batch) {
        need(ctx, "ctx");
        on(*ctx->c, batch);
        if (batch) {
            need(a, "a");
            need(b, "b");
            need(b_shoup, "b_shoup");
        }
        const size_t pe = dev->L * dev->n;
        io = {Io::inout(a, batch, pe), Io::in(b, batch, pe), Io::in(b_shoup, batch, pe)};
    }
    void run(const Ptrs<3> &d, size_t n, hipStream_t s) const {
        const Ctx &c = *dev;
        const u64 total = (u64)n * c.L * c.n;
        if (!total) return;
        launch_ew<k::mul_shoup_kernel>("mul_shoup", total, s, d[0], d[1], d[2], c.dmods(), (uint32_t)c.L, (uint32_t)c.logn, total);
    }
};
fhe_status fhe_poly_mul_shoup(const fhe_ctx *ctx, uint64_t *a, const uint64_t *b, const uint64_t *b_shoup,
                              size_t batch) {
    return host_call<MulShoup>(ctx, a, b, b_shoup, batch);
}
fhe_status fhe_poly_mul_shoup_dev(const fhe_ctx *ctx, uint64_t *a, const uint64_t *b, const uint64_t *b_shoup,
                                  size_t batch, void *stream) {
    return dev_call<MulShoup>(stream, ctx, a, b, b_shoup, batch);
}
fhe_status fhe_poly_shoup(const fhe_ctx *ctx, const uint64_t *a, uint64_t *a_shoup, size_t batch) {
    return guard([&] {
        need(ctx, "ctx");
        const Ctx &c = *ctx->c;
        if (batch) {
            need(a, "a");
            need(a_shoup, "a_shoup");
        }
        // setup-time host computation (128/64-bit division), M/zq/mod.rs:195-199
        for (size_t b = 0; b < batch; b++)
            for (size_t r = 0; r < c.L; r++)
                for (size_t j = 0; j < c.n; j++) {
                    const size_t i = (b * c.L + r) * c.n + j;
                    a_shoup[i] = shoup(a[i], c.moduli[r]);
                }
    });
}

struct Substitute : Paired {   // Poly::substitute; `out` is written only (the host form stages it separately)
    size_t exponent;
    bool ntt;
    std::array<Io, 2> io;
    Substitute(const fhe_ctx *ctx, size_t exponent, const uint64_t *in, uint64_t *out, size_t batch, int repr_is_ntt)
        : exponent(exponent), ntt(repr_is_ntt != 0) {
        need(ctx, "ctx");
        on(*ctx->c, batch);
        if (batch) {
            need(in, "in");
            need(out, "out");
        }
        const size_t pe = dev->L * dev->n;
        io = {Io::in(in, batch, pe), Io::out(out, batch, pe)};
    }
    void run(const Ptrs<2> &d, size_t n, hipStream_t s) const { substitute_polys(*dev, exponent, d[0], d[1], n, ntt, s); }
};
fhe_status fhe_poly_substitute(const fhe_ctx *ctx, size_t exponent, const uint64_t *in, uint64_t *out, size_t batch,
                               int repr_is_ntt) {
    return host_call<Substitute>(ctx, exponent, in, out, batch, repr_is_ntt);
}
fhe_status fhe_poly_substitute_dev(const fhe_ctx *ctx, size_t exponent, const uint64_t *in, uint64_t *out,
                                   size_t batch, int repr_is_ntt, void *stream) {
    return guard([&] {
        Substitute op(ctx, exponent, in, out, batch, repr_is_ntt);
        // (device form only: the kernel does not work in place, and here `in` and `out` are the kernel's own arrays;
        // the host form stages them into separate blocks and so accepts in == out)
        if (in == out) throw StatusError(FHE_E_ARG, "substitute is not in-place");
        run_dev(op, stream);
    });
}

size_t fhe_poly_serialized_size(const fhe_ctx *ctx) { return ctx ? wire_poly_bytes(*ctx->c) : 0; }
// Rq wire format: the byte arrays are staged in bytes
struct Serialize : Paired {
    bool from_ntt;
    std::array<Io, 2> io;
    Serialize(const fhe_ctx *ctx, const uint64_t *polys, uint8_t *bytes, size_t batch, int from_ntt)
        : from_ntt(from_ntt != 0) {
        need(ctx, "ctx");
        on(*ctx->c, batch);
        if (batch) {
            need(polys, "polys");
            need(bytes, "bytes");
        }
        io = {Io::in(polys, batch, dev->L * dev->n), Io{bytes, batch, wire_poly_bytes(*dev), Io::OUT}};
    }
    void run(const Ptrs<2> &d, size_t n, hipStream_t s) const {
        wire_serialize(*dev, d[0], reinterpret_cast<uint8_t *>(d[1]), n, from_ntt, s);
    }
};
fhe_status fhe_poly_serialize(const fhe_ctx *ctx, const uint64_t *polys, uint8_t *bytes, size_t batch, int from_ntt) {
    return host_call<Serialize>(ctx, polys, bytes, batch, from_ntt);
}
fhe_status fhe_poly_serialize_dev(const fhe_ctx *ctx, const uint64_t *polys, uint8_t *bytes, size_t batch, int from_ntt,
                                  void *stream) {
    return dev_call<Serialize>(stream, ctx, polys, bytes, batch, from_ntt);
}
struct Deserialize : Paired {
    bool to_ntt;
    std::array<Io, 2> io;
    Deserialize(const fhe_ctx *ctx, const uint8_t *bytes, uint64_t *polys, size_t batch, int to_ntt) : to_ntt(to_ntt != 0) {
        need(ctx, "ctx");
        on(*ctx->c, batch);
        if (batch) {
            need(polys, "polys");
            need(bytes, "bytes");
        }
        io = {Io{bytes, batch, wire_poly_bytes(*dev), Io::IN}, Io::out(polys, batch, dev->L * dev->n)};
    }
    void run(const Ptrs<2> &d, size_t n, hipStream_t s) const {
        wire_deserialize(*dev, reinterpret_cast<const uint8_t *>(d[0]), d[1], n, to_ntt, s);
    }
};
fhe_status fhe_poly_deserialize(const fhe_ctx *ctx, const uint8_t *bytes, uint64_t *polys, size_t batch, int to_ntt) {
    return host_call<Deserialize>(ctx, bytes, polys, batch, to_ntt);
}
fhe_status fhe_poly_deserialize_dev(const fhe_ctx *ctx, const uint8_t *bytes, uint64_t *polys, size_t batch, int to_ntt,
                                    void *stream) {
    return dev_call<Deserialize>(stream, ctx, bytes, polys, batch, to_ntt);
}

struct SwitchDown : Paired {   // Poly::<PowerBasis>::switch_down
    std::array<Io, 2> io;
    SwitchDown(const fhe_ctx *ctx, const uint64_t *in, uint64_t *out, size_t batch) {
        need(ctx, "ctx");
        on(*ctx->c, batch);
        if (!dev->next) throw StatusError(FHE_E_NO_MORE_CONTEXT, "NoMoreContext");
        if (batch) {
            need(in, "in");
            need(out, "out");
        }
        const size_t pe = dev->L * dev->n;
        io = {Io::in(in, batch, pe), Io::out(out, batch, pe - dev->n)};
    }
    void run(const Ptrs<2> &d, size_t n, hipStream_t s) const {
        const size_t pe = dev->L * dev->n;
        switch_down_polys(*dev, d[0], pe, d[1], pe - dev->n, n, s);
    }
};
fhe_status fhe_poly_switch_down(const fhe_ctx *ctx, const uint64_t *in, uint64_t *out, size_t batch) {
    return host_call<SwitchDown>(ctx, in, out, batch);
}
fhe_status fhe_poly_switch_down_dev(const fhe_ctx *ctx, const uint64_t *in, uint64_t *out, size_t batch, void *stream) {
    return dev_call<SwitchDown>(stream, ctx, in, out, batch);
}

struct SwitchDownTo : Paired {   // Poly::<PowerBasis>::switch_down_to
    size_t iters = 0;
    std::array<Io, 2> io;
    SwitchDownTo(const fhe_ctx *from, const fhe_ctx *to, const uint64_t *in, uint64_t *out, size_t batch) {
        need(from, "from");
        need(to, "to");
        on(*from->c, batch);
        const long it = from->c->niterations_to(*to->c);
        if (it < 0) throw StatusError(FHE_E_CONTEXT_NOT_REACHABLE, "ContextNotReachable");
        iters = (size_t)it;
        if (batch) {
            need(in, "in");
            need(out, "out");
        }
        const size_t pe = dev->L * dev->n;
        io = {Io::in(in, batch, pe), Io::out(out, batch, pe - iters * dev->n)};
    }
    void run(const Ptrs<2> &d, size_t n, hipStream_t s) const {
        const size_t pe = dev->L * dev->n;
        switch_down_to_pb(*dev, iters, d[0], pe, d[1], pe - iters * dev->n, n, s);
    }
};
fhe_status fhe_poly_switch_down_to(const fhe_ctx *from, const fhe_ctx *to, const uint64_t *in, uint64_t *out,
                                   size_t batch) {
    return host_call<SwitchDownTo>(from, to, in, out, batch);
}
fhe_status fhe_poly_switch_down_to_dev(const fhe_ctx *from, const fhe_ctx *to, const uint64_t *in, uint64_t *out,
                                       size_t batch, void *stream) {
    return dev_call<SwitchDownTo>(stream, from, to, in, out, batch);
}

// -------------------------------------------------------------------------- scaler ----
fhe_status fhe_scaler_create(const fhe_ctx *from, const fhe_ctx *to, const uint64_t *numerator, size_t numerator_limbs,
                             const uint64_t *denominator, size_t denominator_limbs, fhe_scaler **out) {
    return guard([&] {
        need(from, "from");
        need(to, "to");
        need(out, "out");
        need(numerator, "numerator");
        need(denominator, "denominator");
        *out = nullptr;
        set_device(*from->c);
        BigUint num = BigUint::from_limbs(numerator, numerator_limbs);
        BigUint den = BigUint::from_limbs(denominator, denominator_limbs);
        auto h = std::make_unique<fhe_scaler>();
        h->s = scaler_create(*from->c, *to->c, num, den);
        *out = h.release();
    });
}
fhe_status fhe_scaler_create_from_constants(const fhe_ctx *from, const fhe_ctx *to, size_t number_common_moduli,
                                            int is_one, const uint64_t *gamma, const uint64_t *gamma_shoup,
                                            const uint64_t *omega, const uint64_t *omega_shoup, uint64_t theta_gamma_lo,
                                            uint64_t theta_gamma_hi, int theta_gamma_sign,
                                            const uint64_t *theta_omega_lo, const uint64_t *theta_omega_hi,
                                            const uint8_t *theta_omega_sign, const uint64_t *theta_garner_lo,
                                            const uint64_t *theta_garner_hi, size_t theta_garner_shift,
                                            fhe_scaler **out) {
    return guard([&] {
        need(from, "from");
        need(to, "to");
        need(out, "out");
        *out = nullptr;
        need(gamma, "gamma");
        need(gamma_shoup, "gamma_shoup");
        need(omega, "omega");
        need(omega_shoup, "omega_shoup");
        need(theta_omega_lo, "theta_omega_lo");
        need(theta_omega_hi, "theta_omega_hi");
        need(theta_omega_sign, "theta_omega_sign");
        need(theta_garner_lo, "theta_garner_lo");
        need(theta_garner_hi, "theta_garner_hi");
        const Ctx &f = *from->c, &t = *to->c;
        require(f.n == t.n, E_DEGREE_MISMATCH, "DegreeMismatch");
        require(f.device == t.device, E_PARAMETER_MISMATCH, "contexts live on different devices");
        require(theta_garner_shift >= 2 && theta_garner_shift <= 127, E_ARG, "theta_garner_shift out of range");
        require(number_common_moduli <= std::min(f.L, t.L), E_ARG, "number_common_moduli too large");
        set_device(f);
        auto h = std::make_unique<fhe_scaler>();
        h->s = std::make_unique<Scaler>();
        Scaler &s = *h->s;
        s.from = &f;
        s.to = &t;
        s.ncommon = number_common_moduli;
        ScalerConstants &c = s.c;
        c.nfrom = f.L;
        c.nto = t.L;
        c.is_one = is_one != 0;
        c.gamma.assign(gamma, gamma + t.L);
        c.gamma_shoup.assign(gamma_shoup, gamma_shoup + t.L);
        c.omega.assign(omega, omega + t.L * f.L);
        c.omega_shoup.assign(omega_shoup, omega_shoup + t.L * f.L);
        c.theta_gamma_lo = theta_gamma_lo;
        c.theta_gamma_hi = theta_gamma_hi;
        c.theta_gamma_sign = theta_gamma_sign != 0;
        c.theta_omega_lo.assign(theta_omega_lo, theta_omega_lo + f.L);
        c.theta_omega_hi.assign(theta_omega_hi, theta_omega_hi + f.L);
        c.theta_omega_sign.assign(theta_omega_sign, theta_omega_sign + f.L);
        c.theta_garner_lo.assign(theta_garner_lo, theta_garner_lo + f.L);
        c.theta_garner_hi.assign(theta_garner_hi, theta_garner_hi + f.L);
        c.theta_garner_shift = theta_garner_shift;
        scaler_upload(s);
        *out = h.release();
    });
}
fhe_status fhe_switcher_create(const fhe_ctx *from, const fhe_ctx *to, fhe_scaler **out) {
    return guard([&] {
        need(from, "from");
        need(to, "to");
        need(out, "out");
        *out = nullptr;
        set_device(*from->c);
        RnsContext rf(from->c->moduli), rt(to->c->moduli);
        auto h = std::make_unique<fhe_scaler>();
        h->s = scaler_create(*from->c, *to->c, rt.product, rf.product);
        *out = h.release();
    });
}
void fhe_scaler_destroy(fhe_scaler *s) { delete s; }
size_t fhe_scaler_number_common_moduli(const fhe_scaler *s) { return s ? s->s->ncommon : 0; }
fhe_status fhe_scaler_get_constants(const fhe_scaler *s, int which, uint64_t *out) {
    return guard([&] {
        need(s, "scaler");
        need(out, "out");
        const ScalerConstants &c = s->s->c;
        auto cp = [&](const std::vector<u64> &v) { std::copy(v.begin(), v.end(), out); };
        switch (which) {
            case 0: cp(c.gamma); break;
            case 1: cp(c.gamma_shoup); break;
            case 2: cp(c.omega); break;
            case 3: cp(c.omega_shoup); break;
            case 4: cp(c.theta_omega_lo); break;
            case 5: cp(c.theta_omega_hi); break;
            case 6: for (size_t i = 0; i < c.nfrom; i++) out[i] = c.theta_omega_sign[i]; break;
            case 7: cp(c.theta_garner_lo); break;
            case 8: cp(c.theta_garner_hi); break;
            case 9:
                out[0] = c.theta_gamma_lo;
                out[1] = c.theta_gamma_hi;
                out[2] = c.theta_gamma_sign ? 1 : 0;
                out[3] = c.theta_garner_shift;
                out[4] = c.is_one ? 1 : 0;
                break;
            default: throw StatusError(FHE_E_ARG, "unknown constant selector");
        }
    });
}
struct Scale : Paired {   // Scaler::scale
    const Scaler *sc;
    bool ntt;
    std::array<Io, 2> io;
    Scale(const fhe_scaler *s, const uint64_t *in, uint64_t *out, size_t batch, int repr_is_ntt) : ntt(repr_is_ntt != 0) {
        need(s, "scaler");
        sc = s->s.get();
        on(*sc->from, batch);
        if (batch) {
            need(in, "in");
            need(out, "out");
        }
        io = {Io::in(in, batch, sc->from->L * sc->from->n), Io::out(out, batch, sc->to->L * sc->to->n, Io::ZEROED)};
    }
    void run(const Ptrs<2> &d, size_t n, hipStream_t s) const { scale_polys(*sc, d[0], d[1], n, ntt, s); }
};
fhe_status fhe_poly_scale(const fhe_scaler *s, const uint64_t *in, uint64_t *out, size_t batch, int repr_is_ntt) {
    return host_call<Scale>(s, in, out, batch, repr_is_ntt);
}
fhe_status fhe_poly_scale_dev(const fhe_scaler *s, const uint64_t *in, uint64_t *out, size_t batch, int repr_is_ntt,
                              void *stream) {
    return dev_call<Scale>(stream, s, in, out, batch, repr_is_ntt);
}

// ----------------------------------------------------------------------------- ksk ----
// fhe_ksk_create(_dev)'s checks: handles, the key's geometry and device (make_ksk), then the key arrays.
static std::unique_ptr<fhe_ksk> ksk_new(const fhe_ctx *ct_ctx, const fhe_ctx *ksk_ctx, size_t ndigits, const void *c0,
                                        const void *c1, size_t log_base, fhe_ksk **out) {
    need(ct_ctx, "ct_ctx");
    need(ksk_ctx, "ksk_ctx");
    need(out, "out");
    *out = nullptr;
    set_device(*ksk_ctx->c);
    auto h = std::make_unique<fhe_ksk>();
    h->k = make_ksk(*ct_ctx->c, *ksk_ctx->c, ndigits, log_base);
    need(c0, "c0");
    need(c1, "c1");
    return h;
}
// The handle's arrays from its key words: c0 and c1 (host or device arrays, by `kind`) copied into it on `s`, then
// ksk_finish.  Every coefficient must be a canonical residue (the Shoup quotient of an unreduced value does not fit 64
// bits and the key would silently give wrong results); supplied twins (host arrays) must be the twins the device
// wrote.  Waits for `s`: the key is usable from any stream afterwards.
static void ksk_fill(Ksk &k_, const u64 *c0, const u64 *c0_shoup, const u64 *c1, const u64 *c1_shoup, hipMemcpyKind kind,
                     hipStream_t s) {
    const size_t bytes = k_.ndigits * k_.ksk_ctx->L * k_.ksk_ctx->n * sizeof(u64);
    ksk_alloc(k_);
    FHE_HIP_CHECK(hipMemcpyAsync(k_.c0.p, c0, bytes, kind, s));
    FHE_HIP_CHECK(hipMemcpyAsync(k_.c1.p, c1, bytes, kind, s));
    ksk_finish(k_, s);
    FHE_HIP_CHECK(hipStreamSynchronize(s));
    for (auto given : {std::make_pair(c0_shoup, k_.c0s.p), std::make_pair(c1_shoup, k_.c1s.p)}) {
        if (!given.first) continue;
        std::vector<u64> v(bytes / sizeof(u64));
        FHE_HIP_CHECK(hipMemcpy(v.data(), given.second, bytes, hipMemcpyDeviceToHost));
        require(std::memcmp(v.data(), given.first, bytes) == 0, E_ARG, "Shoup twin is not floor(c * 2^64 / q)");
    }
}
fhe_status fhe_ksk_create(const fhe_ctx *ct_ctx, const fhe_ctx *ksk_ctx, size_t ndigits, const uint64_t *c0,
                          const uint64_t *c0_shoup, const uint64_t *c1, const uint64_t *c1_shoup, size_t log_base,
                          fhe_ksk **out) {
    return guard([&] {
        auto h = ksk_new(ct_ctx, ksk_ctx, ndigits, c0, c1, log_base, out);
        ksk_fill(*h->k, c0, c0_shoup, c1, c1_shoup, hipMemcpyHostToDevice, nullptr);
        *out = h.release();
    });
}
fhe_status fhe_ksk_create_dev(const fhe_ctx *ct_ctx, const fhe_ctx *ksk_ctx, size_t ndigits, const uint64_t *c0,
                              const uint64_t *c1, size_t log_base, void *stream, fhe_ksk **out) {
    return guard([&] {
        auto h = ksk_new(ct_ctx, ksk_ctx, ndigits, c0, c1, log_base, out);
        ksk_fill(*h->k, c0, nullptr, c1, nullptr, hipMemcpyDeviceToDevice, as_stream(stream));
        *out = h.release();
    });
}
void fhe_ksk_destroy(fhe_ksk *k_) { delete k_; }
fhe_status fhe_ksk_set_mode(fhe_ksk *k_, int mode, size_t w_budget) {
    return guard([&] {
        need(k_, "ksk");
        require(mode >= KS_AUTO && mode <= KS_FUSED_SUB, E_ARG, "mode must be 0 (auto), 1 (fused), 2 (unfused), 3 (unfused on sub-block tiles) or 4 (fused on sub-block tiles)");
        k_->k->mode.store(mode, std::memory_order_relaxed);
        k_->k->w_budget.store(w_budget, std::memory_order_relaxed);
    });
}
fhe_status fhe_ksk_get_mode(const fhe_ksk *k_, int *mode, size_t *w_budget) {
    return guard([&] {
        need(k_, "ksk");
        if (mode) *mode = k_->k->mode.load(std::memory_order_relaxed);
        if (w_budget) *w_budget = k_->k->w_budget.load(std::memory_order_relaxed);
    });
}

struct KeySwitch : Paired {   // KeySwitchingKey::key_switch: two outputs
    const Ksk *ks;
    std::array<Io, 3> io;
    KeySwitch(const fhe_ksk *k_, const uint64_t *p, uint64_t *c0_out, uint64_t *c1_out, size_t batch) {
        need(k_, "ksk");
        ks = k_->k.get();
        on(*ks->ksk_ctx, batch);
        if (batch) {
            need(p, "p");
            need(c0_out, "c0_out");
            need(c1_out, "c1_out");
        }
        const size_t ie = ks->ct_ctx->L * ks->ct_ctx->n, oe = ks->ksk_ctx->L * ks->ksk_ctx->n;
        io = {Io::in(p, batch, ie), Io::out(c0_out, batch, oe), Io::out(c1_out, batch, oe)};
    }
    void run(const Ptrs<3> &d, size_t n, hipStream_t s) const {
        key_switch_polys(*ks, d[0], (u64)ks->ct_ctx->L * ks->ct_ctx->n, d[1], d[2], (u64)ks->ksk_ctx->L * ks->ksk_ctx->n,
                         nullptr, nullptr, 0, n, s);
    }
};
fhe_status fhe_key_switch(const fhe_ksk *k_, const uint64_t *p, uint64_t *c0_out, uint64_t *c1_out, size_t batch) {
    return host_call<KeySwitch>(k_, p, c0_out, c1_out, batch);
}
fhe_status fhe_key_switch_dev(const fhe_ksk *k_, const uint64_t *p, uint64_t *c0_out, uint64_t *c1_out, size_t batch,
                              void *stream) {
    return dev_call<KeySwitch>(stream, k_, p, c0_out, c1_out, batch);
}

// RelinearizationKey::relinearizes on device arrays; keyed (optional): ciphertext b under key (b / per_key) % nkeys of the
// set, `ks` then being the set's first key
static void relinearize_polys(const Ksk &ks, const u64 *ct3, u64 *out, size_t n, hipStream_t s, const KsKeyed *keyed = nullptr) {
    const Ctx &cc = *ks.ct_ctx;
    const u64 PL = (u64)cc.L * cc.n;
    if (!n) return;
    WsGuard c2(n * PL * sizeof(u64), s);
    launch_ntt(cc, true, ct3 + 2 * PL, c2.u(), strided_map(cc, cc.L, 3 * PL, PL), n, s);
    // (c2 in Ntt form doubles as the transforms of digit j under key modulus j)
    key_switch_add(ks, c2.u(), PL, ct3, ct3 + PL, 3 * PL, out, out + PL, 2 * PL, n, s, ct3 + 2 * PL, 3 * PL, 0, nullptr, keyed);
}
struct Relinearize : Paired {   // RelinearizationKey::relinearizes: ct3 [b][3][L][N] -> out [b][2][L][N]
    static constexpr bool sliced = true;
    const Ksk *ks;
    std::array<Io, 2> io;
    Relinearize(const fhe_ksk *rk, const uint64_t *ct3, uint64_t *out, size_t batch) {
        need(rk, "rk");
        ks = rk->k.get();
        on(*ks->ksk_ctx, batch);
        if (batch) {
            need(ct3, "ct3");
            need(out, "out");
        }
        const size_t pe = ks->ct_ctx->L * ks->ct_ctx->n;
        io = {Io::in(ct3, batch, 3 * pe), Io::out(out, batch, 2 * pe)};
    }
    void run(const Ptrs<2> &d, size_t n, hipStream_t s) const { relinearize_polys(*ks, d[0], d[1], n, s); }
};
fhe_status fhe_bfv_relinearize(const fhe_ksk *rk, const uint64_t *ct3, uint64_t *out, size_t batch) {
    return host_call<Relinearize>(rk, ct3, out, batch);
}
fhe_status fhe_bfv_relinearize_dev(const fhe_ksk *rk, const uint64_t *ct3, uint64_t *out, size_t batch, void *stream) {
    return dev_call<Relinearize>(stream, rk, ct3, out, batch);
}

struct Galois : Paired {   // GaloisKey::relinearize
    static constexpr bool sliced = true;
    const Ksk *ks;
    size_t exponent;
    std::array<Io, 2> io;
    Galois(const fhe_ksk *gk, size_t exponent, const uint64_t *ct, uint64_t *out, size_t batch) : exponent(exponent) {
        need(gk, "gk");
        ks = gk->k.get();
        on(*ks->ksk_ctx, batch);
        if (batch) {
            need(ct, "ct");
            need(out, "out");
        }
        const size_t pe = ks->ct_ctx->L * ks->ct_ctx->n;
        io = {Io::in(ct, batch, 2 * pe), Io::out(out, batch, 2 * pe)};
    }
    void run(const Ptrs<2> &d, size_t n, hipStream_t s) const { galois_apply(*ks, exponent, d[0], d[1], n, s); }
};
fhe_status fhe_bfv_galois(const fhe_ksk *gk, size_t exponent, const uint64_t *ct, uint64_t *out, size_t batch) {
    return host_call<Galois>(gk, exponent, ct, out, batch);
}
fhe_status fhe_bfv_galois_dev(const fhe_ksk *gk, size_t exponent, const uint64_t *ct, uint64_t *out, size_t batch,
                              void *stream) {
    return dev_call<Galois>(stream, gk, exponent, ct, out, batch);
}

struct BfvSwitchDown : Paired {   // Ciphertext::switch_down
    size_t nparts;
    std::array<Io, 2> io;
    BfvSwitchDown(const fhe_ctx *ctx, size_t nparts, const uint64_t *ct, uint64_t *out, size_t batch) : nparts(nparts) {
        need(ctx, "ctx");
        on(*ctx->c, batch);
        if (!dev->next) throw StatusError(FHE_E_NO_MORE_CONTEXT, "NoMoreContext");
        if (batch && nparts) {
            need(ct, "ct");
            need(out, "out");
        }
        const size_t pe = dev->L * dev->n;
        io = {Io::in(ct, batch, nparts * pe), Io::out(out, batch, nparts * (pe - dev->n))};
    }
    void run(const Ptrs<2> &d, size_t n, hipStream_t s) const { bfv_switch_down(*dev, nparts, d[0], d[1], n, s); }
};
fhe_status fhe_bfv_switch_down(const fhe_ctx *ctx, size_t nparts, const uint64_t *ct, uint64_t *out, size_t batch) {
    return host_call<BfvSwitchDown>(ctx, nparts, ct, out, batch);
}
fhe_status fhe_bfv_switch_down_dev(const fhe_ctx *ctx, size_t nparts, const uint64_t *ct, uint64_t *out, size_t batch,
                                   void *stream) {
    return dev_call<BfvSwitchDown>(stream, ctx, nparts, ct, out, batch);
}

struct SwitchToLevel : Paired {   // Ciphertext::switch_to_level (F/bfv/ciphertext.rs:164-183), `levels` = target_level - level
    size_t levels, nparts;
    std::array<Io, 2> io;
    SwitchToLevel(const fhe_ctx *ctx, size_t levels, size_t nparts, const uint64_t *ct, uint64_t *out, size_t batch)
        : levels(levels), nparts(nparts) {
        need(ctx, "ctx");
        on(*ctx->c, batch);
        if (!dev->at_level(levels))
            throw StatusError(FHE_E_INVALID_LEVEL, "InvalidLevel: the context chain has " + std::to_string(dev->L - 1) +
                                                       " levels below this one, asked for " + std::to_string(levels));
        if (batch && nparts) {
            need(ct, "ct");
            need(out, "out");
        }
        const size_t pe = dev->L * dev->n;
        io = {Io::in(ct, batch, nparts * pe), Io::out(out, batch, nparts * (pe - levels * dev->n))};
    }
    void run(const Ptrs<2> &d, size_t n, hipStream_t s) const { switch_down_to_ntt(*dev, levels, d[0], d[1], n * nparts, s); }
};
fhe_status fhe_bfv_switch_to_level(const fhe_ctx *ctx, size_t levels, size_t nparts, const uint64_t *ct, uint64_t *out,
                                   size_t batch) {
    return host_call<SwitchToLevel>(ctx, levels, nparts, ct, out, batch);
}
fhe_status fhe_bfv_switch_to_level_dev(const fhe_ctx *ctx, size_t levels, size_t nparts, const uint64_t *ct,
                                       uint64_t *out, size_t batch, void *stream) {
    return dev_call<SwitchToLevel>(stream, ctx, levels, nparts, ct, out, batch);
}

// ------------------------------------------------------ PIR / RGSW / inner sum ----
struct DotProduct : Paired {   // bfv::dot_product_scalar; a shared operand is one item for the whole batch
    size_t nparts, count;
    bool cts_shared, pts_shared;
    std::array<Io, 3> io;
    DotProduct(const fhe_ctx *ctx, size_t nparts, size_t count, const uint64_t *cts, int cts_shared, const uint64_t *pts,
               int pts_shared, uint64_t *out, size_t batch)
        : nparts(nparts), count(count), cts_shared(cts_shared != 0), pts_shared(pts_shared != 0) {
        need(ctx, "ctx");
        on(*ctx->c, batch);
        if (count == 0) throw StatusError(FHE_E_EMPTY_DOT_PRODUCT, "EmptyDotProduct: no operands");
        if (batch && nparts) {
            need(cts, "cts");
            need(pts, "pts");
            need(out, "out");
        }
        const size_t pe = dev->L * dev->n;
        io = {Io::in(cts, this->cts_shared ? 1 : batch, count * nparts * pe),
              Io::in(pts, this->pts_shared ? 1 : batch, count * pe), Io::out(out, batch, nparts * pe)};
    }
    void run(const Ptrs<3> &d, size_t n, hipStream_t s) const {
        dot_product_scalar(*dev, nparts, count, d[0], cts_shared, d[1], pts_shared, d[2], n, s);
    }
};
fhe_status fhe_bfv_dot_product_scalar(const fhe_ctx *ctx, size_t nparts, size_t count, const uint64_t *cts,
                                      int cts_shared, const uint64_t *pts, int pts_shared, uint64_t *out,
                                      size_t batch) {
    return host_call<DotProduct>(ctx, nparts, count, cts, cts_shared, pts, pts_shared, out, batch);
}
fhe_status fhe_bfv_dot_product_scalar_dev(const fhe_ctx *ctx, size_t nparts, size_t count, const uint64_t *cts,
                                          int cts_shared, const uint64_t *pts, int pts_shared, uint64_t *out,
                                          size_t batch, void *stream) {
    return dev_call<DotProduct>(stream, ctx, nparts, count, cts, cts_shared, pts, pts_shared, out, batch);
}
struct MulPlain : Paired {   // `Ciphertext * Plaintext`
    size_t nparts;
    bool pt_shared;
    std::array<Io, 3> io;
    MulPlain(const fhe_ctx *ctx, size_t nparts, const uint64_t *ct, const uint64_t *pt, int pt_shared, uint64_t *out,
             size_t batch)
        : nparts(nparts), pt_shared(pt_shared != 0) {
        need(ctx, "ctx");
        on(*ctx->c, batch);
        if (batch && nparts) {
            need(ct, "ct");
            need(pt, "pt");
            need(out, "out");
        }
        const size_t pe = dev->L * dev->n;
        io = {Io::in(ct, batch, nparts * pe), Io::in(pt, this->pt_shared ? 1 : batch, pe), Io::out(out, batch, nparts * pe)};
    }
    void run(const Ptrs<3> &d, size_t n, hipStream_t s) const { mul_plain(*dev, nparts, d[0], d[1], pt_shared, d[2], n, s); }
};
fhe_status fhe_bfv_mul_plain(const fhe_ctx *ctx, size_t nparts, const uint64_t *ct, const uint64_t *pt, int pt_shared,
                             uint64_t *out, size_t batch) {
    return host_call<MulPlain>(ctx, nparts, ct, pt, pt_shared, out, batch);
}
fhe_status fhe_bfv_mul_plain_dev(const fhe_ctx *ctx, size_t nparts, const uint64_t *ct, const uint64_t *pt,
                                 int pt_shared, uint64_t *out, size_t batch, void *stream) {
    return dev_call<MulPlain>(stream, ctx, nparts, ct, pt, pt_shared, out, batch);
}
struct RgswMul : Paired {   // `&Ciphertext * &RGSWCiphertext`
    const Ksk *k0, *k1;
    std::array<Io, 2> io;
    RgswMul(const fhe_ksk *ksk0, const fhe_ksk *ksk1, const uint64_t *ct, uint64_t *out, size_t batch) {
        need(ksk0, "ksk0");
        need(ksk1, "ksk1");
        k0 = ksk0->k.get(), k1 = ksk1->k.get();
        on(*k0->ksk_ctx, batch);
        if (batch) {
            need(ct, "ct");
            need(out, "out");
        }
        const size_t pe = k0->ct_ctx->L * k0->ct_ctx->n;
        io = {Io::in(ct, batch, 2 * pe), Io::out(out, batch, 2 * pe)};
    }
    void run(const Ptrs<2> &d, size_t n, hipStream_t s) const { rgsw_mul(*k0, *k1, d[0], d[1], n, s); }
};
fhe_status fhe_bfv_rgsw_mul(const fhe_ksk *ksk0, const fhe_ksk *ksk1, const uint64_t *ct, uint64_t *out, size_t batch) {
    return host_call<RgswMul>(ksk0, ksk1, ct, out, batch);
}
fhe_status fhe_bfv_rgsw_mul_dev(const fhe_ksk *ksk0, const fhe_ksk *ksk1, const uint64_t *ct, uint64_t *out,
                                size_t batch, void *stream) {
    return dev_call<RgswMul>(stream, ksk0, ksk1, ct, out, batch);
}
// The key lists of inner sum and expand: the array, at least one key, every key.
static std::vector<const Ksk *> key_list(const fhe_ksk *const *gks, size_t ngk, const char *empty) {
    need(gks, "gks");
    if (ngk == 0) throw StatusError(FHE_E_ARG, empty);
    std::vector<const Ksk *> v;
    for (size_t i = 0; i < ngk; i++) {
        need(gks[i], "gks[i]");
        v.push_back(gks[i]->k.get());
    }
    return v;
}
struct InnerSum : Paired {   // EvaluationKey::computes_inner_sum
    std::vector<const Ksk *> gks;
    const size_t *exponents;
    std::array<Io, 2> io;
    InnerSum(const fhe_ksk *const *gks, const size_t *exponents, size_t ngk, const uint64_t *ct, uint64_t *out,
             size_t batch)
        : exponents(exponents) {
        need(exponents, "exponents");
        this->gks = key_list(gks, ngk, "inner sum needs at least one Galois key");
        on(*this->gks[0]->ksk_ctx, batch);
        if (batch) {
            need(ct, "ct");
            need(out, "out");
        }
        const size_t pe = this->gks[0]->ct_ctx->L * this->gks[0]->ct_ctx->n;
        io = {Io::in(ct, batch, 2 * pe), Io::out(out, batch, 2 * pe)};
    }
    void run(const Ptrs<2> &d, size_t n, hipStream_t s) const {
        inner_sum(gks.data(), exponents, gks.size(), d[0], d[1], n, s);
    }
};
fhe_status fhe_bfv_inner_sum(const fhe_ksk *const *gks, const size_t *exponents, size_t ngk, const uint64_t *ct,
                             uint64_t *out, size_t batch) {
    return host_call<InnerSum>(gks, exponents, ngk, ct, out, batch);
}
fhe_status fhe_bfv_inner_sum_dev(const fhe_ksk *const *gks, const size_t *exponents, size_t ngk, const uint64_t *ct,
                                 uint64_t *out, size_t batch, void *stream) {
    return dev_call<InnerSum>(stream, gks, exponents, ngk, ct, out, batch);
}

struct FromSeed : Paired {   // Poly::<Ntt>::random_from_seed: 32-byte seeds, staged in bytes
    std::array<Io, 2> io;
    FromSeed(const fhe_ctx *ctx, const uint8_t *seeds, uint64_t *out, size_t batch) {
        need(ctx, "ctx");
        on(*ctx->c, batch);
        if (batch) {
            need(seeds, "seeds");
            need(out, "out");
        }
        io = {Io{seeds, batch, 32, Io::IN}, Io::out(out, batch, dev->L * dev->n)};
    }
    void run(const Ptrs<2> &d, size_t n, hipStream_t s) const {
        polys_from_seeds(*dev, reinterpret_cast<const uint8_t *>(d[0]), d[1], n, s);
    }
};
fhe_status fhe_poly_from_seed(const fhe_ctx *ctx, const uint8_t *seeds, uint64_t *out, size_t batch) {
    return host_call<FromSeed>(ctx, seeds, out, batch);
}
fhe_status fhe_poly_from_seed_dev(const fhe_ctx *ctx, const uint8_t *seeds, uint64_t *out, size_t batch, void *stream) {
    return dev_call<FromSeed>(stream, ctx, seeds, out, batch);
}
struct Decrypt : Paired {   // SecretKey::try_decrypt
    const Scaler *sc;
    u64 t;
    size_t nparts;
    std::array<Io, 3> io;
    Decrypt(const fhe_scaler *scaler, uint64_t t, const uint64_t *s_ntt, const uint64_t *ct, size_t nparts, uint64_t *out,
            size_t batch)
        : t(t), nparts(nparts) {
        need(scaler, "cipher_plain_scaler");
        sc = scaler->s.get();
        on(*sc->from, batch);
        need(s_ntt, "s_ntt");
        if (batch) {
            need(ct, "ct");
            need(out, "out");
        }
        const Ctx &cc = *sc->from;
        const size_t pe = cc.L * cc.n;
        // the host form's staged secret key and plaintext are cleared on the device before their blocks are released
        // (the reference wraps s, c and the result in Zeroizing, F/bfv/keys/secret_key.rs:198-226)
        io = {Io::in(s_ntt, 1, pe, Io::SECRET), Io::in(ct, batch, nparts * pe), Io::out(out, batch, cc.n, Io::SECRET)};
    }
    void run(const Ptrs<3> &d, size_t n, hipStream_t s) const { decrypt(*sc, t, d[0], d[1], nparts, d[2], n, s); }
};
fhe_status fhe_bfv_decrypt(const fhe_scaler *sc, uint64_t t, const uint64_t *s_ntt, const uint64_t *ct, size_t nparts,
                           uint64_t *out, size_t batch) {
    return host_call<Decrypt>(sc, t, s_ntt, ct, nparts, out, batch);
}
fhe_status fhe_bfv_decrypt_dev(const fhe_scaler *sc, uint64_t t, const uint64_t *s_ntt, const uint64_t *ct, size_t nparts,
                               uint64_t *out, size_t batch, void *stream) {
    return dev_call<Decrypt>(stream, sc, t, s_ntt, ct, nparts, out, batch);
}

struct Expand : Paired {   // EvaluationKey::expands: out [size][batch][2][L][N]
    std::vector<const Ksk *> gks;
    size_t size;
    std::array<Io, 2> io;
    Expand(const fhe_ksk *const *gks, size_t nlevels, const uint64_t *ct, uint64_t *out, size_t size, size_t batch)
        : size(size) {
        this->gks = key_list(gks, nlevels, "expansion needs at least one Galois key");
        on(*this->gks[0]->ksk_ctx, batch);
        if (batch && size) {
            need(ct, "ct");
            need(out, "out");
        }
        const Ctx &cc = *this->gks[0]->ct_ctx;
        const size_t ce = 2 * cc.L * cc.n;
        const bool ok = size >= 1 && size <= cc.n;  // (the engine reports the error; do not size buffers from it)
        io = {Io::in(ct, batch, ce), Io::out(out, ok ? size * batch : 0, ce)};
    }
    void run(const Ptrs<2> &d, size_t n, hipStream_t s) const { expand(gks.data(), gks.size(), d[0], d[1], size, n, s); }
};
fhe_status fhe_bfv_expand(const fhe_ksk *const *gks, size_t nlevels, const uint64_t *ct, uint64_t *out, size_t size,
                          size_t batch) {
    return host_call<Expand>(gks, nlevels, ct, out, size, batch);
}
fhe_status fhe_bfv_expand_dev(const fhe_ksk *const *gks, size_t nlevels, const uint64_t *ct, uint64_t *out, size_t size,
                              size_t batch, void *stream) {
    return dev_call<Expand>(stream, gks, nlevels, ct, out, size, batch);
}

// ------------------------------------------------------------------- keyed batches ----
// One key per client (KskSet): device-pointer forms only.  Checks in the order of the paired calls: handles, the batch
// against the set's size, then the buffers; an empty batch is a no-op.
fhe_status fhe_kskset_create(const fhe_ksk *const *keys, size_t nkeys, fhe_kskset **out) {
    return guard([&] {
        need(out, "out");
        *out = nullptr;
        if (nkeys == 0) throw StatusError(FHE_E_ARG, "a key set needs at least one key");
        need(keys, "keys");
        std::vector<const Ksk *> v;
        for (size_t i = 0; i < nkeys; i++) {
            need(keys[i], "keys[i]");
            v.push_back(keys[i]->k.get());
        }
        set_device(*v[0]->ksk_ctx);
        auto h = std::make_unique<fhe_kskset>();
        h->s = kskset_create(v.data(), v.size());
        *out = h.release();
    });
}
void fhe_kskset_destroy(fhe_kskset *s) { delete s; }
size_t fhe_kskset_size(const fhe_kskset *s) { return s ? s->s->keys.size() : 0; }
fhe_status fhe_kskset_set_w_budget(fhe_kskset *s, size_t bytes) {
    return guard([&] {
        need(s, "set");
        s->s->w_budget.store(bytes, std::memory_order_relaxed);
    });
}
fhe_status fhe_kskset_get_w_budget(const fhe_kskset *s, size_t *bytes) {
    return guard([&] {
        need(s, "set");
        need(bytes, "bytes");
        *bytes = s->s->w_budget.load(std::memory_order_relaxed);
    });
}
fhe_status fhe_kskset_set_rot_split(fhe_kskset *s, size_t groups) {
    return guard([&] {
        need(s, "set");
        s->s->rot_split.store(groups, std::memory_order_relaxed);
    });
}
fhe_status fhe_kskset_get_rot_split(const fhe_kskset *s, size_t *groups) {
    return guard([&] {
        need(s, "set");
        need(groups, "groups");
        *groups = s->s->rot_split.load(std::memory_order_relaxed);
    });
}
fhe_status fhe_kskset_set_bsgs_tile(fhe_kskset *s, size_t gt) {
    return guard([&] {
        need(s, "set");
        if (gt != 0 && gt != 1 && gt != 2 && gt != 4)
            throw StatusError(FHE_E_ARG, "bsgs tile: 0 (the rule), 1, 2 or 4 giant groups per block, not " + std::to_string(gt));
        s->s->bsgs_tile.store(gt, std::memory_order_relaxed);
    });
}
fhe_status fhe_kskset_get_bsgs_tile(const fhe_kskset *s, size_t *gt) {
    return guard([&] {
        need(s, "set");
        need(gt, "gt");
        *gt = s->s->bsgs_tile.load(std::memory_order_relaxed);
    });
}
// The checks every keyed call shares; returns items per key (0: nothing to do).
static size_t keyed_per_key(const KskSet &set, size_t batch) {
    set.ksk_ctx->need_device();
    const size_t nkeys = set.keys.size();
    if (batch % nkeys != 0)
        throw StatusError(FHE_E_ARG, "keyed batches: batch " + std::to_string(batch) + " is not a multiple of the set's " +
                                         std::to_string(nkeys) + " keys");
    set_device(*set.ksk_ctx);
    return batch / nkeys;
}
// A list of sets (one per rotation / level) of one size; returns their first keys next to the KsKeyed entries.
static void keyed_list(const fhe_kskset *const *gks, size_t n, const char *empty, size_t batch, std::vector<const Ksk *> &first,
                       std::vector<KsKeyed> &keyed) {
    need(gks, "gks");
    if (n == 0) throw StatusError(FHE_E_ARG, empty);
    for (size_t i = 0; i < n; i++) need(gks[i], "gks[i]");
    for (size_t i = 0; i < n; i++) {
        const KskSet &set = *gks[i]->s;
        if (set.keys.size() != gks[0]->s->keys.size())
            throw StatusError(FHE_E_PARAMETER_MISMATCH, "keyed batches: the sets of one call must have the same size");
        first.push_back(set.keys[0]);
        keyed.push_back(KsKeyed{&set, 0});
    }
    const size_t m = keyed_per_key(*gks[0]->s, batch);
    for (KsKeyed &kd : keyed) kd.per_key = m;
}
fhe_status fhe_key_switch_keyed_dev(const fhe_kskset *s, const uint64_t *p, uint64_t *c0_out, uint64_t *c1_out, size_t batch,
                                    void *stream) {
    return guard([&] {
        need(s, "set");
        const KskSet &set = *s->s;
        const size_t m = keyed_per_key(set, batch);
        if (!batch) return;
        need(p, "p");
        need(c0_out, "c0_out");
        need(c1_out, "c1_out");
        const KsKeyed kd{&set, m};
        key_switch_polys(*set.keys[0], p, (u64)set.ct_ctx->L * set.ct_ctx->n, c0_out, c1_out, (u64)set.ksk_ctx->L * set.ksk_ctx->n,
                         nullptr, nullptr, 0, batch, as_stream(stream), nullptr, 0, 0, nullptr, &kd);
    });
}
fhe_status fhe_bfv_relinearize_keyed_dev(const fhe_kskset *rks, const uint64_t *ct3, uint64_t *out, size_t batch,
                                         void *stream) {
    return guard([&] {
        need(rks, "rks");
        const KskSet &set = *rks->s;
        const size_t m = keyed_per_key(set, batch);
        if (!batch) return;
        need(ct3, "ct3");
        need(out, "out");
        const KsKeyed kd{&set, m};
        relinearize_polys(*set.keys[0], ct3, out, batch, as_stream(stream), &kd);
    });
}
fhe_status fhe_bfv_galois_keyed_dev(const fhe_kskset *gks, size_t exponent, const uint64_t *ct, uint64_t *out, size_t batch,
                                    void *stream) {
    return guard([&] {
        need(gks, "gks");
        const KskSet &set = *gks->s;
        const size_t m = keyed_per_key(set, batch);
        if (!batch) return;
        need(ct, "ct");
        need(out, "out");
        const KsKeyed kd{&set, m};
        galois_apply(*set.keys[0], exponent, ct, out, batch, as_stream(stream), &kd);
    });
}
fhe_status fhe_bfv_inner_sum_keyed_dev(const fhe_kskset *const *gks, const size_t *exponents, size_t ngk, const uint64_t *ct,
                                       uint64_t *out, size_t batch, void *stream) {
    return guard([&] {
        need(exponents, "exponents");
        std::vector<const Ksk *> first;
        std::vector<KsKeyed> keyed;
        keyed_list(gks, ngk, "inner sum needs at least one Galois key", batch, first, keyed);
        if (!batch) return;
        need(ct, "ct");
        need(out, "out");
        inner_sum(first.data(), exponents, ngk, ct, out, batch, as_stream(stream), keyed.data());
    });
}
fhe_status fhe_bfv_expand_keyed_dev(const fhe_kskset *const *gks, size_t nlevels, const uint64_t *ct, uint64_t *out, size_t size,
                                    size_t batch, void *stream) {
    return guard([&] {
        std::vector<const Ksk *> first;
        std::vector<KsKeyed> keyed;
        keyed_list(gks, nlevels, "expansion needs at least one Galois key", batch, first, keyed);
        if (batch && size) {
            need(ct, "ct");
            need(out, "out");
        }
        expand(first.data(), nlevels, ct, out, size, batch, as_stream(stream), keyed.data());
    });
}
// Hoisted rotations: nrot Galois elements of each ciphertext on one digit decomposition (engine.hpp: galois_hoisted).
fhe_status fhe_bfv_galois_hoisted_dev(const fhe_kskset *gks, const size_t *exponents, size_t nrot, const uint64_t *ct,
                                      uint64_t *out, size_t batch, void *stream) {
    return guard([&] {
        need(gks, "gks");
        need(exponents, "exponents");
        const KskSet &set = *gks->s;
        if (nrot != set.keys.size())
            throw StatusError(FHE_E_ARG, "hoisted rotations: " + std::to_string(nrot) + " exponents for a set of " +
                                             std::to_string(set.keys.size()) + " keys");
        set.ksk_ctx->need_device();
        set_device(*set.ksk_ctx);
        if (batch) {
            need(ct, "ct");
            need(out, "out");
        }
        galois_hoisted(set, exponents, nrot, ct, out, batch, as_stream(stream));
    });
}
// Hoisted matrix-vector product: the rotations, the products with the diagonals and their sum in one stage B (engine.hpp:
// matvec_hoisted).
fhe_status fhe_bfv_matvec_hoisted_dev(const fhe_kskset *gks, const size_t *exponents, size_t nrot, const uint64_t *ct,
                                      const uint64_t *pts, int pts_shared, const uint64_t *pt0, uint64_t *out, size_t batch,
                                      void *stream) {
    return guard([&] {
        need(gks, "gks");
        need(exponents, "exponents");
        const KskSet &set = *gks->s;
        if (nrot != set.keys.size())
            throw StatusError(FHE_E_ARG, "hoisted matvec: " + std::to_string(nrot) + " exponents for a set of " +
                                             std::to_string(set.keys.size()) + " keys");
        set.ksk_ctx->need_device();
        set_device(*set.ksk_ctx);
        if (batch) {
            need(ct, "ct");
            need(pts, "pts");
            need(out, "out");
        }
        matvec_hoisted(set, exponents, nrot, ct, pts, pts_shared != 0, pt0, out, batch, as_stream(stream));
    });
}
// The two hoisted calls with one Galois key set per client (engine.hpp: galois_hoisted_keyed, matvec_hoisted_keyed): the
// refusals of the client count, in this order, then those of the unkeyed calls.
static void hoisted_keyed_counts(const char *what, const KskSet &set, size_t nclients, size_t nrot, size_t batch) {
    if (nclients == 0)
        throw StatusError(FHE_E_ARG, std::string(what) + ": 0 clients for a set of " + std::to_string(set.keys.size()) + " keys");
    if (nrot != set.keys.size() / nclients || nclients * nrot != set.keys.size())
        throw StatusError(FHE_E_ARG, std::string(what) + ": " + std::to_string(nclients) + " clients x " + std::to_string(nrot) +
                                         " exponents for a set of " + std::to_string(set.keys.size()) + " keys");
    if (batch % nclients != 0)
        throw StatusError(FHE_E_ARG, std::string(what) + ": batch " + std::to_string(batch) + " is not a multiple of the " +
                                         std::to_string(nclients) + " clients");
}
fhe_status fhe_bfv_galois_hoisted_keyed_dev(const fhe_kskset *gks, size_t nclients, const size_t *exponents, size_t nrot,
                                            const uint64_t *ct, uint64_t *out, size_t batch, void *stream) {
    return guard([&] {
        need(gks, "gks");
        need(exponents, "exponents");
        const KskSet &set = *gks->s;
        hoisted_keyed_counts("keyed hoisted rotations", set, nclients, nrot, batch);
        set.ksk_ctx->need_device();
        set_device(*set.ksk_ctx);
        if (batch) {
            need(ct, "ct");
            need(out, "out");
        }
        galois_hoisted_keyed(set, nclients, exponents, nrot, ct, out, batch, as_stream(stream));
    });
}
fhe_status fhe_bfv_matvec_hoisted_keyed_dev(const fhe_kskset *gks, size_t nclients, const size_t *exponents, size_t nrot,
                                            const uint64_t *ct, const uint64_t *pts, int pts_shared, const uint64_t *pt0,
                                            uint64_t *out, size_t batch, void *stream) {
    return guard([&] {
        need(gks, "gks");
        need(exponents, "exponents");
        const KskSet &set = *gks->s;
        hoisted_keyed_counts("keyed hoisted matvec", set, nclients, nrot, batch);
        set.ksk_ctx->need_device();
        set_device(*set.ksk_ctx);
        if (batch) {
            need(ct, "ct");
            need(pts, "pts");
            need(out, "out");
        }
        matvec_hoisted_keyed(set, nclients, exponents, nrot, ct, pts, pts_shared != 0, pt0, out, batch, as_stream(stream));
    });
}
// Baby-step/giant-step hoisted matrix-vector product (engine.hpp: matvec_bsgs).
fhe_status fhe_bfv_matvec_bsgs_dev(const fhe_kskset *baby, const size_t *baby_exps, size_t nbaby, const fhe_kskset *giant,
                                   const size_t *giant_exps, size_t ngiant, const uint64_t *ct, const uint64_t *pts,
                                   int pts_shared, uint64_t *out, size_t batch, void *stream) {
    return guard([&] {
        need(baby, "baby");
        need(baby_exps, "baby_exps");
        need(giant, "giant");
        need(giant_exps, "giant_exps");
        const KskSet &bs = *baby->s, &gs = *giant->s;
        auto count = [](const char *which, size_t n, const KskSet &set) {
            if (n != set.keys.size())
                throw StatusError(FHE_E_ARG, std::string("bsgs matvec: ") + std::to_string(n) + " " + which +
                                                 " exponents for a set of " + std::to_string(set.keys.size()) + " keys");
        };
        count("baby", nbaby, bs);
        count("giant", ngiant, gs);
        bs.ksk_ctx->need_device();
        set_device(*bs.ksk_ctx);
        if (batch) {
            need(ct, "ct");
            need(pts, "pts");
            need(out, "out");
        }
        matvec_bsgs(bs, baby_exps, nbaby, gs, giant_exps, ngiant, ct, pts, pts_shared != 0, out, batch, as_stream(stream));
    });
}

// ----------------------------------------------------------------------------- mul ----
static std::unique_ptr<Mul> make_mul(const Scaler *el, const Scaler *er, const Scaler *dn, const Ksk *rk,
                                     bool mod_switch) {
    require(el->from->same_ring(*er->from) && el->to->same_ring(*er->to), E_PARAMETER_MISMATCH,
            "extenders disagree on contexts");
    require(dn->from->same_ring(*el->to) && dn->to->same_ring(*el->from), E_PARAMETER_MISMATCH,
            "down scaler does not invert the extenders' contexts");
    auto m = std::make_unique<Mul>();
    m->ext_lhs = el;
    m->ext_rhs = er;
    m->down = dn;
    m->rk = rk;
    m->mod_switch = mod_switch;
    m->base = el->from;
    m->mulc = el->to;
    // the extenders hand their common rows over in Ntt form (M/rq/scaler.rs:61-65): those moduli must be evaluated in
    // the same order on both sides, i.e. both contexts were built from the same NTT tables
    require(m->base->same_tables(*m->mulc, std::min(el->ncommon, er->ncommon)) &&
                el->from->same_tables(*er->from, el->from->L) && el->to->same_tables(*er->to, el->to->L) &&
                dn->from->same_tables(*el->to, el->to->L) && dn->to->same_tables(*el->from, el->from->L),
            E_PARAMETER_MISMATCH, "ParameterMismatch: the multiplicator's contexts were built with different NTT tables");
    if (rk) {  // enable_relinearization (mul.rs:141-151)
        require(rk->ct_ctx->same_ring(*m->base), E_PARAMETER_MISMATCH,
                "ParameterMismatch: relinearization key level != multiplicator level");
        require(rk->ct_ctx->same_tables(*m->base, m->base->L), E_PARAMETER_MISMATCH,
                "ParameterMismatch: relinearization key and multiplicator were built with different NTT tables");
    }
    if (mod_switch) require(m->base->next != nullptr, E_NO_MORE_CONTEXT, "NoMoreContext");  // mul.rs:155-162
    return m;
}
fhe_status fhe_mul_create(const fhe_scaler *extender_lhs, const fhe_scaler *extender_rhs, const fhe_scaler *down_scaler,
                          const fhe_ksk *rk_or_null, int mod_switch, fhe_mul **out) {
    return guard([&] {
        need(extender_lhs, "extender_lhs");
        need(extender_rhs, "extender_rhs");
        need(down_scaler, "down_scaler");
        need(out, "out");
        *out = nullptr;
        auto h = std::make_unique<fhe_mul>();
        h->m = make_mul(extender_lhs->s.get(), extender_rhs->s.get(), down_scaler->s.get(),
                        rk_or_null ? rk_or_null->k.get() : nullptr, mod_switch != 0);
        *out = h.release();
    });
}
void fhe_mul_destroy(fhe_mul *m) { delete m; }
fhe_status fhe_mul_out_shape(const fhe_mul *m, size_t *parts, size_t *rows) {
    return guard([&] {
        need(m, "mul");
        if (parts) *parts = m->m->out_parts();
        if (rows) *rows = m->m->out_rows();
    });
}
fhe_status fhe_mul_basis(const fhe_mul *m, size_t *count, uint64_t *moduli) {
    return guard([&] {
        need(m, "mul");
        need(count, "count");
        *count = m->m->mulc->L;
        if (moduli) std::copy(m->m->mulc->moduli.begin(), m->m->mulc->moduli.end(), moduli);
    });
}
fhe_status fhe_mul_set_chunk(fhe_mul *m, size_t chunk) {
    return guard([&] {
        need(m, "mul");
        m->m->chunk.store(chunk, std::memory_order_relaxed);
    });
}
fhe_status fhe_mul_set_streams(fhe_mul *m, size_t streams) {
    return guard([&] {
        need(m, "mul");
        require(streams == 1 || streams == 2, E_ARG, "streams must be 1 or 2");
        m->m->streams.store(streams, std::memory_order_relaxed);
    });
}
fhe_status fhe_mul_get_options(const fhe_mul *m, size_t *chunk, size_t *streams) {
    return guard([&] {
        need(m, "mul");
        if (chunk) *chunk = m->m->chunk.load(std::memory_order_relaxed);
        if (streams) *streams = m->m->streams.load(std::memory_order_relaxed);
    });
}
struct BfvMul : Paired {   // Multiplicator::multiply
    static constexpr bool sliced = true;
    const Mul *mm;
    std::array<Io, 3> io;
    BfvMul(const fhe_mul *m, const uint64_t *lhs, const uint64_t *rhs, uint64_t *out, size_t batch) {
        need(m, "mul");
        mm = m->m.get();
        on(*mm->base, batch);
        if (batch) {
            need(lhs, "lhs");
            need(rhs, "rhs");
            need(out, "out");
        }
        const size_t ie = 2 * mm->base->L * mm->base->n, oe = mm->out_parts() * mm->out_rows() * mm->base->n;
        // (lhs == rhs: one upload, and the squaring shortcut of bfv_mul)
        io = {Io::in(lhs, batch, ie), Io::in(rhs, batch, ie), Io::out(out, batch, oe)};
    }
    void run(const Ptrs<3> &d, size_t n, hipStream_t s) const { bfv_mul(*mm, d[0], d[1], d[2], n, s); }
};
fhe_status fhe_bfv_mul(const fhe_mul *m, const uint64_t *lhs, const uint64_t *rhs, uint64_t *out, size_t batch) {
    return host_call<BfvMul>(m, lhs, rhs, out, batch);
}
fhe_status fhe_bfv_mul_dev(const fhe_mul *m, const uint64_t *lhs, const uint64_t *rhs, uint64_t *out, size_t batch,
                           void *stream) {
    return dev_call<BfvMul>(stream, m, lhs, rhs, out, batch);
}

struct Tensor : Paired {   // `Mul<&Ciphertext> for &Ciphertext` with any number of parts
    const Mul *mm;
    size_t lhs_parts, rhs_parts;
    std::array<Io, 3> io;
    Tensor(const fhe_mul *m, size_t lhs_parts, size_t rhs_parts, const uint64_t *lhs, const uint64_t *rhs, uint64_t *out,
           size_t batch)
        : lhs_parts(lhs_parts), rhs_parts(rhs_parts) {
        need(m, "mul");
        mm = m->m.get();
        on(*mm->base, batch);
        if (lhs_parts < 1 || rhs_parts < 1)
            throw StatusError(FHE_E_MUL_POLY_COUNT, "a ciphertext has at least one part");
        if (batch) {
            need(lhs, "lhs");
            need(rhs, "rhs");
            need(out, "out");
        }
        const size_t pe = mm->base->L * mm->base->n;
        io = {Io::in(lhs, batch, lhs_parts * pe), Io::in(rhs, batch, rhs_parts * pe),
              Io::out(out, batch, (lhs_parts + rhs_parts - 1) * pe)};
    }
    void run(const Ptrs<3> &d, size_t n, hipStream_t s) const {
        bfv_tensor(*mm, lhs_parts, rhs_parts, d[0], d[1], d[2], n, s);
    }
};
fhe_status fhe_bfv_tensor(const fhe_mul *m, size_t lhs_parts, size_t rhs_parts, const uint64_t *lhs, const uint64_t *rhs,
                          uint64_t *out, size_t batch) {
    return host_call<Tensor>(m, lhs_parts, rhs_parts, lhs, rhs, out, batch);
}
fhe_status fhe_bfv_tensor_dev(const fhe_mul *m, size_t lhs_parts, size_t rhs_parts, const uint64_t *lhs,
                              const uint64_t *rhs, uint64_t *out, size_t batch, void *stream) {
    return dev_call<Tensor>(stream, m, lhs_parts, rhs_parts, lhs, rhs, out, batch);
}

// -------------------------------------------------------------------------- params ----
static void params_create(int device, size_t degree, size_t nmoduli, const uint64_t *moduli, const BigUint &t,
                          fhe_ntt_tables_fn tables, void *user, fhe_params **out) {
    need(out, "out");
    *out = nullptr;
    if (nmoduli == 0) throw StatusError(FHE_E_EMPTY_MODULI, "EmptyModuli");
    need(moduli, "moduli");
    require(t >= BigUint(2), E_ARG, "plaintext modulus must be >= 2");
    auto p = std::make_unique<fhe_params>();
    p->device = device;
    p->host_tables = tables != nullptr;
    p->degree = degree;
    p->plaintext = t.fits_u64() ? t.to_u64() : 0;
    p->plaintext_big = t;
    p->moduli.assign(moduli, moduli + nmoduli);
    for (u64 q : p->moduli) p->moduli_sizes.push_back(64 - (size_t)__builtin_clzll(q | 1));
    p->top = wrap_ctx(ctx_create_cb(device, degree, p->moduli, tables, user, p->host_tables, p->table_cache));
    if (!t.fits_u64()) {
        // PlaintextModulus::Large: t below Q, invertible modulo every q_i (parameters.rs:607-633)
        require(t < ctx_modulus(*p->top->c), E_INVALID_MODULUS, "the plaintext modulus must be below the ciphertext modulus");
        for (u64 q : p->moduli)
            require(t.mod_u64(q) != 0, E_INVALID_MODULUS, "the plaintext modulus must be invertible modulo every q_i");
    }
    // extended basis: n+1 primes of 62 bits (parameters.rs:660-676)
    std::vector<u64> ext = extended_basis_primes(degree, p->moduli, nmoduli + 1);
    for (size_t level = 0; level < nmoduli; level++) {
        const size_t nl = nmoduli - level;
        size_t modulus_size = 0;
        for (size_t i = 0; i < nl; i++) modulus_size += p->moduli_sizes[i];
        const size_t n_moduli = (modulus_size + 60 + 61) / 62;  // div_ceil
        std::vector<u64> mm(p->moduli.begin(), p->moduli.begin() + nl);
        mm.insert(mm.end(), ext.begin(), ext.begin() + n_moduli);
        auto mc = wrap_ctx(ctx_create_cb(device, degree, mm, tables, user, p->host_tables, p->table_cache));
        const Ctx &base = *p->top->c->at_level(level);
        RnsContext rb(base.moduli);
        auto e = std::make_unique<fhe_scaler>();
        e->s = scaler_create(base, *mc->c, BigUint(1), BigUint(1));
        auto d = std::make_unique<fhe_scaler>();
        d->s = scaler_create(*mc->c, base, t, rb.product);
        p->mul_ctx.push_back(std::move(mc));
        p->extender.push_back(std::move(e));
        p->down.push_back(std::move(d));
    }
    *out = p.release();
}
fhe_status fhe_params_create_with_tables(int device, size_t degree, size_t nmoduli, const uint64_t *moduli,
                                         uint64_t plaintext_modulus, fhe_ntt_tables_fn tables, void *user,
                                         fhe_params **out) {
    return guard([&] { params_create(device, degree, nmoduli, moduli, BigUint(plaintext_modulus), tables, user, out); });
}
// BfvParametersBuilder::set_plaintext_modulus_biguint + build (F/bfv/parameters.rs:560-738)
fhe_status fhe_params_create_big_with_tables(int device, size_t degree, size_t nmoduli, const uint64_t *moduli,
                                             const uint64_t *t_limbs, size_t t_nlimbs, fhe_ntt_tables_fn tables,
                                             void *user, fhe_params **out) {
    return guard([&] {
        need(out, "out");
        *out = nullptr;
        need(t_limbs, "t_limbs");
        const BigUint t = BigUint::from_limbs(t_limbs, t_nlimbs);
        if (!t.fits_u64()) {
            require(t.w.size() <= (size_t)k::BIGT_WMAX, E_INVALID_MODULUS, "the plaintext modulus must be below 2^256");
        } else if (nmoduli) {
            // (the reference's PlaintextModulus::Small holds a Modulus: below 2^62)
            require((t.to_u64() >> 62) == 0, E_INVALID_MODULUS, "InvalidPlaintextModulus: a 64-bit t must be below 2^62");
        }
        params_create(device, degree, nmoduli, moduli, t, tables, user, out);
    });
}
fhe_status fhe_params_create_big(int device, size_t degree, size_t nmoduli, const uint64_t *moduli, const uint64_t *t_limbs,
                                 size_t t_nlimbs, fhe_params **out) {
    return fhe_params_create_big_with_tables(device, degree, nmoduli, moduli, t_limbs, t_nlimbs, nullptr, nullptr, out);
}
size_t fhe_params_plaintext_limbs(const fhe_params *p) { return p ? std::max<size_t>(1, p->plaintext_big.w.size()) : 0; }
fhe_status fhe_params_create(int device, size_t degree, size_t nmoduli, const uint64_t *moduli,
                             uint64_t plaintext_modulus, fhe_params **out) {
    return fhe_params_create_with_tables(device, degree, nmoduli, moduli, plaintext_modulus, nullptr, nullptr, out);
}
void fhe_params_destroy(fhe_params *p) { delete p; }
size_t fhe_params_max_level(const fhe_params *p) { return p ? p->moduli.size() - 1 : 0; }
#define FHE_PARAMS_LEVEL_CHECK()                                                          \
    need(p, "params");                                                                    \
    need(out, "out");                                                                     \
    if (level >= p->moduli.size()) throw StatusError(FHE_E_INVALID_LEVEL, "InvalidLevel")
fhe_status fhe_params_ctx(const fhe_params *p, size_t level, const fhe_ctx **out) {
    return guard([&] {
        FHE_PARAMS_LEVEL_CHECK();
        *out = ctx_level_handle(p->top.get(), level);
    });
}
fhe_status fhe_params_mul_ctx(const fhe_params *p, size_t level, const fhe_ctx **out) {
    return guard([&] {
        FHE_PARAMS_LEVEL_CHECK();
        *out = p->mul_ctx[level].get();
    });
}
fhe_status fhe_params_extender(const fhe_params *p, size_t level, const fhe_scaler **out) {
    return guard([&] {
        FHE_PARAMS_LEVEL_CHECK();
        *out = p->extender[level].get();
    });
}
fhe_status fhe_params_down_scaler(const fhe_params *p, size_t level, const fhe_scaler **out) {
    return guard([&] {
        FHE_PARAMS_LEVEL_CHECK();
        *out = p->down[level].get();
    });
}
fhe_status fhe_mul_create_default(const fhe_params *p, size_t level, const fhe_ksk *rk_or_null, int mod_switch,
                                  fhe_mul **out) {
    return guard([&] {
        FHE_PARAMS_LEVEL_CHECK();
        *out = nullptr;
        auto h = std::make_unique<fhe_mul>();
        const Scaler *ext = p->extender[level]->s.get(), *down = p->down[level]->s.get();
        if (rk_or_null) {
            // Multiplicator::default (mul.rs:101-138): the extension primes skip only the moduli of rk's level
            // (parameters.rs:660-676 skips every top-level modulus).  Where the two bases differ -- a dropped
            // top-level modulus is itself one of the first 62-bit NTT primes -- the handle gets its own
            // multiplication context and scalers, exactly the reference's new_leveled_internal.
            const Ctx &base = *p->top->c->at_level(level);
            size_t modulus_size = 0;
            for (size_t i = 0; i < base.L; i++) modulus_size += p->moduli_sizes[i];
            const size_t n_moduli = (modulus_size + 60 + 61) / 62;
            std::vector<u64> mm = base.moduli;
            const std::vector<u64> extp = extended_basis_primes(p->degree, base.moduli, n_moduli);
            mm.insert(mm.end(), extp.begin(), extp.end());
            if (mm != p->mul_ctx[level]->c->moduli) {
                // (every prime of this basis is a top-level modulus or one of the cached extension primes)
                auto mc = wrap_ctx(ctx_create_cb(p->device, p->degree, mm, nullptr, nullptr, p->host_tables,
                                                 const_cast<fhe_params *>(p)->table_cache));
                RnsContext rb(base.moduli);
                auto e = std::make_unique<fhe_scaler>();
                e->s = scaler_create(base, *mc->c, BigUint(1), BigUint(1));
                auto d = std::make_unique<fhe_scaler>();
                d->s = scaler_create(*mc->c, base, p->plaintext_big, rb.product);
                ext = e->s.get();
                down = d->s.get();
                h->ctxs.push_back(std::move(mc));
                h->scalers.push_back(std::move(e));
                h->scalers.push_back(std::move(d));
            }
        }
        h->m = make_mul(ext, ext, down, rk_or_null ? rk_or_null->k.get() : nullptr, mod_switch != 0);
        *out = h.release();
    });
}

// ------------------------------------------------------------------ plaintext encoding ----
// Device-pointer forms only (like fhe_synth_uniform_dev): a host without PyTorch stages through fhe_buf_*.
fhe_status fhe_encoder_create(const fhe_params *par, fhe_ntt_tables_fn tables, void *user, fhe_encoder **out) {
    return guard([&] {
        need(par, "params");
        need(out, "out");
        *out = nullptr;
        const Ctx &top = *par->top->c;
        top.need_device();
        set_device(top);
        // NttOperator::new(t, N) exists iff t supports it (parameters.rs:71-75, 598); otherwise SIMD is unavailable
        if (!par->plaintext_big.fits_u64()) {   // PlaintextModulus::Large: no ntt_operator, SIMD unavailable
            auto h = std::make_unique<fhe_encoder>();
            h->e = encoder_create_big(top, par->plaintext_big);
            *out = h.release();
            return;
        }
        std::unique_ptr<Ctx> tctx;
        if (supports_ntt(par->plaintext, par->degree)) {
            std::map<u64, HostTables> cache;
            tctx = ctx_create_cb(par->device, par->degree, {par->plaintext}, tables, user, tables != nullptr, cache);
        }
        auto h = std::make_unique<fhe_encoder>();
        h->e = encoder_create(top, par->plaintext, std::move(tctx));
        *out = h.release();
    });
}
void fhe_encoder_destroy(fhe_encoder *enc) { delete enc; }
fhe_status fhe_bfv_encode_dev(const fhe_encoder *enc, int encoding, int scaled, size_t level, const uint64_t *values,
                              size_t nvalues, uint64_t *out, size_t batch, void *stream) {
    return guard([&] {
        need(enc, "encoder");
        require(encoding == FHE_ENCODING_POLY || encoding == FHE_ENCODING_SIMD, E_ARG, "unknown encoding");
        if (batch) {
            if (nvalues) need(values, "values");
            need(out, "out");
        }
        set_device(*enc->e->top);
        encode(*enc->e, encoding == FHE_ENCODING_SIMD, scaled != 0, level, values, nvalues, out, batch, as_stream(stream));
    });
}
fhe_status fhe_bfv_decode_dev(const fhe_encoder *enc, int encoding, const uint64_t *coeffs, uint64_t *out, size_t batch,
                              void *stream) {
    return guard([&] {
        need(enc, "encoder");
        require(encoding == FHE_ENCODING_POLY || encoding == FHE_ENCODING_SIMD, E_ARG, "unknown encoding");
        if (batch) {
            need(coeffs, "coeffs");
            need(out, "out");
        }
        set_device(*enc->e->top);
        decode(*enc->e, encoding == FHE_ENCODING_SIMD, coeffs, out, batch, as_stream(stream));
    });
}
fhe_status fhe_bfv_encode_bytes_dev(const fhe_encoder *enc, int scaled, size_t level, const uint8_t *bytes, size_t nbytes,
                                    size_t item_bytes, size_t nbits, uint64_t *out, size_t batch, void *stream) {
    return guard([&] {
        need(enc, "encoder");
        if (batch) {
            if (nbytes) need(bytes, "bytes");
            need(out, "out");
        }
        set_device(*enc->e->top);
        encode_stream(*enc->e, scaled != 0, level, bytes, true, nbytes, 8, 1, item_bytes, nbits, out, batch, as_stream(stream));
    });
}
size_t fhe_bfv_encode_words_count(const fhe_encoder *enc, size_t in_bits, size_t nseg, size_t seg_len, size_t nbits) {
    return enc ? (size_t)stream_plaintexts(*enc->e, in_bits, nseg, seg_len, nbits) : 0;
}
fhe_status fhe_bfv_encode_words_dev(const fhe_encoder *enc, int scaled, size_t level, const uint64_t *words, size_t in_bits,
                                    size_t nseg, size_t seg_len, size_t nbits, uint64_t *out, size_t batch, void *stream) {
    return guard([&] {
        need(enc, "encoder");
        if (batch && nseg && seg_len) {
            need(words, "words");
            need(out, "out");
        }
        set_device(*enc->e->top);
        require(nseg == 0 || seg_len == 0 || batch <= ((size_t)1 << 62) / nseg / seg_len, E_ARG, "encode: too many elements");
        encode_stream(*enc->e, scaled != 0, level, words, false, (u64)batch * nseg * seg_len, in_bits, nseg, seg_len, nbits,
                      out, batch, as_stream(stream));
    });
}
size_t fhe_transcode_count(size_t in_bits, size_t nin, size_t out_bits) {
    if (in_bits < 1 || in_bits > 64 || out_bits < 1 || out_bits > 64 || nin > TRANSCODE_MAX_ELEMS) return 0;
    return (size_t)transcode_count(in_bits, nin, out_bits);
}
fhe_status fhe_transcode_dev(const void *in, int in_is_bytes, size_t in_bits, size_t nin, void *out, int out_is_bytes,
                             size_t out_bits, size_t batch, void *stream) {
    return guard([&] {
        if (batch && nin) {
            need(in, "in");
            need(out, "out");
        }
        transcode(in, in_is_bytes != 0, in_bits, nin, out, out_is_bytes != 0, out_bits, batch, as_stream(stream));
    });
}
fhe_status fhe_bfv_add_plain_dev(const fhe_ctx *ctx, int subtract, size_t nparts, const uint64_t *ct, const uint64_t *pt,
                                 int pt_shared, uint64_t *out, size_t batch, void *stream) {
    return guard([&] {
        need(ctx, "ctx");
        const Ctx &c = *ctx->c;
        c.need_device();
        if (batch) {
            need(ct, "ct");
            need(pt, "pt");
            need(out, "out");
        }
        set_device(c);
        add_plain(c, subtract != 0, nparts, ct, pt, pt_shared != 0, out, batch, as_stream(stream));
    });
}

// --------------------------------------------------------------------- lift and noise ----
// Device-pointer forms only: the phase and the error polynomial never pass through host memory.
size_t fhe_ctx_lift_limbs(const fhe_ctx *ctx) { return ctx ? lift_limbs(*ctx->c) : 0; }
fhe_status fhe_poly_lift_dev(const fhe_ctx *ctx, const uint64_t *polys, uint64_t *out, size_t batch, void *stream) {
    return guard([&] {
        need(ctx, "ctx");
        const Ctx &c = *ctx->c;
        c.need_device();
        if (batch) {
            need(polys, "polys");
            need(out, "out");
        }
        set_device(c);
        poly_lift(c, polys, out, batch, as_stream(stream));
    });
}
fhe_status fhe_poly_centered_bits_dev(const fhe_ctx *ctx, const uint64_t *polys, uint64_t *out_bits, size_t batch,
                                      void *stream) {
    return guard([&] {
        need(ctx, "ctx");
        const Ctx &c = *ctx->c;
        c.need_device();
        if (batch) {
            need(polys, "polys");
            need(out_bits, "out_bits");
        }
        set_device(c);
        centered_bits(c, polys, k::lift_sub_none(), out_bits, batch, as_stream(stream));
    });
}
fhe_status fhe_bfv_measure_noise_dev(const fhe_encoder *enc, const fhe_scaler *sc, const uint64_t *s_ntt, const uint64_t *ct,
                                     size_t nparts, const uint64_t *m_or_null, uint64_t *noise_bits, size_t batch,
                                     void *stream) {
    return guard([&] {
        need(enc, "encoder");
        need(sc, "cipher_plain_scaler");
        sc->s->from->need_device();
        if (batch) {
            need(s_ntt, "s_ntt");
            need(ct, "ct");
            need(noise_bits, "noise_bits");
        }
        set_device(*sc->s->from);
        measure_noise(*enc->e, *sc->s, s_ntt, ct, nparts, m_or_null, noise_bits, batch, as_stream(stream));
    });
}

// ------------------------------------------------------ plaintext moduli above 64 bits ----
// Device-pointer forms only, like the u64 encoding entry points.
fhe_status fhe_bfv_encode_big_dev(const fhe_encoder *enc, int encoding, int scaled, size_t level, const uint64_t *values,
                                  size_t nvalues, uint64_t *out, size_t batch, void *stream) {
    return guard([&] {
        need(enc, "encoder");
        require(encoding == FHE_ENCODING_POLY || encoding == FHE_ENCODING_SIMD, E_ARG, "unknown encoding");
        if (batch) {
            if (nvalues) need(values, "values");
            need(out, "out");
        }
        set_device(*enc->e->top);
        encode_big(*enc->e, encoding == FHE_ENCODING_SIMD, scaled != 0, level, values, nvalues, out, batch, as_stream(stream));
    });
}
size_t fhe_encoder_plain_rows(const fhe_encoder *enc) {
    if (!enc) return 0;
    const Encoder &e = *enc->e;
    return e.big() ? e.plain->L : plain_rows(*e.top, 64 - (size_t)__builtin_clzll(e.t | 1));
}
fhe_status fhe_bfv_reduce_big_dev(const fhe_encoder *enc, const uint64_t *polys, size_t rows, uint64_t *out, size_t batch,
                                  void *stream) {
    return guard([&] {
        need(enc, "encoder");
        if (batch) {
            need(polys, "polys");
            need(out, "out");
        }
        set_device(*enc->e->top);
        reduce_big(*enc->e, polys, rows, out, batch, as_stream(stream));
    });
}
fhe_status fhe_bfv_decrypt_big_dev(const fhe_encoder *enc, const fhe_scaler *sc, const uint64_t *s_ntt, const uint64_t *ct,
                                   size_t nparts, uint64_t *out, size_t batch, void *stream) {
    return guard([&] {
        need(enc, "encoder");
        need(sc, "cipher_plain_scaler");
        sc->s->from->need_device();
        if (batch) {
            need(s_ntt, "s_ntt");
            need(ct, "ct");
            need(out, "out");
        }
        set_device(*sc->s->from);
        decrypt_big(*enc->e, *sc->s, s_ntt, ct, nparts, out, batch, as_stream(stream));
    });
}
fhe_status fhe_mbfv_decrypt_big_dev(const fhe_encoder *enc, const fhe_scaler *sc, const uint64_t *ct, const uint64_t *shares,
                                    size_t nshares, size_t share_stride, uint64_t *out, size_t batch, void *stream) {
    return guard([&] {
        need(enc, "encoder");
        need(sc, "cipher_plain_scaler");
        sc->s->from->need_device();
        if (batch) {
            need(ct, "ct");
            need(shares, "shares");
            need(out, "out");
        }
        set_device(*sc->s->from);
        mbfv_decrypt_big(*enc->e, *sc->s, ct, shares, nshares, share_stride, out, batch, as_stream(stream));
    });
}

// ------------------------------------------------------------------------- encryption ----
// Device-pointer forms only, like the encoding entry points: secrets and errors are never staged through host memory
// by the engine.
fhe_status fhe_bfv_sample_small_dev(const fhe_ctx *ctx, size_t variance, const uint8_t *seeds, int to_ntt, uint64_t *out,
                                    size_t batch, void *stream) {
    return guard([&] {
        need(ctx, "ctx");
        const Ctx &c = *ctx->c;
        c.need_device();
        check_variance(variance);
        if (batch) {
            need(seeds, "seeds");
            need(out, "out");
        }
        set_device(c);
        sample_small(c, variance, seeds, to_ntt != 0, out, batch, as_stream(stream));
    });
}
fhe_status fhe_bfv_encrypt_sk_dev(const fhe_ctx *ctx, size_t variance, const uint64_t *s_ntt, const uint8_t *a_seeds,
                                  const uint8_t *e_seeds, const uint64_t *pt, int pt_shared, uint64_t *out, size_t batch,
                                  void *stream) {
    return guard([&] {
        need(ctx, "ctx");
        const Ctx &c = *ctx->c;
        c.need_device();
        check_variance(variance);
        if (batch) {
            need(s_ntt, "s_ntt");
            need(a_seeds, "a_seeds");
            need(e_seeds, "e_seeds");
            need(out, "out");
        }
        set_device(c);
        encrypt_sk(c, variance, s_ntt, a_seeds, e_seeds, pt, pt_shared != 0, out, batch, as_stream(stream));
    });
}
fhe_status fhe_bfv_encrypt_pk_dev(const fhe_ctx *ctx, size_t variance, const uint64_t *pk, const uint8_t *seeds,
                                  const uint64_t *pt, int pt_shared, uint64_t *out, size_t batch, void *stream) {
    return guard([&] {
        need(ctx, "ctx");
        const Ctx &c = *ctx->c;
        c.need_device();
        check_variance(variance);
        if (batch) {
            need(pk, "pk");
            need(seeds, "seeds");
            need(out, "out");
        }
        set_device(c);
        encrypt_pk(c, variance, pk, seeds, pt, pt_shared != 0, out, batch, as_stream(stream));
    });
}

// --------------------------------------------------------------------- key generation ----
// Device-pointer forms only, like encryption.  Each checks its handles, the device, the variance and the key's
// geometry before it looks at a buffer; nkeys == 0 is a no-op.  The handles are made all or none: on an error none is
// returned and none leaks.
static void keygen_checks(const fhe_ctx *ct_ctx, const fhe_ctx *key_ctx, size_t variance) {
    need(ct_ctx, "ct_ctx");
    need(key_ctx, "key_ctx");
    key_ctx->c->need_device();
    check_variance(variance);
}
static void keygen_out(std::vector<std::unique_ptr<Ksk>> keys, fhe_ksk **out) {
    std::vector<std::unique_ptr<fhe_ksk>> hs;
    for (auto &k_ : keys) {
        hs.push_back(std::make_unique<fhe_ksk>());
        hs.back()->k = std::move(k_);
    }
    for (size_t i = 0; i < hs.size(); i++) out[i] = hs[i].release();
}
fhe_status fhe_ksk_generate_dev(const fhe_ctx *ct_ctx, const fhe_ctx *ksk_ctx, size_t variance, const uint64_t *s_ntt,
                                const uint64_t *from_ntt, const uint8_t *seeds, size_t nkeys, uint8_t *seeds_out,
                                void *stream, fhe_ksk **out) {
    return guard([&] {
        keygen_checks(ct_ctx, ksk_ctx, variance);
        const Ctx &ct = *ct_ctx->c, &kc = *ksk_ctx->c;
        const auto dg = ksk_digits(ct, kc);
        ksk_validate(ct, kc, dg.first, dg.second);
        if (!nkeys) return;
        need(out, "out");
        for (size_t i = 0; i < nkeys; i++) out[i] = nullptr;
        need(s_ntt, "s_ntt");
        need(from_ntt, "from_ntt");
        need(seeds, "seeds");
        set_device(kc);
        keygen_out(ksk_generate(ct, kc, variance, s_ntt, from_ntt, seeds, nkeys, seeds_out, as_stream(stream)), out);
    });
}
fhe_status fhe_bfv_relin_key_generate_dev(const fhe_ctx *ct_ctx, const fhe_ctx *key_ctx, size_t variance,
                                          const uint64_t *s_ntt, const uint8_t *seed, uint8_t *seed_out, void *stream,
                                          fhe_ksk **out) {
    return guard([&] {
        keygen_checks(ct_ctx, key_ctx, variance);
        const Ctx &ct = *ct_ctx->c, &kc = *key_ctx->c;
        require(kc.L >= 2, E_KEYSWITCH_UNSUPPORTED, "KeySwitchingNotSupported: a relinearization key needs two key moduli");
        ksk_validate(ct, kc, ct.L, 0);
        need(out, "out");
        *out = nullptr;
        need(s_ntt, "s_ntt");
        need(seed, "seed");
        set_device(kc);
        hipStream_t s = as_stream(stream);
        WsGuard from(kc.L * kc.n * sizeof(u64), s, true);   // s^2: a secret
        relin_from(ct, kc, s_ntt, from.u(), s);
        keygen_out(ksk_generate(ct, kc, variance, s_ntt, from.u(), seed, 1, seed_out, s), out);
    });
}
fhe_status fhe_bfv_galois_keys_generate_dev(const fhe_ctx *ct_ctx, const fhe_ctx *key_ctx, size_t variance,
                                            const uint64_t *s_ntt, const size_t *exponents, const uint8_t *seeds,
                                            size_t nkeys, uint8_t *seeds_out, void *stream, fhe_ksk **out) {
    return guard([&] {
        keygen_checks(ct_ctx, key_ctx, variance);
        const Ctx &ct = *ct_ctx->c, &kc = *key_ctx->c;
        if (nkeys) need(exponents, "exponents");
        for (size_t i = 0; i < nkeys; i++)
            require((exponents[i] % (2 * ct.n)) & 1, E_INVALID_SUBST, "InvalidSubstitutionExponent");
        const auto dg = ksk_digits(ct, kc);
        ksk_validate(ct, kc, dg.first, dg.second);
        if (!nkeys) return;
        need(out, "out");
        for (size_t i = 0; i < nkeys; i++) out[i] = nullptr;
        need(s_ntt, "s_ntt");
        need(seeds, "seeds");
        set_device(kc);
        hipStream_t s = as_stream(stream);
        std::vector<std::unique_ptr<Ksk>> keys;
        // chunks of 256 keys bound the `from` scratch (the substituted secrets, cleared after use)
        for (size_t b0 = 0; b0 < nkeys; b0 += 256) {
            const size_t nb = std::min<size_t>(256, nkeys - b0);
            WsGuard from(nb * kc.L * kc.n * sizeof(u64), s, true);
            galois_from(ct, kc, s_ntt, exponents + b0, nb, from.u(), s);
            for (auto &k_ : ksk_generate(ct, kc, variance, s_ntt, from.u(), seeds + b0 * 32, nb,
                                         seeds_out ? seeds_out + b0 * 32 : nullptr, s))
                keys.push_back(std::move(k_));
        }
        keygen_out(std::move(keys), out);
    });
}
size_t fhe_ksk_ndigits(const fhe_ksk *ksk) { return ksk ? ksk->k->ndigits : 0; }
fhe_status fhe_ksk_export_dev(const fhe_ksk *ksk, uint64_t *c0, uint64_t *c1, uint64_t *c0_shoup, uint64_t *c1_shoup,
                              void *stream) {
    return guard([&] {
        need(ksk, "ksk");
        need(c0, "c0");
        need(c1, "c1");
        const Ksk &k_ = *ksk->k;
        const Ctx &kc = *k_.ksk_ctx;
        set_device(kc);
        const size_t bytes = k_.ndigits * kc.L * kc.n * sizeof(u64);
        hipStream_t s = as_stream(stream);
        const std::pair<u64 *, const DevBuf<u64> *> parts[] = {{c0, &k_.c0}, {c1, &k_.c1}, {c0_shoup, &k_.c0s},
                                                               {c1_shoup, &k_.c1s}};
        for (const auto &pr : parts)
            if (pr.first) FHE_HIP_CHECK(hipMemcpyAsync(pr.first, pr.second->p, bytes, hipMemcpyDeviceToDevice, s));
    });
}

// ------------------------------------------------------------------- keys on the wire ----
// Device-pointer forms only.  The load call checks its handles, the device and the key's geometry before it looks at a
// buffer; nkeys == 0 is a no-op.  The handles are made all or none, like the generation calls'.
fhe_status fhe_ksk_load_wire_dev(const fhe_ctx *ct_ctx, const fhe_ctx *ksk_ctx, size_t log_base, const uint8_t *c0_bytes,
                                 const uint8_t *c1_bytes, const uint8_t *seeds, size_t nkeys, void *stream, fhe_ksk **out) {
    return guard([&] {
        need(ct_ctx, "ct_ctx");
        need(ksk_ctx, "ksk_ctx");
        const Ctx &ct = *ct_ctx->c, &kc = *ksk_ctx->c;
        kc.need_device();
        ksk_validate(ct, kc, ksk_wire_digits(ct, kc, log_base), log_base);
        if (!nkeys) return;
        need(out, "out");
        for (size_t i = 0; i < nkeys; i++) out[i] = nullptr;
        need(c0_bytes, "c0_bytes");
        require((c1_bytes != nullptr) != (seeds != nullptr), E_ARG, "exactly one of c1_bytes and seeds");
        set_device(kc);
        keygen_out(ksk_load_wire(ct, kc, log_base, c0_bytes, c1_bytes, seeds, nkeys, as_stream(stream)), out);
    });
}
fhe_status fhe_ksk_serialize_dev(const fhe_ksk *ksk, uint8_t *c0_bytes, uint8_t *c1_bytes, void *stream) {
    return guard([&] {
        need(ksk, "ksk");
        need(c0_bytes, "c0_bytes");
        set_device(*ksk->k->ksk_ctx);
        ksk_serialize_wire(*ksk->k, c0_bytes, c1_bytes, as_stream(stream));
    });
}

// --------------------------------------------------------------------- multiparty BFV ----
// Device-pointer forms only, like encryption.  Each checks its handle, the device and the variance before it looks at a
// buffer; batch == 0 is a no-op.
static const Ctx &mbfv_ctx(const fhe_ctx *ctx, size_t variance) {
    need(ctx, "ctx");
    const Ctx &c = *ctx->c;
    c.need_device();
    check_variance(variance);
    return c;
}
static void mbfv_need_rlk(const Ctx &c) {
    require(c.L >= 2, E_KEYSWITCH_UNSUPPORTED, "KeySwitchingNotSupported: a relinearization key needs two moduli");
}
fhe_status fhe_mbfv_pk_share_dev(const fhe_ctx *ctx, size_t variance, const uint64_t *crp, const uint64_t *s_ntt,
                                 int s_shared, const uint8_t *seeds, uint64_t *out, size_t batch, void *stream) {
    return guard([&] {
        const Ctx &c = mbfv_ctx(ctx, variance);
        if (!batch) return;
        need(crp, "crp");
        need(s_ntt, "s_ntt");
        need(seeds, "seeds");
        need(out, "out");
        set_device(c);
        mbfv_pk_share(c, variance, crp, s_ntt, s_shared != 0, seeds, out, batch, as_stream(stream));
    });
}
fhe_status fhe_mbfv_sks_share_dev(const fhe_ctx *ctx, size_t variance, const uint64_t *s_in_ntt,
                                  const uint64_t *s_out_ntt_or_null, int s_shared, const uint64_t *c1, size_t c1_stride,
                                  const uint8_t *seeds, uint64_t *out, size_t batch, void *stream) {
    return guard([&] {
        const Ctx &c = mbfv_ctx(ctx, variance);
        if (!batch) return;
        need(s_in_ntt, "s_in_ntt");
        need(c1, "c1");
        need(seeds, "seeds");
        need(out, "out");
        set_device(c);
        mbfv_sks_share(c, variance, s_in_ntt, s_out_ntt_or_null, s_shared != 0, c1, (u64)c1_stride, seeds, out, batch,
                       as_stream(stream));
    });
}
fhe_status fhe_mbfv_pks_share_dev(const fhe_ctx *ctx, size_t variance, const uint64_t *s_ntt, int s_shared,
                                  const uint64_t *pk, const uint64_t *ct, int ct_shared, const uint8_t *seeds,
                                  uint64_t *out, size_t batch, void *stream) {
    return guard([&] {
        const Ctx &c = mbfv_ctx(ctx, variance);
        if (!batch) return;
        need(s_ntt, "s_ntt");
        need(pk, "pk");
        need(ct, "ct");
        need(seeds, "seeds");
        need(out, "out");
        set_device(c);
        mbfv_pks_share(c, variance, s_ntt, s_shared != 0, pk, ct, ct_shared != 0, seeds, out, batch, as_stream(stream));
    });
}
fhe_status fhe_mbfv_rlk_round1_dev(const fhe_ctx *ctx, size_t variance, const uint64_t *s_ntt, const uint64_t *u_ntt,
                                   int s_shared, const uint64_t *crp, const uint8_t *seeds, uint64_t *out_h0,
                                   uint64_t *out_h1, size_t batch, void *stream) {
    return guard([&] {
        const Ctx &c = mbfv_ctx(ctx, variance);
        mbfv_need_rlk(c);
        if (!batch) return;
        need(s_ntt, "s_ntt");
        need(u_ntt, "u_ntt");
        need(crp, "crp");
        need(seeds, "seeds");
        need(out_h0, "out_h0");
        need(out_h1, "out_h1");
        set_device(c);
        mbfv_rlk_round1(c, variance, s_ntt, u_ntt, s_shared != 0, crp, seeds, out_h0, out_h1, batch, as_stream(stream));
    });
}
fhe_status fhe_mbfv_rlk_round2_dev(const fhe_ctx *ctx, size_t variance, const uint64_t *s_ntt, const uint64_t *u_ntt,
                                   int s_shared, const uint64_t *r1_h0, const uint64_t *r1_h1, const uint8_t *seeds,
                                   uint64_t *out_h0, uint64_t *out_h1, size_t batch, void *stream) {
    return guard([&] {
        const Ctx &c = mbfv_ctx(ctx, variance);
        mbfv_need_rlk(c);
        if (!batch) return;
        need(s_ntt, "s_ntt");
        need(u_ntt, "u_ntt");
        need(r1_h0, "r1_h0");
        need(r1_h1, "r1_h1");
        need(seeds, "seeds");
        need(out_h0, "out_h0");
        need(out_h1, "out_h1");
        set_device(c);
        mbfv_rlk_round2(c, variance, s_ntt, u_ntt, s_shared != 0, r1_h0, r1_h1, seeds, out_h0, out_h1, batch,
                        as_stream(stream));
    });
}
fhe_status fhe_mbfv_aggregate_dev(const fhe_ctx *ctx, const uint64_t *shares, size_t nshares, size_t share_stride,
                                  size_t npolys, const uint64_t *base_or_null, uint64_t *out, void *stream) {
    return guard([&] {
        need(ctx, "ctx");
        const Ctx &c = *ctx->c;
        c.need_device();
        require(nshares >= 1, E_ARG, "NoShares: an aggregation needs at least one share");
        if (!npolys) return;
        need(shares, "shares");
        need(out, "out");
        set_device(c);
        mbfv_sum(c, shares, nshares, (u64)share_stride, npolys, base_or_null, (u64)c.L * c.n, out, as_stream(stream));
    });
}
fhe_status fhe_mbfv_relin_key_aggregate_dev(const fhe_ctx *ctx, const uint64_t *r2_h0, const uint64_t *r2_h1,
                                            size_t nshares, size_t share_stride, const uint64_t *r1_h1, void *stream,
                                            fhe_ksk **out) {
    return guard([&] {
        need(ctx, "ctx");
        need(out, "out");
        *out = nullptr;
        const Ctx &c = *ctx->c;
        c.need_device();
        mbfv_need_rlk(c);
        require(nshares >= 1, E_ARG, "NoShares: an aggregation needs at least one share");
        need(r2_h0, "r2_h0");
        need(r2_h1, "r2_h1");
        need(r1_h1, "r1_h1");
        set_device(c);
        hipStream_t s = as_stream(stream);
        const size_t L = c.L;
        auto h = ksk_new(ctx, ctx, L, r2_h0, r1_h1, 0, out);
        Ksk &k_ = *h->k;
        ksk_alloc(k_);
        u64 *c0 = k_.c0.p;   // the sums go straight into the handle
        mbfv_sum(c, r2_h0, nshares, (u64)share_stride, L, nullptr, 0, c0, s);
        mbfv_sum(c, r2_h1, nshares, (u64)share_stride, L, c0, (u64)L * c.n, c0, s);
        FHE_HIP_CHECK(hipMemcpyAsync(k_.c1.p, r1_h1, L * L * c.n * sizeof(u64), hipMemcpyDeviceToDevice, s));
        ksk_finish(k_, s);
        FHE_HIP_CHECK(hipStreamSynchronize(s));   // (the call waits for `stream`, as fhe_ksk_create_dev does)
        *out = h.release();
    });
}
fhe_status fhe_mbfv_decrypt_dev(const fhe_scaler *sc, uint64_t t, const uint64_t *ct, const uint64_t *shares,
                                size_t nshares, size_t share_stride, uint64_t *out, size_t batch, void *stream) {
    return guard([&] {
        need(sc, "cipher_plain_scaler");
        sc->s->from->need_device();
        require(nshares >= 1, E_ARG, "NoShares: an aggregation needs at least one share");
        if (!batch) return;
        need(ct, "ct");
        need(shares, "shares");
        need(out, "out");
        set_device(*sc->s->from);
        mbfv_decrypt(*sc->s, t, ct, shares, nshares, (u64)share_stride, out, batch, as_stream(stream));
    });
}

// --------------------------------------------------------------------------- primes ----
uint64_t fhe_generate_prime(size_t num_bits, uint64_t modulo, uint64_t upper_bound) {
    return generate_prime(num_bits, modulo, upper_bound);
}
int fhe_supports_opt(uint64_t p) { return supports_opt(p) ? 1 : 0; }
int fhe_is_prime(uint64_t p) { return is_prime_u64(p) ? 1 : 0; }
fhe_status fhe_generate_moduli(const size_t *sizes, size_t count, size_t degree, uint64_t *out) {
    return guard([&] {
        need(sizes, "sizes");
        need(out, "out");
        std::vector<size_t> sz(sizes, sizes + count);
        auto m = generate_moduli(sz, degree);
        std::copy(m.begin(), m.end(), out);
    });
}

// ---------------------------------------------------------------------- bench / test ----
fhe_status fhe_synth_uniform_dev(const fhe_ctx *ctx, uint64_t seed, uint64_t ct0, uint64_t part0, size_t nparts,
                                 uint64_t *out, size_t batch, void *stream) {
    return guard([&] {
        need(ctx, "ctx");
        const Ctx &c = *ctx->c;
        c.need_device();
        set_device(c);
        const u64 total = (u64)batch * nparts * c.L * c.n;
        if (!total) return;
        need(out, "out");
        launch_ew<k::synth_kernel>("synth", total, as_stream(stream), out, c.dmods(), (uint32_t)c.L, (uint32_t)c.logn,
                                   (uint32_t)nparts, seed, ct0, part0, total);
    });
}
size_t fhe_workspace_trim(void) {
    AuxStreams::get().drop(-1, nullptr, true);   // internal streams, their blocks and the pooled events go too
    const size_t freed = Workspace::get().trim();
    DevPools::get().trim();                      // what the private pools kept (scratch blocks, fhe_buf_alloc_async)
    return freed;
}
fhe_status fhe_workspace_set_limit(size_t per_stream_bytes, size_t total_bytes) {
    return guard([&] { Workspace::get().set_limits(per_stream_bytes, total_bytes); });
}
fhe_status fhe_workspace_get_limit(size_t *per_stream_bytes, size_t *total_bytes) {
    return guard([&] { Workspace::get().get_limits(per_stream_bytes, total_bytes); });
}
fhe_status fhe_workspace_stats(size_t *held_bytes, size_t *in_use_bytes, size_t *blocks, size_t *owners,
                               size_t *internal_streams) {
    return guard([&] {
        Workspace::get().stats(held_bytes, in_use_bytes, blocks, owners);
        if (internal_streams) *internal_streams = AuxStreams::get().count();
    });
}
fhe_status fhe_workspace_pool_stats(int device, size_t *scratch_reserved_bytes, size_t *scratch_used_bytes,
                                    size_t *buffers_reserved_bytes, size_t *buffers_used_bytes) {
    return guard([&] {
        size_t v[4] = {0, 0, 0, 0};
        DevPools::get().stats(device, v);
        if (scratch_reserved_bytes) *scratch_reserved_bytes = v[0];
        if (scratch_used_bytes) *scratch_used_bytes = v[1];
        if (buffers_reserved_bytes) *buffers_reserved_bytes = v[2];
        if (buffers_used_bytes) *buffers_used_bytes = v[3];
    });
}
fhe_status fhe_ubench_int(int device, int which, double min_seconds, double *ops_per_s) {
    return guard([&] {
        need(ops_per_s, "ops_per_s");
        *ops_per_s = 0;
        int ndev = 0;
        FHE_HIP_CHECK(hipGetDeviceCount(&ndev));
        require(device >= 0 && device < ndev, E_NO_DEVICE, "no such HIP device");
        *ops_per_s = ub::run(device, which, min_seconds);
    });
}
fhe_status fhe_ubench_scaler(const fhe_scaler *scaler, double min_seconds, double *columns_per_s) {
    return guard([&] {
        need(scaler, "scaler");
        need(columns_per_s, "columns_per_s");
        *columns_per_s = ub::run_scaler(*scaler->s, min_seconds);
    });
}
fhe_status fhe_ubench_copy(int device, size_t bytes, double min_seconds, double *bytes_per_s) {
    return guard([&] {
        need(bytes_per_s, "bytes_per_s");
        *bytes_per_s = 0;
        int ndev = 0;
        FHE_HIP_CHECK(hipGetDeviceCount(&ndev));
        require(device >= 0 && device < ndev, E_NO_DEVICE, "no such HIP device");
        *bytes_per_s = ub::run_copy(device, bytes, min_seconds);
    });
}
void fhe_engine_set_f64(int on) { f64_enabled_flag().store(on != 0, std::memory_order_relaxed); }
int fhe_engine_get_f64(void) { return f64_enabled_flag().load(std::memory_order_relaxed) ? 1 : 0; }
void fhe_prof_enable(int on) { Profiler::get().enabled = on != 0; }
void fhe_prof_reset(void) {
    try {
        Profiler::get().reset();
    } catch (...) {
    }
}
size_t fhe_prof_count(void) {
    try {
        Profiler::get().drain();
    } catch (...) {
    }
    return Profiler::get().entries.size();
}
fhe_status fhe_prof_get(size_t index, char *name, size_t name_cap, uint64_t *launches, double *total_ms) {
    return guard([&] {
        Profiler &p = Profiler::get();
        p.drain();
        if (index >= p.entries.size()) throw StatusError(FHE_E_ARG, "profile index out of range");
        const auto &e = p.entries[index];
        if (name && name_cap) std::snprintf(name, name_cap, "%s", e.name.c_str());
        if (launches) *launches = e.launches;
        if (total_ms) *total_ms = e.ms;
    });
}
fhe_status fhe_prof_get_symbol(size_t index, char *symbol, size_t symbol_cap) {
    return guard([&] {
        Profiler &p = Profiler::get();
        std::lock_guard<std::mutex> lk(p.mu);
        if (index >= p.entries.size()) throw StatusError(FHE_E_ARG, "profile index out of range");
        if (!symbol || !symbol_cap) throw StatusError(FHE_E_ARG, "symbol buffer is null");
        const auto &e = p.entries[index];
        const char *mangled = e.fn ? hipKernelNameRefByPtr(e.fn, nullptr) : nullptr;
        std::string text = e.name;                     // (no symbol known to the runtime: the label)
        if (mangled && *mangled) {
            int st = 0;
            char *dm = abi::__cxa_demangle(mangled, nullptr, nullptr, &st);
            text = (st == 0 && dm) ? dm : mangled;
            std::free(dm);
        }
        std::snprintf(symbol, symbol_cap, "%s", text.c_str());
    });
}

}  // extern "C"
