// engine.hpp -- host runtime above the kernels: handles (contexts, scalers, keys,
// multiplicators, parameter sets), stream-ordered workspace, launch geometry and the batched
// pipelines (Scaler::scale, key switch, relinearise, rotate, modulus switch, ct x ct).
// C++ because the reference's host is compiled code (Rust) and no Rust toolchain exists in
// this image; the C ABI in fhe_hip.cpp is a thin layer over these classes.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "hostmath.hpp"
#include "kernels.hpp"

namespace fhe {

// ------------------------------------------------------------------ error plumbing ----
enum : int {
    E_OK = 0, E_ARG = -1, E_HIP = -2, E_INVALID_MODULUS = -3, E_INVALID_DEGREE = -4, E_NTT_UNAVAILABLE = -5,
    E_CONTEXT_MISMATCH = -6, E_DEGREE_MISMATCH = -7, E_NO_MORE_CONTEXT = -8, E_CONTEXT_NOT_REACHABLE = -9,
    E_INVALID_SUBST = -10, E_PARAMETER_MISMATCH = -11, E_INVALID_LEVEL = -12, E_MUL_POLY_COUNT = -13,
    E_EMPTY_MODULI = -14, E_NON_COPRIME = -15, E_NOT_ENOUGH_PRIMES = -16, E_KEYSWITCH_UNSUPPORTED = -17,
    E_NO_DEVICE = -18, E_EMPTY_DOT = -19, E_EXPANSION_SIZE = -20, E_EXPANSION_UNSUPPORTED = -21,
    E_SIMD_UNAVAILABLE = -22, E_TOO_MANY_VALUES = -23, E_INVALID_VARIANCE = -24
};

#define FHE_HIP_CHECK(expr)                                                                        \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            throw StatusError(E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));           \
    } while (0)

inline void require(bool cond, int code, const char *msg) {
    if (!cond) throw StatusError(code, msg);
}

// The F64 kernels for moduli below 2^50 (round 6) are the product default.  fhe_engine_set_f64(0) sends every launch to
// the integer kernels instead -- an execution option like fhe_ksk_set_mode (same results either way; tests run both, A/B
// timings flip it inside one process).  Read once per launch.
inline std::atomic<bool> &f64_enabled_flag() {
    static std::atomic<bool> on{true};
    return on;
}
inline bool f64_disabled() { return !f64_enabled_flag().load(std::memory_order_relaxed); }
// compute units of a device (persistent launches size their grids with it)
inline int device_cus(int device) {
#if defined(FHE_HOST_EMULATION)
    (void)device;
    return 3;   // (few, so that the emulated suite runs several items through one workgroup)
#else
    static std::mutex mu;
    static std::vector<int> cache;
    std::lock_guard<std::mutex> g(mu);
    if (device < 0) return 1;
    if ((size_t)device >= cache.size()) cache.resize((size_t)device + 1, 0);
    if (!cache[(size_t)device]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n <= 0) n = 256;
        cache[(size_t)device] = n;
    }
    return cache[(size_t)device];
#endif
}

// ------------------------------------------------------------------------ profiling ----
// Optional per-kernel timing with HIP events recorded on the launching stream
// (bench.py reads these to compute the dominant kernel's achieved bytes/s live).
class Profiler {
public:
    static Profiler &get() {
        static Profiler p;
        return p;
    }
    bool enabled = false;
    // launches of THIS thread that must not be recorded (the microbenchmarks time themselves): a per-thread count, so a
    // thread profiling real work at the same time loses nothing (ubench used to flip `enabled` for everyone)
    static int &suppressed() {
        static thread_local int n = 0;
        return n;
    }
    struct Suppress {
        Suppress() { ++suppressed(); }
        ~Suppress() { --suppressed(); }
    };
    struct Pending {
        int id;
        hipEvent_t a, b;
    };
    // One entry per (label, kernel symbol): two instantiations of one template launched under one label -- the wide and
    // the narrow ntt_kernel<false, 13, ...> behind "ntt_fwd" -- stay apart, as rocprofv3 keeps them apart (VERDICT r05:
    // the label-keyed table named the wrong dominant kernel).  fhe_prof_get reports (label, launches, ms) per entry,
    // fhe_prof_get_symbol the kernel's demangled symbol; callers that want families sum the entries of a label.
    struct Entry {
        std::string name;
        const void *fn = nullptr;
        uint64_t launches = 0;
        double ms = 0;
    };
    int id_of(const char *name, const void *fn) {
        for (size_t i = 0; i < entries.size(); i++)
            if (entries[i].fn == fn && entries[i].name == name) return (int)i;
        entries.push_back(Entry{name, fn, 0, 0});
        return (int)entries.size() - 1;
    }
    hipEvent_t take_event() {
        if (!pool.empty()) {
            hipEvent_t e = pool.back();
            pool.pop_back();
            return e;
        }
        hipEvent_t e;
        FHE_HIP_CHECK(hipEventCreate(&e));
        return e;
    }
    // The two events of a launch travel WITH it (hipExtLaunchKernelGGL stamps them from the dispatch itself) instead
    // of being recorded around it: the interval is the kernel's own duration, and the stream carries no extra
    // barrier packets -- round 3: the record-around form cost the timed region of bench.py 2.4-3.5 %.
    Pending &begin(const char *name, const void *fn) {
        cur = Pending{id_of(name, fn), take_event(), take_event()};
        return cur;
    }
    void end() { pending.push_back(cur); }
    void drain() {
        for (auto &p : pending) {
            FHE_HIP_CHECK(hipEventSynchronize(p.b));
            float ms = 0;
            FHE_HIP_CHECK(hipEventElapsedTime(&ms, p.a, p.b));
            entries[p.id].launches++;
            entries[p.id].ms += ms;
            pool.push_back(p.a);
            pool.push_back(p.b);
        }
        pending.clear();
    }
    void reset() {
        drain();
        entries.clear();
    }
    std::vector<Entry> entries;
    std::mutex mu;

private:
    Pending cur{};
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;
};

#define FHE_LAUNCH(name, kernel, grid, block, smem, stream, ...)                         \
    do {                                                                                 \
        Profiler &_pf = Profiler::get();                                                 \
        if (_pf.enabled && !Profiler::suppressed()) {                                    \
            std::lock_guard<std::mutex> _lk(_pf.mu);                                     \
            auto &_ev = _pf.begin(name, reinterpret_cast<const void *>(kernel));         \
            hipExtLaunchKernelGGL(kernel, grid, block, smem, stream, _ev.a, _ev.b, 0, __VA_ARGS__); \
            _pf.end();                                                                   \
        } else {                                                                         \
            hipLaunchKernelGGL(kernel, grid, block, smem, stream, __VA_ARGS__);          \
        }                                                                                \
        FHE_HIP_CHECK(hipGetLastError());                                                \
    } while (0)

// --------------------------------------------------------------- device allocations ----
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t count = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
        count = 0;
    }
    void alloc(size_t n) {
        reset();
        if (n) FHE_HIP_CHECK(hipMalloc((void **)&p, n * sizeof(T)));
        count = n;
    }
    void upload(const std::vector<T> &h) {
        alloc(h.size());
        if (!h.empty()) FHE_HIP_CHECK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    }
};

// Two PRIVATE stream-ordered memory pools per device (hipMemPoolCreate): SCRATCH serves the engine's workspace blocks,
// BUFFERS the ABI's fhe_buf_alloc_async.  (Round 3 raised the release threshold of the device's DEFAULT pool instead, which
// changed the behaviour of every other hipMallocAsync user in the process.)
// Round 5: the scratch pool's release threshold IS the workspace's total limit -- what the engine evicts
// goes back to the driver (hipMemPoolTrimTo right after an eviction, and the threshold at the next synchronisation for
// blocks whose stream-ordered free had not retired yet), so fhe_workspace_set_limit bounds the device memory the process
// holds for scratch, not only the bookkeeping.  The buffers pool keeps what is freed into it (a host that allocates and
// drops a result per call must not pay the driver for it each time) until fhe_workspace_trim.
class DevPools {
public:
    enum Kind : int { SCRATCH = 0, BUFFERS = 1 };
    static DevPools &get() {
        static DevPools p;
        return p;
    }
    hipMemPool_t pool(int device, Kind kind) {
        std::lock_guard<std::mutex> g(mu);
        return pool_locked(device, kind);
    }
    void *alloc(int device, size_t bytes, hipStream_t s, Kind kind) {
        void *p = nullptr;
        FHE_HIP_CHECK(hipMallocFromPoolAsync(&p, bytes ? bytes : 8, pool(device, kind), s));
        return p;
    }
    // bytes of reserved scratch the pools may keep once it is idle (0 = everything): Workspace's total limit
    void set_scratch_threshold(int device, size_t bytes) {
        std::lock_guard<std::mutex> g(mu);
        if ((size_t)device >= thresholds.size()) thresholds.resize((size_t)device + 1, ~0ull);
        const uint64_t keep = bytes ? (uint64_t)bytes : ~0ull;
        if (thresholds[(size_t)device] == keep && (size_t)(2 * device) < pools.size() && pools[(size_t)(2 * device)]) return;
        thresholds[(size_t)device] = keep;
        hipMemPool_t mp = pool_locked(device, SCRATCH);
        uint64_t v = keep;
        (void)hipMemPoolSetAttribute(mp, hipMemPoolAttrReleaseThreshold, &v);
    }
    // hands idle scratch beyond `keep` bytes back to the driver now -- when the pool holds more than `slack` bytes over
    // it (a working set sitting AT the limit must not free to the driver and re-map on every call; the
    // pool's release threshold takes care of the rest at the next synchronisation)
    void trim_scratch_to(int device, size_t keep, size_t slack = 0) {
        std::lock_guard<std::mutex> g(mu);
        const size_t i = (size_t)(2 * device + SCRATCH);
        if (i >= pools.size() || !pools[i]) return;
        if (slack) {
            uint64_t reserved = 0;
            if (hipMemPoolGetAttribute(pools[i], hipMemPoolAttrReservedMemCurrent, &reserved) == hipSuccess &&
                reserved <= (uint64_t)keep + slack)
                return;
        }
        (void)hipMemPoolTrimTo(pools[i], keep);
    }
    // hands the pools' idle memory back to the driver
    void trim() {
        std::lock_guard<std::mutex> g(mu);
        for (hipMemPool_t mp : pools)
            if (mp) (void)hipMemPoolTrimTo(mp, 0);
    }
    // what the driver says the pools hold: reserved (backed by device memory) and used (handed out) bytes
    void stats(int device, size_t out[4]) {
        std::lock_guard<std::mutex> g(mu);
        for (int k = 0; k < 2; k++) {
            uint64_t r = 0, u = 0;
            const size_t i = (size_t)(2 * device + k);
            if (device >= 0 && i < pools.size() && pools[i]) {
                (void)hipMemPoolGetAttribute(pools[i], hipMemPoolAttrReservedMemCurrent, &r);
                (void)hipMemPoolGetAttribute(pools[i], hipMemPoolAttrUsedMemCurrent, &u);
            }
            out[2 * k] = (size_t)r;
            out[2 * k + 1] = (size_t)u;
        }
    }

private:
    hipMemPool_t pool_locked(int device, Kind kind) {
        const size_t i = (size_t)(2 * device + (int)kind);
        if (i >= pools.size()) pools.resize(i + 1, nullptr);
        if (!pools[i]) {
            hipMemPoolProps props;
            std::memset(&props, 0, sizeof(props));
            props.allocType = hipMemAllocationTypePinned;
            props.location.type = hipMemLocationTypeDevice;
            props.location.id = device;
            hipMemPool_t mp = nullptr;
            FHE_HIP_CHECK(hipMemPoolCreate(&mp, &props));
            uint64_t keep = ~0ull;
            if (kind == SCRATCH && (size_t)device < thresholds.size()) keep = thresholds[(size_t)device];
            FHE_HIP_CHECK(hipMemPoolSetAttribute(mp, hipMemPoolAttrReleaseThreshold, &keep));
            pools[i] = mp;
        }
        return pools[i];
    }
    std::mutex mu;
    std::vector<hipMemPool_t> pools;        // [2 * device + kind]
    std::vector<uint64_t> thresholds;       // scratch release threshold per device
};

// Scratch blocks, reused in stream order: a block released by stream S is handed out again only to work enqueued on
// S, so there is no cross-stream hazard and no allocation per call.  Round 4: bounded.
//  * Blocks come from the device's private stream-ordered pool (DevPools).  A stream's own too-small blocks go back to
//    it in stream order (hipFreeAsync on the acquiring stream, which is alive by construction), so growing a stream's
//    block no longer synchronises the device.
//  * Limits (fhe_workspace_set_limit): `per_stream` and `total` bound the bytes the engine RETAINS -- idle blocks
//    beyond them are evicted least-recently-used first, on release and before growing.  Blocks in use are never
//    refused: a call that needs more than the limit still runs, its blocks just are not kept afterwards.  Blocks of
//    OTHER streams are evicted with hipFree (it waits for the device): the engine cannot know whether their stream still
//    exists -- a host that makes and destroys its own HIP streams never says so, and this runtime's hipStreamQuery
//    dereferences a destroyed handle (segmentation fault, tools/probe/hip_pool_probe.cpp) -- and hipFree is correct
//    either way.  That is also what bounds such a host: dead streams' blocks are simply the least recently used.
//    Default: no per-stream bound, total = a quarter of the device's memory (at least 8 GiB); 0 = unbounded.
//    `total` is PER DEVICE (round 5, ADVICE r04: it used to be one sum over all devices with a default taken from
//    whichever device was current first, so an in-process multi-GPU host evicted other devices' blocks -- hipSetDevice +
//    hipFree under the global mutex -- in steady state): each device's blocks are counted and evicted against its own
//    bound, and the default is a quarter of THAT device's memory.  What is evicted also leaves the scratch pool
//    (DevPools above): the bound holds for the device memory the process keeps, not just for this table.
//  * A recycled handle value that inherits an old block is harmless: the block was idle, and whatever ran on the old
//    stream is ordered before the new owner's work by the device itself (same queue slot) or long finished.
class Workspace {
public:
    static Workspace &get() {
        static Workspace w;
        return w;
    }
    void *acquire(size_t bytes, hipStream_t s);
    void release(void *p) {
        std::unique_lock<std::mutex> lk(mu);
        hipStream_t owner = nullptr;
        int dev = -1;
        for (auto &b : blocks)
            if (b.ptr == p) {
                b.in_use = false;
                b.last_use = ++tick;
                owner = b.stream;
                dev = b.device;
            }
        // (the releasing call ran on `owner`, which therefore exists: its blocks may go back in stream order)
        enforce_limits_locked(owner, dev, 0);
        flush_trims(lk);
    }
    // A stream is about to be destroyed: its idle blocks can never be handed out again.
    void drop_stream(hipStream_t s) {
        std::lock_guard<std::mutex> lk(mu);
        drop_stream_locked(s, true);
    }
    // Frees every idle block (all devices); returns the number of bytes released.
    size_t trim() {
        std::lock_guard<std::mutex> lk(mu);
        int cur = 0;
        (void)hipGetDevice(&cur);
        size_t freed = 0;
        for (auto &b : blocks)
            if (!b.in_use && b.ptr) {
                (void)hipSetDevice(b.device);
                (void)hipFree(b.ptr);   // (waits for the device: whatever still read the block is done)
                freed += b.bytes;
                b.ptr = nullptr;
            }
        (void)hipSetDevice(cur);
        compact_locked();
        return freed;
    }
    static constexpr size_t LIMIT_DEFAULT = ~(size_t)0;   // "a quarter of the device's memory, at least 8 GiB"
    void set_limits(size_t per_stream, size_t total) {
        std::unique_lock<std::mutex> lk(mu);
        limit_stream = per_stream;
        limit_total = total;
        thresholds_set.clear();   // (every device's scratch pool learns the new bound at its next use)
        for (auto &b : blocks) sync_threshold_locked(b.device);
        enforce_limits_locked(nullptr, -1, 0);
        for (auto &t : deferred_trims) t.slack = 0;   // (a new bound is applied to the letter, now)
        flush_trims(lk);
    }
    void get_limits(size_t *per_stream, size_t *total) {
        std::lock_guard<std::mutex> lk(mu);
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (per_stream) *per_stream = limit_stream;
        if (total) *total = total_limit_locked(dev);
    }
    // bytes held (idle + in use), bytes in use, number of blocks, number of distinct (device, stream) owners
    void stats(size_t *held, size_t *in_use, size_t *nblocks, size_t *nstreams) {
        std::lock_guard<std::mutex> lk(mu);
        size_t h = 0, u = 0;
        std::vector<std::pair<int, hipStream_t>> owners;
        for (auto &b : blocks) {
            h += b.bytes;
            if (b.in_use) u += b.bytes;
            if (std::find(owners.begin(), owners.end(), std::make_pair(b.device, b.stream)) == owners.end())
                owners.emplace_back(b.device, b.stream);
        }
        if (held) *held = h;
        if (in_use) *in_use = u;
        if (nblocks) *nblocks = blocks.size();
        if (nstreams) *nstreams = owners.size();
    }
    // (AuxStreams tells the pool which of its keys are not real streams, and which internal streams it destroyed)
    void drop_internal_stream(hipStream_t aux) {
        std::lock_guard<std::mutex> lk(mu);
        drop_stream_locked(aux, true);
    }

private:
    struct Block {
        void *ptr = nullptr;
        size_t bytes = 0;
        hipStream_t stream = nullptr;
        int device = 0;
        bool in_use = false;
        uint64_t last_use = 0;
    };
    std::vector<Block> blocks;
    std::mutex mu;
    uint64_t tick = 0;
    size_t limit_stream = 0, limit_total = LIMIT_DEFAULT;
    std::vector<size_t> default_total;   // per device, resolved on first use
    std::vector<char> thresholds_set;    // per device: the scratch pool has been told the current bound

    size_t total_limit_locked(int dev) {
        if (limit_total != LIMIT_DEFAULT) return limit_total;
        if (dev < 0) dev = 0;
        if ((size_t)dev >= default_total.size()) default_total.resize((size_t)dev + 1, 0);
        if (!default_total[(size_t)dev]) {
            size_t total_b = 0;
            if (hipDeviceTotalMem(&total_b, dev) != hipSuccess || !total_b) total_b = (size_t)32 << 30;
            default_total[(size_t)dev] = std::max<size_t>((size_t)8 << 30, total_b / 4);
        }
        return default_total[(size_t)dev];
    }
    void sync_threshold_locked(int dev) {
        if (dev < 0) return;
        if ((size_t)dev >= thresholds_set.size()) thresholds_set.resize((size_t)dev + 1, 0);
        if (thresholds_set[(size_t)dev]) return;
        DevPools::get().set_scratch_threshold(dev, total_limit_locked(dev));
        thresholds_set[(size_t)dev] = 1;
    }
    void compact_locked() {
        blocks.erase(std::remove_if(blocks.begin(), blocks.end(), [](const Block &b) { return !b.ptr; }), blocks.end());
    }
    // frees one idle block: stream-ordered on its own stream when that stream is known to be alive, else hipFree
    void free_block_locked(Block &b, bool owner_alive) {
        int cur = 0;
        (void)hipGetDevice(&cur);
        if (cur != b.device) (void)hipSetDevice(b.device);
        if (!owner_alive || hipFreeAsync(b.ptr, b.stream) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(b.ptr);
        }
        if (cur != b.device) (void)hipSetDevice(cur);
        b.ptr = nullptr;
        b.bytes = 0;
    }
    void drop_stream_locked(hipStream_t s, bool owner_alive) {
        for (auto &b : blocks)
            if (!b.in_use && b.ptr && b.stream == s) free_block_locked(b, owner_alive);
        compact_locked();
    }
    // Evicts idle blocks, least recently used first, until the retained bytes respect the limits; `extra` bytes on
    // (`dev`, `s`) are about to be added (acquire) and count against both.  Only blocks of (`dev`, `s`) -- the stream
    // the current call runs on -- are returned in stream order; every other owner's go through hipFree.
    void enforce_limits_locked(hipStream_t s, int dev, size_t extra) {
        if (!limit_stream && limit_total == 0) return;
        std::vector<int> trimmed;
        for (;;) {
            // per device: the device whose retained bytes exceed its bound gives up its least recently used idle block
            Block *victim = nullptr;
            std::vector<int> devs;
            for (auto &b : blocks)
                if (std::find(devs.begin(), devs.end(), b.device) == devs.end()) devs.push_back(b.device);
            if (dev >= 0 && std::find(devs.begin(), devs.end(), dev) == devs.end()) devs.push_back(dev);
            for (int d : devs) {
                const size_t lim_total = total_limit_locked(d);
                if (!lim_total) continue;
                size_t total = d == dev ? extra : 0;
                for (auto &b : blocks)
                    if (b.device == d) total += b.bytes;
                if (total <= lim_total) continue;
                for (auto &b : blocks)
                    if (b.device == d && !b.in_use && b.ptr && (!victim || b.last_use < victim->last_use)) victim = &b;
                if (victim) break;
            }
            if (!victim && limit_stream) {
                // any (device, stream) owner over its own limit gives up its oldest idle block
                for (auto &b : blocks) {
                    if (b.in_use || !b.ptr) continue;
                    size_t own = (dev >= 0 && b.device == dev && b.stream == s) ? extra : 0;
                    for (auto &o : blocks)
                        if (o.device == b.device && o.stream == b.stream) own += o.bytes;
                    if (own > limit_stream && (!victim || b.last_use < victim->last_use)) victim = &b;
                }
            }
            if (!victim) break;
            const int vdev = victim->device;
            free_block_locked(*victim, dev >= 0 && victim->device == dev && victim->stream == s);
            compact_locked();
            if (std::find(trimmed.begin(), trimmed.end(), vdev) == trimmed.end()) trimmed.push_back(vdev);
        }
        // what was evicted leaves the scratch pool too (blocks whose stream-ordered free has not retired yet follow at the
        // next synchronisation: the pool's release threshold is this bound).  The driver call happens in flush_trims, after
        // the table's mutex is dropped, and only when the pool holds more than an eighth of the bound over what is kept
        // (hipMemPoolTrimTo under the global mutex after every eviction serialised every thread and device
        // behind an unmap, and a working set at the limit paid unmap + map per call).
        for (int d : trimmed) {
            size_t keep = d == dev ? extra : 0;
            for (auto &b : blocks)
                if (b.device == d) keep += b.bytes;
            deferred_trims.push_back(Trim{d, keep, total_limit_locked(d) / 8});
        }
    }
    struct Trim {
        int device;
        size_t keep, slack;
    };
    std::vector<Trim> deferred_trims;
    void flush_trims(std::unique_lock<std::mutex> &lk) {
        if (deferred_trims.empty()) return;
        std::vector<Trim> todo;
        todo.swap(deferred_trims);
        lk.unlock();
        for (const Trim &t : todo) DevPools::get().trim_scratch_to(t.device, t.keep, t.slack);
    }
};
// `wipe`: the block held secret-dependent data (decryption intermediates, which the reference keeps in
// Zeroizing buffers, F/bfv/keys/secret_key.rs:198-226): it is cleared on its stream before it returns to the pool.
struct WsGuard {
    void *p;
    size_t bytes;
    hipStream_t stream;
    bool wipe;
    WsGuard(size_t bytes_, hipStream_t s, bool wipe_ = false)
        : p(Workspace::get().acquire(bytes_, s)), bytes(bytes_), stream(s), wipe(wipe_) {}
    ~WsGuard() {
        if (wipe && bytes) (void)hipMemsetAsync(p, 0, bytes, stream);
        Workspace::get().release(p);
    }
    u64 *u() const { return (u64 *)p; }
};

// ---------------------------------------------------------------------- rq::Context ----
struct Ctx {
    int device = -1;
    size_t n = 0, logn = 0, L = 0;
    std::vector<u64> moduli;
    const Ctx *root = nullptr;  // owner of the tables (children are moduli prefixes of it)
    // host tables (root only)
    std::vector<NttTables> tabs;
    std::vector<ModConsts> mods;
    // one 64-bit fingerprint per modulus over the four NTT tables and N^-1 (root only): two contexts agree on the
    // evaluation order of a shared modulus -- and may exchange Ntt-form rows -- exactly when these are equal
    std::vector<u64> tab_fp;
    // per-context
    std::vector<u64> inv_last, inv_last_shoup;  // M/rq/context.rs:66-73
    std::unique_ptr<Ctx> next;                  // next_context
    // device tables (owned by root; children alias them)
    DevBuf<DevMod> d_mods;
    DevBuf<k::u64x2> d_tw, d_itw, d_ninv, d_inv_last, d_pow2;
    // Round 6: the F64 twins of d_tw / d_itw / d_ninv -- {w, w / p} as doubles, same indexing -- for the rows whose
    // modulus is below 2^50 (zq_f64.hpp; rows of wider moduli are left zero and never read: a launch takes the F64
    // kernels only when every one of its rows qualifies, f64_class below).  Empty when no modulus qualifies.
    DevBuf<k::u64x2> d_tw_f, d_itw_f, d_ninv_f;
    // The lift's public constants (kernels_noise.hpp: q_i, M_i, q_j^-1 mod q_i with Shoup twins, the limbs of q), per
    // context -- levels included --, built by the first call that needs them (lift_consts below): handles are shared by
    // concurrent callers, hence the once_flag.
    mutable std::once_flag lift_once;
    mutable DevBuf<u64> d_lift;
    size_t lift_w = 0;   // W = ceil(bitlen(q) / 64), q the product of the moduli (set at creation, host-only handles too)

    const k::u64x2 *dtw_f() const { return root->d_tw_f.p; }
    const k::u64x2 *ditw_f() const { return root->d_itw_f.p; }
    const k::u64x2 *dninv_f() const { return root->d_ninv_f.p; }
    // The F64 class HR of the moduli [first, first + rows) of the ROOT's list: 5 when all are below 2^48, 4 below 2^49,
    // 3 below 2^50, 0 when one of them is wider (integer kernels).  The kernels are instantiated for these three.
    int f64_class(size_t first, size_t rows) const {
        if (!root->d_tw_f.p || rows == 0 || f64_disabled()) return 0;
        u64 mx = 0;
        for (size_t i = first; i < first + rows; i++) mx = std::max(mx, root->moduli[i]);
        if (mx >> 50) return 0;
        return (mx >> 49) ? 3 : (mx >> 48) ? 4 : 5;
    }
    // The F64 class of those rows for a launch on whole-row tiles (4096 ... 16384 points: the sizes the F64 instances
    // exist for), 0 otherwise.  `f64_on`: a caller's own reading of the switch, taken once for all launches of a call.
    int f64_rows(size_t first, size_t rows, bool f64_on = true) const {
        return f64_on && logn >= 12 && logn <= 14 ? f64_class(first, rows) : 0;
    }
    // every modulus [first, first + rows) of the ROOT's list below 2^60: the narrow passes apply
    bool below_2p60(size_t first, size_t rows) const {
        for (size_t i = first; i < first + rows; i++)
            if (root->moduli[i] >> 60) return false;
        return true;
    }
    const DevMod *dmods() const { return root->d_mods.p; }
    const k::u64x2 *dtw() const { return root->d_tw.p; }
    const k::u64x2 *ditw() const { return root->d_itw.p; }
    const k::u64x2 *dninv() const { return root->d_ninv.p; }
    const k::u64x2 *dpow2() const { return root->d_pow2.p; }
    const NttTables &tab(size_t i) const { return root->tabs[i]; }
    // Do the first `rows` moduli of this context and of `o` use the same NTT tables?  (Handles built from different
    // table sources -- the engine's own psi, fhe_ctx_create with host tables, fhe_params_create_with_tables -- can
    // share moduli and still disagree on the evaluation order; Ntt-form rows then must not cross between them.)
    bool same_tables(const Ctx &o, size_t rows) const {
        if (rows > L || rows > o.L) return false;
        for (size_t i = 0; i < rows; i++)
            if (moduli[i] != o.moduli[i] || root->tab_fp[i] != o.root->tab_fp[i]) return false;
        return true;
    }
    size_t poly_elems() const { return L * n; }
    void need_device() const { require(device >= 0, E_NO_DEVICE, "handle was created host-only (device = -1)"); }
    bool same_ring(const Ctx &o) const { return n == o.n && moduli == o.moduli; }
    const Ctx *at_level(size_t i) const {
        const Ctx *c = this;
        for (size_t k = 0; k < i; k++) {
            if (!c->next) return nullptr;
            c = c->next.get();
        }
        return c;
    }
    // Context::niterations_to (M/rq/context.rs:117-141); -1 if unreachable
    long niterations_to(const Ctx &to) const {
        long it = 0;
        for (const Ctx *c = this; c; c = c->next.get(), it++)
            if (c->same_ring(to)) return it;
        return -1;
    }
};

inline void ctx_fill_inv_last(Ctx &c) {
    BigUint q(1);
    for (u64 m : c.moduli) q = q * BigUint(m);
    c.lift_w = (q.bits() + 63) / 64;
    c.inv_last.clear();
    c.inv_last_shoup.clear();
    const u64 q_last = c.moduli.back();
    for (size_t i = 0; i + 1 < c.L; i++) {
        const u64 qi = c.moduli[i];
        const u64 inv = powmod(q_last % qi, qi - 2, qi);
        c.inv_last.push_back(inv);
        c.inv_last_shoup.push_back(shoup(inv, qi));
    }
    if (c.device >= 0) {
        std::vector<k::u64x2> h(std::max<size_t>(c.L - 1, 1), k::u64x2{0, 0});
        for (size_t i = 0; i + 1 < c.L; i++) h[i] = k::u64x2{c.inv_last[i], c.inv_last_shoup[i]};
        c.d_inv_last.upload(h);
    }
}

inline std::unique_ptr<Ctx> ctx_create(int device, size_t degree, const std::vector<u64> &moduli,
                                       const u64 *omegas, const u64 *omegas_shoup, const u64 *zetas_inv,
                                       const u64 *zetas_inv_shoup, const u64 *size_inv,
                                       const u64 *size_inv_shoup) {
    require(degree >= 8 && (degree & (degree - 1)) == 0 && degree <= 65536, E_INVALID_DEGREE,
            "InvalidPolynomialDegree: degree must be a power of two in [8, 65536]");
    RnsContext rns_check(moduli);  // EmptyModuli / NonCoprimeModuli / InvalidModulus
    auto c = std::make_unique<Ctx>();
    c->device = device;
    c->n = degree;
    while (((size_t)1 << c->logn) < degree) c->logn++;
    c->L = moduli.size();
    c->moduli = moduli;
    c->root = c.get();
    const bool have_tables = omegas != nullptr;
    if (have_tables)
        require(omegas_shoup && zetas_inv && zetas_inv_shoup && size_inv && size_inv_shoup, E_ARG,
                "either all six NTT tables or none must be supplied");
    for (size_t i = 0; i < c->L; i++) {
        c->mods.push_back(make_mod_consts(moduli[i]));
        if (have_tables) {
            if (!supports_ntt(moduli[i], degree)) throw StatusError(E_NTT_UNAVAILABLE, "NttOperatorUnavailable");
            NttTables t;
            t.omegas.assign(omegas + i * degree, omegas + (i + 1) * degree);
            t.omegas_shoup.assign(omegas_shoup + i * degree, omegas_shoup + (i + 1) * degree);
            t.zetas_inv.assign(zetas_inv + i * degree, zetas_inv + (i + 1) * degree);
            t.zetas_inv_shoup.assign(zetas_inv_shoup + i * degree, zetas_inv_shoup + (i + 1) * degree);
            t.size_inv = size_inv[i];
            t.size_inv_shoup = size_inv_shoup[i];
            c->tabs.push_back(std::move(t));
        } else {
            c->tabs.push_back(make_ntt_tables(moduli[i], degree));
        }
    }
    for (size_t i = 0; i < c->L; i++) {
        const NttTables &t = c->tabs[i];
        u64 h = splitmix64(moduli[i] ^ degree);
        for (size_t j = 0; j < degree; j++) {
            h = splitmix64(h ^ t.omegas[j]) + t.omegas_shoup[j];
            h = splitmix64(h ^ t.zetas_inv[j]) + t.zetas_inv_shoup[j];
        }
        c->tab_fp.push_back(splitmix64(h ^ t.size_inv) + t.size_inv_shoup);
    }
    if (device >= 0) {
        int ndev = 0;
        FHE_HIP_CHECK(hipGetDeviceCount(&ndev));
        require(device < ndev, E_HIP, "no such HIP device");
        FHE_HIP_CHECK(hipSetDevice(device));
        std::vector<DevMod> hm(c->L);
        static_assert(sizeof(DevMod) == sizeof(ModConsts), "DevMod layout");
        std::memcpy(hm.data(), c->mods.data(), c->L * sizeof(DevMod));
        c->d_mods.upload(hm);
        std::vector<k::u64x2> tw(c->L * degree), itw(c->L * degree), ninv(2 * c->L);
        for (size_t i = 0; i < c->L; i++) {
            const NttTables &t = c->tabs[i];
            for (size_t j = 0; j < degree; j++) {
                tw[i * degree + j] = k::u64x2{t.omegas[j], t.omegas_shoup[j]};
                itw[i * degree + j] = k::u64x2{t.zetas_inv[j], t.zetas_inv_shoup[j]};
            }
            // {N^-1, shoup} and {z_last * N^-1, shoup}: the last inverse stage (one block, twiddle
            // zetas_inv[N-2]) absorbs the N^-1 scaling
            const u64 zn = mulmod(t.zetas_inv[degree - 2], t.size_inv, moduli[i]);
            ninv[2 * i] = k::u64x2{t.size_inv, t.size_inv_shoup};
            ninv[2 * i + 1] = k::u64x2{zn, shoup(zn, moduli[i])};
        }
        c->d_tw.upload(tw);
        c->d_itw.upload(itw);
        c->d_ninv.upload(ninv);
        // F64 twins for moduli below 2^50 (host doubles: conversion exact, division correctly rounded)
        bool any_f64 = false;
        for (size_t i = 0; i < c->L; i++) any_f64 = any_f64 || (moduli[i] >> 50) == 0;
        if (any_f64) {
            auto bits = [](double d) {
                u64 u;
                std::memcpy(&u, &d, sizeof(u));
                return u;
            };
            std::vector<k::u64x2> twf(c->L * degree, k::u64x2{0, 0}), itwf(c->L * degree, k::u64x2{0, 0}), ninvf(2 * c->L, k::u64x2{0, 0});
            for (size_t i = 0; i < c->L; i++) {
                if (moduli[i] >> 50) continue;
                const double pd = (double)moduli[i];
                auto pair = [&](u64 w) { return k::u64x2{bits((double)w), bits((double)w / pd)}; };
                for (size_t j = 0; j < degree; j++) {
                    twf[i * degree + j] = pair(tw[i * degree + j].x);
                    itwf[i * degree + j] = pair(itw[i * degree + j].x);
                }
                ninvf[2 * i] = pair(ninv[2 * i].x);
                ninvf[2 * i + 1] = pair(ninv[2 * i + 1].x);
            }
            c->d_tw_f.upload(twf);
            c->d_itw_f.upload(itwf);
            c->d_ninv_f.upload(ninvf);
        }
        std::vector<k::u64x2> pow2(c->L);
        for (size_t i = 0; i < c->L; i++) {
            const u64 two64 = (u64)((((u128)1) << 64) % moduli[i]);
            pow2[i] = k::u64x2{two64, mulmod(two64, two64, moduli[i])};
        }
        c->d_pow2.upload(pow2);
    }
    ctx_fill_inv_last(*c);
    // next_context chain (M/rq/context.rs:75-79): prefixes sharing the root's tables
    Ctx *parent = c.get();
    for (size_t l = c->L - 1; l >= 1; l--) {
        auto ch = std::make_unique<Ctx>();
        ch->device = device;
        ch->n = degree;
        ch->logn = c->logn;
        ch->L = l;
        ch->moduli.assign(moduli.begin(), moduli.begin() + l);
        ch->root = c.get();
        ctx_fill_inv_last(*ch);
        parent->next = std::move(ch);
        parent = parent->next.get();
    }
    return c;
}

// ------------------------------------------------------------------- launch helpers ----
inline hipStream_t as_stream(void *s) { return (hipStream_t)s; }
constexpr unsigned EW_THREADS = 256;

template <class K>
inline void allow_big_lds(K kernel, size_t bytes) {
    if (bytes > 48 * 1024)
        FHE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
}

// One launch of KERNEL (a compile-time constant, so that the call in FHE_LAUNCH stays a direct one)
template <auto KERNEL, class... A>
inline void launch_k(const char *name, dim3 grid, dim3 block, size_t lds, hipStream_t s, A... args) {
    allow_big_lds(KERNEL, lds);
    FHE_LAUNCH(name, KERNEL, grid, block, lds, s, args...);
}

// ---- launch geometry: a site names its kernel, its label, what it runs over and its arguments; how that becomes a
// grid, and what is refused, is written here.  The two limits are this file's only assumptions about a grid: x below
// 2^31 blocks (beyond it the `unsigned` of a dim3 would wrap), y and z at most GRID_YZ_MAX (nothing here relies on what
// the runtime does with more: a site either refuses a larger batch or cuts it with for_groups).
constexpr size_t GRID_YZ_MAX = 65535;
inline u64 blocks_for(u64 total, u64 threads) { return (total + threads - 1) / threads; }
inline unsigned grid_x(u64 blocks, const char *what, const char *advice = "") {
    if (blocks > 0x7fffffffu) throw StatusError(E_ARG, std::string(what) + ": the launch exceeds the grid limit" + advice);
    return (unsigned)blocks;
}
// `blocks` workgroups of `threads` lanes in one dimension
template <auto KERNEL, class... A>
inline void launch_blocks(const char *name, u64 blocks, unsigned threads, size_t lds, hipStream_t s, A... args) {
    launch_k<KERNEL>(name, dim3(grid_x(blocks, name)), dim3(threads), lds, s, args...);
}
// element-wise: one lane per element of `total`
template <auto KERNEL, unsigned THREADS = EW_THREADS, class... A>
inline void launch_ew(const char *name, u64 total, hipStream_t s, A... args) {
    launch_blocks<KERNEL>(name, blocks_for(total, THREADS), THREADS, 0, s, args...);
}
// x: one lane per element of `per`; y and z: whatever else the kernel's grid runs over (rows, parts, items of a batch)
template <auto KERNEL, unsigned THREADS = EW_THREADS, size_t LDS = 0, class... A>
inline void launch_rows(const char *name, u64 per, size_t y, size_t z, hipStream_t s, A... args) {
    if (y > GRID_YZ_MAX || z > GRID_YZ_MAX) throw StatusError(E_ARG, std::string(name) + ": batch exceeds the grid limit");
    launch_k<KERNEL>(name, dim3(grid_x(blocks_for(per, THREADS), name), (unsigned)y, (unsigned)z), dim3(THREADS), LDS, s, args...);
}
// (a kernel as a value, for the local launch lambdas of a site: decltype(kernel)::value is the kernel)
template <auto KERNEL>
struct kernel_c {
    static constexpr auto value = KERNEL;
};

// ---- instance selection: a run-time property of a launch becomes a template argument of its kernel ----
// Each helper hands its callback a std::integral_constant; the callback names the kernel's template-id with
// decltype(x)::value.  A callback is instantiated for EVERY value its helper offers, so a site that must not create an
// instance (F64 below 4096 points, a gathering loader below 4096, ...) narrows the bounds or tests with `if constexpr`.
template <int V>
using int_c = std::integral_constant<int, V>;

// f(int_c<LM>) for LM == logn in [LO, HI]; E_ARG with `what` outside
template <int LO, int... I, class F>
inline bool with_logn_from(size_t logn, std::integer_sequence<int, I...>, F &f) {
    return ((logn == (size_t)(LO + I) && (f(int_c<LO + I>{}), true)) || ...);
}
template <int LO, int HI, class F>
inline void with_logn(size_t logn, const char *what, F &&f) {
    if (!with_logn_from<LO>(logn, std::make_integer_sequence<int, HI - LO + 1>{}, f)) throw StatusError(E_ARG, what);
}

// the same for any other small integer of a launch (a modulus count): f(int_c<V>) for V == v in [LO, HI]
template <int LO, int HI, class F>
inline void with_int(size_t v, const char *what, F &&f) {
    with_logn<LO, HI>(v, what, std::forward<F>(f));
}

// f(bool_constant<NARROW>, int_c<HR>) for rows of 2^LM points: the F64 class hr = 3, 4, 5 (Ctx::f64_class) exists for
// whole rows of 4096 ... 16384 points only; otherwise the integer instances, narrow (every modulus below 2^60) or general
template <int LM, class F>
inline void with_row_kind(bool narrow, int hr, F &&f) {
    if constexpr (LM >= 12 && LM <= 14) {
        if (hr == 3) return f(std::false_type{}, int_c<3>{});
        if (hr == 4) return f(std::false_type{}, int_c<4>{});
        if (hr == 5) return f(std::false_type{}, int_c<5>{});
    }
    if (narrow) f(std::true_type{}, int_c<0>{});
    else f(std::false_type{}, int_c<0>{});
}

template <class F>
inline void with_bool(bool b, F &&f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// The kernels that hold one tile of 2^logm points in LDS (logm in [LO, 14]): f(int_c<LM>, bool_constant<NARROW>, int_c<HR>)
template <int LO = 3, class F>
inline void with_tile(size_t logm, const char *what, bool narrow, int hr, F &&f) {
    with_logn<LO, 14>(logm, what, [&](auto lm) {
        with_row_kind<decltype(lm)::value>(narrow, hr, [&](auto nrw, auto h) { f(lm, nrw, h); });
    });
}
// ... and their launch: `grid` workgroups of one 2^lm-point tile each
template <auto KERNEL, class... A>
inline void launch_tile(const char *name, int lm, size_t grid, hipStream_t s, A... args) {
    launch_blocks<KERNEL>(name, grid, k::ntt_threads_c(lm), k::lds_words(1u << lm) * sizeof(u64), s, args...);
}

// A whole-row launch (rows of at most one LDS tile, N <= 16384: the encoding, sampling, encryption, key-generation
// and share kernels) over the moduli [0, rows) of a context.  It decides the instance -- integer (narrow: every modulus
// below 2^60) or the F64 class of those rows (Ctx::f64_rows; `f64_on`: the caller's reading of the switch, taken once
// for all launches of a call) -- and the twiddle table that goes with it.  A site names its kernel as a generic lambda
// (lm, nrw, h) -> kernel_c<...<lm(), nrw(), h()>> and its own arguments: rows(name, grid, s, kernel, args...).
constexpr const char *ENC_TILE = "unsupported encoding tile size";
struct RowLaunch {
    const Ctx &c;
    bool narrow;
    int hr;
    RowLaunch(const Ctx &c_, size_t rows, bool f64_on) : c(c_), narrow(c_.below_2p60(0, rows)), hr(c_.f64_rows(0, rows, f64_on)) {}
    bool f64() const { return hr > 0; }
    const k::u64x2 *tw() const { return hr > 0 ? c.dtw_f() : c.dtw(); }
    const k::u64x2 *itw() const { return hr > 0 ? c.ditw_f() : c.ditw(); }
    template <class K, class... A>
    void operator()(const char *name, size_t grid, hipStream_t s, K kernel, A... args) const {
        with_tile(c.logn, ENC_TILE, narrow, hr, [&](auto lm, auto nrw, auto h) {
            launch_tile<decltype(kernel(lm, nrw, h))::value>(name, lm, grid, s, args...);
        });
    }
};

// f(int_c<V>) for V == v in [LO, HI], f(int_c<0>) above: a compile-time count where an instance exists, else the
// generic instance (run-time count, arrays in scratch); E_ARG with `what` below LO
template <int LO, int HI, class F>
inline void with_int_or_generic(size_t v, const char *what, F &&f) {
    if (v > (size_t)HI) f(int_c<0>{});
    else with_int<LO, HI>(v, what, std::forward<F>(f));
}

// f(b0, nb) for the launch groups [b0, b0 + nb) of a batch, `group` items each (the last one the rest)
template <class F>
inline void for_groups(size_t batch, size_t group, F &&f) {
    for (size_t b0 = 0; b0 < batch; b0 += group) f(b0, std::min(group, batch - b0));
}

// One launch of ntt_kernel on `grid` tiles of 2^logm points.  hr != 0 (Ctx::f64_rows: whole rows of 4096 / 8192 / 16384
// points, every modulus of the launch below 2^50): the F64 instances, under the label name_f64.
// (GATHER: galois_apply folds the substitution from N = 4096 on: three tile sizes)
template <bool INV, bool GATHER = false>
inline void launch_ntt_lds(const Ctx &c, const char *name, const char *name_f64, uint32_t logm, bool narrow, int hr,
                           size_t grid, hipStream_t s, const u64 *in, u64 *out, const k::RowMap &map, uint32_t logn) {
    with_tile<GATHER ? 12 : 3>(
        logm, GATHER ? "unsupported NTT tile size for the gathering loader" : "unsupported NTT tile size", narrow, hr,
        [&](auto lm, auto nrw, auto h) {
            constexpr int LM = decltype(lm)::value, HR = decltype(h)::value;
            launch_tile<k::ntt_kernel<INV, LM, decltype(nrw)::value, 1, GATHER, HR>>(
                HR ? name_f64 : name, LM, grid, s, in, out, map, c.dmods(),
                HR ? (INV ? c.ditw_f() : c.dtw_f()) : (INV ? c.ditw() : c.dtw()), HR ? c.dninv_f() : c.dninv(), logn);
        });
}

// The logn - 13 global radix stages of rows larger than LDS (N = 32768 / 65536), over `rows` residue rows.
template <bool INV>
inline void launch_ntt_global(const Ctx &c, u64 rows, hipStream_t s, const u64 *in, u64 *out, const k::RowMap &map) {
    const char *name = INV ? "ntt_inv_global" : "ntt_fwd_global";
    const u64 blocks = rows * ((1u << 13) / 256);
    auto launch = [&](auto kernel) {
        launch_blocks<decltype(kernel)::value>(name, blocks, 256, 0, s, in, out, map, c.dmods(), INV ? c.ditw() : c.dtw(), c.dninv(),
                                               (uint32_t)c.logn);
    };
    if (c.logn == 15) launch(kernel_c<k::ntt_global_kernel<INV, 2>>{});
    else launch(kernel_c<k::ntt_global_kernel<INV, 3>>{});
}

// Forward / inverse NTT of `npolys * map.rows` residue rows.  N <= 16384: one LDS-resident
// kernel.  N = 32768 / 65536: G0 global radix stages + LDS kernel on 8192-point sub-blocks.
inline void launch_ntt(const Ctx &c, bool inverse, const u64 *in, u64 *out, k::RowMap map, size_t npolys,
                       hipStream_t s) {
    if (npolys == 0 || map.rows == 0) return;
    const uint32_t logn = (uint32_t)c.logn;
    const unsigned rows_total = grid_x(npolys * map.rows, "ntt");
    const size_t first = (size_t)((int32_t)map.row_begin + map.mod_offset);
    // every modulus of the launch below 2^60: the transform without per-stage conditional subtractions
    const bool narrow = c.below_2p60(first, map.rows);
    // (inverse: with subst_exp the source rows are read through the substitution x -> x^subst_exp, galois_apply)
    auto inverse_lds = [&](uint32_t logm, int hr, size_t grid) {
        with_bool(map.subst_exp != 0, [&](auto gather) {
            launch_ntt_lds<true, decltype(gather)::value>(c, "ntt_inv", "ntt_inv_f64", logm, narrow, hr, grid, s, in, out, map,
                                                          logn);
        });
    };
    if (logn <= 14) {
        // every modulus of the launch below 2^50: the FP64-FMA instances (round 6)
        const int hr = c.f64_rows(first, map.rows);
        if (inverse) return inverse_lds(logn, hr, rows_total);
        launch_ntt_lds<false>(c, "ntt_fwd", "ntt_fwd_f64", logn, narrow, hr, rows_total, s, in, out, map, logn);
        return;
    }
    const uint32_t logm = 13, g0 = logn - logm;
    const size_t tiles = (size_t)rows_total << g0;
    // (the LDS halves take the bound-tracked narrow passes here too)
    k::RowMap inplace = map;
    inplace.src_poly_stride = map.dst_poly_stride;
    inplace.src_row_fixed = -1;
    inplace.in2 = nullptr;   // (the second half of the transform works in `out`: one array)
    inplace.subst_exp = 0;
    if (!inverse) {
        launch_ntt_global<false>(c, rows_total, s, in, out, map);
        if (narrow)   // (the global stages above leave values below 4p: FWD_B0 = 4)
            launch_tile<k::ntt_kernel<false, 13, true, 4>>("ntt_fwd", 13, tiles, s, out, out, inplace, c.dmods(), c.dtw(),
                                                           c.dninv(), logn);
        else
            launch_ntt_lds<false>(c, "ntt_fwd", nullptr, logm, false, 0, tiles, s, out, out, inplace, logn);
    } else {
        inverse_lds(logm, 0, tiles);
        launch_ntt_global<true>(c, rows_total, s, out, out, inplace);
    }
}

// Fused tensor + inverse NTT over the extended basis.  Rows that fit LDS (logn <= 14): one kernel.
// N = 32768 / 65536: the same kernel on 8192-point sub-blocks, then the global inverse stages.
// (Defined after full_map.)
inline void launch_tensor_intt(const Ctx &e, const k::TensorSrc &ts, u64 *out, size_t nb, hipStream_t s, bool reverse = false);

// all rows of [npolys][rows_in_poly][N], modulus = row index
inline k::RowMap full_map(const Ctx &c, size_t rows_in_poly) {
    k::RowMap m{};
    m.rows = (uint32_t)rows_in_poly;
    m.row_begin = 0;
    m.mod_offset = 0;
    m.src_row_fixed = -1;
    m.src_poly_stride = m.dst_poly_stride = (u64)rows_in_poly * c.n;
    m.in2 = nullptr;
    m.split = 0;
    m.reverse = 0;
    m.subst_exp = 0;
    return m;
}

// ... with its own source and destination polynomial strides
inline k::RowMap strided_map(const Ctx &c, size_t rows_in_poly, u64 src_stride, u64 dst_stride) {
    k::RowMap m = full_map(c, rows_in_poly);
    m.src_poly_stride = src_stride;
    m.dst_poly_stride = dst_stride;
    return m;
}
// the rows after the first `ncommon` of [npolys][c.L][N] (what a basis extension adds to the rows both bases share)
inline k::RowMap new_rows_map(const Ctx &c, size_t ncommon) {
    k::RowMap m = full_map(c, c.L);
    m.rows = (uint32_t)(c.L - ncommon);
    m.row_begin = (uint32_t)ncommon;
    return m;
}

inline void launch_tensor_intt_rows(const Ctx &e, const k::TensorSrc &ts, u64 *out, size_t nb, uint32_t row_begin,
                                    uint32_t lrows, bool narrow, hipStream_t s, bool reverse, int f64_hr = 0) {
    const uint32_t logn = (uint32_t)e.logn, logm = logn <= 14 ? logn : 13;
    // 8 (row, pair, sub-block) combinations x 3 slots per group
    const size_t groups = ((((size_t)lrows * nb) << (logn - logm)) + 7) / 8;
    auto launch = [&](auto kernel, bool nrw, bool f64) {
        launch_tile<decltype(kernel)::value>(f64 ? "tensor_intt_f64" : nrw ? "tensor_intt_narrow" : "tensor_intt", (int)logm,
                                             groups * 24, s, ts, out, e.dmods(), f64 ? e.ditw_f() : e.ditw(),
                                             f64 ? e.dninv_f() : e.dninv(), (uint32_t)e.L, (uint32_t)nb, logn, row_begin, lrows,
                                             reverse ? 1u : 0u);
    };
    if (logn > 14) {   // 8192-point sub-blocks
        with_bool(narrow,
                  [&](auto nrw) { launch(kernel_c<k::tensor_intt_kernel<13, true, decltype(nrw)::value>>{}, nrw, false); });
        return;
    }
    // (round 6: rows below 2^50 on the F64 instances)
    with_tile(logn, "unsupported tensor tile size", narrow, f64_hr, [&](auto lm, auto nrw, auto h) {
        constexpr int HR = decltype(h)::value;
        launch(kernel_c<k::tensor_intt_kernel<decltype(lm)::value, false, decltype(nrw)::value, HR>>{}, nrw, HR != 0);
    });
}

inline void launch_tensor_intt(const Ctx &e, const k::TensorSrc &ts, u64 *out, size_t nb, hipStream_t s, bool reverse) {
    // maximal runs of rows of the same kind (moduli below 2^60 or not): one launch each (reverse: last run first)
    bool allow = true;
    // A launch that does not fill the device anyway (its workgroups all run at once: a single ciphertext pair, a handful)
    // takes ONE workgroup's time whatever its passes cost, so two launches -- narrow rows, then general rows -- take twice
    // that: such a launch runs every row on the general passes (valid for any modulus below 2^62) in one go.
    // (C2, one pair: tensor_intt 2 x 16.4 us -> 1 x; profiles/r05_latency_breakdown.json)
    {
        const uint32_t lsub = e.logn > 14 ? (uint32_t)e.logn - 13 : 0;
        // (threshold: one round of workgroups -- two fit a CU with 8192-point tiles and smaller, one with 16384-point
        // tiles; C2 at 8 / 16 pairs: profiles/r05_tensor_one_launch_ab.jsonl)
        const size_t slots = (size_t)device_cus(e.device) * (e.logn == 14 ? 1 : 2);
        if ((((size_t)3 * e.L * nb) << lsub) <= slots && device_cus(e.device) > 8) allow = false;
    }
    struct Run {
        uint32_t r0, n;
        int kind;   // 0: general passes, 1: moduli below 2^60 (narrow passes), 2: below 2^50 (round 6: the F64 instances)
    };
    std::vector<Run> runs;
    auto kind_of = [&](uint32_t r) { return !allow ? 0 : e.f64_rows(r, 1) ? 2 : e.below_2p60(r, 1) ? 1 : 0; };
    uint32_t r0 = 0;
    while (r0 < e.L) {
        const int kd = kind_of(r0);
        uint32_t r1 = r0 + 1;
        while (r1 < e.L && kind_of(r1) == kd) r1++;
        runs.push_back(Run{r0, r1 - r0, kd});
        r0 = r1;
    }
    if (reverse) std::reverse(runs.begin(), runs.end());
    for (const Run &r : runs)
        launch_tensor_intt_rows(e, ts, out, nb, r.r0, r.n, r.kind == 1, s, reverse, r.kind == 2 ? e.f64_class(r.r0, r.n) : 0);
    if (e.logn > 14) launch_ntt_global<true>(e, nb * 3 * e.L, s, out, out, full_map(e, e.L));   // (they finish every row)
}

inline void ntt_polys(const Ctx &c, bool inverse, const u64 *in, u64 *out, size_t npolys, hipStream_t s) {
    c.need_device();
    launch_ntt(c, inverse, in, out, full_map(c, c.L), npolys, s);
}

inline void ew_op(const Ctx &c, u64 *a, const u64 *b, size_t npolys, uint32_t op, hipStream_t s) {
    c.need_device();
    const u64 total = (u64)npolys * c.L * c.n;
    if (!total) return;
    launch_ew<k::ew_kernel>("ew", total, s, a, b, c.dmods(), (uint32_t)c.L, (uint32_t)c.logn, op, total);
}

// `npolys` runs of `per` words, run i from in + i * in_stride to out + i * out_stride
inline void copy_rows(const u64 *in, u64 in_stride, u64 *out, u64 out_stride, u64 per, size_t npolys, hipStream_t s) {
    launch_ew<k::copy_rows_kernel>("copy_rows", per * npolys, s, in, out, in_stride, out_stride, per, per * npolys);
}

// ------------------------------------------------------------------ Rq wire format ----
inline size_t wire_poly_bytes(const Ctx &c) {
    size_t b = 0;
    for (size_t i = 0; i < c.L; i++) b += (size_t)(64 - __builtin_clzll(c.moduli[i] - 1)) * (c.n / 8);
    return b;
}
// One launch per 32768 polynomials (the grid's z) of a wire kernel pair: rows of >= 128 coefficients between 16-byte
// aligned buffers (every row then starts on a 16-byte boundary) take the word-granular kernel over `word_lanes` lanes a
// row, the others the byte-granular one, a lane per eight coefficients.
template <auto WORDS, auto BYTES, class In, class Out>
inline void launch_wire(const char *name, const Ctx &c, u64 word_lanes, const In *in, u64 in_stride, Out *out, u64 out_stride,
                        size_t npolys, hipStream_t s) {
    const u64 wb = wire_poly_bytes(c), groups = c.n / 8;
    const bool words = c.n >= 128 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0;
    for_groups(npolys, 32768, [&](size_t p0, size_t np) {
        auto launch = [&](auto kernel, auto threads, u64 per) {
            launch_rows<decltype(kernel)::value, decltype(threads)::value>(name, per, c.L, np, s, in + p0 * in_stride,
                                                                           out + p0 * out_stride, c.dmods(), (uint32_t)c.L,
                                                                           (uint32_t)c.logn, wb);
        };
        if (words) launch(kernel_c<WORDS>{}, int_c<256>{}, word_lanes);
        else if (groups < 256) launch(kernel_c<BYTES>{}, int_c<64>{}, groups);
        else launch(kernel_c<BYTES>{}, int_c<256>{}, groups);
    });
}
// polys [npolys][L][N] -> bytes [npolys][wire_poly_bytes]; from_ntt: inverse NTT first (into scratch).
inline void wire_serialize(const Ctx &c, const u64 *polys, uint8_t *bytes, size_t npolys, bool from_ntt, hipStream_t s) {
    c.need_device();
    if (!npolys) return;
    const u64 pe = (u64)c.L * c.n;
    WsGuard pb(from_ntt ? npolys * pe * sizeof(u64) : 8, s);
    if (from_ntt) {
        launch_ntt(c, true, polys, pb.u(), full_map(c, c.L), npolys, s);
        polys = pb.u();
    }
    // (the word-granular grid covers the widest row, 62 bits)
    launch_wire<k::wire_pack_words_kernel, k::wire_pack_kernel>("wire_pack", c, (c.n >> 7) * 64, polys, pe, bytes,
                                                                wire_poly_bytes(c), npolys, s);
}
inline void wire_deserialize(const Ctx &c, const uint8_t *bytes, u64 *polys, size_t npolys, bool to_ntt, hipStream_t s) {
    c.need_device();
    if (!npolys) return;
    launch_wire<k::wire_unpack_words_kernel, k::wire_unpack_kernel>("wire_unpack", c, c.n / 2, bytes, wire_poly_bytes(c), polys,
                                                                    (u64)c.L * c.n, npolys, s);
    if (to_ntt) launch_ntt(c, false, polys, polys, full_map(c, c.L), npolys, s);
}

// Poly::random_from_seed (M/rq/mod.rs:276-292): seeds [npolys][32] -> polys [npolys][L][N]
inline void polys_from_seeds(const Ctx &c, const uint8_t *seeds, u64 *polys, size_t npolys, hipStream_t s) {
    c.need_device();
    if (!npolys) return;
    launch_blocks<k::seed_expand_kernel>("seed_expand", npolys, k::SEED_THREADS, k::SEED_SMEM_BYTES, s, seeds, polys, c.dmods(),
                                         (uint32_t)c.L, (uint32_t)c.logn);
}

// ----------------------------------------------------------------------- rq::Scaler ----
struct Scaler {
    const Ctx *from = nullptr, *to = nullptr;
    size_t ncommon = 0;
    bool wide_num = false;   // the numerator exceeds 64 bits: a cipher -> plain scaler of a plaintext modulus above 2^64
    ScalerConstants c;
    DevBuf<u64> d_all;
    k::ScalerDev dev{};
};

// The NF of the scale_kernel<NF> instances (the column's residues live in registers: NF >= the source moduli).
// 4 / 9 / 17 / 33: the operand and product bases of BASELINE's configs (L = 4, 8, 16; K = 9, 17, 33).  Round 5 added
// 6 / 12 / 20 for the reference's stock sets (default_parameters_128: L = 3, 5, 9 and K = 6, 10, 18), which ran on
// the next instance up -- K = 10 on NF = 17, K = 18 on NF = 33: up to 1.8 x the term loops, all of it zero padding.
// Round 6: the exact fits that were still padded -- 3 / 5 / 10 / 18 (stock sets: L = 3 on NF = 4, L = 5 on 6, K = 10 on
// 12, K = 18 on 20: 10-25 % of the terms were zeros) and 8 / 16 (C3's and C5's operand bases, on 9 and 17); 14 / 23 /
// 27 / 31 for the levels of C5's chain (L = 15 ... 10: K = 31, 29, 27, 25, 23, 21 all ran on NF = 33, up to 57 % padding).
using ScaleNFs = std::integer_sequence<int, 3, 4, 5, 6, 8, 9, 10, 12, 14, 16, 17, 18, 20, 23, 27, 31, 33, 64>;
// f(int_c<NF>) for the smallest NF that holds `nfrom` source moduli; false when there is none
template <int... NF, class F>
inline bool with_scale_nf(size_t nfrom, std::integer_sequence<int, NF...>, F &&f) {
    return ((nfrom <= (size_t)NF && (f(int_c<NF>{}), true)) || ...);
}
inline size_t scale_kernel_nf(size_t nfrom) {
    size_t nf = 64;   // (more than 64 source moduli: refused by scaler_upload and launch_scale)
    with_scale_nf(nfrom, ScaleNFs{}, [&](auto c) { nf = (size_t)decltype(c)::value; });
    return nf;
}

inline void scaler_upload(Scaler &s) {
    const ScalerConstants &c = s.c;
    if (s.from->device < 0) return;
    require(c.nfrom <= 64, E_ARG, "RNS scaler supports at most 64 source moduli");
    std::vector<u64> all;
    auto push = [&](const std::vector<u64> &v) {
        size_t off = all.size();
        all.insert(all.end(), v.begin(), v.end());
        return off;
    };
    // device-side derived tables (see scale_kernel): gamma_neg and the 16-entry fold tables
    // (the kernel takes v's bits from limb 3 of the sum on: theta_garner_shift - 1 in [96, 126]; RnsScaler::new's
    // choice, scaler.rs:130-142, is 123 ... 127 for moduli below 2^62 and at most 64 of them)
    require(c.theta_garner_shift >= 97 && c.theta_garner_shift <= 127, E_ARG, "theta_garner_shift out of range");
    std::vector<u64> gneg(c.nto), vtab(c.nto * 16), wtab(c.nto * 32), c128(c.nto * 16);
    for (size_t j = 0; j < c.nto; j++) {
        const u64 q = s.to->moduli[j];
        gneg[j] = (q - c.gamma[j] % q) % q;
        const u64 two64 = (u64)((((u128)1) << 64) % q);
        const u64 two128 = mulmod(two64, two64, q);
        const u64 g64 = mulmod(two64, gneg[j], q);
        for (u64 k = 0; k < 16; k++) {
            vtab[j * 16 + k] = mulmod(k % q, g64, q);
            // +w = w_hi 2^64 + w_lo: w_hi 2^64 mod q;  -w = ~w_lo + (1 - (w_hi + 1) 2^64): that constant mod q
            wtab[j * 32 + k] = mulmod(k % q, two64, q);
            wtab[j * 32 + 16 + k] = (q + 1 % q - mulmod((k + 1) % q, two64, q)) % q;
            c128[j * 16 + k] = mulmod(k % q, two128, q);
        }
    }
    // fold_mask / fold_tab (any factor): v_lo < 2^64 and the small addends (w's low word or its complement
    // < 2^64 + q, table values < 3q) give  sum_j <= (2^64 - 1 + sum_i (p_i - 1)) (q_j - 1) + 2^65 + 4 q_j;  where that
    // is below 2^(2 k_j + 6) the bits above 2^(2 k_j) index a 64-entry table of their residues.
    std::vector<u64> fold(c.nto * 64, 0);
    u64 fold_mask = 0;
    if (c.nto <= 64) {
        BigUint sum_p = BigUint::pow2(64) - BigUint(1);
        for (size_t i = 0; i < c.nfrom; i++) sum_p = sum_p + BigUint(s.from->moduli[i] - 1);
        for (size_t j = 0; j < c.nto; j++) {
            const u64 q = s.to->moduli[j];
            const size_t k = 64 - (size_t)__builtin_clzll(q);
            const BigUint bound = sum_p * BigUint(q - 1) + BigUint::pow2(65) + BigUint(q) * BigUint(4);
            if (bound < BigUint::pow2(std::min<size_t>(2 * k + 6, 128))) {   // (< 2^128: nothing above the 128-bit sum)
                fold_mask |= (u64)1 << j;
                const u64 unit = (BigUint::pow2(2 * k) % BigUint(q)).to_u64();
                for (u64 i = 0; i < 64; i++) fold[j * 64 + i] = mulmod(i % q, unit, q);
            }
        }
    }
    // per-source tables zero-padded to the NF of the scale_kernel instance that serves this scaler (launch_scale):
    // the kernel's term loops then need no bounds checks
    const size_t nf = scale_kernel_nf(c.nfrom);
    auto padded = [&](const std::vector<u64> &v) {
        std::vector<u64> r(v);
        r.resize(nf, 0);
        return r;
    };
    std::vector<u64> omega_p(c.nto * nf, 0);
    for (size_t j = 0; j < c.nto; j++)
        std::copy(c.omega.begin() + j * c.nfrom, c.omega.begin() + (j + 1) * c.nfrom, omega_p.begin() + j * nf);
    std::vector<u64> sign64(c.theta_omega_sign.begin(), c.theta_omega_sign.end());
    // one-accumulator form of w (scale_kernel): subtracted terms enter as (~x) * theta, and the host sums what that
    // adds too much: (2^64 - 1) * theta_omega_i over the subtracted sources, plus (2^128 - 1) * theta_gamma when the
    // v * theta_gamma term is subtracted (v = v_hi 2^64 + v_lo, both words complemented); all mod 2^256
    std::vector<u64> mask64(c.nfrom, 0);
    BigUint wk(0);
    for (size_t i = 0; i < c.nfrom; i++)
        if (c.theta_omega_sign[i]) {
            mask64[i] = ~0ull;
            const u64 limbs[2] = {c.theta_omega_lo[i], c.theta_omega_hi[i]};
            wk = wk + BigUint::from_limbs(limbs, 2) * (BigUint::pow2(64) - BigUint(1));
        }
    if (!c.theta_gamma_sign) {
        const u64 limbs[2] = {c.theta_gamma_lo, c.theta_gamma_hi};
        wk = wk + BigUint::from_limbs(limbs, 2) * (BigUint::pow2(128) - BigUint(1));
    }
    wk = wk % BigUint::pow2(256);
    size_t o_fold = push(fold);
    size_t o_gn = push(gneg), o_om = push(omega_p), o_vt = push(vtab), o_wt = push(wtab), o_c128 = push(c128);
    size_t o_tol = push(padded(c.theta_omega_lo)), o_toh = push(padded(c.theta_omega_hi)), o_tos = push(padded(sign64));
    size_t o_tgl = push(padded(c.theta_garner_lo)), o_tgh = push(padded(c.theta_garner_hi));
    size_t o_tom = push(padded(mask64));
    s.d_all.upload(all);
    u64 *b = s.d_all.p;
    s.dev.gamma_neg = b + o_gn;
    s.dev.omega = b + o_om;
    s.dev.vhi_tab = b + o_vt;
    s.dev.w_tab = b + o_wt;
    s.dev.c128_tab = b + o_c128;
    s.dev.theta_omega_lo = b + o_tol;
    s.dev.theta_omega_hi = b + o_toh;
    s.dev.theta_omega_sign = b + o_tos;
    s.dev.theta_omega_mask = b + o_tom;
    for (size_t i = 0; i < 4; i++) s.dev.w_const[i] = wk.limb(i);
    s.dev.theta_garner_lo = b + o_tgl;
    s.dev.theta_garner_hi = b + o_tgh;
    s.dev.theta_gamma_lo = c.theta_gamma_lo;
    s.dev.theta_gamma_hi = c.theta_gamma_hi;
    // narrow_mask: for a factor-one scaler v = round(sum_i r_i theta_i / 2^shift) <= sum_i r_i + 2 (theta_i / 2^shift
    // ~ garner_i / Q < 1), so target j's sum  sum_i r_i omega_ij + v gamma_neg_j + (small terms < 4 q_j)  is at most
    // (2 * sum_i (q_i - 1) + 2) * (q_j - 1) + 4 q_j.  Where that is below 2^(2 k_j + 1), k_j = bits(q_j), the
    // kernel reduces with the single-word Barrett instead of the 128-bit-ratio reduction.
    s.dev.narrow_mask = 0;
    if (c.is_one && c.nto <= 64) {
        BigUint sum_q(0);
        for (size_t i = 0; i < c.nfrom; i++) sum_q = sum_q + BigUint(s.from->moduli[i] - 1);
        for (size_t j = 0; j < c.nto; j++) {
            const u64 q = s.to->moduli[j];
            const size_t k = 64 - (size_t)__builtin_clzll(q);
            const BigUint bound = (sum_q * BigUint(2) + BigUint(2)) * BigUint(q - 1) + BigUint(q) * BigUint(4);
            if (bound < BigUint::pow2(2 * k + 1)) s.dev.narrow_mask |= (u64)1 << j;
        }
    }
    // for a factor-one scaler v <= sum_i r_i + 2 (see narrow_mask above); when sum_i (q_i - 1) + 2 is below 2^64 the
    // kernel never needs v's high word
    s.dev.v_fits_64 = 0;
    if (c.is_one) {
        BigUint sum_q(2);
        for (size_t i = 0; i < c.nfrom; i++) sum_q = sum_q + BigUint(s.from->moduli[i] - 1);
        if (sum_q < BigUint::pow2(64)) s.dev.v_fits_64 = 1;
    }
    // wide_w: can |t| = |sum_i +/- r_i theta_omega_i -/+ v theta_gamma| reach 2^191?  Below that the kernel's fast path
    // (sign from bit 255, 68 bits of w) IS the reference's `t >> 191 > 0` test and 128-bit w; at or above it the
    // reference's result is defined by those bit tests and the launch takes the instance that reproduces them
    // (ADVICE r03).  Bound: r_i <= q_i - 1, v <= sum_i (q_i - 1) + 2 (theta_garner_i / 2^shift < 1).
    s.dev.wide_w = 0;
    if (!c.is_one) {
        BigUint bound(0), vmax(2);
        for (size_t i = 0; i < c.nfrom; i++) {
            const u64 limbs[2] = {c.theta_omega_lo[i], c.theta_omega_hi[i]};
            bound = bound + BigUint::from_limbs(limbs, 2) * BigUint(s.from->moduli[i] - 1);
            vmax = vmax + BigUint(s.from->moduli[i] - 1);
        }
        const u64 gl[2] = {c.theta_gamma_lo, c.theta_gamma_hi};
        bound = bound + BigUint::from_limbs(gl, 2) * vmax;
        if (!(bound < BigUint::pow2(191))) s.dev.wide_w = 1;
    }
    s.dev.fold_mask = fold_mask;
    s.dev.fold_tab = b + o_fold;
    s.dev.theta_gamma_sign = c.theta_gamma_sign ? 1 : 0;
    s.dev.is_one = c.is_one ? 1 : 0;
    s.dev.shift = (uint32_t)c.theta_garner_shift;
    s.dev.nfrom = (uint32_t)c.nfrom;
    s.dev.nto = (uint32_t)c.nto;
    s.dev.ncommon = (uint32_t)s.ncommon;
}

// Scaler::new (M/rq/scaler.rs:27-52)
inline std::unique_ptr<Scaler> scaler_create(const Ctx &from, const Ctx &to, const BigUint &num,
                                             const BigUint &den) {
    require(from.n == to.n, E_DEGREE_MISMATCH, "DegreeMismatch");
    require(from.device == to.device, E_PARAMETER_MISMATCH, "contexts live on different devices");
    auto s = std::make_unique<Scaler>();
    s->from = &from;
    s->to = &to;
    RnsContext rf(from.moduli), rt(to.moduli);
    s->c = make_scaler_constants(rf, rt, num, den);
    s->wide_num = !num.fits_u64();
    if (s->c.is_one) {
        size_t k = 0;
        while (k < from.L && k < to.L && from.moduli[k] == to.moduli[k]) k++;
        s->ncommon = k;
    }
    scaler_upload(*s);
    return s;
}

// RnsScaler::scale over `npolys * N` coefficient columns (register-resident residues: NF >= nfrom).
inline void launch_scale(const Scaler &sc, const u64 *in, u64 in_stride, u64 *out, u64 out_stride, size_t npolys,
                         hipStream_t s, bool ascending = false) {
    const Ctx &f = *sc.from, &t = *sc.to;
    const u64 total = (u64)npolys * f.n;
    if (!total) return;
    // profiler label: basis extension (more output rows than input) vs down-scaling
    const char *label = t.L > f.L ? "scale_extend" : "scale_down";
    // PLAIN instances carry no w / v_hi code: factor-one scalers whose v fits one word (every basis extension of BFV)
    const bool plain = sc.dev.is_one && sc.dev.v_fits_64;
    const uint32_t asc = ascending ? 1u : 0u;
    require(f.L <= 64, E_ARG, "RNS scaler supports at most 64 source moduli");
    with_scale_nf(f.L, ScaleNFs{}, [&](auto nf) {   // (the same NF scaler_upload padded the tables to)
        constexpr int NF = decltype(nf)::value;
        auto launch = [&](auto kernel) {
            launch_ew<decltype(kernel)::value>(label, total, s, in, out, in_stride, out_stride, sc.dev, t.dmods(), (uint32_t)f.logn,
                                               total, asc);
        };
        if (plain) launch(kernel_c<k::scale_kernel<NF, true>>{});
        else if (sc.dev.wide_w) launch(kernel_c<k::scale_kernel<NF, false, true>>{});   // the reference's bit tests on an out-of-range t, to the letter
        else launch(kernel_c<k::scale_kernel<NF, false>>{});
    });
}

// Scaler::scale (M/rq/scaler.rs:55-127) on npolys polynomials.
// `copy_common = false` leaves rows [0, ncommon) of `out` untouched (callers that read those
// rows from the source instead, see bfv_mul).
inline void scale_polys(const Scaler &sc, const u64 *in, u64 *out, size_t npolys, bool repr_is_ntt, hipStream_t s,
                        bool copy_common = true) {
    const Ctx &f = *sc.from, &t = *sc.to;
    f.need_device();
    if (!npolys) return;
    const u64 in_stride = (u64)f.L * f.n, out_stride = (u64)t.L * t.n;
    if (sc.ncommon > 0 && copy_common) copy_rows(in, in_stride, out, out_stride, (u64)sc.ncommon * f.n, npolys, s);
    if (sc.ncommon >= t.L) return;
    if (repr_is_ntt) {
        WsGuard pb(npolys * in_stride * sizeof(u64), s);
        launch_ntt(f, true, in, pb.u(), full_map(f, f.L), npolys, s);
        launch_scale(sc, pb.u(), in_stride, out, out_stride, npolys, s);
        launch_ntt(t, false, out, out, new_rows_map(t, sc.ncommon), npolys, s);
    } else {
        launch_scale(sc, in, in_stride, out, out_stride, npolys, s);
    }
}

// Scaler::scale of TWO operand arrays (Ntt form, npolys polynomials each, the same scaler) in one pass of three
// launches: out [2 * npolys][to.L][N] (in0's polynomials first).  What bfv_mul's two operand extensions are when both
// sides use the same extender (Multiplicator::default): launches twice as large, half as many of them -- each
// launch's tail (the last, partly filled round of workgroups) is paid once instead of twice.
inline void scale_polys_pair(const Scaler &sc, const u64 *in0, const u64 *in1, u64 *out, size_t npolys, hipStream_t s,
                             bool copy_common) {
    const Ctx &f = *sc.from, &t = *sc.to;
    f.need_device();
    if (!npolys) return;
    const u64 in_stride = (u64)f.L * f.n, out_stride = (u64)t.L * t.n;
    if (sc.ncommon > 0 && copy_common)
        for (int h = 0; h < 2; h++)
            copy_rows(h ? in1 : in0, in_stride, out + (u64)h * npolys * out_stride, out_stride, (u64)sc.ncommon * f.n, npolys, s);
    if (sc.ncommon >= t.L) return;
    WsGuard pb(2 * npolys * in_stride * sizeof(u64), s);
    k::RowMap mi = full_map(f, f.L);
    mi.in2 = in1;
    mi.split = (uint32_t)npolys;
    launch_ntt(f, true, in0, pb.u(), mi, 2 * npolys, s);
    launch_scale(sc, pb.u(), in_stride, out, out_stride, 2 * npolys, s);
    launch_ntt(t, false, out, out, new_rows_map(t, sc.ncommon), 2 * npolys, s);
}

// Poly::<PowerBasis>::switch_down (M/rq/mod.rs:433-492) on npolys polynomials.
inline void switch_down_polys(const Ctx &c, const u64 *in, u64 in_stride, u64 *out, u64 out_stride, size_t npolys,
                              hipStream_t s) {
    c.need_device();
    require(c.next != nullptr, E_NO_MORE_CONTEXT, "NoMoreContext");
    const u64 total = (u64)npolys * c.n;
    if (!total) return;
    launch_ew<k::switch_down_kernel>("switch_down", total, s, in, out, in_stride, out_stride, c.dmods(), c.d_inv_last.p,
                                     (uint32_t)c.L, (uint32_t)c.logn, total);
}

inline void substitute_polys(const Ctx &c, size_t exponent, const u64 *in, u64 *out, size_t npolys, bool ntt,
                             hipStream_t s) {
    c.need_device();
    const size_t e = exponent % (2 * c.n);
    require((e & 1) == 1, E_INVALID_SUBST, "InvalidSubstitutionExponent");
    const u64 total = (u64)npolys * c.L * c.n;
    if (!total) return;
    const u64 stride = (u64)c.L * c.n;
    launch_ew<k::substitute_kernel>("substitute", total, s, in, out, stride, stride, c.dmods(), (uint32_t)c.L, (uint32_t)c.logn,
                                    (uint32_t)e, ntt ? 1u : 0u, total);
}

// ------------------------------------------------------------------ KeySwitchingKey ----
struct Ksk {
    const Ctx *ct_ctx = nullptr, *ksk_ctx = nullptr;
    size_t ndigits = 0, log_base = 0;
    // how far a digit can exceed the key moduli (ks_fused_kernel's lift_mode): RNS digits are residues
    // < q_i, so q_i < 2 q_j for all i, j -> 1, < 4 q_j -> 2, otherwise (and for base-2^k digits) 0
    uint32_t lift_mode() const {
        if (log_base != 0) return 0;
        u64 mx = 0, mn = ~0ull;
        for (u64 q : ct_ctx->moduli) mx = std::max(mx, q);
        for (u64 q : ksk_ctx->moduli) mn = std::min(mn, q);
        if (mx < 2 * mn) return 1;          // (moduli < 2^62: no overflow)
        if (mx < 4 * mn) return 2;
        return 0;
    }
    uint32_t digit_arg() const { return (uint32_t)log_base | (lift_mode() << 8); }
    DevBuf<u64> c0, c0s, c1, c1s;  // [ndigits][Lk][N]
    // Round 6: the key words as doubles (bit patterns) when every key modulus is below 2^50 and the digits are RNS rows
    // (ksk_f64_eligible; empty otherwise): what ks_fused_kernel's F64 instances read in place of (c0, c0s, c1, c1s) -- 16 bytes
    // per coefficient and digit instead of 32: their accumulate takes its quotient from h / p, so no k / q_j twin exists.
    DevBuf<u64> c0f, c1f;
    // Execution options of this handle (fhe_ksk_set_mode; read once per call, like Mul's):
    //   mode      KS_AUTO: the engine picks per shape and launch (ks_use_unfused, key_switch_polys); KS_FUSED: ks_fused_kernel
    //             (rows larger than LDS: on 16384-point parts); KS_FUSED_SUB: rows larger than LDS on 8192-point sub-blocks
    //             (ks_fused_split_kernel), otherwise KS_FUSED;
    //             KS_UNFUSED: batched digit transforms + streaming MAC (RNS digits only; decomposition keys stay fused);
    //             KS_UNFUSED_SUB: the same with 8192-point sub-block tiles at N = 16384 as well
    //   w_budget  bytes of transformed digit rows (W) one stage-A / stage-B launch pair may have in flight; 0 = default
    std::atomic<int> mode{0};
    std::atomic<size_t> w_budget{0};
};
enum : int { KS_AUTO = 0, KS_FUSED = 1, KS_UNFUSED = 2, KS_UNFUSED_SUB = 3, KS_FUSED_SUB = 4 };

// Keyed batches: the keys of many clients for ONE operation (every client's relinearization key, or every client's
// Galois key of one exponent), applied to a batch in which items [c * m, (c + 1) * m) belong to key c.  The keys are
// borrowed (they outlive the set); `table` holds their (c0, c1) pointers on the device, built once at creation (one
// upload, one wait), which is what ks_mac_keyed_kernel indexes.  The keyed key switch rests on the unfused form, whose
// stage A reads no key: only RNS-digit keys of one geometry can share its launches.
struct KskSet {
    std::vector<const Ksk *> keys;
    DevBuf<k::KsKeyPtr> table;   // [nkeys]
    const Ctx *ct_ctx = nullptr, *ksk_ctx = nullptr;
    size_t ndigits = 0;
    std::atomic<size_t> w_budget{0};   // as Ksk::w_budget; 0 = default
    std::atomic<size_t> rot_split{0};  // rotation groups of a hoisted matvec launch (hoist_rot_group); 0 = the rule
    std::atomic<size_t> bsgs_tile{0};  // giant groups per block of bsgs_baby_kernel (bsgs_group_tile); 0 = the rule, 1 / 2 / 4
};
// The trailing optional argument of key_switch_polys / key_switch_add / galois_apply (one), inner_sum (one per rotation)
// and expand (one per level): polynomial b of the call takes key (b / per_key) % nkeys of `set`.
struct KsKeyed {
    const KskSet *set = nullptr;
    size_t per_key = 0;
};
inline std::unique_ptr<KskSet> kskset_create(const Ksk *const *keys, size_t nkeys) {
    require(keys != nullptr && nkeys > 0, E_ARG, "a key set needs at least one key");
    for (size_t i = 0; i < nkeys; i++) require(keys[i] != nullptr, E_ARG, "null argument: keys[i]");
    const Ksk &k0 = *keys[0];
    auto set = std::make_unique<KskSet>();
    std::vector<k::KsKeyPtr> tab(nkeys);
    for (size_t i = 0; i < nkeys; i++) {
        const Ksk &ki = *keys[i];
        require(ki.log_base == 0, E_ARG, "keyed batches take RNS-digit keys");
        // (one parameter set, one (ciphertext level, key level) pair: stage A and the moduli tables are the first key's)
        require(ki.ct_ctx->same_ring(*k0.ct_ctx) && ki.ksk_ctx->same_ring(*k0.ksk_ctx) && ki.ndigits == k0.ndigits &&
                    ki.ksk_ctx->device == k0.ksk_ctx->device && ki.ksk_ctx->same_tables(*k0.ksk_ctx, k0.ksk_ctx->L),
                E_PARAMETER_MISMATCH, "keyed batches: the keys differ in parameters, levels or digit count");
        tab[i] = k::KsKeyPtr{ki.c0.p, ki.c1.p};
        set->keys.push_back(&ki);
    }
    k0.ksk_ctx->need_device();
    set->ct_ctx = k0.ct_ctx;
    set->ksk_ctx = k0.ksk_ctx;
    set->ndigits = k0.ndigits;
    set->table.upload(tab);
    return set;
}

// Does a key over `kc` with these digits carry the F64 words (c0f, c1f)?  RNS digits, the device's F64 tables, and every
// key modulus below 2^50 (so that a canonical key word is an exact double).  Every route asks here: generation
// (ksk_generate), the wire loader (ksk_load_wire) and creation from given words (ksk_finish).
inline bool ksk_f64_eligible(const Ctx &kc, size_t log_base) {
    if (log_base != 0 || kc.device < 0 || !kc.root->d_tw_f.p) return false;
    for (u64 q : kc.moduli)
        if (q >> 50) return false;
    return true;
}

inline void ksk_validate(const Ctx &ct_ctx, const Ctx &ksk_ctx, size_t ndigits, size_t log_base) {
    require(ct_ctx.n == ksk_ctx.n, E_DEGREE_MISMATCH, "DegreeMismatch");
    require(ct_ctx.device == ksk_ctx.device, E_PARAMETER_MISMATCH, "contexts live on different devices");
    require(ksk_ctx.niterations_to(ct_ctx) >= 0, E_CONTEXT_NOT_REACHABLE,
            "ciphertext context is not reachable from the key context");
    // the key switch adds Ntt-form rows of the two contexts (and reads the caller's Ntt-form digit rows as
    // transforms under the key moduli, `xhat`): both must evaluate the shared moduli in the same order
    require(ksk_ctx.same_tables(ct_ctx, ct_ctx.L), E_PARAMETER_MISMATCH,
            "ParameterMismatch: ciphertext and key contexts were built with different NTT tables");
    if (log_base != 0) {
        require(ksk_ctx.L == 1 && ct_ctx.L == 1, E_PARAMETER_MISMATCH,
                "decomposition keys need single-modulus contexts");
        require(log_base < 63 && ndigits * log_base < 64 + log_base, E_ARG, "bad log_base / ndigits");
    } else {
        require(ndigits == ct_ctx.L, E_PARAMETER_MISMATCH, "ndigits must equal the ciphertext context's moduli count");
        require(ksk_ctx.L >= 2, E_KEYSWITCH_UNSUPPORTED, "KeySwitchingNotSupported: single-modulus key without log_base");
    }
}

// A key handle with its geometry checked and no arrays yet (ksk_alloc adds them).
inline std::unique_ptr<Ksk> make_ksk(const Ctx &ct, const Ctx &kc, size_t ndigits, size_t log_base) {
    ksk_validate(ct, kc, ndigits, log_base);
    kc.need_device();
    auto k_ = std::make_unique<Ksk>();
    k_->ct_ctx = &ct;
    k_->ksk_ctx = &kc;
    k_->ndigits = ndigits;
    k_->log_base = log_base;
    return k_;
}

// The handle's arrays: c0, c1 and their Shoup twins, and the F64 words when the key is eligible.
inline void ksk_alloc(Ksk &k_) {
    const Ctx &kc = *k_.ksk_ctx;
    const size_t count = k_.ndigits * kc.L * kc.n;
    for (DevBuf<u64> *d : {&k_.c0, &k_.c0s, &k_.c1, &k_.c1s}) d->alloc(count);
    if (ksk_f64_eligible(kc, k_.log_base)) {
        k_.c0f.alloc(count);
        k_.c1f.alloc(count);
    }
}

// The two instance rules every form of the key switch reads.  narrow: key moduli below 2^60, the transform runs without
// most conditional subtractions (fwd_butterfly_narrow).  rns: residue-row digits of same-width moduli (lift_mode 1).
inline bool ks_narrow(const Ctx &kc) { return kc.below_2p60(0, kc.L); }
inline bool ks_rns(const Ksk &k_) { return k_.digit_arg() == (1u << 8); }

template <int LOGN>
inline void launch_ks_fused(const Ksk &k_, const u64 *p, u64 p_stride, u64 *o0, u64 *o1, u64 out_stride,
                            const u64 *a0, const u64 *a1, u64 a_stride, size_t npolys, hipStream_t s,
                            const u64 *xhat, u64 xhat_stride, uint32_t gal) {
    const Ctx &kc = *k_.ksk_ctx;
    const size_t lds = (k::lds_words(1u << LOGN) + (k::ks_acc1_in_lds_c(LOGN) ? (size_t)1 << LOGN : 0)) * sizeof(u64);
    const bool narrow = ks_narrow(kc);
    // N = 8192: one workgroup owns a CU (132 KiB of LDS), so the items of a launch go to one resident workgroup per
    // CU, each prefetching its next item's first row across its epilogue
    const uint32_t items = grid_x(npolys * kc.L, "key switch");
    unsigned ks_grid = items;
#if defined(FHE_HOST_EMULATION)
    constexpr bool ks_persist_size = true;   // (every size, so that the emulated suite walks the item loop)
#else
    constexpr bool ks_persist_size = LOGN == 13;
#endif
    if (ks_persist_size) ks_grid = std::min<unsigned>(items, device_cus(kc.device));
    // RNS instances (N = 4096, 8192): residue-row digits of same-width moduli, see the kernel.  (Not at N = 16384: in
    // round 3 that instance spilled 52 B; it no longer does, and measured again at C3 in round 4 it changes nothing --
    // relinearise of 512: 4.09 / 4.18 / 4.18 ms against 4.17 / 4.14 / 4.13, profiles/r04_ks14_rns_ab.jsonl.)
    const bool rns = (LOGN == 12 || LOGN == 13) && ks_rns(k_);
    const size_t lds_tile = k::lds_words(1u << LOGN) * sizeof(u64);   // (tile-only LDS: both accumulator sets in registers)
    // one launch of ks_fused_kernel; the F64 instances read the key's F64 words and the F64 tables
    auto launch = [&](const char *name, auto kernel, unsigned grid, int threads, size_t lds_k, bool f64) {
        launch_k<decltype(kernel)::value>(
            name, dim3(grid), dim3(threads), lds_k, s, p, p_stride, o0, o1, out_stride, a0, a1, a_stride, f64 ? k_.c0f.p : k_.c0.p,
            f64 ? k_.c0f.p : k_.c0s.p, f64 ? k_.c1f.p : k_.c1.p, f64 ? k_.c1f.p : k_.c1s.p, kc.dmods(), f64 ? kc.dtw_f() : kc.dtw(),
            (uint32_t)k_.ndigits, (uint32_t)kc.L, k_.digit_arg(), xhat, xhat_stride, items, gal);
    };
    // Round 6: every key modulus below 2^50 and RNS digits -> the F64 instances (no lift: any residue row of the basis is
    // a representative under every key modulus, whatever the widths)
    if constexpr (LOGN >= 12 && LOGN <= 14) {
        const int hr = (k_.c0f.p && k_.log_base == 0) ? kc.f64_class(0, kc.L) : 0;
        if (hr) {
            // Geometry of the F64 instances.  N = 16384: the tile's own 1024 threads x 16 coefficients.  N = 8192:
            // 512 threads x 16 coefficients, BOTH accumulator sets in registers, tile-only LDS, one
            // workgroup per item -- TWO workgroups per CU, so one's barriers and LDS round trips hide behind the other's
            // arithmetic.  (The same shape at N = 4096, 256 threads: 1,024 / 256 relinearisations -2 %, 64 +23 %,
            // profiles/r06_l_f64_geometry_ab.jsonl -- N = 4096 keeps 512 threads x 8.)
            // Rounds 3 and 6 measured this cut slower with the passes it could afford then (mixed radix-8 /
            // radix-4: profiles/r03_ks13_t512_rns_ab.txt, r06_ks13_f64_t512_ab_rejected.jsonl); with one-word per-lane twiddles
            // radix-8 passes fit (126 VGPRs, no scratch) and it is ahead: relinearise of 1,024 at the stock n = 8192 set 1.114
            // -> 1.032 ms, of 64 0.114 -> 0.106 (profiles/r06_ks13_f64_t512_radix8_ab.jsonl, same digest).
            // A launch with at most one workgroup per CU has no second workgroup to overlap with: there the tile's own 1024
            // threads (N = 8192: 1024 x 8, c1 accumulators in LDS, resident item loop) finish a single workgroup sooner --
            // 0.052-0.055 ms against 0.062-0.070 for up to 256 workgroups (profiles/r06_l_f64_ks_modes.jsonl,
            // r06_m_f64_ks_modes_grid.jsonl) -- so the 512-thread instance is taken from the second workgroup per CU on.
            constexpr int F64_TT = LOGN == 13 ? (1 << LOGN) / 16 : 0;
            const bool two_per_cu = F64_TT != 0 && npolys * kc.L > (size_t)device_cus(kc.device);
            constexpr int GMV = k::KS_GMAX;   // radix-8 passes at every size: one-word twiddles leave the N = 16384 tile room
            with_row_kind<LOGN>(false, hr, [&](auto, auto h) {
                constexpr int HR = decltype(h)::value;
                if constexpr (HR != 0)
                    with_bool(gal != 0, [&](auto galv) {
                        with_bool(two_per_cu, [&](auto two) {
                            constexpr int TTV = decltype(two)::value ? F64_TT : 0;
                            launch("key_switch_fused_f64",
                                   kernel_c<k::ks_fused_kernel<LOGN, false, GMV, TTV, true, 0, decltype(galv)::value, HR>>{},
                                   TTV ? items : ks_grid, k::ks_threads_tt(LOGN, TTV), TTV ? lds_tile : lds, true);
                        });
                    });
            });
            return;
        }
    }
    if constexpr (LOGN < 12) require(!gal, E_ARG, "folded Galois substitution below N = 4096");
    // the integer instances with GM = gm
    auto launch_gm = [&](auto gm) {
        with_bool(narrow, [&](auto nw) {
            with_bool(rns, [&](auto r) {
                with_bool(gal != 0, [&](auto g) {
                    // (RNS: see `rns` above; the Galois instances exist from N = 4096 on: galois_apply folds the
                    // substitution only there)
                    constexpr bool RNS = decltype(r)::value && (LOGN == 12 || LOGN == 13);
                    constexpr bool GALV = decltype(g)::value && LOGN >= 12;
                    launch("key_switch_fused",
                           kernel_c<k::ks_fused_kernel<LOGN, decltype(nw)::value, decltype(gm)::value, 0, RNS, 0, GALV>>{},
                           ks_grid, k::ks_threads_c(LOGN), lds, false);
                });
            });
        });
    };
    // N = 16384 (ks_fused_kernel's GM): radix-8 while the twiddles are scalar, radix-4 after (GM_MIXED; radix-8 throughout
    // spills 24 VGPRs).  (radix-4 passes at N = 8192 measured slower: 0.559 vs 0.532 ms per launch)
    if constexpr (LOGN == 14) launch_gm(int_c<k::GM_MIXED>{});
    else launch_gm(int_c<k::KS_GMAX>{});
}

// ---- unfused key switch (kernels_ks.hpp: ks_ntt_kernel + ks_mac_kernel) ----
// Default W budget.  Measured (profiles/r04_ks_unfused_ab.txt): keeping W on-die does not pay -- launch pairs cut to
// 64 ... 256 MiB of W run 8-30 % slower than one pair over the whole batch (the cut launches are small, and stage B
// streams at 3.4 TB/s either way) -- so the budget only bounds the scratch block.
constexpr size_t KS_W_BUDGET_DEFAULT = (size_t)4 << 30;
// Which shapes take the unfused path when the handle says KS_AUTO.  Measured on the MI355X, same process, alternating
// (profiles/r04_ks_unfused_ab.txt; key-switch kernel time per launch, fused vs unfused stage A + stage B):
//   C5  N = 32768, 16 moduli, 16 polynomials   1.198 ms   vs 0.809 + 0.345 = 1.154 ms   (inside the multiply: 3.25 vs 3.33 ms per step)
//   C5  the same, 64 polynomials                4.713 ms   vs 3.396 + 1.308 = 4.704 ms
//   C3  N = 16384,  8 moduli, 512 polynomials   3.545 ms   vs 2.802 + 1.492 = 4.294 ms   (8192-point tiles: 3.34 + 1.46)
//   C2  N =  8192,  4 moduli, 1024 polynomials  0.831 ms   vs 0.553 + 0.420 = 0.973 ms
// Stage A runs at the NTT kernels' rate (20 M 8192-point tiles/s with the two folded stages, 26 M without), but W
// -- L * Lk rows per polynomial, 1 GiB at C5 / 16 -- costs stage B what the transforms gained: a tie at N = 32768, a
// loss below (and since the fused kernel takes rows larger than LDS as 16384-point parts, a loss at N = 32768 too: 1.08 vs
// 1.23 ms, profiles/r04_final3_ks_modes_ab_c5.jsonl).  For launches that FILL the device KS_AUTO therefore stays on the
// fused kernels at every size.
// Launches that do not are the opposite regime (profiles/r04_ks_small_batches_all_modes.txt): a fused launch has
// batch x key moduli workgroups, each walking its digits one after the other, so its time is one workgroup's whatever the
// batch -- 0.054 ms at C2, 0.22 ms at C3, 0.52 / 0.32 ms at C5 -- while stage A of the unfused form has digits x more
// tiles and fills the device from a single ciphertext on: C3 batch 1 0.220 -> 0.055 ms, batch 16 0.225 -> 0.155; C5 batch 1
// 0.32 -> 0.12 ms; C2 batch 1 0.054 -> 0.030, batch 32 0.063 -> 0.054.  The crossover sits between 128 and 256 fused
// workgroups at every size measured (N = 4096 ... 32768): KS_AUTO takes the unfused form while 2 x workgroups <= compute
// units (at least three digits, N >= 4096: below that the second launch costs what the parallelism gains).  Round 5
// refines the rule by the fused launch's LAST round of workgroups: see the end of ks_use_unfused.
inline bool ks_use_unfused(const Ksk &k_, int mode, size_t npolys) {
    if (k_.log_base != 0) return false;                 // base-2^k digits of one row: the fused loader extracts them
    if (mode == KS_UNFUSED || mode == KS_UNFUSED_SUB) return true;
    if (mode == KS_FUSED || mode == KS_FUSED_SUB) return false;
    const Ctx &kc = *k_.ksk_ctx;
    if (kc.logn < 12 || k_.ndigits < 3) return false;
    const size_t fused_wg = (npolys * kc.L) << (kc.logn > 14 ? kc.logn - 14 : 0);
    const size_t cus = (size_t)device_cus(kc.device);
    // (rows larger than LDS with short digit loops: the 8192-point fused sub-blocks take over earlier -- N = 32768, 4
    // moduli: 96 parts 0.093 vs 0.092 ms, 128 parts 0.112 vs 0.101; profiles/r04_final5_ks_small_launch_ab.jsonl)
    if (kc.logn > 14 && k_.ndigits < 8) return 8 * fused_wg < 3 * cus;
    // Round 5 (profiles/r05_ks_small_launch_stock.jsonl, r05_ks_rounds12_ab.jsonl): the fused kernels have ONE workgroup
    // per CU from N = 8192 on, so a fused launch's time is a step function of its rounds of workgroups, while the unfused
    // form's grows with the work.  (a) N = 4096 (two workgroups per CU, three short digits): unfused only up to a fifth of
    // the CUs' worth (3 moduli: 48 workgroups 0.0310 vs 0.0311 ms, 72: 0.0330 vs 0.0319).  (b) Less than 0.6 of one round
    // (was 0.5; 9 moduli at N = 16384, 144 workgroups: 0.217 vs 0.267 ms).  (c) One or two full rounds and a last round at
    // most half full: 288 / 320 / 384 workgroups at C2 0.095 / 0.105 / 0.115 vs 0.113 / 0.114 / 0.117 ms, at C3 0.349 /
    // 0.382 / 0.443 vs 0.461 / 0.465 / 0.479, at C5 (320 / 384 parts) 0.834 / 0.967 vs 1.040 / 1.045; 576: 0.669 vs 0.727
    // (C3), 1.440 vs 1.562 (C5); with the last round more than half full the fused kernel is ahead again (448: 0.120 vs 0.128).
    if (kc.logn == 12) return 5 * fused_wg <= cus;
    const size_t full = fused_wg / cus, rem = fused_wg % cus;
    // Round 6, the F64 instances (profiles/r06_m_f64_ks_modes_grid.jsonl, r06_n_f64_ks_modes_grid_after.jsonl,
    // r06_p_f64_ks_modes_grid_two_geometries.jsonl; stock sets, relinearise of 8 ... 1,024): their fused kernels are ahead of
    // the integer ones by more than their stage A is, so the windows after a full round shrink.  Below one round nothing
    // changes (N = 8192, 1024-thread instance: 140 workgroups 0.0542 vs 0.0567 ms, 160: 0.0574 vs 0.0571, 255: 0.0754 vs
    // 0.0639; N = 16384: 144: 0.160 vs 0.172, 180: 0.192 vs 0.173).  N = 8192 from the second workgroup per CU on (512-thread
    // instance; a CU's second workgroup costs it ~0.7 of the first, so the steps stay one per CUs' worth): unfused up to 4/9 of
    // the round after the first (320: 0.0926 vs 0.0989; 360: 0.0976 vs 0.1001; 400: 0.1104 vs 0.1018); N = 16384: up to a
    // quarter (288: 0.306 vs 0.336; 360: 0.377 vs 0.354); never after two (560 at N = 8192: 0.157 vs 0.145; 576 at N = 16384:
    // 0.598 vs 0.536).
    if (kc.logn <= 14 && k_.c0f.p && kc.f64_class(0, kc.L)) {
        if (5 * fused_wg <= 3 * cus) return true;
        return full == 1 && rem > 0 && (kc.logn == 13 ? 9 * rem <= 4 * cus : 4 * rem <= cus);
    }
    if (5 * fused_wg <= 3 * cus) return true;
    // (after two full rounds only up to 0.4 of a third: 640 workgroups at C2 0.192 vs 0.182 ms)
    return rem > 0 && ((full == 1 && 2 * rem <= cus) || (full == 2 && 5 * rem <= 2 * cus));
}
// `extra` (optional, G0 == 0): residue rows transformed in place by `extra_grid` more workgroups of the same launch
struct KsExtraFwd {
    u64 *rows = nullptr;      // [npolys][nrows][N], row r under modulus r of the key context, canonical in / out
    u64 poly_stride = 0;
    size_t npolys = 0, nrows = 0;
};
template <int LOGM, int G0>
inline void launch_ks_ntt(const Ksk &k_, bool narrow, bool rns, unsigned grid, hipStream_t s, const u64 *p, u64 p_stride,
                          u64 *w, uint32_t j0, uint32_t jg, uint32_t skip_own, const KsExtraFwd *extra = nullptr) {
    const Ctx &kc = *k_.ksk_ctx;
    const bool with_extra = G0 == 0 && extra != nullptr && extra->rows != nullptr;
    u64 *const erows = with_extra ? extra->rows : nullptr;
    const u64 estride = with_extra ? extra->poly_stride : 0;
    const uint32_t enr = with_extra ? (uint32_t)extra->nrows : 1u;
    const size_t egrid = with_extra ? extra->npolys * extra->nrows : 0;
    auto launch = [&](const char *name, auto kernel, const k::u64x2 *tw) {
        launch_tile<decltype(kernel)::value>(name, LOGM, grid + egrid, s, p, p_stride, w, kc.dmods(), tw, (uint32_t)k_.ndigits, j0,
                                             jg, k_.digit_arg(), skip_own, erows, estride, enr, (uint32_t)grid);
    };
    // Round 6: RNS digits under key moduli that are all below 2^50 -> the F64 stage A (whole-row tiles of 4096 ... 16384
    // points; W in canonical words, so stage B is unchanged)
    const int hr = G0 == 0 && k_.log_base == 0 ? kc.f64_rows(0, kc.L) : 0;
    with_row_kind<G0 == 0 ? LOGM : 0>(narrow, hr, [&](auto nw, auto h) {   // (no F64 instances on sub-block tiles)
        constexpr int HR = decltype(h)::value;
        if constexpr (HR != 0)
            launch("ks_digit_ntt_f64", kernel_c<k::ks_ntt_kernel<LOGM, 0, false, true, HR>>{}, kc.dtw_f());
        else
            with_bool(rns, [&](auto r) {   // (the RNS instances exist from N = 4096 on)
                constexpr bool RNS = decltype(r)::value && LOGM >= 12;
                launch("ks_digit_ntt", kernel_c<k::ks_ntt_kernel<LOGM, G0, decltype(nw)::value, RNS>>{}, kc.dtw());
            });
    });
}
// The geometry of an unfused call, stated once for the single-key, keyed and hoisted forms (the Python restatement of the
// cut: chunk_rule in tests/keyed_cases.py).  `items` polynomials or ciphertexts, each `granule` rows of W per digit
// and key modulus (hoist_each_w; 1 otherwise); k_: the key, or the first key of a set (only its key-independent
// fields are read).
//  * Stage A's tile: whole rows up to 16384 points, 8192-point sub-blocks above, and at 16384 on request (sub14_always)
//    or, where the caller allows it (sub14_small), while whole-row tiles would leave half the device idle -- one
//    ciphertext at 8 moduli: 64 rows, 0.0527 vs 0.0556 ms; four: 256 rows, 0.0684 vs 0.0668.
//  * W = [pc][granule][nd][jg][N]: groups of jg key moduli over chunks of pc items, as large as the budget allows
//    (0: KS_W_BUDGET_DEFAULT).  Key-modulus groups are cut first: a group's key slice is then still read once per
//    launch pair.  Equal groups and equal chunks: no small tail launch.
struct KsGeometry {
    uint32_t logm, g0;   // stage A: tiles of 2^logm points, g0 stages folded into the loader
    bool narrow, rns;
    size_t pc, jg;       // items per chunk, key moduli per group
    size_t w_bytes;
};
inline KsGeometry ks_unfused_geometry(const Ksk &k_, size_t items, size_t budget, bool sub14_small, bool sub14_always = false,
                                      size_t granule = 1) {
    const Ctx &kc = *k_.ksk_ctx;
    const size_t nd = k_.ndigits, Lk = kc.L;
    const uint32_t logn = (uint32_t)kc.logn;
    KsGeometry g;
    const bool sub14 = logn == 14 && (sub14_always ||
                                      (sub14_small && 2 * items * granule * nd * Lk <= (size_t)device_cus(kc.device)));
    g.logm = logn > 14 ? 13 : sub14 ? 13 : logn;
    g.g0 = logn - g.logm;
    g.narrow = ks_narrow(kc);
    g.rns = ks_rns(k_);
    if (!budget) budget = KS_W_BUDGET_DEFAULT;
    const size_t row_bytes = granule * kc.n * sizeof(u64);
    size_t pc = items, jg = Lk;
    if (pc * nd * jg * row_bytes > budget) {
        jg = std::max<size_t>(1, budget / (pc * nd * row_bytes));
        if (jg > Lk) jg = Lk;
        if (pc * nd * jg * row_bytes > budget) pc = std::max<size_t>(1, budget / (nd * jg * row_bytes));
    }
    g.jg = (Lk + ((Lk + jg - 1) / jg) - 1) / ((Lk + jg - 1) / jg);
    g.pc = (items + ((items + pc - 1) / pc) - 1) / ((items + pc - 1) / pc);
    g.w_bytes = g.pc * nd * g.jg * row_bytes;
    return g;
}
// Stage A of one (chunk, group): `rows` polynomials (items x granule) from p, key moduli [j0, j0 + njg), into w.
inline void launch_ks_stage_a(const Ksk &k_, const KsGeometry &g, size_t rows, size_t j0, size_t njg, hipStream_t s, const u64 *p,
                              u64 p_stride, u64 *w, uint32_t skip_own, const KsExtraFwd *ride = nullptr) {
    const unsigned grid_a = grid_x((rows * k_.ndigits * njg) << g.g0, "unfused key switch");
    auto stage_a = [&](auto lm, auto g0, const KsExtraFwd *ex) {
        launch_ks_ntt<decltype(lm)::value, decltype(g0)::value>(k_, g.narrow, g.rns, grid_a, s, p, p_stride, w, (uint32_t)j0,
                                                                (uint32_t)njg, skip_own, ex);
    };
    if (g.g0 == 0)
        with_logn<3, 14>(g.logm, "unsupported key-switch row size", [&](auto lm) { stage_a(lm, int_c<0>{}, ride); });
    else if (g.g0 == 1) stage_a(int_c<13>{}, int_c<1>{}, nullptr);
    else if (g.g0 == 2) stage_a(int_c<13>{}, int_c<2>{}, nullptr);
    else stage_a(int_c<13>{}, int_c<3>{}, nullptr);
}
// Blocks of a stage B (kernels_ksmac.hpp: KsMacAt) over njg key moduli x nb polynomials or ciphertexts x `m` of whatever
// else the kernel's grid runs over: key ranges in eights.
inline unsigned ks_grid_b(const Ctx &kc, size_t njg, size_t nb, size_t m = 1, const char *what = "unfused key switch") {
    return grid_x((((njg * k::ks_mac_chunks_per_row(kc.n)) + 7) / 8) * nb * m * 8, what, "; lower the W budget");
}
// Extra residue rows (KsExtraFwd) that do not ride on a stage-A launch: their own forward transform, in place
inline void ks_extra_forward(const Ctx &kc, const KsExtraFwd &extra, hipStream_t s) {
    const k::RowMap m = strided_map(kc, extra.nrows, extra.poly_stride, extra.poly_stride);
    launch_ntt(kc, false, extra.rows, extra.rows, m, extra.npolys, s);
}
inline unsigned hoist_grid_b(const Ctx &kc, size_t njg, size_t nb, size_t m) { return ks_grid_b(kc, njg, nb, m, "hoisted rotations"); }
inline void key_switch_polys_unfused(const Ksk &k_, int mode, const u64 *p, u64 p_stride, u64 *o0, u64 *o1,
                                     u64 out_stride, const u64 *a0, const u64 *a1, u64 a_stride, size_t npolys,
                                     hipStream_t s, const u64 *xhat, u64 xhat_stride, uint32_t gal,
                                     const KsExtraFwd *extra = nullptr) {
    const Ctx &kc = *k_.ksk_ctx;
    const size_t nd = k_.ndigits, Lk = kc.L;
    const uint32_t logn = (uint32_t)kc.logn;
    // (with extra rows to transform in the same launch -- bfv_mul's c0, c1 -- whole-row tiles: saving that launch is worth
    // more than the smaller tiles, 21 us against 3 us at one ciphertext)
    const KsGeometry g = ks_unfused_geometry(k_, npolys, k_.w_budget.load(std::memory_order_relaxed), mode == KS_AUTO && !extra,
                                             mode == KS_UNFUSED_SUB);
    WsGuard w(g.w_bytes, s);
    const uint32_t skip_own = xhat != nullptr ? 1u : 0u;
    // the extra rows ride on the stage-A launch only when there is exactly one (whole-row tiles, one chunk of polynomials,
    // one group of key moduli); otherwise they get their own forward transform first, as before
    const bool merge_extra = extra != nullptr && g.g0 == 0 && g.logm == logn && g.pc == npolys && g.jg == Lk;
    if (extra != nullptr && !merge_extra) ks_extra_forward(kc, *extra, s);
    const KsExtraFwd *ride = merge_extra ? extra : nullptr;
    for (size_t b0 = 0; b0 < npolys; b0 += g.pc) {
        const size_t nb = std::min(g.pc, npolys - b0);
        for (size_t j0 = 0; j0 < Lk; j0 += g.jg) {
            const size_t njg = std::min(g.jg, Lk - j0);
            launch_ks_stage_a(k_, g, nb, j0, njg, s, p + b0 * p_stride, p_stride, w.u(), skip_own, ride);
            const unsigned grid_b = ks_grid_b(kc, njg, nb);
            FHE_LAUNCH("ks_mac", k::ks_mac_kernel, dim3(grid_b), dim3(256), 0, s, w.u(), o0 + b0 * out_stride,
                       o1 + b0 * out_stride, out_stride, a0 ? a0 + b0 * a_stride : nullptr, a1 ? a1 + b0 * a_stride : nullptr,
                       a_stride, k_.c0.p, k_.c1.p, kc.dmods(), (uint32_t)nd, (uint32_t)Lk, (uint32_t)j0, (uint32_t)njg, logn,
                       xhat ? xhat + b0 * xhat_stride : nullptr, xhat_stride, (uint32_t)nb, gal);
        }
    }
}

// The keyed form (KskSet, kernels_kskeyed.hpp): key_switch_polys_unfused with ks_mac_keyed_kernel as its stage B, on the
// same geometry (no extra rows here) and the same stage A, which reads only the key-independent fields of the first
// key.  Each stage-B launch is told the index of its first polynomial within the call, so a chunk of polynomials need
// not end on a key boundary.
inline void key_switch_polys_keyed(const KskSet &set, size_t per_key, const u64 *p, u64 p_stride, u64 *o0, u64 *o1,
                                   u64 out_stride, const u64 *a0, const u64 *a1, u64 a_stride, size_t npolys,
                                   hipStream_t s, const u64 *xhat, u64 xhat_stride, uint32_t gal) {
    const Ksk &k_ = *set.keys[0];
    const Ctx &kc = *set.ksk_ctx;
    kc.need_device();
    require(per_key > 0, E_ARG, "keyed batches: at least one polynomial per key");
    if (!npolys) return;
    const size_t nd = set.ndigits, Lk = kc.L, nkeys = set.keys.size();
    const KsGeometry g = ks_unfused_geometry(k_, npolys, set.w_budget.load(std::memory_order_relaxed), true);
    WsGuard w(g.w_bytes, s);
    const uint32_t skip_own = xhat != nullptr ? 1u : 0u;
    for (size_t b0 = 0; b0 < npolys; b0 += g.pc) {
        const size_t nb = std::min(g.pc, npolys - b0);
        for (size_t j0 = 0; j0 < Lk; j0 += g.jg) {
            const size_t njg = std::min(g.jg, Lk - j0);
            launch_ks_stage_a(k_, g, nb, j0, njg, s, p + b0 * p_stride, p_stride, w.u(), skip_own);
            const unsigned grid_b = ks_grid_b(kc, njg, nb);
            FHE_LAUNCH("ks_mac_keyed", k::ks_mac_keyed_kernel, dim3(grid_b), dim3(256), 0, s, w.u(),
                       o0 + b0 * out_stride, o1 + b0 * out_stride, out_stride, a0 ? a0 + b0 * a_stride : nullptr,
                       a1 ? a1 + b0 * a_stride : nullptr, a_stride, set.table.p, (uint32_t)nkeys, (uint32_t)per_key, (uint32_t)b0,
                       kc.dmods(), (uint32_t)nd, (uint32_t)Lk, (uint32_t)j0, (uint32_t)njg, (uint32_t)kc.logn,
                       xhat ? xhat + b0 * xhat_stride : nullptr, xhat_stride, (uint32_t)nb, gal);
        }
    }
}

// KeySwitchingKey::key_switch (:241-320): p [npolys][L][N] PowerBasis (poly stride p_stride) ->
// o0,o1 [npolys][Lk][N] Ntt over ksk_ctx (poly stride out_stride).  If a0/a1 are given (and the
// key lives at the ciphertext level) the result is added to them on the fly.
// xhat (optional, poly stride xhat_stride): the same polynomials in Ntt form, when the caller has them (it
// produced p by an inverse transform): row j of xhat is digit j's transform under key modulus j, which the
// kernels then read instead of recomputing (L of the L * Lk transforms).
// gal != 0 (galois_apply): `xhat` and `a0` are the caller's UNPERMUTED Ntt rows, read through the substitution
// x -> x^gal inside the kernels (needs xhat; a1 must be null).
// extra (optional): residue rows over the key context to be forward-transformed IN PLACE before the sums are formed
// (bfv_mul's c0, c1, which are also a0 / a1): they ride on the unfused form's stage-A launch when that is one launch,
// and get their own launch otherwise.
inline void key_switch_polys(const Ksk &k_, const u64 *p, u64 p_stride, u64 *o0, u64 *o1, u64 out_stride,
                             const u64 *a0, const u64 *a1, u64 a_stride, size_t npolys, hipStream_t s,
                             const u64 *xhat = nullptr, u64 xhat_stride = 0, uint32_t gal = 0,
                             const KsExtraFwd *extra = nullptr, const KsKeyed *keyed = nullptr) {
    require(!gal || (xhat != nullptr && a1 == nullptr), E_ARG, "galois key switch: needs the Ntt rows, adds to c0 only");
    if (keyed != nullptr) {   // one key per group of polynomials: `k_` is the set's first key
        require(extra == nullptr, E_ARG, "keyed batches take no extra rows");
        key_switch_polys_keyed(*keyed->set, keyed->per_key, p, p_stride, o0, o1, out_stride, a0, a1, a_stride, npolys, s, xhat,
                               xhat_stride, gal);
        return;
    }
    const Ctx &kc = *k_.ksk_ctx;
    kc.need_device();
    if (!npolys) return;
    {
        const int mode = k_.mode.load(std::memory_order_relaxed);
        if (ks_use_unfused(k_, mode, npolys)) {
            key_switch_polys_unfused(k_, mode, p, p_stride, o0, o1, out_stride, a0, a1, a_stride, npolys, s, xhat, xhat_stride, gal,
                                     extra);
            return;
        }
    }
    if (extra != nullptr && extra->rows != nullptr) ks_extra_forward(kc, *extra, s);   // (a fused launch: their transform is its own)
    if (kc.logn <= 14) {   // rows that fit LDS: the whole-row kernel
        with_logn<3, 14>(kc.logn, "unsupported key-switch row size", [&](auto ln) {
            launch_ks_fused<decltype(ln)::value>(k_, p, p_stride, o0, o1, out_stride, a0, a1, a_stride, npolys, s, xhat, xhat_stride,
                                                 gal);
        });
        return;
    }
    // Rows larger than LDS (N >= 32768): one workgroup per part of a row, the first stages folded into its loader.
    const bool narrow = ks_narrow(kc);
    // N = 32768 / 65536 as two / four 16384-point parts on the N = 16384 kernel (one / two folded stages; the RNS
    // loader where the key's digits are residue rows, the generic loader otherwise) -- 15 % ahead of the
    // 8192-point sub-blocks below once a launch fills the device (profiles/r04_ks_half15_ab.txt).  A launch whose
    // 8192-point sub-blocks all fit the device at once (one workgroup per CU) is a different regime: its time is ONE
    // workgroup's, and a 16384-point part takes 1.7 x as long as an 8192-point one (N = 65536, 4 moduli, 8 polynomials:
    // 128 parts 0.158 ms, 256 sub-blocks 0.129 ms, profiles/r04_final3_n65536_ab.jsonl) -- KS_AUTO takes the small tiles
    // there; KS_FUSED / KS_FUSED_SUB force either form.
    const int ks_mode = k_.mode.load(std::memory_order_relaxed);
    const bool fits_at_once = ((npolys * kc.L) << (kc.logn - 13)) <= (size_t)device_cus(kc.device);
    const bool parts16k = ks_mode != KS_FUSED_SUB && (ks_mode == KS_FUSED || !fits_at_once);
    if ((kc.logn == 15 || kc.logn == 16) && parts16k) {
        const size_t lds_ = k::lds_words(1u << 14) * sizeof(u64);
        const unsigned grid = grid_x((npolys * kc.L) << (kc.logn - 14), "key switch");
        const bool rns = ks_rns(k_);
        with_bool(kc.logn == 15, [&](auto one) {
            with_bool(narrow, [&](auto nw) {
                with_bool(rns, [&](auto r) {
                    with_bool(gal != 0, [&](auto g) {
                        constexpr int G0 = decltype(one)::value ? 1 : 2;
                        launch_k<k::ks_fused_kernel<14, decltype(nw)::value, k::GM_MIXED, 0, decltype(r)::value, G0, decltype(g)::value>>(
                            "key_switch_fused", dim3(grid), dim3(k::ks_threads_c(14)), lds_, s, p, p_stride, o0, o1, out_stride, a0,
                            a1, a_stride, k_.c0.p, k_.c0s.p, k_.c1.p, k_.c1s.p, kc.dmods(), kc.dtw(), (uint32_t)k_.ndigits,
                            (uint32_t)kc.L, k_.digit_arg(), xhat, xhat_stride, grid, gal);
                    });
                });
            });
        });
        return;
    }
    // 8192-point sub-blocks, logn - 13 folded stages (ks_fused_split_kernel; rounds 1-3: every launch)
    auto launch_split = [&](auto g0) {
        constexpr int G0 = decltype(g0)::value, LM = 13;
        const size_t lds_ = (k::lds_words(1u << LM) + ((size_t)1 << LM)) * sizeof(u64);
        with_bool(narrow, [&](auto nw) {
            with_bool(ks_rns(k_), [&](auto r) {
                launch_blocks<k::ks_fused_split_kernel<G0, LM, decltype(nw)::value, decltype(r)::value>>(
                    "key_switch_fused_sub", (npolys * kc.L) << G0, (1u << LM) / 8, lds_, s, p, p_stride, o0,
                    o1, out_stride, a0, a1, a_stride, k_.c0.p, k_.c0s.p, k_.c1.p, k_.c1s.p, kc.dmods(), kc.dtw(),
                    (uint32_t)k_.ndigits, (uint32_t)kc.L, k_.digit_arg(), xhat, xhat_stride, gal);
            });
        });
    };
    with_logn<15, 16>(kc.logn, "unsupported key-switch row size",
                      [&](auto ln) { launch_split(int_c<decltype(ln)::value - 13>{}); });
}

// Poly::<PowerBasis>::switch_down_to (M/rq/mod.rs:498-507): `iters` applications of switch_down.
// in [npolys][from.L][N] (poly stride in_stride) -> out [npolys][from.L - iters][N] (poly stride out_stride), both
// PowerBasis.  Intermediate levels live in one scratch block at a constant stride, updated in place (a lane reads its
// column's rows before it writes them), so `iters` levels cost one scratch block whatever `iters` is.
inline void switch_down_to_pb(const Ctx &from, size_t iters, const u64 *in, u64 in_stride, u64 *out, u64 out_stride,
                              size_t npolys, hipStream_t s) {
    from.need_device();
    require(from.at_level(iters) != nullptr, E_NO_MORE_CONTEXT, "NoMoreContext");
    if (!npolys) return;
    if (iters == 0) {
        copy_rows(in, in_stride, out, out_stride, (u64)from.L * from.n, npolys, s);
        return;
    }
    if (iters == 1) {
        switch_down_polys(from, in, in_stride, out, out_stride, npolys, s);
        return;
    }
    const u64 ts = (u64)(from.L - 1) * from.n;
    WsGuard tmp(npolys * ts * sizeof(u64), s);
    const Ctx *c = &from;
    for (size_t i = 0; i < iters; i++, c = c->next.get()) {
        const bool first = i == 0, last = i + 1 == iters;
        switch_down_polys(*c, first ? in : tmp.u(), first ? in_stride : ts, last ? out : tmp.u(), last ? out_stride : ts,
                          npolys, s);
    }
}

// The same for Ntt polys living over `from` (Ciphertext::switch_down / switch_to_level, F/bfv/ciphertext.rs:148-183,
// one part at a time there): in [npolys][from.L][N] Ntt -> out [npolys][from.L-iters][N] Ntt.  The reference goes
// PowerBasis -> switch_down -> Ntt once per level; the Ntt -> PowerBasis -> Ntt round trips between levels are the
// identity on canonical residues, so one inverse transform, `iters` switch_downs and one forward transform give
// the same values.
inline void switch_down_to_ntt(const Ctx &from, size_t iters, const u64 *in, u64 *out, size_t npolys, hipStream_t s) {
    require(from.at_level(iters) != nullptr, E_NO_MORE_CONTEXT, "NoMoreContext");
    if (!npolys) return;
    const Ctx &to = *from.at_level(iters);
    const u64 stride = (u64)from.L * from.n, ostride = (u64)to.L * to.n;
    WsGuard a(npolys * stride * sizeof(u64), s);
    launch_ntt(from, true, in, a.u(), full_map(from, from.L), npolys, s);
    switch_down_to_pb(from, iters, a.u(), stride, out, ostride, npolys, s);
    launch_ntt(to, false, out, out, full_map(to, to.L), npolys, s);
}

// key switch followed by the level fix-up and "+= (a0, a1)" used by relinearise / rotate:
// out0/out1 [npolys][Lct][N] (poly stride out_stride) = a + switch_down_to(key_switch(p), ct_ctx)
inline void key_switch_add(const Ksk &k_, const u64 *p, u64 p_stride, const u64 *a0, const u64 *a1, u64 a_stride,
                           u64 *out0, u64 *out1, u64 out_stride, size_t npolys, hipStream_t s,
                           const u64 *xhat = nullptr, u64 xhat_stride = 0, uint32_t gal = 0,
                           const KsExtraFwd *extra = nullptr, const KsKeyed *keyed = nullptr) {
    const Ctx &kc = *k_.ksk_ctx, &cc = *k_.ct_ctx;
    const long iters = kc.niterations_to(cc);
    if (iters == 0) {
        key_switch_polys(k_, p, p_stride, out0, out1, out_stride, a0, a1, a_stride, npolys, s, xhat, xhat_stride, gal, extra,
                         keyed);
        return;
    }
    require(extra == nullptr, E_ARG, "extra rows ride only on a key switch at the ciphertext's level");
    require(!gal, E_ARG, "the folded Galois substitution needs the key at the ciphertext's level");
    const u64 kstride = (u64)kc.L * kc.n, cstride = (u64)cc.L * cc.n;
    WsGuard r0(npolys * kstride * sizeof(u64), s), r1(npolys * kstride * sizeof(u64), s);
    WsGuard d0(npolys * cstride * sizeof(u64), s), d1(npolys * cstride * sizeof(u64), s);
    key_switch_polys(k_, p, p_stride, r0.u(), r1.u(), kstride, nullptr, nullptr, 0, npolys, s, xhat, xhat_stride, 0, nullptr,
                     keyed);
    switch_down_to_ntt(kc, (size_t)iters, r0.u(), d0.u(), npolys, s);
    switch_down_to_ntt(kc, (size_t)iters, r1.u(), d1.u(), npolys, s);
    // out = a + d  (strided copy of a -- or of d when there is no addend -- then add)
    struct {
        const u64 *a, *d;
        u64 *o;
    } jobs[2] = {{a0, d0.u(), out0}, {a1, d1.u(), out1}};
    for (auto &jb : jobs) {
        if (jb.a) {
            copy_rows(jb.a, a_stride, jb.o, out_stride, cstride, npolys, s);
            for (size_t i = 0; i < npolys; i++) ew_op(cc, jb.o + i * out_stride, jb.d + i * cstride, 1, k::EW_ADD, s);
        } else {
            copy_rows(jb.d, cstride, jb.o, out_stride, cstride, npolys, s);
        }
    }
}

// --------------------------------------------------- PIR / RGSW / inner sum ----
// dot_product_scalar (F/bfv/ops/dot_product.rs:54-180) / rq::dot_product (M/rq/ops.rs:449-570)
inline void dot_product_scalar(const Ctx &c, size_t nparts, size_t count, const u64 *cts, bool cts_shared,
                               const u64 *pts, bool pts_shared, u64 *out, size_t batch, hipStream_t s) {
    c.need_device();
    require(count > 0, E_EMPTY_DOT, "EmptyDotProduct: no operands");
    if (!batch || !nparts) return;
    const u64 pl = (u64)c.L * c.n;
    require(batch <= GRID_YZ_MAX && nparts <= GRID_YZ_MAX, E_ARG, "dot product: batch / parts exceed the grid limits");
    const u64 cstride = cts_shared ? (u64)0 : (u64)count * nparts * pl, pstride = pts_shared ? (u64)0 : (u64)count * pl;
    auto launch = [&](auto kernel, size_t y) {
        launch_rows<decltype(kernel)::value>("dot_product", pl / 2, y, batch, s, cts, cstride, pts, pstride, out, c.dmods(),
                                             c.dpow2(), (uint32_t)nparts, (uint32_t)count, (uint32_t)c.logn, pl);
    };
    if (nparts == 1) launch(kernel_c<k::dot_kernel<1>>{}, 1);
    else launch(kernel_c<k::dot_kernel<2>>{}, (nparts + 1) / 2);   // (two parts per lane, further parts in extra grid rows)
}

// `Ciphertext * Plaintext` (F/bfv/ops/mod.rs:229-257)
inline void mul_plain(const Ctx &c, size_t nparts, const u64 *ct, const u64 *pt, bool pt_shared, u64 *out,
                      size_t batch, hipStream_t s) {
    c.need_device();
    if (!batch || !nparts) return;
    const u64 pl = (u64)c.L * c.n;
    require(batch <= GRID_YZ_MAX && nparts <= GRID_YZ_MAX, E_ARG, "mul_plain: batch / parts exceed the grid limits");
    // (the kernel moves 16 bytes per lane: every device allocator hands out 256-byte aligned blocks and rows are whole
    // multiples of 64 bytes, so only a pointer into the middle of a coefficient pair can fail this)
    require((((uintptr_t)ct | (uintptr_t)pt | (uintptr_t)out) & 15) == 0, E_ARG, "mul_plain: buffers must be 16-byte aligned");
    launch_rows<k::mul_plain_kernel>("mul_plain", pl / 2, 1, batch, s, ct, pt, pt_shared ? (u64)0 : pl, out, c.dmods(),
                                     (uint32_t)nparts, (uint32_t)c.logn, pl);
}

// GaloisKey::relinearize (F/bfv/keys/galois_key.rs:63-86): ct, out [batch][2][L][N] Ntt
// keyed (optional): ciphertext b under key (b / per_key) % nkeys of the set; `ks` is then the set's first key
inline void galois_apply(const Ksk &ks, size_t exponent, const u64 *ct, u64 *out, size_t batch, hipStream_t s,
                         const KsKeyed *keyed = nullptr) {
    const Ctx &cc = *ks.ct_ctx;
    const u64 PL = (u64)cc.L * cc.n;
    if (!batch) return;
    const size_t e = exponent % (2 * cc.n);
    require((e & 1) == 1, E_INVALID_SUBST, "InvalidSubstitutionExponent");
    // Round 5: no separate permutation pass from N = 4096 on when the key sits at the ciphertext's level (every
    // EvaluationKey the reference builds by default; smaller rows keep the copying path and its kernel instances) -- the Ntt-domain substitution is a gather, and its three consumers read through it:
    //   c2 = PowerBasis(substitute(c1))     the inverse transform's loader            (ntt_kernel<true, ..., GATHER>)
    //   digit j under key modulus j         = row j of substitute(c1): the key switch's own-row read
    //   out0 = key_switch0 + substitute(c0) the key switch's addend read              (galois_key.rs:66-79)
    // (before: substitute_kernel wrote both permuted parts -- 2 polynomials out, 3 row sets read back: 9 % of a rotation)
    // (the consumers gather from `ct` while `out` is being written: a caller that rotates in place takes the copying path)
    const bool overlap = out < ct + batch * 2 * PL && ct < out + batch * 2 * PL;
    if (cc.logn >= 12 && ks.ksk_ctx->niterations_to(cc) == 0 && !overlap) {
        WsGuard c2(batch * PL * sizeof(u64), s);
        k::RowMap m = strided_map(cc, cc.L, 2 * PL, PL);
        m.subst_exp = (uint32_t)e;
        launch_ntt(cc, true, ct + PL, c2.u(), m, batch, s);
        key_switch_add(ks, c2.u(), PL, ct, nullptr, 2 * PL, out, out + PL, 2 * PL, batch, s, ct + PL, 2 * PL, (uint32_t)e,
                       nullptr, keyed);
        return;
    }
    // substitute both parts at once: sub [b][2][L][N]; c2 = PowerBasis(substitute(c1))
    WsGuard sub(batch * 2 * PL * sizeof(u64), s), c2(batch * PL * sizeof(u64), s);
    substitute_polys(cc, exponent, ct, sub.u(), batch * 2, true, s);
    launch_ntt(cc, true, sub.u() + PL, c2.u(), strided_map(cc, cc.L, 2 * PL, PL), batch, s);
    // out0 = key_switch0 + substitute(c0) ; out1 = key_switch1   (galois_key.rs:66-79)
    // (substitute(c1) in Ntt form doubles as the transforms of digit j under key modulus j)
    key_switch_add(ks, c2.u(), PL, sub.u(), nullptr, 2 * PL, out, out + PL, 2 * PL, batch, s, sub.u() + PL, 2 * PL, 0,
                   nullptr, keyed);
}

// What galois_hoisted, matvec_hoisted and matvec_bsgs share.  hoist_exponents: the refusals of the exponent list and the
// level, the exponents reduced mod 2N.  hoist_exps_arg: exponents [r0, r0 + nr) as a kernel argument (nothing is
// uploaded).  hoist_each_w: one inverse transform of c1 (no substitution), then the unfused geometry
// (ks_unfused_geometry: chunks of ciphertexts, groups of key moduli) and ONE stage A per (chunk, group);
// stage_b(b0, nb, j0, njg, w) then runs on that W.
// `granule` (matvec_bsgs's giant pass): every ciphertext of the batch stands for `granule` items, `ct` holding the batch x
// granule 2-part polynomial pairs ciphertext-major, and a chunk holds WHOLE ciphertexts -- W is [nb x granule][nd][jg][N],
// b0 and nb still count ciphertexts.  The budget rule is the same with a ciphertext costing `granule`
// rows per digit and key modulus; where the budget is below one ciphertext's items at one key modulus the chunk is one
// ciphertext (pc = max(1, ...)).  granule = 1: the ciphertexts themselves, what galois_hoisted and matvec_hoisted launch.
// nclients (the keyed forms): the set holds nclients x nrot keys, client-major, and the list has one exponent per rotation.
inline std::vector<uint32_t> hoist_exponents(const KskSet &set, const size_t *exponents, size_t nrot, const std::string &what,
                                             size_t nclients = 1) {
    const Ctx &kc = *set.ksk_ctx, &cc = *set.ct_ctx;
    require(exponents != nullptr, E_ARG, "null argument: exponents");
    if (nclients == 1)
        require(nrot == set.keys.size(), E_ARG, (what + ": one exponent per key of the set").c_str());
    else
        require(nclients != 0 && nrot == set.keys.size() / nclients && nclients * nrot == set.keys.size(), E_ARG,
                (what + ": one exponent per key of a client, clients x exponents keys in the set").c_str());
    std::vector<uint32_t> exps(nrot);
    for (size_t r = 0; r < nrot; r++) {
        exps[r] = (uint32_t)(exponents[r] % (2 * kc.n));
        require((exps[r] & 1) == 1, E_INVALID_SUBST, "InvalidSubstitutionExponent");
    }
    if (kc.niterations_to(cc) != 0)
        throw StatusError(E_ARG, what + ": the keys must sit at the ciphertext's level (" + std::to_string(cc.L) +
                                     " moduli), not above it (" + std::to_string(kc.L) + ")");
    return exps;
}
inline k::HoistExps hoist_exps_arg(const std::vector<uint32_t> &exps, size_t r0, size_t nr) {
    k::HoistExps he{};
    for (size_t r = 0; r < nr; r++) he.e[r] = exps[r0 + r];
    return he;
}
template <class StageB>
inline void hoist_each_w(const KskSet &set, const u64 *ct, size_t batch, hipStream_t s, StageB &&stage_b, size_t granule = 1) {
    const Ksk &k_ = *set.keys[0];
    const Ctx &kc = *set.ksk_ctx, &cc = *set.ct_ctx;
    const size_t Lk = kc.L;
    const u64 PL = (u64)cc.L * kc.n;
    kc.need_device();
    WsGuard c2(batch * granule * PL * sizeof(u64), s);
    launch_ntt(cc, true, ct + PL, c2.u(), strided_map(cc, cc.L, 2 * PL, PL), batch * granule, s);
    const KsGeometry g = ks_unfused_geometry(k_, batch, set.w_budget.load(std::memory_order_relaxed), true, false, granule);
    WsGuard w(g.w_bytes, s);
    for (size_t b0 = 0; b0 < batch; b0 += g.pc) {
        const size_t nb = std::min(g.pc, batch - b0);
        for (size_t j0 = 0; j0 < Lk; j0 += g.jg) {
            const size_t njg = std::min(g.jg, Lk - j0);
            launch_ks_stage_a(k_, g, nb * granule, j0, njg, s, c2.u() + b0 * granule * PL, PL, w.u(), 1u);
            stage_b(b0, nb, j0, njg, w.u());
        }
    }
}
inline void mbfv_sum(const Ctx &c, const u64 *shares, size_t nshares, u64 share_stride, size_t npolys, const u64 *base,
                     u64 base_stride, u64 *out, hipStream_t s);   // (defined with the multiparty protocols below)
// Rotation or giant groups planned ONCE, on the first W -- the largest: chunks and key-modulus groups are equal but for the
// last -- and serving every W, so that the call has ONE number of partial sums and every (ciphertext, key modulus) is
// written in each of them exactly once.  One group in all: the launches write `out` directly.  Otherwise group i writes
// partial sum i, [batch][2][L][N] in wiped workspace, and ONE mbfv_sum_kernel launch (its layout serves: `shares` =
// partial sums, polynomials = batch x 2) adds them into `out` at the end.
struct HoistPartials {
    size_t nparts = 0;
    u64 part_words = 0;
    std::unique_ptr<WsGuard> ws;
    template <class Plan>
    void plan_on_first_w(Plan &&plan, u64 words, hipStream_t s) {   // plan(): the call's number of groups
        if (nparts) return;
        nparts = plan();
        part_words = words;
        if (nparts > 1) ws = std::make_unique<WsGuard>(nparts * part_words * sizeof(u64), s, true);
    }
    u64 *dest(u64 *out, size_t first) const { return nparts > 1 ? ws->u() + first * part_words : out; }   // of group `first`
    void close(const Ctx &cc, size_t batch, u64 *out, hipStream_t s) const {
        if (nparts > 1) mbfv_sum(cc, ws->u(), nparts, part_words, batch * 2, nullptr, 0, out, s);
    }
};

// Hoisted rotations (kernels_kshoist.hpp; not in the reference, whose words this does NOT reproduce except at exponent
// 1 -- the restatement is tests/hoist_ref.py): the Galois elements exponents[r], r < nrot, of each ciphertext under key r
// of `set`, from ONE digit decomposition.  ct [batch][2][L][N] Ntt -> out [batch][nrot][2][L][N] Ntt.
// The transforms and geometry of hoist_each_w, and on each W one hoist_mac_kernel launch per k::HOIST_ROTS rotations.
// Nothing is uploaded: the exponents travel as kernel arguments.  R rotations cost one stage A and R
// multiply-accumulates; a loop of galois_apply pays the transforms R times.
inline void galois_hoisted(const KskSet &set, const size_t *exponents, size_t nrot, const u64 *ct, u64 *out, size_t batch,
                           hipStream_t s) {
    const Ctx &kc = *set.ksk_ctx, &cc = *set.ct_ctx;
    const std::vector<uint32_t> exps = hoist_exponents(set, exponents, nrot, "hoisted rotations");
    if (!batch) return;
    const u64 PL = (u64)cc.L * kc.n;
    require(!(out < ct + batch * 2 * PL && ct < out + batch * nrot * 2 * PL), E_ARG,
            "hoisted rotations: `out` overlaps `ct` (every rotation gathers from the whole input)");
    hoist_each_w(set, ct, batch, s, [&](size_t b0, size_t nb, size_t j0, size_t njg, const u64 *w) {
        for (size_t r0 = 0; r0 < nrot; r0 += k::HOIST_ROTS) {
            const size_t nr = std::min<size_t>(k::HOIST_ROTS, nrot - r0);
            const k::HoistExps he = hoist_exps_arg(exps, r0, nr);
            const unsigned grid_b = hoist_grid_b(kc, njg, nb, nr);
            u64 *o = out + (b0 * nrot + r0) * 2 * PL;
            FHE_LAUNCH("hoist_mac", k::hoist_mac_kernel, dim3(grid_b), dim3(256), 0, s, w, o, o + PL,
                       (u64)nrot * 2 * PL, 2 * PL, ct + b0 * 2 * PL, 2 * PL, set.table.p, (uint32_t)r0, he, kc.dmods(),
                       (uint32_t)set.ndigits, (uint32_t)kc.L, (uint32_t)j0, (uint32_t)njg, (uint32_t)kc.logn,
                       ct + b0 * 2 * PL + PL, 2 * PL, (uint32_t)nb, (uint32_t)nr);
        }
    });
}

// Hoisted rotations with one Galois key set per client (kernels_kshoistkeyed.hpp): `set` holds nclients x nrot keys,
// client-major (entry c * nrot + r: client c's key for exponents[r]); with m = batch / nclients, ciphertexts
// [c m, (c + 1) m) belong to client c.  Word for word galois_hoisted client by client on each client's nrot keys and slice
// of `ct`, in galois_hoisted's launches: stage A reads no key, so hoist_each_w serves as it stands (its b0 is the
// item0 of a launch: a chunk need not end on a client boundary), and on each W one hoist_mac_keyed_kernel launch per
// k::HOIST_ROTS rotations, however many clients there are.
inline void galois_hoisted_keyed(const KskSet &set, size_t nclients, const size_t *exponents, size_t nrot, const u64 *ct, u64 *out,
                                 size_t batch, hipStream_t s) {
    const Ctx &kc = *set.ksk_ctx, &cc = *set.ct_ctx;
    const std::vector<uint32_t> exps = hoist_exponents(set, exponents, nrot, "keyed hoisted rotations", nclients);
    require(batch % nclients == 0, E_ARG, "keyed hoisted rotations: the batch is a multiple of the clients");
    if (!batch) return;
    const size_t per_client = batch / nclients;
    const u64 PL = (u64)cc.L * kc.n;
    require(!(out < ct + batch * 2 * PL && ct < out + batch * nrot * 2 * PL), E_ARG,
            "hoisted rotations: `out` overlaps `ct` (every rotation gathers from the whole input)");
    hoist_each_w(set, ct, batch, s, [&](size_t b0, size_t nb, size_t j0, size_t njg, const u64 *w) {
        for (size_t r0 = 0; r0 < nrot; r0 += k::HOIST_ROTS) {
            const size_t nr = std::min<size_t>(k::HOIST_ROTS, nrot - r0);
            const k::HoistExps he = hoist_exps_arg(exps, r0, nr);
            const unsigned grid_b = hoist_grid_b(kc, njg, nb, nr);
            u64 *o = out + (b0 * nrot + r0) * 2 * PL;
            FHE_LAUNCH("hoist_mac_keyed", k::hoist_mac_keyed_kernel, dim3(grid_b), dim3(256), 0, s, w, o, o + PL,
                       (u64)nrot * 2 * PL, 2 * PL, ct + b0 * 2 * PL, 2 * PL, set.table.p, (uint32_t)b0, (uint32_t)per_client,
                       (uint32_t)nclients, (uint32_t)nrot, (uint32_t)r0, he, kc.dmods(), (uint32_t)set.ndigits, (uint32_t)kc.L,
                       (uint32_t)j0, (uint32_t)njg, (uint32_t)kc.logn, ct + b0 * 2 * PL + PL, 2 * PL, (uint32_t)nb, (uint32_t)nr);
        }
    });
}

// The rotation groups of one hoist_matvec_kernel launch over nr rotations (the ONE statement of the rule).  A block per
// (ciphertext, key range) leaves a small batch short of the device -- batch 1 at N = 8192 x 4 moduli is 64 blocks -- so
// the rotations are cut into groups whose blocks run side by side until the launch has two blocks per compute unit
// (256 lanes a block, four blocks resident on a unit at the kernel's register count: two per unit keep every SIMD busy
// with room for the tail), never into more groups than rotations.  A shape rule in the manner of sub14, no fit to
// timings.  forced != 0 (fhe_kskset_set_rot_split): that many groups, clamped likewise.  Returns rotations per group;
// the groups are ceil(nr / it), so none is empty.
inline size_t hoist_rot_group(const Ctx &kc, size_t forced, size_t nb, size_t njg, size_t nr) {
    const size_t cpr = k::ks_mac_chunks_per_row(kc.n);
    size_t groups = forced;
    if (!groups) {
        const size_t blocks = nb * njg * cpr, want = 2 * (size_t)device_cus(kc.device);
        groups = blocks >= want ? 1 : (want + blocks - 1) / blocks;
    }
    groups = std::min(groups, nr);
    return (nr + groups - 1) / groups;
}
// The giant groups one block of bsgs_baby_kernel<GT> serves (the ONE statement of this rule, hoist_rot_group's twin): a
// larger tile reads every baby key and every row of W once for GT inner sums, and leaves 1 / GT of the blocks.  So: the
// largest instance, no wider than the G groups, whose launch still has two blocks per compute unit; else 1.  A shape
// rule like sub14, no fit to timings.  forced (fhe_kskset_set_bsgs_tile on the BABY set): 1, 2 or 4.
inline size_t bsgs_group_tile(const Ctx &kc, size_t forced, size_t nb, size_t njg, size_t G) {
    if (forced) return forced;
    const size_t cpr = k::ks_mac_chunks_per_row(kc.n);
    const size_t want = 2 * (size_t)device_cus(kc.device);
    for (size_t gt : {(size_t)4, (size_t)2})
        if (gt <= G && nb * njg * cpr * ((G + gt - 1) / gt) >= want) return gt;
    return 1;
}

// Hoisted matrix-vector product (hoist_matvec_kernel; a restatement like galois_hoisted, whose caveat it inherits): the
// diagonal form of a plaintext matrix times an encrypted vector, out = pt0 ct + sum_r pts_r rot_r(ct), in ONE call whose
// only output is the result: word for word galois_hoisted followed by dot_product_scalar over (ct, rotations) and (pt0,
// pts), without the [batch][nrot] block of rotated ciphertexts between them.
// ct [batch][2][L][N] Ntt; pts [nrot][L][N] (pts_shared) or [batch][nrot][L][N]; pt0 NULL, [L][N] or [batch][L][N]; out
// [batch][2][L][N].  galois_hoisted's transforms and geometry (hoist_each_w); on each W one launch per k::HOIST_ROTS
// rotations, each cut into rotation groups (hoist_rot_group).  A call with ONE group in all writes `out` directly.
// Otherwise every group writes a partial [batch][2][L][N] sum into wiped workspace and ONE mbfv_sum_kernel launch (its
// layout serves: `shares` = partial sums, polynomials = batch x 2) adds them into `out` at the end.
inline void matvec_hoisted(const KskSet &set, const size_t *exponents, size_t nrot, const u64 *ct, const u64 *pts,
                           bool pts_shared, const u64 *pt0, u64 *out, size_t batch, hipStream_t s) {
    const Ctx &kc = *set.ksk_ctx, &cc = *set.ct_ctx;
    const std::vector<uint32_t> exps = hoist_exponents(set, exponents, nrot, "hoisted matvec");
    if (!batch) return;
    const u64 PL = (u64)cc.L * kc.n;
    auto overlaps = [&](const u64 *p, u64 words) { return p != nullptr && out < p + words && p < out + batch * 2 * PL; };
    require(!overlaps(ct, batch * 2 * PL), E_ARG,
            "hoisted matvec: `out` overlaps `ct` (every rotation gathers from the whole input)");
    require(!overlaps(pts, (pts_shared ? 1 : batch) * nrot * PL), E_ARG, "hoisted matvec: `out` overlaps `pts`");
    require(!overlaps(pt0, (pts_shared ? 1 : batch) * PL), E_ARG, "hoisted matvec: `out` overlaps `pt0`");
    require((((uintptr_t)ct | (uintptr_t)pts | (uintptr_t)pt0 | (uintptr_t)out) & 15) == 0, E_ARG,
            "hoisted matvec: buffers must be 16-byte aligned");
    const size_t forced = set.rot_split.load(std::memory_order_relaxed);
    // The launches on one W and where their groups' partial sums go (HoistPartials: planned on the first W).
    struct Launch {
        size_t r0, nr, rpg, ngroups, first;   // `first`: index of its group 0 among the call's partial sums
    };
    std::vector<Launch> plan;
    HoistPartials parts;
    hoist_each_w(set, ct, batch, s, [&](size_t b0, size_t nb, size_t j0, size_t njg, const u64 *w) {
        parts.plan_on_first_w([&] {
            size_t total = 0;
            for (size_t r0 = 0; r0 < nrot; r0 += k::HOIST_ROTS) {
                const size_t nr = std::min<size_t>(k::HOIST_ROTS, nrot - r0);
                const size_t rpg = hoist_rot_group(kc, forced, nb, njg, nr);
                const size_t ng = (nr + rpg - 1) / rpg;
                plan.push_back({r0, nr, rpg, ng, total});
                total += ng;
            }
            return total;
        }, (u64)batch * 2 * PL, s);
        for (const Launch &l : plan) {
            const k::HoistExps he = hoist_exps_arg(exps, l.r0, l.nr);
            const unsigned grid_b = hoist_grid_b(kc, njg, nb, l.ngroups);
            u64 *o = parts.dest(out, l.first) + b0 * 2 * PL;
            const u64 *c = ct + b0 * 2 * PL;
            FHE_LAUNCH("hoist_matvec", k::hoist_matvec_kernel, dim3(grid_b), dim3(256), 0, s, w, o, o + PL, 2 * PL,
                       parts.part_words, c, c + PL, 2 * PL, set.table.p, (uint32_t)l.r0, he,
                       pts + (pts_shared ? 0 : b0 * nrot * PL) + l.r0 * PL, pts_shared ? (u64)0 : (u64)nrot * PL, PL,
                       l.r0 == 0 && pt0 ? pt0 + (pts_shared ? 0 : b0 * PL) : nullptr, pts_shared ? (u64)0 : PL, kc.dmods(),
                       (uint32_t)set.ndigits, (uint32_t)kc.L, (uint32_t)j0, (uint32_t)njg, (uint32_t)kc.logn, (uint32_t)nb,
                       (uint32_t)l.nr, (uint32_t)l.rpg, (uint32_t)l.ngroups);
        }
    });
    parts.close(cc, batch, out, s);
}

// Hoisted matrix-vector product with one Galois key set per client (hoist_matvec_keyed_kernel): matvec_hoisted client by
// client on each client's nrot keys and slices of `ct`, `pts` and `pt0`, word for word, in matvec_hoisted's launches -- the
// set and the ownership rule of galois_hoisted_keyed, the layouts, refusals, rotation groups and partial sums of
// matvec_hoisted.  One stage-B launch per W and k::HOIST_ROTS rotations, however many clients there are.
inline void matvec_hoisted_keyed(const KskSet &set, size_t nclients, const size_t *exponents, size_t nrot, const u64 *ct,
                                 const u64 *pts, bool pts_shared, const u64 *pt0, u64 *out, size_t batch, hipStream_t s) {
    const Ctx &kc = *set.ksk_ctx, &cc = *set.ct_ctx;
    const std::vector<uint32_t> exps = hoist_exponents(set, exponents, nrot, "keyed hoisted matvec", nclients);
    require(batch % nclients == 0, E_ARG, "keyed hoisted matvec: the batch is a multiple of the clients");
    if (!batch) return;
    const size_t per_client = batch / nclients;
    const u64 PL = (u64)cc.L * kc.n;
    auto overlaps = [&](const u64 *p, u64 words) { return p != nullptr && out < p + words && p < out + batch * 2 * PL; };
    require(!overlaps(ct, batch * 2 * PL), E_ARG,
            "hoisted matvec: `out` overlaps `ct` (every rotation gathers from the whole input)");
    require(!overlaps(pts, (pts_shared ? 1 : batch) * nrot * PL), E_ARG, "hoisted matvec: `out` overlaps `pts`");
    require(!overlaps(pt0, (pts_shared ? 1 : batch) * PL), E_ARG, "hoisted matvec: `out` overlaps `pt0`");
    require((((uintptr_t)ct | (uintptr_t)pts | (uintptr_t)pt0 | (uintptr_t)out) & 15) == 0, E_ARG,
            "hoisted matvec: buffers must be 16-byte aligned");
    const size_t forced = set.rot_split.load(std::memory_order_relaxed);
    struct Launch {
        size_t r0, nr, rpg, ngroups, first;   // as matvec_hoisted's
    };
    std::vector<Launch> plan;
    HoistPartials parts;
    hoist_each_w(set, ct, batch, s, [&](size_t b0, size_t nb, size_t j0, size_t njg, const u64 *w) {
        parts.plan_on_first_w([&] {
            size_t total = 0;
            for (size_t r0 = 0; r0 < nrot; r0 += k::HOIST_ROTS) {
                const size_t nr = std::min<size_t>(k::HOIST_ROTS, nrot - r0);
                const size_t rpg = hoist_rot_group(kc, forced, nb, njg, nr);
                const size_t ng = (nr + rpg - 1) / rpg;
                plan.push_back({r0, nr, rpg, ng, total});
                total += ng;
            }
            return total;
        }, (u64)batch * 2 * PL, s);
        for (const Launch &l : plan) {
            const k::HoistExps he = hoist_exps_arg(exps, l.r0, l.nr);
            const unsigned grid_b = hoist_grid_b(kc, njg, nb, l.ngroups);
            u64 *o = parts.dest(out, l.first) + b0 * 2 * PL;
            const u64 *c = ct + b0 * 2 * PL;
            FHE_LAUNCH("hoist_matvec_keyed", k::hoist_matvec_keyed_kernel, dim3(grid_b), dim3(256), 0, s, w, o, o + PL, 2 * PL,
                       parts.part_words, c, c + PL, 2 * PL, set.table.p, (uint32_t)b0, (uint32_t)per_client, (uint32_t)nclients,
                       (uint32_t)nrot, (uint32_t)l.r0, he, pts + (pts_shared ? 0 : b0 * nrot * PL) + l.r0 * PL,
                       pts_shared ? (u64)0 : (u64)nrot * PL, PL, l.r0 == 0 && pt0 ? pt0 + (pts_shared ? 0 : b0 * PL) : nullptr,
                       pts_shared ? (u64)0 : PL, kc.dmods(), (uint32_t)set.ndigits, (uint32_t)kc.L, (uint32_t)j0, (uint32_t)njg,
                       (uint32_t)kc.logn, (uint32_t)nb, (uint32_t)l.nr, (uint32_t)l.rpg, (uint32_t)l.ngroups);
        }
    });
    parts.close(cc, batch, out, s);
}

// Baby-step/giant-step hoisted matrix-vector product (kernels_bsgs.hpp; a restatement like its two parents, whose
// caveat it inherits).  G = ngiant + 1 groups of B = nbaby + 1 diagonals, pts [G][B][L][N] (pts_shared) or
// [batch][G][B][L][N]; column 0 of a group is its identity diagonal, row 0 the group without a giant rotation:
//   inner_g = matvec_hoisted(baby, baby_exps, ct, pts[g][1..B), pt0 = pts[g][0])                       g = 0 .. ngiant
//   out     = inner_0 + sum_{g = 1 .. ngiant} galois_hoisted({giant key g - 1}, {giant_exps[g - 1]}, inner_g)
// word for word.  (1) hoist_each_w over `ct` under the baby set's budget: one bsgs_baby_kernel launch per W writes the G
// inner sums into workspace, ciphertext-major: inner_0 into `first` [batch][2][L][N] and inner_1.. into `inner`
// [batch][ngiant][2][L][N] -- apart, so that the items of the giant pass are ONE uniform array and its inverse transform
// one launch ([batch][G] would leave a hole per ciphertext: a launch per ciphertext, measured at 3.8 of 5.5 ms for batch
// 256 at N = 8192).  The tile of groups per block is bsgs_group_tile's.  (2) a second hoist_each_w pass over the ngiant x
// batch items of `inner` under the giant set's budget and geometry, with the ciphertext as the item granule, and one
// bsgs_giant_kernel launch per W; the giants are cut into groups by
// hoist_rot_group (the giant set's rot_split forces it).  A call that is one group writes `out` directly, otherwise the
// groups write partial sums into wiped workspace and ONE mbfv_sum_kernel launch adds them, as matvec_hoisted does.
// A key table holds k::HOIST_ROTS rotations: at most 65 x 65 diagonals per call.
inline void matvec_bsgs(const KskSet &baby, const size_t *baby_exps, size_t nbaby, const KskSet &giant,
                        const size_t *giant_exps, size_t ngiant, const u64 *ct, const u64 *pts, bool pts_shared, u64 *out,
                        size_t batch, hipStream_t s) {
    const Ctx &kc = *baby.ksk_ctx, &cc = *baby.ct_ctx;
    require(baby.ct_ctx->same_ring(*giant.ct_ctx) && baby.ksk_ctx->same_ring(*giant.ksk_ctx) && baby.ndigits == giant.ndigits &&
                baby.ksk_ctx->device == giant.ksk_ctx->device && baby.ksk_ctx->same_tables(*giant.ksk_ctx, kc.L),
            E_PARAMETER_MISMATCH, "bsgs matvec: the baby and giant sets differ in parameters, levels, device or digit count");
    const std::vector<uint32_t> bexps = hoist_exponents(baby, baby_exps, nbaby, "bsgs matvec (baby set)");
    const std::vector<uint32_t> gexps = hoist_exponents(giant, giant_exps, ngiant, "bsgs matvec (giant set)");
    require(nbaby <= k::HOIST_ROTS && ngiant <= k::HOIST_ROTS, E_ARG,
            "bsgs matvec: at most 64 baby and 64 giant rotations per call (65 x 65 diagonals); split the giants over calls");
    if (!batch) return;
    const size_t G = ngiant + 1, B = nbaby + 1;
    const u64 PL = (u64)cc.L * kc.n;
    auto overlaps = [&](const u64 *p, u64 words) { return out < p + words && p < out + batch * 2 * PL; };
    require(!overlaps(ct, batch * 2 * PL), E_ARG, "bsgs matvec: `out` overlaps `ct`");
    require(!overlaps(pts, (pts_shared ? 1 : batch) * G * B * PL), E_ARG, "bsgs matvec: `out` overlaps `pts`");
    require((((uintptr_t)ct | (uintptr_t)pts | (uintptr_t)out) & 15) == 0, E_ARG, "bsgs matvec: buffers must be 16-byte aligned");
    const size_t tile_forced = baby.bsgs_tile.load(std::memory_order_relaxed);
    const size_t split_forced = giant.rot_split.load(std::memory_order_relaxed);
    const k::HoistExps be = hoist_exps_arg(bexps, 0, nbaby), ge = hoist_exps_arg(gexps, 0, ngiant);
    WsGuard first(batch * 2 * PL * sizeof(u64), s), inner(batch * ngiant * 2 * PL * sizeof(u64), s);
    const u64 IS = (u64)ngiant * 2 * PL;   // words of one ciphertext's inner sums 1 .. ngiant
    hoist_each_w(baby, ct, batch, s, [&](size_t b0, size_t nb, size_t j0, size_t njg, const u64 *w) {
        const size_t gt = bsgs_group_tile(kc, tile_forced, nb, njg, G);
        const size_t ntiles = (G + gt - 1) / gt;
        const unsigned grid_b = hoist_grid_b(kc, njg, nb, ntiles);
        u64 *o = inner.u() + b0 * IS, *f = first.u() + b0 * 2 * PL;
        const u64 *c = ct + b0 * 2 * PL;
        auto launch = [&](auto t) {
            FHE_LAUNCH("bsgs_baby", k::bsgs_baby_kernel<decltype(t)::value>, dim3(grid_b), dim3(256), 0, s, w, f, f + PL,
                       2 * PL, o, o + PL, IS, 2 * PL, c, c + PL, 2 * PL, baby.table.p, be, pts + (pts_shared ? 0 : b0 * G * B * PL),
                       pts_shared ? (u64)0 : (u64)G * B * PL, (u64)B * PL, PL, kc.dmods(), (uint32_t)baby.ndigits, (uint32_t)kc.L,
                       (uint32_t)j0, (uint32_t)njg, (uint32_t)kc.logn, (uint32_t)nb, (uint32_t)nbaby, (uint32_t)G,
                       (uint32_t)ntiles);
        };
        if (gt == 4) launch(int_c<4>{});
        else if (gt == 2) launch(int_c<2>{});
        else launch(int_c<1>{});
    });
    size_t gpg = 0;   // giants per group (HoistPartials: planned on the first W)
    HoistPartials parts;
    hoist_each_w(giant, inner.u(), batch, s, [&](size_t b0, size_t nb, size_t j0, size_t njg, const u64 *w) {
        parts.plan_on_first_w([&] {
            gpg = hoist_rot_group(kc, split_forced, nb, njg, ngiant);
            return (ngiant + gpg - 1) / gpg;
        }, (u64)batch * 2 * PL, s);
        const size_t ngroups = parts.nparts;
        const unsigned grid_b = hoist_grid_b(kc, njg, nb, ngroups);
        u64 *o = parts.dest(out, 0) + b0 * 2 * PL;
        const u64 *in = inner.u() + b0 * IS, *f = first.u() + b0 * 2 * PL;
        FHE_LAUNCH("bsgs_giant", k::bsgs_giant_kernel, dim3(grid_b), dim3(256), 0, s, w, o, o + PL, 2 * PL, parts.part_words,
                   f, f + PL, 2 * PL, in, in + PL, IS, 2 * PL, giant.table.p, ge, kc.dmods(), (uint32_t)giant.ndigits, (uint32_t)kc.L, (uint32_t)j0,
                   (uint32_t)njg, (uint32_t)kc.logn, (uint32_t)nb, (uint32_t)ngiant, (uint32_t)gpg, (uint32_t)ngroups);
    }, ngiant);
    parts.close(cc, batch, out, s);
}

// `&Ciphertext * &RGSWCiphertext` (F/bfv/rgsw_ciphertext.rs:122-156)
inline void rgsw_mul(const Ksk &k0, const Ksk &k1, const u64 *ct, u64 *out, size_t batch, hipStream_t s) {
    const Ctx &cc = *k0.ct_ctx;
    require(k0.ct_ctx->same_ring(*k1.ct_ctx) && k0.ksk_ctx->same_ring(*k0.ct_ctx) &&
                k1.ksk_ctx->same_ring(*k1.ct_ctx),
            E_PARAMETER_MISMATCH, "RGSW: both key-switching keys must live at the ciphertext level");
    cc.need_device();
    if (!batch) return;
    const u64 PL = (u64)cc.L * cc.n;
    WsGuard pb(batch * 2 * PL * sizeof(u64), s), t(batch * 2 * PL * sizeof(u64), s);
    launch_ntt(cc, true, ct, pb.u(), full_map(cc, cc.L), batch * 2, s);   // ct0, ct1 -> PowerBasis
    // (c0, c1) = ksk0.key_switch(ct0);  out = (c0, c1) + ksk1.key_switch(ct1)
    key_switch_polys(k0, pb.u(), 2 * PL, t.u(), t.u() + PL, 2 * PL, nullptr, nullptr, 0, batch, s, ct, 2 * PL);
    key_switch_polys(k1, pb.u() + PL, 2 * PL, out, out + PL, 2 * PL, t.u(), t.u() + PL, 2 * PL, batch, s, ct + PL,
                     2 * PL);
}

// EvaluationKey::computes_inner_sum (F/bfv/keys/evaluation_key.rs:56-100)
// keyed (optional): one set per rotation, keyed[i] next to gks[i] (the set's first key)
inline void inner_sum(const Ksk *const *gks, const size_t *exps, size_t ngk, const u64 *ct, u64 *out, size_t batch,
                      hipStream_t s, const KsKeyed *keyed = nullptr) {
    require(ngk > 0, E_ARG, "inner sum needs at least one Galois key");
    const Ctx &cc = *gks[0]->ct_ctx;
    cc.need_device();
    if (!batch) return;
    const u64 total = (u64)batch * 2 * cc.L * cc.n;
    WsGuard tmp(total * sizeof(u64), s);
    FHE_HIP_CHECK(hipMemcpyAsync(out, ct, total * sizeof(u64), hipMemcpyDeviceToDevice, s));
    for (size_t i = 0; i < ngk; i++) {
        require(gks[i]->ct_ctx->same_ring(cc), E_PARAMETER_MISMATCH, "inner sum: Galois keys of different levels");
        galois_apply(*gks[i], exps[i], out, tmp.u(), batch, s, keyed ? keyed + i : nullptr);
        ew_op(cc, out, tmp.u(), batch * 2, k::EW_ADD, s);
    }
}

// SecretKey::try_decrypt, small-plaintext branch (F/bfv/keys/secret_key.rs:198-247):
// ct [batch][nparts][L][N] Ntt, s_ntt [L][N] -> out [batch][N] in [0, t).
// (the three steps are shared with measure_noise, which lifts the same PowerBasis phase)
inline void check_plain_context(const Scaler &sc) {
    // (deep levels may be shorter than the plaintext context; only q_0 has to agree, :232-234)
    require(sc.to->L >= 1 && sc.to->moduli[0] == sc.from->moduli[0], E_PARAMETER_MISMATCH,
            "the plaintext context must start with the first ciphertext modulus");
}
// c0 + c1 s + c2 s^2 + ... in Ntt form: ph [batch][L][N]  (the ciphertext is the grid's second dimension)
inline void launch_phase(const Ctx &cc, const u64 *s_ntt, const u64 *ct, size_t nparts, u64 *ph, size_t batch, hipStream_t s) {
    const u64 PL = (u64)cc.L * cc.n;
    for_groups(batch, GRID_YZ_MAX, [&](size_t b0, size_t nb) {
        launch_rows<k::phase_kernel>("phase", PL, nb, 1, s, ct + b0 * nparts * PL, s_ntt, ph + b0 * PL, cc.dmods(),
                                     (uint32_t)nparts, (uint32_t)cc.logn, PL);
    });
}
// ... and in PowerBasis
inline void phase_power_basis(const Ctx &cc, const u64 *s_ntt, const u64 *ct, size_t nparts, u64 *ph, size_t batch,
                              hipStream_t s) {
    launch_phase(cc, s_ntt, ct, nparts, ph, batch, s);
    launch_ntt(cc, true, ph, ph, full_map(cc, cc.L), batch, s);
}
// Scaler::scale (t / q) of the PowerBasis phase, then ((d_0 + t) mod q_0) mod t: out [batch][N]
inline void decrypt_tail(const Scaler &sc, u64 t, const u64 *ph, u64 *out, size_t batch, hipStream_t s) {
    const Ctx &cc = *sc.from, &pc = *sc.to;
    const ModConsts tm = make_mod_consts(t);
    WsGuard d(batch * pc.L * cc.n * sizeof(u64), s, true);   // the scaled plaintext: secret-dependent
    scale_polys(sc, ph, d.u(), batch, false, s);
    DevMod q0, tmd;
    static_assert(sizeof(DevMod) == sizeof(ModConsts), "DevMod layout");
    std::memcpy(&q0, &cc.root->mods[0], sizeof(DevMod));  // (host tables live on the chain's root)
    std::memcpy(&tmd, &tm, sizeof(DevMod));
    const u64 total = (u64)batch * cc.n;
    launch_ew<k::decrypt_tail_kernel>("decrypt_tail", total, s, d.u(), (u64)pc.L * cc.n, out, q0, tmd, (uint32_t)cc.logn, total);
}
inline void decrypt(const Scaler &sc, u64 t, const u64 *s_ntt, const u64 *ct, size_t nparts, u64 *out, size_t batch,
                    hipStream_t s) {
    const Ctx &cc = *sc.from;
    cc.need_device();
    require(nparts >= 1, E_ARG, "a ciphertext has at least one part");
    check_plain_context(sc);
    require(!sc.wide_num, E_PARAMETER_MISMATCH, "the scaler's plaintext modulus exceeds 64 bits: use fhe_bfv_decrypt_big_dev");
    if (!batch) return;
    // the phase is secret-dependent: cleared before the block goes back to the pool
    WsGuard ph(batch * (u64)cc.L * cc.n * sizeof(u64), s, true);
    phase_power_basis(cc, s_ntt, ct, nparts, ph.u(), batch, s);
    decrypt_tail(sc, t, ph.u(), out, batch, s);
}

// EvaluationKey::expands (F/bfv/keys/evaluation_key.rs:192-256): ct [batch][2][L][N] ->
// out [size][batch][2][L][N] (slot-major, so that the 2^l * batch ciphertexts a level works on
// are contiguous and go through one batched Galois key switch).
// keyed (optional): one set per level, keyed[l] next to gks[l] (the set's first key), each with batch == nkeys * per_key:
// level l works on 2^l * batch slot-major items, and (item / per_key) % nkeys maps each back to its client.
inline void expand(const Ksk *const *gks, size_t nlevels, const u64 *ct, u64 *out, size_t size, size_t batch,
                   hipStream_t s, const KsKeyed *keyed = nullptr) {
    require(nlevels > 0, E_ARG, "expansion needs at least one Galois key");
    const Ctx &cc = *gks[0]->ct_ctx;
    cc.need_device();
    if (size < 1 || size > cc.n)
        throw StatusError(E_EXPANSION_SIZE,
                          "InvalidExpansionSize: size " + std::to_string(size) + ", degree " + std::to_string(cc.n));
    size_t level = 0;
    while (((size_t)1 << level) < size) level++;
    if (level > nlevels)
        throw StatusError(E_EXPANSION_UNSUPPORTED, "expansion to level " + std::to_string(level) +
                                                       " needs the Galois keys of (N >> l) + 1, l < level");
    if (!batch) return;
    const u64 PL = (u64)cc.L * cc.n, CT = 2 * PL;
    FHE_HIP_CHECK(hipMemcpyAsync(out, ct, batch * CT * sizeof(u64), hipMemcpyDeviceToDevice, s));
    if (level == 0) return;
    for (size_t l = 0; l < level; l++)
        require(gks[l]->ct_ctx->same_ring(cc), E_PARAMETER_MISMATCH, "expansion: Galois keys of different levels");
    // monomials -x^(N - 2^l) in Ntt form (the reference keeps them in the EvaluationKey, :467-474)
    WsGuard mono(level * PL * sizeof(u64), s), sub(((size_t)1 << (level - 1)) * batch * CT * sizeof(u64), s);
    FHE_HIP_CHECK(hipMemsetAsync(mono.u(), 0, level * PL * sizeof(u64), s));
    launch_ew<k::monomial_kernel, 64>("monomial", level * cc.L, s, mono.u(), cc.dmods(), (uint32_t)level, (uint32_t)cc.L,
                                      (uint32_t)cc.logn);
    launch_ntt(cc, false, mono.u(), mono.u(), full_map(cc, cc.L), level, s);
    for (size_t l = 0; l < level; l++) {
        const size_t step = (size_t)1 << l, cnt = step * batch;
        const size_t nhigh = std::min(step, size - step) * batch;
        galois_apply(*gks[l], (cc.n >> l) + 1, out, sub.u(), cnt, s, keyed ? keyed + l : nullptr);
        // (the polynomial is the grid's second dimension; a group's share of the 2 nhigh high polynomials: those after its first)
        for_groups(cnt * 2, GRID_YZ_MAX, [&](size_t r0, size_t nr) {
            const size_t high = std::min(nr, std::max(nhigh * 2, r0) - r0);
            launch_rows<k::expand_step_kernel>("expand_step", PL, nr, 1, s, out + r0 * PL, sub.u() + r0 * PL,
                                               out + step * batch * CT + r0 * PL, mono.u() + l * PL, cc.dmods(), (uint32_t)cc.logn,
                                               PL, (uint32_t)high);
        });
    }
}

// --------------------------------------------------------------------- Multiplicator ----
// Execution options live on the handle (not in process globals): concurrent callers that share a Mul all see the
// same, atomically read values, and a call reads them exactly once on entry.
//   chunk   ciphertext pairs per pipeline pass; 0 = default (equal chunks under a workspace budget)
//   streams 2 (default): the chunks of a multiply alternate between the caller's stream and an internal one
//           (fork / join through events): while one chunk's launch drains, the other chunk's kernels fill the
//           idle workgroup slots, which makes small, cache-friendly chunks affordable (+4.5 % at C2).
//           1: the whole pipeline on the caller's stream (exact per-kernel attribution for profiling).
struct Mul {
    const Scaler *ext_lhs = nullptr, *ext_rhs = nullptr, *down = nullptr;
    const Ksk *rk = nullptr;
    bool mod_switch = false;
    const Ctx *base = nullptr, *mulc = nullptr;
    std::atomic<size_t> chunk{0}, streams{2};
    size_t out_parts() const { return rk ? 2 : 3; }
    size_t out_rows() const { return mod_switch ? base->L - 1 : base->L; }
};
// The internal second stream of a (device, caller stream) pair.  The fork / join events are taken from a pool PER CALL
// (an event that two concurrent callers record and wait on would tie their orderings together); concurrent callers on
// the SAME user stream still share its one internal stream and therefore serialise there, which is all stream order
// promises them anyway.  fhe_stream_destroy / fhe_workspace_trim drop what belongs to a stream that is gone.
class AuxStreams {
public:
    static AuxStreams &get() {
        static AuxStreams a;
        return a;
    }
    // The internal stream that shadows `user` on `device`; the caller holds it until done(device, user).
    // `tag_key`: `user` is not a stream but the address of a static tag (host_sliced's three internal streams).
    // At most CAP user streams keep an internal one: beyond that the least recently used idle entry goes (stream
    // synchronised and destroyed, its scratch blocks freed) -- which is also what eventually collects the entries of
    // user streams that no longer exist (a host's own streams: the engine is never told, and cannot ask, see Workspace).
    hipStream_t stream_for(int device, hipStream_t user, bool tag_key = false) {
        std::vector<std::pair<int, hipStream_t>> victims;
        hipStream_t out;
        {
            std::lock_guard<std::mutex> lk(mu);
            const std::pair<int, hipStream_t> key{device, user};
            Entry &a = reg[key];
            if (!a.aux) {
                // A parked stream of this device first (retire): the runtime multiplexes a process's streams onto a few
                // hardware queues (four by default), assigned round-robin at CREATION -- after a dozen streams have come and
                // gone a new one can land on the caller's own queue, and the two lanes of a multiply then run one after the
                // other (bench.py's legs trim the workspace between configs: after its microbenchmarks' sixteen short-lived
                // streams the stock n = 8192 mul_and_relin fell from 182 k to 165 k ops/s,
                // profiles/r06_x_aux_priority_ab_rejected.jsonl, rows of the `before` build).  A stream that is kept keeps its queue.
                for (auto it = parked.begin(); it != parked.end(); ++it)
                    if (it->first == device) {
                        a.aux = it->second;
                        parked.erase(it);
                        break;
                    }
            }
            if (!a.aux) {
                hipStream_t made = nullptr;
                const hipError_t err = hipStreamCreateWithFlags(&made, hipStreamNonBlocking);
                if (err != hipSuccess) {   // (no half-made entry stays behind: a later eviction would retire a NULL stream)
                    reg.erase(key);
                    throw StatusError(E_HIP, std::string("hipStreamCreateWithFlags: ") + hipGetErrorString(err));
                }
                a.aux = made;
            }
            a.tag_key = tag_key;
            if (!tag_key) a.users++;      // (tag keys are never evicted: their holders do not report back)
            a.last_use = ++tick;
            out = a.aux;
            while (reg.size() > CAP) {
                auto lru = reg.end();
                for (auto it = reg.begin(); it != reg.end(); ++it)
                    if (!it->second.tag_key && it->second.users == 0 && (lru == reg.end() || it->second.last_use < lru->second.last_use))
                        lru = it;
                if (lru == reg.end()) break;
                victims.emplace_back(lru->first.first, lru->second.aux);
                reg.erase(lru);
            }
        }
        retire(victims);
        return out;
    }
    void done(int device, hipStream_t user) {
        std::lock_guard<std::mutex> lk(mu);
        auto it = reg.find({device, user});
        if (it != reg.end() && it->second.users > 0) it->second.users--;
    }
    hipEvent_t take_event() {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (!pool.empty()) {
                hipEvent_t e = pool.back();
                pool.pop_back();
                return e;
            }
        }
        hipEvent_t e;
        FHE_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return e;
    }
    void give_event(hipEvent_t e) {
        std::lock_guard<std::mutex> lk(mu);
        pool.push_back(e);
    }
    // the internal stream that shadows `user` on `device` (device < 0: on any device; all: every internal stream and the
    // pooled events as well) is synchronised and destroyed, and the scratch blocks keyed to it are freed (ADVICE r03:
    // they used to stay in the pool under a handle that no longer existed)
    void drop(int device, hipStream_t user, bool all) {
        std::vector<std::pair<int, hipStream_t>> victims;
        {
            std::lock_guard<std::mutex> lk(mu);
            for (auto it = reg.begin(); it != reg.end();) {
                if (all || ((device < 0 || it->first.first == device) && it->first.second == user)) {
                    if (it->second.aux) victims.emplace_back(it->first.first, it->second.aux);
                    it = reg.erase(it);
                } else {
                    ++it;
                }
            }
            if (all) {
                for (hipEvent_t e : pool) (void)hipEventDestroy(e);
                pool.clear();
            }
        }
        retire(victims);
    }
    size_t count() {
        std::lock_guard<std::mutex> lk(mu);
        return reg.size();
    }
    static constexpr size_t CAP = 32;

private:
    struct Entry {
        hipStream_t aux = nullptr;
        bool tag_key = false;
        unsigned users = 0;
        uint64_t last_use = 0;
    };
    // An internal stream that is no longer wanted: synchronised, its scratch blocks freed -- and the handle PARKED for the
    // next stream_for on its device (at most PARK of them; the rest are destroyed).  A stream holds no device memory.
    void retire(const std::vector<std::pair<int, hipStream_t>> &victims) {
        for (const auto &v : victims) {
            hipStream_t aux = v.second;
            if (!aux) continue;
            (void)hipStreamSynchronize(aux);
            Workspace::get().drop_internal_stream(aux);   // (its work is over: plain frees)
            bool keep = false;
            {
                std::lock_guard<std::mutex> lk(mu);
                if (parked.size() < PARK) {
                    parked.emplace_back(v.first, aux);
                    keep = true;
                }
            }
            if (!keep) (void)hipStreamDestroy(aux);
        }
    }
    static constexpr size_t PARK = 8;
    std::vector<std::pair<int, hipStream_t>> parked;
    std::mutex mu;
    std::map<std::pair<int, hipStream_t>, Entry> reg;
    std::vector<hipEvent_t> pool;
    uint64_t tick = 0;
};

inline void *Workspace::acquire(size_t bytes, hipStream_t s) {
    int dev = 0;
    FHE_HIP_CHECK(hipGetDevice(&dev));
    std::unique_lock<std::mutex> lk(mu);
    Block *best = nullptr;
    for (auto &b : blocks)
        if (!b.in_use && b.device == dev && b.stream == s && b.bytes >= bytes && (!best || b.bytes < best->bytes))
            best = &b;
    if (!best) {
        // growing.  Idle blocks of this (device, stream) that are too small go back to the pool in stream order (the
        // allocation below may reuse their memory, ordered behind whatever still reads them), the limits are
        // enforced, then the new block is taken from the device's pool on this stream.
        for (auto &b : blocks)
            if (!b.in_use && b.device == dev && b.stream == s && b.ptr) free_block_locked(b, true);
        compact_locked();
        enforce_limits_locked(s, dev, bytes);
        Block nb;
        sync_threshold_locked(dev);
        nb.ptr = DevPools::get().alloc(dev, bytes, s, DevPools::SCRATCH);
        nb.bytes = bytes ? bytes : 8;
        nb.stream = s;
        nb.device = dev;
        blocks.push_back(nb);
        best = &blocks.back();
    }
    best->in_use = true;
    best->last_use = ++tick;
    void *const ptr = best->ptr;
    flush_trims(lk);   // (after the new block is taken: it may reuse what the eviction just returned to the pool)
    return ptr;
}

// How a batch is cut into chunks, and whether the chunks alternate between two streams.
// One stream: every launch should cover >> 512 workgroup slots (64-pair chunks are 15 % slower at C2), but beyond
// ~3 GiB of workspace nothing is gained and the step-to-step reuse in the 256 MiB Infinity Cache is lost (chunks of
// 256-512 pairs measured 1.5 % ahead of one 1024-pair chunk): equal chunks under that budget.
// Two streams: while one chunk's launch drains, the other chunk's kernels fill the idle workgroup slots, so small,
// cache-friendly chunks pay: 384 MiB of workspace per chunk (64 pairs at C2: 168.1 k against 163.4-166.9 k ops/s
// for 128-pair chunks, same box; 48 pairs 161.8-163.2 k), but at least 8 pairs (C5, 90 MiB per pair: chunks of 8-12
// 4.46-4.51 k ops/s, chunks of 4 4.31-4.34 k).  Fewer than four such chunks do not overlap enough to pay for the
// smaller launches (C5 at batch 16: 4.04 k in two chunks of 8, 4.14-4.20 k in one chunk): the batch then takes the
// one-stream cut.  (profiles/r02_chunk_sweeps.txt)
struct ChunkPlan {
    size_t chunk;
    bool dual;
};
inline ChunkPlan plan_chunks(const Ctx &base, const Ctx &mulc, size_t batch, size_t chunk_opt, size_t streams_opt) {
    auto nchunks = [&](size_t c) { return (batch + c - 1) / c; };
    if (chunk_opt) {
        const size_t c = std::min(batch, chunk_opt);
        return ChunkPlan{c, streams_opt >= 2 && nchunks(c) >= 2};
    }
    const size_t per_ct = (7 * mulc.L + 7 * base.L) * mulc.n * sizeof(u64);
    auto equal_chunks = [&](size_t budget, size_t min_pairs) {
        const size_t cap = std::max<size_t>(min_pairs, std::min<size_t>(budget / per_ct, 4096));
        const size_t nc = (batch + cap - 1) / cap;
        return (batch + nc - 1) / nc;
    };
    // Round 5 (profiles/r05_plan14_ab.jsonl: same box, alternating builds; r05_chunk_sweep_n16384.jsonl, r05_chunk_sweep_c5.jsonl):
    // at N = 16384 the small-chunk plan below is skipped -- two or three large chunks alternating between the two streams
    // (the 3 GiB cut at the end) run the reference's stock n = 16384 set 6.7 % (256 pairs) / 8.4 % (1,024 pairs) faster and
    // a 12-moduli basis 3.6 %, at the price of 1.0-1.6 % on 4- and 8-moduli bases: at this size every NTT-type kernel is one
    // 1024-thread workgroup per CU and so is the key switch, so small launches are mostly tail (9 digits x 32 pairs = 288
    // key-switch workgroups: one round and an eighth).  N = 8192 (C2, stock n = 8192: unchanged in the same A/B) and
    // N = 32768 (C5 at 32 / 64 / 128 pairs, 8 moduli at 128 pairs: the default plan is the best cell of the sweep) keep it.
    if (streams_opt >= 2 && base.logn != 14) {
        // Two streams: chunks small enough that a chunk's intermediates mostly stay in the 256 MiB Infinity Cache, at
        // least four of them.  Round 3 (profiles/r03_chunk_sweep_event_free.jsonl, C2): 64 ... 256 pairs per chunk are
        // within 1 % of each other, 96 - 128 best at 8,192 pairs -- but 66 pairs (what the 384 MB budget gave there)
        // lost 5 %: 66 * 16 rows is two full rounds of the 512 resident workgroups plus a nearly empty third.  Chunks
        // of 64 pairs or more are therefore cut to a multiple of 32.
        for (const size_t budget : {(size_t)768 << 20, (size_t)384 << 20}) {
            size_t c = equal_chunks(budget, 8);
            if (c >= 64) {
                c = c / 32 * 32;
                // (round 5: rounding down can leave a small ragged last chunk -- 1,024 pairs of the stock n = 4096 set: 342 ->
                // 320 = 320 + 320 + 320 + 64; equal chunks over the same count instead: 4 x 256, profiles/r05_plan_ragged_ab.jsonl)
                const size_t nc = nchunks(c), ce = (batch + nc - 1) / nc;
                if (ce >= 64 && ce % 32 == 0) c = ce;
            }
            if (nchunks(c) >= 4) return ChunkPlan{c, true};
        }
    }
    // (the large cut is taken on up to two lanes, so it is clamped to a quarter of the device's workspace bound
    // per lane -- a host with a tight fhe_workspace_set_limit, or a small device, must not be planned past its own limit)
    size_t total_limit = 0;
    Workspace::get().get_limits(nullptr, &total_limit);
    size_t big = (size_t)3 << 30;
    if (total_limit) big = std::min(big, std::max<size_t>(per_ct, total_limit / 4));
    const size_t c = equal_chunks(big, 1);
    return ChunkPlan{c, streams_opt >= 2 && nchunks(c) >= 2};
}

// Ciphertext::switch_down (F/bfv/ciphertext.rs:148-161): ct [b][nparts][L][N] Ntt -> [b][nparts][L-1][N] Ntt
inline void bfv_switch_down(const Ctx &c, size_t nparts, const u64 *ct, u64 *out, size_t batch, hipStream_t s) {
    c.need_device();
    require(c.next != nullptr, E_NO_MORE_CONTEXT, "NoMoreContext");
    switch_down_to_ntt(c, 1, ct, out, batch * nparts, s);
}

// Multiplicator::multiply (F/bfv/ops/mul.rs:165-243) on `batch` ciphertext pairs.
// `&ct * &ct` with any number of parts (F/bfv/ops/mod.rs:259-358), the generic (unfused) pipeline:
// lhs [batch][la][L][N], rhs [batch][lb][L][N] -> out [batch][la+lb-1][L][N], all Ntt.
inline void bfv_tensor(const Mul &m, size_t la, size_t lb, const u64 *lhs, const u64 *rhs, u64 *out, size_t batch,
                       hipStream_t s) {
    const Ctx &b = *m.base, &e = *m.mulc;
    b.need_device();
    require(la >= 1 && lb >= 1, E_MUL_POLY_COUNT, "a ciphertext has at least one part");
    if (!batch) return;
    const u64 PL = (u64)b.L * b.n, PK = (u64)e.L * e.n;
    const size_t lo = la + lb - 1;
    // bound the workspace like bfv_mul does: chunks of ciphertext pairs
    const size_t per_pair = (la + lb + lo) * PK * sizeof(u64);
    const size_t chunk = std::max<size_t>(1, std::min<size_t>({batch, (size_t)32768, ((size_t)8 << 30) / per_pair}));
    WsGuard ea(chunk * la * PK * sizeof(u64), s), eb(chunk * lb * PK * sizeof(u64), s), ten(chunk * lo * PK * sizeof(u64), s);
    for (size_t b0 = 0; b0 < batch; b0 += chunk) {
        const size_t nb = std::min(chunk, batch - b0);
        scale_polys(*m.ext_lhs, lhs + b0 * la * PL, ea.u(), nb * la, true, s);
        scale_polys(*m.ext_rhs, rhs + b0 * lb * PL, eb.u(), nb * lb, true, s);
        launch_rows<k::tensor_general_kernel>("tensor_general", PK, lo, nb, s, ea.u(), eb.u(), ten.u(), e.dmods(), (uint32_t)la,
                                              (uint32_t)lb, (uint32_t)e.logn, PK);
        scale_polys(*m.down, ten.u(), out + b0 * lo * PL, nb * lo, true, s);
    }
}

// Workspace per chunk of nb pairs (all slot-major so that every step is ONE launch over
// nb * {2,3} polynomials):  extL/extR [nb][2][K][N] extended operands,  ten [3][nb][K][N]
// tensor,  d [3][nb][L][N] down-scaled parts (c0, c1 Ntt; c2 PowerBasis for the key switch).
inline void bfv_mul(const Mul &m, const u64 *lhs, const u64 *rhs, u64 *out, size_t batch, hipStream_t s0) {
    const Ctx &b = *m.base, &e = *m.mulc;
    b.need_device();
    const size_t L = b.L, K = e.L, N = b.n;
    const u64 PL = (u64)L * N, PK = (u64)K * N;
    const size_t parts = m.out_parts();
    if (!batch) return;
    const ChunkPlan plan = plan_chunks(b, e, batch, m.chunk.load(std::memory_order_relaxed),
                                       m.streams.load(std::memory_order_relaxed));
    const size_t chunk = plan.chunk;
    // the extenders copy the shared prefix rows verbatim; when both share all L rows the tensor
    // kernel reads those rows from the inputs directly and the copy is skipped
    const bool skip_copy = m.ext_lhs->ncommon == L && m.ext_rhs->ncommon == L;
    struct ChunkWs {   // (ext: the extended lhs parts of the chunk, then the extended rhs parts)
        WsGuard ext, ten, d, pre;
        ChunkWs(size_t chunk, u64 PK, u64 PL, size_t pre_bytes, hipStream_t st)
            : ext(chunk * 4 * PK * sizeof(u64), st), ten(chunk * 3 * PK * sizeof(u64), st),
              d(chunk * 3 * PL * sizeof(u64), st), pre(pre_bytes, st) {}
    };
    const size_t pre_bytes = m.mod_switch ? chunk * parts * PL * sizeof(u64) : 8;
    const bool dual = plan.dual;
    hipStream_t lanes[2] = {s0, s0};
    struct Join {  // the internal stream always rejoins the caller's, also on an error path
        hipStream_t aux = nullptr, to = nullptr;
        hipEvent_t fork = nullptr, join = nullptr;
        int device = 0;
        ~Join() {
            if (aux && hipEventRecord(join, aux) == hipSuccess) (void)hipStreamWaitEvent(to, join, 0);
            if (aux) AuxStreams::get().done(device, to);
            // (a wait captures the event's state when it is enqueued: both events may be reused right away)
            if (fork) AuxStreams::get().give_event(fork);
            if (join) AuxStreams::get().give_event(join);
        }
    } join;
    // A batch that is ONE chunk has nothing to alternate: there the two operand extensions (independent chains of
    // five launches each: inverse NTT, scaler, forward NTT of the new rows) run side by side, lhs on the caller's
    // stream and rhs on the internal one, and meet again in front of the tensor kernel -- the tail of one chain's
    // launch is filled by the other's (C5 at batch 16: launches of 4.25 waves; profiles/r03_split_ext_ab.txt).
    // Squaring (`&ct * &ct` with both operands the same buffer, the reference's bench ID "square", F/bfv/ops/mod.rs:
    // 259-358): the rhs extension would recompute the lhs one bit for bit, so it is skipped and the tensor kernel
    // reads the one extended operand twice (10 launches -> 7 per chunk; same values by construction).
    const bool square = lhs == rhs && m.ext_lhs == m.ext_rhs;
    // Both operands through the same extender (Multiplicator::default; not the second HPS strategy): the two
    // extensions are ONE pass of three launches over 4 nb polynomials (scale_polys_pair) -- round 4,
    // profiles/r04_merged_ext_ab.txt, r04_merged_ext_dirflags_ab.txt: batch 1024 unchanged, batch 64 -5 %, batch 16
    // -12.5 %.  Otherwise, for a batch that is one chunk, the two extension chains run side by
    // side on the caller's and the internal stream (round 3's split_ext).
    const bool merged_ext = !square && m.ext_lhs == m.ext_rhs;
    const bool split_ext = !dual && !square && !merged_ext && m.streams.load(std::memory_order_relaxed) >= 2 &&
                           batch <= chunk;
    hipEvent_t ext_done = nullptr;
    struct EventBack {
        hipEvent_t &e;
        ~EventBack() {
            if (e) AuxStreams::get().give_event(e);
        }
    } ext_done_back{ext_done};
    if (dual || split_ext) {
        AuxStreams &ax = AuxStreams::get();
        join.to = s0;
        join.fork = ax.take_event();
        join.join = ax.take_event();
        join.device = b.device;
        hipStream_t aux = ax.stream_for(b.device, s0);
        join.aux = aux;   // (from here on ~Join reports the stream back, whatever throws below)
        if (dual) lanes[1] = aux;
        if (split_ext) ext_done = ax.take_event();
        FHE_HIP_CHECK(hipEventRecord(join.fork, s0));
        FHE_HIP_CHECK(hipStreamWaitEvent(aux, join.fork, 0));
    }
    ChunkWs ws0(chunk, PK, PL, pre_bytes, lanes[0]);
    std::unique_ptr<ChunkWs> ws1;
    if (dual) ws1 = std::make_unique<ChunkWs>(chunk, PK, PL, pre_bytes, lanes[1]);
    size_t ci = 0;
    for (size_t b0 = 0; b0 < batch; b0 += chunk, ci++) {
        const size_t nb = std::min(chunk, batch - b0);
        const hipStream_t s = lanes[dual ? ci & 1 : 0];
        ChunkWs &w = (dual && (ci & 1)) ? *ws1 : ws0;
        WsGuard &ten = w.ten, &d = w.d, &pre = w.pre;
        u64 *const extL = w.ext.u(), *const extR = w.ext.u() + nb * 2 * PK;
        const u64 *l = lhs + b0 * 2 * PL, *r = rhs + b0 * 2 * PL;
        // EXTEND (mul.rs:192-195): both parts of every lhs (rhs) ciphertext in one go
        if (merged_ext) {
            scale_polys_pair(*m.ext_lhs, l, r, extL, nb * 2, s, !skip_copy);
        } else {
            scale_polys(*m.ext_lhs, l, extL, nb * 2, true, s, !skip_copy);
            if (square) {
                // (nothing: extR is never read)
            } else if (split_ext) {   // (one chunk: the fork above put the internal stream behind the caller's earlier work)
                scale_polys(*m.ext_rhs, r, extR, nb * 2, true, join.aux, !skip_copy);
                FHE_HIP_CHECK(hipEventRecord(ext_done, join.aux));
                FHE_HIP_CHECK(hipStreamWaitEvent(s, ext_done, 0));
            } else {
                scale_polys(*m.ext_rhs, r, extR, nb * 2, true, s, !skip_copy);
            }
        }
        // TENSOR (mul.rs:198-201) + the inverse NTT of the down-scaler (M/rq/scaler.rs:69-79):
        // ten [3][nb][K][N] ends up in PowerBasis.  Rows that fit LDS: one fused kernel;
        // larger rows: element-wise tensor kernel, then the two-kernel inverse NTT.
        const bool fused_tensor = e.logn <= 16;
        if (fused_tensor) {
            require(nb <= 32768, E_ARG, "chunk too large for the fused tensor kernel");  // 3*K*nb blocks in a 1-D grid
            k::TensorSrc ts{extL, square ? extL : extR, skip_copy ? l : nullptr, skip_copy ? r : nullptr,
                            (uint32_t)L, (uint32_t)L};
            launch_tensor_intt(e, ts, ten.u(), nb, s);
        } else {
            for_groups(nb, 32768, [&](size_t t0, size_t tn) {   // (the pair is the grid's second dimension)
                launch_rows<k::tensor_kernel>("tensor", PK, tn, 1, s, extL + t0 * 2 * PK, (square ? extL : extR) + t0 * 2 * PK,
                                              skip_copy ? l + t0 * 2 * PL : nullptr, skip_copy ? r + t0 * 2 * PL : nullptr,
                                              ten.u() + t0 * PK, e.dmods(), (uint32_t)K, (uint32_t)L, (uint32_t)L,
                                              (uint32_t)e.logn, (u64)nb, 0u);
            });
        }
        if (!fused_tensor) launch_ntt(e, true, ten.u(), ten.u(), full_map(e, K), nb * 3, s);
        u64 *dst = m.mod_switch ? pre.u() : out + b0 * parts * PL;
        // DOWN-SCALE (mul.rs:204-206) to PowerBasis rows of d [3][nb][L][N]
        launch_scale(*m.down, ten.u(), PK, d.u(), PL, nb * 3, s);
        const k::RowMap back = full_map(b, L);
        if (m.rk) {
            // c0, c1 go back to Ntt; c2 stays in PowerBasis for the key switch (the reference
            // transforms c2 forward and, at mul.rs:212, back again; iNTT(NTT(x)) = x exactly).
            // (Transforming c2 as well and handing it to the key switch as `xhat` was measured at C2: the key
            // switch gains 1.0 ms per 10 steps, the larger forward launch costs 1.6: profiles/r02_mul_xhat_ab.txt.)
            // Round 5: when the key switch of this chunk runs unfused (a launch that does not fill the device) and the key
            // sits at the ciphertext's level, the forward transform of (c0, c1) rides on its stage-A launch -- one launch
            // less on the critical path of a small call (C2, one pair: 0.088 -> 0.077 ms, profiles/r05_merged_fwd_ab.jsonl)
            const bool ride = m.rk->ksk_ctx->niterations_to(*m.rk->ct_ctx) == 0 && b.logn <= 14 &&
                              ks_use_unfused(*m.rk, m.rk->mode.load(std::memory_order_relaxed), nb);
            KsExtraFwd ex;
            ex.rows = d.u();
            ex.poly_stride = PL;
            ex.npolys = nb * 2;
            ex.nrows = L;
            if (!ride) launch_ntt(b, false, d.u(), d.u(), back, nb * 2, s);
            // RELINEARIZE (mul.rs:211-227): (c0, c1) += key_switch(c2), written to the output layout
            key_switch_add(*m.rk, d.u() + 2 * nb * PL, PL, d.u(), d.u() + nb * PL, PL, dst, dst + PL, 2 * PL, nb, s, nullptr, 0, 0,
                           ride ? &ex : nullptr);
        } else {
            // no relinearisation: three Ntt parts, slot-major scratch -> [b][3][L][N]
            launch_ntt(b, false, d.u(), d.u(), back, nb * 3, s);
            for (size_t slot = 0; slot < 3; slot++) copy_rows(d.u() + slot * nb * PL, PL, dst + slot * PL, 3 * PL, PL, nb, s);
        }
        if (m.mod_switch) bfv_switch_down(b, parts, pre.u(), out + b0 * parts * (PL - N), nb, s);
    }
}

// ------------------------------------------------------------------- plaintext encoding ----
// The encoding half of bfv::BfvParameters (F/bfv/parameters.rs:598, 607-633, 711-725) on one device: t's NTT operator
// as a one-modulus context (the same tables, DevMod and F64 twins as any modulus), SEAL's index map and its inverse,
// and per level q_mod_t and delta.
struct Encoder {
    const Ctx *top = nullptr;         // the parameter set's level-0 context (the encoder borrows it)
    size_t n = 0, logn = 0;
    u64 t = 0;
    DevMod tm{};                      // t's constants (by value: the Poly path has no transform mod t)
    std::unique_ptr<Ctx> tctx;        // null when t admits no degree-N NTT: SIMD unavailable
    DevBuf<uint32_t> d_map, d_inv_map;
    std::vector<u64> q_mod_t;         // per level (parameters.rs:616-633)
    std::vector<std::unique_ptr<DevBuf<k::u64x2>>> d_delta;   // per level [L] {delta_i, shoup}, delta_i = (-t)^-1 mod q_i
    // The big form (PlaintextModulus::Large, t >= 2^64; encoder_create_big): wt = W_t > 1 limbs, `t` and `tm` unused, no
    // tctx.  t, mu = floor(2^(128 W_t) / t) and the per-level q_mod_t travel to the kernels by value.
    size_t wt = 1;
    BigUint t_big;
    std::vector<u64> mu_big;                    // [wt + 2]
    std::vector<std::vector<u64>> q_mod_t_big;  // per level [wt]
    const Ctx *plain = nullptr;                 // the plaintext context: the level of `top` with the first P moduli
    bool big() const { return wt > 1; }
};

// matrix_reps_index_map (parameters.rs:711-725): generator 3, m = 2N, bit-reversed positions
inline std::vector<uint32_t> simd_index_map(size_t n, size_t logn) {
    std::vector<uint32_t> map(n);
    const u64 m = 2 * (u64)n;
    u64 pos = 1;
    for (size_t i = 0; i < n / 2; i++) {
        map[i] = k::bitrev_n((uint32_t)((pos - 1) >> 1), (uint32_t)logn);
        map[n / 2 + i] = k::bitrev_n((uint32_t)((m - pos - 1) >> 1), (uint32_t)logn);
        pos = (pos * 3) & (m - 1);
    }
    return map;
}

// One level's [L] {delta_i, shoup}, delta_i = (-t)^-1 mod q_i, uploaded; t_mod(q) = t mod q
template <class TMod>
inline void push_delta(Encoder &e, const Ctx &c, TMod &&t_mod) {
    std::vector<k::u64x2> d(c.L);
    for (size_t i = 0; i < c.L; i++) {
        const u64 q = c.moduli[i];
        const u64 neg_t = (q - t_mod(q)) % q;
        require(neg_t != 0, E_INVALID_MODULUS, "the plaintext modulus must be invertible modulo every q_i");
        const u64 inv = powmod(neg_t, q - 2, q);
        d[i] = k::u64x2{inv, shoup(inv, q)};
    }
    e.d_delta.push_back(std::make_unique<DevBuf<k::u64x2>>());
    e.d_delta.back()->upload(d);
}

// `tctx`: the context over {t} (null when t admits no degree-N NTT).
inline std::unique_ptr<Encoder> encoder_create(const Ctx &top, u64 t, std::unique_ptr<Ctx> tctx) {
    top.need_device();
    auto e = std::make_unique<Encoder>();
    e->top = &top;
    e->n = top.n;
    e->logn = top.logn;
    e->t = t;
    const ModConsts tmc = make_mod_consts(t);
    static_assert(sizeof(DevMod) == sizeof(ModConsts), "DevMod layout");
    std::memcpy(&e->tm, &tmc, sizeof(DevMod));
    e->tctx = std::move(tctx);
    if (e->tctx) {
        const std::vector<uint32_t> map = simd_index_map(e->n, e->logn);
        std::vector<uint32_t> inv(e->n);
        for (size_t i = 0; i < e->n; i++) inv[map[i]] = (uint32_t)i;
        e->d_map.upload(map);
        e->d_inv_map.upload(inv);
    }
    for (const Ctx *c = &top; c; c = c->next.get()) {
        u64 qt = 1 % t;
        for (u64 q : c->moduli) qt = mulmod(qt, q % t, t);
        push_delta(*e, *c, [&](u64 q) { return t % q; });
        e->q_mod_t.push_back(qt);
    }
    return e;
}

// {w, shoup(w)} or, for the F64 instances, the double pair {w, w / p} (Ctx's F64 tables)
inline k::u64x2 scale_pair(u64 w, u64 p, bool f64) {
    if (!f64) return k::u64x2{w, shoup(w, p)};
    const double d = (double)w, q = d / (double)p;
    k::u64x2 r;
    std::memcpy(&r.x, &d, 8);
    std::memcpy(&r.y, &q, 8);
    return r;
}

// The encoding, sampling, encryption and key-generation kernels work on whole rows (N <= 16384) through RowLaunch.
// PlaintextVec::try_encode (F/bfv/plaintext_vec.rs:70-102) -> Plaintext::poly_ntt, or with `scaled` Plaintext::to_poly
// (F/bfv/plaintext.rs:172-196): values [batch][nvalues] -> out [batch][L_level][N] Ntt.
inline void encode(const Encoder &e, bool simd, bool scaled, size_t level, const u64 *values, size_t nvalues, u64 *out,
                   size_t batch, hipStream_t s) {
    require(!e.big(), E_PARAMETER_MISMATCH, "the plaintext modulus exceeds 64 bits: use fhe_bfv_encode_big_dev");
    const Ctx *qc = e.top->at_level(level);
    if (!qc) throw StatusError(E_INVALID_LEVEL, "InvalidLevel");
    if (simd && !e.tctx) throw StatusError(E_SIMD_UNAVAILABLE, "SimdUnavailable: the plaintext modulus admits no degree-N NTT");
    if (nvalues > e.n) throw StatusError(E_TOO_MANY_VALUES, "TooManyValues: more values than the degree");
    if (!batch) return;
    grid_x(batch * qc->L, "encode");
    const bool f64_on = !f64_disabled();   // (read once per call: every transform of the call takes the same kind)
    const u64 qmt = e.q_mod_t[level];
    k::LiftSrc ls{values, nvalues, nvalues, e.tm, k::u64x2{qmt, shoup(qmt, e.t)}, scaled ? 1u : 0u,
                  scaled ? e.d_delta[level]->p : nullptr};
    // the mod-t rows of a SIMD encoding are plaintext coefficients: cleared before the block returns to the pool
    // (the reference zeroizes them, plaintext.rs:104, 178)
    std::unique_ptr<WsGuard> trows;
    if (simd) {
        trows = std::make_unique<WsGuard>(batch * e.n * sizeof(u64), s, true);
        const Ctx &tc = *e.tctx;
        if (e.logn <= 14) {
            const RowLaunch rows(tc, 1, f64_on);
            // the inverse transform's N^-1 times q_mod_t for the scaled form (the same value mod t as multiplying after)
            const NttTables &tt = tc.tab(0);
            const u64 c = scaled ? mulmod(tt.size_inv, qmt, e.t) : tt.size_inv;
            const u64 zc = mulmod(tt.zetas_inv[e.n - 2], c, e.t);
            const k::u64x2 ns = scale_pair(c, e.t, rows.f64()), zs = scale_pair(zc, e.t, rows.f64());
            rows("encode_simd_t", batch, s,
                 [](auto lm, auto nrw, auto h) { return kernel_c<k::encode_simd_t_kernel<lm(), nrw(), h()>>{}; },
                 values, (u64)nvalues, e.d_inv_map.p, trows->u(), tc.dmods(), rows.itw(), ns, zs);
            ls.mul_t = 0;
        } else {   // rows larger than one LDS tile: the gather as a pass of its own, then launch_ntt
            const u64 total = (u64)batch * e.n;
            launch_ew<k::perm_reduce_kernel>("encode_gather", total, s, values, (u64)nvalues, (u64)nvalues, e.d_inv_map.p,
                                             trows->u(), e.tm, (uint32_t)e.logn, total);
            launch_ntt(tc, true, trows->u(), trows->u(), full_map(tc, 1), batch, s);
        }
        ls.src = trows->u();
        ls.stride = ls.nvalues = e.n;
    }
    if (qc->logn <= 14) {
        const RowLaunch rows(*qc, qc->L, f64_on);
        rows("encode_lift", batch * qc->L, s,
             [](auto lm, auto nrw, auto h) { return kernel_c<k::encode_lift_kernel<lm(), nrw(), h()>>{}; },
             ls, out, (uint32_t)qc->L, qc->dmods(), rows.tw());
    } else {
        const u64 total = (u64)batch * qc->L * e.n;
        launch_ew<k::encode_lift_ew_kernel>("encode_lift", total, s, ls, out, (uint32_t)qc->L, qc->dmods(), (uint32_t)e.logn, total);
        launch_ntt(*qc, false, out, out, full_map(*qc, qc->L), batch, s);
    }
}

// Vec<u64>::try_decode (F/bfv/plaintext.rs:157-170, 408-431): coefficients mod t [batch][N] -> values [batch][N].
inline void decode(const Encoder &e, bool simd, const u64 *coeffs, u64 *out, size_t batch, hipStream_t s) {
    require(!e.big(), E_PARAMETER_MISMATCH, "the plaintext modulus exceeds 64 bits: the coefficients are limbs");
    if (simd && !e.tctx) throw StatusError(E_SIMD_UNAVAILABLE, "SimdUnavailable: the plaintext modulus admits no degree-N NTT");
    if (!batch) return;
    grid_x(batch, "decode");
    const u64 total = (u64)batch * e.n;
    if (!simd) {
        launch_ew<k::perm_reduce_kernel>("decode_poly", total, s, coeffs, (u64)e.n, (u64)e.n, (const uint32_t *)nullptr, out, e.tm,
                                         (uint32_t)e.logn, total);
        return;
    }
    const Ctx &tc = *e.tctx;
    if (e.logn <= 14) {
        const RowLaunch rows(tc, 1, !f64_disabled());
        rows("decode_simd", batch, s,
             [](auto lm, auto nrw, auto h) { return kernel_c<k::decode_simd_kernel<lm(), nrw(), h()>>{}; },
             coeffs, e.d_map.p, out, tc.dmods(), rows.tw());
        return;
    }
    // rows larger than one LDS tile: reduce, launch_ntt, then the index map as a gather pass
    WsGuard tmp(total * sizeof(u64), s, true);
    launch_ew<k::perm_reduce_kernel>("decode_reduce", total, s, coeffs, (u64)e.n, (u64)e.n, (const uint32_t *)nullptr, tmp.u(),
                                     e.tm, (uint32_t)e.logn, total);
    launch_ntt(tc, false, tmp.u(), tmp.u(), full_map(tc, 1), batch, s);
    launch_ew<k::perm_reduce_kernel>("decode_gather", total, s, (const u64 *)tmp.u(), (u64)e.n, (u64)e.n,
                                     (const uint32_t *)e.d_map.p, out, e.tm, (uint32_t)e.logn, total);
}

// ------------------------------------------------------- plaintexts from packed bits ----
// fhe_util::transcode_* (fhe-util/src/lib.rs:71-190): ceil(nin in_bits / out_bits) output elements, the last one partial.
constexpr size_t TRANSCODE_MAX_ELEMS = (size_t)1 << 56;   // (keeps nin * in_bits below 2^63)
inline bool transcode_bits_ok(size_t bits, bool bytes) { return bits >= 1 && bits <= (bytes ? 8u : 64u); }
inline u64 transcode_count(size_t in_bits, size_t nin, size_t out_bits) {
    return ((u64)nin * in_bits + out_bits - 1) / out_bits;
}

// One launch of transcode_ew_kernel: `rows` rows of nin elements, row i at i * in_stride of `in` (bounded by total_in),
// written at (i / grp) * out_stride + (i % grp) * nout of `out`.
inline void launch_transcode(const void *in, bool in_bytes, size_t in_bits, u64 total_in, u64 in_stride, u64 nin, void *out,
                             bool out_bytes, size_t out_bits, u64 grp, u64 out_stride, size_t rows, hipStream_t s) {
    const u64 nout = transcode_count(in_bits, nin, out_bits);
    if (!rows || !nout) return;
    const u64 bpr = blocks_for(nout, EW_THREADS);
    const u64 blocks = (u64)grid_x(rows, "transcode") * grid_x(bpr, "transcode");   // (each factor first: the product cannot wrap)
    grid_x(blocks, "transcode");
    k::TranscodeIo io{in, out, total_in, in_stride, nin, nout, grp, out_stride, in_bytes ? 1u : 0u, (uint32_t)in_bits,
                      out_bytes ? 1u : 0u, (uint32_t)out_bits, (uint32_t)bpr};
    launch_blocks<k::transcode_ew_kernel>("transcode", blocks, EW_THREADS, 0, s, io);
}

// fhe_util::transcode_from_bytes / transcode_to_bytes / transcode_bidirectional: rows [batch][nin] -> [batch][nout].
inline void transcode(const void *in, bool in_bytes, size_t in_bits, size_t nin, void *out, bool out_bytes, size_t out_bits,
                      size_t batch, hipStream_t s) {
    require(transcode_bits_ok(in_bits, in_bytes), E_ARG, "transcode: in_bits must be in [1, 64] ([1, 8] for bytes)");
    require(transcode_bits_ok(out_bits, out_bytes), E_ARG, "transcode: out_bits must be in [1, 64] ([1, 8] for bytes)");
    require(nin <= TRANSCODE_MAX_ELEMS && (!nin || batch <= ((size_t)1 << 62) / nin), E_ARG, "transcode: too many elements");
    const u64 nout = transcode_count(in_bits, nin, out_bits);
    launch_transcode(in, in_bytes, in_bits, (u64)batch * nin, nin, nin, out, out_bytes, out_bits, 1, nout, batch, s);
}

// Plaintexts per item of encode_stream: ceil(nseg * M / N), M = ceil(seg_len * in_bits / nbits).
// (0 for widths or lengths encode_stream refuses)
inline u64 stream_plaintexts(const Encoder &e, size_t in_bits, size_t nseg, size_t seg_len, size_t nbits) {
    if (!transcode_bits_ok(in_bits, false) || !transcode_bits_ok(nbits, false) || seg_len > TRANSCODE_MAX_ELEMS) return 0;
    u64 nv;
    if (__builtin_mul_overflow((u64)nseg, transcode_count(in_bits, seg_len, nbits), &nv) || nv >> 62) return 0;
    return (nv + e.n - 1) / e.n;
}

// Plaintext::try_encode(Encoding::poly_at_level) (or, scaled, Plaintext::to_poly) of the transcoded values of a packed
// source (k::StreamSrc): per item nseg segments of seg_len elements, `total` elements in all (what lies beyond reads as
// zero) -> out [batch][nplain][L_level][N] Ntt.
inline void encode_stream(const Encoder &e, bool scaled, size_t level, const void *src, bool bytes, u64 total, size_t in_bits,
                          size_t nseg, size_t seg_len, size_t nbits, u64 *out, size_t batch, hipStream_t s) {
    require(!e.big(), E_PARAMETER_MISMATCH, "the plaintext modulus exceeds 64 bits: use fhe_bfv_encode_big_dev");
    const Ctx *qc = e.top->at_level(level);
    if (!qc) throw StatusError(E_INVALID_LEVEL, "InvalidLevel");
    require(nbits >= 1 && nbits <= 64, E_ARG, "encode: nbits must be in [1, 64]");
    require(transcode_bits_ok(in_bits, bytes), E_ARG, "encode: in_bits must be in [1, 64]");
    require(seg_len <= TRANSCODE_MAX_ELEMS, E_ARG, "encode: too many elements");
    const u64 M = transcode_count(in_bits, seg_len, nbits);
    u64 nv;
    require(!__builtin_mul_overflow((u64)nseg, M, &nv) && !(nv >> 62), E_ARG, "encode: too many elements");
    if (bytes && (u64)seg_len * 8 > (u64)e.n * nbits)
        throw StatusError(E_TOO_MANY_VALUES, "TooManyValues: more bits than a plaintext of the degree holds");
    const u64 nplain = bytes ? 1 : stream_plaintexts(e, in_bits, nseg, seg_len, nbits);
    if (!batch || !nplain) return;
    const u64 items = (u64)batch * nplain;
    grid_x(items * qc->L, "encode");
    const u64 qmt = e.q_mod_t[level];
    const k::u64x2 qm{qmt, shoup(qmt, e.t)};
    const k::u64x2 *delta = scaled ? e.d_delta[level]->p : nullptr;
    if (qc->logn <= 14) {
        k::StreamSrc ss{src, total, M ? (u64)nseg : 0, (u64)seg_len, (u64)seg_len, M ? M : 1, bytes ? 1u : 0u,
                        (uint32_t)in_bits, (uint32_t)nbits, (uint32_t)nplain, e.tm, qm, scaled ? 1u : 0u, delta};
        const RowLaunch rows(*qc, qc->L, !f64_disabled());
        rows("encode_stream", items * qc->L, s,
             [](auto lm, auto nrw, auto h) { return kernel_c<k::encode_stream_kernel<lm(), nrw(), h()>>{}; },
             ss, out, (uint32_t)qc->L, qc->dmods(), rows.tw());
        return;
    }
    // rows larger than one LDS tile: the values as a pass of their own into scratch that is cleared before it is reused
    // (plaintext coefficients: the reference zeroizes them, plaintext.rs:104, 178), then the element-wise lift and launch_ntt
    const u64 per_item = nplain * e.n;
    WsGuard vals(items * e.n * sizeof(u64), s, true);
    if ((u64)nseg * M < per_item) FHE_HIP_CHECK(hipMemsetAsync(vals.p, 0, vals.bytes, s));
    launch_transcode(src, bytes, in_bits, total, seg_len, seg_len, vals.p, false, nbits, nseg, per_item, batch * nseg, s);
    k::LiftSrc ls{vals.u(), e.n, e.n, e.tm, qm, scaled ? 1u : 0u, delta};
    const u64 all = items * qc->L * e.n;
    launch_ew<k::encode_lift_ew_kernel>("encode_lift", all, s, ls, out, (uint32_t)qc->L, qc->dmods(), (uint32_t)e.logn, all);
    launch_ntt(*qc, false, out, out, full_map(*qc, qc->L), items, s);
}

// ------------------------------------------------------------------------ encryption ----
// Poly::small (M/rq/mod.rs:298-330) and sample_vec_cbd (fhe-util/src/lib.rs:22-66).
inline void check_variance(size_t variance) {
    require(variance >= 1 && variance <= 32, E_INVALID_VARIANCE, "InvalidVariance: the variance must be in [1, 32]");
}

// next_u64 words one sample_vec_cbd draw of n samples consumes (each draw starts at a word boundary)
inline u64 cbd_words_per_draw(size_t variance, u64 n) {
    return variance <= 16 ? (n * 4 * variance + 63) / 64 : 2 * n;
}

// (int8 scratch rounded up to whole 16-byte words)
inline size_t small_bytes(size_t count) { return (count + 15) & ~(size_t)15; }

// Rows larger than one LDS tile (and PowerBasis output): the samples of `npolys` polynomials lifted to residue rows as a
// pass of its own, then (to_ntt) launch_ntt; the callers' combine stages follow as element-wise passes.
inline void small_lift(const Ctx &c, const int8_t *smp, u64 *x, size_t npolys, bool to_ntt, hipStream_t s) {
    const u64 total = (u64)npolys * c.L * c.n;
    launch_ew<k::small_lift_ew_kernel>("small_lift", total, s, smp, x, (uint32_t)c.L, c.dmods(), (uint32_t)c.logn, total);
    if (to_ntt) launch_ntt(c, false, x, x, full_map(c, c.L), npolys, s);
}

// The draws of one launch group: `kdraws` consecutive sample_vec_cbd draws of N samples per item, from next_u64 word
// `word0` of ChaCha8Rng::from_seed(seeds[b]) (key generation draws after the 32 bytes of K: word0 = 4), as int8
// e() [nb][kdraws N]; for rows larger than one LDS tile (!whole) also x() [nb][kdraws][L][N], lifted and transformed.
// The samples are secrets (SecretKey::random, the errors): both blocks are cleared before they return to the pool.
struct GroupDraws {
    WsGuard smp;
    std::unique_ptr<WsGuard> xw;
    GroupDraws(const Ctx &c, const uint8_t *seeds, size_t variance, size_t kdraws, u64 word0, size_t nb, bool whole,
               hipStream_t s)
        : smp(small_bytes(nb * kdraws * c.n), s, true) {
        const u64 ns = (u64)kdraws * c.n;
        const u64 wpd = cbd_words_per_draw(variance, c.n);
        if (word0)   // (the item is the grid's second dimension)
            launch_rows<k::cbd_sample_at_kernel, k::CBD_THREADS, k::CBD_AT_SMEM_BYTES>(
                "cbd_sample_at", ns, nb, 1, s, seeds, (int8_t *)smp.p, (uint32_t)variance, ns, (uint32_t)c.logn, wpd, word0);
        else
            launch_rows<k::cbd_sample_kernel, k::CBD_THREADS, k::CBD_SMEM_BYTES>(
                "cbd_sample", ns, nb, 1, s, seeds, (int8_t *)smp.p, (uint32_t)variance, ns, (uint32_t)c.logn, wpd);
        if (whole) return;
        xw = std::make_unique<WsGuard>(nb * kdraws * c.L * c.n * sizeof(u64), s, true);
        small_lift(c, e(), xw->u(), nb * kdraws, true, s);
    }
    const int8_t *e() const { return (const int8_t *)smp.p; }
    const u64 *x() const { return xw->u(); }
};

// Poly::small(ctx, variance, ChaCha8Rng::from_seed(seeds[b])): out [batch][L][N], PowerBasis or (to_ntt) Ntt.
inline void sample_small(const Ctx &c, size_t variance, const uint8_t *seeds, bool to_ntt, u64 *out, size_t batch,
                         hipStream_t s) {
    c.need_device();
    check_variance(variance);
    if (!batch) return;
    require(batch <= GRID_YZ_MAX, E_ARG, "sample_small: batch exceeds the grid limit");
    const GroupDraws d(c, seeds, variance, 1, 0, batch, true, s);   // (larger rows: lifted into `out`, not into scratch)
    if (to_ntt && c.logn <= 14) {
        const RowLaunch rows(c, c.L, !f64_disabled());
        rows("small_ntt", batch * c.L, s,
             [](auto lm, auto nrw, auto h) { return kernel_c<k::small_ntt_kernel<lm(), nrw(), h()>>{}; },
             d.e(), out, (uint32_t)c.L, c.dmods(), rows.tw());
        return;
    }
    small_lift(c, d.e(), out, batch, to_ntt, s);
}

// Items per launch group of an encryption: the u64 scratch rows of one group (`rows_per_item` polynomials per item:
// the seeded `a`, and for rows larger than one LDS tile the transformed samples) stay within `budget` bytes, and the
// batch is split into groups of equal size (a small tail group would underfill the device).  `cap`: most items a launch takes.
inline size_t encrypt_group(const Ctx &c, size_t rows_per_item, size_t batch, size_t budget, size_t cap = GRID_YZ_MAX) {
    const size_t per = std::max<size_t>(1, rows_per_item) * c.L * c.n * sizeof(u64);
    const size_t most = std::max<size_t>(1, std::min<size_t>(cap, budget / per));
    const size_t groups = (batch + most - 1) / most;
    return (batch + groups - 1) / groups;
}

// SecretKey::encrypt_poly (F/bfv/keys/secret_key.rs:100-134) with a = Poly::random_from_seed(a_seeds[b]) and
// e = Poly::small(ChaCha8Rng::from_seed(e_seeds[b])): out [batch][2][L][N] Ntt, c0 = e - a s + pt, c1 = a.
// s_ntt [L][N]; pt [batch][L][N] Delta-scaled (pt_shared: [L][N]; null: zero).
inline void encrypt_sk(const Ctx &c, size_t variance, const u64 *s_ntt, const uint8_t *a_seeds, const uint8_t *e_seeds,
                       const u64 *pt, bool pt_shared, u64 *out, size_t batch, hipStream_t s) {
    c.need_device();
    check_variance(variance);
    if (!batch) return;
    grid_x(batch * c.L, "encrypt");
    const bool whole = c.logn <= 14;
    const RowLaunch rows(c, c.L, !f64_disabled());   // (read once per call: every transform of the call takes the same kind)
    const u64 PL = (u64)c.L * c.n;
    // `a` is expanded into scratch: the unchanged seed_expand_kernel writes whole polynomials back to back
    // ([npolys][L][N]), so it cannot place them at out[b][1] (item stride 2 L N); the epilogue copies a into c1 while
    // it reads it for a (.) s.  Whole rows: groups of up to 1 GiB of `a` (seed_expand_kernel walks one polynomial per
    // workgroup and needs wide launches); larger rows: 256 MiB of `a` and transformed samples.
    const size_t group = whole ? encrypt_group(c, 1, batch, (size_t)1 << 30) : encrypt_group(c, 2, batch, (size_t)256 << 20);
    for_groups(batch, group, [&](size_t b0, size_t nb) {
        const u64 *ptb = pt ? pt + (pt_shared ? 0 : b0 * PL) : nullptr;
        const u64 pts = pt_shared ? (u64)0 : PL;
        u64 *outb = out + b0 * 2 * PL;
        const GroupDraws d(c, e_seeds + b0 * 32, variance, 1, 0, nb, whole, s);
        WsGuard a(nb * PL * sizeof(u64), s);
        polys_from_seeds(c, a_seeds + b0 * 32, a.u(), nb, s);
        if (whole)
            return rows("encrypt_sk", nb * c.L, s,
                        [](auto lm, auto nrw, auto h) { return kernel_c<k::encrypt_sk_kernel<lm(), nrw(), h()>>{}; },
                        d.e(), (const u64 *)a.u(), s_ntt, ptb, pts, outb, (uint32_t)c.L, c.dmods(), rows.tw());
        // rows larger than one LDS tile: the epilogue as a pass of its own over the transformed samples
        const u64 total = (u64)nb * PL;
        launch_ew<k::encrypt_combine_ew_kernel>("encrypt_combine", total, s, d.x(), (const u64 *)a.u(), s_ntt, ptb, pts, outb,
                                                (uint32_t)c.L, c.dmods(), (uint32_t)c.logn, 0u, total);
    });
}

// PublicKey::try_encrypt (F/bfv/keys/public_key.rs:47-97) with u, e1, e2 three consecutive Poly::small draws of
// ChaCha8Rng::from_seed(seeds[b]): out [batch][2][L][N] Ntt, c0 = u pk0 + e1 + pt, c1 = u pk1 + e2.  pk [2][L][N] over
// this context.
inline void encrypt_pk(const Ctx &c, size_t variance, const u64 *pk, const uint8_t *seeds, const u64 *pt, bool pt_shared,
                       u64 *out, size_t batch, hipStream_t s) {
    c.need_device();
    check_variance(variance);
    if (!batch) return;
    grid_x(batch * c.L, "encrypt");
    const bool whole = c.logn <= 14;
    const RowLaunch rows(c, c.L, !f64_disabled());
    const u64 PL = (u64)c.L * c.n;
    const size_t group = whole ? GRID_YZ_MAX : encrypt_group(c, 3, batch, (size_t)256 << 20);
    for_groups(batch, group, [&](size_t b0, size_t nb) {
        const u64 *ptb = pt ? pt + (pt_shared ? 0 : b0 * PL) : nullptr;
        const u64 pts = pt_shared ? (u64)0 : PL;
        u64 *outb = out + b0 * 2 * PL;
        const GroupDraws d(c, seeds + b0 * 32, variance, 3, 0, nb, whole, s);
        if (whole) {
            for (uint32_t stage = 0; stage < 3; stage++)
                rows("encrypt_pk", nb * c.L, s,
                     [](auto lm, auto nrw, auto h) { return kernel_c<k::encrypt_pk_kernel<lm(), nrw(), h()>>{}; },
                     d.e(), pk, ptb, pts, outb, (uint32_t)c.L, c.dmods(), rows.tw(), stage);
            return;
        }
        const u64 total = (u64)nb * PL;
        launch_ew<k::encrypt_combine_ew_kernel>("encrypt_combine", total, s, d.x(), (const u64 *)nullptr, pk, ptb, pts, outb,
                                                (uint32_t)c.L, c.dmods(), (uint32_t)c.logn, 1u, total);
    });
}

// ------------------------------------------------------------------ key generation ----
// KeySwitchingKey::new's digits over the key context (F/bfv/keys/key_switching_key.rs:97-136): RNS digits, one per
// ciphertext modulus, or for a single-modulus key context the decomposition in base 2^log_base with
// log_base = log_modulus / 2, log_modulus = q.next_power_of_two().ilog2().  -> (ndigits, log_base)
inline std::pair<size_t, size_t> ksk_digits(const Ctx &ct, const Ctx &kc) {
    if (kc.L == 1) {
        const size_t log_modulus = 64 - __builtin_clzll(kc.moduli[0] - 1);
        const size_t lb = log_modulus / 2;
        return {(log_modulus + lb - 1) / lb, lb};
    }
    return {ct.L, 0};
}

// `nkeys` handles of one geometry with their arrays allocated.
inline std::vector<std::unique_ptr<Ksk>> ksk_new_keys(const Ctx &ct, const Ctx &kc, size_t nd, size_t lb, size_t nkeys) {
    std::vector<std::unique_ptr<Ksk>> keys;
    for (size_t b = 0; b < nkeys; b++) {
        keys.push_back(make_ksk(ct, kc, nd, lb));
        ksk_alloc(*keys.back());
    }
    return keys;
}

// What the launches of one key call share, stated once for ksk_generate, ksk_load_wire and ksk_finish: the public
// constants of ksk_consts_kernel in scratch -- rq [Lk] {2^64 mod q_j, q_j^-1}, then g [nd][Lk] -- the group rule, a
// group's output table, and the element-wise pass over words already in the handles.  `checked`: a route that reads
// untrusted words also gets the zeroed flag word of the range check behind g (ksk_generate has none: its stream holds
// no memset).
struct KskCall {
    const Ctx &kc;
    const size_t nd, Lk;
    const u64 PK;   // words of one key array
    const bool wf, whole;
    hipStream_t s;
    WsGuard cst;
    KskCall(const Ctx &kc_, size_t nd_, size_t lb, bool checked, hipStream_t s_)
        : kc(kc_), nd(nd_), Lk(kc_.L), PK((u64)nd_ * kc_.L * kc_.n), wf(ksk_f64_eligible(kc_, lb)), whole(kc_.logn <= 14),
          s(s_), cst((2 * Lk + nd * Lk + (checked ? 1 : 0)) * sizeof(u64), s_) {
        if (checked) FHE_HIP_CHECK(hipMemsetAsync(flag(), 0, sizeof(u64), s));
        launch_ew<k::ksk_consts_kernel, 64>("ksk_consts", nd * Lk, s, kc.dmods(), (uint32_t)nd, (uint32_t)Lk, (uint32_t)lb,
                                            cst.u() + 2 * Lk, (k::u64x2 *)cst.p);
    }
    const k::u64x2 *rq() const { return (const k::u64x2 *)cst.p; }
    const u64 *g() const { return cst.u() + 2 * Lk; }
    uint32_t *flag() const { return (uint32_t *)(cst.u() + 2 * Lk + nd * Lk); }
    // groups: at most KG_KEYS keys (the output table travels in the kernel arguments) and 1 GiB of scratch rows, nd per
    // key (256 MiB at 2 nd per key for rows larger than one LDS tile), split into groups of equal size
    size_t group(size_t nkeys) const {
        return whole ? encrypt_group(kc, nd, nkeys, (size_t)1 << 30, k::KG_KEYS)
                     : encrypt_group(kc, 2 * nd, nkeys, (size_t)256 << 20, k::KG_KEYS);
    }
    static k::KskOut out(const Ksk &kk) { return k::KskOut{kk.c0.p, kk.c0s.p, kk.c1.p, kk.c1s.p, kk.c0f.p, kk.c1f.p}; }
    static k::KskOutTable table(const std::unique_ptr<Ksk> *keys, size_t nb) {
        k::KskOutTable tab{};
        for (size_t b = 0; b < nb; b++) tab.k[b] = out(*keys[b]);
        return tab;
    }
    // ksk_twin_ew_kernel over c0 (parts & 1) and c1 (parts & 2) of a group's nb keys: the range check into the flag word
    // and, unless check_only, the Shoup twins and F64 words.  Without check_only every word must be below its modulus.
    void twins(const k::KskOutTable &tab, size_t nb, uint32_t parts, uint32_t check_only) const {
        const u64 pairs = (u64)nb * PK / 2;
        launch_ew<k::ksk_twin_ew_kernel>("ksk_twin", pairs, s, tab, parts, check_only, rq(), (uint32_t)nd, (uint32_t)Lk, (uint32_t)wf,
                                         kc.dmods(), (uint32_t)kc.logn, pairs, flag());
    }
    // reads the flag word, waiting for `s`: a word >= q_j anywhere raised it (ksk_load_wire's one wait; ksk_finish's
    // callers wait once more before they return)
    void check() const {
        uint32_t bad = 0;
        FHE_HIP_CHECK(hipMemcpyAsync(&bad, flag(), sizeof(bad), hipMemcpyDeviceToHost, s));
        FHE_HIP_CHECK(hipStreamSynchronize(s));
        require(!bad, E_ARG, "key coefficient not reduced");
    }
};

// KeySwitchingKey::new (F/bfv/keys/key_switching_key.rs:71-236) for `nkeys` keys, key b with
// rng = ChaCha8Rng::from_seed(seeds[b]): K = the rng's first 32 bytes (written to seeds_out[b] when given),
// c1[i] = Poly::random_from_seed(ctx_ksk, bytes [32 i, 32 i + 32) of ChaCha8Rng::from_seed(K)), e_i = the rng's i-th
// Poly::small draw (from u64 word 4 on), c0[i] = NTT(e_i) - c1[i] (.) s + g_i (.) from[b].  s_ntt: the level-0 secret
// in Ntt form (its first Lk rows are read); from_ntt [nkeys][Lk][N] Ntt over the key context.  The handles are ready to
// use on `s`: no host synchronisation, and no key word passes through host memory.  The sampler, the seed expansion
// and the combine stage are one launch each per group of up to KG_KEYS keys.
inline std::vector<std::unique_ptr<Ksk>> ksk_generate(const Ctx &ct, const Ctx &kc, size_t variance, const u64 *s_ntt,
                                                      const u64 *from_ntt, const uint8_t *seeds, size_t nkeys,
                                                      uint8_t *seeds_out, hipStream_t s) {
    kc.need_device();
    check_variance(variance);
    const auto dg = ksk_digits(ct, kc);
    const size_t nd = dg.first, lb = dg.second, Lk = kc.L, N = kc.n;
    ksk_validate(ct, kc, nd, lb);
    auto keys = ksk_new_keys(ct, kc, nd, lb, nkeys);
    if (!nkeys) return keys;
    const KskCall kk(kc, nd, lb, false, s);
    const u64 PK = kk.PK;
    const bool whole = kk.whole;
    const RowLaunch rows(kc, Lk, !f64_disabled());   // (read once per call: every transform of the call takes the same kind)
    const size_t group = kk.group(nkeys);   // (the c1 scratch, and the transformed errors of larger rows)
    grid_x(group * nd * Lk, "ksk_generate");
    for_groups(nkeys, group, [&](size_t b0, size_t nb) {
        const k::KskOutTable tab = KskCall::table(&keys[b0], nb);
        WsGuard ds(nb * nd * 32, s), c1(nb * PK * sizeof(u64), s);
        const uint8_t *sd = seeds + b0 * 32;
        launch_ew<k::ksk_seeds_kernel, 64>("ksk_seeds", nb * nd, s, sd, seeds_out ? seeds_out + b0 * 32 : nullptr, (uint8_t *)ds.p,
                                           (uint32_t)nd, (uint32_t)(nb * nd));
        const GroupDraws d(kc, sd, variance, nd, 4, nb, whole, s);   // the errors: nd draws per key, after K
        polys_from_seeds(kc, (const uint8_t *)ds.p, c1.u(), nb * nd, s);
        const u64 *fb = from_ntt + b0 * Lk * N;
        if (whole)
            return rows("ksk_gen", nb * nd * Lk, s,
                        [](auto lm, auto nrw, auto h) { return kernel_c<k::ksk_gen_kernel<lm(), nrw(), h()>>{}; },
                        d.e(), (const u64 *)c1.u(), s_ntt, fb, kk.g(), kk.rq(), tab, (uint32_t)nd, (uint32_t)Lk,
                        (uint32_t)kk.wf, kc.dmods(), rows.tw());
        // rows larger than one LDS tile: the epilogue as a pass of its own over the transformed errors
        const u64 total = (u64)nb * PK;
        launch_ew<k::ksk_combine_ew_kernel>("ksk_combine", total, s, d.x(), (const u64 *)c1.u(), s_ntt, fb, kk.g(), kk.rq(), tab,
                                            (uint32_t)nd, (uint32_t)Lk, (uint32_t)kk.wf, kc.dmods(), (uint32_t)kc.logn, total);
    });
    return keys;
}

// Switcher(ctx_ct -> ctx_key) on Ntt rows (the switch-up of RelinearizationKey / GaloisKey::new when the key level is
// below the ciphertext level): in [np][ct.L][N] Ntt -> out [np][kc.L][N] Ntt, through a wiped PowerBasis scratch.  The
// switcher's tables are built on the host (public constants, as fhe_switcher_create); the call waits for the stream
// before they are freed.
inline void switch_up_ntt(const Ctx &ct, const Ctx &kc, const u64 *in, u64 *out, size_t np, hipStream_t s) {
    RnsContext rf(ct.moduli), rt(kc.moduli);
    auto sc = scaler_create(ct, kc, rt.product, rf.product);
    {
        WsGuard pb(np * ct.L * ct.n * sizeof(u64), s, true);
        launch_ntt(ct, true, in, pb.u(), full_map(ct, ct.L), np, s);
        launch_scale(*sc, pb.u(), (u64)ct.L * ct.n, out, (u64)kc.L * kc.n, np, s);
        launch_ntt(kc, false, out, out, full_map(kc, kc.L), np, s);
    }
    FHE_HIP_CHECK(hipStreamSynchronize(s));
}

// RelinearizationKey::new_leveled's `from` (F/bfv/keys/relinearization_key.rs:43-64): Switcher(ctx_ct -> ctx_key)
// applied to s_ct (.) s_ct, in Ntt form over the key context: out [kc.L][N].  s_ntt: the level-0 secret.
inline void relin_from(const Ctx &ct, const Ctx &kc, const u64 *s_ntt, u64 *out, hipStream_t s) {
    const size_t bytes = ct.L * ct.n * sizeof(u64);
    if (kc.L == ct.L) {
        FHE_HIP_CHECK(hipMemcpyAsync(out, s_ntt, bytes, hipMemcpyDeviceToDevice, s));
        ew_op(ct, out, s_ntt, 1, k::EW_MUL, s);
        return;
    }
    WsGuard t(bytes, s, true);
    FHE_HIP_CHECK(hipMemcpyAsync(t.p, s_ntt, bytes, hipMemcpyDeviceToDevice, s));
    ew_op(ct, t.u(), s_ntt, 1, k::EW_MUL, s);
    switch_up_ntt(ct, kc, t.u(), out, 1, s);
}

// GaloisKey::new's `from` (F/bfv/keys/galois_key.rs:26-58) for a batch of exponents: Switcher(ctx_ct -> ctx_key) of
// substitute(s_ct, exponents[b]), Ntt over the key context: out [nkeys][kc.L][N].  Exponents must be odd mod 2N
// (checked by the caller).
inline void galois_from(const Ctx &ct, const Ctx &kc, const u64 *s_ntt, const size_t *exponents, size_t nkeys, u64 *out,
                        hipStream_t s) {
    const u64 pc = (u64)ct.L * ct.n;
    std::unique_ptr<WsGuard> t;   // (the substituted rows over the ciphertext context, when they still switch up)
    if (kc.L != ct.L) t = std::make_unique<WsGuard>(nkeys * pc * sizeof(u64), s, true);
    u64 *dst = t ? t->u() : out;
    for_groups(nkeys, k::KG_KEYS, [&](size_t b0, size_t nb) {
        k::KgExps e{};
        for (size_t b = 0; b < nb; b++) e.e[b] = (uint32_t)(exponents[b0 + b] % (2 * ct.n));
        const u64 total = (u64)nb * pc;
        launch_ew<k::galois_from_kernel>("galois_from", total, s, s_ntt, dst + b0 * pc, e, (uint32_t)ct.L, (uint32_t)ct.logn, total);
    });
    if (t) switch_up_ntt(ct, kc, t->u(), out, nkeys, s);
}

// --------------------------------------------------------------- keys on the wire ----
// The digit count KeySwitchingKey::try_convert_from reads off a message (F/bfv/keys/key_switching_key.rs:394-412):
// ceil(log_modulus / log_base) for a decomposition key, else the ciphertext context's moduli count.
inline size_t ksk_wire_digits(const Ctx &ct, const Ctx &kc, size_t log_base) {
    if (!log_base) return ct.L;
    const size_t log_modulus = 64 - __builtin_clzll(kc.moduli[0] - 1);
    return (log_modulus + log_base - 1) / log_base;
}

// KeySwitchingKey::try_convert_from(&KeySwitchingKeyProto) (:387-482) for `nkeys` keys of one geometry: c0b
// [nkeys][ndigits][wire_poly_bytes(kc)] packed PowerBasis polynomials; c1b the same (explicit c1) or K [nkeys][32] the
// messages' seeds -- exactly one of the two.  No unpacked copy and no key word passes through host memory: whole rows
// (N <= 16384) go from the bytes through the transform into the handles in one launch per group of up to KG_KEYS keys
// (ksk_generate's groups); larger rows through wire_deserialize into the handle, the element-wise compare, launch_ntt
// and the element-wise twins.  A seeded
// c1 is expanded by the unchanged seed_expand_kernel straight into each handle's c1 (it writes a key's digits back to
// back, the handle's layout), one launch per key.  A word >= q_j anywhere raises the call's flag word: the call waits
// for `s` once, after its last launch, reads it, and throws E_ARG -- the handles are freed with the vector.
inline std::vector<std::unique_ptr<Ksk>> ksk_load_wire(const Ctx &ct, const Ctx &kc, size_t lb, const uint8_t *c0b,
                                                       const uint8_t *c1b, const uint8_t *K, size_t nkeys, hipStream_t s) {
    kc.need_device();
    const size_t nd = ksk_wire_digits(ct, kc, lb), Lk = kc.L, N = kc.n;
    ksk_validate(ct, kc, nd, lb);
    auto keys = ksk_new_keys(ct, kc, nd, lb, nkeys);
    if (!nkeys) return keys;
    const KskCall kk(kc, nd, lb, true, s);   // (ksk_consts_kernel's g is not read here)
    const u64 wb = wire_poly_bytes(kc);
    const bool whole = kk.whole;
    const RowLaunch rows(kc, Lk, !f64_disabled());
    // the word-granular loader: rows of >= 128 coefficients and 16-byte aligned byte pointers (see ksk_load_kernel)
    const bool words = N >= 128 && ((uintptr_t)c0b & 15) == 0 && ((uintptr_t)c1b & 15) == 0;
    const size_t group = kk.group(nkeys);
    grid_x(2 * group * nd * Lk, "ksk_load_wire");
    for_groups(nkeys, group, [&](size_t b0, size_t nb) {
        const k::KskOutTable tab = KskCall::table(&keys[b0], nb);
        const uint8_t *b0p = c0b + b0 * nd * wb, *b1p = c1b ? c1b + b0 * nd * wb : nullptr;
        uint32_t ew_parts = whole ? 0u : 3u;   // what ksk_twin_ew_kernel still has to do for this group
        if (K) {
            WsGuard ds(nb * nd * 32, s);
            launch_ew<k::ksk_dseeds_kernel, 64>("ksk_dseeds", nb * nd, s, K + b0 * 32, (uint8_t *)ds.p, (uint32_t)nd,
                                                (uint32_t)(nb * nd));
            for (size_t b = 0; b < nb; b++)
                polys_from_seeds(kc, (const uint8_t *)ds.p + b * nd * 32, keys[b0 + b]->c1.p, nd, s);
            ew_parts |= 2u;
        }
        if (whole) {
            rows("ksk_load", (b1p ? 2 : 1) * nb * nd * Lk, s,
                 [](auto lm, auto nrw, auto h) { return kernel_c<k::ksk_load_kernel<lm(), nrw(), h()>>{}; }, b0p, b1p, wb,
                 (uint32_t)words, kk.rq(), tab, (uint32_t)nd, (uint32_t)Lk, (uint32_t)(nb * nd), (uint32_t)kk.wf, kc.dmods(),
                 rows.tw(), kk.flag());
        }
        if (!whole) {
            // unpack into the handles, compare the PowerBasis words with their moduli, then transform in place
            for (size_t b = 0; b < nb; b++) {
                wire_deserialize(kc, b0p + b * nd * wb, keys[b0 + b]->c0.p, nd, false, s);
                if (b1p) wire_deserialize(kc, b1p + b * nd * wb, keys[b0 + b]->c1.p, nd, false, s);
            }
            kk.twins(tab, nb, b1p ? 3u : 1u, 1u);
            for (size_t b = 0; b < nb; b++) {
                launch_ntt(kc, false, keys[b0 + b]->c0.p, keys[b0 + b]->c0.p, full_map(kc, Lk), nd, s);
                if (b1p) launch_ntt(kc, false, keys[b0 + b]->c1.p, keys[b0 + b]->c1.p, full_map(kc, Lk), nd, s);
            }
        }
        if (ew_parts) kk.twins(tab, nb, ew_parts, 0u);
    });
    kk.check();
    return keys;
}

// The one way to finish a handle whose c0 and c1 already hold Ntt words on `s` (fhe_ksk_create(_dev), the multiparty
// relinearization key).  The words are untrusted: the range check runs as a pass of its own and the call waits for `s`
// to read its flag -- the twin pass must never see a word >= q_j -- then come the Shoup twins and, when eligible, the
// F64 words.
inline void ksk_finish(const Ksk &k_, hipStream_t s) {
    const KskCall kk(*k_.ksk_ctx, k_.ndigits, k_.log_base, true, s);
    k::KskOutTable tab{};
    tab.k[0] = KskCall::out(k_);
    kk.twins(tab, 1, 3u, 1u);
    kk.check();
    kk.twins(tab, 1, 3u, 0u);
}

// From<&KeySwitchingKey> for KeySwitchingKeyProto (:365-385): c0 (and c1 when c1b is given) taken to PowerBasis and
// packed, straight from the handle's arrays.
inline void ksk_serialize_wire(const Ksk &k_, uint8_t *c0b, uint8_t *c1b, hipStream_t s) {
    const Ctx &kc = *k_.ksk_ctx;
    wire_serialize(kc, k_.c0.p, c0b, k_.ndigits, true, s);
    if (c1b) wire_serialize(kc, k_.c1.p, c1b, k_.ndigits, true, s);
}

// ------------------------------------------------------------------ multiparty BFV ----
// The shares of F/mbfv/ (kernels_mbfv.hpp).  One part of a call: the form, the operands (e, edraws filled in by
// mbfv_shares) and out [batch][k][L][N].
struct MbfvPart {
    int form;
    k::MbfvArgs g;
    u64 *out;
};

// `edraws` consecutive Poly::small draws of ChaCha8Rng::from_seed(seeds[b]) per item, then every part's launch over the
// draws [e0, e0 + k) of each item.  The samples and their transforms are secrets: cleared before their blocks return
// to the pool.
inline void mbfv_shares(const Ctx &c, size_t variance, const uint8_t *seeds, size_t edraws, std::vector<MbfvPart> parts,
                        size_t batch, hipStream_t s) {
    c.need_device();
    check_variance(variance);
    if (!batch) return;
    grid_x(batch * edraws * c.L, "mbfv");
    const bool whole = c.logn <= 14;
    const RowLaunch rows(c, c.L, !f64_disabled());   // (read once per call: every transform of the call takes the same kind)
    const u64 PL = (u64)c.L * c.n;
    const size_t group = whole ? encrypt_group(c, 1, batch, ~(size_t)0 >> 1) : encrypt_group(c, edraws, batch, (size_t)256 << 20);
    for_groups(batch, group, [&](size_t b0, size_t nb) {
        const GroupDraws d(c, seeds + b0 * 32, variance, edraws, 0, nb, whole, s);
        for (const MbfvPart &pt : parts) {
            k::MbfvArgs g = pt.g;
            g.e = d.e();
            g.edraws = (uint32_t)edraws;
            g.rows = (uint32_t)c.L;
            g.A += b0 * g.a_stride;
            g.X += b0 * g.s_stride;
            if (g.X2) g.X2 += b0 * g.s_stride;
            if (g.Y) g.Y += b0 * g.s_stride;
            u64 *outb = pt.out + b0 * g.k * PL;
            if (whole) {
                with_int<0, 2>((size_t)pt.form, "unknown share form", [&](auto form) {
                    rows("mbfv_share", nb * g.k * c.L, s,
                         [](auto lm, auto nrw, auto h) {
                             return kernel_c<k::mbfv_share_kernel<lm(), nrw(), h(), decltype(form)::value>>{};
                         },
                         g, outb, c.dmods(), rows.tw());
                });
                continue;
            }
            // rows larger than one LDS tile: the epilogues as passes over the transformed draws
            const u64 total = (u64)nb * g.k * PL;
            launch_ew<k::mbfv_share_ew_kernel>("mbfv_share", total, s, d.x(), g, (uint32_t)pt.form, outb, c.dmods(), (uint32_t)c.logn,
                                               total);
        }
    });
}

// words between the secrets of consecutive items: none when one party serves the batch, else a level-0 secret (the
// first L rows of each are read, as key generation reads them)
inline u64 mbfv_secret_stride(const Ctx &c, bool s_shared) { return s_shared ? 0 : (u64)c.root->L * c.n; }

inline k::MbfvArgs mbfv_args(const u64 *A, u64 a_stride, const u64 *X, const u64 *X2, const u64 *Y, const u64 *w,
                             u64 s_stride, size_t e0, size_t kd, bool neg) {
    return k::MbfvArgs{nullptr, A, X, X2, Y, w, a_stride, s_stride, 0u, (uint32_t)e0, (uint32_t)kd, 0u, neg ? 1u : 0u};
}

// PublicKeyShare::new (F/mbfv/public_key_gen.rs:32-57): out[b] = e_b - crp (.) s_b.  crp [L][N]; s [L][N] shared or
// a level-0 secret per item; one draw per item.
inline void mbfv_pk_share(const Ctx &c, size_t variance, const u64 *crp, const u64 *s_ntt, bool s_shared,
                          const uint8_t *seeds, u64 *out, size_t batch, hipStream_t s) {
    mbfv_shares(c, variance, seeds, 1,
                {{k::MBFV_AX, mbfv_args(crp, 0, s_ntt, nullptr, nullptr, nullptr, mbfv_secret_stride(c, s_shared), 0, 1, true),
                  out}},
                batch, s);
}

// SecretKeySwitchShare::new (F/mbfv/secret_key_switch.rs:38-95): out[b] = e_b + c1_b (.) (s_in - s_out); s_out null:
// DecryptionShare::new (:133-142), the zero output key, with no zero key built.  c1 at c1_stride words per item.
inline void mbfv_sks_share(const Ctx &c, size_t variance, const u64 *s_in, const u64 *s_out, bool s_shared, const u64 *c1,
                           u64 c1_stride, const uint8_t *seeds, u64 *out, size_t batch, hipStream_t s) {
    mbfv_shares(c, variance, seeds, 1,
                {{s_out ? k::MBFV_AXX : k::MBFV_AX,
                  mbfv_args(c1, c1_stride, s_in, s_out, nullptr, nullptr, mbfv_secret_stride(c, s_shared), 0, 1, false), out}},
                batch, s);
}

// PublicKeySwitchShare::new (F/mbfv/public_key_switch.rs:33-92): h0 = pk0 (.) u + s (.) c1 + e0, h1 = pk1 (.) u + e1
// with u, e0, e1 three consecutive draws: encrypt_pk with the addend s (.) c1, which is secret-dependent and lives in
// scratch that is cleared before reuse.  ct [batch][2][L][N] ([2][L][N] when shared); out [batch][2][L][N].
inline void mbfv_pks_share(const Ctx &c, size_t variance, const u64 *s_ntt, bool s_shared, const u64 *pk, const u64 *ct,
                           bool ct_shared, const uint8_t *seeds, u64 *out, size_t batch, hipStream_t s) {
    c.need_device();
    check_variance(variance);
    if (!batch) return;
    const u64 PL = (u64)c.L * c.n, total = (u64)batch * PL;
    WsGuard sc1(total * sizeof(u64), s, true);
    launch_ew<k::mbfv_mul_ew_kernel>("mbfv_mul", total, s, s_ntt, mbfv_secret_stride(c, s_shared), ct + PL,
                                     ct_shared ? (u64)0 : 2 * PL, sc1.u(), (uint32_t)c.L, c.dmods(), (uint32_t)c.logn, total);
    encrypt_pk(c, variance, pk, seeds, sc1.u(), false, out, batch, s);
}

// RelinKeyShare<R1>::new (F/mbfv/relin_key_gen.rs:141-197): 2L draws per item, h0_i = e_i - a_i (.) u + g_i s (draws
// 0 ... L - 1), h1_i = e'_i + a_i (.) s (draws L ... 2L - 1); g_i = get_garner(i) mod q_r from ksk_consts_kernel.
// crp [L][L][N]; out_h0, out_h1 [batch][L][L][N].
inline void mbfv_rlk_round1(const Ctx &c, size_t variance, const u64 *s_ntt, const u64 *u_ntt, bool s_shared,
                            const u64 *crp, const uint8_t *seeds, u64 *out_h0, u64 *out_h1, size_t batch, hipStream_t s) {
    c.need_device();
    check_variance(variance);
    require(c.L >= 2, E_KEYSWITCH_UNSUPPORTED, "KeySwitchingNotSupported: a relinearization key needs two moduli");
    if (!batch) return;
    const size_t L = c.L;
    const u64 st = mbfv_secret_stride(c, s_shared);
    WsGuard cst((2 * L + L * L) * sizeof(u64), s);
    k::u64x2 *rq = (k::u64x2 *)cst.p;
    u64 *g = cst.u() + 2 * L;
    launch_ew<k::ksk_consts_kernel, 64>("ksk_consts", L * L, s, c.dmods(), (uint32_t)L, (uint32_t)L, 0u, g, rq);
    mbfv_shares(c, variance, seeds, 2 * L,
                {{k::MBFV_AX_WY, mbfv_args(crp, 0, u_ntt, nullptr, s_ntt, g, st, 0, L, true), out_h0},
                 {k::MBFV_AX, mbfv_args(crp, 0, s_ntt, nullptr, nullptr, nullptr, st, L, L, false), out_h1}},
                batch, s);
}

// RelinKeyShare<R2>::new (F/mbfv/relin_key_gen.rs:243-296): h0'_i = e_i + H0_i (.) s, h1'_i = e'_i + H1_i (.) (u - s),
// H0, H1 [L][L][N] the aggregated round-1 shares; draws as round 1.
inline void mbfv_rlk_round2(const Ctx &c, size_t variance, const u64 *s_ntt, const u64 *u_ntt, bool s_shared,
                            const u64 *r1_h0, const u64 *r1_h1, const uint8_t *seeds, u64 *out_h0, u64 *out_h1,
                            size_t batch, hipStream_t s) {
    c.need_device();
    check_variance(variance);
    require(c.L >= 2, E_KEYSWITCH_UNSUPPORTED, "KeySwitchingNotSupported: a relinearization key needs two moduli");
    if (!batch) return;
    const size_t L = c.L;
    const u64 st = mbfv_secret_stride(c, s_shared);
    mbfv_shares(c, variance, seeds, 2 * L,
                {{k::MBFV_AX, mbfv_args(r1_h0, 0, s_ntt, nullptr, nullptr, nullptr, st, 0, L, false), out_h0},
                 {k::MBFV_AXX, mbfv_args(r1_h1, 0, u_ntt, s_ntt, nullptr, nullptr, st, L, L, false), out_h1}},
                batch, s);
}

// Aggregate::from_shares: out[j] = base[j] + sum_p shares[p][j] over npolys polynomials [L][N]; polynomial j of base at
// j base_stride words.  Strides are even and the buffers 16-byte aligned (the kernel moves two words at a time).
inline void mbfv_sum(const Ctx &c, const u64 *shares, size_t nshares, u64 share_stride, size_t npolys, const u64 *base,
                     u64 base_stride, u64 *out, hipStream_t s) {
    c.need_device();
    require(nshares >= 1, E_ARG, "NoShares: an aggregation needs at least one share");
    require(nshares <= 0xffffffffu && (share_stride & 1) == 0 && (base_stride & 1) == 0, E_ARG,
            "mbfv: share strides must be even");
    require(((uintptr_t)shares | (uintptr_t)base | (uintptr_t)out) % 16 == 0, E_ARG, "mbfv: buffers must be 16-byte aligned");
    if (!npolys) return;
    const u64 PL = (u64)c.L * c.n;
    grid_x(PL / 2, "mbfv");   // (the kernel takes the pairs of a polynomial as a 32-bit count)
    for_groups(npolys, GRID_YZ_MAX, [&](size_t j0, size_t nj) {   // (the polynomial is the grid's second dimension)
        launch_rows<k::mbfv_sum_kernel>("mbfv_sum", PL / 2, nj, 1, s, shares + j0 * PL, (uint32_t)nshares, share_stride,
                                        base ? base + j0 * base_stride : nullptr, base_stride, out + j0 * PL, c.dmods(),
                                        (uint32_t)c.logn, (uint32_t)(PL / 2));
    });
}

// Plaintext::from_shares (F/mbfv/secret_key_switch.rs:145-186): c0 + the sum of the decryption shares in one launch,
// then the inverse transform, the scale and the tail of decrypt().  ct [batch][2][L][N]; shares [nshares] x
// [batch][L][N] at share_stride words; out [batch][N] in [0, t).
inline void mbfv_decrypt(const Scaler &sc, u64 t, const u64 *ct, const u64 *shares, size_t nshares, u64 share_stride,
                         u64 *out, size_t batch, hipStream_t s) {
    const Ctx &cc = *sc.from;
    cc.need_device();
    require(nshares >= 1, E_ARG, "NoShares: an aggregation needs at least one share");
    check_plain_context(sc);
    require(!sc.wide_num, E_PARAMETER_MISMATCH, "the scaler's plaintext modulus exceeds 64 bits: use fhe_mbfv_decrypt_big_dev");
    if (!batch) return;
    const u64 PL = (u64)cc.L * cc.n;
    WsGuard ph(batch * PL * sizeof(u64), s, true);   // the phase: cleared before the block goes back to the pool
    mbfv_sum(cc, shares, nshares, share_stride, batch, ct, 2 * PL, ph.u(), s);
    launch_ntt(cc, true, ph.u(), ph.u(), full_map(cc, cc.L), batch, s);
    decrypt_tail(sc, t, ph.u(), out, batch, s);
}

// `&Ciphertext + &Plaintext` / `-` (F/bfv/ops/mod.rs:71-108, 166-203): c0 +- to_poly(pt), the other parts unchanged.
// ct, out [batch][nparts][L][N]; pt [batch][L][N] Delta-scaled (pt_shared: [L][N]); out == ct allowed.
inline void add_plain(const Ctx &c, bool subtract, size_t nparts, const u64 *ct, const u64 *pt, bool pt_shared, u64 *out,
                      size_t batch, hipStream_t s) {
    c.need_device();
    require(nparts >= 1, E_ARG, "a ciphertext has at least one part");
    if (!batch) return;
    const u64 pl = (u64)c.L * c.n;
    // (the ciphertext is the grid's second dimension: a batch above GRID_YZ_MAX is refused)
    launch_rows<k::add_plain_kernel>("add_plain", pl, batch, 1, s, ct, pt, pt_shared ? (u64)0 : pl, out, c.dmods(), (uint32_t)nparts,
                                     (uint32_t)c.logn, pl, subtract ? 1u : 0u, out != ct ? 1u : 0u);
}

// --------------------------------------------------------------------- lift and noise ----
inline BigUint ctx_modulus(const Ctx &c) {
    BigUint q(1);
    for (u64 m : c.moduli) q = q * BigUint(m);
    return q;
}
inline size_t lift_limbs(const Ctx &c) { return c.lift_w; }

// The table kernels_noise.hpp describes, built and uploaded once per context.  The upload is a synchronous hipMalloc +
// hipMemcpy inside the first call: that call blocks the host and cannot be part of a stream capture (fhe_hip.h says so).
inline const u64 *lift_consts(const Ctx &c) {
    std::call_once(c.lift_once, [&] {
        const uint32_t L = (uint32_t)c.L;
        std::vector<u64> h(k::lift_table_words(L), 0);
        for (uint32_t i = 0; i < L; i++) {
            const u64 qi = c.moduli[i];
            h[i] = qi;
            h[L + i] = qi * (u64)((((u128)1 << 62) + qi - 1) / qi);
            for (uint32_t j = 0; j < i; j++) {
                const u64 inv = inv_mod_general(c.moduli[j] % qi, qi);
                const size_t at = k::lift_pairs_at(L) + (size_t)i * (i - 1) + 2 * j;
                h[at] = inv;
                h[at + 1] = shoup(inv, qi);
            }
        }
        const BigUint q = ctx_modulus(c);
        for (uint32_t i = 0; i < L; i++) h[k::lift_q_at(L) + i] = q.limb(i);
        c.d_lift.upload(h);
    });
    return c.d_lift.p;
}

// lift_kernel<L, BITS> over polys [batch][L][N]; the instantiated L = 1 ... 16 cover the stock sets (3, 5, 9), C2 (4) and
// C5's chain; longer chains take the generic instance.
constexpr int LIFT_LC_MAX = 16;
template <bool BITS>
inline void launch_lift(const Ctx &c, const u64 *polys, const k::LiftSub &sub, u64 *out, uint32_t *partial, size_t w,
                        size_t batch, hipStream_t s) {
    require(c.L <= (size_t)k::LIFT_LMAX, E_ARG, "lift: more moduli than the generic instance holds");
    const u64 nblk = blocks_for(c.n, k::LIFT_THREADS);
    const unsigned grid = grid_x(batch * nblk, "lift");
    const u64 *tab = lift_consts(c);
    const size_t lds = BITS ? k::LIFT_SMEM_BYTES : 0;
    const char *name = BITS ? "centered_bits" : "lift";
    with_int_or_generic<1, LIFT_LC_MAX>(c.L, "lift: no moduli", [&](auto lc) {
        launch_blocks<k::lift_kernel<decltype(lc)::value, BITS>>(name, grid, k::LIFT_THREADS, lds, s, polys, tab, sub, out, partial,
                                                                 (uint32_t)c.L, (uint32_t)w, (uint32_t)c.logn, (uint32_t)nblk,
                                                                 (uint32_t)batch);
    });
}

// RnsContext::lift per coefficient (M/rns/mod.rs:138-143): polys [batch][L][N] -> out [batch][N][W] limbs.
inline void poly_lift(const Ctx &c, const u64 *polys, u64 *out, size_t batch, hipStream_t s) {
    c.need_device();
    if (!batch) return;
    launch_lift<false>(c, polys, k::lift_sub_none(), out, nullptr, lift_limbs(c), batch, s);
}

// max over the coefficients of min(bits(x), bits(q - x)) (secret_key.rs:88-95) of polys [batch][L][N] minus, when
// sub.m is given, the Delta-scaled plaintext: the per-workgroup maxima go through wiping scratch, then one thread per
// polynomial reduces them.
inline void centered_bits(const Ctx &c, const u64 *polys, const k::LiftSub &sub, u64 *out_bits, size_t batch,
                          hipStream_t s) {
    c.need_device();
    if (!batch) return;
    const size_t nblk = blocks_for(c.n, k::LIFT_THREADS);
    WsGuard part(batch * nblk * sizeof(uint32_t), s, true);
    launch_lift<true>(c, polys, sub, nullptr, (uint32_t *)part.p, 0, batch, s);
    launch_ew<k::noise_max_kernel>("noise_max", batch, s, (const uint32_t *)part.p, (uint32_t)nblk, (uint32_t)batch, out_bits);
}

// ------------------------------------------------------- plaintext moduli above 64 bits ----
// PlaintextModulus::Large (F/bfv/parameters.rs:560-738): the encoder of a t with W_t = 2 ... 4 limbs.  The plaintext
// context is the shortest prefix of the moduli with at least bits(t) + 60 bits, capped at all of them (:578-595).
inline size_t plain_rows(const Ctx &top, size_t t_bits) {
    size_t acc = 0, count = 0;
    for (u64 q : top.moduli) {
        acc += 64 - (size_t)__builtin_clzll(q | 1);
        count++;
        if (acc >= t_bits + 60) break;
    }
    return count;
}
inline std::unique_ptr<Encoder> encoder_create_big(const Ctx &top, const BigUint &t) {
    top.need_device();
    auto e = std::make_unique<Encoder>();
    e->top = &top;
    e->n = top.n;
    e->logn = top.logn;
    e->wt = t.w.size();
    require(e->wt >= 2 && e->wt <= (size_t)k::BIGT_WMAX, E_INVALID_MODULUS, "the plaintext modulus must be below 2^256");
    e->t_big = t;
    const BigUint mu = BigUint::pow2(128 * e->wt) / t;
    for (size_t i = 0; i < e->wt + 2; i++) e->mu_big.push_back(mu.limb(i));
    e->plain = top.at_level(top.L - plain_rows(top, t.bits()));
    // the tail reduces a value below Q_p with a Barrett step that holds 2 W_t limbs
    require(e->plain->lift_w <= 2 * e->wt && e->plain->L >= e->wt, E_INVALID_MODULUS,
            "the plaintext context is too long for the plaintext modulus");
    for (const Ctx *c = &top; c; c = c->next.get()) {
        push_delta(*e, *c, [&](u64 q) { return t.mod_u64(q); });
        const BigUint qt = ctx_modulus(*c) % t;
        std::vector<u64> limbs(e->wt);
        for (size_t i = 0; i < e->wt; i++) limbs[i] = qt.limb(i);
        e->q_mod_t_big.push_back(limbs);
    }
    return e;
}
template <int WT>
inline k::BigT<WT> bigt_consts(const Encoder &e) {
    k::BigT<WT> bt;
    for (int i = 0; i < WT; i++) bt.t[i] = e.t_big.limb(i);
    for (int i = 0; i < WT + 2; i++) bt.mu[i] = e.mu_big[i];
    return bt;
}
inline void need_big(const Encoder &e) {
    require(e.big(), E_PARAMETER_MISMATCH, "the plaintext modulus fits 64 bits: use the u64 entry point");
}

// PlaintextVec::try_encode for Vec<BigUint>, Encoding::poly (F/bfv/plaintext_vec.rs:105-132), or with `scaled`
// Plaintext::to_poly's Large branch (F/bfv/plaintext.rs:172-197): values [batch][nvalues][W_t] -> out
// [batch][L_level][N] Ntt.  The projection writes the rows, the forward transform runs on them in place.
inline void encode_big(const Encoder &e, bool simd, bool scaled, size_t level, const u64 *values, size_t nvalues, u64 *out,
                       size_t batch, hipStream_t s) {
    need_big(e);
    const Ctx *qc = e.top->at_level(level);
    if (!qc) throw StatusError(E_INVALID_LEVEL, "InvalidLevel");
    if (simd) throw StatusError(E_SIMD_UNAVAILABLE, "SimdUnavailable: no NTT modulo a plaintext modulus above 64 bits");
    if (nvalues > e.n) throw StatusError(E_TOO_MANY_VALUES, "TooManyValues: more values than the degree");
    if (!batch) return;
    const u64 total = (u64)batch * e.n;
    grid_x(blocks_for(total, k::BIGT_THREADS), "encode");
    with_int<2, k::BIGT_WMAX>(e.wt, "encode: unsupported plaintext limbs", [&](auto w) {
        constexpr int WT = decltype(w)::value;
        k::BigVal<WT> qmt;
        for (int i = 0; i < WT; i++) qmt.w[i] = e.q_mod_t_big[level][i];
        launch_ew<k::bigt_project_kernel<WT>, k::BIGT_THREADS>("bigt_project", total, s, values, (u64)nvalues, out, (uint32_t)qc->L,
                                                               qc->dmods(), (const k::u64x2 *)e.d_delta[level]->p,
                                                               bigt_consts<WT>(e), qmt, scaled ? 1u : 0u, (uint32_t)e.logn, total);
    });
    launch_ntt(*qc, false, out, out, full_map(*qc, qc->L), batch, s);
}

// The tail of the Large branch of SecretKey::try_decrypt (F/bfv/keys/secret_key.rs:238-250): polys [batch][P][N],
// PowerBasis residues over the plaintext context -> out [batch][N][W_t], ((x + t) mod Q_p) mod t of the lifted x.
constexpr int BIGT_PC_MAX = 8;
inline void reduce_big(const Encoder &e, const u64 *polys, size_t rows, u64 *out, size_t batch, hipStream_t s) {
    need_big(e);
    const Ctx &pc = *e.plain;
    require(rows == pc.L, E_PARAMETER_MISMATCH, "reduce: the polynomials must have one row per plaintext-context modulus");
    if (!batch) return;
    require(pc.L <= (size_t)k::LIFT_LMAX, E_ARG, "reduce: more plaintext-context moduli than the generic instance holds");
    const u64 nblk = blocks_for(pc.n, k::BIGT_THREADS);
    const unsigned grid = grid_x(batch * nblk, "reduce");
    const u64 *tab = lift_consts(pc);
    with_int<2, k::BIGT_WMAX>(e.wt, "reduce: unsupported plaintext limbs", [&](auto w) {
        constexpr int WT = decltype(w)::value;
        const k::BigT<WT> bt = bigt_consts<WT>(e);
        with_int_or_generic<WT, BIGT_PC_MAX>(pc.L, "reduce: plaintext context shorter than the plaintext modulus", [&](auto p) {
            launch_blocks<k::bigt_tail_kernel<decltype(p)::value, WT>>("bigt_tail", grid, k::BIGT_THREADS, 0, s, polys, tab, bt, out,
                                                                       (uint32_t)pc.L, (uint32_t)pc.logn, (uint32_t)nblk);
        });
    });
}
// Scaler::scale (t / Q_level) of the PowerBasis phase into the plaintext context, then the tail: out [batch][N][W_t]
inline void check_plain_context_big(const Encoder &e, const Scaler &sc) {
    const Ctx *lc = e.top;
    while (lc && !lc->same_ring(*sc.from)) lc = lc->next.get();
    require(lc != nullptr, E_PARAMETER_MISMATCH, "the scaler's source is not a level of the encoder's parameter set");
    require(sc.to->same_ring(*e.plain), E_PARAMETER_MISMATCH, "the scaler's target is not the plaintext context");
    require(e.top->device == sc.from->device, E_PARAMETER_MISMATCH, "the encoder and the scaler live on different devices");
}
inline void decrypt_tail_big(const Encoder &e, const Scaler &sc, const u64 *ph, u64 *out, size_t batch, hipStream_t s) {
    WsGuard d(batch * sc.to->L * sc.from->n * sizeof(u64), s, true);   // the scaled plaintext: secret-dependent
    scale_polys(sc, ph, d.u(), batch, false, s);
    reduce_big(e, d.u(), sc.to->L, out, batch, s);
}
// SecretKey::try_decrypt, Large branch (F/bfv/keys/secret_key.rs:198-250): ct [batch][nparts][L][N] Ntt, s_ntt [L][N]
// -> out [batch][N][W_t].
inline void decrypt_big(const Encoder &e, const Scaler &sc, const u64 *s_ntt, const u64 *ct, size_t nparts, u64 *out,
                        size_t batch, hipStream_t s) {
    need_big(e);
    const Ctx &cc = *sc.from;
    cc.need_device();
    require(nparts >= 1, E_ARG, "a ciphertext has at least one part");
    check_plain_context_big(e, sc);
    if (!batch) return;
    WsGuard ph(batch * (u64)cc.L * cc.n * sizeof(u64), s, true);   // the phase: cleared before the block is reused
    phase_power_basis(cc, s_ntt, ct, nparts, ph.u(), batch, s);
    decrypt_tail_big(e, sc, ph.u(), out, batch, s);
}
// Plaintext::from_shares (F/mbfv/secret_key_switch.rs:145-186) with the Large tail: as mbfv_decrypt, out [batch][N][W_t].
inline void mbfv_decrypt_big(const Encoder &e, const Scaler &sc, const u64 *ct, const u64 *shares, size_t nshares,
                             u64 share_stride, u64 *out, size_t batch, hipStream_t s) {
    need_big(e);
    const Ctx &cc = *sc.from;
    cc.need_device();
    require(nshares >= 1, E_ARG, "NoShares: an aggregation needs at least one share");
    check_plain_context_big(e, sc);
    if (!batch) return;
    const u64 PL = (u64)cc.L * cc.n;
    WsGuard ph(batch * PL * sizeof(u64), s, true);
    mbfv_sum(cc, shares, nshares, share_stride, batch, ct, 2 * PL, ph.u(), s);
    launch_ntt(cc, true, ph.u(), ph.u(), full_map(cc, cc.L), batch, s);
    decrypt_tail_big(e, sc, ph.u(), out, batch, s);
}
// SecretKey::measure_noise with a Large plaintext modulus: to_poly(m) comes from encode_big in Ntt form and is
// subtracted from the phase before the inverse transform (one forward transform more than the u64 path, whose loader
// subtracts in PowerBasis); m [batch][N][W_t] or null.
inline void measure_noise_big(const Encoder &e, const Scaler &sc, size_t level, const u64 *s_ntt, const u64 *ct,
                              size_t nparts, const u64 *m, u64 *noise_bits, size_t batch, hipStream_t s) {
    const Ctx &cc = *sc.from;
    if (!m) check_plain_context_big(e, sc);
    if (!batch) return;
    const u64 PL = (u64)cc.L * cc.n;
    WsGuard ph(batch * PL * sizeof(u64), s, true), mp(batch * PL * sizeof(u64), s, true);
    launch_phase(cc, s_ntt, ct, nparts, ph.u(), batch, s);
    std::unique_ptr<WsGuard> dec;
    if (!m) {
        dec = std::make_unique<WsGuard>(batch * cc.n * e.wt * sizeof(u64), s, true);
        launch_ntt(cc, true, ph.u(), mp.u(), full_map(cc, cc.L), batch, s);
        decrypt_tail_big(e, sc, mp.u(), dec->u(), batch, s);
        m = dec->u();
    }
    encode_big(e, false, true, level, m, e.n, mp.u(), batch, s);
    ew_op(cc, ph.u(), mp.u(), batch, k::EW_SUB, s);
    launch_ntt(cc, true, ph.u(), ph.u(), full_map(cc, cc.L), batch, s);
    centered_bits(cc, ph.u(), k::lift_sub_none(), noise_bits, batch, s);
}

// SecretKey::measure_noise (F/bfv/keys/secret_key.rs:55-98): the phase in PowerBasis minus Plaintext::to_poly of m --
// the ciphertext's own decryption (m == null, the reference) or the plaintext the caller expects, [batch][N] in
// [0, t) --, lifted and measured.  ct [batch][nparts][L][N] Ntt, s_ntt [L][N] -> noise_bits [batch].
inline void measure_noise(const Encoder &e, const Scaler &sc, const u64 *s_ntt, const u64 *ct, size_t nparts, const u64 *m,
                          u64 *noise_bits, size_t batch, hipStream_t s) {
    const Ctx &cc = *sc.from;
    cc.need_device();
    require(nparts >= 1, E_ARG, "a ciphertext has at least one part");
    size_t level = 0;
    const Ctx *lc = e.top;
    while (lc && !lc->same_ring(cc)) lc = lc->next.get(), level++;
    require(lc != nullptr, E_PARAMETER_MISMATCH, "the ciphertext context is not a level of the encoder's parameter set");
    require(e.top->device == cc.device, E_PARAMETER_MISMATCH, "the encoder and the scaler's context live on different devices");
    if (e.big()) return measure_noise_big(e, sc, level, s_ntt, ct, nparts, m, noise_bits, batch, s);
    if (!m) check_plain_context(sc);
    if (!batch) return;
    const u64 PL = (u64)cc.L * cc.n;
    // phase, decrypted coefficients (and centered_bits' partial maxima) are secret-dependent: cleared before reuse
    WsGuard ph(batch * PL * sizeof(u64), s, true);
    phase_power_basis(cc, s_ntt, ct, nparts, ph.u(), batch, s);
    std::unique_ptr<WsGuard> dec;
    if (!m) {
        dec = std::make_unique<WsGuard>(batch * cc.n * sizeof(u64), s, true);
        decrypt_tail(sc, e.t, ph.u(), dec->u(), batch, s);
        m = dec->u();
    }
    const u64 qmt = e.q_mod_t[level];
    centered_bits(cc, ph.u(), k::LiftSub{m, e.d_delta[level]->p, e.t, k::u64x2{qmt, shoup(qmt, e.t)}}, noise_bits, batch, s);
}

}  // namespace fhe
