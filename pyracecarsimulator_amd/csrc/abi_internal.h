// abi_internal.h — what the translation units of libscan_amd.so share: the owners of every device resource (DevBuf,
// DevPtr, Pinned, Stream, Event), HostCall (one synchronous host-pointer call: staging up, results down, the wait, and
// the drain of a call that is refused on the way), launch (THE kernel launch of every unit: typed by the kernel's own
// parameter list, asked at once, reported by name), the derived tables of a method (StepMap, LutTable, CddtTable,
// BlPadMaps, FanTabs: one struct each, owning its buffers, parameter block and cache) with their one cache protocol
// (TableCache), the handles behind include/scanlib.h's opaque pointers (rl_method: options, streams, staging, launch
// contexts and the five tables), the error slot, and the few internal entry points one unit calls in another.
//   abi_map.hip    errors, check_device, the caller's pinned host blocks, rl_map_* (EDT, bit map, edge list, stamps)
//   abi_fan.hip    rl_method_*: options, the tables' builds, the launch planner's C ABI, every fan / ray launch (told its
//                  noise offset, store mode and timing by LaunchArgs / FanCall below, not by the handle), the
//                  device-pointer entry points, the single-device host-pointer paths, the fused crash test; the
//                  particle-filter weights (repeat-angle scans, sensor model) and localisation (rl_pf_*)
//   abi_multi.hip  the host-pointer entry points and their multi-device forms (run_blocks below: one block per device)
//   abi_car.hip    roll-out generator, FollowGap, the policy network, batched races and the race scan; the closed-loop
//                  session (loop_args, SteerSource, Loop: the checks, who answers the scans, the locks and the
//                  scan-then-consume step of every closed loop) and its three users: the roll-outs (drive_loop), the driving
//                  environment (rl_env_*), the MCTS planner and its closed-loop drive (rl_mcts_*); 16-bit ranges,
//                  probes, the car-outline table and cells
#pragma once
// (the units are built with -fvisibility=hidden: only the C ABI leaves the library)
#pragma GCC visibility push(default)
#include "../../include/scanlib.h"
#pragma GCC visibility pop
#include "scan_params.h"
#include "literal_math.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

using namespace scan;

// ------------------------------------------------------------------------------
// errors (abi_map.hip): one message per thread
// ------------------------------------------------------------------------------
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
const std::string &last_error();
void set_last_error(const std::string &msg);
int fail_map_broken();           // RL_ERR_INVALID: what every call on a multi-device map answers once `broken` is set

#define HIPCHK(expr)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(RL_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                              \
    } while (0)


// is [p, p+bytes) inside a block of rl_host_alloc?  `device` >= 0: a launch on that device is about to write it
bool in_host_block(const void *p, size_t bytes, int device = -1);

// ------------------------------------------------------------------------------
// owners: every device buffer, pinned block, stream and event of a handle is held by one of these.  Move-only; each
// gives back what it holds in its destructor, so a handle is freed by `delete` and a failed create by leaving scope.
// None of them calls hipSetDevice: a *_destroy makes the handle's device current (and synchronises its streams) BEFORE
// it deletes.  This header is the only place that frees device memory, streams or events.
// ------------------------------------------------------------------------------
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    // exactly `bytes` (what was held is freed first): tables whose size is known
    int alloc(size_t bytes)
    {
        release();
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(RL_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        }
        cap = bytes;
        return RL_OK;
    }
    // at least `bytes`, grown by a quarter when too small: per-call staging (`cap` changes when the buffer was replaced)
    int ensure(size_t bytes) { return bytes <= cap ? (int)RL_OK : alloc(bytes + bytes / 4 + 256); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// a device array of T; reads as the T* the launches take.  A table is allocated by its bytes, per-call staging is sized
// by its ELEMENT count (a flattened record by its scalars: R * 11 doubles of car state, n * 3 floats of poses) and grows
// as DevBuf::ensure grows count * sizeof(T) bytes
template <class T>
struct DevPtr {
    DevBuf buf;
    int alloc(size_t bytes) { return buf.alloc(bytes); }
    int ensure(size_t count) { return buf.ensure(count * sizeof(T)); }
    void release() { buf.release(); }
    operator T *() const { return (T *)buf.p; }
};

// one raw handle and the call that gives it back (pinned blocks, streams, events)
template <class H, hipError_t (*Free)(H)>
struct Owned {
    H h = nullptr;
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : h(o.h) { o.h = nullptr; }
    Owned &operator=(Owned &&o) noexcept
    {
        if (this != &o) {
            release();
            h = o.h;
            o.h = nullptr;
        }
        return *this;
    }
    ~Owned() { release(); }
    void release()
    {
        if (h) (void)Free(h);
        h = nullptr;
    }
};
static inline hipError_t free_pinned(void *p) { return hipHostFree(p); }
static inline hipError_t free_stream(hipStream_t s) { return hipStreamDestroy(s); }
static inline hipError_t free_event(hipEvent_t e) { return hipEventDestroy(e); }

// pinned host memory of T, hipHostMallocDefault as at every site of the handles (what was held is freed first)
template <class T>
struct Pinned : Owned<void *, free_pinned> {
    hipError_t alloc(size_t bytes)
    {
        release();
        const hipError_t e = hipHostMalloc(&h, bytes, hipHostMallocDefault);
        if (e != hipSuccess) h = nullptr;
        return e;
    }
    operator T *() const { return (T *)h; }
};
// create() makes the stream / event on the first call and is a pointer test afterwards (those made on first use)
struct Stream : Owned<hipStream_t, free_stream> {
    hipError_t create() { return h ? hipSuccess : hipStreamCreateWithFlags(&h, hipStreamNonBlocking); }
    operator hipStream_t() const { return h; }
};
struct Event : Owned<hipEvent_t, free_event> {
    hipError_t create(unsigned flags = hipEventDefault) { return h ? hipSuccess : hipEventCreateWithFlags(&h, flags); }
    operator hipEvent_t() const { return h; }
};
static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_constructible<DevPtr<float>>::value &&
                  !std::is_copy_constructible<Pinned<int>>::value && !std::is_copy_constructible<Stream>::value &&
                  !std::is_copy_constructible<Event>::value,
              "an owner frees what it holds exactly once");

// One synchronous host-pointer call on stream `st`: the caller's arrays go up through a handle's staging, the launches
// follow on st, the results come down, finish() waits.  Every method is the HIP call it names, enqueued where it stands;
// counts are elements of T, and T has to agree between the host pointer and the buffer.  A call that returns before
// finish() — an argument a launch refuses, a failed HIP call — is drained by the destructor: nothing of it is left in
// flight, neither on the handle's staging nor into the caller's arrays.
struct HostCall {
    const hipStream_t st;
    bool finished = false;
    explicit HostCall(hipStream_t s) : st(s) {}
    HostCall(const HostCall &) = delete;
    HostCall &operator=(const HostCall &) = delete;
    ~HostCall()
    {
        if (!finished) (void)hipStreamSynchronize(st);
    }
    template <class T>
    int room(DevPtr<T> &b, size_t n)             // outputs and scratch: at least n elements
    {
        return b.ensure(n);
    }
    template <class T>
    int up(T *dev, const T *host, size_t n)      // into room made before (a buffer's second half)
    {
        HIPCHK(hipMemcpyAsync(dev, host, n * sizeof(T), hipMemcpyHostToDevice, st));
        return RL_OK;
    }
    template <class T>
    int up(DevPtr<T> &b, const T *host, size_t n)
    {
        const int rc = b.ensure(n);
        return rc ? rc : up((T *)b, host, n);
    }
    template <class T>
    int fill(DevPtr<T> &b, int byte, size_t n)   // every byte of n elements (0xff: NaN)
    {
        const int rc = b.ensure(n);
        if (rc) return rc;
        HIPCHK(hipMemsetAsync((T *)b, byte, n * sizeof(T), st));
        return RL_OK;
    }
    template <class T>
    int zero(DevPtr<T> &b, size_t n)
    {
        return fill(b, 0, n);
    }
    template <class T>
    int down(T *host_or_null, const T *dev, size_t n)
    {
        if (host_or_null) HIPCHK(hipMemcpyAsync(host_or_null, dev, n * sizeof(T), hipMemcpyDeviceToHost, st));
        return RL_OK;
    }
    template <class T>
    int down(T *host_or_null, const DevPtr<T> &dev, size_t n)
    {
        return down(host_or_null, (const T *)dev, n);
    }
    int finish()
    {
        finished = true;
        HIPCHK(hipStreamSynchronize(st));
        return RL_OK;
    }
};

// THE kernel launch of the library: `kernel` over grid x block with lds bytes on st, asked at once.  The kernel's own parameter
// list is what the arguments are converted to — a DevPtr<T> goes where T * or const T * is taken, nullptr where any
// pointer is, an int where a size_t is —, so a site writes no casts and an array of the wrong element type does not
// compile.  A launch the runtime refuses answers RL_ERR_HIP with `name` (the kernel's; the family's for a table entry) and
// HIP's reason; the caller enqueues nothing behind it.
template <class... P, class... A>
int launch(const char *name, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A &&...a)
{
    static_assert(sizeof...(P) == sizeof...(A), "one argument per kernel parameter");
    kernel<<<grid, block, lds, st>>>(static_cast<P>(std::forward<A>(a))...);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? (int)RL_OK : fail(RL_ERR_HIP, "%s launch failed: %s", name, hipGetErrorString(e));
}

// ------------------------------------------------------------------------------
// handles
// ------------------------------------------------------------------------------
struct rl_map {
    // a MULTI-DEVICE map (rl_map_create_multi) owns no device memory itself: it holds one ordinary map per
    // device in `reps` (the same device may appear several times) and its own fields describe the shape only
    std::vector<rl_map *> reps;
    int device = 0;
    int clock_khz = 0;
    int rows = 0, cols = 0;
    float res = 0, ox = 0, oy = 0, oyaw = 0;
    DevPtr<uint8_t> d_occ;
    DevPtr<uint8_t> d_occ_base;      // rl_map_stamp_cells: the occupancy as created / last rl_map_update'd (made at the first stamp)
    DevPtr<int32_t> d_stamp;         // ... the cell indices of the stamp in place (restored by the next one)
    Pinned<int32_t> pin_stamp;       // ... pinned, device-mapped landing buffer of a call's indices (no staging copy)
    int stamp_cap = 0, n_stamped = 0;
    DevPtr<int> d_g;             // EDT pass-1 scratch
    DevPtr<float> d_dt;
    DevPtr<uint32_t> d_bits;
    int bits_stride = 0;
    Stream stream;
    std::atomic<uint64_t> epoch{0};   // bumped by rl_map_update; derived tables rebuild lazily
    MapParams mp{};              // (kernels take it by value)
    // edge cells (occupied with a free 4-neighbour), the input of every CDDT table of this map: built
    // with the other map tables once a CDDT method exists, so that a table rebuild knows the count on
    // the host without a read-back of its own (rl_map_update synchronises anyway)
    bool want_edges = false;
    DevPtr<uint32_t> d_edges, d_n_edges;
    Pinned<uint32_t> pin_n_edges;
    uint32_t n_edges = 0;
    int n_cu = 256;
    std::mutex mu;
    // readers: every launch path of every method of this map (held for the whole call, i.e. until
    // the results of a host-pointer call have landed); writer: rl_map_update while it rewrites
    // occ / EDT / bit map.  A map callback thread and a scan thread may share the objects
    // (scripts/ros_interface.py:107-115).
    std::shared_mutex tables_mu;
    // MULTI-DEVICE map only.  readers: the multi_* host-pointer entry points of every method of this map, for the
    // whole batch (every device's block); writer: rl_map_update while it walks the replicas — so one batch is
    // never scanned partly on the old and partly on the new occupancy.  `broken`: an update failed after some
    // replicas had already taken the new cells; the handle then refuses every further call instead of answering
    // from two different maps.
    std::shared_mutex multi_mu;
    std::atomic<bool> broken{false};
};

// Per-launch scratch of a method (pose records, tile order, binning histograms, crash marks) is
// kept PER STREAM: a *_device call only enqueues work, so a second call on another stream may run
// concurrently with the first on the GPU (bench.py pipelines consecutive batches on two streams so
// that batch k+1 fills the CUs batch k's tail leaves idle).  Calls on one stream reuse one context
// in stream order.  More distinct streams than contexts: the least recently used context is handed
// over after a device synchronisation (rare, and needs no handle of the old stream, which the
// caller may have destroyed).
struct LaunchCtx {
    hipStream_t stream = nullptr;
    bool bound = false;
    uint64_t last_use = 0;
    DevBuf rec, rec_sorted, order, keys, hist, pose_first, dbg, d0, cddt_r;   // cddt_r: theta-major CDDT, R[raw bin][pose]
    DevBuf left_rec, left_cnt;     // hand-off march: the leftover list (rm_leftover_kernel), one region per wave of the main grid
    DevBuf pf_r;                   // particle-filter weights of the table kinds: the ranges between pf_angles_kernel and pf_eval_kernel
    int crash_epoch = 0;           // mark value of the last per-pose crash launch (pose_marks)
};
constexpr int N_LAUNCH_CTX = 8;      // (HIP's default 4 hardware queues carry 4 concurrent streams; GPU_MAX_HW_QUEUES=8 carries 8)

// ------------------------------------------------------------------------------
// derived tables: what a method builds from its map, lazily, on the stream of the call that needs it first.  One struct
// per table holds everything that belongs to it — device buffers, the parameter block the kernels take, host copies, its
// cache —, and one protocol (TableCache) says when a table is still good and what a reader or a rebuild has to wait for.
// The builds are in abi_fan.hip (build_* / ensure_*).
// ------------------------------------------------------------------------------
// launches on OTHER streams than the one a table was built on must not start before the build has finished
struct TableDep {
    Event ev;                    // (made by the first build)
    hipStream_t built_on = nullptr;
    bool pending = false;
    int built(hipStream_t stream)                // after (re)building the table on `stream`
    {
        HIPCHK(ev.create(hipEventDisableTiming));
        HIPCHK(hipEventRecord(ev, stream));
        built_on = stream;
        pending = true;
        return RL_OK;
    }
    int wait(hipStream_t stream)                 // before a launch on `stream` reads the table
    {
        if (!pending || stream == built_on) return RL_OK;      // (same stream: stream order)
        if (hipEventQuery(ev) == hipSuccess) {
            pending = false;
            return RL_OK;
        }
        HIPCHK(hipStreamWaitEvent(stream, ev, 0));
        return RL_OK;
    }
};

// The cache protocol of a table that follows the map: fresh_for(map) ? wait(stream) : begin_rebuild(), the build
// enqueued on `stream`, built(map, stream).  A table is good for exactly the map epoch it was stamped with, and it is
// stamped only once its build is enqueued and its event recorded: a build that fails on the way leaves it stale.
struct TableCache {
    static constexpr uint64_t NEVER = ~0ull;
    uint64_t epoch = NEVER;      // map epoch the table was built from
    bool begun = false;          // a build has been started before: launches of other streams may still read that copy
    TableDep dep;
    bool fresh_for(const rl_map *m) const { return epoch == m->epoch; }
    int wait(hipStream_t stream) { return dep.wait(stream); }
    int begin_rebuild()
    {
        epoch = NEVER;
        if (begun) HIPCHK(hipDeviceSynchronize());
        begun = true;
        return RL_OK;
    }
    int built(const rl_map *m, hipStream_t stream)
    {
        const int rc = dep.built(stream);
        if (rc == RL_OK) epoch = m->epoch;
        return rc;
    }
    void invalidate() { epoch = NEVER; }         // (an option the table was built with changed)
};

namespace scan { struct PadMap; }

// Ray marching: the step map — the EDT with a border of `pad` cells of -1, holding the march's step — and, built next
// to it, the CODE map (option code_map = 2): the step map as u16 palette codes + the palette (rm_kernels.h).
struct StepMap {
    struct Addr {                // the march's address constants of one copy
        size_t base_off;         // tiled: the column bias (pad << 4 bytes) folded into the base address
        int stride;              // elements per row (row-major) | M (tiled, see pdt_tiled_byte)
        uint32_t k4, mask;
    };
    DevBuf pdt;
    Addr at{};
    int pad = 0;
    int tiled = -1;              // layout the copy was built with
    // code_n = palette entries with the two stop codes, 0 = none (option off, geometry does not fit, or more distinct
    // steps than plan::CODE_MAX_ENTRIES)
    DevBuf cmap, cval, cidx, ctab, cnum;
    Pinned<uint32_t> pin_cnum;   // (made with the first code map)
    int code_n = 0;
    int code_built = -1;         // code_map value the tables were built for
    Addr code_at{};
    TableCache cache;
    // THE freshness test: built from this map, in the layout these options ask for, for this code_map option
    bool fresh_for(const rl_map *m, float max_range, const rl_plan_opts &o) const;
    // palette size a plan for this map and these options may count on (0: no code map, or not the one built)
    int code_entries_for(const rl_map *m, float max_range, const rl_plan_opts &o) const;
    // the march's address constants of the float32 map, or of the code map
    scan::PadMap pad_map(bool code, float res) const;
};

struct LutTable {                // GiantLUT (K3)
    DevBuf buf;
    LutParams lp{};
    TableCache cache;
};

struct CddtTable {               // CDDT (K3b)
    DevBuf cos, sin, trans, width, boff, offsets, xs2, cursor, tmp, hdr, tab;
    CddtParams cdp{};
    uint32_t buckets = 0;
    std::vector<float> h_cos, h_sin, h_trans;              // per-bin constants (host copies stay alive:
    std::vector<int> h_width;                              //  their uploads are asynchronous)
    std::vector<uint32_t> h_boff;
    int geom_rows = -1, geom_cols = -1;                    // map shape the constants were made for
    bool sort_attr = false;
    bool counts_clean = false;                             // bucket counters are all zero (see build_cddt)
    int lds_sort = (int)CDDT_LDS_SORT;                     // buckets up to this size are sorted in LDS (diagnostics: lower it)
    TableCache cache;
};

struct BlPadMaps {               // K2b: padded normal + transposed bit maps (bl_pad_bits_kernel)
    DevBuf buf;
    BlPad blp{};
    TableCache cache;
};

// beam-direction tables (cos, sin per beam) of the fans a handle has been called with: they depend on the fan, not on
// the map, so each has the dependency half of the protocol only
struct FanTabs {
    struct Tab {
        uint32_t fov_bits = 0;
        int num_rays = 0;
        uint64_t last_use = 0;
        DevBuf tab;
        TableDep dep;
    } tabs[4];
    uint64_t clock = 0;
};


// ------------------------------------------------------------------------------
// Several devices behind one handle (rl_map_create_multi): a single-process caller — the reference's
// scanMany / checkCollisionMany callers are ONE Python process (scripts/mcts.py:237,
// scripts/scan_simulator.py:113-135) — hands over one batch and every device takes a contiguous block of
// it.  One persistent worker thread per device (bound to it with hipSetDevice once) runs the ordinary
// single-device entry point on that device's replica handle; replica 0's block runs on the calling thread.
// Threads and streams only: nothing is forked or re-executed after the GPU has been initialised.
// run_blocks (below) is the one place that says which replica takes which block; how many blocks a batch
// is cut into is decided where it is called (multi_parts and its kin).
// ------------------------------------------------------------------------------
struct MultiPool {
    struct Worker {
        std::thread th;
        std::mutex mu;
        std::condition_variable cv;
        const std::function<int()> *job = nullptr;
        bool has = false, done = false, stop = false;
        int rc = 0;
        std::string err;
        int device = 0;
    };
    std::vector<std::unique_ptr<Worker>> w;

    void start(const std::vector<int> &devices)
    {
        for (size_t i = 1; i < devices.size(); ++i) {       // (replica 0 has the caller's thread)
            auto wk = std::make_unique<Worker>();
            wk->device = devices[i];
            Worker *raw = wk.get();
            wk->th = std::thread([raw]() {
                (void)hipSetDevice(raw->device);
                std::unique_lock<std::mutex> lk(raw->mu);
                for (;;) {
                    raw->cv.wait(lk, [raw]() { return raw->has || raw->stop; });
                    if (raw->stop) return;
                    raw->has = false;
                    lk.unlock();
                    const int rc = (*raw->job)();
                    std::string msg = rc ? last_error() : std::string();
                    lk.lock();
                    raw->rc = rc;
                    raw->err = std::move(msg);
                    raw->done = true;
                    raw->cv.notify_all();
                }
            });
            w.push_back(std::move(wk));
        }
    }

    // jobs[i], where there is one, runs on replica i's thread (jobs[0] on the caller's; a replica without a job is
    // not woken); the failure of the lowest replica index is reported, its message becomes the caller's rl_last_error
    int run(const std::vector<std::function<int()>> &jobs)
    {
        if (jobs.size() > w.size() + 1)
            return fail(RL_ERR_INVALID, "internal: %zu pose blocks for %zu devices", jobs.size(), w.size() + 1);
        for (size_t i = 1; i < jobs.size(); ++i) {
            if (!jobs[i]) continue;
            Worker &x = *w[i - 1];
            std::lock_guard<std::mutex> lk(x.mu);
            x.job = &jobs[i];
            x.has = true;
            x.done = false;
            x.cv.notify_all();
        }
        int rc = !jobs.empty() && jobs[0] ? jobs[0]() : (int)RL_OK;
        std::string err = rc ? last_error() : std::string();
        for (size_t i = 1; i < jobs.size(); ++i) {
            if (!jobs[i]) continue;
            Worker &x = *w[i - 1];
            std::unique_lock<std::mutex> lk(x.mu);
            x.cv.wait(lk, [&x]() { return x.done; });
            if (rc == RL_OK && x.rc != RL_OK) {
                rc = x.rc;
                err = x.err;
            }
        }
        if (rc) set_last_error(err);
        return rc;
    }

    ~MultiPool()
    {
        for (auto &x : w) {
            {
                std::lock_guard<std::mutex> lk(x->mu);
                x->stop = true;
                x->cv.notify_all();
            }
            if (x->th.joinable()) x->th.join();
        }
    }
};

// contiguous block of `rank` when n items are cut into `parts` (the same split as workloads.shard_range)
static inline void block_of(long n, int rank, int parts, long &lo, long &hi)
{
    const long base = n / parts, rem = n % parts;
    lo = rank * base + std::min<long>(rank, rem);
    hi = lo + base + (rank < rem ? 1 : 0);
}

// THE block scheduler of every multi-device entry point: n_units are cut into k contiguous blocks (k <= replicas) and
// job(block) runs for every block that is not empty, replica i's on replica i's thread.  Block 0 goes to replica
// `first` — 0, or the consumer of a device-resident call, so that a batch too small for every device stays where it
// is wanted — and the following blocks to the remaining replicas in index order.  Errors as MultiPool::run.
struct MultiBlock {
    int index, replica;
    long lo, hi;                 // the block's units [lo, hi)
};

template <class Job>
static inline int run_blocks(MultiPool &pool, long n_units, int k, int first, const Job &job)
{
    std::vector<std::function<int()>> jobs(std::max<size_t>(pool.w.size() + 1, (size_t)k));
    for (int b = 0; b < k; ++b) {
        MultiBlock blk{b, b == 0 ? first : (b <= first ? b - 1 : b), 0, 0};
        block_of(n_units, b, k, blk.lo, blk.hi);
        if (blk.hi > blk.lo) jobs[blk.replica] = [&job, blk]() { return job(blk); };
    }
    return pool.run(jobs);
}

struct rl_method {
    // multi-device method (created on a multi-device map): one ordinary method per device + the worker pool;
    // the parent keeps kind / noise / options and owns no device memory
    std::vector<rl_method *> reps;
    std::unique_ptr<MultiPool> pool;
    int multi_min_poses = 512;   // a device is only brought in per this many poses: waking a worker costs ~18 us
                                 // (profiles/r04/host_pointer_rate.txt: a 200-pose roll-out cut over three contexts 60 vs
                                 // 42 us), a 512-pose block's transfer alone ~50 us — the reference's roll-out stays on one device
    rl_map *map = nullptr;
    int kind = 0;
    float max_range = 0;
    float step_coeff = 0.999f;
    int theta_disc = 0;
    float noise_std = 0;
    uint64_t noise_seed = 0, ray_offset = 0;
    rl_plan_opts opt{};          // the planner's options: plan::default_opts with variant = the kind's default (opts_of adds
                                 // code_entries); rl_method_set_option's option table names which of them an option sets
    int timing = 0;              // 1: HIP events around every launch sequence (rl_last_kernel_ms);
                                 // 2: around the march kernel only (pose binning excluded)
    int drain_prio = 0;
    int spec_drain = 8;          // one ray per lane: value-speculating drain loop once <= this many lanes are live (0 = off)
    int spec_stretch = 16;       //   ... after this many plain samples, and between two attempts whose first prediction failed
    int drain_cap = 64;          // several rays per lane: compact a wave's last rays into one slot from <= this many (<= 64)
    int drain_stretch = 8;       //   ... plain samples between two speculation attempts of the compacted rays
    int group_drain = 0;         //   ... and from 2 N / N live rays down 2 / 4 lanes per ray, 8 / 16 samples per round trip (N <= 16; 0: off)
    int handoff = 0;             // several rays per lane, 1: a dry wave hands its last <= handoff_cap rays to rm_leftover_kernel (the
                                 // next launch on the stream) instead of draining them in place (0: drain in place)
    int handoff_cap = 16;        //   ... rays per wave handed over (8, 16, 32 or 64)
    int handoff_wg = 256;        //   ... workgroup size of the leftover launch (64, 128 or 256)
    int nt_store = 1;            // ranges leave the stream kernels with non-temporal stores (0: plain — a consumer kernel reads them next)
    // the derived tables (above): which of them a handle ever builds follows from its kind
    StepMap step;
    LutTable lut;
    CddtTable cddt;
    BlPadMaps blpad;
    FanTabs fans;
    Stream stream;
    Stream copy_stream;                  // big host-pointer calls (made by the first one): the D2H copy of pose slice k overlaps the march of slice k+1
    Event slice_ev[4];
    int overlap_min_rays = 1 << 24;      // ... from this many rays per call (0 = never); below ~16 k poses the slices cost more than they hide
    Event ev0, ev1;
    bool timed = false;
    // the host-pointer forms' staging: (x, y, theta) rows, ranges, hit cells (2 per ray), step counts, the car-outline
    // table, crash indices
    DevPtr<float> poses, outs;
    DevPtr<int32_t> hits;
    DevPtr<uint16_t> steps;
    DevPtr<double> edge;
    DevPtr<int> flag;
    DevPtr<double> cars;         // rl_calc_range_fan_cars: the cars' (x, y, theta) rows
    // particle-filter weights (pf_kernels.h): the sensor-model table (rl_set_sensor_model; width 0 = none set) and the
    // host-pointer forms' staging of angles, observation and weights
    DevPtr<double> sensor;
    int sensor_w = 0;
    DevPtr<float> pf_ang, pf_obs;
    DevPtr<double> pf_w;
    int pf_block = 0;            // particles per tile of the weight kernels (0: sized from the shape, make_pf)
    int lut_refine = 0;          // GiantLUT: the origin-corrected query (lut_kernels.h) in every query path; other kinds ignore it
    int race_cddt = 0;           // CDDT: batched races on the table (cddt_kernels.h race_cddt_kernel); other kinds ignore it
    LaunchCtx ctx[N_LAUNCH_CTX];
    uint64_t use_clock = 0;
    // small host calls (scan(): one pose, scanMany(): a roll-out): poses and ranges go through ONE
    // pinned, device-mapped host buffer the kernels read / write directly — no staging copies
    Pinned<char> pin;
    size_t pin_cap = 0;
    int pinned_max_rays = 262144; // 0 = always stage through device buffers
    int direct_max_rays = 1 << 21; // a result buffer in a pinned block of rl_host_alloc is written by the kernel itself
                                  // up to this many rays (a 200-pose roll-out: 41 vs 61 us, 1024 poses: 113 vs 132); larger
                                  // batches go HBM -> DMA into the pinned block, which moves 4 B per ray faster than the
                                  // kernel's stores over PCIe (4096 poses: 394 vs 449 us; a tie at 2048:
                                  // profiles/r04/host_pointer_rate.txt)
    std::vector<double> edge_host; // the car-outline table last uploaded to `edge` (re-sent only when it changes)
    Pinned<int> pin_flag;          // pinned landing slot for the crash index
    int tile_stripe = -1;        // binning order: tile rows per stripe walked column-major (rm_kernels.h tile_key); 0: row-major, -1: by xcd_bands
    int bin_ppw = POSES_PER_WG;  // ... poses per workgroup of those kernels
    int last_grid = 0;
    void *last_dbg = nullptr;    // stamps buffer of the last launch (in its context)
    rl_launch_plan last_plan{};  // what the last fan launch of this handle was planned as (plan::plan_fan)
    std::vector<float> h_poses;
    std::mutex mu;
};

// A multi-device method for the length of one batch: h->mu (together with the mutexes of `also`, e.g. the car's of a
// roll-out chain) and the map's multi_mu (shared) are held while it lives, the handle's noise is read once, and run()
// refuses a broken map, then hands the batch to run_blocks with the replica's noise set before each block's job — keyed
// by the GLOBAL ray id: the parent's offset + the rays before the block (rays_per_unit each unit).
template <class... Also>
struct MultiCall {
    rl_method *const h;
    std::scoped_lock<Also..., std::mutex> lk;
    std::shared_lock<std::shared_mutex> ml;
    const float nstd;
    const uint64_t seed, off;
    explicit MultiCall(rl_method *m, Also &...also)
        : h(m), lk(also..., m->mu), ml(m->map->multi_mu), nstd(m->noise_std), seed(m->noise_seed), off(m->ray_offset)
    {
    }
    template <class Job>
    int run(MultiPool &pool, long n_units, int k, int first, uint64_t rays_per_unit, const Job &job) const
    {
        if (h->map->broken.load()) return fail_map_broken();
        return run_blocks(pool, n_units, k, first, [&](const MultiBlock &b) {
            const int rc = rl_set_noise(h->reps[b.replica], nstd, seed, off + (uint64_t)b.lo * rays_per_unit);
            return rc ? rc : job(b);
        });
    }
};

// the 64-bit seed of a Philox stream folded to its 32-bit key (np_statement.noise_key; scan_device.h folds the scan
// noise's seed the same way on the device)
static inline uint32_t noise_key(uint64_t seed) { return (uint32_t)seed ^ ((uint32_t)(seed >> 32) * 0x85EBCA6Bu); }

int set_device(const rl_map *m);
int check_device(int device);                       // RL_ERR_NO_DEVICE unless `device` names a visible HIP device; abi_map.hip
int map_build_tables(rl_map *m);                    // EDT + bit map (+ edge list once a CDDT method exists); abi_map.hip
void host_sincosf(float x, float &s, float &c);      // host twin of scan::det_sincosf (abi_map.hip)

// ------------------------------------------------------------------------------
// abi_fan.hip, called from abi_multi.hip / abi_car.hip
// ------------------------------------------------------------------------------
int check_fan_args(const rl_method *h, int n_poses, float fov, int num_rays);
FanParams make_fan(const rl_method *h, int n_poses, float fov, int num_rays, uint64_t ray_offset);   // + the handle's range, coefficient, noise
LiteralParams make_literal(const rl_map *m);                                     // variant 3's per-map constants
namespace scan { struct CrashParams; }

// What a launch is told instead of reading it off the handle.  rl_set_noise and rl_method_set_option are the only writers
// of h->ray_offset, h->nt_store and h->timing; a path that needs another value for one launch (a pose slice, a closed
// loop's tick, a filter step) says so here.  The events and h->timed, last_plan, last_grid, last_dbg stay on the handle:
// they are results.
struct LaunchArgs {
    uint64_t ray_offset;         // global id of the launch's first ray (keys its noise)
    bool plain_store;            // ranges leave the stream kernels with plain stores: a consumer kernel reads them next
    int timing;                  // as the option: 1 events around the launch sequence, 2 around the march kernel only
    static LaunchArgs of(const rl_method *h) { return {h->ray_offset, !h->nt_store, h->timing}; }   // the caller's settings
};

// one fan launch: launch_fan's arguments
struct FanCall : LaunchArgs {
    const float *d_poses;
    int n_poses;
    float fov;
    int num_rays;
    float *d_out;
    int32_t *d_hits;
    uint16_t *d_steps;
    const CrashParams *crash;
    hipStream_t stream;
    // the call for poses [p0, p0 + np): every pointer and the noise offset move on by the poses (rays) before p0.  A
    // per-pose-mark crash test marks through *marks, the slice's own copy with the mark array shifted by p0 (it has to
    // live as long as the slice; not needed without a crash test)
    FanCall slice(int p0, int np, CrashParams *marks = nullptr) const;
};
// one fan launch sequence as the planner picks it (the caller holds h->mu and the map's tables_mu and has checked the
// arguments)
int launch_fan(rl_method *h, const FanCall &c);
int fan_host(rl_method *h, const float *poses, int n_poses, float fov, int num_rays, float *outs, int32_t *hits,
             uint16_t *steps, const double *edge, double crash_thresh, int *first_crashed);
int crash_groups_device(rl_method *h, const LaunchArgs &a, const float *d_poses, int n_groups, int group, float fov,
                        int num_rays, const double *d_edge, double thresh, int *d_first, float *d_ranges, hipStream_t stream);
int upload_edge(rl_method *h, const double *edge, int num_rays);
int rays_host(rl_method *h, const float *ins, float *outs, int n);
int check_groups_args(int n_groups, int group);     // the grouped crash tests' first two checks
int multi_parts(const rl_method *h, long n_poses);
namespace scan { struct RaceParams; }
// one race_cddt_kernel launch of a CDDT handle with option race_cddt (launch_race, abi_car.hip: same caller's duties)
int launch_race_cddt(rl_method *h, const LaunchArgs &a, const FanParams &f, const RaceParams &rp, const float *d_poses,
                     float *d_out, hipStream_t stream);
