// abi_fan.hip — the method handle of libscan_amd.so (C ABI: include/scanlib.h): options, derived tables, launch planning,
// every fan / ray launch, the device-pointer entry points, the single-device host-pointer paths, the fused crash test.
//
// Replaces, for the scan path only, range_libc's PyRayMarching / PyRayMarchingGPU / PyBresenhamsLine / PyCDDTCast /
// PyGiantLUTCast objects that the reference builds at scripts/scan_simulator.py:72-76, scripts/ros_interface.py:210 and
// scripts/two_player/scan.py:45-46.  There is no CPU fallback in this library.
#include "abi_internal.h"
#include "scan_kernels.h"
#include "crash_kernels.h"
#include "pf_kernels.h"
#include "mcl_kernels.h"
#include "launch_plan.h"

#include <array>
#include <utility>

static_assert(plan::WG == scan::WG && plan::STREAM_HDR == scan::STREAM_HDR && plan::STRIPE_BINS == scan::STRIPE_BINS &&
                  plan::STRIPE_MAX_PER_LANE == scan::STRIPE_MAX_PER_LANE && plan::DRAIN_CAP == scan::DRAIN_CAP &&
                  plan::DRAIN_FIELDS == scan::DRAIN_FIELDS && plan::INLINE_REC_BYTES == (int)sizeof(scan::BlockRec),
              "launch_plan.h and rm_kernels.h disagree about the stream kernels' LDS layout");

// ------------------------------------------------------------------------------
// method
// ------------------------------------------------------------------------------
extern "C" int rl_method_create(rl_map *m, int kind, float max_range_px, int theta_disc,
                                rl_method **out)
{
    if (!m || !out) return fail(RL_ERR_INVALID, "rl_method_create: null pointer");
    if (!(max_range_px > 0.0f)) return fail(RL_ERR_INVALID, "max_range_px must be > 0");
    if (kind < RL_BRESENHAM || kind > RL_GIANT_LUT)
        return fail(RL_ERR_INVALID, "unknown range method kind %d", kind);
    if ((kind == RL_CDDT || kind == RL_GIANT_LUT) && (theta_disc < 2 || theta_disc > 65536))
        return fail(RL_ERR_INVALID, "theta_disc must be in [2, 65536] for CDDT / GiantLUT (got %d)",
                    theta_disc);
    std::unique_ptr<rl_method, decltype(&rl_method_destroy)> own(new (std::nothrow) rl_method(), rl_method_destroy);
    rl_method *h = own.get();
    if (!h) return fail(RL_ERR_NOMEM, "out of host memory");
    h->map = m;
    h->kind = kind;
    h->max_range = max_range_px;
    h->theta_disc = theta_disc;
    h->step_coeff = kind == RL_RM_GPU ? 1.0f : 0.999f;   // kernels.cu STEP_COEFF vs RayMarching (also seeds the LUT)
    plan::default_opts(h->opt);
    h->opt.variant = plan::default_variant(kind);         // RL_RM: the upstream-literal arithmetic; the others canonical
    if (!m->reps.empty()) {
        // multi-device: one ordinary method per device replica of the map + one worker thread per extra device
        std::vector<int> devs;
        for (rl_map *rm : m->reps) {
            rl_method *r = nullptr;
            const int rc = rl_method_create(rm, kind, max_range_px, theta_disc, &r);
            if (rc) {
                const std::string keep = last_error();     // (the failing replica's message outlives the clean-up)
                own.reset();
                set_last_error(keep);
                return rc;
            }
            h->reps.push_back(r);
            devs.push_back(rm->device);
        }
        h->pool = std::make_unique<MultiPool>();
        h->pool->start(devs);
        *out = own.release();
        return RL_OK;
    }
    if (kind == RL_CDDT) {
        // the map starts keeping its edge list (and rebuilds it with every rl_map_update)
        std::lock_guard<std::mutex> lk(m->mu);
        std::unique_lock<std::shared_mutex> wl(m->tables_mu);
        if (!m->want_edges) {
            m->want_edges = true;
            int rc_ = hipSetDevice(m->device) == hipSuccess ? map_build_tables(m) : fail(RL_ERR_HIP, "hipSetDevice failed");
            if (rc_) {
                m->want_edges = false;
                return rc_;
            }
        }
    }
    if (hipSetDevice(m->device) != hipSuccess || h->stream.create() != hipSuccess || h->ev0.create() != hipSuccess ||
        h->ev1.create() != hipSuccess)
        return fail(RL_ERR_HIP, "stream/event creation failed");
    *out = own.release();
    return RL_OK;
}

extern "C" void rl_method_destroy(rl_method *h)
{
    if (!h) return;
    if (!h->reps.empty() || h->pool) {
        h->pool.reset();                       // (joins the workers: no job is in flight, the caller owns the handle)
        for (rl_method *r : h->reps) rl_method_destroy(r);
        delete h;
        return;
    }
    if (h->map) (void)hipSetDevice(h->map->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    delete h;
}

extern "C" int rl_method_kind(const rl_method *h) { return h ? h->kind : -1; }

extern "C" int rl_method_n_devices(const rl_method *h) { return h ? (h->reps.empty() ? 1 : (int)h->reps.size()) : 0; }

extern "C" rl_method *rl_method_replica(rl_method *h, int i)
{
    if (!h) return nullptr;
    if (h->reps.empty()) return i == 0 ? h : nullptr;
    return (i >= 0 && i < (int)h->reps.size()) ? h->reps[i] : nullptr;
}

static int cddt_table_stats(rl_method *h, const char *name, int64_t *value_out);

// how many devices of a multi-device handle a batch of n_poses is cut over
int multi_parts(const rl_method *h, long n_poses)
{
    const long by_size = n_poses / std::max(h->multi_min_poses, 1);
    return (int)std::max<long>(1, std::min<long>((long)h->reps.size(), by_size));
}

static int multi_needs_replica(const char *fn)
{
    return fail(RL_ERR_INVALID, "%s: device pointers belong to one device — on a multi-device handle call it with "
                                "rl_method_replica(h, i)", fn);
}

extern "C" int rl_set_noise(rl_method *h, float std, uint64_t seed, uint64_t ray_offset)
{
    if (!h) return fail(RL_ERR_INVALID, "rl_set_noise: null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    h->noise_std = std;
    h->noise_seed = seed;
    h->ray_offset = ray_offset;
    return RL_OK;
}

// Every option of a handle: where its value lives — a planner option (rl_plan_opts field) or a tunable of the handle
// itself —, how rl_method_set_option brings a value into range (nullptr: stored as given), and what else has to follow
// once the value is stored (nullptr: nothing).  get_info reads the same field back.
struct OptionRow {
    const char *name;
    int &(*at)(rl_method *);
    int (*clamp)(int);
    void (*stored)(rl_method *, int);
};
#define PLAN(field) [](rl_method *h) -> int & { return h->opt.field; }
#define OWN(field) [](rl_method *h) -> int & { return h->field; }
static int clamp_int(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static int as_bool(int v) { return v != 0; }
static const OptionRow OPTIONS[] = {
    {"variant", PLAN(variant), nullptr},            // (< 0: the kind's default, rl_method_set_option)
    {"grid_mult", PLAN(grid_mult), [](int v) { return std::max(v, 1); }},
    {"wg_threads", PLAN(wg_threads), [](int v) { return v >= 1024 ? 1024 : (v >= 512 ? 512 : 256); }},
    {"low_water", PLAN(low_water), [](int v) { return v < 0 ? -1 : std::min(v, 63); }},
    {"sort_poses", PLAN(sort_poses), as_bool},
    {"xcd_bands", PLAN(xcd_bands), [](int v) { return std::max(v, 1); }},
    {"slots", PLAN(slots), [](int v) { return v >= 3 ? 3 : std::max(v, 0); }},
    {"tiled", PLAN(tiled), as_bool},
    {"inline_prep", PLAN(inline_prep), as_bool},
    {"inline_max", PLAN(inline_max), nullptr},
    {"inline_map_kb", PLAN(inline_map_kb), [](int v) { return std::max(v, 0); }},
    {"stripe_max", PLAN(stripe_max), [](int v) { return std::max(v, 0); }},
    {"order_inline", PLAN(order_inline), as_bool},
    {"bin_multi_min", PLAN(bin_multi_min), nullptr},
    {"bin_generic", PLAN(bin_generic), as_bool},
    {"run_log2", PLAN(run_log2), [](int v) { return v < 0 ? -1 : std::min(v, 8); }},
    {"cddt_bins", PLAN(cddt_bins), as_bool},
    {"cddt_sort", PLAN(cddt_sort), as_bool},
    {"lut_debug", PLAN(lut_debug), nullptr, [](rl_method *h, int v) { h->lut.lp.debug = h->cddt.cdp.debug = v; }},
    {"debug_stamps", PLAN(debug_stamps), as_bool},
    {"slice_log2", PLAN(slice_log2), [](int v) { return clamp_int(v, 8, 30); }},
    {"cddt_theta_min", PLAN(cddt_theta_min), [](int v) { return std::max(v, 0); }},
    {"cddt_search", PLAN(cddt_search), [](int v) { return clamp_int(v, 0, 2); }},
    {"code_map", PLAN(code_map), [](int v) { return v == 2 ? 2 : 0; }},
    {"code_min_rays", PLAN(code_min_rays), [](int v) { return std::max(v, 0); }},
    {"tail_pct", PLAN(tail_pct), [](int v) { return clamp_int(v, 0, 75); }},
    {"tail_wg_pct", PLAN(tail_wg_pct), [](int v) { return clamp_int(v, 10, 400); }},
    {"timing", OWN(timing), [](int v) { return clamp_int(v, 0, 2); }},
    {"drain_prio", OWN(drain_prio), as_bool},
    {"spec_drain", OWN(spec_drain), [](int v) { return clamp_int(v, 0, 64); }},
    {"spec_stretch", OWN(spec_stretch), [](int v) { return clamp_int(v, 1, 4096); }},
    {"drain_cap", OWN(drain_cap), [](int v) { return clamp_int(v, 1, 64); }},
    {"drain_stretch", OWN(drain_stretch), [](int v) { return clamp_int(v, 1, 4096); }},
    {"group_drain", OWN(group_drain), [](int v) { return clamp_int(v, 0, 16); }},
    {"handoff", OWN(handoff), as_bool},
    {"handoff_cap", OWN(handoff_cap), [](int v) { return v >= 64 ? 64 : (v >= 32 ? 32 : (v >= 16 ? 16 : 8)); }},
    {"handoff_wg", OWN(handoff_wg), [](int v) { return v >= 256 ? 256 : (v >= 128 ? 128 : 64); }},
    {"nt_store", OWN(nt_store), as_bool},
    {"bin_ppw", OWN(bin_ppw), [](int v) { return clamp_int(v, 256, 8192); }},
    {"tile_stripe", OWN(tile_stripe), [](int v) { return v < 0 ? -1 : std::min(v, 4096); }},
    {"pinned_max_rays", OWN(pinned_max_rays), [](int v) { return std::max(v, 0); }},
    {"direct_max_rays", OWN(direct_max_rays), [](int v) { return std::max(v, 0); }},
    {"overlap_min_rays", OWN(overlap_min_rays), [](int v) { return std::max(v, 0); }},
    {"pf_block", OWN(pf_block), [](int v) { return clamp_int(v, 0, PF_WG); }},
    // (the origin-corrected GiantLUT query; stored and ignored by the other kinds, as lut_debug is)
    {"lut_refine", OWN(lut_refine), as_bool},
    // (batched races on the CDDT table, race_args in abi_car.hip; stored and ignored by the other kinds)
    {"race_cddt", OWN(race_cddt), as_bool},
    // (a power of two in [128, CDDT_LDS_SORT]: the bitonic network pads to one)
    {"cddt_lds_sort", OWN(cddt.lds_sort), [](int v) {
         int p = 128;
         while (p * 2 <= v && p * 2 <= (int)CDDT_LDS_SORT) p *= 2;
         return p;
     }, [](rl_method *h, int) { h->cddt.cache.invalidate(); }},      // (the table is rebuilt with the new bound)
};
#undef PLAN
#undef OWN

static const OptionRow *find_option(const char *name)
{
    for (const OptionRow &r : OPTIONS)
        if (!strcmp(name, r.name)) return &r;
    return nullptr;
}

extern "C" int rl_method_set_option(rl_method *h, const char *name, int value)
{
    if (!h || !name) return fail(RL_ERR_INVALID, "rl_method_set_option: null pointer");
    if (!h->reps.empty()) {
        std::lock_guard<std::mutex> lk(h->mu);
        if (!strcmp(name, "multi_min_poses")) {
            h->multi_min_poses = value < 1 ? 1 : value;
            return RL_OK;
        }
        for (rl_method *r : h->reps) {
            const int rc = rl_method_set_option(r, name, value);
            if (rc) return rc;
        }
        return RL_OK;
    }
    std::lock_guard<std::mutex> lk(h->mu);
    const OptionRow *row = find_option(name);
    if (!row) return fail(RL_ERR_INVALID, "unknown option '%s'", name);
    if (!strcmp(name, "variant") && value < 0) value = plan::default_variant(h->kind);
    const int stored = row->at(h) = row->clamp ? row->clamp(value) : value;
    if (row->stored) row->stored(h, stored);
    return RL_OK;
}

extern "C" int rl_method_get_info(rl_method *h, const char *name, int64_t *value_out)
{
    if (!h || !name || !value_out) return fail(RL_ERR_INVALID, "rl_method_get_info: null pointer");
    if (!strcmp(name, "n_devices")) { *value_out = h->reps.empty() ? 1 : (int64_t)h->reps.size(); return RL_OK; }
    if (!h->reps.empty()) {
        if (!strcmp(name, "multi_min_poses")) { *value_out = h->multi_min_poses; return RL_OK; }
        return rl_method_get_info(h->reps[0], name, value_out);
    }
    if (!strcmp(name, "cddt_values") || !strcmp(name, "cddt_buckets") || !strcmp(name, "cddt_nonempty_buckets"))
        return cddt_table_stats(h, name, value_out);
    // (read-only)
    if (!strcmp(name, "n_cu")) *value_out = h->map->n_cu;
    else if (!strcmp(name, "clock_khz")) *value_out = h->map->clock_khz;
    else if (!strcmp(name, "code_entries")) *value_out = h->step.code_n;
    else if (!strcmp(name, "last_grid")) *value_out = h->last_grid;
    else if (!strcmp(name, "map_epoch")) *value_out = (int64_t)h->map->epoch;
    else if (const OptionRow *row = find_option(name)) *value_out = row->at(h);
    else return fail(RL_ERR_INVALID, "unknown info '%s'", name);
    return RL_OK;
}

// ------------------------------------------------------------------------------
// launches
// ------------------------------------------------------------------------------
FanParams make_fan(const rl_method *h, int n_poses, float fov, int num_rays, uint64_t ray_offset)
{
    FanParams f{};
    f.n_poses = n_poses;
    f.num_rays = num_rays;
    f.amin = -0.5f * fov;
    f.inc = fov / (float)num_rays;
    f.max_range = h->max_range;
    f.step_coeff = h->step_coeff;
    f.noise_std = h->noise_std;
    f.noise_seed = h->noise_seed;
    f.ray_offset = ray_offset;
    return f;
}

int check_fan_args(const rl_method *h, int n_poses, float fov, int num_rays)
{
    if (!h) return fail(RL_ERR_INVALID, "null method handle");
    if (n_poses < 0) return fail(RL_ERR_INVALID, "n_poses must be >= 0");
    if (num_rays <= 0) return fail(RL_ERR_INVALID, "num_rays must be > 0");
    if (num_rays > 7680)      // 8 B per beam in LDS next to the other per-workgroup state (<= 64 KiB)
        return fail(RL_ERR_UNSUPPORTED, "num_rays %d exceeds the LDS fan table (7680 beams)", num_rays);
    if (!(fov == fov)) return fail(RL_ERR_INVALID, "fov is NaN");
    return RL_OK;
}


// ------------------------------------------------------------------------------
// launch contexts (see LaunchCtx)
// ------------------------------------------------------------------------------
static int acquire_ctx(rl_method *h, hipStream_t stream, LaunchCtx **out)
{
    LaunchCtx *pick = nullptr;
    for (LaunchCtx &c : h->ctx)
        if (c.bound && c.stream == stream) { pick = &c; break; }
    if (!pick)
        for (LaunchCtx &c : h->ctx)
            if (!c.bound) { pick = &c; break; }
    if (!pick) {
        for (LaunchCtx &c : h->ctx)
            if (!pick || c.last_use < pick->last_use) pick = &c;
        // hand-over: whatever the old stream still has in flight on this scratch must finish first
        HIPCHK(hipDeviceSynchronize());
        // (the theta-major CDDT scratch R[bin][pose] is the one large buffer of a context — up to 2 GiB —: a
        //  context that changes hands gives it back instead of pinning it for the handle's lifetime)
        pick->cddt_r.release();
    }
    pick->bound = true;
    pick->stream = stream;
    pick->last_use = ++h->use_clock;
    *out = pick;
    return RL_OK;
}

// ------------------------------------------------------------------------------
// derived tables (built lazily on the launch stream, rebuilt when the map changed).  A build_* function sizes and
// enqueues one table from the inputs it names; ensure_table runs the cache protocol around it (TableCache)
// ------------------------------------------------------------------------------
template <class Build>
static int ensure_table(TableCache &cache, bool fresh, const rl_map *m, hipStream_t stream, const Build &build)
{
    if (fresh) return cache.wait(stream);
    int rc = cache.begin_rebuild();              // launches of other streams may still read the old copy
    if (rc || (rc = build())) return rc;
    return cache.built(m, stream);
}

// (cos, sin) of the beam angles of fan f: one small table per (fov, num_rays) the handle is called
// with — four are kept, the least recently used one is rebuilt (after a device synchronisation:
// launches of other streams may still read it) when a fifth fan shows up
static int ensure_fan_table(FanTabs &t, const FanParams &f, float fov, hipStream_t stream, const float2 **out)
{
    uint32_t bits;
    memcpy(&bits, &fov, sizeof bits);
    FanTabs::Tab *slot = nullptr;
    for (auto &ft : t.tabs)
        if (ft.tab.p && ft.fov_bits == bits && ft.num_rays == f.num_rays) slot = &ft;
    if (slot) {
        slot->last_use = ++t.clock;
        *out = (const float2 *)slot->tab.p;
        return slot->dep.wait(stream);
    }
    for (auto &ft : t.tabs)
        if (!ft.tab.p) { slot = &ft; break; }
    if (!slot) {
        slot = &t.tabs[0];
        for (auto &ft : t.tabs)
            if (ft.last_use < slot->last_use) slot = &ft;
        HIPCHK(hipDeviceSynchronize());
    }
    int rc = slot->tab.ensure((size_t)f.num_rays * sizeof(float2));
    if (rc) return rc;
    if ((rc = launch("fan_table_kernel", fan_table_kernel, dim3((f.num_rays + 255) / 256), dim3(256), 0, stream, f,
                     (float2 *)slot->tab.p)))
        return rc;
    slot->fov_bits = bits;
    slot->num_rays = f.num_rays;
    slot->last_use = ++t.clock;
    *out = (const float2 *)slot->tab.p;
    return slot->dep.built(stream);
}

static int build_lut(LutTable &t, const rl_map *m, float max_range, float step_coeff, int theta_disc, int debug,
                     hipStream_t stream)
{
    const size_t n = (size_t)m->rows * m->cols * theta_disc;
    int rc = t.buf.ensure(n * sizeof(uint16_t) + 64);      // + slack: rows are read in 16-B pieces
    if (rc) return rc;
    LutParams &lp = t.lp;
    lp.lut = (uint16_t *)t.buf.p;
    lp.theta_disc = theta_disc;
    lp.bins_per_rad = (float)theta_disc * 0.15915494309189535f;
    lp.bin_width = 6.283185307179586f / (float)theta_disc;
    lp.quant = 65535.0f / max_range;
    lp.dequant = max_range / 65535.0f;
    lp.debug = debug;
    const long cells = (long)m->rows * m->cols;
    const int grid = (int)std::min(cells, (long)m->n_cu * 16);
    return launch("lut_build_kernel", lut_build_kernel, dim3(grid), dim3(256), 0, stream, m->mp, lp, max_range, step_coeff, 0,
                  m->rows);
}

static int ensure_lut(rl_method *h, hipStream_t stream)
{
    return ensure_table(h->lut.cache, h->lut.cache.fresh_for(h->map), h->map, stream, [&]() {
        return build_lut(h->lut, h->map, h->max_range, h->step_coeff, h->theta_disc, h->opt.lut_debug, stream);
    });
}

// CDDT table of the current map, ENQUEUED on `stream` with no host synchronisation and no read-back:
// the two-player front-end rebuilds it before every scan (scripts/two_player/rcs_two_player.py:110-121).
// Sizes the host needs are known without asking the device: bucket counts follow from the map shape,
// and the number of stored values is bounded by 3 per (edge cell, theta bin) — a cell's footprint
// (half-width <= sqrt(2)/2) covers at most 3 buckets — with the edge count kept by the map.
static int build_cddt(CddtTable &t, const rl_map *m, int theta_disc, int debug, hipStream_t stream)
{
    const int td = theta_disc, nb = (td + 1) / 2;
    int rc;
    if (t.geom_rows != m->rows || t.geom_cols != m->cols) {
        // per-bin geometry: depends on the map SHAPE only, uploaded once
        t.h_cos.resize(nb); t.h_sin.resize(nb); t.h_trans.resize(nb);
        t.h_width.resize(nb); t.h_boff.resize(nb + 1);
        uint32_t nbk = 0;
        const float W = (float)m->cols, H = (float)m->rows;
        for (int a = 0; a < nb; ++a) {
            float s, c;
            host_sincosf((float)a * (6.283185307179586f / (float)td), s, c);
            t.h_cos[a] = c;
            t.h_sin[a] = s;
            // buckets = height of the rotated map's bounding box; translation lifts the lowest
            // rotated corner to bucket 0
            t.h_width[a] = (int)ceilf((fabsf(W * s) + fabsf(H * c)) - CDDT_EPS) + 1;
            const float lt = H * c, rt = fmaf(W, s, H * c), rb = W * s;
            t.h_trans[a] = fmaxf(0.0f, -fminf(lt, fminf(rt, rb)) - CDDT_EPS);
            t.h_boff[a] = nbk;
            nbk += (uint32_t)t.h_width[a];
        }
        t.h_boff[nb] = nbk;
        t.buckets = nbk;
        if ((rc = t.cos.ensure(nb * 4)) || (rc = t.sin.ensure(nb * 4)) || (rc = t.trans.ensure(nb * 4)) ||
            (rc = t.width.ensure(nb * 4)) || (rc = t.boff.ensure((nb + 1) * 4)) ||
            (rc = t.offsets.ensure(((size_t)nbk + 1) * 4)) || (rc = t.cursor.ensure(((size_t)nbk + 1) * 4)))
            return rc;
        HIPCHK(hipMemcpyAsync(t.cos.p, t.h_cos.data(), nb * 4, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(t.sin.p, t.h_sin.data(), nb * 4, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(t.trans.p, t.h_trans.data(), nb * 4, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(t.width.p, t.h_width.data(), nb * 4, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(t.boff.p, t.h_boff.data(), (nb + 1) * 4, hipMemcpyHostToDevice, stream));
        t.geom_rows = m->rows;
        t.geom_cols = m->cols;
        t.counts_clean = false;
    }
    const uint32_t nbk = t.buckets;
    const size_t cap = std::max<size_t>((size_t)m->n_edges * nb * 3, 1);    // stored values, upper bound
    if (cap > (size_t)INT_MAX) return fail(RL_ERR_UNSUPPORTED, "CDDT table too large (%zu values)", cap);
    if ((rc = t.xs2.ensure(cap * 4))) return rc;
    // the blocked table the queries read (cddt_kernels.h, CddtParams): leaves of 32 values + separator lines;
    // upper bound: every bucket pads its last leaf and, with more than one leaf, its last separator line
    const size_t tab_lines = cap / 32 + cap / 1024 + 2 * (size_t)nbk + 2;
    if (tab_lines > (size_t)UINT32_MAX) return fail(RL_ERR_UNSUPPORTED, "CDDT table too large (%zu lines)", tab_lines);
    if ((rc = t.hdr.ensure((size_t)nbk * 8)) || (rc = t.tab.ensure(tab_lines * 128))) return rc;
    CddtParams &cp = t.cdp;
    cp.theta_disc = td;
    cp.n_bins = nb;
    cp.cosv = (const float *)t.cos.p;
    cp.sinv = (const float *)t.sin.p;
    cp.trans = (const float *)t.trans.p;
    cp.width = (const int *)t.width.p;
    cp.bucket_off = (const uint32_t *)t.boff.p;
    cp.offsets = (uint32_t *)t.offsets.p;
    cp.xs = (float *)t.xs2.p;
    cp.hdr = (uint2 *)t.hdr.p;
    cp.tab = (float *)t.tab.p;
    cp.bins_per_rad = (float)td * 0.15915494309189535f;
    cp.debug = debug;
    if ((rc = t.tmp.ensure(((size_t)nbk + 2 * nb + 64) * 4))) return rc;   // big-bucket count, bin totals (values, lines), list
    if (!t.sort_attr) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&cddt_sort_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)(CDDT_LDS_SORT * sizeof(float))));
        t.sort_attr = true;
    }
    // bucket counters: zeroed once; every complete build returns them to zero (FILL subtracts what
    // COUNT added), so a rebuild starts without a memset
    if (!t.counts_clean) {
        HIPCHK(hipMemsetAsync(t.cursor.p, 0, ((size_t)nbk + 1) * 4, stream));
        t.counts_clean = true;
    }
    // one workgroup per (chunk of edge cells, theta bin), bucket histogram of the bin in LDS
    int wmax = 0;
    for (int a = 0; a < nb; ++a) wmax = std::max(wmax, t.h_width[a]);
    const size_t lds_fill = (size_t)wmax * 2 * sizeof(uint32_t);
    if (lds_fill > 150 * 1024) return fail(RL_ERR_UNSUPPORTED, "CDDT: map too large for the LDS bucket histogram");
    if (lds_fill > 48 * 1024) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&cddt_project_kernel<true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_fill));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&cddt_project_kernel<false>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_fill));
    }
    const dim3 pgrid((unsigned)std::max<uint32_t>(1u, (m->n_edges + CDDT_CHUNK - 1) / CDDT_CHUNK), (unsigned)nb);
    // count -> exclusive scan (CSR offsets) -> fill -> sort every bucket
    if ((rc = launch("cddt_project_kernel", cddt_project_kernel<false>, pgrid, dim3(256), lds_fill / 2, stream, cp, m->d_edges,
                     m->d_n_edges, (uint32_t *)t.cursor.p)))
        return rc;
    // [0] big-bucket count (zeroed by the sort's last reader), [1..64) spare, [64..64+nb) bin totals, then the list
    uint32_t *big_count = (uint32_t *)t.tmp.p, *bin_total = (uint32_t *)t.tmp.p + 64;
    uint32_t *bin_lines = bin_total + nb, *big_list = bin_lines + nb;
    HIPCHK(hipMemsetAsync(big_count, 0, 4, stream));
    // two launches of the sort kernel: the large buckets (workgroup each, 64 KB of LDS) and the small ones
    // (wave each, no LDS — in one launch the LDS size of the large path would cap everybody's occupancy)
    const uint32_t n_big_wg = (uint32_t)m->n_cu;
    const int sgrid = (int)std::max(1L, std::min(((long)nbk + 3) / 4, (long)m->n_cu * 32));
    if ((rc = launch("cddt_scan_bins_kernel", cddt_scan_bins_kernel, dim3(nb), dim3(256), 0, stream, cp,
                     (const uint32_t *)t.cursor.p, bin_total, bin_lines)) ||
        (rc = launch("cddt_scan_add_kernel", cddt_scan_add_kernel, dim3(nb), dim3(256), 0, stream, cp,
                     (const uint32_t *)t.cursor.p, bin_total, bin_lines, big_list, big_count)) ||
        (rc = launch("cddt_project_kernel", cddt_project_kernel<true>, pgrid, dim3(256), lds_fill, stream, cp, m->d_edges,
                     m->d_n_edges, (uint32_t *)t.cursor.p)) ||
        (rc = launch("cddt_sort_kernel", cddt_sort_kernel, dim3(n_big_wg), dim3(256), (size_t)t.lds_sort * sizeof(float), stream,
                     (const uint32_t *)t.offsets.p, nbk, (const float *)t.xs2.p, (const uint2 *)t.hdr.p, (float *)t.tab.p,
                     big_list, big_count, n_big_wg, (uint32_t)t.lds_sort)))
        return rc;
    return launch("cddt_sort_kernel", cddt_sort_kernel, dim3(sgrid), dim3(256), 0, stream, (const uint32_t *)t.offsets.p, nbk,
                  (const float *)t.xs2.p, (const uint2 *)t.hdr.p, (float *)t.tab.p, big_list, big_count, 0u,
                  (uint32_t)t.lds_sort);
}

static int ensure_cddt(rl_method *h, hipStream_t stream)
{
    return ensure_table(h->cddt.cache, h->cddt.cache.fresh_for(h->map), h->map, stream,
                        [&]() { return build_cddt(h->cddt, h->map, h->theta_disc, h->opt.lut_debug, stream); });
}

// diagnostics (bench.py's algorithmic bytes of a CDDT ray): stored values, buckets and non-empty buckets of the
// current table, from the CSR offsets the build leaves behind (builds the table if needed; synchronises)
static int cddt_table_stats(rl_method *h, const char *name, int64_t *value_out)
{
    if (h->kind != RL_CDDT) return fail(RL_ERR_INVALID, "not a CDDT method");
    std::lock_guard<std::mutex> lk(h->mu);
    std::shared_lock<std::shared_mutex> ml(h->map->tables_mu);
    int rc = set_device(h->map);
    if (rc) return rc;
    if ((rc = ensure_cddt(h, h->stream))) return rc;
    HIPCHK(hipDeviceSynchronize());
    const CddtTable &t = h->cddt;
    std::vector<uint32_t> off((size_t)t.buckets + 1);
    HIPCHK(hipMemcpy(off.data(), t.offsets.p, off.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    int64_t nonempty = 0;
    for (size_t b = 0; b < (size_t)t.buckets; ++b) nonempty += off[b + 1] > off[b];
    if (!strcmp(name, "cddt_values")) *value_out = (int64_t)off[t.buckets];
    else if (!strcmp(name, "cddt_buckets")) *value_out = (int64_t)t.buckets;
    else *value_out = nonempty;
    return RL_OK;
}

// K2b's padded bit maps (normal + transposed), rebuilt when the map changed
static int build_blpad(BlPadMaps &t, const rl_map *m, float max_range, hipStream_t stream)
{
    const int reach = (int)max_range + 3 + 2;           // cells a walk can get away from its origin (cap + margin)
    const int near = reach;                             // origins up to here outside the map are still covered
    const int pad = near + reach + 2;
    const int pad32 = (pad + 31) / 32;                  // major-axis padding in words
    const int stride_n = (m->cols + 31) / 32 + 2 * pad32, prow_n = m->rows + 2 * pad;
    const int stride_t = (m->rows + 31) / 32 + 2 * pad32, prow_t = m->cols + 2 * pad;
    const size_t words_n = (size_t)stride_n * prow_n, words_t = (size_t)stride_t * prow_t;
    if ((words_n + words_t) * 4 > (size_t)1 << 31) return fail(RL_ERR_UNSUPPORTED, "map too large for the padded bit maps");
    int rc = t.buf.ensure((words_n + words_t) * 4);
    if (rc) return rc;
    uint32_t *out_n = (uint32_t *)t.buf.p, *out_t = out_n + words_n;
    if ((rc = launch("bl_pad_bits_kernel", bl_pad_bits_kernel, dim3((stride_n + 255) / 256, prow_n), dim3(256), 0, stream, m->d_occ,
                     m->rows, m->cols, 0, pad, pad32, stride_n, prow_n, out_n)) ||
        (rc = launch("bl_pad_bits_kernel", bl_pad_bits_kernel, dim3((stride_t + 255) / 256, prow_t), dim3(256), 0, stream, m->d_occ,
                     m->rows, m->cols, 1, pad, pad32, stride_t, prow_t, out_t)))
        return rc;
    BlPad &bp = t.blp;
    bp.bits = out_n;
    bp.stride_n = stride_n;
    bp.stride_t = stride_t;
    bp.k_n = (uint32_t)(((size_t)pad * stride_n + pad32) * 4);
    bp.k_t = (uint32_t)((words_n + (size_t)pad * stride_t + pad32) * 4);
    bp.near = (float)near;
    return RL_OK;
}

static int ensure_blpad(rl_method *h, hipStream_t stream)
{
    return ensure_table(h->blpad.cache, h->blpad.cache.fresh_for(h->map), h->map, stream,
                        [&]() { return build_blpad(h->blpad, h->map, h->max_range, stream); });
}

static BlParams make_bl(const rl_method *h, int num_rays, size_t &lds_bytes)
{
    BlParams bp{};
    // window radius: a walk takes at most (int)max_range + 3 unit steps, but its float coordinate can gain
    // one more cell on the way — x0 + 1 + 1 + ... rounds UP when it crosses a power of two with a
    // fraction just below 1 (127.99999 + 1 -> 129.0) — found by the 30-minute fuzz of round 2 as a stale
    // LDS read one row outside a window sized with no margin; two cells of margin now
    bp.R = (int)std::ceil(h->max_range) + 5;
    bp.ww = ((2 * bp.R + 32 + 31) / 32) | 1;
    const size_t win = (size_t)(2 * bp.R + 1) * bp.ww * sizeof(uint32_t);
    const size_t fan = (size_t)num_rays * sizeof(float2);
    bp.use_lds = (win + fan) <= 150 * 1024;
    lds_bytes = fan + (bp.use_lds ? win : 0);
    return bp;
}

// pose records in map-tile order (rec_sorted / order) by the binning pass the launch plan names
// (rl_binning, plan::binning_for); walk_outside = Bresenham semantics (origins outside the map still walk)
static int bin_poses(rl_method *h, LaunchCtx &cx, const float *d_poses, int n_poses, int walk_outside,
                     hipStream_t stream, int binning)
{
    const bool keys_only = binning == RL_BIN_SMALL_KEYS;
    const rl_map *m = h->map;
    int rc;
    // ray marching: the sample every ray of a pose takes at t = 0, read once per pose with the record
    // (pose_first_step); the Bresenham walk (walk_outside) has no use for it
    float *d0 = nullptr;
    if (!walk_outside && !keys_only) {
        if ((rc = cx.d0.ensure((size_t)n_poses * sizeof(float)))) return rc;
        d0 = (float *)cx.d0.p;
    }
    const float coeff = h->step_coeff;
    if ((rc = cx.rec.ensure((size_t)n_poses * sizeof(PoseRec)))) return rc;
    if ((rc = cx.order.ensure((size_t)n_poses * sizeof(uint32_t)))) return rc;
    if ((rc = cx.keys.ensure((size_t)n_poses * sizeof(uint32_t)))) return rc;
    if ((rc = cx.rec_sorted.ensure((size_t)n_poses * sizeof(PoseRec)))) return rc;
    const int do_sort = (binning == RL_BIN_GRID_UNSORTED || (binning == RL_BIN_GENERIC && !(h->opt.sort_poses && n_poses >= 64))) ? 0 : 1;
    int shift = 6;
    while ((long)((m->cols >> shift) + 1) * ((m->rows >> shift) + 1) > 8192) ++shift;
    // (tile_key: tile rows in stripes walked column by column; -1: as many tile rows as an XCD band of evenly spread poses holds)
    auto striped = [&](int tx, int sh) {
        const int tiles_y = (m->rows >> sh) + 1;
        int rps = h->tile_stripe < 0 ? std::max(1, (m->rows >> sh) / std::max(1, h->opt.xcd_bands)) : h->tile_stripe;
        if (rps >= tiles_y || !do_sort) rps = 0;
        return tx | (rps << 16);
    };
    const int tiles_x = striped((m->cols >> shift) + 1, shift);
    const int n_tiles = ((m->cols >> shift) + 1) * ((m->rows >> shift) + 1);
    if (binning == RL_BIN_GRID_SORT || binning == RL_BIN_GRID_UNSORTED) {
        const int ppw = h->bin_ppw;
        const int n_wg = (n_poses + ppw - 1) / ppw;
        if (do_sort) {
            // grid-wide binning on coarse tiles (<= 1024): per-workgroup LDS histograms ->
            // one scan over (tile, workgroup) -> scatter from LDS cursors
            int cshift = shift;
            while ((long)((m->cols >> cshift) + 1) * ((m->rows >> cshift) + 1) > 1024) ++cshift;
            const int ctx = striped((m->cols >> cshift) + 1, cshift);
            const int cnt = ((m->cols >> cshift) + 1) * ((m->rows >> cshift) + 1);
            const size_t n_ctr = (size_t)cnt * n_wg;
            if ((rc = cx.hist.ensure((n_ctr + cnt) * sizeof(uint32_t)))) return rc;     // counters, then tile totals
            uint32_t *tile_total = (uint32_t *)cx.hist.p + n_ctr;
            if ((rc = launch("pose_prep_kernel", pose_prep_kernel, dim3(n_wg), dim3(256), (size_t)cnt * 4, stream, m->mp, d_poses,
                             n_poses, (PoseRec *)cx.rec.p, (uint32_t *)cx.keys.p, (uint32_t *)cx.hist.p, n_wg, cshift, ctx, cnt,
                             nullptr, walk_outside, ppw, nullptr, coeff)) ||
                (rc = launch("tile_scan_a_kernel", tile_scan_a_kernel, dim3(cnt), dim3(256), 0, stream, (uint32_t *)cx.hist.p,
                             n_wg, tile_total)))
                return rc;
            return launch("pose_scatter_kernel", pose_scatter_kernel, dim3(n_wg), dim3(256), (size_t)cnt * 4, stream, n_poses,
                          (const PoseRec *)cx.rec.p, (const uint32_t *)cx.keys.p, (const uint32_t *)cx.hist.p, tile_total, n_wg,
                          cnt, (PoseRec *)cx.rec_sorted.p, (uint32_t *)cx.order.p, ppw, m->mp, d0, coeff);
        }
        // caller's order kept: one fully parallel pass, records land in place
        return launch("pose_prep_kernel", pose_prep_kernel, dim3(n_wg), dim3(256), 0, stream, m->mp, d_poses, n_poses,
                      (PoseRec *)cx.rec_sorted.p, nullptr, nullptr, n_wg, shift, tiles_x, n_tiles, (uint32_t *)cx.order.p,
                      walk_outside, ppw, d0, coeff);
    }
    const size_t lds = (size_t)(n_tiles + 1024) * sizeof(uint32_t);
    if (binning == RL_BIN_SMALL_KEYS)
        return launch("pose_bin_small_kernel", pose_bin_small_kernel<true>, dim3(1), dim3(1024), lds, stream, m->mp, d_poses,
                      n_poses, (PoseRec *)cx.rec_sorted.p, (uint32_t *)cx.order.p, shift, tiles_x, n_tiles, walk_outside,
                      nullptr, coeff);
    if (binning == RL_BIN_SMALL_RECORDS)
        return launch("pose_bin_small_kernel", pose_bin_small_kernel<false>, dim3(1), dim3(1024), lds, stream, m->mp, d_poses,
                      n_poses, (PoseRec *)cx.rec_sorted.p, (uint32_t *)cx.order.p, shift, tiles_x, n_tiles, walk_outside, d0,
                      coeff);
    return launch("pose_bin_kernel", pose_bin_kernel, dim3(1), dim3(1024), lds, stream, m->mp, d_poses, n_poses,
                  (PoseRec *)cx.rec.p, (PoseRec *)cx.rec_sorted.p, (uint32_t *)cx.order.p, (uint32_t *)cx.keys.p, shift,
                  tiles_x, n_tiles, do_sort, walk_outside, d0, coeff);
}

static FastDiv make_fastdiv(uint32_t d)
{
    FastDiv f{};
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;
    f.mul = (uint32_t)((((1ull << l) - d) << 32) / d + 1);
    f.sh1 = l < 1 ? l : 1;
    f.sh2 = l > 0 ? l - 1 : 0;
    f.d = d;
    return f;
}

// the options of a handle that shape a launch, as the planner takes them
static rl_plan_opts opts_of(const rl_method *h)
{
    rl_plan_opts o = h->opt;
    o.code_entries = h->step.code_entries_for(h->map, h->max_range, h->opt);
    return o;
}

static int plan_for(const rl_method *h, int n_poses, int num_rays, bool aux, bool crash, rl_launch_plan *out)
{
    plan::In in;
    in.kind = h->kind;
    in.n_cu = h->map->n_cu;
    in.rows = h->map->rows;
    in.cols = h->map->cols;
    in.theta_disc = h->theta_disc;
    in.max_range = h->max_range;
    in.o = opts_of(h);
    in.n_poses = n_poses;
    in.num_rays = num_rays;
    in.aux = aux;
    in.crash = crash;
    return plan::plan_fan(in, out);
}

// the layout of the step map under the `tiled` option (the planner marches on the row-major copy when the tiled geometry
// does not fit the address arithmetic: plan::tiled_fit — elongated maps whose pitch would need K > 24, tables beyond 4 GiB)
static int step_map_layout(const rl_map *m, float max_range, int opt_tiled)
{
    return (opt_tiled && plan::tiled_fit(m->rows, m->cols, max_range).ok) ? 1 : 0;
}

bool StepMap::fresh_for(const rl_map *m, float max_range, const rl_plan_opts &o) const
{
    // (a copy in the layout the option names is the layout wanted — tiled, so it fits — without a look at the geometry;
    //  only a row-major copy under tiled = 1 asks: the fallback of a map that does not fit)
    return cache.fresh_for(m) && code_built == o.code_map &&
           (tiled == (o.tiled != 0) || tiled == step_map_layout(m, max_range, o.tiled));
}

int StepMap::code_entries_for(const rl_map *m, float max_range, const rl_plan_opts &o) const
{
    return (o.code_map && fresh_for(m, max_range, o)) ? code_n : 0;
}

PadMap StepMap::pad_map(bool code, float res) const
{
    const Addr &a = code ? code_at : at;
    PadMap pm{};
    pm.pdt = (const float *)((const char *)(code ? cmap : pdt).p + a.base_off);
    pm.stride = a.stride;
    pm.nstride = (int)a.mask;
    pm.k4 = a.k4;
    pm.pad = pad;                                            // (the border and the divisor are the float32 map's in both)
    pm.div_stride = make_fastdiv((uint32_t)at.stride);
    pm.res = res;
    return pm;
}

// step map of a ray-marching method (the EDT padded, holding the march's step) in the layout the `tiled` option asks
// for, and the code map next to it when `code_map` asks for one
static int build_step_map(StepMap &t, const rl_map *m, float max_range, float step_coeff, int opt_tiled, int code_map,
                          hipStream_t stream)
{
    int rc;
    const int want_tiled = step_map_layout(m, max_range, opt_tiled);
    t.pad = (int)std::ceil(max_range) + 2;
    if (want_tiled) {
        const plan::TiledFit fit = plan::tiled_fit(m->rows, m->cols, max_range);
        const TiledGeom tg{fit.K, fit.pad, fit.padr, fit.pcols, fit.prows};
        const uint32_t M = 4u + (1u << (tg.K - 2));
        t.pad = fit.pad;
        t.at = {(size_t)t.pad << 4, (int)M, (uint32_t)tg.padr * M, 0xCu | (~0u << tg.K)};
        if ((rc = t.pdt.ensure(fit.bytes))) return rc;
        if ((rc = launch("pad_dt_tiled_kernel", pad_dt_tiled_kernel, dim3((tg.pcols + 255) / 256, tg.prows), dim3(256), 0, stream,
                         m->d_dt, m->rows, m->cols, (float *)t.pdt.p, tg, step_coeff)))
            return rc;
    } else {
        const int stride = (m->cols + 2 * t.pad + 31) & ~31, prow = m->rows + 2 * t.pad;
        // (row-major address: v_mad_i32_i24 r * stride + c, then << 2 in 32 bits)
        if (stride >= (1 << 23) || (size_t)prow * stride >= ((size_t)1 << 30))
            return fail(RL_ERR_UNSUPPORTED, "map %dx%d with max_range %g is too large for the step map", m->rows, m->cols,
                        max_range);
        t.at = {0, stride, (uint32_t)(((size_t)t.pad * stride + t.pad) * 4), 0u};
        if ((rc = t.pdt.ensure((size_t)prow * stride * sizeof(float)))) return rc;
        if ((rc = launch("pad_dt_kernel", pad_dt_kernel, dim3((stride + 255) / 256, prow), dim3(256), 0, stream, m->d_dt, m->rows,
                         m->cols, (float *)t.pdt.p, t.pad, stride, step_coeff)))
            return rc;
    }
    // the CODE map next to it: palette of the map's distinct steps (mark -> scan), then the tiled map of their codes.
    // The palette size decides the launches' LDS, so the host reads it back here (a map build, not a scan).
    t.code_n = 0;
    const plan::CodeFit cf = plan::code_fit(m->rows, m->cols, max_range, 1);
    if (code_map == 2 && want_tiled && cf.ok) {
        const uint32_t cap = (uint32_t)plan::CODE_MAX_ENTRIES;
        if ((rc = t.cval.ensure((size_t)cf.nb * sizeof(float)))) return rc;
        if ((rc = t.cidx.ensure((size_t)cf.nb * sizeof(uint32_t)))) return rc;
        if ((rc = t.ctab.ensure((size_t)cap * sizeof(float)))) return rc;
        if ((rc = t.cnum.ensure(2 * sizeof(uint32_t)))) return rc;
        if (!t.pin_cnum) HIPCHK(t.pin_cnum.alloc(2 * sizeof(uint32_t)));
        HIPCHK(hipMemsetAsync(t.cval.p, 0, (size_t)cf.nb * sizeof(float), stream));
        const size_t n_cells = (size_t)m->rows * m->cols;
        if ((rc = launch("code_mark_kernel", code_mark_kernel,
                         dim3((unsigned)std::min<size_t>((n_cells + 255) / 256, (size_t)m->n_cu * 8)), dim3(256), 0, stream, m->d_dt,
                         n_cells, (float *)t.cval.p, cf.nb, step_coeff, max_range)) ||
            (rc = launch("code_scan_kernel", code_scan_kernel, dim3(1), dim3(1024), 0, stream, (const float *)t.cval.p, cf.nb,
                         step_coeff, (uint32_t *)t.cidx.p, (float *)t.ctab.p, cap, (uint32_t *)t.cnum.p)))
            return rc;
        HIPCHK(hipMemcpyAsync(t.pin_cnum, t.cnum.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (t.pin_cnum[1] == 0u && t.pin_cnum[0] <= cap) {
            const TiledGeom tg{cf.K, cf.pad, cf.padr, cf.pcols, cf.prows};
            if ((rc = t.cmap.ensure(cf.bytes))) return rc;
            if ((rc = launch("pad_code_tiled_kernel", pad_code_tiled_kernel<1>, dim3((tg.pcols + 255) / 256, tg.prows), dim3(256), 0,
                             stream, m->d_dt, m->rows, m->cols, t.cmap.p, tg, step_coeff, max_range, (const uint32_t *)t.cidx.p,
                             cf.nb, (const uint32_t *)t.cnum.p)))
                return rc;
            const uint32_t M = (1u << cf.es) + (1u << (cf.K - 3));
            t.code_at = {(size_t)cf.pad << (3 + cf.es), (int)M, (uint32_t)cf.padr * M, (7u << cf.es) | (~0u << cf.K)};
            t.code_n = (int)t.pin_cnum[0];
        }
    }
    t.code_built = code_map;
    t.tiled = want_tiled;
    return RL_OK;
}

// ... rebuilt when the map, the layout option or the code-map option changed
static int ensure_step_map(rl_method *h, hipStream_t stream)
{
    return ensure_table(h->step.cache, h->step.fresh_for(h->map, h->max_range, h->opt), h->map, stream, [&]() {
        return build_step_map(h->step, h->map, h->max_range, h->step_coeff, h->opt.tiled, h->opt.code_map, stream);
    });
}

// rm_fan_stream_kernel by plan::stream_index: every instance of plan::stream_instance, nullptr in the other slots
typedef void (*rm_stream_fn)(PadMap, FanParams, StreamParams, float *, int32_t *, uint16_t *, CrashParams);
template <int I>
static constexpr rm_stream_fn rm_stream_at()
{
    constexpr plan::StreamKey k = plan::stream_key_at(I);
    if constexpr (plan::stream_instance(k)) return rm_fan_stream_kernel<k.a, k.c, k.n, k.inl, k.t, k.s, k.lit, k.code>;
    else return nullptr;
}
template <int... I>
static constexpr std::array<rm_stream_fn, sizeof...(I)> rm_stream_make(std::integer_sequence<int, I...>)
{
    return {{rm_stream_at<I>()...}};
}
static const std::array<rm_stream_fn, plan::STREAM_KEYS> rm_stream_table =
    rm_stream_make(std::make_integer_sequence<int, plan::STREAM_KEYS>());

static int dispatch_rm_stream(const rl_launch_plan &pl, hipStream_t stream, const PadMap &pm, const FanParams &f,
                              const StreamParams &sp, float *d_out, int32_t *d_hits, uint16_t *d_steps,
                              const CrashParams &cp)
{
    const int i = plan::stream_index(plan::stream_key(pl));
    const rm_stream_fn kernel = i >= 0 ? rm_stream_table[i] : nullptr;
    if (!kernel) return fail(RL_ERR_INVALID, "internal: plan names an uninstantiated kernel (%s)", pl.name);
    // (more dynamic LDS than HIP's default cap — fans of several thousand beams, with the crash table —: opt in,
    //  as the BL / occ / CDDT kernels do; the attribute is sticky per function and device, the call is cheap)
    if (pl.lds_bytes > 48 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  pl.lds_bytes);
    return launch("rm_fan_stream_kernel", kernel, dim3(pl.grid), dim3(pl.block), (size_t)pl.lds_bytes, stream, pm, f, sp, d_out,
                  d_hits, d_steps, cp);
}

// enqueue the fan kernels on `stream`; all pointers are device pointers.  What is launched is decided by
// plan::plan_fan (launch_plan.h); this function only executes the plan.
// audit mode (variant 3): the per-map constants of range_libc's RangeMethod, double arithmetic with the host's libm
// (as the CPU checker's upstream-literal statement computes them)
LiteralParams make_literal(const rl_map *m)
{
    LiteralParams lt;
    const double wa = (double)m->mp.wa;
    lt.rotation_const = (float)(-1.0 * wa - 3.0 * M_PI / 2.0);
    lt.wsin = (float)sin(wa);
    lt.wcos = (float)cos(wa);
    return lt;
}


// what a method family's launch function needs: the call, the plan, the launch context
struct FanLaunch : FanCall {
    rl_method *h;
    const rl_map *m;
    const rl_launch_plan &pl;
    LaunchCtx *cx;
    FanParams f;
    bool aux;
    dim3 grid, block;            // (the plan's)
    size_t lds;
};

// RL_K_LUT_LDS (lut_fan_lds_kernel<NL, CH>), RL_K_LUT_FAN (lut_fan_kernel<CH>): NL 1..3, CH 12 | 17
typedef void (*lut_fn)(MapParams, FanParams, LutParams, const float *, float *);
static const lut_fn lut_lds_table[3][2] = {{lut_fan_lds_kernel<1, 12>, lut_fan_lds_kernel<1, 17>},
                                           {lut_fan_lds_kernel<2, 12>, lut_fan_lds_kernel<2, 17>},
                                           {lut_fan_lds_kernel<3, 12>, lut_fan_lds_kernel<3, 17>}};
static const lut_fn lut_fan_table[2] = {lut_fan_kernel<12>, lut_fan_kernel<17>};
// ... and their origin-corrected twins (handle option lut_refine): the plan stays the default's, the launch takes the twin
static const lut_fn lut_lds_refine_table[3][2] = {{lut_fan_lds_refine_kernel<1, 12>, lut_fan_lds_refine_kernel<1, 17>},
                                                  {lut_fan_lds_refine_kernel<2, 12>, lut_fan_lds_refine_kernel<2, 17>},
                                                  {lut_fan_lds_refine_kernel<3, 12>, lut_fan_lds_refine_kernel<3, 17>}};
static const lut_fn lut_fan_refine_table[2] = {lut_fan_refine_kernel<12>, lut_fan_refine_kernel<17>};

static int launch_lut(const FanLaunch &L)
{
    const rl_launch_plan &pl = L.pl;
    const int ch = pl.ch == 12 ? 0 : (pl.ch == 17 ? 1 : -1);
    lut_fn kernel = nullptr;
    const bool refine = L.h->lut_refine != 0;
    if (ch >= 0 && pl.kernel == RL_K_LUT_FAN) kernel = (refine ? lut_fan_refine_table : lut_fan_table)[ch];
    if (ch >= 0 && pl.kernel == RL_K_LUT_LDS && pl.nl >= 1 && pl.nl <= 3)
        kernel = (refine ? lut_lds_refine_table : lut_lds_table)[pl.nl - 1][ch];
    if (!kernel) return fail(RL_ERR_INVALID, "internal: plan names an uninstantiated kernel (%s)", pl.name);
    int rc;
    if ((rc = ensure_lut(L.h, L.stream))) return rc;
    if (L.timing == 2) HIPCHK(hipEventRecord(L.h->ev0, L.stream));
    if (refine && pl.kernel == RL_K_LUT_LDS) {
        // the planned waves in workgroups of LUT_REFINE_WG lanes, each with the beam table in front of its waves' rows
        const unsigned per = LUT_REFINE_WG / L.block.x;
        const size_t lds = L.lds * per + (size_t)lut_dir_dwords(L.f.num_rays) * sizeof(uint32_t);
        return launch("lut_fan_lds_refine_kernel", kernel, dim3((L.grid.x + per - 1) / per), dim3(LUT_REFINE_WG), lds, L.stream,
                      L.m->mp, L.f, L.h->lut.lp, L.d_poses, L.d_out);
    }
    return launch(pl.kernel == RL_K_LUT_LDS ? "lut_fan_lds_kernel" : refine ? "lut_fan_refine_kernel" : "lut_fan_kernel", kernel,
                  L.grid, L.block, L.lds, L.stream, L.m->mp, L.f, L.h->lut.lp, L.d_poses, L.d_out);
}

// RL_K_CDDT_BINS
static int launch_cddt_bins(const FanLaunch &L)
{
    rl_method *h = L.h;
    int rc;
    if ((rc = ensure_cddt(h, L.stream))) return rc;
    // tile-ordered poses in XCD bands: neighbouring origins hit neighbouring buckets (L2 reuse)
    const uint32_t *d_order = nullptr;
    if (L.pl.binning != RL_BIN_NONE) {
        if ((rc = bin_poses(h, *L.cx, L.d_poses, L.n_poses, 0, L.stream, L.pl.binning))) return rc;
        d_order = (const uint32_t *)L.cx->order.p;
    }
    if (L.timing == 2) HIPCHK(hipEventRecord(h->ev0, L.stream));
    return launch("cddt_fan_bins_kernel", cddt_fan_bins_kernel, L.grid, L.block, L.lds, L.stream, L.m->mp, L.f, h->cddt.cdp,
                  L.d_poses, L.d_out, d_order, L.pl.bands, L.pl.nl, L.pl.ch);
}

// RL_K_CDDT_THETA
static int launch_cddt_theta(const FanLaunch &L)
{
    rl_method *h = L.h;
    const int form = plan::cddt_theta_form(L.pl);
    if (form < 0) return fail(RL_ERR_INVALID, "internal: plan names an uninstantiated kernel (%s)", L.pl.name);
    const bool fused = form == plan::CDDT_THETA_FUSED;
    int rc;
    if ((rc = ensure_cddt(h, L.stream))) return rc;
    // scratch of the launch context: R[raw bin][pose] behind the per-pose records {gx, gy, first bin, bins}
    const size_t prep_bytes = (((size_t)L.n_poses * 16) + 255) & ~(size_t)255;
    if ((rc = L.cx->cddt_r.ensure(prep_bytes + (fused ? 0 : (size_t)h->cddt.cdp.theta_disc * (size_t)L.n_poses * sizeof(float)))))
        return rc;
    float4 *d_prep = (float4 *)L.cx->cddt_r.p;
    float *d_r = (float *)((char *)L.cx->cddt_r.p + prep_bytes);
    if (L.timing == 2) HIPCHK(hipEventRecord(h->ev0, L.stream));
    if ((rc = launch("cddt_theta_prep_kernel", cddt_theta_prep_kernel,
                     dim3((unsigned)std::max(1, std::min((L.n_poses + 255) / 256, L.m->n_cu * 8))), dim3(256), 0, L.stream, L.m->mp,
                     L.f, h->cddt.cdp, L.d_poses, d_prep)))
        return rc;
    if (fused)
        return launch("cddt_theta_fused_kernel", cddt_theta_fused_kernel, L.grid, L.block, L.lds, L.stream, L.m->mp, L.f,
                      h->cddt.cdp, L.d_poses, d_prep, L.d_out, L.pl.nl);
    const bool search2 = form == plan::CDDT_THETA_SEARCH2;
    if ((rc = launch(search2 ? "cddt_theta_search2_kernel" : "cddt_theta_search_kernel",
                     search2 ? cddt_theta_search2_kernel : cddt_theta_search_kernel, L.grid, L.block, 0, L.stream, L.m->mp, L.f,
                     h->cddt.cdp, L.d_poses, d_prep, d_r, L.pl.bands)))
        return rc;
    const int n_grp = (L.n_poses + (1 << L.pl.ch) - 1) >> L.pl.ch;
    return launch("cddt_theta_fan_kernel", cddt_theta_fan_kernel, dim3((unsigned)std::max(1, std::min(n_grp, L.m->n_cu * 8))),
                  L.block, L.lds, L.stream, L.m->mp, L.f, h->cddt.cdp, L.d_poses, d_r, L.d_out, L.pl.ch, L.pl.nl);
}

// RL_K_CDDT_RAYS
static int launch_cddt_rays(const FanLaunch &L)
{
    int rc;
    if ((rc = ensure_cddt(L.h, L.stream))) return rc;
    if (L.timing == 2) HIPCHK(hipEventRecord(L.h->ev0, L.stream));
    return launch("cddt_fan_kernel", cddt_fan_kernel, L.grid, L.block, 0, L.stream, L.m->mp, L.f, L.h->cddt.cdp, L.d_poses,
                  L.d_out);
}

// the race scan of a CDDT handle (option race_cddt; launch_race in abi_car.hip checked the shape): one workgroup per race
int launch_race_cddt(rl_method *h, const LaunchArgs &a, const FanParams &f, const RaceParams &rp, const float *d_poses,
                     float *d_out, hipStream_t stream)
{
    int rc;
    if ((rc = ensure_cddt(h, stream))) return rc;
    if (a.timing) HIPCHK(hipEventRecord(h->ev0, stream));
    const size_t lds = (size_t)rp.group * h->cddt.cdp.theta_disc * sizeof(float);
    if ((rc = launch("race_cddt_kernel", race_cddt_kernel, dim3(rp.n_groups), dim3(RACE_WG), lds, stream, h->map->mp, f,
                     h->cddt.cdp, rp, d_poses, d_out)))
        return rc;
    if (a.timing) {
        HIPCHK(hipEventRecord(h->ev1, stream));
        h->timed = true;
    }
    return RL_OK;
}

// RL_K_BL_STREAM
static int launch_bl_stream(const FanLaunch &L)
{
    rl_method *h = L.h;
    int rc;
    // K2b: stream schedule on the cache-resident bit map
    if ((rc = ensure_blpad(h, L.stream))) return rc;
    if ((rc = bin_poses(h, *L.cx, L.d_poses, L.n_poses, 1, L.stream, L.pl.binning))) return rc;
    StreamParams sp{};
    sp.rec = (const PoseRec *)L.cx->rec_sorted.p;
    sp.order = (const uint32_t *)L.cx->order.p;
    sp.div_B = make_fastdiv((uint32_t)L.num_rays);
    sp.low_water = h->opt.low_water >= 0 ? h->opt.low_water : 12;
    sp.n_bands = L.pl.bands;
    sp.div_bands = make_fastdiv((uint32_t)L.pl.bands);
    sp.plain_store = L.plain_store;
    if (L.timing == 2) HIPCHK(hipEventRecord(h->ev0, L.stream));
    return launch("bl_fan_stream_kernel", L.aux ? bl_fan_stream_kernel<true, 1024> : bl_fan_stream_kernel<false, 1024>, L.grid,
                  L.block, L.lds, L.stream, L.m->mp, L.f, sp, h->blpad.blp, L.d_out, L.d_hits, L.d_steps);
}

// RL_K_BL_LDS, RL_K_OCC_LDS
static int launch_bl_lds(const FanLaunch &L)
{
    size_t lds_bl = 0;
    BlParams bp = make_bl(L.h, L.num_rays, lds_bl);
    const bool bl = L.pl.kernel == RL_K_BL_LDS;
    if (lds_bl > 48 * 1024) {          // more dynamic LDS than the default cap: opt in
        const void *fa = bl ? reinterpret_cast<const void *>(&bl_fan_kernel<true>)
                            : reinterpret_cast<const void *>(&occ_fan_lds_kernel<true>);
        const void *fb = bl ? reinterpret_cast<const void *>(&bl_fan_kernel<false>)
                            : reinterpret_cast<const void *>(&occ_fan_lds_kernel<false>);
        HIPCHK(hipFuncSetAttribute(fa, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bl));
        HIPCHK(hipFuncSetAttribute(fb, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bl));
    }
    if (L.timing == 2) HIPCHK(hipEventRecord(L.h->ev0, L.stream));
    // (occ_fan_lds: unit-step march on an LDS-resident occupancy window — A/B partner, approximate)
    return launch(bl ? "bl_fan_kernel" : "occ_fan_lds_kernel",
                  bl ? (L.aux ? bl_fan_kernel<true> : bl_fan_kernel<false>)
                     : (L.aux ? occ_fan_lds_kernel<true> : occ_fan_lds_kernel<false>),
                  L.grid, L.block, lds_bl, L.stream, L.m->mp, L.f, bp, L.d_poses, L.d_out, L.d_hits, L.d_steps);
}

// RL_K_RM_LITERAL
static int launch_rm_literal(const FanLaunch &L)
{
    const LiteralParams lt = make_literal(L.m);
    const long n_rays = (long)L.n_poses * L.num_rays;
    if (L.timing == 2) HIPCHK(hipEventRecord(L.h->ev0, L.stream));
    return launch("rm_literal_kernel", L.aux ? rm_literal_kernel<true, false> : rm_literal_kernel<false, false>, L.grid, L.block,
                  0, L.stream, L.m->mp, L.f, lt, L.d_poses, n_rays, L.d_out, L.d_hits, L.d_steps);
}

// RL_K_RM_CHUNK
static int launch_rm_chunk(const FanLaunch &L)
{
    CrashParams cp{nullptr, 0.0, nullptr, 1};
    if (L.crash) cp = *L.crash;
    if (L.timing == 2) HIPCHK(hipEventRecord(L.h->ev0, L.stream));
    return launch("rm_fan_kernel",
                  L.crash ? (L.aux ? rm_fan_kernel<true, true> : rm_fan_kernel<false, true>)
                          : (L.aux ? rm_fan_kernel<true, false> : rm_fan_kernel<false, false>),
                  L.grid, L.block, L.lds, L.stream, L.m->mp, L.f, L.d_poses, L.d_out, L.d_hits, L.d_steps, cp);
}

// RL_K_RM_STREAM_LIT, RL_K_RM_STREAM
static int launch_rm_stream_family(const FanLaunch &L)
{
    rl_method *h = L.h;
    const rl_launch_plan &pl = L.pl;
    int rc;
    // (1) per-pose records + tile-ordered permutation, (2) banded lane-refill march
    CrashParams cp{nullptr, 0.0, nullptr, 1};
    if (L.crash) cp = *L.crash;
    if ((rc = L.cx->rec.ensure((size_t)L.n_poses * sizeof(PoseRec)))) return rc;
    if ((rc = L.cx->order.ensure((size_t)L.n_poses * sizeof(uint32_t)))) return rc;
    if ((rc = L.cx->keys.ensure((size_t)L.n_poses * sizeof(uint32_t)))) return rc;
    if ((rc = ensure_step_map(h, L.stream))) return rc;
    if (pl.binning != RL_BIN_NONE &&
        (rc = bin_poses(h, *L.cx, L.d_poses, L.n_poses, 0, L.stream, pl.binning)))
        return rc;
    const StepMap &sm = h->step;
    if (pl.code && (sm.code_n <= 0 || pl.code_entries != sm.code_n))
        return fail(RL_ERR_INVALID, "internal: code-map plan (%d entries) without a matching palette (%d)", pl.code_entries, sm.code_n);
    const PadMap pm = sm.pad_map(pl.code != 0, L.m->res);
    StreamParams sp{};
    sp.code_tab = (const float *)sm.ctab.p;
    sp.code_n = pl.code ? sm.code_n : 0;
    sp.tail_g1 = pl.gen1 > 0 ? pl.gen1 / std::max(pl.bands, 1) : 0;
    sp.tail_pct = std::min(h->opt.tail_pct, h->opt.tail_wg_pct);
    sp.rec = (const PoseRec *)L.cx->rec_sorted.p;
    sp.order = (const uint32_t *)L.cx->order.p;
    sp.d0 = (const float *)L.cx->d0.p;
    if ((rc = ensure_fan_table(h->fans, L.f, L.fov, L.stream, &sp.fan_tab))) return rc;
    sp.div_B = make_fastdiv((uint32_t)L.num_rays);
    sp.low_water = h->opt.low_water >= 0 ? h->opt.low_water : ((pl.record_source != 0 && pl.slots >= 2) ? 20 : 12);
    sp.n_bands = pl.bands;
    sp.div_bands = make_fastdiv((uint32_t)pl.bands);
    sp.raw_poses = L.d_poses;
    sp.map = L.m->mp;
    sp.k_max = pl.k_max;
    sp.cpp = (uint32_t)((L.num_rays + 63) / 64);
    sp.div_cpp = make_fastdiv(sp.cpp);
    sp.drain_prio = h->drain_prio;
    sp.spec_drain = h->spec_drain;
    sp.spec_stretch = h->spec_stretch;
    sp.drain_cap = h->drain_cap;
    sp.drain_stretch = h->drain_stretch;
    sp.group_drain = h->group_drain;
    if (pl.kernel == RL_K_RM_STREAM_LIT) sp.lit = make_literal(L.m);
    sp.plain_store = L.plain_store;
    sp.dbg = nullptr;
    const int waves_per_wg = pl.block / 64;
    if (h->opt.debug_stamps) {
        if ((rc = L.cx->dbg.ensure((size_t)pl.grid * waves_per_wg * 4 * sizeof(uint64_t)))) return rc;
        sp.dbg = (unsigned long long *)L.cx->dbg.p;
        h->last_dbg = L.cx->dbg.p;
    }
    sp.stripe = pl.record_source == 2 ? 1 : pl.record_source == 3 ? 2 : 0;
    sp.run_log2 = pl.run_log2;
    h->last_grid = pl.grid * waves_per_wg / WAVES_PER_WG;
    // hand-off march (several rays per lane on the tiled step map): dry waves leave their last rays in the launch
    // context's leftover list — one region of handoff_cap records per wave of the main grid —, the second launch
    // finishes them
    const bool handoff = h->handoff && pl.slots >= 2 && pl.tiled && h->spec_drain > 0 && !h->opt.debug_stamps &&
                         pl.kernel == RL_K_RM_STREAM && !pl.code;   // (the leftover kernel marches the canonical arithmetic on the float32 map)
    int cap_log2 = 4;
    const int n_src = pl.grid * waves_per_wg;
    if (handoff) {
        cap_log2 = h->handoff_cap >= 64 ? 6 : (h->handoff_cap >= 32 ? 5 : (h->handoff_cap >= 16 ? 4 : 3));
        if ((rc = L.cx->left_rec.ensure(((size_t)n_src << cap_log2) * sizeof(LeftoverRec)))) return rc;
        if ((rc = L.cx->left_cnt.ensure((size_t)n_src * sizeof(uint32_t)))) return rc;
        sp.left_rec = (LeftoverRec *)L.cx->left_rec.p;
        sp.left_cnt = (uint32_t *)L.cx->left_cnt.p;
        sp.left_cap_log2 = cap_log2;
        sp.drain_cap = std::min(sp.drain_cap, 1 << cap_log2);
    }
    if (L.timing == 2) HIPCHK(hipEventRecord(h->ev0, L.stream));   // march kernel(s) alone
    if ((rc = dispatch_rm_stream(pl, L.stream, pm, L.f, sp, L.d_out, L.d_hits, L.d_steps, cp))) return rc;
    if (handoff) {
        const int lw = h->handoff_wg / 64;                              // leftover waves per workgroup
        const int n_lw = (n_src + (64 >> cap_log2) - 1) / (64 >> cap_log2);
        const dim3 lgrid((unsigned)((n_lw + lw - 1) / lw)), lblock((unsigned)h->handoff_wg);
        return launch("rm_leftover_kernel", L.crash ? rm_leftover_kernel<true> : rm_leftover_kernel<false>, lgrid, lblock, 0,
                      L.stream, pm, L.f, sp.left_rec, sp.left_cnt, n_src, cap_log2, h->drain_stretch, sp.plain_store, L.d_out, cp);
    }
    return RL_OK;
}

FanCall FanCall::slice(int p0, int np, CrashParams *marks) const
{
    const size_t r0 = (size_t)p0 * num_rays;
    FanCall s = *this;
    s.ray_offset += r0;                              // noise stays keyed by the global ray id
    s.d_poses += (size_t)p0 * 3;
    s.n_poses = np;
    if (d_out) s.d_out += r0;
    if (d_hits) s.d_hits += 2 * r0;
    if (d_steps) s.d_steps += r0;
    if (crash) {
        *marks = *crash;
        marks->first_crashed += p0;
        s.crash = marks;
    }
    return s;
}

// a batch cut into pose slices below 2^slice_log2 rays (plan: slices > 1), each its own launch sequence on the stream
static int launch_fan_sliced(rl_method *h, const rl_launch_plan &pl, const FanCall &c)
{
    // (a fused crash test reaches a sliced launch only in per-pose-mark form — the upstream-literal mode's slices)
    if (c.crash && c.crash->group != 0)
        return fail(RL_ERR_UNSUPPORTED, "a fused crash test over %d poses in the upstream-literal mode needs the per-pose "
                                        "mark form (rl_check_collision_groups*), not one roll-out of that length", c.n_poses);
    // one event pair around the whole sliced sequence (the per-slice pairs would leave the last slice only)
    if (c.timing) HIPCHK(hipEventRecord(h->ev0, c.stream));
    int rc = RL_OK;
    for (int p0 = 0; p0 < c.n_poses && rc == RL_OK; p0 += pl.slice_poses) {
        CrashParams marks;
        FanCall s = c.slice(p0, std::min(pl.slice_poses, c.n_poses - p0), &marks);
        s.timing = 0;
        rc = launch_fan(h, s);
    }
    if (c.timing && rc == RL_OK) { HIPCHK(hipEventRecord(h->ev1, c.stream)); h->timed = true; }
    return rc;
}

int launch_fan(rl_method *h, const FanCall &c)
{
    if (c.n_poses == 0) return RL_OK;
    const rl_map *m = h->map;
    const int num_rays = c.num_rays;
    const hipStream_t stream = c.stream;
    const CrashParams *const crash = c.crash;
    const bool aux = c.d_hits || c.d_steps;
    if (h->kind != RL_RM && h->kind != RL_RM_GPU) {
        if (crash) return fail(RL_ERR_UNSUPPORTED, "fused crash test needs a ray-marching method");
        if (aux && h->kind != RL_BRESENHAM)
            return fail(RL_ERR_UNSUPPORTED, "hit cells / step counts exist only for RM and Bresenham");
    }
    rl_launch_plan pl;
    int rc = RL_OK;
    // (a code-map handle plans with its palette size: the step map and the palette are built before the plan)
    if (h->opt.code_map && (h->kind == RL_RM || h->kind == RL_RM_GPU) && h->opt.variant >= 1 && (rc = ensure_step_map(h, stream))) return rc;
    rc = plan_for(h, c.n_poses, num_rays, aux, crash != nullptr, &pl);
    if (rc == RL_ERR_UNSUPPORTED)
        return fail(rc, (h->opt.variant >= 2 && crash) ? "the fused crash test needs variant 0 or 1 (not the occupancy-window or the audit kernel)"
                        : h->opt.variant == 2 ? "occupancy window of max_range %g does not fit LDS (num_rays %d)"
                                          : "the beam tables of max_range %g, num_rays %d exceed a workgroup's LDS (160 KB)",
                    h->max_range, num_rays);
    if (rc) return fail(rc, "launch planning failed");
    if (pl.slices > 1) return launch_fan_sliced(h, pl, c);
    LaunchCtx *cx = nullptr;
    if ((rc = acquire_ctx(h, stream, &cx))) return rc;
    h->last_plan = pl;
    if (c.timing == 1) HIPCHK(hipEventRecord(h->ev0, stream));
    const FanLaunch L{c, h, m, pl, cx, make_fan(h, c.n_poses, c.fov, num_rays, c.ray_offset), aux,
                      dim3(pl.grid), dim3(pl.block), (size_t)pl.lds_bytes};
    switch (pl.kernel) {
    case RL_K_LUT_LDS:
    case RL_K_LUT_FAN:
        rc = launch_lut(L);
        break;
    case RL_K_CDDT_BINS:
        rc = launch_cddt_bins(L);
        break;
    case RL_K_CDDT_THETA:
        rc = launch_cddt_theta(L);
        break;
    case RL_K_CDDT_RAYS:
        rc = launch_cddt_rays(L);
        break;
    case RL_K_BL_STREAM:
        rc = launch_bl_stream(L);
        break;
    case RL_K_BL_LDS:
    case RL_K_OCC_LDS:
        rc = launch_bl_lds(L);
        break;
    case RL_K_RM_LITERAL:
        rc = launch_rm_literal(L);
        break;
    case RL_K_RM_CHUNK:
        rc = launch_rm_chunk(L);
        break;
    case RL_K_RM_STREAM_LIT:
    case RL_K_RM_STREAM:
        rc = launch_rm_stream_family(L);
        break;
    default:
        return fail(RL_ERR_INVALID, "launch plan names no kernel");
    }
    if (rc) return rc;
    if (c.timing) { HIPCHK(hipEventRecord(h->ev1, stream)); h->timed = true; }
    return RL_OK;
}

static int launch_rays(rl_method *h, const float *d_ins, long n, float *d_out, int32_t *d_hits,
                       uint16_t *d_steps, hipStream_t stream)
{
    if (n == 0) return RL_OK;
    const rl_map *m = h->map;
    const LaunchArgs a = LaunchArgs::of(h);
    FanParams f = make_fan(h, 0, 0.0f, 1, a.ray_offset);
    long want = (n + WG - 1) / WG;
    long cap = (long)m->n_cu * h->opt.grid_mult;
    int grid = (int)std::max(1L, std::min(want, cap));
    if (a.timing) HIPCHK(hipEventRecord(h->ev0, stream));
    int rc;
    if (h->kind == RL_GIANT_LUT) {
        if ((rc = ensure_lut(h, stream))) return rc;
        rc = launch(h->lut_refine ? "lut_rays_refine_kernel" : "lut_rays_kernel",
                    h->lut_refine ? lut_rays_refine_kernel : lut_rays_kernel, dim3(grid), dim3(256), 0, stream, m->mp, f, h->lut.lp,
                    d_ins, n, d_out);
    } else if (h->kind == RL_CDDT) {
        if ((rc = ensure_cddt(h, stream))) return rc;
        rc = launch("cddt_rays_kernel", cddt_rays_kernel, dim3(grid), dim3(256), 0, stream, m->mp, f, h->cddt.cdp, d_ins, n, d_out);
    } else if (h->kind == RL_BRESENHAM) {
        rc = launch("bl_rays_kernel", bl_rays_kernel, dim3(grid), dim3(256), 0, stream, m->mp, f, d_ins, n, d_out);
    } else if (h->opt.variant == 3) {
        // audit mode: the upstream 2-argument form stated literally, one lane per row
        rc = launch("rm_literal_kernel", (d_hits || d_steps) ? rm_literal_kernel<true, true> : rm_literal_kernel<false, true>,
                    dim3(grid), dim3(256), 0, stream, m->mp, f, make_literal(m), d_ins, n, d_out, d_hits, d_steps);
    } else if (h->opt.variant >= 1 && n <= INT_MAX) {
        // a ray is a pose with one beam at alpha = 0: fan(num_rays = 1, fov = 0) gives exactly
        // (cos, sin) of the heading as direction, and the stream kernel packs 64 rays per block
        return launch_fan(h, FanCall{a, d_ins, (int)n, 0.0f, 1, d_out, d_hits, d_steps, nullptr, stream});
    } else {
        rc = launch("rm_rays_kernel", rm_rays_kernel, dim3(grid), dim3(WG), 0, stream, m->mp, f, d_ins, n, d_out, d_hits, d_steps);
    }
    if (rc) return rc;
    if (a.timing) { HIPCHK(hipEventRecord(h->ev1, stream)); h->timed = true; }
    return RL_OK;
}

// ------------------------------------------------------------------------------
// launch planning through the C ABI (pure host arithmetic: works without a device)
// ------------------------------------------------------------------------------
extern "C" int rl_plan_default_opts(rl_plan_opts *out)
{
    if (!out) return fail(RL_ERR_INVALID, "rl_plan_default_opts: null pointer");
    plan::default_opts(*out);
    return RL_OK;
}

extern "C" int rl_plan_fan(int kind, int n_cu, int rows, int cols, float max_range_px, int theta_disc,
                           const rl_plan_opts *opts_or_null, int n_poses, int num_rays, int want_aux,
                           int want_crash, rl_launch_plan *out)
{
    if (!out) return fail(RL_ERR_INVALID, "rl_plan_fan: null pointer");
    if (kind < RL_BRESENHAM || kind > RL_GIANT_LUT) return fail(RL_ERR_INVALID, "unknown range method kind %d", kind);
    if (n_cu <= 0 || rows <= 0 || cols <= 0 || n_poses < 0 || num_rays <= 0 || !(max_range_px > 0.0f))
        return fail(RL_ERR_INVALID, "rl_plan_fan: bad shape arguments");
    plan::In in;
    in.kind = kind;
    in.n_cu = n_cu;
    in.rows = rows;
    in.cols = cols;
    in.max_range = max_range_px;
    in.theta_disc = theta_disc;
    if (opts_or_null) in.o = *opts_or_null; else plan::default_opts(in.o);
    in.n_poses = n_poses;
    in.num_rays = num_rays;
    in.aux = want_aux != 0;
    in.crash = want_crash != 0;
    if (in.crash && kind != RL_RM && kind != RL_RM_GPU)
        return fail(RL_ERR_UNSUPPORTED, "fused crash test needs a ray-marching method");
    const int rc = plan::plan_fan(in, out);
    if (rc) return fail(rc, "no kernel of this variant serves the request");
    return RL_OK;
}

extern "C" int rl_method_plan_fan(rl_method *h, int n_poses, int num_rays, int want_aux, int want_crash,
                                  rl_launch_plan *out)
{
    if (!h || !out) return fail(RL_ERR_INVALID, "rl_method_plan_fan: null pointer");
    if (n_poses < 0 || num_rays <= 0) return fail(RL_ERR_INVALID, "rl_method_plan_fan: bad shape arguments");
    if (!h->reps.empty()) {                     // what ONE device launches for its block of the batch
        long lo, hi;
        block_of(n_poses, 0, multi_parts(h, n_poses), lo, hi);
        return rl_method_plan_fan(h->reps[0], (int)(hi - lo), num_rays, want_aux, want_crash, out);
    }
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = RL_OK;
    if (h->opt.code_map && (h->kind == RL_RM || h->kind == RL_RM_GPU) && h->opt.variant >= 1) {
        if ((rc = set_device(h->map))) return rc;
        std::shared_lock<std::shared_mutex> tl(h->map->tables_mu);
        if ((rc = ensure_step_map(h, h->stream))) return rc;
    }
    rc = plan_for(h, n_poses, num_rays, want_aux != 0, want_crash != 0, out);
    if (rc) return fail(rc, "no kernel of this variant serves the request");
    return RL_OK;
}

extern "C" int rl_method_last_plan(rl_method *h, rl_launch_plan *out)
{
    if (!h || !out) return fail(RL_ERR_INVALID, "rl_method_last_plan: null pointer");
    if (!h->reps.empty()) return rl_method_last_plan(h->reps[0], out);
    std::lock_guard<std::mutex> lk(h->mu);
    *out = h->last_plan;
    return RL_OK;
}

extern "C" int rl_launch_contexts(void) { return N_LAUNCH_CTX; }

extern "C" int rl_calc_range_fan_device(rl_method *h, const float *d_poses, int n_poses, float fov,
                                        int num_rays, float *d_outs, int32_t *d_hits,
                                        uint16_t *d_steps, void *hip_stream)
{
    int rc = check_fan_args(h, n_poses, fov, num_rays);
    if (rc) return rc;
    if (!h->reps.empty()) return multi_needs_replica("rl_calc_range_fan_device");
    if (n_poses > 0 && (!d_poses || !d_outs))
        return fail(RL_ERR_INVALID, "rl_calc_range_fan_device: null device pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    std::shared_lock<std::shared_mutex> ml(h->map->tables_mu);
    rc = set_device(h->map);
    if (rc) return rc;
    return launch_fan(h, FanCall{LaunchArgs::of(h), d_poses, n_poses, fov, num_rays, d_outs, d_hits, d_steps, nullptr,
                                 (hipStream_t)hip_stream});
}

extern "C" int rl_calc_range_many_device(rl_method *h, const float *d_ins, float *d_outs, int n,
                                         void *hip_stream)
{
    if (!h) return fail(RL_ERR_INVALID, "null method handle");
    if (n < 0) return fail(RL_ERR_INVALID, "n must be >= 0");
    if (!h->reps.empty()) return multi_needs_replica("rl_calc_range_many_device");
    if (n > 0 && (!d_ins || !d_outs))
        return fail(RL_ERR_INVALID, "rl_calc_range_many_device: null device pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    std::shared_lock<std::shared_mutex> ml(h->map->tables_mu);
    int rc = set_device(h->map);
    if (rc) return rc;
    return launch_rays(h, d_ins, n, d_outs, nullptr, nullptr, (hipStream_t)hip_stream);
}

// host-pointer forms ---------------------------------------------------------------
// per-pose crash marks: an int per pose that is never cleared between launches — every launch
// writes its own epoch (zeroed when the buffer grows or the epoch wraps)
static int pose_marks(rl_method *h, int n_poses, hipStream_t stream, int &mark, int **d_marks)
{
    LaunchCtx *cx = nullptr;
    int rc = acquire_ctx(h, stream, &cx);
    if (rc) return rc;
    const size_t cap_before = cx->pose_first.cap;
    rc = cx->pose_first.ensure((size_t)n_poses * sizeof(int));
    if (rc) return rc;
    if (cx->pose_first.cap != cap_before || cx->crash_epoch >= INT_MAX - 1) {
        HIPCHK(hipMemsetAsync(cx->pose_first.p, 0, cx->pose_first.cap, stream));
        cx->crash_epoch = 0;
    }
    mark = ++cx->crash_epoch;
    *d_marks = (int *)cx->pose_first.p;
    return RL_OK;
}

// pinned, device-mapped host staging of at least `bytes` (small host calls run zero-copy through it)
static int pin_ensure(rl_method *h, size_t bytes)
{
    if (bytes <= h->pin_cap) return RL_OK;
    h->pin_cap = 0;
    if (h->pin.alloc(bytes * 2) != hipSuccess) return fail(RL_ERR_NOMEM, "pinned allocation of %zu bytes failed", bytes * 2);
    h->pin_cap = bytes * 2;
    return RL_OK;
}

// car-outline table -> h->edge, re-sent only when its contents changed since the last call
int upload_edge(rl_method *h, const double *edge, int num_rays)
{
    const size_t cap_before = h->edge.buf.cap;
    int rc = h->edge.ensure(num_rays);
    if (rc) return rc;
    if (h->edge.buf.cap != cap_before || h->edge_host.size() != (size_t)num_rays ||
        memcmp(h->edge_host.data(), edge, (size_t)num_rays * sizeof(double)) != 0) {
        HIPCHK(hipMemcpyAsync(h->edge, edge, (size_t)num_rays * sizeof(double), hipMemcpyHostToDevice, h->stream));
        h->edge_host.assign(edge, edge + num_rays);
    }
    return RL_OK;
}

int fan_host(rl_method *h, const float *poses, int n_poses, float fov, int num_rays,
                    float *outs, int32_t *hits, uint16_t *steps, const double *edge,
                    double crash_thresh, int *first_crashed)
{
    const size_t n_rays = (size_t)n_poses * num_rays;
    int rc = set_device(h->map);
    if (rc) return rc;
    if (n_poses == 0) {
        if (first_crashed) *first_crashed = -1;
        return RL_OK;
    }
    HostCall hc(h->stream);
    // small calls: zero-copy through pinned host memory (scan() 45 -> ~25 us host-visible)
    // output buffer inside a pinned block of rl_host_alloc: the kernel writes the ranges straight into it
    const bool direct_out = outs && !hits && !steps && n_rays <= (size_t)h->direct_max_rays &&
                            in_host_block(outs, n_rays * sizeof(float), h->map->device);
    const bool zc = !hits && !steps && (direct_out || n_rays <= (size_t)h->pinned_max_rays);
    const size_t off_out = ((size_t)n_poses * 3 * sizeof(float) + 255) & ~(size_t)255;
    const size_t off_end = off_out + (direct_out ? 0 : ((n_rays * sizeof(float) + 255) & ~(size_t)255));
    if (zc) {
        if ((rc = pin_ensure(h, off_end))) return rc;
        memcpy(h->pin, poses, (size_t)n_poses * 3 * sizeof(float));
    } else if ((rc = hc.up(h->poses, poses, (size_t)n_poses * 3)) ||
               ((outs || !first_crashed) && (rc = hc.room(h->outs, n_rays))) || (hits && (rc = hc.room(h->hits, n_rays * 2))) ||
               (steps && (rc = hc.room(h->steps, n_rays))))
        return rc;
    char *const pin = h->pin;
    const float *d_poses = zc ? (const float *)pin : (const float *)h->poses;
    CrashParams cp{nullptr, 0.0, nullptr, 1, 0};
    const bool crash_direct = first_crashed && n_poses <= 512;
    if (first_crashed) {
        if ((rc = upload_edge(h, edge, num_rays))) return rc;
        if ((rc = hc.room(h->flag, 1))) return rc;
        if (!h->pin_flag && h->pin_flag.alloc(64) != hipSuccess) return fail(RL_ERR_NOMEM, "pinned allocation of 64 bytes failed");
        cp.edge = h->edge;
        cp.thresh = crash_thresh;
        if (crash_direct) {
            // one roll-out: atomicMin straight into the result word (few poses, little contention)
            if ((rc = launch("fill_int_kernel", fill_int_kernel, dim3(1), dim3(64), 0, h->stream, h->flag, 1, INT_MAX))) return rc;
            cp.first_crashed = h->flag;
            cp.group = n_poses;
        } else {
            // big batches: the kernel marks crashed poses (a word per pose), the first one is reduced
            // on the device afterwards (see crash_reduce_kernel)
            if ((rc = pose_marks(h, n_poses, h->stream, cp.mark, &cp.first_crashed))) return rc;
            cp.group = 0;
        }
    }
    float *d_out = (outs || !first_crashed)
                       ? (direct_out ? outs : zc ? (float *)(pin + off_out) : (float *)h->outs)
                       : nullptr;
    const FanCall call{LaunchArgs::of(h), d_poses, n_poses, fov, num_rays, d_out, hits ? (int32_t *)h->hits : nullptr,
                       steps ? (uint16_t *)h->steps : nullptr, first_crashed ? &cp : nullptr, h->stream};
    if (outs && !zc && !first_crashed && !hits && !steps && h->overlap_min_rays > 0 &&
        n_rays >= (size_t)h->overlap_min_rays && n_poses >= 4 && !call.timing &&
        (h->kind == RL_RM || h->kind == RL_RM_GPU || h->kind == RL_BRESENHAM)) {
        // big plain scans are bound by the 4 B per ray going back over PCIe: four pose slices, the copy of slice k on
        // a second stream while slice k+1 marches (the march of a 65536-pose batch is ~10 % of the call).  The table
        // methods keep one launch: their kernels take 2-4 % of the call, and the theta-major CDDT search wants the
        // whole batch (>= 32768 poses) in one launch
        constexpr int S = 4;
        HIPCHK(h->copy_stream.create());
        const int per = (n_poses + S - 1) / S;
        rc = RL_OK;
        for (int k = 0, p0 = 0; p0 < n_poses && rc == RL_OK; ++k, p0 += per) {
            const int np = std::min(per, n_poses - p0);
            const size_t r0 = (size_t)p0 * num_rays, nr = (size_t)np * num_rays;
            rc = launch_fan(h, call.slice(p0, np));
            if (rc) break;
            if (h->slice_ev[k].create(hipEventDisableTiming) != hipSuccess) {
                rc = fail(RL_ERR_HIP, "hipEventCreate failed");
                break;
            }
            if (hipEventRecord(h->slice_ev[k], h->stream) != hipSuccess ||
                hipStreamWaitEvent(h->copy_stream, h->slice_ev[k], 0) != hipSuccess ||
                hipMemcpyAsync(outs + r0, d_out + r0, nr * sizeof(float), hipMemcpyDeviceToHost, h->copy_stream) != hipSuccess)
                rc = fail(RL_ERR_HIP, "sliced device-to-host copy failed");
        }
        // (both streams are drained whatever happened; a kernel fault or a copy error that only surfaces here
        //  must not come back as RL_OK with garbage in `outs`)
        const hipError_t e_launch = hipGetLastError();
        const hipError_t e_march = hipStreamSynchronize(h->stream);
        const hipError_t e_copy = hipStreamSynchronize(h->copy_stream);
        if (rc == RL_OK && (e_launch != hipSuccess || e_march != hipSuccess || e_copy != hipSuccess))
            rc = fail(RL_ERR_HIP, "sliced host-pointer scan failed: launch %s, march stream %s, copy stream %s",
                      hipGetErrorString(e_launch), hipGetErrorString(e_march), hipGetErrorString(e_copy));
        return rc;
    }
    if ((rc = launch_fan(h, call))) return rc;
    if (!zc && ((rc = hc.down(outs, h->outs, n_rays)) || (rc = hc.down(hits, h->hits, n_rays * 2)) ||
                (rc = hc.down(steps, h->steps, n_rays))))
        return rc;
    if (first_crashed) {
        if (!crash_direct && (rc = launch("crash_reduce_kernel", crash_reduce_kernel, dim3(1), dim3(64), 0, h->stream,
                                          cp.first_crashed, cp.mark, 1, n_poses, h->flag)))
            return rc;
        HIPCHK(hipMemcpyAsync(h->pin_flag, h->flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    if ((rc = hc.finish())) return rc;
    int flag = first_crashed ? *h->pin_flag : 0;
    if (crash_direct && flag == INT_MAX) flag = -(n_poses + 1);
    if (zc && !direct_out) {
        if (outs) memcpy(outs, pin + off_out, n_rays * sizeof(float));
    }
    if (first_crashed) *first_crashed = flag;      // first crashed pose, or -(n_poses + 1)
    return RL_OK;
}


// rl_calc_range_many on one device: (x, y, theta) rows in, ranges out
int rays_host(rl_method *h, const float *ins, float *outs, int n)
{
    std::lock_guard<std::mutex> lk(h->mu);
    std::shared_lock<std::shared_mutex> ml(h->map->tables_mu);
    int rc = set_device(h->map);
    if (rc) return rc;
    HostCall hc(h->stream);
    if (n <= h->pinned_max_rays) {                       // one scan's worth of rows: zero-copy
        const size_t off_out = ((size_t)n * 3 * sizeof(float) + 255) & ~(size_t)255;
        if ((rc = pin_ensure(h, off_out + (size_t)n * sizeof(float)))) return rc;
        memcpy(h->pin, ins, (size_t)n * 3 * sizeof(float));
        char *const pin = h->pin;
        float *p_out = (float *)(pin + off_out);
        if ((rc = launch_rays(h, (const float *)pin, n, p_out, nullptr, nullptr, h->stream)) || (rc = hc.finish())) return rc;
        memcpy(outs, p_out, (size_t)n * sizeof(float));
        return RL_OK;
    }
    if ((rc = hc.up(h->poses, ins, (size_t)n * 3)) || (rc = hc.room(h->outs, n)) ||
        (rc = launch_rays(h, h->poses, n, h->outs, nullptr, nullptr, hc.st)) || (rc = hc.down(outs, h->outs, n)))
        return rc;
    return hc.finish();
}

// ------------------------------------------------------------------------------
// particle-filter weights (include/scanlib.h "particle-filter weights"; kernels: pf_kernels.h)
// ------------------------------------------------------------------------------
static int check_pf_shape(const rl_method *h, const char *fn, int n_particles, int n_angles)
{
    if (!h) return fail(RL_ERR_INVALID, "%s: null method handle", fn);
    if (!h->reps.empty()) return fail(RL_ERR_INVALID, "%s: multi-device handles are not served (call it on rl_method_replica(h, i))", fn);
    if (n_particles < 0) return fail(RL_ERR_INVALID, "%s: n_particles must be >= 0", fn);
    if (n_angles < 1 || n_angles > PF_MAX_ANGLES)
        return fail(RL_ERR_INVALID, "%s: n_angles must be in [1, %d] (got %d)", fn, PF_MAX_ANGLES, n_angles);
    if ((long)n_particles * n_angles > (long)INT_MAX)
        return fail(RL_ERR_INVALID, "%s: n_particles * n_angles must stay below 2^31", fn);
    return RL_OK;
}

// which arithmetic the handle's kind and variant cast a repeat-angle ray with (PF_* of pf_kernels.h)
static int pf_kind_of(const rl_method *h, int *kind)
{
    if (h->kind == RL_CDDT || h->kind == RL_GIANT_LUT) {
        *kind = h->kind == RL_CDDT ? PF_CDDT : (h->lut_refine ? PF_LUT_REFINE : PF_LUT);
        return RL_OK;
    }
    if (h->kind != RL_RM && h->kind != RL_RM_GPU)
        return fail(RL_ERR_UNSUPPORTED, "repeat-angle scans are not served by Bresenham's line");
    if (h->opt.variant == 2) return fail(RL_ERR_UNSUPPORTED, "repeat-angle scans need variant 0, 1 or 3 (not the occupancy window)");
    *kind = h->opt.variant == 3 ? PF_RM_LITERAL : PF_RM;
    return RL_OK;
}

static PfParams make_pf(const rl_method *h, int n_particles, int n_angles)
{
    // tiles of about PF_TILE_RAYS rays when there are enough particles for four tiles per CU, smaller ones down to one
    // pass of the workgroup otherwise (a 4000-particle update still fills the device); option pf_block forces a size
    int block = pf_block(n_particles, n_angles);
    const int spread = (int)(((long)n_particles + 4L * h->map->n_cu - 1) / (4L * h->map->n_cu));
    block = std::max(std::max(1, PF_WG / n_angles), std::min(block, spread));
    if (h->pf_block > 0) block = h->pf_block;
    block = std::max(1, std::min(std::min(block, PF_WG), std::max(n_particles, 1)));
    while (block > 1 && pf_lds_bytes(block, n_angles) > 65536) --block;
    return PfParams{n_particles, n_angles, block, h->sensor, h->sensor_w, (float)(h->sensor_w - 1)};
}

static int launch_pf_angles(rl_method *h, const LaunchArgs &a, int kind, const float *d_poses, int n_particles, const float *d_angles,
                            int n_angles, float *d_out, int32_t *d_hits, uint16_t *d_steps, hipStream_t stream)
{
    const rl_map *m = h->map;
    const bool aux = d_hits || d_steps;
    if (aux && pf_table_kind(kind))
        return fail(RL_ERR_UNSUPPORTED, "hit cells / step counts exist only for the ray-marching methods");
    int rc;
    if ((kind == PF_LUT || kind == PF_LUT_REFINE) && (rc = ensure_lut(h, stream))) return rc;
    if (kind == PF_CDDT && (rc = ensure_cddt(h, stream))) return rc;
    const FanParams f = make_fan(h, n_particles, 0.0f, n_angles, a.ray_offset);
    const LiteralParams lt = make_literal(m);
    const long n = (long)n_particles * n_angles;
    const int grid = (int)std::max(1L, std::min((n + PF_WG - 1) / PF_WG, (long)m->n_cu * 16));
    decltype(&pf_angles_kernel<PF_RM, true>) kernel;
    switch (kind) {
    case PF_RM:
        kernel = aux ? pf_angles_kernel<PF_RM, true> : pf_angles_kernel<PF_RM, false>;
        break;
    case PF_RM_LITERAL:
        kernel = aux ? pf_angles_kernel<PF_RM_LITERAL, true> : pf_angles_kernel<PF_RM_LITERAL, false>;
        break;
    case PF_CDDT:
        kernel = pf_angles_kernel<PF_CDDT, false>;
        break;
    case PF_LUT_REFINE:
        kernel = pf_angles_kernel<PF_LUT_REFINE, false>;
        break;
    default:
        kernel = pf_angles_kernel<PF_LUT, false>;
        break;
    }
    return launch("pf_angles_kernel", kernel, dim3(grid), dim3(PF_WG), 0, stream, m->mp, f, lt, h->cddt.cdp, h->lut.lp, d_poses,
                  d_angles, n, d_out, d_hits, d_steps);
}

static int launch_pf_eval(rl_method *h, const float *d_obs, const float *d_ranges, int n_angles, int n_particles,
                          double *d_weights, hipStream_t stream)
{
    const PfParams pp = make_pf(h, n_particles, n_angles);
    const int tiles = (n_particles + pp.block - 1) / pp.block;
    const int grid = std::max(1, std::min(tiles, h->map->n_cu * 8));
    return launch("pf_eval_kernel", pf_eval_kernel, dim3(grid), dim3(PF_WG), pf_lds_bytes(pp.block, n_angles), stream, h->map->mp,
                  pp, d_obs, d_ranges, d_weights);
}

// the fused call.  RM / RMGPU: pf_weight_kernel, nothing but the weights leaves the kernel.  CDDT / GiantLUT:
// pf_angles_kernel into the launch context's scratch, then pf_eval_kernel — the same contract, 4 B per ray through HBM
static int launch_pf_weights(rl_method *h, const LaunchArgs &a, int kind, const float *d_poses, int n_particles, const float *d_angles,
                             const float *d_obs, int n_angles, double *d_weights, hipStream_t stream)
{
    int rc;
    if (pf_table_kind(kind)) {
        LaunchCtx *cx = nullptr;
        if ((rc = acquire_ctx(h, stream, &cx))) return rc;
        if ((rc = cx->pf_r.ensure((size_t)n_particles * n_angles * sizeof(float)))) return rc;
        if ((rc = launch_pf_angles(h, a, kind, d_poses, n_particles, d_angles, n_angles, (float *)cx->pf_r.p, nullptr, nullptr, stream)))
            return rc;
        return launch_pf_eval(h, d_obs, (const float *)cx->pf_r.p, n_angles, n_particles, d_weights, stream);
    }
    const rl_map *m = h->map;
    const PfParams pp = make_pf(h, n_particles, n_angles);
    const FanParams f = make_fan(h, n_particles, 0.0f, n_angles, a.ray_offset);
    const LiteralParams lt = make_literal(m);
    const int tiles = (n_particles + pp.block - 1) / pp.block;
    const dim3 grid(std::max(1, std::min(tiles, m->n_cu * 8)));
    const size_t lds = pf_lds_bytes(pp.block, n_angles);
    return launch("pf_weight_kernel", kind == PF_RM_LITERAL ? pf_weight_kernel<true> : pf_weight_kernel<false>, grid, dim3(PF_WG),
                  lds, stream, m->mp, f, lt, pp, d_poses, d_angles, d_obs, d_weights);
}

extern "C" int rl_set_sensor_model(rl_method *h, const double *table, int width)
{
    if (!h || !table) return fail(RL_ERR_INVALID, "rl_set_sensor_model: null pointer");
    if (!h->reps.empty()) return fail(RL_ERR_INVALID, "rl_set_sensor_model: multi-device handles are not served (call it on rl_method_replica(h, i))");
    if (width < 2 || width > PF_MAX_WIDTH)
        return fail(RL_ERR_INVALID, "rl_set_sensor_model: width must be in [2, %d] (got %d)", PF_MAX_WIDTH, width);
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = set_device(h->map);
    if (rc) return rc;
    const size_t bytes = (size_t)width * width * sizeof(double);
    DevPtr<double> fresh;
    if ((rc = fresh.alloc(bytes))) return rc;
    if (hipMemcpy(fresh, table, bytes, hipMemcpyHostToDevice) != hipSuccess)
        return fail(RL_ERR_HIP, "rl_set_sensor_model: the copy of the table failed");
    if (h->sensor) HIPCHK(hipDeviceSynchronize());      // launches of other streams may still read the old table
    h->sensor = std::move(fresh);
    h->sensor_w = width;
    return RL_OK;
}

extern "C" int rl_calc_range_repeat_angles_device(rl_method *h, const float *d_ins_p3, int n_particles,
                                                  const float *d_angles, int n_angles, float *d_outs,
                                                  int32_t *d_hit_cells_or_null, uint16_t *d_steps_or_null,
                                                  void *hip_stream)
{
    int rc = check_pf_shape(h, "rl_calc_range_repeat_angles_device", n_particles, n_angles), kind = 0;
    if (rc) return rc;
    if (!d_ins_p3 || !d_angles || !d_outs) return fail(RL_ERR_INVALID, "rl_calc_range_repeat_angles_device: null device pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    std::shared_lock<std::shared_mutex> ml(h->map->tables_mu);
    if ((rc = pf_kind_of(h, &kind)) || n_particles == 0 || (rc = set_device(h->map))) return rc;
    return launch_pf_angles(h, LaunchArgs::of(h), kind, d_ins_p3, n_particles, d_angles, n_angles, d_outs, d_hit_cells_or_null,
                            d_steps_or_null, (hipStream_t)hip_stream);
}

extern "C" int rl_eval_sensor_model_device(rl_method *h, const float *d_obs, const float *d_ranges, int n_angles,
                                           int n_particles, double *d_weights, void *hip_stream)
{
    int rc = check_pf_shape(h, "rl_eval_sensor_model_device", n_particles, n_angles);
    if (rc) return rc;
    if (!d_obs || !d_ranges || !d_weights) return fail(RL_ERR_INVALID, "rl_eval_sensor_model_device: null device pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->sensor_w) return fail(RL_ERR_INVALID, "rl_eval_sensor_model_device: no sensor model set (rl_set_sensor_model)");
    if (n_particles == 0 || (rc = set_device(h->map))) return rc;
    return launch_pf_eval(h, d_obs, d_ranges, n_angles, n_particles, d_weights, (hipStream_t)hip_stream);
}

extern "C" int rl_calc_range_repeat_angles_eval_sensor_model_device(rl_method *h, const float *d_ins_p3, int n_particles,
                                                                    const float *d_angles, const float *d_obs,
                                                                    int n_angles, double *d_weights, void *hip_stream)
{
    int rc = check_pf_shape(h, "rl_calc_range_repeat_angles_eval_sensor_model_device", n_particles, n_angles), kind = 0;
    if (rc) return rc;
    if (!d_ins_p3 || !d_angles || !d_obs || !d_weights)
        return fail(RL_ERR_INVALID, "rl_calc_range_repeat_angles_eval_sensor_model_device: null device pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    std::shared_lock<std::shared_mutex> ml(h->map->tables_mu);
    if ((rc = pf_kind_of(h, &kind))) return rc;
    if (!h->sensor_w) return fail(RL_ERR_INVALID, "rl_calc_range_repeat_angles_eval_sensor_model_device: no sensor model set (rl_set_sensor_model)");
    if (n_particles == 0 || (rc = set_device(h->map))) return rc;
    return launch_pf_weights(h, LaunchArgs::of(h), kind, d_ins_p3, n_particles, d_angles, d_obs, n_angles, d_weights, (hipStream_t)hip_stream);
}

// host-pointer forms: staged through the handle's device buffers on its own stream, synchronous
struct PfHost {
    const float *ins, *angles, *obs, *ranges;      // host inputs (null: not part of the call)
    float *outs;                                   // host outputs
    int32_t *hits;
    uint16_t *steps;
    double *weights;
};

static int pf_host(rl_method *h, const char *fn, const PfHost &a, int n_particles, int n_angles)
{
    int rc = check_pf_shape(h, fn, n_particles, n_angles), kind = 0;
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    std::shared_lock<std::shared_mutex> ml(h->map->tables_mu);
    if (a.ins && (rc = pf_kind_of(h, &kind))) return rc;
    if (a.weights && !h->sensor_w) return fail(RL_ERR_INVALID, "%s: no sensor model set (rl_set_sensor_model)", fn);
    if (n_particles == 0 || (rc = set_device(h->map))) return rc;
    const size_t n = (size_t)n_particles * n_angles;
    HostCall hc(h->stream);
    hipStream_t s = hc.st;
    if ((a.ins && ((rc = hc.up(h->poses, a.ins, (size_t)n_particles * 3)) || (rc = hc.up(h->pf_ang, a.angles, n_angles)))) ||
        (a.obs && ((rc = hc.up(h->pf_obs, a.obs, n_angles)) || (rc = hc.room(h->pf_w, n_particles)))) ||
        (a.ranges && (rc = hc.up(h->outs, a.ranges, n))) || (a.outs && (rc = hc.room(h->outs, n))) ||
        (a.hits && (rc = hc.room(h->hits, n * 2))) || (a.steps && (rc = hc.room(h->steps, n))))
        return rc;
    if (a.outs)
        rc = launch_pf_angles(h, LaunchArgs::of(h), kind, h->poses, n_particles, h->pf_ang, n_angles, h->outs,
                              a.hits ? (int32_t *)h->hits : nullptr, a.steps ? (uint16_t *)h->steps : nullptr, s);
    else if (a.ranges)
        rc = launch_pf_eval(h, h->pf_obs, h->outs, n_angles, n_particles, h->pf_w, s);
    else
        rc = launch_pf_weights(h, LaunchArgs::of(h), kind, h->poses, n_particles, h->pf_ang, h->pf_obs, n_angles, h->pf_w, s);
    if (rc || (rc = hc.down(a.outs, h->outs, n)) || (rc = hc.down(a.hits, h->hits, n * 2)) ||
        (rc = hc.down(a.steps, h->steps, n)) || (rc = hc.down(a.weights, h->pf_w, n_particles)))
        return rc;
    return hc.finish();
}

extern "C" int rl_calc_range_repeat_angles(rl_method *h, const float *ins_p3, int n_particles, const float *angles,
                                           int n_angles, float *outs, int32_t *hit_cells_or_null, uint16_t *steps_or_null)
{
    if (!ins_p3 || !angles || !outs) return fail(RL_ERR_INVALID, "rl_calc_range_repeat_angles: null pointer");
    return pf_host(h, "rl_calc_range_repeat_angles", PfHost{ins_p3, angles, nullptr, nullptr, outs, hit_cells_or_null, steps_or_null, nullptr},
                   n_particles, n_angles);
}

extern "C" int rl_eval_sensor_model(rl_method *h, const float *obs, const float *ranges, int n_angles, int n_particles,
                                    double *weights)
{
    if (!obs || !ranges || !weights) return fail(RL_ERR_INVALID, "rl_eval_sensor_model: null pointer");
    return pf_host(h, "rl_eval_sensor_model", PfHost{nullptr, nullptr, obs, ranges, nullptr, nullptr, nullptr, weights}, n_particles, n_angles);
}

extern "C" int rl_calc_range_repeat_angles_eval_sensor_model(rl_method *h, const float *ins_p3, int n_particles,
                                                             const float *angles, const float *obs, int n_angles,
                                                             double *weights)
{
    if (!ins_p3 || !angles || !obs || !weights)
        return fail(RL_ERR_INVALID, "rl_calc_range_repeat_angles_eval_sensor_model: null pointer");
    return pf_host(h, "rl_calc_range_repeat_angles_eval_sensor_model", PfHost{ins_p3, angles, obs, nullptr, nullptr, nullptr, nullptr, weights},
                   n_particles, n_angles);
}

// ------------------------------------------------------------------------------
// particle-filter localisation (include/scanlib.h "particle-filter localisation"; kernels: mcl_kernels.h): T whole MCL
// updates per call on the handle's stream, the likelihood through launch_pf_weights
// ------------------------------------------------------------------------------
struct rl_pf {
    rl_method *h = nullptr;        // borrowed
    int device = 0;
    int P = 0, A = 0, NB = 0;
    double std[3] = {0, 0, 0}, ratio = 0;
    uint32_t key = 0;
    long t = 0;                    // steps since the reset
    bool ready = false;            // a reset has been made
    // state: X (cur), X' (prop), the float32 poses of the scan, w, L, omega, the in-chunk sums, cum, ancestors; the chunk
    // totals ([1 + MCL_SUMS][NB]: omega's, then the six of the estimate), the chunk bases, W; a call's inputs and outputs
    // (counted in scalars: 3 a pose or an odometry row, 4 an estimate)
    DevPtr<float> ang, q, obs;
    DevPtr<double> cur, prop, w, lik, omega, part, cum, tot, base, scal, odom, est, neff;
    DevPtr<int32_t> anc;
    DevPtr<int> flags;
    std::mutex mu;
};

static bool bad_std(double v) { return !(v >= 0.0); }      // negative or NaN

extern "C" int rl_pf_create(rl_method *h, const rl_pf_params *p, const float *angles, rl_pf **out)
{
    if (out) *out = nullptr;
    if (!h || !p || !angles || !out) return fail(RL_ERR_INVALID, "rl_pf_create: null pointer");
    int rc = check_pf_shape(h, "rl_pf_create", p->n_particles, p->n_angles), kind = 0;
    if (rc) return rc;
    if (p->n_particles < 1 || p->n_particles > MCL_MAX_PARTICLES)
        return fail(RL_ERR_INVALID, "rl_pf_create: n_particles must be in [1, %d] (got %d)", MCL_MAX_PARTICLES, p->n_particles);
    if (bad_std(p->motion_std[0]) || bad_std(p->motion_std[1]) || bad_std(p->motion_std[2]) || bad_std(p->resample_ratio))
        return fail(RL_ERR_INVALID, "rl_pf_create: motion_std and resample_ratio must be >= 0");
    std::lock_guard<std::mutex> lk(h->mu);
    if ((rc = pf_kind_of(h, &kind))) return rc;
    if (!h->sensor_w) return fail(RL_ERR_INVALID, "rl_pf_create: no sensor model set (rl_set_sensor_model)");
    if ((rc = set_device(h->map))) return rc;
    std::unique_ptr<rl_pf, decltype(&rl_pf_destroy)> f(new (std::nothrow) rl_pf, rl_pf_destroy);
    if (!f) return fail(RL_ERR_NOMEM, "rl_pf_create: out of memory");
    f->h = h;
    f->device = h->map->device;
    f->P = p->n_particles;
    f->A = p->n_angles;
    f->NB = (f->P + MCL_CHUNK - 1) / MCL_CHUNK;
    for (int a = 0; a < 3; ++a) f->std[a] = p->motion_std[a];
    f->ratio = p->resample_ratio;
    const size_t P = (size_t)f->P, NB = (size_t)f->NB;
    if ((rc = f->ang.ensure(f->A)) || (rc = f->cur.ensure(P * 3)) || (rc = f->prop.ensure(P * 3)) || (rc = f->q.ensure(P * 3)) ||
        (rc = f->w.ensure(P)) || (rc = f->lik.ensure(P)) || (rc = f->omega.ensure(P)) || (rc = f->part.ensure(P)) ||
        (rc = f->cum.ensure(P)) || (rc = f->anc.ensure(P)) || (rc = f->tot.ensure((1 + MCL_SUMS) * NB)) ||
        (rc = f->base.ensure(NB)) || (rc = f->scal.ensure(1)))
        return rc;
    if (hipMemcpy(f->ang, angles, (size_t)f->A * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return fail(RL_ERR_HIP, "rl_pf_create: the copy of the angles failed");
    *out = f.release();
    return RL_OK;
}

extern "C" void rl_pf_destroy(rl_pf *f)
{
    if (!f) return;
    (void)hipSetDevice(f->device);       // (every call is synchronous: nothing of the filter's is in flight, h is not touched)
    delete f;
}

extern "C" int rl_pf_reset(rl_pf *f, const double *particles_p3, const double *weights_or_null, uint64_t seed)
{
    if (!f || !particles_p3) return fail(RL_ERR_INVALID, "rl_pf_reset: null pointer");
    std::scoped_lock lk(f->mu, f->h->mu);
    int rc = set_device(f->h->map);
    if (rc) return rc;
    const size_t P = (size_t)f->P;
    std::vector<double> uniform;
    if (!weights_or_null) uniform.assign(P, 1.0 / (double)f->P);
    HostCall hc(f->h->stream);                   // (after `uniform`: it stays until the call has drained)
    if ((rc = hc.up(f->cur, particles_p3, P * 3)) || (rc = hc.up(f->w, weights_or_null ? weights_or_null : uniform.data(), P)) ||
        (rc = hc.zero(f->prop, P * 3)) || (rc = hc.zero(f->lik, P)) || (rc = hc.zero(f->omega, P)) ||
        (rc = hc.zero(f->part, P)) || (rc = hc.zero(f->cum, P)) || (rc = hc.zero(f->anc, P)) || (rc = hc.finish()))
        return rc;
    f->key = noise_key(seed);
    f->t = 0;
    f->ready = true;
    return RL_OK;
}

// one update, enqueued on `s`: step `k` of this call (its odometry and observation rows), step f->t + k since the reset
static int launch_mcl_step(rl_pf *f, const LaunchArgs &a, int kind, const MclParams &mp, int k, hipStream_t s)
{
    rl_method *h = f->h;
    const uint32_t t = (uint32_t)(f->t + k);
    const int grid = (f->P + MCL_WG - 1) / MCL_WG;
    double *tot = f->tot, *tot6 = tot + f->NB;
    int rc;
    if ((rc = launch("mcl_motion_kernel", mcl_motion_kernel, dim3(grid), dim3(MCL_WG), 0, s, mp, f->odom + 3 * (size_t)k, t, f->cur,
                     f->prop, f->q)) ||
        (rc = launch_pf_weights(h, a, kind, f->q, f->P, f->ang, f->obs + (size_t)k * f->A, f->A, f->lik, s)) ||
        (rc = launch("mcl_weight_kernel", mcl_weight_kernel, dim3((f->NB + MCL_GROUP - 1) / MCL_GROUP), dim3(MCL_WG), 0, s, mp, f->w,
                     f->lik, f->omega, tot)) ||
        (rc = launch("mcl_norm_kernel", mcl_norm_kernel, dim3((f->NB + MCL_NGROUP - 1) / MCL_NGROUP), dim3(MCL_WG), 0, s, mp, tot,
                     f->omega, f->prop, f->w, f->part, tot6, f->scal)) ||
        (rc = launch("mcl_base_kernel", mcl_base_kernel, dim3(1), dim3(64 * MCL_SUMS), 0, s, mp, tot6, f->scal, f->base,
                     f->est + 4 * (size_t)k, f->neff + k, f->flags + k)))
        return rc;
    return launch("mcl_resample_kernel", mcl_resample_kernel, dim3(grid), dim3(MCL_WG), 0, s, mp, t, f->flags + k, f->base, f->part,
                  f->prop, f->cur, f->w, f->anc, f->cum);
}

extern "C" int rl_pf_run(rl_pf *f, int n_steps, const double *odom_t3, const float *obs_tA, double *est_t4, double *neff_t,
                         int *flags_t)
{
    if (!f) return fail(RL_ERR_INVALID, "rl_pf_run: null filter handle");
    if (n_steps < 0) return fail(RL_ERR_INVALID, "rl_pf_run: n_steps must be >= 0");
    std::scoped_lock lk(f->mu, f->h->mu);
    if (!f->ready) return fail(RL_ERR_INVALID, "rl_pf_run: the filter has not been reset (rl_pf_reset)");
    if (f->t + (long)n_steps > (1L << 26)) return fail(RL_ERR_INVALID, "rl_pf_run: more than 2^26 steps since the reset");
    if (n_steps == 0) return RL_OK;
    if (!odom_t3 || !obs_tA || !est_t4 || !neff_t || !flags_t) return fail(RL_ERR_INVALID, "rl_pf_run: null pointer");
    rl_method *h = f->h;
    std::shared_lock<std::shared_mutex> ml(h->map->tables_mu);
    int rc, kind = 0;
    if ((rc = pf_kind_of(h, &kind)) || (rc = set_device(h->map))) return rc;
    const size_t T = (size_t)n_steps;
    HostCall hc(h->stream);
    hipStream_t s = hc.st;
    if ((rc = hc.up(f->odom, odom_t3, T * 3)) || (rc = hc.up(f->obs, obs_tA, T * f->A)) || (rc = hc.room(f->est, T * 4)) ||
        (rc = hc.room(f->neff, T)) || (rc = hc.room(f->flags, T)))
        return rc;
    MclParams mp{f->P, f->NB, 1.0 / (double)f->P, {f->std[0], f->std[1], f->std[2]}, f->ratio * (double)f->P, f->key};
    LaunchArgs a = LaunchArgs::of(h);            // the scans' noise: step t's rays are off + t P A + p A + j
    const uint64_t off = a.ray_offset;
    for (int k = 0; k < n_steps && !rc; ++k) {
        a.ray_offset = off + (uint64_t)(f->t + k) * (uint64_t)f->P * (uint64_t)f->A;
        rc = launch_mcl_step(f, a, kind, mp, k, s);
    }
    if (rc) {
        f->ready = false;                         // part of the steps may have run: the state is no step's; reset again
        return rc;
    }
    if ((rc = hc.down(est_t4, f->est, T * 4)) || (rc = hc.down(neff_t, f->neff, T)) || (rc = hc.down(flags_t, f->flags, T)) ||
        (rc = hc.finish()))
        return rc;
    f->t += n_steps;
    return RL_OK;
}

extern "C" int rl_pf_read(rl_pf *f, double *particles_p3, double *weights, int32_t *ancestors, double *cum, double *likelihood)
{
    if (!f) return fail(RL_ERR_INVALID, "rl_pf_read: null filter handle");
    std::scoped_lock lk(f->mu, f->h->mu);
    if (!f->ready) return fail(RL_ERR_INVALID, "rl_pf_read: the filter has not been reset (rl_pf_reset)");
    int rc = set_device(f->h->map);
    if (rc) return rc;
    HostCall hc(f->h->stream);
    const size_t P = (size_t)f->P;
    if ((rc = hc.down(particles_p3, f->cur, P * 3)) || (rc = hc.down(weights, f->w, P)) || (rc = hc.down(ancestors, f->anc, P)) ||
        (rc = hc.down(cum, f->cum, P)) || (rc = hc.down(likelihood, f->lik, P)))
        return rc;
    return hc.finish();
}

extern "C" int rl_method_read_lut(rl_method *h, int row0, int row1, uint16_t *out)
{
    if (!h || !out) return fail(RL_ERR_INVALID, "rl_method_read_lut: null pointer");
    if (h->kind != RL_GIANT_LUT) return fail(RL_ERR_INVALID, "not a GiantLUT method");
    if (!h->reps.empty()) return rl_method_read_lut(h->reps[0], row0, row1, out);
    std::lock_guard<std::mutex> lk(h->mu);
    std::shared_lock<std::shared_mutex> ml(h->map->tables_mu);
    int rc = set_device(h->map);
    if (rc) return rc;
    if (row0 < 0 || row1 > h->map->rows || row0 > row1)
        return fail(RL_ERR_INVALID, "row range [%d,%d) outside the map", row0, row1);
    if ((rc = ensure_lut(h, h->stream))) return rc;
    const size_t per_row = (size_t)h->map->cols * h->theta_disc;
    HostCall hc(h->stream);
    if ((rc = hc.down(out, (const uint16_t *)h->lut.buf.p + (size_t)row0 * per_row, (size_t)(row1 - row0) * per_row))) return rc;
    return hc.finish();
}

extern "C" int rl_debug_read_stamps(rl_method *h, uint64_t *out, int max_words)
{
    if (!h || !out) return fail(RL_ERR_INVALID, "rl_debug_read_stamps: null pointer");
    if (!h->reps.empty()) return rl_debug_read_stamps(h->reps[0], out, max_words);
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = set_device(h->map);
    if (rc) return rc;
    size_t words = (size_t)h->last_grid * WAVES_PER_WG * 4;
    if (!h->last_dbg || words == 0) return fail(RL_ERR_INVALID, "no stamps recorded (set debug_stamps=1)");
    if ((size_t)max_words < words) words = (size_t)max_words;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, h->last_dbg, words * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return (int)words;
}

// ------------------------------------------------------------------------------
// grouped crash test and the roll-out generator ("next" rows)
// ------------------------------------------------------------------------------
int check_groups_args(int n_groups, int group)
{
    if (n_groups < 0 || group <= 0) return fail(RL_ERR_INVALID, "n_groups >= 0 and group > 0 required");
    if ((long)n_groups * group > INT_MAX) return fail(RL_ERR_INVALID, "too many poses");
    return RL_OK;
}

// d_first[g] <- first crashed pose of group g, or -(group+1) when none.  Ray-marching methods fuse the
// test into the march kernel; the others scan into d_ranges (required then) and run one pass over the ranges.
int crash_groups_device(rl_method *h, const LaunchArgs &a, const float *d_poses, int n_groups, int group, float fov,
                        int num_rays, const double *d_edge, double thresh, int *d_first, float *d_ranges, hipStream_t stream)
{
    const int n_poses = n_groups * group;
    // the kernels mark crashed POSES (one word each, no contended atomics); groups are reduced after
    int rc;
    int mark;
    int *d_pose_first = nullptr;
    if ((rc = pose_marks(h, n_poses, stream, mark, &d_pose_first))) return rc;
    const CrashParams cp{d_edge, thresh, d_pose_first, 0, mark};
    const bool fused = h->kind == RL_RM || h->kind == RL_RM_GPU;
    if (!fused && !d_ranges) return fail(RL_ERR_INVALID, "this range method needs a ranges buffer for the crash test");
    if ((rc = launch_fan(h, FanCall{a, d_poses, n_poses, fov, num_rays, d_ranges, nullptr, nullptr, fused ? &cp : nullptr, stream})))
        return rc;
    const int grid = (int)std::max(1L, std::min(((long)n_poses + 3) / 4, (long)h->map->n_cu * 8));
    if (!fused && (rc = launch("crash_groups_kernel", crash_groups_kernel, dim3(grid), dim3(256), 0, stream, d_ranges, d_edge, thresh,
                               n_poses, num_rays, 0, mark, d_pose_first)))
        return rc;
    const int rgrid = (int)std::max(1L, std::min(((long)n_groups + 3) / 4, (long)h->map->n_cu * 8));
    return launch("crash_reduce_kernel", crash_reduce_kernel, dim3(rgrid), dim3(256), 0, stream, d_pose_first, mark, n_groups, group,
                  d_first);
}

extern "C" int rl_check_collision_groups_device(rl_method *h, const float *d_poses, int n_groups,
                                                int group, float fov, int num_rays,
                                                const double *d_edge, double crash_thresh,
                                                int *d_first_crashed, float *d_ranges_or_null,
                                                void *hip_stream)
{
    int rc = check_groups_args(n_groups, group);
    if (rc || (rc = check_fan_args(h, n_groups * group, fov, num_rays))) return rc;
    if (n_groups == 0) return RL_OK;
    if (!h->reps.empty()) return multi_needs_replica("rl_check_collision_groups_device");
    if (!d_poses || !d_edge || !d_first_crashed)
        return fail(RL_ERR_INVALID, "rl_check_collision_groups_device: null device pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    std::shared_lock<std::shared_mutex> ml(h->map->tables_mu);
    if ((rc = set_device(h->map))) return rc;
    return crash_groups_device(h, LaunchArgs::of(h), d_poses, n_groups, group, fov, num_rays, d_edge, crash_thresh,
                               d_first_crashed, d_ranges_or_null, (hipStream_t)hip_stream);
}


extern "C" int rl_last_kernel_ms(rl_method *h, float *ms_out)
{
    if (!h || !ms_out) return fail(RL_ERR_INVALID, "rl_last_kernel_ms: null pointer");
    if (!h->reps.empty()) return rl_last_kernel_ms(h->reps[0], ms_out);
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->timed) return fail(RL_ERR_INVALID, "no launch has been timed on this handle (set option \"timing\"=1 first)");
    int rc = set_device(h->map);
    if (rc) return rc;
    HIPCHK(hipEventSynchronize(h->ev1));
    HIPCHK(hipEventElapsedTime(ms_out, h->ev0, h->ev1));
    return RL_OK;
}

