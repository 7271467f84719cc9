// abi_multi.hip — the host-pointer entry points of libscan_amd.so (C ABI: include/scanlib.h) and their multi-device forms
// on a handle made by rl_map_create_multi: each says what a block is and how many there are; MultiCall / run_blocks
// (abi_internal.h) say under which locks, with which noise offset, and which replica's thread takes which block.
// (scripts/scan_simulator.py:113-135 scanMany, scripts/mcts.py:237 checkCollisionMany: ONE Python process hands over a batch.)
#include "abi_internal.h"

// ------------------------------------------------------------------------------
// multi-device forms of the host-pointer entry points: contiguous blocks, one per device, each
// device writing its block of the results straight into the caller's buffer (in a pinned block of
// rl_host_alloc the kernels write it directly: 4 B per ray over that device's own PCIe link).  Noise
// stays keyed by the GLOBAL ray id (the replica's ray offset is the parent's + the block's first ray),
// crash indices are global: the result is bit-identical to the single-device call.
// ------------------------------------------------------------------------------
static int multi_fan(rl_method *h, const float *poses, const float *rows3, int n_poses, float fov, int num_rays,
                     float *outs, int32_t *hits, uint16_t *steps)
{
    MultiCall mc(h);
    return mc.run(*h->pool, n_poses, multi_parts(h, n_poses), 0, num_rays, [=](const MultiBlock &b) {
        rl_method *r = h->reps[b.replica];
        const int np = (int)(b.hi - b.lo);
        const size_t r0 = (size_t)b.lo * num_rays;
        if (rows3)          // the fork's sparse 4-argument layout: pose p in row p * num_rays
            return rl_calc_range_many_fan(r, rows3 + r0 * 3, outs + r0, np * num_rays, fov, num_rays);
        return rl_calc_range_fan(r, poses + 3 * b.lo, np, fov, num_rays, outs + r0, hits ? hits + 2 * r0 : nullptr,
                                 steps ? steps + r0 : nullptr);
    });
}

// A per-ray call has no poses to hold against multi_min_poses: MULTI_RAYS_PER_POSE rays count as one (and a device is
// brought in per multi_min_poses of those).
constexpr long MULTI_RAYS_PER_POSE = 64L * 16;

static int multi_rays(rl_method *h, const float *ins, float *outs, int n)
{
    MultiCall mc(h);
    const long by_size = (long)n / (MULTI_RAYS_PER_POSE * std::max(h->multi_min_poses, 1));
    const int k = (int)std::max<long>(1, std::min<long>((long)h->reps.size(), by_size));
    return mc.run(*h->pool, n, k, 0, 1, [=](const MultiBlock &b) {
        return rl_calc_range_many(h->reps[b.replica], ins + 3 * b.lo, outs + b.lo, (int)(b.hi - b.lo));
    });
}

// groups of `group` poses (group == n_poses, n_groups == 1 with `single`: rl_check_collision_many's one index)
static int multi_crash(rl_method *h, const float *poses, int n_groups, int group, float fov, int num_rays,
                       const double *edge, double thresh, int *first_crashed, float *ranges, bool single)
{
    MultiCall mc(h);
    const long n_units = single ? group : n_groups;              // what is cut: poses of the one batch | roll-outs
    const long poses_per_unit = single ? 1 : group;
    const int k = (int)std::max<long>(1, std::min<long>(multi_parts(h, n_units * poses_per_unit), n_units));
    std::vector<int> part(k, -1);                                // single: block i's first crashed pose (global index), < 0: none
    int *const part_p = part.data();
    const int rc = mc.run(*h->pool, n_units, k, 0, (uint64_t)poses_per_unit * num_rays, [=](const MultiBlock &b) {
        rl_method *r = h->reps[b.replica];
        const int n = (int)(b.hi - b.lo);
        const size_t p0 = (size_t)b.lo * poses_per_unit, r0 = p0 * num_rays;
        float *rg = ranges ? ranges + r0 : nullptr;
        if (!single)
            return rl_check_collision_groups(r, poses + 3 * p0, n, group, fov, num_rays, edge, thresh, first_crashed + b.lo, rg);
        int &first = part_p[b.index];
        const int rc1 = rl_check_collision_many(r, poses + 3 * p0, n, fov, num_rays, edge, thresh, &first, rg);
        if (rc1 == RL_OK && first >= 0) first += (int)b.lo;
        return rc1;
    });
    if (rc || !single) return rc;
    *first_crashed = -(group + 1);                                // Car::isCrashed: -(poses + 1) when none crashed
    for (int first : part)
        if (first >= 0) {
            *first_crashed = first;
            break;
        }
    return RL_OK;
}

// ------------------------------------------------------------------------------
// DEVICE-RESIDENT exchange of the one-process multi-device handle (round 6).  The reference's caller is ONE process
// (scripts/mcts.py:237 -> scripts/racecar_simulator_v2.py:146-167): the only way it ever moves ranges over xGMI is a
// library that does so behind one call.  Every replica marches its contiguous pose block into its own HBM, chunk by
// chunk; behind every chunk its copy stream sends the chunk to the CONSUMER device with hipMemcpyPeerAsync (device to
// device over xGMI once peer access is enabled; the runtime stages through the host where it is not), so chunk k
// travels under chunk k + 1's march.  The consumer's own block is marched straight into the destination.  Worker
// threads as everywhere in this unit: nothing is forked or re-executed after GPU initialisation.  Results bit-identical
// to the single-device scan (noise keyed by the global ray id, crash indices global).
// ------------------------------------------------------------------------------
static int ensure_copy_stream(rl_method *r)
{
    HIPCHK(r->copy_stream.create());
    for (Event &e : r->slice_ev) HIPCHK(e.create(hipEventDisableTiming));
    return RL_OK;
}

// (device `from` is current) let its copies reach `to` directly; a refusal only means staged copies
static void try_peer(int from, int to)
{
    if (from == to) return;
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, from, to) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(to, 0);
    (void)hipGetLastError();                            // ("already enabled" is not an error worth keeping)
}

// (run from a MultiCall: the replica's noise stands at the block's first ray, off0; every further chunk moves it on)
static int replica_fan_to_consumer(rl_method *r, const float *poses_blk, int np, float fov, int num_rays, float nstd,
                                   uint64_t seed, uint64_t off0, bool is_consumer, int consumer_dev, float *d_dst, int chunks)
{
    int rc = set_device(r->map);
    if (rc) return rc;
    const int dev = r->map->device;
    const size_t n_rays = (size_t)np * num_rays;
    float *d_poses = nullptr, *d_local = nullptr;
    {
        std::lock_guard<std::mutex> lk(r->mu);
        if ((rc = r->poses.ensure((size_t)np * 3))) return rc;
        if (!is_consumer && (rc = r->outs.ensure(n_rays))) return rc;
        if ((rc = ensure_copy_stream(r))) return rc;
        d_poses = r->poses;
        d_local = is_consumer ? d_dst : (float *)r->outs;
    }
    if (!is_consumer) try_peer(dev, consumer_dev);
    HIPCHK(hipMemcpyAsync(d_poses, poses_blk, (size_t)np * 3 * sizeof(float), hipMemcpyHostToDevice, r->stream));
    const int k = std::max(1, std::min(chunks, np));
    for (int c = 0; c < k; ++c) {
        long lo, hi;
        block_of(np, c, k, lo, hi);
        const size_t r0 = (size_t)lo * num_rays, nr = (size_t)(hi - lo) * num_rays;
        if (c > 0 && (rc = rl_set_noise(r, nstd, seed, off0 + r0))) return rc;
        if ((rc = rl_calc_range_fan_device(r, d_poses + 3 * lo, (int)(hi - lo), fov, num_rays, d_local + r0, nullptr, nullptr,
                                           (void *)r->stream)))
            return rc;
        if (!is_consumer) {
            hipEvent_t ev = r->slice_ev[c & 3];
            HIPCHK(hipEventRecord(ev, r->stream));
            HIPCHK(hipStreamWaitEvent(r->copy_stream, ev, 0));
            HIPCHK(hipMemcpyPeerAsync(d_dst + r0, consumer_dev, d_local + r0, dev, nr * sizeof(float), r->copy_stream));
        }
    }
    HIPCHK(hipStreamSynchronize(r->stream));
    if (!is_consumer) HIPCHK(hipStreamSynchronize(r->copy_stream));
    return RL_OK;
}

static int replica_crash_to_consumer(rl_method *r, const float *poses_blk, int n_groups, int group, float fov, int num_rays,
                                     const double *edge, double thresh, bool is_consumer, int consumer_dev, int *d_dst)
{
    int rc = set_device(r->map);
    if (rc) return rc;
    const int dev = r->map->device;
    const size_t np = (size_t)n_groups * group;
    float *d_poses = nullptr;
    int *d_local = nullptr;
    const double *d_edge = nullptr;
    {
        std::lock_guard<std::mutex> lk(r->mu);
        if ((rc = r->poses.ensure(np * 3)) || (rc = upload_edge(r, edge, num_rays))) return rc;
        if (!is_consumer && (rc = r->flag.ensure(n_groups))) return rc;
        if ((rc = ensure_copy_stream(r))) return rc;
        d_poses = r->poses;
        d_edge = r->edge;
        d_local = is_consumer ? d_dst : (int *)r->flag;
    }
    if (!is_consumer) try_peer(dev, consumer_dev);
    HIPCHK(hipMemcpyAsync(d_poses, poses_blk, np * 3 * sizeof(float), hipMemcpyHostToDevice, r->stream));
    if ((rc = rl_check_collision_groups_device(r, d_poses, n_groups, group, fov, num_rays, d_edge, thresh, d_local, nullptr,
                                               (void *)r->stream)))
        return rc;
    if (!is_consumer)
        HIPCHK(hipMemcpyPeerAsync(d_dst, consumer_dev, d_local, dev, (size_t)n_groups * sizeof(int), r->stream));
    HIPCHK(hipStreamSynchronize(r->stream));
    return RL_OK;
}

static int multi_device_check(rl_method *h, int consumer, const void *dst, const char *fn)
{
    if (!h) return fail(RL_ERR_INVALID, "%s: null method handle", fn);
    if (h->reps.empty()) return fail(RL_ERR_INVALID, "%s needs a method of a multi-device map (rl_map_create_multi)", fn);
    if (consumer < 0 || consumer >= (int)h->reps.size())
        return fail(RL_ERR_INVALID, "%s: consumer %d is not a replica index of this handle (0..%zu)", fn, consumer, h->reps.size() - 1);
    if (!dst) return fail(RL_ERR_INVALID, "%s: null destination", fn);
    return RL_OK;
}

extern "C" int rl_calc_range_fan_multi_device(rl_method *h, const float *poses, int n_poses, float fov, int num_rays,
                                              int consumer, float *d_outs_on_consumer, int chunks)
{
    int rc = check_fan_args(h, n_poses, fov, num_rays);
    if (rc) return rc;
    if (n_poses == 0) return RL_OK;
    if ((rc = multi_device_check(h, consumer, d_outs_on_consumer, "rl_calc_range_fan_multi_device"))) return rc;
    if (!poses) return fail(RL_ERR_INVALID, "rl_calc_range_fan_multi_device: null pose pointer");
    MultiCall mc(h);
    const int consumer_dev = h->reps[consumer]->map->device, ch = chunks > 0 ? chunks : 4;
    const float nstd = mc.nstd;
    const uint64_t seed = mc.seed, off = mc.off;
    // (every device takes part from multi_min_poses poses per device up; the consumer always owns a block — block 0 is its own)
    return mc.run(*h->pool, n_poses, multi_parts(h, n_poses), consumer, num_rays, [=](const MultiBlock &b) {
        const size_t r0 = (size_t)b.lo * num_rays;
        return replica_fan_to_consumer(h->reps[b.replica], poses + 3 * b.lo, (int)(b.hi - b.lo), fov, num_rays, nstd, seed, off + r0,
                                       b.replica == consumer, consumer_dev, d_outs_on_consumer + r0, ch);
    });
}

extern "C" int rl_check_collision_groups_multi_device(rl_method *h, const float *poses, int n_groups, int group, float fov,
                                                      int num_rays, const double *edge, double crash_thresh, int consumer,
                                                      int *d_first_on_consumer)
{
    int rc = check_groups_args(n_groups, group);
    if (rc || (rc = check_fan_args(h, n_groups * group, fov, num_rays))) return rc;
    if (n_groups == 0) return RL_OK;
    if ((rc = multi_device_check(h, consumer, d_first_on_consumer, "rl_check_collision_groups_multi_device"))) return rc;
    if (!poses || !edge) return fail(RL_ERR_INVALID, "rl_check_collision_groups_multi_device: null pointer");
    if (h->kind != RL_RM && h->kind != RL_RM_GPU) return fail(RL_ERR_UNSUPPORTED, "fused crash test needs a ray-marching method");
    MultiCall mc(h);
    const int consumer_dev = h->reps[consumer]->map->device;
    const int k = (int)std::max<long>(1, std::min<long>(multi_parts(h, (long)n_groups * group), n_groups));
    return mc.run(*h->pool, n_groups, k, consumer, (uint64_t)group * num_rays, [=](const MultiBlock &b) {
        return replica_crash_to_consumer(h->reps[b.replica], poses + 3 * (size_t)b.lo * group, (int)(b.hi - b.lo), group, fov, num_rays,
                                         edge, crash_thresh, b.replica == consumer, consumer_dev, d_first_on_consumer + b.lo);
    });
}

extern "C" int rl_calc_range_fan(rl_method *h, const float *poses, int n_poses, float fov,
                                 int num_rays, float *outs, int32_t *hits, uint16_t *steps)
{
    int rc = check_fan_args(h, n_poses, fov, num_rays);
    if (rc) return rc;
    if (n_poses > 0 && (!poses || !outs))
        return fail(RL_ERR_INVALID, "rl_calc_range_fan: null pointer");
    if (!h->reps.empty()) return n_poses ? multi_fan(h, poses, nullptr, n_poses, fov, num_rays, outs, hits, steps) : RL_OK;
    std::lock_guard<std::mutex> lk(h->mu);
    std::shared_lock<std::shared_mutex> ml(h->map->tables_mu);
    return fan_host(h, poses, n_poses, fov, num_rays, outs, hits, steps, nullptr, 0.0, nullptr);
}

extern "C" int rl_calc_range_many_fan(rl_method *h, const float *ins_rows3, float *outs, int n_rows,
                                      float fov, int num_rays)
{
    if (!h) return fail(RL_ERR_INVALID, "null method handle");
    if (num_rays <= 0) return fail(RL_ERR_INVALID, "num_rays must be > 0");
    if (n_rows < 0) return fail(RL_ERR_INVALID, "n_rows must be >= 0");
    // n_poses = ins.shape[0] / num_rays; trailing rows that do
    // not make a whole fan are left untouched
    const int n_poses = n_rows / num_rays;
    int rc = check_fan_args(h, n_poses, fov, num_rays);
    if (rc) return rc;
    if (n_poses > 0 && (!ins_rows3 || !outs))
        return fail(RL_ERR_INVALID, "rl_calc_range_many_fan: null pointer");
    if (!h->reps.empty()) return n_poses ? multi_fan(h, nullptr, ins_rows3, n_poses, fov, num_rays, outs, nullptr, nullptr) : RL_OK;
    std::lock_guard<std::mutex> lk(h->mu);
    std::shared_lock<std::shared_mutex> ml(h->map->tables_mu);
    // gather the live row of every pose (row p*num_rays): 12 B per pose cross PCIe,
    // not the reference's 12 B per ray (scripts/scan_simulator.py:39-40)
    h->h_poses.resize((size_t)n_poses * 3);
    for (int p = 0; p < n_poses; ++p) {
        const float *row = ins_rows3 + (size_t)p * num_rays * 3;
        h->h_poses[3 * (size_t)p] = row[0];
        h->h_poses[3 * (size_t)p + 1] = row[1];
        h->h_poses[3 * (size_t)p + 2] = row[2];
    }
    return fan_host(h, h->h_poses.data(), n_poses, fov, num_rays, outs, nullptr, nullptr, nullptr,
                    0.0, nullptr);
}

extern "C" int rl_calc_range_many(rl_method *h, const float *ins, float *outs, int n)
{
    if (!h) return fail(RL_ERR_INVALID, "null method handle");
    if (n < 0) return fail(RL_ERR_INVALID, "n must be >= 0");
    if (n == 0) return RL_OK;
    if (!ins || !outs) return fail(RL_ERR_INVALID, "rl_calc_range_many: null pointer");
    if (!h->reps.empty()) return multi_rays(h, ins, outs, n);
    return rays_host(h, ins, outs, n);
}

extern "C" int rl_check_collision_many(rl_method *h, const float *poses, int n_poses, float fov,
                                       int num_rays, const double *edge, double crash_thresh,
                                       int *first_crashed, float *ranges_or_null)
{
    int rc = check_fan_args(h, n_poses, fov, num_rays);
    if (rc) return rc;
    if (!first_crashed || !edge || (n_poses > 0 && !poses))
        return fail(RL_ERR_INVALID, "rl_check_collision_many: null pointer");
    if (n_poses == 0) {
        *first_crashed = -1;
        return RL_OK;
    }
    if (!h->reps.empty())
        return multi_crash(h, poses, 1, n_poses, fov, num_rays, edge, crash_thresh, first_crashed, ranges_or_null, true);
    if (h->kind != RL_RM && h->kind != RL_RM_GPU)      // generic: scan, then one crash pass
        return rl_check_collision_groups(h, poses, 1, n_poses, fov, num_rays, edge, crash_thresh,
                                         first_crashed, ranges_or_null);
    std::lock_guard<std::mutex> lk(h->mu);
    std::shared_lock<std::shared_mutex> ml(h->map->tables_mu);
    return fan_host(h, poses, n_poses, fov, num_rays, ranges_or_null, nullptr, nullptr, edge,
                    crash_thresh, first_crashed);
}


extern "C" int rl_check_collision_groups(rl_method *h, const float *poses, int n_groups, int group,
                                         float fov, int num_rays, const double *edge,
                                         double crash_thresh, int *first_crashed, float *ranges_or_null)
{
    int rc = check_groups_args(n_groups, group);
    if (rc) return rc;
    const int n_poses = n_groups * group;
    if ((rc = check_fan_args(h, n_poses, fov, num_rays))) return rc;
    if (n_groups == 0) return RL_OK;
    if (!poses || !edge || !first_crashed) return fail(RL_ERR_INVALID, "rl_check_collision_groups: null pointer");
    if (!h->reps.empty())
        return multi_crash(h, poses, n_groups, group, fov, num_rays, edge, crash_thresh, first_crashed, ranges_or_null, false);
    std::lock_guard<std::mutex> lk(h->mu);
    std::shared_lock<std::shared_mutex> ml(h->map->tables_mu);
    if ((rc = set_device(h->map))) return rc;
    const size_t n_rays = (size_t)n_poses * num_rays;
    HostCall hc(h->stream);
    if ((rc = hc.up(h->poses, poses, (size_t)n_poses * 3)) || (rc = hc.room(h->outs, n_rays)) ||
        (rc = upload_edge(h, edge, num_rays)) || (rc = hc.room(h->flag, n_groups)) ||
        (rc = crash_groups_device(h, LaunchArgs::of(h), h->poses, n_groups, group, fov, num_rays, h->edge, crash_thresh, h->flag,
                                  h->outs, hc.st)) ||
        (rc = hc.down(first_crashed, h->flag, n_groups)) || (rc = hc.down(ranges_or_null, h->outs, n_rays)))
        return rc;
    return hc.finish();
}

