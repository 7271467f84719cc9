// abi_car.hip — what sits in front of and behind the scan path in libscan_amd.so (C ABI: include/scanlib.h; SURVEY.md
// section 8f): the MCTS roll-out generator, FollowGap, the policy network, the race scan; the closed-loop session (loop_args,
// SteerSource and Loop: handle checks, who steers, locks, scan-then-consume) with its users drive_loop, rl_env_*, rl_mcts_*;
// track-guided planning (include/scanlib_track_plan.h: the planner's track, rl_car_rollout_track); per-seat drivers
// (include/scanlib_seats.h: rl_car_race_seats, rl_env_attach_seats); policy populations (include/scanlib_population.h:
// rl_policy_pop_*, rl_car_drive_population); league races (include/scanlib_league.h: rl_policy_pop_eval_rows,
// rl_car_race_league); league line-ups in the race environment (include/scanlib_league_env.h: rl_env_attach_league,
// rl_env_set_league_entries*, rl_env_read_league_*); track progress of the roll-outs (include/scanlib_track_drive.h:
// rl_car_attach_track, rl_car_read_track*);
// 16-bit ranges for the xGMI exchange, diagnostics probes, the car-outline table and Car::isCrashed on the host.
#include "abi_internal.h"
#pragma GCC visibility push(default)
#include "../../include/scanlib_track_plan.h"
#include "../../include/scanlib_seats.h"
#include "../../include/scanlib_population.h"
#include "../../include/scanlib_league.h"
#include "../../include/scanlib_league_env.h"
#include "../../include/scanlib_track_drive.h"
#pragma GCC visibility pop
#include <array>
#include <utility>
#include "car_kernels.h"
#include "consumer_kernels.h"
#include "drive_kernels.h"
#include "env_kernels.h"
#include "track_kernels.h"
#include "drive_track_kernels.h"
#include "mcts_kernels.h"
#include "plan_track_kernels.h"
#include "plan_pursuit_kernels.h"
#include "policy_kernels.h"
#include "probe_kernels.h"
#include "race_kernels.h"
#include "league_kernels.h"

struct rl_car {
    std::vector<rl_car *> reps;          // multi-device (rl_car_create_multi): one ordinary handle per device
    std::unique_ptr<MultiPool> pool;
    int device = 0;
    CarParams P{};
    Stream stream;
    // per-call staging, counted in scalars: 11 doubles a car state, 2 an action, 3 floats a pose
    DevPtr<double> states, actions, states_out, vel, edge;
    DevPtr<float> poses, ranges;
    DevPtr<int> first;
    DevPtr<double> speeds, tr_states;                          // rl_car_drive_followgap, rl_car_drive_policy
    DevPtr<float> steer0, tr_steers, tr_poses;
    DevPtr<float> mlp;                                         // rl_car_drive_policy: the network's steers of a tick
    DevPtr<int> seat_rows;                                     // rl_car_race_seats: the cars in policy seats
    DevPtr<double> pop_states0, pop_fitness;                   // rl_car_drive_population: the starts, fitness [n][2]
                                                               // (rl_car_race_league: the starts, standings [N][4])
    DevPtr<double> o_cars;                                     // rl_car_outline_cells
    DevPtr<int32_t> o_cells;
    DevPtr<int> o_counts;
    // rl_car_rollout_track: the roll-outs' f64 positions, their terms and s, and the per-roll-out roots (PlanRoots)
    DevPtr<double> tk_xy, tk_terms, tk_s, tk_start_s, tk_root_s, tk_point, tk_points_in;
    DevPtr<int> tk_seg, tk_root_seg, tk_goal, tk_has;
    // track progress of the roll-outs (rl_car_attach_track): the borrowed track, its options (goal: L where the caller
    // gave 0), the rows of the last tracked call, its R (0: none yet) and the shape of the scores it left (0: none)
    rl_track *track = nullptr;
    int dt_window = 0;
    double dt_goal = 0.0;
    DevPtr<double> dt_rows, dt_scores;
    DevPtr<int> dt_ints;
    int dt_cars = 0, dt_score_rows = 0, dt_score_cols = 0;
    std::mutex mu;
};

extern "C" int rl_car_create(int device, const double *p, rl_car **out)
{
    if (!p || !out) return fail(RL_ERR_INVALID, "rl_car_create: null pointer");
    int rc = check_device(device);
    if (rc) return rc;
    std::unique_ptr<rl_car, decltype(&rl_car_destroy)> c(new (std::nothrow) rl_car(), rl_car_destroy);
    if (!c) return fail(RL_ERR_NOMEM, "out of host memory");
    c->device = device;
    c->P = CarParams{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11], p[12],
                     p[13], p[14], p[15], p[16]};
    if (hipSetDevice(device) != hipSuccess || c->stream.create() != hipSuccess) return fail(RL_ERR_HIP, "stream creation failed");
    *out = c.release();
    return RL_OK;
}

extern "C" int rl_car_create_multi(const int *devices, int n_devices, const double *p, rl_car **out)
{
    if (!p || !out || !devices) return fail(RL_ERR_INVALID, "rl_car_create_multi: null pointer");
    if (n_devices < 1 || n_devices > 64) return fail(RL_ERR_INVALID, "rl_car_create_multi: 1..64 devices (got %d)", n_devices);
    std::unique_ptr<rl_car, decltype(&rl_car_destroy)> c(new (std::nothrow) rl_car(), rl_car_destroy);
    if (!c) return fail(RL_ERR_NOMEM, "out of host memory");
    std::vector<int> devs;
    for (int i = 0; i < n_devices; ++i) {
        rl_car *r = nullptr;
        const int rc = rl_car_create(devices[i], p, &r);
        if (rc) {
            const std::string keep = last_error();     // (the failing replica's message outlives the clean-up)
            c.reset();
            set_last_error(keep);
            return rc;
        }
        c->reps.push_back(r);
        devs.push_back(devices[i]);
    }
    c->device = devices[0];
    c->P = c->reps[0]->P;
    c->pool = std::make_unique<MultiPool>();
    c->pool->start(devs);
    *out = c.release();
    return RL_OK;
}

extern "C" void rl_car_destroy(rl_car *c)
{
    if (!c) return;
    if (!c->reps.empty() || c->pool) {
        c->pool.reset();
        for (rl_car *r : c->reps) rl_car_destroy(r);
        delete c;
        return;
    }
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;
}

static int check_rollout_args(int R, int n_steps, int every)
{
    if (R < 0 || n_steps <= 0 || every <= 0) return fail(RL_ERR_INVALID, "n_rollouts >= 0, n_steps > 0, action_every > 0 required");
    return RL_OK;
}

// the roll-outs of hc's call (on c's stream): states and actions up, rollout_kernel into c->poses (and, when wanted,
// c->states_out and c->vel; d_xy: the f64 positions [R][n_steps][2] where the caller wants them)
static int car_rollout_device(rl_car *c, HostCall &hc, const double *states_in, const double *actions, int R, int n_steps,
                              int every, double dt, bool want_states, bool want_vel, double *d_xy = nullptr)
{
    int rc = check_rollout_args(R, n_steps, every);
    if (rc) return rc;
    if ((long)R * n_steps > INT_MAX / 4) return fail(RL_ERR_INVALID, "too many roll-out poses");
    HIPCHK(hipSetDevice(c->device));
    if (R == 0) return RL_OK;
    const size_t n_act = (size_t)(n_steps + every - 1) / every, n_poses = (size_t)R * n_steps;
    if ((rc = hc.up(c->states, states_in, (size_t)R * 11)) || (rc = hc.up(c->actions, actions, R * n_act * 2)) ||
        (rc = hc.room(c->poses, n_poses * 3)) || (rc = hc.room(c->states_out, (size_t)R * 11)) ||
        (rc = hc.room(c->vel, n_poses)))
        return rc;
    if (d_xy)           // (rl_car_rollout_track: poses, velocities and positions, no final states)
        return launch("rollout_xy_kernel", rollout_xy_kernel, dim3((R + 63) / 64), dim3(64), 0, hc.st, c->P, c->states, c->actions, R,
                      n_steps, every, dt, c->poses, c->vel, d_xy);
    return launch("rollout_kernel", rollout_kernel, dim3((R + 63) / 64), dim3(64), 0, hc.st, c->P, c->states, c->actions, R, n_steps,
                  every, dt, c->poses, want_states ? (double *)c->states_out : nullptr, want_vel ? (double *)c->vel : nullptr);
}

extern "C" int rl_car_rollout(rl_car *c, const double *states_in, const double *actions, int R,
                              int n_steps, int every, double dt, float *poses_out, double *states_out,
                              double *vel_out)
{
    if (!c || (R > 0 && (!states_in || !actions || !poses_out))) return fail(RL_ERR_INVALID, "rl_car_rollout: null pointer");
    if (!c->reps.empty()) {
        // roll-outs are independent: contiguous blocks of them, one per device (a device per 64 roll-outs)
        const int rc = check_rollout_args(R, n_steps, every);
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(c->mu);
        const int k = (int)std::max<long>(1, std::min<long>((long)c->reps.size(), (long)R / 64));
        const size_t n_act = (size_t)(n_steps + every - 1) / every;
        return run_blocks(*c->pool, R, k, 0, [=](const MultiBlock &b) {
            const long lo = b.lo;
            return rl_car_rollout(c->reps[b.replica], states_in + 11 * lo, actions + 2 * n_act * lo, (int)(b.hi - lo), n_steps, every,
                                  dt, poses_out + (size_t)3 * n_steps * lo, states_out ? states_out + 11 * lo : nullptr,
                                  vel_out ? vel_out + (size_t)n_steps * lo : nullptr);
        });
    }
    std::lock_guard<std::mutex> lk(c->mu);
    HostCall hc(c->stream);
    int rc = car_rollout_device(c, hc, states_in, actions, R, n_steps, every, dt, states_out != nullptr, vel_out != nullptr);
    if (rc || R == 0) return rc;
    const size_t n_poses = (size_t)R * n_steps;
    if ((rc = hc.down(poses_out, c->poses, n_poses * 3)) || (rc = hc.down(states_out, c->states_out, (size_t)R * 11)) ||
        (rc = hc.down(vel_out, c->vel, n_poses)))
        return rc;
    return hc.finish();
}

extern "C" int rl_car_rollout_check(rl_car *c, rl_method *h, const double *states_in, const double *actions,
                                    int R, int n_steps, int every, double dt, float fov, int num_rays,
                                    const double *edge, double crash_thresh, int *first_crashed,
                                    double *states_out, double *vel_out)
{
    if (!c || !h || (R > 0 && (!states_in || !actions || !edge || !first_crashed)))
        return fail(RL_ERR_INVALID, "rl_car_rollout_check: null pointer");
    if (c->reps.empty() != h->reps.empty() || c->reps.size() != h->reps.size())
        return fail(RL_ERR_INVALID, "car and range method must both be single-device or span the same devices");
    if (!c->reps.empty()) {
        // MCTS.rollout + checkCollisionMany for R roll-outs over several devices: contiguous blocks of roll-outs,
        // each device integrates, scans and tests its own (nothing but the crash indices comes back)
        const int rc = check_rollout_args(R, n_steps, every);
        if (rc) return rc;
        for (size_t i = 0; i < c->reps.size(); ++i)
            if (c->reps[i]->device != h->reps[i]->map->device)
                return fail(RL_ERR_INVALID, "car and range method replicas live on different devices");
        MultiCall mc(h, c->mu);
        const int k = (int)std::max<long>(1, std::min<long>(multi_parts(h, (long)R * n_steps), std::max(R, 1)));
        const size_t n_act = (size_t)(n_steps + every - 1) / every;
        return mc.run(*c->pool, R, k, 0, (uint64_t)n_steps * num_rays, [=](const MultiBlock &b) {
            const long lo = b.lo;
            return rl_car_rollout_check(c->reps[b.replica], h->reps[b.replica], states_in + 11 * lo, actions + 2 * n_act * lo,
                                        (int)(b.hi - lo), n_steps, every, dt, fov, num_rays, edge, crash_thresh, first_crashed + lo,
                                        states_out ? states_out + 11 * lo : nullptr,
                                        vel_out ? vel_out + (size_t)n_steps * lo : nullptr);
        });
    }
    if (c->device != h->map->device) return fail(RL_ERR_INVALID, "car and range method live on different devices");
    std::scoped_lock lk(c->mu, h->mu);
    std::shared_lock<std::shared_mutex> ml(h->map->tables_mu);
    HostCall hc(c->stream);
    int rc = car_rollout_device(c, hc, states_in, actions, R, n_steps, every, dt, states_out != nullptr, vel_out != nullptr);
    if (rc || R == 0) return rc;
    if ((rc = check_fan_args(h, R * n_steps, fov, num_rays))) return rc;
    const size_t n_poses = (size_t)R * n_steps;
    if ((rc = hc.room(c->ranges, n_poses * num_rays)) || (rc = hc.up(c->edge, edge, num_rays)) || (rc = hc.room(c->first, R)) ||
        (rc = crash_groups_device(h, LaunchArgs::of(h), c->poses, R, n_steps, fov, num_rays, c->edge, crash_thresh, c->first,
                                  c->ranges, hc.st)) ||
        (rc = hc.down(first_crashed, c->first, R)) || (rc = hc.down(states_out, c->states_out, (size_t)R * 11)) ||
        (rc = hc.down(vel_out, c->vel, n_poses)))
        return rc;
    return hc.finish();
}


// ---------------------------------------------------------------- FollowGap
struct rl_followgap {
    int device = 0;
    FollowGapParams P{};
    int window_size = 0;           // kept for the caller; FollowGap::eval never reads it
    int n_cu = 256;                // (queried once: hipGetDeviceProperties costs the host tens of microseconds per call)
    bool walk_kernel = false;      // diagnostics (environment RL_FOLLOWGAP_WALK=1 at create): followgap_kernel at every size
    Stream stream;
    DevPtr<float> scans, angles;
    std::mutex mu;
};

extern "C" int rl_followgap_create(int device, int window_size, float max_distance, float max_angle,
                                   float angle_inc, rl_followgap **out)
{
    if (!out) return fail(RL_ERR_INVALID, "rl_followgap_create: null pointer");
    int rc = check_device(device);
    if (rc) return rc;
    std::unique_ptr<rl_followgap, decltype(&rl_followgap_destroy)> g(new (std::nothrow) rl_followgap(), rl_followgap_destroy);
    if (!g) return fail(RL_ERR_NOMEM, "out of host memory");
    g->device = device;
    g->window_size = window_size;
    g->P.max_distance = max_distance;
    g->P.max_angle = max_angle;
    g->P.angle_inc = angle_inc;
    const char *walk = getenv("RL_FOLLOWGAP_WALK");
    g->walk_kernel = walk && walk[0] == '1';
    if (hipSetDevice(device) != hipSuccess || g->stream.create() != hipSuccess) return fail(RL_ERR_HIP, "stream creation failed");
    int n_cu = 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n_cu > 0) g->n_cu = n_cu;
    *out = g.release();
    return RL_OK;
}

extern "C" void rl_followgap_destroy(rl_followgap *g)
{
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    delete g;
}

// a kernel's ROWS = 1 ... FG_ROWS instantiations, indexed by ROWS - 1: make(std::integral_constant<int, ROWS>) names one
template <class Fn, class Make, int... R>
static std::array<Fn, sizeof...(R)> rows_table(Make make, std::integer_sequence<int, R...>)
{
    return {{make(std::integral_constant<int, R + 1>())...}};
}
template <class Fn, class Make>
static std::array<Fn, FG_ROWS> rows_table(Make make)
{
    return rows_table<Fn>(make, std::make_integer_sequence<int, FG_ROWS>());
}

typedef void (*fg_bits_fn)(const float *, int, FollowGapParams, float *);
static const std::array<fg_bits_fn, FG_ROWS> fg_bits_table =
    rows_table<fg_bits_fn>([](auto rows) { return followgap_bits_kernel<rows>; });

static int followgap_launch(rl_followgap *g, const float *d_scans, int n_scans, int size,
                            float *d_angles, hipStream_t stream)
{
    if (n_scans < 0) return fail(RL_ERR_INVALID, "n_scans must be >= 0");
    // (the reference's preprocessLidar runs off its vector below 10 beams, followgap.hpp:21)
    if (size < 10) return fail(RL_ERR_INVALID, "FollowGap needs at least 10 beams per scan (got %d)", size);
    if (size > 12288) return fail(RL_ERR_UNSUPPORTED, "at most 12288 beams per scan (got %d)", size);
    if (n_scans == 0) return RL_OK;
    FollowGapParams p = g->P;
    p.size = size;
    const int grid = std::min(n_scans, g->n_cu * 32);
    if (size <= 64 * FG_ROWS && !g->walk_kernel)
        return launch("followgap_bits_kernel", fg_bits_table[(size + 63) / 64 - 1], dim3(grid), dim3(64), 0, stream, d_scans, n_scans,
                      p, d_angles);
    return launch("followgap_kernel", followgap_kernel, dim3(grid), dim3(64), (size_t)size * sizeof(float), stream, d_scans, n_scans,
                  p, d_angles);
}

extern "C" int rl_followgap_eval(rl_followgap *g, const float *scans, int n_scans, int size,
                                 float *angles)
{
    if (!g || !scans || !angles) return fail(RL_ERR_INVALID, "rl_followgap_eval: null pointer");
    std::lock_guard<std::mutex> lk(g->mu);
    HIPCHK(hipSetDevice(g->device));
    if (n_scans < 0 || size < 10)
        return followgap_launch(g, nullptr, n_scans, size, nullptr, g->stream);   // (argument errors)
    if (n_scans == 0) return RL_OK;
    HostCall hc(g->stream);
    int rc;
    if ((rc = hc.up(g->scans, scans, (size_t)n_scans * size)) || (rc = hc.room(g->angles, n_scans)) ||
        (rc = followgap_launch(g, g->scans, n_scans, size, g->angles, hc.st)) || (rc = hc.down(angles, g->angles, n_scans)))
        return rc;
    return hc.finish();
}

extern "C" int rl_followgap_eval_device(rl_followgap *g, const float *d_scans, int n_scans, int size,
                                        float *d_angles, void *hip_stream)
{
    if (!g || (n_scans > 0 && (!d_scans || !d_angles)))
        return fail(RL_ERR_INVALID, "rl_followgap_eval_device: null pointer");
    std::lock_guard<std::mutex> lk(g->mu);
    HIPCHK(hipSetDevice(g->device));
    return followgap_launch(g, d_scans, n_scans, size, d_angles, (hipStream_t)hip_stream);
}

// ---------------------------------------------------------------- batched races (race_kernels.h)
// the canonical outline's host-side constants (include/scanlib.h)
static int race_outline(const rl_map *m, double length, double width, OutlineParams &o)
{
    if (!(length > 0.0 && width > 0.0 && std::isfinite(length) && std::isfinite(width)))
        return fail(RL_ERR_INVALID, "car length and width must be finite and > 0 (got %g, %g)", length, width);
    if (m->rows > 32767 || m->cols > 32767)
        return fail(RL_ERR_UNSUPPORTED, "races need a map below 32768 cells a side (got %d x %d)", m->rows, m->cols);
    const double res = (double)m->mp.res, spacing = 0.5 * res;
    const double n_l = std::max(1.0, std::ceil(length / spacing)), n_w = std::max(1.0, std::ceil(width / spacing));
    if (2.0 * (n_l + n_w) > RACE_MAX_POINTS)
        return fail(RL_ERR_UNSUPPORTED, "a %g x %g m car at %g m per cell takes %.0f outline points (at most %d)", length,
                    width, res, 2.0 * (n_l + n_w), RACE_MAX_POINTS);
    o.half_l = length / 2.0;
    o.half_w = width / 2.0;
    o.n_l = (int)n_l;
    o.n_w = (int)n_w;
    o.ox = (double)m->mp.ox;
    o.oy = (double)m->mp.oy;
    o.inv_res = 1.0 / res;
    o.wa_cos = (double)m->mp.wa_cos;
    o.wa_sin = (double)m->mp.wa_sin;
    o.rows = m->rows;
    o.cols = m->cols;
    return RL_OK;
}

static int race_group(int group)
{
    if (group < 1 || group > RACE_MAX_GROUP)
        return fail(RL_ERR_INVALID, "group must lie in [1, %d] cars (got %d)", RACE_MAX_GROUP, group);
    return RL_OK;
}

static int race_args(rl_method *h, long n_groups, int group, int num_rays)
{
    if (!h->reps.empty()) return fail(RL_ERR_INVALID, "races are single-device only: pass an ordinary (not multi-device) method");
    int rc = race_group(group);
    if (rc) return rc;
    if (n_groups < 0) return fail(RL_ERR_INVALID, "n_groups must be >= 0 (got %ld)", n_groups);
    if (num_rays < 10 || num_rays > RACE_MAX_RAYS)
        return fail(RL_ERR_INVALID, "num_rays must lie in [10, %d] (got %d)", RACE_MAX_RAYS, num_rays);
    if (n_groups * group * num_rays >= (1L << 31)) return fail(RL_ERR_INVALID, "n_groups * group * num_rays must stay below 2^31");
    if (h->kind == RL_CDDT && h->race_cddt) {
        // race_cddt_kernel's per-bin ranges: group x theta_disc floats of LDS
        if ((long)group * h->theta_disc > RACE_CDDT_MAX_BINS)
            return fail(RL_ERR_UNSUPPORTED, "a CDDT race keeps group x theta_disc per-bin ranges in LDS: at most %d (got %d x %d)",
                        RACE_CDDT_MAX_BINS, group, h->theta_disc);
        return RL_OK;
    }
    if (h->kind != RL_RM && h->kind != RL_RM_GPU)
        return fail(RL_ERR_UNSUPPORTED, "races run on ray marching only (RM, RMGPU): a CDDT, GiantLUT or Bresenham table "
                                        "covers the whole map and cannot see the other cars");
    if (h->opt.variant == 2)
        return fail(RL_ERR_UNSUPPORTED, "races need the canonical (variant 0 / 1) or the upstream-literal (3) arithmetic, "
                                        "not the occupancy window (2)");
    return RL_OK;
}

typedef void (*race_fn)(MapParams, FanParams, LiteralParams, RaceParams, const float *, float *, int32_t *, uint16_t *);
static const race_fn race_table[2][2] = {{race_fan_kernel<false, false>, race_fan_kernel<false, true>},
                                         {race_fan_kernel<true, false>, race_fan_kernel<true, true>}};

// one race_fan_kernel launch on `stream`: the caller holds h->mu and the map's tables_mu and has checked the arguments
static int launch_race(rl_method *h, const LaunchArgs &a, const float *d_poses, const double *d_cars, int car_stride, int n_groups,
                       int group, const OutlineParams &o, float fov, int num_rays, float *d_out, int32_t *d_hits,
                       uint16_t *d_steps, hipStream_t stream)
{
    if (n_groups == 0) return RL_OK;
    const bool lit = h->opt.variant == 3, aux = d_hits || d_steps;
    const FanParams f = make_fan(h, n_groups * group, fov, num_rays, a.ray_offset);
    const LiteralParams lp = lit ? make_literal(h->map) : LiteralParams{};
    const RaceParams rp{o, d_cars, car_stride, group, n_groups};
    if (h->kind == RL_CDDT) {                    // (option race_cddt: race_args let the handle through)
        if (aux) return fail(RL_ERR_UNSUPPORTED, "hit cells / step counts exist only for RM and Bresenham");
        return launch_race_cddt(h, a, f, rp, d_poses, d_out, stream);
    }
    if (a.timing) HIPCHK(hipEventRecord(h->ev0, stream));
    const int rc = launch("race_fan_kernel", race_table[lit][aux], dim3(n_groups), dim3(RACE_WG), 0, stream, h->map->mp, f, lp, rp,
                          d_poses, d_out, d_hits, d_steps);
    if (rc) return rc;
    if (a.timing) {
        HIPCHK(hipEventRecord(h->ev1, stream));
        h->timed = true;
    }
    return RL_OK;
}

static int fan_cars_checks(rl_method *h, int n_groups, int group, float fov, int num_rays, double length, double width,
                           bool aux, OutlineParams &o)
{
    int rc = race_args(h, n_groups, group, num_rays);
    if (rc) return rc;
    if (aux && h->kind == RL_CDDT) return fail(RL_ERR_UNSUPPORTED, "hit cells / step counts exist only for RM and Bresenham");
    if ((rc = check_fan_args(h, n_groups * group, fov, num_rays))) return rc;
    return race_outline(h->map, length, width, o);
}

extern "C" int rl_calc_range_fan_cars_device(rl_method *h, const float *d_poses, const double *d_cars, int n_groups,
                                             int group, double length, double width, float fov, int num_rays,
                                             float *d_outs, int32_t *d_hits, uint16_t *d_steps, void *hip_stream)
{
    if (!h || (n_groups > 0 && (!d_poses || !d_cars || !d_outs)))
        return fail(RL_ERR_INVALID, "rl_calc_range_fan_cars_device: null pointer");
    OutlineParams o{};
    int rc = fan_cars_checks(h, n_groups, group, fov, num_rays, length, width, d_hits || d_steps, o);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    std::shared_lock<std::shared_mutex> ml(h->map->tables_mu);
    if ((rc = set_device(h->map))) return rc;
    return launch_race(h, LaunchArgs::of(h), d_poses, d_cars, 3, n_groups, group, o, fov, num_rays, d_outs, d_hits, d_steps,
                       (hipStream_t)hip_stream);
}

extern "C" int rl_calc_range_fan_cars(rl_method *h, const float *poses, const double *cars, int n_groups, int group,
                                      double length, double width, float fov, int num_rays, float *outs,
                                      int32_t *hits_or_null, uint16_t *steps_or_null)
{
    if (!h || (n_groups > 0 && (!poses || !cars || !outs))) return fail(RL_ERR_INVALID, "rl_calc_range_fan_cars: null pointer");
    OutlineParams o{};
    int rc = fan_cars_checks(h, n_groups, group, fov, num_rays, length, width, hits_or_null || steps_or_null, o);
    if (rc || n_groups == 0) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    std::shared_lock<std::shared_mutex> ml(h->map->tables_mu);
    if ((rc = set_device(h->map))) return rc;
    const size_t n = (size_t)n_groups * group, n_rays = n * num_rays;
    HostCall hc(h->stream);
    if ((rc = hc.up(h->poses, poses, n * 3)) || (rc = hc.up(h->cars, cars, n * 3)) || (rc = hc.room(h->outs, n_rays)) ||
        (hits_or_null && (rc = hc.room(h->hits, n_rays * 2))) || (steps_or_null && (rc = hc.room(h->steps, n_rays))) ||
        (rc = launch_race(h, LaunchArgs::of(h), h->poses, h->cars, 3, n_groups, group, o, fov, num_rays, h->outs,
                          hits_or_null ? (int32_t *)h->hits : nullptr, steps_or_null ? (uint16_t *)h->steps : nullptr, hc.st)) ||
        (rc = hc.down(outs, h->outs, n_rays)) || (rc = hc.down(hits_or_null, h->hits, n_rays * 2)) ||
        (rc = hc.down(steps_or_null, h->steps, n_rays)))
        return rc;
    return hc.finish();
}

extern "C" int rl_car_outline_cells(rl_car *c, rl_map *m, const double *cars_p3, int n, int max_cells, int32_t *cells,
                                    int *counts)
{
    if (!c || !m || (n > 0 && (!cars_p3 || !cells || !counts))) return fail(RL_ERR_INVALID, "rl_car_outline_cells: null pointer");
    if (!c->reps.empty() || !m->reps.empty())
        return fail(RL_ERR_INVALID, "rl_car_outline_cells is single-device only: pass ordinary (not multi-device) handles");
    if (c->device != m->device) return fail(RL_ERR_INVALID, "car and map live on different devices");
    if (n < 0) return fail(RL_ERR_INVALID, "n must be >= 0 (got %d)", n);
    OutlineParams o{};
    int rc = race_outline(m, c->P.LENGTH, c->P.WIDTH, o);
    if (rc) return rc;
    const int n_pts = 2 * (o.n_l + o.n_w);
    if (max_cells < n_pts) return fail(RL_ERR_INVALID, "max_cells must be >= the %d outline points of a car (got %d)", n_pts, max_cells);
    if (n == 0) return RL_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(hipSetDevice(c->device));
    const size_t n_cells = (size_t)n * max_cells;
    HostCall hc(c->stream);
    if ((rc = hc.up(c->o_cars, cars_p3, (size_t)n * 3)) || (rc = hc.room(c->o_cells, n_cells)) || (rc = hc.room(c->o_counts, n)))
        return rc;
    if ((rc = launch("outline_cells_kernel", outline_cells_kernel, dim3((n + 3) / 4), dim3(256), 0, hc.st, o, c->o_cars, n, max_cells,
                     c->o_cells, c->o_counts)) ||
        (rc = hc.down(cells, c->o_cells, n_cells)) || (rc = hc.down(counts, c->o_counts, n)))
        return rc;
    return hc.finish();
}

// ---------------------------------------------------------------- the steering policy network (policy_kernels.h)
struct rl_policy {
    int device = 0;
    PolicyParams P{};                  // device pointers into `weights`
    Stream stream;
    DevPtr<float> weights, scans, steers;
    std::mutex mu;
};

extern "C" int rl_policy_create(int device, int n_layers, const int *dims, const float *const *weights,
                                const float *const *biases, const unsigned char *relu, int in_start, float clip,
                                float scale, rl_policy **out)
{
    if (!dims || !weights || !biases || !relu || !out) return fail(RL_ERR_INVALID, "rl_policy_create: null pointer");
    if (n_layers < 1) return fail(RL_ERR_INVALID, "rl_policy_create: n_layers must be >= 1 (got %d)", n_layers);
    if (n_layers > PM_MAX_LAYERS)
        return fail(RL_ERR_UNSUPPORTED, "rl_policy_create: at most %d layers (got %d)", PM_MAX_LAYERS, n_layers);
    for (int l = 0; l <= n_layers; ++l)
        if (dims[l] < 1) return fail(RL_ERR_INVALID, "rl_policy_create: dims[%d] = %d must be >= 1", l, dims[l]);
    for (int l = 0; l < n_layers; ++l)
        if (!weights[l] || !biases[l]) return fail(RL_ERR_INVALID, "rl_policy_create: null pointer (layer %d)", l);
    if (dims[0] > PM_MAX_IN) return fail(RL_ERR_UNSUPPORTED, "rl_policy_create: input width %d > %d", dims[0], PM_MAX_IN);
    for (int l = 1; l < n_layers; ++l)
        if (dims[l] > PM_MAX_W)
            return fail(RL_ERR_UNSUPPORTED, "rl_policy_create: width %d of layer %d > %d", dims[l], l, PM_MAX_W);
    if (dims[n_layers] != 1)
        return fail(RL_ERR_UNSUPPORTED, "rl_policy_create: one output only (got %d)", dims[n_layers]);
    if (in_start < 0) return fail(RL_ERR_INVALID, "rl_policy_create: in_start must be >= 0 (got %d)", in_start);
    int rc = check_device(device);
    if (rc) return rc;
    // one block: per layer W [K][ceil4(N)] then b [ceil4(N)], zero-padded (16-byte rows for the float4 loads)
    std::vector<float> host;
    std::vector<size_t> offW(n_layers), offB(n_layers);
    for (int l = 0; l < n_layers; ++l) {
        const int K = dims[l], N = dims[l + 1], Np = (N + 3) & ~3;
        offW[l] = host.size();
        host.resize(host.size() + (size_t)K * Np, 0.0f);
        for (int k = 0; k < K; ++k)
            std::memcpy(&host[offW[l] + (size_t)k * Np], weights[l] + (size_t)k * N, (size_t)N * sizeof(float));
        offB[l] = host.size();
        host.resize(host.size() + Np, 0.0f);
        std::memcpy(&host[offB[l]], biases[l], (size_t)N * sizeof(float));
    }
    std::unique_ptr<rl_policy, decltype(&rl_policy_destroy)> p(new (std::nothrow) rl_policy(), rl_policy_destroy);
    if (!p) return fail(RL_ERR_NOMEM, "out of host memory");
    p->device = device;
    if (hipSetDevice(device) != hipSuccess || p->stream.create() != hipSuccess) return fail(RL_ERR_HIP, "stream creation failed");
    if ((rc = p->weights.ensure(host.size()))) return rc;
    if (hipMemcpy(p->weights, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return fail(RL_ERR_HIP, "rl_policy_create: weight upload failed");
    p->P.n_layers = n_layers;
    p->P.relu = 0;
    for (int l = 0; l <= n_layers; ++l) p->P.dims[l] = dims[l];
    for (int l = 0; l < n_layers; ++l) {
        p->P.W[l] = p->weights + offW[l];
        p->P.b[l] = p->weights + offB[l];
        if (relu[l]) p->P.relu |= 1u << l;
    }
    p->P.in_start = in_start;
    p->P.clip = clip;
    p->P.scale = scale;
    *out = p.release();
    return RL_OK;
}

extern "C" void rl_policy_destroy(rl_policy *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    delete p;
}

// scans of `size` beams hold the network's input window (fn: the callers that name themselves in this message)
static int policy_window(const PolicyParams &P, int size, const char *fn = nullptr)
{
    if (size < P.in_start + P.dims[0])
        return fail(RL_ERR_INVALID, "%s%sscans of %d beams do not hold the policy's window [%d, %d)", fn ? fn : "", fn ? ": " : "",
                    size, P.in_start, P.in_start + P.dims[0]);
    return RL_OK;
}

static int policy_args(const rl_policy *p, int n_scans, int size)
{
    if (n_scans < 0) return fail(RL_ERR_INVALID, "n_scans must be >= 0 (got %d)", n_scans);
    return policy_window(p->P, size);
}

static int policy_launch(rl_policy *p, const float *d_scans, int n_scans, int size, float *d_steers, hipStream_t st)
{
    if (n_scans == 0) return RL_OK;
    return launch("policy_mlp_kernel", policy_mlp_kernel, dim3((n_scans + PM_CARS - 1) / PM_CARS), dim3(64), 0, st, p->P, d_scans,
                  n_scans, size, d_steers);
}

// the row-indexed form: the network for the n_rows scans d_rows names, answers to d_steers[row]
static int policy_rows_launch(const PolicyParams &P, const float *d_scans, const int *d_rows, int n_rows, int size,
                              float *d_steers, hipStream_t st)
{
    if (n_rows == 0) return RL_OK;
    return launch("policy_mlp_rows_kernel", policy_mlp_rows_kernel, dim3((n_rows + PM_CARS - 1) / PM_CARS), dim3(64), 0, st, P,
                  d_scans, d_rows, n_rows, size, d_steers);
}

extern "C" int rl_policy_eval(rl_policy *p, const float *scans, int n_scans, int size, float *steers)
{
    if (!p || (n_scans > 0 && (!scans || !steers))) return fail(RL_ERR_INVALID, "rl_policy_eval: null pointer");
    int rc = policy_args(p, n_scans, size);
    if (rc || n_scans == 0) return rc;
    std::lock_guard<std::mutex> lk(p->mu);
    HIPCHK(hipSetDevice(p->device));
    HostCall hc(p->stream);
    if ((rc = hc.up(p->scans, scans, (size_t)n_scans * size)) || (rc = hc.room(p->steers, n_scans)) ||
        (rc = policy_launch(p, p->scans, n_scans, size, p->steers, hc.st)) || (rc = hc.down(steers, p->steers, n_scans)))
        return rc;
    return hc.finish();
}

extern "C" int rl_policy_eval_device(rl_policy *p, const float *d_scans, int n_scans, int size, float *d_steers,
                                     void *hip_stream)
{
    if (!p || (n_scans > 0 && (!d_scans || !d_steers)))
        return fail(RL_ERR_INVALID, "rl_policy_eval_device: null pointer");
    int rc = policy_args(p, n_scans, size);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(p->mu);
    HIPCHK(hipSetDevice(p->device));
    return policy_launch(p, d_scans, n_scans, size, d_steers, (hipStream_t)hip_stream);
}

// ---------------------------------------------------------------- policy populations (include/scanlib_population.h)
// n_members networks of one architecture in one device block: member m's padded block (rl_policy_create's layout) at
// m * stride floats; P.W / P.b point into member 0's.
struct rl_policy_pop {
    int device = 0, n_members = 0, n_params = 0;
    size_t stride = 0;                 // floats of a member's padded block: a multiple of 4
    PolicyParams P{};
    PopLayout L{};
    Stream stream;
    DevPtr<float> weights, theta, scans, steers;
    // league calls (include/scanlib_league.h): the call's member per row, and what the grouping makes of it: per member
    // the count, the segment start in lg_rows and the start in the workgroup table; the table's length in lg_total
    DevPtr<int> lg_member, lg_count, lg_start, lg_wg_start, lg_rows, lg_total;
    DevPtr<int2> lg_table;
    // a caller's stream has work of this handle on it (rl_policy_pop_set_device, rl_policy_pop_eval_device): a call that
    // launches on another stream waits for the device first
    bool foreign = false;
    hipStream_t foreign_st = nullptr;
    std::mutex mu;
};

extern "C" int rl_policy_pop_create(int device, int n_members, int n_layers, const int *dims, const unsigned char *relu,
                                    int in_start, float clip, float scale, rl_policy_pop **out)
{
    if (!dims || !relu || !out) return fail(RL_ERR_INVALID, "rl_policy_pop_create: null pointer");
    if (n_members < 1) return fail(RL_ERR_INVALID, "rl_policy_pop_create: n_members must be >= 1 (got %d)", n_members);
    // (rl_policy_create's checks and codes)
    if (n_layers < 1) return fail(RL_ERR_INVALID, "rl_policy_pop_create: n_layers must be >= 1 (got %d)", n_layers);
    if (n_layers > PM_MAX_LAYERS)
        return fail(RL_ERR_UNSUPPORTED, "rl_policy_pop_create: at most %d layers (got %d)", PM_MAX_LAYERS, n_layers);
    for (int l = 0; l <= n_layers; ++l)
        if (dims[l] < 1) return fail(RL_ERR_INVALID, "rl_policy_pop_create: dims[%d] = %d must be >= 1", l, dims[l]);
    if (dims[0] > PM_MAX_IN)
        return fail(RL_ERR_UNSUPPORTED, "rl_policy_pop_create: input width %d > %d", dims[0], PM_MAX_IN);
    for (int l = 1; l < n_layers; ++l)
        if (dims[l] > PM_MAX_W)
            return fail(RL_ERR_UNSUPPORTED, "rl_policy_pop_create: width %d of layer %d > %d", dims[l], l, PM_MAX_W);
    if (dims[n_layers] != 1)
        return fail(RL_ERR_UNSUPPORTED, "rl_policy_pop_create: one output only (got %d)", dims[n_layers]);
    if (in_start < 0) return fail(RL_ERR_INVALID, "rl_policy_pop_create: in_start must be >= 0 (got %d)", in_start);
    int rc = check_device(device);
    if (rc) return rc;
    std::unique_ptr<rl_policy_pop, decltype(&rl_policy_pop_destroy)> p(new (std::nothrow) rl_policy_pop(), rl_policy_pop_destroy);
    if (!p) return fail(RL_ERR_NOMEM, "out of host memory");
    p->device = device;
    p->n_members = n_members;
    // per layer W [K][ceil4(N)] then b [ceil4(N)], as rl_policy_create lays one network out
    size_t off = 0;
    int theta = 0;
    p->L.n_layers = p->P.n_layers = n_layers;
    for (int l = 0; l <= n_layers; ++l) p->L.dims[l] = p->P.dims[l] = dims[l];
    for (int l = 0; l < n_layers; ++l) {
        const int K = dims[l], N = dims[l + 1], Np = (N + 3) & ~3;
        p->L.theta_off[l] = theta;
        theta += (K + 1) * N;
        p->L.w_off[l] = (int)off;
        off += (size_t)K * Np;
        p->L.b_off[l] = (int)off;
        off += Np;
        if (relu[l]) p->P.relu |= 1u << l;
    }
    p->L.theta_off[n_layers] = p->n_params = theta;
    p->stride = off;
    p->P.in_start = in_start;
    p->P.clip = clip;
    p->P.scale = scale;
    if (hipSetDevice(device) != hipSuccess || p->stream.create() != hipSuccess) return fail(RL_ERR_HIP, "stream creation failed");
    const size_t bytes = (size_t)n_members * p->stride * sizeof(float);
    if ((rc = p->weights.alloc(bytes))) return rc;
    if (hipMemset(p->weights, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(RL_ERR_HIP, "rl_policy_pop_create: zeroing the members failed");
    for (int l = 0; l < n_layers; ++l) {
        p->P.W[l] = p->weights + p->L.w_off[l];
        p->P.b[l] = p->weights + p->L.b_off[l];
    }
    *out = p.release();
    return RL_OK;
}

extern "C" void rl_policy_pop_destroy(rl_policy_pop *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->foreign) (void)hipDeviceSynchronize();
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    delete p;
}

extern "C" int rl_policy_pop_layout(rl_policy_pop *p, int *n_members, int *n_params)
{
    if (!p) return fail(RL_ERR_INVALID, "rl_policy_pop_layout: null pointer");
    if (n_members) *n_members = p->n_members;
    if (n_params) *n_params = p->n_params;
    return RL_OK;
}

// members [first, first + n) of the population, E cars each over scans of `size` beams
static int pop_range(const char *fn, const rl_policy_pop *p, int first, int n)
{
    if (first < 0 || n < 0 || first > p->n_members - n)
        return fail(RL_ERR_INVALID, "%s: members [%d, %d + %d) do not lie in the population's [0, %d)", fn, first, first, n,
                    p->n_members);
    return RL_OK;
}

static int pop_args(const char *fn, const rl_policy_pop *p, int first, int n, int E, int size)
{
    int rc = pop_range(fn, p, first, n);
    if (rc) return rc;
    if (E < 1) return fail(RL_ERR_INVALID, "%s: cars_per_member must be >= 1 (got %d)", fn, E);
    if ((rc = policy_window(p->P, size))) return rc;
    const long cars = (long)n * E;     // (n, E < 2^31: no overflow; then cars < 2^31 before the second product)
    if (cars >= (1L << 31) || cars * std::max(size, 1) >= (1L << 31))
        return fail(RL_ERR_INVALID, "%s: %d members of %d cars, scans of %d beams: their product must stay below 2^31", fn, n,
                    E, size);
    return RL_OK;
}

// before a launch of the handle on st (under its mutex): work a caller left on another stream is waited for
static int pop_enter(rl_policy_pop *p, hipStream_t st)
{
    HIPCHK(hipSetDevice(p->device));
    if (p->foreign && st != p->foreign_st) {
        HIPCHK(hipDeviceSynchronize());
        p->foreign = false;
    }
    if (st != (hipStream_t)p->stream) p->foreign = true, p->foreign_st = st;
    return RL_OK;
}

static int pop_pack_launch(rl_policy_pop *p, int first, int n, const float *d_theta, hipStream_t st)
{
    const size_t total = (size_t)n * p->n_params;
    const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 65536);
    return launch("policy_pop_pack_kernel", policy_pop_pack_kernel, dim3(grid), dim3(256), 0, st, p->L, d_theta, first, n, p->stride,
                  p->weights);
}

extern "C" int rl_policy_pop_set(rl_policy_pop *p, int first, int n, const float *theta_nP)
{
    if (!p || (n > 0 && !theta_nP)) return fail(RL_ERR_INVALID, "rl_policy_pop_set: null pointer");
    int rc = pop_range("rl_policy_pop_set", p, first, n);
    if (rc || n == 0) return rc;
    std::lock_guard<std::mutex> lk(p->mu);
    if ((rc = pop_enter(p, p->stream))) return rc;
    HostCall hc(p->stream);
    if ((rc = hc.up(p->theta, theta_nP, (size_t)n * p->n_params)) || (rc = pop_pack_launch(p, first, n, p->theta, hc.st)))
        return rc;
    return hc.finish();
}

extern "C" int rl_policy_pop_set_device(rl_policy_pop *p, int first, int n, const float *d_theta_nP, void *hip_stream)
{
    if (!p || (n > 0 && !d_theta_nP)) return fail(RL_ERR_INVALID, "rl_policy_pop_set_device: null pointer");
    int rc = pop_range("rl_policy_pop_set_device", p, first, n);
    if (rc || n == 0) return rc;
    std::lock_guard<std::mutex> lk(p->mu);
    if ((rc = pop_enter(p, (hipStream_t)hip_stream))) return rc;
    return pop_pack_launch(p, first, n, d_theta_nP, (hipStream_t)hip_stream);
}

extern "C" int rl_policy_pop_get(rl_policy_pop *p, int member, float *theta_P)
{
    if (!p || !theta_P) return fail(RL_ERR_INVALID, "rl_policy_pop_get: null pointer");
    int rc = pop_range("rl_policy_pop_get", p, member, 1);
    if (rc) return rc;
    std::vector<float> block(p->stride);
    {
        std::lock_guard<std::mutex> lk(p->mu);
        if ((rc = pop_enter(p, p->stream))) return rc;
        HostCall hc(p->stream);
        if ((rc = hc.down(block.data(), (const float *)p->weights + (size_t)member * p->stride, p->stride)) || (rc = hc.finish()))
            return rc;
    }
    // the padded block back into theta's order: W[l] row by row without its padding columns, then b[l]
    for (int l = 0; l < p->L.n_layers; ++l) {
        const int K = p->L.dims[l], N = p->L.dims[l + 1], Np = (N + 3) & ~3;
        float *t = theta_P + p->L.theta_off[l];
        for (int k = 0; k < K; ++k) std::memcpy(t + (size_t)k * N, &block[p->L.w_off[l] + (size_t)k * Np], (size_t)N * sizeof(float));
        std::memcpy(t + (size_t)K * N, &block[p->L.b_off[l]], (size_t)N * sizeof(float));
    }
    return RL_OK;
}

// the population's network launch: scans [n E][size] -> steers [n E], member first + i / E answers row i
static int pop_launch(rl_policy_pop *p, int first, int n, int E, const float *d_scans, int size, float *d_steers, hipStream_t st)
{
    if (n == 0) return RL_OK;
    const int wg = (E + PM_CARS - 1) / PM_CARS;
    return launch("policy_mlp_pop_kernel", policy_mlp_pop_kernel, dim3((unsigned)n * wg), dim3(64), 0, st, p->P, p->stride, first, wg,
                  E, d_scans, size, d_steers);
}

extern "C" int rl_policy_pop_eval(rl_policy_pop *p, int first, int n, int cars_per_member, const float *scans, int size,
                                  float *steers)
{
    if (!p || (n > 0 && (!scans || !steers))) return fail(RL_ERR_INVALID, "rl_policy_pop_eval: null pointer");
    int rc = pop_args("rl_policy_pop_eval", p, first, n, cars_per_member, size);
    if (rc || n == 0) return rc;
    const size_t R = (size_t)n * cars_per_member;
    std::lock_guard<std::mutex> lk(p->mu);
    if ((rc = pop_enter(p, p->stream))) return rc;
    HostCall hc(p->stream);
    if ((rc = hc.up(p->scans, scans, R * size)) || (rc = hc.room(p->steers, R)) ||
        (rc = pop_launch(p, first, n, cars_per_member, p->scans, size, p->steers, hc.st)) || (rc = hc.down(steers, p->steers, R)))
        return rc;
    return hc.finish();
}

extern "C" int rl_policy_pop_eval_device(rl_policy_pop *p, int first, int n, int cars_per_member, const float *d_scans,
                                         int size, float *d_steers, void *hip_stream)
{
    if (!p || (n > 0 && (!d_scans || !d_steers))) return fail(RL_ERR_INVALID, "rl_policy_pop_eval_device: null pointer");
    int rc = pop_args("rl_policy_pop_eval_device", p, first, n, cars_per_member, size);
    if (rc || n == 0) return rc;
    std::lock_guard<std::mutex> lk(p->mu);
    if ((rc = pop_enter(p, (hipStream_t)hip_stream))) return rc;
    return pop_launch(p, first, n, cars_per_member, d_scans, size, d_steers, (hipStream_t)hip_stream);
}

// ---------------------------------------------------------------- league calls (include/scanlib_league.h)
// the workgroups of the league network launch over n rows: the host's upper bound of sum_m ceil(count[m] / PM_CARS)
static size_t league_wg_bound(const rl_policy_pop *p, int n)
{
    return (size_t)(n + PM_CARS - 1) / PM_CARS + (size_t)std::min(n, p->n_members);
}

// the grouping of d_member [n] (n > 0) by member into the handle's buffers: three launches, once per call
static int league_group(rl_policy_pop *p, const int *d_member, int n, hipStream_t st)
{
    const int N = p->n_members;
    int rc;
    if ((rc = p->lg_count.ensure(N)) || (rc = p->lg_start.ensure(N)) || (rc = p->lg_wg_start.ensure(N)) ||
        (rc = p->lg_rows.ensure(n)) || (rc = p->lg_table.ensure(league_wg_bound(p, n))) || (rc = p->lg_total.ensure(1)))
        return rc;
    const dim3 per_member((N + LG_WAVES - 1) / LG_WAVES), waves(64 * LG_WAVES);
    if ((rc = launch("league_count_kernel", league_count_kernel, per_member, waves, 0, st, d_member, n, N, p->lg_count)) ||
        (rc = launch("league_offsets_kernel", league_offsets_kernel, dim3(1), dim3(LG_SCAN), 0, st, p->lg_count, N, p->lg_start,
                     p->lg_wg_start, p->lg_total)))
        return rc;
    return launch("league_fill_kernel", league_fill_kernel, per_member, waves, 0, st, d_member, n, N, p->lg_count, p->lg_start,
                  p->lg_wg_start, p->lg_rows, p->lg_table);
}

// the league's network launch over the grouping of n rows: scans [.][size] -> steers [row] for every grouped row
static int league_launch(rl_policy_pop *p, int n, const float *d_scans, int size, float *d_steers, hipStream_t st)
{
    if (n == 0) return RL_OK;
    return launch("policy_mlp_league_kernel", policy_mlp_league_kernel, dim3((unsigned)league_wg_bound(p, n)), dim3(64), 0, st, p->P,
                  p->stride, p->lg_table, p->lg_total, p->lg_start, p->lg_count, p->lg_rows, d_scans, size, d_steers);
}

static int league_rows_args(const char *fn, const rl_policy_pop *p, int n, int size)
{
    if (n < 0) return fail(RL_ERR_INVALID, "%s: n must be >= 0 (got %d)", fn, n);
    const int rc = policy_window(p->P, size);
    if (rc) return rc;
    if ((long)n * std::max(size, 1) >= (1L << 31))
        return fail(RL_ERR_INVALID, "%s: %d scans of %d beams: their product must stay below 2^31", fn, n, size);
    return RL_OK;
}

// the entry walk of every league call: each of the n entries names a member of the population or a code from `lowest`
// up (-1: FollowGap, or a row left alone; -2, the env: the caller's car).  fg: a -1 entry has a FollowGap handle to ask
// (callers that word this refusal themselves pass true).  speed (the env, else null): the speed of seat i % group, which
// a scripted car of it needs finite.  *n_net: the entries that name a member.
static int league_entries(const char *fn, const int *entry, size_t n, int n_members, int lowest, bool fg,
                          const float *speed = nullptr, int group = 1, size_t *n_net = nullptr)
{
    size_t net = 0;
    for (size_t i = 0; i < n; ++i) {
        const int m = entry[i];
        if (m < lowest || m >= n_members)
            return fail(RL_ERR_INVALID, "%s: entry %zu names member %d: not %s and not in the population's [0, %d)", fn, i, m,
                        lowest < -1 ? "-2, -1" : "-1", n_members);
        if (m == -1 && !fg) return fail(RL_ERR_INVALID, "%s: entry %zu is -1 (FollowGap), whose handle is null", fn, i);
        if (speed && m >= -1 && !std::isfinite(speed[i % group]))
            return fail(RL_ERR_INVALID, "%s: the speed of seat %zu must be finite (entry %zu scripts a car of it)", fn, i % group, i);
        net += m >= 0;
    }
    if (n_net) *n_net = net;
    return RL_OK;
}

extern "C" int rl_policy_pop_eval_rows(rl_policy_pop *p, int n, const int *member_n, const float *scans, int size,
                                       float *steers)
{
    if (!p || (n > 0 && (!member_n || !scans || !steers))) return fail(RL_ERR_INVALID, "rl_policy_pop_eval_rows: null pointer");
    int rc = league_rows_args("rl_policy_pop_eval_rows", p, n, size);
    if (rc || n == 0 || (rc = league_entries("rl_policy_pop_eval_rows", member_n, n, p->n_members, -1, true)))
        return rc;
    std::lock_guard<std::mutex> lk(p->mu);
    if ((rc = pop_enter(p, p->stream))) return rc;
    HostCall hc(p->stream);
    // (the caller's steers go up first: a -1 row comes back with the bits it had)
    if ((rc = hc.up(p->steers, (const float *)steers, n)) || (rc = hc.up(p->lg_member, member_n, n)) ||
        (rc = hc.up(p->scans, scans, (size_t)n * size)) || (rc = league_group(p, p->lg_member, n, hc.st)) ||
        (rc = league_launch(p, n, p->scans, size, p->steers, hc.st)) || (rc = hc.down(steers, p->steers, n)))
        return rc;
    return hc.finish();
}

extern "C" int rl_policy_pop_eval_rows_device(rl_policy_pop *p, int n, const int *d_member_n, const float *d_scans, int size,
                                              float *d_steers, void *hip_stream)
{
    if (!p || (n > 0 && (!d_member_n || !d_scans || !d_steers)))
        return fail(RL_ERR_INVALID, "rl_policy_pop_eval_rows_device: null pointer");
    int rc = league_rows_args("rl_policy_pop_eval_rows_device", p, n, size);
    if (rc || n == 0) return rc;
    std::lock_guard<std::mutex> lk(p->mu);
    if ((rc = pop_enter(p, (hipStream_t)hip_stream)) || (rc = league_group(p, d_member_n, n, (hipStream_t)hip_stream))) return rc;
    return league_launch(p, n, d_scans, size, d_steers, (hipStream_t)hip_stream);
}

// ---------------------------------------------------------------- the closed-loop session
// What the closed loops share on the host.  The roll-outs (drive_loop), the driving environment (rl_env_*) and the MCTS
// planner (rl_mcts_*) check their handles with loop_args, and each of their launching calls lives inside one Loop: its
// locks, what it tells its launches, and the scan-then-consume step every one of them is made of.

// the handle checks of every closed loop: `units` cars / envs / poses scan num_rays beams each; the steering source is
// g, p or neither (the environment, the planner's random source)
static int loop_args(const char *name, const rl_car *c, const rl_method *h, const rl_followgap *g, const rl_policy *p,
                     long units, int num_rays)
{
    if (!c->reps.empty() || !h->reps.empty())
        return fail(RL_ERR_INVALID, "%s is single-device only: pass ordinary (not multi-device) handles", name);
    const int src_device = g ? g->device : p ? p->device : c->device;
    if (c->device != h->map->device || src_device != c->device) {
        char src[48] = "";
        if (g || p) snprintf(src, sizeof src, " and %s (device %d)", g ? "FollowGap" : "policy", src_device);
        return fail(RL_ERR_INVALID, "%s: car (device %d)%s range method (device %d)%s must share one device", name, c->device,
                    g || p ? "," : " and", h->map->device, src);
    }
    if (num_rays < 10 || num_rays > 64 * FG_ROWS)
        return fail(RL_ERR_INVALID, "num_rays must lie in [10, %d] (got %d)", 64 * FG_ROWS, num_rays);
    if (units * num_rays >= (1L << 31))
        return fail(RL_ERR_INVALID, "%s: %ld scans of %d beams: their product must stay below 2^31", name, units, num_rays);
    return RL_OK;
}

// Who answers the scans of a closed loop, the handles it borrows and the one launch it puts between a scan and its
// consumer.  Loop locks the handles a source NAMES: g in FollowGap's slot, then p or pop in the network's.  Per kind:
//   NOBODY      the plain and the race env, the planner's random source: no handle, no lock, no launch
//   FOLLOWGAP   g, locked; no launch (the consumer kernel holds FollowGap)
//   POLICY      p, locked; its network over every scan
//   SEATS       `net` over the rows of the cars in the `policy_seats` of every race of `group` (the list: *rows).  A
//               roll-out (rl_car_race_seats) names g and p, each only where a seat uses it, and both are locked.  A race
//               env (rl_env_attach_seats) names NEITHER and so takes neither mutex: it copied FollowGap's parameters at
//               the attach and borrows the policy's weights through `net` alone
//   POPULATION  pop, locked; members [first, first + n) over E scans each
//   LEAGUE      pop over the grouping of the call's entries (league_group has run on it), locked, and g where an entry
//               may be -1, locked: the roll-out (rl_car_race_league; `entry`: its host table) and the race env
//               (rl_env_attach_league) both take both.  n_net: the scans to give the network, 0 for no launch
struct SteerSource {
    enum Kind { NOBODY, FOLLOWGAP, POLICY, SEATS, POPULATION, LEAGUE };
    Kind kind = NOBODY;
    rl_followgap *g = nullptr;
    rl_policy *p = nullptr;
    rl_policy_pop *pop = nullptr;
    const PolicyParams *net = nullptr;
    uint32_t policy_seats = 0;
    int group = 0;
    const DevPtr<int> *rows = nullptr;
    int first = 0, n = 0, E = 0;
    const int *entry = nullptr;
    int n_net = 0;

    static SteerSource followgap(rl_followgap *g) { return {FOLLOWGAP, g}; }
    static SteerSource policy(rl_policy *p) { return {POLICY, nullptr, p}; }
    static SteerSource seats(rl_followgap *g, rl_policy *p, const PolicyParams *net, uint32_t policy_seats, int group,
                             const DevPtr<int> *rows)
    {
        return {SEATS, g, p, nullptr, policy_seats ? net : nullptr, policy_seats, group, rows};
    }
    static SteerSource population(rl_policy_pop *pop, int first, int n, int E)
    {
        SteerSource s{POPULATION, nullptr, nullptr, pop};
        s.first = first, s.n = n, s.E = E;
        return s;
    }
    static SteerSource league(rl_followgap *g, rl_policy_pop *pop, const int *entry, int n_net)
    {
        SteerSource s{LEAGUE, g, nullptr, pop};
        s.entry = entry, s.n_net = n_net;
        return s;
    }
    bool empty() const { return !g && !p && !pop; }

    // loop_args for the handles named: FollowGap's device first, then the policy's
    int check(const char *name, const rl_car *c, const rl_method *h, long units, int num_rays) const
    {
        int rc = loop_args(name, c, h, g, g ? nullptr : p, units, num_rays);
        if (rc == RL_OK && g && p) rc = loop_args(name, c, h, nullptr, p, units, num_rays);
        return rc;
    }
    // the population's device, and the policy's window in n_scans scans of num_rays beams (a population's window is its
    // entry point's to check: pop_args, rl_car_race_league)
    int fits(const char *name, const rl_car *c, int n_scans, int num_rays) const
    {
        if (pop && pop->device != c->device)
            return fail(RL_ERR_INVALID, "%s: car (device %d) and population (device %d) must share one device", name, c->device,
                        pop->device);
        return p ? policy_args(p, n_scans, num_rays) : (int)RL_OK;
    }
    // the network's answers to the n scans in `ranges`, into mlp [n] (SEATS, LEAGUE: the rows it drives and no others)
    int answer(const float *ranges, int n_scans, int num_rays, float *mlp, hipStream_t st) const
    {
        switch (kind) {
        case POLICY: return policy_launch(p, ranges, n_scans, num_rays, mlp, st);
        case SEATS:
            if (!net) return RL_OK;
            return policy_rows_launch(*net, ranges, *rows, n_scans / group * __builtin_popcount(policy_seats), num_rays, mlp, st);
        case POPULATION: return pop_launch(pop, first, n, E, ranges, num_rays, mlp, st);
        case LEAGUE: return league_launch(pop, n_net ? n_scans : 0, ranges, num_rays, mlp, st);
        default: return RL_OK;
        }
    }
};

// one scan of a closed loop: n poses (a race: n / group races over the cars' f64 states, 11 doubles a car) into `ranges`;
// mlp: where the loop's source puts its answers
struct LoopScan {
    const float *poses;
    int n;
    float fov;
    int num_rays;
    float *ranges, *mlp;
    int group;                      // 0: every pose scans alone with the method's planner
    const double *cars;
    const OutlineParams *outline;
};

// One launching call of a closed loop.  Locks in ONE order: the owner's mutex (rl_env::mu, rl_mcts::mu; none for the
// roll-outs), the car's, the method's, the source's (FollowGap's, then the policy's or the population's: SteerSource
// says which a kind names), then the map's tables_mu shared.  The method's
// settings are read under its mutex and never written: `base` is the noise offset the loop walks from, and every launch
// is told its own offset and plain stores (the consumer kernels read the ranges right after the scan).  `ready` of an
// owner is read and written inside only.
struct Loop {
    rl_method *const h;
    const SteerSource src;
    std::unique_lock<std::mutex> lo, lc, lh, ls, ln;
    std::shared_lock<std::shared_mutex> ml;
    const uint64_t base;
    static std::unique_lock<std::mutex> held(std::mutex *m) { return m ? std::unique_lock(*m) : std::unique_lock<std::mutex>(); }
    Loop(std::mutex *owner, rl_car *c, rl_method *h_, const SteerSource &s)
        : h(h_), src(s), lo(held(owner)), lc(c->mu), lh(h_->mu), ls(held(s.g ? &s.g->mu : nullptr)),
          ln(held(s.p ? &s.p->mu : s.pop ? &s.pop->mu : nullptr)), ml(h_->map->tables_mu), base(h_->ray_offset)
    {
    }
    LaunchArgs at(uint64_t off) const { return {off, true, h->timing}; }

    // scan-then-consume on st: the scan at noise offset `off`, the source's answers, then the ROWS instantiation of
    // `table` for num_rays, one wave per unit and per_wg units per workgroup
    template <class Fn, class... Args>
    int scan_then(const LoopScan &s, uint64_t off, const std::array<Fn, FG_ROWS> &table, int per_wg, const char *kernel,
                  hipStream_t st, const Args &...args) const
    {
        const LaunchArgs a = at(off);
        int rc = s.group > 0 ? launch_race(h, a, s.poses, s.cars, 11, s.n / s.group, s.group, *s.outline, s.fov, s.num_rays,
                                           s.ranges, nullptr, nullptr, st)
                             : launch_fan(h, FanCall{a, s.poses, s.n, s.fov, s.num_rays, s.ranges, nullptr, nullptr, nullptr, st});
        if (rc || (rc = src.answer(s.ranges, s.n, s.num_rays, s.mlp, st))) return rc;
        return launch(kernel, table[(s.num_rays + 63) / 64 - 1], dim3((s.n + per_wg - 1) / per_wg), dim3(64 * per_wg), 0, st, args...);
    }
};

// one seat's driver code: FollowGap or the policy, whose handle must be there (the caller's code is the caller's to sort out)
static int seat_code(const char *fn, int k, int d, const rl_followgap *g, const rl_policy *p)
{
    if (d != RL_SEAT_FOLLOWGAP && d != RL_SEAT_POLICY) return fail(RL_ERR_INVALID, "%s: seat %d: unknown driver code %d", fn, k, d);
    const bool net = d == RL_SEAT_POLICY;
    if (!(net ? (const void *)p : (const void *)g))
        return fail(RL_ERR_INVALID, "%s: seat %d is driven by %s, whose handle is null", fn, k, net ? "the policy" : "FollowGap");
    return RL_OK;
}

// the cars in the seats of `mask`, race by race: what SteerSource::rows holds on the device
static std::vector<int> seat_row_list(uint32_t mask, int n_races, int group)
{
    std::vector<int> rows;
    for (int r = 0; r < n_races && mask; ++r)
        for (int k = 0; k < group; ++k)
            if ((mask >> k) & 1u) rows.push_back(r * group + k);
    return rows;
}

// ---------------------------------------------------------------- closed-loop roll-outs (drive_kernels.h)
typedef void (*drive_tick_fn)(DriveParams, DriveBufs, int);
static const std::array<drive_tick_fn, FG_ROWS> fg_tick_table =
    rows_table<drive_tick_fn>([](auto rows) { return drive_tick_kernel<rows, FollowGapSteer>; });
static const std::array<drive_tick_fn, FG_ROWS> policy_tick_table =
    rows_table<drive_tick_fn>([](auto rows) { return drive_tick_kernel<rows, PolicySteer>; });
static const std::array<drive_tick_fn, FG_ROWS> seat_tick_table =
    rows_table<drive_tick_fn>([](auto rows) { return drive_tick_kernel<rows, SeatSteer>; });
static const std::array<drive_tick_fn, FG_ROWS> league_tick_table =
    rows_table<drive_tick_fn>([](auto rows) { return drive_tick_kernel<rows, LeagueSteer>; });

static TrackTable track_table(const rl_track *t);

// what the roll-out entry points share of their arguments (include/scanlib.h names them)
struct DriveCall {
    const double *states_in, *speeds;
    const float *steer0;
    int n_ticks;
    double dt, scan_dist_to_base;
    float fov;
    int num_rays;
    const double *edge;
    double crash_thresh;
    int *first_crashed;
    double *states_out, *velocities;
    float *steers, *scan_poses;
    double *states_trace;
};

// n cars for n_ticks ticks, steered by src (steer_clip: the networks'), each scanning alone with h's planner; race: n
// races of `group` cars, which see each other in every scan (race_fan_kernel).  The tick kernel, what it is told of seats
// and entries, and the uploads a source needs before the first tick all follow from src.kind.  A POPULATION has
// n = src.n src.E cars, car r steered by member src.first + r / src.E; a LEAGUE (a race only) steers car r by member
// src.entry[r] of src.pop, or by src.g when that is -1.  scores: after the last tick a population's fitness [src.n][2] or
// a league's standings [n_members][4], or null.  With a track attached to c (include/scanlib_track_drive.h) the cars are
// placed on it: once on the start states, ahead of every tick's scan, and ranked and scored after the last tick; the
// launches of a handle without a track are the ones below and no others
static int drive_loop(const char *name, rl_car *c, rl_method *h, const SteerSource &src, double steer_clip, int n, bool race,
                      int group, const DriveCall &a, double *scores = nullptr)
{
    if (!c || !h || src.empty() || (n > 0 && (!a.states_in || !a.speeds || !a.edge || !a.first_crashed)))
        return fail(RL_ERR_INVALID, "%s: null pointer", name);
    const int n_ticks = a.n_ticks, num_rays = a.num_rays;
    int rc;
    if (race && n < 0) return fail(RL_ERR_INVALID, "n_races must be >= 0 (got %d)", n);
    if (race && (rc = race_args(h, n, group, num_rays))) return rc;
    const int R = race ? n * group : n;          // (a race: < 2^31 / num_rays, race_args)
    if ((rc = src.check(name, c, h, R, num_rays))) return rc;
    if (R < 0 || n_ticks <= 0) return fail(RL_ERR_INVALID, "n_rollouts >= 0 and n_ticks > 0 required (got %d, %d)", R, n_ticks);
    if ((rc = src.fits(name, c, R, num_rays)) || (rc = check_fan_args(h, R, a.fov, num_rays)) || R == 0) return rc;
    OutlineParams op{};
    if (race && (rc = race_outline(h->map, c->P.LENGTH, c->P.WIDTH, op))) return rc;
    const Loop lp(nullptr, c, h, src);
    HIPCHK(hipSetDevice(c->device));
    rl_policy_pop *const pop = src.pop;
    if (pop && (rc = pop_enter(pop, c->stream))) return rc;
    const bool net = src.p || pop;     // the tick reads the network's answers
    const bool seats = src.kind == SteerSource::SEATS, league = src.kind == SteerSource::LEAGUE;
    const size_t rows = (size_t)R * n_ticks, n_rays = (size_t)R * num_rays;
    // seats: the cars the network drives (declared before hc: the list outlives the call's copies)
    const std::vector<int> seat_rows = seat_row_list(src.policy_seats, n, group);
    HostCall hc(c->stream);
    hipStream_t st = hc.st;
    if (!seat_rows.empty() && (rc = hc.up(c->seat_rows, seat_rows.data(), seat_rows.size()))) return rc;
    // trace rows a car never reaches (after its crash tick; the steer of the crash tick) read NaN: all-ones bytes
    if ((rc = hc.up(c->states, a.states_in, (size_t)R * 11)) || (rc = hc.up(c->speeds, a.speeds, R)) ||
        (rc = a.steer0 ? hc.up(c->steer0, a.steer0, R) : hc.zero(c->steer0, R)) || (rc = hc.up(c->edge, a.edge, num_rays)) ||
        (rc = hc.room(c->first, R)) || (rc = hc.room(c->poses, (size_t)R * 3)) || (rc = hc.room(c->ranges, n_rays)) ||
        (net && (rc = hc.room(c->mlp, R))) || (a.velocities && (rc = hc.fill(c->vel, 0xff, rows))) ||
        (a.steers && (rc = hc.fill(c->tr_steers, 0xff, rows))) || (a.scan_poses && (rc = hc.fill(c->tr_poses, 0xff, rows * 3))) ||
        (a.states_trace && (rc = hc.fill(c->tr_states, 0xff, rows * 11))))
        return rc;
    // a league: the entries go up and are grouped by member once, before the first tick
    if (league && ((rc = hc.up(pop->lg_member, src.entry, R)) || (rc = league_group(pop, pop->lg_member, R, st)))) return rc;
    // the scores read the starts again after the last tick: c->states is stepped in place
    const size_t n_scores = !scores ? 0 : league ? 4 * (size_t)pop->n_members : 2 * (size_t)src.n;
    if (n_scores && ((rc = hc.up(c->pop_states0, a.states_in, (size_t)R * 11)) || (rc = hc.room(c->pop_fitness, n_scores))))
        return rc;
    // a track: the fresh placement reads the start states before drive_start_kernel steps them in place
    const rl_track *const trk = c->track;
    const TrackTable tt = trk ? track_table(trk) : TrackTable{};
    const dim3 track_grid((R + DRIVE_CARS - 1) / DRIVE_CARS), track_block(64 * DRIVE_CARS);
    if (trk) {
        c->dt_cars = c->dt_score_rows = c->dt_score_cols = 0;      // (a call that fails leaves nothing to read)
        if ((rc = hc.room(c->dt_rows, (size_t)R * 4)) || (rc = hc.room(c->dt_ints, (size_t)R * 4))) return rc;
        if ((rc = launch("drive_track_kernel", drive_track_kernel<true>, track_grid, track_block, 0, st, R, tt, c->dt_window,
                         c->dt_goal, DriveTrackBufs{c->dt_rows, c->dt_ints}, c->states, nullptr, 0)))
            return rc;
    }
    const DriveTrackBufs tb{c->dt_rows, c->dt_ints};

    DriveParams dp{};
    dp.P = c->P;
    if (src.g) dp.fg = src.g->P;
    dp.fg.size = num_rays;                        // (for the policy only the crash ballot's beam count)
    dp.dt = a.dt;
    dp.scan_dist_to_base = a.scan_dist_to_base;
    dp.crash_thresh = a.crash_thresh;
    dp.n_cars = R;
    dp.n_ticks = n_ticks;
    dp.steer_clip = steer_clip;
    dp.group = seats ? group : 0;                 // (a league asks the car's entry, not its seat)
    dp.policy_seats = src.policy_seats;
    DriveBufs b{c->states, c->speeds, c->steer0, c->edge, c->first, c->poses, c->ranges,
                a.velocities ? (double *)c->vel : nullptr, a.steers ? (float *)c->tr_steers : nullptr,
                a.scan_poses ? (float *)c->tr_poses : nullptr, a.states_trace ? (double *)c->tr_states : nullptr,
                net ? (const float *)c->mlp : nullptr, league ? (const int *)pop->lg_member : nullptr};
    if ((rc = launch("drive_start_kernel", drive_start_kernel, dim3((R + 63) / 64), dim3(64), 0, st, dp, b))) return rc;
    // the noise offset walks the global ray id t R num_rays + r num_rays of every tick
    // (a race reads every car's outline from its f64 state after this tick's step: all cars step, then all scan)
    const LoopScan scan{b.pose, R, a.fov, num_rays, c->ranges, c->mlp, race ? group : 0, b.state, &op};
    const auto &table = league ? league_tick_table : seats ? seat_tick_table : src.g ? fg_tick_table : policy_tick_table;
    for (int t = 0; t < n_ticks && rc == RL_OK; ++t) {
        // (a track: the cars still running hold the state after tick t's step)
        if (trk && (rc = launch("drive_track_kernel", drive_track_kernel<false>, track_grid, track_block, 0, st, R, tt, c->dt_window,
                                c->dt_goal, tb, c->states, c->first, t)))
            break;
        rc = lp.scan_then(scan, lp.base + (uint64_t)t * n_rays, table, DRIVE_CARS, "drive_tick_kernel", st, dp, b, t);
    }
    if (rc == RL_OK && n_scores) {
        rc = league ? launch("league_standings_kernel", league_standings_kernel, dim3((pop->n_members + 63) / 64), dim3(64), 0, st,
                             c->states, c->pop_states0, c->first, pop->lg_start, pop->lg_count, pop->lg_rows, pop->n_members, group,
                             n_ticks, c->pop_fitness)
                    : launch("policy_pop_fitness_kernel", policy_pop_fitness_kernel, dim3((src.n + 63) / 64), dim3(64), 0, st,
                             c->states, c->pop_states0, c->first, src.n, src.E, c->pop_fitness);
        if (rc == RL_OK) rc = hc.down(scores, c->pop_fitness, n_scores);
    }
    // a track: ranks per race, then the population's or the league's track scores (whether or not `scores` was asked for)
    int score_rows = 0, score_cols = 0;
    if (rc == RL_OK && trk) {
        if (league) score_rows = pop->n_members, score_cols = 4;
        else if (src.kind == SteerSource::POPULATION) score_rows = src.n, score_cols = 3;
        if ((rc = launch("drive_track_rank_kernel", drive_track_rank_kernel, dim3((R + 63) / 64), dim3(64), 0, st, R,
                         race ? group : 0, tt, tb)) ||
            (score_rows && (rc = hc.room(c->dt_scores, (size_t)score_rows * score_cols))))
            return rc;
        if (league)
            rc = launch("drive_track_standings_kernel", drive_track_standings_kernel, dim3((score_rows + 63) / 64), dim3(64), 0, st,
                        tb, pop->lg_start, pop->lg_count, pop->lg_rows, score_rows, group, c->dt_scores);
        else if (score_rows)
            rc = launch("drive_track_fitness_kernel", drive_track_fitness_kernel, dim3((score_rows + 63) / 64), dim3(64), 0, st, tb,
                        src.n, src.E, c->dt_scores);
    }
    if (rc || (rc = hc.down(a.first_crashed, c->first, R)) || (rc = hc.down(a.states_out, c->states, (size_t)R * 11)) ||
        (rc = hc.down(a.velocities, c->vel, rows)) || (rc = hc.down(a.steers, c->tr_steers, rows)) ||
        (rc = hc.down(a.scan_poses, c->tr_poses, rows * 3)) || (rc = hc.down(a.states_trace, c->tr_states, rows * 11)))
        return rc;
    if ((rc = hc.finish())) return rc;
    if (trk) c->dt_cars = R, c->dt_score_rows = score_rows, c->dt_score_cols = score_cols;
    return RL_OK;
}

extern "C" int rl_car_drive_followgap(rl_car *c, rl_method *h, rl_followgap *g, const double *states_in,
                                      const double *speeds, const float *steer0_or_null, int R, int n_ticks, double dt,
                                      double scan_dist_to_base, float fov, int num_rays, const double *edge,
                                      double crash_thresh, int *first_crashed, double *states_out_or_null,
                                      double *velocities_or_null, float *steers_or_null, float *scan_poses_or_null,
                                      double *states_trace_or_null)
{
    const DriveCall a{states_in, speeds, steer0_or_null, n_ticks, dt, scan_dist_to_base, fov, num_rays, edge, crash_thresh,
                      first_crashed, states_out_or_null, velocities_or_null, steers_or_null, scan_poses_or_null,
                      states_trace_or_null};
    return drive_loop("rl_car_drive_followgap", c, h, SteerSource::followgap(g), 0.0, R, false, 0, a);
}

extern "C" int rl_car_race_followgap(rl_car *c, rl_method *h, rl_followgap *g, const double *states_in,
                                     const double *speeds, const float *steer0_or_null, int n_races, int group,
                                     int n_ticks, double dt, double scan_dist_to_base, float fov, int num_rays,
                                     const double *edge, double crash_thresh, int *first_crashed,
                                     double *states_out_or_null, double *velocities_or_null, float *steers_or_null,
                                     float *scan_poses_or_null, double *states_trace_or_null)
{
    const DriveCall a{states_in, speeds, steer0_or_null, n_ticks, dt, scan_dist_to_base, fov, num_rays, edge, crash_thresh,
                      first_crashed, states_out_or_null, velocities_or_null, steers_or_null, scan_poses_or_null,
                      states_trace_or_null};
    return drive_loop("rl_car_race_followgap", c, h, SteerSource::followgap(g), 0.0, n_races, true, group, a);
}

extern "C" int rl_car_drive_policy(rl_car *c, rl_method *h, rl_policy *p, const double *states_in,
                                   const double *speeds, const float *steer0_or_null, int R, int n_ticks, double dt,
                                   double scan_dist_to_base, float fov, int num_rays, const double *edge,
                                   double crash_thresh, double steer_clip, int *first_crashed,
                                   double *states_out_or_null, double *velocities_or_null, float *steers_or_null,
                                   float *scan_poses_or_null, double *states_trace_or_null)
{
    const DriveCall a{states_in, speeds, steer0_or_null, n_ticks, dt, scan_dist_to_base, fov, num_rays, edge, crash_thresh,
                      first_crashed, states_out_or_null, velocities_or_null, steers_or_null, scan_poses_or_null,
                      states_trace_or_null};
    return drive_loop("rl_car_drive_policy", c, h, SteerSource::policy(p), steer_clip, R, false, 0, a);
}

extern "C" int rl_car_drive_population(rl_car *c, rl_method *h, rl_policy_pop *pop, int first, int n, int cars_per_member,
                                       double steer_clip, const double *states_in, const double *speeds,
                                       const float *steer0_or_null, int n_ticks, double dt, double scan_dist_to_base,
                                       float fov, int num_rays, const double *edge, double crash_thresh, int *first_crashed,
                                       double *states_out_or_null, double *velocities_or_null, float *steers_or_null,
                                       float *scan_poses_or_null, double *states_trace_or_null, double *fitness_n2_or_null)
{
    if (!c || !h || !pop) return fail(RL_ERR_INVALID, "rl_car_drive_population: null pointer");
    // (R = n E must be a number of cars before the loop's checks read it)
    const int rc = pop_args("rl_car_drive_population", pop, first, n, cars_per_member, num_rays);
    if (rc) return rc;
    const DriveCall a{states_in, speeds, steer0_or_null, n_ticks, dt, scan_dist_to_base, fov, num_rays, edge, crash_thresh,
                      first_crashed, states_out_or_null, velocities_or_null, steers_or_null, scan_poses_or_null,
                      states_trace_or_null};
    return drive_loop("rl_car_drive_population", c, h, SteerSource::population(pop, first, n, cars_per_member), steer_clip,
                      n * cars_per_member, false, 0, a, fitness_n2_or_null);
}

extern "C" int rl_car_race_seats(rl_car *c, rl_method *h, rl_followgap *g_or_null, rl_policy *p_or_null,
                                 const int *seat_driver, double steer_clip, const double *states_in, const double *speeds,
                                 const float *steer0_or_null, int n_races, int group, int n_ticks, double dt,
                                 double scan_dist_to_base, float fov, int num_rays, const double *edge, double crash_thresh,
                                 int *first_crashed, double *states_out_or_null, double *velocities_or_null,
                                 float *steers_or_null, float *scan_poses_or_null, double *states_trace_or_null)
{
    if (!c || !h || !seat_driver) return fail(RL_ERR_INVALID, "rl_car_race_seats: null pointer");
    int rc = race_group(group);
    if (rc) return rc;
    bool fg = false;
    uint32_t policy_seats = 0;
    for (int k = 0; k < group; ++k) {
        const int d = seat_driver[k];
        if (d == RL_SEAT_CALLER)
            return fail(RL_ERR_INVALID, "rl_car_race_seats: seat %d is the caller's: a roll-out has no caller to ask", k);
        if ((rc = seat_code("rl_car_race_seats", k, d, g_or_null, p_or_null))) return rc;
        if (d == RL_SEAT_POLICY) policy_seats |= 1u << k;
        else fg = true;
    }
    const DriveCall a{states_in, speeds, steer0_or_null, n_ticks, dt, scan_dist_to_base, fov, num_rays, edge, crash_thresh,
                      first_crashed, states_out_or_null, velocities_or_null, steers_or_null, scan_poses_or_null,
                      states_trace_or_null};
    // (a handle no seat uses is not looked at)
    rl_policy *const p = policy_seats ? p_or_null : nullptr;
    const SteerSource src = SteerSource::seats(fg ? g_or_null : nullptr, p, p ? &p->P : nullptr, policy_seats, group, &c->seat_rows);
    return drive_loop("rl_car_race_seats", c, h, src, steer_clip, n_races, true, group, a);
}

extern "C" int rl_car_race_league(rl_car *c, rl_method *h, rl_followgap *g_or_null, rl_policy_pop *pop, const int *entry_RP,
                                  double steer_clip, const double *states_in, const double *speeds,
                                  const float *steer0_or_null, int n_races, int group, int n_ticks, double dt,
                                  double scan_dist_to_base, float fov, int num_rays, const double *edge, double crash_thresh,
                                  int *first_crashed, double *states_out_or_null, double *velocities_or_null,
                                  float *steers_or_null, float *scan_poses_or_null, double *states_trace_or_null,
                                  double *standings_N4_or_null)
{
    if (!c || !h || !pop || (n_races > 0 && !entry_RP)) return fail(RL_ERR_INVALID, "rl_car_race_league: null pointer");
    int rc = race_group(group);
    if (rc) return rc;
    if (n_races < 0) return fail(RL_ERR_INVALID, "n_races must be >= 0 (got %d)", n_races);
    // (n_races group must be a number of cars before the entries are walked: the race scan's own bound, here first)
    if ((long)n_races * group * std::max(num_rays, 1) >= (1L << 31))
        return fail(RL_ERR_INVALID, "rl_car_race_league: %d races of %d cars, scans of %d beams: their product must stay below 2^31",
                    n_races, group, num_rays);
    const size_t R = (size_t)n_races * group;
    size_t n_net = 0;
    if ((rc = league_entries("rl_car_race_league", entry_RP, R, pop->n_members, -1, true, nullptr, 1, &n_net))) return rc;
    if (n_net < R && !g_or_null)
        return fail(RL_ERR_INVALID, "rl_car_race_league: an entry is -1 (FollowGap), whose handle is null");
    if (n_net && (rc = policy_window(pop->P, num_rays))) return rc;
    const DriveCall a{states_in, speeds, steer0_or_null, n_ticks, dt, scan_dist_to_base, fov, num_rays, edge, crash_thresh,
                      first_crashed, states_out_or_null, velocities_or_null, steers_or_null, scan_poses_or_null,
                      states_trace_or_null};
    // (a FollowGap handle no entry uses is not looked at)
    const SteerSource src = SteerSource::league(n_net < R ? g_or_null : nullptr, pop, entry_RP, (int)n_net);
    return drive_loop("rl_car_race_league", c, h, src, steer_clip, n_races, true, group, a, standings_N4_or_null);
}

// ---------------------------------------------------------------- the driving environment (env_kernels.h)
typedef void (*env_observe_fn)(EnvParams, EnvBufs, float *, float *, int *, float *);
static const std::array<env_observe_fn, FG_ROWS> env_observe_table =
    rows_table<env_observe_fn>([](auto rows) { return env_observe_kernel<rows>; });
typedef void (*race_env_observe_fn)(EnvParams, EnvBufs, RaceEnvBufs, float *, float *, int *, float *);
static const std::array<race_env_observe_fn, FG_ROWS> race_env_observe_table =
    rows_table<race_env_observe_fn>([](auto rows) { return race_env_observe_kernel<rows>; });
typedef void (*race_env_seat_observe_fn)(EnvParams, EnvBufs, RaceEnvBufs, SeatBufs, float *, float *, int *, float *);
static const std::array<race_env_seat_observe_fn, FG_ROWS> race_env_seat_observe_table =
    rows_table<race_env_seat_observe_fn>([](auto rows) { return race_env_seat_observe_kernel<rows>; });
typedef void (*race_env_league_observe_fn)(EnvParams, EnvBufs, RaceEnvBufs, LeagueEnvBufs, float *, float *, int *, float *);
static const std::array<race_env_league_observe_fn, FG_ROWS> race_env_league_observe_table =
    rows_table<race_env_league_observe_fn>([](auto rows) { return race_env_league_observe_kernel<rows>; });

// a track (rl_track_create): the table of track_kernels.h in one device block, and the host's copy of cum
struct rl_track {
    int device = 0, W = 0, S = 0, closed = 0;
    DevPtr<double> table;          // x, y [W]; dx, dy, q, len [S]; cum [S + 1]
    std::vector<double> cum;       // [S + 1]; L = cum[S]
};

struct rl_env {
    rl_car *c = nullptr;
    rl_method *h = nullptr;
    rl_env_params prm{};
    EnvParams ep{};
    int device = 0, n_starts = 0;
    DevPtr<double> state, starts, edge, moved;
    DevPtr<int> tick, episode, start_index, done, phase;
    DevPtr<float> pose, ranges;
    // a race env (rl_env_create_race): group > 0, the races' counters [n_envs / group] and the cars' outline
    int group = 0, min_running = 0;
    DevPtr<int> race_tick, race_episode, race_start_index, race_over;
    OutlineParams outline{};
    // the host forms' staging: actions and start indices in, observation, reward, done and aux out
    DevPtr<float> h_actions, h_obs, h_reward, h_aux;
    DevPtr<int> h_sidx, h_done;
    // track progress (rl_env_attach_track): the borrowed track, its options and the per-env rows
    rl_track *track = nullptr;
    TrackParams tp{};
    DevPtr<double> track_st;
    DevPtr<float> track_rows;
    DevPtr<int> track_ints;
    // who drives the cars: src.kind is the env's driver mode.  NOBODY: the caller drives every car.  SEATS
    // (rl_env_attach_seats) or LEAGUE (rl_env_attach_league): the source with its borrowed handles, and the network's
    // answers of a call and the kept answers, N floats each, which the mode's kernel table points into
    SteerSource src;
    DevPtr<float> mlp, answer;
    // per-seat drivers: the kernels' table and the cars in policy seats
    SeatBufs seats{};
    DevPtr<int> seat_rows;
    // league line-ups: the kernels' table (the pending and live entries, the results, the host's copy of the seat
    // speeds).  src.n_net > 0: a pending or live entry may name a member (a host-set table since the attach held one, or
    // a device setter ran) and the scans hold the network's window: the network launch is made
    LeagueEnvBufs lg{};
    DevPtr<int> lg_pending, lg_live;
    DevPtr<unsigned long long> lg_results;
    bool ready = false;            // reset done and no launch failed since (read and written under mu only)
    bool foreign = false;          // the last launches went to a caller's stream: a host form waits for the device first
    uint64_t k = 0;                // calls since the last reset (the reset is slot 0)
    uint64_t base = 0;             // h's ray offset at the last reset
    std::mutex mu;
};

static EnvBufs env_bufs(rl_env *e)
{
    return EnvBufs{e->state, e->starts, e->edge, e->tick, e->episode, e->start_index, e->done, e->phase, e->moved, e->pose,
                   e->ranges};
}

static RaceEnvBufs race_env_bufs(rl_env *e)
{
    return RaceEnvBufs{e->group, e->min_running, e->race_tick, e->race_episode, e->race_start_index, e->race_over};
}

// The Loop of a launching call of env e: the env's mutex first (its source is read under it), then Loop's order.
struct EnvLoop {
    std::unique_lock<std::mutex> own;
    const Loop lp;
    explicit EnvLoop(rl_env *e) : own(e->mu), lp(nullptr, e->c, e->h, e->src) {}
};

// the scan's own refusals, checked before every launching call: a race env adds those of rl_calc_range_fan_cars
static int env_scan_args(rl_env *e)
{
    int rc = check_fan_args(e->h, e->prm.n_envs, e->prm.fov, e->prm.num_rays);
    if (rc == RL_OK && e->group > 0) rc = race_args(e->h, e->prm.n_envs / e->group, e->group, e->prm.num_rays);
    return rc;
}

extern "C" void rl_env_destroy(rl_env *e)
{
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->foreign) (void)hipDeviceSynchronize();
    else if (e->c && e->c->stream) (void)hipStreamSynchronize(e->c->stream);
    delete e;
}

// rl_env_create (group = 0) and rl_env_create_race (group = P >= 1: the pool holds n_starts line-ups of P rows)
static int env_create(rl_car *c, rl_method *h, const rl_env_params *params, const double *edge, const double *starts_m11,
                      int n_starts, int group, int min_running, rl_env **out)
{
    if (!c || !h || !params || !edge || !starts_m11 || !out) return fail(RL_ERR_INVALID, "rl_env_create: null pointer");
    const rl_env_params q = *params;
    const int per = group > 0 ? group : 1;      // pool rows per start
    int rc = loop_args("rl_env_create", c, h, nullptr, nullptr, q.n_envs, q.num_rays);
    if (rc) return rc;
    if (q.n_envs < 1) return fail(RL_ERR_INVALID, "rl_env_create: n_envs must be >= 1 (got %d)", q.n_envs);
    if (q.substeps < 1 || q.substeps > 512)
        return fail(RL_ERR_INVALID, "rl_env_create: substeps must lie in [1, 512] (got %d)", q.substeps);
    if (q.obs_count < 1 || q.obs_stride < 1 || q.obs_start < 0 ||
        (long)q.obs_start + ((long)q.obs_count - 1) * q.obs_stride >= q.num_rays)
        return fail(RL_ERR_INVALID, "rl_env_create: the observation window (start %d, count %d, stride %d) must lie in "
                    "[0, %d) with count and stride >= 1", q.obs_start, q.obs_count, q.obs_stride, q.num_rays);
    if (!(q.steer_clip >= 0.0) || !(q.obs_clip >= 0.0f) || !(q.obs_scale >= 0.0f))
        return fail(RL_ERR_INVALID, "rl_env_create: steer_clip, obs_clip and obs_scale must be >= 0 and not NaN");
    if (q.crash_reward != q.crash_reward || !std::isfinite(q.dt))
        return fail(RL_ERR_INVALID, "rl_env_create: crash_reward must not be NaN and dt must be finite");
    if (q.max_ticks < 0) return fail(RL_ERR_INVALID, "rl_env_create: max_ticks must be >= 0 (got %d)", q.max_ticks);
    if (n_starts < 1) return fail(RL_ERR_INVALID, "rl_env_create: n_starts must be >= 1 (got %d)", n_starts);
    if (n_starts > INT_MAX / (11 * per)) return fail(RL_ERR_INVALID, "rl_env_create: too many start states (%d)", n_starts);
    for (size_t i = 0; i < (size_t)n_starts * per * 11; ++i)
        if (!std::isfinite(starts_m11[i]))
            return fail(RL_ERR_INVALID, "rl_env_create: start state %zu holds a non-finite value", i / 11);
    if ((rc = check_fan_args(h, q.n_envs, q.fov, q.num_rays))) return rc;
    OutlineParams outline{};
    if (group > 0 && ((rc = race_args(h, q.n_envs / group, group, q.num_rays)) ||
                      (rc = race_outline(h->map, c->P.LENGTH, c->P.WIDTH, outline))))
        return rc;
    std::unique_ptr<rl_env, decltype(&rl_env_destroy)> e(new (std::nothrow) rl_env(), rl_env_destroy);
    if (!e) return fail(RL_ERR_NOMEM, "out of host memory");
    e->c = c;
    e->h = h;
    e->prm = q;
    e->device = c->device;
    e->n_starts = n_starts;
    e->group = group;
    e->min_running = min_running;
    e->outline = outline;
    EnvParams &ep = e->ep;
    ep.P = c->P;
    ep.dt = q.dt;
    ep.scan_dist_to_base = q.scan_dist_to_base;
    ep.crash_thresh = q.crash_thresh;
    ep.steer_clip = q.steer_clip;
    ep.crash_reward = q.crash_reward;
    ep.n_envs = q.n_envs;
    ep.substeps = q.substeps;
    ep.num_rays = q.num_rays;
    ep.obs_start = q.obs_start;
    ep.obs_count = q.obs_count;
    ep.obs_stride = q.obs_stride;
    ep.obs_clip = q.obs_clip;
    ep.obs_scale = q.obs_scale;
    ep.max_ticks = q.max_ticks;
    ep.auto_reset = q.auto_reset != 0;
    ep.n_starts = n_starts;
    if (hipSetDevice(e->device) != hipSuccess) return fail(RL_ERR_HIP, "rl_env_create: hipSetDevice failed");
    const size_t N = q.n_envs, B = q.num_rays, M = (size_t)n_starts * per, R = N / per;
    if ((group > 0 && ((rc = e->race_tick.ensure(R)) || (rc = e->race_episode.ensure(R)) ||
                       (rc = e->race_start_index.ensure(R)) || (rc = e->race_over.ensure(R)))) ||
        (rc = e->state.ensure(N * 11)) || (rc = e->starts.ensure(M * 11)) || (rc = e->edge.ensure(B)) || (rc = e->tick.ensure(N)) ||
        (rc = e->episode.ensure(N)) || (rc = e->start_index.ensure(N)) || (rc = e->done.ensure(N)) || (rc = e->phase.ensure(N)) ||
        (rc = e->moved.ensure(N)) || (rc = e->pose.ensure(N * 3)) || (rc = e->ranges.ensure(N * B)) ||
        (rc = e->h_actions.ensure(N * 2)) || (rc = e->h_sidx.ensure(N)) || (rc = e->h_obs.ensure(N * q.obs_count)) ||
        (rc = e->h_reward.ensure(N)) || (rc = e->h_done.ensure(N)) || (rc = e->h_aux.ensure(N * 4)))
        return rc;
    if (hipMemcpy(e->starts, starts_m11, M * 11 * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(e->edge, edge, B * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return fail(RL_ERR_HIP, "rl_env_create: upload failed");
    *out = e.release();
    return RL_OK;
}

extern "C" int rl_env_create(rl_car *c, rl_method *h, const rl_env_params *params, const double *edge,
                             const double *starts_m11, int n_starts, rl_env **out)
{
    return env_create(c, h, params, edge, starts_m11, n_starts, 0, 0, out);
}

extern "C" int rl_env_create_race(rl_car *c, rl_method *h, const rl_race_env_params *params, const double *edge,
                                  const double *starts_mp11, int n_starts, rl_env **out)
{
    if (!params) return fail(RL_ERR_INVALID, "rl_env_create_race: null pointer");
    const int P = params->group;
    if (P < 1 || P > RACE_MAX_GROUP)
        return fail(RL_ERR_INVALID, "rl_env_create_race: group must lie in [1, %d] cars (got %d)", RACE_MAX_GROUP, P);
    if (params->env.n_envs % P != 0)
        return fail(RL_ERR_INVALID, "rl_env_create_race: n_envs (%d) must be a multiple of group (%d)", params->env.n_envs, P);
    if (params->min_running < 1 || params->min_running > P)
        return fail(RL_ERR_INVALID, "rl_env_create_race: min_running must lie in [1, %d] (got %d)", P, params->min_running);
    return env_create(c, h, &params->env, edge, starts_mp11, n_starts, P, params->min_running, out);
}

static TrackTable track_table(const rl_track *t)
{
    const double *p = t->table;
    const size_t W = t->W, S = t->S;
    return TrackTable{p, p + W, p + 2 * W, p + 2 * W + S, p + 2 * W + 2 * S, p + 2 * W + 3 * S, p + 2 * W + 4 * S,
                      t->W, t->S, t->closed, t->cum[S]};
}

// the track kernel of an env with a track, behind phase B on st: it reads this call's phase, done and states
static int track_launch(rl_env *e, float *d_reward, hipStream_t st)
{
    if (!e->track) return RL_OK;
    const int N = e->prm.n_envs;
    const TrackTable T = track_table(e->track);
    const TrackBufs tb{e->track_st, e->track_rows, e->track_ints};
    if (e->group > 0)
        return launch("track_kernel", track_kernel<true>, dim3(N / e->group), dim3(64 * e->group), 0, st, N, T, e->tp, tb, e->state,
                      e->phase, e->done, d_reward);
    return launch("track_kernel", track_kernel<false>, dim3((N + DRIVE_CARS - 1) / DRIVE_CARS), dim3(64 * DRIVE_CARS), 0, st, N, T,
                  e->tp, tb, e->state, e->phase, e->done, d_reward);
}

// one call's launches on st: phase A (reset: the spawn), the scan at slot k, the source's answers, phase B, then the
// track kernel where a track is attached.  lp: the call's Loop, owner e.  The env's kind picks phase A and B: a plain
// env; a race env (whole races spawn and end, and the cars see each other in the scan); one with drivers in its seats
// (the SEATS instances); one with a league (the LEAGUE instances: phase A adopts the pending entries, so the live ones
// are grouped by member behind it, for the members' network behind the scan)
static int env_launch(rl_env *e, const Loop &lp, bool reset, uint64_t k, const float *d_actions, const int *d_start_index,
                      float *d_obs, float *d_reward, int *d_done, float *d_aux, hipStream_t st)
{
    const int N = e->prm.n_envs, B = e->prm.num_rays;
    const EnvBufs b = env_bufs(e);
    const RaceEnvBufs rb = race_env_bufs(e);
    const uint64_t off = e->base + k * (uint64_t)N * (uint64_t)B;
    const bool race = e->group > 0, seats = lp.src.kind == SteerSource::SEATS, league = lp.src.kind == SteerSource::LEAGUE;
    const LoopScan scan{e->pose, N, e->prm.fov, B, e->ranges, e->mlp, e->group, e->state, &e->outline};
    // phase A and phase B of a kind: `mode` is what its kernels take between the env's buffers and the call's
    const auto step = [&](auto kernel, const char *name, const auto &...mode) {
        return launch(name, kernel, dim3((N + 63) / 64), dim3(64), 0, st, e->ep, b, mode..., d_actions, d_start_index, reset ? 1 : 0);
    };
    const auto observe = [&](const auto &table, int per_wg, const char *name, const auto &...mode) {
        return lp.scan_then(scan, off, table, per_wg, name, st, e->ep, b, mode..., d_obs, d_reward, d_done, d_aux);
    };
    int rc = league ? pop_enter(lp.src.pop, st) : (int)RL_OK;
    if (rc == RL_OK)
        rc = seats    ? step(race_env_seat_step_kernel, "race_env_seat_step_kernel", rb, e->seats)
             : league ? step(race_env_league_step_kernel, "race_env_league_step_kernel", rb, e->lg)
             : race   ? step(race_env_step_kernel, "race_env_step_kernel", rb)
                      : step(env_step_kernel, "env_step_kernel");
    if (rc == RL_OK && league) rc = league_group(lp.src.pop, e->lg_live, N, st);
    if (rc == RL_OK)
        rc = seats    ? observe(race_env_seat_observe_table, e->group, "race_env_seat_observe_kernel", rb, e->seats)
             : league ? observe(race_env_league_observe_table, e->group, "race_env_league_observe_kernel", rb, e->lg)
             : race   ? observe(race_env_observe_table, e->group, "race_env_observe_kernel", rb)
                      : observe(env_observe_table, DRIVE_CARS, "env_observe_kernel");
    return rc ? rc : track_launch(e, d_reward, st);
}

// a host form after launches on a caller's stream: c's stream is not ordered behind that one
static int env_settle(rl_env *e)
{
    if (e->foreign) {
        HIPCHK(hipDeviceSynchronize());
        e->foreign = false;
    }
    return RL_OK;
}

// a device form: this call enqueues on the caller's stream st
static int env_on_stream(rl_env *e, void *hip_stream, hipStream_t &st)
{
    HIPCHK(hipSetDevice(e->device));
    st = (hipStream_t)hip_stream;
    if (st != (hipStream_t)e->c->stream) e->foreign = true;
    return RL_OK;
}

// what a call asks of env e under its mutex: the driver mode the call is about (NOBODY: any), and a reset
static int env_ready(const rl_env *e, const char *name, SteerSource::Kind mode = SteerSource::NOBODY, bool need_reset = true)
{
    if (mode == SteerSource::SEATS && e->src.kind != mode)
        return fail(RL_ERR_INVALID, "%s: no seats attached (rl_env_attach_seats)", name);
    if (mode == SteerSource::LEAGUE && e->src.kind != mode)
        return fail(RL_ERR_INVALID, "%s: no league attached (rl_env_attach_league)", name);
    if (need_reset && !e->ready) return fail(RL_ERR_INVALID, "%s: reset the environment first (rl_env_reset)", name);
    return RL_OK;
}

// a host form that launches nothing: the env's and the car's mutex, the call's own refusals, the device, the wait for a
// caller's stream, then body's copies on one HostCall and its wait
template <class Refusals, class Body>
static int env_host_call(rl_env *e, Refusals refusals, Body body)
{
    std::scoped_lock lk(e->mu, e->c->mu);
    int rc = refusals();
    if (rc) return rc;
    HIPCHK(hipSetDevice(e->device));
    if ((rc = env_settle(e))) return rc;
    HostCall hc(e->c->stream);
    if ((rc = body(hc))) return rc;
    return hc.finish();
}

static int env_reset_locked(rl_env *e, const Loop &lp, uint64_t seed, const int *d_start_index, float *d_obs,
                            float *d_aux, int *d_done, hipStream_t st)
{
    e->ready = false;
    e->ep.key = noise_key(seed);
    e->base = lp.base;
    const int rc = env_launch(e, lp, true, 0, nullptr, d_start_index, d_obs, nullptr, d_done, d_aux, st);
    if (rc) return rc;
    e->k = 0;
    e->ready = true;
    return RL_OK;
}

static int env_step_locked(rl_env *e, const Loop &lp, const float *d_actions, float *d_obs, float *d_reward, int *d_done,
                           float *d_aux, hipStream_t st)
{
    const int rc = env_launch(e, lp, false, e->k + 1, d_actions, nullptr, d_obs, d_reward, d_done, d_aux, st);
    if (rc) {
        e->ready = false;                   // part of the step may have run: the env needs a reset
        return rc;
    }
    e->k += 1;
    return RL_OK;
}

extern "C" int rl_env_reset_device(rl_env *e, uint64_t seed, const int *d_start_index_or_null, float *d_obs,
                                   float *d_aux_or_null, int *d_done, void *hip_stream)
{
    if (!e || !d_obs || !d_done) return fail(RL_ERR_INVALID, "rl_env_reset_device: null pointer");
    int rc = env_scan_args(e);
    if (rc) return rc;
    const EnvLoop el(e);
    hipStream_t st;
    if ((rc = env_on_stream(e, hip_stream, st))) return rc;
    return env_reset_locked(e, el.lp, seed, d_start_index_or_null, d_obs, d_aux_or_null, d_done, st);
}

extern "C" int rl_env_step_device(rl_env *e, const float *d_actions_n2, float *d_obs, float *d_reward, int *d_done,
                                  float *d_aux_or_null, void *hip_stream)
{
    if (!e || !d_actions_n2 || !d_obs || !d_reward || !d_done) return fail(RL_ERR_INVALID, "rl_env_step_device: null pointer");
    const EnvLoop el(e);
    hipStream_t st;
    int rc;
    if ((rc = env_ready(e, "rl_env_step_device")) || (rc = env_scan_args(e)) || (rc = env_on_stream(e, hip_stream, st))) return rc;
    return env_step_locked(e, el.lp, d_actions_n2, d_obs, d_reward, d_done, d_aux_or_null, st);
}

// the host forms' way back: the staged results to the caller, then the wait (a failure leaves the env to be reset)
static int env_download(rl_env *e, HostCall &hc, float *obs, float *reward, int *done, float *aux)
{
    const size_t N = e->prm.n_envs;
    int rc;
    if ((rc = hc.down(obs, e->h_obs, N * e->prm.obs_count)) || (rc = hc.down(reward, e->h_reward, N)) ||
        (rc = hc.down(done, e->h_done, N)) || (rc = hc.down(aux, e->h_aux, N * 4)) || (rc = hc.finish()))
        e->ready = false;
    return rc;
}

extern "C" int rl_env_reset(rl_env *e, uint64_t seed, const int *start_index_or_null, float *obs, float *aux_or_null,
                            int *done)
{
    if (!e || !obs || !done) return fail(RL_ERR_INVALID, "rl_env_reset: null pointer");
    const int N = e->prm.n_envs, n_idx = e->group > 0 ? N / e->group : N;     // (a race env: one index per race)
    if (start_index_or_null)
        for (int i = 0; i < n_idx; ++i)
            if (start_index_or_null[i] < 0 || start_index_or_null[i] >= e->n_starts)
                return fail(RL_ERR_INVALID, "rl_env_reset: start_index[%d] = %d lies outside [0, %d)", i,
                            start_index_or_null[i], e->n_starts);
    int rc = env_scan_args(e);
    if (rc) return rc;
    const EnvLoop el(e);
    const Loop &lp = el.lp;
    HIPCHK(hipSetDevice(e->device));
    if ((rc = env_settle(e))) return rc;
    HostCall hc(e->c->stream);
    if ((start_index_or_null && (rc = hc.up(e->h_sidx, start_index_or_null, n_idx))) ||
        (rc = env_reset_locked(e, lp, seed, start_index_or_null ? (int *)e->h_sidx : nullptr, e->h_obs,
                               aux_or_null ? (float *)e->h_aux : nullptr, e->h_done, hc.st)))
        return rc;
    return env_download(e, hc, obs, nullptr, done, aux_or_null);
}

extern "C" int rl_env_step(rl_env *e, const float *actions_n2, float *obs, float *reward, int *done, float *aux_or_null)
{
    if (!e || !actions_n2 || !obs || !reward || !done) return fail(RL_ERR_INVALID, "rl_env_step: null pointer");
    const EnvLoop el(e);
    const Loop &lp = el.lp;
    const int N = e->prm.n_envs;
    int rc;
    if ((rc = env_ready(e, "rl_env_step")) || (rc = env_scan_args(e))) return rc;
    HIPCHK(hipSetDevice(e->device));
    if ((rc = env_settle(e))) return rc;
    HostCall hc(e->c->stream);
    if ((rc = hc.up(e->h_actions, actions_n2, (size_t)N * 2)) ||
        (rc = env_step_locked(e, lp, e->h_actions, e->h_obs, e->h_reward, e->h_done, aux_or_null ? (float *)e->h_aux : nullptr,
                              hc.st)))
        return rc;
    return env_download(e, hc, obs, reward, done, aux_or_null);
}

extern "C" int rl_env_read(rl_env *e, double *states_n11, int *ticks, int *episodes, int *start_index, int *done)
{
    if (!e) return fail(RL_ERR_INVALID, "rl_env_read: null pointer");
    const size_t N = e->prm.n_envs;
    return env_host_call(e, [&] { return env_ready(e, "rl_env_read"); }, [&](HostCall &hc) {
        int rc;
        if ((rc = hc.down(states_n11, e->state, N * 11)) || (rc = hc.down(ticks, e->tick, N)) ||
            (rc = hc.down(episodes, e->episode, N)) || (rc = hc.down(start_index, e->start_index, N)))
            return rc;
        return hc.down(done, e->done, N);
    });
}

extern "C" int rl_env_read_races(rl_env *e, int *race_ticks, int *race_episodes, int *race_start_index, int *race_over)
{
    if (!e) return fail(RL_ERR_INVALID, "rl_env_read_races: null pointer");
    const auto refusals = [&] {
        if (e->group < 1) return fail(RL_ERR_INVALID, "rl_env_read_races: not a race environment (rl_env_create_race)");
        return env_ready(e, "rl_env_read_races");
    };
    return env_host_call(e, refusals, [&](HostCall &hc) {
        const size_t R = e->prm.n_envs / e->group;
        int rc;
        if ((rc = hc.down(race_ticks, e->race_tick, R)) || (rc = hc.down(race_episodes, e->race_episode, R)) ||
            (rc = hc.down(race_start_index, e->race_start_index, R)))
            return rc;
        return hc.down(race_over, e->race_over, R);
    });
}

// ---------------------------------------------------------------- track progress (track_kernels.h)
extern "C" void rl_track_destroy(rl_track *t)
{
    if (!t) return;
    (void)hipSetDevice(t->device);
    (void)hipDeviceSynchronize();       // (an env's last track kernel may still read the table)
    delete t;
}

extern "C" int rl_track_create(int device, const double *xy_w2, int n_points, int closed, rl_track **out)
{
    if (!xy_w2 || !out) return fail(RL_ERR_INVALID, "rl_track_create: null pointer");
    const int W = n_points, S = closed ? W : W - 1;
    if (W < (closed ? 3 : 2) || W > 65536)
        return fail(RL_ERR_INVALID, "rl_track_create: n_points must lie in [%d, 65536] (got %d)", closed ? 3 : 2, W);
    for (int i = 0; i < 2 * W; ++i)
        if (!std::isfinite(xy_w2[i])) return fail(RL_ERR_INVALID, "rl_track_create: point %d holds a non-finite value", i / 2);
    int rc = check_device(device);
    if (rc) return rc;
    // x, y [W]; dx, dy, q, len [S]; cum [S + 1]
    std::vector<double> tab(2 * (size_t)W + 4 * (size_t)S + S + 1);
    double *x = tab.data(), *y = x + W, *dx = y + W, *dy = dx + S, *q = dy + S, *len = q + S, *cum = len + S;
    for (int i = 0; i < W; ++i) x[i] = xy_w2[2 * i], y[i] = xy_w2[2 * i + 1];
    cum[0] = 0.0;
    for (int i = 0; i < S; ++i) {
        const int j = i + 1 == W ? 0 : i + 1;
        dx[i] = x[j] - x[i];
        dy[i] = y[j] - y[i];
        const double a = dx[i] * dx[i], b = dy[i] * dy[i];
        q[i] = a + b;
        if (q[i] == 0.0) return fail(RL_ERR_INVALID, "rl_track_create: segment %d has no length", i);
        if (!std::isfinite(q[i])) return fail(RL_ERR_INVALID, "rl_track_create: segment %d is too long for f64", i);
        len[i] = std::sqrt(q[i]);
        cum[i + 1] = cum[i] + len[i];
    }
    std::unique_ptr<rl_track, decltype(&rl_track_destroy)> t(new (std::nothrow) rl_track(), rl_track_destroy);
    if (!t) return fail(RL_ERR_NOMEM, "out of host memory");
    t->device = device;
    t->W = W;
    t->S = S;
    t->closed = closed != 0;
    t->cum.assign(cum, cum + S + 1);
    HIPCHK(hipSetDevice(device));
    if ((rc = t->table.alloc(tab.size() * sizeof(double)))) return rc;
    HIPCHK(hipMemcpy(t->table, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    *out = t.release();
    return RL_OK;
}

extern "C" int rl_track_read(rl_track *t, double *cum_s_plus_1_or_null, double *length_or_null)
{
    if (!t) return fail(RL_ERR_INVALID, "rl_track_read: null pointer");
    if (cum_s_plus_1_or_null) std::copy(t->cum.begin(), t->cum.end(), cum_s_plus_1_or_null);
    if (length_or_null) *length_or_null = t->cum.back();
    return RL_OK;
}

extern "C" int rl_env_attach_track(rl_env *e, rl_track *t, const rl_track_params *p)
{
    if (!e) return fail(RL_ERR_INVALID, "rl_env_attach_track: null pointer");
    std::scoped_lock lk(e->mu, e->c->mu);
    if (t) {
        if (!p) return fail(RL_ERR_INVALID, "rl_env_attach_track: null params");
        if (p->window < 0 || p->window > 65536 || p->goal_span < 0 || p->goal_span > 65536)
            return fail(RL_ERR_INVALID, "rl_env_attach_track: window and goal_span must lie in [0, 65536] (got %d, %d)",
                        p->window, p->goal_span);
        if (p->reward_mode != 0 && p->reward_mode != 1)
            return fail(RL_ERR_INVALID, "rl_env_attach_track: reward_mode must be 0 or 1 (got %d)", p->reward_mode);
        if (!std::isfinite(p->lookahead) || !(p->lookahead > 0.0))
            return fail(RL_ERR_INVALID, "rl_env_attach_track: lookahead must be finite and > 0");
        if (t->device != e->device)
            return fail(RL_ERR_INVALID, "rl_env_attach_track: track (device %d) and env (device %d) must share one device",
                        t->device, e->device);
        HIPCHK(hipSetDevice(e->device));
        const size_t N = e->prm.n_envs;
        int rc;
        if ((rc = e->track_st.ensure(N * 3)) || (rc = e->track_rows.ensure(N * 8)) || (rc = e->track_ints.ensure(N * 4)))
            return rc;
        e->tp = TrackParams{p->window, p->goal_span, p->reward_mode, e->group, p->lookahead};
    }
    e->track = t;
    e->ready = false;                   // the rows of the new track start at the next reset
    return RL_OK;
}

extern "C" int rl_env_read_track(rl_env *e, float *rows_n8, int *ints_n4)
{
    if (!e) return fail(RL_ERR_INVALID, "rl_env_read_track: null pointer");
    const auto refusals = [&] {
        if (!e->track) return fail(RL_ERR_INVALID, "rl_env_read_track: no track attached (rl_env_attach_track)");
        return env_ready(e, "rl_env_read_track");
    };
    return env_host_call(e, refusals, [&](HostCall &hc) {
        const size_t N = e->prm.n_envs;
        const int rc = hc.down(rows_n8, e->track_rows, N * 8);
        return rc ? rc : hc.down(ints_n4, e->track_ints, N * 4);
    });
}

extern "C" int rl_env_read_track_device(rl_env *e, float *d_rows_n8, int *d_ints_n4, void *hip_stream)
{
    if (!e) return fail(RL_ERR_INVALID, "rl_env_read_track_device: null pointer");
    std::scoped_lock lk(e->mu, e->c->mu);
    if (!e->track) return fail(RL_ERR_INVALID, "rl_env_read_track_device: no track attached (rl_env_attach_track)");
    hipStream_t st;
    int rc;
    if ((rc = env_ready(e, "rl_env_read_track_device")) || (rc = env_on_stream(e, hip_stream, st))) return rc;
    const size_t N = e->prm.n_envs;
    if (d_rows_n8) HIPCHK(hipMemcpyAsync(d_rows_n8, e->track_rows, N * 8 * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (d_ints_n4) HIPCHK(hipMemcpyAsync(d_ints_n4, e->track_ints, N * 4 * sizeof(int), hipMemcpyDeviceToDevice, st));
    return RL_OK;
}

// ---------------------------------------------------------------- track progress of the roll-outs
// (include/scanlib_track_drive.h; the launches are drive_loop's)
extern "C" int rl_car_attach_track(rl_car *c, rl_track *t, const rl_drive_track_params *p)
{
    if (!c) return fail(RL_ERR_INVALID, "rl_car_attach_track: null pointer");
    std::scoped_lock lk(c->mu);
    if (t) {
        if (!p) return fail(RL_ERR_INVALID, "rl_car_attach_track: null params");
        if (!c->reps.empty()) return fail(RL_ERR_INVALID, "rl_car_attach_track is single-device only: pass an ordinary car handle");
        if (p->window < 0 || p->window > 65536)
            return fail(RL_ERR_INVALID, "rl_car_attach_track: window must lie in [0, 65536] (got %d)", p->window);
        if (!std::isfinite(p->goal_dist) || p->goal_dist < 0.0)
            return fail(RL_ERR_INVALID, "rl_car_attach_track: goal_dist must be finite and >= 0");
        if (t->device != c->device)
            return fail(RL_ERR_INVALID, "rl_car_attach_track: track (device %d) and car (device %d) must share one device",
                        t->device, c->device);
        c->dt_window = p->window;
        c->dt_goal = p->goal_dist == 0.0 ? t->cum.back() : p->goal_dist;
    }
    c->track = t;
    c->dt_cars = c->dt_score_rows = c->dt_score_cols = 0;      // the rows of the new track start at the next roll-out
    return RL_OK;
}

extern "C" int rl_car_read_track(rl_car *c, int n_cars, double *rows_n4, int *ints_n4)
{
    if (!c) return fail(RL_ERR_INVALID, "rl_car_read_track: null pointer");
    std::scoped_lock lk(c->mu);
    if (!c->track) return fail(RL_ERR_INVALID, "rl_car_read_track: no track attached (rl_car_attach_track)");
    if (!c->dt_cars) return fail(RL_ERR_INVALID, "rl_car_read_track: no roll-out has run with the track yet");
    if (n_cars != c->dt_cars)
        return fail(RL_ERR_INVALID, "rl_car_read_track: the last tracked roll-out had %d cars (got n_cars %d)", c->dt_cars, n_cars);
    HIPCHK(hipSetDevice(c->device));
    HostCall hc(c->stream);
    int rc;
    if ((rc = hc.down(rows_n4, c->dt_rows, (size_t)n_cars * 4)) || (rc = hc.down(ints_n4, c->dt_ints, (size_t)n_cars * 4))) return rc;
    return hc.finish();
}

extern "C" int rl_car_read_track_scores(rl_car *c, int n_rows, int n_cols, double *scores)
{
    if (!c || !scores) return fail(RL_ERR_INVALID, "rl_car_read_track_scores: null pointer");
    std::scoped_lock lk(c->mu);
    if (!c->track) return fail(RL_ERR_INVALID, "rl_car_read_track_scores: no track attached (rl_car_attach_track)");
    if (!c->dt_score_rows)
        return fail(RL_ERR_INVALID, "rl_car_read_track_scores: the last tracked roll-out was no population's and no league's");
    if (n_rows != c->dt_score_rows || n_cols != c->dt_score_cols)
        return fail(RL_ERR_INVALID, "rl_car_read_track_scores: the last tracked roll-out left scores [%d][%d] (got [%d][%d])",
                    c->dt_score_rows, c->dt_score_cols, n_rows, n_cols);
    HIPCHK(hipSetDevice(c->device));
    HostCall hc(c->stream);
    const int rc = hc.down(scores, c->dt_scores, (size_t)n_rows * n_cols);
    return rc ? rc : hc.finish();
}

// ---------------------------------------------------------------- the env's drivers: seats and leagues
// (include/scanlib_seats.h, include/scanlib_league_env.h)
// how both attach calls begin once they have refused what they refuse: launches in flight may still read the tables
// replaced below, the attached drivers of `mode` go, and the answers of new ones start at the next reset
static int env_detach(rl_env *e, SteerSource::Kind mode)
{
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipDeviceSynchronize());
    e->foreign = false;
    if (e->src.kind == mode) e->src = SteerSource();
    e->ready = false;
    return RL_OK;
}

extern "C" int rl_env_attach_seats(rl_env *e, rl_followgap *g_or_null, rl_policy *p_or_null, const rl_seat_params *sp_or_null)
{
    if (!e) return fail(RL_ERR_INVALID, "rl_env_attach_seats: null pointer");
    std::scoped_lock lk(e->mu, e->c->mu);
    if (e->group < 1) return fail(RL_ERR_INVALID, "rl_env_attach_seats: not a race environment (rl_env_create_race)");
    if (sp_or_null && e->src.kind == SteerSource::LEAGUE)
        return fail(RL_ERR_INVALID, "rl_env_attach_seats: a league is attached (rl_env_attach_league): detach it first");
    const int N = e->prm.n_envs, P = e->group, B = e->prm.num_rays;
    SeatBufs S{};
    int rc;
    if (sp_or_null) {
        for (int k = 0; k < P; ++k) {
            const int d = sp_or_null->driver[k];
            if (d == RL_SEAT_CALLER) continue;
            if ((rc = seat_code("rl_env_attach_seats", k, d, g_or_null, p_or_null))) return rc;
            const bool net = d == RL_SEAT_POLICY;
            const int dev = net ? p_or_null->device : g_or_null->device;
            if (dev != e->device)
                return fail(RL_ERR_INVALID, "rl_env_attach_seats: %s (device %d) and env (device %d) must share one device",
                            net ? "policy" : "FollowGap", dev, e->device);
            if (!std::isfinite(sp_or_null->speed[k]))
                return fail(RL_ERR_INVALID, "rl_env_attach_seats: the speed of seat %d must be finite", k);
            S.scripted |= 1u << k;
            if (net) S.policy |= 1u << k;
            S.speed[k] = sp_or_null->speed[k];
        }
        if (S.policy && (rc = policy_args(p_or_null, N, B))) return rc;
    }
    if ((rc = env_detach(e, SteerSource::SEATS)) || !sp_or_null) return rc;
    if ((rc = e->answer.ensure(N))) return rc;
    if (S.policy) {
        const std::vector<int> rows = seat_row_list(S.policy, N / P, P);
        if ((rc = e->mlp.ensure(N)) || (rc = e->seat_rows.ensure(rows.size()))) return rc;
        HIPCHK(hipMemcpy(e->seat_rows, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    if (S.scripted & ~S.policy) S.fg = g_or_null->P;
    S.fg.size = B;
    S.mlp = e->mlp;
    S.answer = e->answer;
    e->seats = S;
    // (neither handle is named: SteerSource says why)
    e->src = SteerSource::seats(nullptr, nullptr, S.policy ? &p_or_null->P : nullptr, S.policy, P, &e->seat_rows);
    return RL_OK;
}

// the seat drivers' or the league's kept answers, to the host (dev = false) or on the caller's stream
static int env_read_answers(rl_env *e, const char *name, SteerSource::Kind mode, float *steer_n, bool dev, void *hip_stream)
{
    if (!e) return fail(RL_ERR_INVALID, "%s: null pointer", name);
    const size_t N = e->prm.n_envs;
    if (!dev)
        return env_host_call(e, [&] { return env_ready(e, name, mode); },
                             [&](HostCall &hc) { return hc.down(steer_n, e->answer, N); });
    std::scoped_lock lk(e->mu, e->c->mu);
    hipStream_t st;
    int rc;
    if ((rc = env_ready(e, name, mode)) || (rc = env_on_stream(e, hip_stream, st))) return rc;
    if (steer_n) HIPCHK(hipMemcpyAsync(steer_n, e->answer, N * sizeof(float), hipMemcpyDeviceToDevice, st));
    return RL_OK;
}

extern "C" int rl_env_read_seats(rl_env *e, float *steer_n)
{
    return env_read_answers(e, "rl_env_read_seats", SteerSource::SEATS, steer_n, false, nullptr);
}

extern "C" int rl_env_read_seats_device(rl_env *e, float *d_steer_n, void *hip_stream)
{
    return env_read_answers(e, "rl_env_read_seats_device", SteerSource::SEATS, d_steer_n, true, hip_stream);
}

// the host forms' look at an entry table of env e with population pop, FollowGap g and the seat speeds `speed`
static int league_env_entries(const char *fn, const rl_env *e, const rl_policy_pop *pop, const rl_followgap *g,
                              const int *entry, const float *speed, bool *any_net)
{
    size_t n_net = 0;
    int rc = league_entries(fn, entry, (size_t)e->prm.n_envs, pop->n_members, -2, g != nullptr, speed, e->group, &n_net);
    if (rc == RL_OK && n_net) rc = policy_window(pop->P, e->prm.num_rays, fn);
    *any_net = n_net > 0;
    return rc;
}

extern "C" int rl_env_attach_league(rl_env *e, rl_followgap *g_or_null, rl_policy_pop *pop, const int *entry_N_or_null,
                                    const float *speed_P)
{
    if (!e) return fail(RL_ERR_INVALID, "rl_env_attach_league: null pointer");
    std::scoped_lock lk(e->mu, e->c->mu);
    if (e->group < 1) return fail(RL_ERR_INVALID, "rl_env_attach_league: not a race environment (rl_env_create_race)");
    const size_t N = e->prm.n_envs;
    LeagueEnvBufs L{};
    bool any_net = false;
    int rc;
    if (entry_N_or_null) {
        if (!pop || !speed_P) return fail(RL_ERR_INVALID, "rl_env_attach_league: null pointer");
        if (e->src.kind == SteerSource::SEATS)
            return fail(RL_ERR_INVALID, "rl_env_attach_league: seats are attached (rl_env_attach_seats): detach them first");
        if (pop->device != e->device || (g_or_null && g_or_null->device != e->device))
            return fail(RL_ERR_INVALID, "rl_env_attach_league: %s (device %d) and env (device %d) must share one device",
                        pop->device != e->device ? "population" : "FollowGap",
                        pop->device != e->device ? pop->device : g_or_null->device, e->device);
        if ((rc = league_env_entries("rl_env_attach_league", e, pop, g_or_null, entry_N_or_null, speed_P, &any_net))) return rc;
    }
    if ((rc = env_detach(e, SteerSource::LEAGUE)) || !entry_N_or_null) return rc;
    const size_t rows = (size_t)pop->n_members + 2;
    if ((rc = e->lg_pending.ensure(N)) || (rc = e->lg_live.ensure(N)) || (rc = e->mlp.ensure(N)) ||
        (rc = e->answer.ensure(N)) || (rc = e->lg_results.ensure(rows * 8)))
        return rc;
    HIPCHK(hipMemcpy(e->lg_pending, entry_N_or_null, N * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(e->lg_results, 0, rows * 8 * sizeof(unsigned long long)));
    const bool window = e->prm.num_rays >= pop->P.in_start + pop->P.dims[0];
    L.lo = g_or_null ? -1 : 0;
    L.hi = window ? pop->n_members : 0;
    L.n_members = pop->n_members;
    for (int k = 0; k < e->group; ++k) L.speed[k] = speed_P[k];
    if (g_or_null) L.fg = g_or_null->P;
    L.fg.size = e->prm.num_rays;
    L.pending = e->lg_pending;
    L.live = e->lg_live;
    L.mlp = e->mlp;
    L.answer = e->answer;
    L.results = e->lg_results;
    e->lg = L;
    // (the entries live on the device: the grouping is env_launch's; an entry that names a member has a window, so L.hi > 0)
    e->src = SteerSource::league(g_or_null, pop, nullptr, any_net ? (int)N : 0);
    return RL_OK;
}

extern "C" int rl_env_set_league_entries(rl_env *e, const int *entry_N)
{
    if (!e || !entry_N) return fail(RL_ERR_INVALID, "rl_env_set_league_entries: null pointer");
    bool any_net = false;
    const auto refusals = [&] {
        const int rc = env_ready(e, "rl_env_set_league_entries", SteerSource::LEAGUE, false);
        return rc ? rc : league_env_entries("rl_env_set_league_entries", e, e->src.pop, e->src.g, entry_N, e->lg.speed, &any_net);
    };
    return env_host_call(e, refusals, [&](HostCall &hc) {
        const int rc = hc.up((int *)e->lg_pending, entry_N, (size_t)e->prm.n_envs);
        if (rc == RL_OK && any_net) e->src.n_net = e->prm.n_envs;
        return rc;
    });
}

extern "C" int rl_env_set_league_entries_device(rl_env *e, const int *d_entry_N, void *hip_stream)
{
    if (!e || !d_entry_N) return fail(RL_ERR_INVALID, "rl_env_set_league_entries_device: null pointer");
    std::scoped_lock lk(e->mu, e->c->mu);
    hipStream_t st;
    int rc;
    if ((rc = env_ready(e, "rl_env_set_league_entries_device", SteerSource::LEAGUE, false)) ||
        (rc = env_on_stream(e, hip_stream, st)))
        return rc;
    HIPCHK(hipMemcpyAsync(e->lg_pending, d_entry_N, (size_t)e->prm.n_envs * sizeof(int), hipMemcpyDeviceToDevice, st));
    if (e->lg.hi > 0) e->src.n_net = e->prm.n_envs;     // (the host cannot look at these entries: one may name a member)
    return RL_OK;
}

extern "C" int rl_env_read_league_steers(rl_env *e, float *steer_n)
{
    return env_read_answers(e, "rl_env_read_league_steers", SteerSource::LEAGUE, steer_n, false, nullptr);
}

extern "C" int rl_env_read_league_steers_device(rl_env *e, float *d_steer_n, void *hip_stream)
{
    return env_read_answers(e, "rl_env_read_league_steers_device", SteerSource::LEAGUE, d_steer_n, true, hip_stream);
}

extern "C" int rl_env_read_league_entries(rl_env *e, int *live_N_or_null, int *pending_N_or_null)
{
    if (!e) return fail(RL_ERR_INVALID, "rl_env_read_league_entries: null pointer");
    const auto refusals = [&] {
        return env_ready(e, "rl_env_read_league_entries", SteerSource::LEAGUE, live_N_or_null != nullptr);
    };
    return env_host_call(e, refusals, [&](HostCall &hc) {
        const size_t N = e->prm.n_envs;
        const int rc = hc.down(live_N_or_null, e->lg_live, N);
        return rc ? rc : hc.down(pending_N_or_null, e->lg_pending, N);
    });
}

extern "C" int rl_env_read_league_results(rl_env *e, int64_t *results, int clear)
{
    if (!e || !results) return fail(RL_ERR_INVALID, "rl_env_read_league_results: null pointer");
    const auto refusals = [&] { return env_ready(e, "rl_env_read_league_results", SteerSource::LEAGUE); };
    return env_host_call(e, refusals, [&](HostCall &hc) {
        const size_t n = ((size_t)e->lg.n_members + 2) * 8;
        const int rc = hc.down((unsigned long long *)results, e->lg_results, n);
        if (rc) return rc;
        if (clear) HIPCHK(hipMemsetAsync(e->lg_results, 0, n * sizeof(unsigned long long), hc.st));
        return (int)RL_OK;
    });
}

// ---------------------------------------------------------------- diagnostics: HBM stream probe
static int probe_hbm_modes(int device, size_t bytes, double *gbs_out, int mode_lo, int mode_hi);

extern "C" int rl_probe_hbm(int device, size_t bytes, double *gbs_out5)
{
    return probe_hbm_modes(device, bytes, gbs_out5, 0, 5);
}

extern "C" int rl_probe_hbm_nt(int device, size_t bytes, double *gbs_out3)
{
    return probe_hbm_modes(device, bytes, gbs_out3, 5, 8);
}

extern "C" int rl_probe_literal_sincosf(int device, const float *x, size_t n, float *sin_out, float *cos_out)
{
    if (!x || !sin_out || !cos_out) return fail(RL_ERR_INVALID, "rl_probe_literal_sincosf: null pointer");
    int rc = check_device(device);
    if (rc || n == 0) return rc;
    HIPCHK(hipSetDevice(device));
    DevPtr<float> buf;
    if (buf.alloc(3 * n * sizeof(float))) return fail(RL_ERR_NOMEM, "rl_probe_literal_sincosf: %zu floats", 3 * n);
    float *const d = buf;
    if (hipMemcpy(d, x, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return fail(RL_ERR_HIP, "upload failed");
    const int grid = (int)std::min<size_t>((n + 255) / 256, 4096);
    if ((rc = launch("literal_sincosf_kernel", literal_sincosf_kernel, dim3(grid), dim3(256), 0, nullptr, d, (long)n, d + n,
                     d + 2 * n)))
        return rc;
    if (hipMemcpy(sin_out, d + n, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(cos_out, d + 2 * n, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(RL_ERR_HIP, "rl_probe_literal_sincosf: kernel or download failed");
    return RL_OK;
}

static int probe_hbm_modes(int device, size_t bytes, double *gbs_out5, int mode_lo, int mode_hi)
{
    if (!gbs_out5) return fail(RL_ERR_INVALID, "rl_probe_hbm: null pointer");
    if (bytes < ((size_t)1 << 20)) return fail(RL_ERR_INVALID, "rl_probe_hbm: at least 1 MiB per buffer");
    int rc = check_device(device);
    if (rc) return rc;
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    Stream st;                          // (declared first: the buffers go before it, and freeing them drains the device)
    Event e0, e1;
    DevPtr<uint4> a, b;
    DevPtr<uint32_t> sink;
    const size_t n16 = bytes / 16;
    if (a.alloc(n16 * 16) || b.alloc(n16 * 16) || sink.alloc(4) || e0.create() != hipSuccess || e1.create() != hipSuccess ||
        st.create() != hipSuccess || hipMemsetAsync(a, 1, n16 * 16, st) != hipSuccess ||
        hipMemsetAsync(b, 2, n16 * 16, st) != hipSuccess)
        return fail(RL_ERR_NOMEM, "rl_probe_hbm: setup failed (2 x %zu bytes)", n16 * 16);
    const int grid = prop.multiProcessorCount * 8, reps = 10;
    for (int mode = mode_lo; mode < mode_hi; ++mode) {
        // (the first one warms)
        if ((rc = launch("hbm_probe_kernel", hbm_probe_kernel, dim3(grid), dim3(256), 0, st, a, b, n16, mode, sink))) return rc;
        (void)hipEventRecord(e0, st);
        for (int r = 0; r < reps; ++r)
            if ((rc = launch("hbm_probe_kernel", hbm_probe_kernel, dim3(grid), dim3(256), 0, st, a, b, n16, mode, sink))) return rc;
        (void)hipEventRecord(e1, st);
        float ms = 0.f;
        if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess || !(ms > 0.f))
            return fail(RL_ERR_HIP, "rl_probe_hbm: launch failed");
        const double moved = (double)n16 * 16.0 * ((mode == 0 || mode == 3 || mode == 6 || mode == 7) ? 2.0 : 1.0);
        gbs_out5[mode - mode_lo] = moved * reps / ((double)ms * 1e-3) / 1e9;
    }
    return RL_OK;
}

// ---------------------------------------------------------------- 16-bit ranges for the xGMI exchange (opt-in, lossy)
static int u16_args(int device, size_t n, float max_range_m, const void *a, const void *b)
{
    if (!(max_range_m > 0.0f)) return fail(RL_ERR_INVALID, "max_range_m must be > 0");
    if (n > 0 && (!a || !b)) return fail(RL_ERR_INVALID, "null device pointer");
    return check_device(device);
}

// leading elements until the u16 pointer is 16-B aligned, and whether the f32 pointer is aligned there too
static void u16_split(const void *f32, const void *u16, size_t n, size_t &head, int &vec)
{
    head = ((16 - ((uintptr_t)u16 & 15)) & 15) / 2;
    if (head > n) head = n;
    vec = (((uintptr_t)f32 + 4 * head) & 15) == 0 && ((uintptr_t)u16 & 1) == 0 && ((uintptr_t)f32 & 3) == 0;
}

extern "C" int rl_ranges_to_u16_device(int device, const float *d_ranges, size_t n, float max_range_m,
                                       uint16_t *d_out, void *hip_stream)
{
    int rc = u16_args(device, n, max_range_m, d_ranges, d_out);
    if (rc || n == 0) return rc;
    HIPCHK(hipSetDevice(device));
    size_t head;
    int vec;
    u16_split(d_ranges, d_out, n, head, vec);
    const int grid = (int)std::min<size_t>((n / 8 + 255) / 256 + 1, 256 * 16);
    return launch("ranges_to_u16_kernel", ranges_to_u16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)hip_stream, d_ranges, n,
                  max_range_m, 65535.0f / max_range_m, d_out, head, vec);
}

extern "C" int rl_ranges_from_u16_device(int device, const uint16_t *d_in, size_t n, float max_range_m,
                                         float *d_ranges, void *hip_stream)
{
    int rc = u16_args(device, n, max_range_m, d_in, d_ranges);
    if (rc || n == 0) return rc;
    HIPCHK(hipSetDevice(device));
    size_t head;
    int vec;
    u16_split(d_ranges, d_in, n, head, vec);
    const int grid = (int)std::min<size_t>((n / 8 + 255) / 256 + 1, 256 * 16);
    return launch("ranges_from_u16_kernel", ranges_from_u16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)hip_stream, d_in, n,
                  max_range_m / 65535.0f, d_ranges, head, vec);
}

// ---------------------------------------------------------------- diagnostics: gather-rate probe
extern "C" int rl_probe_gather_rate(int device, int active_lanes, double *lanes_per_clk_per_cu,
                                    double *clock_hz, int *n_cu_out)
{
    if (!lanes_per_clk_per_cu) return fail(RL_ERR_INVALID, "rl_probe_gather_rate: null pointer");
    if (active_lanes < 1 || active_lanes > 64) return fail(RL_ERR_INVALID, "active_lanes must be in [1,64]");
    int rc = check_device(device);
    if (rc) return rc;
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    const int n_cu = prop.multiProcessorCount;
    const double clk = (double)prop.clockRate * 1e3;
    Stream st;                          // (declared first: the buffers go before it, and freeing them drains the device)
    Event e0, e1;
    DevPtr<float> tab, sink;
    DevPtr<int> d_off;
    // random cells of a 32x32 window in the 4-row-interleaved layout of the step map, fixed seed
    int off[64];
    uint32_t lcg = 12345u;
    auto rnd = [&]() { lcg = lcg * 1664525u + 1013904223u; return (lcg >> 8) & 0xffffu; };
    for (int l = 0; l < 64; ++l) {
        const int r = (int)(rnd() % 32), c = (int)(rnd() % 32) + 3;
        off[l] = (r >> 2) * 4 * 64 + 4 * c + (r & 3);
    }
    unsigned long long mask = 0;
    while (__builtin_popcountll(mask) < active_lanes) mask |= 1ull << (rnd() % 64);
    const int iters = 2000, grid = n_cu * 2;
    float ms = 0.f;
    if (tab.alloc(4 * 2048 * sizeof(float)) || sink.alloc(4) || d_off.alloc(sizeof off) || e0.create() != hipSuccess ||
        e1.create() != hipSuccess || st.create() != hipSuccess ||
        hipMemsetAsync(tab, 0, 4 * 2048 * sizeof(float), st) != hipSuccess ||
        hipMemcpyAsync(d_off, off, sizeof off, hipMemcpyHostToDevice, st) != hipSuccess)
        return fail(RL_ERR_HIP, "gather probe: setup failed");
    if ((rc = launch("gather_probe_kernel", gather_probe_kernel, dim3(grid), dim3(1024), 0, st, tab, d_off, mask, 10, sink)))
        return rc;
    (void)hipEventRecord(e0, st);
    if ((rc = launch("gather_probe_kernel", gather_probe_kernel, dim3(grid), dim3(1024), 0, st, tab, d_off, mask, iters, sink)))
        return rc;
    (void)hipEventRecord(e1, st);
    if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess || !(ms > 0.f))
        return fail(RL_ERR_HIP, "gather probe: launch failed");
    // 2 workgroups x 16 waves per CU, each iters x 8 wave-loads
    const double clk_per_wave_load = (double)ms * 1e-3 * clk / (2.0 * 16 * iters * 8);
    *lanes_per_clk_per_cu = (double)active_lanes / clk_per_wave_load;
    if (clock_hz) *clock_hz = clk;
    if (n_cu_out) *n_cu_out = n_cu;
    return RL_OK;
}

// ---------------------------------------------------------------- Car outline table and crash test (host)
// Car::setCarEdgeDistances (racecar/src/racecar.cpp:239-292): for every beam, how far from the lidar
// the car's own outline lies.  A one-off table per configuration, so it is host C++ (the crash test
// over scanned batches is fused into the march kernels, see CrashParams).  The reference's quirks are
// part of the contract (the crash codes scripts/mcts.py acts on depend on them): the beam angle is
// advanced BEFORE it is used (the table is shifted by one increment, :256), pi is 3.145
// (racecar.hpp:117), and a beam at exactly 0 rad is nudged to +1e-4 rad while still being treated as a
// non-positive angle, so its side distance is width/2 / sin(-1e-4): about -1016 m, and that beam
// reports a crash for any range (:277-283).  The nudge stays in the running angle.
extern "C" int rl_car_edge_distances(int num_rays, double min_ang, double ang_inc, double scan_dist_to_base,
                                     double width, double wheelbase, double *edge_out)
{
    if (num_rays < 0 || (num_rays > 0 && !edge_out))
        return fail(RL_ERR_INVALID, "rl_car_edge_distances: bad arguments");
    const double quarter_turn = 3.145 / 2.0;
    const double to_side = width / 2.0, to_front = wheelbase - scan_dist_to_base, to_back = scan_dist_to_base;
    double beam = min_ang;
    for (int j = 0; j < num_rays; ++j) {
        beam += ang_inc;
        const bool left = beam > 0.0;                           // decided before the nudge
        if (!left && beam == 0.0) beam += 0.0001;
        const double turned = left ? beam : -beam;              // angle away from straight ahead
        const bool ahead = turned < quarter_turn;               // hits the front edge, else the rear edge
        const double off_axis = ahead ? turned : turned - quarter_turn;
        const double along = (ahead ? to_front : to_back) / cos(off_axis);
        const double across = to_side / sin(off_axis);
        edge_out[j] = across < along ? across : along;
    }
    return RL_OK;
}

// Car::isCrashed (racecar/src/racecar.cpp:305-328) over host ranges: index of the first scan with a
// beam inside the car outline (+ threshold), else -(n_scans + 1).
extern "C" int rl_car_is_crashed(const float *ranges, int num_rays, int n_scans, const double *edge,
                                 double crash_thresh, int *first_crashed)
{
    if (!first_crashed || num_rays < 0 || n_scans < 0 || ((size_t)num_rays * n_scans > 0 && (!ranges || !edge)))
        return fail(RL_ERR_INVALID, "rl_car_is_crashed: bad arguments");
    *first_crashed = -(n_scans + 1);
    for (int k = 0; k < n_scans; ++k) {
        const float *scan = ranges + (size_t)k * num_rays;
        for (int j = 0; j < num_rays; ++j)
            if (((double)scan[j] - edge[j]) < crash_thresh) {
                *first_crashed = k;
                return RL_OK;
            }
    }
    return RL_OK;
}


// ---------------------------------------------------------------- the MCTS planner (mcts_kernels.h)
typedef void (*mcts_act_fn)(MctsParams, MctsBufs, int);
static const std::array<mcts_act_fn, FG_ROWS> mcts_act_table =
    rows_table<mcts_act_fn>([](auto rows) { return mcts_act_kernel<rows>; });

struct rl_mcts {
    rl_car *c = nullptr;
    rl_method *h = nullptr;
    SteerSource src;               // FollowGap, the policy or nobody (the random and the track source)
    rl_mcts_params prm{};
    MctsParams mp{};
    int device = 0;
    // node arrays and per-tree scratch (MctsBufs)
    DevPtr<int> parent, first_child, next_sibling, last_child, n_children, visits, child_visits, terminal, crash;
    DevPtr<double> reward, action, state, logtab, cstate, actions, edge, vel, roots, best_a;
    DevPtr<float> pose, answer, cpose, ranges, mlp, rposes, rranges;
    DevPtr<int> n_nodes, child, exp_term, first, best_v, best_n;
    DevPtr<uint32_t> keys;
    // rl_mcts_drive: the root crash flags, the K x D keys and the per-decision outputs
    DevPtr<int> root_crash, dr_first, dr_visits;
    DevPtr<uint32_t> dr_keys;
    DevPtr<double> dr_actions, dr_trace;
    // track-guided planning (rl_mcts_attach_track, rl_mcts_set_points): the borrowed track, its options, the explicit
    // points, the roots' rows (PlanRoots) and the roll-outs' f64 positions and terms
    rl_track *track = nullptr;
    PlanTrackParams tp{};
    bool has_points = false;
    int points_mode = PLAN_WAYPOINT;   // the reward mode of explicit points without a track (rl_mcts_attach_track(m, NULL, p))
    DevPtr<double> tk_points, tk_s, tk_point, rxy, terms;
    DevPtr<int> tk_seg, tk_goal, tk_has;
    bool ready = false;            // reset done and no launch failed since (read and written under mu only)
    long iters = 0;                // iterations since reset
    uint64_t base = 0;             // h's ray offset at reset
    std::mutex mu;
};

// math.log(n) for n = 0 ... n_max (log(0) = -inf, never read: a node with children has a visit sum >= 1)
static std::vector<double> mcts_log_table(int n_max)
{
    std::vector<double> t((size_t)n_max + 1);
    for (int n = 0; n <= n_max; ++n) t[n] = std::log((double)n);
    return t;
}

static MctsBufs mcts_bufs(rl_mcts *m)      // (root_crash: rl_mcts_drive sets it)
{
    return MctsBufs{m->parent, m->first_child, m->next_sibling, m->last_child, m->n_children, m->visits, m->child_visits,
                    m->terminal, m->crash, m->reward, m->action, m->state, m->pose, m->answer, m->n_nodes, m->child,
                    m->exp_term, m->keys, m->logtab, m->cstate, m->cpose, m->actions, m->ranges, m->edge, m->mlp, m->vel,
                    m->first, nullptr};
}

extern "C" void rl_mcts_destroy(rl_mcts *m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->c && m->c->stream) (void)hipStreamSynchronize(m->c->stream);
    delete m;
}

extern "C" int rl_mcts_create(rl_car *c, rl_method *h, rl_followgap *g, rl_policy *p, const rl_mcts_params *params,
                              const double *edge, rl_mcts **out)
{
    if (!c || !h || !params || !edge || !out) return fail(RL_ERR_INVALID, "rl_mcts_create: null pointer");
    const rl_mcts_params q = *params;
    if (q.source == RL_MCTS_FG && !g) return fail(RL_ERR_INVALID, "rl_mcts_create: the FG source needs a FollowGap handle");
    if (q.source == RL_MCTS_NN && !p) return fail(RL_ERR_INVALID, "rl_mcts_create: the NN source needs a policy handle");
    if (q.source != RL_MCTS_FG && q.source != RL_MCTS_NN && q.source != RL_MCTS_RANDOM && q.source != RL_MCTS_PURSUIT)
        return fail(RL_ERR_INVALID, "rl_mcts_create: unknown source %d", q.source);
    if (q.rollout_source != 0 && q.rollout_source != 1)
        return fail(RL_ERR_INVALID, "rl_mcts_create: rollout_source must be 0 (random) or 1 (pursuit) (got %d)", q.rollout_source);
    if (q.rollout_source == 1 && (!std::isfinite(q.rollout_dev) || q.rollout_dev < 0.0))
        return fail(RL_ERR_INVALID, "rl_mcts_create: rollout_dev must be finite and >= 0");
    g = q.source == RL_MCTS_FG ? g : nullptr;
    const SteerSource src = g ? SteerSource::followgap(g) : q.source == RL_MCTS_NN ? SteerSource::policy(p) : SteerSource();
    if (q.n_trees < 1 || q.max_nodes < 1 || q.action_every < 1 || q.rollout_steps < 1 || q.rollout_steps > MCTS_MAX_STEPS)
        return fail(RL_ERR_INVALID, "rl_mcts_create: n_trees >= 1, max_nodes >= 1, action_every >= 1 and 1 <= "
                    "rollout_steps <= %d required (got %d, %d, %d, %d)", MCTS_MAX_STEPS, q.n_trees, q.max_nodes,
                    q.action_every, q.rollout_steps);
    int rc = src.check("rl_mcts_create", c, h, (long)q.n_trees * q.rollout_steps, q.num_rays);      // (the roll-out scans)
    if (rc || (rc = src.fits("rl_mcts_create", c, q.n_trees, q.num_rays))) return rc;
    if ((long)q.n_trees * q.max_nodes >= (1L << 31) / 11)
        return fail(RL_ERR_INVALID, "rl_mcts_create: the node arrays (n_trees * max_nodes * 11) must stay below 2^31");
    std::unique_ptr<rl_mcts, decltype(&rl_mcts_destroy)> m(new (std::nothrow) rl_mcts(), rl_mcts_destroy);
    if (!m) return fail(RL_ERR_NOMEM, "out of host memory");
    m->c = c;
    m->h = h;
    m->src = src;
    m->prm = q;
    m->device = c->device;
    MctsParams &mp = m->mp;
    mp.P = c->P;
    if (g) mp.fg = g->P;
    mp.fg.size = q.num_rays;
    mp.K = q.n_trees;
    mp.N = q.max_nodes;
    mp.L = q.rollout_steps;
    mp.every = q.action_every;
    mp.n_act = (q.rollout_steps + q.action_every - 1) / q.action_every;
    mp.source = q.source;
    mp.speed = q.speed;
    mp.dt = q.dt;
    mp.scan_dist_to_base = q.scan_dist_to_base;
    mp.C = q.C;
    mp.crash_pen = q.crash_pen;
    mp.uni_dev = q.uni_dev;
    mp.max_steer = q.max_steer;
    mp.max_speed = q.max_speed;
    mp.crash_thresh = q.crash_thresh;
    const size_t K = q.n_trees, N = (size_t)q.n_trees * q.max_nodes, B = q.num_rays;
    if (hipSetDevice(m->device) != hipSuccess) return fail(RL_ERR_HIP, "rl_mcts_create: hipSetDevice failed");
    const size_t L = q.rollout_steps;
    for (DevPtr<int> *b : {&m->parent, &m->first_child, &m->next_sibling, &m->last_child, &m->n_children, &m->visits,
                           &m->child_visits, &m->terminal, &m->crash})
        if ((rc = b->ensure(N))) return rc;
    for (DevPtr<int> *b : {&m->n_nodes, &m->child, &m->exp_term, &m->first, &m->best_v, &m->best_n})
        if ((rc = b->ensure(K))) return rc;
    // (roots: 11 doubles of state, then one action, a tree)
    if ((rc = m->reward.ensure(N)) || (rc = m->action.ensure(N)) || (rc = m->state.ensure(N * 11)) || (rc = m->pose.ensure(N * 3)) ||
        (rc = m->answer.ensure(N)) || (rc = m->keys.ensure(K)) || (rc = m->mlp.ensure(K)) || (rc = m->best_a.ensure(K)) ||
        (rc = m->logtab.ensure((size_t)q.max_nodes + 1)) || (rc = m->cstate.ensure(K * 11)) || (rc = m->roots.ensure(K * 12)) ||
        (rc = m->cpose.ensure(K * 3)) || (rc = m->actions.ensure(K * mp.n_act * 2)) || (rc = m->ranges.ensure(K * B)) ||
        (rc = m->edge.ensure(B)) || (rc = m->rposes.ensure(K * L * 3)) || (rc = m->vel.ensure(K * L)))
        return rc;
    const std::vector<double> lt = mcts_log_table(q.max_nodes);
    if (hipMemcpy(m->logtab, lt.data(), lt.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(m->edge, edge, B * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return fail(RL_ERR_HIP, "rl_mcts_create: upload failed");
    *out = m.release();
    return RL_OK;
}

static PlanRoots plan_roots_of(rl_mcts *m);

// the act scans of the K nodes in m->cpose at ray offset `off`, the network for NN, then mcts_act_kernel on b and, for
// the track source, mcts_pursuit_answer_kernel behind it
static int mcts_act(rl_mcts *m, const Loop &lp, const MctsBufs &b, uint64_t off, int root, hipStream_t st)
{
    const LoopScan scan{m->cpose, m->prm.n_trees, m->prm.fov, m->prm.num_rays, m->ranges, m->mlp, 0, nullptr, nullptr};
    int rc = lp.scan_then(scan, off, mcts_act_table, MCTS_TREES, "mcts_act_kernel", st, m->mp, b, root);
    if (rc || m->prm.source != RL_MCTS_PURSUIT) return rc;
    // the track source: the node's answer is the pursuit of the tree's point from its own state
    const int K = m->prm.n_trees;
    return launch("mcts_pursuit_answer_kernel", mcts_pursuit_answer_kernel, dim3((K + 63) / 64), dim3(64), 0, st, m->mp, b,
                  plan_roots_of(m));
}

// the reward mode the planner runs: the attached track's; for explicit points alone the waypoint reward, or the mode
// kept by an attach without a track; else velocity
static int plan_mode(const rl_mcts *m)
{
    return m->track ? m->tp.mode : m->has_points ? m->points_mode : PLAN_VELOCITY;
}

static PlanRoots plan_roots_of(rl_mcts *m)
{
    return PlanRoots{m->tk_seg, m->tk_s, m->tk_goal, m->tk_point, m->tk_has};
}

// does the planner read the goal rule's lookahead: the waypoint reward and the track source without explicit points,
// the pursuit roll-outs always
static bool plan_needs_lookahead(const rl_mcts *m, int mode, bool points)
{
    return ((mode == PLAN_WAYPOINT || m->prm.source == RL_MCTS_PURSUIT) && !points) || m->prm.rollout_source == 1;
}

// what a reset, a run and a drive refuse of the track options before anything is launched
static int plan_args(const rl_mcts *m, const char *name)
{
    if (m->prm.source == RL_MCTS_PURSUIT && !m->track && !m->has_points)
        return fail(RL_ERR_INVALID, "%s: the track source needs a track (rl_mcts_attach_track) or explicit points", name);
    if (m->prm.rollout_source == 1 && !m->track)
        return fail(RL_ERR_INVALID, "%s: pursuit roll-outs need a track (rl_mcts_attach_track)", name);
    if (m->track && plan_needs_lookahead(m, PLAN_VELOCITY, m->has_points) &&
        (!std::isfinite(m->tp.lookahead) || !(m->tp.lookahead > 0.0)))
        return fail(RL_ERR_INVALID, "%s: the track source without explicit points and pursuit roll-outs need a finite "
                    "lookahead > 0", name);
    if (plan_mode(m) == PLAN_WAYPOINT && !m->has_points && (!std::isfinite(m->tp.lookahead) || !(m->tp.lookahead > 0.0)))
        return fail(RL_ERR_INVALID, "%s: the waypoint reward without explicit points needs a finite lookahead > 0", name);
    return RL_OK;
}

// plan_root_kernel over the K root states in m->roots, on st: at a reset, and behind every mcts_advance_kernel that
// wrote new roots.  A planner with neither track nor points launches nothing.
static int plan_roots(rl_mcts *m, hipStream_t st)
{
    if (!m->track && !m->has_points) return RL_OK;
    const int K = m->prm.n_trees;
    const TrackTable T = m->track ? track_table(m->track) : TrackTable{};
    return launch("plan_root_kernel", plan_root_kernel, dim3((K + MCTS_TREES - 1) / MCTS_TREES), dim3(64 * MCTS_TREES), 0, st, K, T,
                  m->tp, m->roots, m->has_points ? (const double *)m->tk_points : nullptr, plan_roots_of(m));
}

// how rl_mcts_reset and rl_mcts_drive begin: the keys go up to d_keys, the K root states and root (recent) actions into
// m->roots, then mcts_start_kernel makes the root nodes
static int mcts_start(rl_mcts *m, HostCall &hc, const MctsBufs &b, DevPtr<uint32_t> &d_keys, const std::vector<uint32_t> &keys,
                      const double *states, const double *actions)
{
    const size_t K = m->prm.n_trees;
    double *d_states = m->roots, *d_actions = d_states + K * 11;
    int rc;
    if ((rc = hc.up(d_keys, keys.data(), keys.size())) || (rc = hc.up(d_states, states, K * 11)) ||
        (rc = hc.up(d_actions, actions, K)) ||
        (rc = launch("mcts_start_kernel", mcts_start_kernel, dim3((K + 63) / 64), dim3(64), 0, hc.st, m->mp, b, d_states, d_actions)))
        return rc;
    return plan_roots(m, hc.st);
}

extern "C" int rl_mcts_reset(rl_mcts *m, const double *root_states, const double *root_actions, const uint64_t *seeds)
{
    if (!m || !root_states || !root_actions || !seeds) return fail(RL_ERR_INVALID, "rl_mcts_reset: null pointer");
    const int K = m->prm.n_trees;
    int rc = check_fan_args(m->h, K, m->prm.fov, m->prm.num_rays);
    if (rc) return rc;
    const Loop lp(&m->mu, m->c, m->h, m->src);
    if ((rc = plan_args(m, "rl_mcts_reset"))) return rc;
    HIPCHK(hipSetDevice(m->device));
    m->ready = false;
    std::vector<uint32_t> keys(K);
    for (int k = 0; k < K; ++k) keys[k] = noise_key(seeds[k]);
    const uint64_t base = lp.base;
    HostCall hc(m->c->stream);                                // (after `keys`: they stay until the call has drained)
    if ((rc = mcts_start(m, hc, mcts_bufs(m), m->keys, keys, root_states, root_actions)) ||
        (rc = mcts_act(m, lp, mcts_bufs(m), base, 1, hc.st)) || (rc = hc.finish()))
        return rc;
    m->base = base;
    m->iters = 0;
    m->ready = true;
    return RL_OK;
}

// iterations it0 ... it0 + n - 1 of every tree, enqueued on st: select, the act, the roll-outs and their crash
// test, the backup.  base: the ray offset of the trees' reset.  lp: the call's Loop; the caller has sized m->rranges.
// With a reward mode other than velocity the roll-outs also give their f64 positions, plan_term_kernel turns them into
// the terms, and the backup sums those.  rollout_source 1: rollout_pursuit_kernel stands where the roll-out kernel stood
// and hands over the same outputs.
static int mcts_iterations(rl_mcts *m, const Loop &lp, const MctsBufs &bufs, uint64_t base, long it0, int n, hipStream_t st)
{
    const int K = m->prm.n_trees, L = m->prm.rollout_steps, B = m->prm.num_rays;
    const bool terms = plan_mode(m) != PLAN_VELOCITY, pursuit = m->prm.rollout_source == 1;
    const TrackTable T = m->track ? track_table(m->track) : TrackTable{};
    PlanTrackParams tp = m->tp;
    tp.mode = plan_mode(m);
    MctsBufs b = bufs;
    if (terms) b.vel = m->terms;
    const uint64_t KB = (uint64_t)K * B, per_it = (uint64_t)K * (1 + L) * B;
    for (int t = 0; t < n; ++t) {
        const long it = it0 + t;
        const uint64_t off = base + KB + (uint64_t)it * per_it;
        int rc;
        if ((rc = launch("mcts_select_kernel", mcts_select_kernel, dim3((K + 63) / 64), dim3(64), 0, st, m->mp, b, (int)it)) ||
            (rc = mcts_act(m, lp, b, off, 0, st)) ||
            (rc = pursuit ? launch("rollout_pursuit_kernel", rollout_pursuit_kernel, dim3((K + MCTS_TREES - 1) / MCTS_TREES),
                                   dim3(64 * MCTS_TREES), 0, st, m->mp, b, T, m->tp, plan_roots_of(m), (int)it, m->prm.rollout_dev,
                                   m->rposes, m->vel, m->rxy)
                  : terms ? launch("rollout_xy_kernel", rollout_xy_kernel, dim3((K + 63) / 64), dim3(64), 0, st, m->c->P, m->cstate,
                                   m->actions, K, L, m->prm.action_every, m->prm.dt, m->rposes, m->vel, m->rxy)
                          : launch("rollout_kernel", rollout_kernel, dim3((K + 63) / 64), dim3(64), 0, st, m->c->P, m->cstate,
                                   m->actions, K, L, m->prm.action_every, m->prm.dt, m->rposes, nullptr, m->vel)) ||
            (terms && (rc = launch("plan_term_kernel", plan_term_kernel, dim3(K), dim3(64 * PLAN_TERM_WAVES), 0, st, T, tp, L,
                                   m->cstate, m->rxy, m->vel, plan_roots_of(m), m->terms, nullptr, nullptr, nullptr))) ||
            (rc = crash_groups_device(m->h, lp.at(off + KB), m->rposes, K, L, m->prm.fov, B, m->edge, m->prm.crash_thresh, m->first,
                                      m->rranges, st)) ||
            (rc = launch("mcts_backup_kernel", mcts_backup_kernel, dim3((K + 63) / 64), dim3(64), 0, st, m->mp, b)))
            return rc;
    }
    return RL_OK;
}

extern "C" int rl_mcts_run(rl_mcts *m, int n_iterations)
{
    if (!m) return fail(RL_ERR_INVALID, "rl_mcts_run: null pointer");
    if (n_iterations < 0) return fail(RL_ERR_INVALID, "rl_mcts_run: n_iterations must be >= 0 (got %d)", n_iterations);
    const Loop lp(&m->mu, m->c, m->h, m->src);
    int rc;
    if ((rc = plan_args(m, "rl_mcts_run"))) return rc;
    if (!m->ready) return fail(RL_ERR_INVALID, "rl_mcts_run: reset the planner first (rl_mcts_reset)");
    if (1 + m->iters + (long)n_iterations > m->prm.max_nodes)
        return fail(RL_ERR_INVALID, "rl_mcts_run: %d more iterations exceed max_nodes = %d (%ld done since reset)",
                    n_iterations, m->prm.max_nodes, m->iters);
    const int K = m->prm.n_trees, L = m->prm.rollout_steps, B = m->prm.num_rays;
    if ((rc = check_fan_args(m->h, K, m->prm.fov, B)) || (rc = check_fan_args(m->h, K * L, m->prm.fov, B))) return rc;
    if (n_iterations == 0) return RL_OK;
    HIPCHK(hipSetDevice(m->device));
    if ((rc = m->rranges.ensure((size_t)K * L * B))) return rc;
    hipStream_t st = m->c->stream;
    rc = mcts_iterations(m, lp, mcts_bufs(m), m->base, m->iters, n_iterations, st);
    const hipError_t e = hipStreamSynchronize(st);
    if (!rc && e != hipSuccess) rc = fail(RL_ERR_HIP, "rl_mcts_run: %s", hipGetErrorString(e));
    if (rc) {
        m->ready = false;                   // part of an iteration may have run: the trees need a reset
        return rc;
    }
    m->iters += n_iterations;
    return RL_OK;
}

// The closed loop of scripts/mcts_driver.py:207-264 (contract: include/scanlib.h).  Everything goes up before
// decision 0; between decisions the stream carries kernels only (mcts_advance_kernel ends one decision and writes
// the next one's roots), and the host waits once, for the downloads.
extern "C" int rl_mcts_drive(rl_mcts *m, const double *states_in, const double *recent_in, const uint64_t *seeds,
                             int n_decisions, int n_iterations, int steps_per_decision, double steer_clip, int *first,
                             double *states_out, double *recent_out, double *actions, int *visits,
                             double *trace_states_or_null)
{
    if (!m || !states_in || !recent_in || !seeds || !first || !states_out || !recent_out ||
        (n_decisions > 0 && (!actions || !visits)))
        return fail(RL_ERR_INVALID, "rl_mcts_drive: null pointer");
    if (n_decisions < 0) return fail(RL_ERR_INVALID, "rl_mcts_drive: n_decisions must be >= 0 (got %d)", n_decisions);
    if (n_iterations < 1) return fail(RL_ERR_INVALID, "rl_mcts_drive: n_iterations must be >= 1 (got %d)", n_iterations);
    if ((long)n_iterations + 1 > m->prm.max_nodes)
        return fail(RL_ERR_INVALID, "rl_mcts_drive: %d iterations exceed max_nodes = %d", n_iterations, m->prm.max_nodes);
    if (steps_per_decision < 1)
        return fail(RL_ERR_INVALID, "rl_mcts_drive: steps_per_decision must be >= 1 (got %d)", steps_per_decision);
    if (!(steer_clip >= 0.0)) return fail(RL_ERR_INVALID, "rl_mcts_drive: steer_clip must be >= 0 (0: no clamp)");
    const int K = m->prm.n_trees, L = m->prm.rollout_steps, B = m->prm.num_rays, D = n_decisions, I = n_iterations;
    int rc;
    if ((rc = check_fan_args(m->h, K, m->prm.fov, B)) || (rc = check_fan_args(m->h, K * L, m->prm.fov, B))) return rc;
    {
        std::lock_guard<std::mutex> lk(m->mu);
        if (m->has_points)
            return fail(RL_ERR_INVALID, "rl_mcts_drive: explicit points (rl_mcts_set_points) cannot be driven: attach a track, "
                        "which re-chooses the point at every decision");
        if ((rc = plan_args(m, "rl_mcts_drive"))) return rc;
    }
    if (D == 0) {
        for (int k = 0; k < K; ++k) first[k] = -1;
        if (states_out != states_in) memmove(states_out, states_in, (size_t)K * 11 * sizeof(double));
        if (recent_out != recent_in) memmove(recent_out, recent_in, (size_t)K * sizeof(double));
        return RL_OK;
    }
    const size_t rows = (size_t)K * D;
    const Loop lp(&m->mu, m->c, m->h, m->src);
    HIPCHK(hipSetDevice(m->device));
    std::vector<uint32_t> keys(rows);                  // [D][K]: decision d's seed is seeds[k] + d mod 2^64
    for (int d = 0; d < D; ++d)
        for (int k = 0; k < K; ++k) keys[(size_t)d * K + k] = noise_key(seeds[k] + (uint64_t)d);
    HostCall hc(m->c->stream);                         // (after `keys`: they stay until the call has drained)
    hipStream_t st = hc.st;
    if ((rc = hc.room(m->rranges, (size_t)K * L * B)) || (rc = hc.room(m->root_crash, K)) || (rc = hc.room(m->dr_first, K)) ||
        (rc = hc.room(m->dr_actions, rows)) || (rc = hc.room(m->dr_visits, rows)) ||
        (trace_states_or_null && (rc = hc.room(m->dr_trace, rows * 11))))
        return rc;
    m->ready = false;
    double *d_states = m->roots, *d_recent = d_states + (size_t)K * 11;
    MctsBufs b = mcts_bufs(m);
    b.root_crash = m->root_crash;
    const MctsDrive dv{d_states, d_recent, m->dr_first, m->dr_actions, m->dr_visits,
                       trace_states_or_null ? (double *)m->dr_trace : nullptr, D, steps_per_decision, steer_clip};
    const uint64_t stride = (uint64_t)K * B * (1 + (uint64_t)I * (1 + L));
    if ((rc = mcts_start(m, hc, b, m->dr_keys, keys, states_in, recent_in))) return rc;
    uint64_t base = lp.base;
    for (int d = 0; d < D; ++d) {
        base = lp.base + (uint64_t)d * stride;
        b.keys = m->dr_keys + (size_t)d * K;
        // (plan_roots: the next decision's roots, their segment, goal and point; a refused launch: the trees need a reset)
        if ((rc = mcts_act(m, lp, b, base, 1, st)) || (rc = mcts_iterations(m, lp, b, base, 0, I, st)) ||
            (rc = launch("mcts_advance_kernel", mcts_advance_kernel, dim3((K + 63) / 64), dim3(64), 0, st, m->mp, b, dv, d)) ||
            (d + 1 < D && (rc = plan_roots(m, st))))
            return rc;
    }
    // the planner keeps the last decision's trees: its keys, ray offset and iteration count are that decision's
    HIPCHK(hipMemcpyAsync(m->keys, b.keys, (size_t)K * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    if ((rc = hc.down(first, m->dr_first, K)) || (rc = hc.down(states_out, (const double *)d_states, (size_t)K * 11)) ||
        (rc = hc.down(recent_out, (const double *)d_recent, K)) || (rc = hc.down(actions, m->dr_actions, rows)) ||
        (rc = hc.down(visits, m->dr_visits, rows)) || (rc = hc.down(trace_states_or_null, m->dr_trace, rows * 11)) ||
        (rc = hc.finish()))
        return rc;
    m->base = base;
    m->iters = I;
    m->ready = true;
    return RL_OK;
}

extern "C" int rl_mcts_best(rl_mcts *m, double *actions, int *visits, int *n_nodes)
{
    if (!m || !actions || !visits || !n_nodes) return fail(RL_ERR_INVALID, "rl_mcts_best: null pointer");
    std::scoped_lock lk(m->mu, m->c->mu);
    if (!m->ready) return fail(RL_ERR_INVALID, "rl_mcts_best: reset the planner first (rl_mcts_reset)");
    HIPCHK(hipSetDevice(m->device));
    HostCall hc(m->c->stream);
    const int K = m->prm.n_trees;
    int rc;
    if ((rc = launch("mcts_best_kernel", mcts_best_kernel, dim3((K + 63) / 64), dim3(64), 0, hc.st, m->mp, mcts_bufs(m), m->best_a,
                     m->best_v, m->best_n)) ||
        (rc = hc.down(actions, m->best_a, K)) || (rc = hc.down(visits, m->best_v, K)) || (rc = hc.down(n_nodes, m->best_n, K)))
        return rc;
    return hc.finish();
}

extern "C" int rl_mcts_read_tree(rl_mcts *m, int tree, int *parent, int *first_child, int *next_sibling,
                                 int *n_children, int *visits, int *child_visits, double *reward, double *action,
                                 int *terminal, double *state, float *scan_pose, float *answer, int *crash,
                                 int *n_nodes_out)
{
    if (!m || !n_nodes_out) return fail(RL_ERR_INVALID, "rl_mcts_read_tree: null pointer");
    if (tree < 0 || tree >= m->prm.n_trees)
        return fail(RL_ERR_INVALID, "rl_mcts_read_tree: tree %d outside [0, %d)", tree, m->prm.n_trees);
    std::scoped_lock lk(m->mu, m->c->mu);
    if (!m->ready) return fail(RL_ERR_INVALID, "rl_mcts_read_tree: reset the planner first (rl_mcts_reset)");
    HIPCHK(hipSetDevice(m->device));
    HostCall hc(m->c->stream);
    int n = 0, rc;
    if ((rc = hc.down(&n, m->n_nodes + tree, 1))) return rc;
    HIPCHK(hipStreamSynchronize(hc.st));
    n = std::min(std::max(n, 0), m->prm.max_nodes);
    // the tree's first n nodes of an array of `per` scalars a node, when the caller wants it
    const size_t t0 = (size_t)tree * m->prm.max_nodes;
    const auto rows = [&](auto *dst, const auto &src, size_t per) {
        return n > 0 ? hc.down(dst, src + t0 * per, (size_t)n * per) : (int)RL_OK;
    };
    if ((rc = rows(parent, m->parent, 1)) || (rc = rows(first_child, m->first_child, 1)) ||
        (rc = rows(next_sibling, m->next_sibling, 1)) || (rc = rows(n_children, m->n_children, 1)) ||
        (rc = rows(visits, m->visits, 1)) || (rc = rows(child_visits, m->child_visits, 1)) || (rc = rows(reward, m->reward, 1)) ||
        (rc = rows(action, m->action, 1)) || (rc = rows(terminal, m->terminal, 1)) || (rc = rows(state, m->state, 11)) ||
        (rc = rows(scan_pose, m->pose, 3)) || (rc = rows(answer, m->answer, 1)) || (rc = rows(crash, m->crash, 1)) ||
        (rc = hc.finish()))
        return rc;
    *n_nodes_out = n;
    return RL_OK;
}

extern "C" int rl_mcts_probe_ucb(int device, const double *reward, const int *visits, const int *sum, size_t n,
                                 double C, double *out)
{
    if (n > 0 && (!reward || !visits || !sum || !out)) return fail(RL_ERR_INVALID, "rl_mcts_probe_ucb: null pointer");
    int s_max = 1;
    for (size_t i = 0; i < n; ++i) {
        if (visits[i] < 1 || sum[i] < 1 || sum[i] > (1 << 24))
            return fail(RL_ERR_INVALID, "rl_mcts_probe_ucb: visits >= 1 and 1 <= sum <= 2^24 required (entry %zu)", i);
        s_max = std::max(s_max, sum[i]);
    }
    int rc = check_device(device);
    if (rc || n == 0) return rc;
    HIPCHK(hipSetDevice(device));
    const std::vector<double> lt = mcts_log_table(s_max);
    DevBuf dr, dv, ds, dl, dout;
    if ((rc = dr.ensure(n * 8)) || (rc = dv.ensure(n * 4)) || (rc = ds.ensure(n * 4)) || (rc = dl.ensure(lt.size() * 8)) ||
        (rc = dout.ensure(n * 8)))
        return rc;
    if (hipMemcpy(dr.p, reward, n * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dv.p, visits, n * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ds.p, sum, n * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dl.p, lt.data(), lt.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
        return fail(RL_ERR_HIP, "rl_mcts_probe_ucb: upload failed");
    const int grid = (int)std::min<size_t>((n + 255) / 256, 4096);
    if ((rc = launch("mcts_ucb_probe_kernel", mcts_ucb_probe_kernel, dim3(grid), dim3(256), 0, nullptr, (const double *)dr.p,
                     (const int *)dv.p, (const int *)ds.p, (const double *)dl.p, (long)n, C, (double *)dout.p)))
        return rc;
    if (hipMemcpy(out, dout.p, n * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(RL_ERR_HIP, "rl_mcts_probe_ucb: kernel or download failed");
    return RL_OK;
}

// ---------------------------------------------------------------- track-guided planning (plan_track_kernels.h)
// what rl_mcts_attach_track and rl_car_rollout_track refuse of *p (contract: include/scanlib_track_plan.h); `points`:
// explicit points stand in for the goal rule
static int plan_track_args(const char *name, const rl_plan_track_params *p, bool points)
{
    if (!p) return fail(RL_ERR_INVALID, "%s: null params", name);
    if (p->reward_mode < PLAN_VELOCITY || p->reward_mode > PLAN_PROGRESS)
        return fail(RL_ERR_INVALID, "%s: reward_mode must be 0, 1 or 2 (got %d)", name, p->reward_mode);
    if (p->window < 0 || p->window > 65536 || p->goal_span < 0 || p->goal_span > 65536)
        return fail(RL_ERR_INVALID, "%s: window and goal_span must lie in [0, 65536] (got %d, %d)", name, p->window,
                    p->goal_span);
    if (p->reward_mode == PLAN_WAYPOINT && !points && (!std::isfinite(p->lookahead) || !(p->lookahead > 0.0)))
        return fail(RL_ERR_INVALID, "%s: the waypoint reward without explicit points needs a finite lookahead > 0", name);
    return RL_OK;
}

extern "C" int rl_mcts_attach_track(rl_mcts *m, rl_track *t, const rl_plan_track_params *p)
{
    if (!m) return fail(RL_ERR_INVALID, "rl_mcts_attach_track: null pointer");
    std::scoped_lock lk(m->mu, m->c->mu);
    if (t) {
        int rc = plan_track_args("rl_mcts_attach_track", p, m->has_points);
        if (rc) return rc;
        if (plan_needs_lookahead(m, PLAN_VELOCITY, m->has_points) && (!std::isfinite(p->lookahead) || !(p->lookahead > 0.0)))
            return fail(RL_ERR_INVALID, "rl_mcts_attach_track: the track source without explicit points and pursuit roll-outs "
                        "need a finite lookahead > 0");
        if (t->device != m->device)
            return fail(RL_ERR_INVALID, "rl_mcts_attach_track: track (device %d) and planner (device %d) must share one device",
                        t->device, m->device);
        HIPCHK(hipSetDevice(m->device));
        const size_t K = m->prm.n_trees, L = m->prm.rollout_steps;
        if ((rc = m->tk_seg.ensure(K)) || (rc = m->tk_s.ensure(K)) || (rc = m->tk_goal.ensure(K)) ||
            (rc = m->tk_point.ensure(K * 2)) || (rc = m->tk_has.ensure(K)) || (rc = m->rxy.ensure(K * L * 2)) ||
            (rc = m->terms.ensure(K * L)))
            return rc;
        m->tp = PlanTrackParams{p->reward_mode, p->window, p->goal_span, p->lookahead};
    } else if (p && p->reward_mode != PLAN_VELOCITY && p->reward_mode != PLAN_WAYPOINT) {
        return fail(RL_ERR_INVALID, "rl_mcts_attach_track: without a track reward_mode must be 0 or 1 (got %d)", p->reward_mode);
    }
    if (!t) m->points_mode = p ? p->reward_mode : PLAN_WAYPOINT;     // (explicit points alone: the waypoint reward unless told)
    m->track = t;
    m->ready = false;                   // the roots of the new track are found at the next reset
    return RL_OK;
}

extern "C" int rl_mcts_set_points(rl_mcts *m, const double *xy_k2_or_null)
{
    if (!m) return fail(RL_ERR_INVALID, "rl_mcts_set_points: null pointer");
    std::scoped_lock lk(m->mu, m->c->mu);
    if (xy_k2_or_null) {
        HIPCHK(hipSetDevice(m->device));
        const size_t K = m->prm.n_trees, L = m->prm.rollout_steps;
        int rc;
        if ((rc = m->tk_points.ensure(K * 2)) || (rc = m->tk_seg.ensure(K)) || (rc = m->tk_s.ensure(K)) ||
            (rc = m->tk_goal.ensure(K)) || (rc = m->tk_point.ensure(K * 2)) || (rc = m->tk_has.ensure(K)) ||
            (rc = m->rxy.ensure(K * L * 2)) || (rc = m->terms.ensure(K * L)))
            return rc;
        HostCall hc(m->c->stream);      // (the planner's launches read the points on this stream)
        if ((rc = hc.up((double *)m->tk_points, xy_k2_or_null, K * 2)) || (rc = hc.finish())) return rc;
    }
    m->has_points = xy_k2_or_null != nullptr;
    m->ready = false;
    return RL_OK;
}

extern "C" int rl_mcts_read_track(rl_mcts *m, int *segment, double *s, int *goal, double *point_k2)
{
    if (!m) return fail(RL_ERR_INVALID, "rl_mcts_read_track: null pointer");
    std::scoped_lock lk(m->mu, m->c->mu);
    if (!m->track && !m->has_points)
        return fail(RL_ERR_INVALID, "rl_mcts_read_track: no track attached and no points set (rl_mcts_attach_track)");
    if (!m->ready) return fail(RL_ERR_INVALID, "rl_mcts_read_track: reset the planner first (rl_mcts_reset)");
    HIPCHK(hipSetDevice(m->device));
    HostCall hc(m->c->stream);
    const size_t K = m->prm.n_trees;
    int rc;
    if ((rc = hc.down(segment, m->tk_seg, K)) || (rc = hc.down(s, m->tk_s, K)) || (rc = hc.down(goal, m->tk_goal, K)) ||
        (rc = hc.down(point_k2, m->tk_point, K * 2)))
        return rc;
    return hc.finish();
}

extern "C" int rl_car_rollout_track(rl_car *c, rl_track *t, const rl_plan_track_params *p, const double *states,
                                    const double *actions, int R, int n_steps, int every, double dt,
                                    const int *anchor_segment_or_null, const double *points_or_null, double *terms,
                                    double *s_or_null, int *segment_or_null, double *start_s_or_null)
{
    if (!c || (R > 0 && (!states || !actions || !terms))) return fail(RL_ERR_INVALID, "rl_car_rollout_track: null pointer");
    if (!c->reps.empty()) return fail(RL_ERR_INVALID, "rl_car_rollout_track is single-device only: pass an ordinary car handle");
    int rc = plan_track_args("rl_car_rollout_track", p, points_or_null != nullptr);
    if (rc || (rc = check_rollout_args(R, n_steps, every))) return rc;
    if (n_steps > MCTS_MAX_STEPS)
        return fail(RL_ERR_INVALID, "rl_car_rollout_track: n_steps must not exceed %d (got %d)", MCTS_MAX_STEPS, n_steps);
    const int mode = p->reward_mode;
    if (!t && (mode == PLAN_PROGRESS || (mode == PLAN_WAYPOINT && !points_or_null)))
        return fail(RL_ERR_INVALID, "rl_car_rollout_track: reward_mode %d needs a track%s", mode,
                    mode == PLAN_WAYPOINT ? " or explicit points" : "");
    if (t && t->device != c->device)
        return fail(RL_ERR_INVALID, "rl_car_rollout_track: track (device %d) and car (device %d) must share one device",
                    t->device, c->device);
    const bool anchors = mode == PLAN_PROGRESS && anchor_segment_or_null, points = mode == PLAN_WAYPOINT && points_or_null;
    if (anchors)
        for (int r = 0; r < R; ++r)
            if (anchor_segment_or_null[r] < 0 || anchor_segment_or_null[r] >= t->S)
                return fail(RL_ERR_INVALID, "rl_car_rollout_track: anchor segment %d of roll-out %d lies outside [0, %d)",
                            anchor_segment_or_null[r], r, t->S);
    std::lock_guard<std::mutex> lk(c->mu);
    HostCall hc(c->stream);
    const size_t n = (size_t)std::max(R, 0), rows = n * n_steps;
    HIPCHK(hipSetDevice(c->device));
    if (R == 0) return RL_OK;
    if ((rc = hc.room(c->tk_xy, rows * 2)) || (rc = hc.room(c->tk_terms, rows)) || (rc = hc.room(c->tk_s, rows)) ||
        (rc = hc.room(c->tk_seg, rows)) || (rc = hc.room(c->tk_start_s, n)) || (rc = hc.room(c->tk_root_seg, n)) ||
        (rc = hc.room(c->tk_root_s, n)) || (rc = hc.room(c->tk_goal, n)) || (rc = hc.room(c->tk_point, n * 2)) ||
        (rc = hc.room(c->tk_has, n)) || (points && (rc = hc.up(c->tk_points_in, points_or_null, n * 2))) ||
        (rc = car_rollout_device(c, hc, states, actions, R, n_steps, every, dt, false, true, c->tk_xy)))
        return rc;
    // the roots of the roll-outs: their start states (c->states, uploaded above); the caller's anchors replace the search's
    const TrackTable T = t ? track_table(t) : TrackTable{};
    const PlanTrackParams tp{mode, p->window, p->goal_span, p->lookahead};
    const PlanRoots roots{c->tk_root_seg, c->tk_root_s, c->tk_goal, c->tk_point, c->tk_has};
    const bool progress = mode == PLAN_PROGRESS;
    if ((rc = launch("plan_root_kernel", plan_root_kernel, dim3((R + MCTS_TREES - 1) / MCTS_TREES), dim3(64 * MCTS_TREES), 0, hc.st, R,
                     T, tp, c->states, points ? (const double *)c->tk_points_in : nullptr, roots)) ||
        (anchors && (rc = hc.up((int *)c->tk_root_seg, anchor_segment_or_null, n))) ||
        (rc = launch("plan_term_kernel", plan_term_kernel, dim3(R), dim3(64 * PLAN_TERM_WAVES), 0, hc.st, T, tp, n_steps, c->states,
                     c->tk_xy, c->vel, roots, c->tk_terms, c->tk_s, c->tk_seg, c->tk_start_s)) ||
        (rc = hc.down(terms, c->tk_terms, rows)) || (rc = hc.down(progress ? s_or_null : nullptr, c->tk_s, rows)) ||
        (rc = hc.down(progress ? segment_or_null : nullptr, c->tk_seg, rows)) ||
        (rc = hc.down(progress ? start_s_or_null : nullptr, c->tk_start_s, n)))
        return rc;
    return hc.finish();
}
