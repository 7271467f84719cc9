// plan_track_kernels.h — the track in the MCTS planner and in the roll-outs (include/scanlib_track_plan.h): a per-step
// reward term for every roll-out, either the reference's waypoint reward (mcts.py:233-234) or the track progress of the
// step, from the table of track_kernels.h and with its search, compare and wrap (track_window, track_nearest,
// track_goal, track_wrap; nothing of them is restated here).
//   plan_root_kernel   one wave per tree (MCTS_TREES a workgroup, no barrier): the nearest segment of the root position
//                      over ALL segments, its s, the goal waypoint and the tree's track point.  Behind mcts_start_kernel
//                      at a reset and behind mcts_advance_kernel at every decision of the drive: the roots never leave
//                      the device.  rl_car_rollout_track runs it over the roll-outs' start states.
//   rollout_xy_kernel  rollout_kernel's lane with the f64 (x, y) behind every pose as a further output.
//   plan_term_kernel   one workgroup of PLAN_TERM_WAVES waves per roll-out, between rollout_xy_kernel (which hands over
//                      the f64 positions) and the backup, which reads the terms where it read the velocities.
//                      Progress: wave w takes positions w, w + 16, ... of the L + 1 (the start state, then every step);
//                      its lanes stride over the tree's candidate segments and the wave minimum gives s_i, which goes to
//                      LDS (L + 1 doubles, 4104 bytes at L = 512); after the one barrier thread i writes
//                      wrap(s_i - s_(i-1)).  The candidates are the tree's (the window around the root's segment), the same
//                      for every step, so the steps are independent and no lane walks steps x segments.  The lowest index
//                      wins among equal d2, so the result does not depend on which wave or lane saw a candidate.
//                      Waypoint and velocity: one thread per step.
// The table stays in global memory for the reasons at the top of track_kernels.h; here every workgroup reads the same
// candidates L + 1 times, which L2 serves.  Cost without a window: (L + 1) S projections a roll-out, about 20 f64
// operations (a division among them) and 40 bytes each.  A 65536-point track at L = 200 is 13.2 M projections and 527 MB
// of L2 reads per roll-out and iteration, against 200 x 1081 rays of its scans: long tracks want a window (window = 64
// is 129 candidates, 26 k projections a roll-out).
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "mcts_kernels.h"
#include "track_kernels.h"

namespace scan {

constexpr int PLAN_TERM_WAVES = 16;     // (4 waves: a lone roll-out on 4096 segments took 2.1 x as long, K = 1024 the same)
enum : int { PLAN_VELOCITY = 0, PLAN_WAYPOINT = 1, PLAN_PROGRESS = 2 };

struct PlanTrackParams {
    int mode, window, goal_span;
    double lookahead;
};

// per tree (or roll-out): the root's nearest segment, its s, the goal waypoint (-1: none), the track point and whether
// there is one (a goal, or the caller's explicit point)
struct PlanRoots {
    int *seg;
    double *s;
    int *goal;
    double *point;                     // [n][2]
    int *has;
};

// s of (cx, cy) on segment seg
__device__ inline double plan_arc(const TrackTable &T, int seg, double cx, double cy)
{
    double t;
    track_project(T, seg, cx, cy, &t);
    return T.cum[seg] + t * T.len[seg];
}

// rollout_kernel with the f64 (x, y) behind every pose as well (xy_out [R][n_steps][2]): what the track terms of
// plan_track_kernels.h are computed from.  A kernel of its own: as one more nullable output of rollout_kernel the stores
// cost that kernel six VGPRs and a wave per SIMD at every call site, and as a template instance its schedule changed
// (+1.5 % on a lone tree's iteration, which is this one lane's 200 serial steps).
__global__ __launch_bounds__(64) void rollout_xy_kernel(CarParams P, const double *__restrict__ states_in,
                                                        const double *__restrict__ actions,
                                                        int n_rollouts, int n_steps, int action_every,
                                                        double dt, float *__restrict__ poses_out,
                                                        double *__restrict__ velocities_out,
                                                        double *__restrict__ xy_out)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rollouts) return;
    CarState cs = drive_load_state(states_in + (size_t)r * 11);
    const int n_act = (n_steps + action_every - 1) / action_every;
    double speed = 0.0, steer = 0.0;
    for (int i = 0; i < n_steps; ++i) {
        if (i % action_every == 0) {
            const double *a = actions + ((size_t)r * n_act + i / action_every) * 2;
            speed = a[0];
            steer = a[1];
        }
        car_step(P, cs, speed, steer, dt);
        const size_t at = (size_t)r * n_steps + i;
        poses_out[3 * at + 0] = (float)cs.x;
        poses_out[3 * at + 1] = (float)cs.y;
        poses_out[3 * at + 2] = (float)cs.theta;
        velocities_out[at] = cs.velocity;
        xy_out[2 * at + 0] = cs.x;
        xy_out[2 * at + 1] = cs.y;
    }
}

// state: [n][11]; points: the explicit points [n][2] or null.  T.S == 0: no track (explicit points alone).
__global__ __launch_bounds__(64 * MCTS_TREES) void plan_root_kernel(int n, TrackTable T, PlanTrackParams tp,
                                                                    const double *__restrict__ state,
                                                                    const double *__restrict__ points, PlanRoots r)
{
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = blockIdx.x * MCTS_TREES + w;
    if (k >= n) return;                                         // (wave-uniform; no barrier below)
    int seg = -1, goal = -1;
    double s = __builtin_nan(""), px = 0.0, py = 0.0;
    if (T.S > 0) {
        const double cx = state[(size_t)k * 11 + 0], cy = state[(size_t)k * 11 + 1];
        seg = track_nearest(T, 0, T.S, cx, cy, lane);
        s = plan_arc(T, seg, cx, cy);
        goal = track_goal(T, tp.lookahead, tp.goal_span, seg, cx, cy, lane);
        if (goal >= 0) px = T.x[goal], py = T.y[goal];
    }
    int has = goal >= 0;
    if (points) px = points[2 * (size_t)k], py = points[2 * (size_t)k + 1], has = 1;
    if (lane != 0) return;
    r.seg[k] = seg;
    r.s[k] = s;
    r.goal[k] = goal;
    r.point[2 * (size_t)k + 0] = px;
    r.point[2 * (size_t)k + 1] = py;
    r.has[k] = has;
}

// start: the roll-outs' start states [R][11]; xy [R][L][2] and vel [R][L] from rollout_kernel; terms [R][L]; s_out,
// seg_out [R][L] and start_s [R] are optional and written in the progress mode only.  L <= MCTS_MAX_STEPS.
__global__ __launch_bounds__(64 * PLAN_TERM_WAVES) void plan_term_kernel(TrackTable T, PlanTrackParams tp, int L,
                                                                         const double *__restrict__ start,
                                                                         const double *__restrict__ xy,
                                                                         const double *__restrict__ vel, PlanRoots r,
                                                                         double *__restrict__ terms,
                                                                         double *__restrict__ s_out,
                                                                         int *__restrict__ seg_out,
                                                                         double *__restrict__ start_s)
{
    __shared__ double sh_s[MCTS_MAX_STEPS + 1];
    const int k = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t row = (size_t)k * L;
    const double *p = xy + 2 * row;
    if (tp.mode != PLAN_PROGRESS) {                             // (uniform over the workgroup)
        const bool waypoint = tp.mode == PLAN_WAYPOINT && r.has[k];
        const double px = r.point[2 * (size_t)k], py = r.point[2 * (size_t)k + 1];
        for (int i = threadIdx.x; i < L; i += 64 * PLAN_TERM_WAVES) {
            double term = vel[row + i];
            if (waypoint) {
                const double ex = px - p[2 * i], ey = py - p[2 * i + 1];
                term = term / sqrt(ex * ex + ey * ey);
            }
            terms[row + i] = term;
        }
        return;
    }
    int first, count;
    track_window(T, tp.window, r.seg[k], first, count);
    for (int j = w; j <= L; j += PLAN_TERM_WAVES) {             // position j: the start state, then step j - 1
        const double cx = j == 0 ? start[(size_t)k * 11 + 0] : p[2 * (j - 1)];
        const double cy = j == 0 ? start[(size_t)k * 11 + 1] : p[2 * (j - 1) + 1];
        const int seg = track_nearest(T, first, count, cx, cy, lane);
        const double s = plan_arc(T, seg, cx, cy);
        if (lane != 0) continue;
        sh_s[j] = s;
        if (j == 0) {
            if (start_s) start_s[k] = s;
        } else {
            if (s_out) s_out[row + j - 1] = s;
            if (seg_out) seg_out[row + j - 1] = seg;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < L; i += 64 * PLAN_TERM_WAVES) {
        double d = sh_s[i + 1] - sh_s[i];
        track_wrap(T, d);
        terms[row + i] = d;
    }
}

}  // namespace scan
