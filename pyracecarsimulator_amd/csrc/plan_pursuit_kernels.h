// plan_pursuit_kernels.h — the track steering the MCTS planner (include/scanlib.h, "the pursuit steer", RL_MCTS_PURSUIT
// and rl_mcts_params.rollout_source): where plan_track_kernels.h scores roll-outs along the track, these two kernels
// drive along it, with the table, search and goal rule of track_kernels.h (track_window, track_nearest, track_goal) and
// the one statement of pursuit_device.h.  The planner's other kernels do not know about them.
//   mcts_pursuit_answer_kernel  one lane per tree, behind mcts_act_kernel for the source RL_MCTS_PURSUIT only: the new
//                               node's (or root's) stored expansion answer becomes the pursuit of the tree's track
//                               point (PlanRoots) from the node's own state; 0.0f for a tree without a point.
//   rollout_pursuit_kernel      rollout_xy_kernel's outputs with the steer of every action taken from the track.  One
//                               WAVE per roll-out (MCTS_TREES a workgroup, no barrier): rollout_kernel's one lane per
//                               roll-out is one wave on the whole device at K = 64, so the 63 idle lanes of each
//                               roll-out's wave do the searches.  Per action the lanes stride over the candidate
//                               segments, then over the candidate waypoints (wave minima by __shfl_xor, no LDS); lane 0
//                               runs the f64 car steps of the action and the wave-uniform (x, y, theta) goes back to
//                               every lane with three __shfl from lane 0.  All branches around the searches are
//                               wave-uniform (they depend on m, the tree and broadcast values only).
// Cost per roll-out: the L dependent car steps of rollout_kernel plus, per action, (candidate segments + candidate
// waypoints) / 64 lane passes of about 20 f64 operations each; without a window or a goal span that is the whole table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plan_track_kernels.h"
#include "pursuit_device.h"

namespace scan {

__global__ __launch_bounds__(64) void mcts_pursuit_answer_kernel(MctsParams p, MctsBufs b, PlanRoots r)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= p.K) return;
    const int c = b.child[k];
    if (c < 0) return;
    const size_t n = (size_t)k * p.N + c;
    const double *s = b.state + 11 * n;
    float ans = 0.0f;
    if (r.has[k]) ans = pursuit_steer(p.P.WB, p.max_steer, s[0], s[1], s[2], r.point[2 * (size_t)k], r.point[2 * (size_t)k + 1]);
    b.answer[n] = ans;
}

// iteration `it` of tree k: the roll-out from b.cstate with the speeds of b.actions (mcts_select_kernel drew them) and,
// for action m, steer = clamp(pursuit(state, goal point) + uniform(-dev, dev; the draw d = 1 + 2m), +-max_steer).
// poses_out [K][L][3], vel_out [K][L], xy_out [K][L][2]: what rollout_xy_kernel writes.
__global__ __launch_bounds__(64 * MCTS_TREES) void rollout_pursuit_kernel(MctsParams p, MctsBufs b, TrackTable T,
                                                                          PlanTrackParams tp, PlanRoots r, int it, double dev,
                                                                          float *__restrict__ poses_out,
                                                                          double *__restrict__ vel_out,
                                                                          double *__restrict__ xy_out)
{
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = blockIdx.x * MCTS_TREES + w;
    if (k >= p.K) return;                                       // (wave-uniform; no barrier below)
    CarState cs = drive_load_state(b.cstate + 11 * (size_t)k);
    const uint32_t key = b.keys[k];
    const double *act = b.actions + (size_t)k * p.n_act * 2;
    double cx = cs.x, cy = cs.y, th = cs.theta;
    int seg = r.seg[k];                                         // the root's segment, then the one the last action found
    for (int m = 0; m < p.n_act; ++m) {
        int first, count;
        track_window(T, tp.window, seg, first, count);
        seg = track_nearest(T, first, count, cx, cy, lane);
        const int goal = track_goal(T, tp.lookahead, tp.goal_span, seg, cx, cy, lane);
        double base = 0.0;
        if (goal >= 0) base = (double)pursuit_steer(p.P.WB, p.max_steer, cx, cy, th, T.x[goal], T.y[goal]);
        const double u = mcts_uniform01(key, 1u + 2u * m, (uint32_t)it);
        const double steer = fmin(fmax(base + mcts_uniform(-dev, dev, u), -p.max_steer), p.max_steer);
        const double speed = act[2 * m];
        const int i0 = m * p.every, n = min(p.every, p.L - i0);
        if (lane == 0) {
            for (int i = i0; i < i0 + n; ++i) {
                car_step(p.P, cs, speed, steer, p.dt);
                const size_t at = (size_t)k * p.L + i;
                poses_out[3 * at + 0] = (float)cs.x;
                poses_out[3 * at + 1] = (float)cs.y;
                poses_out[3 * at + 2] = (float)cs.theta;
                vel_out[at] = cs.velocity;
                xy_out[2 * at + 0] = cs.x;
                xy_out[2 * at + 1] = cs.y;
            }
        }
        cx = __shfl(cs.x, 0);
        cy = __shfl(cs.y, 0);
        th = __shfl(cs.theta, 0);
    }
}

}  // namespace scan
