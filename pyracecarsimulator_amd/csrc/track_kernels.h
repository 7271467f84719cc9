// track_kernels.h — track progress of the driving and race environments (include/scanlib.h "track progress"): where
// every car is on a polyline of W waypoints, how far it came along it this call, its laps, the lookahead waypoint in
// the car's frame and, in a race, its position.  One kernel, enqueued after phase B of every reset and step of an env
// with a track attached (abi_car.hip); the env kernels do not know about it.
//   track_kernel<false>   DRIVE_CARS envs per workgroup, one wave each, no barrier
//   track_kernel<true>    one workgroup per race, one wave per car (blockDim = 64 P as race_env_observe_kernel): the
//                         spawn offset against car 0 and the rank meet in LDS
// A wave's lanes stride over the candidate segments, then over the candidate waypoints, each lane keeping its own
// (value, index) minimum; a butterfly of lexicographic compares leaves the wave's minimum, the lowest index among exact
// ties, in every lane; lane 0 finishes the row.
// The table stays in global memory.  A wave reads every candidate's five doubles once, lane-contiguous (whole lines),
// and the eight waves of a workgroup are the only reuse a staged copy would have: staging costs the copy itself per
// workgroup and per call, the same bytes through L2 plus an LDS write and a barrier, and a table of 65536 points (3.5 MiB)
// does not fit in LDS at all.  With a window the candidates differ per car and there is no reuse.  Per candidate there
// are about 20 f64 operations, a division among them, to 40 bytes read (docs/history/track.md has the figures).
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "drive_kernels.h"
#include "env_kernels.h"
#include "race_kernels.h"

namespace scan {

// the track's table, structure of arrays (rl_track_create fills it on the host): points x, y [W]; per segment dx, dy,
// q = dx dx + dy dy, len = sqrt(q) [S]; cum [S + 1]; L = cum[S]
struct TrackTable {
    const double *x, *y, *dx, *dy, *q, *len, *cum;
    int W, S, closed;
    double L;
};

struct TrackParams {
    int window, goal_span, reward_mode, group;
    double lookahead;
};

// per env: st [N, 3] = (s_prev, progress, offset); rows [N, 8] f32 and ints [N, 4] as the caller reads them
struct TrackBufs {
    double *st;
    float *rows;
    int *ints;
};

enum : int { TRACK_SEGMENT = 0, TRACK_GOAL = 1, TRACK_LAPS = 2, TRACK_RANK = 3 };

// (v, i) < (bv, bi) lexicographically; a NaN v never wins
__device__ inline bool track_less(double v, int i, double bv, int bi) { return v < bv || (v == bv && i < bi); }

// the wave's lexicographic minimum of (v, i), in every lane
__device__ inline void track_wave_min(double &v, int &i)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(v, m);
        const int oi = __shfl_xor(i, m);
        if (track_less(ov, oi, v, i)) v = ov, i = oi;
    }
}

// the projection of (cx, cy) onto segment i: d2, and t where asked for
__device__ inline double track_project(const TrackTable &T, int i, double cx, double cy, double *t_out)
{
    const double dx = T.dx[i], dy = T.dy[i];
    const double ax = cx - T.x[i], ay = cy - T.y[i];
    const double u = ax * dx + ay * dy;
    const double t = fmin(fmax(u / T.q[i], 0.0), 1.0);
    const double ex = ax - t * dx, ey = ay - t * dy;
    if (t_out) *t_out = t;
    return ex * ex + ey * ey;
}

// the ±L rule of a closed track: a difference of arc lengths taken the short way round; returns the lap it crossed
__device__ inline int track_wrap(const TrackTable &T, double &d)
{
    if (!T.closed) return 0;
    const double half = 0.5 * T.L;
    if (d < -half) {
        d += T.L;
        return 1;
    }
    if (d > half) {
        d -= T.L;
        return -1;
    }
    return 0;
}

// the candidate segments of a search around segment p: `count` of them from `first`, wrapping on a closed track; all
// of them when window == 0 or once 2 window + 1 >= S
__device__ inline void track_window(const TrackTable &T, int window, int p, int &first, int &count)
{
    first = 0;
    count = T.S;
    if (window <= 0 || 2 * window + 1 >= T.S) return;
    if (T.closed) {
        first = p - window;
        if (first < 0) first += T.S;
        count = 2 * window + 1;
    } else {
        first = max(p - window, 0);
        count = min(p + window, T.S - 1) - first + 1;
    }
}

// the nearest of the candidate segments to (cx, cy), the lowest index among equal d2, in every lane of the wave
__device__ inline int track_nearest(const TrackTable &T, int first, int count, double cx, double cy, int lane)
{
    double bv = INFINITY;
    int bi = INT_MAX;
    for (int m = lane; m < count; m += 64) {
        int i = first + m;
        if (i >= T.S) i -= T.S;
        const double d2 = track_project(T, i, cx, cy, nullptr);
        if (track_less(d2, i, bv, bi)) bv = d2, bi = i;
    }
    track_wave_min(bv, bi);
    return bi == INT_MAX ? first : bi;                          // (every d2 a NaN: coordinates beyond 1e154)
}

// the goal waypoint seen from (cx, cy) with nearest segment seg (-1: none), in every lane of the wave: candidates in
// order of m, the first among equals, and only inside 2 lookahead
__device__ inline int track_goal(const TrackTable &T, double lookahead, int goal_span, int seg, double cx, double cy, int lane)
{
    int gfirst = 0, gcount = T.W;
    if (goal_span > 0) {
        gfirst = seg + 1;
        gcount = T.closed ? min(goal_span, T.W) : min(goal_span, T.W - 1 - seg);
    }
    double gv = INFINITY;
    int gm = INT_MAX;
    for (int m = lane; m < gcount; m += 64) {
        int j = gfirst + m;
        if (j >= T.W) j -= T.W;
        const double rx = T.x[j] - cx, ry = T.y[j] - cy;
        const double g = fabs(lookahead - sqrt(rx * rx + ry * ry));
        if (track_less(g, m, gv, gm)) gv = g, gm = m;
    }
    track_wave_min(gv, gm);
    if (gm == INT_MAX || !(gv < 2.0 * lookahead)) return -1;
    const int goal = gfirst + gm;
    return goal >= T.W ? goal - T.W : goal;
}

template <bool RACE>
__global__ __launch_bounds__(64 * (RACE ? RACE_MAX_GROUP : DRIVE_CARS)) void track_kernel(
    int n_envs, TrackTable T, TrackParams tp, TrackBufs tb, const double *__restrict__ state,
    const int *__restrict__ phase, const int *__restrict__ done, float *__restrict__ reward)
{
    __shared__ double sh_s0;
    __shared__ double sh_dist[RACE_MAX_GROUP];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int e = RACE ? blockIdx.x * tp.group + w : blockIdx.x * DRIVE_CARS + w;
    if (!RACE && e >= n_envs) return;                           // (wave-uniform; the barriers below are RACE's)
    const int ph = phase[e];
    const bool fresh = ph == ENV_FRESH, live = fresh || ph == ENV_STEPPED;
    double *st = tb.st + 3 * (size_t)e;
    int *ints = tb.ints + 4 * (size_t)e;
    float *row = tb.rows + 8 * (size_t)e;

    double cx = 0.0, cy = 0.0, s = 0.0, t = 0.0;
    int seg = 0, goal = -1;
    if (live) {                                                 // (wave-uniform)
        cx = state[(size_t)e * 11 + 0];
        cy = state[(size_t)e * 11 + 1];
        // the candidate segments: all for a fresh env, otherwise those within the window of the previous nearest one
        int first = 0, count = T.S;
        if (!fresh) track_window(T, tp.window, ints[TRACK_SEGMENT], first, count);
        seg = track_nearest(T, first, count, cx, cy, lane);
        track_project(T, seg, cx, cy, &t);
        s = T.cum[seg] + t * T.len[seg];
        goal = track_goal(T, tp.lookahead, tp.goal_span, seg, cx, cy, lane);
    }

    // the spawn offset against car 0 of the race (a race spawns as a whole: car 0 is fresh with the others)
    double offset = 0.0;
    if (RACE) {
        if (threadIdx.x == 0) sh_s0 = s;
        __syncthreads();
        if (fresh) {
            offset = s - sh_s0;
            track_wrap(T, offset);
        }
    }
    // fresh: D = 0, progress = 0, laps = 0 and the offset above; otherwise what the env holds, advanced if it stepped
    double delta = 0.0, progress = 0.0;
    int laps = 0;
    if (!fresh) {
        progress = st[1];
        offset = st[2];
        laps = ints[TRACK_LAPS];
        if (live) {
            delta = s - st[0];
            laps += track_wrap(T, delta);
            progress = progress + delta;
        }
    }
    const double race_dist = offset + progress;
    int rank = 0;
    if (RACE) {
        if (lane == 0) sh_dist[w] = race_dist;
        __syncthreads();
        for (int k = 0; k < tp.group; ++k) rank += sh_dist[k] > race_dist || (sh_dist[k] == race_dist && k < w);
    }
    if (lane != 0) return;
    ints[TRACK_RANK] = rank;
    row[0] = (float)delta;
    row[7] = (float)race_dist;
    if (!live) return;                                          // frozen, a wreck, a refused action: the rest stands
    const double th = state[(size_t)e * 11 + 2];
    const double hx = cos(th), hy = sin(th);
    const double dx = T.dx[seg], dy = T.dy[seg];
    const double ax = cx - T.x[seg], ay = cy - T.y[seg];
    double gx = 0.0, gy = 0.0;
    if (goal >= 0) {
        const double rx = T.x[goal] - cx, ry = T.y[goal] - cy;
        gx = hx * rx + hy * ry;
        gy = hx * ry - hy * rx;
    }
    st[0] = s;
    st[1] = progress;
    st[2] = offset;
    ints[TRACK_SEGMENT] = seg;
    ints[TRACK_GOAL] = goal;
    ints[TRACK_LAPS] = laps;
    row[1] = (float)s;
    row[2] = (float)((dx * ay - dy * ax) / T.len[seg]);
    row[3] = (float)atan2(dx * hy - dy * hx, dx * hx + dy * hy);
    row[4] = (float)gx;
    row[5] = (float)gy;
    row[6] = (float)progress;
    if (reward && tp.reward_mode == 1 && ph == ENV_STEPPED && done[e] != ENV_CRASHED) reward[e] = (float)delta;
}

}  // namespace scan
