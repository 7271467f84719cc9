// drive_track_kernels.h — track progress of the closed-loop roll-outs (include/scanlib_track_drive.h): where every car
// of a roll-out is on a track after each step it takes, how far it came, its laps, the tick at which it reached the goal
// distance and, in a race, its place; then the population's and the league's scores built on that.  Opt-in: a car handle
// without a track launches none of this (abi_car.hip, drive_loop), and drive_tick_kernel does not know about it.
//   drive_track_kernel<true>    once per call, on the start states before drive_start_kernel steps them: all segments
//   drive_track_kernel<false>   before every tick's scan: the cars still running (first[r] < 0) hold the state after
//                               that tick's step; a frozen car's wave returns at once
//                               Both: DRIVE_CARS cars per workgroup, one wave each, no barrier.  The search is
//                               track_kernels.h's (track_window, track_nearest, track_project, track_wrap), the lanes
//                               striding over the candidates; lane 0 finishes the row.
//   drive_track_rank_kernel     after the last tick, one lane per car: the spawn offset against car 0 of its race from
//                               the s0 column, race_dist and the rank.  Every lane recomputes the race_dist of the at
//                               most 8 cars of its race from s0 and progress, which nobody writes here, so no two lanes
//                               meet in memory and the kernel needs neither LDS nor a barrier.
//   drive_track_fitness_kernel, drive_track_standings_kernel   one lane per member, serial f64 in ascending car order:
//                               the order of the sums is the contract, as in policy_pop_fitness_kernel and
//                               league_standings_kernel.
// The table stays in global memory for the reasons track_kernels.h gives.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "track_kernels.h"

namespace scan {

// per car: rows [R][4] f64 = (s0, s, progress, race_dist), ints [R][4] = (segment, laps, goal_tick, rank), as the
// caller reads them; s is also the s_prev of the next placement
struct DriveTrackBufs {
    double *rows;
    int *ints;
};

enum : int { DT_S0 = 0, DT_S = 1, DT_PROGRESS = 2, DT_RACE_DIST = 3 };
enum : int { DT_SEGMENT = 0, DT_LAPS = 1, DT_GOAL_TICK = 2, DT_RANK = 3 };

template <bool FRESH>
__global__ __launch_bounds__(64 * DRIVE_CARS) void drive_track_kernel(int n_cars, TrackTable T, int window, double goal_dist,
                                                                      DriveTrackBufs tb, const double *__restrict__ state,
                                                                      const int *__restrict__ first, int t)
{
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * DRIVE_CARS + w;
    if (r >= n_cars) return;                                    // (wave-uniform; the kernel has no barrier)
    if (!FRESH && first[r] >= 0) return;                        // frozen by a crash at an earlier tick: nothing changes
    double *row = tb.rows + 4 * (size_t)r;
    int *ints = tb.ints + 4 * (size_t)r;
    const double cx = state[(size_t)r * 11 + 0], cy = state[(size_t)r * 11 + 1];
    int c0 = 0, count = T.S;
    if (!FRESH) track_window(T, window, ints[DT_SEGMENT], c0, count);
    const int seg = track_nearest(T, c0, count, cx, cy, lane);
    if (lane != 0) return;
    double tt;
    track_project(T, seg, cx, cy, &tt);
    double s = T.cum[seg] + tt * T.len[seg];
    // a position that is not a number: fmax drops the NaN of u / q (t = 0); the rule keeps it, so s and all that is
    // added up from it read NaN
    const double u = (cx - T.x[seg]) * T.dx[seg] + (cy - T.y[seg]) * T.dy[seg];
    if (u != u) s = u;
    if (FRESH) {
        row[DT_S0] = s;
        row[DT_S] = s;
        row[DT_PROGRESS] = 0.0;
        row[DT_RACE_DIST] = 0.0;
        ints[DT_SEGMENT] = seg;
        ints[DT_LAPS] = 0;
        ints[DT_GOAL_TICK] = -1;
        ints[DT_RANK] = 0;
        return;
    }
    double d = s - row[DT_S];
    const int laps = ints[DT_LAPS] + track_wrap(T, d);
    const double progress = row[DT_PROGRESS] + d;
    row[DT_S] = s;
    row[DT_PROGRESS] = progress;
    ints[DT_SEGMENT] = seg;
    ints[DT_LAPS] = laps;
    if (ints[DT_GOAL_TICK] < 0 && progress >= goal_dist) ints[DT_GOAL_TICK] = t;
}

// race_dist of car o, whose race starts at car r0: the spawn offset (wrapped, no lap counted) plus its progress
__device__ inline double drive_track_race_dist(const TrackTable &T, const double *rows, int r0, int o)
{
    double offset = rows[4 * (size_t)o + DT_S0] - rows[4 * (size_t)r0 + DT_S0];
    track_wrap(T, offset);
    return offset + rows[4 * (size_t)o + DT_PROGRESS];
}

// group > 0: races of `group` cars; 0: every car alone (offset 0, race_dist = progress, rank 0)
__global__ __launch_bounds__(64) void drive_track_rank_kernel(int n_cars, int group, TrackTable T, DriveTrackBufs tb)
{
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= n_cars) return;
    if (group <= 0) {
        tb.rows[4 * (size_t)r + DT_RACE_DIST] = 0.0 + tb.rows[4 * (size_t)r + DT_PROGRESS];
        tb.ints[4 * (size_t)r + DT_RANK] = 0;
        return;
    }
    const int k = r % group, r0 = r - k;
    const double mine = drive_track_race_dist(T, tb.rows, r0, r);
    int rank = 0;
    for (int k2 = 0; k2 < group; ++k2) {
        const double other = drive_track_race_dist(T, tb.rows, r0, r0 + k2);
        rank += other > mine || (other == mine && k2 < k);
    }
    tb.rows[4 * (size_t)r + DT_RACE_DIST] = mine;
    tb.ints[4 * (size_t)r + DT_RANK] = rank;
}

// scores [n][3] of a population roll-out: per member the sum of progress over its E cars, how many reached the goal,
// and the sum of their goal ticks
__global__ __launch_bounds__(64) void drive_track_fitness_kernel(DriveTrackBufs tb, int n, int E, double *__restrict__ scores)
{
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= n) return;
    double sum = 0.0, ticks = 0.0;
    int reached = 0;
    for (int e = 0; e < E; ++e) {
        const size_t r = (size_t)m * E + e;
        const int goal = tb.ints[4 * r + DT_GOAL_TICK];
        sum = sum + tb.rows[4 * r + DT_PROGRESS];
        if (goal >= 0) {
            reached += 1;
            ticks = ticks + (double)goal;
        }
    }
    scores[3 * (size_t)m + 0] = sum;
    scores[3 * (size_t)m + 1] = (double)reached;
    scores[3 * (size_t)m + 2] = ticks;
}

// scores [n_members][4] of a league roll-out over the grouping of the call's entries (league_kernels.h: the rows of a
// member ascending): cars entered, the sum of their progress, how many reached the goal, and the cars of their own
// races they are ahead of (a strictly larger race_dist; ties and NaN beat nobody).  Behind drive_track_rank_kernel.
__global__ __launch_bounds__(64) void drive_track_standings_kernel(DriveTrackBufs tb, const int *__restrict__ start,
                                                                   const int *__restrict__ count, const int *__restrict__ rows,
                                                                   int n_members, int group, double *__restrict__ scores)
{
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= n_members) return;
    const int cnt = count[m], s0 = start[m];
    double sum = 0.0;
    int reached = 0, beaten = 0;
    for (int j = 0; j < cnt; ++j) {
        const int a = rows[s0 + j];
        const double dist_a = tb.rows[4 * (size_t)a + DT_RACE_DIST];
        sum = sum + tb.rows[4 * (size_t)a + DT_PROGRESS];
        reached += tb.ints[4 * (size_t)a + DT_GOAL_TICK] >= 0;
        const int r0 = a - a % group;
        for (int k = 0; k < group; ++k) beaten += dist_a > tb.rows[4 * (size_t)(r0 + k) + DT_RACE_DIST];
    }
    double *o = scores + 4 * (size_t)m;
    o[0] = (double)cnt;
    o[1] = sum;
    o[2] = (double)reached;
    o[3] = (double)beaten;
}

}  // namespace scan
