// league_kernels.h — league races (include/scanlib_league.h): population members as per-race seat drivers.  A call
// names a member (or -1) for every scan row / car, in any order, and policy_mlp_body stages ONE member's weights per
// workgroup: so the rows are first grouped by member, on the device, once per call:
//   league_count_kernel    one wave per member walks member[n] in 64-row steps: a ballot of the rows that name it, the
//                          popcount is its count;
//   league_offsets_kernel  one workgroup, an exclusive scan over the members (in trips of LG_SCAN members) of the
//                          counts (segment starts) and of ceil(count / PM_CARS) (workgroup-table starts); the total
//                          of the latter is the device word the network launch reads;
//   league_fill_kernel     the same walk again: a matching row's slot is the segment start + the matches before it
//                          (earlier steps + the popcount of the lower lanes): the row list comes out ordered by member
//                          and ASCENDING inside each member, with no atomic deciding a slot; the wave then writes its
//                          member's entries of the workgroup table, (member, chunk) per PM_CARS rows.
// An entry outside [0, n_members) matches no wave: it is in no segment and is never answered.
// policy_mlp_league_kernel is policy_mlp_body<true> over that table; LeagueSteer the steering source of
// drive_tick_kernel that asks the car's entry; league_standings_kernel the per-member sums after the last tick.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "drive_kernels.h"
#include "policy_kernels.h"

namespace scan {

constexpr int LG_WAVES = 4;            // members (waves) per workgroup of the count and fill passes
constexpr int LG_SCAN = 256;           // members per trip of the offsets scan

// the rows of one 64-row step that name member m, as a wave-wide mask (rows past n: none)
__device__ inline uint64_t league_match(const int *__restrict__ member, int n, int base, int lane, int m)
{
    const int i = base + lane;
    return __ballot(i < n && member[i] == m);
}

__global__ __launch_bounds__(64 * LG_WAVES) void league_count_kernel(const int *__restrict__ member, int n, int n_members,
                                                                     int *__restrict__ count)
{
    const int m = blockIdx.x * LG_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (m >= n_members) return;                            // (wave-uniform; the kernel has no barrier)
    int c = 0;
    for (int base = 0; base < n; base += 64) c += __popcll(league_match(member, n, base, lane, m));
    if (lane == 0) count[m] = c;
}

__global__ __launch_bounds__(LG_SCAN) void league_offsets_kernel(const int *__restrict__ count, int n_members,
                                                                 int *__restrict__ start, int *__restrict__ wg_start,
                                                                 int *__restrict__ total)
{
    __shared__ int sc[LG_SCAN], sw[LG_SCAN];
    const int t = threadIdx.x;
    int carry_c = 0, carry_w = 0;
    for (int base = 0; base < n_members; base += LG_SCAN) {        // (every thread makes every trip)
        const int m = base + t;
        const int c = m < n_members ? count[m] : 0, w = (c + PM_CARS - 1) / PM_CARS;
        sc[t] = c;
        sw[t] = w;
        __syncthreads();
        for (int d = 1; d < LG_SCAN; d <<= 1) {
            const int ac = t >= d ? sc[t - d] : 0, aw = t >= d ? sw[t - d] : 0;
            __syncthreads();
            sc[t] += ac;
            sw[t] += aw;
            __syncthreads();
        }
        if (m < n_members) {
            start[m] = carry_c + sc[t] - c;
            wg_start[m] = carry_w + sw[t] - w;
        }
        carry_c += sc[LG_SCAN - 1];
        carry_w += sw[LG_SCAN - 1];
        __syncthreads();                                           // (the next trip overwrites sc / sw)
    }
    if (t == 0) total[0] = carry_w;
}

// rows [n] and table [sum_m ceil(count[m] / PM_CARS)].  A slot is written only below the count the first pass took, so
// a member array that changed between the passes cannot push a store out of its segment.
__global__ __launch_bounds__(64 * LG_WAVES) void league_fill_kernel(const int *__restrict__ member, int n, int n_members,
                                                                    const int *__restrict__ count,
                                                                    const int *__restrict__ start,
                                                                    const int *__restrict__ wg_start,
                                                                    int *__restrict__ rows, int2 *__restrict__ table)
{
    const int m = blockIdx.x * LG_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (m >= n_members) return;
    const int cnt = count[m], s0 = start[m];
    int before = 0;
    for (int base = 0; base < n; base += 64) {
        const uint64_t hit = league_match(member, n, base, lane, m);
        const int slot = before + __popcll(hit & ((1ull << lane) - 1ull));
        if (((hit >> lane) & 1ull) && slot < cnt) rows[s0 + slot] = base + lane;
        before += __popcll(hit);
    }
    const int w0 = wg_start[m], nw = (cnt + PM_CARS - 1) / PM_CARS;
    for (int c = lane; c < nw; c += 64) table[w0 + c] = make_int2(m, c);
}

// The league form of the network: workgroup w of the host's upper bound answers chunk table[w].y of member table[w].x,
// the rows of its segment; past the device's total there is nothing to do.  scans [.][size] -> out [row].
__global__ __launch_bounds__(64) void policy_mlp_league_kernel(PolicyParams p, size_t stride, const int2 *__restrict__ table,
                                                               const int *__restrict__ total, const int *__restrict__ start,
                                                               const int *__restrict__ count, const int *__restrict__ rows,
                                                               const float *__restrict__ scans, int size,
                                                               float *__restrict__ out)
{
    if ((int)blockIdx.x >= total[0]) return;               // (workgroup-uniform, before any barrier)
    const int2 e = table[blockIdx.x];
    policy_mlp_body<true>(p, (size_t)e.x * stride, scans, rows + start[e.x], 0, e.y * PM_CARS, count[e.x], size, out);
}

// League races (rl_car_race_league): car r is driven by b.entry[r], member m >= 0 of the population (the network's
// answer, b.mlp[r], clamped as PolicySteer clamps it) or -1: FollowGap, never clamped.  One wave is one car, so
// answer()'s branch is wave-uniform.
struct LeagueSteer {
    template <int ROWS>
    __device__ static float answer(const DriveParams &dp, const DriveBufs &b, int r, const float (&raw)[ROWS], uint32_t *bits)
    {
        if (b.entry[r] >= 0) return PolicySteer::answer<ROWS>(dp, b, r, raw, bits);
        return FollowGapSteer::answer<ROWS>(dp, b, r, raw, bits);
    }
    __device__ static double steer(const DriveParams &dp, const DriveBufs &b, int r, float a)
    {
        return b.entry[r] >= 0 ? PolicySteer::steer(dp, b, r, a) : FollowGapSteer::steer(dp, b, r, a);
    }
};

// standings [n_members][4] of a league roll-out: one lane per member, serial f64 over its segment (ascending car index:
// the order of the sum is the contract).  [0] cars entered, [1] the sum of their gains (travel_dist now less
// travel_dist at the start), [2] how many crashed, [3] the cars of their own races they beat: a beats b when it lived
// longer, or as long with the larger gain; ties and NaN beat nobody.
__global__ __launch_bounds__(64) void league_standings_kernel(const double *__restrict__ states, const double *__restrict__ states0,
                                                              const int *__restrict__ first_crashed, const int *__restrict__ start,
                                                              const int *__restrict__ count, const int *__restrict__ rows,
                                                              int n_members, int group, int n_ticks,
                                                              double *__restrict__ standings)
{
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= n_members) return;
    const int cnt = count[m], s0 = start[m];
    double sum = 0.0;
    int crashed = 0, beaten = 0;
    for (int j = 0; j < cnt; ++j) {
        const int a = rows[s0 + j];
        const double gain_a = states[(size_t)a * 11 + 8] - states0[(size_t)a * 11 + 8];
        const double alive_a = first_crashed[a] >= 0 ? (double)first_crashed[a] : (double)n_ticks;
        sum = sum + gain_a;
        crashed += first_crashed[a] >= 0;
        const int r0 = a - a % group;
        for (int k = 0; k < group; ++k) {
            const int o = r0 + k;
            const double gain_o = states[(size_t)o * 11 + 8] - states0[(size_t)o * 11 + 8];
            const double alive_o = first_crashed[o] >= 0 ? (double)first_crashed[o] : (double)n_ticks;
            beaten += alive_a > alive_o || (alive_a == alive_o && gain_a > gain_o);
        }
    }
    double *o = standings + 4 * (size_t)m;
    o[0] = (double)cnt;
    o[1] = sum;
    o[2] = (double)crashed;
    o[3] = (double)beaten;
}

}  // namespace scan
