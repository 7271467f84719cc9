// drive_kernels.h — closed-loop roll-outs (rl_car_drive_followgap, rl_car_race_followgap, rl_car_drive_policy;
// include/scanlib.h; rl_car_race_seats, include/scanlib_seats.h): the reference's simulator tick (scripts/ros_interface.py:119-148: updatePose, runScan,
// checkCollision >= 0) driven by a steering source's answer to every scan — FollowGap (scripts/two_player/
// simple_driver.py:31,48-53) or the policy network (scripts/policy_driver.py) — for many cars at once with nothing
// crossing PCIe between ticks.  Per tick the host enqueues on one stream:
//   1. the scan of every car's lidar pose: the ordinary fan planner (launch_fan, abi_fan.hip) or, in races,
//      race_fan_kernel (race_kernels.h); for the policy, then policy_mlp_kernel over every scan (policy_kernels.h);
//   2. drive_tick_kernel<ROWS, Steer>: one wave per car — the scan into registers, Car::isCrashed's f64 compare
//      (racecar.cpp:305-328) as a ballot, the source's answer (FollowGapSteer: followgap_bits_eval's four passes,
//      consumer_kernels.h; PolicySteer: the network's output; SeatSteer: whichever of the two drives the car's seat
//      of its race; LeagueSteer, league_kernels.h: the population member or FollowGap its entry names) —, then one lane per car: the car step of the NEXT tick with the new steering angle and that
//      tick's lidar pose.
// drive_start_kernel (one lane per car) is the prologue: tick 0's step with the initial steer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "car_kernels.h"
#include "consumer_kernels.h"

namespace scan {

struct DriveParams {
    CarParams P;
    FollowGapParams fg;          // fg.size = num_rays (the policy source sets nothing else)
    double dt, scan_dist_to_base, crash_thresh;
    int n_cars, n_ticks;
    double steer_clip;           // policy source: > 0 clamps the network's steer to +-steer_clip
    int group;                   // seat source: cars per race (car r sits in seat r % group); 0 otherwise
    uint32_t policy_seats;       // seat source: bit k set: the network drives seat k; clear: FollowGap
};

struct DriveBufs {
    double *state;               // [R, 11] getState layout: the state after the last step taken
    const double *speed;         // [R] commanded speed (constant over the roll-out)
    const float *steer0;         // [R] steering input of tick 0's step
    const double *edge;          // [num_rays] car-outline table
    int *first;                  // [R] crash tick, -(T+1) while alive
    float *pose;                 // [R, 3] f32 lidar pose the next scan reads
    const float *ranges;         // [R, num_rays] this tick's scans
    double *vel;                 // optional traces [R, T] (pre-filled with NaN by the host)
    float *steers;
    float *scan_poses;           // [R, T, 3]
    double *states_trace;        // [R, T, 11]
    const float *mlp;            // policy source: [R] the network's answers to this tick's scans (seat source: the rows
                                 // of the cars in policy seats; the others are never read)
    const int *entry;            // league source (league_kernels.h): [R] the car's driver, a member of the population or
                                 // -1 for FollowGap; null otherwise
};

__device__ inline CarState drive_load_state(const double *s)
{
    CarState cs;
    cs.x = s[0]; cs.y = s[1]; cs.theta = s[2]; cs.velocity = s[3]; cs.steer_angle = s[4];
    cs.angular_velocity = s[5]; cs.slip_angle = s[6]; cs.st_dyn = s[7] > 0.0;
    cs.travel_dist = s[8]; cs.total_velo = s[9]; cs.update_count = (int)s[10];
    return cs;
}

__device__ inline void drive_store_state(const CarState &cs, double *o)
{
    o[0] = cs.x; o[1] = cs.y; o[2] = cs.theta; o[3] = cs.velocity; o[4] = cs.steer_angle;
    o[5] = cs.angular_velocity; o[6] = cs.slip_angle; o[7] = cs.st_dyn ? 1.0 : 0.0;
    o[8] = cs.travel_dist; o[9] = cs.total_velo; o[10] = (double)cs.update_count;
}

// Car::control + updatePosition for tick t of car r, then its lidar pose (car_scan_pose) and the trace rows of tick t.
// One lane.
__device__ inline void drive_step(const DriveParams &dp, const DriveBufs &b, int r, int t, double steer)
{
    double *s = b.state + (size_t)r * 11;
    CarState cs = drive_load_state(s);
    car_step(dp.P, cs, b.speed[r], steer, dp.dt);
    drive_store_state(cs, s);
    float pose[3];
    car_scan_pose(cs, dp.scan_dist_to_base, pose);
    b.pose[3 * r + 0] = pose[0];
    b.pose[3 * r + 1] = pose[1];
    b.pose[3 * r + 2] = pose[2];
    const size_t row = (size_t)r * dp.n_ticks + t;
    if (b.vel) b.vel[row] = cs.velocity;
    if (b.scan_poses) {
        b.scan_poses[3 * row + 0] = pose[0];
        b.scan_poses[3 * row + 1] = pose[1];
        b.scan_poses[3 * row + 2] = pose[2];
    }
    if (b.states_trace) drive_store_state(cs, b.states_trace + 11 * row);
}

// Car::isCrashed on one scan of `size` beams (lidar) against the outline table, one wave: (double)range - edge[j] <
// crash_thresh for any beam (NaN never crashes), as a ballot (wave-uniform).  raw: the scan, ROWS beams per lane
// (zero past size).
template <int ROWS>
__device__ inline bool drive_crashed(const float *lidar, const double *edge_tab, int size, double crash_thresh, int lane,
                                     float (&raw)[ROWS])
{
    double edge[ROWS];
#pragma unroll
    for (int u = 0; u < ROWS; ++u) {
        const bool in = u < ROWS - 1 || 64 * u + lane < size;
        raw[u] = in ? lidar[64 * u + lane] : 0.0f;
        edge[u] = in ? edge_tab[64 * u + lane] : 0.0;
    }
    bool hit = false;
#pragma unroll
    for (int u = 0; u < ROWS; ++u)
        if (u < ROWS - 1 || 64 * u + lane < size) hit |= ((double)raw[u] - edge[u]) < crash_thresh;
    return __ballot(hit) != 0;
}

// tick 0's step, one lane per car (b.state holds the start states)
__global__ __launch_bounds__(64) void drive_start_kernel(DriveParams dp, DriveBufs b)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= dp.n_cars) return;
    b.first[r] = -(dp.n_ticks + 1);
    drive_step(dp, b, r, 0, (double)b.steer0[r]);
}

// The steering sources of drive_tick_kernel.  answer(): car r's f32 answer to its scan of this tick (the steers trace),
// in every lane of the car's wave; steer(): the f64 steer car r gets from it, in the lane of wave 0 that steps it.
struct FollowGapSteer {
    template <int ROWS>
    __device__ static float answer(const DriveParams &dp, const DriveBufs &, int, const float (&raw)[ROWS], uint32_t *bits)
    {
        return followgap_bits_eval<ROWS>(raw, dp.fg, bits);
    }
    __device__ static double steer(const DriveParams &, const DriveBufs &, int, float a) { return (double)a; }
};

// policy_mlp_kernel's output (every car's scan, frozen ones included).  steer_clip > 0: the car gets
// clamp((double)a, -clip, clip) (scripts/policy_driver.py:33); otherwise (double)a, clamped later by Car::control
// (scripts/mcts.py).
struct PolicySteer {
    template <int ROWS>
    __device__ static float answer(const DriveParams &, const DriveBufs &b, int r, const float (&)[ROWS], uint32_t *)
    {
        return b.mlp[r];
    }
    __device__ static double steer(const DriveParams &dp, const DriveBufs &, int, float a)
    {
        const double s = (double)a;
        return dp.steer_clip > 0.0 ? fmin(fmax(s, -dp.steer_clip), dp.steer_clip) : s;
    }
};

// Per-seat drivers (rl_car_race_seats): car r of a race of dp.group cars sits in seat r % dp.group, and that seat's
// driver, FollowGap or the network (dp.policy_seats), answers and steers exactly as its own source above does: the
// clip never touches a FollowGap seat.  One wave is one car, so answer()'s branch is wave-uniform.
struct SeatSteer {
    __device__ static bool policy(const DriveParams &dp, int r) { return (dp.policy_seats >> (r % dp.group)) & 1u; }
    template <int ROWS>
    __device__ static float answer(const DriveParams &dp, const DriveBufs &b, int r, const float (&raw)[ROWS], uint32_t *bits)
    {
        if (policy(dp, r)) return PolicySteer::answer<ROWS>(dp, b, r, raw, bits);
        return FollowGapSteer::answer<ROWS>(dp, b, r, raw, bits);
    }
    __device__ static double steer(const DriveParams &dp, const DriveBufs &b, int r, float a)
    {
        return policy(dp, r) ? PolicySteer::steer(dp, b, r, a) : FollowGapSteer::steer(dp, b, r, a);
    }
};

// tick t after its scan: crash test, the source's answer, and the step of tick t + 1.  A workgroup holds DRIVE_CARS
// cars, one wave each for the scan-wide work (ROWS = ceil(num_rays / 64)); the f64 steps of the workgroup's cars then
// run one lane per car in wave 0.  (One step on lane 0 of every wave cost the full wave's f64 issue per car: at 4096
// cars that was most of the kernel's time.)  A frozen car (crashed at an earlier tick) was scanned at its last pose with
// the others; its wave skips the work.
constexpr int DRIVE_CARS = 8;

template <int ROWS, class Steer>
__global__ __launch_bounds__(64 * DRIVE_CARS) void drive_tick_kernel(DriveParams dp, DriveBufs b, int t)
{
    __shared__ uint32_t bits[DRIVE_CARS][2 * ROWS + 4];   // (FollowGap's bit rows: PolicySteer never touches them)
    __shared__ float answer_next[DRIVE_CARS];
    __shared__ int step_next[DRIVE_CARS];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * DRIVE_CARS + w;
    bool go = false;
    float answer = 0.0f;
    if (r < dp.n_cars && b.first[r] < 0) {                // (wave-uniform)
        float raw[ROWS];
        if (drive_crashed<ROWS>(b.ranges + (size_t)r * dp.fg.size, b.edge, dp.fg.size, dp.crash_thresh, lane, raw)) {
            if (lane == 0) b.first[r] = t;                // frozen from here: its trace rows after t stay NaN
        } else {
            answer = Steer::template answer<ROWS>(dp, b, r, raw, bits[w]);
            if (lane == 0 && b.steers) b.steers[(size_t)r * dp.n_ticks + t] = answer;
            go = t + 1 < dp.n_ticks;
        }
    }
    if (lane == 0) {
        answer_next[w] = answer;
        step_next[w] = go;
    }
    __syncthreads();
    if (threadIdx.x < DRIVE_CARS && step_next[threadIdx.x]) {
        const int rs = blockIdx.x * DRIVE_CARS + threadIdx.x;
        drive_step(dp, b, rs, t + 1, Steer::steer(dp, b, rs, answer_next[threadIdx.x]));
    }
}

}  // namespace scan
