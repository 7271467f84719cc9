// env_kernels.h — the driving environment (rl_env_*; include/scanlib.h): the closed loop of drive_kernels.h opened at
// the steering source.  Every call takes one (speed, steer) pair per env from the caller and, for N envs with nothing
// crossing PCIe in between, enqueues on one stream:
//   A. env_step_kernel, one lane per env: re-spawn (auto_reset) or the action check, the steer clamp and `substeps`
//      car steps in f64, then the f32 lidar pose.  One lane per env from the start: a step on lane 0 of a wave each
//      spends the whole wave's f64 issue on one car (drive_tick_kernel's comment has the figure).
//   -. the scan of all N lidar poses: the ordinary fan planner (launch_fan, abi_fan.hip).
//   B. env_observe_kernel<ROWS>, one wave per env: Car::isCrashed as a ballot (drive_crashed), truncation, the reward,
//      the observation window (lane-contiguous stores), the optional aux row.
// A reset is the same sequence with env_step_kernel in spawn mode.
// A race environment (rl_env_create_race) makes the race of P cars the episode: race_env_step_kernel spawns, freezes
// and steps whole races, the scan is race_fan_kernel over the cars' f64 states (race_kernels.h), and
// race_env_observe_kernel<ROWS>, one workgroup per race, decides after every car's code when the race is over.
// What happens to one car is stated once, for both environments:
//   env_spawn_index, env_spawn   the draw and the start of an episode
//   env_act, env_stand           a running env's action; an env that stays where it is
//   car_scan_pose                the lidar pose, straight into EnvBufs::pose (car_kernels.h)
//   env_done, env_reward         the verdict after the scan
//   env_emit                     what the caller sees: done, reward, the observation window, the aux row
// The race kernels add only the race's rule: the pool row and the race's counters at a spawn, the race's tick, the
// wreck, and when the race is over.
// Seats (rl_env_attach_seats, include/scanlib_seats.h): a race env whose seats have drivers runs the SEATS instances of
// the two race kernels.  Phase B's wave answers its car's scan with the seat's driver (FollowGap from the registers
// the crash ballot filled; the network from policy_mlp_rows_kernel, enqueued between the scan and phase B) into
// SeatBufs::answer, and the next call's phase A takes a scripted car's pair from there instead of `actions`.  An env
// without seats launches the plain instances, which hold none of this.
// League line-ups (rl_env_attach_league, include/scanlib_league_env.h): the LEAGUE instances ask a per-car ENTRY where
// the SEATS ones ask a per-seat bit.  Phase A copies a car's pending entry to its live one in the lane that spawns the
// car; phase B's wave answers the scan with the live entry's driver (FollowGap as above; a member's answer from
// policy_mlp_league_kernel over this call's grouping of the live entries) and, in the call that ends the race, adds
// the race's results to the drivers' rows of LeagueEnvBufs::results with 64-bit vector atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "car_kernels.h"
#include "drive_kernels.h"
#include "policy_kernels.h"
#include "race_kernels.h"
#include "scan_device.h"

namespace scan {

// what a call did to an env (EnvBufs::phase), phase A's message to phase B
enum : int { ENV_FROZEN = 0, ENV_STEPPED = 1, ENV_FRESH = 2, ENV_INVALID = 3 };
// done codes (include/scanlib.h)
enum : int { ENV_RUNNING = 0, ENV_CRASHED = 1, ENV_TRUNCATED = 2, ENV_BAD_ACTION = 3 };

struct EnvParams {
    CarParams P;
    double dt, scan_dist_to_base, crash_thresh, steer_clip, crash_reward;
    int n_envs, substeps, num_rays;
    int obs_start, obs_count, obs_stride;
    float obs_clip, obs_scale;
    int max_ticks, auto_reset;
    int n_starts;
    uint32_t key;                // noise_key(seed) of the last reset: the spawn draws
};

struct EnvBufs {
    double *state;               // [N, 11] getState layout
    const double *starts;        // [M, 11] the start pool
    const double *edge;          // [num_rays] car-outline table
    int *tick, *episode, *start_index, *done;     // [N] each
    int *phase;                  // [N] ENV_* of this call
    double *moved;               // [N] travel_dist gained by this call's steps
    float *pose;                 // [N, 3] f32 lidar pose the scan reads
    const float *ranges;         // [N, num_rays] this call's scans
};

// the start of episode q for whatever draws at counter `id` (an env, or a race for all its cars): the caller's index
// (clamped to the pool) or the planner's uniform at counter (id, q)
__device__ inline int env_spawn_index(const EnvParams &p, int id, int q, const int *given)
{
    if (given) return min(max(given[id], 0), p.n_starts - 1);
    const double u = mcts_uniform01(p.key, (uint32_t)id, (uint32_t)q);
    return min(p.n_starts - 1, (int)(u * (double)p.n_starts));
}

// env e starts episode q, drawn as start idx, from row `row` of the pool
__device__ inline void env_spawn(const EnvBufs &b, int e, int q, int idx, size_t row, CarState &cs)
{
    const double *s = b.starts + row * 11;
    double *o = b.state + (size_t)e * 11;
#pragma unroll
    for (int i = 0; i < 11; ++i) o[i] = s[i];
    cs = drive_load_state(s);
    b.tick[e] = 0;
    b.episode[e] = q;
    b.start_index[e] = idx;
    b.done[e] = ENV_RUNNING;
    b.phase[e] = ENV_FRESH;
    b.moved[e] = 0.0;
}

// env e stands where it is (frozen, a wreck, or after a refused action): scanned again from the same state
__device__ inline void env_stand(const EnvBufs &b, int e, int phase)
{
    b.phase[e] = phase;
    b.moved[e] = 0.0;
}

// a running env e takes the pair (speed, steer), two f32 widened: `substeps` car steps from cs, or ENV_BAD_ACTION
__device__ inline void env_act_pair(const EnvParams &p, const EnvBufs &b, int e, double speed, double steer, CarState &cs)
{
    if (!(isfinite(speed) && isfinite(steer))) {
        b.done[e] = ENV_BAD_ACTION;              // the state stays as it is: nothing non-finite reaches car_step
        env_stand(b, e, ENV_INVALID);
        return;
    }
    if (p.steer_clip > 0.0) steer = fmin(fmax(steer, -p.steer_clip), p.steer_clip);   // PolicySteer::steer
    const double before = cs.travel_dist;
    for (int i = 0; i < p.substeps; ++i) car_step(p.P, cs, speed, steer, p.dt);
    drive_store_state(cs, b.state + (size_t)e * 11);
    b.tick[e] += 1;
    b.phase[e] = ENV_STEPPED;
    b.moved[e] = cs.travel_dist - before;
}

// ... its pair of actions [N, 2] f32 (speed, steer)
__device__ inline void env_act(const EnvParams &p, const EnvBufs &b, int e, const float *actions, CarState &cs)
{
    env_act_pair(p, b, e, (double)actions[2 * e + 0], (double)actions[2 * e + 1], cs);
}

// phase A.  reset != 0: every env spawns with q = 0 (start_index: the caller's indices or null); otherwise one step
// of the state machine with actions [N, 2] f32 (speed, steer).
__global__ __launch_bounds__(64) void env_step_kernel(EnvParams p, EnvBufs b, const float *__restrict__ actions,
                                                      const int *__restrict__ start_index, int reset)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= p.n_envs) return;
    CarState cs;
    if (reset) {
        const int idx = env_spawn_index(p, e, 0, start_index);
        env_spawn(b, e, 0, idx, idx, cs);
    } else if (b.done[e] != ENV_RUNNING) {
        if (p.auto_reset) {
            const int q = b.episode[e] + 1, idx = env_spawn_index(p, e, q, nullptr);
            env_spawn(b, e, q, idx, idx, cs);
        } else {
            cs = drive_load_state(b.state + (size_t)e * 11);
            env_stand(b, e, ENV_FROZEN);         // frozen: scanned again where it stands
        }
    } else {
        cs = drive_load_state(b.state + (size_t)e * 11);
        env_act(p, b, e, actions, cs);
    }
    car_scan_pose(cs, p.scan_dist_to_base, b.pose + 3 * e);
}

// The verdict on env e after this call's scan, in two scalars (a pair in one struct cost race_env_observe_kernel
// registers across its barrier).  env_done: the done code; `hit` is Car::isCrashed's ballot, `tick` the count that
// max_ticks bounds (the env's own, or its race's).  A crash outranks a truncation at the same tick.
__device__ inline int env_done(const EnvParams &p, const EnvBufs &b, int e, bool hit, int tick)
{
    const int phase = b.phase[e];
    int done = b.done[e];
    const bool stepped = phase == ENV_STEPPED;
    if (stepped && p.max_ticks > 0 && tick == p.max_ticks) done = ENV_TRUNCATED;
    if ((stepped || phase == ENV_FRESH) && hit) done = ENV_CRASHED;
    return done;
}

// env_reward: the distance of a step that did not crash; crash_reward where this call's action ended the episode with
// 1 or 3; 0 for fresh envs (their action was ignored, even where the start lies inside the crash margin) and frozen
// ones.  done: env_done's answer.
__device__ inline float env_reward(const EnvParams &p, const EnvBufs &b, int e, int done)
{
    const int phase = b.phase[e];
    if (phase == ENV_STEPPED) return done == ENV_CRASHED ? (float)p.crash_reward : (float)b.moved[e];
    return phase == ENV_INVALID ? (float)p.crash_reward : 0.0f;
}

// env e's wave writes what the caller sees: the verdict (lane 0), the observation window of its scan `row`, the aux
// row.  reward may be null (a reset has none), aux too.
__device__ inline void env_emit(const EnvParams &p, const EnvBufs &b, int e, int lane, const float *row, int done,
                                float r, float *obs, float *reward, int *done_out, float *aux)
{
    if (lane == 0) {
        b.done[e] = done;
        done_out[e] = done;
        if (reward) reward[e] = r;
    }
    float *o = obs + (size_t)e * p.obs_count;
    for (int i = lane; i < p.obs_count; i += 64) {              // lane i of a round stores word i: whole lines
        const float v = row[p.obs_start + i * p.obs_stride];
        o[i] = p.obs_scale > 0.0f ? policy_input(v, p.obs_clip, p.obs_scale) : v;
    }
    if (aux && lane < 4) aux[4 * (size_t)e + lane] = (float)b.state[(size_t)e * 11 + 3 + lane];
}

// phase B: DRIVE_CARS envs per workgroup, one wave each (ROWS = ceil(num_rays / 64)).
template <int ROWS>
__global__ __launch_bounds__(64 * DRIVE_CARS) void env_observe_kernel(EnvParams p, EnvBufs b, float *__restrict__ obs,
                                                                      float *__restrict__ reward,
                                                                      int *__restrict__ done_out,
                                                                      float *__restrict__ aux)
{
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int e = blockIdx.x * DRIVE_CARS + w;
    if (e >= p.n_envs) return;                                  // (wave-uniform; no block barrier below)
    const float *row = b.ranges + (size_t)e * p.num_rays;
    float raw[ROWS];
    const bool hit = drive_crashed<ROWS>(row, b.edge, p.num_rays, p.crash_thresh, lane, raw);
    const int done = env_done(p, b, e, hit, b.tick[e]);
    env_emit(p, b, e, lane, row, done, env_reward(p, b, e, done), obs, reward, done_out, aux);
}

// ---- the race environment: the episode is a race of p.n_envs / R.group cars; car k of race r is env r P + k
// why a race is over (RaceEnvBufs::over; include/scanlib.h)
enum : int { RACE_RUNNING = 0, RACE_ATTRITION = 1, RACE_TRUNCATED = 2 };

struct RaceEnvBufs {
    int group, min_running;      // P cars a race; the race is over below min_running running cars
    int *tick, *episode, *start_index, *over;     // [R] each; starts: [M, P, 11]
};

// car k of race r joins the race's spawn at episode q (every lane of the race draws the same idx)
__device__ inline void race_env_spawn(const EnvParams &p, const EnvBufs &b, const RaceEnvBufs &R, int e, int q,
                                      const int *given, CarState &cs)
{
    const int r = e / R.group, k = e - r * R.group;
    const int idx = env_spawn_index(p, r, q, given);
    env_spawn(b, e, q, idx, (size_t)idx * R.group + k, cs);
    if (k == 0) {
        R.tick[r] = 0;
        R.episode[r] = q;
        R.start_index[r] = idx;
    }
}

// the seats of a race env: who drives seat k = e % group, and the scripted cars' answers
struct SeatBufs {
    uint32_t scripted, policy;   // bit k: seat k has a driver (else the caller's); ... and it is the network
    float speed[RACE_MAX_GROUP]; // the commanded speed of a scripted seat
    FollowGapParams fg;          // fg.size = num_rays
    const float *mlp;            // [N] the network's answers to this call's scans: the rows of the cars in policy seats
    float *answer;               // [N] the seat driver's f32 answer to the car's latest scan; NaN: a caller's seat, or a
                                 // car that was not running after that scan's phase B
};

// the league of a race env: who drives car e (an entry per car, pending and live), the scripted cars' answers and the
// drivers' results.  An entry in [lo, hi) is SCRIPTED: -1 FollowGap (lo = -1 only with a FollowGap handle), m >= 0
// member m (hi = n_members only where the scans hold the network's window, else 0); every other value is the caller's.
struct LeagueEnvBufs {
    int lo, hi, n_members;
    float speed[RACE_MAX_GROUP]; // the commanded speed of a scripted car in seat k
    FollowGapParams fg;          // fg.size = num_rays
    const int *pending;          // [N] the line-up a car adopts at its next spawn
    int *live;                   // [N] the line-up the race runs with
    const float *mlp;            // [N] the members' answers to this call's scans: the rows of the cars with a live entry >= 0
    float *answer;               // [N] as SeatBufs::answer
    unsigned long long *results; // [n_members + 2][8]: the members, FollowGap, the caller's cars
};

__device__ inline bool league_scripted(const LeagueEnvBufs &L, int entry) { return entry >= L.lo && entry < L.hi; }

// car a beats car b of its race (include/scanlib_league_env.h): more ticks; as many and a survivor (done 2) against a
// car that is out (1 or 3); as many, the same of the two classes and the larger gain.  Ties and NaN beat nobody.
__device__ inline bool league_beats(int ticks_a, int done_a, double gain_a, int ticks_b, int done_b, double gain_b)
{
    if (ticks_a != ticks_b) return ticks_a > ticks_b;
    const bool up_a = done_a == ENV_TRUNCATED, up_b = done_b == ENV_TRUNCATED;
    const bool out_a = done_a == ENV_CRASHED || done_a == ENV_BAD_ACTION;
    const bool out_b = done_b == ENV_CRASHED || done_b == ENV_BAD_ACTION;
    if (up_a && out_b) return true;
    return ((up_a && up_b) || (out_a && out_b)) && gain_a > gain_b;
}

// phase A of a race env, one lane per car.  Races straddle blocks, so no word is written by one lane and read by
// another in here: R.over is read only, R.tick / R.episode / R.start_index are written by car 0's lane and read in
// phase B, and every lane takes the race's episode from its own car's mirror.  SEATS: a car in a scripted seat that
// reaches the action check takes (S.speed[k], S.answer[e]), the answer phase B of the call before left for it, and its
// row of `actions` is not read.  LEAGUE: the lane that spawns a car copies the car's pending entry to its live one (a
// running race is never re-seated), and a car whose live entry is scripted takes (L.speed[k], L.answer[e]).
template <bool SEATS, bool LEAGUE = false>
__device__ __forceinline__ void race_env_step_body(const EnvParams &p, const EnvBufs &b, const RaceEnvBufs &R,
                                                   const SeatBufs *S, const float *__restrict__ actions,
                                                   const int *__restrict__ start_index, int reset,
                                                   const LeagueEnvBufs *L = nullptr)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= p.n_envs) return;
    const int r = e / R.group;
    CarState cs;
    if (reset) {
        race_env_spawn(p, b, R, e, 0, start_index, cs);
        if (LEAGUE) L->live[e] = L->pending[e];
    } else if (R.over[r] != RACE_RUNNING) {
        if (p.auto_reset) {
            race_env_spawn(p, b, R, e, b.episode[e] + 1, nullptr, cs);
            if (LEAGUE) L->live[e] = L->pending[e];
        } else {
            cs = drive_load_state(b.state + (size_t)e * 11);
            env_stand(b, e, ENV_FROZEN);         // a finished race stands
        }
    } else {
        if (e == r * R.group) R.tick[r] += 1;
        cs = drive_load_state(b.state + (size_t)e * 11);
        const int k = e - r * R.group;
        if (b.done[e] != ENV_RUNNING) {
            env_stand(b, e, ENV_FROZEN);         // a wreck: scanned again, and the others see it
        } else if (SEATS && ((S->scripted >> k) & 1u)) {
            float speed = 0.0f;                  // (a select chain: a lane-indexed kernel argument would go to scratch)
#pragma unroll
            for (int i = 0; i < RACE_MAX_GROUP; ++i) speed = i == k ? S->speed[i] : speed;
            env_act_pair(p, b, e, (double)speed, (double)S->answer[e], cs);
        } else if (LEAGUE && league_scripted(*L, L->live[e])) {
            float speed = 0.0f;
#pragma unroll
            for (int i = 0; i < RACE_MAX_GROUP; ++i) speed = i == k ? L->speed[i] : speed;
            env_act_pair(p, b, e, (double)speed, (double)L->answer[e], cs);
        } else {
            env_act(p, b, e, actions, cs);
        }
    }
    car_scan_pose(cs, p.scan_dist_to_base, b.pose + 3 * e);
}

__global__ __launch_bounds__(64) void race_env_step_kernel(EnvParams p, EnvBufs b, RaceEnvBufs R,
                                                           const float *__restrict__ actions,
                                                           const int *__restrict__ start_index, int reset)
{
    race_env_step_body<false>(p, b, R, nullptr, actions, start_index, reset);
}

__global__ __launch_bounds__(64) void race_env_seat_step_kernel(EnvParams p, EnvBufs b, RaceEnvBufs R, SeatBufs S,
                                                                const float *__restrict__ actions,
                                                                const int *__restrict__ start_index, int reset)
{
    race_env_step_body<true>(p, b, R, &S, actions, start_index, reset);
}

__global__ __launch_bounds__(64) void race_env_league_step_kernel(EnvParams p, EnvBufs b, RaceEnvBufs R, LeagueEnvBufs L,
                                                                  const float *__restrict__ actions,
                                                                  const int *__restrict__ start_index, int reset)
{
    race_env_step_body<false, true>(p, b, R, nullptr, actions, start_index, reset, &L);
}

// phase B of a race env: one workgroup per race, one wave per car (blockDim = 64 P, always P live waves).  Each wave
// reaches its car's verdict as env_observe_kernel does, with the race's tick, parks the code in LDS, and after the
// barrier applies the race's rule before the emit.  SEATS: a scripted seat's wave (w is the seat: wave-uniform) also
// answers the scan with its driver, and S.answer[e] keeps the answer where the car runs on after the race's rule.
// LEAGUE: the wave asks its car's live entry (one car a wave: wave-uniform) instead; every wave parks its car's entry,
// ticks and gain beside the code, and in the call that ends the race (over leaves RACE_RUNNING) adds its car's eight
// columns to its driver's row.  The other cars' codes after the race's rule follow from codes[] and `over`.
template <int ROWS, bool SEATS, bool LEAGUE = false>
__device__ __forceinline__ void race_env_observe_body(const EnvParams &p, const EnvBufs &b, const RaceEnvBufs &R,
                                                      const SeatBufs *S, uint32_t *bits, float *__restrict__ obs,
                                                      float *__restrict__ reward, int *__restrict__ done_out,
                                                      float *__restrict__ aux, const LeagueEnvBufs *L = nullptr)
{
    __shared__ int codes[RACE_MAX_GROUP];
    __shared__ int lg_entry[LEAGUE ? RACE_MAX_GROUP : 1], lg_ticks[LEAGUE ? RACE_MAX_GROUP : 1];
    __shared__ double lg_gain[LEAGUE ? RACE_MAX_GROUP : 1];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x, e = r * R.group + w;
    const float *row = b.ranges + (size_t)e * p.num_rays;
    float raw[ROWS];
    const bool hit = drive_crashed<ROWS>(row, b.edge, p.num_rays, p.crash_thresh, lane, raw);
    int done = env_done(p, b, e, hit, R.tick[r]);
    const float rw = env_reward(p, b, e, done);                 // (before the race's rule: a survivor's reward stays)
    float answer = __builtin_nanf("");
    if (SEATS && ((S->scripted >> w) & 1u))
        answer = ((S->policy >> w) & 1u) ? S->mlp[e] : followgap_bits_eval<ROWS>(raw, S->fg, bits);
    int entry = -2;
    if (LEAGUE) {
        entry = L->live[e];
        if (league_scripted(*L, entry)) answer = entry >= 0 ? L->mlp[e] : followgap_bits_eval<ROWS>(raw, L->fg, bits);
        if (lane == 0) {
            lg_entry[w] = entry;
            lg_ticks[w] = b.tick[e];
            lg_gain[w] = b.state[(size_t)e * 11 + 8] - b.starts[((size_t)b.start_index[e] * R.group + w) * 11 + 8];
        }
    }
    // a race spawns as a whole: a fresh car means a fresh race, whatever R.over still holds from the last episode
    const int over0 = b.phase[e] == ENV_FRESH ? RACE_RUNNING : R.over[r];
    if (lane == 0) codes[w] = done;
    __syncthreads();
    if (over0 == RACE_RUNNING) {                                // (a finished race that stands: nothing changes)
        int running = 0;
        bool truncated = false;                                 // (a running race held no 2 before this call)
        for (int k = 0; k < R.group; ++k) {
            running += codes[k] == ENV_RUNNING;
            truncated |= codes[k] == ENV_TRUNCATED;
        }
        const int over = truncated ? RACE_TRUNCATED : running < R.min_running ? RACE_ATTRITION : RACE_RUNNING;
        if (over == RACE_ATTRITION && done == ENV_RUNNING) done = ENV_TRUNCATED;    // it survived: its reward stays
        if (threadIdx.x == 0) R.over[r] = over;
        if (LEAGUE && over != RACE_RUNNING && lane < 8) {       // the race ends in this call: lane c adds column c
            const bool callers_car = !league_scripted(*L, entry);
            int beaten = 0, callers = 0, callers_beaten = 0, callers_won = 0;
            for (int k = 0; k < R.group; ++k) {
                if (k == w) continue;
                const int dk = over == RACE_ATTRITION && codes[k] == ENV_RUNNING ? ENV_TRUNCATED : codes[k];
                const bool win = league_beats(lg_ticks[w], done, lg_gain[w], lg_ticks[k], dk, lg_gain[k]);
                const bool caller = !league_scripted(*L, lg_entry[k]);
                beaten += win;
                callers += caller;
                callers_beaten += caller && win;
                callers_won += caller && league_beats(lg_ticks[k], dk, lg_gain[k], lg_ticks[w], done, lg_gain[w]);
            }
            const int col[8] = {1, done == ENV_CRASHED || done == ENV_BAD_ACTION, lg_ticks[w], R.group - 1, beaten, callers,
                                callers_beaten, callers_won};
            int v = 0;
#pragma unroll
            for (int c = 0; c < 8; ++c) v = c == lane ? col[c] : v;
            const int row = callers_car ? L->n_members + 1 : entry < 0 ? L->n_members : entry;
            if (v) atomicAdd(L->results + 8 * (size_t)row + lane, (unsigned long long)v);
        }
    }
    if (SEATS && lane == 0) S->answer[e] = done == ENV_RUNNING ? answer : __builtin_nanf("");
    if (LEAGUE && lane == 0) L->answer[e] = done == ENV_RUNNING ? answer : __builtin_nanf("");
    env_emit(p, b, e, lane, row, done, rw, obs, reward, done_out, aux);
}

template <int ROWS>
__global__ __launch_bounds__(64 * RACE_MAX_GROUP) void race_env_observe_kernel(EnvParams p, EnvBufs b, RaceEnvBufs R,
                                                                               float *__restrict__ obs,
                                                                               float *__restrict__ reward,
                                                                               int *__restrict__ done_out,
                                                                               float *__restrict__ aux)
{
    race_env_observe_body<ROWS, false>(p, b, R, nullptr, nullptr, obs, reward, done_out, aux);
}

template <int ROWS>
__global__ __launch_bounds__(64 * RACE_MAX_GROUP) void race_env_seat_observe_kernel(EnvParams p, EnvBufs b, RaceEnvBufs R,
                                                                                    SeatBufs S, float *__restrict__ obs,
                                                                                    float *__restrict__ reward,
                                                                                    int *__restrict__ done_out,
                                                                                    float *__restrict__ aux)
{
    __shared__ uint32_t bits[RACE_MAX_GROUP][2 * ROWS + 4];     // FollowGap's bit rows, one set per wave
    race_env_observe_body<ROWS, true>(p, b, R, &S, bits[threadIdx.x >> 6], obs, reward, done_out, aux);
}

template <int ROWS>
__global__ __launch_bounds__(64 * RACE_MAX_GROUP) void race_env_league_observe_kernel(EnvParams p, EnvBufs b, RaceEnvBufs R,
                                                                                      LeagueEnvBufs L, float *__restrict__ obs,
                                                                                      float *__restrict__ reward,
                                                                                      int *__restrict__ done_out,
                                                                                      float *__restrict__ aux)
{
    __shared__ uint32_t bits[RACE_MAX_GROUP][2 * ROWS + 4];     // FollowGap's bit rows, one set per wave
    race_env_observe_body<ROWS, false, true>(p, b, R, nullptr, bits[threadIdx.x >> 6], obs, reward, done_out, aux, &L);
}

}  // namespace scan
