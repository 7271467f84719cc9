// mcts_kernels.h — the MCTS planner (rl_mcts_*, include/scanlib.h): scripts/mcts.py's tree search for K independent
// trees in lock step, one node added per tree per iteration, every iteration enqueued without a host synchronisation:
//   1. mcts_select_kernel (one lane per tree): the literal descent of MCTS.mctsIteration (:150-185) with its visit
//      increments, the expansion action, the roll-out draws, the act step from the expanded node and the new child;
//   2. the act scans (launch_fan over the K children's lidar poses), policy_mlp_kernel for the NN source;
//   3. mcts_act_kernel<ROWS> (one wave per tree): drive_crashed's f64 crash ballot (drive_kernels.h) -> the terminal
//      flag, and the child's expansion answer (followgap_bits_eval or the network's output);
//   4. rollout_kernel + crash_groups_device over the K x L roll-out poses (MCTS.rollout, :202-245);
//   5. mcts_backup_kernel (one lane per tree): the reward sum in NumPy's pairwise order, or crash_pen, and the
//      repeated adds of Node.propagate at every recursion level.
// mcts_start_kernel writes the roots at reset; mcts_best_kernel answers MCTS.mcts (:126-131).
// The closed loop (rl_mcts_drive; scripts/mcts_driver.py:207-264) adds mcts_advance_kernel between two decisions (one
// lane per car): the car's crash test from the root act's ballot, the best root child, the car's steps with that
// action, the per-decision outputs and the next decision's root.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_device.h"
#include "car_kernels.h"
#include "consumer_kernels.h"
#include "drive_kernels.h"

namespace scan {

constexpr int MCTS_TREES = 8;          // trees per workgroup of mcts_act_kernel (one wave each)
constexpr int MCTS_MAX_STEPS = 512;    // roll-out length cap: mcts_pairwise_sum<3> covers it
constexpr double MCTS_RANDOM_DEV = 0.41;   // generateActionFromRandom: uniSample(0, 0.41) (mcts.py:259-260)

struct MctsParams {
    CarParams P;
    FollowGapParams fg;                // fg.size = num_rays
    int K, N, L, every, n_act, source; // source: RL_MCTS_FG / NN / RANDOM
    double speed, dt, scan_dist_to_base, C, crash_pen, uni_dev, max_steer, max_speed, crash_thresh;
};

struct MctsBufs {
    // node arrays, [K][N] (state [K][N][11], pose [K][N][3])
    int *parent, *first_child, *next_sibling, *last_child, *n_children, *visits, *child_visits, *terminal, *crash;
    double *reward, *action, *state;
    float *pose, *answer;
    int *n_nodes;                      // [K]
    int *child;                        // [K] node added this iteration (-1: none)
    int *exp_term;                     // [K] 1: it was added under a terminal node (the recursion's early return)
    const uint32_t *keys;              // [K] Philox keys, noise_key(seed)
    const double *logtab;              // [N + 1] math.log(n) from the host
    double *cstate;                    // [K][11] the children's states (rollout_kernel's input)
    float *cpose;                      // [K][3] their lidar poses (the act scans)
    double *actions;                   // [K][n_act][2] roll-out (speed, steer)
    const float *ranges;               // [K][num_rays] the act scans
    const double *edge;
    const float *mlp;                  // [K] the network's answers (NN)
    const double *vel;                 // [K][L] roll-out velocities
    const int *first;                  // [K] roll-out crash indices
    int *root_crash;                   // [K] or null: isCrashed(root scan) >= 0, kept by the root act (rl_mcts_drive)
};

// rl_mcts_drive's per-car arrays (D decisions)
struct MctsDrive {
    double *state;                     // [K][11] the cars' current states
    double *recent;                    // [K] their recent actions
    int *first;                        // [K] crash decision, -(D+1) while alive
    double *actions;                   // [K][D] best root action of every decision (NaN once crashed)
    int *visits;                       // [K][D] its visits (-1 once crashed)
    double *trace;                     // [K][D][11] or null: the state every decision was planned from
    int D, S;                          // decisions; car steps per decision
    double steer_clip;                 // > 0: the next recent action is the best action clamped to +-steer_clip
};

// (mcts_uniform01, the 53-bit Philox uniform of every draw, lives in scan_device.h: the particle filter draws with it too)

// numpy.random.uniform(lo, hi): lo + (hi - lo) u, each operation rounded
__device__ inline double mcts_uniform(double lo, double hi, double u)
{
    return lo + (hi - lo) * u;
}

// the UCB key of mcts.py:165-166, separately rounded f64 operations; lg = math.log(sum_of_visits) from the host table
__host__ __device__ inline double mcts_ucb(double reward, int visits, double lg, double C)
{
    const double v = (double)visits;
    return reward / v + C * sqrt(lg / v);
}

// numpy.add.reduce over a contiguous float64 array (pairwise_sum of NumPy's loops): 0.0 + P(a, n) with
// P(a, n) = a sequential sum from 0.0 for n < 8; eight strided accumulators folded as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7))
// and the tail added in order for n <= 128; P(a, n2) + P(a + n2, n - n2) with n2 = n/2 - (n/2) % 8 above.
__device__ inline double mcts_pairwise_block(const double *a, int n)
{
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}

template <int D>
__device__ inline double mcts_pairwise(const double *a, int n)
{
    if (D == 0 || n <= 128) return mcts_pairwise_block(a, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    return mcts_pairwise<(D > 0 ? D - 1 : 0)>(a, n2) + mcts_pairwise<(D > 0 ? D - 1 : 0)>(a + n2, n - n2);
}

__device__ inline double mcts_pairwise_sum(const double *a, int n)
{
    return 0.0 + mcts_pairwise<3>(a, n);      // depth 3: exact up to ~920 elements (MCTS_MAX_STEPS = 512)
}

// node 0 of tree k is the state `state` (getState layout) and the recent action `action` (visits 1, never terminal);
// its lidar pose goes to the act-scan buffer so that the root scan and answer come from the ordinary act launches
__device__ inline void mcts_write_root(const MctsParams &p, const MctsBufs &b, int k, const double *state, double action)
{
    const size_t n = (size_t)k * p.N;
    b.parent[n] = -1;
    b.first_child[n] = -1;
    b.next_sibling[n] = -1;
    b.last_child[n] = -1;
    b.n_children[n] = 0;
    b.visits[n] = 1;
    b.child_visits[n] = 0;
    b.terminal[n] = 0;
    b.crash[n] = -1;
    b.reward[n] = 0.0;
    b.action[n] = action;
    b.answer[n] = __builtin_nanf("");
    const CarState cs = drive_load_state(state);
    drive_store_state(cs, b.state + 11 * n);
    car_scan_pose(cs, p.scan_dist_to_base, b.pose + 3 * n);
    car_scan_pose(cs, p.scan_dist_to_base, b.cpose + 3 * k);
    b.n_nodes[k] = 1;
    b.child[k] = 0;
    b.exp_term[k] = 0;
}

// reset: the roots are the caller's states and recent actions
__global__ __launch_bounds__(64) void mcts_start_kernel(MctsParams p, MctsBufs b, const double *__restrict__ states,
                                                        const double *__restrict__ actions)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= p.K) return;
    mcts_write_root(p, b, k, states + 11 * (size_t)k, actions[k]);
}

// iteration `it` (counted from reset) of tree k: the descent of mctsIteration with its visits, then the new child
__global__ __launch_bounds__(64) void mcts_select_kernel(MctsParams p, MctsBufs b, int it)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= p.K) return;
    const size_t t0 = (size_t)k * p.N;
    int *parent = b.parent + t0, *first_child = b.first_child + t0, *next_sibling = b.next_sibling + t0;
    int *last_child = b.last_child + t0, *n_children = b.n_children + t0, *visits = b.visits + t0;
    int *child_visits = b.child_visits + t0, *terminal = b.terminal + t0;
    const double *reward = b.reward + t0;
    double *action = b.action + t0;
    const uint32_t key = b.keys[k];
    int node = 0, exp_term = 0;
    for (;;) {
        if (terminal[node]) {                       // `if node.isTerminal(): return 0, False` — the level above
            exp_term = 1;                           // expands at this (terminal) node, which is not visited
            break;
        }
        visits[node] += 1;                          // node.visit()
        if (parent[node] >= 0) child_visits[parent[node]] += 1;
        const int nc = n_children[node];
        const int s = child_visits[node];           // sum_of_visits (the children are not visited yet)
        if (nc == 0) break;                         // sqrt(0) < 0 is false: expand here
        const double lg = b.logtab[min(max(s, 0), p.N)];
        int best = -1;
        double best_key = 0.0;
        for (int c = first_child[node]; c >= 0; c = next_sibling[c]) {      // Python max: first strict maximum
            const double key_c = mcts_ucb(reward[c], visits[c], lg, p.C);
            if (best < 0 || key_c > best_key) {
                best = c;
                best_key = key_c;
            }
        }
        if (sqrt((double)s) < (double)nc) {
            node = best;
            continue;
        }
        break;
    }
    const int c = b.n_nodes[k];
    if (c >= p.N) {                                 // (the host refuses runs past the capacity)
        b.child[k] = -1;
        return;
    }
    // the expansion action: counter d = 0
    double a;
    const double u0 = mcts_uniform01(key, 0u, (uint32_t)it);
    if (p.source == RL_MCTS_RANDOM) {
        a = mcts_uniform(0.0 - MCTS_RANDOM_DEV, 0.0 + MCTS_RANDOM_DEV, u0);
    } else if (n_children[node] > 0) {
        const double pred = action[first_child[node]];
        a = mcts_uniform(pred - p.uni_dev, pred + p.uni_dev, u0);
    } else {
        a = (double)b.answer[t0 + node];
    }
    // the roll-out's actions: steer (d = 1 + 2m) drawn before speed (d = 2 + 2m)
    double *act = b.actions + (size_t)k * p.n_act * 2;
    for (int m = 0; m < p.n_act; ++m) {
        const double steer = mcts_uniform(-p.max_steer, p.max_steer, mcts_uniform01(key, 1u + 2u * m, (uint32_t)it));
        const double speed = mcts_uniform(0.0, p.max_speed, mcts_uniform01(key, 2u + 2u * m, (uint32_t)it));
        act[2 * m + 0] = speed;
        act[2 * m + 1] = steer;
    }
    // act (mcts.py:187-200): one step from the expanded node with (speed, a)
    CarState cs = drive_load_state(b.state + 11 * (t0 + node));
    car_step(p.P, cs, p.speed, a, p.dt);
    drive_store_state(cs, b.state + 11 * (t0 + c));
    drive_store_state(cs, b.cstate + 11 * (size_t)k);
    car_scan_pose(cs, p.scan_dist_to_base, b.pose + 3 * (t0 + c));
    car_scan_pose(cs, p.scan_dist_to_base, b.cpose + 3 * (size_t)k);
    parent[c] = node;
    first_child[c] = -1;
    next_sibling[c] = -1;
    last_child[c] = -1;
    n_children[c] = 0;
    visits[c] = 1;
    child_visits[c] = 0;
    terminal[c] = 0;
    b.crash[t0 + c] = -1;
    b.reward[t0 + c] = 0.0;
    action[c] = a;
    b.answer[t0 + c] = __builtin_nanf("");
    if (n_children[node] == 0) first_child[node] = c;
    else next_sibling[last_child[node]] = c;
    last_child[node] = c;
    n_children[node] += 1;
    child_visits[node] += 1;
    b.n_nodes[k] = c + 1;
    b.child[k] = c;
    b.exp_term[k] = exp_term;
}

// after the act scans: the new node's terminal flag (isCrashed >= 0, never for a root) and its expansion answer.
// One wave per tree; the FollowGap passes run for terminal nodes too (a terminal node can be expanded).
template <int ROWS>
__global__ __launch_bounds__(64 * MCTS_TREES) void mcts_act_kernel(MctsParams p, MctsBufs b, int root)
{
    __shared__ uint32_t bits[MCTS_TREES][2 * ROWS + 4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = blockIdx.x * MCTS_TREES + w;
    if (k >= p.K) return;                           // (wave-uniform; no block barrier below)
    const int c = b.child[k];
    if (c < 0) return;
    float raw[ROWS];
    const bool crashed =
        drive_crashed<ROWS>(b.ranges + (size_t)k * p.fg.size, b.edge, p.fg.size, p.crash_thresh, lane, raw);
    float ans = __builtin_nanf("");
    if (p.source == RL_MCTS_FG) ans = followgap_bits_eval<ROWS>(raw, p.fg, bits[w]);
    else if (p.source == RL_MCTS_NN) ans = b.mlp[k];
    if (lane == 0) {
        const size_t n = (size_t)k * p.N + c;
        b.answer[n] = ans;
        b.terminal[n] = root ? 0 : (crashed ? 1 : 0);
        if (root && b.root_crash) b.root_crash[k] = crashed ? 1 : 0;
    }
}

// the value of the new child (terminal: crash_pen; else the roll-out's reward sum / |action|, IEEE inf / NaN kept)
// and Node.propagate at every level of the recursion: walking up from the child, its j-th ancestor (j = 1: the node
// it was added under) receives rv j + 1 times, or j times when that node is terminal; the root receives nothing.
__global__ __launch_bounds__(64) void mcts_backup_kernel(MctsParams p, MctsBufs b)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= p.K) return;
    const int c = b.child[k];
    if (c < 0) return;
    const size_t t0 = (size_t)k * p.N;
    double rv;
    if (b.terminal[t0 + c]) {
        rv = p.crash_pen;
    } else {
        const int idx = b.first[k];
        const int n = idx >= 0 ? min(idx, p.L) : p.L;
        rv = mcts_pairwise_sum(b.vel + (size_t)k * p.L, n) / fabs(b.action[t0 + c]);
        b.crash[t0 + c] = idx;
    }
    double *reward = b.reward + t0;
    const int *parent = b.parent + t0;
    reward[c] += rv;
    const int extra = b.exp_term[k] ? 0 : 1;
    int node = parent[c];
    for (int j = 1; node >= 0 && parent[node] >= 0; ++j, node = parent[node])
        for (int r = 0; r < j + extra; ++r) reward[node] += rv;
}

// MCTS.mcts's answer (:125-131): the root child with the most visits, the first of equals (NaN / -1 without children)
__device__ inline void mcts_best_child(const MctsBufs &b, size_t t0, double &a, int &v)
{
    a = __builtin_nan("");
    v = -1;
    for (int c = b.first_child[t0]; c >= 0; c = b.next_sibling[t0 + c])
        if (b.visits[t0 + c] > v) {
            v = b.visits[t0 + c];
            a = b.action[t0 + c];
        }
}

__global__ __launch_bounds__(64) void mcts_best_kernel(MctsParams p, MctsBufs b, double *actions, int *visits,
                                                       int *n_nodes)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= p.K) return;
    double a;
    int v;
    mcts_best_child(b, (size_t)k * p.N, a, v);
    actions[k] = a;
    visits[k] = v;
    n_nodes[k] = b.n_nodes[k];
}

// the end of decision d of the closed loop (mcts_driver.py:207-264), one lane per car.  A car whose root scan crashed
// (Car::isCrashed >= 0, drive_tick_kernel's convention) freezes at d: first = d, NaN / -1 rows from d on, its state and
// recent action stay.  A live car takes the best root child's raw action for S steps of Car::control + updatePosition
// (car_step, as rollout_kernel runs it; mcts_driver.py:249), and its next recent action is that action clamped to
// +-steer_clip (:254).  Then, unless d is the last decision, node 0 becomes the car's state and recent action: the
// next decision's reset.  A frozen car's tree is re-rooted at its frozen state and searched with the others.
__global__ __launch_bounds__(64) void mcts_advance_kernel(MctsParams p, MctsBufs b, MctsDrive dv, int d)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= p.K) return;
    double *s = dv.state + 11 * (size_t)k;
    int f = d == 0 ? -(dv.D + 1) : dv.first[k];
    if (f < 0 && b.root_crash[k]) f = d;
    const size_t row = (size_t)k * dv.D + d;
    double a = __builtin_nan("");
    int v = -1;
    if (f < 0) {
        mcts_best_child(b, (size_t)k * p.N, a, v);
        if (dv.trace)
            for (int j = 0; j < 11; ++j) dv.trace[11 * row + j] = s[j];
        CarState cs = drive_load_state(s);
        for (int i = 0; i < dv.S; ++i) car_step(p.P, cs, p.speed, a, p.dt);
        drive_store_state(cs, s);
        dv.recent[k] = dv.steer_clip > 0.0 ? clampd(a, -dv.steer_clip, dv.steer_clip) : a;
    } else if (dv.trace) {
        for (int j = 0; j < 11; ++j) dv.trace[11 * row + j] = __builtin_nan("");
    }
    dv.first[k] = f;
    dv.actions[row] = a;
    dv.visits[row] = v;
    if (d + 1 < dv.D) mcts_write_root(p, b, k, s, dv.recent[k]);
}

// rl_mcts_probe_ucb: the device UCB of n (reward, visits, sum) triples
__global__ __launch_bounds__(256) void mcts_ucb_probe_kernel(const double *__restrict__ reward,
                                                             const int *__restrict__ visits,
                                                             const int *__restrict__ sum,
                                                             const double *__restrict__ logtab, long n, double C,
                                                             double *__restrict__ out)
{
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        out[i] = mcts_ucb(reward[i], visits[i], logtab[sum[i]], C);
}

}  // namespace scan
