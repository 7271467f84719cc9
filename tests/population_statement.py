"""Host statement of policy populations (include/scanlib_population.h), in NumPy and plain Python:

    theta      : for l = 0 ... n_layers - 1, W[l] as dims[l] x dims[l+1] row-major, then b[l]; P values
    evaluation : scan row i of a call over members [first, first + n) with E cars each is answered by member
                 first + i // E, by the canonical form of tests/policy_statement.py
    roll-out   : rl_car_drive_policy's loop with car r's steer from member first + r // E
    fitness    : [m][0] the ascending, separately rounded f64 sum of states_out[r][8] - states_in[r][8] over member m's
                 cars, [m][1] the number of them with first_crashed >= 0

The GPU tests hold the library to it with the real scan and car, the host tests with a fake one-dimensional world.
No tests live here."""
import numpy as np

import policy_statement as S
from support import D_BASE, lidar_poses

NAN32 = np.float32(np.nan)


def n_params(dims):
    return sum((dims[l] + 1) * dims[l + 1] for l in range(len(dims) - 1))


def pack(layers):
    """[(W (K, N), b (N,))] -> theta float32 (P,), value by value."""
    out = []
    for W, b in layers:
        for k in range(W.shape[0]):
            out.extend(np.float32(v) for v in W[k])
        out.extend(np.float32(v) for v in b)
    return np.array(out, np.float32)


def unpack(theta, dims):
    layers, o = [], 0
    for l in range(len(dims) - 1):
        K, N = dims[l], dims[l + 1]
        W = np.asarray(theta[o:o + K * N], np.float32).reshape(K, N)        # W[k][j] = theta[o + k N + j]
        b = np.asarray(theta[o + K * N:o + K * N + N], np.float32)
        layers.append((W.copy(), b.copy()))
        o += (K + 1) * N
    assert o == len(theta)
    return layers


def member_of(i, first, E):
    """The member that answers row / drives car i."""
    return first + i // E


def evaluate(thetas, dims, relu, scans, E, first=0, n=None, in_start=180, clip=15.0, scale=15.0):
    """Steers float32 (n E,) of scans (n E, size): thetas (N, P) is the whole population."""
    n = (len(thetas) - first) if n is None else n
    scans = np.asarray(scans, np.float32)
    assert scans.shape[0] == n * E
    out = np.empty(n * E, np.float32)
    member = np.array([member_of(i, first, E) for i in range(n * E)], int)
    for m in np.unique(member):                    # (a row's chain reads its own scan and its member's weights only)
        rows = np.nonzero(member == m)[0]
        out[rows] = S.forward(scans[rows], unpack(thetas[m], dims), relu, in_start=in_start, clip=clip, scale=scale)
    return out


def fitness(states_in, states_out, first_crashed, E):
    """float64 (n, 2) of a roll-out over n E cars."""
    n = len(states_in) // E
    fit = np.zeros((n, 2))
    for m in range(n):
        total = np.float64(0.0)
        for r in range(m * E, (m + 1) * E):
            total = total + (np.float64(states_out[r][8]) - np.float64(states_in[r][8]))
        fit[m, 0] = total
        fit[m, 1] = sum(1 for r in range(m * E, (m + 1) * E) if first_crashed[r] >= 0)
    return fit


def population_rollout(states, speeds, steer0, n_ticks, first, E, steer_clip, step_cars, scan, is_crashed, answer,
                       scan_dist_to_base=D_BASE):
    """rl_car_drive_population.  states (R, 11) with R = n E, speeds (R,), steer0 (R,) float32;
    step_cars(states (k, 11), speed (k,), steer (k,)) -> the states after one tick; scan(poses float32 (R, 3), cars
    float64 (R, 3), t) -> ranges (R, B) at tick t's ray offset; answer(member, ranges_row) -> float32.
    Returns (first crash tick (R,), final states, steers float32 (R, T), state trace (R, T, 11), fitness (n, 2))."""
    R, T = len(states), int(n_ticks)
    assert R % E == 0
    state = np.array(states, np.float64)
    steer = np.asarray(steer0, np.float32).astype(np.float64)
    crashed_at = np.full(R, -(T + 1), np.int32)
    steers = np.full((R, T), NAN32, np.float32)
    trace = np.full((R, T, 11), np.nan)
    for t in range(T):
        live = np.nonzero(crashed_at < 0)[0]
        if live.size:
            state[live] = step_cars(state[live].copy(), np.asarray(speeds, np.float64)[live], steer[live])
            trace[live, t] = state[live]
        ranges = np.asarray(scan(lidar_poses(state, scan_dist_to_base), state[:, :3].copy(), t), np.float32).reshape(R, -1)
        for r in live:
            if is_crashed(ranges[r]):
                crashed_at[r] = t
                continue
            a = np.float32(answer(member_of(r, first, E), ranges[r]))
            steers[r, t] = a
            s = np.float64(a)
            if steer_clip > 0:
                s = np.minimum(np.maximum(s, -steer_clip), steer_clip)
            steer[r] = s
    return crashed_at, state, steers, trace, fitness(np.asarray(states, np.float64), state, crashed_at, E)
