"""The car model's cases as plain data: three cars, three time steps, a grid of start states and commands that takes
every branch of Car::control + Car::updatePosition, and the regime a step takes named from its inputs alone.  Used by
tests/test_car_regimes_host.py (the reference's compiled Car alone) and tests/test_gpu_car_regimes.py (every kernel
that steps a car).  docs/history/car_regimes.md has the tables."""
import itertools

import numpy as np

from oracle import reference
from pyracecarsimulator_amd import racecar as RC

# ---------------------------------------------------------------- the cars and the time steps
SIMPLE_CAR = dict(RC.DEFAULT_CAR, fc=0.523, cs_f=4.718, cs_r=5.4562, mass=3.47, I_z=0.04712, max_accel=7.51,
                  max_decel=8.26, max_steer_vel=3.2, ttc_thresh=0.01)
#: every value differs from DEFAULT_CAR; fc != 1, cs_f != cs_r, wb != l_f + l_r
SKEW_CAR = dict(wb=0.31, fc=0.8, h_cg=0.07, l_f=0.14, l_r=0.18, cs_f=4.0, cs_r=5.0, mass=3.6, I_z=0.05,
                ttc_thresh=0.02, width=0.25, length=0.5, max_steer_vel=2.5, max_steer_ang=0.35, max_speed=5.0,
                max_accel=6.0, max_decel=9.0)
CARS = {"default": dict(RC.DEFAULT_CAR), "simple": SIMPLE_CAR, "skew": SKEW_CAR}
DTS = (0.01, 0.001, 0.05)
SEEDS = {"default": 11, "simple": 12, "skew": 13}         # grid(car, seed) of each car, in every test
PAIRS = [(c, dt) for c in CARS for dt in DTS]
LOOP_PAIRS = [("simple", 0.001), ("skew", 0.05)]       # what the closed loops and the environments run

ROOM_N, RACE_ROOM_N, RES = 200, 560, 0.05              # maps.make_room(n): n cells of 0.05 m
D_SCAN = 0.4                                           # the closed loops' scan_dist_to_base (not the 0.275 default)
STRIDE = 8
RACE_PITCH, ENV_PITCH = 5.0, 8.0                       # start boxes of a race's cars, centre to centre: 1 m boxes
                                                       # 4 m apart in the 3-tick races, 7 m in the 7-step environments


def params(car):
    """The 17 constructor values of ``car`` in CAR_PARAM_ORDER."""
    return [float(car[k]) for k in RC.CAR_PARAM_ORDER]


# ---------------------------------------------------------------- the grid
def axes(car):
    ms, ma = car["max_speed"], car["max_steer_ang"]
    return ((-ms - 2, -ms, -3, -0.2, -1e-12, 0, 1e-12, 0.2, 0.4999999, 0.5, 0.51, 0.5299999, 0.53, 0.6, 2, ms - 0.01,
             ms, ms + 2),                                              # velocity
            (-20, -ms, -1, 0, 0.3, 2, ms, 20),                         # commanded speed
            (-ma, -0.2, 0, 5e-5, 0.2, ma),                             # steer angle
            (-1, -ma, -0.2, 0, 1.5e-4, 0.2, ma, 1),                    # commanded steer
            (0, 1, 0.5, -1))                                           # state[7]


def _fill(vel, ang, s7, rng):
    """(n, 11) states with the given velocity, steer angle and state[7]; every other field seeded, all finite."""
    n = len(vel)
    st = np.zeros((n, 11))
    st[:, :2] = ROOM_N * RES / 2 + rng.uniform(-0.5, 0.5, (n, 2))
    st[:, 2] = rng.uniform(-40.0, 40.0, n)
    st[:, 3], st[:, 4], st[:, 7] = vel, ang, s7
    moving = (st[:, 7] > 0) | (rng.random(n) < 0.25)
    st[:, 5] = np.where(moving, rng.uniform(-2.0, 2.0, n), 0.0)
    st[:, 6] = np.where(moving, rng.uniform(-0.3, 0.3, n), 0.0)
    st[:, 8] = rng.uniform(0.0, 100.0, n)
    st[:, 9] = rng.uniform(0.0, 1000.0, n)
    whole = rng.integers(0, 1_000_000, n).astype(np.float64)
    st[:, 10] = np.choose(rng.integers(0, 4, n), [np.zeros(n), np.full(n, 3.7), np.full(n, 99999.0), whole])
    return st


def grid(car, seed):
    """(states (27648, 11), commanded speeds, commanded steers), float64: the Cartesian product of ``axes(car)``.  Rows
    run in product order, except that in every run of 8 (the commanded steers of one combination of the other four)
    the commanded steer is rotated by the sum of the other four indices: row 0 of run k holds commanded steer number
    (-k's index sum) mod 8.  A stride of 8 through the rows therefore meets every combination of the other four axes
    once and every value of every axis equally often."""
    ax = axes(car)
    assert len(ax[3]) == STRIDE
    outer = np.array(list(itertools.product(*(range(len(a)) for a in (ax[0], ax[1], ax[2], ax[4])))))
    i_v, i_s, i_a, i_7 = (np.repeat(outer[:, k], STRIDE) for k in range(4))
    i_c = (np.tile(np.arange(STRIDE), len(outer)) - (i_v + i_s + i_a + i_7)) % STRIDE
    val = lambda k, idx: np.asarray(ax[k], np.float64)[idx]
    st = _fill(val(0, i_v), val(2, i_a), val(4, i_7), np.random.default_rng(seed))
    return st, val(1, i_s), val(3, i_c)


def rollout_grid(car, seed):
    """``grid`` plus the rows only float64 commands can state: steer angle 0 and a commanded steer of exactly +-1e-4
    (|dif_steer| == 0.0001: still the dead band), for every velocity, commanded speed and state[7]."""
    st, speed, steer = grid(car, seed)
    ax = axes(car)
    rows = np.array(list(itertools.product(ax[0], ax[1], ax[4], (1e-4, -1e-4))), np.float64)
    more = _fill(rows[:, 0], np.zeros(len(rows)), rows[:, 2], np.random.default_rng(seed + 1))
    return np.concatenate([st, more]), np.concatenate([speed, rows[:, 1]]), np.concatenate([steer, rows[:, 3]])


def subset(car, seed):
    """Every 8th row of ``grid`` (3456 rows): the closed loops' cars."""
    return tuple(a[::STRIDE].copy() for a in grid(car, seed))


def f32(v):
    """What an entry point that takes float32 commands (steer0, the environments' actions) is given."""
    return np.asarray(v, np.float64).astype(np.float32)


# ---------------------------------------------------------------- regimes
REGIMES = ("accel v>0 dif>0 linear", "accel v>0 dif>0 saturated", "accel v>0 dif<=0", "accel v<=0 dif>0",
           "accel v<=0 dif<=0 linear", "accel v<=0 dif<=0 saturated",
           "steer dead band", "steer +", "steer -",
           "kinematic after kinematic", "kinematic after dynamic", "dynamic after kinematic", "dynamic after dynamic")


def regimes(car, state, speed, steer):
    """bool (n, 13), columns as REGIMES: the branches one step from ``state`` under the command (speed, steer) takes.
    Every comparison is the reference's own on the step's inputs (racecar.cpp computeFromInput, updatePosition), in
    float64, so no rounded intermediate decides a branch.  Each row holds exactly three ones."""
    state = np.asarray(state, np.float64).reshape(-1, 11)
    speed, steer = np.asarray(speed, np.float64), np.asarray(steer, np.float64)
    v = state[:, 3]
    kp = 2.0 * car["max_accel"] / car["max_speed"]
    dif = speed - v
    lin = np.abs(kp * dif) <= car["max_accel"]
    fwd, up = v > 0, dif > 0
    dst = steer - state[:, 4]
    dead = ~(np.abs(dst) > 0.0001)
    was_dyn = state[:, 7] > 0.0
    kin = v < np.where(was_dyn, 0.53, 0.5)
    return np.stack([fwd & up & lin, fwd & up & ~lin, fwd & ~up, ~fwd & up, ~fwd & ~up & lin, ~fwd & ~up & ~lin,
                     dead, ~dead & (dst > 0), ~dead & ~(dst > 0),
                     kin & ~was_dyn, kin & was_dyn, ~kin & ~was_dyn, ~kin & was_dyn], -1)


# ---------------------------------------------------------------- the reference
def ref_steps(car, states, speeds, steers, dt, n=1):
    """RefCar(car).step(state, speed, steer, dt, n) of every row, (len, 11)."""
    reference.require()
    states = np.asarray(states, np.float64).reshape(-1, 11)
    speeds = np.broadcast_to(np.asarray(speeds, np.float64), (len(states),))
    steers = np.broadcast_to(np.asarray(steers, np.float64), (len(states),))
    out = np.empty_like(states)
    with reference.RefCar(params(car)) as ref:
        for k in range(len(states)):
            out[k] = ref.step(states[k], speeds[k], steers[k], dt, n)
    return out


def ref_scan_poses(car, states, d):
    """RefCar.scan_pose of every row, float64 (len, 3)."""
    states = np.asarray(states, np.float64).reshape(-1, 11)
    with reference.RefCar(params(car)) as ref:
        return np.stack([ref.scan_pose(s, d) for s in states])


def decoded(car, states):
    """Car::setState then getState of every row: state[7] as 0 or 1, state[10] as the int it is cast to.  What a kernel
    that stores a state it has loaded (the planner's roots) hands back."""
    states = np.asarray(states, np.float64).reshape(-1, 11)
    out = np.empty_like(states)
    with reference.RefCar(params(car)) as ref:
        for k in range(len(states)):
            ref.set_state(states[k])
            out[k] = ref.get_state()
    return out


def assert_steps(got, want, what):
    """The project's bound for the float64 car (rtol = atol = 1e-9) and the two decoded fields exactly."""
    got, want = np.asarray(got).reshape(-1, 11), np.asarray(want).reshape(-1, 11)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    close = np.isclose(got, want, rtol=1e-9, atol=1e-9)
    bad = np.nonzero(~close.all(1))[0]
    assert bad.size == 0, (what, bad[:5], got[bad[:1]], want[bad[:1]])
    assert (got[:, 7] == want[:, 7]).all() and (got[:, 10] == want[:, 10]).all(), what


# ---------------------------------------------------------------- closed-loop geometry
def max_move(car, dt, steps):
    """No car moves further in ``steps`` steps whatever it is told: its speed is at most max_speed + 2 (the largest
    start velocity; the clamp holds it at max_speed from the first step on)."""
    return (car["max_speed"] + 2.0) * dt * steps


def race_starts(states, group, pitch=RACE_PITCH):
    """``states`` (R * group, 11) as races (R, group, 11) in maps.make_room(RACE_ROOM_N): car k of a race keeps its
    place in the 1 m box but the box moves to slot k of a (group / 2) x 2 lattice of ``pitch`` m round the room's
    centre (group 1: the centre)."""
    st = np.array(states, np.float64).reshape(-1, group, 11)
    shift = (RACE_ROOM_N - ROOM_N) * RES / 2
    cols = max(group // 2, 1)
    for k in range(group):
        st[:, k, 0] += shift + (k % cols - (cols - 1) / 2) * pitch
        st[:, k, 1] += shift + ((k // cols) - (0.5 if group > 1 else 0.0)) * pitch
    return st


# ---------------------------------------------------------------- the planner's roots
def mcts_speeds(car):
    """The planner speeds: max_speed + 2, -1.5 and -max_speed.  With a constant commanded speed s <= 0 the branch
    v <= 0, dif <= 0 holds |dif| <= |s|, so only an s below -max_speed / 2 saturates it: -1.5 alone never does."""
    return (car["max_speed"] + 2.0, -1.5, -car["max_speed"])


def mcts_roots(car, states, k=16):
    """The indices of ``k`` rows of ``states`` that between them take, under the planner's speeds, every acceleration
    regime and every model regime at the root, hold a root at each end of the steering range (the steering regime
    itself depends on the action the search draws) and, after those, one root per velocity not yet there."""
    reg = np.any([regimes(car, states, s, 0.0) for s in mcts_speeds(car)], 0)
    # (columns 6 and 7 stand in for "steer angle at -max_steer_ang / at +max_steer_ang": such a root steers + / - under
    #  any action inside the steering range)
    reg[:, 6], reg[:, 7] = states[:, 4] == -car["max_steer_ang"], states[:, 4] == car["max_steer_ang"]
    need, rows = set(range(8)) | set(range(9, 13)), []
    for r in range(len(states)):
        new = {c for c in need if reg[r, c]}
        if new and len(rows) < k:
            rows.append(r)
            need -= new
    assert not need, need
    angles = axes(car)[2]
    for r in range(len(states)):                     # then one root per velocity not yet there (v = 0 among them),
        if len(rows) < k and states[r, 3] not in states[rows, 3] and states[r, 4] == angles[len(rows) % len(angles)]:
            rows.append(r)                           # the steer angles in turn
    return np.array(rows)
