"""The race environment (rl_env_create_race, rl_env_read_races, RaceEnv, RacecarSimulator.raceEnv) on the MI355X:
against the DriveEnv it becomes with one car a race, against rl_car_race_followgap when fed FollowGap's answers, and
against the statement (tests/race_env_statement.py) driven by the composed public calls (CarBatch.rollout,
calc_range_fan_cars, is_crashed)."""
import ctypes as C
import math

import numpy as np
import pytest

import consumer_shapes as CS
import drive_cases as DC
import race_env_statement as RES
import support
from env_statement import observation, spawn_index
from support import D_BASE, FOV, THRESH, same_bits
from pyracecarsimulator_amd import DriveEnv, RaceEnv, RacecarSimulator, _lib, maps, range_libc
from pyracecarsimulator_amd import racecar as RC

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

MRX = DC.RACE_MRX
RL_ERR_INVALID, RL_ERR_UNSUPPORTED = -1, -4           # include/scanlib.h rl_status


class RaceComposed(DC.Composed):
    """The race statement's callbacks from the public calls: DC.Composed with the race scan."""

    def __init__(self, m, cars, n, group, num_rays, edge, substeps, std=0.0, seed=0, base=0):
        super().__init__(m, cars, n, num_rays, edge, substeps, std, seed, base)
        self.group = group

    def scan_alone(self, poses, k):
        return DC.Composed.scan(self, poses, k)

    def scan(self, poses, car_poses, k):
        self.m.set_noise(self.std, self.seed, self.base + k * self.N * self.B)
        ranges = self.m.calc_range_fan_cars(np.ascontiguousarray(poses, np.float32), car_poses, self.group, FOV, self.B)
        self.m.set_noise(self.std, self.seed, self.base)
        return ranges.reshape(self.N, self.B)


def lineups(g, dt, n, group, seed, spread=0.9, v_lo=1.0, v_hi=5.0):
    """n line-ups (n, group, 11) of cars under way within `spread` m of a free centre (DC.race_clusters)."""
    states = np.zeros((n * group, 11))
    states[:, :3] = DC.race_clusters(g, dt, n, group, seed, spread)
    states[:, 3] = np.random.default_rng(seed).uniform(v_lo, v_hi, n * group)
    return states.reshape(n, group, 11)


def against_statement(env, stmt, actions, seed, start_index=None):
    """reset + every step of ``actions`` on the env and on the statement: all outputs, the states, the per-car and the
    per-race counters, bit for bit.  Returns per call (done before, done, reward, read())."""
    R, P = stmt.R, stmt.P

    def counters(k):
        rd = env.read()
        assert same_bits(rd["states"], stmt.states.reshape(R, P, 11)), k
        for key, want in (("ticks", stmt.tick), ("episodes", stmt.episode), ("start_index", stmt.start_index),
                          ("done", stmt.done)):
            assert same_bits(rd[key], want.reshape(R, P)), (k, key)
        for key, want in (("race_ticks", stmt.race_tick), ("race_episodes", stmt.race_episode),
                          ("race_start_index", stmt.race_start_index), ("race_over", stmt.race_over)):
            assert same_bits(rd[key], want), (k, key)
        return rd

    obs = env.reset(seed=seed, start_index=start_index)
    want_obs, want_done = stmt.reset(seed, start_index)
    assert same_bits(obs, want_obs.reshape(R, P, -1))
    log = [(None, want_done.copy(), None, counters(0))]
    for k, a in enumerate(actions, 1):
        prev_done = stmt.done.copy()
        obs, rew, dn = env.step(a.reshape(R, P, 2))
        want_obs, want_rew, want_done = stmt.step(a)
        assert same_bits(obs, want_obs.reshape(R, P, -1)), k
        assert same_bits(rew, want_rew.reshape(R, P)), k
        assert same_bits(dn, want_done.reshape(R, P)), k
        log.append((prev_done, want_done.copy(), want_rew.copy(), counters(k)))
    return log


# ---------------------------------------------------------------- 1. a race of one car is the DriveEnv
@pytest.mark.parametrize("kind", ["RM", "RMGPU"])
def test_race_env_of_one_equals_drive_env(kind):
    """DC.maze_case, 70 cars x 100 beams, 2 substeps, noise on at a non-zero base, auto_reset, max_ticks 5, window
    (7, 40, 2), 16 steps with one NaN action: a RaceEnv of P = 1 and a DriveEnv twin agree in every output, state and
    counter at every step."""
    g, states, _ = DC.maze_case(lambda g_: range_libc.PyOMap(g_).distance_transform())
    N, B, T = 70, 100, 16
    actions = DC.actions(5, T, N)
    actions[6, 11, 1] = np.nan
    m = (range_libc.PyRayMarching if kind == "RM" else range_libc.PyRayMarchingGPU)(range_libc.PyOMap(g), MRX)
    assert kind != "RM" or m.get_info("variant") == 3             # RM: the upstream-literal march
    m.set_noise(0.05, 99, 7 * N * B + 13)
    edge = support.edge(B)
    cars = RC.CarBatch()
    kw = dict(substeps=2, obs_window=(7, 40, 2), max_ticks=5, auto_reset=True, crash_reward=-1.5, car=cars)
    race = RaceEnv(m, states[:, None, :], N, B, FOV, edge, THRESH, min_running=1, **kw)
    one = DriveEnv(m, states, N, B, FOV, edge, THRESH, **kw)
    assert race.n_envs == N and race.n_races == N and race.group == 1 and race.obs_shape == (N, 40)

    def same_state(k):
        a, b = race.read(), one.read()
        for key in b:
            assert same_bits(a[key].reshape(b[key].shape), b[key]), (k, key)
        assert same_bits(a["race_episodes"], b["episodes"]) and same_bits(a["race_start_index"], b["start_index"])
        assert ((a["race_over"] != 0) == (b["done"] != 0)).all(), k
        return b

    o_r, x_r = race.reset(seed=3, aux=True)
    o_1, x_1 = one.reset(seed=3, aux=True)
    assert o_r.shape == (N, 1, 40) and same_bits(o_r[:, 0], o_1) and same_bits(x_r[:, 0], x_1)
    same_state(0)
    codes, respawned = set(), False
    for k in range(T):
        got, want = race.step(actions[k][:, None, :], aux=True), one.step(actions[k], aux=True)
        for x, y in zip(got, want):
            assert same_bits(x[:, 0], y), k
        rd = same_state(k + 1)
        codes |= set(want[2].tolist())
        respawned |= bool((rd["episodes"] > 0).any())
    assert {0, 1, 2, 3} <= codes and respawned
    m.set_noise(0.0, 0, 0)


# ---------------------------------------------------------------- 2. fed FollowGap it is rl_car_race_followgap
def _race_starts(g, dt, n_races, group, seed, clear_px=14.0, apart=1.0, within=2.0):
    """(states (R, P, 11), speeds (R, P)) with every start clear of the crash margin: each car `clear_px` cells from a
    wall (0.7 m: its lidar sits 0.275 m ahead of it, the noise reaches 0.2 m), the cars of a race at least `apart` m
    from each other (an outline reaches 0.23 m from its centre) and within `within` m of the first."""
    cand = maps.sample_free_poses(g, 4000, seed, clear_px, dt).astype(np.float64)
    free = np.ones(len(cand), bool)
    races = []
    for first in range(len(cand)):
        if len(races) == n_races:
            break
        if not free[first]:
            continue
        picked = [first]
        for c in np.nonzero(free)[0]:
            d = np.hypot(*(cand[picked, :2] - cand[c, :2]).T)
            if len(picked) < group and c != first and d.min() >= apart and d[0] <= within:
                picked.append(c)
        free[first] = False
        if len(picked) == group:
            free[picked] = False
            races.append(cand[picked])
    assert len(races) == n_races
    rng = np.random.default_rng(seed)
    states = np.zeros((n_races * group, 11))
    states[:, :3] = np.concatenate(races)
    speeds = rng.uniform(1.0, 4.0, n_races * group)
    states[:, 3] = rng.uniform(0.0, 1.0, n_races * group) * speeds
    return states.reshape(n_races, group, 11), speeds.reshape(n_races, group)


# the seed of the starts: no car inside the crash margin at the spawn (the drive would step it once more), some cars
# crash within the 50 ticks and some do not
CASE2 = {2: 52, 4: 54}


@pytest.mark.parametrize("kind,P", [("RMGPU", 2), ("RM", 4)])
def test_race_env_fed_followgap_equals_race_followgap(kind, P):
    """race_maze, 4 races x 50 ticks at 1081 beams, auto_reset off, min_running 1, max_ticks 0, noise on: with actions
    (speed, FollowGap's answer to the last observation) the env repeats rl_car_race_followgap — crash ticks, the state
    trace of the running cars, steers and final states.  The drive's noise base lies N B above the env's."""
    g = DC.race_maze()
    omap = range_libc.PyOMap(g)
    m = (range_libc.PyRayMarching if kind == "RM" else range_libc.PyRayMarchingGPU)(omap, MRX)
    fg = support.followgap()
    R, T, B = 4, 50, 1081
    N = R * P
    states, speeds = _race_starts(g, omap.distance_transform(), R, P, CASE2[P])
    speeds = speeds.astype(np.float32).astype(np.float64)        # the env takes its actions in float32
    edge = support.edge(B)
    cars = RC.CarBatch()
    base = 4321
    m.set_noise(0.05, 17, base)
    env = RaceEnv(m, states, R, B, FOV, edge, THRESH, min_running=1, max_ticks=0, auto_reset=False, car=cars)
    obs = env.reset(seed=0, start_index=np.arange(R))
    assert (env.read()["done"] == 0).all()
    steer0 = fg.eval_many(np.ascontiguousarray(obs.reshape(N, B)))
    m.set_noise(0.05, 17, base + N * B)
    first, final, vel, steers, sp, st = cars.race_followgap(m, fg, states, T, speeds, FOV, B, edge, THRESH,
                                                            steer0=steer0.reshape(R, P), trace=True)
    m.set_noise(0.05, 17, base)
    assert (first >= 0).any() and (first < 0).any()
    steer = steer0.reshape(R, P)
    want_first = np.full((R, P), -(T + 1), np.int32)
    for t in range(T):
        alive = want_first < 0
        obs, rew, dn = env.step(np.stack([speeds, steer], -1).astype(np.float32))
        rd = env.read()
        want_first[alive & (dn == 1)] = t
        assert same_bits(rd["states"][alive], st[:, :, t][alive]), t
        go = want_first < 0
        steer = fg.eval_many(np.ascontiguousarray(obs.reshape(N, B))).reshape(R, P)
        assert same_bits(steer[go], steers[:, :, t][go]), t
        assert np.isnan(steers[:, :, t][alive & ~go]).all()
        assert same_bits(rd["race_over"], (~go.any(1)).astype(np.int32)), t      # over once no car runs
    assert same_bits(want_first, first)
    assert same_bits(env.read()["states"], final)
    m.set_noise(0.0, 0, 0)


# ---------------------------------------------------------------- 3. against the statement over the public calls
CASE3 = dict(R=23, P=3, B=100, S=2, M=5, pool_seed=7, seed=1, base=555, std=0.02, noise_seed=3)
CASE3_KW = dict(min_running=2, max_ticks=15, auto_reset=True, crash_reward=-2.5, obs_window=(3, 45, 2))


def _case3(R=CASE3["R"], P=CASE3["P"], B=CASE3["B"], M=CASE3["M"], steps=40, pool_seed=CASE3["pool_seed"]):
    """(method, CarBatch, pool, edge, actions, callbacks) of test 3 (and, at other extents, of tests 5 and 6)."""
    g = DC.race_maze()
    omap = range_libc.PyOMap(g)
    m = range_libc.PyRayMarchingGPU(omap, MRX)
    m.set_noise(CASE3["std"], CASE3["noise_seed"], CASE3["base"])
    pool = lineups(g, omap.distance_transform(), M, P, pool_seed)
    cars = RC.CarBatch()
    edge = support.edge(B)
    actions = DC.actions(31 + P, steps, R * P)
    if steps > 9:
        actions[9, 4, 0] = np.nan
    pub = RaceComposed(m, cars, R * P, P, B, edge, CASE3["S"], CASE3["std"], CASE3["noise_seed"], CASE3["base"])
    return m, cars, pool, edge, actions, pub


def _statement(pool, R, B, pub, **kw):
    return RES.RaceEnvStatement(pool, R, B, pub.step_cars, pub.scan, pub.is_crashed, scan_dist_to_base=D_BASE, **kw)


def case3_conditions(log, P):
    """What test 3's run must contain, from against_statement's log (or the statement's own): a dict of booleans."""
    seen = dict(attrition_with_survivor=False, truncated=False, respawned=False, wreck_frozen_3=False)
    frozen = None
    for prev_done, done, rew, rd in log:
        over = np.asarray(rd["race_over"])
        d = np.asarray(done).reshape(-1, P)
        seen["attrition_with_survivor"] |= bool(((over == 1) & (d == 2).any(1) & (d == 1).any(1)).any())
        seen["truncated"] |= bool((over == 2).any())
        seen["respawned"] |= bool((np.asarray(rd["race_episodes"]) > 0).any())
        if prev_done is None:
            frozen = np.zeros(d.size, int)
            continue
        # a wreck of this call: done before it, in a race that ran on (its tick moved)
        ran = np.repeat(np.asarray(rd["race_ticks"]) > 0, P)
        wreck = (prev_done != 0) & (np.asarray(done) == prev_done) & ran
        frozen = np.where(wreck, frozen + 1, 0)
        seen["wreck_frozen_3"] |= bool((frozen >= 3).any())
    return seen


def test_race_env_equals_the_statement_over_public_calls():
    """23 races of 3 cars (race 21 straddles phase A's 64-lane boundary), 100 beams, 2 substeps, RMGPU with noise, a
    pool of five line-ups drawn by seed, min_running 2, max_ticks 15, auto_reset, 40 steps with one NaN action."""
    R, P, B = CASE3["R"], CASE3["P"], CASE3["B"]
    m, cars, pool, edge, actions, pub = _case3()
    env = RaceEnv(m, pool, R, B, FOV, edge, THRESH, substeps=CASE3["S"], car=cars, **CASE3_KW)
    stmt = _statement(pool, R, B, pub, **CASE3_KW)
    log = against_statement(env, stmt, actions, CASE3["seed"])
    assert all(case3_conditions(log, P).values()), case3_conditions(log, P)
    # another car was seen: the last scan differs from the plain fan of the same poses at the same ray offsets
    win = CASE3_KW["obs_window"]
    alone = observation(pub.scan_alone(support.lidar_poses(stmt.states), stmt.k), win, 0, 0)
    seen = observation(stmt.ranges, win, 0, 0)
    assert (alone != seen).any() and not (alone != seen).all()
    rd = log[-1][3]
    assert len(set(rd["race_start_index"].tolist())) > 1
    for r in range(R):
        assert rd["race_start_index"][r] == spawn_index(CASE3["seed"], r, rd["race_episodes"][r], CASE3["M"])
    m.set_noise(0.0, 0, 0)


# ---------------------------------------------------------------- 4. the room
def _room_env(s, min_running, substeps=1, B=1081):
    g = maps.make_room(200)
    m = range_libc.PyRayMarchingGPU(range_libc.PyOMap(g), MRX)
    env = RaceEnv(m, s, 1, B, FOV, support.edge(B), THRESH, min_running=min_running, auto_reset=False, crash_reward=-1.0,
                  substeps=substeps)
    env.reset(start_index=[0])
    assert (env.read()["done"] == 0).all()
    return env


def test_race_env_room_head_on_and_wreck():
    """An empty 10 m walled room, the poses of test_head_on_and_wreck, every car driven straight at 3 m/s."""
    a = np.tile(np.float32([3.0, 0.0]), (1, 2, 1))
    s = np.zeros((1, 2, 11))
    s[0, 0, :4] = (4.4, 5.0, 0.0, 3.0)
    s[0, 1, :4] = (5.6, 5.0, math.pi, 3.0)
    # The two cars close 6 cm per 0.01 s tick on a 5 cm grid, where the outline cells and the march's last sample are
    # mirror images only to within a cell: at one substep the car heading east reads its crash on tick 11 and the
    # other not yet.  A step of two substeps closes 12 cm, more than that cell, and holds both.
    env = _room_env(s, 2, substeps=2)
    for k in range(20):
        obs, rew, dn = env.step(a)
        if dn.any():
            break
    # head-on: both read 1 on the same step, long before a wall is within reach
    assert dn.tolist() == [[1, 1]] and rew.tolist() == [[-1.0, -1.0]], (k, dn, rew)
    rd = env.read()
    assert rd["race_over"].tolist() == [1] and rd["states"][0, 0, 0] < 5.0 < rd["states"][0, 1, 0]

    # wall then follower: A 0.35 m from the east wall, B 0.75 m behind it
    s = np.zeros((1, 2, 11))
    s[0, 0, :4] = (9.3, 5.0, 0.0, 3.0)
    s[0, 1, :4] = (8.55, 5.0, 0.0, 3.0)
    env = _room_env(s, 2)
    for k in range(30):
        before = env.read()["states"]
        obs, rew, dn = env.step(a)
        if dn.any():
            break
    rd = env.read()
    moved = np.float32(rd["states"][0, 1, 8] - before[0, 1, 8])
    assert dn.tolist() == [[1, 2]] and rd["race_over"].tolist() == [1]      # B survived the race
    assert rew[0, 0] == np.float32(-1.0) and rew[0, 1] == moved and moved > 0
    a_step = k

    env = _room_env(s, 1)
    wreck, b_step = None, None
    for k in range(60):
        obs, rew, dn = env.step(a)
        rd = env.read()
        if wreck is None and dn[0, 0] == 1:
            assert k == a_step and dn[0, 1] == 0 and rd["race_over"].tolist() == [0]    # B drives on
            wreck = rd["states"][0, 0].copy()
        if dn[0, 1] != 0:
            b_step = k
            break
    assert wreck is not None and b_step is not None and b_step > a_step
    assert dn.tolist() == [[1, 1]] and rd["race_over"].tolist() == [1]
    assert same_bits(rd["states"][0, 0], wreck)                              # the wreck stood at its crash-step state
    assert rd["states"][0, 1, 0] < wreck[0] - 0.3                            # B stopped behind it, not at the wall
    assert rd["ticks"].tolist() == [[a_step + 1, b_step + 1]] and rd["race_ticks"].tolist() == [b_step + 1]


# ---------------------------------------------------------------- 5. extents
@pytest.mark.parametrize("P,B,R", [(8, 1280, 2), (8, 10, 3), (2, 100, 1)])
def test_race_env_extents(P, B, R):
    """A full 512-thread workgroup at ROWS = 20, the smallest fan, and a single race of two: 4 steps against the
    statement over the public calls."""
    m, cars, pool, edge, actions, pub = _case3(R=R, P=P, B=B, M=3, steps=4, pool_seed=11 + P)
    win = (1, B // 2, 2)
    kw = dict(min_running=max(1, P // 2), max_ticks=3, auto_reset=True, crash_reward=-1.0, obs_window=win, obs_clip=6.0,
              obs_scale=3.0)
    env = RaceEnv(m, pool, R, B, FOV, edge, THRESH, substeps=CASE3["S"], car=cars, **kw)
    assert env.obs_shape == (R * P, B // 2)
    stmt = _statement(pool, R, B, pub, **kw)
    against_statement(env, stmt, actions, seed=2)
    m.set_noise(0.0, 0, 0)


@pytest.mark.parametrize("B", CS.SIZES)
def test_race_env_observe_ballot_at_every_row_count(B):
    """race_env_observe_kernel<ROWS> at every ROWS = 1 ... 20 (consumer_shapes.SIZES): three races of three cars — a
    workgroup per race, waves 0 ... 2 —, a reset and two steps against the statement over the public calls, once per
    beam that decides the crash alone and once with an outline no beam reaches; window, clip, scale and noise as in
    test_gpu_env.py's test of the same name."""
    rows, R, P, S = CS.rows_of(B), 3, 3, CASE3["S"]
    odd = rows % 2 == 1
    g = DC.race_maze()
    omap = range_libc.PyOMap(g)
    m = range_libc.PyRayMarchingGPU(omap, MRX)
    pool = lineups(g, omap.distance_transform(), 3, P, 11 + P)
    cars = RC.CarBatch()
    std, nseed, base = (CASE3["std"], CASE3["noise_seed"], CASE3["base"]) if odd else (0.0, 0, 0)
    win = (B - 2 * (B // 2) + 1, B // 2, 2)
    kw = dict(min_running=1, auto_reset=True, crash_reward=-1.0, obs_window=win,
              **(dict(obs_clip=6.0, obs_scale=3.0) if odd else {}))
    actions = DC.actions(31 + P, 2, R * P)
    for j in CS.one_hot_beams(B) + (None,):
        edge = CS.one_hot_edge(B, j)
        m.set_noise(std, nseed, base)
        env = RaceEnv(m, pool, R, B, FOV, edge, THRESH, substeps=S, car=cars, **kw)
        pub = RaceComposed(m, cars, R * P, P, B, edge, S, std, nseed, base)
        log = against_statement(env, _statement(pool, R, B, pub, **kw), actions, seed=2)
        for _, dn, _, _ in log:                 # beam j alone decides: every car crashes, or none does
            assert (dn == (RES.RUNNING if j is None else RES.CRASHED)).all(), (B, j, dn)
    m.set_noise(0.0, 0, 0)


def test_race_env_steer_clip_clamps_the_action():
    """steer_clip 0.25 and steers of +-0.4 (beyond it) and +-0.2 (within), two races of three cars clear of every crash
    margin, four steps: the race env equals the statement, whose clamp is np.minimum / np.maximum in f64; the same six
    cars as races of one equal a DriveEnv twin.  The cars start with 0.2 rad of steer towards their action, so the
    first step already turns past the clamp: the statement without the clamp ends somewhere else."""
    R, P, B, T = 2, 3, 100, 4
    g = DC.race_maze()
    omap = range_libc.PyOMap(g)
    m = range_libc.PyRayMarchingGPU(omap, MRX)
    pool, _ = _race_starts(g, omap.distance_transform(), R, P, 54)
    steer = np.float32([0.4, -0.4, 0.2, -0.2, -0.4, 0.4])
    pool[..., 4] = 0.2 * np.sign(steer).reshape(R, P)
    actions = np.tile(np.stack([np.full(R * P, 3.0, np.float32), steer], -1), (T, 1, 1))
    cars = RC.CarBatch()
    edge = support.edge(B)
    m.set_noise(CASE3["std"], CASE3["noise_seed"], CASE3["base"])
    kw = dict(min_running=1, auto_reset=False, crash_reward=-1.0, obs_window=(3, 45, 2), steer_clip=0.25)
    pub = RaceComposed(m, cars, R * P, P, B, edge, CASE3["S"], CASE3["std"], CASE3["noise_seed"], CASE3["base"])
    env = RaceEnv(m, pool, R, B, FOV, edge, THRESH, substeps=CASE3["S"], car=cars, **kw)
    stmt = _statement(pool, R, B, pub, **kw)
    log = against_statement(env, stmt, actions, seed=1, start_index=np.arange(R))
    assert (log[-1][1] == RES.RUNNING).all()                       # every car drove all four steps
    # (the car turns at max_steer_vel towards its target and overshoots it by less than one substep's turn)
    clamped = stmt.states.reshape(R * P, 11)[:, 4]
    turn = RC.DEFAULT_CAR["max_steer_vel"] * 0.01
    assert (np.abs(clamped) < 0.25 + turn).all()
    free = _statement(pool, R, B, pub, **dict(kw, steer_clip=0.0))
    free.reset(1, np.arange(R))
    for a in actions:
        free.step(a)
    beyond = np.abs(steer) > 0.25
    assert (np.abs(free.states.reshape(R * P, 11)[beyond, 4]) > 0.4 - turn).all()
    assert same_bits(free.states.reshape(R * P, 11)[~beyond], stmt.states.reshape(R * P, 11)[~beyond])
    # P = 1: the race env of one car per race and the DriveEnv, the same clamp
    flat = pool.reshape(R * P, 11)
    m.set_noise(CASE3["std"], CASE3["noise_seed"], CASE3["base"])
    race = RaceEnv(m, flat[:, None, :], R * P, B, FOV, edge, THRESH, substeps=CASE3["S"], car=cars, **kw)
    kw1 = {k: v for k, v in kw.items() if k != "min_running"}
    one = DriveEnv(m, flat, R * P, B, FOV, edge, THRESH, substeps=CASE3["S"], car=cars, **kw1)
    idx = np.arange(R * P)
    assert same_bits(race.reset(seed=1, start_index=idx)[:, 0], one.reset(seed=1, start_index=idx))
    for k, a in enumerate(actions):
        for x, y in zip(race.step(a[:, None, :]), one.step(a)):
            assert same_bits(x[:, 0], y), k
        assert same_bits(race.read()["states"][:, 0], one.read()["states"]), k
    assert np.array_equal(one.read()["states"][:, 4], clamped)       # (alone, a car turns the same way)
    m.set_noise(0.0, 0, 0)


# ---------------------------------------------------------------- 6. the device form
def test_race_env_device_form_equals_host_form():
    """Test 3's configuration on two twin envs, 10 steps: torch tensors on the current stream (every other step on a
    side stream) give the bits of the NumPy form, read() included."""
    import torch
    R, P, B = CASE3["R"], CASE3["P"], CASE3["B"]
    N = R * P
    m, cars, pool, edge, actions, pub = _case3(steps=11)
    kw = dict(substeps=CASE3["S"], car=cars, **CASE3_KW)
    host = RaceEnv(m, pool, R, B, FOV, edge, THRESH, **kw)
    dev = RaceEnv(m, pool, R, B, FOV, edge, THRESH, **kw)
    sidx = (np.arange(R) % CASE3["M"]).astype(np.int32)
    o_h, x_h = host.reset(seed=9, start_index=sidx, aux=True)
    o_d, x_d = dev.reset(seed=9, start_index=torch.from_numpy(sidx).cuda(), aux=True)
    assert o_d.is_cuda and tuple(o_d.shape) == (R, P, 45) and tuple(x_d.shape) == (R, P, 4)
    assert same_bits(o_d.cpu().numpy(), o_h) and same_bits(x_d.cpu().numpy(), x_h)

    def same_reads(k):
        rd_h, rd_d = host.read(), dev.read()
        for key in rd_h:
            assert same_bits(rd_h[key], rd_d[key]), (k, key)
        return rd_h

    same_reads(0)
    stream = torch.cuda.Stream()
    over = set()
    for k in range(10):
        a_np = actions[k].reshape(R, P, 2)
        o_h, r_h, d_h, x_h = host.step(a_np, aux=True)
        a = torch.from_numpy(a_np).cuda()
        if k % 2:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                out = dev.step(a, aux=True)
            torch.cuda.current_stream().wait_stream(stream)
        else:
            out = dev.step(a, aux=True)
        assert out[0].data_ptr() == dev._torch["obs"].data_ptr() and tuple(out[1].shape) == (R, P)
        o_d, r_d, d_d, x_d = (t.cpu().numpy() for t in out)
        assert same_bits(o_d, o_h) and same_bits(r_d, r_h) and same_bits(d_d, d_h) and same_bits(x_d, x_h), k
        over |= set(same_reads(k + 1)["race_over"].tolist())
    assert 0 in over and len(over) > 1
    # seeded draws on the device form, the per-car rows as actions, and a NumPy step on the env that stepped on the device
    assert same_bits(dev.reset(seed=4, on_device=True).cpu().numpy(), host.reset(seed=4))
    o1, r1, d1 = dev.step(actions[10])
    o2, r2, d2 = (t.cpu().numpy() for t in host.step(torch.from_numpy(actions[10]).cuda()))
    assert o1.shape == (R, P, 45) and same_bits(o1, o2) and same_bits(r1, r2) and same_bits(d1, d2)
    with pytest.raises(ValueError):
        dev.reset(start_index=torch.zeros(N, dtype=torch.int32).cuda())       # one index per race, not per car
    m.set_noise(0.0, 0, 0)


# ---------------------------------------------------------------- 7. refusals
def test_race_env_errors_leave_everything_usable():
    g = DC.race_maze()
    omap = range_libc.PyOMap(g)
    dt = omap.distance_transform()
    R, P, B, M = 5, 3, 100, 4
    N = R * P
    pool = lineups(g, dt, M, P, 5)
    edge = support.edge(B)
    actions = DC.actions(3, 6, N).reshape(6, R, P, 2)
    mA, mB = range_libc.PyRayMarchingGPU(omap, MRX), range_libc.PyRayMarchingGPU(omap, MRX)
    carsA, carsB = RC.CarBatch(), RC.CarBatch()
    for m in (mA, mB):
        m.set_noise(0.05, 7, 321)
    kw = dict(substeps=2, max_ticks=5, crash_reward=-4.0, obs_window=(0, 50, 2), min_running=2)
    A = RaceEnv(mA, pool, R, B, FOV, edge, THRESH, car=carsA, **kw)
    Bt = RaceEnv(mB, pool, R, B, FOV, edge, THRESH, car=carsB, **kw)
    Lb = _lib.lib()
    f64p, i32p = _lib.f64p, _lib.i32p
    race_buf = np.empty(R, np.int32)

    def refused(rc, code=RL_ERR_INVALID):
        assert rc == code, rc
        with pytest.raises(_lib.ScanLibError):
            _lib.check(rc)

    def create(h=mA._h, car=carsA._h, starts=pool, n_starts=M, group=P, min_running=2, **over):
        rp = _lib.RaceEnvParams()
        rp.env = _lib.EnvParams.from_buffer_copy(A.params)
        rp.group, rp.min_running = group, min_running
        for key, v in over.items():
            setattr(rp.env, key, v)
        handle = C.c_void_p()
        rc = Lb.rl_env_create_race(car, h, C.byref(rp), edge.ctypes.data_as(f64p), starts.ctypes.data_as(f64p), n_starts,
                                   C.byref(handle))
        assert not handle.value or rc == 0
        if handle.value:
            Lb.rl_env_destroy(handle)
        return rc

    def run(env, steps):
        return [env.step(actions[k], aux=True) for k in steps]

    def same(xs, ys):
        for x, y in zip(xs, ys):
            for a, b in zip(x, y):
                assert same_bits(a, b)

    # rl_env_read_races before a reset, and on an env that is no race env
    refused(Lb.rl_env_read_races(A._h, race_buf.ctypes.data_as(i32p), None, None, None))
    refused(Lb.rl_env_read_races(None, None, None, None, None))
    plain = DriveEnv(mA, pool.reshape(-1, 11), N, B, FOV, edge, THRESH, car=carsA)
    plain.reset(seed=1)
    refused(Lb.rl_env_read_races(plain._h, race_buf.ctypes.data_as(i32p), None, None, None))
    plain.close()

    assert create() == 0
    assert same_bits(A.reset(seed=5), Bt.reset(seed=5))
    same(run(A, (0, 1)), run(Bt, (0, 1)))

    # the race constructor's own refusals, and one of rl_env_create's through it
    for over in (dict(group=0), dict(group=9), dict(group=-1), dict(group=2), dict(group=4), dict(min_running=0),
                 dict(min_running=P + 1), dict(n_envs=N + 1), dict(n_envs=0), dict(substeps=0), dict(num_rays=9),
                 dict(obs_count=51), dict(max_ticks=-1), dict(n_starts=0)):
        refused(create(**over))
    bad = pool.copy()
    bad[M - 1, P - 1, 5] = np.inf                                   # the pool's last row: M * P rows are read
    refused(create(starts=bad))
    refused(Lb.rl_env_create_race(carsA._h, mA._h, None, edge.ctypes.data_as(f64p), pool.ctypes.data_as(f64p), M,
                                  C.byref(C.c_void_p())))
    multi = RC.CarBatch(device=[0])
    refused(create(car=multi._h))
    # the race scan's refusals come back with their codes, at create and through the class
    for cls, args in ((range_libc.PyCDDTCast, (112,)), (range_libc.PyGiantLUTCast, (112,)),
                      (range_libc.PyBresenhamsLine, ())):
        h = cls(omap, MRX, *args)
        refused(create(h=h._h), RL_ERR_UNSUPPORTED)
        with pytest.raises(_lib.ScanLibError) as e:
            RaceEnv(h, pool, R, B, FOV, edge, THRESH)
        assert e.value.code == RL_ERR_UNSUPPORTED and "ray marching" in str(e.value)
    # ... while an ordinary DriveEnv still runs on a table method
    cddt = range_libc.PyCDDTCast(omap, MRX, 112)
    d1 = DriveEnv(cddt, pool.reshape(-1, 11), N, B, FOV, edge, THRESH)
    d1.reset(seed=2)
    obs, rew, dn = d1.step(actions[0].reshape(N, 2))
    assert obs.shape == (N, B) and np.isfinite(obs).all() and (rew[dn == 0] >= 0).all()
    d1.close()
    mv = range_libc.PyRayMarchingGPU(omap, MRX)
    mv.set_option("variant", 2)
    refused(create(h=mv._h), RL_ERR_UNSUPPORTED)
    long_car = RC.CarBatch(dict(length=30.0))
    refused(create(car=long_car._h), RL_ERR_UNSUPPORTED)            # more than 512 outline points
    # variant 2 set on a running env's method: the step is refused with the code, and goes on once it is taken back
    v0 = mA.get_info("variant")
    mA.set_option("variant", 2)
    with pytest.raises(_lib.ScanLibError) as e:
        A.step(actions[2])
    assert e.value.code == RL_ERR_UNSUPPORTED
    mA.set_option("variant", v0)

    # start indices: one per race, inside the pool (host form)
    for v in (-1, M):
        sidx = np.zeros(R, np.int32)
        sidx[R - 1] = v
        obs_buf, done_buf = np.empty((N, 50), np.float32), np.empty(N, np.int32)
        refused(Lb.rl_env_reset(A._h, 0, sidx.ctypes.data_as(i32p), obs_buf.ctypes.data_as(_lib.f32p), None,
                                done_buf.ctypes.data_as(i32p)))
        with pytest.raises(ValueError):
            A.reset(start_index=sidx)
    with pytest.raises(ValueError):
        A.reset(start_index=np.zeros(N, np.int32))
    with pytest.raises(ValueError):
        A.step(actions[0].astype(np.float64))
    with pytest.raises(ValueError):
        A.step(actions[0][:-1])
    with pytest.raises(ValueError):
        RaceEnv(mA, pool, R, B, FOV, edge, THRESH, min_running=P + 1)

    # the env that saw all this answers as its twin
    same(run(A, (2, 3, 4)), run(Bt, (2, 3, 4)))
    rd_a, rd_b = A.read(), Bt.read()
    for key in rd_a:
        assert same_bits(rd_a[key], rd_b[key]), key
    poses = support.lidar_poses(pool.reshape(-1, 11))
    sa, sb = np.empty(M * P * B, np.float32), np.empty(M * P * B, np.float32)
    mA.calc_range_fan(poses, sa, FOV, B)
    mB.calc_range_fan(poses, sb, FOV, B)
    assert same_bits(sa, sb)
    for m in (mA, mB):
        m.set_noise(0.0, 0, 0)


# ---------------------------------------------------------------- 8. the facade
def test_race_env_facade_matches_hand_built():
    """RacecarSimulator(cfg).raceEnv(...) is a RaceEnv on the simulator's method, car, fan, edge table and thresholds."""
    g = DC.race_maze()
    cfg = dict(RC.DEFAULT_CAR)
    cfg.update(scan_dist_to_base=D_BASE, batch_size=40, scan_beams=1080, scan_fov=FOV, scan_std=0.01,
               scan_max_range=15.0, free_thresh=0.8)
    sim = RacecarSimulator(cfg)
    omap = range_libc.PyOMap(g)
    sim.setMap(omap, g.resolution, g.origin)
    sim.setRaytracingMethod("RMGPU")
    R, P = 4, 3
    pool = lineups(g, omap.distance_transform(), 3, P, 21)
    kw = dict(substeps=2, obs_window=(180, 720, 1), obs_clip=15, obs_scale=15, max_ticks=3, crash_reward=-1.0,
              min_running=2)
    env = sim.raceEnv(R, pool, **kw)
    assert isinstance(env, RaceEnv) and env.obs_shape == (R * P, 720) and env.group == P
    hand = RaceEnv(sim.scan_simulator.scan_method, pool, R, 1080, FOV, sim.edge_distances, cfg["ttc_thresh"],
                   car=sim.car, scan_dist_to_base=D_BASE, **kw)
    actions = DC.actions(21, 5, R * P).reshape(5, R, P, 2)
    assert same_bits(env.reset(seed=2), hand.reset(seed=2))
    for a in actions:
        for x, y in zip(env.step(a, aux=True), hand.step(a, aux=True)):
            assert same_bits(x, y)
    rd_a, rd_b = env.read(), hand.read()
    for key in rd_a:
        assert same_bits(rd_a[key], rd_b[key]), key
    assert (rd_a["race_episodes"] > 0).any()
