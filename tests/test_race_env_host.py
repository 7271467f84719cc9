"""The race environment's host side (no GPU): the statement's state machine (tests/race_env_statement.py) on a fake
one-dimensional world through every case of the header section, RaceEnv's argument checks and rl_race_env_params'
layout."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import env_statement as E
import race_env_statement as RE
from pyracecarsimulator_amd import _lib
from pyracecarsimulator_amd import env as ENV

WALL, B, EDGE, THRESH = 10.0, 10, 0.5, 0.001


class World1D:
    """x along a corridor towards a wall at WALL: a step moves speed / 10 (either way), every beam reads the nearer of
    the wall and the closest other car of the race."""

    def __init__(self, group):
        self.P = group
        self.slots = []

    def step_cars(self, states, speed, steer):
        out = states.copy()
        dx = speed * 0.1
        out[:, 0] += dx
        out[:, 4] = steer
        out[:, 8] += np.abs(dx)
        return out

    def scan(self, poses, cars, k):
        self.slots.append(k)
        x = cars[:, 0].reshape(-1, self.P)
        gap = np.abs(x[:, :, None] - x[:, None, :])
        gap[:, np.arange(self.P), np.arange(self.P)] = np.inf
        r = np.minimum(WALL - x, gap.min(2)).reshape(-1)
        assert np.array_equal(poses[:, 0], cars[:, 0].astype(np.float32))     # (scan_dist_to_base = 0 here)
        return np.repeat(r[:, None], B, 1).astype(np.float32)

    @staticmethod
    def is_crashed(r):
        return bool(((r.astype(np.float64) - EDGE) < THRESH).any())


def _lineup(*xs):
    s = np.zeros((len(xs), 11))
    s[:, 0] = xs
    return s


def _env(lineups, n_races, **kw):
    starts = np.stack(lineups)
    w = World1D(starts.shape[1])
    return RE.RaceEnvStatement(starts, n_races, B, w.step_cars, w.scan, w.is_crashed, scan_dist_to_base=0.0, **kw), w


def _acts(*speeds):
    return np.stack([np.float32(speeds), np.zeros(len(speeds), np.float32)], -1)


def test_same_step_double_crash_reads_one_for_both():
    env, w = _env([_lineup(0.0, 2.0)], 1, crash_reward=-3.0, auto_reset=False)
    obs, done = env.reset(seed=1, start_index=[0])
    assert done.tolist() == [0, 0] and env.race_over.tolist() == [0]
    assert obs[0, 0] == np.float32(2.0) and obs[1, 0] == np.float32(2.0)       # each sees the other, not the wall
    obs, rew, done = env.step(_acts(5.0, -5.0))
    assert done.tolist() == [0, 0] and rew.tolist() == [0.5, 0.5] and env.race_over.tolist() == [0]
    obs, rew, done = env.step(_acts(5.0, -5.0))                               # both at x = 1
    assert done.tolist() == [1, 1] and rew.tolist() == [-3.0, -3.0]
    assert env.race_over.tolist() == [1] and env.race_tick.tolist() == [2] and env.tick.tolist() == [2, 2]


@pytest.mark.parametrize("min_running", [1, 2, 3])
def test_attrition_ends_the_race_below_min_running(min_running):
    """Three cars at x = 0, 3 and 8.9 moving 1.0, 2.0 and 0.6 m a step: car 2 enters the wall's margin on step 1
    (x = 9.5), car 1 comes within 0.5 m of that wreck on step 3 (x = 9), car 0 is still far away after step 4."""
    env, w = _env([_lineup(0.0, 3.0, 8.9)], 1, min_running=min_running, crash_reward=-1.0, auto_reset=False)
    env.reset(seed=0, start_index=[0])
    a = _acts(10.0, 20.0, 6.0)
    log = []
    while len(log) < 4 and not env.race_over[0]:
        obs, rew, done = env.step(a)
        log.append((done.tolist(), rew.tolist(), int(env.race_over[0])))
    want = {
        # one car still runs after step 3: the race goes on; a wreck reads reward 0
        1: [([0, 0, 1], [1.0, 2.0, -1.0], 0), ([0, 0, 1], [1.0, 2.0, 0.0], 0), ([0, 1, 1], [1.0, -1.0, 0.0], 0),
            ([0, 1, 1], [1.0, 0.0, 0.0], 0)],
        # the second crash ends it: the survivor reads 2 and keeps the distance of the step
        2: [([0, 0, 1], [1.0, 2.0, -1.0], 0), ([0, 0, 1], [1.0, 2.0, 0.0], 0), ([2, 1, 1], [1.0, -1.0, 0.0], 1)],
        # the first crash ends it
        3: [([2, 2, 1], [1.0, 2.0, -1.0], 1)],
    }[min_running]
    assert log == want
    assert env.tick[2] == 1 and env.states[2, 0] == 9.5                        # the wreck stood where it crashed
    assert env.race_tick[0] == len(log)


def test_truncation_beats_attrition():
    # max_ticks = 2: on step 2 car 1 crashes (running 1 < min_running 2) and the race tick reaches max_ticks
    env, w = _env([_lineup(0.0, 8.5)], 1, min_running=2, max_ticks=2, crash_reward=-2.0, auto_reset=False)
    env.reset(seed=0, start_index=[0])
    obs, rew, done = env.step(_acts(5.0, 5.0))
    assert done.tolist() == [0, 0] and env.race_over[0] == 0
    obs, rew, done = env.step(_acts(5.0, 5.0))                                 # x = 1.0, 9.5
    assert done.tolist() == [2, 1] and rew.tolist() == [0.5, -2.0]
    assert env.race_over[0] == RE.RACE_TRUNCATED
    # the same run without the tick limit: attrition, and the survivor reads 2 as well
    env, w = _env([_lineup(0.0, 8.5)], 1, min_running=2, crash_reward=-2.0, auto_reset=False)
    env.reset(seed=0, start_index=[0])
    env.step(_acts(5.0, 5.0))
    obs, rew, done = env.step(_acts(5.0, 5.0))
    assert done.tolist() == [2, 1] and rew.tolist() == [0.5, -2.0] and env.race_over[0] == RE.RACE_ATTRITION
    # a wreck from before the max_ticks step keeps its code: truncation touches stepped cars only
    env, w = _env([_lineup(0.0, 9.0)], 1, max_ticks=2, auto_reset=False)
    env.reset(seed=0, start_index=[0])
    assert env.step(_acts(5.0, 5.0))[2].tolist() == [0, 1]
    obs, rew, done = env.step(_acts(5.0, 5.0))
    assert done.tolist() == [2, 1] and rew.tolist() == [0.5, 0.0] and env.race_over[0] == RE.RACE_TRUNCATED


def test_invalid_action_turns_a_car_into_a_wreck():
    env, w = _env([_lineup(0.0, 2.0)], 1, crash_reward=-4.0, auto_reset=False, steer_clip=0.25)
    env.reset(seed=0, start_index=[0])
    a = _acts(5.0, np.nan)
    a[0, 1] = 0.9
    before = env.states.copy()
    obs, rew, done = env.step(a)
    assert done.tolist() == [0, 3] and rew.tolist() == [0.5, -4.0] and env.race_over[0] == 0
    assert (env.states[1] == before[1]).all() and env.tick.tolist() == [1, 0]
    assert env.states[0, 4] == 0.25                                            # the steer was clamped
    # the wreck's later actions are ignored, finite or not; the other car runs into it where it stands
    obs, rew, done = env.step(_acts(5.0, 5.0))
    assert done.tolist() == [0, 3] and rew.tolist() == [0.5, 0.0] and env.states[1, 0] == 2.0
    obs, rew, done = env.step(_acts(5.0, np.inf))
    assert done.tolist() == [1, 3] and rew.tolist() == [-4.0, 0.0]             # x = 1.5: 0.5 from the wreck
    assert env.race_over[0] == 1 and env.race_tick[0] == 3 and env.tick.tolist() == [3, 0]


def test_whole_race_respawns_with_the_race_draw():
    pool = [_lineup(0.0, 9.0), _lineup(1.0, 5.0), _lineup(2.0, 6.0)]
    env, w = _env(pool, 3, max_ticks=3, auto_reset=True, crash_reward=-1.0)
    seed = 4
    env.reset(seed=seed, start_index=[0, 1, 2])
    a = _acts(*([5.0] * 6))
    obs, rew, done = env.step(a)                                   # race 0: car 1 hits the wall, car 0 runs on
    assert done.tolist() == [0, 1, 0, 0, 0, 0] and env.race_over.tolist() == [0, 0, 0]
    env.step(a)
    obs, rew, done = env.step(a)                                   # race tick 3: everything truncates
    assert done.tolist() == [2, 1, 2, 2, 2, 2] and env.race_over.tolist() == [2, 2, 2]
    assert env.tick.tolist() == [3, 1, 3, 3, 3, 3] and env.race_tick.tolist() == [3, 3, 3]
    obs, rew, done = env.step(a)                                   # every race spawns as a whole with q = 1
    for r in range(3):
        idx = E.spawn_index(seed, r, 1, 3)
        assert env.race_start_index[r] == idx and env.race_episode[r] == 1 and env.race_tick[r] == 0
        for c in range(2):
            e = 2 * r + c
            assert (env.states[e] == pool[idx][c]).all() and env.tick[e] == 0 and rew[e] == 0.0
            assert env.episode[e] == 1 and env.start_index[e] == idx
            assert obs[e, 0] == np.float32(min(WALL - pool[idx][c, 0], abs(pool[idx][0, 0] - pool[idx][1, 0])))
    assert (done == 0).all() and (env.race_over == 0).all()        # (no line-up of the pool is over at its spawn)
    assert w.slots == list(range(5))
    # without start indices the reset draws (r, 0)
    env.reset(seed=9)
    assert env.race_start_index.tolist() == [E.spawn_index(9, r, 0, 3) for r in range(3)]
    with pytest.raises(ValueError):
        env.reset(seed=9, start_index=[0, 3, 0])


def test_finished_races_stand_without_auto_reset():
    env, w = _env([_lineup(0.0, 9.0), _lineup(0.0, 4.0)], 2, min_running=2, auto_reset=False, crash_reward=-1.0)
    env.reset(seed=0, start_index=[0, 1])
    a = _acts(5.0, 5.0, 5.0, 5.0)
    obs, rew, done = env.step(a)
    assert done.tolist() == [2, 1, 0, 0] and env.race_over.tolist() == [1, 0] and rew.tolist() == [0.5, -1.0, 0.5, 0.5]
    before = env.states.copy()
    for k in range(2, 5):
        obs, rew, done = env.step(a)
        assert done.tolist() == [2, 1, 0, 0] and env.race_over.tolist() == [1, 0]
        assert rew.tolist() == [0.0, 0.0, 0.5, 0.5]
        assert (env.states[:2] == before[:2]).all() and env.tick.tolist() == [1, 1, k, k]
        assert env.race_tick.tolist() == [1, k]
        assert obs[0, 0] == np.float32(9.0) and obs[1, 0] == np.float32(0.5)   # scanned again where they stand
    assert w.slots == list(range(5))


def test_a_lineup_that_is_over_at_the_reset():
    # race 0: two cars 0.3 m apart, both crashed at the spawn.  race 1 (min_running = 2): one car inside the wall's
    # margin, so the other reads 2 at the reset
    env, w = _env([_lineup(1.0, 1.3), _lineup(0.0, 9.6)], 2, min_running=2, auto_reset=True, crash_reward=-1.0)
    obs, done = env.reset(seed=3, start_index=[0, 1])
    assert done.tolist() == [1, 1, 2, 1] and env.race_over.tolist() == [1, 1]
    assert env.tick.tolist() == [0] * 4 and env.race_tick.tolist() == [0, 0]
    obs, rew, done = env.step(_acts(5.0, 5.0, 5.0, 5.0))                     # both races re-spawn: fresh, reward 0
    assert (rew == 0).all() and env.race_episode.tolist() == [1, 1] and (env.tick == 0).all()
    for r in range(2):
        idx = E.spawn_index(3, r, 1, 2)
        assert env.race_start_index[r] == idx
        assert done[2 * r:2 * r + 2].tolist() == ([1, 1] if idx == 0 else [2, 1])   # over again, at the spawn
    assert env.race_over.tolist() == [1, 1]
    # the same line-ups with min_running = 1: race 1 runs with one car and a wreck
    env, w = _env([_lineup(1.0, 1.3), _lineup(0.0, 9.6)], 2, min_running=1, auto_reset=False)
    obs, done = env.reset(seed=3, start_index=[0, 1])
    assert done.tolist() == [1, 1, 0, 1] and env.race_over.tolist() == [1, 0]


def test_a_race_of_one_is_the_env_statement():
    """P = 1, min_running = 1: every output and counter of the env's statement on the same world, with crashes,
    truncation, a NaN action and re-spawns."""
    pool = np.stack([_lineup(0.0), _lineup(7.6), _lineup(9.8), _lineup(1.0), _lineup(8.9)])
    N = 7
    kw = dict(max_ticks=4, auto_reset=True, crash_reward=-3.0, steer_clip=0.25, obs_window=(1, 4, 2))
    race, w = _env(list(pool), N, **kw)
    w1 = World1D(1)
    one = E.EnvStatement(pool[:, 0], N, B, w1.step_cars, lambda poses, k: w1.scan(poses, one.states[:, :3], k),
                         w1.is_crashed, scan_dist_to_base=0.0, **kw)
    o_r, d_r = race.reset(seed=5)
    o_1, d_1 = one.reset(seed=5)
    assert o_r.tobytes() == o_1.tobytes() and d_r.tolist() == d_1.tolist()
    rng = np.random.default_rng(2)
    codes = set()
    for k in range(14):
        a = np.stack([rng.uniform(0.0, 9.0, N), rng.uniform(-0.5, 0.5, N)], -1).astype(np.float32)
        if k == 3:
            a[2, 0] = np.nan
        got, want = race.step(a), one.step(a)
        for x, y in zip(got, want):
            assert x.tobytes() == y.tobytes(), k
        for x, y in ((race.states, one.states), (race.tick, one.tick), (race.episode, one.episode),
                     (race.start_index, one.start_index), (race.race_episode, one.episode)):
            assert x.tobytes() == y.tobytes(), k
        assert ((race.race_over != 0) == (one.done != 0)).all()
        codes |= set(got[2].tolist())
    assert codes == {0, 1, 2, 3} and (race.episode > 0).all()


def test_statement_refuses_a_step_before_reset():
    env, w = _env([_lineup(0.0, 2.0)], 2)
    with pytest.raises(RuntimeError):
        env.step(np.zeros((4, 2), np.float32))


# ---------------------------------------------------------------- RaceEnv's argument checks
def test_race_env_params_layout_matches_the_header():
    # rl_env_params (88 bytes, tests/test_env_host.py) then two ints
    assert C.sizeof(_lib.RaceEnvParams) == 96
    assert _lib.RaceEnvParams.env.offset == 0 and _lib.RaceEnvParams.group.offset == 88
    assert _lib.RaceEnvParams.min_running.offset == 92
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "scanlib.h")).read()
    body = re.search(r"typedef struct rl_race_env_params \{(.*?)\} rl_race_env_params;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [decl.split()[-1] for decl in body.split(";") if decl.strip()]
    assert fields == [n for n, _ in _lib.RaceEnvParams._fields_] == ["env", "group", "min_running"]
    assert _lib.RaceEnvParams._fields_[0][1] is _lib.EnvParams
    assert "rl_env_params env" in body


def test_race_env_argument_checks():
    starts = np.zeros((5, 3, 11))
    edge = np.zeros(100)
    st, ed, win, P = ENV.race_env_args(23, 100, starts, edge, 2)
    assert P == 3 and st.shape == (5, 3, 11) and ed.shape == (100,) and win == (0, 100, 1)
    assert ENV.race_env_args(1, 100, np.zeros((1, 8, 11)), edge, 8, obs_window=(7, 40, 2))[2:] == ((7, 40, 2), 8)
    assert ENV.race_env_args(4, 100, np.zeros((2, 1, 11)), edge)[3] == 1
    bad = [dict(n_races=0), dict(n_races=1.5), dict(min_running=0), dict(min_running=4), dict(min_running=1.5),
           dict(starts=np.zeros((5, 11))), dict(starts=np.zeros((5, 9, 11))), dict(starts=np.zeros((5, 0, 11))),
           dict(starts=np.zeros((0, 3, 11))), dict(starts=np.zeros((5, 3, 10))), dict(starts=starts.astype(np.float32)),
           dict(num_rays=9), dict(num_rays=1281), dict(substeps=0), dict(max_ticks=-1), dict(obs_window=(7, 48, 2)),
           dict(steer_clip=-0.1), dict(crash_reward=float("nan")), dict(dt=float("inf")), dict(edge=edge[:-1]),
           dict(n_races=(1 << 31) // 300 + 1)]
    for kw in bad:
        args = dict(n_races=23, num_rays=100, starts=starts, edge=edge, min_running=1)
        args.update(kw)
        with pytest.raises(ValueError):
            ENV.race_env_args(**args)
    nf = starts.copy()
    nf[4, 2, 7] = np.nan
    with pytest.raises(ValueError):
        ENV.race_env_args(23, 100, nf, edge)


def test_package_exports_the_race_environment():
    import pyracecarsimulator_amd as P
    assert P.RaceEnv is ENV.RaceEnv and "RaceEnv" in P.__all__ and issubclass(P.RaceEnv, P.DriveEnv)
    assert hasattr(P.RacecarSimulator, "raceEnv")
    for name in ("rl_env_create_race", "rl_env_read_races"):
        assert name in _lib.SYMBOLS and getattr(_lib.lib(), name) is not None
