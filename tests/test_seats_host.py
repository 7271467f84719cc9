"""Per-seat drivers without a GPU: the statement (tests/seat_statement.py) on a fake one-dimensional world,
what include/scanlib_seats.h says beyond its prototypes (tests/test_py_calls_host.py pins those to
``_lib.SEAT_SYMBOLS``), and every Python-side refusal."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import race_env_statement as RE
import scanlib_header as H
import seat_statement as SS
from test_population_host import no_calls  # noqa: F401  (a fixture)
from test_race_env_host import B, World1D, _acts, _lineup
from pyracecarsimulator_amd import _lib, seats
from pyracecarsimulator_amd import racecar as RC
from pyracecarsimulator_amd.env import RaceEnv
from pyracecarsimulator_amd.followgap import PyFollowGap
from pyracecarsimulator_amd.policy import Policy

SEAT_HEADER = H.read("scanlib_seats.h")


# ---------------------------------------------------------------- the statement on the fake world
def hundredth(row):
    """A driver: a hundredth of the first beam."""
    return np.float32(row[0]) / np.float32(100.0)


def tenth(row):
    return np.float32(row[0]) / np.float32(10.0)


def shy(row):
    """A driver that gives up within 3 m of anything."""
    return np.float32(np.inf) if row[0] < 3.0 else np.float32(0.125)


def _answer(driver, row):
    assert row.shape == (B,) and row.dtype == np.float32         # the whole scan, whatever the window shows
    return driver(row)


def _seated(lineups, n_races, drivers, speed, **kw):
    starts = np.stack(lineups)
    w = World1D(starts.shape[1])
    env = SS.SeatEnvStatement(starts, n_races, B, w.step_cars, w.scan, w.is_crashed, _answer, drivers, speed,
                              scan_dist_to_base=0.0, **kw)
    return env, w


def test_scripted_car_takes_its_drivers_pair_and_never_reads_its_row():
    """Two cars 6 m apart, car 1 scripted at 5 m/s away from car 0... towards the wall at 10: its steer (World1D keeps it
    in state[4]) is the driver's answer to the scan of the call BEFORE, its row of the actions is NaN throughout, and a
    plain statement fed the pairs agrees in everything."""
    env, _ = _seated([_lineup(0.0, 6.0)], 1, [None, hundredth], [9.0, 5.0], auto_reset=False, obs_window=(0, 2, 1))
    plain, _ = _seated([_lineup(0.0, 6.0)], 1, [None, None], 0.0, auto_reset=False, obs_window=(0, 2, 1))
    obs, done = env.reset(seed=0, start_index=[0])
    plain.reset(seed=0, start_index=[0])
    assert obs.shape == (2, 2) and done.tolist() == [0, 0]
    assert np.isnan(env.seat_steers()[0]) and env.seat_steers()[1] == np.float32(0.04)      # wall 4 m, car 6 m away
    a = _acts(1.0, np.nan)
    a[1, 1] = np.nan
    for k in range(1, 4):
        before = env.seat_steers()
        obs, rew, done = env.step(a)
        assert done.tolist() == [0, 0], k
        assert env.states[1, 0] == 6.0 + 0.5 * k and env.states[0, 0] == 0.1 * k       # seat_speed 5, the caller's 1
        assert np.float32(env.states[1, 4]) == before[1], k                             # the answer of the call before
        assert rew.tolist() == [np.float32(0.1), np.float32(0.5)]
        want = plain.step(env.fed)
        assert all(np.array_equal(x, y) for x, y in zip((obs, rew, done), want)) and np.array_equal(env.states, plain.states)
        assert env.fed[1].tolist() == [5.0, float(before[1])]
        assert env.seat_steers()[1] == np.float32(np.float32(10.0 - env.states[1, 0]) / np.float32(100.0))
    assert env.tick.tolist() == [3, 3]


def test_fresh_car_ignores_its_answer_and_a_wreck_reads_nan():
    """Car 1 scripted runs into the wall's margin on step 2; min_running 2 ends the race there, the re-spawn on step 3
    is fresh (no step, whatever the answer), and step 4 takes the answer to the fresh scan."""
    env, _ = _seated([_lineup(0.0, 8.5)], 1, [None, tenth], 5.0, min_running=2, auto_reset=True, crash_reward=-1.0)
    env.reset(seed=0, start_index=[0])
    assert env.seat_steers()[1] == np.float32(0.15)
    a = _acts(0.0, np.nan)
    obs, rew, done = env.step(a)                                   # x = 9.0: one metre from the wall
    assert done.tolist() == [0, 0] and env.seat_steers()[1] == np.float32(0.1)
    obs, rew, done = env.step(a)                                   # x = 9.5: inside the margin
    assert done.tolist() == [2, 1] and rew.tolist() == [0.0, -1.0] and env.race_over.tolist() == [RE.RACE_ATTRITION]
    assert np.isnan(env.seat_steers()).all()                       # a wreck, and a survivor of a finished race
    obs, rew, done = env.step(a)                                   # the re-spawn: fresh, nothing steps
    assert done.tolist() == [0, 0] and env.states[:, 0].tolist() == [0.0, 8.5] and env.tick.tolist() == [0, 0]
    assert np.isnan(env.fed[1, 1]) and env.race_episode.tolist() == [1]
    assert env.seat_steers()[1] == np.float32(0.15)
    obs, rew, done = env.step(a)
    assert env.states[1, 0] == 9.0 and np.float32(env.states[1, 4]) == np.float32(0.15)

    # a wreck in a race that runs on: its answer reads NaN, it stands, the other scripted car drives on
    env, _ = _seated([_lineup(0.0, 9.2)], 1, [hundredth, hundredth], [1.0, 5.0], min_running=1, auto_reset=False)
    env.reset(seed=0, start_index=[0])
    obs, rew, done = env.step(np.full((2, 2), np.nan, np.float32))
    assert done.tolist() == [0, 1] and env.race_over.tolist() == [0]
    s = env.seat_steers()
    assert np.isnan(s[1]) and s[0] == np.float32(np.float32(9.6) / np.float32(100.0))    # car 0 sees the wreck at 9.7
    obs, rew, done = env.step(np.full((2, 2), np.nan, np.float32))
    assert done.tolist() == [0, 1] and env.states[1, 0] == 9.7 and env.tick.tolist() == [2, 1]
    assert np.float32(env.states[0, 4]) == s[0]


def test_non_finite_answer_reads_done_3():
    env, _ = _seated([_lineup(0.0, 6.4)], 1, [None, shy], 5.0, auto_reset=False, crash_reward=-4.0)
    env.reset(seed=0, start_index=[0])
    a = _acts(0.0, 0.0)
    obs, rew, done = env.step(a)                                   # x = 6.9: 3.1 m from the wall
    assert done.tolist() == [0, 0] and env.seat_steers()[1] == np.float32(0.125)
    obs, rew, done = env.step(a)                                   # x = 7.4: the driver answers inf
    assert done.tolist() == [0, 0] and np.isinf(env.seat_steers()[1])
    before = env.states.copy()
    obs, rew, done = env.step(a)                                   # the pair is refused like a caller's
    assert done.tolist() == [0, 3] and rew.tolist() == [0.0, -4.0] and np.array_equal(env.states, before)
    assert np.isnan(env.seat_steers()[1])                          # a wreck from here on
    obs, rew, done = env.step(a)
    assert done.tolist() == [0, 3] and rew.tolist() == [0.0, 0.0]


def test_seated_rollout_statement():
    """Three cars a race, two races: car n gets seat n % 3's driver (not n // 3's), the clip touches the clipped
    driver's seats only, the steers record the raw answers, a wreck stops."""
    w = World1D(3)
    states = np.concatenate([_lineup(0.0, 3.0, 8.0), _lineup(1.0, 4.0, 6.0)])
    speeds = np.array([1.0, 1.0, 5.0, 1.0, 1.0, 1.0])
    drivers = [hundredth, tenth, hundredth]
    first, final, steers, trace = SS.seated_rollout(
        states, speeds, np.zeros(6, np.float32), 4, drivers, lambda d: d is tenth, 0.125, w.step_cars, w.scan,
        w.is_crashed, _answer, scan_dist_to_base=0.0)
    assert w.slots == [0, 1, 2, 3]
    assert first.tolist() == [-5, -5, 2, -5, -5, -5]               # car 2: 8.5, 9.0, 9.5
    assert np.isnan(steers[2, 2:]).all() and np.isnan(trace[2, 3]).all() and final[2, 0] == 9.5
    # tick 0: car 1 sees car 0 at 3 m (x = 0.1, 3.1): tenth answers 0.3, clamped to 0.125 at the step of tick 1
    assert steers[1, 0] == np.float32(0.3) and trace[1, 1, 4] == 0.125
    # car 3 (race 1, seat 0) is hundredth's: 3 m to car 4, unclamped
    assert steers[3, 0] == np.float32(0.03) and np.float32(trace[3, 1, 4]) == np.float32(0.03)
    # car 4 (seat 1) is tenth's: 2 m to car 5 -> 0.2, clamped
    assert steers[4, 0] == np.float32(0.2) and trace[4, 1, 4] == 0.125
    assert trace[0, 0, 4] == 0.0 and np.array_equal(final[[0, 1, 3, 4, 5]], trace[[0, 1, 3, 4, 5], 3])


# ---------------------------------------------------------------- the header
def test_seats_header_is_pinned_to_seat_symbols():
    protos = SEAT_HEADER.prototypes()
    # rl_car_race_seats: rl_car_race_followgap's arguments from states_in on, behind its own six
    names = protos["rl_car_race_seats"][2]
    assert names[:6] == ["c", "h", "g_or_null", "p_or_null", "seat_driver", "steer_clip"]
    assert protos["rl_car_race_seats"][1][6:] == _lib.SYMBOLS["rl_car_race_followgap"][1][3:]
    declared = SEAT_HEADER.structs()
    assert set(declared) == {"rl_seat_params"}
    assert [n for n, _ in _lib.SeatParams._fields_] == [n for n, _ in declared["rl_seat_params"]] == ["driver", "speed"]
    assert C.sizeof(_lib.SeatParams) == 64
    # the driver codes: one plain enum, restated as a dictionary and in seats.py, never as RL_* names of _lib
    m = re.search(r"enum\s+rl_seat_driver\s*\{([^{}]*)\}\s*;", SEAT_HEADER.text())
    codes = {k.strip(): int(v) for k, v in (item.split("=") for item in m.group(1).split(","))}
    assert codes == {"RL_SEAT_CALLER": 0, "RL_SEAT_FOLLOWGAP": 1, "RL_SEAT_POLICY": 2}
    assert _lib.SEAT_DRIVERS == {"caller": 0, "followgap": 1, "policy": 2}
    assert (seats.SEAT_CALLER, seats.SEAT_FOLLOWGAP, seats.SEAT_POLICY) == (0, 1, 2)
    assert not [n for n in vars(_lib) if n.startswith("RL_") and "SEAT" in n]
    # the header carries its contract and builds on scanlib.h
    raw = open(SEAT_HEADER.path).read()
    assert '#include "scanlib.h"' in raw and "The rule." in raw and raw.count("Errors (RL_ERR_INVALID") == 2


# ---------------------------------------------------------------- the wrappers' refusals
def _drivers():
    """A FollowGap and a policy object (window [5, 45)) that never saw the library."""
    fg, pol = PyFollowGap.__new__(PyFollowGap), Policy.__new__(Policy)
    pol.in_start, pol.dims = 5, (40, 8, 1)
    return fg, pol


def test_seat_args(no_calls):
    fg, pol = _drivers()
    codes, g, p = seats.seat_args([fg, pol, fg], 3, 64, caller_ok=False)
    assert codes.tolist() == [1, 2, 1] and codes.dtype == np.int32 and g is fg and p is pol
    codes, g, p = seats.seat_args([None, fg], 2, 10, caller_ok=True)
    assert codes.tolist() == [0, 1] and g is fg and p is None
    assert seats.seat_args([pol], 1, 45, caller_ok=False)[0].tolist() == [2]
    fg2, pol2 = _drivers()
    for drivers, group, rays, caller_ok, word in (
            ([fg, None], 2, 64, False, "caller"),                  # a roll-out has no caller
            ([fg], 2, 64, False, "one driver per seat"),
            ([fg] * 9, 9, 64, False, "group"),
            ([], 0, 64, True, "group"),
            ([fg, "fg"], 2, 64, True, "unknown driver"),
            ([fg, 1], 2, 64, False, "unknown driver"),
            ([fg, fg2], 2, 64, False, "at most one PyFollowGap"),
            ([pol, fg, pol2], 3, 64, True, "at most one Policy"),
            ([fg, pol], 2, 44, True, "do not hold the policy's window [5, 45)")):
        with pytest.raises(ValueError, match=re.escape(word)):
            seats.seat_args(drivers, group, rays, caller_ok)
    sp, g, p = seats.seat_env_args([None, fg, pol], [math.nan, 1.5, 2.5], 3, 64)
    assert list(sp.driver)[:3] == [0, 1, 2] and list(sp.speed)[:3] == [0.0, 1.5, 2.5] and g is fg and p is pol
    assert list(seats.seat_env_args([fg, fg], 3.0, 2, 64)[0].speed)[:2] == [3.0, 3.0]
    for speed in ([1.0, math.inf], [1.0, math.nan], [1.0], [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            seats.seat_env_args([None, fg], speed, 2, 64)


def test_wrappers_refuse_before_the_library(no_calls):
    fg, pol = _drivers()
    cars = RC.CarBatch.__new__(RC.CarBatch)
    st, edge = np.zeros((2, 3, 11)), np.zeros(64)
    ok = dict(states=st, n_ticks=4, speed=2.0, fov=4.7, num_rays=64, edge=edge, crash_thresh=0.001)
    for kw in (dict(drivers=[fg, pol]), dict(drivers=[fg, None, pol]), dict(drivers=[fg, pol, object()]),
               dict(drivers=[fg, pol, fg], steer_clip=0.0), dict(drivers=[fg, pol, fg], steer_clip=-1.0),
               dict(drivers=[fg, pol, fg], num_rays=44, edge=np.zeros(44)), dict(drivers=[fg, pol, fg], states=st[0]),
               dict(drivers=[fg, pol, fg], states=st.astype(np.float32)), dict(drivers=[fg, pol, fg], edge=np.zeros(63)),
               dict(drivers=[fg, pol, fg], speed=np.zeros(5)), dict(drivers=[fg, pol, fg], steer0=np.zeros((2, 3)))):
        with pytest.raises(ValueError):
            cars.race_seats(None, **dict(ok, **kw))
    env = RaceEnv.__new__(RaceEnv)
    env._group, env._n, env.seats = 3, 6, None
    env.params = _lib.EnvParams()
    env.params.num_rays = 44
    for args in (([fg, pol],), ([fg, pol, fg],), ([None, None, 3],), ([fg, fg, fg], math.inf), ([fg, fg, fg], [1.0, 2.0])):
        with pytest.raises(ValueError):
            env.attach_seats(*args)
    with pytest.raises(ValueError, match="no seats attached"):
        env.seat_steers()
    with pytest.raises(ValueError, match="no seats attached"):
        env.seat_steers(on_device=True)
