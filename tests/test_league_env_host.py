"""League line-ups in the race environment without a GPU: the statement (tests/league_env_statement.py) on the fake
one-dimensional world of test_race_env_host.py — adoption only at a spawn, every clause of "beats", the results'
columns — what include/scanlib_league_env.h says beyond its prototypes (tests/test_py_calls_host.py pins those to
``_lib.LEAGUE_ENV_SYMBOLS``) and every Python-side refusal."""
import ctypes as C
import inspect
import math
import re

import numpy as np
import pytest

import env_statement as E
import league_env_statement as LE
import scanlib_header as H
from test_population_host import _pop, no_calls  # noqa: F401  (no_calls: a fixture)
from test_race_env_host import B, World1D, _acts, _lineup
from pyracecarsimulator_amd import RaceEnv, _lib, league

HEADER = H.read("scanlib_league_env.h")
N_MEMBERS = 3


def _answer(entry, row):
    assert row.shape == (B,) and row.dtype == np.float32
    if entry < 0:
        return np.float32(row[0]) / np.float32(100.0)              # "FollowGap"
    return np.float32(row[0]) / np.float32(10.0 * (entry + 1))     # member m


def _env(lineups, n_races, entries, seat_speed, world=None, **kw):
    starts = np.stack(lineups)
    w = world or World1D(starts.shape[1])
    env = LE.LeagueEnvStatement(starts, n_races, B, w.step_cars, w.scan, w.is_crashed, _answer, entries, seat_speed,
                                N_MEMBERS, scan_dist_to_base=0.0, **kw)
    return env, w


def _row(**kw):
    return [kw.get(k, 0) for k in LE.COLUMNS]


# ---------------------------------------------------------------- adoption
def test_entries_are_adopted_only_when_a_race_spawns():
    """Race 0 (a car 0.5 m short of the wall's margin) ends at step 1 and re-spawns at step 2 with the table set in
    between, while race 1 runs on with its old line-up until its own re-spawn after max_ticks."""
    pool = [_lineup(0.0, 9.0), _lineup(0.0, 4.0)]
    first, second, third = [[0, -1], [1, -2]], [[2, 2], [-1, 0]], [[-2, 1], [2, -2]]
    env, w = _env(pool, 2, first, (5.0, 5.0), min_running=2, max_ticks=4, auto_reset=True, crash_reward=-1.0)
    env.reset(seed=6, start_index=[0, 1])
    assert env.live.reshape(2, 2).tolist() == first and env.pending.reshape(2, 2).tolist() == first
    env.set_entries(second)
    assert env.live.reshape(2, 2).tolist() == first                 # nothing spawned: nothing adopted
    a = _acts(5.0, 5.0, 5.0, 5.0)
    obs, rew, done = env.step(a)                                    # race 0: car 1 reaches 9.5
    assert done.tolist() == [2, 1, 0, 0] and env.race_over.tolist() == [1, 0]
    assert env.live.reshape(2, 2).tolist() == first                 # the race that ended still shows what it ran with
    # ... and was counted with it: member 0 survived, FollowGap crashed
    assert env.results[0].tolist() == _row(entered=1, ticks=1, faced=1, beaten=1)
    assert env.results[N_MEMBERS].tolist() == _row(entered=1, out=1, ticks=1, faced=1)
    assert not env.results[[1, 2, N_MEMBERS + 1]].any()
    obs, rew, done = env.step(a)                                    # race 0 re-spawns; race 1 runs on
    assert env.race_episode.tolist() == [1, 0] and env.race_tick.tolist() == [0, 2]
    assert env.live.reshape(2, 2).tolist() == [second[0], first[1]]
    # race 1's scripted car (member 1, seat 0) still takes its driver's answer: the steer of the call before
    want = _answer(1, env.ranges[2])
    assert env.steers[2] == want and want != 0
    env.set_entries(third)
    env.step(a)
    assert env.states[2, 4] == np.float64(want) and env.steers[2] == _answer(1, env.ranges[2])
    assert env.live.reshape(2, 2)[1].tolist() == first[1]
    while env.race_episode[1] == 0:
        env.step(a)
    assert env.live.reshape(2, 2)[1].tolist() == third[1]           # (race 1 skipped the second table altogether)
    assert env.k == 5                                               # max_ticks = 4: over at step 4, spawned at step 5
    assert env.pending.reshape(2, 2).tolist() == third


def test_a_scripted_car_takes_its_own_drivers_answer_and_the_seat_speed():
    """Two races, the same seat with different drivers: the caller's rows of scripted cars are never read."""
    pool = [_lineup(0.0, 3.0), _lineup(1.0, 5.0)]
    env, w = _env(pool, 2, [[0, -1], [2, -2]], (2.0, 4.0), auto_reset=False, steer_clip=0.05)
    env.reset(seed=0, start_index=[0, 1])
    assert np.isnan(env.league_steers()[3]) and not np.isnan(env.league_steers()[:3]).any()
    s0 = env.league_steers()
    assert s0[0] == np.float32(3.0) / np.float32(10.0) and s0[1] == np.float32(3.0) / np.float32(100.0)
    assert s0[2] == np.float32(4.0) / np.float32(30.0)
    a = _acts(np.nan, np.nan, np.nan, 7.0)
    obs, rew, done = env.step(a)
    assert done.tolist() == [0, 0, 0, 0]
    assert env.states[:, 0].tolist() == pytest.approx([0.2, 3.4, 1.2, 5.7])    # seat speeds 2 and 4, the caller's 7
    assert env.states[0, 4] == 0.05 and env.states[2, 4] == 0.05    # the members' answers, over the clip
    assert env.states[1, 4] == np.float64(s0[1])
    assert env.fed[:3, 0].tolist() == [2.0, 4.0, 2.0]


# ---------------------------------------------------------------- beats
def test_every_clause_of_beats():
    up, crash, bad = LE.TRUNCATED, LE.CRASHED, LE.BAD_ACTION
    assert LE.beats(3, crash, 0.0, 2, up, 9.0) and not LE.beats(2, up, 9.0, 3, crash, 0.0)          # the ticks decide
    for out in (crash, bad):
        assert LE.beats(3, up, 0.0, 3, out, 9.0) and not LE.beats(3, out, 9.0, 3, up, 0.0)          # then the class
    assert LE.beats(3, up, 2.0, 3, up, 1.0) and not LE.beats(3, up, 1.0, 3, up, 2.0)                # then the gain
    assert LE.beats(3, crash, 2.0, 3, bad, 1.0) and not LE.beats(3, bad, 1.0, 3, crash, 2.0)        # (1 and 3: one class)
    assert not LE.beats(3, up, 1.0, 3, up, 1.0)                                                      # a tie
    assert not LE.beats(3, up, math.nan, 3, up, 1.0) and not LE.beats(3, up, 1.0, 3, up, math.nan)  # NaN
    assert LE.beats(4, up, math.nan, 3, up, 1.0)                                                     # (never asked)


def test_results_of_a_race_with_every_kind_of_driver():
    """test_attrition's race with min_running = 2: car 2 (FollowGap) crashes at step 1, car 1 (member 1) at step 3 with
    the larger gain, car 0 (the caller's) survives with as many ticks: done 2 beats done 1 whatever the gains."""
    env, w = _env([_lineup(0.0, 3.0, 8.9)], 1, [[-2, 1, -1]], (0.0, 20.0, 6.0), min_running=2, crash_reward=-1.0,
                  auto_reset=False)
    env.reset(seed=0, start_index=[0])
    a = _acts(10.0, np.nan, np.nan)
    for k in range(3):
        assert not env.results.any()
        obs, rew, done = env.step(a)
    assert done.tolist() == [2, 1, 1] and env.tick.tolist() == [3, 3, 1] and env.race_over.tolist() == [1]
    assert env.states[1, 8] - 0.0 > env.states[0, 8]
    res = env.read_results()
    assert res[N_MEMBERS + 1].tolist() == _row(entered=1, ticks=3, faced=2, beaten=2)
    assert res[1].tolist() == _row(entered=1, out=1, ticks=3, faced=2, beaten=1, callers_faced=1, callers_won=1)
    assert res[N_MEMBERS].tolist() == _row(entered=1, out=1, ticks=1, faced=2, callers_faced=1, callers_won=1)
    assert not res[0].any() and not res[2].any()                    # members that entered nothing
    # the finished race stands: counted once
    for k in range(3):
        env.step(a)
    assert env.read_results(clear=True).tolist() == res.tolist()
    assert not env.read_results().any()


def test_an_invalid_action_counts_as_out_and_a_tie_beats_nobody():
    # the caller's car 1 sends NaN at step 1: done 3 with 0 ticks; member 0 in seat 0 survives the attrition
    env, w = _env([_lineup(0.0, 2.0)], 1, [[0, -2]], (5.0, 5.0), min_running=2, auto_reset=False)
    env.reset(seed=0, start_index=[0])
    obs, rew, done = env.step(_acts(np.nan, np.nan))
    assert done.tolist() == [2, 3] and env.tick.tolist() == [1, 0]
    assert env.results[0].tolist() == _row(entered=1, ticks=1, faced=1, beaten=1, callers_faced=1, callers_beaten=1)
    assert env.results[N_MEMBERS + 1].tolist() == _row(entered=1, out=1, faced=1)
    # two members at the same speed until max_ticks: the same ticks, class and gain
    env, w = _env([_lineup(0.0, 4.0)], 1, [[0, 2]], (5.0, 5.0), max_ticks=2, auto_reset=False)
    env.reset(seed=0, start_index=[0])
    env.step(_acts(np.nan, np.nan))
    assert env.step(_acts(np.nan, np.nan))[2].tolist() == [2, 2]
    assert env.results[0].tolist() == env.results[2].tolist() == _row(entered=1, ticks=2, faced=1)
    # two cars of ONE member: its row takes both
    env, w = _env([_lineup(0.0, 4.0)], 1, [[1, 1]], (5.0, 2.0), max_ticks=2, auto_reset=False)
    env.reset(seed=0, start_index=[0])
    env.step(_acts(np.nan, np.nan))
    env.step(_acts(np.nan, np.nan))
    assert env.results[1].tolist() == _row(entered=2, ticks=4, faced=2, beaten=1)


class NanWorld(World1D):
    """World1D whose cars at speed 7 lose their travelled distance to NaN."""

    def step_cars(self, states, speed, steer):
        out = super().step_cars(states, speed, steer)
        out[speed == 7.0, 8] = np.nan
        return out


def test_a_nan_gain_beats_nobody_and_is_beaten_by_nobody():
    env, w = _env([_lineup(0.0, 3.0, 6.0)], 1, [[0, 1, 2]], (7.0, 3.0, 2.0), world=NanWorld(3), max_ticks=1,
                  auto_reset=False)
    env.reset(seed=0, start_index=[0])
    assert env.step(_acts(np.nan, np.nan, np.nan))[2].tolist() == [2, 2, 2]
    assert np.isnan(env.states[0, 8])
    assert env.results[:3, 4].tolist() == [0, 1, 0] and env.results[:3, 3].tolist() == [2, 2, 2]


def test_a_reset_mid_race_counts_nothing_and_keeps_the_tally():
    env, w = _env([_lineup(0.0, 9.0), _lineup(0.0, 4.0)], 2, [[0, 1], [2, -1]], (5.0, 5.0), min_running=2,
                  auto_reset=True)
    env.reset(seed=0, start_index=[0, 1])
    env.step(_acts(*[np.nan] * 4))                                  # race 0 ends, race 1 runs
    tally = env.results.copy()
    assert tally[:2, 0].tolist() == [1, 1] and not tally[2:].any()
    env.reset(seed=1, start_index=[1, 1])                           # race 1 is cut off: its cars are never counted
    assert env.results.tolist() == tally.tolist()                   # ... and a reset clears nothing
    assert env.live.reshape(2, 2).tolist() == [[0, 1], [2, -1]]


def test_entries_the_device_form_cannot_refuse_behave_as_the_callers():
    env, w = _env([_lineup(0.0, 4.0, 8.0)], 1, [[N_MEMBERS, -3, 0]], (5.0, 5.0, 5.0), max_ticks=1, auto_reset=False)
    env.reset(seed=0, start_index=[0])
    assert np.isnan(env.league_steers()[:2]).all() and not np.isnan(env.league_steers()[2])
    env.step(_acts(1.0, 2.0, np.nan))
    assert env.states[:2, 0].tolist() == pytest.approx([0.1, 4.2])  # their rows of `actions` are read
    assert env.results[N_MEMBERS + 1].tolist() == _row(entered=2, ticks=2, faced=4, beaten=1, callers_faced=2,
                                                       callers_beaten=1, callers_won=1)
    assert env.results[0, 5:].tolist() == [2, 2, 0]
    # no FollowGap handle: -1 is the caller's; scans below the window: so is every member
    env, w = _env([_lineup(0.0, 4.0)], 1, [[-1, 0]], (5.0, 5.0), followgap=False, auto_reset=False)
    env.reset(seed=0, start_index=[0])
    assert np.isnan(env.league_steers()[0]) and not np.isnan(env.league_steers()[1])
    env, w = _env([_lineup(0.0, 4.0)], 1, [[-1, 0]], (5.0, 5.0), window=False, auto_reset=False)
    env.reset(seed=0, start_index=[0])
    assert not np.isnan(env.league_steers()[0]) and np.isnan(env.league_steers()[1])


def test_the_spawn_draw_is_the_race_envs():
    pool = [_lineup(0.0, 9.0), _lineup(1.0, 5.0), _lineup(2.0, 6.0)]
    env, w = _env(pool, 2, [[0, 1], [2, 0]], (5.0, 5.0), max_ticks=1, auto_reset=True)
    env.reset(seed=4)
    env.step(_acts(*[np.nan] * 4))
    env.step(_acts(*[np.nan] * 4))
    assert env.race_start_index.tolist() == [E.spawn_index(4, r, 1, 3) for r in range(2)]


# ---------------------------------------------------------------- the header
def test_header_is_pinned_to_league_env_symbols():
    protos = HEADER.prototypes()
    assert protos["rl_env_attach_league"][2] == ["e", "g_or_null", "pop", "entry_N_or_null", "speed_P"]
    assert protos["rl_env_read_league_results"][2] == ["e", "results", "clear"]
    assert protos["rl_env_read_league_results"][1][1] is C.POINTER(C.c_int64)
    for name in ("rl_env_set_league_entries_device", "rl_env_read_league_steers_device"):
        assert protos[name][2][-1] == "hip_stream"
        assert protos[name][1] == list(_lib.SEAT_SYMBOLS["rl_env_read_seats_device"][1])
    assert not HEADER.structs() and not HEADER.handles()
    raw = open(HEADER.path).read()
    assert '#include "scanlib_league.h"' in raw and raw.count("#include") == 1
    assert "Out of scope" in raw and "Errors (RL_ERR_INVALID" in raw
    for phrase in ("Ties and NaN beat nobody", "never re-seated", "behaves as -2, by construction", "reset does not clear them",
                   "64-bit vector atomics", "FollowGap's, then the population's", "graph capture",
                   "A race cut off by a reset adds nothing"):
        assert phrase in raw, phrase
    assert (league.CALLER, league.FOLLOWGAP) == (LE.CALLER, LE.FOLLOWGAP) == (-2, -1)
    assert league.RESULT_COLUMNS == LE.COLUMNS and len(LE.COLUMNS) == 8
    import pyracecarsimulator_amd as P
    for name in ("attach_league", "set_entries", "entries", "league_steers", "league_results"):
        assert callable(getattr(P.RaceEnv, name)), name
    assert "league" in inspect.signature(P.RaceEnv.__init__).parameters
    assert "league" in inspect.getsource(P.RacecarSimulator.raceEnv)


# ---------------------------------------------------------------- the wrappers' refusals
def test_league_env_args(no_calls):  # noqa: F811
    pop, fg = _pop(), object()                                      # 5 members on the window [5, 45)
    spd = league.seat_speeds(2.0, 3)
    assert spd.tolist() == [2.0, 2.0, 2.0] and spd.dtype == np.float32
    ok = np.array([[-2, -1, 4], [0, 0, -2]])
    out = league.league_env_args(ok, 2, 3, pop, fg, 64, spd)
    assert out.tolist() == [-2, -1, 4, 0, 0, -2] and out.dtype == np.int32 and out.flags.c_contiguous
    for kw, word in ((dict(entries=np.array([[-2, -1, 5], [0, 0, -2]])), "member in [0, 5)"),
                     (dict(entries=np.array([[-3, -1, 4], [0, 0, -2]])), "-2 (the caller)"),
                     (dict(entries=ok.reshape(-1)), "(R, P) = (2, 3)"), (dict(entries=ok[:1]), "(R, P)"),
                     (dict(entries=ok.astype(np.float64)), "integers"), (dict(followgap=None), "no followgap"),
                     (dict(num_rays=44), "do not hold the policy's window [5, 45)"),
                     (dict(speeds=np.float32([2.0, math.nan, 2.0])), "speed of seat 1"),
                     (dict(speeds=np.float32([math.inf, 2.0, 2.0])), "speed of seat 0")):
        args = dict(entries=ok, n_races=2, group=3, pop=pop, followgap=fg, num_rays=64, speeds=spd)
        args.update(kw)
        with pytest.raises(ValueError, match=re.escape(word)):
            league.league_env_args(**args)
    # what is no refusal: a non-finite speed of a seat with caller's cars only; no FollowGap without a -1; a narrow scan
    # without a member
    only = np.array([[-2, 1, -2], [-2, 0, -2]])
    assert league.league_env_args(only, 2, 3, pop, None, 64, np.float32([math.nan, 2.0, math.inf])).shape == (6,)
    assert league.league_env_args(np.array([[-2, -1]]), 1, 2, pop, fg, 20, league.seat_speeds(1.0, 2)).tolist() == [-2, -1]
    for speed in ([1.0, 2.0], [[1.0, 2.0, 3.0]]):
        with pytest.raises(ValueError):
            league.seat_speeds(speed, 3)
    raw = np.arange(7 * 8, dtype=np.int64).reshape(7, 8)
    d = league.results_dict(raw, 5)
    assert d["entered"].tolist() == [0, 8, 16, 24, 32] and d["callers_won"].tolist() == [7, 15, 23, 31, 39]
    assert d["followgap"]["entered"] == 40 and d["caller"]["callers_won"] == 55 and set(d) == set(LE.COLUMNS) | {"followgap", "caller"}


def test_race_env_refuses_before_the_library(no_calls):  # noqa: F811
    pop, fg = _pop(), object()
    env = RaceEnv.__new__(RaceEnv)
    env._group, env._n, env._races, env.seats = 3, 6, 2, None
    env.params = _lib.EnvParams()
    env.params.num_rays = 64
    assert env.league is None
    for call in (lambda: env.set_entries(np.zeros((2, 3), int)), env.entries, env.league_steers, env.league_results,
                 lambda: env.league_steers(on_device=True)):
        with pytest.raises(ValueError, match="no league attached"):
            call()
    ok = np.array([[-2, -1, 4], [0, 0, -2]])
    for args in ((pop, ok[:1], fg), (pop, ok, None), (pop, ok + 1, fg), (pop, ok, fg, math.nan), (pop, ok, fg, [1.0, 2.0])):
        with pytest.raises(ValueError):
            env.attach_league(*args)
    env.seats = ("a seat table",)
    with pytest.raises(ValueError, match="seats are attached"):
        env.attach_league(pop, ok, fg)
    env.seats, env.league = None, (pop, fg, league.seat_speeds(2.0, 3))
    with pytest.raises(ValueError, match="a league is attached"):
        env.attach_seats([None, None, None])
    for bad in (ok[:1], ok + 1, ok - 1, ok.astype(np.float32)):
        with pytest.raises(ValueError):
            env.set_entries(bad)
    env.league = (pop, None, league.seat_speeds(2.0, 3))
    with pytest.raises(ValueError, match="no followgap"):
        env.set_entries(ok)
    env.league = (pop, fg, np.float32([2.0, math.nan, 2.0]))
    with pytest.raises(ValueError, match="speed of seat 1"):
        env.set_entries(ok)
    with pytest.raises(ValueError):
        RaceEnv(None, np.zeros((1, 3, 11)), 2, 64, 4.7, np.zeros(64), 0.001, seats=[None] * 3, league=(pop, ok))
