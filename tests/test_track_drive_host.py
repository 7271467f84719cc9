"""Track progress of the roll-outs without a GPU: what include/scanlib_track_drive.h says beyond its prototypes
(tests/test_py_calls_host.py pins those to ``_lib.TRACK_DRIVE_SYMBOLS``), the statement
(tests/track_drive_statement.py) on hand-made trajectories with the expected numbers written out, and every Python-side
refusal."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import scanlib_header as H
import track_drive_statement as DS
import track_statement as TS
from conftest import ROOT
from test_mcts_track_host import no_calls  # noqa: F401  (a fixture)
from test_track_host import SQUARE
from pyracecarsimulator_amd import RacecarSimulator, Track, _lib
from pyracecarsimulator_amd import racecar as RC

HEADER = H.read("scanlib_track_drive.h")
CORNER = [(0.0, 0.0), (4.0, 0.0), (4.0, 3.0)]                  # 3 points: closed 4 + 3 + 5 = 12 m, open 4 + 3 = 7 m
NAN = float("nan")


def run(T, paths, first, window=0, goal=0.0, group=0):
    """placements() of cars given as [(x, y) of the start, of tick 0, of tick 1, ...]: the trace rows behind a car's crash
    tick are NaN, as the roll-outs leave them."""
    n_ticks = len(paths[0]) - 1
    st0 = np.zeros((len(paths), 11))
    trace = np.full((len(paths), n_ticks, 11), np.nan)
    for r, path in enumerate(paths):
        st0[r, :2] = path[0]
        for t in DS.reached(first[r], n_ticks):
            trace[r, t] = 0.0
            trace[r, t, :2] = path[t + 1]
    return DS.placements(T, st0, trace, np.asarray(first), n_ticks, window, goal, group)


def row(pl, r):
    return [pl[k][r].item() for k in DS.KEYS]


# ---------------------------------------------------------------- the statement, by hand
def test_a_forward_lap_counts_plus_one_and_goal_tick_is_pinned_at_equality():
    T = TS.build(SQUARE, True)
    path = [(0.0, 0.25), (0.25, 0.0), (0.5, 0.0), (0.75, 0.0)]   # s 3.75 | 0.25 (D = -3.5 + 4), 0.5, 0.75
    pl = run(T, [path], [-4], goal=0.75)
    assert row(pl, 0) == [3.75, 0.75, 1.0, 1.0, 0, 1, 1, 0]       # 0.5, 0.75, 1.0: met AT tick 1, by equality, and kept
    pl = run(T, [path[:3]], [-3], goal=0.75)
    assert row(pl, 0) == [3.75, 0.5, 0.75, 0.75, 0, 1, 1, 0]
    assert run(T, [path[:3]], [-3], goal=0.5)["goal_tick"][0] == 0 and run(T, [path[:3]], [-3], goal=0.8)["goal_tick"][0] == -1
    # goal_dist 0 is one track length
    assert run(T, [path[:3]], [-3], goal=0.0)["goal_tick"][0] == -1
    lap = [(0.5, 0.0), (1.0, 0.5), (0.5, 1.0), (0.0, 0.5), (0.5, 0.0)]
    assert row(run(T, [lap], [-5]), 0) == [0.5, 0.5, 4.0, 4.0, 0, 1, 3, 0]


def test_a_reverse_crossing_counts_minus_one():
    T = TS.build(SQUARE, True)
    pl = run(T, [[(0.25, 0.0), (0.0, 0.25), (0.0, 0.5)]], [-3], goal=0.25)
    assert row(pl, 0) == [0.25, 3.5, -0.75, -0.75, 3, -1, -1, 0]  # D = 3.5 - 4, then -0.25


def test_an_open_track_never_wraps():
    T = TS.build(CORNER, False)
    assert T["L"] == 7.0
    pl = run(T, [[(1.0, 0.0), (3.0, 0.0), (4.0, 1.0)], [(0.5, 0.0), (4.0, 3.0), (0.5, 0.0)]], [-3, -3], goal=4.0)
    assert row(pl, 0) == [1.0, 5.0, 4.0, 4.0, 1, 0, 1, 0]
    assert row(pl, 1) == [0.5, 0.5, 0.0, 0.0, 0, 0, 0, 0]         # +6.5 and -6.5, beyond half the length: as they are
    closed = TS.build(CORNER, True)
    assert closed["L"] == 12.0
    pl = run(closed, [[(0.5, 0.0), (4.0, 3.0), (0.5, 0.0)]], [-3])
    assert row(pl, 0) == [0.5, 0.5, 0.0, 0.0, 0, 0, -1, 0]        # s = 7: D = 6.5 - 12 = -5.5 and a lap back, then forth


def test_a_crash_freezes_the_car_behind_the_crash_ticks_own_step():
    T = TS.build(SQUARE, True)
    path = [(0.25, 0.0), (0.5, 0.0), (0.75, 0.0), (1.0, 0.25), (1.0, 0.5)]
    free, hit, at_once = run(T, [path] * 3, [-5, 1, 0], goal=0.5)["progress"].tolist()
    assert (free, hit, at_once) == (1.25, 0.5, 0.25)              # ticks 0 ... 3 | 0, 1 | 0: the crash tick's step counts
    pl = run(T, [path] * 3, [-5, 1, 0], goal=0.5)
    assert pl["goal_tick"].tolist() == [1, 1, -1] and pl["s"].tolist() == [1.5, 0.75, 0.5]
    assert pl["segment"].tolist() == [1, 0, 0]


def test_the_window_follows_the_previous_segment():
    T = TS.build([(float(i), 0.0) for i in range(6)] + [(float(i), 0.2) for i in range(5, -1, -1)], True)   # a hairpin
    # the car hops to the return leg: all segments find it there, a window of 1 keeps the outbound leg
    path = [(1.5, 0.0), (2.5, 0.2)]
    assert run(T, [path], [-2], window=0)["segment"][0] == 8 and run(T, [path], [-2], window=1)["segment"][0] == 2
    assert run(T, [path], [-2], window=1)["progress"][0] == 1.0


def test_a_race_offset_wraps_without_a_lap_and_a_tie_goes_by_k():
    T = TS.build(SQUARE, True)
    # car 1 spawns 0.5 ahead of car 0 and drives 0.25; car 0 drives 0.75: both stand at 0.75
    a = [(0.25, 0.0), (0.5, 0.0), (1.0, 0.0)]
    b = [(0.75, 0.0), (0.875, 0.0), (1.0, 0.0)]
    pl = run(T, [a, b], [-3, -3], group=2)
    assert row(pl, 0) == [0.25, 1.0, 0.75, 0.75, 0, 0, -1, 0]
    assert row(pl, 1) == [0.75, 1.0, 0.25, 0.75, 0, 0, -1, 1]     # equal race_dist: the lower k is ahead
    st = DS.track_standings(pl, [0, 1], 3, 2)
    assert st.tolist() == [[1.0, 0.75, 0.0, 0.0], [1.0, 0.25, 0.0, 0.0], [0.0] * 4]   # ... and neither beats the other
    # car 1 spawns behind the line: offset 3.75 - 0.25 = 3.5 wraps to -0.5, and no lap is counted for it
    c = [(0.0, 0.25), (0.0, 0.125), (0.0, 0.0)]
    pl = run(T, [a, c], [-3, -3], group=2)
    assert row(pl, 1) == [3.75, 0.0, 0.25, -0.25, 0, 1, -1, 1]
    # a wreck keeps its race_dist and is ranked with the rest, ahead of a running car behind it
    pl = run(T, [c, a], [-3, 0], group=2)
    assert pl["race_dist"].tolist() == [0.25, -3.5 + 4.0 + 0.25] and pl["rank"].tolist() == [1, 0]
    assert DS.track_standings(pl, [1, 0], 2, 2)[:, 3].tolist() == [1.0, 0.0]
    # outside races: offset 0, rank 0
    pl = run(T, [a, b], [-3, -3])
    assert pl["race_dist"].tolist() == [0.75, 0.25] and pl["rank"].tolist() == [0, 0]


def test_a_nan_car_reads_nan_and_beats_nobody():
    T = TS.build(SQUARE, True)
    with np.errstate(invalid="ignore"):
        ok = [(0.25, 0.0), (0.5, 0.0), (0.75, 0.0)]
        pl = run(T, [[(NAN, 0.0)] * 3, ok], [-3, -3], goal=0.25, group=2)
        assert pl["segment"][0] == 0 and pl["laps"][0] == 0 and pl["goal_tick"][0] == -1
        assert np.isnan([pl[k][0] for k in ("s0", "s", "progress", "race_dist")]).all()
        assert row(pl, 1)[4:] == [0, 0, 0, 0] and pl["progress"][1] == 0.5 and np.isnan(pl["race_dist"][1])   # car 0's s0
        assert pl["rank"].tolist() == [0, 0]                       # no compare with a NaN holds
        st = DS.track_standings(pl, [0, 1], 2, 2)
        assert st[:, 3].tolist() == [0.0, 0.0] and np.isnan(st[0, 1]) and st[1].tolist() == [1.0, 0.5, 1.0, 0.0]
        # the first candidate of the window, not the lowest index: segment 3, window 1 of 4 -> candidates 2, 3, 0
        pl = run(T, [[(0.0, 0.5), (NAN, 0.5)]], [-2], window=1)
        assert TS.candidates(T, 3, 1, False) == [2, 3, 0] and pl["segment"][0] == 2 and np.isnan(pl["s"][0])
        fit = DS.track_fitness(run(T, [[(NAN, 0.0)] * 3, ok], [-3, -3], goal=0.25), 1, 2)
        assert np.isnan(fit[0, 0]) and fit[0, 1:].tolist() == [1.0, 0.0]


def test_track_fitness_sums_upwards():
    pl = dict(progress=np.array([1e16, 1.0, 1.0, 1.0, 2.0, 3.0, 0.5, 0.25]), goal_tick=np.array([3, -1, 5, 7, -1, -1, -1, 0]))
    fit = DS.track_fitness(pl, 2, 4)
    assert fit[0].tolist() == [1e16, 3.0, 15.0] and fit[0, 0] != ((1.0 + 1.0) + 1.0) + 1e16
    assert fit[1].tolist() == [5.75, 1.0, 0.0]
    # the league sums in ascending CAR index, whatever the order of the members
    pl = dict(progress=np.array([1.0, 1e16, 1.0, 1.0]), goal_tick=np.array([2, -1, -1, 4]), race_dist=np.array([1.0, 1e16, 1.0, 1.0]))
    st = DS.track_standings(pl, [1, 0, 1, 1], 2, 1)
    assert st.tolist() == [[1.0, 1e16, 0.0, 0.0], [3.0, 3.0, 2.0, 0.0]]
    st = DS.track_standings(pl, [1, 0, 1, 1], 2, 4)                # one race of four: car 1 is ahead of the three others
    assert st[:, 3].tolist() == [3.0, 0.0]


# ---------------------------------------------------------------- the header
def test_header_is_pinned_to_track_drive_symbols():
    protos = HEADER.prototypes()
    assert protos["rl_car_attach_track"][2] == ["c", "t", "p"]
    assert protos["rl_car_read_track"][2] == ["c", "n_cars", "rows_n4", "ints_n4"]
    assert protos["rl_car_read_track_scores"][2] == ["c", "n_rows", "n_cols", "scores"]
    structs = HEADER.structs()
    assert list(structs) == ["rl_drive_track_params"]
    assert structs["rl_drive_track_params"] == [("window", C.c_int), ("goal_dist", C.c_double)] == _lib.DriveTrackParams._fields_
    P = _lib.DriveTrackParams
    assert C.sizeof(P) == 16 and (P.window.offset, P.goal_dist.offset) == (0, 8)
    assert not HEADER.handles()
    raw = open(HEADER.path).read()
    assert '#include "scanlib_league.h"' in raw and "Out of scope" in raw and "Refused (RL_ERR_INVALID" in raw
    for phrase in ("progress >= goal_dist", "goal_dist == 0 means the track length L", "The step of the crash tick counts",
                   "A frozen car", "with no lap counted", "an equal one and k' < k", "ties and NaN beat nobody",
                   "ascending car order from +0.0", "four zeros", "keeps its meaning and bits", "rl_mcts_drive",
                   "graph capture", "multi-device", "off-track", "device-pointer forms"):
        assert phrase in raw, phrase
    # the two headers that named the gap now name what is left of it
    for name in ("scanlib_league.h", "scanlib_league_env.h"):
        text = open(os.path.join(ROOT, "include", name)).read()
        assert "scanlib_track_drive.h" in text, name


def test_the_kernels_are_built_budgeted_and_shared_and_the_wrappers_take_a_track():
    csrc = os.path.join(ROOT, "pyracecarsimulator_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "drive_track_kernels.h" in make                        # (the public header: test_py_calls_host.py asks make)
    budgets = open(os.path.join(csrc, "check_resources.py")).read()
    for kernel in ("drive_track_kernel<", "drive_track_rank_kernel", "drive_track_fitness_kernel", "drive_track_standings_kernel"):
        assert '("scan::%s", {"scratch": 0})' % kernel in budgets, kernel
    # the search is shared with the env's kernel, not copied
    kern = open(os.path.join(csrc, "drive_track_kernels.h")).read()
    for fn in ("track_window(", "track_nearest(", "track_project(", "track_wrap("):
        assert fn in kern and "inline" not in [ln for ln in kern.splitlines() if fn in ln][0], fn
    for fn in ("attach_track", "detach_track", "track_state", "track_scores"):
        assert hasattr(RC.CarBatch, fn), fn
    for fn in ("driveFollowGapMany", "raceFollowGapMany", "drivePolicyMany", "raceSeatsMany", "drivePopulationMany",
               "raceLeagueMany"):
        sig = inspect.signature(getattr(RacecarSimulator, fn)).parameters
        assert [sig[k].default for k in ("track", "track_window", "goal_dist")] == [None, 0, None], fn


# ---------------------------------------------------------------- the wrappers' refusals
def test_python_argument_checks(no_calls):  # noqa: F811
    cars = RC.CarBatch.__new__(RC.CarBatch)
    trk = Track.__new__(Track)
    for args in (("wp_u.csv",), (None,), (trk, -1), (trk, 65537), (trk, 1.5), (trk, True), (trk, 0, 0.0), (trk, 0, -1.0),
                 (trk, 0, np.inf), (trk, 0, np.nan), (trk, 0, "far")):
        with pytest.raises(ValueError):
            cars.attach_track(*args)
    # nothing attached, or no roll-out since: nothing to read
    for read in (cars.track_state, cars.track_scores):
        with pytest.raises(ValueError):
            read()
    cars._track = trk
    for read in (cars.track_state, cars.track_scores):
        with pytest.raises(ValueError):
            read()
    cars._tracked((3, 2))                                         # a race: a state to read, and no scores
    assert cars._track_shape == (3, 2) and cars._score_shape is None
    with pytest.raises(ValueError):
        cars.track_scores()
    with pytest.raises(AssertionError, match="rl_car_read_track"):
        cars.track_state()                                        # (the fixture: this one does enter the library)
    plain = RC.CarBatch.__new__(RC.CarBatch)
    plain._tracked((4,), (2, 3))                                  # without a track a roll-out records nothing
    assert plain._track_shape is None and plain._score_shape is None
