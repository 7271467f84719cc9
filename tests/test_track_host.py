"""Track progress without a GPU: known answers of the statement (tests/track_statement.py) on a unit square, a line,
a hairpin and the reference's waypoint file (tests/golden/wp_u.csv), every Python-side argument check, and the layout
of rl_track_params."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import track_statement as TS
from conftest import GOLD
from pyracecarsimulator_amd import DriveEnv, RaceEnv, Track, _lib
from pyracecarsimulator_amd.track import ROW_NAMES, track_args, track_env_args

SQUARE = [(0, 0), (1, 0), (1, 1), (0, 1)]                       # closed: segments 0 east, 1 north, 2 west, 3 south
LINE = [(float(i), 0.0) for i in range(6)]                      # open: 5 segments along x
# out along y = 0, back along y = 0.2, 0.2 m apart: 12 points, segments 0-4 out, 5 the turn, 6-10 back, 11 closing
HAIRPIN = [(float(i), 0.0) for i in range(6)] + [(float(i), 0.2) for i in range(5, -1, -1)]


def wp_u():
    return Track.read_csv(os.path.join(GOLD, "wp_u.csv"))


def test_table_of_the_square_and_of_the_waypoint_file():
    T = TS.build(SQUARE, True)
    assert (T["W"], T["S"], T["L"]) == (4, 4, 4.0) and T["cum"].tolist() == [0, 1, 2, 3, 4]
    assert T["dx"].tolist() == [1, 0, -1, 0] and T["dy"].tolist() == [0, 1, 0, -1]
    T = TS.build(LINE, False)
    assert (T["W"], T["S"], T["L"]) == (6, 5, 5.0)
    xy = wp_u()
    assert xy.shape == (36, 2) and xy[0].tolist() == [0.500746, 0.128211]
    T = TS.build(xy, True)
    assert T["S"] == 36 and (np.diff(T["cum"]) > 0).all() and T["cum"][-1] == T["L"]
    assert abs(T["len"][0] - math.hypot(1.500582 - 0.500746, 0.110646 - 0.128211)) < 1e-15
    assert 30.0 < T["L"] < 60.0
    for bad, closed in ((SQUARE[:2], True), (SQUARE[:1], False), (SQUARE + [(0, 1)], True), ([(0, 0), (np.nan, 1)], False),
                        ([(0, 0), (0, 0), (1, 1)], True)):
        with pytest.raises(ValueError):
            TS.build(bad, closed)


def test_corner_bisector_takes_the_lower_index():
    """(1.5, -0.5) lies on the bisector outside corner (1, 0): t = 1 on segment 0 and t = 0 on segment 1, d2 = 0.5 on
    both.  At corner (0, 0) the tie is between segments 3 and 0, and a window that lists 3 first still gives 0."""
    T = TS.build(SQUARE, True)
    a, b = TS.project(T, 0, 1.5, -0.5), TS.project(T, 1, 1.5, -0.5)
    assert (a[0], a[1]) == (0.5, 1.0) and (b[0], b[1]) == (0.5, 0.0)
    assert TS.nearest(T, 1.5, -0.5) == 0
    s, lat, head, _, _ = TS.quantities(T, 0, 1.5, -0.5, 0.0)
    assert (s, lat, head) == (1.0, -0.5, 0.0)                   # right of the direction of travel: negative
    assert TS.candidates(T, 0, 1, False) == [3, 0, 1]
    assert TS.project(T, 3, -0.5, -0.5)[:2] == (0.5, 1.0) and TS.project(T, 0, -0.5, -0.5)[:2] == (0.5, 0.0)
    assert TS.nearest(T, -0.5, -0.5, 0, 1, False) == 0
    # on the waypoint file: a car standing on waypoint 5 is at t = 1 of segment 4 and t = 0 of segment 5
    U = TS.build(wp_u(), True)
    assert TS.nearest(U, U["x"][5], U["y"][5]) == 4
    assert TS.quantities(U, 4, U["x"][5], U["y"][5], 0.0)[0] == U["cum"][5]
    # heading error: along segment 1 (north) a car heading west is a quarter turn to the left
    assert abs(TS.quantities(T, 1, 1.0, 0.5, math.pi)[2] - math.pi / 2) < 1e-15


def test_start_line_crossings_forward_and_backward():
    T = TS.build(SQUARE, True)
    env = TS.TrackEnv(T, 1)
    st = np.zeros((1, 11))
    st[0, :2] = (0.0, 0.25)                                     # on segment 3, s = 3.75
    rows, ints = env.call(st, [TS.FRESH])
    assert rows[0, [0, 1, 2, 6, 7]].tolist() == [0, 3.75, 0, 0, 0] and ints[0].tolist()[::2] == [3, 0]
    assert rows[0, 3] == np.float32(math.pi / 2)                # heading east on the segment that runs south
    st[0, :2] = (0.25, 0.0)                                     # across the line: s = 0.25, D = -3.5 + 4
    rows, ints = env.call(st, [TS.STEPPED])
    assert (rows[0, 0], rows[0, 1], rows[0, 6]) == (0.5, 0.25, 0.5) and ints[0, 0] == 0 and ints[0, 2] == 1
    rows, ints = env.call(st, [TS.FROZEN])                      # frozen: D = 0, nothing else changes
    assert (rows[0, 0], rows[0, 1], rows[0, 6]) == (0.0, 0.25, 0.5) and ints[0, 2] == 1
    st[0, :2] = (0.0, 0.25)                                     # back across it: D = 3.5 - 4
    rows, ints = env.call(st, [TS.STEPPED])
    assert (rows[0, 0], rows[0, 6]) == (-0.5, 0.0) and ints[0, 2] == 0
    rows, ints = env.call(st, [TS.INVALID])
    assert rows[0, 0] == 0.0 and ints[0, 2] == 0
    st[0, :2] = (0.5, 1.0)                                      # half a lap in one call: D = 2.25 - 3.75 is not wrapped
    rows, ints = env.call(st, [TS.STEPPED])
    assert (rows[0, 0], rows[0, 1]) == (-1.25, 2.5) and ints[0, 2] == 0
    assert TS.wrap(T, np.float64(2.0)) == (2.0, 0) and TS.wrap(T, np.float64(-2.0)) == (-2.0, 0)     # half itself stays


def test_open_track_clamps_the_window_and_never_wraps():
    T = TS.build(LINE, False)
    assert TS.candidates(T, 0, 1, False) == [0, 1] and TS.candidates(T, 4, 1, False) == [3, 4]
    assert TS.candidates(T, 2, 1, False) == [1, 2, 3] and TS.candidates(T, 2, 2, False) == [0, 1, 2, 3, 4]
    assert TS.candidates(T, 2, 1, True) == [0, 1, 2, 3, 4] and TS.candidates(T, 2, 0, False) == [0, 1, 2, 3, 4]
    assert TS.nearest(T, 7.0, 0.0, 4, 1, False) == 4 and TS.quantities(T, 4, 7.0, 0.0, 0.0)[0] == 5.0
    assert TS.nearest(T, 3.5, 0.0, 0, 1, False) == 1            # the window holds it back
    assert TS.wrap(T, np.float64(-4.5)) == (-4.5, 0)


def test_window_wraps_from_segment_34_to_2_of_36():
    U = TS.build(wp_u(), True)
    assert TS.candidates(U, 0, 2, False) == [34, 35, 0, 1, 2]
    assert TS.candidates(U, 35, 2, False) == [33, 34, 35, 0, 1]
    mx, my = 0.5 * (U["x"][35] + U["x"][0]), 0.5 * (U["y"][35] + U["y"][0])
    assert TS.nearest(U, mx, my, 1, 2, False) == 35
    assert TS.nearest(U, mx, my, 3, 2, False) != 35             # out of the window's reach
    assert TS.candidates(U, 0, 18, False) == list(range(36))    # 2 window + 1 >= S: all of them


def test_hairpin_window_keeps_the_leg():
    """The car was on segment 1 and now stands at (2.5, 0.15): 0.05 m from the returning leg (segment 8), 0.15 m from
    its own (segment 2).  window = 0 jumps across, window = 3 does not."""
    T = TS.build(HAIRPIN, True)
    assert T["S"] == 12 and (T["x"][8], T["y"][8], T["x"][9]) == (3.0, 0.2, 2.0)
    assert TS.nearest(T, 2.5, 0.15, 1, 0, False) == 8
    assert TS.candidates(T, 1, 3, False) == [10, 11, 0, 1, 2, 3, 4]
    assert TS.nearest(T, 2.5, 0.15, 1, 3, False) == 2
    assert TS.nearest(T, 2.5, 0.15, 1, 3, True) == 8            # a fresh env searches everything


def test_goal_rule():
    T = TS.build(SQUARE, True)
    assert TS.goal(T, 0, 10.0, 10.0, 1.0, 0) == -1              # none inside 2 l
    assert TS.goal_point(T, -1, 10.0, 10.0, 1.0, 0.0) == (0.0, 0.0, 0.0)
    assert TS.goal(T, 0, 0.5, 0.5, 1.5, 0) == 0                 # four equally good: the first
    assert TS.goal(T, 0, 0.5, 0.5, 1.5, 2) == 1                 # candidates 1, 2
    assert TS.goal(T, 3, 0.5, 0.5, 1.5, 2) == 0                 # candidates 0, 1: the span wraps
    assert TS.goal(T, 3, 0.5, 0.5, 1.5, 9) == 0                 # a second visit cannot win
    Ln = TS.build(LINE, False)
    assert TS.goal(Ln, 0, 0.2, 0.0, 1.5, 0) == 2                # |1.5 - 1.8| = 0.3 is the best of all
    assert TS.goal(Ln, 0, 0.2, 0.0, 1.5, 1) == 1                # the one waypoint ahead
    assert TS.goal(Ln, 4, 4.9, 0.0, 1.5, 10) == 5               # an open track stops at W - 1
    assert TS.goal(Ln, 0, 0.25, 0.0, 0.75, 0) == 1              # g = 0 at waypoint 1 beats g = 0.5 at waypoint 0
    assert TS.goal(Ln, 0, 0.5, 0.0, 0.25, 0) == 0               # g = 0.25 at waypoints 0 and 1: the first
    hx, hy = np.cos(np.float64(math.pi / 2)), np.sin(np.float64(math.pi / 2))
    gx, gy, r = TS.goal_point(Ln, 1, 0.0, 0.0, hx, hy)          # heading north, the goal due east: on the right
    assert abs(gx) < 1e-15 and gy == -1.0 and r == 1.0


def test_goal_without_the_loop_is_the_goal_as_written():
    rng = np.random.default_rng(3)
    U, Ln = TS.build(wp_u(), True), TS.build(LINE, False)
    for T in (U, Ln, TS.build(SQUARE, True)):
        for _ in range(60):
            cx, cy = rng.uniform(-4, 9, 2)
            i, la, span = int(rng.integers(T["S"])), float(rng.choice([0.3, 1.5, 4.0])), int(rng.choice([0, 1, 10, 50]))
            assert TS.goal(T, i, cx, cy, la, span) == TS.goal_loop(T, i, cx, cy, la, span)
    assert TS.goal_loop(TS.build(SQUARE, True), 0, 0.5, 0.5, 1.5, 0) == 0


def test_race_offset_and_rank_with_a_tie():
    T = TS.build(SQUARE, True)
    assert TS.ranks([1.0, 2.0, 1.0, 2.0]).tolist() == [2, 0, 3, 1]
    assert TS.race_offset(T, np.float64(3.75), np.float64(0.25)) == -0.5      # just behind the line, not 3.5 ahead
    assert TS.race_offset(T, np.float64(0.25), np.float64(3.75)) == 0.5
    env = TS.TrackEnv(T, 3, group=3)
    st = np.zeros((3, 11))
    st[:, :2] = ((0.25, 0.0), (0.0, 0.25), (0.25, 0.0))
    rows, ints = env.call(st, [TS.FRESH] * 3)
    assert rows[:, 7].tolist() == [0.0, -0.5, 0.0] and ints[:, 3].tolist() == [0, 2, 1]
    st[1, :2] = (0.5, 0.0)                                      # car 1 passes both; car 2 is a wreck and stays ranked
    rows, ints = env.call(st, [TS.STEPPED, TS.STEPPED, TS.FROZEN])
    assert rows[:, 0].tolist() == [0.0, 0.75, 0.0] and rows[:, 7].tolist() == [0.0, 0.25, 0.0]
    assert ints[:, 3].tolist() == [1, 0, 2] and ints[:, 2].tolist() == [0, 1, 0]
    solo = TS.TrackEnv(T, 2)
    rows, ints = solo.call(st[:2], [TS.FRESH] * 2)
    assert rows[:, 7].tolist() == [0.0, 0.0] and ints[:, 3].tolist() == [0, 0]     # a DriveEnv: offset 0, rank 0


def test_phases():
    done = np.array([0, 1, 0, 2])
    a = np.ones((4, 2), np.float32)
    a[2, 1] = np.nan
    assert TS.phases_drive(done, a, True).tolist() == [TS.STEPPED, TS.FRESH, TS.INVALID, TS.FRESH]
    assert TS.phases_drive(done, a, False).tolist() == [TS.STEPPED, TS.FROZEN, TS.INVALID, TS.FROZEN]
    assert TS.phases_race([0, 1], done, a, True, 2).tolist() == [TS.STEPPED, TS.FROZEN, TS.FRESH, TS.FRESH]
    assert TS.phases_race([0, 1], done, a, False, 2).tolist() == [TS.STEPPED, TS.FROZEN, TS.FROZEN, TS.FROZEN]


def test_python_argument_checks():
    assert track_args(SQUARE).dtype == np.float64 and track_args(SQUARE).shape == (4, 2)
    assert track_args(SQUARE[:2], closed=False).shape == (2, 2)
    for xy, closed in ((SQUARE[:2], True), (SQUARE[:1], False), ([0.0, 1.0, 2.0], True), (np.zeros((4, 3)), True),
                       ([(0, 0), (1, 0), (np.inf, 1)], True), ([(0, 0), (1, 0), (1, 0), (0, 1)], True),
                       ([(0, 0), (1, 1), (0, 0)], True), (np.zeros((65537, 2)), False)):
        with pytest.raises(ValueError):
            track_args(xy, closed)
    assert track_args([(0, 0), (1, 1), (0, 0)], closed=False).shape == (3, 2)     # open: first = last is no segment
    p = track_env_args(4, 2.0, 10, True)
    assert (p.window, p.goal_span, p.reward_mode, p.lookahead) == (4, 10, 1, 2.0)
    p = track_env_args()
    assert (p.window, p.goal_span, p.reward_mode, p.lookahead) == (0, 0, 0, 1.5)
    for kw in (dict(track_window=-1), dict(track_window=65537), dict(track_window=1.5), dict(goal_span=-1),
               dict(goal_span=65537), dict(goal_span=True), dict(lookahead=0), dict(lookahead=-1.0),
               dict(lookahead=np.inf), dict(lookahead=np.nan), dict(progress_reward=2), dict(progress_reward="yes")):
        with pytest.raises(ValueError):
            track_env_args(**kw)
    # the envs check the track keywords before any library call
    starts, edge = np.zeros((1, 11)), np.ones(100)
    for kw in (dict(track="wp_u.csv"), dict(lookahead=0.0), dict(track_window=-2), dict(goal_span=-2)):
        with pytest.raises(ValueError):
            DriveEnv(None, starts, 4, 100, 4.7, edge, 0.001, **kw)
        with pytest.raises(ValueError):
            RaceEnv(None, starts[None], 4, 100, 4.7, edge, 0.001, **kw)
    assert ROW_NAMES == ("delta", "s", "lateral", "heading_err", "gx", "gy", "progress", "race_dist")


def test_track_params_layout():
    """typedef struct rl_track_params { int window, goal_span, reward_mode; double lookahead; }."""
    P = _lib.TrackParams
    assert C.sizeof(P) == 24
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("window", 0), ("goal_span", 4), ("reward_mode", 8),
                                                                  ("lookahead", 16)]
    assert set(n for n in _lib.SYMBOLS if "track" in n) == {"rl_track_create", "rl_track_destroy", "rl_track_read",
                                                            "rl_env_attach_track", "rl_env_read_track",
                                                            "rl_env_read_track_device"}
