"""include/scanlib_track_plan.h in plain NumPy float64: the root rule and the three term rules of the track-guided
planner, built on tests/track_statement.py (build, project, nearest, candidates, wrap, goal) and, for the value of a
roll-out, on tests/mcts_statement.py (pairwise_sum, reward_of).  Every f64 operation is one NumPy operation, so each is
separately rounded as on the device.  The trees need no change to the statement of the search: its ``rollout`` phase is
answered with (crash index, terms) where it was answered with velocities."""
import numpy as np

import mcts_statement as MS
import track_statement as TS

VELOCITY, WAYPOINT, PROGRESS = 0, 1, 2
f64 = np.float64


def arc(T, i, cx, cy):
    """s of (cx, cy) on segment i."""
    _, t, _, _ = TS.project(T, i, cx, cy)
    return T["cum"][i] + t * T["len"][i]


def root(T, cx, cy, lookahead=1.5, goal_span=0, point=None):
    """What a tree keeps of its root position: dict of segment (the nearest over ALL segments), s, goal (-1: none),
    point (px, py) and has (is there a track point: a goal, or the explicit ``point``).  T None: no track."""
    seg, s, g, p = -1, f64("nan"), -1, (f64(0), f64(0))
    if T is not None:
        seg = TS.nearest(T, cx, cy)
        s = arc(T, seg, cx, cy)
        g = TS.goal(T, seg, cx, cy, lookahead, goal_span)
        if g >= 0:
            p = (T["x"][g], T["y"][g])
    has = g >= 0
    if point is not None:
        p, has = (f64(point[0]), f64(point[1])), True
    return dict(segment=seg, s=s, goal=g, point=p, has=has)


def waypoint_terms(vel, xy, point):
    """mcts.py:234 per step: v_i / sqrt((px-x_i)*(px-x_i) + (py-y_i)*(py-y_i)), IEEE inf / NaN kept."""
    px, py = f64(point[0]), f64(point[1])
    out = np.empty(len(vel))
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(len(vel)):
            ex, ey = px - f64(xy[i][0]), py - f64(xy[i][1])
            out[i] = f64(vel[i]) / np.sqrt(ex * ex + ey * ey)
    return out


def progress_terms(T, anchor, window, start_xy, xy):
    """(terms, s, segment, start_s): every position searched over the candidates around ``anchor`` (all when window is
    0), term_i = wrap(s_i - s_(i-1)) with s_(-1) = s of the start."""
    n = len(xy)
    seg = np.empty(n, np.int32)
    s = np.empty(n)
    terms = np.empty(n)
    i0 = TS.nearest(T, start_xy[0], start_xy[1], anchor, window, False)
    start_s = arc(T, i0, start_xy[0], start_xy[1])
    prev = start_s
    for i in range(n):
        seg[i] = TS.nearest(T, xy[i][0], xy[i][1], anchor, window, False)
        s[i] = arc(T, int(seg[i]), xy[i][0], xy[i][1])
        terms[i] = TS.wrap(T, s[i] - prev)[0]
        prev = s[i]
    return terms, s, seg, start_s


def terms(T, mode, window, rt, start_xy, xy, vel):
    """The terms of one roll-out of a tree with root ``rt`` (``root``'s dict)."""
    if mode == PROGRESS:
        return progress_terms(T, rt["segment"], window, start_xy, xy)[0]
    if mode == WAYPOINT and rt["has"]:
        return waypoint_terms(vel, xy, rt["point"])
    return np.array(vel, f64)


def value(index, terms_, action):
    """The value of a roll-out (mcts.py:240-245) from its terms."""
    return MS.reward_of(index, terms_, action)
