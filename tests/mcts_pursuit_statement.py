"""include/scanlib.h "the track steering the search" in plain NumPy float64: the pursuit steer, the expansion answer
of the source RL_MCTS_PURSUIT and the steer of a pursuit roll-out's action, built on tests/track_statement.py (nearest,
goal), tests/mcts_track_statement.py (root) and tests/mcts_statement.py (the draws, the tree).  Every f64 operation is
one NumPy operation, so each is separately rounded as on the device.  The tree needs no change: ``Tree(source="track")``
takes the FG / NN branch of generateAction with the pursuit answers it is given."""
import numpy as np

import mcts_statement as MS
import mcts_track_statement as MTS
import track_statement as TS

RANDOM, PURSUIT = 0, 1                              # rl_mcts_params.rollout_source
f64, f32 = np.float64, np.float32


def pursuit(state, point, wb, max_steer):
    """The float32 steer of a car with state (x, y, th, ...) towards the world point (X, Y)."""
    x, y, th = f64(state[0]), f64(state[1]), f64(state[2])
    X, Y, ms = f64(point[0]), f64(point[1]), f64(max_steer)
    with np.errstate(all="ignore"):
        rx, ry = X - x, Y - y
        hx, hy = np.cos(th), np.sin(th)
        gx = hx * rx + hy * ry
        gy = hx * ry - hy * rx
        d2 = gx * gx + gy * gy
        if not d2 > 0:
            return f32(0)
        a = np.arctan(((f64(2) * f64(wb)) * gy) / d2)
        a = np.fmin(np.fmax(a, -ms), ms)
        return f32(a)


def answer(state, rt, wb, max_steer):
    """The stored expansion answer of a node of a tree with root ``rt`` (``mcts_track_statement.root``'s dict)."""
    return pursuit(state, rt["point"], wb, max_steer) if rt["has"] else f32(0)


def action_steer(T, state, prev_seg, u, *, wb, max_steer, dev, window=0, lookahead=1.5, goal_span=0):
    """Roll-out action m's (steer, nearest segment, goal) from the state before its first step: ``prev_seg`` is the
    tree's root segment for m = 0 and the segment action m - 1 found otherwise; u the draw d = 1 + 2m."""
    cx, cy, ms = f64(state[0]), f64(state[1]), f64(max_steer)
    seg = TS.nearest(T, cx, cy, int(prev_seg), window, False)
    g = TS.goal(T, seg, cx, cy, lookahead, goal_span)
    base = f64(pursuit(state, (T["x"][g], T["y"][g]), wb, max_steer)) if g >= 0 else f64(0)
    steer = np.fmin(np.fmax(base + f64(MS.uniform(-f64(dev), f64(dev), u)), -ms), ms)
    return float(steer), seg, g


def rollout(T, root_seg, state, seed, it, L, every, step, *, max_speed, **kw):
    """One pursuit roll-out of iteration ``it`` from the child state ``state``: ``step(state, speed, steer, n)`` gives
    the (n, 11) states after each of n car steps.  Returns (states (L, 11), actions (n_act, 2) as (speed, steer),
    segments (n_act,), goals (n_act,)).  The draws are the random roll-out's: d = 1 + 2m the steer's, d = 2 + 2m the
    speed's."""
    n_act = (L + every - 1) // every
    states, acts = np.empty((L, 11)), np.empty((n_act, 2))
    segs, goals = np.empty(n_act, np.int32), np.empty(n_act, np.int32)
    cur, seg = np.asarray(state, f64), int(root_seg)
    for m in range(n_act):
        us = MS.uniform01(seed, 1 + 2 * m, it)
        uv = MS.uniform01(seed, 2 + 2 * m, it)
        steer, seg, g = action_steer(T, cur, seg, us, **kw)
        speed = MS.uniform(0, max_speed, uv)
        n = min(every, L - m * every)
        out = np.asarray(step(cur, speed, steer, n), f64).reshape(n, 11)
        states[m * every:m * every + n] = out
        acts[m], segs[m], goals[m] = (speed, steer), seg, g
        cur = out[-1]
    return states, acts, segs, goals


def root(T, cx, cy, lookahead=1.5, goal_span=0, point=None):
    """The tree's root on the track (``mcts_track_statement.root``): its segment starts every roll-out's search, its
    point is what the source pursues."""
    return MTS.root(T, cx, cy, lookahead, goal_span, point)
