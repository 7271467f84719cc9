"""The track-guided planner's cases and checks (include/scanlib_track_plan.h): the per-step float64 states of a
roll-out from the public roll-out call, the statement of the search (tests/mcts_checks.py ``replay``, unchanged) answered
with the statement's terms (tests/mcts_track_statement.py), and the device run with a track attached."""
import math

import numpy as np

import mcts_checks as MC
import mcts_track_statement as S
import support
import track_statement as TS
from support import FOV, THRESH, same_bits
from pyracecarsimulator_amd.mcts import REWARDS, MCTSPlanner

STD = 0.01
MODES = {"velocity": S.VELOCITY, "waypoint": S.WAYPOINT, "progress": S.PROGRESS}
assert MODES == REWARDS


def step_states(cars, states, actions, n_steps, action_every):
    """The float64 states after every step of R roll-outs, (R, n_steps, 11): step i is the final state of
    ``cars.rollout(..., n_steps=i + 1)``, which the car tests pin to the reference ``Car``."""
    states = np.asarray(states, np.float64).reshape(-1, 11)
    R = states.shape[0]
    actions = np.asarray(actions, np.float64).reshape(R, -1, 2)
    out = np.empty((R, n_steps, 11))
    for i in range(n_steps):
        n_act = (i + 1 + action_every - 1) // action_every
        _, fin, _ = cars.rollout(states, np.ascontiguousarray(actions[:, :n_act]), n_steps=i + 1, action_every=action_every)
        out[:, i] = fin
    return out


def ring(centre, rx, ry, n, phase=0.3):
    """n points on an ellipse, counter-clockwise."""
    a = phase + 2 * math.pi * np.arange(n) / n
    return np.stack([centre[0] + rx * np.cos(a), centre[1] + ry * np.sin(a)], -1)


def ring_around(states, n=70):
    """A closed ring of n waypoints through the region the root states lie in."""
    xy = np.asarray(states)[:, :2]
    c = xy.mean(0)
    r = np.maximum(0.75 * (xy.max(0) - xy.min(0)), 2.0)
    return ring(c, r[0], r[1], n)


class TermCars:
    """``cars`` for ``mcts_checks.replay``: its roll-outs answer with the statement's terms where the velocities stood.
    roots: the K trees' ``mcts_track_statement.root`` dicts; ``log`` receives (crash index, terms, velocities) of
    every roll-out of every tree, terminal children included."""

    def __init__(self, cars, T, mode, window, roots):
        self.cars, self.T, self.mode, self.window, self.roots, self.log = cars, T, mode, window, roots, []

    def rollout(self, *a, **kw):
        return self.cars.rollout(*a, **kw)

    def rollout_check(self, m, states, actions, fov, num_rays, edge, thresh, n_steps, action_every):
        first, out, vel = self.cars.rollout_check(m, states, actions, fov, num_rays, edge, thresh, n_steps=n_steps,
                                                  action_every=action_every)
        st = step_states(self.cars, states, actions, n_steps, action_every)
        assert same_bits(st[:, :, 3], vel) and same_bits(st[:, -1], out)
        terms = np.stack([S.terms(self.T, self.mode, self.window, self.roots[k], states[k, :2], st[k, :, :2], vel[k])
                          for k in range(len(states))])
        self.log.extend((int(first[k]), terms[k], vel[k]) for k in range(len(states)))
        return first, out, terms


def statement_roots(T, states, lookahead, goal_span, points=None):
    return [S.root(T, states[k, 0], states[k, 1], lookahead, goal_span, None if points is None else points[k])
            for k in range(len(states))]


def attach(pl, track, reward, lookahead, window, goal_span, points=None):
    if points is not None:
        pl.set_points(points)
    if track is not None:
        pl.attach_track(track, reward, lookahead=lookahead, window=window, goal_span=goal_span)


def device(cars, m, base, source, h, states, actions, seeds, n_it, track, reward, *, lookahead=1.5, window=0, goal_span=0,
           points=None, num_rays=MC.B, rollout_steps=MC.L, action_every=MC.EVERY):
    """``mcts_checks.device`` with a track attached (or explicit points set) before the reset."""
    m.set_noise(STD, 99, base)
    pl = MCTSPlanner(cars, m, len(states), n_it + 1, FOV, num_rays, support.edge(num_rays), THRESH, source=source,
                     followgap=h if source == "fg" else None, rollout_steps=rollout_steps, action_every=action_every)
    attach(pl, track, reward, lookahead, window, goal_span, points)
    pl.reset(states, actions, seeds)
    pl.run(n_it)
    return pl, [pl.read_tree(k) for k in range(len(states))], pl.best()


def replay(cars, m, base, source, h, states, actions, seeds, n_it, dev_trees, T, reward, *, lookahead=1.5, window=0,
           goal_span=0, points=None, num_rays=MC.B, rollout_steps=MC.L, action_every=MC.EVERY):
    """The statement of the K trees with the track's terms: (trees, arrays of every tree after n_it iterations, the
    statement's roots, the roll-out log)."""
    rts = statement_roots(T, states, lookahead, goal_span, points)
    mode = MODES[reward] if T is not None else (S.WAYPOINT if points is not None else S.VELOCITY)
    tc = TermCars(cars, T, mode, window, rts)
    trees, snaps = MC.replay(tc, m, STD, base, source, h, states, actions, seeds, n_it, dev_trees, (n_it,),
                             num_rays=num_rays, rollout_steps=rollout_steps, action_every=action_every)
    return trees, snaps[n_it], rts, tc.log


def assert_roots(got, want, what):
    """``MCTSPlanner.read_track`` against the statement's roots."""
    for k, rt in enumerate(want):
        assert got["segment"][k] == rt["segment"] and got["goal"][k] == rt["goal"], (what, k)
        assert same_bits(got["s"][k:k + 1], np.array([rt["s"]])), (what, k)
        assert same_bits(got["point"][k], np.array(rt["point"], np.float64)), (what, k)


def conditions(trees, log, L):
    """(roll-outs of non-terminal children that crashed at 0 < index < L, those that did not crash, terminal
    children), counted from the statement."""
    live = [n for t in trees for n in t.nodes[1:] if not n.terminal]
    mid = sum(1 for n in live if 0 < n.crash < L)
    none = sum(1 for n in live if n.crash < 0)
    term = sum(1 for t in trees for n in t.nodes[1:] if n.terminal)
    return mid, none, term
