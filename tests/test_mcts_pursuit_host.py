"""The track steering the MCTS without a GPU (include/scanlib.h "the track steering the search"): the statement
(tests/mcts_pursuit_statement.py) on known answers, a pursuit roll-out that holds a ring, the draws it consumes, what
the header and ``_lib`` say of the new source and fields, and every Python-side refusal."""
import ctypes as C
import math

import numpy as np
import pytest

import mcts_pursuit_statement as S
import mcts_statement as MS
import scanlib_header as H
import track_statement as TS
from test_population_host import no_calls  # noqa: F401  (a fixture)
from pyracecarsimulator_amd import _lib
from pyracecarsimulator_amd import racecar as RC
from pyracecarsimulator_amd.mcts import MCTS, ROLLOUTS, SOURCES, MCTSPlanner, rollout_args, steering_args
from pyracecarsimulator_amd.racecar_simulator import RacecarSimulator

WB, MAX_STEER = RC.DEFAULT_CAR["wb"], RC.DEFAULT_CAR["max_steer_ang"]


def _bits(a):
    return np.float32(a).tobytes()


# ---------------------------------------------------------------- the pursuit steer
def test_pursuit_known_answers():
    p = lambda st, pt: S.pursuit(st, pt, WB, MAX_STEER)              # noqa: E731
    for th in (0.0, 0.7, -2.9, math.pi / 2):
        st = np.array([1.5, -2.0, th])
        hx, hy = math.cos(th), math.sin(th)
        left = (st[0] + 2.0 * hx - 0.5 * hy, st[1] + 2.0 * hy + 0.5 * hx)
        right = (st[0] + 2.0 * hx + 0.5 * hy, st[1] + 2.0 * hy - 0.5 * hx)
        a = p(st, left)
        assert isinstance(a, np.float32) and 0 < a < MAX_STEER
        assert isinstance(p(st, right), np.float32) and p(st, right) < 0
    # dead ahead, and the mirror image bit for bit (heading 0: the mirror is exact)
    st = np.array([0.25, 0.5, 0.0])
    assert _bits(p(st, (3.25, 0.5))) == _bits(0.0)
    for gx, gy in ((2.0, 0.5), (0.75, 0.125), (-1.0, 0.25), (5.0, 3.0)):
        a, b = p(st, (0.25 + gx, 0.5 + gy)), p(st, (0.25 + gx, 0.5 - gy))
        assert a > 0 and _bits(a) == _bits(-b), (gx, gy)
        want = min(math.atan(2.0 * WB * gy / (gx * gx + gy * gy)), MAX_STEER)
        assert abs(float(a) - want) <= 2.0 ** -24 * want + 1e-12
    # the point at the car, NaN anywhere
    assert _bits(p(st, (0.25, 0.5))) == _bits(0.0)
    for bad in (np.array([math.nan, 0.5, 0.0]), np.array([0.25, math.nan, 0.0]), np.array([0.25, 0.5, math.nan])):
        assert _bits(p(bad, (1.0, 1.0))) == _bits(0.0)
    assert _bits(p(st, (math.nan, 1.0))) == _bits(0.0) and _bits(p(st, (1.0, math.nan))) == _bits(0.0)
    # the clamp, from both sides: a point close beside the car
    assert _bits(p(st, (0.25, 0.5 + 0.2))) == _bits(MAX_STEER) and _bits(p(st, (0.25, 0.5 - 0.2))) == _bits(-MAX_STEER)
    assert _bits(p(st, (0.3, 0.6))) == _bits(MAX_STEER)
    # the answer of a tree: the point's pursuit, 0.0f without one
    rt = dict(point=(3.0, 1.0), has=True)
    assert _bits(S.answer(st, rt, WB, MAX_STEER)) == _bits(p(st, (3.0, 1.0))) != _bits(0.0)
    assert _bits(S.answer(st, dict(point=(0.0, 0.0), has=False), WB, MAX_STEER)) == _bits(0.0)


# ---------------------------------------------------------------- holding the path
def ring(n=150, centre=(2.5, 4.5), rx=4.6, ry=4.2):
    a = 2 * math.pi * np.arange(n) / n
    return np.stack([centre[0] + rx * np.cos(a), centre[1] + ry * np.sin(a)], -1)


def kinematic_step(state, speed, steer, n, dt=0.01, steer_vel=5.0):
    """A kinematic single-track car at constant speed (the form of Car::updateNormal): the (n, 11) states after each step."""
    x, y, th, sa = (float(v) for v in (state[0], state[1], state[2], state[4]))
    out = np.zeros((n, 11))
    for i in range(n):
        x, y, th = x + speed * math.cos(th) * dt, y + speed * math.sin(th) * dt, th + speed / WB * math.tan(sa) * dt
        d = steer - sa
        sa = min(max(sa + (math.copysign(steer_vel, d) if abs(d) > 1e-4 else 0.0) * dt, -MAX_STEER), MAX_STEER)
        out[i, :5] = (x, y, th, speed, sa)
    return out


def test_a_pursuit_rollout_holds_the_ring():
    """600 steps at 2 m/s from a start on a 150-point ellipse, action_every 10, window 2, goal_span 8, no deviation:
    every action has a goal, and the nearest segment never moves backwards."""
    xy = ring()
    T = TS.build(xy, True)
    st = np.zeros(11)
    st[:2] = 0.5 * (xy[3] + xy[4])
    st[2] = math.atan2(T["dy"][3], T["dx"][3])
    rt = S.root(T, st[0], st[1], 1.5, 8)
    assert rt["segment"] == 3 and rt["goal"] >= 0
    states, acts, segs, goals = S.rollout(T, rt["segment"], st, 11, 0, 600, 10,
                                          lambda s, v, a, n: kinematic_step(s, 2.0, a, n), max_speed=7.0, wb=WB,
                                          max_steer=MAX_STEER, dev=0.0, window=2, lookahead=1.5, goal_span=8)
    assert (goals >= 0).all() and len(goals) == 60
    step = (np.diff(segs.astype(int)) + T["S"]) % T["S"]
    assert (step <= 2).all(), step                                   # forwards by at most the window, never backwards
    assert (segs[-1] - segs[0]) % T["S"] >= 40                       # 12 m of a 27.7 m ring
    d2 = [TS.project(T, TS.nearest(T, s[0], s[1]), s[0], s[1])[0] for s in states[::10]]
    assert max(d2) < 0.3 ** 2, max(d2)
    assert (np.abs(acts[:, 1]) <= MAX_STEER).all() and (acts[:, 0] >= 0).all() and (acts[:, 0] < 7.0).all()


# ---------------------------------------------------------------- the draws
def test_pursuit_rollouts_consume_the_random_rollouts_draws(monkeypatch):
    """A tree with the track source and pursuit roll-outs with a deviation: iteration i reads the counters (d, i) with
    d = 1 + 2m and 2 + 2m for every action m, d = 0 where the expansion samples, and no other."""
    seen = []
    real = MS.uniform01

    def spy(seed, d, i):
        seen.append((int(seed), int(np.asarray(d).reshape(-1)[0]), int(np.asarray(i).reshape(-1)[0])))
        assert np.asarray(d).size == 1
        return real(seed, d, i)
    monkeypatch.setattr(MS, "uniform01", spy)
    xy = ring()
    T = TS.build(xy, True)
    st = np.zeros(11)
    st[:2], st[2] = 0.5 * (xy[0] + xy[1]), math.pi / 2
    rt = S.root(T, st[0], st[1], 1.5, 0)
    L, every, seed = 23, 5, 77
    n_act = 5
    tree = MS.Tree(st, np.zeros(3, np.float32), float(S.answer(st, rt, WB, MAX_STEER)), 0.1, seed, source="track")
    steers = []

    def act(i, reqs):
        out = []
        for _, node, a in reqs:
            new = kinematic_step(node.state, 2.0, a, 1)[0]
            out.append((new, node.pose, float(S.answer(new, rt, WB, MAX_STEER)), False))
        return out

    def ro(i, reqs, acts):
        out = []
        for _, child in reqs:
            states, a, _, _ = S.rollout(T, rt["segment"], child.state, seed, i, L, every,
                                        lambda s, v, a_, n: kinematic_step(s, 2.0, a_, n), max_speed=7.0, wb=WB,
                                        max_steer=MAX_STEER, dev=0.2, window=3, lookahead=1.5, goal_span=6)
            steers.append(a[:, 1])
            assert a[:, 0].tolist() == [MS.uniform(0, 7.0, real(seed, 2 + 2 * m, i)) for m in range(n_act)]   # the same speeds
            out.append((-(L + 1), states[:, 3]))
        return out
    n_it = 6
    seen.clear()
    arr = MS.run_lockstep([tree], n_it, act, ro, snapshots=(n_it,))[n_it][0]
    rollout = {d for m in range(n_act) for d in (1 + 2 * m, 2 + 2 * m)}
    sampled = 0
    for i in range(n_it):
        mine = sorted(d for s, d, j in seen if j == i and s == seed)
        assert set(mine) - {0} == rollout and len(mine) == len(set(mine)), (i, mine)
        sampled += 0 in mine
    assert {s for s, _, _ in seen} == {seed} and {j for _, _, j in seen} == set(range(n_it))
    assert 0 < sampled < n_it                                        # first children take the answer, later ones sample
    assert arr["action"][1] == float(np.float32(arr["answer"][0]))   # the root's first child: (double)answer
    assert len({s.tobytes() for s in steers}) == n_it                # the deviation differs per iteration


# ---------------------------------------------------------------- the header and the table
def test_header_and_table():
    hdr = H.read("scanlib.h")
    src = hdr.enums()["rl_mcts_source"]
    assert len(src) == 4 and sorted(src.values()) == [0, 1, 2, 3]
    assert {getattr(_lib, n) for n in src} == {0, 1, 2, 3} and all(getattr(_lib, n) == v for n, v in src.items())
    assert SOURCES == {"fg": 0, "nn": 1, "random": 2, "track": 3} and ROLLOUTS == {"random": 0, "pursuit": 1}
    fields = [n for n, _ in hdr.structs()["rl_mcts_params"]]
    assert fields[-2:] == ["rollout_source", "rollout_dev"]
    assert fields == [n for n, _ in _lib.MctsParams._fields_]
    assert [t for _, t in hdr.structs()["rl_mcts_params"]][-2:] == [C.c_int, C.c_double]
    z = _lib.MctsParams()
    assert z.rollout_source == 0 and z.rollout_dev == 0.0 and z.source == 0
    assert len(_lib.HEADERS) == 7 and sum(len(h.symbols) for h in _lib.HEADERS) == 135
    raw = open(hdr.path).read()
    assert "atan(((2.0 WB) gy) / d2)" in raw and raw.count("atan(((2.0 WB) gy) / d2)") == 1


# ---------------------------------------------------------------- the wrappers' refusals
def test_wrappers_refuse_before_the_library(no_calls):
    assert rollout_args() == (0, 0.1) and rollout_args("pursuit", 0.0) == (1, 0.0)
    for kw in (dict(rollout="track"), dict(rollout=1), dict(rollout="pursuit", rollout_dev=-0.1),
               dict(rollout_dev=math.nan), dict(rollout_dev=math.inf)):
        with pytest.raises(ValueError):
            rollout_args(**kw)
    steering_args("track", "random", None, True)
    steering_args("track", "pursuit", object(), False)
    steering_args("fg", "random", None, False)
    for a in (("track", "random", None, False), ("fg", "pursuit", None, False), ("track", "pursuit", None, True)):
        with pytest.raises(ValueError):
            steering_args(*a)
    # the planner: its constructor's keywords, and what it needs before a search
    with pytest.raises(ValueError):
        MCTSPlanner(None, None, 1, 2, 4.7, 10, np.zeros(10), 0.1, source="track", rollout="fast")
    with pytest.raises(ValueError):
        MCTSPlanner(None, None, 1, 2, 4.7, 10, np.zeros(10), 0.1, rollout="pursuit", rollout_dev=-1.0)
    for source, rollout in (("track", "random"), ("fg", "pursuit")):
        pl = MCTSPlanner.__new__(MCTSPlanner)
        pl.n_trees, pl.source, pl.rollout = 2, source, rollout
        with pytest.raises(ValueError):
            pl.reset(np.zeros((2, 11)), 0.0, [1, 2])
        with pytest.raises(ValueError):
            pl.run(1)
        with pytest.raises(ValueError):
            pl.drive(np.zeros((2, 11)), 0.0, [1, 2], 1, 2)
        with pytest.raises(ValueError):
            pl.attach_track(object(), "velocity", lookahead=0.0)
        with pytest.raises(ValueError):
            pl.attach_track(object(), "progress", lookahead=math.nan)
    with pytest.raises(ValueError):
        pl.set_points(np.zeros((2, 2)), reward="progress")
    # the drop-in and the batched calls
    for kw in (dict(source="track"), dict(rollout="pursuit"), dict(rollout="pursuit", track_point=(1.0, 2.0), source="track"),
               dict(rollout="walk"), dict(rollout_dev=-0.5), dict(source="pursuit")):
        with pytest.raises(ValueError):
            MCTS.__new__(MCTS).__init__(None, None, 0.0, 10, **kw)
    cars = RC.CarBatch.__new__(RC.CarBatch)
    sim = RacecarSimulator.__new__(RacecarSimulator)
    st = np.zeros((2, 11))
    for kw in (dict(source="track"), dict(rollout="pursuit"), dict(rollout="uniform"), dict(rollout_dev=math.nan)):
        with pytest.raises(ValueError):
            cars.plan_mcts(None, None, st, 3, [1, 2], 4.7, 10, np.zeros(10), 0.1, **kw)
        with pytest.raises(ValueError):
            cars.drive_mcts(None, None, st, 2, 3, [1, 2], 4.7, 10, np.zeros(10), 0.1, **kw)
        with pytest.raises(ValueError):
            sim.planMCTSMany(st, 3, **kw)
        with pytest.raises(ValueError):
            sim.driveMCTSMany(st, 2, 3, **kw)
