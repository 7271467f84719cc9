"""The track steering the MCTS on the MI355X (include/scanlib.h "the track steering the search": the source
RL_MCTS_PURSUIT, rl_mcts_params.rollout_source / rollout_dev; kernels csrc/plan_pursuit_kernels.h): every node array,
state, action, reward, crash index and best action of every tree bit-identical to the statement
(tests/mcts_pursuit_statement.py on tests/mcts_statement.py) replayed with the public calls, every stored answer equal
to the statement's pursuit of that node's own device state, the drive equal to the loop composed on the host, nothing
else moved, and every refusal of the contract.

Shapes: K = 9 trees (past one workgroup of 8 waves), 65 beams, L = 12 with action_every = 5 (three actions, the last cut
short), in test_gpu_track.py's room around the waypoint file; a closed 150-point ring (the lanes stride over more than 64
segments and the window wraps over the start line) and an open 3-point track."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import mcts_checks as MC
import mcts_pursuit_checks as PC
import mcts_track_checks as TC
import support
import track_statement as TS
from conftest import GOLD
from support import FOV, THRESH, same_bits
from pyracecarsimulator_amd import MCTS, RacecarSimulator, Track, _lib, maps, range_libc
from pyracecarsimulator_amd import racecar as RC
from pyracecarsimulator_amd.mcts import MCTSPlanner

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

K, B, I, L, EVERY, BASE = 9, 65, 37, 12, 5, 777
SHAPE = dict(num_rays=B, rollout_steps=L, action_every=EVERY)
RL_ERR_INVALID = -1
WALL = (8.55, 5.0, 0.0)                         # 0.4 m short of the room's wall at x = 9, heading for it


def ring150():
    a = np.sort(np.random.default_rng(150).uniform(0.0, 2 * math.pi, 150))       # uneven spacing
    return np.stack([2.5 + 4.6 * np.cos(a), 4.5 + 4.2 * np.sin(a)], -1)


TRACKS = {"wp36": (Track.read_csv(os.path.join(GOLD, "wp_u.csv")), True), "ring150": (ring150(), True),
          "open3": (np.array([(0.0, 1.0), (6.0, 1.0), (3.0, 7.0)]), False)}


@pytest.fixture(scope="module")
def world():
    """test_gpu_track.py's 13 m room (x -4 .. 9, y -2 .. 11), RMGPU, one CarBatch, FollowGap, and per track its table, its
    handle and K roots on it (the last one in front of the wall)."""
    g = maps.make_room(260, resolution=0.05, origin=(-4.0, -2.0, 0.0))
    omap = range_libc.PyOMap(g)
    w = {"g": g, "omap": omap, "m": range_libc.PyRayMarchingGPU(omap, 300), "cars": RC.CarBatch(), "fg": support.followgap()}
    for name, (xy, closed) in TRACKS.items():
        T = TS.build(xy, closed)
        w[name] = dict(T=T, track=Track(xy, closed), roots=PC.roots_on(T, K, 5, wall=WALL))
    return w


def both(world, name, source, reward, n_it=I, what=None, **kw):
    c = world[name]
    st, ac, sd = kw.pop("roots", c["roots"])
    shape = dict(SHAPE)
    shape.update({k: kw.pop(k) for k in list(kw) if k in SHAPE})
    h = world["fg"] if source == "fg" else None
    track, T = (None, None) if kw.pop("no_track", False) else (c["track"], c["T"])
    out = PC.run_both(world["cars"], world["m"], BASE, source, h, st, ac, sd, n_it, track, T, reward, what, **shape, **kw)
    out[0].close()
    world["m"].set_noise(0.0, 0, 0)
    return out[1:]


# ---------------------------------------------------------------- 1. the track as the expansion source
@pytest.mark.parametrize("goal_span", [0, 2])
@pytest.mark.parametrize("reward", ["velocity", "waypoint", "progress"])
def test_track_source_equals_the_statement(world, reward, goal_span):
    """37 iterations of 9 trees in every reward mode: the trees are the statement's, the stored answers the pursuit of
    the tree's point from the node's own state; there are terminal children and crashed and whole roll-outs among them."""
    dev, trees, rts, log, _ = both(world, "wp36", "track", reward, goal_span=goal_span, window=goal_span)
    assert all(rt["goal"] >= 0 for rt in rts)
    ans = np.concatenate([t["answer"] for t in dev])
    assert np.isfinite(ans).all() and (ans != 0).sum() > ans.size // 2 and (np.abs(ans) <= np.float32(support.MAX_STEER)).all()
    mid, none, term = TC.conditions(trees, log, L)
    print("roll-outs crashed mid-way %d, not crashed %d, terminal children %d" % (mid, none, term))
    assert none >= 1 and mid + term >= 1, (mid, none, term)
    for k in range(K):                              # the first child of every node took (double)answer
        t = dev[k]
        first = t["first_child"][t["first_child"] >= 0]
        assert same_bits(t["action"][first], t["answer"][t["first_child"] >= 0].astype(np.float64)), k


def test_track_source_without_a_goal_answers_zero(world):
    """A lookahead of 0.3 m with goal_span 2: some roots have no goal; every answer of their trees reads 0.0f, the first
    children take 0.0, and the search runs on (its value is sum / |0| = inf, as FollowGap's 0 answer gives).  The
    roots are all on the track, far from the walls: every sum of velocities is positive, so no inf meets a -inf."""
    roots = PC.roots_on(world["wp36"]["T"], K, 5)
    dev, trees, rts, _, _ = both(world, "wp36", "track", "velocity", n_it=9, lookahead=0.3, goal_span=2, roots=roots)
    without = [k for k in range(K) if rts[k]["goal"] < 0]
    assert 0 < len(without) < K, without
    for k in range(K):
        zero = (dev[k]["answer"].view(np.uint32) == 0).all()
        assert zero == (k in without), k
        assert len(dev[k]["parent"]) == 10


@pytest.mark.parametrize("reward,track", [("waypoint", False), ("velocity", False), ("progress", True)])
def test_track_source_with_explicit_points(world, reward, track):
    """rl_mcts_set_points: the explicit point is pursued; alone it carries the waypoint reward or, if told, the velocity
    reward; with a track attached the track's reward mode and the given point."""
    st = world["wp36"]["roots"][0]
    pts = st[:, :2] + np.random.default_rng(9).uniform(-3.0, 3.0, (K, 2))
    dev, _, rts, _, _ = both(world, "wp36", "track", reward, n_it=9, points=pts, no_track=not track)
    assert all(rt["has"] and rt["point"] == (pts[k, 0], pts[k, 1]) for k, rt in enumerate(rts))
    assert all((rt["segment"] >= 0) == track for rt in rts)
    assert all((t["answer"] != 0).any() for t in dev)


# ---------------------------------------------------------------- 2. pursuit roll-outs
CASES = [  # source, track, window, goal_span, rollout_dev, reward, iterations, shape
    ("random", "ring150", 0, 0, 0.0, "progress", I, {}),
    ("fg", "ring150", 1, 2, 0.2, "progress", I, {}),
    ("track", "ring150", 8, 2, 0.2, "waypoint", I, {}),
    ("track", "ring150", 8, 0, 0.0, "progress", 9, {}),
    ("random", "open3", 0, 2, 0.2, "progress", 9, {}),
    ("fg", "open3", 1, 0, 0.0, "waypoint", 9, {}),
    ("track", "wp36", 1, 2, 0.2, "progress", 9, dict(rollout_steps=1)),
    ("random", "wp36", 8, 2, 0.2, "velocity", 9, dict(action_every=L + 3)),
]


@pytest.mark.parametrize("source,name,window,goal_span,dev,reward,n_it,shape", CASES)
def test_pursuit_rollouts_equal_the_statement(world, source, name, window, goal_span, dev, reward, n_it, shape):
    trees_dev, trees, rts, log, goals = both(world, name, source, reward, n_it=n_it, rollout="pursuit", rollout_dev=dev,
                                             window=window, goal_span=goal_span, **shape)
    goals = np.stack(goals)                                     # (iterations, K, n_act)
    T = world[name]["T"]
    print("goals found %d of %d; roll-outs %s" % ((goals >= 0).sum(), goals.size, TC.conditions(trees, log, shape.get("rollout_steps", L))))
    assert (goals >= 0).sum() > (0 if name == "open3" else goals.size // 2)      # (open3's waypoints lie 6 m apart)
    if name == "ring150" and window:
        segs = [rt["segment"] for rt in rts]
        assert min(segs) - window < 0 or max(segs) + window >= T["S"], segs      # a window wraps over the start line
    # the trees are not those of random roll-outs, where the reward sees the positions (the velocities of a roll-out do
    # not depend on its steers, and one step does not depend on its own steer)
    if reward == "velocity" or shape.get("rollout_steps", L) == 1:
        return
    pl, plain, _ = PC.device(world["cars"], world["m"], BASE, source, world["fg"] if source == "fg" else None,
                             *world[name]["roots"], n_it, world[name]["track"], reward, window=window, goal_span=goal_span,
                             **dict(SHAPE, **shape))
    pl.close()
    world["m"].set_noise(0.0, 0, 0)
    assert any(not same_bits(plain[k]["reward"], trees_dev[k]["reward"]) for k in range(K))


# ---------------------------------------------------------------- 3. the drive
def test_drive_equals_the_host_composed_loop(world):
    """D = 3 decisions x 5 iterations x 2 steps, the track source with pursuit roll-outs, the last car inside the crash
    margin: drive equals reset / run / best composed on the host on a second planner, read_track gives the last
    decision's roots, the handle's option and noise offset read as before."""
    cars, m, c = world["cars"], world["m"], world["ring150"]
    D, I_, S_ = 3, 5, 2
    st, rec, sd = (a.copy() for a in c["roots"])
    st[K - 1, 0] = 8.72                                          # the front of the car is in the wall
    mk = lambda: PC.planner(cars, m, K, I_, "track", None, rollout="pursuit", rollout_dev=0.2, **SHAPE)     # noqa: E731
    host_pl, dev_pl = mk(), mk()
    try:
        for pl in (host_pl, dev_pl):
            pl.attach_track(c["track"], "progress", lookahead=1.5, window=8, goal_span=2)
        want = MC.host_loop(cars, m, host_pl, TC.STD, BASE, st, rec, sd, D, I_, S_, MC.CLIP, num_rays=B, rollout_steps=L)
        print("first (host loop):", want[0])
        assert want[0][K - 1] == 0 and (want[0][:K - 1] < 0).any()
        m.set_noise(TC.STD, 99, BASE)
        probe = st[:2, :3].astype(np.float32)
        before, nt = MC.scan_keep(m, probe, B), m.get_info("nt_store")
        got = dev_pl.drive(st, rec, sd, D, I_, steps_per_decision=S_, steer_clip=MC.CLIP, trace=True)
        MC.assert_drive(got, want, "pursuit")
        for k in range(K):
            MC.assert_tree(dev_pl.read_tree(k), host_pl.read_tree(k), ("drive", k))
        last = np.where(np.isnan(got[5][:, D - 1]), got[1], got[5][:, D - 1])
        rts = TC.statement_roots(c["T"], last, 1.5, 2)
        TC.assert_roots(dev_pl.read_track(), rts, "drive")
        TC.assert_roots(host_pl.read_track(), rts, "drive")
        PC.assert_answers([dev_pl.read_tree(k) for k in range(K)], rts, "track")
        assert m.get_info("nt_store") == nt and same_bits(MC.scan_keep(m, probe, B), before)
        # explicit points are still refused by the drive
        dev_pl.set_points(st[:, :2] + 1.0)
        with pytest.raises(ValueError):
            dev_pl.drive(st, rec, sd, D, I_)
    finally:
        host_pl.close()
        dev_pl.close()
        m.set_noise(0.0, 0, 0)


# ---------------------------------------------------------------- 4. nothing else moved
def test_nothing_else_moved(world):
    """Source fg with a track attached and random roll-outs: the trees of a planner whose new fields are zero, whatever
    rollout_dev holds.  For the new modes: n iterations equal n/2 followed by n/2, and h reads as before every call."""
    cars, m, c = world["cars"], world["m"], world["wp36"]
    st, ac, sd = c["roots"]
    n = 8
    pl0, want, best0 = TC.device(cars, m, BASE, "fg", world["fg"], st, ac, sd, n, c["track"], "progress", window=3, **SHAPE)
    assert pl0.params.rollout_source == 0
    pl0.close()
    pl1, got, best1 = PC.device(cars, m, BASE, "fg", world["fg"], st, ac, sd, n, c["track"], "progress", window=3,
                                rollout="random", rollout_dev=0.7, **SHAPE)
    pl1.close()
    for k in range(K):
        MC.assert_tree(got[k], want[k], ("fg twin", k))
    assert all(same_bits(a, b) for a, b in zip(best0, best1))
    probe = st[:2, :3].astype(np.float32)
    for source, rollout in (("track", "random"), ("random", "pursuit"), ("track", "pursuit")):
        m.set_noise(TC.STD, 99, BASE)
        before, nt = MC.scan_keep(m, probe, B), m.get_info("nt_store")
        pl, whole, _ = PC.device(cars, m, BASE, source, None, st, ac, sd, n, c["track"], "progress", window=3, goal_span=2,
                                 rollout=rollout, rollout_dev=0.2, **SHAPE)
        try:
            assert m.get_info("nt_store") == nt and same_bits(MC.scan_keep(m, probe, B), before), (source, rollout)
            pl.reset(st, ac, sd)
            pl.run(n // 2)
            assert m.get_info("nt_store") == nt and same_bits(MC.scan_keep(m, probe, B), before), (source, rollout)
            pl.run(n // 2)
            for k in range(K):
                MC.assert_tree(pl.read_tree(k), whole[k], (source, rollout, k))
        finally:
            pl.close()
            m.set_noise(0.0, 0, 0)


# ---------------------------------------------------------------- 5. the refusals
def _params(mode=2, window=0, span=0, la=1.5):
    p = _lib.PlanTrackParams()
    p.reward_mode, p.window, p.goal_span, p.lookahead = mode, window, span, la
    return p


def _refused(name, *args):
    with pytest.raises(_lib.ScanLibError) as e:
        _lib.call(name, *args)
    assert e.value.code == RL_ERR_INVALID, (name, str(e.value))


def test_refusals_leave_the_handles_usable(world):
    cars, m, c = world["cars"], world["m"], world["wp36"]
    Kr, Ir = 3, 4
    st, ac, sd = (np.ascontiguousarray(a[:Kr]) for a in c["roots"])
    edge = support.edge(B)
    # create: source 3 takes no handle; the roll-out fields
    good = PC.planner(cars, m, Kr, Ir, "track", None, rollout="pursuit", rollout_dev=0.2, **SHAPE)
    for field, bad in (("rollout_source", 2), ("rollout_source", -1), ("rollout_dev", -0.1), ("rollout_dev", math.nan),
                       ("rollout_dev", math.inf), ("source", 4)):
        p = _lib.MctsParams.from_buffer_copy(good.params)
        setattr(p, field, bad)
        h = C.c_void_p()
        _refused("rl_mcts_create", cars, m, None, None, p, edge, h)
        assert not h.value
    p = _lib.MctsParams.from_buffer_copy(good.params)                     # rollout_dev is not read with rollout_source 0
    p.rollout_source, p.rollout_dev = 0, math.nan
    h = C.c_void_p()
    _lib.call("rl_mcts_create", cars, m, None, None, p, edge, h)
    _lib.call("rl_mcts_destroy", h)
    drive_out = (np.empty(Kr, np.int32), np.empty((Kr, 11)), np.empty(Kr), np.empty((Kr, 1)), np.empty((Kr, 1), np.int32), None)
    try:
        m.set_noise(TC.STD, 99, BASE)
        # neither a track nor points: reset, run and drive
        _refused("rl_mcts_reset", good, st, ac, sd)
        _refused("rl_mcts_run", good, 1)
        _refused("rl_mcts_drive", good, st, ac, sd, 1, 2, 1, 0.0, *drive_out)
        # points do not help a roll-out
        good.set_points(st[:, :2] + 1.0)
        _refused("rl_mcts_reset", good, st, ac, sd)
        _refused("rl_mcts_drive", good, st, ac, sd, 1, 2, 1, 0.0, *drive_out)
        good.set_points(None)
        # attach: the lookahead in every reward mode
        for mode in (0, 1, 2):
            for la in (0.0, -1.0, math.nan, math.inf):
                _refused("rl_mcts_attach_track", good, c["track"], _params(mode=mode, la=la))
        _refused("rl_mcts_attach_track", good, None, _params(mode=2))     # (points alone cannot run the progress reward)
        good.attach_track(c["track"], "velocity", lookahead=1.5, window=2, goal_span=2)
        good.reset(st, ac, sd)
        good.run(Ir)
        want = [good.read_tree(k) for k in range(Kr)]
        _refused("rl_mcts_attach_track", good, c["track"], _params(mode=0, la=0.0))
        for k in range(Kr):
            MC.assert_tree(good.read_tree(k), want[k], ("after a refused attach", k))
        good.detach_track()
        _refused("rl_mcts_run", good, 1)
        _refused("rl_mcts_reset", good, st, ac, sd)
        m.set_noise(TC.STD, 99, BASE)
        good.attach_track(c["track"], "velocity", lookahead=1.5, window=2, goal_span=2)
        good.reset(st, ac, sd)
        good.run(Ir)
        for k in range(Kr):
            MC.assert_tree(good.read_tree(k), want[k], ("usable", k))
    finally:
        good.close()
        m.set_noise(0.0, 0, 0)
    # the track source alone: explicit points excuse the lookahead, and are refused by the drive as before
    pl = PC.planner(cars, m, Kr, Ir, "track", None, **SHAPE)
    try:
        _refused("rl_mcts_attach_track", pl, c["track"], _params(mode=2, la=0.0))
        pl.set_points(st[:, :2] + 1.0)
        _lib.call("rl_mcts_attach_track", pl, c["track"], _params(mode=2, la=0.0))
        m.set_noise(TC.STD, 99, BASE)
        pl.reset(st, ac, sd)
        pl.run(2)
        keep = pl.read_tree(0)
        _refused("rl_mcts_drive", pl, st, ac, sd, 1, 2, 1, 0.0, *drive_out)
        assert same_bits(pl.read_tree(0)["reward"], keep["reward"])
        pl.set_points(None)                                               # the lookahead is needed again
        _refused("rl_mcts_reset", pl, st, ac, sd)
        _refused("rl_mcts_drive", pl, st, ac, sd, 1, 2, 1, 0.0, *drive_out)
    finally:
        pl.close()
        m.set_noise(0.0, 0, 0)


# ---------------------------------------------------------------- 6. the Python façades
def test_the_drop_in_and_the_batched_calls(world):
    """MCTS(..., track_point=p, source="track") pursues p with the velocity reward (with_global=True: the waypoint
    reward), as a planner with set_points does; MCTS(..., track=, rollout="pursuit") and planMCTSMany / driveMCTSMany
    with source="track" run a planner with the track attached."""
    g, c = world["g"], world["wp36"]
    st = c["roots"][0]
    cfg = dict(RC.DEFAULT_CAR)
    cfg.update(scan_dist_to_base=0.275, batch_size=L, scan_beams=B - 1, scan_fov=4.71, scan_std=0.01, scan_max_range=15.0,
               free_thresh=0.8)
    sim = RacecarSimulator(cfg)
    sim.setMap(world["omap"], g.resolution, g.origin)
    sim.setRaytracingMethod("RMGPU")
    sim.setState(st[0])
    p, n = (float(st[0, 0]) + 1.5, float(st[0, 1]) + 0.5), 6
    m = sim.scan_simulator.scan_method
    for with_global, reward in ((False, "velocity"), (True, "waypoint")):
        pl = MCTSPlanner(sim.car, m, 1, n + 1, sim.scan_fov, sim.num_rays, sim.edge_distances, sim.ttc_thresh, source="track",
                         rollout_steps=L, max_steer=sim.max_steer_ang, max_speed=sim.max_speed)
        try:
            pl.set_points(p, reward=reward)
            pl.reset(sim.getState()[None, :], [0.05], [3])
            pl.run(n)
            want = pl.read_tree(0)
        finally:
            pl.close()
        agent = MCTS(sim, None, 0.05, L, n_iterations=n, seed=3, source="track", track_point=p, with_global=with_global)
        agent.mcts()
        MC.assert_tree(agent._planner.read_tree(0), want, with_global)
        assert want["answer"][0] != 0 and want["action"][1] == float(want["answer"][0])
    agent = MCTS(sim, None, 0.05, L, n_iterations=n, seed=3, source="track", track=c["track"], rollout="pursuit",
                 rollout_dev=0.0, goal_span=2, track_window=2)
    assert agent.mcts() is not None and agent._planner.read_track()["goal"][0] >= 0
    a, v, nn = sim.planMCTSMany(st[:3], n, source="track", track=c["track"], track_reward="velocity", rollout="pursuit",
                                rollout_dev=0.1, goal_span=2)
    assert np.isfinite(a).all() and (nn == n + 1).all()
    first, out, rec, acts, vis = sim.driveMCTSMany(st[:3], 2, n, source="track", track=c["track"], rollout="pursuit",
                                                  goal_span=2, track_window=2)
    assert acts.shape == (3, 2) and (first < 0).all() and np.isfinite(acts).all()
