"""Track-guided MCTS on the MI355X (include/scanlib_track_plan.h: rl_car_rollout_track, rl_mcts_attach_track,
rl_mcts_set_points, rl_mcts_read_track; CarBatch.rollout_track, MCTSPlanner.attach_track / set_points / read_track, the
drop-in MCTS with a track point): the terms of plain roll-outs, every node array of every tree and every decision of
the drive bit-identical to the statement (tests/mcts_track_statement.py) fed with the float64 states of the public
roll-out call; the twin without a track; every error of the contract."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import mcts_checks as MC
import mcts_track_checks as TC
import mcts_track_statement as S
import support
import track_statement as TS
from conftest import GOLD, gpu_count
from support import FOV, THRESH, same_bits
from pyracecarsimulator_amd import MCTS, RacecarSimulator, Track, _lib, maps, range_libc
from pyracecarsimulator_amd import racecar as RC
from pyracecarsimulator_amd.mcts import MCTSPlanner, plan_track_args

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

B, EVERY, R = 181, 10, 7
RL_ERR_INVALID = -1
TRI = np.array([(0.0, 1.0), (6.0, 1.0), (3.0, 7.0)])
TRACKS = {"tri3": (TRI, True), "open2": (np.array([(0.0, 0.0), (4.0, 1.0)]), False),
          "ring70": (TC.ring((2.5, 4.5), 4.6, 4.2, 70), True),
          "wp36": (Track.read_csv(os.path.join(GOLD, "wp_u.csv")), True)}


@pytest.fixture(scope="module")
def world():
    g = maps.load_colombia()
    omap = range_libc.PyOMap(g)
    return {"g": g, "omap": omap, "dt": omap.distance_transform(), "m": range_libc.PyRayMarchingGPU(omap, 300),
            "cars": RC.CarBatch(), "fg": support.followgap()}


def at_arc(T, s, side=0.0):
    """(x, y, heading of the segment) at arc length s of the table T, `side` m to the left."""
    i = int(min(np.searchsorted(T["cum"], s, "right") - 1, T["S"] - 1))
    t = (s - T["cum"][i]) / T["len"][i]
    ux, uy = T["dx"][i] / T["len"][i], T["dy"][i] / T["len"][i]
    return T["x"][i] + t * T["dx"][i] - side * uy, T["y"][i] + t * T["dy"][i] + side * ux, math.atan2(uy, ux)


def cars_on(T, n, L, seed):
    """(states (n, 11), actions (n, n_act, 2)): cars spread along the track, up to 0.4 m beside it, heading within
    0.3 rad of it, the last one a few metres off the track."""
    rng = np.random.default_rng(seed)
    st = np.zeros((n, 11))
    for e in range(n):
        st[e, :3] = at_arc(T, T["L"] * (e + 0.37) / n, rng.uniform(-0.4, 0.4))
        st[e, 2] += rng.uniform(-0.3, 0.3)
        st[e, 3] = rng.uniform(1.0, 3.0)
    st[n - 1, :2] += (3.0, -2.5)
    n_act = (L + EVERY - 1) // EVERY
    act = np.stack([rng.uniform(1.0, 6.0, (n, n_act)), rng.uniform(-0.4, 0.4, (n, n_act))], -1)
    return st, act


# ---------------------------------------------------------------- 1. rollout_track against the statement
@pytest.mark.parametrize("L", [5, 24, 136])
@pytest.mark.parametrize("name", sorted(TRACKS))
def test_rollout_track_equals_the_statement(world, name, L):
    """R = 7 roll-outs of L steps (the reward sum's three forms) on a closed triangle, an open 2-point track (S = 1), a
    closed 70-point ellipse (a second, partial lane pass) and the waypoint file; progress with window 0 and 3, anchors
    given (one segment on from the nearest) and searched; the waypoint reward with the goal rule at the start
    (goal_span 0 and 5) and with given points: terms, s, segment and start_s bit-equal."""
    cars = world["cars"]
    xy, closed = TRACKS[name]
    T, trk = TS.build(xy, closed), Track(xy, closed)
    st, act = cars_on(T, R, L, 11 + L)
    steps = TC.step_states(cars, st, act, L, EVERY)
    pos, vel = steps[:, :, :2], steps[:, :, 3]
    near = np.array([TS.nearest(T, st[r, 0], st[r, 1]) for r in range(R)], np.int32)
    for window in (0, 3):
        for anchors in (None, (near + 1) % T["S"]):
            got = cars.rollout_track(trk, st, act, "progress", window=window, anchors=anchors, n_steps=L, action_every=EVERY)
            for r in range(R):
                want = S.progress_terms(T, int(near[r] if anchors is None else anchors[r]), window, st[r, :2], pos[r])
                what = (name, L, window, anchors is None, r)
                assert same_bits(got["terms"][r], want[0]), (what, got["terms"][r], want[0])
                assert same_bits(got["s"][r], want[1]) and same_bits(got["segment"][r], want[2]), what
                assert same_bits(got["start_s"][r:r + 1], np.array([want[3]])), what
    rng = np.random.default_rng(5)
    given = st[:, :2] + rng.uniform(-2.0, 2.0, (R, 2))
    n_goal = 0
    for span, points in ((0, None), (5, None), (0, given)):
        got = cars.rollout_track(trk, st, act, "waypoint", lookahead=1.5, goal_span=span, points=points, n_steps=L,
                                 action_every=EVERY)
        assert set(got) == {"terms"}
        for r in range(R):
            rt = S.root(T, st[r, 0], st[r, 1], 1.5, span, None if points is None else points[r])
            n_goal += int(rt["goal"] >= 0)
            want = S.terms(T, S.WAYPOINT, 0, rt, st[r, :2], pos[r], vel[r])
            assert same_bits(got["terms"][r], want), (name, L, span, points is None, r)
    assert n_goal >= 2 * (R - 1), n_goal                        # (the car off the track may see no waypoint)
    got = cars.rollout_track(None, st, act, "velocity", n_steps=L, action_every=EVERY)
    assert same_bits(got["terms"], vel)


def test_a_duplicated_point_is_refused_at_the_track():
    """The section's rule for a degenerate segment (q = 0) is refusal at rl_track_create, so no search ever meets
    one: the 70-point ellipse with one point doubled does not become a track."""
    xy = np.insert(TRACKS["ring70"][0], 30, TRACKS["ring70"][0][30], axis=0)
    assert xy.shape == (71, 2)
    with pytest.raises(ValueError):
        Track(xy, True)
    h = C.c_void_p()
    with pytest.raises(_lib.ScanLibError) as e:
        _lib.call("rl_track_create", 0, np.ascontiguousarray(xy), 71, 1, h)
    assert e.value.code == RL_ERR_INVALID and not h.value


# ---------------------------------------------------------------- 2. wrap and ties
@pytest.mark.parametrize("name", ["tri3", "ring70", "wp36"])
def test_progress_across_the_start_line(world, name):
    """Starts one step short of s = 0 on the closed tracks, on the track and heading along it, forwards and (with a
    negative speed) backwards: the raw difference of arc lengths jumps by the track's length where the car crosses,
    the terms stay small and of the car's direction, bit-equal to the statement."""
    cars = world["cars"]
    xy, closed = TRACKS[name]
    T, trk = TS.build(xy, closed), Track(xy, closed)
    L, v = 5, 3.0
    st = np.zeros((2, 11))
    st[0, :3] = at_arc(T, T["L"] - 0.04)
    st[1, :3] = at_arc(T, 0.04)
    st[:, 3] = (v, -v)
    act = np.array([[[v, 0.0]], [[-v, 0.0]]])
    steps = TC.step_states(cars, st, act, L, EVERY)
    got = cars.rollout_track(trk, st, act, "progress", n_steps=L, action_every=EVERY)
    for r, sign in ((0, 1.0), (1, -1.0)):
        near = TS.nearest(T, st[r, 0], st[r, 1])
        terms, s, seg, s0 = S.progress_terms(T, near, 0, st[r, :2], steps[r, :, :2])
        raw = np.diff(np.concatenate([[s0], s]))
        assert (sign * raw < -0.5 * T["L"]).any(), (name, r, raw)           # the car crossed s = 0
        assert same_bits(got["terms"][r], terms) and same_bits(got["s"][r], s), (name, r)
        assert (sign * terms >= 0).all() and sign * terms.sum() > 0.02 and (np.abs(terms) < 0.1).all(), (name, r, terms)


def test_a_tie_between_two_segments_takes_the_lower_index(world):
    """On the outer bisector of a vertex both segments clamp to the vertex and d2 is equal to the bit: at vertex 1 of
    the triangle segment 0 wins over 1; at vertex 0 segment 0 wins over 2, so s reads 0 and not the track's length.
    The cars stand still (speed 0), so every step repeats the tie."""
    cars = world["cars"]
    T, trk = TS.build(TRI, True), Track(TRI, True)
    assert TS.project(T, 0, 6.5, 0.5)[0] == TS.project(T, 1, 6.5, 0.5)[0] == 0.5
    assert TS.project(T, 0, -0.5, 0.5)[0] == TS.project(T, 2, -0.5, 0.5)[0] == 0.5
    st = np.zeros((2, 11))
    st[0, :2], st[1, :2] = (6.5, 0.5), (-0.5, 0.5)
    act = np.zeros((2, 1, 2))
    for window in (0, 1):
        got = cars.rollout_track(trk, st, act, "progress", window=window, n_steps=5, action_every=EVERY)
        assert (got["segment"] == 0).all(), got["segment"]
        assert got["start_s"].tolist() == [6.0, 0.0] and (got["s"][0] == 6.0).all() and (got["s"][1] == 0.0).all()
        assert (got["terms"] == 0.0).all()


# ---------------------------------------------------------------- 3. whole trees against the statement
K_TREES, I_TREES, L_TREES, BASE = 9, 12, 24, 777


@pytest.fixture(scope="module")
def tree_case(world):
    """The K = 9 roots (past one mcts_act workgroup of 8 trees), a 70-point ring around them, and the trees of a
    planner that never saw a track, per source."""
    states, actions, seeds = MC.roots(world["g"], world["dt"], K_TREES, 31)
    xy = TC.ring_around(states)
    plain = {}
    for source in ("random", "fg"):
        h = world["fg"] if source == "fg" else None
        pl, trees, best = MC.device(world["cars"], world["m"], TC.STD, BASE, source, h, states, actions, seeds, I_TREES,
                                    num_rays=B, rollout_steps=L_TREES, action_every=EVERY)
        pl.close()
        plain[source] = (trees, best)
    return dict(states=states, actions=actions, seeds=seeds, xy=xy, T=TS.build(xy, True), track=Track(xy, True),
                plain=plain)


def run_both(world, case, source, reward, I, L, *, K=None, lookahead=3.0, window=0, goal_span=0, points=None, track=True):
    K = K or len(case["states"])
    h = world["fg"] if source == "fg" else None
    st, ac, sd = case["states"][:K], case["actions"][:K], case["seeds"][:K]
    kw = dict(lookahead=lookahead, window=window, goal_span=goal_span, points=points, num_rays=B, rollout_steps=L,
              action_every=EVERY)
    pl, dev, best = TC.device(world["cars"], world["m"], BASE, source, h, st, ac, sd, I, case["track"] if track else None,
                              reward, **kw)
    try:
        trees, want, rts, log = TC.replay(world["cars"], world["m"], BASE, source, h, st, ac, sd, I, dev,
                                          case["T"] if track else None, reward, **kw)
        for k in range(K):
            MC.assert_tree(dev[k], want[k], (source, reward, window, k))
            a, v = trees[k].best()
            assert best[0][k] == a and best[1][k] == v, (source, reward, k)
        TC.assert_roots(pl.read_track(), rts, (source, reward, window))
    finally:
        pl.close()
        world["m"].set_noise(0.0, 0, 0)
    return dev, trees, rts, log


@pytest.mark.parametrize("window", [0, 3])
@pytest.mark.parametrize("reward", ["waypoint", "progress"])
@pytest.mark.parametrize("source", ["random", "fg"])
def test_trees_equal_the_statement(world, tree_case, source, reward, window):
    """K = 9, I = 12, L = 24, 181 beams, noise 0.01: every node array of every tree equals the statement replayed with
    the public calls and answered with the statement's terms; read_track gives the statement's roots.  Among the
    roll-outs some crashed mid-way, some did not, and some children were terminal.  The progress trees differ from the
    trees of the same seeds without a track."""
    dev, trees, rts, log = run_both(world, tree_case, source, reward, I_TREES, L_TREES, window=window, goal_span=window)
    mid, none, term = TC.conditions(trees, log, L_TREES)
    print("roll-outs crashed mid-way %d, not crashed %d, terminal children %d; goals %s" %
          (mid, none, term, [rt["goal"] for rt in rts]))
    assert mid >= 1 and none >= 1 and term >= 1, (mid, none, term)
    plain = tree_case["plain"][source][0]
    if reward == "waypoint":
        assert sum(rt["goal"] >= 0 for rt in rts) >= 1
    differs = [not same_bits(dev[k]["reward"], plain[k]["reward"]) for k in range(K_TREES)]
    assert any(differs) if reward == "waypoint" else sum(differs) >= K_TREES - 2, differs


def test_trees_with_a_split_reward_sum(world, tree_case):
    """L = 136 (the pairwise sum splits above 128), K = 2, I = 3, progress with a window."""
    run_both(world, tree_case, "random", "progress", 3, 136, K=2, window=3)


# ---------------------------------------------------------------- 4. the twin, no goal
def test_velocity_mode_and_a_detached_track_change_nothing(world, tree_case):
    """A planner with mode 0 attached, and one that attached a progress track and detached it again, give the trees
    and best() of a planner that never saw a track."""
    c, m = tree_case, world["m"]
    plain, best = c["plain"]["random"]
    for detach in (False, True):
        m.set_noise(TC.STD, 99, BASE)
        pl = MC.planner(world["cars"], m, K_TREES, I_TREES, "random", None, num_rays=B, rollout_steps=L_TREES,
                        action_every=EVERY)
        try:
            pl.attach_track(c["track"], "progress" if detach else "velocity", window=3)
            if detach:
                pl.detach_track()
            pl.reset(c["states"], c["actions"], c["seeds"])
            pl.run(I_TREES)
            for k in range(K_TREES):
                MC.assert_tree(pl.read_tree(k), plain[k], ("twin", detach, k))
            for got, want in zip(pl.best(), best):
                assert same_bits(got, want), ("twin", detach)
            if not detach:
                TC.assert_roots(pl.read_track(), TC.statement_roots(c["T"], c["states"], 1.5, 0), "twin")
        finally:
            pl.close()
            m.set_noise(0.0, 0, 0)


def test_without_a_goal_the_waypoint_reward_is_the_velocity(world, tree_case):
    """A lookahead so small that no waypoint lies within twice of it: goal -1 for every tree, and the waypoint trees
    equal the trees without a track."""
    c = tree_case
    pl, dev, best = TC.device(world["cars"], world["m"], BASE, "random", None, c["states"], c["actions"], c["seeds"],
                              I_TREES, c["track"], "waypoint", lookahead=1e-3, num_rays=B, rollout_steps=L_TREES,
                              action_every=EVERY)
    try:
        rt = pl.read_track()
        assert (rt["goal"] == -1).all() and (rt["point"] == 0.0).all() and (rt["segment"] >= 0).all()
        for k in range(K_TREES):
            MC.assert_tree(dev[k], c["plain"]["random"][0][k], ("no goal", k))
    finally:
        pl.close()
        world["m"].set_noise(0.0, 0, 0)


# ---------------------------------------------------------------- 5. the drive
@pytest.mark.parametrize("reward", ["waypoint", "progress"])
def test_drive_equals_the_host_composed_loop(world, tree_case, reward):
    """K = 5, D = 3, I = 6, S = 2, L = 16: drive on a planner with the track equals reset / run / best composed on the
    host on a second planner with the same track; read_track gives the last decision's roots; the handle's option and
    noise offset read as before the call."""
    cars, m, c = world["cars"], world["m"], tree_case
    K, D, I, S_, L = 5, 3, 6, 2, 16
    st, rec, sd = c["states"][:K], c["actions"][:K], c["seeds"][:K]
    shape = dict(num_rays=B, rollout_steps=L, action_every=EVERY)
    host_pl, dev_pl = MC.planner(cars, m, K, I, "random", None, **shape), MC.planner(cars, m, K, I, "random", None, **shape)
    try:
        for pl in (host_pl, dev_pl):
            pl.attach_track(c["track"], reward, lookahead=3.0, window=3, goal_span=3)
        want = MC.host_loop(cars, m, host_pl, TC.STD, BASE, st, rec, sd, D, I, S_, MC.CLIP, num_rays=B, rollout_steps=L)
        m.set_noise(TC.STD, 99, BASE)
        probe = st[:2, :3].astype(np.float32)
        before, nt = MC.scan_keep(m, probe, B), m.get_info("nt_store")
        got = dev_pl.drive(st, rec, sd, D, I, steps_per_decision=S_, steer_clip=MC.CLIP, trace=True)
        MC.assert_drive(got, want, reward)
        for k in range(K):
            MC.assert_tree(dev_pl.read_tree(k), host_pl.read_tree(k), (reward, k))
        last = np.where(np.isnan(got[5][:, D - 1]), got[1], got[5][:, D - 1])     # (a frozen car is planned from where it froze)
        rts = TC.statement_roots(c["T"], last, 3.0, 3)
        TC.assert_roots(dev_pl.read_track(), rts, reward)
        TC.assert_roots(host_pl.read_track(), rts, reward)
        assert m.get_info("nt_store") == nt and same_bits(MC.scan_keep(m, probe, B), before)
        # the trees of the drive are not those of a drive without the track
        plain = MC.planner(cars, m, K, I, "random", None, **shape)
        try:
            m.set_noise(TC.STD, 99, BASE)
            plain.drive(st, rec, sd, D, I, steps_per_decision=S_, steer_clip=MC.CLIP)
            assert any(not same_bits(plain.read_tree(k)["reward"], dev_pl.read_tree(k)["reward"]) for k in range(K))
        finally:
            plain.close()
    finally:
        host_pl.close()
        dev_pl.close()
        m.set_noise(0.0, 0, 0)


# ---------------------------------------------------------------- 6. explicit points
def test_explicit_points_and_the_drop_in(world, tree_case):
    """Trees with explicit points and no track equal the statement's waypoint trees; the drop-in MCTS with
    with_global=True and a track_point gives the tree of a planner with set_points, with_global=False today's tree;
    drive with explicit points is refused."""
    c = tree_case
    pts = c["states"][:, :2] + np.random.default_rng(9).uniform(-3.0, 3.0, (K_TREES, 2))
    dev, _, rts, _ = run_both(world, c, "random", "waypoint", 6, L_TREES, points=pts, track=False)
    assert all(rt["segment"] == -1 and rt["goal"] == -1 and rt["has"] for rt in rts)
    assert any(not same_bits(dev[k]["reward"][:7], c["plain"]["random"][0][k]["reward"][:7]) for k in range(K_TREES))

    g = world["g"]
    cfg = dict(RC.DEFAULT_CAR)
    cfg.update(scan_dist_to_base=0.275, batch_size=200, scan_beams=1080, scan_fov=4.71, scan_std=0.01,
               scan_max_range=15.0, free_thresh=0.8)
    sim = RacecarSimulator(cfg)
    sim.setMap(world["omap"], g.resolution, g.origin)
    sim.setRaytracingMethod("RMGPU")
    sim.setState(c["states"][0])
    p, n = (float(pts[0, 0]), float(pts[0, 1])), 8
    m = sim.scan_simulator.scan_method
    trees = {}
    for name, points in (("points", p), ("plain", None)):
        pl = MCTSPlanner(sim.car, m, 1, n + 1, sim.scan_fov, sim.num_rays, sim.edge_distances, sim.ttc_thresh,
                         source="random", rollout_steps=L_TREES, max_steer=sim.max_steer_ang, max_speed=sim.max_speed)
        try:
            pl.set_points(points)
            pl.reset(sim.getState()[None, :], [0.05], [3])
            pl.run(n)
            trees[name] = pl.read_tree(0)
            if points is not None:
                assert pl.read_track()["point"].tolist() == [list(p)]
                with pytest.raises(ValueError):
                    pl.drive(c["states"][:1], 0.0, [3], 1, 2)
                st1, out1 = np.ascontiguousarray(c["states"][:1]), np.empty((1, 11))
                with pytest.raises(_lib.ScanLibError) as e:
                    _lib.call("rl_mcts_drive", pl, st1, np.zeros(1), np.array([3], np.uint64), 1, 2, 1, 0.0,
                              np.empty(1, np.int32), out1, np.empty(1), np.empty((1, 1)), np.empty((1, 1), np.int32), None)
                assert e.value.code == RL_ERR_INVALID
                assert same_bits(pl.read_tree(0)["reward"], trees[name]["reward"])      # (the planner is as it was)
        finally:
            pl.close()
    assert not same_bits(trees["points"]["reward"], trees["plain"]["reward"])
    for name, kw in (("points", dict(with_global=True, track_point=p)), ("plain", dict(with_global=False, track_point=p))):
        agent = MCTS(sim, None, 0.05, L_TREES, n_iterations=n, seed=3, source="random", **kw)
        agent.mcts()
        arr = agent._planner.read_tree(0)
        MC.assert_tree(arr, trees[name], name)
        assert agent.root.reward == 0.0 and len(agent.root.children) == arr["n_children"][0]
    with pytest.raises(ValueError):
        MCTS(sim, None, 0.05, L_TREES, with_global=True)


# ---------------------------------------------------------------- 7. every error of the contract
def test_errors_leave_the_handles_usable(world, tree_case):
    cars, m, c = world["cars"], world["m"], tree_case
    K, I, L = 3, 3, 8
    st, ac, sd = c["states"][:K], c["actions"][:K], c["seeds"][:K]
    trk = c["track"]

    def refused(name, *args):
        with pytest.raises(_lib.ScanLibError) as e:
            _lib.call(name, *args)
        assert e.value.code == RL_ERR_INVALID, (name, str(e.value))

    def params(mode=2, window=0, span=0, la=1.5):
        p = _lib.PlanTrackParams()
        p.reward_mode, p.window, p.goal_span, p.lookahead = mode, window, span, la
        return p

    pl = MC.planner(cars, m, K, I, "random", None, num_rays=B, rollout_steps=L, action_every=EVERY)
    try:
        m.set_noise(TC.STD, 99, BASE)
        pl.attach_track(trk, "progress", window=3)
        pl.reset(st, ac, sd)
        pl.run(I)
        want = [pl.read_tree(k) for k in range(K)]
        roots = pl.read_track()
        # attach: null params, the mode, the window and the span, the lookahead of the waypoint reward
        refused("rl_mcts_attach_track", pl, trk, None)
        for bad in (params(mode=3), params(mode=-1), params(window=-1), params(window=65537), params(span=-1),
                    params(span=65537), params(mode=1, la=0.0), params(mode=1, la=-1.0), params(mode=1, la=math.nan),
                    params(mode=1, la=math.inf)):
            refused("rl_mcts_attach_track", pl, trk, bad)
        if gpu_count() > 1:
            other = Track(c["xy"], True, device=1)
            refused("rl_mcts_attach_track", pl, other, params())
            refused("rl_car_rollout_track", cars, other, params(), st, np.zeros((K, 1, 2)), K, L, EVERY, 0.01, None, None,
                    np.empty((K, L)), None, None, None)
        # none of it touched the planner: the same trees, the same roots, and it runs on
        for k in range(K):
            MC.assert_tree(pl.read_tree(k), want[k], ("after refusals", k))
        assert same_bits(pl.read_track()["s"], roots["s"])
        # read_track: before a reset, and without a track or points
        pl.attach_track(trk, "waypoint", lookahead=2.0)
        refused("rl_mcts_read_track", pl, np.empty(K, np.int32), np.empty(K), np.empty(K, np.int32), np.empty((K, 2)))
        refused("rl_mcts_run", pl, 1)                                         # (attaching asks for a reset)
        pl.detach_track()
        pl.reset(st, ac, sd)
        refused("rl_mcts_read_track", pl, np.empty(K, np.int32), np.empty(K), np.empty(K, np.int32), np.empty((K, 2)))
        # a waypoint track whose lookahead only explicit points excuse: refused at the reset once they are gone
        pl.set_points(st[:, :2] + 1.0)
        _lib.call("rl_mcts_attach_track", pl, trk, params(mode=1, la=0.0))
        pl.reset(st, ac, sd)
        pl.run(1)
        refused("rl_mcts_drive", pl, st, ac, sd, 1, 2, 1, 0.0, np.empty(K, np.int32), np.empty((K, 11)), np.empty(K),
                np.empty((K, 1)), np.empty((K, 1), np.int32), None)
        keep = pl.read_tree(0)
        pl.set_points(None)
        refused("rl_mcts_reset", pl, st, ac, sd)
        refused("rl_mcts_drive", pl, st, ac, sd, 1, 2, 1, 0.0, np.empty(K, np.int32), np.empty((K, 11)), np.empty(K),
                np.empty((K, 1)), np.empty((K, 1), np.int32), None)
        pl.attach_track(trk, "progress", window=3)
        pl.reset(st, ac, sd)
        pl.run(I)
        for k in range(K):
            MC.assert_tree(pl.read_tree(k), want[k], ("usable", k))
        assert len(keep["parent"]) == 2
    finally:
        pl.close()
        m.set_noise(0.0, 0, 0)
    # the roll-outs
    act = np.zeros((K, 1, 2))
    out = (np.empty((K, L)), None, None, None)
    refused("rl_car_rollout_track", cars, trk, None, st, act, K, L, EVERY, 0.01, None, None, *out)
    refused("rl_car_rollout_track", cars, None, params(mode=2), st, act, K, L, EVERY, 0.01, None, None, *out)
    refused("rl_car_rollout_track", cars, None, params(mode=1), st, act, K, L, EVERY, 0.01, None, None, *out)
    refused("rl_car_rollout_track", cars, trk, params(mode=1, la=0.0), st, act, K, L, EVERY, 0.01, None, None, *out)
    refused("rl_car_rollout_track", cars, trk, params(mode=4), st, act, K, L, EVERY, 0.01, None, None, *out)
    refused("rl_car_rollout_track", cars, trk, params(window=-2), st, act, K, L, EVERY, 0.01, None, None, *out)
    for bad in (-1, trk.n_segments):
        refused("rl_car_rollout_track", cars, trk, params(), st, act, K, L, EVERY, 0.01, np.array([0, bad, 0], np.int32),
                None, *out)
    big = np.zeros((K, 52, 2))
    refused("rl_car_rollout_track", cars, trk, params(), st, big, K, 513, EVERY, 0.01, None, None, np.empty((K, 513)), None,
            None, None)
    refused("rl_car_rollout_track", cars, trk, params(), st, act, K, 0, EVERY, 0.01, None, None, *out)
    # mode 1 with points needs neither a track nor a lookahead, and the car handle works on
    _lib.call("rl_car_rollout_track", cars, None, params(mode=1, la=0.0), st, act, K, L, EVERY, 0.01, None,
              np.ascontiguousarray(st[:, :2] + 1.0), *out)
    got = cars.rollout_track(trk, st, act, "progress", n_steps=L, action_every=EVERY)
    assert np.isfinite(got["terms"]).all()
    with pytest.raises(ValueError):
        cars.rollout_track(None, st, act, "progress", n_steps=L, action_every=EVERY)
    with pytest.raises(ValueError):
        cars.rollout_track(trk, st, act, "progress", anchors=[0, 70, 0], n_steps=L, action_every=EVERY)
    assert plan_track_args("waypoint", lookahead=0.0, points=True).reward_mode == 1
