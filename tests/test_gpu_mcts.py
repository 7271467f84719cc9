"""The MCTS planner on the MI355X (rl_mcts_*, mcts.MCTSPlanner, mcts.MCTS, CarBatch.plan_mcts,
RacecarSimulator.planMCTSMany): every act link against the public calls and the reference's compiled Car, every node
array of every tree bit-identical to the statement (tests/mcts_statement.py) replayed with the public calls,
chunking and batching invariance, errors, the façade, and the device UCB against Python's."""
import ctypes as C
import math
import os
import time

import numpy as np
import pytest

from conftest import GOLD
import policy_statement as PS
import support
from mcts_checks import B, EVERY, L, MAX_SPEED, SPEED, answers, assert_tree, device, replay, roots, scan
from oracle import reference
from support import D_BASE, FOV, MAX_STEER, THRESH, same_bits, within_one_ulp
from pyracecarsimulator_amd import MCTS, Policy, RacecarSimulator, _lib, maps, range_libc
from pyracecarsimulator_amd import racecar as RC
from pyracecarsimulator_amd.mcts import MCTSPlanner

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]


@pytest.fixture(scope="module")
def handles():
    layers, relu = PS.load_fixture(os.path.join(GOLD, "policy_mlp720.npz"))
    return {"fg": support.followgap(), "nn": Policy.from_arrays(layers, relu), "random": None}


# ---------------------------------------------------------------- 1. the act links
@pytest.mark.parametrize("source", ["fg", "nn"])
def test_act_links_against_public_calls_and_reference(handles, source):
    reference.require()
    g = maps.load_colombia()
    omap = range_libc.PyOMap(g)
    dt = omap.distance_transform()
    m = range_libc.PyRayMarchingGPU(omap, 300)
    h = handles[source]
    cars = RC.CarBatch()
    K, n_it, std, base = 6, 24, 0.05, 777
    states, actions, seeds = roots(g, dt, K, 31)
    pl, trees, _ = device(cars, m, std, base, source, h, states, actions, seeds, n_it)
    assert m.get_info("nt_store") == 1
    edge = support.edge(B)
    ref = reference.RefCar()
    n_term = 0
    try:
        for k in range(K):
            t = trees[k]
            assert len(t["parent"]) == n_it + 1 and same_bits(t["state"][0], states[k])
            for c in range(n_it + 1):
                st = t["state"][c]
                assert within_one_ulp(support.lidar_poses(st), t["scan_pose"][c]), (k, c)
                off = base + (k * B if c == 0 else (K + (c - 1) * K * (1 + L) + k) * B)
                ranges = scan(m, std, off, t["scan_pose"][c][None, :])
                assert same_bits(answers(source, h, ranges), t["answer"][c:c + 1]), (k, c)
                crashed = RC.is_crashed(ranges[0], B, 1, edge, THRESH) >= 0
                assert t["terminal"][c] == (int(crashed) if c > 0 else 0), (k, c)
                n_term += int(t["terminal"][c])
                if c == 0:
                    continue
                par = t["parent"][c]
                _, out, _ = cars.rollout(t["state"][par][None, :], np.array([[[SPEED, t["action"][c]]]]), n_steps=1,
                                         action_every=1)
                assert same_bits(out[0], st), (k, c)
                assert np.allclose(st, ref.step(t["state"][par], SPEED, t["action"][c]), rtol=1e-9, atol=1e-9), (k, c)
    finally:
        ref.close()
        m.set_noise(0.0, 0, 0)
    assert n_term >= 0


# ---------------------------------------------------------------- 2. whole trees against the statement
def _method_factories(omap, mrx):
    return [("RM", lambda: range_libc.PyRayMarching(omap, mrx), 0.0),
            ("RMGPU", lambda: range_libc.PyRayMarchingGPU(omap, mrx), 0.05),
            ("CDDT", lambda: range_libc.PyCDDTCast(omap, mrx, 112), 0.0),
            ("Bresenham", lambda: range_libc.PyBresenhamsLine(omap, mrx), 0.0),
            ("GiantLUT", lambda: range_libc.PyGiantLUTCast(omap, mrx, 112), 0.0)]


@pytest.fixture(scope="module")
def maze():
    g = maps.make_maze(256, cell=40, wall=3, p=0.45, seed=11)
    omap = range_libc.PyOMap(g)
    return g, omap, omap.distance_transform()


@pytest.mark.parametrize("method", ["RM", "RMGPU", "CDDT", "Bresenham", "GiantLUT"])
@pytest.mark.parametrize("source", ["fg", "nn", "random"])
def test_whole_trees_equal_statement(handles, maze, method, source):
    g, omap, dt = maze
    name, make, std = [x for x in _method_factories(omap, 300) if x[0] == method][0]
    m = make()
    h = handles[source]
    cars = RC.CarBatch()
    base = 4242
    n_term = 0
    for K in (1, 7, 64):
        states, actions, seeds = roots(g, dt, K, 100 + K)
        _, trees37, best37 = device(cars, m, std, base, source, h, states, actions, seeds, 37)
        stmt, snaps = replay(cars, m, std, base, source, h, states, actions, seeds, 37, trees37, (1, 2, 37))
        for n in (1, 2, 37):
            if n == 37:
                trees, best = trees37, best37
            else:
                _, trees, best = device(cars, m, std, base, source, h, states, actions, seeds, n)
            for k in range(K):
                assert_tree(trees[k], snaps[n][k], (name, source, K, n, k))
            if n == 37:
                for k in range(K):
                    a, v = stmt[k].best()
                    assert best[1][k] == v and same_bits(best[0][k:k + 1], np.array([a])), (K, k)
                    assert best[2][k] == 38
        for k in range(K):
            t = snaps[37][k]
            n_term += int(t["terminal"].sum())
    m.set_noise(0.0, 0, 0)
    assert n_term > 0, "no terminal child in the grid"
    assert m.get_info("nt_store") == 1


# ---------------------------------------------------------------- 3. invariance
def test_chunking_and_batching_invariance(handles, maze):
    g, omap, dt = maze
    cars = RC.CarBatch()
    m = range_libc.PyRayMarchingGPU(omap, 300)
    h = handles["fg"]
    K, n = 16, 30
    states, actions, seeds = roots(g, dt, K, 7)
    m.set_noise(0.05, 99, 555)
    pl = MCTSPlanner(cars, m, K, n + 1, FOV, B, support.edge(B), THRESH, source="fg", followgap=h)
    pl.reset(states, actions, seeds)
    pl.run(n)
    whole = [pl.read_tree(k) for k in range(K)]
    pl.reset(states, actions, seeds)
    pl.run(n // 2)
    pl.run(0)
    pl.run(n - n // 2)
    for k in range(K):
        assert_tree(pl.read_tree(k), whole[k], ("chunked", k))
    # tree k alone with seeds[k] == tree k in the batch (noise off: the ray ids depend on K)
    m.set_noise(0.0, 0, 0)
    _, batch, _ = device(cars, m, 0.0, 0, "fg", h, states, actions, seeds, n)
    for k in (0, 5, 15):
        _, alone, _ = device(cars, m, 0.0, 0, "fg", h, states[k:k + 1], actions[k:k + 1], seeds[k:k + 1], n)
        assert_tree(alone[0], batch[k], ("alone", k))


# ---------------------------------------------------------------- 4. errors
def test_errors_leave_handles_usable(handles, maze):
    g, omap, dt = maze
    cars = RC.CarBatch()
    m = range_libc.PyRayMarchingGPU(omap, 300)
    fg, pol = handles["fg"], handles["nn"]
    K = 4
    states, actions, seeds = roots(g, dt, K, 9)
    m.set_noise(0.05, 7, 321)
    poses = maps.sample_free_poses(g, 8, 3, 4.0, dt)
    scan0 = np.empty(8 * B, np.float32)
    m.calc_range_fan(poses, scan0, FOV, B)
    _, want, _ = device(cars, m, 0.05, 321, "fg", fg, states, actions, seeds, 3)
    m.set_noise(0.05, 7, 321)

    def still_usable():
        again = np.empty_like(scan0)
        m.calc_range_fan(poses, again, FOV, B)
        assert same_bits(again, scan0)
        assert m.get_info("nt_store") == 1
        _, got, _ = device(cars, m, 0.05, 321, "fg", fg, states, actions, seeds, 3)
        for k in range(K):
            assert_tree(got[k], want[k], k)
        m.set_noise(0.05, 7, 321)

    Lb = _lib.lib()
    edge = support.edge(B)

    def params(**kw):
        p = _lib.MctsParams()
        vals = dict(n_trees=K, max_nodes=8, rollout_steps=L, action_every=EVERY, source=_lib.RL_MCTS_FG, speed=SPEED,
                    dt=0.01, scan_dist_to_base=D_BASE, C=0.5, crash_pen=-10.0, uni_dev=0.05, max_steer=MAX_STEER,
                    max_speed=MAX_SPEED, fov=FOV, num_rays=B, crash_thresh=THRESH)
        vals.update(kw)
        for k, v in vals.items():
            setattr(p, k, v)
        return p

    def create(p, car=cars._h, meth=m._h, g_=fg._h, pol_=None, ed=edge):
        out = C.c_void_p()
        rc = Lb.rl_mcts_create(car, meth, g_, pol_, C.byref(p) if p is not None else None,
                               ed.ctypes.data_as(_lib.f64p) if ed is not None else None, C.byref(out))
        return rc, out

    def expect_error(rc):
        assert rc == -1, rc
        still_usable()

    expect_error(create(params(), car=None)[0])
    expect_error(create(None)[0])
    expect_error(create(params(), ed=None)[0])
    expect_error(create(params(), g_=None)[0])                                    # FG without its handle
    expect_error(create(params(source=_lib.RL_MCTS_NN))[0])                       # NN without its handle
    expect_error(create(params(source=7))[0])
    for nr in (9, 1281):
        expect_error(create(params(num_rays=nr), ed=support.edge(nr))[0])
    expect_error(create(params(source=_lib.RL_MCTS_NN, num_rays=899), pol_=pol._h, ed=support.edge(899))[0])  # window [180, 900)
    for bad in (dict(n_trees=0), dict(max_nodes=0), dict(rollout_steps=0), dict(rollout_steps=513),
                dict(action_every=0)):
        expect_error(create(params(**bad))[0])
    # capacity, checked before any launch; the planner stays usable
    pl = MCTSPlanner(cars, m, K, 4, FOV, B, edge, THRESH, source="fg", followgap=fg)
    with pytest.raises(_lib.ScanLibError, match="reset"):
        pl.run(1)
    pl.reset(states, actions, seeds)
    pl.run(2)
    before = [pl.read_tree(k) for k in range(K)]
    with pytest.raises(_lib.ScanLibError, match="max_nodes"):
        pl.run(2)
    for k in range(K):
        assert_tree(pl.read_tree(k), before[k], k)
    pl.run(1)
    assert (pl.best()[2] == 4).all()
    assert Lb.rl_mcts_run(None, 1) == -1 and Lb.rl_mcts_reset(pl._h, None, None, None) == -1
    assert Lb.rl_mcts_read_tree(pl._h, K, *([None] * 13), C.byref(C.c_int())) == -1
    still_usable()
    # a range method rl_car_rollout_check refuses (fov NaN) is refused with the same code
    pl2 = MCTSPlanner(cars, m, K, 8, float("nan"), B, edge, THRESH, source="fg", followgap=fg)
    want_rc = Lb.rl_car_rollout_check(cars._h, m._h, states.ctypes.data_as(_lib.f64p),
                                      np.zeros((K, 20, 2)).ctypes.data_as(_lib.f64p), K, L, EVERY, 0.01,
                                      float("nan"), B, edge.ctypes.data_as(_lib.f64p), THRESH,
                                      np.zeros(K, np.int32).ctypes.data_as(C.POINTER(C.c_int)), None, None)
    assert want_rc != 0
    assert Lb.rl_mcts_run(pl2._h, 1) == -1                                        # not reset yet
    s64 = seeds.astype(np.uint64)
    rc = Lb.rl_mcts_reset(pl2._h, states.ctypes.data_as(_lib.f64p), actions.ctypes.data_as(_lib.f64p),
                          s64.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert rc == want_rc
    still_usable()
    # multi-device handles: refused
    multi = RC.CarBatch(device=[0])
    with pytest.raises(_lib.ScanLibError, match="single-device"):
        MCTSPlanner(multi, m, K, 8, FOV, B, edge, THRESH, source="fg", followgap=fg)
    still_usable()
    if Lb.rl_device_count() >= 2:
        fg1 = support.followgap(device=1)
        with pytest.raises(_lib.ScanLibError, match="device"):
            MCTSPlanner(cars, m, K, 8, FOV, B, edge, THRESH, source="fg", followgap=fg1)
        still_usable()
    m.set_noise(0.0, 0, 0)


# ---------------------------------------------------------------- 5. façade
def _sim():
    g = maps.load_colombia()
    cfg = dict(RC.DEFAULT_CAR)
    cfg.update(scan_dist_to_base=0.275, batch_size=200, scan_beams=1080, scan_fov=4.71, scan_std=0.01,
               scan_max_range=15.0, free_thresh=0.8)
    sim = RacecarSimulator(cfg)
    omap = range_libc.PyOMap(g)
    sim.setMap(omap, g.resolution, g.origin)
    sim.setRaytracingMethod("RMGPU")
    st = np.zeros(11)
    st[:3] = maps.sample_free_poses(g, 1, 5, 8.0, omap.distance_transform())[0]
    sim.setState(st)
    return sim, g, omap


def test_facade_matches_planner():
    sim, g, omap = _sim()
    n = 25
    agent = MCTS(sim, None, 0.05, 200, n_iterations=n, seed=3)
    a = agent.mcts()
    assert agent.action == a and agent.iterations == n
    m = sim.scan_simulator.scan_method
    pl = MCTSPlanner(sim.car, m, 1, n + 1, sim.scan_fov, sim.num_rays, sim.edge_distances, sim.ttc_thresh,
                     source="fg", followgap=agent.fg, max_steer=sim.max_steer_ang, max_speed=sim.max_speed)
    pl.reset(sim.getState()[None, :], [0.05], [3])
    pl.run(n)
    best_a, best_v, n_nodes = pl.best()
    assert a == best_a[0] and n_nodes[0] == n + 1
    arr = pl.read_tree(0)
    nodes = []

    def walk(node):
        nodes.append(node)
        for c in node.children:
            assert c.parent is node
            walk(c)
    walk(agent.root)
    assert len(nodes) == n + 1 and agent.root.parent is None
    for nd in nodes:
        i = nd.index
        assert nd.visits == arr["visits"][i] and nd.terminal == bool(arr["terminal"][i])
        assert same_bits(np.float64(nd.reward), arr["reward"][i]) and same_bits(np.float64(nd.action), arr["action"][i])
        assert same_bits(nd.state, arr["state"][i])
        assert [c.index for c in nd.children] == ([] if arr["first_child"][i] < 0 else
                                                  _siblings(arr, arr["first_child"][i]))
    assert max(agent.root.children, key=lambda c: c.visits).action == a       # (first of equals: max keeps the first)
    # the many-trees façade: the same tree from the same state and seed
    acts, vis, nn = sim.planMCTSMany(sim.getState()[None, :], n, seeds=[3], root_actions=0.05)
    assert same_bits(acts, best_a) and (vis == best_v).all() and (nn == n_nodes).all()


def _siblings(arr, c):
    out = []
    while c >= 0:
        out.append(int(c))
        c = arr["next_sibling"][c]
    return out


def test_facade_budget_stops_within_budget_and_capacity():
    sim, g, omap = _sim()
    agent = MCTS(sim, None, 0.0, 200, budget=0.3, seed=1)
    MCTS(sim, None, 0.0, 200, n_iterations=1).mcts()                            # (warm the kernels)
    t0 = time.time()
    agent.mcts()
    took = time.time() - t0
    assert 1 <= agent.iterations <= agent.max_nodes - 1
    assert took < 0.3 + 0.25, took
    small = MCTS(sim, None, 0.0, 200, budget=5.0, max_nodes=6)
    t0 = time.time()
    small.mcts()
    assert small.iterations == 5 and time.time() - t0 < 5.0
    tiny = MCTS(sim, None, 0.0, 200, budget=0.0)
    tiny.mcts()
    assert tiny.iterations == 1 and tiny.action is not None


# ---------------------------------------------------------------- 6. the UCB probe
def test_ucb_probe_equals_python():
    rng = np.random.default_rng(0)
    n = 100_000
    visits = rng.integers(1, 5000, n).astype(np.int32)
    sums = np.minimum(visits.astype(np.int64) + rng.integers(0, 200_000, n), 1 << 24).astype(np.int32)
    sums[:1000] = 1
    reward = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)
    reward[1000:1010] = [np.inf, -np.inf, np.nan, 0.0, -0.0, 1e308, -1e308, 5e-324, -10.0, 2.5]
    Cc = 0.5
    out = np.empty(n)
    _lib.check(_lib.lib().rl_mcts_probe_ucb(0, reward.ctypes.data_as(_lib.f64p), visits.ctypes.data_as(_lib.i32p),
                                            sums.ctypes.data_as(_lib.i32p), n, Cc, out.ctypes.data_as(_lib.f64p)))
    want = np.array([r / int(v) + Cc * math.sqrt(math.log(int(s)) / int(v)) for r, v, s in zip(reward, visits, sums)])
    nan = np.isnan(want)
    assert (np.isnan(out) == nan).all()
    assert same_bits(out[~nan], want[~nan])
    bad = np.zeros(1, np.int32)
    assert _lib.lib().rl_mcts_probe_ucb(0, reward.ctypes.data_as(_lib.f64p), bad.ctypes.data_as(_lib.i32p),
                                        sums.ctypes.data_as(_lib.i32p), 1, Cc, out.ctypes.data_as(_lib.f64p)) == -1
