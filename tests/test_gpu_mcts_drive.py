"""The closed MCTS loop on the MI355X (rl_mcts_drive, MCTSPlanner.drive, CarBatch.drive_mcts,
RacecarSimulator.driveMCTSMany): every decision of every car bit-identical to the loop composed on the host from the
public calls (reset, run, best, the root scan's crash test, rollout), crash and freeze, chunking and batching
invariance, errors, the façades."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLD
import policy_statement as PS
from test_gpu_drive import _edge, _same_bits, _starts
from test_gpu_mcts import _assert_tree, _roots, _scan
from pyracecarsimulator_amd import Policy, RacecarSimulator, _lib, maps, range_libc
from pyracecarsimulator_amd import mcts as M
from pyracecarsimulator_amd import racecar as RC
from pyracecarsimulator_amd.followgap import PyFollowGap
from pyracecarsimulator_amd.mcts import MCTSPlanner

pytestmark = pytest.mark.gpu

FOV, B, THRESH = 4.71, 1081, 0.001
MAX_STEER = RC.DEFAULT_CAR["max_steer_ang"]
L, EVERY, SPEED = 40, 10, 2.0
CLIP = 0.4189


@pytest.fixture(scope="module", autouse=True)
def _gpu(need_gpu):
    yield


@pytest.fixture(scope="module")
def handles():
    layers, relu = PS.load_fixture(os.path.join(GOLD, "policy_mlp720.npz"))
    return {"fg": PyFollowGap(10, 15.0, MAX_STEER, 0.004), "nn": Policy.from_arrays(layers, relu), "random": None}


@pytest.fixture(scope="module")
def world():
    g = maps.load_colombia()
    omap = range_libc.PyOMap(g)
    return {"g": g, "omap": omap, "dt": omap.distance_transform(), "m": range_libc.PyRayMarchingGPU(omap, 300),
            "cars": RC.CarBatch()}


def _planner(cars, m, K, I, source, h, *, num_rays=B, rollout_steps=L, action_every=EVERY, edge=None):
    return MCTSPlanner(cars, m, K, I + 1, FOV, num_rays, _edge(num_rays) if edge is None else edge, THRESH,
                       source=source, followgap=h if source == "fg" else None, policy=h if source == "nn" else None,
                       rollout_steps=rollout_steps, action_every=action_every)


def _host_loop(cars, m, pl, std, base, states, recent, seeds, D, I, S, clip, *, num_rays=B, rollout_steps=L, edge=None,
               is_crashed=RC.is_crashed):
    """The D decisions composed on the host from the public calls; leaves pl holding the last decision's trees.
    edge: the planner's outline table (the car's by default); is_crashed: the crash test of the root scans."""
    K, nb = len(states), num_rays
    stride = M.drive_stride(K, nb, I, rollout_steps)
    states, recent = states.copy(), np.array(recent, np.float64)
    first = np.full(K, -(D + 1), np.int32)
    actions, visits, trace = np.full((K, D), np.nan), np.full((K, D), -1, np.int32), np.full((K, D, 11), np.nan)
    edge = _edge(nb) if edge is None else edge
    for d in range(D):
        off = base + d * stride
        m.set_noise(std, 99, off)
        pl.reset(states, recent, M.drive_seeds(seeds, d))
        pl.run(I)
        a, v, _ = pl.best()
        poses = np.stack([pl.read_tree(k)["scan_pose"][0] for k in range(K)])
        ranges = _scan(m, std, off, poses, nb)
        for k in range(K):
            if first[k] < 0 and is_crashed(ranges[k], nb, 1, edge, THRESH) >= 0:
                first[k] = d
        live = first < 0
        trace[live, d], actions[live, d], visits[live, d] = states[live], a[live], v[live]
        if live.any():
            acts = np.stack([np.full(int(live.sum()), SPEED), a[live]], axis=1)[:, None, :]
            _, out, _ = cars.rollout(states[live], acts, n_steps=S, action_every=S)
            states[live] = out
            recent[live] = M.drive_recent(a[live], clip)
    m.set_noise(std, 99, base)
    assert _same_bits(np.isnan(actions), M.drive_dead_rows(first, D))
    return first, states, recent, actions, visits, trace


def _assert_drive(got, want, what):
    for name, g_, w_ in zip(("first", "states_out", "recent_out", "actions", "visits", "trace"), got, want):
        assert g_.shape == w_.shape and g_.dtype == w_.dtype, (what, name)
        assert _same_bits(g_, w_), (what, name, np.nonzero(g_ != w_))


# ---------------------------------------------------------------- 1. the loop equals the host-composed loop
def _loop_case(world, m, std, source, h, K, S, D, I, *, num_rays=B, rollout_steps=L, action_every=EVERY, edge=None,
               starts=None, is_crashed=RC.is_crashed):
    """starts: (states, recent actions, seeds) of the K cars (drawn on the world's map by default)."""
    cars, base = world["cars"], 777
    states, recent, seeds = starts if starts is not None else _roots(world["g"], world["dt"], K, 31 + K)
    shape = dict(num_rays=num_rays, rollout_steps=rollout_steps, action_every=action_every, edge=edge)
    host_pl, dev_pl = _planner(cars, m, K, I, source, h, **shape), _planner(cars, m, K, I, source, h, **shape)
    try:
        want = _host_loop(cars, m, host_pl, std, base, states, recent, seeds, D, I, S, CLIP, num_rays=num_rays,
                          rollout_steps=rollout_steps, edge=edge, is_crashed=is_crashed)
        print("first (host loop):", want[0])
        m.set_noise(std, 99, base)
        probe = states[:2, :3].astype(np.float32)
        before = _scan_keep(m, probe, num_rays)
        nt = m.get_info("nt_store")
        got = dev_pl.drive(states, recent, seeds, D, I, steps_per_decision=S, steer_clip=CLIP, trace=True)
        _assert_drive(got, want, (source, K, S))
        for k in range(K):
            _assert_tree(dev_pl.read_tree(k), host_pl.read_tree(k), (source, K, S, k))
        ga, gv, gn = dev_pl.best()
        wa, wv, wn = host_pl.best()
        assert _same_bits(ga, wa) and _same_bits(gv, wv) and _same_bits(gn, wn) and (gn == I + 1).all()
        # the handle reads as before the call: the option the planner overrides, and the noise offset (a plain scan
        # draws the noise of the same ray ids)
        assert m.get_info("nt_store") == nt
        assert _same_bits(_scan_keep(m, probe, num_rays), before)
    finally:
        host_pl.close()
        dev_pl.close()
        m.set_noise(0.0, 0, 0)
    return want


def _scan_keep(m, poses, num_rays=B):
    """A plain scan with the handle's noise settings as they stand."""
    out = np.empty(len(poses) * num_rays, np.float32)
    m.calc_range_fan(np.ascontiguousarray(poses, np.float32), out, FOV, num_rays)
    return out


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("K", [6, 9])
@pytest.mark.parametrize("source", ["fg", "nn", "random"])
def test_loop_equals_host_composed_loop(world, handles, source, K, S):
    _loop_case(world, world["m"], 0.05, source, handles[source], K, S, D=4, I=5)


def test_loop_equals_host_composed_loop_on_a_table_method(world, handles):
    m = range_libc.PyCDDTCast(world["omap"], 300, 112)
    _loop_case(world, m, 0.0, "fg", handles["fg"], 6, 2, D=3, I=4)


# ---------------------------------------------------------------- 2. crash and freeze
POOL, D_CRASH, I_CRASH, S_CRASH = 64, 6, 3, 50        # 50 steps at 2 m/s and dt 0.01: about a metre per decision


@pytest.fixture(scope="module")
def crash_pool(world):
    """The host-composed loop over a pool of near-wall starts (noise off: a car's course does not depend on its
    batch), computed once: (states, recent, seeds, the loop's results)."""
    cars, m = world["cars"], world["m"]
    states, _ = _starts(world["g"], world["dt"], POOL, 5, 1.2, speed_hi=3.0)
    rng = np.random.default_rng(5)
    recent = rng.uniform(-0.3, 0.3, POOL)
    seeds = rng.integers(0, 2 ** 63, POOL, dtype=np.uint64)
    pl = _planner(cars, m, POOL, I_CRASH, "random", None)
    try:
        res = _host_loop(cars, m, pl, 0.0, 0, states, recent, seeds, D_CRASH, I_CRASH, S_CRASH, CLIP)
    finally:
        pl.close()
        m.set_noise(0.0, 0, 0)
    first = res[0]
    print("crash pool: first =", first)
    pick = np.concatenate([np.nonzero(first >= 1)[0][:2], np.nonzero(first == 0)[0][:2], np.nonzero(first < 0)[0][:2]])
    return states, recent, seeds, res, pick


def test_crash_and_freeze(world, crash_pool):
    cars, m = world["cars"], world["m"]
    states, recent, seeds, pool, pick = crash_pool
    first_w = pool[0][pick]
    assert (first_w >= 1).any(), "no car of the pool crashes at a decision >= 1: widen the pool"
    assert (first_w == 0).any(), "no car of the pool is crashed at decision 0: widen the pool"
    assert (first_w < 0).any(), "no car of the pool survives: widen the pool"
    K, D = len(pick), D_CRASH
    pl = _planner(cars, m, K, I_CRASH, "random", None)
    try:
        m.set_noise(0.0, 0, 0)
        first, out, rec, actions, visits, trace = pl.drive(states[pick], recent[pick], seeds[pick], D, I_CRASH,
                                                           steps_per_decision=S_CRASH, steer_clip=CLIP, trace=True)
    finally:
        pl.close()
    _assert_drive((first, out, rec, actions, visits, trace), tuple(a[pick] for a in pool), "crash")
    dead = M.drive_dead_rows(first, D)
    assert (first[first < 0] == -(D + 1)).all()
    assert np.isnan(actions[dead]).all() and not np.isnan(actions[~dead]).any()
    assert (visits[dead] == -1).all() and (visits[~dead] >= 1).all()
    assert np.isnan(trace[dead]).all() and not np.isnan(trace[~dead]).any()
    for k in range(K):
        if first[k] == 0:                     # never moved
            assert _same_bits(out[k], states[pick][k]) and _same_bits(rec[k], recent[pick][k])
        elif first[k] > 0:                    # frozen in the state the last live decision stepped to
            d = first[k] - 1
            acts = np.array([[[SPEED, actions[k, d]]]])
            _, want, _ = cars.rollout(trace[k, d][None, :], acts, n_steps=S_CRASH, action_every=S_CRASH)
            assert _same_bits(out[k], want[0])
            assert _same_bits(rec[k], M.drive_recent(actions[k, d], CLIP))


# ---------------------------------------------------------------- 3. chunking
def test_chunks_of_decisions_equal_the_whole(world, handles):
    cars, m, h = world["cars"], world["m"], handles["fg"]
    K, I, S, std, base = 6, 4, 2, 0.05, 555
    states, _ = _starts(world["g"], world["dt"], K, 7, 6.0, speed_hi=3.0)      # (clear of the walls: a crash is not
    rng = np.random.default_rng(7)                                             #  part of what a chunk hands on)
    recent, seeds = rng.uniform(-0.3, 0.3, K), rng.integers(0, 2 ** 63, K, dtype=np.uint64)
    stride = M.drive_stride(K, B, I, L)
    pl = _planner(cars, m, K, I, "fg", h)
    try:
        m.set_noise(std, 99, base)
        whole = pl.drive(states, recent, seeds, 4, I, steps_per_decision=S, steer_clip=CLIP, trace=True)
        trees = [pl.read_tree(k) for k in range(K)]
        m.set_noise(std, 99, base)
        one = pl.drive(states, recent, seeds, 2, I, steps_per_decision=S, steer_clip=CLIP, trace=True)
        m.set_noise(std, 99, base + 2 * stride)
        two = pl.drive(one[1], one[2], M.drive_seeds(seeds, 2), 2, I, steps_per_decision=S, steer_clip=CLIP, trace=True)
        for k in range(K):
            _assert_tree(pl.read_tree(k), trees[k], ("chunked", k))
    finally:
        pl.close()
        m.set_noise(0.0, 0, 0)
    assert (whole[0] == -5).all(), whole[0]
    first = np.where(two[0] >= 0, two[0] + 2, -5).astype(np.int32)
    joined = (first, two[1], two[2]) + tuple(np.concatenate([a, b], axis=1) for a, b in zip(one[3:], two[3:]))
    _assert_drive(joined, whole, "chunked")


# ---------------------------------------------------------------- 4. batching
def test_cars_in_a_batch_equal_each_car_alone(world, crash_pool):
    cars, m = world["cars"], world["m"]
    states, recent, seeds, pool, pick = crash_pool
    pick = pick[:6]
    K, D, I, S = len(pick), 3, I_CRASH, S_CRASH
    assert K == 6 and (pool[0][pick] >= 0).any(), "the batch needs a crashed car"
    m.set_noise(0.0, 0, 0)
    pl = _planner(cars, m, K, I, "random", None)
    try:
        batch = pl.drive(states[pick], recent[pick], seeds[pick], D, I, steps_per_decision=S, steer_clip=CLIP, trace=True)
        trees = [pl.read_tree(k) for k in range(K)]
    finally:
        pl.close()
    assert (batch[0] >= 0).any() and (batch[0] < 0).any()
    one = _planner(cars, m, 1, I, "random", None)
    try:
        for k in range(K):
            i = pick[k:k + 1]
            alone = one.drive(states[i], recent[i], seeds[i], D, I, steps_per_decision=S, steer_clip=CLIP, trace=True)
            _assert_drive(alone, tuple(a[k:k + 1] for a in batch), ("alone", k))
            _assert_tree(one.read_tree(0), trees[k], ("alone", k))
    finally:
        one.close()


# ---------------------------------------------------------------- 5. errors
def test_errors_leave_handles_usable(world, handles):
    cars, m, fg = world["cars"], world["m"], handles["fg"]
    K, I = 4, 3
    states, recent, seeds = _roots(world["g"], world["dt"], K, 9)
    seeds = seeds.astype(np.uint64)
    poses = maps.sample_free_poses(world["g"], 8, 3, 4.0, world["dt"])
    Lb = _lib.lib()
    pl = _planner(cars, m, K, I, "fg", fg)
    m.set_noise(0.05, 7, 321)
    scan0 = _scan_keep(m, poses)

    def plan():
        m.set_noise(0.05, 7, 321)
        pl.reset(states, recent, seeds)
        pl.run(I)
        return [pl.read_tree(k) for k in range(K)], pl.best()

    want_trees, want_best = plan()

    def still_usable():
        assert _same_bits(_scan_keep(m, poses), scan0)
        assert m.get_info("nt_store") == 1
        trees, best = plan()
        for k in range(K):
            _assert_tree(trees[k], want_trees[k], k)
        assert all(_same_bits(a, b) for a, b in zip(best, want_best))

    D = 2
    bufs = dict(first=np.empty(K, np.int32), out=np.empty((K, 11)), rec=np.empty(K), act=np.empty((K, D)),
                vis=np.empty((K, D), np.int32))

    def call(h=pl._h, D_=D, I_=I, S_=1, clip=CLIP, **null):
        p = lambda name, a, t: None if name in null else a.ctypes.data_as(t)
        return Lb.rl_mcts_drive(h if "m" not in null else None, p("states", states, _lib.f64p),
                                p("recent", recent, _lib.f64p), p("seeds", seeds, C.POINTER(C.c_uint64)), D_, I_, S_,
                                clip, p("first", bufs["first"], _lib.i32p), p("out", bufs["out"], _lib.f64p),
                                p("rec", bufs["rec"], _lib.f64p), p("act", bufs["act"], _lib.f64p),
                                p("vis", bufs["vis"], _lib.i32p), None)

    try:
        for name in ("m", "states", "recent", "seeds", "first", "out", "rec", "act", "vis"):
            assert call(**{name: True}) == -1, name
        still_usable()
        for bad in (dict(D_=-1), dict(I_=0), dict(I_=-3), dict(I_=I + 1), dict(S_=0), dict(S_=-2), dict(clip=-0.1),
                    dict(clip=float("nan"))):
            assert call(**bad) == -1, bad
            still_usable()
        # the range method's refusal (fov NaN), as rl_mcts_run gives it
        pl2 = MCTSPlanner(cars, m, K, I + 1, float("nan"), B, _edge(), THRESH, source="fg", followgap=fg,
                          rollout_steps=L, action_every=EVERY)
        try:
            assert call(h=pl2._h) == -1
            with pytest.raises(_lib.ScanLibError, match="NaN"):
                pl2.drive(states, recent, seeds, D, I)
        finally:
            pl2.close()
        still_usable()
        # no decisions: the documented outputs, the planner's trees untouched
        bufs["first"][:] = 7
        assert call(D_=0) == 0
        assert (bufs["first"] == -1).all() and _same_bits(bufs["out"], states) and _same_bits(bufs["rec"], recent)
        for k in range(K):
            _assert_tree(pl.read_tree(k), want_trees[k], k)
        first, out, rec, act, vis = pl.drive(states, recent, seeds, 0, I)
        assert (first == -1).all() and _same_bits(out, states) and _same_bits(rec, recent)
        assert act.shape == (K, 0) and vis.shape == (K, 0)
        # and a good call still works
        m.set_noise(0.05, 7, 321)
        assert call() == 0 and (bufs["vis"][bufs["first"] < 0] >= 1).all()
        still_usable()
    finally:
        pl.close()
        m.set_noise(0.0, 0, 0)


# ---------------------------------------------------------------- 6. façades
def test_facades_match_planner(world, handles):
    g = world["g"]
    cfg = dict(RC.DEFAULT_CAR)
    cfg.update(scan_dist_to_base=0.275, batch_size=L, scan_beams=1080, scan_fov=4.71, scan_std=0.01,
               scan_max_range=15.0, free_thresh=0.8)
    sim = RacecarSimulator(cfg)
    sim.setMap(world["omap"], g.resolution, g.origin)
    sim.setRaytracingMethod("RMGPU")
    m = sim.scan_simulator.scan_method
    K, D, I, S = 3, 3, 4, 2
    states, recent, seeds = _roots(g, world["dt"], K, 3)
    fg = PyFollowGap(10, 15.0, sim.max_steer_ang, 0.004)
    pl = MCTSPlanner(sim.car, m, K, I + 1, sim.scan_fov, sim.num_rays, sim.edge_distances, sim.ttc_thresh, source="fg",
                     followgap=fg, rollout_steps=L, scan_dist_to_base=sim.scan_dist_to_base)
    try:
        want = pl.drive(states, recent, seeds, D, I, steps_per_decision=S, steer_clip=CLIP)
        want_tr = pl.drive(states, recent, seeds, D, I, steps_per_decision=S, steer_clip=None, trace=True)
    finally:
        pl.close()
    assert len(want) == 5 and len(want_tr) == 6
    got = sim.driveMCTSMany(states, D, I, seeds=seeds, steps_per_decision=S, recent_actions=recent)
    _assert_drive(got, want, "driveMCTSMany")
    got = sim.car.drive_mcts(m, fg, states, D, I, seeds, sim.scan_fov, sim.num_rays, sim.edge_distances, sim.ttc_thresh,
                             recent_actions=recent, steps_per_decision=S, steer_clip=CLIP, rollout_steps=L)
    _assert_drive(got, want, "drive_mcts")
    got = sim.car.drive_mcts(m, fg, states, D, I, seeds, sim.scan_fov, sim.num_rays, sim.edge_distances, sim.ttc_thresh,
                             recent_actions=recent, steps_per_decision=S, rollout_steps=L, trace=True)
    _assert_drive(got, want_tr, "drive_mcts raw")
    with pytest.raises(ValueError, match="policy"):
        sim.driveMCTSMany(states, D, I, source="nn")
