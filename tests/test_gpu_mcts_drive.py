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
import support
from mcts_checks import (B, CLIP, DRIVE_L as L, EVERY, SPEED, assert_drive, assert_tree, host_loop, loop_case, planner,
                         roots, scan_keep)
from support import THRESH, same_bits
from pyracecarsimulator_amd import Policy, RacecarSimulator, _lib, maps, range_libc
from pyracecarsimulator_amd import mcts as M
from pyracecarsimulator_amd import racecar as RC
from pyracecarsimulator_amd.mcts import MCTSPlanner

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]


@pytest.fixture(scope="module")
def handles():
    layers, relu = PS.load_fixture(os.path.join(GOLD, "policy_mlp720.npz"))
    return {"fg": support.followgap(), "nn": Policy.from_arrays(layers, relu), "random": None}


@pytest.fixture(scope="module")
def world():
    g = maps.load_colombia()
    omap = range_libc.PyOMap(g)
    return {"g": g, "omap": omap, "dt": omap.distance_transform(), "m": range_libc.PyRayMarchingGPU(omap, 300),
            "cars": RC.CarBatch()}


# ---------------------------------------------------------------- 1. the loop equals the host-composed loop


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("K", [6, 9])
@pytest.mark.parametrize("source", ["fg", "nn", "random"])
def test_loop_equals_host_composed_loop(world, handles, source, K, S):
    loop_case(world, world["m"], 0.05, source, handles[source], K, S, D=4, I=5)


def test_loop_equals_host_composed_loop_on_a_table_method(world, handles):
    m = range_libc.PyCDDTCast(world["omap"], 300, 112)
    loop_case(world, m, 0.0, "fg", handles["fg"], 6, 2, D=3, I=4)


# ---------------------------------------------------------------- 2. crash and freeze
POOL, D_CRASH, I_CRASH, S_CRASH = 64, 6, 3, 50        # 50 steps at 2 m/s and dt 0.01: about a metre per decision


@pytest.fixture(scope="module")
def crash_pool(world):
    """The host-composed loop over a pool of near-wall starts (noise off: a car's course does not depend on its
    batch), computed once: (states, recent, seeds, the loop's results)."""
    cars, m = world["cars"], world["m"]
    states, _ = support.starts(world["g"], world["dt"], POOL, 5, 1.2, speed_hi=3.0)
    rng = np.random.default_rng(5)
    recent = rng.uniform(-0.3, 0.3, POOL)
    seeds = rng.integers(0, 2 ** 63, POOL, dtype=np.uint64)
    pl = planner(cars, m, POOL, I_CRASH, "random", None)
    try:
        res = host_loop(cars, m, pl, 0.0, 0, states, recent, seeds, D_CRASH, I_CRASH, S_CRASH, CLIP)
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
    pl = planner(cars, m, K, I_CRASH, "random", None)
    try:
        m.set_noise(0.0, 0, 0)
        first, out, rec, actions, visits, trace = pl.drive(states[pick], recent[pick], seeds[pick], D, I_CRASH,
                                                           steps_per_decision=S_CRASH, steer_clip=CLIP, trace=True)
    finally:
        pl.close()
    assert_drive((first, out, rec, actions, visits, trace), tuple(a[pick] for a in pool), "crash")
    dead = M.drive_dead_rows(first, D)
    assert (first[first < 0] == -(D + 1)).all()
    assert np.isnan(actions[dead]).all() and not np.isnan(actions[~dead]).any()
    assert (visits[dead] == -1).all() and (visits[~dead] >= 1).all()
    assert np.isnan(trace[dead]).all() and not np.isnan(trace[~dead]).any()
    for k in range(K):
        if first[k] == 0:                     # never moved
            assert same_bits(out[k], states[pick][k]) and same_bits(rec[k], recent[pick][k])
        elif first[k] > 0:                    # frozen in the state the last live decision stepped to
            d = first[k] - 1
            acts = np.array([[[SPEED, actions[k, d]]]])
            _, want, _ = cars.rollout(trace[k, d][None, :], acts, n_steps=S_CRASH, action_every=S_CRASH)
            assert same_bits(out[k], want[0])
            assert same_bits(rec[k], M.drive_recent(actions[k, d], CLIP))


# ---------------------------------------------------------------- 3. chunking
def test_chunks_of_decisions_equal_the_whole(world, handles):
    cars, m, h = world["cars"], world["m"], handles["fg"]
    K, I, S, std, base = 6, 4, 2, 0.05, 555
    states, _ = support.starts(world["g"], world["dt"], K, 7, 6.0, speed_hi=3.0)      # (clear of the walls: a crash is not
    rng = np.random.default_rng(7)                                             #  part of what a chunk hands on)
    recent, seeds = rng.uniform(-0.3, 0.3, K), rng.integers(0, 2 ** 63, K, dtype=np.uint64)
    stride = M.drive_stride(K, B, I, L)
    pl = planner(cars, m, K, I, "fg", h)
    try:
        m.set_noise(std, 99, base)
        whole = pl.drive(states, recent, seeds, 4, I, steps_per_decision=S, steer_clip=CLIP, trace=True)
        trees = [pl.read_tree(k) for k in range(K)]
        m.set_noise(std, 99, base)
        one = pl.drive(states, recent, seeds, 2, I, steps_per_decision=S, steer_clip=CLIP, trace=True)
        m.set_noise(std, 99, base + 2 * stride)
        two = pl.drive(one[1], one[2], M.drive_seeds(seeds, 2), 2, I, steps_per_decision=S, steer_clip=CLIP, trace=True)
        for k in range(K):
            assert_tree(pl.read_tree(k), trees[k], ("chunked", k))
    finally:
        pl.close()
        m.set_noise(0.0, 0, 0)
    assert (whole[0] == -5).all(), whole[0]
    first = np.where(two[0] >= 0, two[0] + 2, -5).astype(np.int32)
    joined = (first, two[1], two[2]) + tuple(np.concatenate([a, b], axis=1) for a, b in zip(one[3:], two[3:]))
    assert_drive(joined, whole, "chunked")


# ---------------------------------------------------------------- 4. batching
def test_cars_in_a_batch_equal_each_car_alone(world, crash_pool):
    cars, m = world["cars"], world["m"]
    states, recent, seeds, pool, pick = crash_pool
    pick = pick[:6]
    K, D, I, S = len(pick), 3, I_CRASH, S_CRASH
    assert K == 6 and (pool[0][pick] >= 0).any(), "the batch needs a crashed car"
    m.set_noise(0.0, 0, 0)
    pl = planner(cars, m, K, I, "random", None)
    try:
        batch = pl.drive(states[pick], recent[pick], seeds[pick], D, I, steps_per_decision=S, steer_clip=CLIP, trace=True)
        trees = [pl.read_tree(k) for k in range(K)]
    finally:
        pl.close()
    assert (batch[0] >= 0).any() and (batch[0] < 0).any()
    one = planner(cars, m, 1, I, "random", None)
    try:
        for k in range(K):
            i = pick[k:k + 1]
            alone = one.drive(states[i], recent[i], seeds[i], D, I, steps_per_decision=S, steer_clip=CLIP, trace=True)
            assert_drive(alone, tuple(a[k:k + 1] for a in batch), ("alone", k))
            assert_tree(one.read_tree(0), trees[k], ("alone", k))
    finally:
        one.close()


# ---------------------------------------------------------------- 5. errors
def test_errors_leave_handles_usable(world, handles):
    cars, m, fg = world["cars"], world["m"], handles["fg"]
    K, I = 4, 3
    states, recent, seeds = roots(world["g"], world["dt"], K, 9)
    seeds = seeds.astype(np.uint64)
    poses = maps.sample_free_poses(world["g"], 8, 3, 4.0, world["dt"])
    Lb = _lib.lib()
    pl = planner(cars, m, K, I, "fg", fg)
    m.set_noise(0.05, 7, 321)
    scan0 = scan_keep(m, poses)

    def plan():
        m.set_noise(0.05, 7, 321)
        pl.reset(states, recent, seeds)
        pl.run(I)
        return [pl.read_tree(k) for k in range(K)], pl.best()

    want_trees, want_best = plan()

    def still_usable():
        assert same_bits(scan_keep(m, poses), scan0)
        assert m.get_info("nt_store") == 1
        trees, best = plan()
        for k in range(K):
            assert_tree(trees[k], want_trees[k], k)
        assert all(same_bits(a, b) for a, b in zip(best, want_best))

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
        pl2 = MCTSPlanner(cars, m, K, I + 1, float("nan"), B, support.edge(B), THRESH, source="fg", followgap=fg,
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
        assert (bufs["first"] == -1).all() and same_bits(bufs["out"], states) and same_bits(bufs["rec"], recent)
        for k in range(K):
            assert_tree(pl.read_tree(k), want_trees[k], k)
        first, out, rec, act, vis = pl.drive(states, recent, seeds, 0, I)
        assert (first == -1).all() and same_bits(out, states) and same_bits(rec, recent)
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
    states, recent, seeds = roots(g, world["dt"], K, 3)
    fg = support.followgap(max_angle=sim.max_steer_ang)
    pl = MCTSPlanner(sim.car, m, K, I + 1, sim.scan_fov, sim.num_rays, sim.edge_distances, sim.ttc_thresh, source="fg",
                     followgap=fg, rollout_steps=L, scan_dist_to_base=sim.scan_dist_to_base)
    try:
        want = pl.drive(states, recent, seeds, D, I, steps_per_decision=S, steer_clip=CLIP)
        want_tr = pl.drive(states, recent, seeds, D, I, steps_per_decision=S, steer_clip=None, trace=True)
    finally:
        pl.close()
    assert len(want) == 5 and len(want_tr) == 6
    got = sim.driveMCTSMany(states, D, I, seeds=seeds, steps_per_decision=S, recent_actions=recent)
    assert_drive(got, want, "driveMCTSMany")
    got = sim.car.drive_mcts(m, fg, states, D, I, seeds, sim.scan_fov, sim.num_rays, sim.edge_distances, sim.ttc_thresh,
                             recent_actions=recent, steps_per_decision=S, steer_clip=CLIP, rollout_steps=L)
    assert_drive(got, want, "drive_mcts")
    got = sim.car.drive_mcts(m, fg, states, D, I, seeds, sim.scan_fov, sim.num_rays, sim.edge_distances, sim.ttc_thresh,
                             recent_actions=recent, steps_per_decision=S, rollout_steps=L, trace=True)
    assert_drive(got, want_tr, "drive_mcts raw")
    with pytest.raises(ValueError, match="policy"):
        sim.driveMCTSMany(states, D, I, source="nn")
