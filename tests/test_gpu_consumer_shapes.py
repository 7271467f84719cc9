"""The closed-loop kernels off the 1081-beam, 64-tree, 200-step path, on the MI355X (tests/consumer_shapes.py holds
the shapes; tests/test_consumer_shapes_host.py checks them with the references alone):

  A. the crash ballot of drive_tick_kernel<ROWS, FollowGapSteer / PolicySteer> and mcts_act_kernel<ROWS> decided by one
     beam, at every row count 1 ... 20 and every edge of the last row;
  B. whole drive_followgap / drive_policy / race_followgap loops at those sizes against a loop composed on the host from
     the public scan, the oracle's crash test and FollowGap, and rollout(n_steps=1);
  C. planner trees and rl_mcts_drive cars beyond the first 64-lane workgroup;
  D. roll-out lengths in every regime of the reward's pairwise sum, and n_act * every != L;
  E. check_collision_many / check_collision_groups at other beam counts, and the literal handle's refusal below 64 beams.

Every expectation is bit-exact except the lidar poses (one f32 ulp of the f64 formula).  Every test first asserts the
inequality that puts it on its path."""
import math
import os

import numpy as np
import pytest

import consumer_shapes as CS
import drive_cases as DC
import mcts_checks as MC
import policy_statement as PS
import race_statement as RS
import support
from conftest import GOLD
from support import D_BASE, FOV, MAX_STEER, THRESH, same_bits, within_one_ulp
from pyracecarsimulator_amd import Policy, _lib, maps, range_libc
from pyracecarsimulator_amd import racecar as RC
from pyracecarsimulator_amd.mcts import MCTSPlanner

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

MRX = 300
R = CS.R_CARS
CLIP = MC.CLIP
RL_ERR_UNSUPPORTED = -4                               # include/scanlib.h rl_status


class Room:
    """The empty 10 m room of parts A and B: its oracle map, one handle per range method, the car and FollowGap."""

    def __init__(self, oracle_mod):
        self.O = oracle_mod
        self.g = maps.make_room(CS.ROOM)
        self.om = oracle_mod.OracleMap.from_gridmap(self.g, MRX)
        self.omap = range_libc.PyOMap(self.g)
        self.m = {"RMGPU": range_libc.PyRayMarchingGPU(self.omap, MRX), "RM": range_libc.PyRayMarching(self.omap, MRX)}
        self.cars = RC.CarBatch()
        self.fg = support.followgap()

    def oracle_scan(self, poses, n):
        return self.om.rm_fan(np.ascontiguousarray(poses, np.float32), FOV, n, step_coeff=1.0)[0].reshape(-1, n)

    def followgap(self, scan):
        return np.float32(self.O.followgap_eval(scan, 15.0, MAX_STEER, 0.004))


@pytest.fixture(scope="module")
def room(oracle_mod):
    return Room(oracle_mod)


@pytest.fixture(scope="module")
def nets():
    layers, relu = PS.load_fixture(os.path.join(GOLD, "policy_mlp720.npz"))
    return {0: Policy.from_arrays(layers, relu, in_start=0), 180: Policy.from_arrays(layers, relu)}


def _flat(res):
    """A race's (R, P, ...) arrays as drive_followgap's (R P, ...)."""
    return tuple(a.reshape((-1,) + a.shape[2:]) for a in res)


# ---------------------------------------------------------------- A. the crash ballot, beam by beam
def _ballot(room, n, run, answer):
    """run(edge) -> drive_*'s traced tuple of one tick; answer(scan) -> the source's f32 answer to a live car's scan.
    One beam j* of the outline table decides: the oracle's crash test on the oracle's scan at the traced lidar pose."""
    rows = CS.rows_of(n)
    assert CS.MIN_RAYS <= n <= CS.MAX_RAYS and 1 <= rows <= CS.FG_ROWS
    assert R > 2 * CS.DRIVE_CARS and R % CS.DRIVE_CARS, "three workgroups of drive_tick_kernel, the last one partial"
    scans = poses0 = None
    for j in CS.one_hot_beams(n) + (None,):
        edge = CS.one_hot_edge(n, j)
        first, final, vel, steers, sp, st = run(edge)
        assert first.shape == (R,) and steers.shape == (R, 1) and st.shape == (R, 1, 11)
        if scans is None:
            poses0, scans = sp[:, 0].copy(), room.oracle_scan(sp[:, 0], n)
        assert same_bits(sp[:, 0], poses0), (n, j)
        want = [0 if room.O.is_crashed(scans[r], n, 1, edge, THRESH) >= 0 else -2 for r in range(R)]
        assert want == [0 if j is not None else -2] * R, (n, j)          # what the table was built to decide
        assert first.tolist() == want, (n, j, rows)
        assert np.isfinite(st).all() and same_bits(final, st[:, 0]) and same_bits(vel[:, 0], st[:, 0, 3]), (n, j)
        if j is None:
            assert same_bits(steers[:, 0], np.array([answer(scans[r]) for r in range(R)], np.float32)), (n, j)
        else:
            assert np.isnan(steers).all(), (n, j)


@pytest.mark.parametrize("n", CS.SIZES)
def test_ballot_drive_followgap(room, n):
    states, speeds, _ = CS.room_starts(n)
    m = room.m["RMGPU"]
    _ballot(room, n, lambda edge: room.cars.drive_followgap(m, room.fg, states, 1, speeds, FOV, n, edge, THRESH,
                                                            trace=True), room.followgap)


@pytest.mark.parametrize("n", CS.SIZES)
def test_ballot_race_followgap(room, n):
    """rl_car_race_followgap reaches fg_tick_table through drive_loop with group > 0: races of one car."""
    states, speeds, _ = CS.room_starts(n)
    m = room.m["RMGPU"]
    _ballot(room, n, lambda edge: _flat(room.cars.race_followgap(m, room.fg, states[:, None, :], 1, speeds[:, None], FOV,
                                                                 n, edge, THRESH, trace=True)), room.followgap)


@pytest.mark.parametrize("n,in_start", CS.NN_SIZES)
def test_ballot_drive_policy(room, nets, n, in_start):
    states, speeds, _ = CS.room_starts(n)
    m, pol = room.m["RMGPU"], nets[in_start]
    assert in_start + 720 <= n
    _ballot(room, n, lambda edge: room.cars.drive_policy(m, pol, states, 1, speeds, FOV, n, edge, THRESH, trace=True),
            lambda scan: pol.predict_many(scan[None, :])[0])


MCTS_K, MCTS_IT, MCTS_L, MCTS_EVERY = 9, 4, 4, 3


def _ballot_mcts(room, n, source, h):
    """mcts_act_kernel<ROWS>: with the one-hot table every non-root node is terminal, so the trees grow by expansions
    under terminal nodes (exp_term in mcts_select_kernel, the j repeats of mcts_backup_kernel)."""
    assert CS.MIN_RAYS <= n <= CS.MAX_RAYS and MCTS_K > 8, "two workgroups of mcts_act_kernel, the last one of one tree"
    states = CS.room_starts(n)[0][:MCTS_K]
    rng = np.random.default_rng(n)
    actions = rng.uniform(-0.3, 0.3, MCTS_K)
    seeds = rng.integers(0, 2 ** 63, MCTS_K, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    m = room.m["RMGPU"]
    shape = dict(num_rays=n, rollout_steps=MCTS_L, action_every=MCTS_EVERY)
    for j in CS.one_hot_beams(n) + (None,):
        edge = CS.one_hot_edge(n, j)
        pl, trees, best = MC.device(room.cars, m, 0.0, 0, source, h, states, actions, seeds, MCTS_IT, edge=edge, **shape)
        pl.close()
        stmt, snaps = MC.replay(room.cars, m, 0.0, 0, source, h, states, actions, seeds, MCTS_IT, trees, (MCTS_IT,),
                                 edge=edge, is_crashed=room.O.is_crashed, **shape)
        for k in range(MCTS_K):
            t = snaps[MCTS_IT][k]
            if j is None:
                assert not t["terminal"].any(), (n, k)
            else:
                assert t["terminal"].tolist() == [0] + [1] * MCTS_IT, (n, j, k)
                assert (t["parent"] > 0).any(), "no expansion under a terminal node"
            MC.assert_tree(trees[k], t, (source, n, j, k))
            a, v = stmt[k].best()
            assert best[1][k] == v and same_bits(best[0][k:k + 1], np.array([a])), (n, j, k)


@pytest.mark.parametrize("n", CS.SIZES)
def test_ballot_mcts_act_followgap(room, n):
    _ballot_mcts(room, n, "fg", room.fg)


@pytest.mark.parametrize("n,in_start", CS.NN_SIZES)
def test_ballot_mcts_act_policy(room, nets, n, in_start):
    _ballot_mcts(room, n, "nn", nets[in_start])


# ---------------------------------------------------------------- B. whole loops against an independent host loop
def _host_drive(room, m, std, base, n, states, speeds, steer0, T, edge, got, answer, steer_of=lambda a: a.astype(np.float64),
                scan=None):
    """The loop composed on the host, tick by tick: rollout(n_steps=1), the public scan at the traced lidar poses with
    the noise offset base + t R n, the oracle's crash test, answer(scans of the live cars) -> f32 answers.  Asserts
    got (the device loop's traced tuple) against it as it goes."""
    first, final, vel, steers, sp, st = got
    N = states.shape[0]
    cur, steer, alive = states.copy(), steer0.astype(np.float64), np.ones(N, bool)
    want_first = np.full(N, -(T + 1), np.int32)
    last_pose = np.zeros((N, 3), np.float32)
    for t in range(T):
        idx = np.nonzero(alive)[0]
        dead = np.nonzero(~alive)[0]
        for arr in (vel, steers, sp, st):
            assert np.isnan(arr[dead, t]).all(), (n, t)                # rows after a crash stay NaN
        _, out, v1 = room.cars.rollout(cur[idx], np.stack([speeds[idx], steer[idx]], -1)[:, None, :], n_steps=1,
                                       action_every=1)
        assert same_bits(out, st[idx, t]) and same_bits(v1[:, 0], vel[idx, t]), (n, t)
        cur[idx] = out
        assert within_one_ulp(support.lidar_poses(out), sp[idx, t]), (n, t)
        last_pose[idx] = sp[idx, t]                                    # frozen cars keep their last pose
        m.set_noise(std, 99, base + t * N * n)
        if scan is None:
            ranges = np.empty(N * n, np.float32)
            m.calc_range_fan(last_pose, ranges, FOV, n)
        else:
            ranges = scan(last_pose, cur)
        ranges = ranges.reshape(N, n)
        crashed = np.array([room.O.is_crashed(ranges[r], n, 1, edge, THRESH) >= 0 for r in idx], bool)
        want_first[idx[crashed]] = t
        assert (first[idx] == t).tolist() == crashed.tolist(), (n, t)
        assert np.isnan(steers[idx[crashed], t]).all(), (n, t)
        go = idx[~crashed]
        if go.size:
            a = answer(ranges[go])
            assert same_bits(a, steers[go, t]), (n, t, np.nonzero(a != steers[go, t]))
            steer[go] = steer_of(a)
        alive[idx[crashed]] = False
    m.set_noise(0.0, 0, 0)
    assert first.tolist() == want_first.tolist(), n
    assert same_bits(final, cur), n
    return want_first


T_LOOP = 8


@pytest.mark.parametrize("n", CS.SIZES)
def test_loop_drive_followgap(room, n):
    rows = CS.rows_of(n)
    kind, std = CS.room_method(n)
    assert (kind == "RMGPU") == bool(rows % 2) and (std > 0) == (kind == "RMGPU")
    m = room.m[kind]
    states, speeds, steer0 = CS.room_starts(n)
    edge, base = support.edge(n), 5 * R * n + 3
    assert n == 1081 or base + R * n != base + R * 1081                # the noise walk depends on the beam count
    m.set_noise(std, 99, base)
    got = room.cars.drive_followgap(m, room.fg, states, T_LOOP, speeds, FOV, n, edge, THRESH, steer0=steer0, trace=True)
    first = _host_drive(room, m, std, base, n, states, speeds, steer0, T_LOOP, edge, got,
                        lambda scans: np.array([room.followgap(s) for s in scans], np.float32))
    assert (first[list(CS.WALL_CARS)] >= 0).any() and (first < 0).sum() >= 8, first
    live = np.isfinite(got[3])
    assert np.unique(got[3][live]).size >= 3


@pytest.mark.parametrize("n,in_start", CS.NN_SIZES)
def test_loop_drive_policy(room, nets, n, in_start):
    pol = nets[in_start]
    assert in_start + 720 <= n <= CS.MAX_RAYS and CS.rows_of(n) != 17
    clip = CLIP if n in CS.NN_CLIPPED else None
    kind, std = CS.room_method(n)
    m = room.m[kind]
    states, speeds, steer0 = CS.room_starts(n)
    edge, base = support.edge(n), 2 * R * n + 1
    m.set_noise(std, 99, base)
    got = room.cars.drive_policy(m, pol, states, T_LOOP, speeds, FOV, n, edge, THRESH, steer0=steer0, steer_clip=clip,
                                 trace=True)
    first = _host_drive(room, m, std, base, n, states, speeds, steer0, T_LOOP, edge, got,
                        lambda scans: pol.predict_many(np.ascontiguousarray(scans)).astype(np.float32),
                        steer_of=lambda a: np.clip(a.astype(np.float64), -clip, clip) if clip else a.astype(np.float64))
    assert (first >= 0).any() and (first < 0).sum() >= 8, first


def _race_states(n_races, group, seed):
    """Races in the middle of the room, cars within 1.5 m of their race's centre; the last car of every race starts
    side-on 3 cm from the west wall (it crashes at tick 0 and stays in the race as a wreck)."""
    rng = np.random.default_rng(seed)
    N = n_races * group
    states = np.zeros((n_races, group, 11))
    centres = rng.uniform(3.0, 7.0, (n_races, 1, 2))
    states[:, :, :2] = centres + rng.uniform(-1.5, 1.5, (n_races, group, 2))
    states[:, :, 2] = rng.uniform(-math.pi, math.pi, (n_races, group))
    speeds = rng.uniform(1.0, 4.0, (n_races, group))
    states[:, :, 3] = rng.uniform(0.0, 1.0, (n_races, group)) * speeds
    states[:, -1, :4] = np.stack([np.full(n_races, 0.08), rng.uniform(2.0, 8.0, n_races), np.full(n_races, math.pi / 2),
                                  np.zeros(n_races)], -1)
    return states, speeds, rng.uniform(-0.2, 0.2, (n_races, group)).astype(np.float32), N


@pytest.mark.parametrize("n", [65, 720, 1280])
def test_loop_race_followgap(room, n):
    """Two races of 3 cars and one of 8 against the loop composed from calc_range_fan_cars, the oracle's crash test and
    the oracle's FollowGap; the literal RM at 720 beams, RMGPU with noise at 65 and 1280.  1280 beams fill
    race_fan_kernel's fan_cs[RACE_MAX_RAYS]."""
    kind, std = ("RM", 0.0) if n == 720 else ("RMGPU", 0.05)           # (noise on: the offset walks by t R n here too)
    assert n <= CS.MAX_RAYS and CS.rows_of(n) in (2, 12, 20)
    m = room.m[kind]
    edge = support.edge(n)
    firsts = []
    for n_races, group, seed in ((2, 3, 7 + n), (1, 8, 8 + n)):
        states, speeds, steer0, N = _race_states(n_races, group, seed)
        base = 3 * N * n + 11
        m.set_noise(std, 99, base)
        got = _flat(room.cars.race_followgap(m, room.fg, states, T_LOOP, speeds, FOV, n, edge, THRESH, steer0=steer0,
                                             trace=True))
        first = _host_drive(room, m, std, base, n, states.reshape(N, 11), speeds.reshape(N), steer0.reshape(N), T_LOOP,
                            edge, got, lambda scans: np.array([room.followgap(s) for s in scans], np.float32),
                            scan=lambda poses, cur: m.calc_range_fan_cars(poses, cur[:, :3], group, FOV, n))
        assert (first.reshape(n_races, group)[:, -1] == 0).all(), first   # the wall cars: wrecks from tick 0
        firsts.append(first)
    assert (np.concatenate(firsts) < 0).any(), firsts


@pytest.mark.parametrize("kind,variant", [("RMGPU", 1), ("RM", 3)])
@pytest.mark.parametrize("nb", [65, 1280])
def test_fan_cars_equal_the_oracle_on_the_stamped_grid(oracle_mod, kind, variant, nb):
    """calc_range_fan_cars (the race loop's reference above) against stamp-and-scan at 65 and 1280 beams, group 4."""
    assert nb not in (360, 1081) and CS.MIN_RAYS <= nb <= CS.MAX_RAYS        # (the sizes test_gpu_race.py pins it at)
    g = DC.race_maze()
    dt = oracle_mod.edt(g.occ)
    m = (range_libc.PyRayMarching if kind == "RM" else range_libc.PyRayMarchingGPU)(range_libc.PyOMap(g), MRX)
    m.set_option("variant", variant)
    group = 4
    cars = DC.race_clusters(g, dt, 3, group, 13)
    poses = support.lidar_poses(cars)
    N = poses.shape[0]
    hits, steps = np.empty((N * nb, 2), np.int32), np.empty(N * nb, np.uint16)
    outs = m.calc_range_fan_cars(poses, cars, group, FOV, nb, hit_cells=hits, steps=steps)
    cells = RS.outline_cells(cars, RC.DEFAULT_CAR["length"], RC.DEFAULT_CAR["width"], g.resolution, g.origin, g.rows,
                            g.cols, oracle_mod.sincosf)
    want_r, want_h, want_s = DC.race_oracle_fan(oracle_mod, g, cells, group, poses, nb, variant == 3,
                                            0.999 if kind == "RM" else 1.0)
    assert same_bits(outs, want_r) and same_bits(hits, want_h.reshape(-1, 2)) and same_bits(steps, want_s)
    plain = np.empty(N * nb, np.float32)
    m.calc_range_fan(poses, plain, FOV, nb)
    assert (outs != plain).sum() > 10                                  # the other cars are seen


# ---------------------------------------------------------------- C. beyond one 64-lane workgroup
@pytest.fixture(scope="module")
def maze():
    g = maps.make_maze(256, cell=40, wall=3, p=0.45, seed=11)
    omap = range_libc.PyOMap(g)
    return {"g": g, "omap": omap, "dt": omap.distance_transform(), "m": range_libc.PyRayMarchingGPU(omap, MRX),
            "cars": RC.CarBatch(), "fg": support.followgap()}


@pytest.mark.parametrize("source", ["fg", "random"])
@pytest.mark.parametrize("K", CS.TREE_COUNTS)
def test_trees_beyond_one_workgroup(maze, K, source):
    """mcts_start / select / backup / best and the planner's rollout_kernel at blockIdx.x >= 1."""
    assert K > 64 and max(CS.ALONE_TREES) < max(CS.TREE_COUNTS) and (K + 63) // 64 >= 2
    cars, m, h = maze["cars"], maze["m"], maze["fg"] if source == "fg" else None
    n_it, nb, std, base = 10, 65, 0.05, 4242
    shape = dict(num_rays=nb, rollout_steps=20, action_every=10)
    states, actions, seeds = MC.roots(maze["g"], maze["dt"], K, 200 + K)
    pl, trees, best = MC.device(cars, m, std, base, source, h, states, actions, seeds, n_it, **shape)
    pl.close()
    stmt, snaps = MC.replay(cars, m, std, base, source, h, states, actions, seeds, n_it, trees, (n_it,), **shape)
    for k in range(K):
        MC.assert_tree(trees[k], snaps[n_it][k], (source, K, k))
        a, v = stmt[k].best()
        assert best[1][k] == v and same_bits(best[0][k:k + 1], np.array([a])) and best[2][k] == n_it + 1, (K, k)
    # a tree alone with its seed equals its copy in the batch (noise off: the ray ids depend on K)
    alone = [k for k in CS.ALONE_TREES if k < K]
    assert alone and min(alone) >= 64
    pl, batch, _ = MC.device(cars, m, 0.0, 0, source, h, states, actions, seeds, n_it, **shape)
    pl.close()
    for k in alone:
        pl, one, _ = MC.device(cars, m, 0.0, 0, source, h, states[k:k + 1], actions[k:k + 1], seeds[k:k + 1], n_it,
                                **shape)
        pl.close()
        MC.assert_tree(one[0], batch[k], ("alone", K, k))
    m.set_noise(0.0, 0, 0)


def test_drive_cars_beyond_one_workgroup(room):
    """rl_mcts_drive with 70 cars (mcts_advance_kernel at blockIdx.x = 1): car 66 starts inside the wall margin, car 68
    drives into the west wall; both freeze, and the whole batch equals the host-composed loop."""
    K, D, I, S_, nb = 70, 3, 3, 2, 65
    assert K > 64
    rng = np.random.default_rng(70)
    states = np.zeros((K, 11))
    states[:, 0], states[:, 1] = rng.uniform(2.5, 7.5, K), rng.uniform(2.5, 7.5, K)
    states[:, 2], states[:, 3] = rng.uniform(-math.pi, math.pi, K), rng.uniform(0.0, 3.0, K)
    states[66, :4] = (0.09, 5.0, math.pi / 2, 0.0)                     # side-on, 4 cm from the west wall
    states[68, :4] = (0.05 + 0.22 + D_BASE, 6.0, math.pi, 7.0)         # lidar 22 cm from the wall, at 7 m/s
    recent = rng.uniform(-0.3, 0.3, K)
    seeds = rng.integers(0, 2 ** 63, K, dtype=np.uint64)
    world = {"cars": room.cars, "g": room.g, "dt": None}
    first, out, rec, actions, visits, trace = MC.loop_case(
        world, room.m["RMGPU"], 0.05, "fg", room.fg, K, S_, D, I, num_rays=nb, rollout_steps=MC.DRIVE_L,
        starts=(states, recent, seeds), is_crashed=room.O.is_crashed)
    assert first[66] == 0 and 1 <= first[68] < D and (first[:64] < 0).any(), first
    for k in (66, 68):
        d = int(first[k])
        assert np.isnan(actions[k, d:]).all() and (visits[k, d:] == -1).all() and np.isnan(trace[k, d:]).all()
        assert np.isfinite(actions[k, :d]).all() and (visits[k, :d] >= 1).all()
    assert same_bits(out[66], states[66]) and same_bits(rec[66], recent[66])
    d = int(first[68]) - 1                                             # frozen in the state its last live decision stepped to
    _, want, _ = room.cars.rollout(trace[68, d][None, :], np.array([[[MC.SPEED, actions[68, d]]]]), n_steps=S_,
                                   action_every=S_)
    assert same_bits(out[68], want[0]) and rec[68] == np.clip(actions[68, d], -MC.CLIP, MC.CLIP)
    # the one-hot table of part A on the cars beyond the first workgroup alone: the table is per call, so this is a second
    # call with the same seeds, and every car is crashed at decision 0
    tail = slice(64, K)
    n_tail = K - 64
    edge = CS.one_hot_edge(nb, nb - 1)
    pl = MC.planner(room.cars, room.m["RMGPU"], n_tail, I, "fg", room.fg, num_rays=nb, edge=edge)
    try:
        f2, out2, rec2, act2, vis2 = pl.drive(states[tail], recent[tail], seeds[tail], D, I, steps_per_decision=S_,
                                              steer_clip=MC.CLIP)
    finally:
        pl.close()
    assert (f2 == 0).all() and np.isnan(act2).all() and (vis2 == -1).all()
    assert same_bits(out2, states[tail]) and same_bits(rec2, recent[tail])


# ---------------------------------------------------------------- D. roll-out lengths
@pytest.fixture(scope="module")
def big_room():
    g = maps.make_room(CS.BIG_ROOM)
    omap = range_libc.PyOMap(g)
    return {"m": range_libc.PyRayMarchingGPU(omap, MRX), "cars": RC.CarBatch()}


@pytest.mark.parametrize("L,every", CS.ROLLOUT_SHAPES)
def test_rollout_lengths(big_room, L, every):
    """mcts_pairwise_sum's regimes n < 8, 8 ... 128, 129 ... 256 and 257 ... 512 through the planner, and n_act =
    ceil(L / every) with a short last action; the statement replay's own roll-outs reach the regime (asserted here on
    the replay, and in tests/test_consumer_shapes_host.py with the reference's compiled Car)."""
    cars, m = big_room["cars"], big_room["m"]
    K, n_it, nb = CS.ROLLOUT_K, CS.ROLLOUT_ITERS, CS.ROLLOUT_RAYS
    assert 1 <= L <= 512
    n_act = (L + every - 1) // every
    assert (n_act * every != L) == ((L, every) in ((7, 3), (128, 10), (129, 10), (257, 16), (300, 7)))
    states, actions, seeds = CS.big_room_roots()
    shape = dict(num_rays=nb, rollout_steps=L, action_every=every)
    pl, trees, best = MC.device(cars, m, 0.0, 0, "random", None, states, actions, seeds, n_it, **shape)
    pl.close()
    rollouts = []
    stmt, snaps = MC.replay(cars, m, 0.0, 0, "random", None, states, actions, seeds, n_it, trees, (n_it,),
                             rollouts=rollouts, **shape)
    CS.assert_rollout_regime(L, every, rollouts)
    for k in range(K):
        MC.assert_tree(trees[k], snaps[n_it][k], (L, every, k))
        a, v = stmt[k].best()
        assert best[1][k] == v and same_bits(best[0][k:k + 1], np.array([a])), (L, every, k)
    m.set_noise(0.0, 0, 0)


def test_rollout_length_limits(big_room):
    """rl_mcts_create refuses L = 0 and L = 513 (MCTS_MAX_STEPS = 512) and accepts both ends."""
    cars, m = big_room["cars"], big_room["m"]
    for L in (0, 513):
        with pytest.raises(_lib.ScanLibError, match="rollout_steps"):
            MCTSPlanner(cars, m, 2, 4, FOV, 65, support.edge(65), THRESH, source="random", rollout_steps=L)
    for L in (1, 512):
        MCTSPlanner(cars, m, 2, 4, FOV, 65, support.edge(65), THRESH, source="random", rollout_steps=L).close()


# ---------------------------------------------------------------- E. the crash test at other beam counts
class Crash:
    """Colombia, the poses of test_fused_crash_marks_poses_then_reduces, and one handle per method."""

    def __init__(self, oracle_mod):
        self.O = oracle_mod
        self.g = maps.load_colombia()
        self.om = oracle_mod.OracleMap.from_gridmap(self.g, MRX)
        self.omap = range_libc.PyOMap(self.g)
        self.poses = maps.sample_free_poses(self.g, max(CS.CRASH_POSES), 31, dt=self.om.dt)
        self.m = {"RMGPU": range_libc.PyRayMarchingGPU(self.omap, MRX), "RM": range_libc.PyRayMarching(self.omap, MRX),
                  "CDDT": range_libc.PyCDDTCast(self.omap, MRX, 112)}

    def ranges(self, kind, n, nb):
        p = self.poses[:n]
        if kind == "RMGPU":
            return self.om.rm_fan(p, FOV, nb, step_coeff=1.0, nthreads=8, want_hits=False, want_steps=False)[0]
        if kind == "RM":
            return self.om.rm_fan_libm(p, FOV, nb, step_coeff=0.999)[0]
        return self.om.cddt_fan(112, p, FOV, nb, nthreads=8)


@pytest.fixture(scope="module")
def crash(oracle_mod):
    return Crash(oracle_mod)


def _wide_edge(nb):
    return support.edge(nb) + 0.25       # wide car: many crashes


def _crash_cases():
    for nb in CS.CRASH_BEAMS:
        yield "RMGPU", nb
        if nb >= 64:
            yield "RM", nb
        if nb in CS.CRASH_CDDT_BEAMS:
            yield "CDDT", nb


@pytest.mark.parametrize("kind,nb", list(_crash_cases()))
def test_crash_test_at_other_beam_counts(crash, kind, nb):
    m, edge = crash.m[kind], _wide_edge(nb)
    assert kind != "RM" or nb >= 64
    for n in CS.CRASH_POSES:
        assert (n <= 512) == (n == CS.CRASH_POSES[0])
        poses = crash.poses[:n]
        r0 = crash.ranges(kind, n, nb)
        want = crash.O.is_crashed(r0, nb, n, edge, THRESH)
        assert m.check_collision_many(poses, FOV, nb, edge, THRESH) == want, (kind, nb, n)
        kept = np.empty(n * nb, np.float32)
        assert m.check_collision_many(poses, FOV, nb, edge, THRESH, ranges=kept) == want and same_bits(kept, r0)
        assert m.check_collision_many(poses, FOV, nb, np.full(nb, -100.0), THRESH) == -(n + 1)
        grp = 40 if n % 40 == 0 else 27
        assert n % grp == 0
        got = m.check_collision_groups(poses, grp, FOV, nb, edge, THRESH)
        exp = [crash.O.is_crashed(r0[k * grp * nb:(k + 1) * grp * nb], nb, grp, edge, THRESH) for k in range(n // grp)]
        assert got.tolist() == exp, (kind, nb, n)
        assert any(e > 0 for e in exp), (kind, nb, n, exp)
        # one beam decides, at both ends of the scan
        for j in (0, nb - 1):
            assert m.check_collision_many(poses, FOV, nb, CS.one_hot_edge(nb, j), THRESH) == 0, (kind, nb, n, j)


@pytest.mark.parametrize("nb", [10, 63])
def test_literal_handle_refuses_the_crash_test_below_64_beams(crash, maze, nb):
    """PyRayMarching's literal arithmetic has no kernel with a crash test below 64 beams: the call and the planner's run
    are refused (RL_ERR_UNSUPPORTED), the handles stay as they were, and 64 beams plan as the statement says."""
    assert nb < 64
    g, dt, cars, fg = maze["g"], maze["dt"], maze["cars"], maze["fg"]
    m = range_libc.PyRayMarching(maze["omap"], MRX)
    K, n_it = 4, 3
    states, actions, seeds = MC.roots(g, dt, K, 9)
    probe = maps.sample_free_poses(g, 8, 3, 4.0, dt)

    def probes():
        scan = np.empty(8 * nb, np.float32)
        m.calc_range_fan(probe, scan, FOV, nb)
        _, out, _ = cars.rollout(states, np.full((K, 1, 2), 0.1), n_steps=1, action_every=1)
        return scan, fg.eval_many(scan, nb), out

    before = probes()
    with pytest.raises(_lib.ScanLibError) as e:
        m.check_collision_many(probe, FOV, nb, support.edge(nb), THRESH)
    assert e.value.code == RL_ERR_UNSUPPORTED
    pl = MCTSPlanner(cars, m, K, n_it + 1, FOV, nb, support.edge(nb), THRESH, source="fg", followgap=fg,
                     rollout_steps=20)
    try:
        pl.reset(states, actions, seeds)
        with pytest.raises(_lib.ScanLibError) as e:
            pl.run(1)
        assert e.value.code == RL_ERR_UNSUPPORTED
        with pytest.raises(_lib.ScanLibError, match="reset"):          # rl_mcts_run cleared `ready`
            pl.run(1)
        with pytest.raises(_lib.ScanLibError, match="reset"):
            pl.run(0)
        pl.reset(states, actions, seeds)                               # ... and a reset brings the roots back
        assert (pl.best()[2] == 1).all()
    finally:
        pl.close()
    for a, b in zip(probes(), before):
        assert same_bits(a, b)
    shape = dict(num_rays=64, rollout_steps=20, action_every=10)
    pl, trees, best = MC.device(cars, m, 0.0, 0, "fg", fg, states, actions, seeds, n_it, **shape)
    pl.close()
    _, snaps = MC.replay(cars, m, 0.0, 0, "fg", fg, states, actions, seeds, n_it, trees, (n_it,), **shape)
    for k in range(K):
        MC.assert_tree(trees[k], snaps[n_it][k], ("RM at 64 beams", k))
