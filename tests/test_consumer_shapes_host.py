"""The inputs of tests/test_gpu_consumer_shapes.py checked with the references alone (no GPU), so that a pass there
means what it claims: the size list reaches every row count and every edge, the cars of the whole-loop tests do crash
and do steer differently, the roll-out lengths reach the regime of the reward sum they were chosen for, the crash-test
batches hold groups whose first crash is past their first pose, and the generalised helpers of the closed-loop test files still default to the
shapes their own tests run.

The roll-out velocities of part D come from the reference's compiled Car (oracle/reference.py) driving the
statement's trees in an empty room where nothing crashes; the GPU test asserts the same condition again on its own
replay before it compares."""
import inspect
import math

import numpy as np
import pytest

import consumer_shapes as CS
import mcts_checks as MC
import mcts_statement as S
import support
from oracle import reference
from pyracecarsimulator_amd import maps
from pyracecarsimulator_amd import racecar as RC

MAX_STEER, MAX_SPEED = RC.DEFAULT_CAR["max_steer_ang"], RC.DEFAULT_CAR["max_speed"]


def test_size_list_reaches_every_row_count_and_edge():
    rows = {CS.rows_of(n) for n in CS.SIZES}
    assert rows == set(range(1, CS.FG_ROWS + 1))
    assert min(CS.SIZES) == CS.MIN_RAYS == 10 and max(CS.SIZES) == CS.MAX_RAYS == 1280
    assert all(CS.MIN_RAYS <= n <= CS.MAX_RAYS for n in CS.SIZES) and 1081 not in CS.SIZES
    for r in range(2, CS.FG_ROWS + 1):
        family = [n for n in CS.SIZES if CS.rows_of(n) == r]
        assert any(n == 64 * r or n == 64 * (r - 1) + 1 for n in family), (r, family)
        assert CS.ROW_SIZES[r] in family and CS.rows_of(CS.ROW_SIZES[r]) == r
    assert {10, 11, 63, 64} <= set(CS.SIZES)                       # row 1: both edges of the range and of the row
    assert set(CS.EDGE_SIZES) <= set(CS.SIZES)
    # full last rows and single-beam last rows both occur, at the first and the last row count that can hold them
    assert {64, 1280} <= {n for n in CS.SIZES if n % 64 == 0} and {65, 1217} <= {n for n in CS.SIZES if n % 64 == 1}
    for n, in_start in CS.NN_SIZES:
        assert in_start + 720 <= n <= CS.MAX_RAYS
    assert len({CS.rows_of(n) for n, _ in CS.NN_SIZES}) == 5 and set(CS.NN_CLIPPED) <= {n for n, _ in CS.NN_SIZES}
    assert CS.R_CARS == 2 * CS.DRIVE_CARS + 3


def test_one_hot_beams_sit_on_the_row_edges():
    for n in CS.SIZES:
        js, rows = CS.one_hot_beams(n), CS.rows_of(n)
        assert all(0 <= j < n for j in js) and {0, n - 1, 64 * (rows - 1)} <= set(js)
        assert rows == 1 or {63, 64 * (rows - 1) - 1} <= set(js)
        for j in js + (None,):
            edge = CS.one_hot_edge(n, j)
            assert edge.dtype == np.float64 and edge.shape == (n,) and (edge == 100.0).sum() == (j is not None)
            # any range a scan can return (0 ... 15 m) crashes at beam j alone
            for r in (0.0, 15.0):
                hit = (np.full(n, r) - edge) < CS.THRESH
                assert hit.tolist() == [k == j for k in range(n)]


def test_whole_loop_cars_crash_and_steer_differently(oracle_mod):
    """Part B's starts, with the oracle's scans from the start poses: the wall cars are crashed, at least eight cars
    are not, and the live cars' FollowGap answers take at least three values, not all at the clamp."""
    g = maps.make_room(CS.ROOM)
    om = oracle_mod.OracleMap.from_gridmap(g, 300)
    for n in CS.SIZES:
        kind, std = CS.room_method(n)
        assert kind == ("RMGPU" if CS.rows_of(n) % 2 else "RM")
        states, speeds, steer0 = CS.room_starts(n)
        assert states.shape == (CS.R_CARS, 11) and steer0.dtype == np.float32 and len(set(CS.WALL_CARS)) == 6
        assert {r // CS.DRIVE_CARS for r in CS.WALL_CARS} == {0, 1, 2}
        poses = support.lidar_poses(states)
        if kind == "RMGPU":
            scans = om.rm_fan(poses, CS.FOV, n, step_coeff=1.0)[0]
        else:
            scans = om.rm_fan_libm(poses, CS.FOV, n, step_coeff=0.999)[0]
        scans = scans.reshape(CS.R_CARS, n)
        edge = support.oracle_edge(oracle_mod, n)
        crashed = np.array([oracle_mod.is_crashed(scans[r], n, 1, edge, CS.THRESH) >= 0 for r in range(CS.R_CARS)])
        assert crashed[list(CS.WALL_CARS)].all(), (n, crashed)
        assert (~crashed).sum() >= 8, (n, crashed)
        answers = np.array([oracle_mod.followgap_eval(scans[r], 15.0, MAX_STEER, 0.004)
                            for r in np.nonzero(~crashed)[0]], np.float32)
        assert np.unique(answers).size >= 3, (n, answers)
        assert (np.abs(answers) < np.float32(MAX_STEER)).any(), (n, answers)


def _reference_rollouts(L, every):
    """The statement's trees of part D driven by the reference's compiled Car (nothing crashes): every roll-out the
    statement asks for, as (crash index, velocities)."""
    reference.require()
    ref = reference.RefCar()
    n_act = (L + every - 1) // every
    states, actions, seeds = CS.big_room_roots()
    K = len(states)
    trees = [S.Tree(states[k].copy(), support.lidar_poses(states[k]), math.nan, float(actions[k]), int(seeds[k]),
                    source="random") for k in range(K)]
    rollouts = []

    def act_many(i, reqs):
        out = []
        for _, node, a in reqs:
            st = ref.step(node.state, 2.0, a)
            out.append((st, support.lidar_poses(st), math.nan, False))
        return out

    def rollout_many(i, reqs, acts):
        out = []
        for k, child in reqs:
            acts_ro = S.rollout_actions(int(seeds[k]), i, n_act, MAX_STEER, MAX_SPEED)
            assert acts_ro.shape == (n_act, 2)
            ref.set_state(child.state)
            vel = np.array([ref.step(None, *acts_ro[s // every])[3] for s in range(L)])
            out.append((-(L + 1), vel))
        rollouts.extend(out)
        return out

    try:
        S.run_lockstep(trees, CS.ROLLOUT_ITERS, act_many, rollout_many)
        far = max(np.abs(nd.state[:2] - CS.BIG_ROOM * 0.05 / 2).max() for t in trees for nd in t.nodes)
    finally:
        ref.close()
    assert all(len(t.nodes) == CS.ROLLOUT_ITERS + 1 for t in trees)
    return rollouts, far


@pytest.mark.parametrize("L,every", CS.ROLLOUT_SHAPES)
def test_rollout_lengths_reach_their_regime(L, every):
    """n = L at each of 1, 7, 128, 129, 257, 300 and 512; beyond 256 the second-level split shows in a sum's bits.
    L steps at the car's top speed from within 3 m of the centre stay inside the big room."""
    assert [s[0] for s in CS.ROLLOUT_SHAPES] == [1, 7, 128, 129, 257, 300, 512]
    regimes = [0 if l < 8 else 1 if l <= 128 else 2 if l <= 256 else 3 for l, _ in CS.ROLLOUT_SHAPES]
    assert regimes == [0, 0, 1, 2, 3, 3, 3]
    assert 3.0 * math.sqrt(2) + (512 + 1) * 0.01 * MAX_SPEED < CS.BIG_ROOM * 0.05 / 2 - 1.0
    rollouts, far = _reference_rollouts(L, every)
    assert len(rollouts) == CS.ROLLOUT_K * CS.ROLLOUT_ITERS
    CS.assert_rollout_regime(L, every, rollouts)


def test_capped_pairwise_sum_is_numpys_at_full_depth():
    rng = np.random.default_rng(4)
    differ = 0
    for n in (0, 1, 7, 8, 9, 127, 128, 129, 130, 200, 248, 256, 257, 264, 300, 511, 512):
        v = rng.uniform(0.0, 7.0, n)
        assert CS.pairwise_sum_capped(v, 3) == S.pairwise_sum(v) == float(np.add.reduce(v)), n
        assert n > 128 or CS.pairwise_sum_capped(v, 0) == S.pairwise_sum(v)
        # (a second split starts where the larger half exceeds 128: n = 249, since the first half is cut to a multiple of 8)
        assert n > 248 or CS.pairwise_sum_capped(v, 1) == S.pairwise_sum(v)
        differ += n > 256 and CS.pairwise_sum_capped(v, 1) != S.pairwise_sum(v)
    assert differ >= 1


def test_crash_batches_hold_groups_crashed_past_their_first_pose(oracle_mod):
    """Part E's poses and widened outline table on the oracle's ranges: each batch has a crashed pose, and some group's
    first crashed pose is not its first pose (the table of -100 m gives the free batches)."""
    g = maps.load_colombia()
    om = oracle_mod.OracleMap.from_gridmap(g, 300)
    poses = maps.sample_free_poses(g, max(CS.CRASH_POSES), 31, dt=om.dt)
    assert CS.CRASH_POSES == (200, 513) and set(CS.CRASH_CDDT_BEAMS) <= set(CS.CRASH_BEAMS)
    for nb in CS.CRASH_BEAMS:
        edge = support.oracle_edge(oracle_mod, nb) + 0.25
        for n in CS.CRASH_POSES:
            r0 = om.rm_fan(poses[:n], CS.FOV, nb, step_coeff=1.0, nthreads=8, want_hits=False, want_steps=False)[0]
            grp = 40 if n % 40 == 0 else 27
            assert n % grp == 0
            exp = [oracle_mod.is_crashed(r0[k * grp * nb:(k + 1) * grp * nb], nb, grp, edge, CS.THRESH)
                   for k in range(n // grp)]
            assert oracle_mod.is_crashed(r0, nb, n, edge, CS.THRESH) >= 0, (nb, n)
            assert any(e > 0 for e in exp), (nb, n, exp)


def test_generalised_helpers_default_to_their_files_shapes():
    """The keyword arguments of the closed-loop helpers (tests/mcts_checks.py) default to the constants tests/test_gpu_mcts.py
    and tests/test_gpu_mcts_drive.py run with; the edge table (tests/support.py) takes its beam count from the caller."""

    def defaults(fn):
        return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}

    assert (MC.B, MC.L, MC.DRIVE_L, MC.EVERY) == (1081, 200, 40, 10)
    assert defaults(support.edge) == {"fov": 4.71}
    for fn in (MC.answers, MC.scan):
        assert defaults(fn) == {"num_rays": 1081}
    for fn in (MC.replay, MC.device):
        d = defaults(fn)
        assert (d["num_rays"], d["rollout_steps"], d["action_every"], d["edge"]) == (1081, 200, 10, None), fn
    assert defaults(MC.replay)["is_crashed"] is RC.is_crashed
    for fn in (MC.planner, MC.loop_case):
        d = defaults(fn)
        assert (d["num_rays"], d["rollout_steps"], d["action_every"], d["edge"]) == (1081, 40, 10, None), fn
    d = defaults(MC.host_loop)
    assert (d["num_rays"], d["rollout_steps"], d["edge"], d["is_crashed"]) == (1081, 40, None, RC.is_crashed)
    assert defaults(MC.scan_keep) == {"num_rays": 1081} and defaults(MC.loop_case)["starts"] is None
