"""Batched multi-car races on the MI355X (rl_car_outline_cells, rl_calc_range_fan_cars, rl_car_race_followgap and
their Python forms): the outline raster against tests/race_statement.py, the race scan against the oracle on the
stamped grid and against the handle's own scan of a stamped map, the race loop against rl_car_drive_followgap and
against a teacher-forced replay of every link, crashes between cars, chunking, errors and the façade."""
import math

import numpy as np
import pytest

import race_statement as RS
import support
from drive_cases import RACE_MRX as MRX, race_clusters, race_maze, race_oracle_fan, race_teacher_forced_replay
from support import D_BASE, FOV, THRESH, same_bits
from pyracecarsimulator_amd import RacecarSimulator, _lib, maps, range_libc
from pyracecarsimulator_amd import racecar as RC

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

B = 1081
L, W = RC.DEFAULT_CAR["length"], RC.DEFAULT_CAR["width"]
RL_ERR_INVALID, RL_ERR_UNSUPPORTED = -1, -4           # include/scanlib.h rl_status


def test_outline_cells_equal_the_statement(oracle_mod):
    """About 10 000 random cars on colombia and on a yawed maze: the device's counts and cells equal the statement's
    sequence (RS.outline_sequence) element for element."""
    cars_h = RC.CarBatch()
    rng = np.random.default_rng(1)
    col = maps.load_colombia()
    yawed = race_maze()
    yawed = maps.GridMap(yawed.occ, yawed.resolution, (3.1, -2.7, 0.61), "yawed")
    for g, n in ((col, 6000), (yawed, 4000)):
        omap = range_libc.PyOMap(g)
        lo = np.array([g.origin[0], g.origin[1]]) - 2.0
        span = max(g.rows, g.cols) * g.resolution + 4.0
        cars = np.stack([lo[0] + rng.uniform(-span, span, n), lo[1] + rng.uniform(-span, span, n),
                         rng.uniform(-7.0, 7.0, n)], -1)
        cells, counts = cars_h.outline_cells(omap, cars)
        want = RS.outline_sequence(cars, L, W, g.resolution, g.origin, g.rows, g.cols, oracle_mod.sincosf)
        n_some = 0
        for i in range(n):
            assert counts[i] == len(want[i]), (g.name, i)
            assert (cells[i, counts[i]:] == -1).all()
            assert np.array_equal(cells[i, :counts[i]], want[i]), (g.name, i)
            n_some += counts[i] > 0
        assert n_some > n // 10, g.name


@pytest.mark.parametrize("kind,variant", [("RM", 3), ("RM", 1), ("RMGPU", 1)])
def test_fan_cars_equal_the_oracle_on_the_stamped_grid(oracle_mod, kind, variant):
    g = race_maze()
    dt = oracle_mod.edt(g.occ)
    omap = range_libc.PyOMap(g)
    m = (range_libc.PyRayMarching if kind == "RM" else range_libc.PyRayMarchingGPU)(omap, MRX)
    m.set_option("variant", variant)
    coeff = 0.999 if kind == "RM" else 1.0
    nb = 360
    n_changed = 0
    for group, n_groups, seed in ((1, 3, 11), (2, 4, 12), (4, 3, 13), (8, 2, 14)):
        cars = race_clusters(g, dt, n_groups, group, seed)
        poses = support.lidar_poses(cars)
        N = poses.shape[0]
        hits = np.empty((N * nb, 2), np.int32)
        steps = np.empty(N * nb, np.uint16)
        outs = m.calc_range_fan_cars(poses, cars, group, FOV, nb, hit_cells=hits, steps=steps)
        cells = RS.outline_cells(cars, L, W, g.resolution, g.origin, g.rows, g.cols, oracle_mod.sincosf)
        want_r, want_h, want_s = race_oracle_fan(oracle_mod, g, cells, group, poses, nb, variant == 3, coeff)
        assert same_bits(outs, want_r), (group, kind, variant)
        assert same_bits(hits, want_h.reshape(-1, 2)), (group, kind, variant)
        assert same_bits(steps, want_s), (group, kind, variant)
        plain = np.empty(N * nb, np.float32)
        m.calc_range_fan(poses, plain, FOV, nb)
        if group == 1:
            assert same_bits(outs, plain)
        else:
            n_changed += int((outs != plain).sum())
    assert n_changed > 100


@pytest.mark.parametrize("kind", ["RM", "RMGPU"])
def test_fan_cars_with_noise_equal_a_stamped_map(oracle_mod, kind):
    """Noise on: each pose's race scan equals the same handle's ordinary scan of a second map with the other cars laid
    by PyOMap.stamp_cells (the noise at the same global ray id); group 1 equals calc_range_fan."""
    g = race_maze()
    dt = oracle_mod.edt(g.occ)
    cls = range_libc.PyRayMarching if kind == "RM" else range_libc.PyRayMarchingGPU
    m = cls(range_libc.PyOMap(g), MRX)
    omap2 = range_libc.PyOMap(g)
    m2 = cls(omap2, MRX)
    base = 777 * B
    m.set_noise(0.05, 9, base)
    group, n_groups = 4, 3
    cars = race_clusters(g, dt, n_groups, group, 31)
    poses = support.lidar_poses(cars)
    outs = m.calc_range_fan_cars(poses, cars, group, FOV, B)
    cells = RS.outline_cells(cars, L, W, g.resolution, g.origin, g.rows, g.cols, oracle_mod.sincosf)
    for p in range(poses.shape[0]):
        omap2.stamp_cells(RS.others(cells, group, p).astype(np.int64))
        m2.set_noise(0.05, 9, base + p * B)
        one = np.empty(B, np.float32)
        m2.calc_range_fan(poses[p:p + 1], one, FOV, B)
        assert same_bits(outs[p * B:(p + 1) * B], one), p
    outs1 = m.calc_range_fan_cars(poses, cars, 1, FOV, B)
    plain = np.empty(poses.shape[0] * B, np.float32)
    m.calc_range_fan(poses, plain, FOV, B)
    assert same_bits(outs1, plain)


def _race_starts(g, dt, n_races, group, seed, spread=0.9):
    cars = race_clusters(g, dt, n_races, group, seed, spread)
    rng = np.random.default_rng(seed)
    states = np.zeros((n_races * group, 11))
    states[:, :3] = cars
    speeds = rng.uniform(1.0, 4.0, n_races * group)
    states[:, 3] = rng.uniform(0.0, 1.0, n_races * group) * speeds
    return states.reshape(n_races, group, 11), speeds.reshape(n_races, group)


def test_race_of_one_equals_drive_followgap(oracle_mod):
    g = maps.load_colombia()
    dt = oracle_mod.edt(g.occ)
    m = range_libc.PyRayMarchingGPU(range_libc.PyOMap(g), MRX)
    fg = support.followgap()
    states, speeds = _race_starts(g, dt, 48, 1, 41)
    steer0 = np.random.default_rng(2).uniform(-0.2, 0.2, (48, 1)).astype(np.float32)
    cars = RC.CarBatch()
    m.set_noise(0.03, 5, 1000)
    race = cars.race_followgap(m, fg, states, 80, speeds, FOV, B, support.edge(B), THRESH, steer0=steer0, trace=True)
    drive = cars.drive_followgap(m, fg, states[:, 0], 80, speeds[:, 0], FOV, B, support.edge(B), THRESH,
                                 steer0=steer0[:, 0], trace=True)
    m.set_noise(0.0, 0, 0)
    for a, b in zip(race, drive):
        assert same_bits(a.reshape(b.shape), b)


@pytest.mark.parametrize("kind,group", [("RMGPU", 2), ("RM", 4)])
def test_race_teacher_forced_replay(oracle_mod, kind, group):
    """Every link of every tick of a race: the step (rollout of one step), the outline statement of the other cars at
    their states after that tick's step (wrecks at their crash-tick state), the oracle scan of the stamped grid, the
    crash test and FollowGap."""
    g = race_maze()
    dt = oracle_mod.edt(g.occ)
    m = (range_libc.PyRayMarching if kind == "RM" else range_libc.PyRayMarchingGPU)(range_libc.PyOMap(g), MRX)
    n_races, T = 4, 50
    states, speeds = _race_starts(g, dt, n_races, group, 50 + group)
    race_teacher_forced_replay(oracle_mod, g, m, kind == "RM", RC.CarBatch(), support.followgap(), states, speeds, T, B,
                               support.edge(B), L, W)


def _room_race(m, fg, states, speeds, T):
    return RC.CarBatch().race_followgap(m, fg, states, T, speeds, FOV, B, support.edge(B), THRESH, trace=True)


def test_head_on_and_wreck():
    """An empty 10 m walled room.  Two cars nose to nose at 3 m/s both crash before any wall is within reach, and
    neither crashes alone.  A car driven into a wall stays a wreck that the car following it crashes into."""
    g = maps.make_room(200)
    m = range_libc.PyRayMarchingGPU(range_libc.PyOMap(g), MRX)
    fg = support.followgap()
    T = 40
    s = np.zeros((1, 2, 11))
    s[0, 0, :4] = (4.4, 5.0, 0.0, 3.0)
    s[0, 1, :4] = (5.6, 5.0, math.pi, 3.0)
    sp = np.full((1, 2), 3.0)
    first = _room_race(m, fg, s, sp, T)[0]
    assert (first >= 0).all() and (first < 20).all(), first
    alone = _room_race(m, fg, s.reshape(2, 1, 11), sp.reshape(2, 1), T)[0]
    assert (alone < 0).all(), alone
    # wall then follower: A 0.35 m from the east wall at 3 m/s, B 0.75 m behind it
    s = np.zeros((1, 2, 11))
    s[0, 0, :4] = (9.3, 5.0, 0.0, 3.0)
    s[0, 1, :4] = (8.55, 5.0, 0.0, 3.0)
    first, final, vel, steers, poses, st = _room_race(m, fg, s, sp, 60)
    a, b = int(first[0, 0]), int(first[0, 1])
    assert 0 <= a < b, first
    alone_b = _room_race(m, fg, s[:, 1:], sp[:, 1:], 60)[0]
    assert alone_b[0, 0] < 0 or alone_b[0, 0] > b, (alone_b, b)
    assert final[0, 1, 0] < final[0, 0, 0]             # B stopped behind A's wreck
    assert same_bits(final[0, 0], st[0, 0, a])        # the wreck stayed at its crash-tick state


def test_race_chunking_is_invariant(oracle_mod):
    """T ticks in one call == T/2 + T/2 with states, steers and the noise offset chained, for every race whose cars
    are all alive after the first half (a wreck would be stepped again by a second call)."""
    g = race_maze()
    dt = oracle_mod.edt(g.occ)
    m = range_libc.PyRayMarchingGPU(range_libc.PyOMap(g), MRX)
    fg = support.followgap()
    n_races, P, T, H = 32, 2, 60, 30
    states, speeds = _race_starts(g, dt, n_races, P, 71, spread=1.5)
    edge = support.edge(B)
    cars = RC.CarBatch()
    base = 4242
    m.set_noise(0.05, 3, base)
    whole = cars.race_followgap(m, fg, states, T, speeds, FOV, B, edge, THRESH, trace=True)
    a = cars.race_followgap(m, fg, states, H, speeds, FOV, B, edge, THRESH, trace=True)
    ok = (a[0] < 0).all(1)
    st0 = np.where(a[0] < 0, a[3][..., -1], np.float32(0.0)).astype(np.float32)
    m.set_noise(0.05, 3, base + H * n_races * P * B)
    b = cars.race_followgap(m, fg, a[1], T - H, speeds, FOV, B, edge, THRESH, steer0=st0, trace=True)
    m.set_noise(0.0, 0, 0)
    assert ok.sum() >= 4
    for k in range(2, 6):
        assert same_bits(whole[k][:, :, :H], a[k]), k
    assert same_bits(whole[1][ok], b[1][ok])
    for k in range(2, 6):
        assert same_bits(whole[k][ok][:, :, H:], b[k][ok]), k
    want_first = np.where(b[0][ok] >= 0, b[0][ok] + H, -(T + 1))
    assert (whole[0][ok] == want_first).all()


def test_errors_leave_handles_usable(oracle_mod):
    g = race_maze()
    dt = oracle_mod.edt(g.occ)
    omap = range_libc.PyOMap(g)
    cars = race_clusters(g, dt, 2, 2, 3)
    poses = support.lidar_poses(cars)
    for cls, args in ((range_libc.PyCDDTCast, (112,)), (range_libc.PyGiantLUTCast, (112,)),
                      (range_libc.PyBresenhamsLine, ())):
        h = cls(omap, MRX, *args)
        with pytest.raises(_lib.ScanLibError) as e:
            h.calc_range_fan_cars(poses, cars, 2, FOV, 90)
        assert e.value.code == RL_ERR_UNSUPPORTED and "ray marching" in str(e.value)
        out = np.empty(4 * 90, np.float32)
        h.calc_range_fan(poses, out, FOV, 90)                  # still usable
    m = range_libc.PyRayMarchingGPU(omap, MRX)
    want = m.calc_range_fan_cars(poses, cars, 2, FOV, 90)
    for group, nb in ((0, 90), (9, 90), (2, 9), (2, 1281)):
        with pytest.raises((_lib.ScanLibError, ValueError)) as e:
            m.calc_range_fan_cars(np.repeat(poses, 9, 0)[:18] if group == 9 else poses,
                                  np.repeat(cars, 9, 0)[:18] if group == 9 else cars, group, FOV, nb)
        if isinstance(e.value, _lib.ScanLibError):
            assert e.value.code == RL_ERR_INVALID
    # too many outline points: a 30 m car at 0.05 m per cell
    with pytest.raises(_lib.ScanLibError) as e:
        m.calc_range_fan_cars(poses, cars, 2, FOV, 90, length=30.0)
    assert e.value.code == RL_ERR_UNSUPPORTED
    # null pointers through the C ABI
    assert _lib.lib().rl_calc_range_fan_cars(m._h, None, None, 2, 2, L, W, FOV, 90, None, None, None) == RL_ERR_INVALID
    fg = support.followgap()
    cb = RC.CarBatch()
    assert _lib.lib().rl_car_race_followgap(cb._h, m._h, fg._h, None, None, None, 2, 2, 10, 0.01, D_BASE, FOV, B,
                                            None, THRESH, None, None, None, None, None, None) == RL_ERR_INVALID
    st = np.zeros((2, 9, 11))
    with pytest.raises(_lib.ScanLibError):
        cb.race_followgap(m, fg, st, 5, 1.0, FOV, B, support.edge(B), THRESH)
    assert same_bits(m.calc_range_fan_cars(poses, cars, 2, FOV, 90), want)
    assert cb.outline_cells(omap, cars)[1].shape == (4,)


def test_facade_race_many(oracle_mod):
    """RacecarSimulator.raceFollowGapMany equals CarBatch.race_followgap on the façade's method, edge table and
    FollowGap (support.followgap(), as simple_driver.py builds it)."""
    g = race_maze()
    cfg = dict(RC.DEFAULT_CAR)
    cfg.update(scan_dist_to_base=D_BASE, batch_size=40, scan_beams=1080, scan_fov=FOV, scan_std=0.0,
               scan_max_range=15.0, free_thresh=0.8)
    sim = RacecarSimulator(cfg)
    omap = range_libc.PyOMap(g)
    sim.setMap(omap, g.resolution, g.origin)
    sim.setRaytracingMethod("RMGPU")
    states, _ = _race_starts(g, oracle_mod.edt(g.occ), 6, 3, 91)
    got = sim.raceFollowGapMany(states, 30, speed=2.0)
    fg = support.followgap()
    want = RC.CarBatch().race_followgap(sim.scan_simulator.scan_method, fg, states, 30, 2.0, sim.scan_fov,
                                        sim.num_rays, sim.edge_distances, sim.ttc_thresh,
                                        scan_dist_to_base=sim.scan_dist_to_base)
    assert len(got) == 4
    for a, b in zip(got, want):
        assert same_bits(a, b)
