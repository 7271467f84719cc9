"""Closed-loop Follow-the-Gap roll-outs (rl_car_drive_followgap, CarBatch.drive_followgap,
RacecarSimulator.driveFollowGapMany) on the MI355X: every link of the loop — step, lidar pose, scan, crash test,
steering — pinned against the reference's compiled Car and FollowGap and against the same loop composed from
the existing public calls."""
import ctypes as C
import math

import numpy as np
import pytest

import support
from drive_cases import assert_teacher_forced
from oracle import reference
from support import D_BASE, FOV, THRESH, same_bits, within_one_ulp
from pyracecarsimulator_amd import RacecarSimulator, _lib, maps, range_libc
from pyracecarsimulator_amd import racecar as RC

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

B = 1081


def test_drive_teacher_forced_vs_reference(oracle_mod):
    """Colombia, RMGPU, 32 cars x 150 ticks: at every live tick each link of the loop, fed the GPU's own state of
    the tick before, agrees with the reference's compiled Car / FollowGap and the oracle scan."""
    reference.require()
    g = maps.load_colombia()
    mrx = 300
    om = oracle_mod.OracleMap.from_gridmap(g, mrx)
    m = range_libc.PyRayMarchingGPU(range_libc.PyOMap(g), mrx)
    fg = support.followgap()
    R, T = 32, 150
    states, speeds = support.starts(g, om.dt, R, 3, 6.0, speed_hi=4.0)
    drive = RC.CarBatch().drive_followgap(m, fg, states, T, speeds, FOV, B, support.edge(B), THRESH, trace=True)
    assert_teacher_forced(om, states, speeds, drive, T, B)


def test_drive_equals_composed_public_calls(oracle_mod):
    """A 512^2 maze, 256 cars x 40 ticks, five range methods (noise on for RMGPU): the loop equals the same loop
    built from calc_range_fan, eval_many, is_crashed and rollout(n_steps=1), bit for bit."""
    g = maps.make_maze(512, cell=40, wall=3, p=0.45, seed=11)
    mrx = 300
    om = oracle_mod.OracleMap.from_gridmap(g, mrx)
    omap = range_libc.PyOMap(g)
    fg = support.followgap()
    R, T = 256, 40
    far, sp_far = support.starts(g, om.dt, R - 32, 21, 8.0)
    near, sp_near = support.starts(g, om.dt, 32, 22, 1.0)         # next to walls: some crash at once
    states, speeds = np.concatenate([far, near]), np.concatenate([sp_far, sp_near])
    steer0 = np.random.default_rng(5).uniform(-0.3, 0.3, R).astype(np.float32)
    edge = support.edge(B)
    cars = RC.CarBatch()
    for name, m, std in support.five_methods(omap, mrx):
        base = 7 * R * B
        m.set_noise(std, 99, base)
        first, final, vel, steers, sp, st = cars.drive_followgap(m, fg, states, T, speeds, FOV, B, edge, THRESH,
                                                                 steer0=steer0, trace=True)
        assert (first >= 0).any() and (first < 0).any(), name
        assert ((first >= 0) | (first == -(T + 1))).all(), name
        # lidar poses: numpy's f64 formula within one f32 ulp
        alive_t = np.arange(T)[None, :] <= np.where(first >= 0, first, T)[:, None]
        assert within_one_ulp(support.lidar_poses(st[alive_t]), sp[alive_t]), name
        cur = states.copy()
        steer = steer0.astype(np.float64)
        alive = np.ones(R, bool)
        last_pose = np.zeros((R, 3), np.float32)
        for t in range(T):
            # step: rollout(n_steps=1) of the live cars
            idx = np.nonzero(alive)[0]
            _, out, v1 = cars.rollout(cur[idx], np.stack([speeds[idx], steer[idx]], -1)[:, None, :], n_steps=1,
                                      action_every=1)
            assert same_bits(out, st[idx, t]) and same_bits(v1[:, 0], vel[idx, t]), (name, t)
            cur[idx] = out
            last_pose[idx] = sp[idx, t]
            # scan: every car, the frozen ones at their last pose, noise at this tick's ray offset
            ranges = np.empty(R * B, np.float32)
            m.set_noise(std, 99, base + t * R * B)
            m.calc_range_fan(last_pose, ranges, FOV, B)
            ranges = ranges.reshape(R, B)
            crashed = np.array([RC.is_crashed(ranges[r], B, 1, edge, THRESH) >= 0 for r in idx])
            assert (first[idx] == t).tolist() == crashed.tolist(), (name, t)
            go = idx[~crashed]
            a = fg.eval_many(np.ascontiguousarray(ranges[go]))
            assert same_bits(a, steers[go, t]), (name, t)
            assert np.isnan(steers[idx[crashed], t]).all()
            steer[go] = a
            alive[idx[crashed]] = False
        m.set_noise(0.0, 0, 0)
        assert same_bits(final, cur), name


def test_drive_chunking_is_invariant():
    """T ticks in one call == T/2 + T/2 with the states, the last steer and the noise offset chained."""
    g = maps.load_colombia()
    dt = range_libc.PyOMap(g).distance_transform()
    omap = range_libc.PyOMap(g)
    m = range_libc.PyRayMarchingGPU(omap, 300)
    fg = support.followgap()
    R, T, H = 64, 60, 30
    states, speeds = support.starts(g, dt, R, 8, 3.0)
    edge = support.edge(B)
    cars = RC.CarBatch()
    base = 12345
    m.set_noise(0.05, 4, base)
    whole = cars.drive_followgap(m, fg, states, T, speeds, FOV, B, edge, THRESH, trace=True)
    a = cars.drive_followgap(m, fg, states, H, speeds, FOV, B, edge, THRESH, trace=True)
    ok = a[0] < 0                                               # alive after the first half
    st0 = np.where(ok, a[3][:, -1], np.float32(0.0)).astype(np.float32)
    m.set_noise(0.05, 4, base + H * R * B)
    b = cars.drive_followgap(m, fg, a[1], T - H, speeds, FOV, B, edge, THRESH, steer0=st0, trace=True)
    m.set_noise(0.0, 0, 0)
    assert ok.any()
    # first half: identical for every car
    for k in range(2, 6):
        assert same_bits(whole[k][:, :H], a[k]), k
    assert (np.where(a[0] >= 0, a[0], -(T + 1)) == np.where(whole[0] < H, whole[0], -(T + 1))).all()
    # second half: identical for the cars alive at its start
    assert same_bits(whole[1][ok], b[1][ok])
    for k in range(2, 6):
        assert same_bits(whole[k][ok, H:], b[k][ok]), k
    want_first = np.where(b[0][ok] >= 0, b[0][ok] + H, -(T + 1))
    assert (whole[0][ok] == want_first).all()


def test_drive_crash_and_freeze(oracle_mod):
    """Three hand-built cars in an empty 10 m room: into a wall at 7 m/s, inside the margin, in open space."""
    g = maps.make_room(200)
    mrx = 300
    om = oracle_mod.OracleMap.from_gridmap(g, mrx)
    m = range_libc.PyRayMarchingGPU(range_libc.PyOMap(g), mrx)
    fg = support.followgap()
    T = 60
    states = np.zeros((3, 11))
    states[0, :4] = (9.1, 5.0, 0.0, 7.0)                         # 0.6 m from the east wall, heading at it
    states[1, :3] = (0.09, 5.0, math.pi / 2)                     # 4 cm from the west wall: inside the outline
    states[2, :3] = (5.0, 5.0, 0.3)                              # the middle of the room
    speeds = np.array([7.0, 1.0, 1.0])
    edge = support.edge(B)
    first, final, vel, steers, sp, st = RC.CarBatch().drive_followgap(m, fg, states, T, speeds, FOV, B, edge,
                                                                      THRESH, trace=True)
    assert first[1] == 0 and first[2] == -(T + 1) and 0 < first[0] < T, first
    # the wall car's crash tick from its own trace: the first lidar pose whose oracle scan is inside the outline
    k = int(first[0])
    want_r, _, _ = om.rm_fan(np.ascontiguousarray(sp[0, :k + 1]), FOV, B, step_coeff=1.0)
    assert oracle_mod.is_crashed(want_r, B, k + 1, edge, THRESH) == k
    for r in (0, 1):
        t = int(first[r])
        assert np.isnan(steers[r, t]) and np.isfinite(vel[r, t]) and np.isfinite(st[r, t]).all()
        assert np.isfinite(steers[r, :t]).all()
        for arr in (vel, steers, sp, st):
            assert np.isnan(arr[r, t + 1:]).all()
        assert same_bits(final[r], st[r, t])
    assert np.isfinite(steers[2]).all() and np.isfinite(st[2]).all() and same_bits(final[2], st[2, -1])
    assert st[0, first[0], 0] > 9.1                              # it did drive into the wall


def test_drive_errors_leave_handles_usable():
    g = maps.make_maze(512, cell=40, wall=3, p=0.45, seed=11)
    omap = range_libc.PyOMap(g)
    dt = omap.distance_transform()
    m = range_libc.PyRayMarchingGPU(omap, 300)
    fg = support.followgap()
    cars = RC.CarBatch()
    R, T = 8, 10
    states, speeds = support.starts(g, dt, R, 2, 8.0)
    edge = support.edge(B)
    poses = maps.sample_free_poses(g, 16, 3, 4.0, dt)
    m.set_noise(0.05, 7, 321)
    m.set_option("nt_store", 1)
    scan0 = np.empty(16 * B, np.float32)
    m.calc_range_fan(poses, scan0, FOV, B)
    steer0 = fg.eval_many(scan0, B)
    drive0 = cars.drive_followgap(m, fg, states, T, speeds, FOV, B, edge, THRESH)

    def still_usable():
        again = np.empty_like(scan0)
        m.calc_range_fan(poses, again, FOV, B)
        assert same_bits(again, scan0)                          # same noise offset, same ranges
        assert same_bits(fg.eval_many(scan0, B), steer0)
        assert m.get_info("nt_store") == 1

    Lb = _lib.lib()
    f64p, f32p = _lib.f64p, _lib.f32p

    def raw(R_, T_, nr, st_=states, sp_=speeds, ed=edge, h_car=cars._h, h_m=m._h, h_fg=fg._h, first=True):
        fst = np.zeros(max(R_, 1), np.int32)
        return Lb.rl_car_drive_followgap(h_car, h_m, h_fg, st_.ctypes.data_as(f64p) if st_ is not None else None,
                                         sp_.ctypes.data_as(f64p), None, R_, T_, 0.01, D_BASE, FOV, nr,
                                         ed.ctypes.data_as(f64p), THRESH,
                                         fst.ctypes.data_as(C.POINTER(C.c_int)) if first else None,
                                         None, None, None, None, None)

    def expect_error(rc):
        assert rc != 0
        with pytest.raises(_lib.ScanLibError):
            _lib.check(rc)
        still_usable()

    expect_error(raw(R, T, B, st_=None))                         # null states
    expect_error(raw(R, T, B, first=False))                      # null first_crashed
    expect_error(raw(R, T, B, h_fg=None))                        # null handle
    for T_bad in (0, -3):
        expect_error(raw(R, T_bad, B))
        with pytest.raises(_lib.ScanLibError):
            cars.drive_followgap(m, fg, states, T_bad, speeds, FOV, B, edge, THRESH)
        still_usable()
    for nr in (9, 1281):
        with pytest.raises(_lib.ScanLibError):
            cars.drive_followgap(m, fg, states, T, speeds, FOV, nr, support.edge(nr), THRESH)
        still_usable()
    # R num_rays >= 2^31 (refused before anything is read or launched)
    big = (1 << 31) // 1000 + 1
    expect_error(raw(big, 1, 1000, st_=np.zeros((big, 11)), sp_=np.ones(big), ed=support.edge(1000)))
    # multi-device handles: refused (single-device only)
    multi = RC.CarBatch(device=[0])
    with pytest.raises(_lib.ScanLibError, match="single-device"):
        multi.drive_followgap(m, fg, states, T, speeds, FOV, B, edge, THRESH)
    still_usable()
    # handles on different devices (where a second device exists)
    if _lib.lib().rl_device_count() >= 2:
        fg1 = support.followgap(device=1)
        with pytest.raises(_lib.ScanLibError, match="device"):
            cars.drive_followgap(m, fg1, states, T, speeds, FOV, B, edge, THRESH)
        still_usable()
    # python-side validation
    with pytest.raises(ValueError):
        cars.drive_followgap(m, fg, states.astype(np.float32), T, speeds, FOV, B, edge, THRESH)
    with pytest.raises(ValueError):
        cars.drive_followgap(m, fg, states, T, speeds, FOV, B, edge[:-1], THRESH)
    with pytest.raises(ValueError):
        cars.drive_followgap(m, fg, states, T, speeds, FOV, B, edge, THRESH, steer0=np.zeros(R))
    # R = 0 does nothing; the handles still drive as before
    f0 = cars.drive_followgap(m, fg, states[:0], T, speeds[:0], FOV, B, edge, THRESH)
    assert f0[0].shape == (0,)
    again = cars.drive_followgap(m, fg, states, T, speeds, FOV, B, edge, THRESH)
    for x, y in zip(drive0, again):
        assert same_bits(x, y)
    still_usable()


def test_drive_facade_matches_manual_ticks():
    """RacecarSimulator.driveFollowGapMany (R = 1, 100 ticks) against the reference's tick on the same façade:
    drive(2.0, s); updatePose(); runScan(); checkCollision() >= 0; s = fg.eval(getScan())."""
    g = maps.load_colombia()
    cfg = dict(RC.DEFAULT_CAR)
    cfg.update(scan_dist_to_base=0.275, batch_size=40, scan_beams=1080, scan_fov=4.71, scan_std=0.01,
               scan_max_range=15.0, free_thresh=0.8)              # params.yaml:28-39,44-47
    sim = RacecarSimulator(cfg)
    omap = range_libc.PyOMap(g)
    sim.setMap(omap, g.resolution, g.origin)
    sim.setRaytracingMethod("RMGPU")
    dt = omap.distance_transform()
    T = 100
    for seed in (21, 22, 23):
        st0 = np.zeros(11)
        st0[:3] = maps.sample_free_poses(g, 1, seed, 10.0, dt)[0]
        first, final, vel, steers = sim.driveFollowGapMany(st0[None, :], T, speed=2.0)
        fg = support.followgap()
        sim.setState(st0)
        s, crash = 0.0, -(T + 1)
        for t in range(T):
            sim.drive(2.0, s)
            sim.updatePose()
            sim.runScan()
            if sim.checkCollision() >= 0:
                crash = t
                break
            s = fg.eval(sim.getScan(), cfg["scan_beams"])
        assert first[0] == crash, seed
        assert np.abs(final[0, :2] - sim.getState()[:2]).max() < 1e-6, seed
        assert vel.shape == (1, T) and steers.shape == (1, T)
