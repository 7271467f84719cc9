"""The driving environment (rl_env_*, DriveEnv, RacecarSimulator.driveEnv) on the MI355X: every call against the same
tick composed from the public calls (CarBatch.rollout, calc_range_fan, is_crashed), against the closed loops it opens
(drive_followgap, drive_policy), against the statement (tests/env_statement.py) and the reference's compiled Car."""
import ctypes as C
import os

import numpy as np
import pytest

import consumer_shapes as CS
import drive_cases as DC
import env_statement as ES
import policy_statement as PS
import support
from conftest import GOLD
from oracle import reference
from support import D_BASE, FOV, THRESH, same_bits
from pyracecarsimulator_amd import DriveEnv, Policy, RacecarSimulator, _lib, maps, range_libc
from pyracecarsimulator_amd import racecar as RC

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]


def test_env_equals_composed_public_calls(oracle_mod):
    """A 256^2 maze, 70 envs x 12 steps of 3 substeps, five range methods (noise on for RMGPU at a non-zero base),
    window (7, 40, 2): states, observations, done and rewards equal the same tick built from rollout(n_steps=3),
    calc_range_fan at the slot's ray offset and is_crashed, bit for bit; frozen envs are scanned at their last pose."""
    g, states, actions = DC.maze_case(lambda g_: oracle_mod.OracleMap.from_gridmap(g_, 300).dt)
    N, B, S, T, win = 70, 100, 3, 12, (7, 40, 2)
    omap = range_libc.PyOMap(g)
    edge = support.edge(B)
    cars = RC.CarBatch()
    for name, m, std in support.five_methods(omap, 300):
        base = 7 * N * B + 13
        m.set_noise(std, 99, base)
        pub = DC.Composed(m, cars, N, B, edge, S, std, 99, base)
        env = DriveEnv(m, states, N, B, FOV, edge, THRESH, substeps=S, obs_window=win, auto_reset=False, car=cars)
        assert env.n_envs == N and env.obs_shape == (N, 40)
        obs = env.reset(seed=3, start_index=np.arange(N))
        cur = states.copy()
        ranges = pub.scan(support.lidar_poses(cur), 0)
        assert same_bits(obs, ES.observation(ranges, win, 0, 0)), name
        done = np.array([int(pub.is_crashed(r)) for r in ranges], np.int32)
        rd = env.read()
        assert same_bits(rd["states"], cur) and same_bits(rd["done"], done), name
        assert (rd["ticks"] == 0).all() and (rd["start_index"] == np.arange(N)).all()
        for k in range(1, T + 1):
            a = actions[k - 1]
            live = np.nonzero(done == 0)[0]
            obs, rew, dn = env.step(a)
            before = cur[live, 8].copy()
            _, out, _ = cars.rollout(cur[live], a[live].astype(np.float64)[:, None, :], n_steps=S, action_every=S)
            cur[live] = out
            rd = env.read()
            assert same_bits(rd["states"], cur), (name, k)
            ranges = pub.scan(support.lidar_poses(cur), k)                # every env, the frozen ones where they stand
            assert same_bits(obs, ES.observation(ranges, win, 0, 0)), (name, k)
            crashed = np.array([pub.is_crashed(ranges[e]) for e in live], bool)
            want_rew = np.zeros(N, np.float32)
            want_rew[live[~crashed]] = (cur[live, 8] - before).astype(np.float32)[~crashed]
            done[live[crashed]] = 1
            assert same_bits(dn, done) and same_bits(rd["done"], done), (name, k)
            assert same_bits(rew, want_rew), (name, k)
            assert (rd["ticks"][live] == k).all(), (name, k)
        assert (done == 1).any() and (done == 0).any(), name
        assert (done[rd["ticks"] > 0] == 1).any(), name                     # ... and not only at the reset
        m.set_noise(0.0, 0, 0)
        env.close()


def test_env_fed_followgap_equals_drive_followgap():
    """Colombia, 24 envs x 30 steps, 130 beams, noise on, the full raw window: with actions (speed_r, FollowGap's
    answer to the last observation) the env repeats rl_car_drive_followgap — crash ticks, state trace, steers and, through
    the scans of the drive's traced lidar poses, the observations — bit for bit, frozen cars included.  The drive's
    noise base lies N B above the env's (the reset is slot 0)."""
    omap0 = range_libc.PyOMap(maps.load_colombia())
    g, states, speeds = DC.colombia_case(lambda g_: omap0.distance_transform())
    N, B, T = 24, 130, 30
    m = range_libc.PyRayMarchingGPU(omap0, 300)
    fg = support.followgap()
    edge = support.edge(B)
    cars = RC.CarBatch()
    base = 4321
    m.set_noise(0.05, 17, base)
    env = DriveEnv(m, states, N, B, FOV, edge, THRESH, auto_reset=False, car=cars)
    obs = env.reset(seed=0, start_index=np.arange(N))
    assert (env.read()["done"] == 0).all()
    steer0 = fg.eval_many(np.ascontiguousarray(obs))
    m.set_noise(0.05, 17, base + N * B)
    first, final, vel, steers, sp, st = cars.drive_followgap(m, fg, states, T, speeds.astype(np.float64), FOV, B, edge,
                                                             THRESH, steer0=steer0, trace=True)
    m.set_noise(0.05, 17, base)
    assert (first >= 0).any() and (first < 0).any()
    pub = DC.Composed(m, cars, N, B, edge, 1, 0.05, 17, base)
    steer = steer0
    want_first = np.full(N, -(T + 1), np.int32)
    last_pose = np.zeros((N, 3), np.float32)
    for t in range(T):
        alive = want_first < 0
        obs, rew, dn = env.step(np.stack([speeds, steer], -1).astype(np.float32))
        rd = env.read()
        want_first[alive & (dn == 1)] = t
        assert same_bits(rd["states"][alive], st[alive, t]), t
        # the drive's traced lidar poses (frozen cars: the last one) scanned at this slot are the env's observation
        last_pose[alive] = sp[alive, t]
        assert same_bits(obs, pub.scan(last_pose, t + 1)), t
        go = want_first < 0
        steer = fg.eval_many(np.ascontiguousarray(obs))
        assert same_bits(steer[go], steers[go, t]), t
        assert np.isnan(steers[alive & ~go, t]).all()
    assert same_bits(want_first, first)
    assert same_bits(env.read()["states"], final)
    m.set_noise(0.0, 0, 0)


def test_env_fed_the_network_equals_drive_policy():
    """900 beams, 9 envs x 8 steps, the 720-input network of tests/golden/policy_mlp720.npz, with and without
    steer_clip: crash ticks, state trace and steers of rl_car_drive_policy; a twin env with window (180, 720, 1) and
    obs_clip = obs_scale = 15 hands out the network's input form of the same scans."""
    layers, relu = PS.load_fixture(os.path.join(GOLD, "policy_mlp720.npz"))
    pol = Policy.from_arrays(layers, relu)
    g = maps.load_colombia()
    omap = range_libc.PyOMap(g)
    N, B, T = 9, 900, 8
    states, speeds = support.starts(g, omap.distance_transform(), N, 5, 10.0, speed_hi=4.0)     # (0.4 m clear of the margin)
    speeds = speeds.astype(np.float32)
    m = range_libc.PyRayMarchingGPU(omap, 300)
    edge = support.edge(B)
    cars = RC.CarBatch()
    base = 999
    for clip in (None, 0.2):
        m.set_noise(0.05, 5, base)
        env = DriveEnv(m, states, N, B, FOV, edge, THRESH, auto_reset=False, car=cars, steer_clip=clip or 0)
        twin = DriveEnv(m, states, N, B, FOV, edge, THRESH, auto_reset=False, car=cars, steer_clip=clip or 0,
                        obs_window=(180, 720, 1), obs_clip=15, obs_scale=15)
        assert twin.obs_shape == (N, 720)

        def input_form(raw):
            r = raw[:, 180:900]
            return np.where(r <= 15, r / np.float32(15), np.float32(1)).astype(np.float32)

        obs = env.reset(start_index=np.arange(N))
        assert same_bits(twin.reset(start_index=np.arange(N)), input_form(obs))
        assert (env.read()["done"] == 0).all()
        # (the drive takes steer0 unclamped; the starts have steer_angle 0, so the env's clamped first steer and the
        #  drive's raw one, of one sign, turn the wheel alike: tick 0 agrees bit for bit as well)
        steer0 = pol.predict_many(obs)
        m.set_noise(0.05, 5, base + N * B)
        first, final, vel, steers, sp, st = cars.drive_policy(m, pol, states, T, speeds.astype(np.float64), FOV, B, edge,
                                                              THRESH, steer0=steer0, steer_clip=clip, trace=True)
        m.set_noise(0.05, 5, base)
        steer = steer0
        want_first = np.full(N, -(T + 1), np.int32)
        n_clipped = 0
        for t in range(T):
            alive = want_first < 0
            a = np.stack([speeds, steer], -1).astype(np.float32)
            n_clipped += int((np.abs(steer[alive]) > 0.2).sum())
            obs, rew, dn = env.step(a)
            obs2, rew2, dn2 = twin.step(a)
            assert same_bits(obs2, input_form(obs)) and same_bits(rew, rew2) and same_bits(dn, dn2), (clip, t)
            want_first[alive & (dn == 1)] = t
            assert same_bits(env.read()["states"][alive], st[alive, t]), (clip, t)
            go = want_first < 0
            steer = pol.predict_many(obs)
            assert same_bits(steer[go], steers[go, t]), (clip, t)
        assert same_bits(want_first, first), clip
        assert same_bits(env.read()["states"], final) and same_bits(twin.read()["states"], final), clip
        assert n_clipped > 0                                       # the network asked for more than the clip somewhere
        env.close()
        twin.close()
    m.set_noise(0.0, 0, 0)


def _against_statement(env, stmt, actions, seed, start_index=None, aux=False):
    """reset + every step of ``actions`` on the env and on the statement: all outputs and counters, bit for bit."""
    obs = env.reset(seed=seed, start_index=start_index)
    want_obs, want_done = stmt.reset(seed, start_index)
    log = []

    def counters(k):
        rd = env.read()
        assert same_bits(rd["states"], stmt.states), k
        for key, want in (("ticks", stmt.tick), ("episodes", stmt.episode), ("start_index", stmt.start_index),
                          ("done", stmt.done)):
            assert same_bits(rd[key], want), (k, key)
        return rd

    assert same_bits(obs, want_obs)
    counters(0)
    for k, a in enumerate(actions, 1):
        prev_done = stmt.done.copy()
        obs, rew, dn = env.step(a)
        want_obs, want_rew, want_done = stmt.step(a)
        assert same_bits(obs, want_obs), k
        assert same_bits(rew, want_rew), k
        assert same_bits(dn, want_done), k
        rd = counters(k)
        log.append((prev_done, dn.copy(), rew.copy(), rd))
    return log


def test_env_auto_reset_and_truncation_against_the_statement():
    """A 10 m room, a pool of five hand-built starts, 12 envs, max_ticks 6, 25 steps of 3 substeps with auto_reset: done
    codes, ticks, episodes, start indices, states, rewards and observations equal the statement driven by the composed
    public calls; codes 1 and 2 both occur; the step after a done returns reward 0, tick 0 and the drawn start."""
    g, starts, actions = DC.room_case()
    N, B, S = 12, 100, 3
    m = range_libc.PyRayMarchingGPU(range_libc.PyOMap(g), 300)
    edge = support.edge(B)
    cars = RC.CarBatch()
    base, seed = 555, 6
    m.set_noise(0.02, 3, base)
    kw = dict(max_ticks=6, auto_reset=True, crash_reward=-2.5)
    env = DriveEnv(m, starts, N, B, FOV, edge, THRESH, substeps=S, car=cars, **kw)
    pub = DC.Composed(m, cars, N, B, edge, S, 0.02, 3, base)
    stmt = ES.EnvStatement(starts, N, B, pub.step_cars, pub.scan, pub.is_crashed, scan_dist_to_base=D_BASE, **kw)
    log = _against_statement(env, stmt, actions, seed)
    codes = np.concatenate([dn for _, dn, _, _ in log])
    assert (codes == 1).any() and (codes == 2).any() and (codes == 0).any()
    n_fresh = 0
    for prev_done, dn, rew, rd in log:
        for e in np.nonzero(prev_done != 0)[0]:
            n_fresh += 1
            assert rew[e] == 0.0 and rd["ticks"][e] == 0
            assert rd["start_index"][e] == ES.spawn_index(seed, e, rd["episodes"][e], 5)
            assert same_bits(rd["states"][e], starts[rd["start_index"][e]])
    assert n_fresh >= N                                            # every env ended an episode at least once
    assert len(set(np.concatenate([rd["start_index"] for _, _, _, rd in log]).tolist())) == 5
    m.set_noise(0.0, 0, 0)


def test_env_device_form_equals_host_form():
    """Two twin envs, 70 x 100 beams, 6 steps: torch tensors on the current stream give the bits of the NumPy form;
    the method's ray offset and options read the same after every call."""
    import torch
    g, states, actions = DC.maze_case(lambda g_: range_libc.PyOMap(g_).distance_transform())
    N, B = 70, 100
    omap = range_libc.PyOMap(g)
    m = range_libc.PyRayMarchingGPU(omap, 300)
    edge = support.edge(B)
    cars = RC.CarBatch()
    m.set_noise(0.05, 8, 777)
    m.set_option("nt_store", 1)
    probe = np.ascontiguousarray(support.lidar_poses(states[:16]))
    scan0 = np.empty(16 * B, np.float32)
    m.calc_range_fan(probe, scan0, FOV, B)

    def handle_unchanged():
        again = np.empty_like(scan0)
        m.calc_range_fan(probe, again, FOV, B)
        assert same_bits(again, scan0) and m.get_info("nt_store") == 1

    kw = dict(substeps=2, obs_window=(3, 45, 2), max_ticks=4, auto_reset=True, crash_reward=-1.0, car=cars)
    host = DriveEnv(m, states, N, B, FOV, edge, THRESH, **kw)
    dev = DriveEnv(m, states, N, B, FOV, edge, THRESH, **kw)
    o_h, x_h = host.reset(seed=9, aux=True)
    handle_unchanged()
    o_d, x_d = dev.reset(seed=9, aux=True, on_device=True)
    assert o_d.is_cuda and o_d.dtype == torch.float32 and tuple(o_d.shape) == (N, 45)
    assert same_bits(o_d.cpu().numpy(), o_h) and same_bits(x_d.cpu().numpy(), x_h)
    handle_unchanged()
    stream = torch.cuda.Stream()
    seen = set()
    for k in range(6):
        o_h, r_h, d_h, x_h = host.step(actions[k], aux=True)
        handle_unchanged()
        a = torch.from_numpy(actions[k]).cuda()
        if k % 2:                                                  # on a side stream every other step
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                out = dev.step(a, aux=True)
            torch.cuda.current_stream().wait_stream(stream)
        else:
            out = dev.step(a, aux=True)
        o_d, r_d, d_d, x_d = (t.cpu().numpy() for t in out)
        assert out[0].data_ptr() == dev._torch["obs"].data_ptr()    # the env's own tensors, every call
        assert same_bits(o_d, o_h) and same_bits(r_d, r_h) and same_bits(d_d, d_h) and same_bits(x_d, x_h), k
        handle_unchanged()
        seen |= set(d_h.tolist())
    assert {0, 2} <= seen
    rd_h, rd_d = host.read(), dev.read()
    for key in rd_h:
        assert same_bits(rd_h[key], rd_d[key]), key
    # a NumPy step on the env that has been stepping on the device, and the other way round
    o1, r1, d1 = dev.step(actions[6])
    o2, r2, d2 = (t.cpu().numpy() for t in host.step(torch.from_numpy(actions[6]).cuda()))
    assert same_bits(o1, o2) and same_bits(r1, r2) and same_bits(d1, d2)
    with pytest.raises(ValueError):
        dev.step(torch.from_numpy(actions[0].astype(np.float64)).cuda())
    with pytest.raises(ValueError):
        dev.step(torch.from_numpy(actions[0]))                     # a CPU tensor
    m.set_noise(0.0, 0, 0)


@pytest.mark.parametrize("B", [10, 1280])
@pytest.mark.parametrize("N", [1, 9])
def test_env_beam_count_limits(B, N):
    """10 and 1280 beams, 1 and 9 envs, 3 steps against the composed calls."""
    g = maps.make_maze(256, cell=40, wall=3, p=0.45, seed=11)
    omap = range_libc.PyOMap(g)
    m = range_libc.PyRayMarchingGPU(omap, 300)
    states, _ = support.starts(g, omap.distance_transform(), N, 40 + N, 4.0)
    edge = support.edge(B)
    cars = RC.CarBatch()
    m.set_noise(0.03, 2, 10 * B)
    win = (1, B // 2, 2)
    env = DriveEnv(m, states, N, B, FOV, edge, THRESH, substeps=2, obs_window=win, car=cars, obs_clip=6.0, obs_scale=3.0)
    pub = DC.Composed(m, cars, N, B, edge, 2, 0.03, 2, 10 * B)
    stmt = ES.EnvStatement(states, N, B, pub.step_cars, pub.scan, pub.is_crashed, obs_window=win, obs_clip=6.0,
                           obs_scale=3.0, scan_dist_to_base=D_BASE)
    _against_statement(env, stmt, DC.actions(B + N, 3, N), seed=1)
    m.set_noise(0.0, 0, 0)


@pytest.mark.parametrize("B", CS.SIZES)
def test_env_observe_ballot_at_every_row_count(B):
    """env_observe_kernel<ROWS> at every ROWS = 1 ... 20 (consumer_shapes.SIZES: 27 beam counts): nine envs — one past
    a workgroup's eight waves —, a reset and two steps against the statement over the composed public calls, once per
    beam that decides the crash alone (both ends of the first row, the last beam of the last full row, both ends of the
    last row) and once with an outline no beam reaches.  The window's last element is beam B - 1; clip, scale and
    noise on at odd ROWS, the raw window at even ROWS."""
    rows, N, S = CS.rows_of(B), CS.DRIVE_CARS + 1, 2
    odd = rows % 2 == 1
    g = maps.make_maze(256, cell=40, wall=3, p=0.45, seed=11)
    omap = range_libc.PyOMap(g)
    m = range_libc.PyRayMarchingGPU(omap, 300)
    states, _ = support.starts(g, omap.distance_transform(), N, 40 + N, 4.0)
    cars = RC.CarBatch()
    std, nseed, base = (0.03, 2, 10 * B) if odd else (0.0, 0, 0)
    win = (B - 2 * (B // 2) + 1, B // 2, 2)
    assert win[0] + win[2] * (win[1] - 1) == B - 1
    kw = dict(obs_window=win, **(dict(obs_clip=6.0, obs_scale=3.0) if odd else {}))
    for j in CS.one_hot_beams(B) + (None,):
        edge = CS.one_hot_edge(B, j)
        m.set_noise(std, nseed, base)
        env = DriveEnv(m, states, N, B, FOV, edge, THRESH, substeps=S, car=cars, **kw)
        pub = DC.Composed(m, cars, N, B, edge, S, std, nseed, base)
        stmt = ES.EnvStatement(states, N, B, pub.step_cars, pub.scan, pub.is_crashed, scan_dist_to_base=D_BASE, **kw)
        log = _against_statement(env, stmt, DC.actions(B + N, 2, N), seed=1)
        for _, dn, _, _ in log:                 # beam j alone decides: every env crashes, or none does
            assert (dn == (ES.RUNNING if j is None else ES.CRASHED)).all(), (B, j, dn)
    m.set_noise(0.0, 0, 0)


def test_env_teacher_forced_vs_reference_car():
    """8 envs x 10 steps of 3 substeps: every step, fed the env's own state of the step before, agrees with the
    reference's compiled Car to the rtol = atol = 1e-9 of test_drive_teacher_forced_vs_reference."""
    reference.require()
    g = maps.load_colombia()
    omap = range_libc.PyOMap(g)
    N, B, S, T = 8, 100, 3, 10
    states, _ = support.starts(g, omap.distance_transform(), N, 3, 6.0, speed_hi=4.0)
    m = range_libc.PyRayMarchingGPU(omap, 300)
    env = DriveEnv(m, states, N, B, FOV, support.edge(B), THRESH, substeps=S, auto_reset=False)
    env.reset(start_index=np.arange(N))
    actions = DC.actions(77, T, N)
    n_checked = 0
    with reference.RefCar() as ref:
        for k in range(T):
            before = env.read()
            env.step(actions[k])
            after = env.read()
            for e in np.nonzero(before["done"] == 0)[0]:
                want = ref.step(before["states"][e], actions[k, e, 0], actions[k, e, 1], n=S)
                assert np.allclose(after["states"][e], want, rtol=1e-9, atol=1e-9), (k, e)
                n_checked += 1
    assert n_checked >= N * T // 2


def test_env_errors_leave_everything_usable():
    g = maps.make_maze(256, cell=40, wall=3, p=0.45, seed=11)
    omap = range_libc.PyOMap(g)
    dt = omap.distance_transform()
    N, B, M = 9, 100, 4
    states, _ = support.starts(g, dt, M, 2, 8.0)
    edge = support.edge(B)
    actions = DC.actions(3, 8, N)
    # the env that sees the errors and a twin that never does, each on handles of its own
    mA, mB = range_libc.PyRayMarchingGPU(omap, 300), range_libc.PyRayMarchingGPU(omap, 300)
    carsA, carsB = RC.CarBatch(), RC.CarBatch()
    for m in (mA, mB):
        m.set_noise(0.05, 7, 321)
        m.set_option("nt_store", 1)
    kw = dict(substeps=2, max_ticks=5, crash_reward=-4.0, obs_window=(0, 50, 2))
    A = DriveEnv(mA, states, N, B, FOV, edge, THRESH, car=carsA, **kw)
    Bt = DriveEnv(mB, states, N, B, FOV, edge, THRESH, car=carsB, **kw)
    Lb = _lib.lib()
    f32p, f64p, i32p = _lib.f32p, _lib.f64p, _lib.i32p
    INVALID = -1

    obs_buf, rew_buf = np.empty((N, 50), np.float32), np.empty(N, np.float32)
    done_buf = np.empty(N, np.int32)

    def raw_step(h_env, a=actions[0], obs=obs_buf, rew=rew_buf, done=done_buf):
        p = lambda x, t: x.ctypes.data_as(t) if x is not None else None
        return Lb.rl_env_step(h_env, p(a, f32p), p(obs, f32p), p(rew, f32p), p(done, i32p), None)

    def raw_reset(h_env, sidx=None, obs=obs_buf, done=done_buf):
        p = lambda x, t: x.ctypes.data_as(t) if x is not None else None
        return Lb.rl_env_reset(h_env, 0, p(sidx, i32p), p(obs, f32p), None, p(done, i32p))

    def refused(rc, code=INVALID):
        assert rc == code, rc
        with pytest.raises(_lib.ScanLibError):
            _lib.check(rc)

    # a step or a read before the first reset
    refused(raw_step(A._h))
    refused(Lb.rl_env_read(A._h, None, None, None, None, done_buf.ctypes.data_as(i32p)))
    with pytest.raises(_lib.ScanLibError, match="reset"):
        A.step(actions[0])

    def create(car=carsA._h, h=mA._h, starts=states, ed=edge, n_starts=None, params=True, out=True, **over):
        p = _lib.EnvParams.from_buffer_copy(A.params)
        for key, v in over.items():
            setattr(p, key, v)
        handle = C.c_void_p()
        rc = Lb.rl_env_create(car, h, C.byref(p) if params else None,
                              ed.ctypes.data_as(f64p) if ed is not None else None,
                              starts.ctypes.data_as(f64p) if starts is not None else None,
                              starts.shape[0] if n_starts is None else n_starts, C.byref(handle) if out else None)
        assert not handle.value or rc == 0
        if handle.value:
            Lb.rl_env_destroy(handle)
        return rc

    def run(env, steps):
        return [env.step(actions[k], aux=True) for k in steps]

    def same(xs, ys):
        for x, y in zip(xs, ys):
            for a, b in zip(x, y):
                assert same_bits(a, b)

    assert create() == 0                                            # the helper itself creates a valid env
    o_a, o_b = A.reset(seed=5), Bt.reset(seed=5)
    assert same_bits(o_a, o_b)
    same(run(A, (0, 1)), run(Bt, (0, 1)))

    # every refusal of rl_env_create
    refused(create(car=None))
    refused(create(h=None))
    refused(create(params=False))
    refused(create(ed=None))
    refused(create(starts=None, n_starts=M))
    refused(create(out=False))
    nan, inf = float("nan"), float("inf")
    for over in (dict(n_envs=0), dict(n_envs=-3), dict(substeps=0), dict(substeps=513), dict(num_rays=9),
                 dict(num_rays=1281), dict(obs_start=-1), dict(obs_start=2), dict(obs_count=51), dict(obs_count=0),
                 dict(obs_stride=0), dict(obs_stride=3), dict(steer_clip=-0.1), dict(steer_clip=nan), dict(obs_clip=-1.0),
                 dict(obs_clip=nan), dict(obs_scale=-1.0), dict(obs_scale=nan), dict(crash_reward=nan), dict(dt=inf),
                 dict(dt=nan), dict(max_ticks=-1), dict(fov=nan)):
        refused(create(**over))
    refused(create(n_starts=0))
    bad = states.copy()
    bad[2, 5] = inf
    refused(create(starts=bad))
    bad[2, 5] = nan
    refused(create(starts=bad))
    big = (1 << 31) // 1000 + 1
    refused(create(n_envs=big, num_rays=1000, obs_count=1, ed=support.edge(1000)))
    multi = RC.CarBatch(device=[0])
    refused(create(car=multi._h))
    with pytest.raises(_lib.ScanLibError, match="single-device"):
        DriveEnv(mA, states, N, B, FOV, edge, THRESH, car=multi)
    if Lb.rl_device_count() >= 2:
        with pytest.raises(_lib.ScanLibError, match="device"):
            DriveEnv(mA, states, N, B, FOV, edge, THRESH, car=RC.CarBatch(device=1))
    # the range method's own refusal comes back with its code: more beams than its fan table holds is not reached
    # (num_rays is capped first), a NaN fov is (above); RL_ERR_INVALID either way
    # null pointers and a start index outside the pool at the calls; the env goes on as if nothing had happened
    refused(raw_step(None))
    refused(raw_step(A._h, a=None))
    refused(raw_step(A._h, obs=None))
    refused(raw_step(A._h, rew=None))
    refused(raw_step(A._h, done=None))
    refused(raw_reset(None))
    refused(raw_reset(A._h, obs=None))
    refused(raw_reset(A._h, done=None))
    for v in (-1, M):
        sidx = np.zeros(N, np.int32)
        sidx[N - 1] = v
        refused(raw_reset(A._h, sidx=sidx))
        with pytest.raises(ValueError):
            A.reset(start_index=sidx)
    refused(Lb.rl_env_read(None, None, None, None, None, None))
    with pytest.raises(ValueError):
        A.step(actions[0].astype(np.float64))
    with pytest.raises(ValueError):
        A.step(actions[0][:-1])
    same(run(A, (2, 3)), run(Bt, (2, 3)))
    rd_a, rd_b = A.read(), Bt.read()
    for key in rd_a:
        assert same_bits(rd_a[key], rd_b[key]), key
    # the handles scan as a twin's: same noise offset, same options
    poses = maps.sample_free_poses(g, 16, 3, 4.0, dt)
    sa, sb = np.empty(16 * B, np.float32), np.empty(16 * B, np.float32)
    mA.calc_range_fan(poses, sa, FOV, B)
    mB.calc_range_fan(poses, sb, FOV, B)
    assert same_bits(sa, sb) and mA.get_info("nt_store") == 1

    # NaN and inf actions: done = 3, the state unchanged, crash_reward; no other env is affected
    A.reset(seed=11, start_index=np.arange(N) % M)
    Bt.reset(seed=11, start_index=np.arange(N) % M)
    same(run(A, (0,)), run(Bt, (0,)))
    before = A.read()
    assert (before["done"][[1, 4, 6]] == 0).all()
    a = actions[1].copy()
    a[1, 0], a[4, 1], a[6] = np.nan, np.inf, (-np.inf, np.nan)
    o_a, r_a, d_a, x_a = A.step(a, aux=True)
    o_b, r_b, d_b, x_b = Bt.step(actions[1], aux=True)
    hit = np.zeros(N, bool)
    hit[[1, 4, 6]] = True
    after = A.read()
    assert (d_a[hit] == 3).all() and (r_a[hit] == np.float32(-4.0)).all()
    assert same_bits(after["states"][hit], before["states"][hit]) and same_bits(after["ticks"][hit], before["ticks"][hit])
    assert np.isfinite(o_a).all() and np.isfinite(x_a).all() and np.isfinite(after["states"]).all()
    for x, y in ((o_a, o_b), (r_a, r_b), (d_a, d_b), (x_a, x_b), (after["states"], Bt.read()["states"])):
        assert same_bits(x[~hit], y[~hit])
    # with auto_reset (the default) the three re-spawn on the next step
    o_a, r_a, d_a = A.step(actions[2])
    rd = A.read()
    assert (rd["ticks"][hit] == 0).all() and (r_a[hit] == 0).all()
    assert (rd["episodes"][hit] == before["episodes"][hit] + 1).all()
    for m in (mA, mB):
        m.set_noise(0.0, 0, 0)


def test_env_facade_matches_hand_built():
    """RacecarSimulator(cfg).driveEnv(...) is a DriveEnv on the simulator's method, car, fan, edge table and thresholds."""
    g = maps.load_colombia()
    cfg = dict(RC.DEFAULT_CAR)
    cfg.update(scan_dist_to_base=0.275, batch_size=40, scan_beams=1080, scan_fov=4.71, scan_std=0.01,
               scan_max_range=15.0, free_thresh=0.8)
    sim = RacecarSimulator(cfg)
    omap = range_libc.PyOMap(g)
    sim.setMap(omap, g.resolution, g.origin)
    sim.setRaytracingMethod("RMGPU")
    N = 9
    starts, _ = support.starts(g, omap.distance_transform(), 4, 6, 6.0)
    kw = dict(substeps=2, obs_window=(180, 720, 1), obs_clip=15, obs_scale=15, max_ticks=3, crash_reward=-1.0)
    env = sim.driveEnv(N, starts, **kw)
    assert isinstance(env, DriveEnv) and env.obs_shape == (N, 720)
    hand = DriveEnv(sim.scan_simulator.scan_method, starts, N, 1080, 4.71, sim.edge_distances, cfg["ttc_thresh"],
                    car=sim.car, scan_dist_to_base=0.275, **kw)
    actions = DC.actions(21, 5, N)
    assert same_bits(env.reset(seed=2), hand.reset(seed=2))
    for a in actions:
        for x, y in zip(env.step(a, aux=True), hand.step(a, aux=True)):
            assert same_bits(x, y)
    rd_a, rd_b = env.read(), hand.read()
    for key in rd_a:
        assert same_bits(rd_a[key], rd_b[key]), key
    assert (rd_a["episodes"] > 0).any()
