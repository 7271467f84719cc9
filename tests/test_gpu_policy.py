"""The steering policy network on the MI355X (Policy, rl_policy_*, CarBatch.drive_policy, RacecarSimulator.
drivePolicyMany): every output bit-identical to the host statement of the canonical float32 form
(tests/policy_statement.py) on the reference's weights (tests/golden/policy_mlp720.npz) and on random chains, and the
closed loop equal to the same loop composed from the public calls."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLD
import policy_statement as S
import support
from oracle import reference
from support import D_BASE, FOV, THRESH, same_bits
from pyracecarsimulator_amd import Policy, RacecarSimulator, _lib, maps, range_libc
from pyracecarsimulator_amd import racecar as RC

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

B = 1081
CLIP = 0.4189                                            # scripts/policy_driver.py:33


@pytest.fixture(scope="module")
def net():
    layers, relu = S.load_fixture(os.path.join(GOLD, "policy_mlp720.npz"))
    return layers, relu, Policy.from_arrays(layers, relu)


def _hard_scans(n, size, seed):
    """Ranges with the values the input transform must get right: NaN, +inf, beyond the clip, exactly 15 and its
    neighbours, subnormals and zero."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.0, 18.0, (n, size)).astype(np.float32)
    special = np.array([np.nan, np.inf, 15.0, np.nextafter(np.float32(15), np.float32(0)),
                        np.nextafter(np.float32(15), np.float32(99)), 1e-40, 0.0, 30.0, 1e-8], np.float32)
    mask = rng.uniform(size=s.shape) < 0.08
    s[mask] = special[rng.integers(0, len(special), int(mask.sum()))]
    return s


def _same_or_nan(a, b):
    """bit-equal where finite, NaN at the same places (the trace rows a car never reaches are all-ones NaNs)."""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and (na == nb).all() and same_bits(a[~na], b[~nb])


def _rows_to_check(R, rng):
    """every row up to 5000; beyond, a sample plus both ends (the statement is per row)."""
    if R <= 5000:
        return np.arange(R)
    return np.unique(np.concatenate([np.arange(40), np.arange(R - 40, R), rng.integers(0, R, 1500)]))


@pytest.mark.parametrize("R", [1, 15, 16, 17, 1000, 4097, 65536])
def test_predict_many_equals_statement_fixture(net, R):
    layers, relu, pol = net
    scans = _hard_scans(R, B, R)
    got = pol.predict_many(scans)
    rows = _rows_to_check(R, np.random.default_rng(R))
    want = S.forward(scans[rows], layers, relu)
    assert same_bits(got[rows], want)
    assert np.isfinite(got).all()


@pytest.mark.parametrize("dims,in_start,size,relu", [
    ((37, 5, 1), 0, 37, (True, False)),
    ((37, 5, 1), 361, 1081, (True, False)),
    ((3, 1), 7, 10, (False,)),
    ((1024, 256, 3, 255, 17, 1), 50, 1081 + 50, (True, True, False, True, True)),
    ((720, 64, 128, 128, 64, 1), 0, 720, (True, True, True, True, True)),     # cfg5's 720-beam fans, in_start 0
    ((61, 7, 6, 5, 4, 3, 2, 9, 1), 11, 80, (True,) * 8),                       # eight layers
])
def test_predict_many_equals_statement_random_chains(dims, in_start, size, relu):
    rng = np.random.default_rng(sum(dims) + in_start)
    layers = [((rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32),
               (0.1 * rng.standard_normal(dims[i + 1])).astype(np.float32)) for i in range(len(dims) - 1)]
    pol = Policy.from_arrays(layers, relu, in_start=in_start, clip=12.5, scale=7.0)
    for R in (1, 17, 1000):
        scans = _hard_scans(R, size, R + size)
        got = pol.predict_many(scans)
        want = S.forward(scans, layers, relu, in_start=in_start, clip=12.5, scale=7.0)
        assert same_bits(got, want), (dims, R)


def test_device_and_single_forms(net):
    import torch
    layers, relu, pol = net
    R = 777
    scans = _hard_scans(R, B, 5)
    host = pol.predict_many(scans)
    d_in = torch.from_numpy(scans).to("cuda:0")
    d_out = torch.full((R,), float("nan"), dtype=torch.float32, device="cuda:0")
    pol.predict_device(d_in.data_ptr(), R, B, d_out.data_ptr())
    torch.cuda.synchronize()
    assert same_bits(d_out.cpu().numpy(), host)
    one = pol.predict_action(scans[123])
    assert isinstance(one, np.float32) and one.tobytes() == host[123].tobytes()
    # a flat (n * size,) batch as scanMany returns it
    assert same_bits(pol.predict_many(scans.reshape(-1), B), host)


def test_create_caps_and_errors(net):
    layers, relu, pol = net
    L = _lib.lib()
    with pytest.raises(_lib.ScanLibError):                        # 9 layers
        Policy.from_arrays([(np.ones((4, 4), np.float32), np.ones(4, np.float32))] * 8 +
                           [(np.ones((4, 1), np.float32), np.ones(1, np.float32))], in_start=0)
    with pytest.raises(_lib.ScanLibError):                        # width 257
        Policy.from_arrays([(np.ones((4, 257), np.float32), np.ones(257, np.float32)),
                            (np.ones((257, 1), np.float32), np.ones(1, np.float32))], in_start=0)
    with pytest.raises(_lib.ScanLibError):                        # input 1025
        Policy.from_arrays([(np.ones((1025, 1), np.float32), np.ones(1, np.float32))], in_start=0)
    with pytest.raises(_lib.ScanLibError):                        # two outputs
        Policy.from_arrays([(np.ones((4, 2), np.float32), np.ones(2, np.float32))], in_start=0)
    scans = _hard_scans(4, B, 9)
    want = pol.predict_many(scans)
    for size in (899, 1080 - 181):                                # window [180, 900) does not fit
        with pytest.raises(_lib.ScanLibError):
            pol.predict_many(np.ascontiguousarray(scans[:, :size]))
    assert L.rl_policy_eval(pol._h, None, 4, B, None) != 0
    assert pol.predict_many(scans[:0]).shape == (0,)
    assert same_bits(pol.predict_many(scans), want)


# ---------------------------------------------------------------- closed loop
def _methods(omap, mrx):
    return [("RMGPU", range_libc.PyRayMarchingGPU(omap, mrx), 0.05),
            ("RM", range_libc.PyRayMarching(omap, mrx), 0.0),
            ("CDDT", range_libc.PyCDDTCast(omap, mrx, 112), 0.02)]


def _composed(cars, m, std, base, layers, relu, states, speeds, steer0, T, edge, clip):
    """The loop from the public calls: rollout(n_steps=1), calc_range_fan, is_crashed, the statement's policy."""
    R = states.shape[0]
    cur = states.copy()
    steer = steer0.astype(np.float64)
    alive = np.ones(R, bool)
    first = np.full(R, -(T + 1), np.int32)
    steers = np.full((R, T), np.nan, np.float32)
    st = np.full((R, T, 11), np.nan)
    last_pose = np.zeros((R, 3), np.float32)
    for t in range(T):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        _, out, _ = cars.rollout(cur[idx], np.stack([speeds[idx], steer[idx]], -1)[:, None, :], n_steps=1,
                                 action_every=1)
        cur[idx] = out
        st[idx, t] = out
        last_pose[idx] = support.lidar_poses(out)
        ranges = np.empty(R * B, np.float32)
        m.set_noise(std, 99, base + t * R * B)
        m.calc_range_fan(last_pose, ranges, FOV, B)
        ranges = ranges.reshape(R, B)
        crashed = np.array([RC.is_crashed(ranges[r], B, 1, edge, THRESH) >= 0 for r in idx], bool)
        first[idx[crashed]] = t
        alive[idx[crashed]] = False
        go = idx[~crashed]
        if go.size:
            a = S.forward(ranges[go], layers, relu)
            steers[go, t] = a
            s64 = a.astype(np.float64)
            steer[go] = np.clip(s64, -clip, clip) if clip else s64
    return first, cur, steers, st


def test_drive_policy_equals_composed_public_calls(net):
    """A 512^2 maze, 48 cars x 25 ticks, RMGPU (noise on), RM (literal) and CDDT (noise on), both steer_clip
    modes: crash ticks, steers and states bit for bit against the composed loop (which steps the car with
    rollout(n_steps=1), itself pinned to the reference's Car elsewhere); the lidar poses to one f32 ulp."""
    layers, relu, pol = net
    g = maps.make_maze(512, cell=40, wall=3, p=0.45, seed=11)
    mrx = 300
    omap = range_libc.PyOMap(g)
    dt = omap.distance_transform()
    R, T = 48, 25
    far, sp_far = support.starts(g, dt, R - 8, 31, 8.0)
    near, sp_near = support.starts(g, dt, 8, 32, 1.0)
    states, speeds = np.concatenate([far, near]), np.concatenate([sp_far, sp_near])
    steer0 = np.random.default_rng(7).uniform(-0.3, 0.3, R).astype(np.float32)
    edge = support.edge(B)
    cars = RC.CarBatch()
    n_clipped = 0
    for name, m, std in _methods(omap, mrx):
        for clip in (None, CLIP):
            base = 3 * R * B
            m.set_noise(std, 99, base)
            first, final, vel, steers, sp, st = cars.drive_policy(m, pol, states, T, speeds, FOV, B, edge, THRESH,
                                                                  steer0=steer0, steer_clip=clip, trace=True)
            want = _composed(cars, m, std, base, layers, relu, states, speeds, steer0, T, edge, clip or 0.0)
            m.set_noise(0.0, 0, 0)
            assert (first >= 0).any() and (first < 0).any(), name
            assert (first == want[0]).all(), (name, clip)
            assert same_bits(final, want[1]), (name, clip)
            assert _same_or_nan(steers, want[2]), (name, clip)
            assert _same_or_nan(st, want[3]), (name, clip)
            assert _same_or_nan(vel, st[..., 3]), (name, clip)
            n_clipped += int((np.abs(steers[np.isfinite(steers)]) > CLIP).sum())
    assert n_clipped > 0                                          # the clip acted somewhere


def test_drive_policy_steps_match_reference_car(net):
    """Colombia, RMGPU, 16 cars x 60 ticks, clipped: every step, fed the GPU's own state of the tick before and the
    clamped network output, agrees with the reference's compiled Car (as test_gpu_drive pins FollowGap's loop)."""
    layers, relu, pol = net
    reference.require()
    g = maps.load_colombia()
    omap = range_libc.PyOMap(g)
    dt = omap.distance_transform()
    m = range_libc.PyRayMarchingGPU(omap, 300)
    R, T = 16, 60
    states, speeds = support.starts(g, dt, R, 4, 6.0, speed_hi=4.0)
    edge = support.edge(B)
    first, final, vel, steers, sp, st = RC.CarBatch().drive_policy(m, pol, states, T, speeds, FOV, B, edge, THRESH,
                                                                    steer_clip=CLIP, trace=True)
    with reference.RefCar() as ref:
        for r in range(R):
            last = first[r] if first[r] >= 0 else T - 1
            for t in range(last + 1):
                prev = states[r] if t == 0 else st[r, t - 1]
                s_in = 0.0 if t == 0 else float(np.clip(np.float64(steers[r, t - 1]), -CLIP, CLIP))
                assert np.allclose(st[r, t], ref.step(prev, speeds[r], s_in), rtol=1e-9, atol=1e-9), (r, t)


def test_drive_policy_chunking_is_invariant(net):
    """T ticks in one call == T/2 + T/2 with the states, the last steer and the noise offset chained."""
    layers, relu, pol = net
    g = maps.load_colombia()
    omap = range_libc.PyOMap(g)
    dt = omap.distance_transform()
    m = range_libc.PyRayMarchingGPU(omap, 300)
    R, T, H = 64, 60, 30
    states, speeds = support.starts(g, dt, R, 8, 3.0)
    edge = support.edge(B)
    cars = RC.CarBatch()
    base = 12345
    for clip in (None, CLIP):
        m.set_noise(0.05, 4, base)
        whole = cars.drive_policy(m, pol, states, T, speeds, FOV, B, edge, THRESH, steer_clip=clip, trace=True)
        a = cars.drive_policy(m, pol, states, H, speeds, FOV, B, edge, THRESH, steer_clip=clip, trace=True)
        ok = a[0] < 0
        st0 = np.where(ok, a[3][:, -1], np.float32(0.0)).astype(np.float32)
        m.set_noise(0.05, 4, base + H * R * B)
        b = cars.drive_policy(m, pol, a[1], T - H, speeds, FOV, B, edge, THRESH, steer0=st0, steer_clip=clip,
                              trace=True)
        m.set_noise(0.0, 0, 0)
        assert ok.any()
        for k in range(2, 6):
            assert same_bits(whole[k][:, :H], a[k]), (clip, k)
        # steer0 is f32: with the clip on, the chained call equals the whole one for the cars whose last output
        # the clamp leaves alone (a clamped one would get the f32 bound, not the f64 one)
        raw = a[3][:, -1].astype(np.float64)
        exact = ok if not clip else ok & (np.abs(raw) <= clip)
        assert exact.any()
        assert same_bits(whole[1][exact], b[1][exact]), clip
        for k in range(2, 6):
            assert same_bits(whole[k][exact, H:], b[k][exact]), (clip, k)
        want_first = np.where(b[0][exact] >= 0, b[0][exact] + H, -(T + 1))
        assert (whole[0][exact] == want_first).all(), clip


def test_drive_policy_facade_and_errors(net):
    layers, relu, pol = net
    g = maps.make_maze(512, cell=40, wall=3, p=0.45, seed=11)
    omap = range_libc.PyOMap(g)
    dt = omap.distance_transform()
    m = range_libc.PyRayMarchingGPU(omap, 300)
    cars = RC.CarBatch()
    R, T = 8, 10
    states, speeds = support.starts(g, dt, R, 2, 8.0)
    edge = support.edge(B)
    m.set_option("nt_store", 1)
    drive0 = cars.drive_policy(m, pol, states, T, speeds, FOV, B, edge, THRESH)
    scans = _hard_scans(4, B, 1)
    p0 = pol.predict_many(scans)

    def still_usable():
        assert same_bits(pol.predict_many(scans), p0)
        assert m.get_info("nt_store") == 1
        again = cars.drive_policy(m, pol, states, T, speeds, FOV, B, edge, THRESH)
        for x, y in zip(drive0, again):
            assert same_bits(x, y)

    Lb = _lib.lib()
    f64p = _lib.f64p

    def raw(R_, T_, nr, st_=states, ed=edge, h_pol=pol._h, first=True):
        fst = np.zeros(max(R_, 1), np.int32)
        return Lb.rl_car_drive_policy(cars._h, m._h, h_pol, st_.ctypes.data_as(f64p) if st_ is not None else None,
                                      speeds.ctypes.data_as(f64p), None, R_, T_, 0.01, D_BASE, FOV, nr,
                                      ed.ctypes.data_as(f64p), THRESH, 0.0,
                                      fst.ctypes.data_as(C.POINTER(C.c_int)) if first else None,
                                      None, None, None, None, None)

    for rc in (raw(R, T, B, st_=None), raw(R, T, B, first=False), raw(R, T, B, h_pol=None), raw(R, 0, B),
               raw(R, -2, B)):
        assert rc != 0
        with pytest.raises(_lib.ScanLibError):
            _lib.check(rc)
        still_usable()
    # scans too short for the window [180, 900): 720 beams (cfg5's fans need in_start 0), 899
    for nr in (720, 899):
        with pytest.raises(_lib.ScanLibError, match="window"):
            cars.drive_policy(m, pol, states, T, speeds, FOV, nr, support.edge(nr), THRESH)
        still_usable()
    multi = RC.CarBatch(device=[0])
    with pytest.raises(_lib.ScanLibError, match="single-device"):
        multi.drive_policy(m, pol, states, T, speeds, FOV, B, edge, THRESH)
    still_usable()
    if _lib.lib().rl_device_count() >= 2:
        pol1 = Policy.from_arrays(layers, relu, device=1)
        with pytest.raises(_lib.ScanLibError, match="device"):
            cars.drive_policy(m, pol1, states, T, speeds, FOV, B, edge, THRESH)
        still_usable()
    with pytest.raises(ValueError):
        cars.drive_policy(m, pol, states, T, speeds, FOV, B, edge, THRESH, steer_clip=0.0)
    f0 = cars.drive_policy(m, pol, states[:0], T, speeds[:0], FOV, B, edge, THRESH)
    assert f0[0].shape == (0,)
    still_usable()
    # in_start 0 on cfg5-sized 720-beam fans drives
    pol720 = Policy.from_arrays(layers, relu, in_start=0)
    f720 = cars.drive_policy(m, pol720, states, 3, speeds, FOV, 720, support.edge(720), THRESH)
    assert f720[3].shape == (R, 3)
    # the façade: RacecarSimulator.drivePolicyMany is CarBatch.drive_policy on the simulator's method and edge table
    cfg = dict(RC.DEFAULT_CAR)
    cfg.update(scan_dist_to_base=0.275, batch_size=40, scan_beams=1080, scan_fov=4.71, scan_std=0.01,
               scan_max_range=15.0, free_thresh=0.8)
    sim = RacecarSimulator(cfg)
    sim.setMap(omap, g.resolution, g.origin)
    sim.setRaytracingMethod("RMGPU")
    got = sim.drivePolicyMany(states, T, pol, speed=2.0, steer_clip=CLIP)
    want = sim.car.drive_policy(sim.scan_simulator.scan_method, pol, states, T, 2.0, sim.scan_fov, sim.num_rays,
                                sim.edge_distances, sim.ttc_thresh, scan_dist_to_base=sim.scan_dist_to_base,
                                steer_clip=CLIP)
    for x, y in zip(got, want):
        assert same_bits(x, y)
