"""A refused host-pointer call leaves its handles as they were (csrc/abi_internal.h HostCall: one synchronous call's
staging up, launches, results down and wait, drained when it returns before the wait), and every handle whose staging
is counted in elements of its type returns every optional output it has.

Each refusal case records a valid call, makes a call that an argument check refuses AFTER its uploads (or a kernel) were
queued, asserts the rl_status, and repeats the valid call on the same handles: the outputs carry the same bits.  Each
round trip is held to the statement the rest of the suite uses for that entry point: the reference's compiled Car and
FollowGap with the oracle scan (test_gpu_drive), tests/race_statement.py, tests/mcl_statement.py.

The suite's smallest maze (56^2 cells, range 60), 65 beams, RMGPU unless said otherwise.

No case refuses rl_pf_run in the middle of a call: once it has staged its rows, launch_mcl_step / launch_pf_weights can
only fail on a HIP error or an allocation (pf_kind_of and the shape are checked before the uploads), and this file
provokes neither."""
import numpy as np
import pytest

import mcl_statement as MS
import race_statement as RS
import support
from drive_cases import assert_teacher_forced
from oracle import reference
from pf_cases import assert_equal_to_statement
from support import FOV, THRESH, same_bits, within_one_ulp
from pyracecarsimulator_amd import ParticleFilter, _lib, maps, range_libc
from pyracecarsimulator_amd import racecar as RC

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

B, MRX = 65, 60
RL_ERR_INVALID, RL_ERR_UNSUPPORTED = -1, -4           # include/scanlib.h rl_status
R, STEPS, EVERY, DT = 3, 4, 2, 0.01                   # the roll-outs: 3 x 4 steps, an action every 2


@pytest.fixture(scope="module")
def world(oracle_mod):
    g = maps.make_maze(56, cell=14, wall=2, p=0.5, seed=3, origin=(2.0, -1.5, -0.3))
    om = oracle_mod.OracleMap.from_gridmap(g, MRX)
    return g, om, range_libc.PyOMap(g)


@pytest.fixture()
def method(world):
    m = range_libc.PyRayMarchingGPU(world[2], MRX)
    yield m
    m.close()


def _rollout_case(g, om):
    states, _ = support.starts(g, om.dt, R, 21, 4.0, speed_hi=3.0)
    rng = np.random.default_rng(4)
    actions = np.stack([rng.uniform(0.5, 4.0, (R, 2)), rng.uniform(-0.4, 0.4, (R, 2))], -1)
    return states, actions


def _refused(code, call, *args, **kw):
    with pytest.raises(_lib.ScanLibError) as e:
        call(*args, **kw)
    assert e.value.code == code, e.value
    return str(e.value)


def test_rollout_check_refused_after_the_rollout_kernel(world, method):
    """rl_car_rollout_check launches rollout_kernel and only then checks the fan: num_rays 0 and a NaN fov come back
    RL_ERR_INVALID, and the valid call after each (crash indices, final states, velocities) repeats the first one's bits;
    its states and velocities are rl_car_rollout's."""
    g, om, _ = world
    cars = RC.CarBatch()
    states, actions = _rollout_case(g, om)
    edge = support.edge(B)

    def valid():
        return cars.rollout_check(method, states, actions, FOV, B, edge, THRESH, n_steps=STEPS, action_every=EVERY, dt=DT)

    want = valid()
    assert want[0].shape == (R,) and want[1].shape == (R, 11) and want[2].shape == (R, STEPS)
    for fov, num_rays in ((FOV, 0), (float("nan"), B)):
        msg = _refused(RL_ERR_INVALID, cars.rollout_check, method, states, actions, fov, num_rays, edge, THRESH,
                       n_steps=STEPS, action_every=EVERY, dt=DT)
        print("refused:", msg)
        for a, b in zip(valid(), want):
            assert same_bits(a, b), (fov, num_rays)
    _, final, vel = cars.rollout(states, actions, STEPS, EVERY, DT)
    assert same_bits(final, want[1]) and same_bits(vel, want[2])
    cars.close()


def test_staged_fan_refused_after_its_poses_were_queued(world):
    """CDDT, 5 poses with hit cells asked for: the call stages its poses, then launch_fan answers RL_ERR_UNSUPPORTED (hit
    cells exist only for RM and Bresenham).  A plain 5-pose fan before and after carries the same bits, through the
    pinned block and staged through the handle's device buffers."""
    g, om, omap = world
    m = range_libc.PyCDDTCast(omap, MRX, 112)
    poses = maps.sample_free_poses(g, 5, 6, 2.0, om.dt)

    def fans():
        out = []
        for pinned_max in (m.get_info("pinned_max_rays"), 0):
            saved = m.get_info("pinned_max_rays")
            m.set_option("pinned_max_rays", pinned_max)
            r = np.full(len(poses) * B, -7.0, np.float32)
            m.calc_range_fan(poses, r, FOV, B)
            m.set_option("pinned_max_rays", saved)
            out.append(r)
        return out

    before = fans()
    assert not (before[0] == -7.0).any() and same_bits(before[0], before[1])
    hits = np.full((len(poses) * B, 2), -7, np.int32)
    ranges = np.full(len(poses) * B, -7.0, np.float32)
    print("refused:", _refused(RL_ERR_UNSUPPORTED, m.calc_range_fan, poses, ranges, FOV, B, hit_cells=hits))
    for a, b in zip(fans(), before):
        assert same_bits(a, b)
    m.close()


def test_rollout_returns_states_and_velocities(world):
    """rl_car_rollout with states_out and vel_out, 3 roll-outs x 4 steps: every step against the reference's compiled
    Car (f64 state to 1e-9 as test_gpu_drive holds it, the f32 pose within one ulp, the velocity the state's)."""
    g, om, _ = world
    reference.require()
    states, actions = _rollout_case(g, om)
    cars = RC.CarBatch()
    poses, final, vel = cars.rollout(states, actions, STEPS, EVERY, DT)
    assert poses.shape == (R, STEPS, 3) and final.shape == (R, 11) and vel.shape == (R, STEPS)
    with reference.RefCar() as ref:
        for r in range(R):
            ref.set_state(states[r])
            for t in range(STEPS):
                now = ref.step(None, actions[r, t // EVERY, 0], actions[r, t // EVERY, 1], dt=DT)
                assert within_one_ulp(now[:3].astype(np.float32), poses[r, t]), (r, t)
                assert np.allclose(vel[r, t], now[3], rtol=1e-9, atol=1e-9), (r, t)
            assert np.allclose(final[r], now, rtol=1e-9, atol=1e-9), r
            assert vel[r, -1] == final[r, 3]
    cars.close()


def test_followgap_drive_returns_all_four_traces(world, method):
    """2 cars x 3 ticks with velocities, steers, lidar poses and states traced: every link against the reference's Car
    and FollowGap and the oracle's scan, as test_gpu_drive's teacher-forced case holds the 32-car drive."""
    g, om, _ = world
    reference.require()
    states, speeds = support.starts(g, om.dt, 2, 21, 4.0, speed_hi=3.0)
    fg = support.followgap()
    cars = RC.CarBatch()
    drive = cars.drive_followgap(method, fg, states, 3, speeds, FOV, B, support.edge(B), THRESH, trace=True)
    assert len(drive) == 6
    assert_teacher_forced(om, states, speeds, drive, 3, B)
    cars.close()


def test_outline_cells_of_three_cars(oracle_mod, world):
    """rl_car_outline_cells for 3 cars (two on the map, one across its border): the statement's cells as sets, -1 behind
    each car's count."""
    g, om, omap = world
    on_map = maps.sample_free_poses(g, 2, 8, 2.0, om.dt).astype(np.float64)
    cars = np.concatenate([on_map, [[g.origin[0], g.origin[1], 0.4]]])
    ch = RC.CarBatch()
    cells, counts = ch.outline_cells(omap, cars)
    want = RS.outline_cells(cars, RC.DEFAULT_CAR["length"], RC.DEFAULT_CAR["width"], g.resolution, g.origin, g.rows, g.cols,
                            oracle_mod.sincosf)
    assert counts.shape == (3,) and (counts[:2] > 0).all()
    for i in range(3):
        assert set(cells[i, :counts[i]].tolist()) == set(want[i].tolist()), i
        assert (cells[i, counts[i]:] == -1).all()
    ch.close()


def test_filter_read_returns_all_five_arrays(world, method):
    """8 particles x 5 angles, two steps that resample: the run's estimate, neff and flags and rl_pf_read's particles,
    weights, ancestors, cumulative weights and likelihoods equal tests/mcl_statement.py bit for bit."""
    g, om, _ = world
    P, A, T, std, ratio = 8, 5, 2, (0.02, 0.02, 0.01), 2.0
    parts, angles, odom, obs, table = MS.localisation_case(g, om.dt, MRX, FOV, P, A, T)
    method.set_sensor_model(table)
    pf = ParticleFilter(method, angles, P, motion_std=std, resample_ratio=ratio)
    pf.reset(parts, seed=3)
    out = pf.run_raw(odom, obs)
    st = MS.Filter(MS.statement_likelihood(g, om, MRX, "canonical", angles, table), P, std, ratio)
    st.reset(parts, seed=3)
    want = st.run(odom, obs)
    assert sorted(pf.read()) == ["ancestors", "cum", "likelihood", "particles", "weights"]
    assert_equal_to_statement(pf, out, st, want, "8 x 5")
    pf.close()
