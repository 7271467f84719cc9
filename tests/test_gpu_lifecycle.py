"""Handle lifecycle on the MI355X: a long-running caller (the reference's ROS node builds a new
PyOMap on every map message, /root/reference/scripts/ros_interface.py:202-223, and the two-player
simulator rebuilds its map and CDDT table on every tick, scripts/two_player/rcs_two_player.py:110-121)
must get back every byte of HBM and pinned memory a destroyed handle held."""
import gc

import numpy as np
import pytest

import support
from pyracecarsimulator_amd import _lib, maps, range_libc
from pyracecarsimulator_amd.mcts import MCTSPlanner
from pyracecarsimulator_amd.particle_filter import ParticleFilter
from pyracecarsimulator_amd.policy import Policy
from pyracecarsimulator_amd.racecar import CarBatch
from pyracecarsimulator_amd.scan_simulator import ScanSimulator2D

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]


def _free_bytes(torch):
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _one_life(g, poses, B, fov, with_big_tables):
    """Everything a caller can create, used once, then dropped."""
    omap = range_libc.PyOMap(g)
    kinds = [(range_libc.PyRayMarchingGPU, ()), (range_libc.PyRayMarching, ()),
             (range_libc.PyBresenhamsLine, ()), (range_libc.PyCDDTCast, (108,))]
    if with_big_tables:
        kinds.append((range_libc.PyGiantLUTCast, (180,)))
    outs = []
    for cls, args in kinds:
        m = cls(omap, 120, *args)
        out = np.empty(len(poses) * B, np.float32)
        m.calc_range_fan(poses, out, fov, B)
        rays = np.repeat(poses[:4], 8, axis=0).astype(np.float32)
        out2 = np.empty(len(rays), np.float32)
        m.calc_range_many(rays, out2)
        outs.append(out[:16].copy())
        m.close()
    # a map update with methods alive (tables rebuilt in place), then the other handle kinds
    m = range_libc.PyCDDTCast(omap, 120, 108)
    occ2 = g.occ.copy()
    occ2[5:9, 5:9] = 1
    omap.update(occ2)
    out = np.empty(len(poses) * B, np.float32)
    m.calc_range_fan(poses, out, fov, B)
    sim = ScanSimulator2D(B, fov, 0.0, batch_size=len(poses))
    sim.setMap(omap, 120, g.resolution, g.origin)
    sim.setRaytracingMethod("RMGPU")
    sim.scanMany(poses.astype(np.float64))
    fg = support.followgap(inc=fov / B)
    fg.eval(out[:B].copy(), B)
    car = CarBatch(device=0)
    pin = _lib.pinned_zeros((len(poses) * B,), np.float32)
    m.calc_range_fan(poses, pin, fov, B)
    del pin, car, fg, sim
    m.close()
    omap.close()
    return outs


def test_create_use_destroy_cycles_return_all_device_memory():
    torch = pytest.importorskip("torch")
    g = maps.make_maze(160, cell=20, wall=2, p=0.4, seed=5, origin=(-1.0, 0.5, 0.2))
    B, fov = 271, 4.71
    poses = maps.sample_free_poses(g, 96, 11)
    first = _one_life(g, poses, B, fov, True)          # warm-up: runtime pools, code objects, torch context
    _one_life(g, poses, B, fov, True)
    gc.collect()
    base = _free_bytes(torch)
    for i in range(40):
        again = _one_life(g, poses, B, fov, i % 8 == 0)
        for a, b in zip(first, again):
            assert np.array_equal(a, b)                # and a fresh handle computes the same bits
    gc.collect()
    leaked = base - _free_bytes(torch)
    # the HIP runtime may keep a pool block or two; a leaked table would be tens of MB after 40 lives
    assert leaked <= 8 << 20, "%.1f MB of device memory not returned after 40 create/destroy cycles" % (leaked / 2**20)


def test_map_update_in_place_does_not_grow_memory():
    """The two-player tick: same map handle, rl_map_update + CDDT rebuild + scan, thousands of times."""
    torch = pytest.importorskip("torch")
    g = maps.make_maze(200, cell=25, wall=2, p=0.4, seed=8)
    omap = range_libc.PyOMap(g)
    m = range_libc.PyCDDTCast(omap, 150, 108)
    rm = range_libc.PyRayMarchingGPU(omap, 150)
    B, fov = 360, 6.2
    poses = maps.sample_free_poses(g, 8, 3)
    out = np.empty(len(poses) * B, np.float32)
    rng = np.random.default_rng(0)

    def tick():
        occ = g.occ.copy()
        r, c = rng.integers(10, 180, 2)
        occ[r:r + 6, c:c + 10] = 1                     # the opponent's car drawn into the grid
        omap.update(occ)
        m.calc_range_fan(poses, out, fov, B)
        rm.calc_range_fan(poses, out, fov, B)

    for _ in range(20):
        tick()
    base = _free_bytes(torch)
    for _ in range(300):
        tick()
    leaked = base - _free_bytes(torch)
    assert leaked <= 4 << 20, "%.1f MB grown over 300 ticks" % (leaked / 2**20)


def test_stamp_growth_cycles_return_device_memory():
    """rl_map_stamp_cells growing its index buffers (n past stamp_cap) and shrinking back, over and over, then the map
    destroyed: the device memory is back at its starting level."""
    torch = pytest.importorskip("torch")
    g = maps.make_maze(200, cell=25, wall=2, p=0.4, seed=9)
    B, fov = 180, 6.2
    poses = maps.sample_free_poses(g, 8, 4)
    out = np.empty(len(poses) * B, np.float32)
    rng = np.random.default_rng(2)

    def life(cycles):
        omap = range_libc.PyOMap(g)
        m = range_libc.PyRayMarchingGPU(omap, 120)
        for _ in range(cycles):
            for n in (10, 5000, 10):
                omap.stamp_cells(rng.choice(g.occ.size, n, replace=False))
                m.calc_range_fan(poses, out, fov, B)
        m.close()
        omap.close()

    life(2)                                            # warm-up: runtime pools, code objects
    gc.collect()
    base = _free_bytes(torch)
    for _ in range(20):                                # each life grows the buffers once, then reuses them
        life(3)
    gc.collect()
    leaked = base - _free_bytes(torch)
    assert leaked <= 4 << 20, "%.1f MB not returned after 20 maps of stamp growth cycles" % (leaked / 2**20)


def _every_handle_life(g, poses, B, fov):
    """One life of what the first test leaves out: policy, closed-loop drives and races, the race scan, roll-outs,
    outline cells, the MCTS planner and its drive, sensor model + repeat-angle calls + particle filter, and multi-device
    handles — each created, used once and dropped.  Returns (16 ranges of one scan, the planner's chosen actions)."""
    rng = np.random.default_rng(3)
    edge = support.edge(B, fov)
    states = np.zeros((4, 11))
    states[:, :3] = poses[:4]
    omap = range_libc.PyOMap(g)
    m = range_libc.PyRayMarchingGPU(omap, 120)
    cars = CarBatch()
    fg = support.followgap(inc=fov / B)
    # the smallest network of tests/test_gpu_policy.py: 3 -> 1, window [7, 10)
    pol = Policy.from_arrays([(rng.standard_normal((3, 1)).astype(np.float32), np.zeros(1, np.float32))], (False,),
                             in_start=7, clip=12.5, scale=7.0)
    pol.predict_many(np.ones((2, 10), np.float32))
    cars.drive_followgap(m, fg, states[:2], 4, 2.0, fov, B, edge, 0.001)
    cars.drive_policy(m, pol, states[:2], 4, 2.0, fov, B, edge, 0.001, steer_clip=0.4189)
    cars.race_followgap(m, fg, states.reshape(2, 2, 11), 4, 2.0, fov, B, edge, 0.001)
    ranges = m.calc_range_fan_cars(poses[:4], states[:, :3], 2, fov, B)[:16].copy()
    cars.rollout(states, np.tile([2.0, 0.1], (4, 2, 1)), n_steps=8, action_every=4)
    cars.outline_cells(omap, states[:, :3])
    pl = MCTSPlanner(cars, m, 4, 16, fov, B, edge, 0.001, source="fg", followgap=fg, rollout_steps=8, action_every=4)
    pl.reset(states, 0.0, np.arange(4, dtype=np.uint64))
    pl.run(6)
    chosen = pl.best()[0].copy()
    pl.read_tree(0)
    pl.close()
    cars.drive_mcts(m, fg, states, 2, 6, np.arange(4), fov, B, edge, 0.001, rollout_steps=8, action_every=4)
    # particle-filter weights: two tables of two widths on one method (the first one is freed), the three repeat-angle
    # calls on ray marching and on CDDT (whose fused call takes the launch context's scratch), then a filter
    P, A = 64, 16
    parts = np.ascontiguousarray(np.resize(poses, (P, 3)), np.float32)
    angles = np.linspace(-2.0, 2.0, A).astype(np.float32)
    obs = np.full(A, 1.5, np.float32)
    cd = range_libc.PyCDDTCast(omap, 120, 108)
    for h in (m, cd):
        for width in (32, 48):
            h.set_sensor_model(np.ascontiguousarray(rng.uniform(0.1, 1.0, (width, width))))
        r, w = np.empty(P * A, np.float32), np.empty(P)
        h.calc_range_repeat_angles(parts, angles, r)
        h.eval_sensor_model(obs, r, w, A, P)
        h.calc_range_repeat_angles_eval_sensor_model(parts, angles, obs, w)
    pf = ParticleFilter(m, angles, P, motion_std=(0.02, 0.02, 0.01))
    pf.reset(parts.astype(np.float64), seed=1)
    pf.run(np.tile([0.05, 0.0, 0.01], (2, 1)), np.tile(obs, (2, 1)))
    pf.read()
    pf.close()
    cd.close()
    # several devices behind one handle (device 0 named twice), the batch cut in two
    mmap = range_libc.PyOMap(g, device=[0, 0])
    mm = range_libc.PyRayMarchingGPU(mmap, 120)
    mcar = CarBatch(device=[0, 0])
    mm.set_option("multi_min_poses", 1)
    out = np.empty(8 * B, np.float32)
    mm.calc_range_fan(poses[:8], out, fov, B)
    mcar.close()
    mm.close()
    mmap.close()
    for h in (pol, fg):                                # (close() twice: the second call finds nothing to give back)
        h.close()
        h.close()
        assert not h._h.value
    cars.close()
    m.close()
    omap.close()
    return ranges, chosen


def test_every_handle_kind_returns_all_device_memory():
    """The handles the first test does not reach, 20 lives of each: the same bound on what is not returned.  At these
    shapes most buffers of the planner, the filter and the car are a few KB, so the bound catches a leaked map, table or
    scan buffer, not every member: that no member can be forgotten is what the owners of csrc/abi_internal.h and
    tests/test_host.py::test_housekeeping_gates guarantee."""
    torch = pytest.importorskip("torch")
    g = maps.make_maze(160, cell=20, wall=2, p=0.4, seed=5, origin=(-1.0, 0.5, 0.2))
    B, fov = 271, 4.71
    poses = maps.sample_free_poses(g, 96, 11)
    first = _every_handle_life(g, poses, B, fov)       # warm-up: runtime pools, code objects, torch context
    _every_handle_life(g, poses, B, fov)
    gc.collect()
    base = _free_bytes(torch)
    for _ in range(20):
        again = _every_handle_life(g, poses, B, fov)
        for a, b in zip(first, again):
            assert a.tobytes() == b.tobytes()          # and fresh handles compute the same bits
    gc.collect()
    leaked = base - _free_bytes(torch)
    print("not returned after 20 lives: %.2f MB" % (leaked / 2**20))
    assert leaked <= 8 << 20, "%.1f MB of device memory not returned after 20 create/destroy cycles" % (leaked / 2**20)
