"""The origin-corrected GiantLUT query (option ``lut_refine``) on the MI355X: every query path of a GiantLUT handle
against tests/lut_refine_statement.py, bit for bit.  The statement reads the handle's own table (``table()``: the device
build is pinned to the oracle's elsewhere) and the oracle's distance transform."""
import numpy as np
import pytest

import lut_refine_statement as S
import support
from noise_checks import SEED_HI, check_noise
from oracle import np_statement as N
from support import D_BASE, THRESH, same_bits
from pyracecarsimulator_amd import DriveEnv, ScanSimulator2D, maps, range_libc
from pyracecarsimulator_amd import racecar as RC

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

FOV, MRX = 4.71, 60
FAR = 3.0e5          # a heading beyond 2^22 bins at every theta_disc used here (112 bins: 17.8 per radian)


class World:
    def __init__(self, oracle_mod):
        self.g = maps.make_maze(128, cell=16, wall=2, p=0.4, seed=5)
        self.om = oracle_mod.OracleMap.from_gridmap(self.g, MRX)
        self.dt = self.om.dt
        self.omap = range_libc.PyOMap(self.g, device=0)
        assert np.array_equal(self.omap.distance_transform(), self.dt)
        self._m = {}

    def method(self, td):
        """(refined handle, its table) at theta_disc ``td``, grid_mult 1 so that 2048 waves are a launch's most."""
        if td not in self._m:
            m = range_libc.PyGiantLUTCast(self.omap, MRX, td, refine=True)
            m.set_option("grid_mult", 1)
            self._m[td] = (m, m.table())
        return self._m[td]

    def poses(self, n, seed):
        """``n`` poses: clear and wall-hugging ones, integer-coordinate ones, border cells, an occupied cell, one outside
        the map and one heading beyond 2^22 bins."""
        g, res = self.g, self.g.resolution
        ox, oy, _ = g.origin
        special = np.array([[ox - 1.0, oy + 1.0, 0.3],                                   # outside the map
                            [ox + 0.6 * res, oy + 40.3 * res, 1.0],                     # in the border wall
                            [ox + 127.7 * res, oy + 127.8 * res, -2.0],                 # the last cell: both corners clamp
                            [ox + 127.6 * res, oy + 50.2 * res, 0.5],
                            [ox + 60.4 * res, oy + 127.9 * res, 2.5]], np.float32)
        ints = S.integer_poses(g, self.dt, 16, seed + 1)
        k = n - len(special) - len(ints)
        p = np.concatenate([maps.sample_free_poses(g, k // 2, seed, 2.0, dt=self.dt),
                            S.near_wall_poses(g, self.dt, k - k // 2, seed + 2), ints, special])
        p[7, 2] = FAR
        return np.ascontiguousarray(p)

    def want_fan(self, lut, poses, fov, beams):
        return S.lut_refine_fan(lut, self.dt, self.g.resolution, self.g.origin, MRX, poses, fov, beams)


@pytest.fixture(scope="module")
def world(oracle_mod):
    return World(oracle_mod)


def scan(m, poses, fov, beams):
    out = np.full(len(poses) * beams, -7.0, np.float32)
    m.calc_range_fan(poses, out, fov, beams)
    return out


def test_pose_mix_holds_every_case(world):
    p = world.poses(2200, 1)
    took, fell = S.census(world.dt, world.g.resolution, world.g.origin, p)
    assert took >= 20 and fell >= 20, (took, fell)
    gx, gy, _ = N._pose_grid(world.g.resolution, world.g.origin, p)
    inb, c, r, fx, fy, _, _ = S.corner(world.dt, gx, gy)
    assert (~inb).sum() == 1 and (world.dt[r[inb], c[inb]] == 0).any()
    assert (gx[inb] >= 127.5).any() and (gy[inb] >= 127.5).any() and ((fx == 0) & (fy == 0) & inb).sum() >= 16


# theta_disc 112 / 700 / 1442: one, two, three 16-B loads per lane and row; 720 / 1081 beams: 12 / 17 chunks
@pytest.mark.parametrize("td,beams,debug,name", [
    (112, 720, 0, "scan::lut_fan_lds_kernel<1, 12>"), (112, 1081, 0, "scan::lut_fan_lds_kernel<1, 17>"),
    (700, 720, 0, "scan::lut_fan_lds_kernel<2, 12>"), (700, 1081, 0, "scan::lut_fan_lds_kernel<2, 17>"),
    (1442, 720, 0, "scan::lut_fan_lds_kernel<3, 12>"), (1442, 1081, 0, "scan::lut_fan_lds_kernel<3, 17>"),
    (701, 720, 0, "scan::lut_fan_kernel<12>"), (701, 1081, 0, "scan::lut_fan_kernel<17>"),
    (700, 720, 4, "scan::lut_fan_kernel<12>"), (700, 1081, 4, "scan::lut_fan_kernel<17>"),
    (700, 10, 0, "scan::lut_fan_lds_kernel<2, 12>"), (700, 64, 0, "scan::lut_fan_lds_kernel<2, 12>"),
    (700, 65, 0, "scan::lut_fan_lds_kernel<2, 12>"), (700, 1088, 0, "scan::lut_fan_lds_kernel<2, 17>"),
    (700, 1280, 0, "scan::lut_fan_kernel<17>")])
def test_every_refined_fan_instance_equals_the_statement(world, td, beams, debug, name):
    """The plan names the default instance, the launch takes its refined twin; more poses than the launch has waves, so
    that every wave's pose loop iterates (twice for the 1280-beam fan's two rounds per pose)."""
    m, lut = world.method(td)
    m.set_option("lut_debug", debug)
    try:
        poses = world.poses(2200, td + beams)
        got = scan(m, poses, FOV, beams)
        pl = m.last_plan()
        assert pl["name"] == name, pl
        assert len(poses) > 4 * m.get_info("last_grid")
        want = world.want_fan(lut, poses, FOV, beams)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (np.flatnonzero(got != want)[:8], int((got != want).sum()))
        plain = N.lut_fan(lut, world.g.occ.shape, world.g.resolution, world.g.origin, MRX, poses, FOV, beams)
        assert (got != plain).mean() > 0.5               # (and it is not the default query)
    finally:
        m.set_option("lut_debug", 0)


def test_general_path_negative_fov_and_noise(world):
    m, lut = world.method(1442)
    poses = world.poses(2200, 77)
    for beams in (1081, 720):
        got = scan(m, poses, -FOV, beams)
        assert np.array_equal(got, world.want_fan(lut, poses, -FOV, beams)), beams
    # noise: the default's normals for the same ray ids, added to the corrected range (LDS kernel and fall-back kernel)
    for td in (1442, 701):
        m, lut = world.method(td)
        p = poses[:300]
        check_noise(m, p, FOV, 1081, world.want_fan(lut, p, FOV, 1081), SEED_HI, 2 ** 32 - 1000, what="refined td %d" % td)
    # ... and the per-ray call
    g, rows = world.g, poses[:700]

    def many():
        out = np.full(len(rows), -7.0, np.float32)
        m.calc_range_many(rows, out)
        return out
    check_noise(m, None, None, None, S.lut_refine_rays(lut, world.dt, g.resolution, g.origin, MRX, rows), SEED_HI, 5, scan=many,
                what="refined rows")


def test_option_reads_back_and_switching_off_restores_the_default(world):
    m, lut = world.method(700)
    fresh = range_libc.PyGiantLUTCast(world.omap, MRX, 700)
    fresh.set_option("grid_mult", 1)
    assert fresh.get_info("lut_refine") == 0 and m.get_info("lut_refine") == 1
    poses = world.poses(2200, 5)
    try:
        m.set_option("lut_refine", 0)
        assert m.get_info("lut_refine") == 0
        a, b = scan(m, poses, FOV, 1081), scan(fresh, poses, FOV, 1081)
        assert same_bits(a, b) and m.last_plan() == fresh.last_plan()
        assert np.array_equal(a, N.lut_fan(lut, world.g.occ.shape, world.g.resolution, world.g.origin, MRX, poses, FOV, 1081))
        rows = np.ascontiguousarray(poses[:500])
        ra, rb = np.empty(500, np.float32), np.empty(500, np.float32)
        m.calc_range_many(rows, ra)
        fresh.calc_range_many(rows, rb)
        assert same_bits(ra, rb)
        m.set_option("lut_refine", 7)                      # any other value stores 1
        assert m.get_info("lut_refine") == 1
        assert np.array_equal(scan(m, poses, FOV, 1081), world.want_fan(lut, poses, FOV, 1081))
    finally:
        m.set_option("lut_refine", 1)


def test_rows_repeat_angles_and_sensor_weights(world):
    m, lut = world.method(1442)
    g = world.g
    rows = world.poses(3000, 9)
    got = np.empty(len(rows), np.float32)
    m.calc_range_many(rows, got)
    assert np.array_equal(got, S.lut_refine_rays(lut, world.dt, g.resolution, g.origin, MRX, rows))
    # the fan's own angles: the refined fan; an arbitrary table: the statement
    p = world.poses(600, 10)
    for beams in (65, 1081):
        ang = N._fan_alpha(FOV, beams)
        out = np.empty(len(p) * beams, np.float32)
        m.calc_range_repeat_angles(p, ang, out)
        assert np.array_equal(out, scan(m, p, FOV, beams)), beams
    ang = np.random.default_rng(4).uniform(-7.0, 7.0, 77).astype(np.float32)
    out = np.empty(len(p) * 77, np.float32)
    m.calc_range_repeat_angles(p, ang, out)
    assert np.array_equal(out, S.lut_refine_angles(lut, world.dt, g.resolution, g.origin, MRX, p, ang))
    # weights of the fused call = eval_sensor_model of the refined ranges
    width = MRX + 1
    table = np.random.default_rng(5).uniform(0.5, 1.5, (width, width))
    m.set_sensor_model(table)
    obs = out[:77].copy()
    fused, apart = np.empty(len(p)), np.empty(len(p))
    m.calc_range_repeat_angles_eval_sensor_model(p, ang, obs, fused)
    m.eval_sensor_model(obs, out, apart, 77, len(p))
    assert same_bits(fused, apart)


def test_corner_fallback_follows_a_stamped_wall(world, oracle_mod):
    """A pose whose nearest corner belongs to a free neighbour cell; a wall stamped on that cell turns the corner choice
    back to the pose's own cell — the dt probe reads the live map — and the table is rebuilt."""
    g = world.g
    omap = range_libc.PyOMap(g, device=0)
    m = range_libc.PyGiantLUTCast(omap, MRX, 112, refine=True)
    poses = world.poses(400, 21)
    gx, gy, _ = N._pose_grid(g.resolution, g.origin, poses)
    inb, c, r, _, _, _, _ = S.corner(world.dt, gx, gy)
    moved = np.flatnonzero(inb & ((c != np.trunc(gx)) | (r != np.trunc(gy))))[:40]
    assert moved.size == 40
    before = scan(m, poses, FOV, 270)
    assert np.array_equal(before, world.want_fan(m.table(), poses, FOV, 270))
    omap.stamp_cells(r[moved] * g.cols + c[moved])
    occ2 = g.occ.copy()
    occ2[r[moved], c[moved]] = 1
    om2 = oracle_mod.OracleMap(occ2, g.resolution, g.origin, MRX)
    _, c2, r2, _, _, _, fell = S.corner(om2.dt, gx, gy)
    assert fell[moved].all() and (c2[moved] == np.trunc(gx[moved])).all()
    after = scan(m, poses, FOV, 270)
    want = S.lut_refine_fan(m.table(), om2.dt, g.resolution, g.origin, MRX, poses, FOV, 270)
    assert np.array_equal(after, want) and not np.array_equal(after, before)
    # ... and through rl_map_update
    omap.update(g.occ)
    assert np.array_equal(scan(m, poses, FOV, 270), before)


def test_free_border_cells_clamp_the_corner(oracle_mod):
    """A map whose last column and row are free: gx in [cols - 0.5, cols) takes the last column's corner, not a cell
    past the row's end."""
    occ = np.zeros((48, 40), np.uint8)
    occ[10:14, 5:30] = 1
    occ[30, 37:] = 1
    g = maps.GridMap(occ, 0.05, (0.0, 0.0, 0.0), "free_border")
    om = oracle_mod.OracleMap.from_gridmap(g, 50)
    rng = np.random.default_rng(2)
    n = 300
    gx = np.where(rng.random(n) < 0.5, 39.5 + 0.5 * rng.random(n), 40 * rng.random(n))
    gy = np.where(rng.random(n) < 0.5, 47.5 + 0.5 * rng.random(n), 48 * rng.random(n))
    poses = np.stack([gx * 0.05, gy * 0.05, rng.uniform(-np.pi, np.pi, n)], 1).astype(np.float32)
    pgx, pgy, _ = N._pose_grid(g.resolution, g.origin, poses)
    assert ((pgx >= 39.5) & (pgx < 40)).sum() > 50 and ((pgy >= 47.5) & (pgy < 48)).sum() > 50
    m = range_libc.PyGiantLUTCast(range_libc.PyOMap(g, device=0), 50, 112, refine=True)
    got = scan(m, poses, FOV, 100)
    assert np.array_equal(got, S.lut_refine_fan(m.table(), om.dt, g.resolution, g.origin, 50, poses, FOV, 100))
    rows = np.empty(n, np.float32)
    m.calc_range_many(poses, rows)
    assert np.array_equal(rows, S.lut_refine_rays(m.table(), om.dt, g.resolution, g.origin, 50, poses))


def test_consumers_of_the_fan_launch_inherit_the_option(world):
    g = world.g
    m, lut = world.method(112)
    # a multi-device handle forwards the option to every replica and gives the single-device bits
    momap = range_libc.PyOMap(g, device=[0, 0])
    mm = range_libc.PyGiantLUTCast(momap, MRX, 112, refine=True)
    assert mm.n_devices == 2 and mm.get_info("lut_refine") == 1 and mm.replica(1).get_info("lut_refine") == 1
    poses = world.poses(2200, 31)
    assert same_bits(scan(mm, poses, FOV, 270), scan(m, poses, FOV, 270))
    # the driving environment scans its lidar poses through the handle's fan launch
    n, beams = 40, 100
    states, _ = support.starts(g, world.dt, n, 8, 3.0)
    env = DriveEnv(m, states, n, beams, FOV, support.edge(beams), THRESH, auto_reset=False, car=RC.CarBatch())
    obs = env.reset(seed=1, start_index=np.arange(n))
    assert same_bits(obs.ravel(), world.want_fan(lut, support.lidar_poses(states, D_BASE), FOV, beams))
    act = np.stack([np.full(n, 2.0), np.linspace(-0.3, 0.3, n)], -1).astype(np.float32)
    obs, _, _ = env.step(act)
    now = env.read()["states"]
    assert not np.array_equal(now, states)
    assert same_bits(obs.ravel(), world.want_fan(lut, support.lidar_poses(now, D_BASE), FOV, beams))
    env.close()
    # ScanSimulator2D passes the option on ("GLT"; theta_disc defaults to one bin per beam spacing)
    sim = ScanSimulator2D(100, FOV, 0.01, batch_size=8)
    sim.setMap(world.omap, MRX, g.resolution, g.origin)
    sim.setRaytracingMethod("GLT", theta_disc=112, lut_refine=True)
    assert sim.scan_method.get_info("lut_refine") == 1
    assert same_bits(sim.scanMany(poses[:8]).copy(), world.want_fan(lut, poses[:8], FOV, 100))
    assert same_bits(sim.scan(*poses[3]).copy(), world.want_fan(lut, poses[3:4], FOV, 100))
    wide = ScanSimulator2D(1081, FOV, 0.01, batch_size=1)
    wide.setMap(world.omap, MRX, g.resolution, g.origin)
    wide.setRaytracingMethod("GLT")
    assert wide.scan_method.theta_disc == 1442 and wide.scan_method.get_info("lut_refine") == 0
    # the other kinds store the option and ignore it
    for other in (range_libc.PyCDDTCast(world.omap, MRX, 112), range_libc.PyRayMarchingGPU(world.omap, MRX)):
        before = scan(other, poses[:200], FOV, 270)
        other.set_option("lut_refine", 1)
        assert other.get_info("lut_refine") == 1
        assert same_bits(scan(other, poses[:200], FOV, 270), before)
