"""Batched races on CDDT (handle option ``race_cddt``; include/scanlib.h "Races on CDDT") on the MI355X: the race scan
against tests/race_cddt_statement.py bit for bit, past one round of the kernel's work, against the device's own stamp,
rebuild, scan where the two conditions hold, after a map update, under the race loops and the race environment (composed
the way the ray-marching race tests compose them, with this scan in the scan's place), and the refusals.  Every test sets
the option first."""
import math

import numpy as np
import pytest

import race_cddt_statement as S
import race_statement as RS
import seat_statement as SS
import support
from noise_checks import SEED_HI, check_noise
from oracle import np_statement as NS
from support import D_BASE, FOV, THRESH, same_bits
from test_gpu_race_env import RaceComposed, against_statement
from test_gpu_seats import small_net, teacher_forced
from pyracecarsimulator_amd import Policy, RaceEnv, ScanSimulator2D, _lib, maps, range_libc
from pyracecarsimulator_amd import racecar as RC

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

L, W = S.L, S.W
RL_ERR_INVALID, RL_ERR_UNSUPPORTED = -1, -4           # include/scanlib.h rl_status


def racing(omap, td, mrx=S.MRX):
    h = range_libc.PyCDDTCast(omap, mrx, td)
    h.set_option("race_cddt", 1)
    return h


@pytest.fixture(scope="module")
def world(oracle_mod):
    g = S.maze()
    omap = range_libc.PyOMap(g)
    tables = {}

    def table(td):
        if td not in tables:
            tables[td] = NS.CddtTable(g.occ, td)
        return tables[td]
    return dict(g=g, omap=omap, dt=oracle_mod.edt(g.occ), table=table, sincosf=oracle_mod.sincosf)


def clusters(g, dt, n_groups, group, seed, spread=0.8, clear=5):
    """Cars float64 (n_groups * group, 3): the cars of a race within ``spread`` m of a centre ``clear`` cells off the
    walls, wherever that puts them (walls and each other included: the statement holds everywhere)."""
    rng = np.random.default_rng(seed)
    pool = np.argwhere(dt >= clear)
    res, (ox, oy, _) = g.resolution, g.origin
    cars = np.zeros((n_groups, group, 3))
    for r in range(n_groups):
        rr, cc = pool[rng.integers(len(pool))]
        cars[r, :, 0] = ox + (cc + 0.5) * res + rng.uniform(-spread, spread, group)
        cars[r, :, 1] = oy + (rr + 0.5) * res + rng.uniform(-spread, spread, group)
        cars[r, :, 2] = rng.uniform(-math.pi, math.pi, group)
    return cars.reshape(-1, 3)


def with_specials(poses, cars, group):
    """One NaN lidar pose, one pose far outside the map (its ly leaves the bucket range), one other car off the grid."""
    if len(poses) >= 6:
        poses[1, 0] = np.nan
        poses[2, :2] = 1e6
        cars[group + (1 if group > 1 else 0), 0] = 100.0
    return poses, cars


def statement(world, td, poses, cars, group, beams, mrx=S.MRX, g=None, table=None):
    g = g or world["g"]
    cells = RS.outline_cells(cars, L, W, g.resolution, g.origin, g.rows, g.cols, world["sincosf"])
    return S.fan(table or world["table"](td), g.resolution, g.origin, mrx, poses, cells, group, FOV, beams)


def device_form(m, poses, cars, group, beams):
    import torch
    dev = torch.device("cuda:0")
    n = len(poses) * beams
    d_poses = torch.from_numpy(np.ascontiguousarray(poses, np.float32)).to(dev)
    d_cars = torch.from_numpy(np.ascontiguousarray(cars, np.float64)).to(dev)
    d_out = torch.full((n,), -3.0, dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    m.calc_range_fan_cars_device(d_poses.data_ptr(), d_cars.data_ptr(), len(poses) // group, group, FOV, beams,
                                 d_out.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    return d_out.cpu().numpy()


# ---------------------------------------------------------------- 1. the race scan against the statement
@pytest.mark.parametrize("beams", [10, 65, 1280])
@pytest.mark.parametrize("td", [36, 37, 108])                    # 37: the odd-theta_disc guard
def test_fan_cars_equal_the_statement(world, td, beams):
    """Groups 1, 2, 3 and 8 over 3 races on the 96-cell maze, host and device forms; a group of 1 is the plain fan."""
    g = world["g"]
    m = racing(world["omap"], td)
    n_changed = 0
    for group in (1, 2, 3, 8):
        cars = clusters(g, world["dt"], 3, group, 100 + group)
        poses, cars = with_specials(support.lidar_poses(cars), cars, group)
        got = m.calc_range_fan_cars(poses, cars, group, FOV, beams)
        want = statement(world, td, poses, cars, group, beams)
        assert same_bits(got, want), (group, int((got != want).sum()))
        assert same_bits(device_form(m, poses, cars, group, beams), want), group
        plain = np.empty(len(poses) * beams, np.float32)
        m.calc_range_fan(poses, plain, FOV, beams)
        if group == 1:
            assert same_bits(got, plain)
        else:
            assert (got <= plain).all()
            n_changed += int((got < plain).sum())
    assert n_changed > beams // 2                                  # the other cars are seen


def test_fan_cars_noise_is_keyed_by_the_global_ray_id(world):
    """theta_disc 108, 65 beams, 3 races of 3: a 64-bit seed and a ray offset across 2^32, against the reference normal
    of every ray's global id; with a group of 1 the noisy scan is the plain fan's, bit for bit."""
    g, td, beams, group = world["g"], 108, 65, 3
    m = racing(world["omap"], td)
    cars = clusters(g, world["dt"], 3, group, 7)
    poses = support.lidar_poses(cars)
    want = statement(world, td, poses, cars, group, beams)
    offset = (1 << 32) - 100
    check_noise(m, poses, FOV, beams, want, SEED_HI, offset, what="race_cddt_kernel",
                scan=lambda: m.calc_range_fan_cars(poses, cars, group, FOV, beams))
    m.set_noise(0.05, SEED_HI, offset)
    try:
        plain = np.empty(len(poses) * beams, np.float32)
        m.calc_range_fan(poses, plain, FOV, beams)
        assert same_bits(m.calc_range_fan_cars(poses, cars, 1, FOV, beams), plain)
        assert same_bits(device_form(m, poses, cars, 1, beams), plain)
    finally:
        m.set_noise(0.0, 0, 0)


# ---------------------------------------------------------------- 2. past one round of work
def test_more_units_than_lanes(world):
    """P = 8 at theta_disc 108: 8 x 54 = 432 (car, table bin) units for 256 lanes, 1280 beams: five rounds of stores."""
    g, td, beams, group = world["g"], 108, 1280, 8
    m = racing(world["omap"], td)
    cars = clusters(g, world["dt"], 2, group, 21)
    poses = support.lidar_poses(cars)
    got = m.calc_range_fan_cars(poses, cars, group, FOV, beams)
    assert same_bits(got, statement(world, td, poses, cars, group, beams))


def test_outlines_beyond_one_pass(world):
    """0.02 m per cell: the reference car's outline is 124 points, two 64-lane passes of the raster."""
    g = maps.make_maze(120, cell=30, wall=2, p=0.4, seed=9)
    g = maps.GridMap(g.occ, 0.02, (-1.2, -1.2, 0.0), "fine")
    n_l, n_w = RS.edge_counts(L, W, g.resolution)
    assert 2 * (n_l + n_w) == 124
    td, beams, group, mrx = 36, 65, 3, 80
    omap = range_libc.PyOMap(g)
    m = racing(omap, td, mrx)
    dt = omap.distance_transform()
    cars = clusters(g, dt, 3, group, 5, spread=0.4, clear=8)
    poses = support.lidar_poses(cars)
    got = m.calc_range_fan_cars(poses, cars, group, FOV, beams)
    want = statement(world, td, poses, cars, group, beams, mrx, g, NS.CddtTable(g.occ, td))
    assert same_bits(got, want)
    plain = np.empty(len(poses) * beams, np.float32)
    m.calc_range_fan(poses, plain, FOV, beams)
    assert (got < plain).any()


# ---------------------------------------------------------------- 3. the device's own stamp, rebuild, scan
def test_equals_stamp_rebuild_scan_where_the_conditions_hold(world):
    """One race of 3 cars that meets (i) and (ii): for each car the others' rl_car_outline_cells stamped on a second
    map, a plain CDDT handle's scan of it, the stamp taken off again."""
    g, td, beams, group = world["g"], 36, 97, 3
    cb = RC.CarBatch()
    m = racing(world["omap"], td)
    omap2 = range_libc.PyOMap(g)
    plain = range_libc.PyCDDTCast(omap2, S.MRX, td)
    rng = np.random.default_rng(11)
    for _ in range(50):                                            # (a host-side draw: the first line-up that qualifies)
        cars = S.lineup(g, world["dt"], rng, 7)[1]                 # three cars on cells with EDT >= 7
        lists = RS.outline_cells(cars, L, W, g.resolution, g.origin, g.rows, g.cols, world["sincosf"])
        if all(S.meets_conditions(g.occ, RS.others(lists, group, n)) for n in range(group)):
            break
    else:
        raise AssertionError("no line-up met the conditions")
    poses = support.lidar_poses(cars)
    got = m.calc_range_fan_cars(poses, cars, group, FOV, beams).reshape(group, beams)
    cells, counts = cb.outline_cells(omap2, cars)
    n_seen = 0
    for n in range(group):
        stamp = np.concatenate([cells[k, :counts[k]] for k in range(group) if k != n]).astype(np.int64)
        omap2.stamp_cells(stamp)
        one = np.empty(beams, np.float32)
        plain.calc_range_fan(poses[n:n + 1], one, FOV, beams)
        omap2.stamp_cells(np.zeros(0, np.int64))
        assert same_bits(got[n], one), n
        alone = np.empty(beams, np.float32)
        plain.calc_range_fan(poses[n:n + 1], alone, FOV, beams)
        n_seen += int((one != alone).sum())
    assert n_seen > 0


def test_the_race_scan_follows_a_map_update(world):
    g, td, beams, group = world["g"], 36, 65, 3
    omap = range_libc.PyOMap(g)
    m = racing(omap, td)
    cars = clusters(g, world["dt"], 3, group, 31)
    poses = support.lidar_poses(cars)
    before = m.calc_range_fan_cars(poses, cars, group, FOV, beams)
    assert same_bits(before, statement(world, td, poses, cars, group, beams))
    occ = g.occ.copy()
    occ[20:76:8, 10:86] = 1                                        # bars across the corridors
    omap.update(occ)
    g2 = maps.GridMap(occ, g.resolution, g.origin, "barred")
    after = m.calc_range_fan_cars(poses, cars, group, FOV, beams)
    assert same_bits(after, statement(world, td, poses, cars, group, beams, g=g2, table=NS.CddtTable(occ, td)))
    assert (after != before).any()


# ---------------------------------------------------------------- 4. the race loops
def room_rig(td=36):
    g = maps.make_room(120)
    omap = range_libc.PyOMap(g)
    m = racing(omap, td, 100)
    return dict(g=g, omap=omap, m=m, fg=support.followgap(), pol=Policy(layers=small_net(), in_start=5), cars=RC.CarBatch())


def room_states(g):
    """3 races of 3 in the walled room, far from its walls: in race 0 cars 0 and 1 nose to nose 0.85 m apart at 3 m/s
    (they meet within 12 ticks); the others spread out."""
    side = g.cols * g.resolution
    c = side / 2.0
    s = np.zeros((3, 3, 11))
    s[0, 0, :4] = (c - 0.425, c, 0.0, 3.0)
    s[0, 1, :4] = (c + 0.425, c, math.pi, 3.0)
    s[0, 2, :4] = (c, c + 1.2, 0.3, 2.0)
    rng = np.random.default_rng(3)
    for r in (1, 2):
        for k in range(3):
            s[r, k, :4] = (c + (k - 1) * 1.1 + rng.uniform(-0.1, 0.1), c + (r - 1.5) * 1.6 + rng.uniform(-0.1, 0.1),
                           rng.uniform(-math.pi, math.pi), 2.0)
    speeds = np.ascontiguousarray(s[:, :, 3])
    return s, speeds


def test_race_followgap_against_the_composed_loop():
    """R = 3, P = 3, 65 beams, 12 ticks, noise on: rl_car_race_followgap on the CDDT handle against the seated roll-out
    statement over the public calls (rollout, the CDDT race scan, is_crashed, FollowGap), link by link."""
    rig = room_rig()
    m, fg, cars, g = rig["m"], rig["fg"], rig["cars"], rig["g"]
    R, P, B, T = 3, 3, 65, 12
    N = R * P
    states, speeds = room_states(g)
    edge = support.edge(B)
    std, seed, base = 0.02, 3, 777
    m.set_noise(std, seed, base)
    try:
        first, final, vel, steers, sp, st = cars.race_followgap(m, fg, states, T, speeds, FOV, B, edge, THRESH, trace=True)
        pub = RaceComposed(m, cars, N, P, B, edge, 1, std, seed, base)
        w_first, w_final, w_steers, w_trace = SS.seated_rollout(
            states.reshape(N, 11), speeds.reshape(N), np.zeros(N, np.float32), T, [fg] * P, lambda d: False, 0.0,
            pub.step_cars, pub.scan, pub.is_crashed, lambda d, row: d.eval_many(np.ascontiguousarray(row[None]))[0])
        assert same_bits(first.reshape(N), w_first)
        assert same_bits(final.reshape(N, 11), w_final)
        for got, want in ((steers.reshape(N, T), w_steers), (st.reshape(N, T, 11), w_trace)):
            gone = np.isnan(want)                                  # (a wreck's rows: NaN in both, whatever its payload)
            assert (np.isnan(got) == gone).all() and same_bits(got[~gone], want[~gone])
        # one car drove into another: cars 0 and 1 of race 0 crash, and neither does alone
        assert (first[0, :2] >= 0).all(), first
        alone = cars.race_followgap(m, fg, states[:1, :2].reshape(2, 1, 11), T, speeds[:1, :2].reshape(2, 1), FOV, B,
                                    edge, THRESH)[0]
        assert (alone < 0).all(), alone
    finally:
        m.set_noise(0.0, 0, 0)


def test_race_seats_with_one_policy_seat():
    """The same races through rl_car_race_seats with the network in seat 1: test_gpu_seats' teacher-forced replay of
    every link over the public calls, on the CDDT handle."""
    rig = room_rig()
    states, speeds = room_states(rig["g"])
    try:
        census = teacher_forced(rig, [rig["fg"], rig["pol"], rig["fg"]], states, speeds, 12, 65, 0.2)
        assert census["crashed"] >= 2 and census["seen"] > 0, census
    finally:
        rig["m"].set_noise(0.0, 0, 0)


def test_race_env_against_the_statement():
    """RaceEnv on the CDDT handle, FollowGap scripted in seat 1: reset and 3 steps against the seated race-environment
    statement whose scan is the CDDT race scan."""
    rig = room_rig()
    m, fg, cars, g = rig["m"], rig["fg"], rig["cars"], rig["g"]
    R, P, B = 3, 3, 65
    pool, _ = room_states(g)
    edge = support.edge(B)
    std, seed, base = 0.02, 3, 555
    m.set_noise(std, seed, base)
    try:
        seats = [None, fg, None]
        env = RaceEnv(m, pool, R, B, FOV, edge, THRESH, car=cars, seats=seats, seat_speed=2.5, min_running=1)
        pub = RaceComposed(m, cars, R * P, P, B, edge, 1, std, seed, base)
        stmt = SS.SeatEnvStatement(pool, R, B, pub.step_cars, pub.scan, pub.is_crashed,
                                   lambda d, row: d.eval_many(np.ascontiguousarray(row[None]))[0], seats, 2.5,
                                   min_running=1, scan_dist_to_base=D_BASE)
        rng = np.random.default_rng(8)
        actions = np.stack([np.full((3, R * P), 3.0), rng.uniform(-0.3, 0.3, (3, R * P))], -1).astype(np.float32)
        against_statement(env, stmt, actions, 1)
        assert same_bits(env.seat_steers().reshape(-1), stmt.seat_steers())
        # the cars see each other: the last scan differs from the plain fan of the same poses at the same ray offsets
        alone = pub.scan_alone(support.lidar_poses(stmt.states), stmt.k)
        assert (stmt.ranges != alone).any() and not (stmt.ranges != alone).all()
    finally:
        m.set_noise(0.0, 0, 0)


# ---------------------------------------------------------------- 5. refusals and the option
def test_refusals_leave_the_handles_usable(world):
    g, omap = world["g"], world["omap"]
    cars = clusters(g, world["dt"], 2, 2, 3)
    poses = support.lidar_poses(cars)
    out = np.empty(4 * 65, np.float32)

    def refused(h, code, text=None, group=2, p=poses, c=cars, **kw):
        with pytest.raises(_lib.ScanLibError) as e:
            h.calc_range_fan_cars(p, c, group, FOV, 65, **kw)
        assert e.value.code == code and (text is None or text in str(e.value)), str(e.value)
        h.calc_range_fan(poses, out, FOV, 65)                      # still usable

    h = range_libc.PyCDDTCast(omap, S.MRX, 36)
    h.set_option("race_cddt", 0)
    refused(h, RL_ERR_UNSUPPORTED, "ray marching")                 # option 0: as today
    for cls, args in ((range_libc.PyGiantLUTCast, (36,)), (range_libc.PyBresenhamsLine, ())):
        t = cls(omap, S.MRX, *args)
        t.set_option("race_cddt", 1)                               # stored and ignored
        assert t.get_info("race_cddt") == 1
        refused(t, RL_ERR_UNSUPPORTED, "ray marching")
    m = racing(omap, 36)
    want = m.calc_range_fan_cars(poses, cars, 2, FOV, 65)
    n = 4 * 65
    refused(m, RL_ERR_UNSUPPORTED, "hit cells", hit_cells=np.empty((n, 2), np.int32))
    refused(m, RL_ERR_UNSUPPORTED, "hit cells", steps=np.empty(n, np.uint16))
    # the LDS bound: group x theta_disc <= 8192 per-bin ranges
    big = racing(omap, 1100)
    refused(big, RL_ERR_UNSUPPORTED, "8192", group=8, p=np.repeat(poses, 2, 0), c=np.repeat(cars, 2, 0))
    # 8 x 1024 = 8192, the bound itself, runs: with the other cars off the grid every car's scan is the plain fan's
    ok = racing(omap, 1024)
    p8, c8 = np.repeat(poses, 2, 0), np.repeat(cars, 2, 0)
    c8[:, 0] = 100.0
    plain = np.empty(8 * 65, np.float32)
    ok.calc_range_fan(p8, plain, FOV, 65)
    assert same_bits(ok.calc_range_fan_cars(p8, c8, 8, FOV, 65), plain)
    # a multi-device handle
    omap_m = range_libc.PyOMap(g, device=[0])
    mm = range_libc.PyCDDTCast(omap_m, S.MRX, 36, races=True)
    assert mm.get_info("race_cddt") == 1                           # the option went to the replica
    refused(mm, RL_ERR_INVALID, "single-device")
    assert same_bits(m.calc_range_fan_cars(poses, cars, 2, FOV, 65), want)


def test_get_info_reads_the_option(world):
    h = range_libc.PyCDDTCast(world["omap"], S.MRX, 36)
    assert h.get_info("race_cddt") == 0
    for v, want in ((0, 0), (1, 1), (7, 1)):
        h.set_option("race_cddt", v)
        assert h.get_info("race_cddt") == want
    assert range_libc.PyCDDTCast(world["omap"], S.MRX, 36, races=True).get_info("race_cddt") == 1
    g = world["g"]
    sim = ScanSimulator2D(65, FOV, 0.01, batch_size=4)
    sim.setMap(world["omap"], S.MRX, g.resolution, g.origin)
    for races in (False, True):
        sim.setRaytracingMethod("CDDT", theta_disc=36, races=races)
        assert isinstance(sim.scan_method, range_libc.PyCDDTCast) and sim.scan_method.theta_disc == 36
        assert sim.scan_method.get_info("race_cddt") == int(races)
