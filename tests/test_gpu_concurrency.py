"""Concurrency promises of the C ABI (include/scanlib.h "Rules of the boundary"), on the MI355X:
one method handle used from several streams at once (bench.py's pipelined steps), one handle
shared by threads (the reference's rospy timer + subscriber callbacks,
/root/reference/scripts/ros_interface.py:107-115,142,189), a map updated while scans run."""
import threading

import numpy as np
import pytest

import support
from drive_cases import maze_case
from support import FOV, THRESH, same_bits
from pyracecarsimulator_amd import DriveEnv, maps, range_libc
from pyracecarsimulator_amd import racecar as RC
from pyracecarsimulator_amd.mcts import MCTSPlanner
from pyracecarsimulator_amd.pipeline import concurrent_streams

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]


@pytest.mark.parametrize("opts", [
    {},                                            # defaults: small map -> records derived in the march kernel
    {"inline_map_kb": 0},                          # big-map policy: keys-only binning launch + inline march
    {"inline_map_kb": 0, "order_inline": 0, "stripe_max": 0},   # binning launch writes records
    {"inline_map_kb": 0, "bin_multi_min": 64},     # grid-wide binning kernels (hist / keys scratch)
    {"grid_mult": 4},                              # half-machine grids: two launches co-resident
    {"grid_mult": 3, "slots": 2},                  # bench.py's pipelined configuration: two rays per lane
])
def test_interleaved_batches_on_concurrent_streams_are_bit_exact(oracle_mod, opts):
    """Batches enqueued round robin on 3 concurrent streams through ONE handle: each stream's
    launch context has its own pose records / tile order, so overlapping launches cannot corrupt
    one another; every batch equals the oracle bit for bit."""
    torch = pytest.importorskip("torch")
    g = maps.make_maze(600, cell=40, wall=3, p=0.45, seed=31, origin=(-4.0, 2.0, 0.3))
    om = oracle_mod.OracleMap.from_gridmap(g, 300)
    omap = range_libc.PyOMap(g)
    B, fov = 1081, 4.71
    m = range_libc.PyRayMarchingGPU(omap, 300)
    for k, v in opts.items():
        m.set_option(k, v)
    streams = concurrent_streams(3)
    assert len(streams) >= 2, "this box runs no two streams concurrently"
    sizes = [3000, 2000, 700]                     # a different batch per stream
    batches = [maps.sample_free_poses(g, n, 40 + i, dt=om.dt) for i, n in enumerate(sizes)]
    want = [om.rm_fan(p, fov, B, step_coeff=1.0, nthreads=oracle_mod.max_threads())[0] for p in batches]
    d_poses = [torch.from_numpy(p).cuda() for p in batches]
    d_out = [torch.zeros(len(p) * B, dtype=torch.float32, device="cuda") for p in batches]
    torch.cuda.synchronize()
    for rep in range(12):
        for i in range(len(batches)):
            s = streams[i % len(streams)]
            m.calc_range_fan_device(d_poses[i].data_ptr(), len(batches[i]), fov, B, d_out[i].data_ptr(),
                                    stream=s.cuda_stream)
    torch.cuda.synchronize()
    for i in range(len(batches)):
        assert np.array_equal(d_out[i].cpu().numpy(), want[i]), i
    # grouped crash test on two streams at once (per-stream crash marks)
    edge = support.oracle_edge(oracle_mod, B, fov)
    d_edge = torch.from_numpy(edge).cuda()
    firsts = [torch.zeros(len(p) // 100, dtype=torch.int32, device="cuda") for p in batches]
    for rep in range(6):
        for i in range(len(batches)):
            s = streams[i % len(streams)]
            m.check_collision_groups_device(d_poses[i].data_ptr(), len(batches[i]) // 100, 100, fov, B,
                                            d_edge.data_ptr(), 0.001, firsts[i].data_ptr(),
                                            d_out[i].data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    for i, p in enumerate(batches):
        exp = [oracle_mod.is_crashed(want[i][k * 100 * B:(k + 1) * 100 * B], B, 100, edge, 0.001)
               for k in range(len(p) // 100)]
        assert firsts[i].cpu().numpy().tolist() == exp, i


def test_more_streams_than_launch_contexts(oracle_mod):
    """Two streams more than a handle has launch contexts (rl_launch_contexts): contexts are handed over
    after a device synchronisation, results stay exact."""
    torch = pytest.importorskip("torch")
    from pyracecarsimulator_amd import _lib
    n_streams = _lib.lib().rl_launch_contexts() + 2
    g = maps.make_maze(300, cell=30, wall=2, p=0.5, seed=5)
    om = oracle_mod.OracleMap.from_gridmap(g, 200)
    omap = range_libc.PyOMap(g)
    m = range_libc.PyRayMarching(omap, 200)
    m.set_option("variant", 1)
    m.set_option("inline_map_kb", 0)
    B, fov = 360, 6.0
    streams = [torch.cuda.Stream() for _ in range(n_streams)]
    batches = [maps.sample_free_poses(g, 600 + 50 * i, 70 + i, dt=om.dt) for i in range(n_streams)]
    d_poses = [torch.from_numpy(p).cuda() for p in batches]
    d_out = [torch.zeros(len(p) * B, dtype=torch.float32, device="cuda") for p in batches]
    for rep in range(3):
        for i, s in enumerate(streams):
            m.calc_range_fan_device(d_poses[i].data_ptr(), len(batches[i]), fov, B, d_out[i].data_ptr(),
                                    stream=s.cuda_stream)
    torch.cuda.synchronize()
    for i, p in enumerate(batches):
        assert np.array_equal(d_out[i].cpu().numpy(), om.rm_fan(p, fov, B, nthreads=4)[0]), i


def test_threads_share_one_method_handle(oracle_mod):
    """The rospy pattern: a timer thread calling scan() (one pose, 4-arg calc_range_many) and a
    callback thread calling scanMany() / the fused crash test on the SAME range method object, a few
    thousand calls, every result checked against the oracle."""
    g = maps.load_colombia()
    mrx, B, fov = 300, 1081, 4.71
    om = oracle_mod.OracleMap.from_gridmap(g, mrx)
    omap = range_libc.PyOMap(g)
    m = range_libc.PyRayMarchingGPU(omap, mrx)
    poses = maps.sample_free_poses(g, 64, 9, dt=om.dt)
    want = om.rm_fan(poses, fov, B, step_coeff=1.0, nthreads=4)[0].reshape(len(poses), B)
    edge = support.oracle_edge(oracle_mod, B, fov)
    errors = []

    def scan_thread(n_calls):
        ins = np.zeros((B, 3), np.float32)
        outs = np.zeros(B, np.float32)
        try:
            for k in range(n_calls):
                p = k % len(poses)
                ins[0] = poses[p]
                m.calc_range_many(ins, outs, fov, B)          # scan(): scripts/scan_simulator.py:103-106
                if not np.array_equal(outs, want[p]):
                    errors.append(("scan", k))
                    return
        except Exception as e:                                  # noqa: BLE001
            errors.append(("scan", repr(e)))

    def many_thread(n_calls):
        nb = 8
        ins = np.zeros((nb * B, 3), np.float32)
        outs = np.zeros(nb * B, np.float32)
        try:
            for k in range(n_calls):
                p0 = (3 * k) % (len(poses) - nb)
                ins[::B] = poses[p0:p0 + nb]
                m.calc_range_many(ins, outs, fov, B)          # scanMany(): scripts/scan_simulator.py:130-133
                if not np.array_equal(outs, want[p0:p0 + nb].ravel()):
                    errors.append(("scanMany", k))
                    return
                if k % 4 == 0:                                  # checkCollisionMany on the same handle
                    code = m.check_collision_many(poses[p0:p0 + nb], fov, B, edge, 0.001)
                    if code != oracle_mod.is_crashed(want[p0:p0 + nb].ravel(), B, nb, edge, 0.001):
                        errors.append(("crash", k))
                        return
        except Exception as e:                                  # noqa: BLE001
            errors.append(("scanMany", repr(e)))

    threads = [threading.Thread(target=scan_thread, args=(3000,)),
               threading.Thread(target=many_thread, args=(1500,)),
               threading.Thread(target=scan_thread, args=(3000,))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
        assert not t.is_alive()
    assert not errors, errors[:3]


def test_map_update_thread_races_scan_threads(oracle_mod):
    """A map callback thread swaps the occupancy between two grids (rl_map_update) while two scan
    threads keep scanning through methods of that map: every scan must equal the oracle on ONE of the
    two grids, never a mixture of old and new tables."""
    g = maps.make_maze(256, cell=32, wall=3, p=0.5, seed=8)
    occ_a = g.occ.copy()
    occ_b = g.occ.copy()
    occ_b[60:200, 120:126] = 1
    occ_b[100:106, 20:230] = 1
    mrx, B, fov = 200, 360, 6.2
    om_a = oracle_mod.OracleMap(occ_a, g.resolution, g.origin, mrx)
    om_b = oracle_mod.OracleMap(occ_b, g.resolution, g.origin, mrx)
    omap = range_libc.PyOMap(g)
    methods = [range_libc.PyRayMarching(omap, mrx), range_libc.PyRayMarchingGPU(omap, mrx)]
    coeff = [0.999, 1.0]
    poses = maps.sample_free_poses(g, 24, 3, dt=np.minimum(om_a.dt, om_b.dt))
    # (PyRayMarching computes the upstream-literal arithmetic, PyRayMarchingGPU the canonical one)
    want = [[(o.rm_fan_libm if c == 0.999 else o.rm_fan)(poses, fov, B, step_coeff=c)[0] for o in (om_a, om_b)] for c in coeff]
    assert not np.array_equal(want[0][0], want[0][1])
    stop = threading.Event()
    errors = []
    seen = [set(), set()]

    def updater():
        k = 0
        while not stop.is_set():
            omap.update(occ_b if k % 2 == 0 else occ_a)
            k += 1

    def scanner(i):
        out = np.empty(len(poses) * B, np.float32)
        try:
            for k in range(400):
                methods[i].calc_range_fan(poses, out, fov, B)
                if np.array_equal(out, want[i][0]):
                    seen[i].add("a")
                elif np.array_equal(out, want[i][1]):
                    seen[i].add("b")
                else:
                    errors.append((i, k))
                    return
        except Exception as e:                                  # noqa: BLE001
            errors.append((i, repr(e)))

    up = threading.Thread(target=updater)
    sc = [threading.Thread(target=scanner, args=(i,)) for i in range(2)]
    up.start()
    for t in sc:
        t.start()
    for t in sc:
        t.join(300)
    stop.set()
    up.join(60)
    assert not errors, errors[:3]
    assert seen[0] == {"a", "b"} or seen[1] == {"a", "b"}     # the updates really interleaved with scans


def test_closed_loops_share_their_handles_across_threads():
    """One CarBatch, one RMGPU method with noise on and one PyFollowGap, used at once by a FollowGap roll-out, a driving
    environment (reset + 6 steps) and an MCTS planner (reset, run(2), best) in three threads: every call holds the
    method's mutex from its first launch to its last and puts the ray offset and nt_store back before it lets go, so
    every output equals the serial run's bit for bit and the method is left as it was.  9 units (one past DRIVE_CARS =
    8: a second workgroup with one live wave), 65 beams (two beam rows, the second holding one beam), 6 ticks."""
    N, B, T, base = 9, 65, 6, 4242
    g, states, actions = maze_case(lambda g_: range_libc.PyOMap(g_).distance_transform())
    states = np.ascontiguousarray(states[[0, 1, 2, 3, 4, 5, 46, 47, 48]])       # six in the open, three near a wall
    actions = np.ascontiguousarray(actions[:T, :N])
    speeds = np.linspace(1.0, 5.0, N)
    m = range_libc.PyRayMarchingGPU(range_libc.PyOMap(g), 300)
    m.set_noise(0.01, 77, base)
    cars, fg, edge = RC.CarBatch(), support.followgap(), support.edge(B)
    env = DriveEnv(m, states, N, B, FOV, edge, THRESH, car=cars)
    pl = MCTSPlanner(cars, m, N, 4, FOV, B, edge, THRESH, source="fg", followgap=fg, rollout_steps=4,
                     action_every=2)
    seeds = np.arange(N, dtype=np.uint64) * np.uint64(2 ** 33 + 7) + np.uint64(1)
    poses = np.ascontiguousarray(states[:, :3], np.float32)

    def fan():
        out = np.empty(N * B, np.float32)
        m.calc_range_fan(poses, out, FOV, B)
        return out

    def drive():
        return cars.drive_followgap(m, fg, states, T, speeds, FOV, B, edge, THRESH, trace=True)

    def drive_env():
        out = [env.reset(seed=5, start_index=np.arange(N, dtype=np.int32))]
        for k in range(T):
            out.extend(env.step(actions[k]))
        return out + [env.read()["states"]]

    def plan():
        pl.reset(states, np.linspace(-0.2, 0.2, N), seeds)
        pl.run(2)
        return pl.best()

    work = [drive, drive_env, plan]
    before = fan()
    serial = [[np.array(a) for a in w()] for w in work]
    got, errors = [None] * len(work), []

    def runner(i):
        try:
            got[i] = [np.array(a) for a in work[i]()]
        except Exception as e:                                  # noqa: BLE001
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=runner, args=(i,), daemon=True) for i in range(len(work))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not any(t.is_alive() for t in threads), "a closed loop did not return within 60 s"
    assert not errors, errors
    for i, w in enumerate(work):
        assert len(got[i]) == len(serial[i]), w.__name__
        for j, (a, b) in enumerate(zip(got[i], serial[i])):
            assert same_bits(a, b), (w.__name__, j)
    assert m.get_info("nt_store") == 1
    assert same_bits(fan(), before)
    pl.close()
    env.close()
    m.set_noise(0.0, 0, 0)


def test_league_and_seat_loops_share_their_handles_across_threads():
    """The sibling of the case above for the steering sources it leaves out, each of which takes its own set of
    mutexes: a league race env (the env's, the car's, the method's, FollowGap's and the population's), a league roll-out
    followed by the population's row-indexed evaluation (the same handles without an env's; then the population's
    alone) and a race env with drivers in its seats (neither seat handle's).  One CarBatch, one RMGPU method with noise
    on, one PyFollowGap and one 3-member population of the seat tests' 40 -> 16 -> 8 -> 1 network on 65 beams (two beam
    rows, the second holding one beam); 2 races of 3 cars.  Serially first, then in three threads at once: every output
    equals its serial twin bit for bit and the method is left as it was.  A thread still alive after 30 s fails the
    case (the work takes milliseconds), so a lock-order mistake shows as a failure, not as a run that hangs."""
    import drive_cases as DC
    import test_gpu_population as TP
    from test_gpu_race_env import _race_starts
    from pyracecarsimulator_amd import RaceEnv, league
    R, P, B, T, base = 2, 3, 65, 4, 4242
    g = DC.race_maze()
    omap = range_libc.PyOMap(g)
    m = range_libc.PyRayMarchingGPU(omap, DC.RACE_MRX)
    m.set_noise(0.01, 77, base)
    cars, fg, edge = RC.CarBatch(), support.followgap(), support.edge(B)
    pop, _, _ = TP.make_pop("small", 3)
    pol = pop.member(0)
    pool, _ = _race_starts(g, omap.distance_transform(), 3, P, 52)
    pool[:, :, 3] = 3.0
    entries = np.array([[-2, -1, 0], [2, -2, -1]], np.int32)           # the caller's, FollowGap's, members 0 and 2
    kw = dict(car=cars, seat_speed=(3.0, 3.5, 4.0), min_running=2, max_ticks=8, auto_reset=True, steer_clip=0.2,
              substeps=4, obs_window=(5, 40, 1), obs_clip=15.0, obs_scale=15.0)
    league_env = RaceEnv(m, pool, R, B, FOV, edge, THRESH, league=(pop, entries), followgap=fg, **kw)
    seat_env = RaceEnv(m, pool, R, B, FOV, edge, THRESH, seats=[None, fg, pol], **kw)
    acts = DC.actions(31, T, R * P).reshape(T, R, P, 2)
    league_acts, seat_acts = acts.copy(), acts.copy()
    league_acts[:, entries != -2] = np.nan                                # (a scripted car's action is not read)
    seat_acts[:, :, 1:] = np.nan
    roll_entries = np.array([[-1, 0, 2], [2, -1, 0]], np.int32)
    states = np.ascontiguousarray(pool[:R])
    rows = np.random.default_rng(9).uniform(0.2, 12.0, (R * P, B)).astype(np.float32)
    row_members = np.array([0, -1, 2, 1, -1, 0], np.int32)
    poses = np.ascontiguousarray(states.reshape(-1, 11)[:, :3], np.float32)

    def fan():
        out = np.empty(R * P * B, np.float32)
        m.calc_range_fan(poses, out, FOV, B)
        return out

    def run_league_env():
        out = [league_env.reset(seed=5, start_index=np.arange(R, dtype=np.int32))]
        for k in range(T):
            out.extend(league_env.step(league_acts[k]))
        steers, res = league_env.league_steers(), league_env.league_results()
        out.extend(res[k] for k in league.RESULT_COLUMNS)
        out.append(np.array([[res[who][k] for k in league.RESULT_COLUMNS] for who in ("followgap", "caller")]))
        return out + [steers]

    def run_league_rollout():
        out = list(cars.race_league(m, pop, roll_entries, states, 3, (3.0, 3.5, 4.0) * R, FOV, B, edge, THRESH,
                                    followgap=fg, steer_clip=0.2, trace=True))
        return out + [pop.predict_rows(rows, row_members)]

    def run_seat_env():
        out = [seat_env.reset(seed=5, start_index=np.arange(R, dtype=np.int32))]
        for k in range(T):
            out.extend(seat_env.step(seat_acts[k]))
        return out + [seat_env.seat_steers()]

    work = [run_league_env, run_league_rollout, run_seat_env]
    before = fan()
    serial = [[np.array(a) for a in w()] for w in work]
    got, errors = [None] * len(work), []

    def runner(i):
        try:
            got[i] = [np.array(a) for a in work[i]()]
        except Exception as e:                                  # noqa: BLE001
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=runner, args=(i,), daemon=True) for i in range(len(work))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(30)
    assert not any(t.is_alive() for t in threads), "a closed loop did not return within 30 s"
    assert not errors, errors
    for i, w in enumerate(work):
        assert len(got[i]) == len(serial[i]), w.__name__
        for j, (a, b) in enumerate(zip(got[i], serial[i])):
            assert same_bits(a, b), (w.__name__, j)
    # (the case is about the locks, not the drivers: still, a line-up that scripted nothing would test nothing)
    assert np.isfinite(serial[0][-1]).any() and np.isfinite(serial[2][-1]).any()
    assert m.get_info("nt_store") == 1
    assert same_bits(fan(), before)
    league_env.close()
    seat_env.close()
    m.set_noise(0.0, 0, 0)
