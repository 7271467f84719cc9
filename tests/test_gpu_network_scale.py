"""The population, seat and track-plan kernels past one block of work on the MI355X (tests/network_scale.py holds the
shapes; docs/history/network_scale.md the index arithmetic each case is the first to execute): the pack launch past one
trip of its capped grid, the population's network grid with three workgroups a member and more than ten in all, the
fitness kernel and rollout_xy_kernel with a second, part-filled workgroup, the seated env and roll-out with a race
across the step kernel's 64-lane blocks, whole trees past eight workgroups of plan_root_kernel.  Every comparison is
bit equality with the statement (tests/population_statement.py, seat_statement.py, mcts_track_statement.py) or with the
entry point the contract names as equal; every census is counted from the statement's side of the comparison."""
import os

import numpy as np
import pytest

import mcts_checks as MC
import mcts_track_checks as TC
import mcts_track_statement as MTS
import network_scale as NS
import policy_statement as S
import population_statement as PS
import seat_statement as SS
import support
import test_gpu_mcts_track as TT
import test_gpu_population as TP
import test_gpu_seats as TSE
import track_statement as TS
from conftest import GOLD
from support import FOV, THRESH, same_bits
from test_gpu_policy import _hard_scans
from test_gpu_race_env import RaceComposed, _race_starts
from pyracecarsimulator_amd import Policy, PolicyPopulation, RaceEnv, Track, maps, population, range_libc
from pyracecarsimulator_amd import racecar as RC
from pyracecarsimulator_amd.mcts import MCTSPlanner

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]


# ================================================================ A. populations
# ---------------------------------------------------------------- 1. the pack launch past one trip of its grid
@pytest.fixture(scope="module")
def pack_case():
    layers, relu = S.load_fixture(os.path.join(GOLD, "policy_mlp720.npz"))
    pol = Policy.from_arrays(layers, relu)
    P = population.n_params(pol.dims)
    return dict(pol=pol, P=P, control=NS.pack_thetas(NS.PACK["control_n"], P, seed=6), wrap=NS.pack_thetas(NS.PACK["n"], P, seed=5),
                scans=_hard_scans(3, 1081, 9))


def _check_pack(pop, pol, thetas, first, scans, what):
    """Members [first, first + len(thetas)) hold thetas' bits, answer as their own Policy does, and the members the
    call leaves alone are still zero."""
    n, P = thetas.shape
    trip, member, param = NS.pack_wrap(P)
    probe = sorted({first, first + 1, first + n - 2, first + n - 1} | ({first + member, first + member + 1} if n * P > trip else set()))
    for m in probe:
        got = pop.get(m)
        bad = np.nonzero(got.view(np.uint32) != thetas[m - first].view(np.uint32))[0]
        assert bad.size == 0, (what, "member", m, "first wrong parameter", int(bad[0]), "of", bad.size)
    zero = np.zeros(P, np.float32)
    for m in (0, first - 1, pop.n_members - 2, pop.n_members - 1):
        assert same_bits(pop.get(m), zero), (what, "member", m, "was written")
    ask = {first, first + n - 1} | ({first + member, first + member + 1} if n * P > trip else set())
    for m in sorted(ask):
        own = Policy.from_arrays(population.unpack(thetas[m - first], pol.dims), pol.relu, in_start=pol.in_start)
        assert same_bits(pop.predict_many(scans, 3, first=m, n=1), own.predict_many(scans)), (what, "member", m)
    return probe


@pytest.mark.parametrize("form", ["host", "device"])
def test_pack_launch_past_one_trip_of_its_grid(pack_case, form):
    """220 members of the fixture architecture (P = 79 297).  A control set of 211 members at first = 3 stays inside one
    trip of the grid (256 threads x 65 536 workgroups); then one set of 215 members at first = 3, other values, wraps
    inside call-member 211 (member 214) at parameter 45 549.  Host form and device form."""
    import torch
    pol, P = pack_case["pol"], pack_case["P"]
    C_, first = NS.PACK, NS.PACK["first"]
    trip, member, param = NS.pack_wrap(P)
    assert P == 79297 and (member, param) == (211, 45549)
    assert C_["control_n"] * P <= trip < C_["n"] * P and first + member + 3 < first + C_["n"] <= C_["members"] - 2
    pop = PolicyPopulation(pol.dims, C_["members"], relu=pol.relu, in_start=pol.in_start)
    assert pop.n_params == P

    def put(thetas):
        if form == "host":
            pop.set(thetas, first=first)
        else:
            t = torch.from_numpy(thetas).to("cuda:0")
            pop.set_device(t, first=first)
            torch.cuda.synchronize()

    put(pack_case["control"])
    _check_pack(pop, pol, pack_case["control"], first, pack_case["scans"], (form, "control"))
    assert same_bits(pop.get(first + member), np.zeros(P, np.float32))
    put(pack_case["wrap"])
    probe = _check_pack(pop, pol, pack_case["wrap"], first, pack_case["scans"], (form, "wrap"))
    assert probe == [3, 4, 214, 215, 216, 217]
    assert same_bits(pop.get(213), pack_case["wrap"][210])          # the last member before the one the wrap starts in


# ---------------------------------------------------------------- 2. the evaluation grid
@pytest.mark.parametrize("name,n,E", NS.EVAL)
def test_eval_grid_past_ten_workgroups(name, n, E):
    """67 members x 17 cars (3 workgroups a member, the last with 1 car of 8: 201 workgroups) and 130 x 1: the
    statement, the members' own Policy at 0, 63, 64 and n - 1, and a sub-range across member 64."""
    dims, in_start, relu, B = TP.NETS[name]
    pop, thetas, relu_ = TP.make_pop(name, n, seed=n)
    scans = TP.shared_scans(name, n, E, 10 * n + E)
    got = pop.predict_many(scans, E)
    assert same_bits(got, PS.evaluate(thetas, dims, relu_, scans, E, in_start=in_start))
    for m in (0, 63, 64, n - 1):
        assert same_bits(got[m * E:(m + 1) * E], pop.member(m).predict_many(scans[:E])), (name, n, E, m)
    assert TP.differ_pairwise([got[m * E:(m + 1) * E] for m in range(n)])
    f, k = NS.SUB["first"], NS.SUB["n"]
    sub = pop.predict_many(scans[:k * E], E, first=f, n=k)
    assert same_bits(sub, got[f * E:(f + k) * E])                    # (every member sees the same E scans)
    assert same_bits(sub, PS.evaluate(thetas, dims, relu_, scans[:k * E], E, first=f, n=k, in_start=in_start))


# ---------------------------------------------------------------- 3. the roll-out and its fitness past one block
@pytest.fixture(scope="module")
def pop_rig():
    g = maps.make_maze(512, cell=40, wall=3, p=0.45, seed=11)
    omap = range_libc.PyOMap(g)
    rig = dict(g=g, omap=omap, dt=omap.distance_transform(), cars=RC.CarBatch(), m=range_libc.PyRayMarchingGPU(omap, TP.MRX))
    yield rig
    rig["m"].set_noise(0.0, 0, 0)


@pytest.mark.parametrize("n,E", sorted(NS.ROLLOUTS))
def test_rollout_and_fitness_past_one_block(pop_rig, n, E):
    """67 members x 3 cars and 130 x 1, the small network, 64 beams, RMGPU, 25 ticks, clip 0.2, noise off, every car
    its own start: the per-member drive_policy calls, the fitness statement over the returned states, the crash
    counts; then members [60, 67) alone."""
    cars, m = pop_rig["cars"], pop_rig["m"]
    cfg, B, T, clip = NS.ROLLOUTS[(n, E)], NS.ROLLOUT_B, NS.ROLLOUT_T, TP.CLIP
    pop, thetas, _ = TP.make_pop("small", n, cfg["net_seed"], cfg["gain"])
    pols = [pop.member(k) for k in range(n)]
    states, speeds = NS.rollout_starts(pop_rig["g"], pop_rig["dt"], cfg, n, E)
    edge = support.edge(B)
    m.set_noise(0.0, 0, 0)
    got = cars.drive_population(m, pop, states, T, speeds, FOV, B, edge, THRESH, E, steer_clip=clip, trace=True)
    want = TP.per_member_drive(cars, m, pols, states, speeds, T, B, edge, clip, E)
    for i, (x, y) in enumerate(zip(got[:6], want)):
        assert same_bits(x, y), (n, E, i)
    first, final, fit = got[0], got[1], got[6]
    want_fit = PS.fitness(states, final, first, E)
    assert fit.shape == (n, 2) and same_bits(fit[:, 0], want_fit[:, 0]), np.nonzero(fit[:, 0] != want_fit[:, 0])
    assert same_bits(fit[:, 1], (first >= 0).reshape(n, E).sum(1).astype(np.float64))
    census = NS.rollout_census(want[0], want[3], want_fit, n, E, clip)
    print("roll-out %d x %d on the device: %s, %d of %d cars crash" % (n, E, census, (first >= 0).sum(), n * E))
    assert all(census.values()), census
    if E >= 3:                                                      # the order of the sum shows in these bits
        d = final[:, 8] - states[:, 8]
        down = np.array([np.cumsum(d[k * E:(k + 1) * E][::-1])[-1] for k in range(n)])
        assert (down != fit[:, 0]).any()
    f, k = NS.SUB["first"], NS.SUB["n"]
    rows = slice(f * E, (f + k) * E)
    sub = cars.drive_population(m, pop, states[rows], T, speeds[rows], FOV, B, edge, THRESH, E, first=f, steer_clip=clip,
                                trace=True)
    for i in range(6):
        assert same_bits(sub[i], want[i][rows]), (n, E, "sub", i)
    assert same_bits(sub[6], want_fit[f:f + k])


# ================================================================ B. seats
@pytest.fixture(scope="module")
def seat_rig():
    g = TSE.DC.race_maze()
    omap = range_libc.PyOMap(g)
    m = range_libc.PyRayMarchingGPU(omap, TSE.MRX)
    layers = TSE.small_net()
    rig = dict(g=g, omap=omap, dt=omap.distance_transform(), m=m, fg=support.followgap(), pol=Policy(layers=layers, in_start=5),
               layers=layers, cars=RC.CarBatch())
    yield rig
    m.set_noise(0.0, 0, 0)


def _answer(rig):
    def answer(driver, row):
        row = np.ascontiguousarray(row[None])
        return (driver.eval_many(row) if driver is rig["fg"] else driver.predict_many(row))[0]
    return answer


# ---------------------------------------------------------------- 4. the seated env across the step kernel's blocks
@pytest.mark.parametrize("name", sorted(NS.SEAT_ENVS))
def test_seated_env_across_blocks(seat_rig, name):
    """23 races x 3 cars (race 21 = cars 63, 64, 65) with seats policy / FollowGap / policy and policy / FollowGap /
    caller, and 9 races x 8 cars: 12 steps against the statement over the public calls, noise off, every race truncated
    after 5 ticks and re-spawned.  Observations, rewards, done codes, the seats' answers, the states and every per-car
    and per-race counter after every call."""
    case = NS.SEAT_ENVS[name]
    m, cars, fg, pol = seat_rig["m"], seat_rig["cars"], seat_rig["fg"], seat_rig["pol"]
    R, P, B = case["R"], case["P"], case["B"]
    N = R * P
    assert N > 64 and case["watch"] * P < 64
    pool = NS.seat_pool(seat_rig["g"], seat_rig["dt"], case)
    edge = support.edge(B)
    m.set_noise(0.0, 0, 0)
    pub = RaceComposed(m, cars, N, P, B, edge, NS.SEAT_ENV_KW["substeps"])
    stmt, seats = NS.seat_statement(case, pool, pub.step_cars, pub.scan, pub.is_crashed, _answer(seat_rig), {"p": pol, "f": fg})
    env = RaceEnv(m, pool, R, B, FOV, edge, THRESH, car=cars, seats=seats, seat_speed=case["speed"], **NS.SEAT_WINDOW,
                  **NS.SEAT_ENV_KW)

    def counters(k):
        rd = env.read()
        assert same_bits(rd["states"], stmt.states.reshape(R, P, 11)), k
        for key, want in (("ticks", stmt.tick), ("episodes", stmt.episode), ("start_index", stmt.start_index),
                          ("done", stmt.done)):
            assert same_bits(rd[key], want.reshape(R, P)), (k, key)
        for key, want in (("race_ticks", stmt.race_tick), ("race_episodes", stmt.race_episode),
                          ("race_start_index", stmt.race_start_index), ("race_over", stmt.race_over)):
            assert same_bits(rd[key], want), (k, key)
        got, want = env.seat_steers(), stmt.seat_steers().reshape(R, P)
        assert same_bits(got, want), (k, np.nonzero(got.view(np.uint32) != want.view(np.uint32)))

    obs = env.reset(seed=case["seed"])
    want_obs, _ = stmt.reset(case["seed"])
    assert same_bits(obs, want_obs.reshape(R, P, -1))
    counters(0)
    census = NS.SeatCensus(stmt, case)
    for k, a in enumerate(NS.seat_actions(case), 1):
        census.before()
        obs, rew, dn = env.step(a.reshape(R, P, 2))
        want_obs, want_rew, want_done = stmt.step(a)
        census.after(want_done)
        assert same_bits(obs, want_obs.reshape(R, P, -1)), k
        assert same_bits(rew, want_rew.reshape(R, P)), (k, np.nonzero(rew != want_rew.reshape(R, P)))
        assert same_bits(dn, want_done.reshape(R, P)), (k, np.nonzero(dn != want_done.reshape(R, P)))
        counters(k)
    on_device = env.seat_steers(on_device=True)                     # rl_env_read_seats_device: the same answers
    assert same_bits(on_device.cpu().numpy(), env.seat_steers())
    print("seated env %s on the device: %s" % (name, census.seen))
    assert census.ok(), census.seen


# ---------------------------------------------------------------- 5. the seated roll-out across blocks
@pytest.mark.parametrize("R,P,B,mix,seed", NS.SEAT_ROLLOUTS)
def test_seated_rollout_across_blocks(seat_rig, R, P, B, mix, seed):
    """69 and 72 cars, 40 ticks, noise on: mixed seats (46 and 45 rows through the network's row-list launch, its sixth
    workgroup part filled) and every seat the policy's against the statement over the public calls, every seat
    FollowGap's against rl_car_race_followgap."""
    m, fg, pol, cars = seat_rig["m"], seat_rig["fg"], seat_rig["pol"], seat_rig["cars"]
    N, T = R * P, NS.SEAT_ROLLOUT_T
    states, speeds = _race_starts(seat_rig["g"], seat_rig["dt"], R, P, seed)
    speeds = speeds + 2.0
    edge = support.edge(B)
    steer0 = np.random.default_rng(seed).uniform(-0.2, 0.2, (R, P)).astype(np.float32)
    std, noise_seed, base = TSE.STD, TSE.NOISE_SEED, TSE.BASE
    m.set_noise(std, noise_seed, base)
    want = cars.race_followgap(m, fg, states, T, speeds, FOV, B, edge, THRESH, steer0=steer0, trace=True)
    got = cars.race_seats(m, [fg] * P, states, T, speeds, FOV, B, edge, THRESH, steer_clip=0.01, steer0=steer0, trace=True)
    for i, (x, y) in enumerate(zip(got, want)):
        assert same_bits(x, y), ("followgap", i)
    assert (want[0].reshape(-1)[64:] >= 0).any() and (want[0].reshape(-1)[64:] < 0).any()
    pub = RaceComposed(m, cars, N, P, B, edge, 1, std, noise_seed, base)
    for seats_mix in (mix, "p" * P):
        seats = [fg if c == "f" else pol for c in seats_mix]
        n_rows = sum(c == "p" for c in seats_mix) * R
        assert n_rows > 40 and (seats_mix != mix or n_rows % 8 != 0)
        m.set_noise(std, noise_seed, base)
        first, final, vel, steers, sp, st = (a.reshape((N,) + a.shape[2:]) for a in cars.race_seats(
            m, seats, states, T, speeds, FOV, B, edge, THRESH, steer_clip=NS.SEAT_CLIP, steer0=steer0, trace=True))
        w_first, w_final, w_steers, w_trace = SS.seated_rollout(
            states.reshape(N, 11), speeds.reshape(N), steer0.reshape(N), T, seats, lambda d: d is pol, NS.SEAT_CLIP,
            pub.step_cars, pub.scan, pub.is_crashed, _answer(seat_rig))
        m.set_noise(0.0, 0, 0)
        assert same_bits(first, w_first), (seats_mix, np.nonzero(first != w_first))
        assert TP.same_or_nan(steers, w_steers), (seats_mix, np.nonzero(~((steers == w_steers) | np.isnan(w_steers))))
        assert TP.same_or_nan(st, w_trace) and same_bits(final, w_final), seats_mix
        assert TP.same_or_nan(vel, w_trace[:, :, 3]), seats_mix
        net = np.array([c == "p" for c in seats_mix] * R)
        with np.errstate(invalid="ignore"):
            clamped = (np.abs(w_steers[:, :-1]) > NS.SEAT_CLIP) & net[:, None]
        assert (w_first[64:] >= 0).any() and (w_first[64:] < 0).any() and clamped[64:].any(), seats_mix


# ================================================================ C. the track plan
@pytest.fixture(scope="module")
def cars_only():
    return RC.CarBatch()


_TRACK_CASES = {}


def _track_case(cars, name, every):
    """The 130 roll-outs of (track, steps an action) and their per-step states, computed once: R = 64 and 65 are its
    first rows."""
    if (name, every) not in _TRACK_CASES:
        xy, closed = TT.TRACKS[name]
        T = TS.build(xy, closed)
        n, L = max(NS.TRACK_R), NS.TRACK_L
        st, act = NS.track_cars(T, TT.at_arc, n, L, every, 100 + every)
        steps = TC.step_states(cars, st, act, L, every)
        near = np.array([TS.nearest(T, st[r, 0], st[r, 1]) for r in range(n)], np.int32)
        _TRACK_CASES[(name, every)] = dict(T=T, trk=Track(xy, closed), st=st, act=act, steps=steps, near=near, want={})
    return _TRACK_CASES[(name, every)]


def _progress_want(c, window, r):
    key = ("progress", window, r)
    if key not in c["want"]:
        c["want"][key] = MTS.progress_terms(c["T"], int(c["near"][r]), window, c["st"][r, :2], c["steps"][r, :, :2])
    return c["want"][key]


def _waypoint_want(c, r):
    key = ("waypoint", r)
    if key not in c["want"]:
        rt = MTS.root(c["T"], c["st"][r, 0], c["st"][r, 1], 1.5, 5, None)
        c["want"][key] = MTS.terms(c["T"], MTS.WAYPOINT, 0, rt, c["st"][r, :2], c["steps"][r, :, :2], c["steps"][r, :, 3])
    return c["want"][key]


@pytest.mark.parametrize("every", [1, 5])
@pytest.mark.parametrize("name", ["ring70", "wp36"])
@pytest.mark.parametrize("R", NS.TRACK_R)
def test_rollout_track_past_one_block(cars_only, name, every, R):
    """R = 64 (one full workgroup of rollout_xy_kernel), 65 (one lane of a second) and 130 (a third, two lanes) roll-outs
    of 24 steps, an action every step and every fifth: progress with window 0 and 3 (terms, s, segment, start_s) and
    the waypoint reward, bit-equal to the statement row by row; the f64 poses and velocities behind them are those of
    the public roll-out call."""
    cars = cars_only
    c = _track_case(cars, name, every)
    L = NS.TRACK_L
    st, act = c["st"][:R], c["act"][:R]
    # (R = 64 and 65 run the first rows of the 130: the final states of the public call agree with the shared ones)
    _, fin, vel = cars.rollout(st, act, n_steps=L, action_every=every)
    assert same_bits(fin, c["steps"][:R, -1]) and same_bits(vel, c["steps"][:R, :, 3])
    for window in (0, 3):
        got = cars.rollout_track(c["trk"], st, act, "progress", window=window, n_steps=L, action_every=every)
        for r in range(R):
            terms, s, seg, s0 = _progress_want(c, window, r)
            what = (name, every, R, window, r)
            assert same_bits(got["terms"][r], terms), what
            assert same_bits(got["s"][r], s) and same_bits(got["segment"][r], seg), what
            assert same_bits(got["start_s"][r:r + 1], np.array([s0])), what
        rows = sorted({63, 64, R - 1} & set(range(R)))
        assert TP.differ_pairwise([_progress_want(c, window, r)[0] for r in rows]), (name, every, R, window)
        assert TP.differ_pairwise([_progress_want(c, window, r)[1] for r in rows])
    got = cars.rollout_track(c["trk"], st, act, "waypoint", lookahead=1.5, goal_span=5, n_steps=L, action_every=every)
    for r in range(R):
        assert same_bits(got["terms"][r], _waypoint_want(c, r)), (name, every, R, "waypoint", r)
    assert TP.differ_pairwise([_waypoint_want(c, r) for r in sorted({63, 64, R - 1} & set(range(R)))])
    got = cars.rollout_track(None, st, act, "velocity", n_steps=L, action_every=every)
    assert same_bits(got["terms"], c["steps"][:R, :, 3])


# ---------------------------------------------------------------- 7. whole trees past eight workgroups of roots
def test_trees_past_one_block():
    """K = 65 trees (9 workgroups of plan_root_kernel, the last with one tree; a second, one-lane workgroup of
    rollout_xy_kernel; 65 workgroups of plan_term_kernel), I = 3, L = 8, 64 beams, random roll-outs, noise off, the
    progress reward with window 3: every node array of every tree, best() and the roots against the statement."""
    c = NS.TREES
    K, I, L, B = c["K"], c["I"], c["L"], c["B"]
    g = maps.load_colombia()
    omap = range_libc.PyOMap(g)
    m, cars = range_libc.PyRayMarchingGPU(omap, 300), RC.CarBatch()
    states, actions, seeds = MC.roots(g, omap.distance_transform(), K, c["seed"])
    xy = TC.ring_around(states)
    T, trk = TS.build(xy, True), Track(xy, True)
    m.set_noise(0.0, 99, c["base"])
    pl = MCTSPlanner(cars, m, K, I + 1, FOV, B, support.edge(B), THRESH, source="random", rollout_steps=L,
                     action_every=TT.EVERY)
    try:
        pl.attach_track(trk, "progress", lookahead=1.5, window=c["window"], goal_span=0)
        pl.reset(states, actions, seeds)
        pl.run(I)
        dev = [pl.read_tree(k) for k in range(K)]
        best = pl.best()
        rts = TC.statement_roots(T, states, 1.5, 0)
        tc = TC.TermCars(cars, T, MTS.PROGRESS, c["window"], rts)
        trees, snaps = MC.replay(tc, m, 0.0, c["base"], "random", None, states, actions, seeds, I, dev, (I,), num_rays=B,
                                 rollout_steps=L, action_every=TT.EVERY)
        for k in range(K):
            MC.assert_tree(dev[k], snaps[I][k], ("trees", k))
            a, v = trees[k].best()
            assert best[0][k] == a and best[1][k] == v, k
        TC.assert_roots(pl.read_track(), rts, "trees")
        # the trees past the first 64 are trees of their own: rewards differ from one another and from tree 0's
        assert TP.differ_pairwise([dev[k]["reward"] for k in (0, 63, 64)])
        assert len({rt["segment"] for rt in rts}) > 1
    finally:
        pl.close()
        m.set_noise(0.0, 0, 0)
