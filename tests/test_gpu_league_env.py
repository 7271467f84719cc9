"""League line-ups in the race environment (include/scanlib_league_env.h: rl_env_attach_league, rl_env_set_league_entries*,
rl_env_read_league_*; RaceEnv(league=...), RacecarSimulator.raceEnv(league=...)) on the MI355X, every comparison bit for
bit: against the seated env and the plain env it becomes with one kind of line-up, against a plain env whose caller
writes the drivers' pairs, against the statement (tests/league_env_statement.py) over the composed public calls — line-ups
handed over mid-run, members re-set mid-run, other league calls in between — and the results against the statement over
the run's own outputs.

Shapes: the rig of test_gpu_seats.py (its map, 64 / 65 beams): 5 races x 3 cars and 2 x 8 (tests/league_env_cases.py,
seeds from tools/league_env_census.py), the 720-input fixture network on 1081 beams once, 24 -> 1 where the population
is large (70 and 300 members: second trips of the grouping's passes; 520 cars of one member in one call)."""
import ctypes as C
import math

import numpy as np
import pytest

import drive_cases as DC
import league_env_cases as CASES
import league_env_statement as LE
import support
import test_gpu_population as TP
from env_statement import observation
from league_env_cases import BASE, CLIP, MIXED, N_POP, NOISE_SEED, STD, SWAP, WINDOW
from support import D_BASE, FOV, THRESH, same_bits
from test_gpu_race_env import RaceComposed, _race_starts
from test_gpu_seats import ring_track
from pyracecarsimulator_amd import DriveEnv, PolicyPopulation, RaceEnv, RacecarSimulator, _lib, league, range_libc
from pyracecarsimulator_amd import racecar as RC

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

MRX = DC.RACE_MRX
RL_ERR_INVALID = -1


@pytest.fixture(scope="module")
def rig():
    g = DC.race_maze()
    omap = range_libc.PyOMap(g)
    m = range_libc.PyRayMarchingGPU(omap, MRX)
    pop, thetas, relu = TP.make_pop("small", N_POP, CASES.NET_SEED, CASES.GAIN)
    rig = dict(g=g, omap=omap, dt=omap.distance_transform(), m=m, fg=support.followgap(), cars=RC.CarBatch(), pop=pop,
               thetas=thetas, pools={})
    yield rig
    m.set_noise(0.0, 0, 0)


def pool_of(rig, c):
    key = (c["M"], c["P"], c["pool_seed"])
    if key not in rig["pools"]:
        pool, _ = _race_starts(rig["g"], rig["dt"], c["M"], c["P"], c["pool_seed"])
        pool[:, :, 3] = 3.0
        rig["pools"][key] = pool
    return rig["pools"][key]


def league_env(rig, c, entries=None, pop=None, **over):
    rig["m"].set_noise(STD, NOISE_SEED, BASE)
    kw = dict(CASES.env_kw(c), **WINDOW)
    kw.update(over)
    return RaceEnv(rig["m"], pool_of(rig, c), c["R"], c["B"], FOV, support.edge(c["B"]), THRESH, car=rig["cars"],
                   league=(pop or rig["pop"], np.array(c["entries"] if entries is None else entries)), followgap=rig["fg"],
                   seat_speed=c["speed"], **kw)


def snapshot(env, out, results=True):
    snap = dict(out=tuple(np.array(x) for x in out), read={k: v.copy() for k, v in env.read().items()},
                steers=env.league_steers(), entries=env.entries())
    if results:
        snap["results"] = env.league_results()
    return snap


def results_block(d):
    """``league_results``' dict back as the (n_members + 2, 8) block."""
    rows = np.stack([d[k] for k in LE.COLUMNS], -1)
    return np.concatenate([rows, [[d[key][k] for k in LE.COLUMNS] for key in ("followgap", "caller")]]).astype(np.int64)


def answers(rig, raw, live, pop=None):
    """The drivers' answers to full raw scans (N, B) by the public calls, NaN for the caller's cars."""
    pop = pop or rig["pop"]
    live = np.asarray(live).reshape(-1)
    member = np.where((live >= 0) & (live < pop.n_members), live, -1).astype(np.int32)
    raw = np.ascontiguousarray(raw, np.float32)
    out = pop.predict_rows(raw, member)
    fg = live == -1
    if fg.any():
        out[fg] = rig["fg"].eval_many(np.ascontiguousarray(raw[fg]))
    return out


@pytest.fixture(scope="module")
def runs(rig):
    """The league envs of cases 3, 4, 7 and 8 run once each in the host form (noise, auto-reset, the network's input
    window): one snapshot per call."""
    done = {}

    def run(name):
        if name not in done:
            c = MIXED[name]
            env = league_env(rig, c)
            live = np.array(c["entries"])
            acts = [CASES.masked(a, live) for a in CASES.actions(c)]
            log = [snapshot(env, (env.reset(seed=c["seed"]),))]
            for a in acts:
                log.append(snapshot(env, env.step(a)))
            done[name] = dict(env=env, acts=acts, log=log)
        return done[name]
    return run


# ---------------------------------------------------------------- 1. one member in the same seats: the seated env
@pytest.mark.parametrize("P,B,mix", [(3, 65, "cfm"), (8, 64, "cfmmmfmf"), (3, 1081, "cmf")])
def test_one_member_in_the_same_seats_equals_the_seated_env(rig, P, B, mix):
    m, cars, fg = rig["m"], rig["cars"], rig["fg"]
    R, steps, member = (3, 10, 2) if B == 1081 else (4, 14, 3)
    if B == 1081:
        pop, _, _ = TP.make_pop("fixture", 3)
        window = dict(obs_window=(180, 720, 1), obs_clip=15.0, obs_scale=15.0)
        clip = 0.4189
    else:
        pop, window, clip = rig["pop"], WINDOW, CLIP
    pol = pop.member(member)
    pool, _ = _race_starts(rig["g"], rig["dt"], 3, P, 52 if P == 3 else 58)
    pool[:, :, 3] = 3.0
    edge = support.edge(B)
    speed = (np.arange(P) % 3 + 3.5).astype(np.float32)
    kw = dict(min_running=min(2, P), max_ticks=8, auto_reset=True, crash_reward=-2.5, steer_clip=clip, substeps=4,
              car=cars, track=ring_track(), progress_reward=True, **window)
    code = {"c": -2, "f": -1, "m": member}
    entries = np.tile([code[ch] for ch in mix], (R, 1))
    m.set_noise(STD, NOISE_SEED, BASE)
    a = RaceEnv(m, pool, R, B, FOV, edge, THRESH, league=(pop, entries), followgap=fg, seat_speed=speed, **kw)
    b = RaceEnv(m, pool, R, B, FOV, edge, THRESH, seats=[{"c": None, "f": fg, "m": pol}[ch] for ch in mix],
                seat_speed=speed, **kw)

    def same(k, x, y):
        for i, (u, v) in enumerate(zip(x, y)):
            assert same_bits(u, v), (k, i)
        ra, rb = a.read(), b.read()
        for key in rb:
            assert same_bits(ra[key], rb[key]), (k, key)
        ta, tb = a.track_state(), b.track_state()
        for key in tb:
            assert same_bits(np.asarray(ta[key]), np.asarray(tb[key])), (k, key)
        assert same_bits(a.league_steers(), b.seat_steers()), k

    same(0, a.reset(seed=7, aux=True), b.reset(seed=7, aux=True))
    acts = DC.actions(31, steps, R * P).reshape(steps, R, P, 2)
    acts[:, :, [i for i, ch in enumerate(mix) if ch != "c"]] = np.nan
    for k, act in enumerate(acts, 1):
        same(k, a.step(act, aux=True), b.step(act, aux=True))
    rd = b.read()
    assert (rd["race_episodes"] > 0).any() and np.isfinite(b.seat_steers()).any()


# ---------------------------------------------------------------- 2. one kind of entry everywhere
def test_every_entry_the_callers_equals_the_plain_env(rig):
    c = MIXED["5x3"]
    a = league_env(rig, c, entries=np.full((c["R"], c["P"]), -2))
    rig["m"].set_noise(STD, NOISE_SEED, BASE)
    b = RaceEnv(rig["m"], pool_of(rig, c), c["R"], c["B"], FOV, support.edge(c["B"]), THRESH, car=rig["cars"],
                **CASES.env_kw(c), **WINDOW)
    assert same_bits(a.reset(seed=3), b.reset(seed=3))
    for k, act in enumerate(CASES.actions(c)[:12]):
        for x, y in zip(a.step(act, aux=True), b.step(act, aux=True)):
            assert same_bits(x, y), k
        ra, rb = a.read(), b.read()
        assert all(same_bits(ra[key], rb[key]) for key in rb), k
        assert np.isnan(a.league_steers()).all()
    res = a.league_results()
    assert res["caller"]["entered"] > 0 and not res["entered"].any() and res["followgap"]["entered"] == 0
    assert res["caller"]["callers_faced"] == res["caller"]["faced"] == res["caller"]["entered"] * (c["P"] - 1)


@pytest.mark.parametrize("P,B,seed", [(3, 64, 52), (8, 65, 58), (1, 65, 51)])
def test_every_entry_followgap_equals_race_followgap(rig, P, B, seed):
    """auto_reset off, every entry -1, NaN actions: first crash ticks and steers of rl_car_race_followgap, whose noise
    base lies N B above the env's (the reset takes slot 0)."""
    m, fg, cars = rig["m"], rig["fg"], rig["cars"]
    R, T = 5, 30
    N = R * P
    states, speeds = _race_starts(rig["g"], rig["dt"], R, P, seed)
    seat_speed = (np.arange(P) % 3 + 4.5).astype(np.float32)
    edge = support.edge(B)
    m.set_noise(STD, NOISE_SEED, BASE)
    env = RaceEnv(m, states, R, B, FOV, edge, THRESH, min_running=1, auto_reset=False, car=cars,
                  league=(rig["pop"], np.full((R, P), -1)), followgap=fg, seat_speed=seat_speed, obs_window=(0, 10, 1))
    env.reset(seed=0, start_index=np.arange(R))
    assert (env.read()["done"] == 0).all()
    steer0 = env.league_steers()
    m.set_noise(STD, NOISE_SEED, BASE + N * B)
    first, final, vel, steers = cars.race_followgap(m, fg, states, T, np.tile(seat_speed.astype(np.float64), (R, 1)),
                                                    FOV, B, edge, THRESH, steer0=steer0)
    m.set_noise(STD, NOISE_SEED, BASE)
    assert (first >= 0).any() and (first < 0).any()
    want_first = np.full((R, P), -(T + 1), np.int32)
    nan_actions = np.full((R, P, 2), np.nan, np.float32)
    for t in range(T):
        alive = want_first < 0
        obs, rew, dn = env.step(nan_actions)
        want_first[alive & (dn == 1)] = t
        assert not (dn == 3).any()
        go = want_first < 0
        got = env.league_steers()
        assert same_bits(got[go], steers[:, :, t][go]), t
        assert np.isnan(got[~go]).all()
    assert same_bits(want_first, first)
    rd = env.read()
    assert same_bits(rd["states"], final)
    # the finished races stand (auto_reset off): each was counted once, in the call that ended it
    over = rd["race_over"] != 0
    res = env.league_results()
    assert res["followgap"]["entered"] == P * int(over.sum()) and (P != 1 or over.any())
    assert res["followgap"]["ticks"] == int(rd["ticks"][over].sum()) and not res["entered"].any()


# ---------------------------------------------------------------- 3. a plain env fed the drivers' pairs
@pytest.mark.parametrize("name", ["5x3", "2x8"])
def test_league_env_equals_plain_env_fed_the_drivers_pairs(rig, runs, name):
    """The parent commit's only way: a plain RaceEnv on the raw full window, the population's row-indexed evaluation
    and FollowGap on its observations from Python, their answers scattered into the action rows."""
    c, run = MIXED[name], runs(name)
    R, P, B, log = c["R"], c["P"], c["B"], run["log"]
    live = np.array(c["entries"], np.int32)
    scripted = live >= -1
    rig["m"].set_noise(STD, NOISE_SEED, BASE)
    plain = RaceEnv(rig["m"], pool_of(rig, c), R, B, FOV, support.edge(B), THRESH, car=rig["cars"], **CASES.env_kw(c))
    win = (WINDOW["obs_window"], WINDOW["obs_clip"], WINDOW["obs_scale"])
    speed = np.tile(np.float32(c["speed"]), (R, 1))

    def compare(k, out):
        snap = log[k]
        raw = out[0]
        assert same_bits(observation(raw.reshape(R * P, B), *win).reshape(R, P, -1), snap["out"][0]), k
        for x, y in zip(out[1:], snap["out"][1:]):
            assert same_bits(x, y), k
        rd = plain.read()
        for key in rd:
            assert same_bits(rd[key], snap["read"][key]), (k, key)
        ans = answers(rig, raw.reshape(R * P, B), live).reshape(R, P)
        kept = ans.copy()
        kept[rd["done"] != 0] = np.nan
        assert same_bits(kept, snap["steers"]), k
        assert same_bits(snap["entries"]["live"], live) and same_bits(snap["entries"]["pending"], live)
        return ans

    ans = compare(0, (plain.reset(seed=c["seed"]),))
    for k, a in enumerate(run["acts"], 1):
        assert np.isnan(a[scripted]).all() and not np.isnan(a[~scripted]).any()
        fed = a.copy()
        fed[scripted, 0] = speed[scripted]
        fed[scripted, 1] = ans[scripted]
        ans = compare(k, plain.step(fed))
    rd = plain.read()
    assert (rd["race_episodes"] > 0).all()


# ---------------------------------------------------------------- 4 / 5 / 6. the statement over the public calls
def lockstep(rig, c, env, acts, before_step=None, pop=None, log=None):
    """``env`` (or, with ``log``, its recorded run) and the statement over the composed public calls, call by call:
    outputs, counters, kept answers, both entry tables and the results.  ``before_step(k, env, stmt)`` runs before step
    k on both.  Returns the census of the run."""
    pop = pop or rig["pop"]
    R, P, B = c["R"], c["P"], c["B"]
    N = R * P
    pub = RaceComposed(rig["m"], rig["cars"], N, P, B, support.edge(B), c["S"], STD, NOISE_SEED, BASE)
    census = CASES.Census()
    entered = sorted({int(v) for t in [c["entries"]] + [t for _, t in c.get("at", {}).values()] for v in np.reshape(t, -1)
                      if 0 <= v < pop.n_members})

    def answer(entry, row):
        row = np.ascontiguousarray(row[None])
        if entry < 0:
            return rig["fg"].eval_many(row)[0]
        mine = pop.predict_rows(row, [entry])[0]
        others = [k for k in entered if k != entry]
        theirs = pop.predict_rows(np.tile(row, (len(others), 1)), others)
        census.net_answers += 1
        census.differ += int(any(t.tobytes() != mine.tobytes() for t in theirs))
        return mine

    kw = {k: v for k, v in CASES.env_kw(c).items() if k != "substeps"}
    stmt = LE.LeagueEnvStatement(pool_of(rig, c), R, B, pub.step_cars, pub.scan, pub.is_crashed, answer, c["entries"],
                                 c["speed"], pop.n_members, scan_dist_to_base=D_BASE, **WINDOW, **kw)

    def compare(k, snap, want_obs, want_done, want_rew=None):
        assert same_bits(snap["out"][0], want_obs.reshape(R, P, -1)), k
        if want_rew is not None:
            assert same_bits(snap["out"][1], want_rew.reshape(R, P)) and same_bits(snap["out"][2], want_done.reshape(R, P)), k
        rd = snap["read"]
        assert same_bits(rd["states"], stmt.states.reshape(R, P, 11)), k
        for key, want in (("ticks", stmt.tick), ("episodes", stmt.episode), ("start_index", stmt.start_index),
                          ("done", stmt.done)):
            assert same_bits(rd[key], want.reshape(R, P)), (k, key)
        for key, want in (("race_ticks", stmt.race_tick), ("race_episodes", stmt.race_episode),
                          ("race_start_index", stmt.race_start_index), ("race_over", stmt.race_over)):
            assert same_bits(rd[key], want), (k, key)
        assert same_bits(snap["steers"], stmt.league_steers().reshape(R, P)), k
        assert same_bits(snap["entries"]["live"], stmt.live.reshape(R, P)), k
        assert same_bits(snap["entries"]["pending"], stmt.pending.reshape(R, P)), k
        assert results_block(snap["results"]).tolist() == stmt.read_results().tolist(), k

    obs, done = stmt.reset(c["seed"])
    compare(0, log[0] if log else snapshot(env, (env.reset(seed=c["seed"]),)), obs, done)
    for k, a in enumerate(acts, 1):
        if before_step:
            before_step(k, env, stmt)
        before = stmt.done.copy(), stmt.race_over.copy(), stmt.live.copy()
        a = CASES.masked(a, stmt.live.reshape(R, P))
        obs, rew, done = stmt.step(a.reshape(N, 2))
        compare(k, log[k] if log else snapshot(env, env.step(a)), obs, done, rew)
        census.step(stmt, *before)
        net = (stmt.live >= 0) & (stmt.live < pop.n_members) & ~np.isnan(stmt.steers)
        census.clamped += int((np.abs(stmt.steers[net]) > CLIP).sum())
        census.seen += int((stmt.ranges != pub.scan_alone(support.lidar_poses(stmt.states), stmt.k)).sum())
    return census, stmt


@pytest.mark.parametrize("name", ["5x3", "2x8"])
def test_league_env_equals_the_statement_over_public_calls(rig, runs, name):
    c, run = MIXED[name], runs(name)
    census, stmt = lockstep(rig, c, None, CASES.actions(c), log=run["log"])
    assert census.ok(), str(census)
    assert stmt.results[N_POP - 1].sum() == 0 and stmt.results[:N_POP - 1, 0].all()      # member 4 entered nothing


@pytest.mark.parametrize("form", ["host", "device"])
def test_set_entries_mid_run(rig, form):
    """Line-ups handed over while races run, in the host form and (on a torch stream, a host-form step right behind it)
    the device form: every race picks its new line-up up at its own next spawn.  The device-form table names n_members
    and -3, which behave as the caller's."""
    import torch
    c = SWAP
    env = league_env(rig, c)
    dev = torch.device("cuda", env.device)
    stream = torch.cuda.Stream(device=dev)
    keep = []

    def hand_over(k, env, stmt):
        if k not in c["at"]:
            return
        table = np.array(c["at"][k][1], np.int32)
        if form == "host" and ((table < -2) | (table >= N_POP)).any():
            with pytest.raises(ValueError):
                env.set_entries(table)
            table = np.where((table < -2) | (table >= N_POP), -2, table).astype(np.int32)
        if form == "device":
            with torch.cuda.stream(stream):
                t = torch.from_numpy(table).to(dev)
                env.set_entries(t)
            keep.append(t)                        # (the step right behind it is the host form: it waits for the device)
        else:
            env.set_entries(table)
        stmt.set_entries(table)

    census, stmt = lockstep(rig, c, env, CASES.actions(c), before_step=hand_over)
    assert census.ok(need_mixed=True), str(census)
    if form == "device":
        assert ((stmt.live < -2) | (stmt.live >= N_POP)).any()          # the entries nobody could refuse ran as the caller's


def test_member_weights_reset_between_steps_take_effect_from_the_next_scan(rig):
    """``pop.set_device`` of member 1 between steps 4 and 5: step 5 still takes the answers kept from step 4's scan,
    step 5's scan is answered by the new weights, and no other member's car changes."""
    import torch
    c = dict(MIXED["5x3"], steps=9)
    pop, thetas, _ = TP.make_pop("small", N_POP, CASES.NET_SEED, CASES.GAIN)
    env = league_env(rig, c, pop=pop)
    old = [pop.member(k) for k in range(N_POP)]
    new_theta = TP.make_pop("small", 1, 9, CASES.GAIN)[1]
    seen = {}

    def swap(k, env, stmt):
        if k == 5:
            seen["kept"] = stmt.league_steers()
            pop.set_device(torch.from_numpy(new_theta).to(torch.device("cuda", env.device)), first=1)
        if k == 6:
            seen["after"] = (stmt.fed.copy(), stmt.league_steers(), stmt.ranges.copy(), stmt.live.copy())

    lockstep(rig, c, env, CASES.actions(c)[:c["steps"]], before_step=swap, pop=pop)
    fed, steers, ranges, live = seen["after"]
    took = ~np.isnan(seen["kept"])                # the scripted cars that ran into step 5: the answers from before the swap
    assert (took & (live == 1)).any() and same_bits(fed[took, 1], seen["kept"][took])
    ones = np.nonzero((live == 1) & ~np.isnan(steers))[0]
    rest = np.nonzero((live >= 0) & (live != 1) & ~np.isnan(steers))[0]
    assert ones.size and rest.size
    for e in ones:                                # member 1's cars: the new weights, not the old ones
        assert steers[e].tobytes() != old[1].predict_many(ranges[e][None])[0].tobytes(), e
    for e in rest:                                # everybody else: the member's own Policy from before the swap
        assert steers[e].tobytes() == old[live[e]].predict_many(ranges[e][None])[0].tobytes(), e
    assert same_bits(pop.get(1), new_theta[0]) and same_bits(pop.get(0), thetas[0])


# ---------------------------------------------------------------- 7. other league calls in between
def test_other_league_calls_between_steps_change_nothing(rig, runs):
    """``predict_rows`` and a ``race_league`` roll-out regroup the population's buffers between two env steps."""
    c, run = MIXED["5x3"], runs("5x3")
    env = league_env(rig, c)
    pop, cars, m = rig["pop"], rig["cars"], rig["m"]
    states, speeds = _race_starts(rig["g"], rig["dt"], 2, 3, 52)
    scans = np.random.default_rng(1).uniform(0.2, 12.0, (7, c["B"])).astype(np.float32)
    got = [snapshot(env, (env.reset(seed=c["seed"]),))]
    for k, a in enumerate(run["acts"][:12]):
        pop.predict_rows(scans, [4, 4, -1, 0, 4, 2, 4])
        if k % 3 == 0:
            cars.race_league(m, pop, [[4, 4, -1], [0, 4, 4]], states, 3, speeds, FOV, c["B"], support.edge(c["B"]), THRESH,
                             followgap=rig["fg"], steer_clip=CLIP)
            m.set_noise(STD, NOISE_SEED, BASE)
        got.append(snapshot(env, env.step(a)))
    for k, (x, y) in enumerate(zip(got, run["log"])):
        for u, v in zip(x["out"], y["out"]):
            assert same_bits(u, v), k
        assert same_bits(x["steers"], y["steers"]), k
        assert results_block(x["results"]).tolist() == results_block(y["results"]).tolist(), k


# ---------------------------------------------------------------- 8. the results
def results_from_outputs(c, log, n_members, pool):
    """The statement's per-race results over the run's own ``read()`` outputs: a race is counted in the call after
    which it reads over, when the call before left it running or over (then this call spawned it anew)."""
    R, P = c["R"], c["P"]
    total = np.zeros((n_members + 2, 8), np.int64)
    want = [total.copy()]
    prev = None
    for snap in log:
        rd = snap["read"]
        for r in range(R):
            fresh = prev is None or prev["race_over"][r] != 0 and rd["race_episodes"][r] != prev["race_episodes"][r]
            ran = prev is not None and prev["race_over"][r] == 0
            if rd["race_over"][r] == 0 or not (fresh or ran):
                continue
            gains = [rd["states"][r, k, 8] - pool[rd["start_index"][r, k], k, 8] for k in range(P)]
            for row, col in LE.race_results(snap["entries"]["live"][r], rd["ticks"][r], gains, rd["done"][r], n_members,
                                            lambda e: -1 <= e < n_members):
                total[row] += col
        prev = rd
        want.append(total.copy())
    return want[1:]


@pytest.mark.parametrize("name", ["5x3", "2x8"])
def test_results_equal_the_statement_over_the_runs_own_outputs(rig, runs, name):
    c, run = MIXED[name], runs(name)
    want = results_from_outputs(c, run["log"], N_POP, pool_of(rig, c))
    for k, (snap, w) in enumerate(zip(run["log"], want)):
        assert results_block(snap["results"]).tolist() == w.tolist(), k
    final = want[-1]
    assert final[:, 0].sum() >= 2 * c["R"] * c["P"] and not final[N_POP - 1].any()      # every race over at least twice
    assert (final[:, 4] > 0).sum() >= 3 and final[N_POP + 1, 7] + final[N_POP + 1, 4] > 0
    assert final[:, 3].sum() == final[:, 0].sum() * (c["P"] - 1)
    assert final[:, 5].sum() - final[N_POP + 1, 5] == final[N_POP + 1, 3] - final[N_POP + 1, 5]  # callers faced = faced by callers
    env = run["env"]
    assert results_block(env.league_results(clear=True)).tolist() == final.tolist()
    assert not results_block(env.league_results()).any()
    env.reset(seed=1)                             # a reset neither clears nor counts
    assert not results_block(env.league_results()).any()


@pytest.mark.parametrize("n_members", [70, 300])
def test_results_and_answers_of_a_large_population(rig, n_members):
    """524 cars at 64 beams, 520 of them one member's (65 network workgroups from one table segment), the others the last
    member of each 64-member block, FollowGap and the caller: the kept answers are the population's row-indexed
    evaluation of the env's own observations, and the results the statement's over the env's own outputs."""
    m, cars, fg = rig["m"], rig["cars"], rig["fg"]
    R, P, B = 262, 2, 64
    pop, thetas, _ = TP.make_pop("single", n_members, 5)
    big = n_members - 1
    entries = np.full((R, P), big, np.int32)
    entries[[3, 100, 200, 261], [1, 0, 1, 0]] = (63 if n_members > 64 else 0, -1, -2, 64 % n_members)
    assert (entries == big).sum() == 520
    pool, _ = _race_starts(rig["g"], rig["dt"], 4, P, 52)
    pool[:, :, 3] = 3.0
    m.set_noise(STD, NOISE_SEED, BASE)
    env = RaceEnv(m, pool, R, B, FOV, support.edge(B), THRESH, car=cars, league=(pop, entries), followgap=fg,
                  seat_speed=5.0, min_running=1, max_ticks=3, auto_reset=True, substeps=4, steer_clip=CLIP)
    c = dict(R=R, P=P)
    log = [snapshot(env, (env.reset(seed=2),))]
    acts = np.full((R, P, 2), np.nan, np.float32)
    acts[entries == -2] = (3.0, 0.1)
    for k in range(5):
        log.append(snapshot(env, env.step(acts)))
    for k, snap in enumerate(log):
        raw = snap["out"][0].reshape(R * P, B)
        ans = answers(rig, raw, entries, pop).reshape(R, P)
        ans[snap["read"]["done"] != 0] = np.nan
        assert same_bits(ans, snap["steers"]), k
    want = results_from_outputs(c, log, n_members, pool)
    for k, (snap, w) in enumerate(zip(log, want)):
        assert results_block(snap["results"]).tolist() == w.tolist(), k
    final = want[-1]
    assert final[big, 0] >= 520 and final[n_members, 0] >= 1 and final[n_members + 1, 0] >= 1
    untouched = np.setdiff1d(np.arange(n_members), np.unique(entries[entries >= 0]))
    assert untouched.size >= n_members - 3 and not final[untouched].any()
    assert len({np.float32(x).tobytes() for x in log[0]["steers"][entries == big][:8]}) > 1


# ---------------------------------------------------------------- 9. refusals
def test_refusals_leave_the_handles_usable(rig):
    torch = pytest.importorskip("torch")
    m, fg, pop, cars = rig["m"], rig["fg"], rig["pop"], rig["cars"]
    L = _lib.lib()
    c = dict(MIXED["5x3"], R=2, entries=[[-2, 0, -1], [1, -1, -2]])
    R, P, B = 2, 3, 64
    c["B"] = B
    N = R * P
    i32p, f32p = _lib.i32p, _lib.f32p
    good = np.array(c["entries"], np.int32).reshape(-1)
    acts = [CASES.masked(a[:R], np.array(c["entries"])) for a in CASES.actions(MIXED["5x3"])[:6]]

    def reference_run():
        env = league_env(rig, c)
        return [env.reset(seed=4)] + [env.step(a) for a in acts]

    want = reference_run()

    def usable(env):
        got = [env.reset(seed=4)] + [env.step(a) for a in acts]
        for x, y in zip(got, want):
            for u, v in zip(x if isinstance(x, tuple) else (x,), y if isinstance(y, tuple) else (y,)):
                assert same_bits(u, v)

    def attach(e, entry=good, g=fg._h, p=pop._h, speed=(3.5, 4.5, 5.5), null_entries=False):
        sp = np.array(speed, np.float32)
        en = np.ascontiguousarray(entry, np.int32)
        return L.rl_env_attach_league(e, g, p, None if null_entries else en.ctypes.data_as(i32p), sp.ctypes.data_as(f32p))

    m.set_noise(STD, NOISE_SEED, BASE)
    kw = dict(CASES.env_kw(c), **WINDOW)
    env = RaceEnv(m, pool_of(rig, c), R, B, FOV, support.edge(B), THRESH, car=cars, **kw)
    drive = DriveEnv(m, pool_of(rig, c).reshape(-1, 11), N, B, FOV, support.edge(B), THRESH, car=cars)
    wide = PolicyPopulation((40, 16, 8, 1), 2, in_start=30)             # window [30, 70): 64 beams do not hold it
    buf_f, buf_i = np.zeros(N, np.float32), np.zeros(N, np.int32)
    res = np.zeros((N_POP + 2, 8), np.int64)
    res_p = res.ctypes.data_as(C.POINTER(C.c_int64))

    d_good = torch.from_numpy(good).cuda()
    torch.cuda.synchronize()

    def reads(e):
        return (L.rl_env_set_league_entries(e, good.ctypes.data_as(i32p)),
                L.rl_env_set_league_entries_device(e, d_good.data_ptr(), None),
                L.rl_env_read_league_steers(e, buf_f.ctypes.data_as(f32p)), L.rl_env_read_league_steers_device(e, None, None),
                L.rl_env_read_league_entries(e, buf_i.ctypes.data_as(i32p), None),
                L.rl_env_read_league_results(e, res_p, 0))

    # no league attached; a null env; an env that is no race env
    assert set(reads(env._h)) == {RL_ERR_INVALID} and set(reads(None)) == {RL_ERR_INVALID}
    assert L.rl_last_error()
    for kw_ in (dict(e=None), dict(e=drive._h), dict(p=None), dict(g=None), dict(entry=np.where(good == 0, N_POP, good)),
                dict(entry=np.where(good == 0, -3, good)), dict(speed=(3.5, math.nan, 5.5)), dict(speed=(3.5, 4.5, math.inf)),
                dict(p=wide._h, entry=np.minimum(good, 1))):
        e = kw_.pop("e", env._h)
        assert attach(e, **kw_) == RL_ERR_INVALID, kw_
    env.reset(seed=1)                                                   # the refusals changed nothing: still a plain env
    assert set(reads(env._h)) == {RL_ERR_INVALID}
    # seats and a league exclude each other, both ways
    env.attach_seats([None, fg, None], 3.0)
    assert attach(env._h) == RL_ERR_INVALID
    env.attach_seats(None)
    # what is no refusal: a null g without a -1, a non-finite speed of a seat with caller's cars only, a narrow scan
    # without a member
    assert attach(env._h, entry=np.where(good == -1, -2, good), g=None, speed=(3.5, 4.5, math.nan)) == 0
    assert attach(env._h, entry=np.where(good >= 0, -1, good), p=wide._h) == 0
    assert attach(env._h) == 0
    sp = _lib.SeatParams()
    sp.driver[:3] = (0, 1, 0)
    sp.speed[:3] = (1.0, 1.0, 1.0)
    assert L.rl_env_attach_seats(env._h, fg._h, None, C.byref(sp)) == RL_ERR_INVALID
    assert L.rl_env_attach_seats(env._h, None, None, None) == 0          # (a null table detaches seats: nothing to refuse)
    assert attach(env._h) == 0
    # before a reset: the steers, the results and the live table; the pending table reads
    r = reads(env._h)
    assert r[:2] == (0, 0) and r[2:] == (RL_ERR_INVALID,) * 4
    assert L.rl_env_read_league_entries(env._h, None, buf_i.ctypes.data_as(i32p)) == 0 and buf_i.tolist() == good.tolist()
    with pytest.raises(_lib.ScanLibError):
        env.step(acts[0])                                               # a reset first, as with seats
    env.league = (pop, fg, league.seat_speeds(c["speed"], P))
    usable(env)
    # refused setters and reads change nothing
    for entry in (np.where(good == 0, N_POP, good), np.where(good == 0, -3, good)):
        assert L.rl_env_set_league_entries(env._h, np.ascontiguousarray(entry, np.int32).ctypes.data_as(i32p)) == RL_ERR_INVALID
    assert L.rl_env_set_league_entries(env._h, None) == RL_ERR_INVALID
    assert L.rl_env_set_league_entries_device(env._h, None, None) == RL_ERR_INVALID
    assert L.rl_env_read_league_results(env._h, None, 0) == RL_ERR_INVALID
    assert same_bits(env.entries()["pending"].reshape(-1), good)
    assert attach(env._h, entry=np.where(good == 0, N_POP, good)) == RL_ERR_INVALID     # a refused attach: the league stays
    assert attach(env._h, p=None) == RL_ERR_INVALID
    usable(env)
    # NaN in a scripted car's action row is no refusal (every run above fed it); a league with a null g and no -1 runs
    env.attach_league(pop, np.where(np.array(c["entries"]) == -1, -2, np.array(c["entries"])), None, c["speed"])
    env.reset(seed=4)
    out = env.step(np.where(np.isnan(acts[0]), np.float32(1.0), acts[0]))
    assert (out[2] != 3).all() and np.isnan(env.league_steers()[np.array(c["entries"]) < 0]).all()
    # with a null g the device form's -1 is the caller's: its action row is read
    with torch.cuda.stream(torch.cuda.Stream()):
        env.set_entries(torch.from_numpy(good).cuda())
    env.reset(seed=4)
    assert np.isnan(env.league_steers().reshape(-1)[good < 0]).all() and same_bits(env.entries()["live"].reshape(-1), good)
    # detached, the env is the plain env again
    env.attach_league(None)
    with pytest.raises(_lib.ScanLibError):
        env.step(acts[0])
    with pytest.raises(ValueError):
        env.league_steers()
    m.set_noise(STD, NOISE_SEED, BASE)
    never = RaceEnv(m, pool_of(rig, c), R, B, FOV, support.edge(B), THRESH, car=cars, **kw)
    fed = CASES.actions(MIXED["5x3"])[:5, :R]
    assert same_bits(env.reset(seed=9), never.reset(seed=9))
    for a in fed:
        for x, y in zip(env.step(a), never.step(a)):
            assert same_bits(x, y)


# ---------------------------------------------------------------- 10. the facade
def test_facade_matches_hand_built():
    g = DC.race_maze()
    cfg = dict(RC.DEFAULT_CAR)
    cfg.update(scan_dist_to_base=D_BASE, batch_size=40, scan_beams=1080, scan_fov=FOV, scan_std=0.01,
               scan_max_range=15.0, free_thresh=0.8)
    sim = RacecarSimulator(cfg)
    omap = range_libc.PyOMap(g)
    sim.setMap(omap, g.resolution, g.origin)
    sim.setRaytracingMethod("RMGPU")
    pop, _, _ = TP.make_pop("fixture", 3)
    R, P = 3, 3
    states, _ = _race_starts(g, omap.distance_transform(), R, P, 52)
    entries = np.array([[-2, -1, 0], [1, -2, 2], [-2, 2, 2]])
    kw = dict(obs_window=(180, 720, 1), obs_clip=15, obs_scale=15, min_running=2, steer_clip=0.4189, max_ticks=4)
    env = sim.raceEnv(R, states, league=(pop, entries), seat_speed=3.0, **kw)
    fg = sim._followgap
    hand = RaceEnv(sim.scan_simulator.scan_method, states, R, 1080, FOV, sim.edge_distances, cfg["ttc_thresh"],
                   car=sim.car, scan_dist_to_base=D_BASE, league=(pop, entries), followgap=fg, seat_speed=3.0, **kw)
    assert env.obs_shape == (R * P, 720) and env.league[0] is pop and env.league[1] is fg
    assert same_bits(env.reset(seed=2), hand.reset(seed=2))
    for a in DC.actions(21, 6, R * P).reshape(6, R, P, 2):
        for x, y in zip(env.step(a), hand.step(a)):
            assert same_bits(x, y)
        assert same_bits(env.league_steers(), hand.league_steers())
    assert results_block(env.league_results()).tolist() == results_block(hand.league_results()).tolist()
    assert results_block(env.league_results())[:, 0].sum() >= R * P
