"""Per-seat drivers (include/scanlib_seats.h: rl_car_race_seats, rl_env_attach_seats, rl_env_read_seats*; CarBatch.
race_seats, RaceEnv(seats=...), RacecarSimulator.raceSeatsMany) on the MI355X: against the entry points they become
with one kind of driver, teacher-forced against the composed public calls, the seated env against a plain env whose
caller writes the drivers' pairs, against the statement (tests/seat_statement.py), and against the roll-out.

Shapes: 5 races x 3 cars = 15 cars (a DRIVE_CARS = 8 workgroup part filled, seats out of step with the waves), groups
1, 3 and 8, 64 beams (ROWS 1, full) and 65 (one lane in the last row); 1081 only with the 720-input fixture network."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import drive_cases as DC
import policy_statement as PS
import seat_statement as SS
import support
from conftest import GOLD
from env_statement import observation
from support import D_BASE, FOV, THRESH, same_bits
from test_gpu_race_env import RaceComposed, _race_starts
from pyracecarsimulator_amd import Policy, RaceEnv, RacecarSimulator, Track, _lib, range_libc
from pyracecarsimulator_amd import racecar as RC

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

MRX = DC.RACE_MRX
RL_ERR_INVALID = -1
CLIP = 0.2                                        # steer_clip of every case: below the small network's larger answers
STD, NOISE_SEED, BASE = 0.02, 3, 777              # scan noise of every case


def small_net(seed=1, gain=0.9):
    """A seeded 40 -> 16 -> 8 -> 1 network on beams [5, 45), its last layer scaled so that some answers pass CLIP."""
    rng = np.random.default_rng(seed)
    dims = (40, 16, 8, 1)
    layers = [(rng.normal(0.0, 1.0 / math.sqrt(k), (k, n)).astype(np.float32), rng.normal(0.0, 0.1, n).astype(np.float32))
              for k, n in zip(dims[:-1], dims[1:])]
    layers[-1] = ((layers[-1][0] * np.float32(gain)).astype(np.float32), layers[-1][1])
    return layers


@pytest.fixture(scope="module")
def rig():
    g = DC.race_maze()
    omap = range_libc.PyOMap(g)
    m = range_libc.PyRayMarchingGPU(omap, MRX)
    layers = small_net()
    pol = Policy(layers=layers, in_start=5)
    rig = dict(g=g, omap=omap, dt=omap.distance_transform(), m=m, fg=support.followgap(), pol=pol, layers=layers,
               cars=RC.CarBatch())
    yield rig
    m.set_noise(0.0, 0, 0)


def same_or_nan(a, b):
    return same_bits(a, b)                        # (the NaN rows of both are the all-ones fill)


# ---------------------------------------------------------------- 1. every seat FollowGap: rl_car_race_followgap
# (seed of the starts: test_gpu_race_env's clear starts; some cars crash within the ticks and some do not)
@pytest.mark.parametrize("P,B,seed", [(3, 64, 52), (3, 65, 52), (8, 65, 58), (1, 64, 51)])
def test_all_followgap_seats_equal_race_followgap(rig, P, B, seed):
    m, fg, cars = rig["m"], rig["fg"], rig["cars"]
    R, T = 5, 40
    states, speeds = _race_starts(rig["g"], rig["dt"], R, P, seed)
    speeds = speeds + 2.0                         # 3 .. 6 m/s: walls within 40 ticks
    edge = support.edge(B)
    steer0 = np.random.default_rng(seed).uniform(-0.2, 0.2, (R, P)).astype(np.float32)
    m.set_noise(STD, NOISE_SEED, BASE)
    want = cars.race_followgap(m, fg, states, T, speeds, FOV, B, edge, THRESH, steer0=steer0, trace=True)
    # (a clip far below FollowGap's answers: it is the network's and must not touch these seats)
    got = cars.race_seats(m, [fg] * P, states, T, speeds, FOV, B, edge, THRESH, steer_clip=0.01, steer0=steer0,
                          trace=True)
    assert (np.abs(want[3][~np.isnan(want[3])]) > 0.01).any()
    assert len(got) == len(want) == 6
    for i, (x, y) in enumerate(zip(got, want)):
        assert same_or_nan(x, y), i
    assert (want[0] >= 0).any() and (want[0] < 0).any()
    # without the traces too
    got = cars.race_seats(m, [fg] * P, states, T, speeds, FOV, B, edge, THRESH, steer0=steer0)
    assert len(got) == 4 and all(same_or_nan(x, y) for x, y in zip(got, want[:4]))


# ---------------------------------------------------------------- 2. one policy seat alone: rl_car_drive_policy
@pytest.mark.parametrize("B,clip", [(64, CLIP), (65, CLIP), (65, None), (1081, 0.4189)])
def test_single_policy_seat_equals_drive_policy(rig, B, clip):
    m, cars = rig["m"], rig["cars"]
    if B == 1081:
        layers, relu = PS.load_fixture(os.path.join(GOLD, "policy_mlp720.npz"))
        pol = Policy.from_arrays(layers, relu)
    else:
        pol = rig["pol"]
    R, T = 15, 30
    states, speeds = support.starts(rig["g"], rig["dt"], R, 21, 10.0)
    edge = support.edge(B)
    m.set_noise(STD, NOISE_SEED, BASE)
    want = cars.drive_policy(m, pol, states, T, speeds, FOV, B, edge, THRESH, steer_clip=clip, trace=True)
    got = cars.race_seats(m, [pol], states[:, None, :], T, speeds[:, None], FOV, B, edge, THRESH, steer_clip=clip,
                          trace=True)
    for i, (x, y) in enumerate(zip(got, want)):
        assert same_or_nan(x[:, 0], y), i
    st = want[3][~np.isnan(want[3])]
    assert st.size and (clip is None or B == 1081 or (np.abs(st) > clip).any())


# ---------------------------------------------------------------- 3. mixed seats, teacher-forced
def teacher_forced(rig, seats, states, speeds, T, B, clip):
    """``race_seats`` traced, and every link of every tick from the composed public calls: the race scan at the traced
    lidar poses and states at that tick's noise offset, is_crashed, the seat driver's answer (and not the other
    driver's), one rollout step with the clamped steer.  Returns a census."""
    m, fg, pol, cars = rig["m"], rig["fg"], rig["pol"], rig["cars"]
    R, P = states.shape[:2]
    N = R * P
    edge = support.edge(B)
    m.set_noise(STD, NOISE_SEED, BASE)
    first, final, vel, steers, sp, st = (a.reshape((N,) + a.shape[2:]) for a in cars.race_seats(
        m, seats, states, T, speeds, FOV, B, edge, THRESH, steer_clip=clip, trace=True))
    pub = RaceComposed(m, cars, N, P, B, edge, 1, STD, NOISE_SEED, BASE)
    flat, fspd = states.reshape(N, 11), speeds.reshape(N)
    last = np.where(first >= 0, first, T - 1)
    census = dict(crashed=int((first >= 0).sum()), clamped=0, seen=0, differ=0)
    for t in range(T):
        now = st[np.arange(N), np.minimum(t, last)]           # a wreck keeps its crash-tick row
        poses = sp[np.arange(N), np.minimum(t, last)]
        ranges = pub.scan(poses, now[:, :3], t)
        census["seen"] += int((ranges != pub.scan_alone(poses, t)).sum())
        a_fg, a_pol = fg.eval_many(ranges), pol.predict_many(ranges)
        for n in range(N):
            if t > last[n]:
                assert np.isnan(st[n, t]).all() and np.isnan(steers[n, t]) and np.isnan(vel[n, t])
                continue
            prev = flat[n] if t == 0 else st[n, t - 1]
            steer_in = 0.0 if t == 0 else float(steers[n, t - 1])
            net = seats[n % P] is pol
            if t > 0 and net and clip and abs(steer_in) > clip:
                steer_in = math.copysign(clip, steer_in)
                census["clamped"] += 1
            _, one, _ = cars.rollout(prev[None], np.array([[[fspd[n], steer_in]]]), n_steps=1, action_every=1)
            assert same_bits(one[0], st[n, t]), (n, t)
            assert vel[n, t] == st[n, t, 3]
            assert same_bits(support.lidar_poses(st[n, t]), sp[n, t]) or support.within_one_ulp(support.lidar_poses(st[n, t]), sp[n, t])
            crashed = RC.is_crashed(ranges[n], B, 1, edge, THRESH) >= 0
            assert crashed == (first[n] == t), (n, t)
            if crashed:
                assert np.isnan(steers[n, t])
                continue
            mine, other = (a_pol, a_fg) if net else (a_fg, a_pol)
            assert mine[n].tobytes() == steers[n, t].tobytes(), (n, t, net)
            census["differ"] += int(other[n].tobytes() != steers[n, t].tobytes())
    assert same_bits(final, st[np.arange(N), last])
    return census


# (seeds of the starts picked on the CPU, docs/history/seats.md: crashes, clamped answers and occluded rays all occur)
@pytest.mark.parametrize("P,B,mix,seed", [(3, 65, "fpf", 52), (8, 64, "pfpppfpf", 58)])
def test_mixed_seats_teacher_forced(rig, P, B, mix, seed):
    R, T = (5, 30) if P == 3 else (2, 24)
    seats = [rig["fg"] if c == "f" else rig["pol"] for c in mix]
    states, speeds = _race_starts(rig["g"], rig["dt"], R, P, seed)
    census = teacher_forced(rig, seats, states, speeds + 2.0, T, B, CLIP)
    assert census["crashed"] >= 1 and census["clamped"] >= 1 and census["seen"] > 0, census
    assert census["differ"] > 0.9 * R * P * T * 0.5, census       # the other driver would have answered otherwise


# ---------------------------------------------------------------- 4 / 5 / 7. the seated env
ENV = dict(R=5, P=3, B=65, M=4, S=2, steps=24, seed=5, pool_seed=54, speed=(0.0, 4.5, 5.5))
ENV_KW = dict(min_running=2, max_ticks=0, auto_reset=True, crash_reward=-2.5, steer_clip=CLIP, substeps=ENV["S"])
WINDOW = dict(obs_window=(5, 40, 1), obs_clip=15.0, obs_scale=15.0)


def ring_track():
    a = np.arange(24) * (2 * math.pi / 24)
    return Track(np.stack([6.4 + 4.0 * np.cos(a), 6.4 + 4.0 * np.sin(a)], -1), True)


def env_actions():
    """(steps, R, P, 2) float32 with NaN in the scripted seats' rows (seats 1 and 2)."""
    R, P = ENV["R"], ENV["P"]
    a = DC.actions(77, ENV["steps"], R * P).reshape(ENV["steps"], R, P, 2)
    a[:, :, 1:, :] = np.nan
    return a


def snapshot(env, out):
    ts = env.track_state()
    return dict(out=tuple(np.array(x) for x in out), read={k: v.copy() for k, v in env.read().items()},
                track={k: np.array(v) for k, v in ts.items()}, steers=env.seat_steers() if env.seats else None)


@pytest.fixture(scope="module")
def seated_run(rig):
    """The seated env of cases 4, 5 and 7 run once in its host form: seats (caller, FollowGap, policy), window
    (5, 40, 1) in the network's input form, noise, auto-reset, a track that pays the reward.  Returns the env, its
    pieces and one snapshot per call."""
    m, cars = rig["m"], rig["cars"]
    R, P, B = ENV["R"], ENV["P"], ENV["B"]
    pool, _ = _race_starts(rig["g"], rig["dt"], ENV["M"], P, ENV["pool_seed"])
    pool[:, :, 3] = 3.0
    edge = support.edge(B)
    m.set_noise(STD, NOISE_SEED, BASE)
    seats = [None, rig["fg"], rig["pol"]]
    trk = ring_track()
    env = RaceEnv(m, pool, R, B, FOV, edge, THRESH, car=cars, seats=seats, seat_speed=ENV["speed"], track=trk,
                  progress_reward=True, **WINDOW, **ENV_KW)
    acts = env_actions()
    log = [snapshot(env, (env.reset(seed=ENV["seed"]),))]
    for a in acts:
        log.append(snapshot(env, env.step(a)))
    return dict(env=env, pool=pool, edge=edge, seats=seats, track=trk, acts=acts, log=log)


def composed_answers(rig, raw_obs):
    """The scripted seats' answers to full raw scans (R, P, B) by the public calls; NaN in the caller's seat."""
    R, P, B = raw_obs.shape
    flat = np.ascontiguousarray(raw_obs.reshape(R * P, B))
    a_fg, a_pol = rig["fg"].eval_many(flat).reshape(R, P), rig["pol"].predict_many(flat).reshape(R, P)
    out = np.full((R, P), np.nan, np.float32)
    out[:, 1], out[:, 2] = a_fg[:, 1], a_pol[:, 2]
    return out


def test_seated_env_equals_plain_env_fed_the_drivers_pairs(rig, seated_run):
    """The parent commit's only way: a plain RaceEnv on the raw full window, FollowGap and the network evaluated on its
    observations from Python, their answers scattered into the action rows."""
    m, cars = rig["m"], rig["cars"]
    R, P, B, log = ENV["R"], ENV["P"], ENV["B"], seated_run["log"]
    m.set_noise(STD, NOISE_SEED, BASE)
    plain = RaceEnv(m, seated_run["pool"], R, B, FOV, seated_run["edge"], THRESH, car=cars, track=seated_run["track"],
                    progress_reward=True, **ENV_KW)
    win = (WINDOW["obs_window"], WINDOW["obs_clip"], WINDOW["obs_scale"])

    def compare(k, out, rd_done):
        snap = log[k]
        raw = out[0]
        assert same_bits(observation(raw.reshape(R * P, B), *win).reshape(R, P, -1), snap["out"][0]), k
        for x, y in zip(out[1:], snap["out"][1:]):
            assert same_bits(x, y), k
        rd = plain.read()
        for key in rd:
            assert same_bits(rd[key], snap["read"][key]), (k, key)
        ts = plain.track_state()
        for key in ts:
            assert same_bits(np.asarray(ts[key]), snap["track"][key]), (k, key)
        ans = composed_answers(rig, raw)
        ans[rd["done"] != 0] = np.nan
        assert same_bits(ans, snap["steers"]), k
        return composed_answers(rig, raw)

    ans = compare(0, (plain.reset(seed=ENV["seed"]),), None)
    census = dict(scripted_crash=False, attrition=False, respawned=False, clamped=False, bad=False)
    speed = np.float32(ENV["speed"])
    for k, a in enumerate(seated_run["acts"], 1):
        before = plain.read()
        fed = a.copy()
        fed[:, 1:, 0] = speed[1:]
        fed[:, 1:, 1] = ans[:, 1:]
        assert np.isnan(a[:, 1:]).all() and not np.isnan(a[:, 0]).any()
        out = plain.step(fed)
        running = (before["done"] == 0) & (before["race_over"] == 0)[:, None]
        census["clamped"] |= bool((running[:, 2] & (np.abs(ans[:, 2]) > CLIP)).any())
        ans = compare(k, out, None)
        rd = plain.read()
        census["scripted_crash"] |= bool((running[:, 1:] & (rd["done"][:, 1:] == 1)).any())
        census["attrition"] |= bool((rd["race_over"] == 1).any())
        census["respawned"] |= bool((rd["race_episodes"] > 0).any())
    assert all(v for k, v in census.items() if k != "bad"), census
    assert len(seated_run["acts"]) >= 16


def test_seated_env_equals_the_statement_over_public_calls(rig, seated_run):
    m, cars, fg, pol = rig["m"], rig["cars"], rig["fg"], rig["pol"]
    R, P, B, log = ENV["R"], ENV["P"], ENV["B"], seated_run["log"]
    N = R * P
    pub = RaceComposed(m, cars, N, P, B, seated_run["edge"], ENV["S"], STD, NOISE_SEED, BASE)

    def answer(driver, row):
        row = np.ascontiguousarray(row[None])
        return (driver.eval_many(row) if driver is fg else driver.predict_many(row))[0]

    kw = {k: v for k, v in ENV_KW.items() if k != "substeps"}
    stmt = SS.SeatEnvStatement(seated_run["pool"], R, B, pub.step_cars, pub.scan, pub.is_crashed, answer,
                               seated_run["seats"], ENV["speed"], scan_dist_to_base=D_BASE, **WINDOW, **kw)
    wreck_seen = 0

    def compare(k, want_obs, want_done, want_rew=None):
        snap = log[k]
        assert same_bits(snap["out"][0], want_obs.reshape(R, P, -1)), k
        if want_rew is not None:
            assert same_bits(snap["out"][2], want_done.reshape(R, P)), k
        rd = snap["read"]
        assert same_bits(rd["states"], stmt.states.reshape(R, P, 11)), k
        for key, want in (("ticks", stmt.tick), ("episodes", stmt.episode), ("start_index", stmt.start_index),
                          ("done", stmt.done)):
            assert same_bits(rd[key], want.reshape(R, P)), (k, key)
        for key, want in (("race_ticks", stmt.race_tick), ("race_episodes", stmt.race_episode),
                          ("race_start_index", stmt.race_start_index), ("race_over", stmt.race_over)):
            assert same_bits(rd[key], want), (k, key)
        assert same_bits(snap["steers"], stmt.seat_steers().reshape(R, P)), k

    obs, done = stmt.reset(ENV["seed"])
    compare(0, obs, done)
    for k, a in enumerate(seated_run["acts"], 1):
        obs, rew, done = stmt.step(a.reshape(N, 2))
        compare(k, obs, done, rew)                # (the reward is the track's: test 4 holds it)
        # a wreck in a race that runs on, seen by a scripted car that still runs: its scan with the wreck far away
        wrecks = (stmt.done != 0) & np.repeat(stmt.race_over == 0, P)
        if wrecks.any():
            away = stmt.states[:, :3].copy()
            away[wrecks, :2] = -100.0
            moved = pub.scan(support.lidar_poses(stmt.states), away, stmt.k)
            rows = [e for e in range(N) if stmt.scripted(e) and stmt.done[e] == 0 and wrecks[e // P * P:(e // P + 1) * P].any()]
            wreck_seen += int((moved[rows] != stmt.ranges[rows]).sum())
    assert wreck_seen > 0


def test_device_form_and_detach(rig, seated_run):
    torch = pytest.importorskip("torch")
    m, cars = rig["m"], rig["cars"]
    R, P, B, log = ENV["R"], ENV["P"], ENV["B"], seated_run["log"]
    m.set_noise(STD, NOISE_SEED, BASE)
    env = RaceEnv(m, seated_run["pool"], R, B, FOV, seated_run["edge"], THRESH, car=cars, seats=seated_run["seats"],
                  seat_speed=ENV["speed"], track=seated_run["track"], progress_reward=True, **WINDOW, **ENV_KW)
    dev = torch.device("cuda", env.device)
    stream = torch.cuda.Stream(device=dev)
    acts = torch.from_numpy(seated_run["acts"]).to(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        got = [(env.reset(seed=ENV["seed"], on_device=True).clone(), None, None, env.seat_steers(on_device=True).clone())]
        for a in acts[:10]:
            o, r, d = env.step(a)
            got.append((o.clone(), r.clone(), d.clone(), env.seat_steers(on_device=True).clone()))
    stream.synchronize()
    for k, (o, r, d, s) in enumerate(got):
        snap = log[k]
        assert same_bits(o.cpu().numpy(), snap["out"][0]), k
        if r is not None:
            assert same_bits(r.cpu().numpy(), snap["out"][1]) and same_bits(d.cpu().numpy(), snap["out"][2]), k
        assert same_bits(s.cpu().numpy(), snap["steers"]), k
    # the host form takes over mid-run
    snap = snapshot(env, env.step(seated_run["acts"][10]))
    for x, y in zip(snap["out"], log[11]["out"]):
        assert same_bits(x, y)
    assert same_bits(snap["steers"], log[11]["steers"])

    # detached, the env gives the bits of one that never had seats
    env.attach_seats(None)
    with pytest.raises(_lib.ScanLibError):
        env.step(seated_run["acts"][0])           # a reset first, as with a track
    never = RaceEnv(m, seated_run["pool"], R, B, FOV, seated_run["edge"], THRESH, car=cars, track=seated_run["track"],
                    progress_reward=True, **WINDOW, **ENV_KW)
    fed = DC.actions(78, 6, R * P).reshape(6, R, P, 2)
    assert same_bits(env.reset(seed=9), never.reset(seed=9))
    for a in fed:
        for x, y in zip(env.step(a), never.step(a)):
            assert same_bits(x, y)
    for key, v in never.read().items():
        assert same_bits(env.read()[key], v), key
    with pytest.raises(ValueError):
        env.seat_steers()


# ---------------------------------------------------------------- 6. every seat FollowGap: the env is the roll-out
@pytest.mark.parametrize("P,B,seed", [(3, 64, 52), (8, 65, 58), (1, 65, 51)])
def test_followgap_seated_env_equals_race_followgap(rig, P, B, seed):
    """auto_reset off, every seat FollowGap, NaN actions: first crash ticks and steers of rl_car_race_followgap, whose
    noise base lies N B above the env's (the reset takes slot 0)."""
    m, fg, cars = rig["m"], rig["fg"], rig["cars"]
    R, T = 5, 40
    N = R * P
    states, speeds = _race_starts(rig["g"], rig["dt"], R, P, seed)
    seat_speed = (np.arange(P) % 3 + 3.5).astype(np.float32)
    edge = support.edge(B)
    m.set_noise(STD, NOISE_SEED, BASE)
    env = RaceEnv(m, states, R, B, FOV, edge, THRESH, min_running=1, auto_reset=False, car=cars, seats=[fg] * P,
                  seat_speed=seat_speed, obs_window=(0, 10, 1))
    env.reset(seed=0, start_index=np.arange(R))
    assert (env.read()["done"] == 0).all()
    steer0 = env.seat_steers()
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
        got = env.seat_steers()
        assert same_bits(got[go], steers[:, :, t][go]), t
        assert np.isnan(got[~go]).all()
    assert same_bits(want_first, first)
    assert same_bits(env.read()["states"], final)


# ---------------------------------------------------------------- 8. refusals
def test_refusals_leave_the_handles_usable(rig):
    m, fg, pol, cars = rig["m"], rig["fg"], rig["pol"], rig["cars"]
    L = _lib.lib()
    R, P, B, T = 2, 3, 64, 3
    states, speeds = _race_starts(rig["g"], rig["dt"], R, P, 52)
    edge = support.edge(B)
    m.set_noise(STD, NOISE_SEED, BASE)
    want = cars.race_seats(m, [fg, pol, fg], states, T, speeds, FOV, B, edge, THRESH)

    def raw(seat=(1, 2, 1), g=fg._h, p=pol._h, c=cars._h, h=m._h, group=P, nr=B, n_ticks=T, null_seats=False, clip=0.0):
        st = np.ascontiguousarray(states.reshape(-1, 11))
        sp = np.ascontiguousarray(speeds.reshape(-1))
        first = np.zeros(R * P, np.int32)
        sd = np.array(seat, np.int32)
        return L.rl_car_race_seats(c, h, g, p, None if null_seats else sd.ctypes.data_as(C.POINTER(C.c_int)), clip,
                                   st.ctypes.data_as(_lib.f64p), sp.ctypes.data_as(_lib.f64p), None, R, group, n_ticks,
                                   0.01, D_BASE, FOV, nr, support.edge(nr).ctypes.data_as(_lib.f64p), THRESH,
                                   first.ctypes.data_as(C.POINTER(C.c_int)), None, None, None, None, None)

    def usable():
        got = cars.race_seats(m, [fg, pol, fg], states, T, speeds, FOV, B, edge, THRESH)
        assert all(same_bits(x, y) for x, y in zip(got, want))

    assert raw() == 0
    pol_wide = Policy(layers=rig["layers"], in_start=30)          # window [30, 70): 64 beams do not hold it
    cdd = range_libc.PyCDDTCast(rig["omap"], MRX, 108)
    for kw in (dict(seat=(1, 0, 1)), dict(seat=(1, 3, 1)), dict(seat=(1, -1, 1)), dict(g=None), dict(p=None),
               dict(c=None), dict(h=None), dict(null_seats=True), dict(group=0), dict(group=9), dict(p=pol_wide._h),
               dict(nr=9), dict(n_ticks=0)):
        assert raw(**kw) == RL_ERR_INVALID, kw
        assert L.rl_last_error()
        usable()
    assert raw(h=cdd._h) < 0                                      # rl_car_race_followgap's own refusal
    assert raw(seat=(1, 1, 1), p=None) == 0 and raw(seat=(2, 2, 2), g=None) == 0      # an unused handle may be null
    usable()

    # the env
    env = RaceEnv(m, states, R, B, FOV, edge, THRESH, car=cars)
    def attach(e=env._h, g=fg._h, p=pol._h, driver=(0, 1, 2), speed=(math.nan, 2.0, 2.0)):
        sp = _lib.SeatParams()
        sp.driver[:3] = driver
        sp.speed[:3] = speed
        return L.rl_env_attach_seats(e, g, p, C.byref(sp))

    from pyracecarsimulator_amd import DriveEnv
    drive = DriveEnv(m, states.reshape(-1, 11), R * P, B, FOV, edge, THRESH, car=cars)
    buf = np.zeros(R * P, np.float32)
    fptr = buf.ctypes.data_as(_lib.f32p)
    assert L.rl_env_read_seats(env._h, fptr) == RL_ERR_INVALID    # no seats attached
    for kw in (dict(e=None), dict(e=drive._h), dict(driver=(0, 1, 3)), dict(driver=(0, -2, 2)), dict(g=None),
               dict(p=None), dict(speed=(0.0, math.inf, 2.0)), dict(speed=(0.0, 2.0, math.nan)), dict(p=pol_wide._h)):
        assert attach(**kw) == RL_ERR_INVALID, kw
    assert L.rl_env_read_seats(None, fptr) == RL_ERR_INVALID
    assert L.rl_env_read_seats_device(None, None, None) == RL_ERR_INVALID
    env.reset(seed=1)                                             # the refusals changed nothing: still a plain env
    assert L.rl_env_read_seats(env._h, fptr) == RL_ERR_INVALID
    assert attach() == 0                                          # (NaN speed in the caller's seat is not read)
    assert L.rl_env_read_seats(env._h, fptr) == RL_ERR_INVALID    # before a reset
    assert L.rl_env_read_seats_device(env._h, None, None) == RL_ERR_INVALID
    env.seats = (None, fg, pol)
    env.reset(seed=1)
    assert env.seat_steers().shape == (R, P) and np.isnan(env.seat_steers()[:, 0]).all()
    assert attach(driver=(0, 1, 9)) == RL_ERR_INVALID             # a refused attach leaves the seats as they were
    assert np.isfinite(env.seat_steers()[:, 1:]).all()
    usable()
    # a FollowGap seat alone needs no policy, and the other way round
    assert attach(p=None, driver=(0, 1, 1)) == 0 and attach(g=None, driver=(2, 0, 2), speed=(2.0, math.nan, 2.0)) == 0


# ---------------------------------------------------------------- 9. the facade
def test_facade_matches_hand_built():
    """RacecarSimulator.raceSeatsMany and raceEnv(seats=...) are race_seats and a seated RaceEnv on the simulator's
    method, car, fan, edge table, thresholds and own FollowGap driver ("fg")."""
    g = DC.race_maze()
    cfg = dict(RC.DEFAULT_CAR)
    cfg.update(scan_dist_to_base=D_BASE, batch_size=40, scan_beams=1080, scan_fov=FOV, scan_std=0.01,
               scan_max_range=15.0, free_thresh=0.8)
    sim = RacecarSimulator(cfg)
    omap = range_libc.PyOMap(g)
    sim.setMap(omap, g.resolution, g.origin)
    sim.setRaytracingMethod("RMGPU")
    layers, relu = PS.load_fixture(os.path.join(GOLD, "policy_mlp720.npz"))
    pol = Policy.from_arrays(layers, relu)
    R, P, T = 3, 3, 12
    states, _ = _race_starts(g, omap.distance_transform(), R, P, 52)
    got = sim.raceSeatsMany(states, T, ["fg", pol, "fg"], speed=3.0, steer_clip=0.4189)
    fg = sim._followgap
    want = sim.car.race_seats(sim.scan_simulator.scan_method, [fg, pol, fg], states, T, 3.0, FOV, 1080,
                              sim.edge_distances, cfg["ttc_thresh"], steer_clip=0.4189, scan_dist_to_base=D_BASE)
    assert len(got) == 4 and all(same_bits(x, y) for x, y in zip(got, want))
    assert got[3].shape == (R, P, T) and np.isfinite(got[3][:, :, 0]).all()
    kw = dict(obs_window=(180, 720, 1), obs_clip=15, obs_scale=15, min_running=2, steer_clip=0.4189)
    env = sim.raceEnv(R, states, seats=[None, "fg", pol], seat_speed=3.0, **kw)
    hand = RaceEnv(sim.scan_simulator.scan_method, states, R, 1080, FOV, sim.edge_distances, cfg["ttc_thresh"],
                   car=sim.car, scan_dist_to_base=D_BASE, seats=[None, fg, pol], seat_speed=3.0, **kw)
    assert env.obs_shape == (R * P, 720) and env.seats[1] is fg and env.seats[2] is pol
    assert same_bits(env.reset(seed=2), hand.reset(seed=2))
    for a in DC.actions(21, 4, R * P).reshape(4, R, P, 2):
        for x, y in zip(env.step(a), hand.step(a)):
            assert same_bits(x, y)
        assert same_bits(env.seat_steers(), hand.seat_steers())
