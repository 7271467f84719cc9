"""Track progress (rl_track_*, rl_env_attach_track, rl_env_read_track*, Track, DriveEnv / RaceEnv track_state) on the
MI355X, held to the statement (tests/track_statement.py): the statement is told the states and phases the env itself
reports and must then agree with the device — the int rows and the columns made of + - * / sqrt bit for bit, the two
that pass through cos, sin and atan2 to the last f32 rounding."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import support
import track_statement as TS
from conftest import GOLD
from support import FOV, THRESH, same_bits
from test_track_host import HAIRPIN, SQUARE
from pyracecarsimulator_amd import DriveEnv, RaceEnv, RacecarSimulator, Track, _lib, maps, range_libc
from pyracecarsimulator_amd import racecar as RC
from pyracecarsimulator_amd.track import track_env_args

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

N, B, T_STEPS, S_SUB = 70, 60, 12, 3              # past one 64-lane block and one 8-env workgroup
RL_ERR_INVALID = -1
EXACT = [0, 1, 2, 6, 7]                           # delta, s, lateral, progress, race_dist: + - * / sqrt only


@pytest.fixture(scope="module")
def rig():
    """A 13 m room around the waypoint file (x -4 .. 9, y -2 .. 11), RMGPU, one CarBatch, the outline table."""
    g = maps.make_room(260, resolution=0.05, origin=(-4.0, -2.0, 0.0))
    m = range_libc.PyRayMarchingGPU(range_libc.PyOMap(g), 300)
    return g, m, RC.CarBatch(), support.edge(B)


def track_points(name):
    if name == "wp36":
        return Track.read_csv(os.path.join(GOLD, "wp_u.csv"))
    if name == "ring150":                         # three rounds of 64 lanes, the last partial; uneven spacing
        a = np.sort(np.random.default_rng(150).uniform(0.0, 2 * math.pi, 150))
        return np.stack([2.5 + 4.6 * np.cos(a), 4.5 + 4.2 * np.sin(a)], -1)
    return np.array([(0.0, 1.0), (6.0, 1.0), (3.0, 7.0)])        # tri3


def at_arc(T, s, side=0.0):
    """(x, y, heading of the segment) at arc length s of the table T, `side` m to the left."""
    i = int(min(np.searchsorted(T["cum"], s, "right") - 1, T["S"] - 1))
    t = (s - T["cum"][i]) / T["len"][i]
    ux, uy = T["dx"][i] / T["len"][i], T["dy"][i] / T["len"][i]
    return T["x"][i] + t * T["dx"][i] - side * uy, T["y"][i] + t * T["dy"][i] + side * ux, math.atan2(uy, ux)


def cars_on(T, n, seed):
    """(starts (n, 11), actions (T_STEPS, n, 2)) by e mod 5: 0 forward somewhere on the track; 1 forward from just
    behind the start line; 2 in reverse from just ahead of it; 3 anywhere in the room; 4 as 0 with NaN actions later."""
    rng = np.random.default_rng(seed)
    st = np.zeros((n, 11))
    act = np.zeros((T_STEPS, n, 2), np.float32)
    act[:, :, 1] = rng.uniform(-0.3, 0.3, (T_STEPS, n))
    for e in range(n):
        kind = e % 5
        if kind == 3:
            st[e, :4] = (rng.uniform(-3, 8), rng.uniform(-1, 10), rng.uniform(-math.pi, math.pi), 2.0)
            act[:, e, 0] = 6.0
            continue
        s = {1: T["L"] - rng.uniform(0.05, 0.3), 2: rng.uniform(0.05, 0.3)}.get(kind, T["L"] * (e + 0.37) / n)
        v = -3.0 if kind == 2 else 3.0
        st[e, :3] = at_arc(T, s, rng.uniform(-0.2, 0.2))
        st[e, 2] += rng.uniform(-0.2, 0.2)
        st[e, 3] = v
        act[:, e, 0] = v
        if kind == 4:
            act[3 + e % 4, e, e % 2] = np.nan
    return st, act


def assert_rows(ts, stmt, what):
    """The device's track_state against the statement after the same call."""
    rows, ints = np.asarray(ts["rows"]).reshape(-1, 8), np.stack([np.asarray(ts[k]).reshape(-1) for k in
                                                                  ("segment", "goal", "laps", "rank")], -1)
    want = stmt.rows
    assert same_bits(ints.astype(np.int32), stmt.ints), (what, np.nonzero((ints != stmt.ints).any(1))[0][:8])
    assert same_bits(rows[:, EXACT], want[:, EXACT]), (what, np.nonzero((rows[:, EXACT] != want[:, EXACT]).any(1))[0][:8])
    assert (np.abs(rows[:, 3].astype(np.float64) - stmt.rows64[:, 3]) <= 2.0 ** -22).all(), what
    tol = 2.0 ** -23 * np.maximum(1.0, stmt.goal_dist)
    for c in (4, 5):
        assert (np.abs(rows[:, c].astype(np.float64) - stmt.rows64[:, c]) <= tol).all(), (what, c)


CASES = [("wp36", True, 0, 0, True), ("wp36", True, 4, 10, False), ("wp36", False, 4, 0, True),
         ("ring150", True, 0, 10, False), ("ring150", True, 4, 0, True), ("ring150", False, 4, 10, True),
         ("tri3", True, 4, 0, True), ("tri3", True, 0, 10, False)]


@pytest.mark.parametrize("name,closed,window,span,auto", CASES)
def test_drive_env_track_state_equals_the_statement(rig, name, closed, window, span, auto):
    """70 envs x 12 steps of 3 substeps on W = 36 / 150 / 3, closed and open, window 0 / 4, goal_span 0 / 10,
    auto_reset on (max_ticks 5: everything re-spawns mid-run) and off: cars drive forward, forward and in reverse across
    the start line, anywhere in the room, and some are handed a NaN.  After the reset and after every step the device's
    rows equal the statement's, and the track changes nothing else: obs, reward and done equal a twin without one."""
    g, m, cars, edge = rig
    xy = track_points(name)
    T = TS.build(xy, closed)
    starts, actions = cars_on(T, N, 7)
    trk = Track(xy, closed)
    assert trk.length == T["L"] and same_bits(trk.cum, T["cum"])
    m.set_noise(0.05, 99, 5 * N * B + 1)
    kw = dict(substeps=S_SUB, max_ticks=5 if auto else 0, auto_reset=auto, crash_reward=-1.0, car=cars)
    env = DriveEnv(m, starts, N, B, FOV, edge, THRESH, track=trk, track_window=window, goal_span=span, lookahead=1.5, **kw)
    twin = DriveEnv(m, starts, N, B, FOV, edge, THRESH, **kw)
    stmt = TS.TrackEnv(T, N, window, 1.5, span)
    obs, obs2 = env.reset(seed=4, start_index=np.arange(N)), twin.reset(seed=4, start_index=np.arange(N))
    assert same_bits(obs, obs2)
    rd = env.read()
    stmt.call(rd["states"], TS.phases_drive(rd["done"], None, auto, reset=True))
    assert_rows(env.track_state(), stmt, "reset")
    seen = set()
    laps_lo = laps_hi = 0
    for k in range(T_STEPS):
        ph = TS.phases_drive(rd["done"], actions[k], auto)
        out, out2 = env.step(actions[k]), twin.step(actions[k])
        for a, b in zip(out, out2):
            assert same_bits(a, b), k
        rd = env.read()
        stmt.call(rd["states"], ph)
        ts = env.track_state()
        assert_rows(ts, stmt, k)
        assert (ts["rank"] == 0).all() and (ts["rows"][:, 7] == ts["rows"][:, 6]).all()      # a DriveEnv: offset 0
        seen |= set(ph.tolist())
        laps_lo, laps_hi = min(laps_lo, int(ts["laps"].min())), max(laps_hi, int(ts["laps"].max()))
    assert {TS.STEPPED, TS.INVALID, TS.FRESH if auto else TS.FROZEN} <= seen, seen
    assert (laps_lo, laps_hi) == ((-1, 1) if closed else (0, 0))
    assert (stmt.ints[:, 1] >= 0).any()
    m.set_noise(0.0, 0, 0)


def test_progress_reward_pays_delta_where_the_env_pays_moved(rig):
    """reward_mode 1 against a twin with reward_mode 0: (float)D exactly where the twin reads (float)moved (a stepped
    env that did not crash), the twin's reward everywhere else; obs and done agree throughout."""
    g, m, cars, edge = rig
    xy = track_points("wp36")
    T = TS.build(xy, True)
    starts, actions = cars_on(T, N, 9)
    trk = Track(xy)
    kw = dict(substeps=S_SUB, max_ticks=5, auto_reset=True, crash_reward=-2.5, car=cars, track=trk, track_window=4)
    env = DriveEnv(m, starts, N, B, FOV, edge, THRESH, progress_reward=True, **kw)
    twin = DriveEnv(m, starts, N, B, FOV, edge, THRESH, **kw)
    assert same_bits(env.reset(seed=1), twin.reset(seed=1))
    paid = differs = 0
    for k in range(T_STEPS):
        done_before = twin.read()["done"]
        ph = TS.phases_drive(done_before, actions[k], True)
        (o1, r1, d1), (o2, r2, d2) = env.step(actions[k]), twin.step(actions[k])
        assert same_bits(o1, o2) and same_bits(d1, d2), k
        ts, ts2 = env.track_state(), twin.track_state()
        assert same_bits(ts["rows"], ts2["rows"]), k
        moved = (ph == TS.STEPPED) & (d2 != 1)
        assert same_bits(r1[moved], ts["rows"][moved, 0]), k
        assert same_bits(r1[~moved], r2[~moved]), k
        paid += int(moved.sum())
        differs += int((r1[moved] != r2[moved]).sum())
    assert paid > 0 and differs > 0


def race_lineups(T):
    """5 line-ups of 3 cars on the waypoint track, 1.2 m apart along it; race 0's car 2 and two cars of race 1 instead
    drive into the east wall (x = 9) at 7 m/s."""
    st = np.zeros((5, 3, 11))
    for r in range(5):
        for k in range(3):
            s = (T["L"] - 0.5 + 7.0 * r + 1.2 * k) % T["L"]               # race 0 straddles the start line
            st[r, k, :3] = at_arc(T, s, 0.25 * (k - 1))
            st[r, k, 3] = 3.0
    st[0, 2, :4] = (8.2, 9.5, 0.0, 7.0)
    st[1, 0, :4] = (8.2, 0.5, 0.0, 7.0)
    st[1, 2, :4] = (8.0, -1.0, 0.0, 7.0)
    return st


def test_race_env_offsets_and_ranks_through_a_crash_an_end_and_a_respawn(rig):
    """R = 5, P = 3, min_running 2, auto_reset: race 0 loses a car to the wall and goes on (the wreck stays ranked),
    race 1 loses two, ends by attrition and re-spawns as a whole.  Every call equals the statement."""
    g, m, cars, edge = rig
    xy = track_points("wp36")
    T = TS.build(xy, True)
    R, P = 5, 3
    st = race_lineups(T)
    trk = Track(xy)
    env = RaceEnv(m, st, R, B, FOV, edge, THRESH, min_running=2, substeps=S_SUB, auto_reset=True, car=cars, track=trk,
                  track_window=4, goal_span=10)
    stmt = TS.TrackEnv(T, R * P, 4, 1.5, 10, group=P)
    env.reset(seed=2, start_index=np.arange(R))
    rd = env.read()
    stmt.call(rd["states"].reshape(-1, 11), TS.phases_race(None, rd["done"].reshape(-1), None, True, P, reset=True))
    ts = env.track_state()
    assert ts["rows"].shape == (R, P, 8) and ts["rank"].shape == (R, P)
    assert_rows(ts, stmt, "reset")
    assert (ts["rows"][:, 0, 7] == 0).all() and (np.sort(ts["rank"], 1) == np.arange(P)).all()
    assert 1.0 < ts["rows"][0, 1, 7] < 1.4                      # car 1 starts across the line: 1.2 m ahead, not L behind
    actions = np.zeros((T_STEPS, R, P, 2), np.float32)
    actions[..., 0] = 3.0
    actions[:, 0, 2, 0] = actions[:, 1, 0, 0] = actions[:, 1, 2, 0] = 7.0
    wreck_ranked = ended = respawned = lapped = False
    for k in range(T_STEPS):
        over, done = rd["race_over"], rd["done"].reshape(-1)
        ph = TS.phases_race(over, done, actions[k], True, P)
        env.step(actions[k])
        rd = env.read()
        stmt.call(rd["states"].reshape(-1, 11), ph)
        ts = env.track_state()
        assert_rows(ts, stmt, k)
        assert (np.sort(ts["rank"], 1) == np.arange(P)).all(), k
        wreck_ranked |= bool(over[0] == 0 and done[2] == 1 and ph[2] == TS.FROZEN)
        ended |= bool(rd["race_over"][1] == 1)
        respawned |= bool(ended and ph[3] == TS.FRESH)
        lapped |= bool(ts["laps"][0, 0] == 1)
    assert wreck_ranked and ended and respawned and lapped


def test_device_form_detach_and_refusals(rig):
    """The device form's rows equal the host form's; every refusal of rl_env_attach_track / rl_env_read_track leaves the
    env as a twin that never saw it; a detached env after a reset is an env that never had a track."""
    import torch
    g, m, cars, edge = rig
    xy = track_points("ring150")
    T = TS.build(xy, True)
    starts, actions = cars_on(T, N, 11)
    trk = Track(xy)
    kw = dict(substeps=S_SUB, max_ticks=5, auto_reset=True, car=cars)
    tkw = dict(track=trk, track_window=4, goal_span=10, progress_reward=True)
    env = DriveEnv(m, starts, N, B, FOV, edge, THRESH, **kw, **tkw)
    twin = DriveEnv(m, starts, N, B, FOV, edge, THRESH, **kw, **tkw)
    plain = DriveEnv(m, starts, N, B, FOV, edge, THRESH, **kw)
    L = _lib.lib()
    for e, name in ((env, "reset"), (plain, "no track attached")):
        with pytest.raises(_lib.ScanLibError, match=name):
            e.track_state()
    idx = np.arange(N, dtype=np.int32)
    env.reset(seed=6, start_index=torch.from_numpy(idx).cuda())
    twin.reset(seed=6, start_index=idx)
    opts = dict(track_window=4, goal_span=10, progress_reward=True)
    good = track_env_args(**opts)
    refused = []
    for field, value in (("window", -1), ("window", 65537), ("goal_span", -1), ("goal_span", 65537), ("reward_mode", 2),
                         ("reward_mode", -1), ("lookahead", 0.0), ("lookahead", -1.0), ("lookahead", math.inf),
                         ("lookahead", math.nan)):
        p = track_env_args(**opts)
        setattr(p, field, value)
        refused.append(L.rl_env_attach_track(env._h, trk._h, C.byref(p)))
    refused.append(L.rl_env_attach_track(env._h, trk._h, None))
    if L.rl_device_count() > 1:
        refused.append(L.rl_env_attach_track(env._h, Track(xy, device=1)._h, C.byref(good)))
    assert refused == [RL_ERR_INVALID] * len(refused)
    assert L.rl_env_read_track(plain._h, None, None) == RL_ERR_INVALID
    for k in range(6):
        a = torch.from_numpy(actions[k]).cuda()
        o, r, d = env.step(a)
        o2, r2, d2 = twin.step(actions[k])
        ts, ts2 = env.track_state(on_device=True), twin.track_state()
        assert same_bits(o.cpu().numpy(), o2) and same_bits(r.cpu().numpy(), r2) and same_bits(d.cpu().numpy(), d2), k
        for key in ts2:
            assert same_bits(ts[key].cpu().numpy(), ts2[key]), (k, key)
        host = env.track_state()                                 # the host form after device-form calls
        assert same_bits(host["rows"], ts2["rows"]) and same_bits(host["laps"], ts2["laps"]), k
    # detach: a reset is needed, and then the env is `plain`
    env.attach_track(None)
    with pytest.raises(_lib.ScanLibError):
        env.step(actions[0])
    assert same_bits(env.reset(seed=8), plain.reset(seed=8))
    for k in range(7):
        for a, b in zip(env.step(actions[k]), plain.step(actions[k])):
            assert same_bits(a, b), k
    with pytest.raises(_lib.ScanLibError, match="no track attached"):
        env.track_state()
    # and back on: the new track's rows start at the reset
    env.attach_track(trk, track_window=0)
    env.reset(seed=8)
    stmt = TS.TrackEnv(T, N)
    stmt.call(env.read()["states"], np.full(N, TS.FRESH))
    assert_rows(env.track_state(), stmt, "re-attached")


def test_hairpin_and_ties_on_the_device(rig):
    """The host test's known answers on the device.  Ties: on the unit square a car on the bisector outside corner
    (1, 0) takes segment 0, one outside corner (0, 0) takes 0 over 3, one at the centre takes segment 0 and goal 0, one
    far outside corner (1, 1) takes 1 over 2 and has no goal.
    Hairpin: a car on the outward leg drifts towards the returning one; window 0 jumps to segment 8, window 3 stays."""
    g, m, cars, edge = rig
    sq = np.zeros((4, 11))
    sq[:, :2] = ((1.5, -0.5), (-0.5, -0.5), (0.5, 0.5), (8.0, 10.0))
    env = DriveEnv(m, sq, 4, B, FOV, edge, THRESH, car=cars, track=Track(SQUARE), lookahead=1.5)
    env.reset(start_index=np.arange(4))
    ts = env.track_state()
    assert ts["segment"].tolist() == [0, 0, 0, 1] and ts["goal"].tolist() == [0, 1, 0, -1]
    assert ts["rows"][:, 1].tolist() == [1.0, 0.0, 0.5, 2.0] and ts["rows"][:, 2].tolist() == [-0.5, -0.5, 0.5, -7.0]
    assert ts["rows"][3, 4:6].tolist() == [0.0, 0.0]
    stmt = TS.TrackEnv(TS.build(SQUARE, True), 4)
    stmt.call(sq, np.full(4, TS.FRESH))
    assert_rows(ts, stmt, "square")
    hp = np.zeros((2, 11))
    hp[:, :4] = (1.5, 0.05, math.atan2(0.1, 1.0), 1.0)
    act = np.array([[1.0, 0.0]] * 2, np.float32)
    T = TS.build(HAIRPIN, True)
    got = {}
    for window in (0, 3):
        env = DriveEnv(m, hp, 2, B, FOV, edge, THRESH, substeps=100, car=cars, track=Track(HAIRPIN), track_window=window)
        env.reset(start_index=np.zeros(2, np.int32))
        stmt = TS.TrackEnv(T, 2, window)
        stmt.call(env.read()["states"], np.full(2, TS.FRESH))
        assert env.track_state()["segment"].tolist() == [1, 1]
        env.step(act)
        x, y = env.read()["states"][0, :2]
        assert 2.2 < x < 2.8 and 0.11 < y < 0.19, (x, y)
        stmt.call(env.read()["states"], np.full(2, TS.STEPPED))
        assert_rows(env.track_state(), stmt, window)
        got[window] = env.track_state()["segment"].tolist()
    assert got == {0: [8, 8], 3: [2, 2]}


def test_simulator_passes_the_track_keywords_through(rig):
    g, m, cars, edge = rig
    cfg = dict(RC.DEFAULT_CAR)
    cfg.update(scan_dist_to_base=0.275, batch_size=8, scan_beams=B, scan_fov=4.71, scan_std=0.0, scan_max_range=15.0,
               free_thresh=0.8)
    sim = RacecarSimulator(cfg)
    sim.setMap(range_libc.PyOMap(g), g.resolution, g.origin)
    sim.setRaytracingMethod("RMGPU")
    trk = Track(track_points("tri3"))
    st = np.zeros((4, 11))
    st[:, :2] = ((1.0, 1.2), (3.0, 1.2), (5.0, 1.2), (3.0, 5.0))
    env = sim.driveEnv(4, st, track=trk, lookahead=2.0, goal_span=2, progress_reward=True)
    env.reset(start_index=np.arange(4))
    assert env.track_state()["segment"].tolist()[:3] == [0, 0, 0]
    race = sim.raceEnv(2, st.reshape(2, 2, 11), track=trk, track_window=1)
    race.reset(start_index=np.arange(2))
    assert race.track_state()["rank"].shape == (2, 2)
