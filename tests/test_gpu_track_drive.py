"""Track progress of the closed-loop roll-outs (include/scanlib_track_drive.h: rl_car_attach_track, rl_car_read_track,
rl_car_read_track_scores; CarBatch.attach_track / track_state / track_scores; the RacecarSimulator façades) on the MI355X.
The oracle is the call's own states_trace and first_crashed fed to the statement (tests/track_drive_statement.py): those
outputs are pinned to the reference Car and the scan oracle elsewhere.  Every column compares bit for bit, rows and ints:
the rule is + - * / sqrt fmin fmax in f64 without contraction.

Shapes: test_gpu_track.py's room and tracks (tri3, wp36, ring150: three 64-lane rounds of candidates, the last partial);
70 cars (8 full workgroups of 8 waves and one of 6), 72 in the races; 60 beams; 20 ticks of 0.02 s."""
import ctypes as C
import math

import numpy as np
import pytest

import league_statement as LS
import support
import test_gpu_population as TP
import track_drive_statement as DS
import track_statement as TS
from support import D_BASE, FOV, THRESH, same_bits
from test_gpu_track import at_arc, track_points
from pyracecarsimulator_amd import RacecarSimulator, Track, _lib, maps, range_libc
from pyracecarsimulator_amd import racecar as RC

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

N, B, TICKS, DT = 70, 60, 20, 0.02
CLIP = 0.2
RL_ERR_INVALID = -1
N_POP, E_POP = 5, 14                              # 5 members x 14 cars = N
#: (track, closed, window, goal_dist): every track closed and open, window 0 and 4, goal 1.0 and 0 (= L)
CASES = [("wp36", True, 0, 1.0), ("wp36", True, 4, 0.0), ("wp36", False, 4, 1.0), ("ring150", True, 4, 1.0),
         ("ring150", True, 0, 0.0), ("ring150", False, 4, 1.0), ("tri3", True, 4, 1.0), ("tri3", True, 0, 0.0)]
SEED = 7                                          # of the starts (docs/history/track_drive.md: the seeds tried)


@pytest.fixture(scope="module")
def rig():
    """test_gpu_track.py's 13 m room (x -4 .. 9, y -2 .. 11), RMGPU, one CarBatch, FollowGap, the small population."""
    g = maps.make_room(260, resolution=0.05, origin=(-4.0, -2.0, 0.0))
    m = range_libc.PyRayMarchingGPU(range_libc.PyOMap(g), 300)
    pop, thetas, relu = TP.make_pop("small", N_POP, 1, 4.0)
    return dict(g=g, m=m, cars=RC.CarBatch(), edge=support.edge(B), fg=support.followgap(), pop=pop, pol=pop.member(2))


def lone_starts(T, n, seed):
    """(states (n, 11), speeds (n,), steer0 (n,)) by r mod 5: 0 forward somewhere on the track, slow and fast; 1 forward
    from just behind the start line; 2 in reverse from just ahead of it; 3 anywhere in the room; 4 at a wall, into it."""
    rng = np.random.default_rng(seed)
    st, sp = np.zeros((n, 11)), np.zeros(n)
    for r in range(n):
        kind = r % 5
        if kind == 3:
            sp[r] = 3.0
            st[r, :4] = (rng.uniform(-3, 8), rng.uniform(-1, 10), rng.uniform(-math.pi, math.pi), sp[r])
        elif kind == 4:
            sp[r] = 5.0
            st[r, :4] = (9.0 - rng.uniform(0.6, 1.6), rng.uniform(0.0, 9.0), rng.uniform(-0.1, 0.1), sp[r])
        else:
            s = {1: T["L"] - rng.uniform(0.05, 0.3), 2: rng.uniform(0.05, 0.3)}.get(kind, T["L"] * (r + 0.37) / n)
            sp[r] = {1: 4.0, 2: -3.0}.get(kind, rng.uniform(1.0, 5.5))
            st[r, :3] = at_arc(T, s, rng.uniform(-0.2, 0.2))
            st[r, 2] += rng.uniform(-0.2, 0.2)
            st[r, 3] = sp[r]
    return st, sp, rng.uniform(-0.2, 0.2, n).astype(np.float32)


def race_starts(T, n_races, P, seed):
    """(states (n_races, P, 11), speeds, steer0 (n_races, P)): the cars of a race in a file along the track, car k ahead
    of car k - 1, race 0 across the start line of a closed track.  In every third race car 1 is fast and car 2 crawls a
    car's length or so ahead of it (car 1 wrecks, ahead of car 0, which runs on).  The last two cars of the last race are
    one and the same car twice: whatever becomes of them, they tie."""
    rng = np.random.default_rng(seed)
    L = T["L"]
    st, sp = np.zeros((n_races, P, 11)), np.zeros((n_races, P))
    span = 0.9 * (P - 1) + 1.5
    for i in range(n_races):
        base = L - 1.0 if i == 0 and T["closed"] else (L - span) * (i + 0.5) / n_races
        at = base + 0.9 * np.arange(P)
        sp[i] = rng.uniform(1.0, 4.5, P)
        if i % 3 == 0 and P >= 3:
            at[2] = at[1] + (0.55, 0.7, 0.85, 1.0)[(i // 3) % 4]
            at[3:] += 1.5
            sp[i, :3] = (1.0, 6.0, 0.3)
        for k in range(P):
            s = at[k] % L if T["closed"] else at[k]
            st[i, k, :3] = at_arc(T, s, 0.12 * (-1) ** k)
            st[i, k, 3] = sp[i, k]
    st0 = rng.uniform(-0.1, 0.1, (n_races, P)).astype(np.float32)
    if P >= 2:
        st[-1, P - 1], sp[-1, P - 1], st0[-1, P - 1] = st[-1, P - 2], sp[-1, P - 2], st0[-1, P - 2]
    return st, sp, st0


def check_state(cars, res, T, st0, window, goal, group=0):
    """track_state() of the call that gave `res` against the statement on res's own trace and crash ticks; returns
    (statement rows, first_crashed flat)."""
    first, trace = np.asarray(res[0]).reshape(-1), np.asarray(res[5]).reshape(-1, TICKS, 11)
    for r in range(len(first)):                   # the placements are the trace rows that are not NaN
        live = np.zeros(TICKS, bool)
        live[list(DS.reached(first[r], TICKS))] = True
        assert (np.isnan(trace[r]).all(1) == ~live).all() and np.isfinite(trace[r][live]).all(), r
    pl = DS.placements(T, np.asarray(st0).reshape(-1, 11), trace, first, TICKS, window, goal, group)
    ts = cars.track_state()
    assert list(ts) == list(DS.KEYS)
    for k in DS.KEYS:
        assert ts[k].shape == np.asarray(res[0]).shape, k
        got = ts[k].reshape(-1)
        assert same_bits(got, pl[k]), (k, np.nonzero(got != pl[k])[0][:8], got[got != pl[k]][:4], pl[k][got != pl[k]][:4])
    return pl, first


def census(pl, first, T, window, goal):
    """What a case must hold so that it cannot pass hollow."""
    S = T["S"]
    if T["closed"]:
        assert (pl["laps"] == 1).any() and (pl["laps"] == -1).any(), np.unique(pl["laps"])
    else:
        assert not pl["laps"].any()
    assert ((first >= 0) & (first < TICKS - 1)).any()              # frozen before the last tick: its progress stopped
    assert (first < 0).any() and (pl["progress"] > 0.3).any() and (pl["progress"] < -0.04).any()
    if goal:
        assert (pl["goal_tick"] >= 0).any() and (pl["goal_tick"] < 0).any()
        assert (pl["goal_tick"] > 0).any()                         # ... and not all at once
    else:
        assert (pl["goal_tick"] == -1).all() and pl["progress"].max() < T["L"]      # one length in 0.4 s: nobody
    if window and 2 * window + 1 < S:
        a, b = pl["trail"][:, :-1], pl["trail"][:, 1:]
        hop = np.where((a >= 0) & (b >= 0), np.abs(b - a), 0)
        hop = np.minimum(hop, S - hop) if T["closed"] else hop
        assert ((hop > 0) & (hop <= window)).any() and hop.max() <= window


# ---------------------------------------------------------------- 1. every source
@pytest.mark.parametrize("name,closed,window,goal", CASES)
def test_every_source_equals_the_statement(rig, name, closed, window, goal):
    """drive_followgap, drive_policy and drive_population (5 x 14) on 70 cars: forward, across the start line both ways,
    anywhere in the room and into a wall.  Rows and ints equal the statement; the population's track scores equal
    track_fitness; each call passes its own census."""
    m, cars, edge = rig["m"], rig["cars"], rig["edge"]
    xy = track_points(name)
    T = TS.build(xy, closed)
    trk = Track(xy, closed)
    st, sp, st0 = lone_starts(T, N, SEED)
    cars.attach_track(trk, window, goal or None)
    try:
        kw = dict(scan_dist_to_base=D_BASE, dt=DT, steer0=st0, trace=True)
        res = cars.drive_followgap(m, rig["fg"], st, TICKS, sp, FOV, B, edge, THRESH, **kw)
        census(*check_state(cars, res, T, st, window, goal), T, window, goal)
        with pytest.raises(_lib.ScanLibError):                     # FollowGap's call leaves no scores
            _lib.call("rl_car_read_track_scores", cars, N_POP, 3, np.empty((N_POP, 3)))
        res = cars.drive_policy(m, rig["pol"], st, TICKS, sp, FOV, B, edge, THRESH, steer_clip=CLIP, **kw)
        census(*check_state(cars, res, T, st, window, goal), T, window, goal)
        res = cars.drive_population(m, rig["pop"], st, TICKS, sp, FOV, B, edge, THRESH, E_POP, steer_clip=CLIP, **kw)
        pl, first = check_state(cars, res, T, st, window, goal)
        census(pl, first, T, window, goal)
        scores = cars.track_scores()
        assert scores.shape == (N_POP, 3) and same_bits(scores, DS.track_fitness(pl, N_POP, E_POP))
        assert TP.differ_pairwise(list(scores))
        assert (pl["rank"] == 0).all() and same_bits(pl["race_dist"], 0.0 + pl["progress"])
    finally:
        cars.detach_track()


# ---------------------------------------------------------------- 2. races
def wreck_ahead(pl, first, P):
    """A race with a wreck ranked ahead of a car that still runs."""
    rank, first = pl["rank"].reshape(-1, P), first.reshape(-1, P)
    return any(first[i, a] >= 0 > first[i, b] and rank[i, a] < rank[i, b]
               for i in range(len(rank)) for a in range(P) for b in range(P))


@pytest.mark.parametrize("source,n_races,P,name,closed,window,goal",
                         [("followgap", 18, 4, "wp36", True, 0, 1.0), ("seats", 18, 4, "ring150", True, 4, 1.0),
                          ("followgap", 9, 8, "ring150", True, 4, 0.0), ("seats", 24, 3, "wp36", False, 4, 1.0)])
def test_races_equal_the_statement(rig, source, n_races, P, name, closed, window, goal):
    """72 cars in races of 4, 8 and 3 (a race of 3 straddles a workgroup of 8 cars): offsets, race_dist and ranks
    included.  Race 0 of a closed track lines up across the start line, so its offsets wrap."""
    m, cars, edge = rig["m"], rig["cars"], rig["edge"]
    xy = track_points(name)
    T = TS.build(xy, closed)
    trk = Track(xy, closed)
    st, sp, st0 = race_starts(T, n_races, P, 11)
    cars.attach_track(trk, window, goal or None)
    try:
        kw = dict(scan_dist_to_base=D_BASE, dt=DT, steer0=st0, trace=True)
        if source == "followgap":
            res = cars.race_followgap(m, rig["fg"], st, TICKS, sp, FOV, B, edge, THRESH, **kw)
        else:
            drivers = [rig["fg"] if k % 2 == 0 else rig["pol"] for k in range(P)]
            res = cars.race_seats(m, drivers, st, TICKS, sp, FOV, B, edge, THRESH, steer_clip=CLIP, **kw)
        pl, first = check_state(cars, res, T, st, window, goal, P)
        assert wreck_ahead(pl, first, P)
        assert sorted(pl["rank"][:P].tolist()) == list(range(P))
        offset = pl["race_dist"] - pl["progress"]
        if closed:                                                 # race 0: the raw s0 differences pass half the length
            raw = pl["s0"][:P] - pl["s0"][0]
            assert (np.abs(raw) > 0.5 * T["L"]).any() and np.abs(offset[:P]).max() <= 0.5 * T["L"]
        assert (offset.reshape(-1, P)[:, 1:] > 0.3).all()          # every car spawns ahead of car 0 of its race
        tie = pl["race_dist"][-2:]                                 # the twins: an exact tie, the lower k ahead
        assert tie[0] == tie[1] and pl["rank"][-1] == pl["rank"][-2] + 1
        with pytest.raises(ValueError):                            # a race without members leaves no scores
            cars.track_scores()
        with pytest.raises(_lib.ScanLibError):
            _lib.call("rl_car_read_track_scores", cars, N_POP, 4, np.empty((N_POP, 4)))
    finally:
        cars.detach_track()


def test_goal_tick_at_equality(rig):
    """goal_dist set to the very progress a car has after tick 7: its goal_tick is 7, not 8 (>=, on the device)."""
    m, cars, edge = rig["m"], rig["cars"], rig["edge"]
    xy = track_points("wp36")
    T, trk = TS.build(xy, True), Track(xy, True)
    st, sp, st0 = lone_starts(T, N, SEED)
    kw = dict(scan_dist_to_base=D_BASE, dt=DT, steer0=st0, trace=True)
    cars.attach_track(trk, 0, None)
    try:
        short = cars.drive_followgap(m, rig["fg"], st, 8, sp, FOV, B, edge, THRESH, **kw)
        progress = cars.track_state()["progress"]
        r = int(np.argmax(np.where(short[0] < 0, progress, -np.inf)))          # the car that came furthest in 8 ticks
        goal = float(progress[r])
        assert goal > 0.5
        cars.attach_track(trk, 0, goal)
        res = cars.drive_followgap(m, rig["fg"], st, TICKS, sp, FOV, B, edge, THRESH, **kw)
        pl, _ = check_state(cars, res, T, st, 0, goal)
        assert same_bits(res[5][:, :8], short[5]) and pl["goal_tick"][r] == 7 and pl["progress"][r] >= goal
        assert (np.delete(pl["goal_tick"], r) != 7).any()
    finally:
        cars.detach_track()


def test_a_frozen_car_stops_searching(rig):
    """Head-on pairs across the middle of ring150, window 4: the car that crosses the middle has its nearest segment
    jump half way round, its window follows 4 segments a tick, and the crash freezes it on the way: its segment stays
    behind the nearest one for good (a frozen car placed again and again would walk on)."""
    m, cars, edge = rig["m"], rig["cars"], rig["edge"]
    xy = track_points("ring150")
    T, trk = TS.build(xy, True), Track(xy, True)
    n_races, P = 6, 2
    st, sp = np.zeros((n_races, P, 11)), np.full((n_races, P), 5.0)
    for i in range(n_races):
        x = 2.5 + 0.03 * i
        st[i, 0, :4] = (x, 4.5 - 0.25 - 0.05 * i, math.pi / 2, 5.0)            # northwards, through the middle
        st[i, 1, :4] = (x, 4.5 + 1.1 + 0.05 * i, -math.pi / 2, 5.0)            # southwards, at it
    cars.attach_track(trk, 4, 1.0)
    try:
        res = cars.race_followgap(m, rig["fg"], st, TICKS, sp, FOV, B, edge, THRESH, dt=DT, trace=True,
                                  scan_dist_to_base=D_BASE)
        pl, first = check_state(cars, res, T, st, 4, 1.0, P)
        final = res[1].reshape(-1, 11)
        behind = [r for r in range(n_races * P) if 0 <= first[r] < TICKS - 4
                  and pl["segment"][r] != TS.nearest(T, final[r, 0], final[r, 1])]
        assert behind, (first, pl["segment"])
    finally:
        cars.detach_track()


# ---------------------------------------------------------------- 3. league and population scores
def league_entries(n_races, P, members, seed):
    e = np.random.default_rng(seed).choice(np.asarray(members), (n_races, P))
    e[0], e[1, 0] = members[0], -1                                 # one member a whole race; FollowGap for sure
    return e


def test_league_scores_equal_the_statement(rig):
    """18 x 4, five members of which member 4 enters nothing, -1 entries mixed in: track_scores equals track_standings,
    track_state the statement, and standings_N4 of the same call what it was."""
    m, cars, edge, pop = rig["m"], rig["cars"], rig["edge"], rig["pop"]
    xy = track_points("wp36")
    T, trk = TS.build(xy, True), Track(xy, True)
    n_races, P = 18, 4
    st, sp, st0 = race_starts(T, n_races, P, 11)
    entries = league_entries(n_races, P, [0, 1, 2, 3, -1], 3)
    assert not (entries == 4).any() and (entries == -1).any() and all((entries == k).any() for k in range(4))
    cars.attach_track(trk, 4, 1.0)
    try:
        res = cars.race_league(m, pop, entries, st, TICKS, sp, FOV, B, edge, THRESH, followgap=rig["fg"], steer_clip=CLIP,
                               steer0=st0, dt=DT, trace=True, scan_dist_to_base=D_BASE)
        pl, first = check_state(cars, res, T, st, 4, 1.0, P)
        scores = cars.track_scores()
        want = DS.track_standings(pl, entries, N_POP, P)
        assert scores.shape == (N_POP, 4) and same_bits(scores, want)
        assert not scores[4].any() and scores[:4, 0].sum() == (entries >= 0).sum() and scores[:, 3].sum() > 0
        assert (scores[:4, 2] > 0).any() and wreck_ahead(pl, first, P)
        assert same_bits(res[6], LS.standings(st, res[1], res[0], entries, N_POP, P, TICKS))
    finally:
        cars.detach_track()


def test_scores_past_one_block_of_members(rig):
    """70 members (24 -> 1): the one-lane-per-member score kernels reach a second workgroup, in a league where three of
    them enter and in a population of 70 x 1 cars."""
    m, cars, edge = rig["m"], rig["cars"], rig["edge"]
    big, thetas, _ = TP.make_pop("single", 70, gain=0.02)
    xy = track_points("ring150")
    T, trk = TS.build(xy, True), Track(xy, True)
    n_races, P = 18, 4
    st, sp, st0 = race_starts(T, n_races, P, 11)
    entries = league_entries(n_races, P, [5, 64, 69, -1], 4)
    cars.attach_track(trk, 0, 0.5)
    try:
        res = cars.race_league(m, big, entries, st, TICKS, sp, FOV, B, edge, THRESH, followgap=rig["fg"], steer_clip=CLIP,
                               steer0=st0, dt=DT, trace=True, scan_dist_to_base=D_BASE)
        pl, _ = check_state(cars, res, T, st, 0, 0.5, P)
        scores = cars.track_scores()
        assert scores.shape == (70, 4) and same_bits(scores, DS.track_standings(pl, entries, 70, P))
        assert scores[[5, 64, 69], 0].all() and not np.delete(scores, [5, 64, 69], 0).any() and scores[:, 3].sum() > 0
        st1, sp1, st01 = lone_starts(T, 70, SEED)
        res = cars.drive_population(m, big, st1, TICKS, sp1, FOV, B, edge, THRESH, 1, steer_clip=CLIP, steer0=st01, dt=DT,
                                    trace=True, scan_dist_to_base=D_BASE)
        pl, _ = check_state(cars, res, T, st1, 0, 0.5)
        fit = cars.track_scores()
        assert fit.shape == (70, 3) and same_bits(fit, DS.track_fitness(pl, 70, 1))
        assert same_bits(fit[:, 0], 0.0 + pl["progress"]) and fit[64:, 1].any() and fit[64:, 2].any()
    finally:
        cars.detach_track()


# ---------------------------------------------------------------- 4. the track changes nothing else
def _six_calls(rig, T):
    """One call per source, each a function of nothing that returns the call's whole result."""
    m, cars, edge, pop, fg, pol = (rig[k] for k in ("m", "cars", "edge", "pop", "fg", "pol"))
    st, sp, st0 = lone_starts(T, N, SEED)
    rs, rsp, rs0 = race_starts(T, 18, 4, 11)
    entries = league_entries(18, 4, [0, 1, 2, 3, -1], 3)
    lone = dict(scan_dist_to_base=D_BASE, dt=DT, steer0=st0, trace=True)
    race = dict(scan_dist_to_base=D_BASE, dt=DT, steer0=rs0, trace=True)
    return {
        "drive_followgap": lambda: cars.drive_followgap(m, fg, st, TICKS, sp, FOV, B, edge, THRESH, **lone),
        "drive_policy": lambda: cars.drive_policy(m, pol, st, TICKS, sp, FOV, B, edge, THRESH, steer_clip=CLIP, **lone),
        "drive_population": lambda: cars.drive_population(m, pop, st, TICKS, sp, FOV, B, edge, THRESH, E_POP,
                                                          steer_clip=CLIP, **lone),
        "race_followgap": lambda: cars.race_followgap(m, fg, rs, TICKS, rsp, FOV, B, edge, THRESH, **race),
        "race_seats": lambda: cars.race_seats(m, [fg, pol, pol, fg], rs, TICKS, rsp, FOV, B, edge, THRESH, steer_clip=CLIP,
                                              **race),
        "race_league": lambda: cars.race_league(m, pop, entries, rs, TICKS, rsp, FOV, B, edge, THRESH, followgap=fg,
                                                steer_clip=CLIP, **race),
    }


@pytest.mark.parametrize("source", ["drive_followgap", "drive_policy", "drive_population", "race_followgap", "race_seats",
                                    "race_league"])
def test_the_track_changes_nothing_else(rig, source):
    """first, final, vel, steers, the traces and fitness / standings: bit-equal without a track, with one, and after
    detach_track(); scan noise on, so that the noise offsets are in the comparison."""
    xy = track_points("wp36")
    T, trk = TS.build(xy, True), Track(xy, True)
    call = _six_calls(rig, T)[source]
    cars, m = rig["cars"], rig["m"]
    m.set_noise(0.02, 3, 777)
    try:
        before = call()
        cars.attach_track(trk, 4, 1.0)
        with_track = call()
        assert np.isfinite(cars.track_state()["progress"]).all()
        cars.detach_track()
        after = call()
    finally:
        cars.detach_track()
        m.set_noise(0.0, 0, 0)
    assert len(before) == len(with_track) == len(after) == (7 if source in ("drive_population", "race_league") else 6)
    for i, (a, b, c) in enumerate(zip(before, with_track, after)):
        assert same_bits(a, b) and same_bits(a, c), (source, i)
    with pytest.raises(ValueError):
        cars.track_state()                                         # detached: nothing to read


# ---------------------------------------------------------------- 5. identities
def test_races_of_one_equal_the_population_and_all_followgap_entries_the_followgap_race(rig):
    m, cars, edge, pop, fg = rig["m"], rig["cars"], rig["edge"], rig["pop"], rig["fg"]
    xy = track_points("ring150")
    T, trk = TS.build(xy, True), Track(xy, True)
    st, sp, st0 = lone_starts(T, N, SEED)
    cars.attach_track(trk, 4, 1.0)
    try:
        kw = dict(steer_clip=CLIP, steer0=st0, dt=DT, scan_dist_to_base=D_BASE)
        cars.drive_population(m, pop, st, TICKS, sp, FOV, B, edge, THRESH, E_POP, **kw)
        lone, fit = cars.track_state(), cars.track_scores()
        entries = (np.arange(N) // E_POP).reshape(N, 1)
        cars.race_league(m, pop, entries, st.reshape(N, 1, 11), TICKS, sp.reshape(N, 1), FOV, B, edge, THRESH,
                         steer_clip=CLIP, steer0=st0.reshape(N, 1), dt=DT, scan_dist_to_base=D_BASE)
        ones, stand = cars.track_state(), cars.track_scores()
        for k in DS.KEYS:
            assert same_bits(ones[k].reshape(-1), lone[k]), k
        assert same_bits(stand[:, 1], fit[:, 0]) and same_bits(stand[:, 2], fit[:, 1]) and (stand[:, 0] == E_POP).all()
        rs, rsp, rs0 = race_starts(T, 18, 4, 11)
        race = dict(steer0=rs0, dt=DT, scan_dist_to_base=D_BASE)
        cars.race_followgap(m, fg, rs, TICKS, rsp, FOV, B, edge, THRESH, **race)
        want = cars.track_state()
        cars.race_league(m, pop, np.full((18, 4), -1), rs, TICKS, rsp, FOV, B, edge, THRESH, followgap=fg, **race)
        got = cars.track_state()
        for k in DS.KEYS:
            assert same_bits(got[k], want[k]), k
        assert not cars.track_scores().any()                       # nobody entered a car
    finally:
        cars.detach_track()


# ---------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_handles_usable(rig):
    m, cars, edge, pop, fg = rig["m"], rig["cars"], rig["edge"], rig["pop"], rig["fg"]
    L = _lib.lib()
    xy = track_points("tri3")
    T, trk = TS.build(xy, True), Track(xy, True)
    st, sp, st0 = lone_starts(T, N, SEED)
    kw = dict(scan_dist_to_base=D_BASE, dt=DT, steer0=st0, trace=True)
    f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rows, ints, sc = np.zeros((N, 4)), np.zeros((N, 4), np.intc), np.zeros((N_POP, 3))
    rp, ip, sp_ = rows.ctypes.data_as(f64p), ints.ctypes.data_as(i32p), sc.ctypes.data_as(f64p)

    def good():
        res = cars.drive_population(m, pop, st, TICKS, sp, FOV, B, edge, THRESH, E_POP, steer_clip=CLIP, **kw)
        pl, _ = check_state(cars, res, T, st, 4, 1.0)
        assert same_bits(cars.track_scores(), DS.track_fitness(pl, N_POP, E_POP))

    # no track attached: nothing to read
    assert L.rl_car_read_track(cars._h, N, rp, ip) == RL_ERR_INVALID and b"no track attached" in L.rl_last_error()
    assert L.rl_car_read_track_scores(cars._h, N_POP, 3, sp_) == RL_ERR_INVALID
    cars.attach_track(trk, 4, 1.0)
    try:
        # attached, and no tracked call yet
        assert L.rl_car_read_track(cars._h, N, rp, ip) == RL_ERR_INVALID and b"no roll-out" in L.rl_last_error()
        assert L.rl_car_read_track_scores(cars._h, N_POP, 3, sp_) == RL_ERR_INVALID
        good()
        # every attach the header refuses: what is attached stays attached, and its rows stay readable
        P = _lib.DriveTrackParams
        multi = RC.CarBatch(device=[0, 0])
        for handle, t, p in ((cars._h, trk._h, None), (cars._h, trk._h, C.byref(P(-1, 1.0))), (cars._h, trk._h, C.byref(P(65537, 1.0))),
                             (cars._h, trk._h, C.byref(P(0, -1.0))), (cars._h, trk._h, C.byref(P(0, math.nan))),
                             (cars._h, trk._h, C.byref(P(0, math.inf))), (multi._h, trk._h, C.byref(P(0, 1.0))),
                             (None, trk._h, C.byref(P(0, 1.0)))):
            assert L.rl_car_attach_track(handle, t, p) == RL_ERR_INVALID, (t, p)
        if _lib.call("rl_device_count") > 1:
            far = Track(xy, True, device=1)
            assert L.rl_car_attach_track(cars._h, far._h, C.byref(P(0, 1.0))) == RL_ERR_INVALID
            assert b"share one device" in L.rl_last_error()
        assert L.rl_car_read_track(cars._h, N, rp, ip) == 0 and L.rl_car_read_track_scores(cars._h, N_POP, 3, sp_) == 0
        good()
        # reads: the wrong number of cars, the wrong shape, a null pointer
        for n in (N - 1, N + 1, 0, -1):
            assert L.rl_car_read_track(cars._h, n, rp, ip) == RL_ERR_INVALID, n
        for shape in ((N_POP, 4), (N_POP - 1, 3), (N_POP, 2), (0, 0)):
            assert L.rl_car_read_track_scores(cars._h, shape[0], shape[1], sp_) == RL_ERR_INVALID, shape
        assert L.rl_car_read_track_scores(cars._h, N_POP, 3, None) == RL_ERR_INVALID
        assert L.rl_car_read_track(cars._h, N, None, None) == 0 and L.rl_car_read_track(cars._h, N, rp, None) == 0
        good()
        # scores after a call that leaves none; a roll-out that is refused keeps the last tracked call's rows
        res = cars.drive_followgap(m, fg, st, TICKS, sp, FOV, B, edge, THRESH, **kw)
        pl, _ = check_state(cars, res, T, st, 4, 1.0)
        assert L.rl_car_read_track_scores(cars._h, N_POP, 3, sp_) == RL_ERR_INVALID and b"no population" in L.rl_last_error()
        with pytest.raises(_lib.ScanLibError):
            cars.drive_followgap(m, fg, st, 0, sp, FOV, B, edge, THRESH, **dict(kw, trace=False))
        assert L.rl_car_read_track(cars._h, N, rp, ip) == 0 and same_bits(rows[:, 2], pl["progress"])
        good()
        # a new attachment forgets the old rows
        cars.attach_track(trk, 0, None)
        assert L.rl_car_read_track(cars._h, N, rp, ip) == RL_ERR_INVALID
    finally:
        cars.detach_track()
    assert L.rl_car_attach_track(cars._h, None, None) == 0          # detaching twice is fine


# ---------------------------------------------------------------- 7. the façades
def test_facades_attach_for_the_call_and_return_what_they_returned(rig):
    g = rig["g"]
    cfg = dict(RC.DEFAULT_CAR)
    cfg.update(scan_dist_to_base=D_BASE, batch_size=40, scan_beams=1080, scan_fov=FOV, scan_std=0.01, scan_max_range=15.0,
               free_thresh=0.8)
    sim = RacecarSimulator(cfg)
    omap = range_libc.PyOMap(g)
    sim.setMap(omap, g.resolution, g.origin)
    sim.setRaytracingMethod("RMGPU")
    pop, _, _ = TP.make_pop("fixture", 3)
    xy = track_points("wp36")
    T, trk = TS.build(xy, True), Track(xy, True)
    ticks = 12
    # a population: 3 members x 2 cars
    st, _, _ = lone_starts(T, 6, SEED)
    plain = sim.drivePopulationMany(st, ticks, pop, 2, speed=3.0, steer_clip=0.4189)
    got = sim.drivePopulationMany(st, ticks, pop, 2, speed=3.0, steer_clip=0.4189, track=trk, track_window=4, goal_dist=0.3)
    assert len(plain) == 5 and len(got) == 7 and sim.car._track is None
    for a, b in zip(plain, got):
        assert same_bits(a, b)
    sim.car.attach_track(trk, 4, 0.3)
    try:
        sim.car.drive_population(sim.scan_simulator.scan_method, pop, st, ticks, 3.0, FOV, 1080, sim.edge_distances,
                                 cfg["ttc_thresh"], 2, steer_clip=0.4189, scan_dist_to_base=D_BASE)
        state, scores = sim.car.track_state(), sim.car.track_scores()
    finally:
        sim.car.detach_track()
    assert list(got[5]) == list(DS.KEYS) and all(same_bits(got[5][k], state[k]) for k in DS.KEYS)
    assert same_bits(got[6], scores) and got[6].shape == (3, 3) and (got[5]["progress"] != 0).any()
    # a league: 3 races of 2
    rs, _, _ = race_starts(T, 3, 2, 11)
    entries = np.array([[0, 1], [1, -1], [2, 0]])
    plain = sim.raceLeagueMany(rs, ticks, pop, entries, speed=3.0, steer_clip=0.4189)
    got = sim.raceLeagueMany(rs, ticks, pop, entries, speed=3.0, steer_clip=0.4189, track=trk, goal_dist=0.3)
    assert len(plain) == 5 and len(got) == 7 and sim.car._track is None
    for a, b in zip(plain, got):
        assert same_bits(a, b)
    sim.car.attach_track(trk, 0, 0.3)
    try:
        sim.car.race_league(sim.scan_simulator.scan_method, pop, entries, rs, ticks, 3.0, FOV, 1080, sim.edge_distances,
                            cfg["ttc_thresh"], followgap=sim._followgap, steer_clip=0.4189, scan_dist_to_base=D_BASE)
        state, scores = sim.car.track_state(), sim.car.track_scores()
    finally:
        sim.car.detach_track()
    assert all(same_bits(got[5][k], state[k]) and got[5][k].shape == (3, 2) for k in DS.KEYS)
    assert same_bits(got[6], scores) and got[6].shape == (3, 4) and got[6][:, 0].tolist() == [2.0, 2.0, 1.0]
    # a refused attach raises before the roll-out and leaves nothing attached
    with pytest.raises(ValueError):
        sim.driveFollowGapMany(st, ticks, track=trk, track_window=-1)
    assert sim.car._track is None and len(sim.driveFollowGapMany(st, ticks)) == 4
    assert len(sim.driveFollowGapMany(st, ticks, track=trk)) == 5
