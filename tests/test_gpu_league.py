"""League races (include/scanlib_league.h: rl_policy_pop_eval_rows*, rl_car_race_league; PolicyPopulation.predict_rows,
CarBatch.race_league, RacecarSimulator.raceLeagueMany) on the MI355X, every comparison bit for bit: the row-indexed
evaluation against each member's own ``Policy`` and against ``predict_many``; the league roll-out against the entry
points it becomes with one kind of line-up (``race_followgap``, ``race_seats``, ``drive_population``), teacher-forced
against the composed public calls with the driver looked up per car, race by race against itself, and its standings
against the statement (tests/league_statement.py).

Shapes: those of test_gpu_seats.py and test_gpu_population.py — 5 races x 3 cars (a DRIVE_CARS = 8 workgroup part
filled) and 2 x 8; the 40 -> 16 -> 8 -> 1 network on beams [5, 45) of 64 and 65, 13 -> 7 -> 5 -> 1, the 720-input
fixture network on 1081 beams once per group, 24 -> 1 where the population is large."""
import ctypes as C
import math

import numpy as np
import pytest

import drive_cases as DC
import league_statement as LS
import support
import test_gpu_population as TP
from support import D_BASE, FOV, THRESH, same_bits
from test_gpu_policy import _hard_scans
from test_gpu_race_env import RaceComposed, _race_starts
from pyracecarsimulator_amd import PolicyPopulation, RacecarSimulator, _lib, league, range_libc
from pyracecarsimulator_amd import racecar as RC

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

MRX = DC.RACE_MRX
RL_ERR_INVALID = -1
CLIP = 0.2                                        # steer_clip of every clipped case
STD, NOISE_SEED, BASE = 0.02, 3, 777              # scan noise of the noisy cases
SENTINEL = np.frombuffer(np.uint32(0x7FC12345).tobytes(), np.float32)[0]      # a NaN with a payload of its own

#: the races' population: 5 seeded 40 -> 16 -> 8 -> 1 members, the last layers scaled so that answers pass CLIP
N_POP, NET_SEED, GAIN = 5, 1, 4.0
#: case 7's line-ups, different in every race: one member twice, a race that is all FollowGap, FollowGap among
#: members; member 4 enters no race.  The seeds of the starts are test_gpu_seats.py's; tools/league_census.py runs the
#: cases on the CPU (docs/history/league.md holds its output)
MIXED = {
    "5x3": dict(P=3, B=65, R=5, T=30, seed=52, entries=[[0, 1, 2], [1, 1, -1], [-1, -1, -1], [3, -1, 0], [2, 3, 1]]),
    "2x8": dict(P=8, B=64, R=2, T=24, seed=58, entries=[[0, 1, 2, 3, -1, 0, 1, 2], [3, 3, -1, 1, 0, 2, -1, 1]]),
}
#: case 8 / 9: member 0 drives 11 of the 15 cars (more than one 8-row network workgroup, spread over every race)
INDEP = dict(P=3, B=65, R=5, T=20, seed=52, odo_seed=4, entries=[[0, 0, 1], [0, 2, 0], [0, 0, -1], [3, 0, 0], [0, 0, 0]])


@pytest.fixture(scope="module")
def rig():
    g = DC.race_maze()
    omap = range_libc.PyOMap(g)
    m = range_libc.PyRayMarchingGPU(omap, MRX)
    pop, thetas, relu = TP.make_pop("small", N_POP, NET_SEED, GAIN)
    rig = dict(g=g, omap=omap, dt=omap.distance_transform(), m=m, fg=support.followgap(), cars=RC.CarBatch(), pop=pop,
               thetas=thetas, pols=[pop.member(k) for k in range(N_POP)])
    yield rig
    m.set_noise(0.0, 0, 0)


def race_inputs(rig, R, P, seed):
    states, speeds = _race_starts(rig["g"], rig["dt"], R, P, seed)
    steer0 = np.random.default_rng(seed).uniform(-0.2, 0.2, (R, P)).astype(np.float32)
    return states, speeds + 2.0, steer0           # 3 .. 6 m/s: walls within the ticks


def same_all(got, want):
    assert len(got) == len(want)
    for i, (x, y) in enumerate(zip(got, want)):
        assert same_bits(x, y), i


# ---------------------------------------------------------------- 1. rows = each member's own Policy
def _row_case(name, n_members):
    dims, in_start, relu, B = TP.NETS[name]
    pop, thetas, relu_ = TP.make_pop(name, n_members, seed=3)
    pols = [pop.member(m) for m in range(n_members)]
    scan = _hard_scans(1, B, 17)
    want = np.array([p.predict_many(scan)[0] for p in pols], np.float32)
    assert TP.differ_pairwise(list(want))         # a mix-up shows as another member's bits
    return pop, thetas, relu_, scan, want


def _check_rows(pop, scan, want, member):
    member = np.asarray(member)
    n = len(member)
    out = np.full(n, SENTINEL, np.float32)
    got = pop.predict_rows(np.tile(scan, (n, 1)), member, out=out)
    assert got is out
    expect = np.where(member >= 0, want[np.maximum(member, 0)], SENTINEL).astype(np.float32)
    assert same_bits(got, expect), (n, np.nonzero(got.view(np.uint32) != expect.view(np.uint32))[0][:8])
    return got


@pytest.mark.parametrize("name", ["small", "odd", "fixture"])
def test_rows_equal_each_members_own_policy(name):
    """Members with 0, 1, 8, 9 and 17 rows in one call (below, at and above PM_CARS: a second and a part-filled
    workgroup), -1 rows interleaved, every row the same scan."""
    n_members = 6 if name != "fixture" else 5
    pop, thetas, relu, scan, want = _row_case(name, n_members)
    counts = {0: 17, 1: 0, 2: 8, 3: 1, 4: 9}      # (member 5 of the small nets: no row either)
    member = np.concatenate([np.full(c, m) for m, c in counts.items()] + [np.full(7, -1)])
    member = np.random.default_rng(5).permutation(member)
    got = _check_rows(pop, scan, want, member)
    assert (member == -1).sum() == 7 and [int((member == m).sum()) for m in range(5)] == [17, 0, 8, 1, 9]
    dims, in_start = TP.NETS[name][0], TP.NETS[name][1]
    stmt = LS.evaluate_rows(thetas, dims, relu, np.tile(scan, (len(member), 1)), member,
                            np.full(len(member), SENTINEL, np.float32), in_start=in_start)
    assert same_bits(got, stmt)
    if name == "fixture":
        return
    # the 64-row step of the grouping's walk
    rng = np.random.default_rng(6)
    for n in (1, 63, 64, 65, 130):
        member = rng.integers(-1, n_members, n)
        member[-1] = n_members - 1                # (the last row of the last step is somebody's)
        _check_rows(pop, scan, want, member)
    # without `out` the unanswered rows read NaN
    assert np.isnan(pop.predict_rows(np.tile(scan, (3, 1)), [-1, 2, -1])[[0, 2]]).all()


# ---------------------------------------------------------------- 2. member[i] = first + i // E: predict_many
@pytest.mark.parametrize("name,E", [("small", 9), ("odd", 3)])
def test_rows_with_the_populations_layout_equal_predict_many_and_the_device_form(name, E):
    import torch
    dims, in_start, relu, B = TP.NETS[name]
    pop, thetas, _ = TP.make_pop(name, 5)
    first, n = 1, 3
    scans = TP.shared_scans(name, n, E, 3)
    member = (first + np.arange(n * E) // E).astype(np.int32)
    want = pop.predict_many(scans, E, first=first, n=n)
    got = pop.predict_rows(scans, member)
    assert same_bits(got, want) and TP.differ_pairwise([got[k * E:(k + 1) * E] for k in range(n)])
    # the device form on a stream of the caller's; entries n_members and -2 stay unanswered
    dev_member = member.copy()
    dev_member[[1, E + 2]] = (5, -2)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_scans = torch.from_numpy(scans).to("cuda:0")
        d_member = torch.from_numpy(dev_member).to("cuda:0")
        d_out = torch.full((n * E,), float("nan"), dtype=torch.float32, device="cuda:0")
        d_out.copy_(torch.from_numpy(np.full(n * E, SENTINEL, np.float32)))
        pop.predict_rows_device(d_scans.data_ptr(), d_member.data_ptr(), n * E, B, d_out.data_ptr(), stream=stream.cuda_stream)
    again = pop.predict_rows(scans, member)       # a host-form call at once: it waits for the caller's stream
    stream.synchronize()
    expect = want.copy()
    expect[[1, E + 2]] = SENTINEL
    assert same_bits(d_out.cpu().numpy(), expect) and same_bits(again, want)
    # n == 0 launches nothing
    assert pop.predict_rows(scans[:0], member[:0]).shape == (0,)


# ---------------------------------------------------------------- 3. shuffling rows changes no row's answer
@pytest.mark.parametrize("name", ["small", "odd"])
def test_shuffled_rows_keep_their_answers(name):
    dims, in_start, relu, B = TP.NETS[name]
    pop, thetas, relu_ = TP.make_pop(name, 5)
    n = 77
    rng = np.random.default_rng(8)
    scans = _hard_scans(n, B, 9)
    member = rng.integers(-1, 5, n)
    base = pop.predict_rows(scans, member, out=np.full(n, SENTINEL, np.float32))
    assert same_bits(base, LS.evaluate_rows(thetas, dims, relu_, scans, member, np.full(n, SENTINEL, np.float32), in_start=in_start))
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(n)
        got = pop.predict_rows(np.ascontiguousarray(scans[perm]), member[perm], out=np.full(n, SENTINEL, np.float32))
        assert same_bits(got, base[perm]), seed


# ---------------------------------------------------------------- 4. every entry -1: rl_car_race_followgap
@pytest.mark.parametrize("P,B,seed", [(3, 64, 52), (8, 65, 58), (1, 64, 51)])
def test_all_followgap_entries_equal_race_followgap(rig, P, B, seed):
    m, fg, cars, pop = rig["m"], rig["fg"], rig["cars"], rig["pop"]
    R, T = 5, 40
    states, speeds, steer0 = race_inputs(rig, R, P, seed)
    edge = support.edge(B)
    m.set_noise(STD, NOISE_SEED, BASE)
    want = cars.race_followgap(m, fg, states, T, speeds, FOV, B, edge, THRESH, steer0=steer0, trace=True)
    entries = np.full((R, P), -1)
    # (a clip far below FollowGap's answers: it is the members' and must not touch these cars)
    got = cars.race_league(m, pop, entries, states, T, speeds, FOV, B, edge, THRESH, followgap=fg, steer_clip=0.01,
                           steer0=steer0, trace=True)
    assert (np.abs(want[3][~np.isnan(want[3])]) > 0.01).any()
    same_all(got[:6], want)
    assert (want[0] >= 0).any() and (want[0] < 0).any()
    assert same_bits(got[6], np.zeros((N_POP, 4)))
    got = cars.race_league(m, pop, entries, states, T, speeds, FOV, B, edge, THRESH, followgap=fg, steer0=steer0)
    assert len(got) == 5
    same_all(got[:4], want[:4])


# ---------------------------------------------------------------- 5. one member in fixed seats: rl_car_race_seats
@pytest.mark.parametrize("B,clip,member", [(65, CLIP, 3), (64, None, 1), (1081, 0.4189, 2)])
def test_one_member_in_fixed_seats_equals_race_seats(rig, B, clip, member):
    """FollowGap, the member, FollowGap ("fpf") in every race."""
    m, fg, cars = rig["m"], rig["fg"], rig["cars"]
    if B == 1081:
        pop, _, _ = TP.make_pop("fixture", 3)
        pol = pop.member(member)
    else:
        pop, pol = rig["pop"], rig["pols"][member]
    R, P, T = 5, 3, 30
    states, speeds, steer0 = race_inputs(rig, R, P, 52)
    edge = support.edge(B)
    m.set_noise(STD, NOISE_SEED, BASE)
    want = cars.race_seats(m, [fg, pol, fg], states, T, speeds, FOV, B, edge, THRESH, steer_clip=clip, steer0=steer0, trace=True)
    entries = np.tile([-1, member, -1], (R, 1))
    got = cars.race_league(m, pop, entries, states, T, speeds, FOV, B, edge, THRESH, followgap=fg, steer_clip=clip,
                           steer0=steer0, trace=True)
    same_all(got[:6], want)
    st = want[3][:, 1][~np.isnan(want[3][:, 1])]
    assert st.size and (clip is None or B == 1081 or (np.abs(st) > clip).any())
    assert got[6][member, 0] == R and not got[6][np.arange(pop.n_members) != member].any()


# ---------------------------------------------------------------- 6. group = 1: rl_car_drive_population
@pytest.mark.parametrize("B,clip", [(65, CLIP), (64, None)])
def test_races_of_one_equal_drive_population(rig, B, clip):
    m, cars, pop = rig["m"], rig["cars"], rig["pop"]
    first, n, E, T = 1, 3, 5, 25
    states, speeds = support.starts(rig["g"], rig["dt"], n * E, 21, 10.0)
    edge = support.edge(B)
    m.set_noise(STD, NOISE_SEED, BASE)
    want = cars.drive_population(m, pop, states, T, speeds, FOV, B, edge, THRESH, E, first=first, steer_clip=clip, trace=True)
    entries = (first + np.arange(n * E) // E)[:, None]
    got = cars.race_league(m, pop, entries, states[:, None, :], T, speeds[:, None], FOV, B, edge, THRESH, steer_clip=clip,
                           trace=True)                       # (no FollowGap: no entry asks for one)
    for i in range(6):
        assert same_bits(got[i][:, 0], want[i]), i
    standings, fitness = got[6], want[6]
    assert same_bits(standings[first:first + n, 1:3], fitness)
    assert (standings[first:first + n, 0] == E).all() and not standings[:, 3].any()
    assert not standings[:first].any() and not standings[first + n:].any()
    assert np.isfinite(want[3][:, 0]).all() and TP.differ_pairwise([want[3][k * E:(k + 1) * E] for k in range(n)])


# ---------------------------------------------------------------- 7. mixed line-ups, teacher-forced, with noise
def teacher_forced(rig, entries, states, speeds, T, B, clip):
    """``race_league`` traced, and every link of every tick from the composed public calls (test_gpu_seats.
    teacher_forced with the driver looked up per car): the race scan at the traced lidar poses and states at that
    tick's noise offset, is_crashed, the answer of the car's own driver — its member's ``Policy`` or FollowGap —, one
    rollout step with the clamped steer.  Returns a census."""
    m, fg, pols, cars, pop = rig["m"], rig["fg"], rig["pols"], rig["cars"], rig["pop"]
    R, P = states.shape[:2]
    N = R * P
    edge = support.edge(B)
    entry = np.asarray(entries).reshape(N)
    entered = sorted(set(entry[entry >= 0].tolist()))
    m.set_noise(STD, NOISE_SEED, BASE)
    res = cars.race_league(m, pop, entries, states, T, speeds, FOV, B, edge, THRESH, followgap=fg, steer_clip=clip, trace=True)
    first, final, vel, steers, sp, st = (a.reshape((N,) + a.shape[2:]) for a in res[:6])
    pub = RaceComposed(m, cars, N, P, B, edge, 1, STD, NOISE_SEED, BASE)
    flat, fspd = states.reshape(N, 11), speeds.reshape(N)
    last = np.where(first >= 0, first, T - 1)
    census = dict(crashed=int((first >= 0).sum()), clamped=0, seen=0, net_answers=0, differ=0)
    for t in range(T):
        now = st[np.arange(N), np.minimum(t, last)]           # a wreck keeps its crash-tick row
        poses = sp[np.arange(N), np.minimum(t, last)]
        ranges = pub.scan(poses, now[:, :3], t)
        census["seen"] += int((ranges != pub.scan_alone(poses, t)).sum())
        a_fg = fg.eval_many(ranges)
        a_net = {k: pols[k].predict_many(ranges) for k in entered}
        for n in range(N):
            if t > last[n]:
                assert np.isnan(st[n, t]).all() and np.isnan(steers[n, t]) and np.isnan(vel[n, t])
                continue
            prev = flat[n] if t == 0 else st[n, t - 1]
            steer_in = 0.0 if t == 0 else float(steers[n, t - 1])
            net = entry[n] >= 0
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
            mine = a_net[entry[n]][n] if net else a_fg[n]
            assert mine.tobytes() == steers[n, t].tobytes(), (n, t, entry[n])
            if net:
                census["net_answers"] += 1
                census["differ"] += any(a_net[k][n].tobytes() != mine.tobytes() for k in entered if k != entry[n])
    assert same_bits(final, st[np.arange(N), last])
    assert same_bits(res[6], LS.standings(states, final, first, entry, pop.n_members, P, T))
    return census, res[6]


@pytest.mark.parametrize("case", sorted(MIXED))
def test_mixed_lineups_teacher_forced(rig, case):
    c = MIXED[case]
    entries = np.array(c["entries"])
    assert entries.shape == (c["R"], c["P"]) and 4 not in entries and (entries == -1).any()
    assert (entries == -1).all(1).any() or c["R"] == 2            # (two races of eight: FollowGap among the members only)
    assert any(len(set(r[r >= 0].tolist())) < (r >= 0).sum() for r in entries)       # one member twice in a race
    states, speeds, _ = race_inputs(rig, c["R"], c["P"], c["seed"])
    census, standings = teacher_forced(rig, entries, states, speeds, c["T"], c["B"], CLIP)
    assert census["crashed"] >= 1 and census["clamped"] >= 1 and census["seen"] > 0, census
    assert census["differ"] >= 0.9 * census["net_answers"] > 0, census
    assert not standings[4].any() and (standings[:4, 0] == [(entries == k).sum() for k in range(4)]).all()


# ---------------------------------------------------------------- 8 / 9. independent races; the standings
@pytest.fixture(scope="module")
def indep_run(rig):
    c = INDEP
    states, speeds, steer0 = race_inputs(rig, c["R"], c["P"], c["seed"])
    # (odometers that start anywhere in [0, 1): the gains are no round numbers, and the order of their sum shows)
    states[:, :, 8] = np.random.default_rng(c["odo_seed"]).uniform(0.0, 1.0, (c["R"], c["P"]))
    entries = np.array(c["entries"])
    edge = support.edge(c["B"])
    rig["m"].set_noise(0.0, 0, 0)
    res = rig["cars"].race_league(rig["m"], rig["pop"], entries, states, c["T"], speeds, FOV, c["B"], edge, THRESH,
                                  followgap=rig["fg"], steer_clip=CLIP, steer0=steer0, trace=True)
    return dict(states=states, speeds=speeds, steer0=steer0, entries=entries, edge=edge, res=res)


def test_races_are_independent(rig, indep_run):
    """Noise off: race r of the call has the bits of a call of that race alone."""
    c, run = INDEP, indep_run
    m, cars = rig["m"], rig["cars"]
    assert (run["entries"] == 0).sum() == 11
    m.set_noise(0.0, 0, 0)
    for r in range(c["R"]):
        one = cars.race_league(m, rig["pop"], run["entries"][r:r + 1], run["states"][r:r + 1], c["T"], run["speeds"][r:r + 1],
                               FOV, c["B"], run["edge"], THRESH, followgap=rig["fg"], steer_clip=CLIP,
                               steer0=run["steer0"][r:r + 1], trace=True)
        for i in range(6):
            assert same_bits(one[i][0], run["res"][i][r]), (r, i)
    # ... and every network answer is the member's own Policy's to the traced scan (the members' answers differ)
    steers = run["res"][3]
    assert np.isfinite(steers[:, :, 0]).all() and (run["res"][0] >= 0).any() and (run["res"][0] < 0).any()


def test_standings_equal_the_statement(rig, indep_run):
    c, run = INDEP, indep_run
    first, final, standings = run["res"][0], run["res"][1], run["res"][6]
    want = LS.standings(run["states"], final, first, run["entries"], N_POP, c["P"], c["T"])
    assert same_bits(standings, want)
    assert standings[:, 0].tolist() == [11.0, 1.0, 1.0, 1.0, 0.0] and not standings[4].any()
    assert standings[:, 2].sum() == (first.reshape(-1)[run["entries"].reshape(-1) >= 0] >= 0).sum()
    assert standings[:, 3].sum() > 0
    # the order is the contract: member 0's eleven gains summed downwards round differently
    gain = (final[:, :, 8] - run["states"][:, :, 8]).reshape(-1)[run["entries"].reshape(-1) == 0]
    down = np.float64(0.0)
    for v in gain[::-1]:
        down = down + v
    assert down != standings[0, 1] and abs(down - standings[0, 1]) < 1e-9


# ---------------------------------------------------------------- 10. past one block
def test_rows_past_one_block_of_members_and_table_entries():
    """300 members: a second trip of the offsets scan (256 members a trip); 520 rows of one member: 65 entries of the
    workgroup table, more than the wave that writes them holds."""
    name, n_members = "single", 300
    dims, in_start, relu, B = TP.NETS[name]
    pop, thetas, relu_ = TP.make_pop(name, n_members)
    counts = {299: 520, 257: 9, 0: 3, 255: 1, 256: 8}
    member = np.concatenate([np.full(c, k) for k, c in counts.items()] + [np.full(5, -1)])
    member = np.random.default_rng(11).permutation(member)
    n = len(member)
    scans = _hard_scans(n, B, 12)
    got = pop.predict_rows(scans, member, out=np.full(n, SENTINEL, np.float32))
    expect = np.full(n, SENTINEL, np.float32)
    for k in counts:
        idx = np.nonzero(member == k)[0]
        expect[idx] = pop.member(k).predict_many(np.ascontiguousarray(scans[idx]))
    assert same_bits(got, expect)
    assert LS.group_rows(member, n_members)[4] == 65 + 2 + 1 + 1 + 1
    assert same_bits(got, LS.evaluate_rows(thetas, dims, relu_, scans, member, np.full(n, SENTINEL, np.float32), in_start=in_start))


def test_standings_past_one_block_of_members(rig):
    """70 members: the standings' one lane per member reaches a second workgroup.  The call equals the call over a
    population of the three members that enter, member by member."""
    m, fg, cars = rig["m"], rig["fg"], rig["cars"]
    name = "single"
    dims, in_start, relu, _ = TP.NETS[name]
    big, thetas, _ = TP.make_pop(name, 70, gain=0.02)
    used = [5, 64, 69]
    few = PolicyPopulation(dims, 3, relu=relu, in_start=in_start)
    few.set(thetas[used])
    R, P, T, B = 5, 3, 20, 64
    states, speeds, steer0 = race_inputs(rig, R, P, 52)
    states[:, :, 8] = np.random.default_rng(5).uniform(0.0, 1000.0, (R, P))
    small = np.array([[0, 1, 2], [2, 2, -1], [1, 0, 2], [-1, 2, 1], [2, 1, 2]])
    entries = np.where(small >= 0, np.array(used)[np.maximum(small, 0)], -1)
    edge = support.edge(B)
    m.set_noise(STD, NOISE_SEED, BASE)
    kw = dict(followgap=fg, steer_clip=CLIP, steer0=steer0, trace=True)
    got = cars.race_league(m, big, entries, states, T, speeds, FOV, B, edge, THRESH, **kw)
    want = cars.race_league(m, few, small, states, T, speeds, FOV, B, edge, THRESH, **kw)
    same_all(got[:6], want[:6])
    assert same_bits(got[6][used], want[6]) and not np.delete(got[6], used, 0).any()
    assert same_bits(got[6], LS.standings(states, got[1], got[0], entries, 70, P, T))
    assert got[6][69, 0] == 7 and np.isfinite(got[3][:, :, 0]).all()


# ---------------------------------------------------------------- 11. refusals
def test_refusals_leave_the_handles_usable(rig):
    m, fg, cars, pop = rig["m"], rig["fg"], rig["cars"], rig["pop"]
    L = _lib.lib()
    R, P, B, T = 2, 3, 64, 3
    states, speeds, _ = race_inputs(rig, R, P, 52)
    edge = support.edge(B)
    entries = np.array([[0, -1, 4], [1, 1, -1]])
    m.set_noise(STD, NOISE_SEED, BASE)
    want = cars.race_league(m, pop, entries, states, T, speeds, FOV, B, edge, THRESH, followgap=fg)
    scans = _hard_scans(6, B, 2)
    rows_member = np.array([0, 4, -1, 2, 2, 1], np.int32)
    want_rows = pop.predict_rows(scans, rows_member)
    i32 = C.POINTER(C.c_int)

    def raw(entry=entries, g=fg._h, p=pop._h, c=cars._h, h=m._h, group=P, nr=B, n_ticks=T, null=()):
        st = np.ascontiguousarray(states.reshape(-1, 11))
        sp = np.ascontiguousarray(speeds.reshape(-1))
        first = np.zeros(R * P, np.int32)
        en = np.ascontiguousarray(np.asarray(entry).reshape(-1), np.int32)
        ptr = dict(entry=en.ctypes.data_as(i32), states=st.ctypes.data_as(_lib.f64p), speeds=sp.ctypes.data_as(_lib.f64p),
                   edge=support.edge(nr).ctypes.data_as(_lib.f64p), first=first.ctypes.data_as(i32))
        for k in null:
            ptr[k] = None
        return L.rl_car_race_league(c, h, g, p, ptr["entry"], 0.0, ptr["states"], ptr["speeds"], None, R, group, n_ticks, 0.01,
                                    D_BASE, FOV, nr, ptr["edge"], THRESH, ptr["first"], None, None, None, None, None, None)

    def raw_rows(member=rows_member, p=pop._h, n=6, size=B, null=()):
        out = np.zeros(6, np.float32)
        ptr = dict(member=np.ascontiguousarray(member, np.int32).ctypes.data_as(i32), scans=scans.ctypes.data_as(_lib.f32p),
                   steers=out.ctypes.data_as(_lib.f32p))
        for k in null:
            ptr[k] = None
        return L.rl_policy_pop_eval_rows(p, n, ptr["member"], ptr["scans"], size, ptr["steers"])

    def usable():
        got = cars.race_league(m, pop, entries, states, T, speeds, FOV, B, edge, THRESH, followgap=fg)
        same_all(got, want)
        assert same_bits(pop.predict_rows(scans, rows_member), want_rows)

    assert raw() == 0 and raw_rows() == 0
    wide = PolicyPopulation((40, 16, 8, 1), 5, in_start=30)       # window [30, 70): 64 beams do not hold it
    for kw in (dict(entry=[[0, -1, 5], [1, 1, -1]]), dict(entry=[[0, -2, 4], [1, 1, -1]]), dict(g=None), dict(p=None),
               dict(c=None), dict(h=None), dict(group=0), dict(group=9), dict(null=("entry",)), dict(null=("states",)),
               dict(null=("speeds",)), dict(null=("edge",)), dict(null=("first",)), dict(p=wide._h), dict(nr=9),
               dict(n_ticks=0)):
        assert raw(**kw) == RL_ERR_INVALID, kw
        assert L.rl_last_error()
        usable()
    for kw in (dict(member=[0, 5, -1, 2, 2, 1]), dict(member=[0, -2, -1, 2, 2, 1]), dict(p=None), dict(n=-1), dict(size=44),
               dict(null=("member",)), dict(null=("scans",)), dict(null=("steers",)), dict(p=wide._h)):
        assert raw_rows(**kw) == RL_ERR_INVALID, kw
        usable()
    assert L.rl_policy_pop_eval_rows_device(pop._h, 6, None, None, B, None, None) == RL_ERR_INVALID
    assert L.rl_policy_pop_eval_rows_device(None, 0, None, None, B, None, None) == RL_ERR_INVALID
    cdd = range_libc.PyCDDTCast(rig["omap"], MRX, 108)
    assert raw(h=cdd._h) < 0                                      # the race scan's own refusal, with its code
    # what is no refusal: no -1 entry needs no FollowGap; all -1 does not read the window; n == 0 and n_races == 0
    assert raw(entry=[[0, 1, 4], [1, 1, 2]], g=None) == 0
    assert raw(entry=np.full((R, P), -1), p=wide._h) == 0
    assert raw_rows(n=0, null=("member", "scans", "steers")) == 0
    assert L.rl_car_race_league(cars._h, m._h, None, pop._h, None, 0.0, None, None, None, 0, P, T, 0.01, D_BASE, FOV, B, None,
                                THRESH, None, None, None, None, None, None, None) == 0
    usable()
    # the Python wrappers refuse the same before the library
    with pytest.raises(ValueError):
        cars.race_league(m, pop, [[0, -1, 5], [1, 1, -1]], states, T, speeds, FOV, B, edge, THRESH, followgap=fg)
    with pytest.raises(ValueError):
        cars.race_league(m, pop, entries, states, T, speeds, FOV, B, edge, THRESH)


# ---------------------------------------------------------------- 12. the facade
def test_facade_matches_hand_built():
    """RacecarSimulator.raceLeagueMany is race_league on the simulator's method, car, fan, edge table, thresholds and
    own FollowGap driver, with round_robin's line-ups."""
    g = DC.race_maze()
    cfg = dict(RC.DEFAULT_CAR)
    cfg.update(scan_dist_to_base=D_BASE, batch_size=40, scan_beams=1080, scan_fov=FOV, scan_std=0.01,
               scan_max_range=15.0, free_thresh=0.8)
    sim = RacecarSimulator(cfg)
    omap = range_libc.PyOMap(g)
    sim.setMap(omap, g.resolution, g.origin)
    sim.setRaytracingMethod("RMGPU")
    pop, _, _ = TP.make_pop("fixture", 3)
    entries = league.round_robin(3, 2)[:3].copy()
    assert entries.tolist() == [[0, 1], [1, 0], [0, 2]]
    entries[2, 0] = -1
    R, P, T = 3, 2, 12
    states, _ = _race_starts(g, omap.distance_transform(), R, P, 52)
    got = sim.raceLeagueMany(states, T, pop, entries, speed=3.0, steer_clip=0.4189)
    want = sim.car.race_league(sim.scan_simulator.scan_method, pop, entries, states, T, 3.0, FOV, 1080, sim.edge_distances,
                               cfg["ttc_thresh"], followgap=sim._followgap, steer_clip=0.4189, scan_dist_to_base=D_BASE)
    assert len(got) == 5
    same_all(got, want)
    assert got[3].shape == (R, P, T) and np.isfinite(got[3][:, :, 0]).all() and got[4].shape == (3, 4)
    assert got[4][:, 0].tolist() == [2.0, 2.0, 1.0]
