"""Policy populations on the MI355X (include/scanlib_population.h: rl_policy_pop_*, rl_car_drive_population;
PolicyPopulation, CarBatch.drive_population, RacecarSimulator.drivePopulationMany): every answer bit for bit the
member's own ``Policy`` and the statement (tests/population_statement.py), and the closed loop bit for bit the
per-member ``drive_policy`` calls (noise off), the loop composed from the public calls (noise on) and, with one member,
``drive_policy`` itself.

Shapes: members N in {1, 3, 5} and cars per member E in {1, 3, 8, 9, 11}: below, at and above PM_CARS = 8, so members fall
out of step with the 8-car network workgroups and the DRIVE_CARS = 8 tick workgroups; 64 beams (ROWS 1, full) and 65
(one lane in the last row) with the small networks, 1081 only with the 720-input fixture network."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import policy_statement as S
import population_statement as PS
import support
from conftest import GOLD
from support import D_BASE, FOV, THRESH, same_bits
from test_gpu_policy import _hard_scans
from pyracecarsimulator_amd import Policy, PolicyPopulation, RacecarSimulator, _lib, maps, population, range_libc
from pyracecarsimulator_amd import racecar as RC

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

MRX = 300
CLIP = 0.2                                        # steer_clip of the clipped cases: below the networks' larger answers
STD, NOISE_SEED, BASE = 0.05, 99, 4242            # scan noise of the noisy cases
N_MEMBERS = (1, 3, 5)
CARS = (1, 3, 8, 9, 11)

#: name -> (dims, in_start, relu or None, beams of its scans)
NETS = {
    "small": ((40, 16, 8, 1), 5, None, 65),       # reads beams [5, 45)
    "odd": ((13, 7, 5, 1), 3, None, 64),          # no width a multiple of 4, no K a multiple of 16
    "single": ((24, 1), 0, (False,), 64),         # one layer
    "wide": ((32, 256, 1), 7, None, 65),          # the width cap
    "fixture": ((720, 64, 128, 128, 64, 1), 180, None, 1081),
}
#: the roll-out cases' starts on the 512^2 maze: seeds of the far (clear 8 px) and near (clear 1 px) cars and the
#: members' seeds, picked on the CPU (tools/population_census.py; docs/history/population.md holds its output)
ROLLOUT = dict(far=3, near=2, far_seed=31, near_seed=32, net_seed=1, gain=4.0)
ROLLOUT_FIXTURE = dict(far=3, near=2, far_seed=31, near_seed=32)


def members(name, n, seed=1, gain=1.0):
    """n seeded members of the network ``name``: a list of layer lists.  The fixture's members are the reference's
    weights with the last layer scaled and shifted member by member."""
    dims = NETS[name][0]
    if name == "fixture":
        layers, _ = S.load_fixture(os.path.join(GOLD, "policy_mlp720.npz"))
        return [[(W, b) for W, b in layers[:-1]] + [((layers[-1][0] * np.float32(1.0 + 0.5 * m)).astype(np.float32),
                                                    (layers[-1][1] + np.float32(0.05 * m)).astype(np.float32))]
                for m in range(n)]
    out = []
    for m in range(n):
        rng = np.random.default_rng(1000 * seed + m)
        layers = [(rng.normal(0.0, 1.0 / math.sqrt(k), (k, w)).astype(np.float32), rng.normal(0.0, 0.1, w).astype(np.float32))
                  for k, w in zip(dims[:-1], dims[1:])]
        layers[-1] = ((layers[-1][0] * np.float32(gain)).astype(np.float32), layers[-1][1])
        out.append(layers)
    return out


def make_pop(name, n, seed=1, gain=1.0):
    """(population, thetas (n, P), relu) of ``members(name, n)``."""
    dims, in_start, relu, _ = NETS[name]
    pop = PolicyPopulation(dims, n, relu=relu, in_start=in_start)
    thetas = np.stack([population.pack(l) for l in members(name, n, seed, gain)])
    pop.set(thetas)
    return pop, thetas, pop.relu


def shared_scans(name, n, E, seed):
    """Every member the same E hard scans: a member mix-up shows as another member's answers."""
    return np.tile(_hard_scans(E, NETS[name][3], seed), (n, 1))


def differ_pairwise(blocks):
    return len({np.asarray(b).tobytes() for b in blocks}) == len(blocks)


@pytest.fixture(scope="module")
def rig():
    g = maps.make_maze(512, cell=40, wall=3, p=0.45, seed=11)
    omap = range_libc.PyOMap(g)
    rig = dict(g=g, omap=omap, dt=omap.distance_transform(), cars=RC.CarBatch(),
               m=range_libc.PyRayMarchingGPU(omap, MRX))
    yield rig
    rig["m"].set_noise(0.0, 0, 0)


def rollout_starts(rig, cfg, n):
    """The 5 starts of a member (some in the open, some a cell from a wall), the same for every one of n members."""
    far, sp_far = support.starts(rig["g"], rig["dt"], cfg["far"], cfg["far_seed"], 8.0)
    near, sp_near = support.starts(rig["g"], rig["dt"], cfg["near"], cfg["near_seed"], 1.0)
    return np.tile(np.concatenate([far, near]), (n, 1)), np.tile(np.concatenate([sp_far, sp_near]), n)


# ---------------------------------------------------------------- 1. set / get
def test_set_get_round_trip_and_zero_members():
    import torch
    name = "odd"
    dims, in_start, relu, B = NETS[name]
    pop = PolicyPopulation(dims, 5, relu=relu, in_start=in_start)
    assert pop.n_params == PS.n_params(dims) == 14 * 7 + 8 * 5 + 6
    scans = shared_scans(name, 5, 3, 1)
    zero = Policy.from_arrays([(np.zeros((k, w), np.float32), np.zeros(w, np.float32)) for k, w in zip(dims[:-1], dims[1:])],
                              in_start=in_start)
    fresh = pop.predict_many(scans, 3)
    assert same_bits(fresh, zero.predict_many(scans)) and same_bits(fresh, np.zeros(15, np.float32))
    assert all(same_bits(pop.get(m), np.zeros(pop.n_params, np.float32)) for m in range(5))
    thetas = np.stack([population.pack(l) for l in members(name, 5)])
    pop.set(thetas)
    assert all(same_bits(pop.get(m), thetas[m]) for m in range(5))
    # a sub-range leaves the others' bits alone (NaN and -0.0 payloads survive: the re-layout moves bits)
    new = np.stack([population.pack(l) for l in members(name, 2, seed=7)])
    new[0, 5], new[1, -1] = np.float32(np.nan), np.float32(-0.0)
    pop.set(new, first=1)
    for m in range(5):
        assert same_bits(pop.get(m), new[m - 1] if m in (1, 2) else thetas[m]), m
    pop.set(new[0], first=4)                                        # one member as (P,)
    assert same_bits(pop.get(4), new[0]) and same_bits(pop.get(3), thetas[3])
    # set_device from a torch tensor equals set
    pop.set(thetas)
    dev = PolicyPopulation(dims, 5, relu=relu, in_start=in_start)
    t = torch.from_numpy(thetas).to("cuda:0")
    dev.set_device(t[1:4].contiguous(), first=1)
    dev.set_device(t[:1].contiguous())
    dev.set_device(t[4], first=4)
    assert all(same_bits(dev.get(m), thetas[m]) for m in range(5))
    assert same_bits(dev.predict_many(scans, 3), pop.predict_many(scans, 3))
    # ... and on a stream of the caller's, followed at once by a host-form call on the handle's own stream
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t2 = torch.from_numpy(new).to("cuda:0", non_blocking=False)
        dev.set_device(t2, first=2)
    got = dev.predict_many(scans, 3)
    pop.set(new, first=2)
    assert same_bits(got, pop.predict_many(scans, 3))
    n, p = C.c_int(), C.c_int()
    _lib.call("rl_policy_pop_layout", pop, n, p)
    assert (n.value, p.value) == (5, pop.n_params)


# ---------------------------------------------------------------- 2. eval = per-member Policy = the statement
@pytest.mark.parametrize("name", ["small", "odd", "single", "wide"])
def test_eval_equals_member_policies_and_statement(name):
    dims, in_start, relu, B = NETS[name]
    for n in N_MEMBERS:
        pop, thetas, relu_ = make_pop(name, n, seed=n)
        pols = [pop.member(m) for m in range(n)]
        for E in CARS:
            scans = shared_scans(name, n, E, 10 * n + E)
            got = pop.predict_many(scans, E)
            want = np.concatenate([pols[m].predict_many(scans[m * E:(m + 1) * E]) for m in range(n)])
            assert same_bits(got, want), (name, n, E)
            assert same_bits(got, PS.evaluate(thetas, dims, relu_, scans, E, in_start=in_start)), (name, n, E)
            assert differ_pairwise([got[m * E:(m + 1) * E] for m in range(n)]), (name, n, E)


@pytest.mark.parametrize("name,E", [("small", 9), ("odd", 3), ("fixture", 11)])
def test_eval_sub_range_and_device_form(name, E):
    """first = 1, n = 2 of 5, host and device form; with the fixture network (1081 beams) also all 5."""
    import torch
    dims, in_start, relu, B = NETS[name]
    pop, thetas, relu_ = make_pop(name, 5)
    pols = [pop.member(m) for m in range(5)]
    scans = shared_scans(name, 2, E, 3)
    want = np.concatenate([pols[1 + m].predict_many(scans[m * E:(m + 1) * E]) for m in range(2)])
    got = pop.predict_many(scans, E, first=1, n=2)
    assert same_bits(got, want) and differ_pairwise([got[:E], got[E:]])
    assert same_bits(got, PS.evaluate(thetas, dims, relu_, scans, E, first=1, n=2, in_start=in_start))
    d_in = torch.from_numpy(scans).to("cuda:0")
    d_out = torch.full((2 * E,), float("nan"), dtype=torch.float32, device="cuda:0")
    pop.predict_device(d_in.data_ptr(), E, B, d_out.data_ptr(), first=1, n=2,
                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert same_bits(d_out.cpu().numpy(), want)
    if name == "fixture":
        scans = shared_scans(name, 5, E, 4)
        got = pop.predict_many(scans, E)
        want = np.concatenate([pols[m].predict_many(scans[m * E:(m + 1) * E]) for m in range(5)])
        assert same_bits(got, want) and differ_pairwise([got[m * E:(m + 1) * E] for m in range(5)])
        assert same_bits(got[:2 * E], PS.evaluate(thetas, dims, relu_, scans[:2 * E], E, n=2))
    # from_policies builds the same population
    again = PolicyPopulation.from_policies(pols)
    assert all(same_bits(again.get(m), thetas[m]) for m in range(5))


# ---------------------------------------------------------------- 3 / 8. the roll-out, noise off: per-member drive_policy
def per_member_drive(cars, m, pols, states, speeds, T, B, edge, clip, E, steer0=None):
    """The parent's way: one drive_policy call per member on its E cars, concatenated."""
    outs = [cars.drive_policy(m, pol, states[k * E:(k + 1) * E], T, speeds[k * E:(k + 1) * E], FOV, B, edge, THRESH,
                              steer_clip=clip, trace=True, steer0=None if steer0 is None else steer0[k * E:(k + 1) * E])
            for k, pol in enumerate(pols)]
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(6))


def census(res, n, E, clip):
    """What a roll-out case has to show on the device's own run."""
    first, steers = res[0], res[3]
    assert differ_pairwise([steers[k * E:(k + 1) * E] for k in range(n)])
    assert (first >= 0).any() and (first < 0).any()
    if clip:
        assert (np.abs(steers[np.isfinite(steers)]) > clip).any()


@pytest.mark.parametrize("method,B,clip", [("RMGPU", 65, None), ("RMGPU", 64, CLIP), ("RM", 64, None), ("RM", 65, CLIP)])
def test_rollout_equals_per_member_drive_policy(rig, method, B, clip):
    """3 members x 5 cars x 25 ticks from the same 5 starts, noise off: every output with its traces."""
    cars = rig["cars"]
    m = rig["m"] if method == "RMGPU" else range_libc.PyRayMarching(rig["omap"], MRX)
    n, E, T = 3, 5, 25
    dims, in_start, relu, _ = NETS["small"]
    pop, thetas, _ = make_pop("small", n, ROLLOUT["net_seed"], ROLLOUT["gain"])
    pols = [pop.member(k) for k in range(n)]
    states, speeds = rollout_starts(rig, ROLLOUT, n)
    edge = support.edge(B)
    m.set_noise(0.0, 0, 0)
    got = cars.drive_population(m, pop, states, T, speeds, FOV, B, edge, THRESH, E, steer_clip=clip, trace=True)
    want = per_member_drive(cars, m, pols, states, speeds, T, B, edge, clip, E)
    assert len(got) == 7
    for i, (x, y) in enumerate(zip(got[:6], want)):
        assert same_bits(x, y), (method, B, clip, i)
    assert same_bits(got[6], PS.fitness(states, got[1], got[0], E))
    census(got, n, E, clip)
    # members [1, 3) of the same population on their cars, and without the traces
    sub = cars.drive_population(m, pop, states[:2 * E], T, speeds[:2 * E], FOV, B, edge, THRESH, E, first=1, steer_clip=clip)
    assert len(sub) == 5
    for i in range(4):
        assert same_bits(sub[i], want[i][E:3 * E]), i


def test_rollout_fixture_network_1081_beams(rig):
    cars, m = rig["cars"], rig["m"]
    n, E, T, B = 3, 5, 25, 1081
    pop, thetas, _ = make_pop("fixture", n)
    pols = [pop.member(k) for k in range(n)]
    states, speeds = rollout_starts(rig, ROLLOUT_FIXTURE, n)
    edge = support.edge(B)
    m.set_noise(0.0, 0, 0)
    got = cars.drive_population(m, pop, states, T, speeds, FOV, B, edge, THRESH, E, steer_clip=CLIP, trace=True)
    want = per_member_drive(cars, m, pols, states, speeds, T, B, edge, CLIP, E)
    for i, (x, y) in enumerate(zip(got[:6], want)):
        assert same_bits(x, y), i
    assert same_bits(got[6], PS.fitness(states, got[1], got[0], E))
    census(got, n, E, CLIP)


# ---------------------------------------------------------------- 4. the roll-out, noise on: composed public calls
def composed(cars, m, std, base, pols, E, states, speeds, steer0, T, B, edge, clip):
    """The loop from the public calls (test_gpu_policy.py's composition with the member of the car answering):
    set_noise at base + t R B, calc_range_fan, per-member predict_many, is_crashed, rollout(n_steps=1)."""
    R = states.shape[0]
    cur = states.copy()
    steer = steer0.astype(np.float64)
    alive = np.ones(R, bool)
    first = np.full(R, -(T + 1), np.int32)
    steers = np.full((R, T), np.nan, np.float32)
    st = np.full((R, T, 11), np.nan)
    last_pose = np.zeros((R, 3), np.float32)
    for t in range(T):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        _, out, _ = cars.rollout(cur[idx], np.stack([speeds[idx], steer[idx]], -1)[:, None, :], n_steps=1, action_every=1)
        cur[idx] = out
        st[idx, t] = out
        last_pose[idx] = support.lidar_poses(out)
        ranges = np.empty(R * B, np.float32)
        m.set_noise(std, NOISE_SEED, base + t * R * B)
        m.calc_range_fan(last_pose, ranges, FOV, B)
        ranges = ranges.reshape(R, B)
        crashed = np.array([RC.is_crashed(ranges[r], B, 1, edge, THRESH) >= 0 for r in idx], bool)
        first[idx[crashed]] = t
        alive[idx[crashed]] = False
        for r in idx[~crashed]:
            a = pols[r // E].predict_many(ranges[r:r + 1])[0]
            steers[r, t] = a
            s64 = np.float64(a)
            steer[r] = np.clip(s64, -clip, clip) if clip else s64
    return first, cur, steers, st


def same_or_nan(a, b):
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and (na == nb).all() and same_bits(a[~na], b[~nb])


@pytest.mark.parametrize("method,B,n,E,clip", [("RMGPU", 65, 3, 5, CLIP), ("RMGPU", 64, 5, 3, None), ("CDDT", 64, 3, 5, None),
                                               ("CDDT", 65, 5, 3, CLIP)])
def test_rollout_noise_on_equals_composed_public_calls(rig, method, B, n, E, clip):
    cars = rig["cars"]
    m, std = (rig["m"], STD) if method == "RMGPU" else (range_libc.PyCDDTCast(rig["omap"], MRX, 112), 0.02)
    T = 25
    pop, thetas, _ = make_pop("small", n, ROLLOUT["net_seed"], ROLLOUT["gain"])
    pols = [pop.member(k) for k in range(n)]
    far, sp_far = support.starts(rig["g"], rig["dt"], n * E - 4, 31, 8.0)
    near, sp_near = support.starts(rig["g"], rig["dt"], 4, 32, 1.0)
    states, speeds = np.concatenate([far, near]), np.concatenate([sp_far, sp_near])
    steer0 = np.random.default_rng(7).uniform(-0.3, 0.3, n * E).astype(np.float32)
    edge = support.edge(B)
    m.set_noise(std, NOISE_SEED, BASE)
    first, final, vel, steers, sp, st, fit = cars.drive_population(m, pop, states, T, speeds, FOV, B, edge, THRESH, E,
                                                                   steer0=steer0, steer_clip=clip, trace=True)
    want = composed(cars, m, std, BASE, pols, E, states, speeds, steer0, T, B, edge, clip or 0.0)
    m.set_noise(0.0, 0, 0)
    assert (first == want[0]).all()
    assert same_bits(final, want[1])
    assert same_or_nan(steers, want[2]) and same_or_nan(st, want[3]) and same_or_nan(vel, st[..., 3])
    assert (first >= 0).any() and (first < 0).any()
    assert same_bits(fit, PS.fitness(states, final, first, E))


# ---------------------------------------------------------------- 5. one member: drive_policy
@pytest.mark.parametrize("E,B", [(11, 65), (8, 64), (1, 64)])
def test_one_member_equals_drive_policy(rig, E, B):
    cars, m = rig["cars"], rig["m"]
    pop, thetas, _ = make_pop("small", 1, ROLLOUT["net_seed"], ROLLOUT["gain"])
    pol = pop.member(0)
    states, speeds = support.starts(rig["g"], rig["dt"], E, 33, 3.0)
    edge = support.edge(B)
    for clip in (None, CLIP):
        m.set_noise(STD, NOISE_SEED, BASE)
        want = cars.drive_policy(m, pol, states, 25, speeds, FOV, B, edge, THRESH, steer_clip=clip, trace=True)
        got = cars.drive_population(m, pop, states, 25, speeds, FOV, B, edge, THRESH, E, steer_clip=clip, trace=True)
        m.set_noise(0.0, 0, 0)
        for i, (x, y) in enumerate(zip(got[:6], want)):
            assert same_bits(x, y), (clip, i)
        assert got[6].shape == (1, 2)


# ---------------------------------------------------------------- 6. chunking
def test_chunking_is_invariant(rig):
    """T ticks in one call == T/2 + T/2 with the states, the last steers and the noise offset chained."""
    cars, m = rig["cars"], rig["m"]
    n, E, T, H, B = 3, 9, 24, 12, 65
    R = n * E
    pop, thetas, _ = make_pop("small", n, ROLLOUT["net_seed"], ROLLOUT["gain"])
    states, speeds = support.starts(rig["g"], rig["dt"], R, 34, 3.0)
    edge = support.edge(B)
    for clip in (None, CLIP):
        m.set_noise(STD, NOISE_SEED, BASE)
        whole = cars.drive_population(m, pop, states, T, speeds, FOV, B, edge, THRESH, E, steer_clip=clip, trace=True)
        a = cars.drive_population(m, pop, states, H, speeds, FOV, B, edge, THRESH, E, steer_clip=clip, trace=True)
        ok = a[0] < 0
        st0 = np.where(ok, a[3][:, -1], np.float32(0.0)).astype(np.float32)
        m.set_noise(STD, NOISE_SEED, BASE + H * R * B)
        b = cars.drive_population(m, pop, a[1], T - H, speeds, FOV, B, edge, THRESH, E, steer0=st0, steer_clip=clip,
                                  trace=True)
        m.set_noise(0.0, 0, 0)
        for k in range(2, 6):
            assert same_bits(whole[k][:, :H], a[k]), (clip, k)
        # steer0 is f32: with the clip on, the chained call equals the whole one for the cars whose last answer the
        # clamp leaves alone (a clamped one would get the f32 bound, not the f64 one)
        raw = a[3][:, -1].astype(np.float64)
        exact = ok if not clip else ok & (np.abs(raw) <= clip)
        assert exact.any()
        assert same_bits(whole[1][exact], b[1][exact]), clip
        for k in range(2, 6):
            assert same_bits(whole[k][exact, H:], b[k][exact]), (clip, k)
        want_first = np.where(b[0][exact] >= 0, b[0][exact] + H, -(T + 1))
        assert (whole[0][exact] == want_first).all(), clip


# ---------------------------------------------------------------- 7. fitness
def test_fitness_is_the_ascending_sum_and_the_crash_count(rig):
    cars, m = rig["cars"], rig["m"]
    n, E, T, B = 5, 11, 25, 64
    pop, thetas, _ = make_pop("small", n, ROLLOUT["net_seed"], ROLLOUT["gain"])
    far, sp_far = support.starts(rig["g"], rig["dt"], n * E - 12, 35, 6.0)
    near, sp_near = support.starts(rig["g"], rig["dt"], 12, 36, 1.0)
    order = np.random.default_rng(3).permutation(n * E)            # the near cars spread over the members
    states, speeds = np.concatenate([far, near])[order], np.concatenate([sp_far, sp_near])[order]
    states[:, 8] = 10.0 ** np.random.default_rng(4).uniform(-6.0, 3.0, n * E)    # travel_dist so far, of every size: the sums round
    m.set_noise(STD, NOISE_SEED, BASE)
    first, final, vel, steers, fit = cars.drive_population(m, pop, states, T, speeds, FOV, B, support.edge(B), THRESH, E)
    m.set_noise(0.0, 0, 0)
    assert fit.shape == (n, 2) and fit.dtype == np.float64
    d = final[:, 8] - states[:, 8]
    want = np.array([np.cumsum(d[k * E:(k + 1) * E])[-1] for k in range(n)])       # (cumsum adds one by one, upwards)
    assert same_bits(fit[:, 0], want)
    assert same_bits(fit, PS.fitness(states, final, first, E))
    down = np.array([np.cumsum(d[k * E:(k + 1) * E][::-1])[-1] for k in range(n)])
    assert (down != want).any()                                     # the order shows in these sums
    assert (fit[:, 1] == (first >= 0).reshape(n, E).sum(1)).all()
    assert 0 < fit[:, 1].sum() < n * E and (d >= 0).all() and d.sum() > 0


# ---------------------------------------------------------------- 9. refusals and the façade
def test_refusals_leave_the_handles_usable_and_the_facade(rig):
    cars, m, g, omap = rig["cars"], rig["m"], rig["g"], rig["omap"]
    n, E, T, B = 3, 3, 10, 65
    R = n * E
    pop, thetas, _ = make_pop("small", 5, ROLLOUT["net_seed"], ROLLOUT["gain"])
    states, speeds = support.starts(g, rig["dt"], R, 2, 8.0)
    edge = support.edge(B)
    scans = shared_scans("small", n, E, 1)
    m.set_noise(0.0, 0, 0)
    drive0 = cars.drive_population(m, pop, states, T, speeds, FOV, B, edge, THRESH, E, first=1)
    p0 = pop.predict_many(scans, E, first=2)

    def still_usable():
        assert same_bits(pop.predict_many(scans, E, first=2), p0)
        assert all(same_bits(pop.get(k), thetas[k]) for k in range(5))
        again = cars.drive_population(m, pop, states, T, speeds, FOV, B, edge, THRESH, E, first=1)
        for x, y in zip(drive0, again):
            assert same_bits(x, y)

    L = _lib.lib()
    f32p, f64p, ip = _lib.f32p, _lib.f64p, C.POINTER(C.c_int)
    out = np.empty(R, np.float32)
    theta2 = np.ascontiguousarray(thetas[:2])

    def ev(first=2, n_=n, E_=E, sc=scans, size=B, o=out, h=pop._h):
        return L.rl_policy_pop_eval(h, first, n_, E_, sc.ctypes.data_as(f32p) if sc is not None else None, size,
                                    o.ctypes.data_as(f32p) if o is not None else None)

    def drive(first=1, n_=n, E_=E, T_=T, nr=B, st_=states, h_pop=pop._h, h_car=cars._h, fst=True):
        f = np.zeros(R, np.int32)
        return L.rl_car_drive_population(h_car, m._h, h_pop, first, n_, E_, 0.0,
                                         st_.ctypes.data_as(f64p) if st_ is not None else None,
                                         speeds.ctypes.data_as(f64p), None, T_, 0.01, D_BASE, FOV, nr,
                                         support.edge(nr).ctypes.data_as(f64p), THRESH,
                                         f.ctypes.data_as(ip) if fst else None, None, None, None, None, None, None)

    bad = [ev(first=-1), ev(n_=-1), ev(first=3), ev(E_=0), ev(size=44, sc=np.ascontiguousarray(scans[:, :44])),
           ev(sc=None), ev(o=None), ev(h=None), ev(n_=1, E_=1 << 20, size=1 << 11),
           L.rl_policy_pop_set(pop._h, 4, 2, theta2.ctypes.data_as(f32p)),
           L.rl_policy_pop_set(pop._h, -1, 2, theta2.ctypes.data_as(f32p)), L.rl_policy_pop_set(pop._h, 0, 2, None),
           L.rl_policy_pop_set_device(pop._h, 0, 2, None, None), L.rl_policy_pop_set_device(pop._h, 5, 1, 64, None),
           L.rl_policy_pop_get(pop._h, 5, out.ctypes.data_as(f32p)), L.rl_policy_pop_get(pop._h, 0, None),
           L.rl_policy_pop_eval_device(pop._h, 0, 2, 3, None, B, None, None),
           L.rl_policy_pop_layout(None, None, None),
           drive(first=-1), drive(first=3), drive(n_=-1), drive(E_=0), drive(T_=0), drive(st_=None), drive(fst=False),
           drive(h_pop=None), drive(h_car=None), drive(nr=44), drive(n_=1, E_=1 << 30)]
    for i, rc in enumerate(bad):
        assert rc == _lib.RL_ERR_INVALID, i
    still_usable()
    # rl_policy_create's refusals with its codes
    h = C.c_void_p()
    relu = np.ones(9, np.uint8)

    def create(n_members, dims, in_start=0, device=0):
        d = np.array(dims, np.int32)
        return L.rl_policy_pop_create(device, n_members, len(dims) - 1, d.ctypes.data_as(_lib.i32p),
                                      relu.ctypes.data_as(_lib.u8p), in_start, 15.0, 15.0, C.byref(h))

    assert create(0, (4, 1)) == create(2, (4, 0, 1)) == create(2, (4, 1), in_start=-1) == create(2, (4,)) == _lib.RL_ERR_INVALID
    assert create(2, (4,) * 9 + (1,)) == create(2, (1025, 1)) == create(2, (4, 257, 1)) == create(2, (4, 2)) \
        == _lib.RL_ERR_UNSUPPORTED
    assert create(2, (4, 1), device=99) != 0 and not h.value
    assert L.rl_policy_pop_create(0, 2, 1, None, None, 0, 15.0, 15.0, C.byref(h)) == _lib.RL_ERR_INVALID
    # n == 0 is RL_OK and launches nothing
    assert ev(n_=0) == 0 and drive(n_=0) == 0 and L.rl_policy_pop_set(pop._h, 5, 0, None) == 0
    assert pop.predict_many(scans[:0], E, first=5).shape == (0,)
    # multi-device handles, and a handle on another device
    with pytest.raises(_lib.ScanLibError, match="single-device"):
        RC.CarBatch(device=[0]).drive_population(m, pop, states, T, speeds, FOV, B, edge, THRESH, E, first=1)
    if L.rl_device_count() >= 2:
        pop1 = PolicyPopulation(NETS["small"][0], 3, in_start=5, device=1)
        with pytest.raises(_lib.ScanLibError, match="device"):
            cars.drive_population(m, pop1, states, T, speeds, FOV, B, edge, THRESH, E)
    still_usable()
    # the façade: drivePopulationMany is drive_population on the simulator's method, edge table and thresholds
    fpop, _, _ = make_pop("fixture", 2)
    cfg = dict(RC.DEFAULT_CAR)
    cfg.update(scan_dist_to_base=0.275, batch_size=40, scan_beams=1080, scan_fov=4.71, scan_std=0.01, scan_max_range=15.0,
               free_thresh=0.8)
    sim = RacecarSimulator(cfg)
    sim.setMap(omap, g.resolution, g.origin)
    sim.setRaytracingMethod("RMGPU")
    got = sim.drivePopulationMany(states[:6], 5, fpop, 3, speed=2.0, steer_clip=0.4189)
    want = sim.car.drive_population(sim.scan_simulator.scan_method, fpop, states[:6], 5, 2.0, sim.scan_fov, sim.num_rays,
                                    sim.edge_distances, sim.ttc_thresh, 3, scan_dist_to_base=sim.scan_dist_to_base,
                                    steer_clip=0.4189)
    assert len(got) == 5 and got[4].shape == (2, 2)
    for x, y in zip(got, want):
        assert same_bits(x, y)
