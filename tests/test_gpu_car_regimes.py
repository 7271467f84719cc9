"""Car::control + Car::updatePosition in every kernel that steps a car (rollout_kernel, drive_start_kernel and
drive_tick_kernel with both steering sources, env_step_kernel, race_env_step_kernel, mcts_act_kernel,
mcts_advance_kernel) against the reference's compiled Car, in every regime of the step, for three cars and three time
steps (tests/car_regimes.py; tests/test_car_regimes_host.py checks the inputs).  Every comparison is teacher-forced: the
reference steps from the GPU's own state before the step, to rtol = atol = 1e-9 with state[7] and state[10] exact, and
every kernel's step equals CarBatch.rollout's bit for bit.  All cases run in an empty room where nothing can crash."""
import os

import numpy as np
import pytest

from conftest import GOLD
import car_regimes as CR
import policy_statement as PS
import support
from oracle import reference
from support import FOV, same_bits, within_one_ulp
from pyracecarsimulator_amd import DriveEnv, Policy, RaceEnv, maps, range_libc
from pyracecarsimulator_amd import racecar as RC

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

MRX, T, D = 300, 3, CR.D_SCAN
B_FG, B_NN = 65, 720


class World:
    """The two empty rooms with an RMGPU handle each, one CarBatch per car, the sources."""

    def __init__(self):
        reference.require()
        self.m = range_libc.PyRayMarchingGPU(range_libc.PyOMap(maps.make_room(CR.ROOM_N)), MRX)
        self.m_race = range_libc.PyRayMarchingGPU(range_libc.PyOMap(maps.make_room(CR.RACE_ROOM_N)), MRX)
        self.cars = {name: RC.CarBatch(car) for name, car in CR.CARS.items()}
        layers, relu = PS.load_fixture(os.path.join(GOLD, "policy_mlp720.npz"))
        self.net = Policy.from_arrays(layers, relu, in_start=0)
        self._sub = {}

    def subset(self, name):
        if name not in self._sub:
            self._sub[name] = CR.subset(CR.CARS[name], CR.SEEDS[name])
        return self._sub[name]

    def followgap(self, name):
        return support.followgap(max_angle=CR.CARS[name]["max_steer_ang"])


@pytest.fixture(scope="module")
def world():
    return World()


def edge(car, num_rays):
    return RC.edge_distances(num_rays, -FOV / 2, FOV / num_rays, D, car["width"], car["wb"])


def one_step(cars, before, speeds, steers, dt, n=1):
    """CarBatch.rollout's n steps under one command per row: the project's one model, in one batched call."""
    before = np.ascontiguousarray(before, np.float64).reshape(-1, 11)
    acts = np.stack([np.broadcast_to(np.asarray(speeds, np.float64), (len(before),)),
                     np.broadcast_to(np.asarray(steers, np.float64), (len(before),))], -1)[:, None, :]
    return cars.rollout(before, np.ascontiguousarray(acts), n_steps=n, action_every=n, dt=dt)[1]


def assert_link(world, name, dt, before, speeds, steers, after, what, n=1):
    """``after`` against n reference steps from ``before`` and, bit for bit, against rollout's."""
    CR.assert_steps(after, CR.ref_steps(CR.CARS[name], before, speeds, steers, dt, n), what)
    assert same_bits(one_step(world.cars[name], before, speeds, steers, dt, n), np.asarray(after).reshape(-1, 11)), what


def assert_regimes(reg, least, what):
    counts = reg.sum(0)
    assert (counts >= least).all(), (what, dict(zip(CR.REGIMES, counts.tolist())))


# ---------------------------------------------------------------- 1. rollout_kernel
@pytest.mark.parametrize("name,dt", CR.PAIRS)
def test_rollout_full_grid(world, name, dt):
    car, cars = CR.CARS[name], world.cars[name]
    st, speed, steer = CR.rollout_grid(car, CR.SEEDS[name])
    acts = np.ascontiguousarray(np.stack([speed, steer], -1)[:, None, :])
    poses, final, vel = cars.rollout(st, acts, n_steps=1, action_every=1, dt=dt)
    assert_regimes(CR.regimes(car, st, speed, steer), 900, (name, dt))
    CR.assert_steps(final, CR.ref_steps(car, st, speed, steer, dt), (name, dt))
    assert same_bits(poses[:, 0], final[:, :3].astype(np.float32)) and same_bits(vel[:, 0], final[:, 3])
    # the dead band's edge leaves the steer angle where it was
    assert (final[27648:, 4] == 0.0).all()
    multi = RC.CarBatch(car, device=[0, 0, 0])
    for got, want in zip(multi.rollout(st, acts, n_steps=1, action_every=1, dt=dt), (poses, final, vel)):
        assert same_bits(got, want), (name, dt)


@pytest.mark.parametrize("name,dt", list(zip(CR.CARS, CR.DTS)))
def test_rollout_schedule(world, name, dt):
    """n_steps = 7, action_every = 3 (three commands, the last one held for one step), scripts/mcts.py's schedule."""
    car = CR.CARS[name]
    st, speed, steer = world.subset(name)
    rng = np.random.default_rng(5)
    acts = np.stack([np.stack([speed, steer], -1), np.stack([rng.permutation(speed), rng.permutation(steer)], -1),
                     np.stack([rng.permutation(speed), rng.permutation(steer)], -1)], 1)
    poses, final, vel = world.cars[name].rollout(st, acts, n_steps=7, action_every=3, dt=dt)
    want = np.empty((len(st), 7, 11))
    with reference.RefCar(CR.params(car)) as ref:
        for r in range(len(st)):
            ref.set_state(st[r])
            for i in range(7):
                want[r, i] = ref.step(None, acts[r, i // 3, 0], acts[r, i // 3, 1], dt)
    # free-running, yet no branch can differ: velocity and steer angle, which alone pick the branches, involve no
    # library function and come out bit-equal (neither build contracts a * b + c)
    assert same_bits(vel, want[:, :, 3]) and same_bits(final[:, 4], want[:, 6, 4])
    CR.assert_steps(final, want[:, 6], (name, dt))
    assert within_one_ulp(poses, want[:, :, :3].astype(np.float32))
    assert same_bits(poses[:, 6], final[:, :3].astype(np.float32)) and same_bits(vel[:, 6], final[:, 3])


# ---------------------------------------------------------------- 2. the closed loops
def check_drive(world, name, dt, states, speeds, steer0, drive, clip, what):
    """A traced closed-loop result: no crash, every state from the one before under the steer the GPU reports, the
    velocity trace, the lidar poses at D_SCAN, the states out."""
    car = CR.CARS[name]
    first, final, vel, steers, sp, st = drive
    R = len(states)
    assert (first < 0).all(), (what, np.nonzero(first >= 0)[0][:5])
    assert st.shape == (R, T, 11) and sp.shape == (R, T, 3) and vel.shape == steers.shape == (R, T)
    assert np.isfinite(st).all() and np.isfinite(steers).all()
    before = np.concatenate([states[:, None, :], st[:, :-1]], 1)
    fed = np.concatenate([steer0[:, None], steers[:, :-1]], 1).astype(np.float64)
    if clip is not None:
        fed[:, 1:] = np.clip(fed[:, 1:], -clip, clip)                  # (tick 0's steer0 goes to the car as it is)
    spd = np.repeat(speeds[:, None], T, 1)
    assert_link(world, name, dt, before, spd.ravel(), fed.ravel(), st, what)
    assert same_bits(vel, st[:, :, 3]) and same_bits(final, st[:, -1])
    assert within_one_ulp(CR.ref_scan_poses(car, st, D).astype(np.float32), sp.reshape(-1, 3)), what
    # tick 0 takes the grid's regimes; the rest of the loop adds what the source steers
    assert_regimes(CR.regimes(car, states, speeds, steer0.astype(np.float64)), 100, what)
    return CR.regimes(car, before, spd.ravel(), fed.ravel())


@pytest.mark.parametrize("name,dt", CR.LOOP_PAIRS)
def test_drive_followgap(world, name, dt):
    car = CR.CARS[name]
    states, speeds, steer = world.subset(name)
    steer0 = CR.f32(steer)
    got = world.cars[name].drive_followgap(world.m, world.followgap(name), states, T, speeds, FOV, B_FG,
                                           edge(car, B_FG), car["ttc_thresh"], scan_dist_to_base=D, dt=dt,
                                           steer0=steer0, trace=True)
    check_drive(world, name, dt, states, speeds, steer0, got, None, ("followgap", name, dt))


@pytest.mark.parametrize("name,dt,clip", [("simple", 0.001, None), ("skew", 0.05, 0.3)])
def test_drive_policy(world, name, dt, clip):
    car = CR.CARS[name]
    states, speeds, steer = world.subset(name)
    steer0 = CR.f32(steer)
    got = world.cars[name].drive_policy(world.m, world.net, states, T, speeds, FOV, B_NN, edge(car, B_NN),
                                        car["ttc_thresh"], scan_dist_to_base=D, dt=dt, steer0=steer0, steer_clip=clip,
                                        trace=True)
    check_drive(world, name, dt, states, speeds, steer0, got, clip, ("policy", name, dt, clip))


@pytest.mark.parametrize("group", [1, 2, 8])
def test_race_followgap(world, group):
    """Races of 1, 2 and 8 cars with (skew, 0.05).  The cars of a race do see each other (a car 4 m off is in the
    scan and may move FollowGap's answer), so the rows are not compared with races of one: each is checked against the
    reference and rollout under the steer the GPU reports, as in the drive loops."""
    name, dt = "skew", 0.05
    car = CR.CARS[name]
    states, speeds, steer = world.subset(name)
    races = CR.race_starts(states, group)
    steer0 = CR.f32(steer)
    got = world.cars[name].race_followgap(world.m_race, world.followgap(name), races, T, speeds.reshape(-1, group), FOV,
                                          B_FG, edge(car, B_FG), car["ttc_thresh"], steer0=steer0.reshape(-1, group),
                                          dt=dt, trace=True, scan_dist_to_base=D)
    flat = tuple(a.reshape((-1,) + a.shape[2:]) for a in got)
    check_drive(world, name, dt, races.reshape(-1, 11), speeds, steer0, flat, None, ("race", group))


# ---------------------------------------------------------------- 3. the environments
def env_actions(car, seed, n):
    """(2, n, 2) float32: speed U(-ms-2, ms+2), steer U(-1, 1)."""
    rng = np.random.default_rng(seed)
    ms = car["max_speed"] + 2.0
    return np.stack([rng.uniform(-ms, ms, (2, n)), rng.uniform(-1.0, 1.0, (2, n))], -1).astype(np.float32)


def check_env(world, name, dt, env, starts, actions, clip, what):
    """reset on pool row e for env e, then one step per (n, 2) float32 row of ``actions``: every env runs before and
    after, its state is substeps reference steps (and rollout's bits) from the state before under the clamped steer,
    and its reward the float32 of the distance it added.  Returns the regime counts of each step."""
    car, race = CR.CARS[name], isinstance(env, RaceEnv)
    n, S = env.n_envs, env.params.substeps
    env.reset(start_index=np.arange(env.n_races if race else n))
    rd = env.read()
    assert same_bits(rd["states"].reshape(-1, 11), starts.reshape(-1, 11)) and (rd["done"] == 0).all(), what
    seen = []
    for k, a in enumerate(actions):
        before = env.read()["states"].reshape(-1, 11)
        _, rew, done = env.step(a.reshape(env.n_races, env.group, 2) if race else a)
        after = env.read()["states"].reshape(-1, 11)
        assert (done == 0).all(), (what, k)
        spd, fed = a[:, 0].astype(np.float64), a[:, 1].astype(np.float64)
        if clip > 0:
            fed = np.clip(fed, -clip, clip)
        assert_link(world, name, dt, before, spd, fed, after, (what, k), n=S)
        assert same_bits(rew.reshape(-1), (after[:, 8] - before[:, 8]).astype(np.float32)), (what, k)
        seen.append(CR.regimes(car, before, spd, fed).sum(0))
    return seen


def run_envs(world, name, dt, clip, make, starts):
    """One step of substeps = 1 with the grid's commands as float32 actions, then two steps of substeps = 3 with seeded
    actions.  An env has one substeps for life, so the second part is a second env whose start pool is the first one's
    states after its step."""
    car = CR.CARS[name]
    _, speed, steer = world.subset(name)
    what = ("races" if starts.ndim == 3 else "envs", name, dt, clip)
    one = make(starts, 1)
    seen = check_env(world, name, dt, one, starts, [np.stack([CR.f32(speed), CR.f32(steer)], -1)], clip, what + (1,))
    assert (seen[0] >= 100).all(), dict(zip(CR.REGIMES, seen[0].tolist()))
    mid = one.read()["states"]
    check_env(world, name, dt, make(mid, 3), mid, env_actions(car, 7, one.n_envs), clip, what + (3,))


@pytest.mark.parametrize("clip", [0.3, 0.0])
@pytest.mark.parametrize("name,dt", CR.LOOP_PAIRS)
def test_drive_env(world, name, dt, clip):
    car = CR.CARS[name]
    states = world.subset(name)[0]
    run_envs(world, name, dt, clip, lambda pool, S: DriveEnv(
        world.m, pool, len(pool), B_FG, FOV, edge(car, B_FG), car["ttc_thresh"], substeps=S, auto_reset=False,
        steer_clip=clip, car=world.cars[name], dt=dt, scan_dist_to_base=D), states)


@pytest.mark.parametrize("clip", [0.3, 0.0])
@pytest.mark.parametrize("name,dt", CR.LOOP_PAIRS)
def test_race_env(world, name, dt, clip):
    car = CR.CARS[name]
    races = CR.race_starts(world.subset(name)[0], 4, CR.ENV_PITCH)
    run_envs(world, name, dt, clip, lambda pool, S: RaceEnv(
        world.m_race, pool, len(pool), B_FG, FOV, edge(car, B_FG), car["ttc_thresh"], substeps=S, auto_reset=False,
        steer_clip=clip, car=world.cars[name], dt=dt, scan_dist_to_base=D, min_running=1), races)


# ---------------------------------------------------------------- 4. the planner
MCTS_DT, MCTS_L, MCTS_EVERY, MCTS_IT, MCTS_K = 0.05, 10, 5, 8, 16


@pytest.mark.parametrize("source", ["fg", "random"])
def test_mcts_act_links(world, source):
    name = "skew"
    car, cars = CR.CARS[name], world.cars[name]
    states = world.subset(name)[0]
    roots = states[CR.mcts_roots(car, states, MCTS_K)]
    seeds = np.arange(1, MCTS_K + 1, dtype=np.uint64) * np.uint64(2654435761)
    seen = np.zeros(13, int)
    for speed in CR.mcts_speeds(car):
        res = cars.plan_mcts(world.m, world.followgap(name) if source == "fg" else None, roots, MCTS_IT, seeds, FOV,
                             B_FG, edge(car, B_FG), car["ttc_thresh"], root_actions=0.1, source=source,
                             rollout_steps=MCTS_L, action_every=MCTS_EVERY, speed=speed, dt=MCTS_DT,
                             scan_dist_to_base=D, trees=True)
        trees, held = res[3], CR.decoded(car, roots)                   # (the planner stores the roots decoded)
        before, after, acts, poses = [], [], [], []
        for k, t in enumerate(trees):
            assert len(t["parent"]) == MCTS_IT + 1 and same_bits(t["state"][0], held[k])
            before.append(t["state"][t["parent"][1:]])
            after.append(t["state"][1:])
            acts.append(t["action"][1:])
            poses.append(t["scan_pose"])
        before, after, acts = np.concatenate(before), np.concatenate(after), np.concatenate(acts)
        assert np.isfinite(acts).all()
        assert_link(world, name, MCTS_DT, before, speed, acts, after, (source, speed))
        all_states = np.concatenate([t["state"] for t in trees])
        assert within_one_ulp(CR.ref_scan_poses(car, all_states, D).astype(np.float32), np.concatenate(poses))
        seen += CR.regimes(car, before, speed, acts).sum(0)
    # the roots take every acceleration and model regime whatever is drawn; the steering regime depends on the drawn
    # action: U(-0.41, 0.41) takes both directions from roots that span the steering range, FollowGap's answers need
    # not, and no drawn action meets the dead band
    print(source, dict(zip(CR.REGIMES, seen.tolist())))
    assert (np.delete(seen, [6, 7, 8]) > 0).all(), dict(zip(CR.REGIMES, seen.tolist()))
    assert source != "random" or (seen[7] > 0 and seen[8] > 0), seen


@pytest.mark.parametrize("source", ["fg", "random"])
def test_mcts_drive(world, source):
    """2 decisions of 3 steps: mcts_advance_kernel drives the car with the raw best action (steer_clip bounds the next
    recent action only, as the reference's driver does)."""
    name, clip, S, n_dec = "skew", 0.3, 3, 2
    car, cars = CR.CARS[name], world.cars[name]
    states = world.subset(name)[0]
    roots = np.ascontiguousarray(states[CR.mcts_roots(car, states, MCTS_K)])
    seeds = np.arange(1, MCTS_K + 1, dtype=np.uint64) * np.uint64(40503)
    for speed in CR.mcts_speeds(car):
        first, out, recent, actions, visits, trace = cars.drive_mcts(
            world.m, world.followgap(name) if source == "fg" else None, roots, n_dec, MCTS_IT, seeds, FOV, B_FG,
            edge(car, B_FG), car["ttc_thresh"], recent_actions=0.1, source=source, steps_per_decision=S,
            steer_clip=clip, rollout_steps=MCTS_L, action_every=MCTS_EVERY, speed=speed, dt=MCTS_DT,
            scan_dist_to_base=D, trace=True)
        assert (first < 0).all() and np.isfinite(actions).all()
        assert same_bits(CR.decoded(car, trace[:, 0]), CR.decoded(car, roots))
        after = np.concatenate([trace[:, 1:], out[:, None, :]], 1)
        assert_link(world, name, MCTS_DT, trace, speed, actions.ravel(), after, (source, speed), n=S)
        assert same_bits(recent, np.clip(actions[:, -1], -clip, clip))
