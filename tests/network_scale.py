"""Cases of the network, seat and track-plan kernels past one block of work (tests/test_gpu_network_scale.py on the
GPU, tests/test_network_scale_host.py and the census tools on the CPU): the shapes, the case builders and the censuses
every case has to show.  The censuses are counted from the statements alone (tests/population_statement.py,
tests/seat_statement.py): on the CPU over the oracle's scan and the compiled reference Car, on the GPU over the public
calls.  docs/history/network_scale.md records the CPU output.  No tests live here."""
import numpy as np

import drive_cases as DC
import policy_statement as S
import population_statement as PS
import race_statement as RS
import seat_statement as SS
import support
import test_gpu_population as TP
from support import FOV, MAX_STEER, THRESH
from test_gpu_race_env import CASE3, _race_starts

# ---------------------------------------------------------------- A1. the pack launch (abi_car.hip pop_pack_launch)
PACK_THREADS, PACK_GRID_CAP = 256, 65536       # one thread a value, the grid capped: past their product the loop wraps
PACK = dict(members=220, first=3, n=215, control_n=211)


def pack_wrap(n_params):
    """(the values one trip of the grid covers, the call-member the second trip starts in, its parameter there)."""
    trip = PACK_THREADS * PACK_GRID_CAP
    return trip, trip // n_params, trip % n_params


def pack_thetas(n, n_params, seed=5):
    """float32 (n, P), member by member from its own seeded generator, scaled small."""
    out = np.empty((n, n_params), np.float32)
    for m in range(n):
        out[m] = (0.05 * np.random.default_rng(1000 * seed + m).standard_normal(n_params)).astype(np.float32)
    return out


# ---------------------------------------------------------------- A2. the evaluation grid
#: (network, members, cars per member): 3 workgroups a member with 1 car of 8 in the last, and 130 of one car
EVAL = [("small", 67, 17), ("odd", 67, 17), ("small", 130, 1), ("odd", 130, 1)]
SUB = dict(first=60, n=7)                      # a sub-range across member 64


# ---------------------------------------------------------------- A3. the roll-out and its fitness
#: members x cars, seeds of the far (clear 8 px) and near (clear 1 px) starts, of the permutation that spreads them
#: over the members, of the travel_dist so far and of the networks: picked on the CPU (tools/population_census.py)
ROLLOUTS = {
    (67, 3): dict(far_seed=41, near_seed=42, order_seed=3, dist_seed=4, net_seed=1, gain=4.0),
    (130, 1): dict(far_seed=43, near_seed=44, order_seed=5, dist_seed=6, net_seed=1, gain=4.0),
}
ROLLOUT_B, ROLLOUT_T = 64, 25


def rollout_starts(g, dt, cfg, n, E):
    """(states (n E, 11), speeds (n E,)): test_gpu_population.rollout_starts' recipe (3 in 5 in the open, 2 in 5 a cell
    from a wall) drawn per car and shuffled, so that every member gets its own mix; travel_dist so far of every size, so
    that the order of the fitness sum shows in its bits."""
    N = n * E
    n_far = (3 * N + 4) // 5
    far, sp_far = support.starts(g, dt, n_far, cfg["far_seed"], 8.0)
    near, sp_near = support.starts(g, dt, N - n_far, cfg["near_seed"], 1.0)
    order = np.random.default_rng(cfg["order_seed"]).permutation(N)
    states, speeds = np.concatenate([far, near])[order], np.concatenate([sp_far, sp_near])[order]
    states[:, 8] = 10.0 ** np.random.default_rng(cfg["dist_seed"]).uniform(-6.0, 3.0, N)
    return states, speeds


def rollout_census(first, steers, fit, n, E, clip):
    """What a roll-out case has to show, from (first_crashed (n E,), steers (n E, T), fitness (n, 2))."""
    first, steers, fit = np.asarray(first), np.asarray(steers), np.asarray(fit)
    hi = first[64 * E:]
    ok = np.isfinite(steers)
    return dict(fitness_distinct=len({v.tobytes() for v in fit[:, 0]}) == n,
                crash_past_64=bool((hi >= 0).any()), finish_past_64=bool((hi < 0).any()),
                crash_counts=len(set(fit[:, 1].tolist())) >= 2,
                beyond_clip=bool((np.abs(steers[ok]) > clip).any()))


class PopWorld:
    """The population statement's callbacks from the oracle and the reference Car (noise off)."""

    def __init__(self, oracle_mod, ref_mod, g, name, B, layer_lists):
        self.O, self.B, self.edge = oracle_mod, B, support.oracle_edge(oracle_mod, B)
        self.car = ref_mod.RefCar()
        self.om = oracle_mod.OracleMap(g.occ, g.resolution, g.origin, TP.MRX)
        dims, self.in_start, relu, _ = TP.NETS[name]
        self.relu = relu or tuple(i < len(dims) - 2 for i in range(len(dims) - 1))
        self.members = layer_lists

    def step_cars(self, states, speed, steer):
        return np.stack([self.car.step(s, v, a) for s, v, a in zip(states, speed, steer)])

    def scan(self, poses, cars, t):
        return self.om.rm_fan(np.ascontiguousarray(poses, np.float32), FOV, self.B, step_coeff=1.0)[0].reshape(-1, self.B)

    def is_crashed(self, r):
        return self.O.is_crashed(np.ascontiguousarray(r), self.B, 1, self.edge, THRESH) >= 0

    def answer(self, member, row):
        return S.forward(row[None], self.members[member], self.relu, in_start=self.in_start)[0]


def rollout_cpu(oracle_mod, ref_mod, g, dt, n, E, cfg=None):
    """The statement of roll-out case (n, E) on the CPU: (first, final, steers, trace, fitness)."""
    cfg = cfg or ROLLOUTS[(n, E)]
    states, speeds = rollout_starts(g, dt, cfg, n, E)
    w = PopWorld(oracle_mod, ref_mod, g, "small", ROLLOUT_B, TP.members("small", n, cfg["net_seed"], cfg["gain"]))
    return PS.population_rollout(states, speeds, np.zeros(n * E, np.float32), ROLLOUT_T, 0, E, TP.CLIP, w.step_cars,
                                 w.scan, w.is_crashed, w.answer)


# ---------------------------------------------------------------- B. seats
SEAT_CLIP = 0.2
#: name -> the seated env's shape: CASE3's 23 x 3 = 69 cars (race 21 = cars 63, 64, 65 straddles the 64-lane blocks)
#: and 9 x 8 = 72 (race 8 = cars 64 ... 71); `watch` is the race that has to finish and re-spawn inside the run; pool
#: seeds and speeds picked on the CPU (tools/seats_census.py)
SEAT_ENVS = {
    "pfp": dict(R=CASE3["R"], P=CASE3["P"], B=CASE3["B"], mix="pfp", M=5, pool_seed=55, seed=1, watch=21, steps=12,
                speed=(5.5, 6.0, 6.5)),
    "pfc": dict(R=CASE3["R"], P=CASE3["P"], B=CASE3["B"], mix="pfc", M=5, pool_seed=55, seed=1, watch=21, steps=12,
                speed=(5.5, 6.0, 0.0)),
    "pfpppfpf": dict(R=9, P=8, B=65, mix="pfpppfpf", M=4, pool_seed=58, seed=1, watch=7, steps=12,
                     speed=(5.5, 6.0, 6.5, 5.0, 5.5, 6.0, 6.5, 5.0)),
}
SEAT_ENV_KW = dict(min_running=2, max_ticks=5, auto_reset=True, crash_reward=-2.5, steer_clip=SEAT_CLIP,
                   substeps=CASE3["S"])
SEAT_WINDOW = dict(obs_window=(5, 40, 1), obs_clip=15.0, obs_scale=15.0)
SEAT_CLEAR_PX = 9.0                            # starts 0.45 m from a wall: some cars reach one within the 12 steps


def seat_pool(g, dt, case):
    """(M, P, 11) line-ups clear of the crash margin, under way at 3 m/s."""
    pool, _ = _race_starts(g, dt, case["M"], case["P"], case["pool_seed"], clear_px=SEAT_CLEAR_PX)
    pool[:, :, 3] = 3.0
    return pool


def seat_actions(case):
    """(steps, N, 2) float32: NaN in every scripted seat's rows, seeded pairs in the caller's."""
    R, P = case["R"], case["P"]
    a = DC.actions(77, case["steps"], R * P).reshape(case["steps"], R, P, 2)
    for k, c in enumerate(case["mix"]):
        if c != "c":
            a[:, :, k, :] = np.nan
    return a.reshape(case["steps"], R * P, 2)


def seat_statement(case, pool, step_cars, scan, is_crashed, answer, drivers):
    """drivers: {"p": ..., "f": ...}: whatever ``answer`` takes for the policy and the FollowGap seats."""
    kw = {k: v for k, v in SEAT_ENV_KW.items() if k != "substeps"}
    seats = [None if c == "c" else drivers[c] for c in case["mix"]]
    return SS.SeatEnvStatement(pool, case["R"], case["B"], step_cars, scan, is_crashed, answer, seats, case["speed"],
                               scan_dist_to_base=support.D_BASE, **SEAT_WINDOW, **kw), seats


class SeatCensus:
    """What a seated env run has to show among the cars past the first 64-lane block, counted from the statement."""

    def __init__(self, stmt, case):
        self.stmt, self.case = stmt, case
        N, P = case["R"] * case["P"], case["P"]
        self.hi = np.arange(N) >= 64
        self.scripted = np.array([case["mix"][e % P] != "c" for e in range(N)])
        self.policy = np.array([case["mix"][e % P] == "p" for e in range(N)])
        self.seen = dict(scripted_crash_past_64=0, respawn_past_64=0, clamped_past_64=0, watch_respawned=0, bad=0)

    def before(self):
        st, P = self.stmt, self.case["P"]
        self.running = (st.done == 0) & np.repeat(st.race_over == 0, P)
        self.episodes = st.race_episode.copy()
        with np.errstate(invalid="ignore"):
            self.seen["clamped_past_64"] += int((self.running & self.policy & self.hi & (np.abs(st.steers) > SEAT_CLIP)).sum())

    def after(self, done):
        st, P = self.stmt, self.case["P"]
        done = np.asarray(done).reshape(-1)
        self.seen["scripted_crash_past_64"] += int((self.running & self.scripted & self.hi & (done == 1)).sum())
        self.seen["bad"] += int((done == 3).sum())
        again = st.race_episode > self.episodes
        self.seen["respawn_past_64"] += int((np.repeat(again, P) & self.hi).sum())
        self.seen["watch_respawned"] += int(again[self.case["watch"]])

    def ok(self):
        s = self.seen
        return bool(s["scripted_crash_past_64"] and s["respawn_past_64"] and s["clamped_past_64"] and s["watch_respawned"]
                    and not s["bad"])


LENGTH, WIDTH = 0.4064, 0.2032


class SeatWorld:
    """The seat statements' callbacks from the oracle's stamped-grid scan, the reference Car, the oracle's FollowGap
    and the network's host statement (noise off)."""

    def __init__(self, oracle_mod, ref_mod, g, group, B, layers, substeps=1):
        self.O, self.g, self.P, self.B, self.S = oracle_mod, g, group, B, substeps
        self.edge = support.oracle_edge(oracle_mod, B)
        self.car = ref_mod.RefCar()
        self.layers, self.relu = layers, [True, True, False]

    def step_cars(self, states, speed, steer):
        return np.stack([self.car.step(s, v, a, n=self.S) for s, v, a in zip(states, speed, steer)])

    def scan(self, poses, cars, k):
        g = self.g
        cells = RS.outline_cells(cars, LENGTH, WIDTH, g.resolution, g.origin, g.rows, g.cols, self.O.sincosf)
        r = DC.race_oracle_fan(self.O, g, cells, self.P, np.ascontiguousarray(poses, np.float32), self.B, False, 1.0)[0]
        return r.reshape(-1, self.B)

    def is_crashed(self, r):
        return self.O.is_crashed(np.ascontiguousarray(r), self.B, 1, self.edge, THRESH) >= 0

    def answer(self, driver, row):
        if driver == "f":
            return np.float32(self.O.followgap_eval(np.ascontiguousarray(row), 15.0, MAX_STEER, 0.004))
        return S.forward(row[None], self.layers, self.relu, in_start=5)[0]


def seat_env_cpu(oracle_mod, ref_mod, g, dt, case, layers):
    """The seated env of ``case`` on the CPU: its census dict."""
    w = SeatWorld(oracle_mod, ref_mod, g, case["P"], case["B"], layers, SEAT_ENV_KW["substeps"])
    stmt, _ = seat_statement(case, seat_pool(g, dt, case), w.step_cars, w.scan, w.is_crashed, w.answer,
                             {"p": "p", "f": "f"})
    census = SeatCensus(stmt, case)
    stmt.reset(case["seed"])
    for a in seat_actions(case):
        census.before()
        _, _, done = stmt.step(a)
        census.after(done)
    return census


#: the seated roll-outs: (races, cars a race, beams, mixed seats, seed of the starts)
SEAT_ROLLOUTS = [(23, 3, 64, "pfp", 52), (9, 8, 65, "pfpppfpf", 58)]
SEAT_ROLLOUT_T = 40


# ---------------------------------------------------------------- C. the track plan
TRACK_R, TRACK_L = (64, 65, 130), 24


def track_cars(T, at_arc, n, L, every, seed):
    """test_gpu_mcts_track.cars_on with the starts and the actions drawn per roll-out and ``every`` steps an action."""
    rng = np.random.default_rng(seed)
    st = np.zeros((n, 11))
    for e in range(n):
        st[e, :3] = at_arc(T, T["L"] * (e + 0.37) / n, rng.uniform(-0.4, 0.4))
        st[e, 2] += rng.uniform(-0.3, 0.3)
        st[e, 3] = rng.uniform(1.0, 3.0)
    st[n - 1, :2] += (3.0, -2.5)
    n_act = (L + every - 1) // every
    act = np.stack([rng.uniform(1.0, 6.0, (n, n_act)), rng.uniform(-0.4, 0.4, (n, n_act))], -1)
    return st, act


TREES = dict(K=65, I=3, L=8, B=64, window=3, base=777, seed=31)
