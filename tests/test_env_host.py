"""The driving environment's host side (no GPU): the spawn draw against the planner's uniform, the statement's state
machine (tests/env_statement.py) on a fake one-dimensional world, and DriveEnv's argument checks."""
import ctypes as C

import numpy as np
import pytest

import env_statement as E
from mcts_statement import uniform01
from pyracecarsimulator_amd import _lib
from pyracecarsimulator_amd import env as ENV


# ---------------------------------------------------------------- the spawn draw
def test_spawn_draw_known_answers():
    # (seed, e, q): the 53-bit uniform of Philox-2x32-10 under noise_key(seed) at counter (e, q)
    known = [(0, 0, 0, 0.9965466469118988), (0, 1, 0, 0.8627457817485537), (7, 3, 2, 0.95016302505178),
             ((3 << 32) | 5, 69, 11, 0.8783800800656895), (1, 0, 1, 0.4953983371440527)]
    for seed, e, q, u in known:
        assert float(uniform01(seed, np.uint64(e), np.uint64(q))) == u
        for M in (1, 2, 3, 5, 7, 1000, 123457):
            assert E.spawn_index(seed, e, q, M) == min(M - 1, int(u * float(M))), (seed, e, q, M)
    assert E.spawn_index((3 << 32) | 5, 69, 11, 1000) == 878
    assert E.spawn_index(1, 0, 1, 1) == 0 and E.spawn_index(0, 0, 0, 5) == 4 and E.spawn_index(1, 0, 1, 5) == 2
    # u close to 1: the last pool row, never M
    u = float(uniform01(9, np.uint64(160461), np.uint64(4)))
    assert u == 0.9999943935200177
    assert E.spawn_index(9, 160461, 4, 100000) == 99999
    assert E.spawn_index(9, 160461, 4, 3) == 2


def test_spawn_draw_never_leaves_the_pool(monkeypatch):
    # the min(M-1, .) guard: even u = 1.0 (one past the largest draw, 1 - 2^-53) stays inside
    for u in (1.0 - 2.0 ** -53, 1.0):
        monkeypatch.setattr(E, "uniform01", lambda seed, d, i, u=u: np.float64(u))
        for M in (1, 3, (1 << 31) - 1):
            assert E.spawn_index(0, 0, 0, M) == M - 1
    monkeypatch.setattr(E, "uniform01", lambda seed, d, i: np.float64(0.0))
    assert E.spawn_index(0, 0, 0, 9) == 0


def test_spawn_draws_cover_the_pool():
    e = np.arange(4000, dtype=np.uint64)
    u = uniform01(5, e, np.zeros(e.size, np.uint64))
    idx = np.array([E.spawn_index(5, int(i), 0, 5) for i in e[:4000]])
    assert (idx == np.minimum(4, (u * 5.0).astype(np.int64))).all()
    assert np.bincount(idx, minlength=5).min() > 600          # uniform over the five rows


# ---------------------------------------------------------------- the state machine on a 1-D world
WALL, B, EDGE, THRESH = 10.0, 10, 0.5, 0.001


class World1D:
    """x along a corridor towards a wall at WALL: a step moves speed / 10, every beam reads WALL - x."""

    def __init__(self):
        self.slots = []

    def step_cars(self, states, speed, steer):
        out = states.copy()
        dx = speed * 0.1
        out[:, 0] += dx
        out[:, 4] = steer                                      # (what the clamp let through)
        out[:, 8] += np.abs(dx)
        return out

    def scan(self, poses, k):
        self.slots.append(k)
        return np.repeat((np.float32(WALL) - poses[:, 0])[:, None], B, 1).astype(np.float32)

    @staticmethod
    def is_crashed(r):
        return bool(((r.astype(np.float64) - EDGE) < THRESH).any())


def _env(starts, n, world, **kw):
    return E.EnvStatement(starts, n, B, world.step_cars, world.scan, world.is_crashed, scan_dist_to_base=0.0, **kw)


def _start(x):
    s = np.zeros(11)
    s[0] = x
    return s


def test_statement_reaches_every_done_code_in_order():
    w = World1D()
    # env 0 far from the wall, env 1 crashes on its 4th step (= max_ticks: reads 1, not 2), env 2 starts inside the
    # margin, env 3 gets a NaN action at step 2, env 4 an inf one at step 1
    starts = np.stack([_start(0.0), _start(7.6), _start(9.8), _start(1.0), _start(2.0)])
    env = _env(starts, 5, w, max_ticks=4, auto_reset=False, crash_reward=-3.0, steer_clip=0.25)
    obs, done = env.reset(seed=1, start_index=np.arange(5))
    assert done.tolist() == [0, 0, 1, 0, 0] and obs.shape == (5, B) and obs.dtype == np.float32
    assert obs[1, 0] == np.float32(WALL) - np.float32(7.6)
    a = np.tile(np.float32([5.0, 0.9]), (5, 1))
    seen = []
    for k in range(1, 7):
        act = a.copy()
        if k == 2:
            act[3, 1] = np.nan
        if k == 1:
            act[4, 0] = np.inf
        before = env.states.copy()
        obs, rew, done = env.step(act)
        seen.append(done.tolist())
        if k == 1:
            assert done.tolist() == [0, 0, 1, 0, 3]
            assert rew.tolist() == [0.5, 0.5, 0.0, 0.5, -3.0]          # frozen 0, invalid crash_reward
            assert (env.states[4] == before[4]).all() and env.tick.tolist() == [1, 1, 0, 1, 0]
            assert env.states[0, 4] == 0.25                           # the steer was clamped to +-steer_clip
        if k == 2:
            assert done.tolist() == [0, 0, 1, 3, 3] and rew[3] == np.float32(-3.0) and rew[4] == 0.0
            assert (env.states[3] == before[3]).all()
        if k == 4:
            # both on tick 4 = max_ticks: env 0 truncates (and keeps its distance), env 1 crashed: 1 wins over 2
            assert done.tolist() == [2, 1, 1, 3, 3]
            assert rew[0] == np.float32(0.5) and rew[1] == np.float32(-3.0)
        if k > 4:
            # everything is frozen: nothing changes, rewards 0, yet every env is scanned again at this slot
            assert done.tolist() == [2, 1, 1, 3, 3] and (rew == 0).all()
            assert (env.states == before).all() and env.tick.tolist() == [4, 4, 0, 1, 0]
            assert obs[0, 0] == np.float32(WALL - 2.0)
    assert w.slots == list(range(7))                                   # the reset is slot 0
    assert {c for row in seen for c in row} == {0, 1, 2, 3}
    assert env.episode.tolist() == [0] * 5


def test_statement_auto_reset_is_fresh_for_one_call():
    w = World1D()
    starts = np.stack([_start(0.0), _start(9.0), _start(9.8)])
    env = _env(starts, 3, w, max_ticks=3, auto_reset=True, crash_reward=-1.0)
    env.reset(seed=4, start_index=[0, 1, 2])
    a = np.tile(np.float32([5.0, 0.0]), (3, 1))
    # step 1: env 2 (done at the reset) re-spawns: fresh, action ignored, tick 0, episode 1, drawn start
    obs, rew, done = env.step(a)
    want = E.spawn_index(4, 2, 1, 3)
    assert env.episode.tolist() == [0, 0, 1] and env.tick.tolist() == [1, 1, 0]
    assert env.start_index[2] == want and (env.states[2] == starts[want]).all()
    # a fresh env spawned inside the margin is done = 1 at once; a fresh env's reward is 0 either way
    assert done[2] == (1 if want == 2 else 0) and rew[2] == 0.0
    assert rew[0] == np.float32(0.5) and done[1] == 1 and rew[1] == np.float32(-1.0)   # 9.5: inside the margin
    # step 2: env 1 re-spawns
    obs, rew, done = env.step(a)
    want1 = E.spawn_index(4, 1, 1, 3)
    assert env.episode[1] == 1 and env.tick[1] == 0 and env.start_index[1] == want1
    assert rew[1] == 0.0 and done[1] == (1 if want1 == 2 else 0)
    assert obs[1, 0] == np.float32(WALL) - np.float32(starts[want1, 0])
    # step 3: env 0 truncates at tick 3; step 4: it re-spawns with q = 1
    obs, rew, done = env.step(a)
    assert done[0] == 2 and env.tick[0] == 3 and rew[0] == np.float32(0.5)
    obs, rew, done = env.step(a)
    assert env.episode[0] == 1 and env.tick[0] == 0 and rew[0] == 0.0
    assert env.start_index[0] == E.spawn_index(4, 0, 1, 3)


def test_statement_observation_window_and_input_form():
    r = np.arange(2 * 20, dtype=np.float32).reshape(2, 20)
    r[1, 9] = np.nan
    r[1, 11] = np.inf
    o = E.observation(r, (3, 5, 2), 0.0, 0.0)
    assert o.tobytes() == r[:, [3, 5, 7, 9, 11]].tobytes()
    o = E.observation(r, (3, 5, 2), 15.0, 15.0)
    assert o[0].tolist() == [np.float32(3) / np.float32(15), np.float32(5) / np.float32(15), np.float32(7) / np.float32(15),
                             np.float32(9) / np.float32(15), np.float32(11) / np.float32(15)]
    assert o[1].tolist() == [1.0] * 5                                  # > clip, NaN and inf read 1.0


def test_statement_refuses_a_step_before_reset_and_bad_indices():
    w = World1D()
    env = _env(np.stack([_start(0.0)]), 2, w)
    with pytest.raises(RuntimeError):
        env.step(np.zeros((2, 2), np.float32))
    with pytest.raises(ValueError):
        env.reset(0, start_index=[0, 1])


# ---------------------------------------------------------------- DriveEnv's argument checks
def test_env_params_layout_matches_the_header():
    # 10 four-byte fields, five doubles, one float, padded to the doubles' alignment
    assert C.sizeof(_lib.EnvParams) == 88
    assert _lib.EnvParams.dt.offset == 40 and _lib.EnvParams.fov.offset == 80
    names = [n for n, _ in _lib.EnvParams._fields_]
    assert names == ["n_envs", "substeps", "num_rays", "obs_start", "obs_count", "obs_stride", "obs_clip", "obs_scale",
                     "max_ticks", "auto_reset", "dt", "scan_dist_to_base", "crash_thresh", "steer_clip", "crash_reward",
                     "fov"]


def test_drive_env_argument_checks():
    starts = np.zeros((3, 11))
    edge = np.zeros(100)
    st, ed, win = ENV.env_args(70, 100, starts, edge)
    assert win == (0, 100, 1) and st.shape == (3, 11) and ed.shape == (100,)
    assert ENV.env_args(70, 100, starts, edge, obs_window=(7, 40, 2))[2] == (7, 40, 2)
    assert ENV.env_args(1, 100, starts, edge, obs_window=(99, 1, 5))[2] == (99, 1, 5)
    bad = [dict(n_envs=0), dict(n_envs=2.5), dict(num_rays=9), dict(num_rays=1281), dict(substeps=0), dict(substeps=513),
           dict(max_ticks=-1), dict(obs_window=(7, 48, 2)), dict(obs_window=(-1, 4, 1)), dict(obs_window=(0, 0, 1)),
           dict(obs_window=(0, 4, 0)), dict(obs_window=(0, 4)), dict(steer_clip=-0.1), dict(steer_clip=float("nan")),
           dict(obs_clip=-1), dict(obs_scale=float("nan")), dict(crash_reward=float("nan")), dict(dt=float("inf")),
           dict(starts=starts.astype(np.float32)), dict(starts=np.zeros((0, 11))), dict(starts=np.zeros(11)),
           dict(edge=edge[:-1]), dict(edge=edge.astype(np.float32)), dict(n_envs=(1 << 31) // 100 + 1)]
    for kw in bad:
        args = dict(n_envs=70, num_rays=100, starts=starts, edge=edge)
        args.update(kw)
        with pytest.raises(ValueError):
            ENV.env_args(**args)
    nf = starts.copy()
    nf[1, 4] = np.inf
    with pytest.raises(ValueError):
        ENV.env_args(70, 100, nf, edge)


def test_package_exports_the_environment():
    import pyracecarsimulator_amd as P
    assert P.DriveEnv is ENV.DriveEnv and "DriveEnv" in P.__all__
    assert hasattr(P.RacecarSimulator, "driveEnv")
    for name in ("rl_env_create", "rl_env_destroy", "rl_env_reset", "rl_env_step", "rl_env_reset_device",
                 "rl_env_step_device", "rl_env_read"):
        assert name in _lib.SYMBOLS and getattr(_lib.lib(), name) is not None
