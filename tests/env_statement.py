"""Host statement of the driving environment (include/scanlib.h, "the driving environment"; rl_env_*): the state
machine of reset and step in plain Python over three callbacks, and the spawn draw.  It is the second statement of
that header section; the GPU tests drive it with the composed public calls (CarBatch.rollout, calc_range_fan,
is_crashed), the host tests with a fake one-dimensional world.

Callbacks:
  step_cars(states float64 (n, 11), speed float64 (n,), steer float64 (n,)) -> states (n, 11) after the env's
      `substeps` car steps (the callback owns substeps and dt)
  scan(poses float32 (N, 3), k) -> ranges float32 (N, B): all N lidar poses at slot k's ray offset,
      base + (k N + e) B (the callback owns the base and the noise)
  is_crashed(ranges float32 (B,)) -> bool: Car::isCrashed on one scan
"""
import numpy as np

from mcts_statement import uniform01
from support import lidar_poses

RUNNING, CRASHED, TRUNCATED, BAD_ACTION = 0, 1, 2, 3


def spawn_index(seed, e, q, n_starts):
    """Env e's start of episode q: min(M-1, (int)(U(e, q) * (double)M)), U the planner's 53-bit uniform."""
    u = float(uniform01(seed, np.uint64(e), np.uint64(q)))
    return min(int(n_starts) - 1, int(u * float(n_starts)))


def observation(ranges, window, obs_clip, obs_scale):
    """Rows of scans -> rows of observations: beams start + i stride, raw or (r <= clip) ? r / scale : 1 in f32."""
    start, count, stride = window
    r = np.asarray(ranges, np.float32)[:, start:start + (count - 1) * stride + 1:stride]
    if not obs_scale > 0:
        return np.ascontiguousarray(r)
    with np.errstate(invalid="ignore"):
        return np.where(r <= np.float32(obs_clip), r / np.float32(obs_scale), np.float32(1.0)).astype(np.float32)


class EnvStatement:
    def __init__(self, starts, n_envs, num_rays, step_cars, scan, is_crashed, obs_window=None, obs_clip=0.0,
                 obs_scale=0.0, max_ticks=0, auto_reset=True, steer_clip=0.0, crash_reward=0.0, scan_dist_to_base=0.275):
        self.starts = np.array(starts, np.float64).reshape(-1, 11)
        self.M, self.N, self.B = self.starts.shape[0], int(n_envs), int(num_rays)
        self.step_cars, self.scan, self.is_crashed = step_cars, scan, is_crashed
        self.window = (0, self.B, 1) if obs_window is None else tuple(obs_window)
        self.obs_clip, self.obs_scale = obs_clip, obs_scale
        self.max_ticks, self.auto_reset = int(max_ticks), bool(auto_reset)
        self.steer_clip, self.crash_reward = float(steer_clip), float(crash_reward)
        self.d_base = scan_dist_to_base
        self.k = None                                   # calls since the reset (None: no reset yet)

    def _spawn(self, e, q, given=None):
        idx = int(given[e]) if given is not None else spawn_index(self.seed, e, q, self.M)
        if not 0 <= idx < self.M:
            raise ValueError("start_index outside [0, M)")
        self.states[e] = self.starts[idx]
        self.tick[e], self.episode[e], self.start_index[e], self.done[e] = 0, q, idx, RUNNING

    def _observe(self, stepped, fresh, invalid, moved):
        """The scan of slot k and phase B; returns (obs, reward)."""
        N = self.N
        ranges = np.asarray(self.scan(lidar_poses(self.states, self.d_base), self.k), np.float32).reshape(N, self.B)
        self.ranges = ranges
        reward = np.zeros(N, np.float32)
        for e in range(N):
            hit = bool(self.is_crashed(ranges[e]))
            if (stepped[e] or fresh[e]) and hit:
                self.done[e] = CRASHED
            elif stepped[e] and self.max_ticks > 0 and self.tick[e] == self.max_ticks:
                self.done[e] = TRUNCATED
            if stepped[e]:
                reward[e] = np.float32(self.crash_reward if self.done[e] == CRASHED else moved[e])
            elif invalid[e]:
                reward[e] = np.float32(self.crash_reward)         # (fresh and frozen envs: 0)
        return observation(ranges, self.window, self.obs_clip, self.obs_scale), reward

    def reset(self, seed=0, start_index=None):
        N = self.N
        self.seed = int(seed)
        self.states = np.zeros((N, 11))
        self.tick, self.episode = np.zeros(N, np.int32), np.zeros(N, np.int32)
        self.start_index, self.done = np.zeros(N, np.int32), np.zeros(N, np.int32)
        for e in range(N):
            self._spawn(e, 0, start_index)
        self.k = 0
        yes, no = np.ones(N, bool), np.zeros(N, bool)
        obs, _ = self._observe(no, yes, no, np.zeros(N))
        return obs, self.done.copy()

    def step(self, actions):
        if self.k is None:
            raise RuntimeError("step before reset")
        N = self.N
        a = np.asarray(actions, np.float32).reshape(N, 2)
        self.k += 1
        stepped, fresh, invalid = np.zeros(N, bool), np.zeros(N, bool), np.zeros(N, bool)
        moved = np.zeros(N)
        for e in range(N):
            if self.done[e] != RUNNING:
                if self.auto_reset:
                    self._spawn(e, int(self.episode[e]) + 1)
                    fresh[e] = True
                continue                                  # (frozen: nothing changes)
            speed, steer = np.float64(a[e, 0]), np.float64(a[e, 1])
            if not (np.isfinite(speed) and np.isfinite(steer)):
                self.done[e] = BAD_ACTION
                invalid[e] = True
                continue
            stepped[e] = True
        go = np.nonzero(stepped)[0]
        if go.size:
            speed, steer = a[go, 0].astype(np.float64), a[go, 1].astype(np.float64)
            if self.steer_clip > 0:
                steer = np.minimum(np.maximum(steer, -self.steer_clip), self.steer_clip)
            before = self.states[go, 8].copy()
            self.states[go] = np.asarray(self.step_cars(self.states[go].copy(), speed, steer), np.float64)
            self.tick[go] += 1
            moved[go] = self.states[go, 8] - before
        obs, reward = self._observe(stepped, fresh, invalid, moved)
        return obs, reward, self.done.copy()
