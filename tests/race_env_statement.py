"""Host statement of the race environment (include/scanlib.h, "the race environment"; rl_env_create_race): the state
machine of reset and step in plain Python over three callbacks.  It is the second statement of that header section;
the GPU tests drive it with the composed public calls (CarBatch.rollout, calc_range_fan_cars, is_crashed), the host
tests with a fake one-dimensional world.

Callbacks:
  step_cars(states float64 (n, 11), speed float64 (n,), steer float64 (n,)) -> states (n, 11) after the env's
      `substeps` car steps (the callback owns substeps and dt)
  scan(poses float32 (N, 3), cars float64 (N, 3), k) -> ranges float32 (N, B): all N lidar poses of all races at slot
      k's ray offset, base + (k N + e) B, each with the other cars of its race (x, y, theta rows of `cars`, race-major)
      in the map (the callback owns the group size, the base and the noise)
  is_crashed(ranges float32 (B,)) -> bool: Car::isCrashed on one scan
"""
import numpy as np

from env_statement import observation, spawn_index
from support import lidar_poses

RUNNING, CRASHED, TRUNCATED, BAD_ACTION = 0, 1, 2, 3
RACE_RUNNING, RACE_ATTRITION, RACE_TRUNCATED = 0, 1, 2


class RaceEnvStatement:
    def __init__(self, starts, n_races, num_rays, step_cars, scan, is_crashed, min_running=1, obs_window=None,
                 obs_clip=0.0, obs_scale=0.0, max_ticks=0, auto_reset=True, steer_clip=0.0, crash_reward=0.0,
                 scan_dist_to_base=0.275):
        self.starts = np.array(starts, np.float64)
        assert self.starts.ndim == 3 and self.starts.shape[2] == 11
        self.M, self.P = self.starts.shape[:2]
        self.R, self.B = int(n_races), int(num_rays)
        self.N = self.R * self.P
        self.min_running = int(min_running)
        assert 1 <= self.min_running <= self.P
        self.step_cars, self.scan, self.is_crashed = step_cars, scan, is_crashed
        self.window = (0, self.B, 1) if obs_window is None else tuple(obs_window)
        self.obs_clip, self.obs_scale = obs_clip, obs_scale
        self.max_ticks, self.auto_reset = int(max_ticks), bool(auto_reset)
        self.steer_clip, self.crash_reward = float(steer_clip), float(crash_reward)
        self.d_base = scan_dist_to_base
        self.k = None                                   # calls since the reset (None: no reset yet)

    def cars_of(self, r):
        return range(r * self.P, (r + 1) * self.P)

    def _spawn(self, r, q, given=None):
        """The whole race from one line-up: the caller's index or the env's draw at counter (r, q)."""
        idx = int(given[r]) if given is not None else spawn_index(self.seed, r, q, self.M)
        if not 0 <= idx < self.M:
            raise ValueError("start_index outside [0, M)")
        for c, e in enumerate(self.cars_of(r)):
            self.states[e] = self.starts[idx, c]
            self.tick[e], self.episode[e], self.start_index[e], self.done[e] = 0, q, idx, RUNNING
        self.race_tick[r], self.race_episode[r], self.race_start_index[r] = 0, q, idx

    def _observe(self, stepped, fresh, invalid, moved, live):
        """The scan of slot k and phase B; `live`: the races this call stepped or spawned.  Returns (obs, reward)."""
        N = self.N
        ranges = np.asarray(self.scan(lidar_poses(self.states, self.d_base), self.states[:, :3].copy(), self.k),
                            np.float32).reshape(N, self.B)
        self.ranges = ranges
        reward = np.zeros(N, np.float32)
        for e in range(N):                                        # per car: the env's rule on the race's tick
            hit = bool(self.is_crashed(ranges[e]))
            r = e // self.P
            if (stepped[e] or fresh[e]) and hit:
                self.done[e] = CRASHED
            elif stepped[e] and self.max_ticks > 0 and self.race_tick[r] == self.max_ticks:
                self.done[e] = TRUNCATED
            if stepped[e]:
                reward[e] = np.float32(self.crash_reward if self.done[e] == CRASHED else moved[e])
            elif invalid[e]:
                reward[e] = np.float32(self.crash_reward)         # (fresh cars, wrecks and frozen ones: 0)
        for r in np.nonzero(live)[0]:                             # per race, once every car has its code
            cars = list(self.cars_of(r))
            running = sum(self.done[e] == RUNNING for e in cars)
            if any(self.done[e] == TRUNCATED for e in cars):      # (a running race held no 2 before this call)
                self.race_over[r] = RACE_TRUNCATED
            elif running < self.min_running:
                self.race_over[r] = RACE_ATTRITION
                for e in cars:
                    if self.done[e] == RUNNING:
                        self.done[e] = TRUNCATED                  # it survived: the reward stays
            else:
                self.race_over[r] = RACE_RUNNING
        return observation(ranges, self.window, self.obs_clip, self.obs_scale), reward

    def reset(self, seed=0, start_index=None):
        N, R = self.N, self.R
        self.seed = int(seed)
        self.states = np.zeros((N, 11))
        self.tick, self.episode = np.zeros(N, np.int32), np.zeros(N, np.int32)
        self.start_index, self.done = np.zeros(N, np.int32), np.zeros(N, np.int32)
        self.race_tick, self.race_episode = np.zeros(R, np.int32), np.zeros(R, np.int32)
        self.race_start_index, self.race_over = np.zeros(R, np.int32), np.zeros(R, np.int32)
        for r in range(R):
            self._spawn(r, 0, start_index)
        self.k = 0
        yes, no = np.ones(N, bool), np.zeros(N, bool)
        obs, _ = self._observe(no, yes, no, np.zeros(N), np.ones(R, bool))
        return obs, self.done.copy()

    def step(self, actions):
        if self.k is None:
            raise RuntimeError("step before reset")
        N = self.N
        a = np.asarray(actions, np.float32).reshape(N, 2)
        self.k += 1
        stepped, fresh, invalid = np.zeros(N, bool), np.zeros(N, bool), np.zeros(N, bool)
        live = np.zeros(self.R, bool)
        moved = np.zeros(N)
        for r in range(self.R):
            if self.race_over[r] != RACE_RUNNING:
                if self.auto_reset:
                    self._spawn(r, int(self.race_episode[r]) + 1)
                    fresh[list(self.cars_of(r))] = True
                    live[r] = True
                continue                                          # (a finished race that stands: nothing changes)
            live[r] = True
            self.race_tick[r] += 1
            for e in self.cars_of(r):
                if self.done[e] != RUNNING:
                    continue                                      # a wreck
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
        obs, reward = self._observe(stepped, fresh, invalid, moved, live)
        return obs, reward, self.done.copy()
