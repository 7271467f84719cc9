"""Host statement of per-seat drivers (include/scanlib_seats.h): the race environment's state machine
(tests/race_env_statement.py) with the scripted seats' rows of `actions` written by their drivers, and the seated
roll-out loop (rl_car_race_seats) in plain Python.  The GPU tests drive both with the composed public calls, the host
tests with a fake one-dimensional world.

Callbacks: RaceEnvStatement's three, and
  answer(driver, ranges_row float32 (B,)) -> float32: the driver's answer to one full scan (`driver` is whatever the
      seat table holds for the seat: the statement only tells None, the caller's seat, from the rest)
"""
import numpy as np

from race_env_statement import RUNNING, RaceEnvStatement
from support import D_BASE, lidar_poses

NAN32 = np.float32(np.nan)


class SeatEnvStatement(RaceEnvStatement):
    """``seats``: one driver per seat (None: the caller's); ``seat_speed``: one float32 per seat."""

    def __init__(self, starts, n_races, num_rays, step_cars, scan, is_crashed, answer, seats, seat_speed, **kw):
        super().__init__(starts, n_races, num_rays, step_cars, scan, is_crashed, **kw)
        self.answer, self.seats = answer, list(seats)
        assert len(self.seats) == self.P
        self.seat_speed = np.broadcast_to(np.asarray(seat_speed, np.float32), (self.P,)).copy()
        self.steers = None

    def scripted(self, e):
        return self.seats[e % self.P] is not None

    def _answers(self):
        """After phase B: the seat driver's answer to each car's scan of this call, NaN for a caller's seat and for a
        car that is not running."""
        self.steers = np.full(self.N, NAN32, np.float32)
        for e in range(self.N):
            if self.scripted(e) and self.done[e] == RUNNING:
                self.steers[e] = np.float32(self.answer(self.seats[e % self.P], self.ranges[e]))

    def reset(self, seed=0, start_index=None):
        out = super().reset(seed, start_index)
        self._answers()
        return out

    def step(self, actions):
        """The parent's step with the scripted rows overwritten: (the seat's speed, the answer to the scan of the call
        before).  What the caller wrote there is never looked at.  A scripted car that is not running holds NaN here,
        and a car that is not running takes no action."""
        if self.k is None:
            raise RuntimeError("step before reset")
        a = np.array(actions, np.float32).reshape(self.N, 2)
        for e in range(self.N):
            if self.scripted(e):
                a[e] = (self.seat_speed[e % self.P], self.steers[e])
        self.fed = a
        out = super().step(a)
        self._answers()
        return out

    def seat_steers(self):
        return self.steers.copy()


def seated_rollout(states, speeds, steer0, n_ticks, seats, clipped, steer_clip, step_cars, scan, is_crashed, answer,
                   scan_dist_to_base=D_BASE):
    """rl_car_race_seats: rl_car_race_followgap's loop with the steer of car n from seat n % P's driver.  states
    (N, 11) race-major, speeds (N,), steer0 (N,) float32, seats: P drivers, clipped(driver) -> bool: the driver is the
    network (steer_clip clamps its seats and no others).  step_cars(states (n, 11), speed (n,), steer (n,)) -> states
    after one tick; scan(poses float32 (N, 3), cars float64 (N, 3), t) -> ranges (N, B) at tick t's ray offset.
    Returns (first (N,), final states (N, 11), steers float32 (N, T), state trace (N, T, 11))."""
    N, T, P = len(states), int(n_ticks), len(seats)
    state = np.array(states, np.float64)
    steer = np.asarray(steer0, np.float32).astype(np.float64)
    first = np.full(N, -(T + 1), np.int32)
    steers = np.full((N, T), NAN32, np.float32)
    trace = np.full((N, T, 11), np.nan)
    for t in range(T):
        live = np.nonzero(first < 0)[0]
        if live.size:
            state[live] = step_cars(state[live].copy(), np.asarray(speeds, np.float64)[live], steer[live])
            trace[live, t] = state[live]
        ranges = np.asarray(scan(lidar_poses(state, scan_dist_to_base), state[:, :3].copy(), t), np.float32).reshape(N, -1)
        for n in live:
            if is_crashed(ranges[n]):
                first[n] = t                              # a wreck from here on: the others keep seeing it
                continue
            driver = seats[n % P]
            a = np.float32(answer(driver, ranges[n]))
            steers[n, t] = a
            s = np.float64(a)
            if steer_clip > 0 and clipped(driver):
                s = np.minimum(np.maximum(s, -steer_clip), steer_clip)
            steer[n] = s
    return first, state, steers, trace
