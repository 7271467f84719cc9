"""Host statement of league line-ups in the race environment (include/scanlib_league_env.h): the seated env's state
machine (tests/seat_statement.py) with a driver per CAR, taken from the race's live entries; pending entries adopted
only when a race spawns; and the per-driver results, added once in the call that ends a race.  The GPU tests drive it
with the composed public calls, the host tests with a fake one-dimensional world.

Callbacks: RaceEnvStatement's three, and
  answer(entry, ranges_row float32 (B,)) -> float32: the answer of the driver `entry` names (-1: FollowGap; m >= 0:
      member m) to one full scan
"""
import numpy as np

from race_env_statement import BAD_ACTION, CRASHED, RACE_RUNNING, RUNNING, TRUNCATED
from seat_statement import NAN32, SeatEnvStatement

CALLER, FOLLOWGAP = -2, -1
COLUMNS = ("entered", "out", "ticks", "faced", "beaten", "callers_faced", "callers_beaten", "callers_won")


def beats(ticks_a, done_a, gain_a, ticks_b, done_b, gain_b):
    """Car a beats car b of its race: more ticks; as many, a survivor (done 2) against a car that is out (1 or 3); as
    many, both in the same of those two classes and the larger gain in plain f64.  Ties and NaN beat nobody."""
    if ticks_a != ticks_b:
        return bool(ticks_a > ticks_b)
    up_a, up_b = done_a == TRUNCATED, done_b == TRUNCATED
    out_a, out_b = done_a in (CRASHED, BAD_ACTION), done_b in (CRASHED, BAD_ACTION)
    if up_a and out_b:
        return True
    return bool(((up_a and up_b) or (out_a and out_b)) and np.float64(gain_a) > np.float64(gain_b))


def race_results(entries, ticks, gains, done, n_members, scripted):
    """The eight columns every car of ONE finished race adds: returns [(row, columns (8,) int64)] per car.  `scripted`
    (entry) -> bool tells a driver's car from a caller's."""
    P = len(entries)
    out = []
    for a in range(P):
        col = np.zeros(8, np.int64)
        col[0], col[1], col[2], col[3] = 1, done[a] in (CRASHED, BAD_ACTION), ticks[a], P - 1
        for b in range(P):
            if b == a:
                continue
            win = beats(ticks[a], done[a], gains[a], ticks[b], done[b], gains[b])
            lose = beats(ticks[b], done[b], gains[b], ticks[a], done[a], gains[a])
            caller = not scripted(entries[b])
            col[4] += win
            col[5] += caller
            col[6] += caller and win
            col[7] += caller and lose
        m = int(entries[a])
        row = n_members + 1 if not scripted(m) else n_members if m < 0 else m
        out.append((row, col))
    return out


class LeagueEnvStatement(SeatEnvStatement):
    """``entries``: the first pending table, int (R, P) or (N,); ``seat_speed``: one float32 per seat; ``n_members`` of
    the population; ``followgap`` False: no FollowGap handle, -1 behaves as the caller's; ``window`` False: the scans
    do not hold the population's window, every m >= 0 behaves as the caller's."""

    def __init__(self, starts, n_races, num_rays, step_cars, scan, is_crashed, answer, entries, seat_speed, n_members,
                 followgap=True, window=True, **kw):
        P = np.asarray(starts).shape[1]
        super().__init__(starts, n_races, num_rays, step_cars, scan, is_crashed, answer, [None] * P, seat_speed, **kw)
        self.n_members = int(n_members)
        self.lo, self.hi = (-1 if followgap else 0), (self.n_members if window else 0)
        self.pending = np.array(entries, np.int32).reshape(self.N)
        self.live = np.zeros(self.N, np.int32)
        self.results = np.zeros((self.n_members + 2, 8), np.int64)

    # -- the line-ups
    def is_scripted(self, entry):
        return self.lo <= int(entry) < self.hi

    def scripted(self, e):
        return self.is_scripted(self.live[e])

    def set_entries(self, entries):
        self.pending = np.array(entries, np.int32).reshape(self.N)

    def _spawn(self, r, q, given=None):
        """The race's spawn, and with it the adoption: car by car, pending -> live."""
        super()._spawn(r, q, given)
        cars = list(self.cars_of(r))
        self.live[cars] = self.pending[cars]

    # -- the answers: the car's own driver
    def _answers(self):
        self.steers = np.full(self.N, NAN32, np.float32)
        for e in range(self.N):
            if self.scripted(e) and self.done[e] == RUNNING:
                self.steers[e] = np.float32(self.answer(int(self.live[e]), self.ranges[e]))

    # -- the results: once, in the call in which the race's `over` leaves RACE_RUNNING
    def _observe(self, stepped, fresh, invalid, moved, live):
        out = super()._observe(stepped, fresh, invalid, moved, live)
        for r in np.nonzero(live)[0]:                             # (a race this call stepped or spawned ran until now)
            if self.race_over[r] == RACE_RUNNING:
                continue
            cars = list(self.cars_of(r))
            gains = [self.states[e, 8] - self.starts[self.start_index[e], c, 8] for c, e in enumerate(cars)]
            for row, col in race_results(self.live[cars], self.tick[cars], gains, self.done[cars], self.n_members,
                                         self.is_scripted):
                self.results[row] += col
        return out

    def league_steers(self):
        return self.steers.copy()

    def read_results(self, clear=False):
        out = self.results.copy()
        if clear:
            self.results[:] = 0
        return out
