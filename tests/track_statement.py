"""include/scanlib.h "track progress" in plain NumPy float64, one function per paragraph of the header.  Every f64
operation is one NumPy operation, scalar or elementwise, so each is separately rounded as on the device.  ``TrackEnv`` strings the
paragraphs together for a whole env: it is told, per call, every env's state and phase, and keeps what the device
keeps (s_prev, progress, offset, segment, laps)."""
import numpy as np

FROZEN, STEPPED, FRESH, INVALID = 0, 1, 2, 3          # what a call did to an env (env_statement's phases)
f64 = np.float64


# ---------------------------------------------------------------- Track
def build(xy, closed):
    """The table of W points: dict of x, y [W], dx, dy, q, len [S], cum [S + 1], L, W, S, closed.  ValueError where the
    header refuses."""
    p = np.asarray(xy, f64)
    W = p.shape[0]
    if W < (3 if closed else 2) or W > 65536 or not np.isfinite(p).all():
        raise ValueError("refused track")
    S = W if closed else W - 1
    x, y = p[:, 0].copy(), p[:, 1].copy()
    dx, dy, q, ln = np.empty(S), np.empty(S), np.empty(S), np.empty(S)
    cum = np.zeros(S + 1)
    for i in range(S):
        j = (i + 1) % W
        dx[i] = x[j] - x[i]
        dy[i] = y[j] - y[i]
        q[i] = dx[i] * dx[i] + dy[i] * dy[i]
        if q[i] == 0 or not np.isfinite(q[i]):
            raise ValueError("refused segment %d" % i)
        ln[i] = np.sqrt(q[i])
        cum[i + 1] = cum[i] + ln[i]
    return dict(x=x, y=y, dx=dx, dy=dy, q=q, len=ln, cum=cum, L=cum[S], W=W, S=S, closed=bool(closed))


# ---------------------------------------------------------------- Projection
def project(T, i, cx, cy):
    """(d2, t, ax, ay) of the car at (cx, cy) on segment i (an index or an array of them: elementwise, every operation
    rounded on its own either way)."""
    cx, cy = f64(cx), f64(cy)
    ax, ay = cx - T["x"][i], cy - T["y"][i]
    u = ax * T["dx"][i] + ay * T["dy"][i]
    t = np.minimum(np.maximum(u / T["q"][i], f64(0)), f64(1))
    ex, ey = ax - t * T["dx"][i], ay - t * T["dy"][i]
    return ex * ex + ey * ey, t, ax, ay


# ---------------------------------------------------------------- Nearest segment
def candidates(T, prev, window, fresh):
    S = T["S"]
    if fresh or window == 0 or 2 * window + 1 >= S:
        return list(range(S))
    if T["closed"]:
        return [(prev - window + m) % S for m in range(2 * window + 1)]
    return list(range(max(prev - window, 0), min(prev + window, S - 1) + 1))


def nearest(T, cx, cy, prev=0, window=0, fresh=True):
    """The candidate with the smallest d2, the lowest index among equals (argmin over ascending indices: the first)."""
    idx = np.array(sorted(candidates(T, prev, window, fresh)))
    return int(idx[np.argmin(project(T, idx, cx, cy)[0])])


# ---------------------------------------------------------------- Per-car quantities
def quantities(T, i, cx, cy, th):
    """(s, lateral, heading_err, hx, hy) from the nearest segment i."""
    _, t, ax, ay = project(T, i, cx, cy)
    dx, dy, ln = T["dx"][i], T["dy"][i], T["len"][i]
    s = T["cum"][i] + t * ln
    lateral = (dx * ay - dy * ax) / ln
    hx, hy = np.cos(f64(th)), np.sin(f64(th))
    heading = np.arctan2(dx * hy - dy * hx, dx * hx + dy * hy)
    return s, lateral, heading, hx, hy


# ---------------------------------------------------------------- Progress
def wrap(T, d):
    """The +-L rule: (d taken the short way round, the lap it crossed)."""
    if T["closed"]:
        half = f64(0.5) * T["L"]
        if d < -half:
            return d + T["L"], 1
        if d > half:
            return d - T["L"], -1
    return d, 0


def progress_step(T, s, s_prev, progress, laps):
    """A stepped env: (delta, progress, laps, s_prev)."""
    d, lap = wrap(T, s - s_prev)
    return d, progress + d, laps + lap, s


# ---------------------------------------------------------------- Goal waypoint
def goal_candidates(T, i, goal_span):
    W = T["W"]
    if goal_span == 0:
        return list(range(W))
    if T["closed"]:
        return [(i + 1 + m) % W for m in range(goal_span)]
    return [i + 1 + m for m in range(goal_span) if i + 1 + m <= W - 1]


def goal_loop(T, i, cx, cy, lookahead, goal_span):
    """The goal waypoint's index (-1: none), the rule as written: the best starts at 2 l, j wins on g_j < best."""
    cx, cy, la = f64(cx), f64(cy), f64(lookahead)
    best, g_idx = f64(2) * la, -1
    for j in goal_candidates(T, i, goal_span):
        rx, ry = T["x"][j] - cx, T["y"][j] - cy
        g = abs(la - np.sqrt(rx * rx + ry * ry))
        if g < best:
            best, g_idx = g, j
    return g_idx


def goal(T, i, cx, cy, lookahead, goal_span):
    """The same winner without the loop: the first candidate that reaches the smallest g, if that lies below 2 l."""
    cx, cy, la = f64(cx), f64(cy), f64(lookahead)
    cand = np.array(goal_candidates(T, i, goal_span))
    rx, ry = T["x"][cand] - cx, T["y"][cand] - cy
    g = np.abs(la - np.sqrt(rx * rx + ry * ry))
    k = int(np.argmin(g))
    return int(cand[k]) if g[k] < f64(2) * la else -1


def goal_point(T, g_idx, cx, cy, hx, hy):
    """(gx, gy, |r|): the goal in the car's frame and its distance; (0, 0, 0) without a goal."""
    if g_idx < 0:
        return f64(0), f64(0), f64(0)
    rx, ry = T["x"][g_idx] - f64(cx), T["y"][g_idx] - f64(cy)
    return hx * rx + hy * ry, hx * ry - hy * rx, np.hypot(rx, ry)


# ---------------------------------------------------------------- Race order
def race_offset(T, s, s_car0):
    return wrap(T, s - s_car0)[0]


def ranks(race_dist):
    """rank[k] = the number of k' with a larger race_dist, or an equal one and k' < k."""
    d = np.asarray(race_dist, f64)
    return np.array([sum(1 for k2 in range(len(d)) if d[k2] > d[k] or (d[k2] == d[k] and k2 < k))
                     for k in range(len(d))], np.int32)


# ---------------------------------------------------------------- a whole env
class TrackEnv:
    """N envs (races of `group` cars when group > 0) on the table T: ``call(states, phases)`` is one reset or step.
    Outputs: rows64 (N, 8) f64 before the cast, rows (N, 8) f32, ints (N, 4) int32, goal_dist (N,) = |r|."""

    def __init__(self, T, n, window=0, lookahead=1.5, goal_span=0, group=0):
        self.T, self.N, self.window, self.la, self.span, self.group = T, n, window, lookahead, goal_span, group
        self.s_prev, self.progress, self.offset = np.zeros(n), np.zeros(n), np.zeros(n)
        self.rows64 = np.zeros((n, 8))
        self.ints = np.zeros((n, 4), np.int32)
        self.goal_dist = np.zeros(n)

    @property
    def rows(self):
        return self.rows64.astype(np.float32)

    def call(self, states, phases):
        T = self.T
        s_now = np.zeros(self.N)
        for e in range(self.N):
            ph = int(phases[e])
            if ph not in (FRESH, STEPPED):
                self.rows64[e, 0] = 0.0
                continue
            cx, cy, th = states[e, 0], states[e, 1], states[e, 2]
            i = nearest(T, cx, cy, int(self.ints[e, 0]), self.window, ph == FRESH)
            s, lat, head, hx, hy = quantities(T, i, cx, cy, th)
            s_now[e] = s
            g = goal(T, i, cx, cy, self.la, self.span)
            gx, gy, r = goal_point(T, g, cx, cy, hx, hy)
            if ph == FRESH:
                d, self.progress[e], laps, self.s_prev[e] = f64(0), 0.0, 0, s
            else:
                d, self.progress[e], laps, self.s_prev[e] = progress_step(T, s, self.s_prev[e], self.progress[e],
                                                                         int(self.ints[e, 2]))
            self.rows64[e, :7] = (d, s, lat, head, gx, gy, self.progress[e])
            self.ints[e, :3] = (i, g, laps)
            self.goal_dist[e] = r
        for e in range(self.N):
            if int(phases[e]) == FRESH:
                car0 = e - e % self.group if self.group > 0 else e
                self.offset[e] = race_offset(T, s_now[e], s_now[car0]) if self.group > 0 else 0.0
        self.rows64[:, 7] = self.offset + self.progress
        if self.group > 0:
            for r0 in range(0, self.N, self.group):
                self.ints[r0:r0 + self.group, 3] = ranks(self.rows64[r0:r0 + self.group, 7])
        return self.rows, self.ints.copy()


def phases_drive(done_before, actions, auto_reset, reset=False):
    """What a DriveEnv call does to every env (include/scanlib.h "the driving environment", phase A)."""
    n = len(done_before)
    if reset:
        return np.full(n, FRESH)
    ok = np.isfinite(np.asarray(actions, np.float32).reshape(n, 2)).all(1)
    return np.where(done_before != 0, FRESH if auto_reset else FROZEN, np.where(ok, STEPPED, INVALID))


def phases_race(over_before, done_before, actions, auto_reset, group, reset=False):
    """The same for a RaceEnv ("the race environment", phase A): per car, from its race's over code and its own done."""
    n = len(done_before)
    if reset:
        return np.full(n, FRESH)
    ok = np.isfinite(np.asarray(actions, np.float32).reshape(n, 2)).all(1)
    over = np.repeat(np.asarray(over_before), group)
    car = np.where(done_before != 0, FROZEN, np.where(ok, STEPPED, INVALID))
    return np.where(over != 0, FRESH if auto_reset else FROZEN, car)
