"""include/scanlib_track_drive.h in plain NumPy float64, on top of tests/track_statement.py: the projection, the nearest
segment, the wrap, the progress step, the race offset and the ranks are that module's and are not restated here.  What
this module adds is the roll-out's side of the rule: which states of a call are a car's placements, the goal tick, and
the population's and the league's track scores.  No tests live here."""
import numpy as np

import track_statement as TS

f64 = np.float64
KEYS = ("s0", "s", "progress", "race_dist", "segment", "laps", "goal_tick", "rank")


def place(T, cx, cy, prev, window, fresh):
    """(segment, s) of a car at (cx, cy).  Where every d2 is NaN the device keeps the first candidate of its window
    (track_nearest's rule), not the lowest index; s is then NaN with the NaN of u."""
    cand = TS.candidates(T, prev, window, fresh)
    if np.isnan(TS.project(T, np.array(cand), cx, cy)[0]).all():
        seg = int(cand[0])
    else:
        seg = TS.nearest(T, cx, cy, prev, window, fresh)
    return seg, TS.quantities(T, seg, cx, cy, 0.0)[0]


def reached(first_crashed, n_ticks):
    """The ticks whose step a car takes: 0 ... first_crashed when it crashes, 0 ... n_ticks - 1 otherwise."""
    return range((int(first_crashed) if first_crashed >= 0 else int(n_ticks) - 1) + 1)


def placements(T, states_in, states_trace, first_crashed, n_ticks, window, goal_dist, group=0):
    """The rows of a tracked roll-out from its own starts, trace and crash ticks: a dict of KEYS, each (R,), and
    "trail" (R, n_ticks + 1) int32: the segment of every placement, the start first, -1 where the car was frozen.
    goal_dist 0 (or None) is the track length; group > 0: races of `group` cars."""
    st0 = np.asarray(states_in, f64).reshape(-1, 11)
    R = st0.shape[0]
    tr = np.asarray(states_trace, f64).reshape(R, int(n_ticks), 11)
    first = np.asarray(first_crashed).reshape(R)
    goal = T["L"] if not goal_dist else f64(goal_dist)
    out = {k: np.zeros(R, f64 if i < 4 else np.int32) for i, k in enumerate(KEYS)}
    out["trail"] = np.full((R, int(n_ticks) + 1), -1, np.int32)
    for r in range(R):
        seg, s0 = place(T, st0[r, 0], st0[r, 1], 0, window, True)
        s_prev, progress, laps, goal_tick = s0, f64(0), 0, -1
        out["trail"][r, 0] = seg
        for t in reached(first[r], n_ticks):
            seg, s = place(T, tr[r, t, 0], tr[r, t, 1], seg, window, False)
            _, progress, laps, s_prev = TS.progress_step(T, s, s_prev, progress, laps)
            if goal_tick < 0 and progress >= goal:
                goal_tick = t
            out["trail"][r, t + 1] = seg
        out["s0"][r], out["s"][r], out["progress"][r] = s0, s_prev, progress
        out["segment"][r], out["laps"][r], out["goal_tick"][r] = seg, laps, goal_tick
    for r in range(R):
        offset = TS.race_offset(T, out["s0"][r], out["s0"][r - r % group]) if group > 0 else f64(0)
        out["race_dist"][r] = offset + out["progress"][r]
    if group > 0:
        for r0 in range(0, R, group):
            out["rank"][r0:r0 + group] = TS.ranks(out["race_dist"][r0:r0 + group])
    return out


def track_fitness(pl, n, E):
    """rl_car_read_track_scores after a population roll-out, (n, 3): member m's cars are m E ... m E + E - 1."""
    out = np.zeros((n, 3))
    for m in range(n):
        total, ticks, hit = f64(0), f64(0), 0
        for r in range(m * E, (m + 1) * E):
            total = total + pl["progress"][r]
            if pl["goal_tick"][r] >= 0:
                hit += 1
                ticks = ticks + f64(pl["goal_tick"][r])
        out[m] = (total, hit, ticks)
    return out


def track_standings(pl, entries, n_members, group):
    """rl_car_read_track_scores after a league roll-out, (n_members, 4): the cars of member m are those whose entry
    is m, in ascending car index."""
    entry = np.asarray(entries).reshape(-1)
    out = np.zeros((n_members, 4))
    for m in range(n_members):
        total, hit, beaten, cnt = f64(0), 0, 0, 0
        for a in np.nonzero(entry == m)[0]:
            r0 = a - a % group
            cnt += 1
            total = total + pl["progress"][a]
            hit += int(pl["goal_tick"][a] >= 0)
            beaten += sum(bool(pl["race_dist"][a] > pl["race_dist"][o]) for o in range(r0, r0 + group))
        out[m] = (cnt, total, hit, beaten)
    return out
