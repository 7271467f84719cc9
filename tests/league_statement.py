"""Host statement of league races (include/scanlib_league.h), in NumPy and plain Python:

    grouping   : the rows of member[n] ordered by member, ascending row index inside each member; per member the
                 segment start and count; a workgroup table with one (member, chunk) per PM_CARS rows of a member; an
                 entry outside [0, n_members) is in no segment (as -1)
    evaluation : scan row i is answered by member member[i], by the canonical form of tests/policy_statement.py; a row
                 in no segment keeps the bits its element of steers had
    roll-out   : rl_car_race_seats' loop (tests/seat_statement.seated_rollout) with a driver per car, not per seat
    standings  : [m][0] cars entered, [m][1] the ascending, separately rounded f64 sum of their gains, [m][2] how many
                 crashed, [m][3] how many cars of their own races they beat

The GPU tests hold the library to it with the real scan and car, the host tests with a fake one-dimensional world.
No tests live here."""
import numpy as np

import policy_statement as S
import population_statement as PS
import seat_statement as SS
from support import D_BASE

PM_CARS = 8
FOLLOWGAP = -1


def group_rows(member, n_members, per_wg=PM_CARS):
    """(rows, start (n_members,), count (n_members,), table [(member, chunk)], total) of member[n]."""
    member = [int(v) for v in member]
    rows, start, count, table = [], [], [], []
    for m in range(n_members):
        mine = [i for i, v in enumerate(member) if v == m]          # (ascending: the order of the standings' sum)
        start.append(len(rows))
        count.append(len(mine))
        rows += mine
        table += [(m, c) for c in range((len(mine) + per_wg - 1) // per_wg)]
    return rows, np.array(start, int), np.array(count, int), table, len(table)


def wg_bound(n, n_members, per_wg=PM_CARS):
    """The host's upper bound of the table's length: ceil(n / per_wg) + min(n, n_members)."""
    return (n + per_wg - 1) // per_wg + min(n, n_members)


def evaluate_rows(thetas, dims, relu, scans, member, steers, in_start=180, clip=15.0, scale=15.0):
    """steers float32 (n,) after the call: the grouped rows answered, the others as they were."""
    scans = np.asarray(scans, np.float32)
    out = np.array(steers, np.float32)
    rows, start, count, table, total = group_rows(member, len(thetas))
    for m, c in table:                                              # (workgroup by workgroup, as the launch goes)
        seg = rows[start[m]:start[m] + count[m]][c * PM_CARS:(c + 1) * PM_CARS]
        out[seg] = S.forward(scans[seg], PS.unpack(thetas[m], dims), relu, in_start=in_start, clip=clip, scale=scale)
    return out


def league_rollout(states, speeds, steer0, n_ticks, entries, steer_clip, step_cars, scan, is_crashed, answer,
                   scan_dist_to_base=D_BASE):
    """rl_car_race_league.  entries (N,) race-major: the driver of every car; answer(entry, ranges_row) -> float32
    (entry -1: FollowGap's).  The clip clamps the cars with an entry >= 0 and no others.  Otherwise
    ``seated_rollout``'s arguments and results: with one "seat" per car its n % P is n."""
    drivers = [int(e) for e in np.asarray(entries).reshape(-1)]
    assert len(drivers) == len(states)
    return SS.seated_rollout(states, speeds, steer0, n_ticks, drivers, lambda d: d >= 0, steer_clip, step_cars, scan,
                             is_crashed, answer, scan_dist_to_base=scan_dist_to_base)


def standings(states_in, states_out, first_crashed, entries, n_members, group, n_ticks):
    """float64 (n_members, 4) of a league roll-out over N = R group cars."""
    s_in, s_out = np.asarray(states_in, np.float64).reshape(-1, 11), np.asarray(states_out, np.float64).reshape(-1, 11)
    first = np.asarray(first_crashed).reshape(-1)
    gain = [np.float64(s_out[r][8]) - np.float64(s_in[r][8]) for r in range(len(first))]
    alive = [np.float64(first[r]) if first[r] >= 0 else np.float64(n_ticks) for r in range(len(first))]
    rows, start, count, _, _ = group_rows(np.asarray(entries).reshape(-1), n_members)
    out = np.zeros((n_members, 4))
    for m in range(n_members):
        total = np.float64(0.0)
        for a in rows[start[m]:start[m] + count[m]]:
            total = total + gain[a]
            out[m, 2] += first[a] >= 0
            r0 = a - a % group
            for b in range(r0, r0 + group):
                out[m, 3] += bool(alive[a] > alive[b] or (alive[a] == alive[b] and gain[a] > gain[b]))
        out[m, 0] = count[m]
        out[m, 1] = total
    return out
