"""League races (include/scanlib_league.h): members of a ``PolicyPopulation`` as per-race seat drivers — what
``PolicyPopulation.predict_rows`` and ``CarBatch.race_league`` share, and the line-ups of a round robin.

An entry names the driver of one scan row or car: ``m >= 0`` is member m of the population, ``-1`` nobody (an
evaluation) or FollowGap (a race).  In a race environment (include/scanlib_league_env.h, ``RaceEnv(league=...)``) a
third code, ``CALLER`` = -2, leaves a car to the caller's actions.  The checks here need no device and word their
refusals as the library does.
"""
from __future__ import annotations

import itertools
import math

import numpy as np


#: entry codes of a race environment's line-ups (include/scanlib_league_env.h); m >= 0 is member m
CALLER, FOLLOWGAP = -2, -1

#: the columns of a driver's row of results, in the library's order
RESULT_COLUMNS = ("entered", "out", "ticks", "faced", "beaten", "callers_faced", "callers_beaten", "callers_won")


def member_args(members, n, n_members):
    """``members`` checked against ``n`` scan rows of a population of ``n_members``: int32 (n,), C-contiguous, every
    value in [-1, n_members)."""
    m = np.asarray(members)
    if m.dtype.kind not in "iu" or m.shape != (int(n),):
        raise ValueError("members must be integers (%d,), one per scan row" % n)
    if m.size and (m.min() < -1 or m.max() >= int(n_members)):
        raise ValueError("every member must be -1 or lie in [0, %d)" % n_members)
    return np.ascontiguousarray(m, dtype=np.int32)


def league_args(entries, n_races, group, pop, followgap, num_rays):
    """``entries`` of a league roll-out checked against R = ``n_races`` races of P = ``group`` cars: returns int32
    (R P,) race-major.  -1 needs ``followgap``; an entry >= 0 needs scans that hold the population's window."""
    if not 1 <= int(group) <= 8:
        raise ValueError("group must lie in [1, 8] cars (got %d)" % group)
    e = np.asarray(entries)
    if e.dtype.kind not in "iu" or e.shape != (int(n_races), int(group)):
        raise ValueError("entries must be integers (R, P) = (%d, %d), one driver per car" % (n_races, group))
    if e.size and (e.min() < -1 or e.max() >= pop.n_members):
        raise ValueError("every entry must be -1 (FollowGap) or a member in [0, %d)" % pop.n_members)
    if (e < 0).any() and followgap is None:
        raise ValueError("an entry is -1 (FollowGap), but no followgap was given")
    if (e >= 0).any() and int(num_rays) < pop.in_start + pop.dims[0]:
        raise ValueError("scans of %d beams do not hold the policy's window [%d, %d)"
                         % (num_rays, pop.in_start, pop.in_start + pop.dims[0]))
    return np.ascontiguousarray(e.reshape(-1), dtype=np.int32)


def seat_speeds(seat_speed, group):
    """``seat_speed`` (a scalar or one value per seat) as float32 (group,)."""
    spd = np.asarray(seat_speed, dtype=np.float32)
    if spd.ndim == 0:
        spd = np.full(int(group), spd, np.float32)
    if spd.shape != (int(group),):
        raise ValueError("seat_speed must be a scalar or one value per seat (%d)" % group)
    return np.ascontiguousarray(spd)


def league_env_args(entries, n_races, group, pop, followgap, num_rays, speeds):
    """``entries`` of a race environment's league checked against R = ``n_races`` races of P = ``group`` cars: returns
    int32 (R P,) race-major.  -2 is the caller's car, -1 needs ``followgap``, an entry >= 0 needs scans that hold the
    population's window, and a seat that holds a scripted car (an entry >= -1) needs a finite speed in ``speeds``
    float32 (P,)."""
    e = np.asarray(entries)
    if e.dtype.kind not in "iu" or e.shape != (int(n_races), int(group)):
        raise ValueError("entries must be integers (R, P) = (%d, %d), one driver per car" % (n_races, group))
    if e.size and (e.min() < CALLER or e.max() >= pop.n_members):
        raise ValueError("every entry must be -2 (the caller), -1 (FollowGap) or a member in [0, %d)" % pop.n_members)
    if (e == FOLLOWGAP).any() and followgap is None:
        raise ValueError("an entry is -1 (FollowGap), but no followgap was given")
    if (e >= 0).any() and int(num_rays) < pop.in_start + pop.dims[0]:
        raise ValueError("scans of %d beams do not hold the policy's window [%d, %d)"
                         % (num_rays, pop.in_start, pop.in_start + pop.dims[0]))
    for k in np.nonzero((e >= FOLLOWGAP).any(axis=0))[0]:
        if not np.isfinite(speeds[k]):
            raise ValueError("the speed of seat %d must be finite" % k)
    return np.ascontiguousarray(e.reshape(-1), dtype=np.int32)


def results_dict(raw, n_members):
    """The int64 (n_members + 2, 8) block of ``rl_env_read_league_results`` as a dict: every column of
    ``RESULT_COLUMNS`` as an (n_members,) array, and the ``followgap`` and ``caller`` rows as dicts of ints."""
    out = {name: raw[:n_members, c].copy() for c, name in enumerate(RESULT_COLUMNS)}
    for row, key in ((n_members, "followgap"), (n_members + 1, "caller")):
        out[key] = {name: int(raw[row, c]) for c, name in enumerate(RESULT_COLUMNS)}
    return out


def round_robin(n_members, group):
    """The entry table int32 (R, P) of a round robin of ``n_members`` members in races of P = ``group`` cars: every
    unordered line-up of P distinct members (in lexicographic order) occurs in P races, its P cyclic rotations, so each
    of its members sits in each seat exactly once.  R = C(n_members, P) · P races; every member enters
    C(n_members - 1, P - 1) · P cars, C(n_members - 1, P - 1) of them in each seat."""
    N, P = int(n_members), int(group)
    if not 1 <= P <= 8:
        raise ValueError("group must lie in [1, 8] cars (got %d)" % P)
    if N < P:
        raise ValueError("a line-up of %d distinct members needs at least %d members (got %d)" % (P, P, N))
    out = np.empty((math.comb(N, P) * P, P), np.int32)
    for i, combo in enumerate(itertools.combinations(range(N), P)):
        for s in range(P):
            out[i * P + s] = combo[s:] + combo[:s]
    return out
