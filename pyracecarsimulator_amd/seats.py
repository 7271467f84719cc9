"""Per-seat drivers in races (include/scanlib_seats.h): what ``CarBatch.race_seats`` and ``RaceEnv(seats=...)`` share.

A seat is the position of a car in its race, and every seat has one driver: a ``PyFollowGap`` (scripts/two_player/
simple_driver.py), a ``Policy`` (scripts/policy_driver.py) or, in the environment only, None: the caller's actions.
The checks here need no device and word their refusals as the library does.
"""
from __future__ import annotations

import numpy as np

from . import _lib

#: enum rl_seat_driver
SEAT_CALLER, SEAT_FOLLOWGAP, SEAT_POLICY = (_lib.SEAT_DRIVERS[k] for k in ("caller", "followgap", "policy"))


def seat_args(drivers, group, num_rays, caller_ok):
    """``drivers`` (one ``PyFollowGap``, ``Policy`` or None per seat) checked against a race of ``group`` cars that scan
    ``num_rays`` beams: returns (codes int32 (group,), the FollowGap object or None, the policy or None).  At most
    one distinct object of each kind may drive seats; None (the caller's seat) only with ``caller_ok``."""
    from .followgap import PyFollowGap
    from .policy import Policy
    drivers = list(drivers)
    if len(drivers) != int(group):
        raise ValueError("one driver per seat: %d seats, got %d drivers" % (group, len(drivers)))
    if not 1 <= int(group) <= 8:
        raise ValueError("group must lie in [1, 8] cars (got %d)" % group)
    codes = np.zeros(int(group), np.int32)
    fg = pol = None
    for k, d in enumerate(drivers):
        if d is None:
            if not caller_ok:
                raise ValueError("seat %d is the caller's: a roll-out has no caller to ask" % k)
            codes[k] = SEAT_CALLER
        elif isinstance(d, PyFollowGap):
            if fg is not None and d is not fg:
                raise ValueError("seat %d: at most one PyFollowGap object may drive seats" % k)
            fg, codes[k] = d, SEAT_FOLLOWGAP
        elif isinstance(d, Policy):
            if pol is not None and d is not pol:
                raise ValueError("seat %d: at most one Policy object may drive seats" % k)
            pol, codes[k] = d, SEAT_POLICY
        else:
            raise ValueError("seat %d: unknown driver %r (a PyFollowGap, a Policy%s)" % (
                k, type(d).__name__, " or None" if caller_ok else ""))
    if pol is not None and int(num_rays) < pol.in_start + pol.dims[0]:
        raise ValueError("scans of %d beams do not hold the policy's window [%d, %d)" % (
            num_rays, pol.in_start, pol.in_start + pol.dims[0]))
    return codes, fg, pol


def seat_env_args(seats, seat_speed, group, num_rays):
    """``RaceEnv``'s ``seats`` and ``seat_speed`` (a scalar or one value per seat) checked and laid out for
    ``rl_env_attach_seats``: returns (rl_seat_params, the FollowGap object or None, the policy or None)."""
    codes, fg, pol = seat_args(seats, group, num_rays, caller_ok=True)
    spd = np.asarray(seat_speed, dtype=np.float32)
    if spd.ndim == 0:
        spd = np.full(len(codes), spd, np.float32)
    if spd.shape != (len(codes),):
        raise ValueError("seat_speed must be a scalar or one value per seat (%d)" % len(codes))
    sp = _lib.SeatParams()
    for k, c in enumerate(codes):
        if c != SEAT_CALLER and not np.isfinite(spd[k]):
            raise ValueError("the speed of seat %d must be finite" % k)
        sp.driver[k] = int(c)
        sp.speed[k] = float(spd[k]) if np.isfinite(spd[k]) else 0.0
    return sp, fg, pol
