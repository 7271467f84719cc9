"""The six closed-loop roll-out wrappers of ``CarBatch`` without a device: ``_lib.call`` is replaced by a recorder and
every wrapper's library call is compared with its prototype, position by position — which handle, each scalar's value
and Python type, each array's dtype, shape and C-contiguity, None where an optional output is off —; what the wrapper
returns, what ``_tracked`` records, and every ``ValueError`` with its exact message, the first fault first."""
import numpy as np
import pytest

from test_population_host import _pop
from pyracecarsimulator_amd import Track, _lib
from pyracecarsimulator_amd import racecar as RC
from pyracecarsimulator_amd.followgap import PyFollowGap
from pyracecarsimulator_amd.policy import Policy

T, B, FOV, THRESH = 2, 12, 4.7, 0.001                              # ticks, beams
DT, BASE = 0.01, 0.275                                             # (the wrappers' defaults)
WIN = dict(dims=(8, 4, 1), in_start=2)                             # the networks' window: beams [2, 10)

# the parameter names of the six prototypes, in their headers' order
IN, MID = "states_in speeds steer0_or_null ", "n_ticks dt scan_dist_to_base fov num_rays edge crash_thresh "
OUT = ("first_crashed states_out_or_null velocities_or_null steers_or_null scan_poses_or_null states_trace_or_null")
ORDER = {"rl_car_drive_followgap": "c h g " + IN + "n_rollouts " + MID + OUT,                       # scanlib.h
         "rl_car_race_followgap": "c h g " + IN + "n_races group " + MID + OUT,
         "rl_car_drive_policy": "c h p " + IN + "n_rollouts " + MID + "steer_clip " + OUT,
         "rl_car_race_seats": "c h g_or_null p_or_null seat_driver steer_clip " + IN + "n_races group " + MID + OUT,
         "rl_car_drive_population": "c h pop first n cars_per_member steer_clip " + IN + MID + OUT + " fitness_n2_or_null",
         "rl_car_race_league": "c h g_or_null pop entry_RP steer_clip " + IN + "n_races group " + MID + OUT
                               + " standings_N4_or_null"}


class Method(_lib.Handle):
    """A range method that never saw the library."""


def _policy():
    pol = Policy.__new__(Policy)
    pol.in_start, pol.dims = WIN["in_start"], WIN["dims"]
    return pol


FG, FG2 = PyFollowGap.__new__(PyFollowGap), PyFollowGap.__new__(PyFollowGap)
POL, POP, METHOD = _policy(), _pop(**WIN), Method()


@pytest.fixture
def calls(monkeypatch):
    """What ``_lib.call`` was asked for, in order: (symbol, arguments)."""
    made = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: made.append((name, args)))
    return made


def _cars(tracked=True):
    cars = RC.CarBatch.__new__(RC.CarBatch)
    cars._track = Track.__new__(Track) if tracked else None
    return cars


def _check(got, want, where):
    if want is None:
        assert got is None, where
    elif isinstance(want, tuple):                                  # an array: (dtype, shape[, values])
        assert isinstance(got, np.ndarray) and got.dtype == want[0] and got.shape == want[1], (where, got)
        assert got.flags.c_contiguous and (len(want) == 2 or np.array_equal(got, want[2])), (where, got)
    elif type(want) in (int, float):                               # a scalar: the value and its Python type
        assert type(got) is type(want) and got == want, (where, got, type(got))
    else:                                                          # a handle: the object itself
        assert got is want, where


#: wrapper, symbol, the cars' shape, its own keywords, its own arguments by name, the score it returns, its track scores
Z = np.zeros
CASES = [
    ("drive_followgap", "rl_car_drive_followgap", (3,), dict(followgap=FG), dict(g=FG, n_rollouts=3), None, None),
    ("drive_policy", "rl_car_drive_policy", (3,), dict(policy=POL), dict(p=POL, n_rollouts=3, steer_clip=0.0), None, None),
    ("drive_policy", "rl_car_drive_policy", (3,), dict(policy=POL, steer_clip=2), dict(p=POL, n_rollouts=3, steer_clip=2.0),
     None, None),
    ("race_followgap", "rl_car_race_followgap", (2, 2), dict(followgap=FG), dict(g=FG, n_races=2, group=2), None, None),
    ("race_seats", "rl_car_race_seats", (2, 2), dict(drivers=[FG, POL], steer_clip=0.3),
     dict(g_or_null=FG, p_or_null=POL, seat_driver=(np.int32, (2,), [1, 2]), steer_clip=0.3, n_races=2, group=2), None, None),
    ("race_seats", "rl_car_race_seats", (2, 2), dict(drivers=[POL, POL]),
     dict(g_or_null=None, p_or_null=POL, seat_driver=(np.int32, (2,), [2, 2]), steer_clip=0.0, n_races=2, group=2), None, None),
    ("race_seats", "rl_car_race_seats", (2, 2), dict(drivers=[FG, FG]),
     dict(g_or_null=FG, p_or_null=None, seat_driver=(np.int32, (2,), [1, 1]), steer_clip=0.0, n_races=2, group=2), None, None),
    ("drive_population", "rl_car_drive_population", (3,), dict(pop=POP, cars_per_member=1, first=1),     # 3 members, 1 car
     dict(pop=POP, first=1, n=3, cars_per_member=1, steer_clip=0.0, fitness_n2_or_null=(np.float64, (3, 2), Z((3, 2)))),
     "fitness_n2_or_null", (3, 3)),
    ("drive_population", "rl_car_drive_population", (3,), dict(pop=POP, cars_per_member=3, first=4, steer_clip=0.25),
     dict(pop=POP, first=4, n=1, cars_per_member=3, steer_clip=0.25, fitness_n2_or_null=(np.float64, (1, 2), Z((1, 2)))),
     "fitness_n2_or_null", (1, 3)),
    ("race_league", "rl_car_race_league", (2, 2), dict(pop=POP, entries=[[0, -1], [4, 4]], followgap=FG, steer_clip=0.3),
     dict(g_or_null=FG, pop=POP, entry_RP=(np.int32, (4,), [0, -1, 4, 4]), steer_clip=0.3, n_races=2, group=2,
          standings_N4_or_null=(np.float64, (5, 4), Z((5, 4)))), "standings_N4_or_null", (5, 4)),
    ("race_league", "rl_car_race_league", (2, 2), dict(pop=POP, entries=np.array([[1, 2], [3, 0]]).T),   # (not contiguous)
     dict(g_or_null=None, pop=POP, entry_RP=(np.int32, (4,), [1, 3, 2, 0]), steer_clip=0.0, n_races=2, group=2,
          standings_N4_or_null=(np.float64, (5, 4), Z((5, 4)))), "standings_N4_or_null", (5, 4)),
]


@pytest.mark.parametrize("tracked", [False, True])
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("wrapper, symbol, shape, own, want, score, score_shape", CASES)
def test_the_library_call_is_the_prototypes(calls, wrapper, symbol, shape, own, want, score, score_shape, full, tracked):
    """``full``: an array speed, a steer0, the trace, and states that are not C-contiguous; otherwise a scalar speed."""
    R = int(np.prod(shape))
    states = np.arange(R * 11, dtype=np.float64).reshape(shape + (11,))
    speed, steer0, edge = 2.5, None, np.linspace(0.1, 0.2, B)
    if full:
        states, speed = np.asfortranarray(states), 1.0 + np.arange(R, dtype=np.float64).reshape(shape)
        steer0 = (0.125 * np.arange(R, dtype=np.float32)).reshape(shape)
        assert not states.flags.c_contiguous
    cars = _cars(tracked)
    res = getattr(cars, wrapper)(METHOD, states=states, n_ticks=T, speed=speed, fov=FOV, num_rays=B, edge=edge,
                                 crash_thresh=THRESH, steer0=steer0, trace=full, **own)
    want = dict(want, c=cars, h=METHOD, n_ticks=T, dt=DT, scan_dist_to_base=BASE, fov=FOV, num_rays=B, crash_thresh=THRESH,
                states_in=(np.float64, (R, 11), states.reshape(-1, 11)), edge=(np.float64, (B,), edge),
                speeds=(np.float64, (R,), np.reshape(speed, -1) if full else np.full(R, speed)),
                steer0_or_null=(np.float32, (R,), steer0.reshape(-1)) if full else None,
                first_crashed=(np.int32, (R,), Z(R)), states_out_or_null=(np.float64, (R, 11)),
                velocities_or_null=(np.float64, (R, T)), steers_or_null=(np.float32, (R, T)),
                scan_poses_or_null=(np.float32, (R, T, 3)) if full else None,
                states_trace_or_null=(np.float64, (R, T, 11)) if full else None)
    # the one recorded call: the prototype's order, and nothing the marshaller would refuse
    assert [name for name, _ in calls] == [symbol]
    args, names = calls[0][1], ORDER[symbol].split()
    assert len(names) == len(_lib.declared(symbol)[1]) == len(args) and set(names) == set(want)
    for i, (name, got, conv) in enumerate(zip(names, args, _lib.converters(symbol)[1])):
        _check(got, want[name], "%s argument %d (%s)" % (symbol, i, name))
        conv(got)
    # what comes back: the recorded outputs, their leading R P as (R, P) after a race, then the score
    sent = dict(zip(names, args))
    outs = OUT.split()[:6 if full else 4]
    assert isinstance(res, tuple) and len(res) == len(outs) + (score is not None)
    for got, name in zip(res, outs):
        assert got.dtype == sent[name].dtype and got.shape == shape + sent[name].shape[1:], name
        assert np.shares_memory(got, sent[name]) and (len(shape) == 2 or got is sent[name]), name
    assert score is None or res[-1] is sent[score]
    assert (cars._track_shape, cars._score_shape) == ((shape, score_shape) if tracked else (None, None))


# ---------------------------------------------------------------- the refusals, the fault that is reported first
OWN = {"drive_followgap": dict(followgap=FG), "race_followgap": dict(followgap=FG), "drive_policy": dict(policy=POL),
       "race_seats": dict(drivers=[FG, POL]), "drive_population": dict(pop=POP, cars_per_member=1),
       "race_league": dict(pop=POP, entries=np.array([[0, -1], [4, 4]]), followgap=FG)}
D3, R22, ENTRIES = Z((3, 11)), Z((2, 2, 11)), OWN["race_league"]["entries"]
STATES = {w: "states must be float64 (R, 11)" if w.startswith("drive") else "states must be float64 (R, P, 11)" for w in OWN}
SPEED, STEER0 = "speed must be a scalar or float64 (R,)", "steer0 must be float32 (R,)"
EDGE, CLIP = "edge must be float64 (num_rays,)", "steer_clip must be None or > 0"
SHORT, WINDOW = dict(num_rays=9, edge=Z(9)), "scans of 9 beams do not hold the policy's window [2, 10)"
PER, WHOLE = "cars_per_member must be >= 1", "states must hold a whole number of members: 3 cars, 2 per member"
SEATS, ENTRY = "one driver per seat: 2 seats, got 1 drivers", "every entry must be -1 (FollowGap) or a member in [0, 5)"
SHAPE, GROUP = "entries must be integers (R, P) = (2, 2), one driver per car", "group must lie in [1, 8] cars (got 9)"

# what every wrapper refuses in the same words: the states' rank and dtype, and what _drive_args checks after them
REFUSALS = [(w, change, message or STATES[w]) for w in OWN for change, message in (
    (dict(states=Z(11)), None), (dict(states=Z((3, 1, 1, 11))), None), (dict(states=Z((2, 2, 10))), None),
    (dict(states=Z((3, 10))), None), (dict(states=(R22 if w.startswith("race") else D3).astype(np.float32)), None),
    (dict(speed=Z(5)), SPEED), (dict(speed=Z((1, 5))), SPEED), (dict(steer0=Z(3)), STEER0), (dict(steer0=Z((2, 2))), STEER0),
    (dict(steer0=Z(5, np.float32)), STEER0), (dict(edge=Z(B - 1)), EDGE), (dict(edge=Z(B, np.float32)), EDGE),
    (dict(states=Z(11), speed=Z(5)), None), (dict(speed=Z(5), steer0=Z(3)), SPEED), (dict(steer0=Z(3), edge=Z(B - 1)), STEER0))]
REFUSALS += [(w, change, CLIP) for w in OWN if "followgap" not in w for change in (
    dict(steer_clip=0.0), dict(steer_clip=0), dict(steer_clip=-0.5), dict(steer_clip=0.0, edge=Z(B - 1)),
    dict(steer_clip=-1, speed=Z(5)))]
REFUSALS += [
    ("drive_policy", dict(steer_clip=0.0, states=D3[0]), CLIP),
    ("drive_population", dict(cars_per_member=0), PER),
    ("drive_population", dict(cars_per_member=2), WHOLE),
    ("drive_population", dict(first=3), "members [3, 6) do not lie in [0, 5)"),
    ("drive_population", dict(first=-1), "members [-1, 2) do not lie in [0, 5)"),
    ("drive_population", SHORT, WINDOW),
    ("drive_population", dict(steer_clip=0.0, cars_per_member=0), CLIP),                  # two faults from here on
    ("drive_population", dict(cars_per_member=0, states=D3.astype(np.float32)), PER),
    ("drive_population", dict(cars_per_member=2, edge=Z(B - 1)), EDGE),
    ("drive_population", dict(cars_per_member=2, first=4), WHOLE),
    ("drive_population", dict(first=3, **SHORT), "members [3, 6) do not lie in [0, 5)"),
    ("race_seats", dict(drivers=[FG]), SEATS),
    ("race_seats", dict(drivers=[FG, None]), "seat 1 is the caller's: a roll-out has no caller to ask"),
    ("race_seats", dict(drivers=[FG, 3]), "seat 1: unknown driver 'int' (a PyFollowGap, a Policy)"),
    ("race_seats", dict(drivers=[FG, FG2]), "seat 1: at most one PyFollowGap object may drive seats"),
    ("race_seats", dict(drivers=[POL, _policy()]), "seat 1: at most one Policy object may drive seats"),
    ("race_seats", dict(states=Z((1, 9, 11)), drivers=[FG] * 9), GROUP),
    ("race_seats", SHORT, WINDOW),
    ("race_seats", dict(states=D3, drivers=[FG]), STATES["race_seats"]),                  # two faults from here on
    ("race_seats", dict(drivers=[FG], steer_clip=0.0), SEATS),
    ("race_seats", dict(steer_clip=0.0, **SHORT), WINDOW),
    ("race_league", dict(states=Z((1, 9, 11)), entries=Z((1, 9), int)), GROUP),
    ("race_league", dict(entries=ENTRIES[0]), SHAPE),
    ("race_league", dict(entries=ENTRIES.astype(float)), SHAPE),
    ("race_league", dict(entries=ENTRIES + 1), ENTRY),
    ("race_league", dict(entries=ENTRIES - 1), ENTRY),
    ("race_league", dict(followgap=None), "an entry is -1 (FollowGap), but no followgap was given"),
    ("race_league", SHORT, WINDOW),
    ("race_league", dict(states=D3, entries=ENTRIES + 1), STATES["race_league"]),         # two faults from here on
    ("race_league", dict(entries=ENTRIES + 1, steer_clip=0.0), ENTRY),
    ("race_league", dict(steer_clip=0.0, steer0=Z((2, 2))), CLIP),
]


@pytest.mark.parametrize("wrapper, change, message", REFUSALS)
def test_refusals_name_the_first_fault_and_never_reach_the_library(calls, wrapper, change, message):
    kw = dict(OWN[wrapper], states=R22 if wrapper.startswith("race") else D3, n_ticks=T, speed=2.0, fov=FOV, num_rays=B,
              edge=Z(B), crash_thresh=THRESH)
    cars = _cars()
    with pytest.raises(ValueError) as e:
        getattr(cars, wrapper)(METHOD, **dict(kw, **change))
    assert str(e.value) == message
    assert calls == [] and cars._track_shape is None
