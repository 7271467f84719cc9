"""League races without a GPU: the grouping, the roll-out and the standings (tests/league_statement.py) in plain Python
and on a fake one-dimensional world, what include/scanlib_league.h says beyond its prototypes
(tests/test_py_calls_host.py pins those to ``_lib.LEAGUE_SYMBOLS``), ``round_robin``'s balance and every Python-side
refusal."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import league_statement as LS
import policy_statement as S
import scanlib_header as H
from test_population_host import DIMS, _layers, _pop, no_calls  # noqa: F401  (no_calls: a fixture)
from test_race_env_host import B, World1D, _lineup
from pyracecarsimulator_amd import _lib, league, population
from pyracecarsimulator_amd import racecar as RC

LEAGUE_HEADER = H.read("scanlib_league.h")


# ---------------------------------------------------------------- the grouping
def test_grouping_is_stable_by_member_with_a_workgroup_table():
    member = [2, 0, -1, 2, 5, 2, 0, -7, 3] + [2] * 9               # 5 and -7: out of range for 4 members
    rows, start, count, table, total = LS.group_rows(member, 4)
    assert rows == [1, 6] + [0, 3, 5] + list(range(9, 18)) + [8]   # by member, ascending inside each
    assert start.tolist() == [0, 2, 2, 14] and count.tolist() == [2, 0, 12, 1]
    assert table == [(0, 0), (2, 0), (2, 1), (3, 0)] and total == 4  # member 2: 12 rows, two workgroups of 8
    assert sorted(rows) == [i for i, m in enumerate(member) if 0 <= m < 4]
    assert total <= LS.wg_bound(len(member), 4) == 3 + 4
    # the bound is met: every member one row over a multiple of 8
    worst = [0] * 9 + [1] * 9 + [2]
    assert LS.group_rows(worst, 3)[4] == 5 <= LS.wg_bound(19, 3) == 3 + 3
    assert LS.group_rows([], 3)[4] == 0 and LS.group_rows([-1, 3], 3)[0] == []
    # exactly 8 rows are one workgroup, 9 are two
    assert LS.group_rows([1] * 8, 2)[3] == [(1, 0)] and LS.group_rows([1] * 9, 2)[3] == [(1, 0), (1, 1)]


def test_rows_statement_is_member_of_row_then_policy_statement():
    thetas = np.stack([population.pack(_layers(DIMS, 10 + m)) for m in range(4)])
    relu = (True, True, False)
    scan = np.random.default_rng(3).uniform(0, 18, (1, 16)).astype(np.float32)
    member = [3, -1, 0, 3, 9, 1, 0]
    scans = np.tile(scan, (len(member), 1))
    before = np.arange(7, dtype=np.float32) + 100
    got = LS.evaluate_rows(thetas, DIMS, relu, scans, member, before, in_start=2)
    want = {m: S.forward(scan, _layers(DIMS, 10 + m), relu, in_start=2)[0] for m in range(4)}
    assert len({w.tobytes() for w in want.values()}) == 4
    for i, m in enumerate(member):
        assert got[i].tobytes() == (want[m] if 0 <= m < 4 else before[i]).tobytes(), i
    # member[i] = first + i // E is the population's evaluation
    import population_statement as PS
    scans = np.random.default_rng(4).uniform(0, 18, (6, 16)).astype(np.float32)
    rows = LS.evaluate_rows(thetas, DIMS, relu, scans, [1 + i // 2 for i in range(6)], np.zeros(6, np.float32), in_start=2)
    assert rows.tobytes() == PS.evaluate(thetas, DIMS, relu, scans, 2, first=1, n=3, in_start=2).tobytes()


# ---------------------------------------------------------------- the roll-out and the standings on the fake world
def _answer(entry, row):
    assert row.shape == (B,) and row.dtype == np.float32
    if entry < 0:
        return np.float32(row[0]) / np.float32(100.0)              # "FollowGap"
    return np.float32(row[0]) / np.float32(10.0 * entry)           # member m


def test_league_rollout_statement():
    """Two races of three: the driver is looked up per car (cars 0 and 3 share seat 0 and not their member), the clip
    clamps the members' cars and never FollowGap's, `steers` keeps the raw answers, a wreck stops and is beaten, a tie
    beats nobody, a member that entered nothing reads zeros."""
    w = World1D(3)
    states = np.concatenate([_lineup(0.0, 3.0, 8.5), _lineup(1.0, 4.0, 6.0)])
    speeds = np.array([1.0, 1.0, 5.0, 1.0, 1.0, 1.0])
    entries = [1, -1, 2, 2, 1, -1]
    T = 3
    first, final, steers, trace = LS.league_rollout(states, speeds, np.zeros(6, np.float32), T, entries, 0.125,
                                                    w.step_cars, w.scan, World1D.is_crashed, _answer, scan_dist_to_base=0.0)
    assert w.slots == [0, 1, 2]
    assert first.tolist() == [-4, -4, 1, -4, -4, -4]               # car 2: 9.0, 9.5
    assert np.isnan(steers[2, 1:]).all() and np.isnan(trace[2, 2]).all() and final[2, 0] == 9.5
    three, two = np.float32(3.0), np.float32(2.0)
    # seat 0 of both races, members 1 and 2: 3 m to the next car
    assert steers[0, 0] == three / np.float32(10.0) and steers[3, 0] == three / np.float32(20.0)
    assert trace[0, 1, 4] == 0.125 and trace[3, 1, 4] == 0.125     # both over the clip: what the cars get
    # car 2 (member 2) 1 m from the wall: 0.05, under the clip
    assert steers[2, 0] == np.float32(1.0) / np.float32(20.0) and np.float32(trace[2, 1, 4]) == steers[2, 0]
    # car 4 (member 1, seat 1): 2 m to car 5
    assert steers[4, 0] == two / np.float32(10.0) and trace[4, 1, 4] == 0.125
    # FollowGap's cars: raw, whatever the clip (a clip below their answers, too)
    assert steers[1, 0] == three / np.float32(100.0) and np.float32(trace[1, 1, 4]) == steers[1, 0]
    low = LS.league_rollout(states, speeds, np.zeros(6, np.float32), T, entries, 0.001, World1D(3).step_cars,
                            World1D(3).scan, World1D.is_crashed, _answer, scan_dist_to_base=0.0)
    assert np.float32(low[3][1, 1, 4]) == steers[1, 0] and low[3][0, 1, 4] == 0.001
    # standings: race 0 — cars 0 and 1 outlive the wreck and tie with each other; race 1 — three ties
    st = LS.standings(states, final, first, entries, 4, 3, T)
    d = final[:, 8] - states[:, 8]
    assert d[0] == d[1] == d[3] == d[4] == d[5] and d[2] == 1.0
    assert st[0].tolist() == [0.0] * 4 and st[3].tolist() == [0.0] * 4
    assert st[1].tolist() == [2.0, (0.0 + d[0]) + d[4], 0.0, 1.0]    # cars 0, 4: car 0 beats the wreck
    assert st[2].tolist() == [2.0, (0.0 + d[2]) + d[3], 1.0, 0.0]    # cars 2, 3: the wreck beats nobody
    # all FollowGap is the seated roll-out with one driver
    import seat_statement as SS
    fg = LS.league_rollout(states, speeds, np.zeros(6, np.float32), T, [-1] * 6, 0.125, World1D(3).step_cars,
                           World1D(3).scan, World1D.is_crashed, _answer, scan_dist_to_base=0.0)
    seated = SS.seated_rollout(states, speeds, np.zeros(6, np.float32), T, [-1] * 3, lambda d: False, 0.125,
                               World1D(3).step_cars, World1D(3).scan, World1D.is_crashed, _answer, scan_dist_to_base=0.0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(fg, seated))


def _states(gains):
    s = np.zeros((len(gains), 11))
    s[:, 8] = gains
    return s


def test_standings_order_ties_and_nan():
    zero = _states([0.0] * 4)
    # one member, four cars alone in their races: the sum runs upwards from +0.0, every addition rounded
    up = LS.standings(zero, _states([1e16, 1.0, 1.0, 1.0]), np.full(4, -5), [0] * 4, 1, 1, 4)
    assert up[0].tolist() == [4.0, 1e16, 0.0, 0.0] and up[0, 1] != ((1.0 + 1.0) + 1.0) + 1e16
    # ... in ascending CAR index, whatever the order of the entries' members
    mixed = LS.standings(zero, _states([1.0, 1e16, 1.0, 1.0]), np.full(4, -5), [1, 0, 1, 1], 2, 1, 4)
    assert mixed[1].tolist() == [3.0, 3.0, 0.0, 0.0] and mixed[0, 1] == 1e16
    # one race of four: alive first, the gain breaks ties, equal pairs and NaN beat nobody
    first = np.array([-5, 2, 2, -5])
    st = LS.standings(zero, _states([1.0, 5.0, 5.0, np.nan]), first, [0, 1, 2, 3], 4, 4, 4)
    assert st[:, 0].tolist() == [1.0] * 4 and st[:, 2].tolist() == [0.0, 1.0, 1.0, 0.0]
    assert st[:, 3].tolist() == [2.0, 0.0, 0.0, 2.0]               # 0 and 3 outlive 1 and 2; NaN against 1.0: nobody
    assert np.isnan(st[3, 1])
    later = LS.standings(zero, _states([1.0, 5.0, 4.0, 2.0]), np.array([-5, 2, 2, -5]), [0, 1, 2, 3], 4, 4, 4)
    assert later[:, 3].tolist() == [2.0, 1.0, 0.0, 3.0]
    # a crash at the last tick is not "never crashed"
    edge = LS.standings(zero[:2], _states([1.0, 1.0]), np.array([3, -5]), [0, 1], 2, 2, 4)
    assert edge[:, 3].tolist() == [0.0, 1.0]


# ---------------------------------------------------------------- the header
def test_league_header_is_pinned_to_league_symbols():
    protos = LEAGUE_HEADER.prototypes()
    # rl_car_race_league: rl_car_race_seats' arguments from states_in on, behind its own six, the standings last
    names = protos["rl_car_race_league"][2]
    assert names[:6] == ["c", "h", "g_or_null", "pop", "entry_RP", "steer_clip"]
    seats = _lib.SEAT_SYMBOLS["rl_car_race_seats"][1]
    assert protos["rl_car_race_league"][1][6:] == list(seats[6:]) + [_lib.f64p]
    assert names[6] == "states_in" and names[-2] == "states_trace_or_null" and names[-1] == "standings_N4_or_null"
    # the row forms: rl_policy_pop_eval's without first / n / cars_per_member, the member array behind n
    assert protos["rl_policy_pop_eval_rows"][2] == ["pop", "n", "member_n", "scans", "size", "steers"]
    ev = list(_lib.POP_SYMBOLS["rl_policy_pop_eval"][1])
    assert protos["rl_policy_pop_eval_rows"][1] == [ev[0], C.c_int, _lib.i32p] + ev[4:]
    assert protos["rl_policy_pop_eval_rows_device"][2][-1] == "hip_stream"
    assert not LEAGUE_HEADER.structs() and not LEAGUE_HEADER.handles()
    raw = open(LEAGUE_HEADER.path).read()
    assert '#include "scanlib_population.h"' in raw and '#include "scanlib_seats.h"' in raw
    assert "Out of scope" in raw and "Errors (RL_ERR_INVALID" in raw
    for phrase in ("ascending car index", "keeps its bits", "never clipped", "ties and\n *            NaN beat nobody",
                   "ceil(n / 8) + min(n, n_members)", "rl_car_race_followgap bit for bit", "rl_car_drive_population"):
        assert phrase in raw, phrase
    import pyracecarsimulator_amd as P
    assert P.league is league and P.round_robin is league.round_robin and {"league", "round_robin"} <= set(P.__all__)
    assert hasattr(P.RacecarSimulator, "raceLeagueMany") and hasattr(P.PolicyPopulation, "predict_rows_device")


# ---------------------------------------------------------------- round_robin
@pytest.mark.parametrize("N,P", [(5, 3), (4, 4), (6, 2), (3, 1), (9, 4)])
def test_round_robin_is_balanced(N, P):
    rr = league.round_robin(N, P)
    per_seat = math.comb(N - 1, P - 1)
    assert rr.dtype == np.int32 and rr.shape == (math.comb(N, P) * P, P)
    assert all(len(set(row)) == P and 0 <= min(row) and max(row) < N for row in rr.tolist())
    for k in range(P):                                              # every member in every seat equally often
        assert np.bincount(rr[:, k], minlength=N).tolist() == [per_seat] * N
    lineups = {}
    for row in rr.tolist():
        lineups.setdefault(tuple(sorted(row)), []).append(row)
    assert set(lineups) == set(itertools.combinations(range(N), P))  # every unordered line-up of distinct members
    for combo, races in lineups.items():                            # ... with each of its members once in each seat
        assert len(races) == P
        for k in range(P):
            assert sorted(r[k] for r in races) == list(combo)


# ---------------------------------------------------------------- the wrappers' refusals
def test_league_refuses_before_the_library(no_calls):  # noqa: F811
    for N, P in ((2, 3), (3, 0), (9, 9)):
        with pytest.raises(ValueError):
            league.round_robin(N, P)
    pop = _pop()                                                    # 5 members on the window [5, 45)
    scans = np.zeros((6, 64), np.float32)
    ok = np.array([0, 4, -1, 2, 2, 1])
    for sc, mem, kw in ((scans.astype(np.float64), ok, {}), (scans.reshape(-1), ok, {}), (scans, ok[:5], {}),
                        (scans, ok.astype(np.float64), {}), (scans, ok.reshape(2, 3), {}),
                        (scans, np.array([0, 5, -1, 2, 2, 1]), {}), (scans, np.array([0, -2, -1, 2, 2, 1]), {}),
                        (scans[:, :44], ok, {}), (scans, ok, dict(out=np.zeros(6))), (scans, ok, dict(out=np.zeros(5, np.float32)))):
        with pytest.raises(ValueError):
            pop.predict_rows(sc, mem, **kw)
    for n, size in ((-1, 64), (6, 44)):
        with pytest.raises(ValueError):
            pop.predict_rows_device(0, 0, n, size, 0)
    cars = RC.CarBatch.__new__(RC.CarBatch)
    st, edge, fg = np.zeros((2, 3, 11)), np.zeros(64), object()
    good = dict(entries=np.array([[0, -1, 4], [1, 1, 2]]), states=st, n_ticks=4, speed=2.0, fov=4.7, num_rays=64, edge=edge,
                crash_thresh=0.001, followgap=fg)
    for kw in (dict(entries=np.array([[0, -1, 5], [1, 1, 2]])), dict(entries=np.array([[0, -2, 4], [1, 1, 2]])),
               dict(entries=np.array([0, -1, 4, 1, 1, 2])), dict(entries=np.array([[0, -1, 4]])),
               dict(entries=np.array([[0.0, -1.0, 4.0], [1.0, 1.0, 2.0]])), dict(followgap=None),
               dict(states=np.zeros((1, 9, 11)), entries=np.zeros((1, 9), int)), dict(states=st.astype(np.float32)),
               dict(states=st.reshape(6, 11)), dict(steer_clip=0.0), dict(steer_clip=-1.0),
               dict(num_rays=44, edge=np.zeros(44)), dict(edge=np.zeros(63)), dict(speed=np.zeros(5)),
               dict(steer0=np.zeros((2, 3)))):
        args = dict(good, **kw)
        with pytest.raises(ValueError):
            cars.race_league(None, pop, args.pop("entries"), args.pop("states"), **args)
    # what is no refusal: -1 nowhere needs no FollowGap, and the window is only the members' business
    assert league.league_args(np.array([[0, 1, 2]]), 1, 3, pop, None, 64).tolist() == [0, 1, 2]
    assert league.league_args(np.array([[-1, -1]]), 1, 2, pop, fg, 20).dtype == np.int32
