"""Policy populations without a GPU: θ's order and the statements (tests/population_statement.py) on a fake
one-dimensional world, what include/scanlib_population.h says beyond its prototypes (tests/test_py_calls_host.py pins
those to ``_lib.POP_SYMBOLS``), and every Python-side refusal."""
import ctypes as C
import re

import numpy as np
import pytest

import policy_statement as S
import population_statement as PS
import scanlib_header as H
from test_race_env_host import B, World1D, _lineup
from pyracecarsimulator_amd import PolicyPopulation, _lib, population
from pyracecarsimulator_amd import racecar as RC
from pyracecarsimulator_amd.policy import Policy

POP_HEADER = H.read("scanlib_population.h")
DIMS = (13, 7, 5, 1)


def _layers(dims, seed):
    rng = np.random.default_rng(seed)
    return [((rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32),
             (0.1 * rng.standard_normal(dims[i + 1])).astype(np.float32)) for i in range(len(dims) - 1)]


# ---------------------------------------------------------------- θ
def test_pack_unpack_round_trip_and_order():
    layers = _layers(DIMS, 1)
    theta = population.pack(layers)
    assert theta.dtype == np.float32 and theta.shape == (population.n_params(DIMS),) == (14 * 7 + 8 * 5 + 6 * 1,)
    assert population.n_params((720, 64, 128, 128, 64, 1)) == 79297
    assert theta.tobytes() == PS.pack(layers).tobytes()
    back = population.unpack(theta, DIMS)
    for (W, b), (W2, b2), (W3, b3) in zip(layers, back, PS.unpack(theta, DIMS)):
        assert W.tobytes() == W2.tobytes() == W3.tobytes() and b.tobytes() == b2.tobytes() == b3.tobytes()
    assert population.pack(back).tobytes() == theta.tobytes()
    # the order, spelt out: W[0] row-major first, b[0] behind it, then layer 1
    assert theta[0] == layers[0][0][0, 0] and theta[1] == layers[0][0][0, 1] and theta[7] == layers[0][0][1, 0]
    assert theta[13 * 7] == layers[0][1][0] and theta[14 * 7] == layers[1][0][0, 0] and theta[-1] == layers[2][1][0]
    # the statement's network of the unpacked layers is the network of the layers
    scans = np.random.default_rng(2).uniform(0, 18, (4, 20)).astype(np.float32)
    relu = (True, True, False)
    assert S.forward(scans, back, relu, in_start=3).tobytes() == S.forward(scans, layers, relu, in_start=3).tobytes()
    for bad in (theta[:-1], theta.astype(np.float64), theta[None, :]):
        with pytest.raises(ValueError):
            population.unpack(bad, DIMS)
    with pytest.raises(ValueError):
        population.pack([layers[0], layers[2]])


def test_eval_statement_is_member_of_row_then_policy_statement():
    """3 members x 3 cars from member 1 of 5: row i by member 1 + i // 3, every member the same 3 scans."""
    thetas = np.stack([population.pack(_layers(DIMS, 10 + m)) for m in range(5)])
    relu = (True, True, False)
    scans = np.tile(np.random.default_rng(3).uniform(0, 18, (3, 16)).astype(np.float32), (3, 1))
    got = PS.evaluate(thetas, DIMS, relu, scans, 3, first=1, n=3, in_start=2)
    assert [PS.member_of(i, 1, 3) for i in range(9)] == [1, 1, 1, 2, 2, 2, 3, 3, 3]
    for m in range(3):
        want = S.forward(scans[:3], _layers(DIMS, 11 + m), relu, in_start=2)
        assert got[3 * m:3 * m + 3].tobytes() == want.tobytes()
    assert len({got[3 * m:3 * m + 3].tobytes() for m in range(3)}) == 3


# ---------------------------------------------------------------- the roll-out on the fake world
def test_population_rollout_statement():
    """Six cars alone in their corridors, 2 cars a member, members 1 ... 3: car r gets member 1 + r // 2's answer (not
    r % 3's, not (1 + r) // 2's), the clip clamps what the car gets and not what `steers` records, a wreck stops, and
    the fitness sum runs in ascending car order."""
    w = World1D(1)
    states = _lineup(0.0, 1.0, 2.0, 3.0, 4.0, 8.5)
    states[:, 8] = [0.25, 0.5, 1e16, 3.0, 0.125, 7.0]
    speeds = np.array([1.0, 1.0, 1.0, 3.0, 1.0, 5.0])
    seen = []

    def answer(member, row):
        assert row.shape == (B,) and row.dtype == np.float32
        seen.append(member)
        return np.float32(row[0]) / np.float32(10.0 * member)

    first, final, steers, trace, fit = PS.population_rollout(
        states, speeds, np.zeros(6, np.float32), 3, 1, 2, 0.5, w.step_cars, w.scan, World1D.is_crashed, answer,
        scan_dist_to_base=0.0)
    assert w.slots == [0, 1, 2]
    assert seen[:6] == [1, 1, 2, 2, 3, 3]
    assert first.tolist() == [-4, -4, -4, -4, -4, 1]               # car 5: 9.0, 9.5
    assert np.isnan(steers[5, 1:]).all() and np.isnan(trace[5, 2]).all() and final[5, 0] == 9.5
    # tick 0: car 0 at 0.1 reads 9.9 -> member 1 answers 0.99, the car gets 0.5 at tick 1's step
    assert steers[0, 0] == np.float32(9.9) / np.float32(10.0) and trace[0, 1, 4] == 0.5
    # car 2 at 2.1 is member 2's: 7.9 / 20, under the clip
    assert steers[2, 0] == np.float32(7.9) / np.float32(20.0) and np.float32(trace[2, 1, 4]) == steers[2, 0]
    # car 4 at 4.1 is member 3's
    assert steers[4, 0] == np.float32(5.9) / np.float32(30.0)
    # fitness: 0.1 a tick and car; member 1 (cars 2, 3) adds a difference lost against 1e16 first
    d = final[:, 8] - states[:, 8]
    assert fit[:, 1].tolist() == [0.0, 0.0, 1.0]
    assert fit[0, 0] == (0.0 + d[0]) + d[1] and fit[1, 0] == (0.0 + d[2]) + d[3] and fit[2, 0] == (0.0 + d[4]) + d[5]
    assert d[2] == 0.0 and abs(d[3] - 0.9) < 1e-12 and d[5] == 1.0
    # the order is the contract: summed downwards the same terms round differently
    big = np.array([[0.0] * 8 + [v] + [0.0] * 2 for v in (1e16, 1.0, 1.0, 1.0)])
    zero = np.zeros_like(big)
    up = PS.fitness(zero, big, np.full(4, -1), 4)[0, 0]
    assert up == 1e16 and up != ((1.0 + 1.0) + 1.0) + 1e16


# ---------------------------------------------------------------- the header
def test_population_header_is_pinned_to_pop_symbols():
    protos = POP_HEADER.prototypes()
    assert all(res is C.c_int or name == "rl_policy_pop_destroy" for name, (res, _, _) in protos.items())
    # rl_car_drive_population: rl_car_drive_policy's arguments behind its own seven, steer_clip moved up, fitness last
    names = protos["rl_car_drive_population"][2]
    assert names[:7] == ["c", "h", "pop", "first", "n", "cars_per_member", "steer_clip"]
    pol = list(_lib.SYMBOLS["rl_car_drive_policy"][1])
    assert protos["rl_car_drive_population"][1][7:] == pol[3:6] + pol[7:14] + pol[15:] + [_lib.f64p]
    assert names[-1] == "fitness_n2_or_null"
    # rl_policy_pop_create: rl_policy_create's without the weights, n_members second
    create = list(_lib.SYMBOLS["rl_policy_create"][1])
    assert protos["rl_policy_pop_create"][1] == create[:1] + [C.c_int] + create[1:3] + create[5:]
    assert not POP_HEADER.structs()
    assert re.search(r"typedef\s+struct\s+rl_policy_pop\s+rl_policy_pop\s*;", POP_HEADER.text())
    raw = open(POP_HEADER.path).read()
    assert '#include "scanlib.h"' in raw and "Out of scope" in raw and "Errors (RL_ERR_INVALID" in raw
    assert "first + i / E" in raw and "first + r / E" in raw and "ascending car order" in raw


# ---------------------------------------------------------------- the wrappers' refusals
@pytest.fixture
def no_calls(monkeypatch):
    def refuse(name, *a):
        raise AssertionError("the library was entered at %s" % name)
    monkeypatch.setattr(_lib, "call", refuse)


def _pop(n_members=5, dims=(40, 16, 8, 1), in_start=5):
    """A population object that never saw the library."""
    pop = PolicyPopulation.__new__(PolicyPopulation)
    pop.dims, pop.relu, pop.n_members, pop.n_params = dims, (True, True, False), n_members, population.n_params(dims)
    pop.in_start, pop.clip, pop.scale, pop.device = in_start, 15.0, 15.0, 0
    return pop


def test_population_refuses_before_the_library(no_calls):
    for kw in (dict(dims=(40,), n_members=2), dict(dims=(40, 8, 1), n_members=0),
               dict(dims=(40, 8, 1), n_members=2, relu=(True,))):
        with pytest.raises(ValueError):
            PolicyPopulation(**kw)
    pop = _pop()
    P = pop.n_params
    ok = np.zeros((2, P), np.float32)
    for theta, first in ((ok.astype(np.float64), 0), (ok[:, :-1], 0), (ok[None], 0), (ok, 4), (ok, -1),
                         (np.zeros((6, P), np.float32), 0)):
        with pytest.raises(ValueError):
            pop.set(theta, first)
    for m in (-1, 5):
        with pytest.raises(ValueError):
            pop.get(m)
        with pytest.raises(ValueError):
            pop.member(m)
    with pytest.raises(ValueError):
        pop.set_device(ok)                                          # a host array is no device tensor
    import torch
    for t in (torch.zeros((2, P), dtype=torch.float64), torch.zeros((2, P + 1), dtype=torch.float32)[:, :P],
              torch.zeros((2, P), dtype=torch.float32)):            # (the last one: on the CPU)
        with pytest.raises(ValueError):
            pop.set_device(t)
    scans = np.zeros((6, 64), np.float32)
    for args, kw in (((scans.astype(np.float64), 3), {}), ((scans.reshape(-1), 3), {}), ((scans, 0), {}),
                     ((scans, 4), {}),                              # 6 rows are no whole number of 4-car members
                     ((scans, 1), {}),                              # 6 members of 5
                     ((scans, 3), dict(first=4)), ((scans, 3), dict(n=3)), ((scans, 3), dict(first=-1)),
                     ((scans[:, :44], 3), {})):                     # the window [5, 45)
        with pytest.raises(ValueError):
            pop.predict_many(*args, **kw)
    with pytest.raises(ValueError):
        pop.predict_device(0, 3, 64, 0, first=3, n=3)
    with pytest.raises(ValueError):
        PolicyPopulation.from_policies([])
    a, b = Policy.__new__(Policy), Policy.__new__(Policy)
    a.dims, a.relu, a.in_start, a.clip, a.scale, a.device = (40, 8, 1), (True, False), 5, 15.0, 15.0, 0
    b.dims, b.relu, b.in_start, b.clip, b.scale, b.device = (40, 9, 1), (True, False), 5, 15.0, 15.0, 0
    with pytest.raises(ValueError, match="one architecture"):
        PolicyPopulation.from_policies([a, b])


def test_drive_population_refuses_before_the_library(no_calls):
    pop = _pop()
    cars = RC.CarBatch.__new__(RC.CarBatch)
    st, edge = np.zeros((6, 11)), np.zeros(64)
    ok = dict(states=st, n_ticks=4, speed=2.0, fov=4.7, num_rays=64, edge=edge, crash_thresh=0.001, cars_per_member=3)
    for kw in (dict(cars_per_member=0), dict(cars_per_member=4), dict(first=4), dict(first=-1), dict(steer_clip=0.0),
               dict(steer_clip=-1.0), dict(num_rays=44, edge=np.zeros(44)), dict(states=st.astype(np.float32)),
               dict(states=st[0]), dict(edge=np.zeros(63)), dict(speed=np.zeros(5)), dict(steer0=np.zeros(6)),
               dict(cars_per_member=1)):                            # 6 members of 5
        with pytest.raises(ValueError):
            cars.drive_population(None, pop, **dict(ok, **kw))
