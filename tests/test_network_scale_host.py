"""The cases of tests/test_gpu_network_scale.py without a GPU: every shape reaches the launch geometry it is there for
(read from the sources, so that a change of a grid cap or of a workgroup's size fails here and does not quietly stop the
GPU cases from testing), and every census the GPU cases assert on the device's own run holds on the CPU from the
statements alone: the oracle's scan, the compiled reference Car, the oracle's FollowGap and the network's host
statement.  The seeds were picked with these runs (tools/population_census.py, tools/seats_census.py)."""
import os
import re

import numpy as np
import pytest

import drive_cases as DC
import network_scale as NS
import test_gpu_population as TP
import test_gpu_seats as TSE
from conftest import ROOT
from oracle import oracle as O
from oracle import reference
from pyracecarsimulator_amd import maps, population

CSRC = os.path.join(ROOT, "pyracecarsimulator_amd", "csrc")
FIXTURE_DIMS = (720, 64, 128, 128, 64, 1)


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _const(text, name):
    return int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text).group(1))


# ---------------------------------------------------------------- the launch geometry the shapes are there for
def test_pack_case_crosses_the_grid_cap_of_the_launch():
    abi = _src("abi_car.hip")
    m = re.search(r"std::min<size_t>\(\(total \+ (\d+)\) / (\d+), (\d+)\);\s*return launch\(\"policy_pop_pack_kernel\", policy_pop_pack_kernel, "
                  r"dim3\(grid\), dim3\((\d+)\)", abi)
    assert m, "pop_pack_launch no longer reads as the case assumes"
    assert int(m.group(1)) + 1 == int(m.group(2)) == int(m.group(4)) == NS.PACK_THREADS
    assert int(m.group(3)) == NS.PACK_GRID_CAP
    kern = _src("policy_kernels.h")
    assert "blockIdx.x * %d + threadIdx.x; e < total; e += (size_t)gridDim.x * %d" % (NS.PACK_THREADS, NS.PACK_THREADS) in kern
    P = population.n_params(FIXTURE_DIMS)
    trip, member, param = NS.pack_wrap(P)
    c = NS.PACK
    assert (P, trip, member, param) == (79297, 16777216, 211, 45549)
    assert c["control_n"] * P <= trip < c["n"] * P                   # the control stays inside one trip, the case wraps
    assert c["n"] - member >= 4                                      # whole members on the far side of the wrap
    assert c["first"] >= 3 and c["first"] + c["n"] + 2 <= c["members"]             # untouched members on both sides
    th = NS.pack_thetas(3, 50)
    assert th.dtype == np.float32 and len({t.tobytes() for t in th}) == 3 and np.abs(th).max() < 1.0


def test_population_shapes_reach_a_third_workgroup_a_member_and_a_second_block():
    kern = _src("policy_kernels.h")
    pm = _const(kern, "PM_CARS")
    assert "const int m = blockIdx.x / wg_per_member, chunk = blockIdx.x - m * wg_per_member;" in kern
    assert "const int m = blockIdx.x * 64 + threadIdx.x;" in kern
    abi = _src("abi_car.hip")
    assert "policy_pop_fitness_kernel, dim3((src.n + 63) / 64), dim3(64)" in abi     # (src.n: the members of the call)
    assert "const int wg = (E + PM_CARS - 1) / PM_CARS;" in abi
    seen = set()
    for name, n, E in NS.EVAL:
        wg = (E + pm - 1) // pm
        seen.add((wg >= 3, E % pm))
        assert n * wg > 10 and n > 64 and n % 64 != 0, (name, n, E)
        assert TP.NETS[name][3] >= TP.NETS[name][1] + TP.NETS[name][0][0]
    assert (True, 1) in seen and (False, 1) in seen                 # 3 workgroups with 1 car in the last; 1 car a member
    f, k = NS.SUB["first"], NS.SUB["n"]
    assert f < 64 < f + k <= min(n for _, n, _ in NS.EVAL)
    for n, E in NS.ROLLOUTS:
        assert n > 64 and n % 64 != 0 and n * E <= 201 and f + k <= n
    assert any(E >= 3 for _, E in NS.ROLLOUTS)                      # the order of the fitness sum shows from 3 terms on


def test_seat_shapes_put_a_race_across_the_step_kernels_blocks():
    env = _src("env_kernels.h")
    assert "Races straddle blocks" in env and "S.answer[e]" in env
    for name, c in NS.SEAT_ENVS.items():
        N, P = c["R"] * c["P"], c["P"]
        assert 64 < N <= 128 and len(c["mix"]) == P == len(c["speed"]), name
        past = [c["mix"][e % P] for e in range(64, N)]
        assert "p" in past and "f" in past and (name != "pfc" or "c" in past), name      # every kind of row in block 1
        assert c["watch"] * P < 64, name
    c = NS.SEAT_ENVS["pfp"]
    assert c["watch"] * c["P"] < 64 < (c["watch"] + 1) * c["P"]                           # race 21 = cars 63, 64, 65
    pm = _const(_src("policy_kernels.h"), "PM_CARS")
    for R, P, B, mix, seed in NS.SEAT_ROLLOUTS:
        rows = mix.count("p") * R
        assert R * P > 64 and (rows + pm - 1) // pm == 6 and rows % pm != 0, (R, P, mix)
        # the part-filled last workgroup holds rows of cars past car 63
        cars = [e for e in range(R * P) if mix[e % P] == "p"]
        assert cars[(rows // pm) * pm] <= 63 < cars[-1] or cars[(rows // pm) * pm] > 63


def test_track_shapes_reach_a_second_workgroup():
    abi = _src("abi_car.hip")
    assert "rollout_xy_kernel, dim3((R + 63) / 64), dim3(64)" in abi and "rollout_xy_kernel, dim3((K + 63) / 64), dim3(64)" in abi
    assert "const int r = blockIdx.x * blockDim.x + threadIdx.x;" in _src("plan_track_kernels.h")
    assert NS.TRACK_R == (64, 65, 130)                              # one full block, one lane of a second, a third
    assert NS.TREES["K"] == 65 and (NS.TREES["K"] + 7) // 8 > 2


# ---------------------------------------------------------------- the censuses, from the statements alone
@pytest.fixture(scope="module")
def cpu():
    reference.require()
    O.build()
    return O


@pytest.mark.parametrize("n,E", sorted(NS.ROLLOUTS))
def test_rollout_census_holds_on_the_cpu(cpu, n, E):
    """The fitness sums pairwise distinct, a car of a member >= 64 crashes and one does not, the crash counts take two
    values, an answer passes the clip."""
    g = maps.make_maze(512, cell=40, wall=3, p=0.45, seed=11)
    first, final, steers, trace, fit = NS.rollout_cpu(O, reference, g, O.edt(g.occ), n, E)
    census = NS.rollout_census(first, steers, fit, n, E, TP.CLIP)
    assert all(census.values()), census
    assert fit.shape == (n, 2) and (fit[:, 1] == (first >= 0).reshape(n, E).sum(1)).all()


@pytest.mark.parametrize("name", sorted(NS.SEAT_ENVS))
def test_seat_env_census_holds_on_the_cpu(cpu, name):
    """Among the cars past car 63: a scripted seat crashes, a finished race re-spawns, a policy answer is clamped; the
    race that straddles the blocks finishes and re-spawns; no start and no answer is refused."""
    g = DC.race_maze()
    census = NS.seat_env_cpu(O, reference, g, O.edt(g.occ), NS.SEAT_ENVS[name], TSE.small_net())
    assert census.ok(), census.seen
