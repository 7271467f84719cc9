#!/usr/bin/env python3
"""CPU census of the seeds tests/test_gpu_population.py runs (no GPU): the roll-out statement of
tests/population_statement.py over the oracle's scan (noise off), the compiled reference Car and the network's host
statement.  Prints, per roll-out case, what the reference alone meets of the censuses the GPU tests assert on the
device's own run: the members' steer traces differ pairwise, a car crashes, a car finishes, an answer passes the clip.
docs/history/population.md records the output.  The last lines are the shapes past one block of work
(tests/network_scale.py: 67 members x 3 cars, 130 x 1) with the censuses tests/test_gpu_network_scale.py asserts;
docs/history/network_scale.md records those.

usage: python tools/population_census.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import policy_statement as S                  # noqa: E402
import population_statement as PS             # noqa: E402
import support                                # noqa: E402
import test_gpu_population as TG              # noqa: E402
from oracle import oracle as O                # noqa: E402
from oracle import reference                  # noqa: E402
from pyracecarsimulator_amd import maps       # noqa: E402
from support import FOV, THRESH               # noqa: E402


class World:
    """The statement's callbacks from the oracle and the reference Car."""

    def __init__(self, g, name, B, layer_lists):
        self.B, self.edge = B, support.oracle_edge(O, B)
        self.car = reference.RefCar()
        self.om = O.OracleMap(g.occ, g.resolution, g.origin, TG.MRX)
        dims, self.in_start, relu, _ = TG.NETS[name]
        self.relu = relu or tuple(i < len(dims) - 2 for i in range(len(dims) - 1))
        self.members = layer_lists

    def step_cars(self, states, speed, steer):
        return np.stack([self.car.step(s, v, a) for s, v, a in zip(states, speed, steer)])

    def scan(self, poses, cars, t):
        return self.om.rm_fan(np.ascontiguousarray(poses, np.float32), FOV, self.B, step_coeff=1.0)[0].reshape(-1, self.B)

    def is_crashed(self, r):
        return O.is_crashed(np.ascontiguousarray(r), self.B, 1, self.edge, THRESH) >= 0

    def answer(self, member, row):
        return S.forward(row[None], self.members[member], self.relu, in_start=self.in_start)[0]


def rollout_case(g, dt, name, cfg, B, n, E, T, clip):
    rig = dict(g=g, dt=dt)
    states, speeds = TG.rollout_starts(rig, cfg, n)
    w = World(g, name, B, TG.members(name, n, cfg.get("net_seed", 1), cfg.get("gain", 1.0)))
    first, final, steers, trace, fit = PS.population_rollout(states, speeds, np.zeros(n * E, np.float32), T, 0, E, clip,
                                                            w.step_cars, w.scan, w.is_crashed, w.answer)
    blocks = [steers[k * E:(k + 1) * E] for k in range(n)]
    ok = np.isfinite(steers)
    print("roll-out %s B %d, %d members x %d cars, %d ticks, seeds %s: members differ pairwise %s, %d of %d cars crash "
          "(ticks %s), %d finish, %d answers beyond %.1f (max |answer| %.3f), fitness %s"
          % (name, B, n, E, T, {k: v for k, v in cfg.items() if "seed" in k}, TG.differ_pairwise(blocks),
             (first >= 0).sum(), n * E, sorted(first[first >= 0].tolist()), (first < 0).sum(),
             (np.abs(steers[ok]) > TG.CLIP).sum(), TG.CLIP, np.abs(steers[ok]).max(), np.round(fit[:, 0], 3).tolist()))


def main():
    O.build()
    g = maps.make_maze(512, cell=40, wall=3, p=0.45, seed=11)
    dt = O.edt(g.occ)
    for B in (64, 65):
        rollout_case(g, dt, "small", TG.ROLLOUT, B, 3, 5, 25, TG.CLIP)
    rollout_case(g, dt, "fixture", TG.ROLLOUT_FIXTURE, 1081, 3, 5, 25, TG.CLIP)
    # the shapes past one block (tests/network_scale.py, tests/test_gpu_network_scale.py)
    import network_scale as NS
    for n, E in sorted(NS.ROLLOUTS):
        first, final, steers, trace, fit = NS.rollout_cpu(O, reference, g, dt, n, E)
        ok = np.isfinite(steers)
        print("roll-out past one block, %d members x %d cars, B %d, %d ticks, seeds %s: %s; %d of %d cars crash, %d of "
              "them of members >= 64, crash counts %s, %d answers beyond %.1f, %d distinct fitness sums"
              % (n, E, NS.ROLLOUT_B, NS.ROLLOUT_T, {k: v for k, v in NS.ROLLOUTS[(n, E)].items() if "seed" in k},
                 NS.rollout_census(first, steers, fit, n, E, TG.CLIP), (first >= 0).sum(), n * E,
                 (first[64 * E:] >= 0).sum(), sorted(set(fit[:, 1].astype(int).tolist())),
                 (np.abs(steers[ok]) > TG.CLIP).sum(), TG.CLIP, len(set(fit[:, 0].tolist()))))


if __name__ == "__main__":
    main()
