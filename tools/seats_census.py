#!/usr/bin/env python3
"""CPU census of the seeds tests/test_gpu_seats.py runs (no GPU): the statements of tests/seat_statement.py over the
oracle's stamped-grid scan (drive_cases.race_oracle_fan, noise off), the compiled reference Car, the oracle's FollowGap
and the network's host statement.  Prints, per case, what the reference alone meets of the censuses the GPU tests
assert: crashes, clamped policy answers, rays the other cars changed, attrition and re-spawn, a wreck seen by a
scripted car.  docs/history/seats.md records the output.  The last lines are the seated envs across the step kernel's
64-lane blocks (tests/network_scale.py: 69 and 72 cars) with the censuses tests/test_gpu_network_scale.py asserts;
docs/history/network_scale.md records those.

usage: python tools/seats_census.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import drive_cases as DC                      # noqa: E402
import policy_statement as PS                 # noqa: E402
import race_statement as RS                   # noqa: E402
import seat_statement as SS                   # noqa: E402
import support                                # noqa: E402
import test_gpu_seats as TG                   # noqa: E402
from oracle import oracle as O                # noqa: E402
from oracle import reference                  # noqa: E402
from support import FOV, MAX_STEER, THRESH    # noqa: E402

LENGTH, WIDTH = 0.4064, 0.2032
FG, NET = "fg", "net"


class World:
    """The statements' callbacks from the oracle and the reference Car."""

    def __init__(self, g, group, B, substeps=1):
        self.g, self.P, self.B, self.S = g, group, B, substeps
        self.edge = support.oracle_edge(O, B)
        self.car = reference.RefCar()
        self.plain = O.OracleMap(g.occ, g.resolution, g.origin, DC.RACE_MRX)
        self.layers = TG.small_net()
        self.relu = [True, True, False]
        self.seen = 0

    def step_cars(self, states, speed, steer):
        return np.stack([self.car.step(s, v, a, n=self.S) for s, v, a in zip(states, speed, steer)])

    def scan(self, poses, cars, k):
        g = self.g
        cells = RS.outline_cells(cars, LENGTH, WIDTH, g.resolution, g.origin, g.rows, g.cols, O.sincosf)
        r = DC.race_oracle_fan(O, g, cells, self.P, np.ascontiguousarray(poses, np.float32), self.B, False, 1.0)[0]
        alone = self.plain.rm_fan(np.ascontiguousarray(poses, np.float32), FOV, self.B, step_coeff=1.0)[0]
        self.seen += int((r != alone).sum())
        return r.reshape(-1, self.B)

    def is_crashed(self, r):
        return O.is_crashed(np.ascontiguousarray(r), self.B, 1, self.edge, THRESH) >= 0

    def answer(self, driver, row):
        if driver == FG:
            return np.float32(O.followgap_eval(np.ascontiguousarray(row), 15.0, MAX_STEER, 0.004))
        return PS.forward(row[None], self.layers, self.relu, in_start=5)[0]


def rollout_case(g, dt, P, B, mix, seed, R, T):
    w = World(g, P, B)
    states, speeds = TG._race_starts(g, dt, R, P, seed)
    seats = [FG if c == "f" else NET for c in mix]
    first, final, steers, trace = SS.seated_rollout(
        states.reshape(-1, 11), (speeds + 2.0).reshape(-1), np.zeros(R * P, np.float32), T, seats, lambda d: d == NET,
        TG.CLIP, w.step_cars, w.scan, w.is_crashed, w.answer)
    net = np.array([s == NET for s in seats] * R)
    clamped = int((np.abs(steers[net, :-1]) > TG.CLIP).sum())
    print("roll-out P %d B %d seats %s seed %d: %d of %d cars crash (ticks %s), %d policy answers clamped, %d rays "
          "changed by other cars" % (P, B, mix, seed, (first >= 0).sum(), R * P, sorted(first[first >= 0].tolist()),
                                     clamped, w.seen))


def env_case(g, dt):
    E = TG.ENV
    R, P, B = E["R"], E["P"], E["B"]
    w = World(g, P, B, E["S"])
    pool, _ = TG._race_starts(g, dt, E["M"], P, E["pool_seed"])
    pool[:, :, 3] = 3.0
    kw = {k: v for k, v in TG.ENV_KW.items() if k != "substeps"}
    stmt = SS.SeatEnvStatement(pool, R, B, w.step_cars, w.scan, w.is_crashed, w.answer, [None, FG, NET], E["speed"],
                               **TG.WINDOW, **kw)
    obs, done = stmt.reset(E["seed"])
    print("env reset: done", done.tolist())
    census = dict(scripted_crash=0, attrition=0, respawned=0, clamped=0, wreck_steps=0, bad=0)
    for k, a in enumerate(TG.env_actions(), 1):
        before, over = stmt.done.copy(), stmt.race_over.copy()
        running = (before == 0) & np.repeat(over == 0, P)
        scripted = np.array([stmt.scripted(e) for e in range(R * P)])
        census["clamped"] += int((running & (np.arange(R * P) % P == 2) & (np.abs(stmt.steers) > TG.CLIP)).sum())
        obs, rew, done = stmt.step(a.reshape(-1, 2))
        census["scripted_crash"] += int((running & scripted & (done == 1)).sum())
        census["bad"] += int((done == 3).sum())
        census["attrition"] += int((stmt.race_over == 1).sum())
        census["respawned"] = int((stmt.race_episode > 0).sum())
        wrecks = (stmt.done != 0) & np.repeat(stmt.race_over == 0, P)
        census["wreck_steps"] += int(wrecks.any())
    print("env seed %d pool %d: %s" % (E["seed"], E["pool_seed"], census))


def main():
    O.build()
    g = DC.race_maze()
    dt = O.edt(g.occ)
    for P, B, mix, seed, R, T in ((3, 64, "fff", 52, 5, 40), (8, 65, "ffffffff", 58, 5, 40), (1, 64, "f", 51, 5, 40),
                                  (3, 65, "fpf", 52, 5, 30), (8, 64, "pfpppfpf", 58, 2, 24)):
        rollout_case(g, dt, P, B, mix, seed, R, T)
    env_case(g, dt)
    # the seated envs across the step kernel's blocks (tests/network_scale.py, tests/test_gpu_network_scale.py)
    import network_scale as NS
    for name, case in sorted(NS.SEAT_ENVS.items()):
        census = NS.seat_env_cpu(O, reference, g, dt, case, TG.small_net())
        print("env across blocks %s: %d races x %d cars, B %d, pool seed %d (%d line-ups, clear %.0f px), seat speeds %s, "
              "%d steps: %s -> %s" % (name, case["R"], case["P"], case["B"], case["pool_seed"], case["M"],
                                      NS.SEAT_CLEAR_PX, case["speed"], case["steps"], census.seen,
                                      "ok" if census.ok() else "MISSING"))


if __name__ == "__main__":
    main()
