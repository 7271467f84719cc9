#!/usr/bin/env python3
"""The MCTS planner: microseconds per iteration of rl_mcts_run against its roll-out floor and against the same search
composed on the host from the public calls, in one process.

Per map (cfg2's 2049^2 maze, colombia) and tree count K (1, 64, 1024, 4096), RMGPU, 1081 beams, FG source,
L = 200 roll-out steps (mcts.py's roll_out_itr), n iterations after a reset:
  planner   MCTSPlanner.run(n): per iteration select, act scan, act kernel, roll-out, roll-out scan + crash, backup
  floor     rl_car_rollout_check of the same K x L roll-outs (one call, host arrays in and out)
  composed  tests/mcts_statement.py's search driven by the public calls (rollout(n_steps=1), calc_range_fan,
            eval_many, is_crashed, rollout_check): two synchronous round trips per iteration (K = 1 and 64 only)
Prints us per iteration and the ratios; --out writes the rows as JSON."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_common import B, FOV, THRESH, free_starts, lidar_poses, world, write_rows  # noqa: E402
from pyracecarsimulator_amd import racecar as RC  # noqa: E402
from pyracecarsimulator_amd.mcts import MCTSPlanner  # noqa: E402
import mcts_statement as S  # noqa: E402

SPEED, L, EVERY = 2.0, 200, 10
MAX_STEER, MAX_SPEED = RC.DEFAULT_CAR["max_steer_ang"], RC.DEFAULT_CAR["max_speed"]


def composed(cars, m, fg, states, n_it, edge, seeds):
    """The search on the host: the statement's recursion, each act and roll-out one synchronous batched call."""
    K = len(states)
    n_act = (L + EVERY - 1) // EVERY
    p0 = lidar_poses(states)
    r0 = np.empty(K * B, np.float32)
    m.calc_range_fan(p0, r0, FOV, B)
    ans0 = fg.eval_many(r0, B)
    trees = [S.Tree(states[k].copy(), p0[k], float(ans0[k]), 0.0, int(seeds[k])) for k in range(K)]
    last = {}

    def act_many(i, reqs):
        st = np.stack([node.state for _, node, _ in reqs])
        _, out, _ = cars.rollout(st, np.array([[SPEED, a] for _, _, a in reqs])[:, None, :], n_steps=1, action_every=1)
        poses = lidar_poses(out)
        ranges = np.empty(K * B, np.float32)
        m.calc_range_fan(poses, ranges, FOV, B)
        ranges = ranges.reshape(K, B)
        crashed = ((ranges.astype(np.float64) - edge) < THRESH).any(1)
        ans = fg.eval_many(ranges)
        last["states"] = out
        return [(out[k], poses[k], float(ans[k]), bool(crashed[k])) for k in range(K)]

    def rollout_many(i, reqs, acts):
        a = np.stack([S.rollout_actions(int(seeds[k]), i, n_act, MAX_STEER, MAX_SPEED) for k in range(K)])
        first, _, vel = cars.rollout_check(m, last["states"], a, FOV, B, edge, THRESH, n_steps=L, action_every=EVERY)
        return [(int(first[k]), vel[k]) for k, _ in reqs]

    S.run_lockstep(trees, n_it, act_many, rollout_many)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iterations", type=int, default=0, help="iterations per timed run (0: 200 for K <= 64, 20 above)")
    ap.add_argument("--sizes", default="1,64,1024,4096")
    ap.add_argument("--maps", default="cfg2,colombia")
    ap.add_argument("--composed-iterations", type=int, default=10)
    ap.add_argument("--composed-max-k", type=int, default=64)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    for mname in a.maps.split(","):
        g, _, dt, m, fg, cars, edge = world(mname)
        for K in (int(s) for s in a.sizes.split(",")):
            n = a.iterations or (200 if K <= 64 else 20)
            states = free_starts(g, dt, K)
            seeds = np.arange(K, dtype=np.uint64)
            pl = MCTSPlanner(cars, m, K, 2 * n + 2, FOV, B, edge, THRESH, source="fg", followgap=fg)
            pl.reset(states, 0.0, seeds)
            pl.run(2)                                            # warm-up (tables, code objects, buffers)
            pl.reset(states, 0.0, seeds)
            t0 = time.perf_counter()
            pl.run(n)
            t_plan = (time.perf_counter() - t0) / n
            _, _, nn = pl.best()
            # the floor: the same K x L roll-outs through rl_car_rollout_check (host arrays, one call)
            acts = np.random.default_rng(0).uniform(0, 1, (K, L // EVERY, 2)) * [MAX_SPEED, 0.0]
            cars.rollout_check(m, states, acts, FOV, B, edge, THRESH, n_steps=L, action_every=EVERY)
            reps = 20 if K <= 64 else 5
            t0 = time.perf_counter()
            for _ in range(reps):
                cars.rollout_check(m, states, acts, FOV, B, edge, THRESH, n_steps=L, action_every=EVERY)
            t_floor = (time.perf_counter() - t0) / reps
            row = dict(map=mname, K=K, L=L, num_rays=B, method="RMGPU", source="fg", iterations=n,
                       us_per_iteration=t_plan * 1e6, floor_us=t_floor * 1e6, plan_over_floor=t_plan / t_floor,
                       iterations_per_100ms=0.1 / t_plan, nodes=int(nn[0]))
            if K <= a.composed_max_k:
                ci = a.composed_iterations
                composed(cars, m, fg, states, 1, edge, seeds)
                t0 = time.perf_counter()
                composed(cars, m, fg, states, ci, edge, seeds)
                t_comp = (time.perf_counter() - t0) / ci
                row.update(composed_us_per_iteration=t_comp * 1e6, composed_over_plan=t_comp / t_plan,
                           composed_iterations=ci)
            rows.append(row)
            print("%-8s K=%5d n=%3d: %10.1f us/iteration (%7.0f it per 0.1 s) | floor %10.1f us, plan/floor %.3f | "
                  "composed %s" % (mname, K, n, row["us_per_iteration"], row["iterations_per_100ms"], row["floor_us"],
                                   row["plan_over_floor"],
                                   ("%10.1f us/iteration, composed/plan %.1f" % (row["composed_us_per_iteration"],
                                                                                 row["composed_over_plan"]))
                                   if "composed_us_per_iteration" in row else "skipped"), flush=True)
            pl.close()
    if a.out:
        write_rows(a.out, "tools/gpu_mcts_bench.py", rows)


if __name__ == "__main__":
    main()
