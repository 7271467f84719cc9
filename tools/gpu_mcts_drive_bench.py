#!/usr/bin/env python3
"""The closed MCTS loop: time per decision of rl_mcts_drive against the same decisions composed on the host from the
public calls, in one process.

colombia, RMGPU, 1081 beams, FG source, L = 200 roll-out steps, one car step per decision; per car count K
(1, 64, 4096) and iterations per decision I (4, 50), D decisions:
  drive     MCTSPlanner.drive(D decisions): everything enqueued at once, one host synchronisation at the end
  composed  per decision reset, run(I), best and CarBatch.rollout of the step: four synchronous calls with their
            uploads and downloads (the crash test of the car, which drive makes, is left out of this side)
  run       MCTSPlanner.run(I) alone after one reset: what a decision's search costs without its reset and step
Prints ms per decision and the ratios; --out writes the rows as JSON."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_common import B, FOV, THRESH, free_starts, world, write_rows  # noqa: E402
from pyracecarsimulator_amd import mcts as M  # noqa: E402

SPEED, L, EVERY, CLIP = 2.0, 200, 10, 0.4189


def composed(cars, m, pl, states, recent, seeds, D, I, base):
    """The decisions on the host: the public calls as they were before rl_mcts_drive."""
    K = len(states)
    states, recent = states.copy(), recent.copy()
    stride = M.drive_stride(K, B, I, L)
    for d in range(D):
        m.set_noise(0.0, 0, base + d * stride)
        pl.reset(states, recent, M.drive_seeds(seeds, d))
        pl.run(I)
        a, _, _ = pl.best()
        acts = np.stack([np.full(K, SPEED), a], axis=1)[:, None, :]
        _, states, _ = cars.rollout(states, acts, n_steps=1, action_every=1)
        recent = M.drive_recent(a, CLIP)
    m.set_noise(0.0, 0, base)
    return states


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="1,64,4096")
    ap.add_argument("--iterations", default="4,50")
    ap.add_argument("--decisions", type=int, default=0, help="decisions per timed run (0: 20 for K <= 64, 3 above)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    g, _, dt, m, fg, cars, edge = world("colombia")
    rows = []
    for K in (int(s) for s in a.sizes.split(",")):
        states = free_starts(g, dt, K)
        recent, seeds = np.zeros(K), np.arange(K, dtype=np.uint64)
        for I in (int(s) for s in a.iterations.split(",")):
            D = a.decisions or (20 if K <= 64 else 3)
            pl = M.MCTSPlanner(cars, m, K, I + 1, FOV, B, edge, THRESH, source="fg", followgap=fg)
            pl.drive(states, recent, seeds, 1, min(I, 2))                     # warm-up (tables, code objects, buffers)
            composed(cars, m, pl, states, recent, seeds, 1, min(I, 2), 0)
            t0 = time.perf_counter()
            first, out, _, _, _ = pl.drive(states, recent, seeds, D, I, steer_clip=CLIP)
            t_drive = (time.perf_counter() - t0) / D
            t0 = time.perf_counter()
            out_c = composed(cars, m, pl, states, recent, seeds, D, I, 0)
            t_comp = (time.perf_counter() - t0) / D
            same = bool((out[first < 0] == out_c[first < 0]).all())          # (noise off: the same decisions)
            pl.reset(states, recent, seeds)
            t0 = time.perf_counter()
            pl.run(I)
            t_run = time.perf_counter() - t0
            pl.close()
            row = dict(map="colombia", K=K, I=I, L=L, num_rays=B, method="RMGPU", source="fg", decisions=D,
                       drive_ms_per_decision=t_drive * 1e3, composed_ms_per_decision=t_comp * 1e3,
                       run_ms=t_run * 1e3, composed_over_drive=t_comp / t_drive, drive_over_run=t_drive / t_run,
                       crashed=int((first >= 0).sum()), same_states=same)
            rows.append(row)
            print("K=%5d I=%3d D=%3d: drive %10.3f ms/decision | composed %10.3f ms/decision, composed/drive %.3f | "
                  "run(I) alone %10.3f ms, drive/run %.3f | crashed %d, same states %s"
                  % (K, I, D, row["drive_ms_per_decision"], row["composed_ms_per_decision"], row["composed_over_drive"],
                     row["run_ms"], row["drive_over_run"], row["crashed"], same), flush=True)
    if a.out:
        write_rows(a.out, "tools/gpu_mcts_drive_bench.py", rows)


if __name__ == "__main__":
    main()
