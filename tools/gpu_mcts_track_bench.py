#!/usr/bin/env python3
"""The track-guided MCTS planner: iterations per second of one planner with the velocity reward (no track), the waypoint
reward and the progress reward, in one process.

tools/gpu_mcts_bench.py's shape (colombia, RMGPU, 1081 beams, FG source, L = 200 roll-out steps), per tree count K
(1, 64, 1024), on three tracks:
  wp36        tests/golden/wp_u.csv, the reference's 36 waypoints, no window
  ring4096    4096 waypoints on a ring around the starts, no window: every roll-out step searches 4096 segments
  ring4096w   the same ring with window = 64 (129 candidate segments) and goal_span = 64
Per row: `repeats` timed runs of n iterations after a reset each, the median and the spread (max - min) of each mode,
and the modes' cost over the velocity reward of the same planner.  Before anything is timed, trees of every track and
mode at a small shape (K = 2, 4 iterations, L = 24, 181 beams) are held to the statement
(tests/mcts_track_statement.py); a difference ends the run.  --out writes the rows as JSON."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_common import B, FOV, ROOT, THRESH, free_starts, world, write_rows  # noqa: E402
from pyracecarsimulator_amd import Track  # noqa: E402
from pyracecarsimulator_amd.mcts import MCTSPlanner  # noqa: E402
import mcts_checks as MC  # noqa: E402
import mcts_track_checks as TC  # noqa: E402
import track_statement as TS  # noqa: E402

L, EVERY, LOOKAHEAD = 200, 10, 1.5
MODES = ("velocity", "waypoint", "progress")


def tracks(states):
    """{name: (points, window, goal_span)}; the ring runs through the region the starts lie in."""
    wp = Track.read_csv(os.path.join(ROOT, "tests", "golden", "wp_u.csv"))
    ring = TC.ring_around(states, 4096)
    return {"wp36": (wp, 0, 0), "ring4096": (ring, 0, 0), "ring4096w": (ring, 64, 64)}


def verify(cars, m, fg, states, cfg):
    """Trees of the small shape against the statement, every track and both track rewards."""
    K, I, Ls, Bs, base = 2, 4, 24, 181, 777
    st, ac, sd = states[:K], np.array([0.05, -0.1]), np.array([3, 5], np.uint64)
    for name, (xy, window, span) in cfg.items():
        T, trk = TS.build(xy, True), Track(xy, True)
        for reward in MODES[1:]:
            kw = dict(lookahead=LOOKAHEAD, window=window, goal_span=span, num_rays=Bs, rollout_steps=Ls, action_every=EVERY)
            pl, dev, _ = TC.device(cars, m, base, "random", None, st, ac, sd, I, trk, reward, **kw)
            try:
                _, want, rts, _ = TC.replay(cars, m, base, "random", None, st, ac, sd, I, dev, T, reward, **kw)
                for k in range(K):
                    MC.assert_tree(dev[k], want[k], (name, reward, k))
                TC.assert_roots(pl.read_track(), rts, (name, reward))
            finally:
                pl.close()
                m.set_noise(0.0, 0, 0)
    print("verified: trees of %d tracks x 2 rewards equal the statement" % len(cfg), flush=True)


def timed_runs(pl, states, seeds, n, repeats):
    """Seconds per iteration of `repeats` runs of n iterations, each after a reset (the first run warms up)."""
    pl.reset(states, 0.0, seeds)
    pl.run(2)
    out = []
    for _ in range(repeats):
        pl.reset(states, 0.0, seeds)
        t0 = time.perf_counter()
        pl.run(n)
        out.append((time.perf_counter() - t0) / n)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iterations", type=int, default=0, help="iterations per timed run (0: 100 for K <= 64, 20 above)")
    ap.add_argument("--sizes", default="1,64,1024")
    ap.add_argument("--tracks", default="wp36,ring4096,ring4096w")
    ap.add_argument("--rewards", default=",".join(MODES), help="the rewards to time (a kernel trace of one mode alone)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    g, _, dt, m, fg, cars, edge = world("colombia")
    sizes = [int(s) for s in a.sizes.split(",")]
    rewards = [r for r in MODES if r in a.rewards.split(",")]
    all_states = free_starts(g, dt, max(sizes + [2]))
    cfg = {k: v for k, v in tracks(all_states).items() if k in a.tracks.split(",")}
    verify(cars, m, fg, all_states, cfg)
    handles = {name: Track(xy, True) for name, (xy, _, _) in cfg.items()}
    rows = []
    for K in sizes:
        n = a.iterations or (100 if K <= 64 else 20)
        states, seeds = all_states[:K], np.arange(K, dtype=np.uint64)
        pl = MCTSPlanner(cars, m, K, n + 3, FOV, B, edge, THRESH, source="fg", followgap=fg, rollout_steps=L,
                         action_every=EVERY)
        for name, (xy, window, span) in cfg.items():
            row = dict(track=name, points=len(xy), window=window, goal_span=span, K=K, L=L, num_rays=B, iterations=n,
                       repeats=a.repeats)
            for reward in rewards:
                if reward == "velocity":
                    pl.detach_track()
                else:
                    pl.attach_track(handles[name], reward, lookahead=LOOKAHEAD, window=window, goal_span=span)
                t = timed_runs(pl, states, seeds, n, a.repeats)
                row[reward + "_us"] = statistics.median(t) * 1e6
                row[reward + "_spread_us"] = (max(t) - min(t)) * 1e6
                row[reward + "_iterations_per_s"] = 1.0 / statistics.median(t)
            if "velocity" in rewards:
                for reward in rewards[1:]:
                    row[reward + "_over_velocity"] = row[reward + "_us"] / row["velocity_us"]
            rows.append(row)
            print("%-10s K=%5d n=%3d: " % (name, K, n) + " | ".join(
                "%s %9.1f us/iteration (+-%.1f, %7.1f it/s)" % (r, row[r + "_us"], row[r + "_spread_us"],
                                                               row[r + "_iterations_per_s"]) for r in rewards) +
                  "".join(" | %s/velocity %.3f" % (r, row[r + "_over_velocity"]) for r in rewards[1:]
                          if r + "_over_velocity" in row), flush=True)
        pl.close()
    if a.out:
        write_rows(a.out, "tools/gpu_mcts_track_bench.py", rows)


if __name__ == "__main__":
    main()
