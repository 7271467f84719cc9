#!/usr/bin/env python3
"""The track steering the MCTS planner (source "track", rollout "pursuit"): what it costs per iteration and what it buys
in a closed loop, in one process.

Cost: tools/gpu_mcts_bench.py's shape (colombia, RMGPU, 1081 beams, L = 200 roll-out steps, action_every 10), K = 1 and
64 trees, on two tracks (wp36: tests/golden/wp_u.csv, no window; ring4096w: 4096 waypoints around the starts, window =
goal_span = 64), the velocity reward with the track attached, four planners:
  a  source fg,    random roll-outs   (the planner as it was; the track attached changes no launch of it but the roots')
  b  source track, random roll-outs
  c  source fg,    pursuit roll-outs
  d  source track, pursuit roll-outs
Per row `repeats` timed runs of n iterations after a reset each: the median, the spread (max - min) and the difference
to row a.  --only a times row a alone (for alternating processes of two checkouts).

Benefit: the room of the tests (13 m, the waypoint file inside it), K = 64 cars started on the track, `drive` with 50
iterations per decision, the progress reward, the same seeds for the four planners: cars crashed, the track progress of
every car (s of read_track after the drive, the state the last decision was planned from, against s of the start, the
short way round: the drive is far shorter than half a lap), and the share of roll-outs of the last decision's trees
that crashed (crash >= 0 among the non-terminal children).

Before anything is timed, trees of both new modes at a small shape are held to the statement
(tests/mcts_pursuit_checks.py); a difference ends the run.  --out writes the rows as JSON."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_common import B, FOV, ROOT, THRESH, free_starts, world, write_rows  # noqa: E402
import support  # noqa: E402
from pyracecarsimulator_amd import Track, maps, range_libc, racecar as RC  # noqa: E402
from pyracecarsimulator_amd.mcts import MCTSPlanner  # noqa: E402
import mcts_pursuit_checks as PC  # noqa: E402
import mcts_track_checks as TC  # noqa: E402
import track_statement as TS  # noqa: E402

L, EVERY, LOOKAHEAD, DEV = 200, 10, 1.5, 0.1
ROWS = {"a": ("fg", "random"), "b": ("track", "random"), "c": ("fg", "pursuit"), "d": ("track", "pursuit")}


def tracks(states):
    wp = Track.read_csv(os.path.join(ROOT, "tests", "golden", "wp_u.csv"))
    return {"wp36": (wp, 0, 0), "ring4096w": (TC.ring_around(states, 4096), 64, 64)}


def verify(cars, m, fg, states):
    """Trees of a small shape (K = 2, 4 iterations, L = 24, 181 beams) against the statement, rows b, c and d."""
    K, I, base = 2, 4, 777
    st, ac, sd = states[:K], np.array([0.05, -0.1]), np.array([3, 5], np.uint64)
    xy = TC.ring_around(states[:K], 70)
    T, trk = TS.build(xy, True), Track(xy, True)
    for row in "bcd":
        source, rollout = ROWS[row]
        pl = PC.run_both(cars, m, base, source, fg if source == "fg" else None, st, ac, sd, I, trk, T, "progress", row,
                         rollout=rollout, rollout_dev=DEV, lookahead=LOOKAHEAD, window=3, goal_span=3, num_rays=181,
                         rollout_steps=24, action_every=EVERY)[0]
        pl.close()
        m.set_noise(0.0, 0, 0)
    print("verified: trees of rows b, c and d equal the statement", flush=True)


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


def cost(a, rows_out):
    g, _, dt, m, fg, cars, edge = world("colombia")
    sizes = [int(s) for s in a.sizes.split(",")]
    all_states = free_starts(g, dt, max(sizes + [2]))
    if a.only != "a":
        verify(cars, m, fg, all_states)
    cfg = tracks(all_states)
    for K in sizes:
        n = a.iterations
        states, seeds = all_states[:K], np.arange(K, dtype=np.uint64)
        for name, (xy, window, span) in cfg.items():
            trk = Track(xy, True)
            row = dict(kind="cost", track=name, points=len(xy), window=window, goal_span=span, K=K, L=L, num_rays=B,
                       iterations=n, repeats=a.repeats)
            for r in (a.only or "abcd"):
                source, rollout = ROWS[r]
                kw = dict(rollout=rollout, rollout_dev=DEV) if r != "a" else {}
                pl = MCTSPlanner(cars, m, K, n + 3, FOV, B, edge, THRESH, source=source, followgap=fg if source == "fg" else None,
                                 rollout_steps=L, action_every=EVERY, **kw)
                try:
                    pl.attach_track(trk, "velocity", lookahead=LOOKAHEAD, window=window, goal_span=span)
                    t = timed_runs(pl, states, seeds, n, a.repeats)
                finally:
                    pl.close()
                row[r + "_us"] = statistics.median(t) * 1e6
                row[r + "_spread_us"] = (max(t) - min(t)) * 1e6
            rows_out.append(row)
            print("%-10s K=%3d n=%3d: " % (name, K, n) + " | ".join(
                "%s %8.1f us/iteration (+-%.1f%s)" % (r, row[r + "_us"], row[r + "_spread_us"],
                                                      ", %+.1f to a" % (row[r + "_us"] - row["a_us"]) if r != "a" and "a_us" in row else "")
                for r in (a.only or "abcd")), flush=True)


def benefit(a, rows_out):
    g = maps.make_room(260, resolution=0.05, origin=(-4.0, -2.0, 0.0))
    m = range_libc.PyRayMarchingGPU(range_libc.PyOMap(g), 300)
    cars, fg, edge = RC.CarBatch(), support.followgap(), support.edge(B)
    xy = Track.read_csv(os.path.join(ROOT, "tests", "golden", "wp_u.csv"))
    T, trk = TS.build(xy, True), Track(xy, True)
    K, I, D, S = 64, 50, a.decisions, a.steps
    states, recent, seeds = PC.roots_on(T, K, 17)
    s0 = np.array([PC.PS.root(T, s[0], s[1])["s"] for s in states])
    for r in "abcd":
        source, rollout = ROWS[r]
        pl = MCTSPlanner(cars, m, K, I + 1, FOV, B, edge, THRESH, source=source, followgap=fg if source == "fg" else None,
                         rollout_steps=L, action_every=EVERY, rollout=rollout, rollout_dev=DEV)
        try:
            pl.attach_track(trk, "progress", lookahead=LOOKAHEAD, window=4, goal_span=4)
            t0 = time.perf_counter()
            first, out, _, _, _ = pl.drive(states, 0.0, seeds, D, I, steps_per_decision=S, steer_clip=0.4189)
            wall = time.perf_counter() - t0
            s1 = pl.read_track()["s"]
            trees = [pl.read_tree(k) for k in range(K)]
        finally:
            pl.close()
        gain = np.array([TS.wrap(T, s1[k] - s0[k])[0] for k in range(K)])
        ro = np.concatenate([t["crash"][1:][t["terminal"][1:] == 0] for t in trees])
        row = dict(kind="benefit", row=r, source=source, rollout=rollout, K=K, iterations=I, decisions=D, steps=S,
                   crashed=int((first >= 0).sum()), progress_mean_m=float(gain.mean()), progress_median_m=float(np.median(gain)),
                   progress_min_m=float(gain.min()), rollouts=int(ro.size), rollouts_crashed=int((ro >= 0).sum()),
                   drive_s=wall)
        rows_out.append(row)
        print("%s source %-6s roll-outs %-7s: crashed %2d of %d, progress mean %.2f median %.2f min %.2f m (last planned "
              "state), roll-outs crashed %d of %d, drive %.1f s" % (r, source, rollout, row["crashed"], K, row["progress_mean_m"],
                                                                   row["progress_median_m"], row["progress_min_m"],
                                                                   row["rollouts_crashed"], row["rollouts"], wall), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iterations", type=int, default=100, help="iterations per timed run")
    ap.add_argument("--sizes", default="1,64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default="", choices=["", "a"], help="time row a alone and skip the benefit part")
    ap.add_argument("--decisions", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10, help="car steps per decision")
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    if not a.skip_cost:
        cost(a, rows)
    if not a.only:
        benefit(a, rows)
    if a.out:
        write_rows(a.out, "tools/gpu_mcts_pursuit_bench.py", rows)


if __name__ == "__main__":
    main()
