#!/usr/bin/env python3
"""What track progress costs the closed-loop roll-outs per tick (include/scanlib_track_drive.h).

Colombia, RMGPU, 1081 beams, the fixture network (720 -> 64 -> 128 -> 128 -> 64 -> 1) with seeded perturbations as the
members, `--ticks` ticks a roll-out call:
  population   CarBatch.drive_population, 256 members x 8 cars
  league       CarBatch.race_league, 280 races x 4 cars: league.round_robin(8, 4)'s line-ups
each of them
  plain        with no track attached: the launches of the parent commit
  wp36         tests/golden/wp_u.csv attached, all 36 segments searched at every tick
  ring4096/64  a ring of 4096 points, window 64: 129 candidates per car and tick
  ring4096/0   the same ring, every segment searched at every tick
A tracked call adds one drive_track_kernel launch per tick, one on the starts, the rank kernel and the score kernel; the
reads (track_state, track_scores) are not in the timing.  The legs are warmed up, then timed `--reps` times in alternation
(a host clock around a synchronous call); medians and [min .. max] per tick are printed, and with --out-dir written as
text and JSON.  Where the tracks lie on the map does not change the work."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_common import B, FOV, THRESH, free_starts, world, write_rows  # noqa: E402
from gpu_race_bench import race_states  # noqa: E402
import policy_statement as PS  # noqa: E402  (tests/: bench_common put it on the path)

N_POP, E_POP = 256, 8
R_LEAGUE, P_LEAGUE = 280, 4
SPEED, CLIP = 2.0, 0.4189
TRACKS = (("plain", None, 0), ("wp36", 36, 0), ("ring4096/64", 4096, 64), ("ring4096/0", 4096, 0))


def track_xy(W):
    from pyracecarsimulator_amd import Track
    if W == 36:
        return Track.read_csv(os.path.join(ROOT, "tests", "golden", "wp_u.csv"))
    a = np.arange(W) * (2 * math.pi / W)
    return np.stack([20.0 + 15.0 * np.cos(a), 20.0 + 12.0 * np.sin(a)], -1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--legs", default="", help="plain,wp36,... (default: all four; plain alone runs on a build without "
                    "the feature, for an A/B of the untracked roll-out with SCANLIB_SO)")
    ap.add_argument("--out-dir", default="")
    a = ap.parse_args()
    from pyracecarsimulator_amd import PolicyPopulation, Track, league, population
    g, _, dt, m, _, cars, edge = world("colombia")
    layers, relu = PS.load_fixture(os.path.join(ROOT, "tests", "golden", "policy_mlp720.npz"))
    dims = (layers[0][0].shape[0],) + tuple(W.shape[1] for W, _ in layers)
    base = population.pack(layers)
    rng = np.random.default_rng(5)
    thetas = base[None, :] + (0.01 * rng.standard_normal((N_POP, base.size), dtype=np.float32)) * np.abs(base)[None, :]
    pop = PolicyPopulation(dims, N_POP, relu=relu)
    pop.set(thetas)
    lone = free_starts(g, dt, N_POP * E_POP)
    races = race_states(g, dt, R_LEAGUE, P_LEAGUE, 9)
    entries = np.ascontiguousarray(league.round_robin(8, P_LEAGUE), np.int32)
    assert entries.shape == (R_LEAGUE, P_LEAGUE)
    names = [n for n in a.legs.split(",") if n] or [name for name, _, _ in TRACKS]
    tracks = {name: (Track(track_xy(W)) if W else None, window) for name, W, window in TRACKS if name in names}
    T = a.ticks

    def leg(kind, name):
        trk, window = tracks[name]

        def run():
            if trk is not None:
                cars.attach_track(trk, window)
            try:
                if kind == "population":
                    cars.drive_population(m, pop, lone, T, SPEED, FOV, B, edge, THRESH, E_POP, steer_clip=CLIP)
                else:
                    cars.race_league(m, pop, entries, races, T, SPEED, FOV, B, edge, THRESH, steer_clip=CLIP)
            finally:
                if trk is not None:
                    cars.detach_track()
        return run

    rows, lines = [], []
    for kind, n_cars in (("population", N_POP * E_POP), ("league", R_LEAGUE * P_LEAGUE)):
        legs = {name: leg(kind, name) for name in tracks}
        for fn in legs.values():
            fn()                                   # warm-up: tables, launch contexts, code objects, staging
        t = {name: [] for name in legs}
        for _ in range(a.reps):                    # alternating: other people's work shares the machine
            for name, fn in legs.items():
                t0 = time.perf_counter()
                fn()
                t[name].append((time.perf_counter() - t0) / T * 1e6)
        med = {k: statistics.median(v) for k, v in t.items()}
        row = dict(kind=kind, cars=n_cars, num_rays=B, ticks=T, reps=a.reps)
        for k in legs:
            row.update({k + "_us_per_tick": med[k], k + "_us_min": min(t[k]), k + "_us_max": max(t[k]),
                        k + "_minus_plain_us": med[k] - med.get("plain", math.nan)})
        rows.append(row)
        lines.append("%-10s %4d cars, us/tick: " % (kind, n_cars) + " | ".join(
            "%s %7.1f [%.1f .. %.1f] (%+.1f)" % (k, med[k], min(t[k]), max(t[k]), med[k] - med.get("plain", math.nan)) for k in legs))
        print(lines[-1], flush=True)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "gpu_track_drive_bench.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        write_rows(os.path.join(a.out_dir, "gpu_track_drive_bench.json"), "tools/gpu_track_drive_bench.py", rows)


if __name__ == "__main__":
    main()
