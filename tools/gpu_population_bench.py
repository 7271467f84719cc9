#!/usr/bin/env python3
"""Policy populations (include/scanlib_population.h) against the parent's only way to run N networks.

Colombia, RMGPU, 1081 beams, the fixture network (720 -> 64 -> 128 -> 128 -> 64 -> 1) with seeded perturbations as the
members, N members x E cars, `--ticks` ticks a roll-out call:
  population  CarBatch.drive_population: per tick one scan, one policy_mlp_pop_kernel launch, one tick kernel;
  parent      N Policy handles and N CarBatch.drive_policy calls of E cars each (the parent's way);
  floor       one CarBatch.drive_policy call of N E cars with a single network: the same scan and tick work;
  bare        the network launch alone on N E scans resident on the device: PolicyPopulation.predict_device once
              against N Policy.predict_device launches of E scans, `--launches` times between two synchronises.
The legs are warmed up, then timed `--reps` times in alternation (a host clock around work that ends in a device
synchronise); medians and [min .. max] are printed, and with --out-dir written as text and JSON."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_common import B, FOV, THRESH, free_starts, world, write_rows  # noqa: E402
import policy_statement as PS  # noqa: E402  (tests/: bench_common put it on the path)

SHAPES = ((8, 8), (64, 8), (256, 8), (256, 4), (1024, 1))
SPEED, CLIP = 2.0, 0.4189


def alternate(legs, reps):
    """legs: [(name, fn, units)]; returns {name: seconds per unit, one per rep}."""
    out = {name: [] for name, _, _ in legs}
    for _ in range(reps):                          # alternating: other people's work shares the host
        for name, fn, n in legs:
            t0 = time.perf_counter()
            fn()
            out[name].append((time.perf_counter() - t0) / n)
    return out


def stats(ts):
    return statistics.median(ts) * 1e6, min(ts) * 1e6, max(ts) * 1e6


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--launches", type=int, default=20, help="bare network launches between two synchronises")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="", help="N,E;N,E;... (default: the five of docs/history/population.md)")
    ap.add_argument("--out-dir", default="")
    a = ap.parse_args()
    import torch
    from pyracecarsimulator_amd import Policy, PolicyPopulation, population
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shapes.split(";")] if a.shapes else SHAPES
    g, _, dt, m, _, cars, edge = world("colombia")
    layers, relu = PS.load_fixture(os.path.join(ROOT, "tests", "golden", "policy_mlp720.npz"))
    dims = (layers[0][0].shape[0],) + tuple(W.shape[1] for W, _ in layers)
    base = population.pack(layers)
    n_max = max(n for n, _ in shapes)
    rng = np.random.default_rng(5)
    thetas = base[None, :] + (0.01 * rng.standard_normal((n_max, base.size), dtype=np.float32)) * np.abs(base)[None, :]
    pols = [Policy.from_arrays(population.unpack(thetas[k], dims), relu) for k in range(n_max)]
    rows, lines = [], []
    for N, E in shapes:
        R, T = N * E, a.ticks
        pop = PolicyPopulation(dims, N, relu=relu)
        pop.set(thetas[:N])
        states = free_starts(g, dt, R)

        def pop_leg():
            cars.drive_population(m, pop, states, T, SPEED, FOV, B, edge, THRESH, E, steer_clip=CLIP)

        def parent_leg():
            for k in range(N):
                cars.drive_policy(m, pols[k], states[k * E:(k + 1) * E], T, SPEED, FOV, B, edge, THRESH, steer_clip=CLIP)

        def floor_leg():
            cars.drive_policy(m, pols[0], states, T, SPEED, FOV, B, edge, THRESH, steer_clip=CLIP)

        d_scans = torch.from_numpy(rng.uniform(0.0, 18.0, (R, B)).astype(np.float32)).cuda()
        d_out = torch.empty(R, dtype=torch.float32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def bare_pop():
            for _ in range(a.launches):
                pop.predict_device(d_scans.data_ptr(), E, B, d_out.data_ptr(), stream=st)
            torch.cuda.synchronize()

        def bare_parent():
            for _ in range(a.launches):
                for k in range(N):
                    pols[k].predict_device(d_scans.data_ptr() + 4 * k * E * B, E, B, d_out.data_ptr() + 4 * k * E, st)
            torch.cuda.synchronize()

        legs = [("population", pop_leg, T), ("parent", parent_leg, T), ("floor", floor_leg, T),
                ("bare_population", bare_pop, a.launches), ("bare_parent", bare_parent, a.launches)]
        for _, fn, _ in legs:
            fn()                                   # warm-up: tables, launch contexts, code objects, staging
        t = alternate(legs, a.reps)
        s = {k: stats(v) for k, v in t.items()}
        row = dict(members=N, cars_per_member=E, num_rays=B, ticks=T, launches=a.launches, reps=a.reps,
                   parent_over_population=s["parent"][0] / s["population"][0],
                   population_over_floor=s["population"][0] / s["floor"][0],
                   bare_parent_over_population=s["bare_parent"][0] / s["bare_population"][0])
        for k, (med, lo, hi) in s.items():
            row.update({k + "_us": med, k + "_us_min": lo, k + "_us_max": hi})
        rows.append(row)
        lines.append("N %4d x E %d: roll-out, us/tick: population %9.1f [%.1f .. %.1f] | parent's way %10.1f [%.1f .. %.1f] | "
                     "floor %8.1f [%.1f .. %.1f] | parent/population %.2f, population/floor %.3f || bare launch, us: "
                     "population %8.1f [%.1f .. %.1f] | N launches %9.1f [%.1f .. %.1f] | ratio %.2f"
                     % ((N, E) + s["population"] + s["parent"] + s["floor"] + (row["parent_over_population"],
                        row["population_over_floor"]) + s["bare_population"] + s["bare_parent"]
                        + (row["bare_parent_over_population"],)))
        print(lines[-1], flush=True)
        pop.close()
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "gpu_population_bench.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        write_rows(os.path.join(a.out_dir, "gpu_population_bench.json"), "tools/gpu_population_bench.py", rows)


if __name__ == "__main__":
    main()
