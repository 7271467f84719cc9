#!/usr/bin/env python3
"""League races (include/scanlib_league.h) against their floor and against the parent's only way to run them.

Colombia, RMGPU, 1081 beams, the fixture network (720 -> 64 -> 128 -> 128 -> 64 -> 1) with seeded perturbations as the
members, 1024 races x 4 cars, N members in round-robin line-ups (``league.round_robin(N, 4)``, cut or repeated to 1024
races), `--ticks` ticks a roll-out call:
  league    CarBatch.race_league: the grouping once, then per tick the race scan, policy_mlp_league_kernel, the tick;
  floor     CarBatch.race_seats over the same cars with ONE network in every seat: the same scan and tick work, the
            dense rows launch of the network;
  composed  the tick composed on the host from the public calls, the parent's way: calc_range_fan_cars, one
            Policy.predict_many per member on its cars, Car::isCrashed in numpy, rollout(n_steps=1)
            (`--composed-ticks` ticks: it is slow);
  grouping  the three grouping launches with an empty network launch behind them: predict_rows_device over 4096 rows
            whose entries are all -1 (no public call groups without launching the network; with nobody entered every
            network workgroup returns at once), `--launches` times between two synchronises; and `rows`, the same call
            with the round-robin entries, against `dense`, PolicyPopulation.predict_device over 4096 rows laid out by
            member.
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
from bench_common import B, FOV, THRESH, lidar_poses, world, write_rows  # noqa: E402
from gpu_race_bench import race_states  # noqa: E402
import policy_statement as PS  # noqa: E402  (tests/: bench_common put it on the path)

R, P, SPEED, CLIP = 1024, 4, 2.0, 0.4189
N_CARS = R * P
MEMBERS = (8, 64, 256)


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


def composed_league(cars, m, pols, entry, states, T, edge):
    """The league tick the way a caller of the public calls writes it (no FollowGap entries here)."""
    cur, steer = states.reshape(-1, 11).copy(), np.zeros(N_CARS)
    alive = np.ones(N_CARS, bool)
    members = [(k, np.nonzero(entry == k)[0]) for k in np.unique(entry)]
    for t in range(T):
        idx = np.nonzero(alive)[0]
        _, out, _ = cars.rollout(cur[idx], np.stack([np.full(idx.size, SPEED), steer[idx]], -1)[:, None, :], n_steps=1,
                                 action_every=1)
        cur[idx] = out
        ranges = m.calc_range_fan_cars(lidar_poses(cur), cur[:, :3].copy(), P, FOV, B).reshape(N_CARS, B)
        crashed = ((ranges.astype(np.float64) - edge) < THRESH).any(1)
        alive &= ~crashed
        for k, rows in members:
            steer[rows] = np.clip(pols[k].predict_many(np.ascontiguousarray(ranges[rows])).astype(np.float64), -CLIP, CLIP)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--composed-ticks", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20, help="bare launches between two synchronises")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--members", default="", help="N,N,... (default 8,64,256)")
    ap.add_argument("--out-dir", default="")
    a = ap.parse_args()
    import torch
    from pyracecarsimulator_amd import Policy, PolicyPopulation, league, population
    members = tuple(int(v) for v in a.members.split(",")) if a.members else MEMBERS
    g, _, dt, m, _, cars, edge = world("colombia")
    states = race_states(g, dt, R, P, 9)
    layers, relu = PS.load_fixture(os.path.join(ROOT, "tests", "golden", "policy_mlp720.npz"))
    dims = (layers[0][0].shape[0],) + tuple(W.shape[1] for W, _ in layers)
    base = population.pack(layers)
    rng = np.random.default_rng(5)
    thetas = base[None, :] + (0.01 * rng.standard_normal((max(members), base.size), dtype=np.float32)) * np.abs(base)[None, :]
    rows, lines = [], []
    for N in members:
        T = a.ticks
        pop = PolicyPopulation(dims, N, relu=relu)
        pop.set(thetas[:N])
        pols = [Policy.from_arrays(population.unpack(thetas[k], dims), relu) for k in range(N)]
        # round robins of 8 (280 races each: C(N, 4) line-ups of all N would be far more than 1024): the members in
        # N / 8 blocks, the first 1024 / (N / 8) races of each block's table (whole rotations; N = 8: repeated), the
        # races then shuffled so that no member's cars lie together
        rr, blocks = league.round_robin(8, P), N // 8
        entries = np.concatenate([np.resize(rr, (R // blocks, P)) + 8 * b for b in range(blocks)])
        entries = np.ascontiguousarray(entries[np.random.default_rng(7).permutation(R)], np.int32)
        flat = entries.reshape(-1)

        def league_leg():
            cars.race_league(m, pop, entries, states, T, SPEED, FOV, B, edge, THRESH, steer_clip=CLIP)

        def floor_leg():
            cars.race_seats(m, [pols[0]] * P, states, T, SPEED, FOV, B, edge, THRESH, steer_clip=CLIP)

        def composed_leg():
            composed_league(cars, m, pols, flat, states, a.composed_ticks, edge)

        d_scans = torch.from_numpy(rng.uniform(0.0, 18.0, (N_CARS, B)).astype(np.float32)).cuda()
        d_out = torch.empty(N_CARS, dtype=torch.float32, device="cuda")
        d_none = torch.full((N_CARS,), -1, dtype=torch.int32, device="cuda")
        d_entry = torch.from_numpy(flat).cuda()
        st = torch.cuda.current_stream().cuda_stream

        def bare(fn):
            def run():
                for _ in range(a.launches):
                    fn()
                torch.cuda.synchronize()
            return run

        grouping = bare(lambda: pop.predict_rows_device(d_scans.data_ptr(), d_none.data_ptr(), N_CARS, B, d_out.data_ptr(), stream=st))
        rows_leg = bare(lambda: pop.predict_rows_device(d_scans.data_ptr(), d_entry.data_ptr(), N_CARS, B, d_out.data_ptr(), stream=st))
        dense = bare(lambda: pop.predict_device(d_scans.data_ptr(), N_CARS // N, B, d_out.data_ptr(), stream=st))
        legs = [("league", league_leg, T), ("floor", floor_leg, T), ("composed", composed_leg, a.composed_ticks),
                ("grouping", grouping, a.launches), ("rows", rows_leg, a.launches), ("dense", dense, a.launches)]
        for _, fn, _ in legs:
            fn()                                   # warm-up: tables, launch contexts, code objects, staging
        s = {k: stats(v) for k, v in alternate(legs, a.reps).items()}
        row = dict(members=N, races=R, group=P, num_rays=B, ticks=T, composed_ticks=a.composed_ticks, launches=a.launches,
                   reps=a.reps, cars_per_member_min=int(np.bincount(flat, minlength=N).min()),
                   cars_per_member_max=int(np.bincount(flat, minlength=N).max()),
                   league_over_floor=s["league"][0] / s["floor"][0], composed_over_league=s["composed"][0] / s["league"][0],
                   rows_over_dense=s["rows"][0] / s["dense"][0])
        for k, (med, lo, hi) in s.items():
            row.update({k + "_us": med, k + "_us_min": lo, k + "_us_max": hi})
        rows.append(row)
        lines.append("N %3d members, %d races x %d: roll-out, us/tick: league %8.1f [%.1f .. %.1f] | floor %8.1f [%.1f .. %.1f] | "
                     "host-composed %10.1f [%.1f .. %.1f] | league/floor %.3f, composed/league %.1f || bare, us a call: "
                     "grouping + empty launch %6.1f [%.1f .. %.1f] | rows %8.1f [%.1f .. %.1f] | dense population %8.1f "
                     "[%.1f .. %.1f] | rows/dense %.3f"
                     % ((N, R, P) + s["league"] + s["floor"] + s["composed"] + (row["league_over_floor"],
                        row["composed_over_league"]) + s["grouping"] + s["rows"] + s["dense"] + (row["rows_over_dense"],)))
        print(lines[-1], flush=True)
        pop.close()
        for p in pols:
            p.close()
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "gpu_league_bench.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        write_rows(os.path.join(a.out_dir, "gpu_league_bench.json"), "tools/gpu_league_bench.py", rows)


if __name__ == "__main__":
    main()
