#!/usr/bin/env python3
"""League line-ups in the race environment (include/scanlib_league_env.h) against their floor and against the host's
only way to run them.

Colombia, RMGPU, 1081 beams, 1024 races x 4 cars, substeps 1, auto_reset, max_ticks 200, min_running 1, a pool of 512
line-ups (tools/gpu_seats_bench.py's env); seat 0 is the caller's (a constant action tensor), seats 1-3 are drawn from N
members (the fixture network with seeded perturbations), a different line-up in every race:
  league    RaceEnv(league=(pop, entries)).step on torch tensors, window (180, 720, 1) in the network's input form: per
            step the grouping of the live entries, the race scan, policy_mlp_league_kernel, the league phase B;
  floor     RaceEnv(seats=[None, X, X, X]) with ONE network X in the three scripted seats: the same scan, step and
            phase-B work with the dense rows launch of the network and no grouping;
  composed  the step composed on the host from the public calls in their NumPy forms, as docs/history/league.md's
            composed tick is: a plain RaceEnv on the raw full window, PolicyPopulation.predict_rows over all 4096
            observations with the entry table, the opponents' answers scattered into the action array, then the step
            (`--composed-steps` steps: every step moves 4096 x 1081 floats down and up again);
  device    the same composition with nothing leaving the device (torch tensors, predict_rows_device): the best a
            caller of the public calls can do without this header — the line-ups fixed for the run, no adoption at a
            spawn, no results;
  grouping  the three grouping launches with an empty network launch behind them: predict_rows_device over 4096 rows
            whose entries are all -1, `--launches` times between two synchronises.
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
from bench_common import B, FOV, THRESH, world, write_rows  # noqa: E402
from gpu_race_bench import race_states  # noqa: E402
from gpu_seats_bench import ENV_KW, POOL, SPEED, WINDOW, P, R, SeatedLeg  # noqa: E402
import policy_statement as PS  # noqa: E402  (tests/: bench_common put it on the path)

N_CARS = R * P
MEMBERS = (8, 64, 256)


class LeagueLeg:
    def __init__(self, w, pool, pop, entries):
        import torch
        from pyracecarsimulator_amd import RaceEnv
        self.torch = torch
        _, _, _, m, _, cars, edge = w
        self.env = RaceEnv(m, pool, R, B, FOV, edge, THRESH, car=cars, league=(pop, entries), seat_speed=SPEED, **WINDOW,
                           **ENV_KW)
        self.act = torch.zeros((R, P, 2), dtype=torch.float32, device="cuda")
        self.act[..., 0] = SPEED
        self.env.reset(seed=1, on_device=True)

    def run(self, steps):
        for _ in range(steps):
            self.env.step(self.act)
        self.torch.cuda.synchronize()


class HostLeg:
    """The NumPy forms: the raw window down, the population's row-indexed evaluation, the scatter, the step."""

    def __init__(self, w, pool, pop, entries):
        from pyracecarsimulator_amd import RaceEnv
        self.pop = pop
        _, _, _, m, _, cars, edge = w
        self.env = RaceEnv(m, pool, R, B, FOV, edge, THRESH, car=cars, **ENV_KW)
        self.act = np.zeros((R, P, 2), np.float32)
        self.act[..., 0] = SPEED
        self.member = np.maximum(entries.reshape(-1), -1).astype(np.int32)
        self.obs = self.env.reset(seed=1)

    def run(self, steps):
        for _ in range(steps):
            ans = self.pop.predict_rows(self.obs.reshape(N_CARS, B), self.member)
            self.act[:, 1:, 1] = ans.reshape(R, P)[:, 1:]
            self.obs, _, _ = self.env.step(self.act)


class ComposedLeg:
    """The raw window, the population's row-indexed evaluation over every observation, the scatter, the step: on the
    device."""

    def __init__(self, w, pool, pop, entries):
        import torch
        from pyracecarsimulator_amd import RaceEnv
        self.torch, self.pop = torch, pop
        _, _, _, m, _, cars, edge = w
        self.env = RaceEnv(m, pool, R, B, FOV, edge, THRESH, car=cars, **ENV_KW)
        self.act = torch.zeros((R, P, 2), dtype=torch.float32, device="cuda")
        self.act[..., 0] = SPEED
        self.ans = torch.zeros(N_CARS, dtype=torch.float32, device="cuda")
        self.member = torch.from_numpy(np.maximum(entries.reshape(-1), -1).astype(np.int32)).cuda()
        self.obs = self.env.reset(seed=1, on_device=True)

    def run(self, steps):
        torch = self.torch
        for _ in range(steps):
            st = torch.cuda.current_stream().cuda_stream
            self.pop.predict_rows_device(self.obs.data_ptr(), self.member.data_ptr(), N_CARS, B, self.ans.data_ptr(), stream=st)
            self.act[:, 1:, 1] = self.ans.view(R, P)[:, 1:]
            self.obs, _, _ = self.env.step(self.act)
        torch.cuda.synchronize()


class GroupingLeg:
    def __init__(self, pop):
        import torch
        self.torch, self.pop = torch, pop
        self.scans = torch.zeros((N_CARS, B), dtype=torch.float32, device="cuda")
        self.none = torch.full((N_CARS,), -1, dtype=torch.int32, device="cuda")
        self.out = torch.empty(N_CARS, dtype=torch.float32, device="cuda")

    def run(self, launches):
        st = self.torch.cuda.current_stream().cuda_stream
        for _ in range(launches):
            self.pop.predict_rows_device(self.scans.data_ptr(), self.none.data_ptr(), N_CARS, B, self.out.data_ptr(), stream=st)
        self.torch.cuda.synchronize()


def alternate(legs, reps):
    """legs: [(name, leg, n)]; returns {name: seconds per unit, one per rep}."""
    out = {name: [] for name, _, _ in legs}
    for _ in range(reps):                          # alternating: other people's work shares the host
        for name, leg, n in legs:
            t0 = time.perf_counter()
            leg.run(n)
            out[name].append((time.perf_counter() - t0) / n)
    return out


def stats(ts):
    return statistics.median(ts) * 1e6, min(ts) * 1e6, max(ts) * 1e6


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200, help="steps of a timed window of the env legs")
    ap.add_argument("--composed-steps", type=int, default=10, help="steps of a timed window of the host-composed leg")
    ap.add_argument("--launches", type=int, default=50, help="bare grouping calls between two synchronises")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--members", default="", help="N,N,... (default 8,64,256)")
    ap.add_argument("--out-dir", default="")
    a = ap.parse_args()
    from pyracecarsimulator_amd import Policy, PolicyPopulation, population
    members = tuple(int(v) for v in a.members.split(",")) if a.members else MEMBERS
    w = world("colombia")
    pool = race_states(w[0], w[2], POOL, P, 9)
    layers, relu = PS.load_fixture(os.path.join(ROOT, "tests", "golden", "policy_mlp720.npz"))
    dims = (layers[0][0].shape[0],) + tuple(W.shape[1] for W, _ in layers)
    base = population.pack(layers)
    rng = np.random.default_rng(5)
    thetas = base[None, :] + (0.01 * rng.standard_normal((max(members), base.size), dtype=np.float32)) * np.abs(base)[None, :]
    rows, lines = [], []
    for N in members:
        pop = PolicyPopulation(dims, N, relu=relu)
        pop.set(thetas[:N])
        pol = Policy.from_arrays(population.unpack(thetas[0], dims), relu)
        entries = np.random.default_rng(7).integers(0, N, (R, P)).astype(np.int32)
        entries[:, 0] = -2
        legs = [("league", LeagueLeg(w, pool, pop, entries), a.steps), ("floor", SeatedLeg(w, pool, pol), a.steps),
                ("device", ComposedLeg(w, pool, pop, entries), a.steps), ("composed", HostLeg(w, pool, pop, entries), a.composed_steps),
                ("grouping", GroupingLeg(pop), a.launches)]
        for name, leg, _ in legs:
            leg.run(3 if name == "composed" else 20)   # warm-up: tables, launch contexts, code objects, torch's kernels
        s = {k: stats(v) for k, v in alternate(legs, a.reps).items()}
        row = dict(members=N, races=R, group=P, num_rays=B, steps=a.steps, composed_steps=a.composed_steps, launches=a.launches,
                   reps=a.reps, league_over_floor=s["league"][0] / s["floor"][0],
                   league_minus_floor_us=s["league"][0] - s["floor"][0], device_over_league=s["device"][0] / s["league"][0],
                   composed_over_league=s["composed"][0] / s["league"][0])
        for k, (med, lo, hi) in s.items():
            row.update({k + "_us": med, k + "_us_min": lo, k + "_us_max": hi})
        rows.append(row)
        lines.append("N %3d members, %d races x %d, us/step: league %8.1f [%.1f .. %.1f] | floor (one network, seats) %8.1f "
                     "[%.1f .. %.1f] | device-composed %8.1f [%.1f .. %.1f] | host-composed %9.1f [%.1f .. %.1f] | grouping + "
                     "empty launch, us a call %6.1f [%.1f .. %.1f] | league - floor %.1f us, league/floor %.3f, device-composed/"
                     "league %.3f, host-composed/league %.1f"
                     % ((N, R, P) + s["league"] + s["floor"] + s["device"] + s["composed"] + s["grouping"]
                        + (row["league_minus_floor_us"], row["league_over_floor"], row["device_over_league"],
                           row["composed_over_league"])))
        print(lines[-1], flush=True)
        for _, leg, _ in legs[:4]:
            leg.env.close()
        pop.close()
        pol.close()
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "gpu_league_env_bench.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        write_rows(os.path.join(a.out_dir, "gpu_league_env_bench.json"), "tools/gpu_league_env_bench.py", rows)


if __name__ == "__main__":
    main()
