#!/usr/bin/env python3
"""The driving environment (rl_env_*, DriveEnv) against the same tick composed from the public calls.

Colombia, RMGPU, 1081 beams, substeps 1, N envs (256 and 4096), auto_reset, max_ticks 200, a pool of 512 starts:
  env       DriveEnv.step on torch tensors (the device form, torch.cuda.current_stream()) under a trivial torch
            controller: constant speed, steer = clamp(gain * (mean of the left third - mean of the right third)).
            Nothing is copied to the host and nothing waits for the GPU between steps; one synchronise ends the window.
  composed  the tick the way a caller of the parent's public calls writes it, the same controller in NumPy:
            CarBatch.rollout(n_steps=1) of the live cars -> lidar poses in NumPy -> calc_range_fan to the host ->
            Car::isCrashed on the host (NumPy, vectorised, as gpu_drive_bench.py) -> re-spawn of the finished cars.
Both legs are warmed up, then timed `--reps` times in alternation over `--steps` steps each (a host clock around work
that ends in a device synchronise); the medians and the spread are printed, and steps/s, env-steps/s and the ratio
written with --out-dir.

--count-launches: kernel launches per step of each leg, from `rocprofv3 --kernel-trace --stats` runs of their own (a
fresh child process per run, each under its own time limit, before this process touches the GPU): the dispatch counts
of a K2-step and a K1-step run of one leg, differenced, so that set-up launches cancel."""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_common import B, FOV, THRESH, free_starts, lidar_poses, world, write_rows  # noqa: E402

SPEED, GAIN, CLIP = 2.0, 0.1, 0.4189
MAX_TICKS, POOL = 200, 512


def setup(N):
    from pyracecarsimulator_amd import DriveEnv
    g, _, dt, m, _, cars, edge = world("colombia")
    starts = free_starts(g, dt, POOL)
    env = DriveEnv(m, starts, N, B, FOV, edge, THRESH, max_ticks=MAX_TICKS, auto_reset=True, car=cars)
    return env, m, cars, edge, starts


class EnvLeg:
    def __init__(self, N):
        import torch
        self.torch = torch
        self.env, *_ = setup(N)
        self.act = torch.empty((N, 2), dtype=torch.float32, device="cuda")
        self.act[:, 0] = SPEED
        self.obs = self.env.reset(seed=1, on_device=True)

    def run(self, steps):
        torch, third = self.torch, B // 3
        for _ in range(steps):
            self.act[:, 1] = torch.clamp(GAIN * (self.obs[:, B - third:].mean(1) - self.obs[:, :third].mean(1)), -CLIP, CLIP)
            self.obs, _, _ = self.env.step(self.act)
        torch.cuda.synchronize()


class ComposedLeg:
    def __init__(self, N):
        _, self.m, self.cars, self.edge, self.starts = setup(N)
        self.N = N
        self.rng = np.random.default_rng(1)
        self.cur = self.starts[self.rng.integers(0, POOL, N)].copy()
        self.tick = np.zeros(N, np.int32)
        self.done = np.zeros(N, bool)
        self.ranges = np.empty(N * B, np.float32)
        self.scan()

    def scan(self):
        self.m.calc_range_fan(lidar_poses(self.cur), self.ranges, FOV, B)
        return self.ranges.reshape(self.N, B)

    def run(self, steps):
        N, third = self.N, B // 3
        obs = self.ranges.reshape(N, B)
        for _ in range(steps):
            steer = np.clip(GAIN * (obs[:, B - third:].mean(1) - obs[:, :third].mean(1)), -CLIP, CLIP)
            fresh = np.nonzero(self.done)[0]
            live = np.nonzero(~self.done)[0]
            if fresh.size:
                self.cur[fresh] = self.starts[self.rng.integers(0, POOL, fresh.size)]
                self.tick[fresh] = 0
                self.done[fresh] = False
            if live.size:
                acts = np.stack([np.full(live.size, SPEED), steer[live].astype(np.float64)], -1)[:, None, :]
                _, out, _ = self.cars.rollout(self.cur[live], acts, n_steps=1, action_every=1)
                self.cur[live] = out
                self.tick[live] += 1
            obs = self.scan()
            crashed = ((obs.astype(np.float64) - self.edge) < THRESH).any(1)
            self.done = crashed | (self.tick == MAX_TICKS)


def child(leg, N, steps):
    """One leg alone for a traced run: set-up, then exactly `steps` steps."""
    (EnvLeg if leg == "env" else ComposedLeg)(N).run(steps)


def dispatches(leg, N, steps, limit):
    """Kernel dispatches of a fresh child that runs `steps` steps of `leg` under rocprofv3 (its own process and limit)."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d,
               "--", sys.executable, os.path.abspath(__file__), "--child", leg, "--n", str(N), "--steps", str(steps)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, env=dict(os.environ, TMPDIR="/tmp"))
        total = 0
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                total += sum(int(row["Calls"]) for row in csv.DictReader(f))
        if total == 0:
            raise RuntimeError("no kernel statistics came back from the traced run of the %s leg" % leg)
        return total


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="256,4096")
    ap.add_argument("--steps", type=int, default=1000, help="steps of a timed window of the env leg")
    ap.add_argument("--composed-steps", type=int, default=20, help="steps of a timed window of the composed leg")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--count-launches", action="store_true")
    ap.add_argument("--limit", type=int, default=240, help="time limit of a traced child, seconds")
    ap.add_argument("--out-dir", default="")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--n", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.n, a.steps)
    sizes = [int(s) for s in a.sizes.split(",")]
    launches = {}
    if a.count_launches:                       # (first: this process has not opened the GPU yet)
        k1, k2 = 10, 30
        for N in sizes:
            for leg in ("env", "composed"):
                c1, c2 = dispatches(leg, N, k1, a.limit), dispatches(leg, N, k2, a.limit)
                launches[(N, leg)] = (c2 - c1) / (k2 - k1)
                print("N=%5d %-8s: %d / %d dispatches at %d / %d steps -> %.2f kernel launches per step"
                      % (N, leg, c1, c2, k1, k2, launches[(N, leg)]), flush=True)
    rows, lines = [], []
    for N in sizes:
        env, comp = EnvLeg(N), ComposedLeg(N)
        env.run(20)                            # warm-up: tables, launch contexts, code objects, torch's kernels
        comp.run(3)
        t_env, t_comp = [], []
        for _ in range(a.reps):                # alternating: other people's work shares the host
            t0 = time.perf_counter()
            env.run(a.steps)
            t_env.append((time.perf_counter() - t0) / a.steps)
            t0 = time.perf_counter()
            comp.run(a.composed_steps)
            t_comp.append((time.perf_counter() - t0) / a.composed_steps)
        e, c = statistics.median(t_env), statistics.median(t_comp)
        row = dict(map="colombia", method="RMGPU", n_envs=N, num_rays=B, substeps=1, steps=a.steps,
                   composed_steps=a.composed_steps, reps=a.reps, env_us_per_step=e * 1e6, env_steps_per_s=1 / e,
                   env_env_steps_per_s=N / e, env_us_min=min(t_env) * 1e6, env_us_max=max(t_env) * 1e6,
                   composed_us_per_step=c * 1e6, composed_steps_per_s=1 / c, composed_us_min=min(t_comp) * 1e6,
                   composed_us_max=max(t_comp) * 1e6, composed_over_env=c / e,
                   env_launches_per_step=launches.get((N, "env")), composed_launches_per_step=launches.get((N, "composed")))
        rows.append(row)
        line = ("colombia N=%5d: env %9.1f us/step [%.1f .. %.1f] (%8.0f steps/s, %.3g env-steps/s) | composed %10.1f "
                "us/step [%.1f .. %.1f] (%7.1f steps/s) | composed/env %.1f | launches per step: env %s, composed %s" % (
                    N, row["env_us_per_step"], row["env_us_min"], row["env_us_max"], row["env_steps_per_s"],
                    row["env_env_steps_per_s"], row["composed_us_per_step"], row["composed_us_min"],
                    row["composed_us_max"], row["composed_steps_per_s"], row["composed_over_env"],
                    "%.2f" % launches[(N, "env")] if (N, "env") in launches else "not counted",
                    "%.2f" % launches[(N, "composed")] if (N, "composed") in launches else "not counted"))
        lines.append(line)
        print(line, flush=True)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "gpu_env_bench.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        write_rows(os.path.join(a.out_dir, "gpu_env_bench.json"), "tools/gpu_env_bench.py", rows)


if __name__ == "__main__":
    main()
