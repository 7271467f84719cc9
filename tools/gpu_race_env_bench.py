#!/usr/bin/env python3
"""The race environment (rl_env_create_race, RaceEnv) against the closed race loop and against the same tick composed
from the public calls.

Colombia, RMGPU, 1081 beams, substeps 1, N = 4096 cars in races of P = 2 and P = 4, auto_reset, max_ticks 200,
min_running 1, a pool of 512 line-ups:
  env       RaceEnv.step on torch tensors (the device form, torch.cuda.current_stream()) under a trivial torch
            controller: constant speed, steer = clamp(gain * (mean of the left third - mean of the right third)).
            Nothing is copied to the host and nothing waits for the GPU between steps; one synchronise ends the window.
  race      a tick of rl_car_race_followgap with the same cars: one synchronous call of --ticks ticks, divided by the
            ticks (FollowGap compiled in; crashed cars freeze, nothing re-spawns).
  composed  the tick the way a caller of the parent's public calls writes it, the same controller in NumPy:
            CarBatch.rollout(n_steps=1) of the running cars -> lidar poses in NumPy -> calc_range_fan_cars to the host
            -> Car::isCrashed on the host (NumPy, vectorised) -> the race rule and the re-spawn of finished races.
The legs are warmed up, then timed `--reps` times in alternation (a host clock around work that ends in a device
synchronise); the medians and the spread are printed, and with --out-dir written as text and JSON."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_common import B, FOV, THRESH, lidar_poses, world, write_rows  # noqa: E402
from gpu_race_bench import race_states  # noqa: E402

SPEED, GAIN, CLIP = 2.0, 0.1, 0.4189
MAX_TICKS, POOL, N = 200, 512, 4096


class EnvLeg:
    def __init__(self, w, pool, P):
        import torch
        from pyracecarsimulator_amd import RaceEnv
        self.torch = torch
        g, _, dt, m, _, cars, edge = w
        self.env = RaceEnv(m, pool, N // P, B, FOV, edge, THRESH, min_running=1, max_ticks=MAX_TICKS, auto_reset=True,
                           car=cars)
        self.act = torch.empty((N // P, P, 2), dtype=torch.float32, device="cuda")
        self.act[..., 0] = SPEED
        self.obs = self.env.reset(seed=1, on_device=True)

    def run(self, steps):
        torch, third = self.torch, B // 3
        for _ in range(steps):
            self.act[..., 1] = torch.clamp(GAIN * (self.obs[..., B - third:].mean(-1) - self.obs[..., :third].mean(-1)),
                                           -CLIP, CLIP)
            self.obs, _, _ = self.env.step(self.act)
        torch.cuda.synchronize()


class RaceLeg:
    def __init__(self, w, pool, P):
        _, _, _, self.m, self.fg, self.cars, self.edge = w
        self.states = np.ascontiguousarray(pool[np.arange(N // P) % POOL])

    def run(self, ticks):
        self.cars.race_followgap(self.m, self.fg, self.states, ticks, SPEED, FOV, B, self.edge, THRESH)


class ComposedLeg:
    def __init__(self, w, pool, P):
        _, _, _, self.m, _, self.cars, self.edge = w
        self.pool, self.P, self.R = pool, P, N // P
        self.rng = np.random.default_rng(1)
        self.cur = pool[self.rng.integers(0, POOL, self.R)].reshape(N, 11).copy()
        self.race_tick = np.zeros(self.R, np.int32)
        self.done = np.zeros(N, bool)
        self.over = np.zeros(self.R, bool)
        self.obs = self.scan()

    def scan(self):
        return self.m.calc_range_fan_cars(lidar_poses(self.cur), self.cur[:, :3], self.P, FOV, B).reshape(N, B)

    def run(self, steps):
        P, third = self.P, B // 3
        obs = self.obs
        for _ in range(steps):
            steer = np.clip(GAIN * (obs[:, B - third:].mean(1) - obs[:, :third].mean(1)), -CLIP, CLIP)
            fresh = np.nonzero(self.over)[0]
            if fresh.size:                                         # finished races spawn as a whole
                self.cur.reshape(self.R, P, 11)[fresh] = self.pool[self.rng.integers(0, POOL, fresh.size)]
                self.race_tick[fresh] = 0
                self.done.reshape(self.R, P)[fresh] = False
            stepping = ~self.done & ~np.repeat(self.over, P)
            self.over[fresh] = False
            live = np.nonzero(stepping)[0]
            if live.size:
                acts = np.stack([np.full(live.size, SPEED), steer[live].astype(np.float64)], -1)[:, None, :]
                _, out, _ = self.cars.rollout(self.cur[live], acts, n_steps=1, action_every=1)
                self.cur[live] = out
            self.race_tick += 1
            self.race_tick[fresh] = 0
            obs = self.scan()
            crashed = ((obs.astype(np.float64) - self.edge) < THRESH).any(1)
            self.done |= crashed
            self.over = (~self.done.reshape(self.R, P)).sum(1) < 1
            self.over |= self.race_tick == MAX_TICKS
        self.obs = obs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--groups", default="2,4")
    ap.add_argument("--steps", type=int, default=300, help="steps of a timed window of the env leg")
    ap.add_argument("--ticks", type=int, default=100, help="ticks of a timed rl_car_race_followgap call")
    ap.add_argument("--composed-steps", type=int, default=5, help="steps of a timed window of the composed leg")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out-dir", default="")
    a = ap.parse_args()
    w = world("colombia")
    rows, lines = [], []
    for P in (int(s) for s in a.groups.split(",")):
        pool = race_states(w[0], w[2], POOL, P, 5 + P)
        env, race, comp = EnvLeg(w, pool, P), RaceLeg(w, pool, P), ComposedLeg(w, pool, P)
        env.run(20)                            # warm-up: tables, launch contexts, code objects, torch's kernels
        race.run(5)
        comp.run(2)
        t_env, t_race, t_comp = [], [], []
        for _ in range(a.reps):                # alternating: other people's work shares the host
            for leg, n, ts in ((env, a.steps, t_env), (race, a.ticks, t_race), (comp, a.composed_steps, t_comp)):
                t0 = time.perf_counter()
                leg.run(n)
                ts.append((time.perf_counter() - t0) / n)
        e, r, c = (statistics.median(t) for t in (t_env, t_race, t_comp))
        row = dict(map="colombia", method="RMGPU", cars=N, group=P, num_rays=B, substeps=1, steps=a.steps, ticks=a.ticks,
                   composed_steps=a.composed_steps, reps=a.reps, env_us_per_step=e * 1e6, env_us_min=min(t_env) * 1e6,
                   env_us_max=max(t_env) * 1e6, race_tick_us=r * 1e6, race_tick_us_min=min(t_race) * 1e6,
                   race_tick_us_max=max(t_race) * 1e6, composed_us_per_step=c * 1e6, composed_us_min=min(t_comp) * 1e6,
                   composed_us_max=max(t_comp) * 1e6, env_over_race_tick=e / r, env_minus_race_tick_us=(e - r) * 1e6,
                   composed_over_env=c / e)
        rows.append(row)
        line = ("colombia N=%d P=%d: env %8.1f us/step [%.1f .. %.1f] | race tick %8.1f us [%.1f .. %.1f] | composed %10.1f "
                "us/step [%.1f .. %.1f] | env/race tick %.3f (%+.1f us) | composed/env %.1f" % (
                    N, P, row["env_us_per_step"], row["env_us_min"], row["env_us_max"], row["race_tick_us"],
                    row["race_tick_us_min"], row["race_tick_us_max"], row["composed_us_per_step"], row["composed_us_min"],
                    row["composed_us_max"], row["env_over_race_tick"], row["env_minus_race_tick_us"],
                    row["composed_over_env"]))
        lines.append(line)
        print(line, flush=True)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "gpu_race_env_bench.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        write_rows(os.path.join(a.out_dir, "gpu_race_env_bench.json"), "tools/gpu_race_env_bench.py", rows)


if __name__ == "__main__":
    main()
