#!/usr/bin/env python3
"""What track progress costs a DriveEnv step, and what the same rows cost composed on the host.

Colombia, RMGPU, 1081 beams, substeps 1, auto_reset, max_ticks 200, a pool of 512 starts, gpu_env_bench.py's torch
controller.  Per case (N envs, W waypoints, window):
  plain     DriveEnv.step in the device form, no track: the baseline, measured in the same run
  track     the same env with a track attached (one more kernel per step, track_kernel)
  host      the plain env's step, then the rows the way a caller without the feature gets them: env.read() (the states
            over PCIe, a device synchronise) and the statement's nearest-segment and goal search in NumPy, vectorised
            over N x S (tests/track_statement.py's arithmetic on arrays)
plain and track are warmed up and timed `--reps` times in alternating windows of `--steps` steps (a host clock around
work that ends in a device synchronise); host is timed over `--host-steps` steps per window.  Medians and the spread are
printed and, with --out-dir, written.  Tracks: W = 36 is tests/golden/wp_u.csv, W = 1024 a ring; where they lie on the
map does not change the work."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_common import B, FOV, ROOT, THRESH, free_starts, world, write_rows  # noqa: E402
from gpu_env_bench import CLIP, GAIN, MAX_TICKS, POOL, SPEED  # noqa: E402


def track_xy(W):
    from pyracecarsimulator_amd import Track
    if W == 36:
        return Track.read_csv(os.path.join(ROOT, "tests", "golden", "wp_u.csv"))
    a = np.arange(W) * (2 * math.pi / W)
    return np.stack([20.0 + 15.0 * np.cos(a), 20.0 + 12.0 * np.sin(a)], -1)


class Leg:
    """A DriveEnv in the device form under the torch controller; `track`: a Track or None."""

    def __init__(self, w, starts, N, track, window):
        import torch
        from pyracecarsimulator_amd import DriveEnv
        self.torch = torch
        _, _, _, m, _, cars, edge = w
        self.env = DriveEnv(m, starts, N, B, FOV, edge, THRESH, max_ticks=MAX_TICKS, auto_reset=True, car=cars,
                            track=track, track_window=window)
        self.act = torch.empty((N, 2), dtype=torch.float32, device="cuda")
        self.act[:, 0] = SPEED
        self.obs = self.env.reset(seed=1, on_device=True)

    def step(self):
        torch, third = self.torch, B // 3
        self.act[:, 1] = torch.clamp(GAIN * (self.obs[:, B - third:].mean(1) - self.obs[:, :third].mean(1)), -CLIP, CLIP)
        self.obs, _, _ = self.env.step(self.act)

    def run(self, steps):
        for _ in range(steps):
            self.step()
        self.torch.cuda.synchronize()


class HostLeg(Leg):
    """The plain env, and after every step the states over PCIe and the search in NumPy."""

    def __init__(self, w, starts, N, xy, window):
        super().__init__(w, starts, N, None, 0)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import track_statement as TS
        self.T, self.window, self.la = TS.build(xy, True), window, 1.5
        self.seg = None

    def search(self, st):
        T = self.T
        cx, cy = st[:, 0:1], st[:, 1:2]
        if self.window and self.seg is not None and 2 * self.window + 1 < T["S"]:
            idx = (self.seg[:, None] + np.arange(-self.window, self.window + 1)[None, :]) % T["S"]
        else:
            idx = np.broadcast_to(np.arange(T["S"]), (st.shape[0], T["S"]))
        ax, ay = cx - T["x"][idx], cy - T["y"][idx]
        t = np.minimum(np.maximum((ax * T["dx"][idx] + ay * T["dy"][idx]) / T["q"][idx], 0.0), 1.0)
        ex, ey = ax - t * T["dx"][idx], ay - t * T["dy"][idx]
        k = np.argmin(ex * ex + ey * ey, 1)
        self.seg = idx[np.arange(st.shape[0]), k]
        rx, ry = T["x"][None, :] - cx, T["y"][None, :] - cy
        g = np.abs(self.la - np.sqrt(rx * rx + ry * ry))
        return self.seg, np.argmin(g, 1)

    def run(self, steps):
        for _ in range(steps):
            self.step()
            self.search(self.env.read()["states"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="256,4096")
    ap.add_argument("--points", default="36,1024")
    ap.add_argument("--windows", default="0,16")
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--host-steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out-dir", default="")
    a = ap.parse_args()
    from pyracecarsimulator_amd import Track
    w = world("colombia")
    starts = free_starts(w[0], w[2], POOL)
    rows, lines = [], []
    for N in (int(s) for s in a.sizes.split(",")):
        for W in (int(s) for s in a.points.split(",")):
            xy = track_xy(W)
            trk = Track(xy)
            for window in (int(s) for s in a.windows.split(",")):
                legs = dict(plain=Leg(w, starts, N, None, 0), track=Leg(w, starts, N, trk, window),
                            host=HostLeg(w, starts, N, xy, window))
                for leg in legs.values():
                    leg.run(10)                                 # warm-up
                t = {k: [] for k in legs}
                for _ in range(a.reps):                         # alternating windows: the machine is shared
                    for k, leg in legs.items():
                        n = a.host_steps if k == "host" else a.steps
                        t0 = time.perf_counter()
                        leg.run(n)
                        t[k].append((time.perf_counter() - t0) / n * 1e6)
                med = {k: statistics.median(v) for k, v in t.items()}
                row = dict(map="colombia", method="RMGPU", n_envs=N, num_rays=B, points=W, window=window, steps=a.steps,
                           host_steps=a.host_steps, reps=a.reps, track_minus_plain_us=med["track"] - med["plain"],
                           track_over_plain=med["track"] / med["plain"], host_over_track=med["host"] / med["track"])
                for k in legs:
                    row.update({k + "_us_per_step": med[k], k + "_us_min": min(t[k]), k + "_us_max": max(t[k])})
                rows.append(row)
                line = ("N=%5d W=%5d window=%3d: plain %8.1f us/step [%.1f .. %.1f] | track %8.1f [%.1f .. %.1f] "
                        "(%+.1f us, x%.3f) | host-composed %9.1f [%.1f .. %.1f] (x%.1f of track)" % (
                            N, W, window, med["plain"], min(t["plain"]), max(t["plain"]), med["track"], min(t["track"]),
                            max(t["track"]), row["track_minus_plain_us"], row["track_over_plain"], med["host"],
                            min(t["host"]), max(t["host"]), row["host_over_track"]))
                lines.append(line)
                print(line, flush=True)
                for leg in legs.values():
                    leg.env.close()
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "gpu_track_bench.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        write_rows(os.path.join(a.out_dir, "gpu_track_bench.json"), "tools/gpu_track_bench.py", rows)


if __name__ == "__main__":
    main()
