#!/usr/bin/env python3
"""Per-seat drivers (include/scanlib_seats.h) against the parent's only way to put scripted opponents on the track.

Colombia, RMGPU, 1081 beams, 1024 races x 4 cars, substeps 1, auto_reset, max_ticks 200, min_running 1, a pool of 512
line-ups; seat 0 is the caller's (a constant action tensor), seats 1-3 the opponents':
  seated    RaceEnv(seats=[None, X, X, X]).step on torch tensors, window (180, 720, 1) in the network's input form: the
            opponents' answers never leave the library (X = FollowGap: no launch more than a plain env; X = the
            network: policy_mlp_rows_kernel over the 3072 opponent cars);
  parent    a plain RaceEnv on the raw full window, then rl_followgap_eval_device / rl_policy_eval_device over all 4096
            observations, then a torch scatter of the opponents' answers into the action tensor, then the step.
  race      CarBatch.race_seats with FollowGap in every seat against CarBatch.race_followgap (the same work a tick:
            the two should lie inside each other's run-to-run spread).
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
import policy_statement as PS  # noqa: E402  (tests/: bench_common put it on the path)

R, P, POOL, MAX_TICKS, SPEED, CLIP = 1024, 4, 512, 200, 2.0, 0.4189
N = R * P
WINDOW = dict(obs_window=(180, 720, 1), obs_clip=15.0, obs_scale=15.0)
ENV_KW = dict(min_running=1, max_ticks=MAX_TICKS, auto_reset=True, steer_clip=CLIP)


class SeatedLeg:
    def __init__(self, w, pool, driver):
        import torch
        from pyracecarsimulator_amd import RaceEnv
        self.torch = torch
        _, _, _, m, _, cars, edge = w
        self.env = RaceEnv(m, pool, R, B, FOV, edge, THRESH, car=cars, seats=[None, driver, driver, driver],
                           seat_speed=SPEED, **WINDOW, **ENV_KW)
        self.act = torch.zeros((R, P, 2), dtype=torch.float32, device="cuda")
        self.act[..., 0] = SPEED
        self.env.reset(seed=1, on_device=True)

    def run(self, steps):
        for _ in range(steps):
            self.env.step(self.act)
        self.torch.cuda.synchronize()


class ParentLeg:
    """The raw window, the driver over every observation, the scatter, the step."""

    def __init__(self, w, pool, driver, is_net):
        import torch
        from pyracecarsimulator_amd import RaceEnv
        self.torch, self.driver, self.is_net = torch, driver, is_net
        _, _, _, m, _, cars, edge = w
        self.env = RaceEnv(m, pool, R, B, FOV, edge, THRESH, car=cars, **ENV_KW)
        self.act = torch.zeros((R, P, 2), dtype=torch.float32, device="cuda")
        self.act[..., 0] = SPEED
        self.ans = torch.zeros(N, dtype=torch.float32, device="cuda")
        self.obs = self.env.reset(seed=1, on_device=True)

    def run(self, steps):
        torch = self.torch
        for _ in range(steps):
            st = torch.cuda.current_stream().cuda_stream
            if self.is_net:
                self.driver.predict_device(self.obs.data_ptr(), N, B, self.ans.data_ptr(), st)
            else:
                self.driver.eval_many_device(self.obs.data_ptr(), N, B, self.ans.data_ptr(), st)
            self.act[:, 1:, 1] = self.ans.view(R, P)[:, 1:]
            self.obs, _, _ = self.env.step(self.act)
        torch.cuda.synchronize()


class RaceLeg:
    def __init__(self, w, pool, seated):
        _, _, _, self.m, self.fg, self.cars, self.edge = w
        self.states, self.seated = np.ascontiguousarray(pool[np.arange(R) % POOL]), seated

    def run(self, ticks):
        if self.seated:
            self.cars.race_seats(self.m, [self.fg] * P, self.states, ticks, SPEED, FOV, B, self.edge, THRESH)
        else:
            self.cars.race_followgap(self.m, self.fg, self.states, ticks, SPEED, FOV, B, self.edge, THRESH)


def alternate(legs, reps):
    """legs: [(name, leg, n)]; returns {name: seconds per unit, one per rep}."""
    out = {name: [] for name, _, _ in legs}
    for _ in range(reps):                          # alternating: other people's work shares the host
        for name, leg, n in legs:
            t0 = time.perf_counter()
            leg.run(n)
            out[name].append((time.perf_counter() - t0) / n)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200, help="steps of a timed window of the env legs")
    ap.add_argument("--ticks", type=int, default=100, help="ticks of a timed roll-out call")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out-dir", default="")
    a = ap.parse_args()
    from pyracecarsimulator_amd import Policy
    w = world("colombia")
    pool = race_states(w[0], w[2], POOL, P, 9)
    layers, relu = PS.load_fixture(os.path.join(ROOT, "tests", "golden", "policy_mlp720.npz"))
    pol, fg = Policy.from_arrays(layers, relu), w[4]
    rows, lines = [], []
    for what, driver, is_net in (("followgap", fg, False), ("policy", pol, True)):
        legs = [("seated", SeatedLeg(w, pool, driver), a.steps), ("parent", ParentLeg(w, pool, driver, is_net), a.steps)]
        for _, leg, _ in legs:
            leg.run(20)                            # warm-up: tables, launch contexts, code objects, torch's kernels
        t = alternate(legs, a.reps)
        s, p = statistics.median(t["seated"]), statistics.median(t["parent"])
        rows.append(dict(leg="env", opponents=what, races=R, group=P, num_rays=B, steps=a.steps, reps=a.reps,
                         seated_us_per_step=s * 1e6, seated_us_min=min(t["seated"]) * 1e6, seated_us_max=max(t["seated"]) * 1e6,
                         parent_us_per_step=p * 1e6, parent_us_min=min(t["parent"]) * 1e6, parent_us_max=max(t["parent"]) * 1e6,
                         parent_over_seated=p / s))
        lines.append("env, 3 %s opponents of 4 cars, %d races: seated %8.1f us/step [%.1f .. %.1f] | parent's way %8.1f "
                     "us/step [%.1f .. %.1f] | parent/seated %.3f" % (
                         what, R, s * 1e6, min(t["seated"]) * 1e6, max(t["seated"]) * 1e6, p * 1e6, min(t["parent"]) * 1e6,
                         max(t["parent"]) * 1e6, p / s))
        print(lines[-1], flush=True)
    legs = [("race_seats", RaceLeg(w, pool, True), a.ticks), ("race_followgap", RaceLeg(w, pool, False), a.ticks)]
    for _, leg, _ in legs:
        leg.run(5)
    t = alternate(legs, a.reps)
    s, p = statistics.median(t["race_seats"]), statistics.median(t["race_followgap"])
    rows.append(dict(leg="race", races=R, group=P, num_rays=B, ticks=a.ticks, reps=a.reps, race_seats_tick_us=s * 1e6,
                     race_seats_us_min=min(t["race_seats"]) * 1e6, race_seats_us_max=max(t["race_seats"]) * 1e6,
                     race_followgap_tick_us=p * 1e6, race_followgap_us_min=min(t["race_followgap"]) * 1e6,
                     race_followgap_us_max=max(t["race_followgap"]) * 1e6, seats_over_followgap=s / p))
    lines.append("roll-out, FollowGap in every seat, %d races x %d: race_seats %8.1f us/tick [%.1f .. %.1f] | race_followgap "
                 "%8.1f us/tick [%.1f .. %.1f] | ratio %.4f" % (
                     R, P, s * 1e6, min(t["race_seats"]) * 1e6, max(t["race_seats"]) * 1e6, p * 1e6,
                     min(t["race_followgap"]) * 1e6, max(t["race_followgap"]) * 1e6, s / p))
    print(lines[-1], flush=True)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "gpu_seats_bench.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        write_rows(os.path.join(a.out_dir, "gpu_seats_bench.json"), "tools/gpu_seats_bench.py", rows)


if __name__ == "__main__":
    main()
