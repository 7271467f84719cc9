#!/usr/bin/env python3
"""Batched multi-car races: what the other cars cost the scan, and what a race tick costs.

  (a) the race scan (rl_calc_range_fan_cars_device) of R P = 4096 cars x 1081 beams on colombia, RMGPU, at P = 2 and
      P = 4, against the same kernel at group = 1 (no other cars) and against rl_calc_range_fan_device of the same
      poses (the production planner).  Device time from HIP events around each launch, median of --reps.
  (b) a race tick (rl_car_race_followgap, P = 2 and 4) against a rl_car_drive_followgap tick with the same 4096 cars:
      host wall time of one synchronous call of --ticks ticks, divided by the ticks.
  (c) the race tick against the per-race stamp-and-scan loop possible without it (PyOMap.stamp_cells of the other
      car's outline, then an ordinary scan, per car), R = 64 races of P = 2: microseconds per race-tick.
Prints one line per row; --out writes the rows as JSON."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_common import B, FOV, THRESH, lidar_poses, world, write_rows  # noqa: E402
from pyracecarsimulator_amd import maps, range_libc  # noqa: E402


def race_states(g, dt, n_races, group, seed, spread=1.0):
    rng = np.random.default_rng(seed)
    centres = maps.sample_free_poses(g, n_races, seed, 12.0, dt).astype(np.float64)
    s = np.zeros((n_races * group, 11))
    s[:, :3] = np.repeat(centres, group, 0)
    s[:, :2] += rng.uniform(-spread, spread, (n_races * group, 2))
    s[:, 2] = rng.uniform(-np.pi, np.pi, n_races * group)
    s[:, 3] = 2.0
    return s.reshape(n_races, group, 11)


def device_ms(fn, reps):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    g, omap, dt, m, fg, cb, edge = world("colombia")
    stream = torch.cuda.current_stream().cuda_stream
    N = 4096

    # (a) the scan
    for P in (2, 4):
        st = race_states(g, dt, N // P, P, 5 + P).reshape(N, 11)
        cars = torch.from_numpy(np.ascontiguousarray(st[:, :3])).cuda()
        poses = torch.from_numpy(lidar_poses(st)).cuda()
        out = torch.empty(N * B, dtype=torch.float32, device="cuda")
        for _ in range(3):
            m.calc_range_fan_cars_device(poses.data_ptr(), cars.data_ptr(), N // P, P, FOV, B, out.data_ptr(), stream=stream)
            m.calc_range_fan_device(poses.data_ptr(), N, FOV, B, out.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        race = device_ms(lambda: m.calc_range_fan_cars_device(poses.data_ptr(), cars.data_ptr(), N // P, P, FOV, B,
                                                              out.data_ptr(), stream=stream), args.reps)
        alone = device_ms(lambda: m.calc_range_fan_cars_device(poses.data_ptr(), cars.data_ptr(), N, 1, FOV, B,
                                                               out.data_ptr(), stream=stream), args.reps)
        plan = device_ms(lambda: m.calc_range_fan_device(poses.data_ptr(), N, FOV, B, out.data_ptr(), stream=stream),
                         args.reps)
        rows.append(dict(row="a_scan", map="colombia", cars=N, group=P, beams=B, race_us=race * 1e3,
                         group1_us=alone * 1e3, planner_us=plan * 1e3, race_over_group1=race / alone,
                         race_over_planner=race / plan))
        print("(a) scan  P=%d  race %.1f us  group=1 %.1f us  planner %.1f us  race/group1 %.2fx  race/planner %.2fx"
              % (P, race * 1e3, alone * 1e3, plan * 1e3, race / alone, race / plan), flush=True)

    # (b) the tick
    T = args.ticks
    for P in (2, 4):
        st = race_states(g, dt, N // P, P, 5 + P)
        cb.race_followgap(m, fg, st, 5, 2.0, FOV, B, edge, THRESH)
        t0 = time.perf_counter()
        cb.race_followgap(m, fg, st, T, 2.0, FOV, B, edge, THRESH)
        race = (time.perf_counter() - t0) / T
        flat = st.reshape(N, 11)
        cb.drive_followgap(m, fg, flat, 5, 2.0, FOV, B, edge, THRESH)
        t0 = time.perf_counter()
        cb.drive_followgap(m, fg, flat, T, 2.0, FOV, B, edge, THRESH)
        drive = (time.perf_counter() - t0) / T
        rows.append(dict(row="b_tick", map="colombia", cars=N, group=P, ticks=T, race_tick_us=race * 1e6,
                         drive_tick_us=drive * 1e6, race_over_drive=race / drive))
        print("(b) tick  P=%d  race %.1f us  drive_followgap %.1f us  ratio %.2fx" % (P, race * 1e6, drive * 1e6,
                                                                                       race / drive), flush=True)

    # (c) against the per-race stamp-and-scan loop, R = 64, P = 2
    R, P = 64, 2
    st = race_states(g, dt, R, P, 77)
    flat = st.reshape(-1, 11)
    cells, counts = cb.outline_cells(omap, flat[:, :3])
    poses = lidar_poses(flat)
    omap2 = range_libc.PyOMap(g)
    m2 = range_libc.PyRayMarchingGPU(omap2, 300)
    one = np.empty(B, np.float32)
    t_loop = []
    for rep in range(3):
        t0 = time.perf_counter()
        for r in range(R):
            for k in range(P):
                other = r * P + (1 - k)
                omap2.stamp_cells(cells[other, :counts[other]].astype(np.int64))
                m2.calc_range_fan(poses[r * P + k:r * P + k + 1], one, FOV, B)
        t_loop.append((time.perf_counter() - t0) / R)
    omap2.stamp_cells(np.zeros(0, np.int64))
    cb.race_followgap(m, fg, st, 5, 2.0, FOV, B, edge, THRESH)
    t0 = time.perf_counter()
    cb.race_followgap(m, fg, st, T, 2.0, FOV, B, edge, THRESH)
    race = (time.perf_counter() - t0) / T / R
    loop = float(np.median(t_loop))
    rows.append(dict(row="c_vs_stamp_loop", map="colombia", races=R, group=P, race_us_per_race_tick=race * 1e6,
                     stamp_loop_us_per_race_tick=loop * 1e6, speedup=loop / race))
    print("(c) R=64 P=2  race %.2f us per race-tick  stamp-and-scan loop %.1f us per race-tick (scans only)  %.0fx"
          % (race * 1e6, loop * 1e6, loop / race), flush=True)
    if args.out:
        write_rows(args.out, None, rows, device=torch.cuda.get_device_name(0))


if __name__ == "__main__":
    main()
