#!/usr/bin/env python3
"""Closed-loop Follow-the-Gap roll-outs: rl_car_drive_followgap against the same loop composed on the host from
the public calls, and against the serial scan floor, in one process.

Per map (cfg2's 2049^2 maze, colombia) and car count R (1, 64, 4096), T ticks (200) at simple_driver.py's
VELOCITY (2 m/s), RMGPU, 1081 beams:
  closed    CarBatch.drive_followgap: every tick one fan launch sequence + one drive_tick_kernel (FollowGap source),
            no host sync
  composed  per tick: CarBatch.rollout(n_steps=1) of the live cars -> lidar poses in numpy -> calc_range_fan to the
            host -> Car::isCrashed on the host (numpy, vectorised) -> eval_many (the ranges go back to the GPU)
  floor     T serial calc_range_fan_device launches of the R start poses (the scan alone, device buffers)
Prints ticks/s, Grays/s (R T num_rays rays over the call time) and the ratios; --out writes the rows as JSON."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402,F401  (before the library: device buffers of the floor leg)
from bench_common import B, FOV, THRESH, composed_drive, free_starts, scan_floor, timed, world, write_rows  # noqa: E402

SPEED = 2.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--sizes", default="1,64,4096")
    ap.add_argument("--maps", default="cfg2,colombia")
    ap.add_argument("--skip-composed-above", type=int, default=1 << 30, help="leave out the composed leg above this R")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    T = a.ticks
    rows = []
    for mname in a.maps.split(","):
        g, _, dt, m, fg, cars, edge = world(mname)
        for R in (int(s) for s in a.sizes.split(",")):
            states = free_starts(g, dt, R)
            reps = 10 if R <= 64 else 3
            t_closed, res = timed(lambda: cars.drive_followgap(m, fg, states, T, SPEED, FOV, B, edge, THRESH), reps)
            first = res[0]
            # the scan floor: T serial fan launches of R poses on device buffers
            floor = scan_floor(m, states, T)
            t_floor, _ = timed(floor, reps)
            row = dict(map=mname, R=R, T=T, num_rays=B, method="RMGPU", closed_s=t_closed,
                       closed_ticks_per_s=T / t_closed, closed_grays_per_s=R * T * B / t_closed / 1e9,
                       floor_s=t_floor, floor_grays_per_s=R * T * B / t_floor / 1e9,
                       closed_over_floor=t_closed / t_floor, crashed=int((first >= 0).sum()))
            if R <= a.skip_composed_above:
                t_comp, first_c = timed(lambda: composed_drive(cars, m, fg.eval_many, states, T, edge, SPEED), 1)
                row.update(composed_s=t_comp, composed_ticks_per_s=T / t_comp,
                           composed_grays_per_s=R * T * B / t_comp / 1e9, composed_over_closed=t_comp / t_closed,
                           same_crash_tick=int((first_c == first).sum()))
            rows.append(row)
            print("%-8s R=%5d T=%d: closed %9.2f ms (%8.0f ticks/s, %6.2f Grays/s) | floor %9.2f ms (%6.2f Grays/s), "
                  "closed/floor %.3f | composed %s | crashed %d" % (
                      mname, R, T, t_closed * 1e3, row["closed_ticks_per_s"], row["closed_grays_per_s"], t_floor * 1e3,
                      row["floor_grays_per_s"], row["closed_over_floor"],
                      ("%9.2f ms (%6.2f Grays/s), composed/closed %.2f, same crash tick %d/%d" % (
                          row["composed_s"] * 1e3, row["composed_grays_per_s"], row["composed_over_closed"],
                          row["same_crash_tick"], R)) if "composed_s" in row else "skipped", row["crashed"]),
                  flush=True)
    if a.out:
        write_rows(a.out, "tools/gpu_drive_bench.py", rows)


if __name__ == "__main__":
    main()
