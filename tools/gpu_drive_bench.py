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
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (device buffers of the floor leg)
from pyracecarsimulator_amd import maps, range_libc, workloads, racecar as RC  # noqa: E402
from pyracecarsimulator_amd.followgap import PyFollowGap  # noqa: E402

FOV, B, THRESH, D_BASE, SPEED = workloads.SCAN_FOV, 1081, 0.001, 0.275, 2.0


def composed(cars, m, fg, states, T, edge):
    """The host-composed loop (steps 1-4 of the tick), the way a caller of the existing calls writes it."""
    R = states.shape[0]
    cur, steer = states.copy(), np.zeros(R)
    first = np.full(R, -(T + 1), np.int32)
    alive = np.ones(R, bool)
    for t in range(T):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        _, out, _ = cars.rollout(cur[idx], np.stack([np.full(idx.size, SPEED), steer[idx]], -1)[:, None, :],
                                 n_steps=1, action_every=1)
        cur[idx] = out
        th = out[:, 2]
        poses = np.stack([out[:, 0] + D_BASE * np.cos(th), out[:, 1] + D_BASE * np.sin(th), th], -1).astype(np.float32)
        ranges = np.empty(idx.size * B, np.float32)
        m.calc_range_fan(poses, ranges, FOV, B)
        ranges = ranges.reshape(idx.size, B)
        crashed = ((ranges.astype(np.float64) - edge) < THRESH).any(1)
        first[idx[crashed]] = t
        alive[idx[crashed]] = False
        go = idx[~crashed]
        if go.size:
            steer[go] = fg.eval_many(np.ascontiguousarray(ranges[~crashed]))
    return first


def timed(fn, reps):
    fn()                                                         # warm-up (tables, launch contexts, code objects)
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


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
        g = workloads.cfg2().gmap if mname == "cfg2" else maps.load_colombia()
        omap = range_libc.PyOMap(g)
        dt = omap.distance_transform()
        m = range_libc.PyRayMarchingGPU(omap, workloads.MAX_RANGE_PX)
        fg = PyFollowGap(10, 15.0, RC.DEFAULT_CAR["max_steer_ang"], 0.004)
        cars = RC.CarBatch()
        edge = RC.edge_distances(B, -FOV / 2, FOV / B, D_BASE, RC.DEFAULT_CAR["width"], RC.DEFAULT_CAR["wb"])
        for R in (int(s) for s in a.sizes.split(",")):
            states = np.zeros((R, 11))
            states[:, :3] = maps.sample_free_poses(g, R, 17, 6.0, dt)
            reps = 10 if R <= 64 else 3
            t_closed, res = timed(lambda: cars.drive_followgap(m, fg, states, T, SPEED, FOV, B, edge, THRESH), reps)
            first = res[0]
            # the scan floor: T serial fan launches of R poses on device buffers
            st = torch.cuda.Stream()
            th = states[:, 2]
            p0 = np.stack([states[:, 0] + D_BASE * np.cos(th), states[:, 1] + D_BASE * np.sin(th), th], -1)
            d_poses = torch.from_numpy(p0.astype(np.float32)).cuda()
            d_out = torch.empty(R * B, dtype=torch.float32, device="cuda")

            def floor():
                for _ in range(T):
                    m.calc_range_fan_device(d_poses.data_ptr(), R, FOV, B, d_out.data_ptr(), stream=st.cuda_stream)
                st.synchronize()
            t_floor, _ = timed(floor, reps)
            row = dict(map=mname, R=R, T=T, num_rays=B, method="RMGPU", closed_s=t_closed,
                       closed_ticks_per_s=T / t_closed, closed_grays_per_s=R * T * B / t_closed / 1e9,
                       floor_s=t_floor, floor_grays_per_s=R * T * B / t_floor / 1e9,
                       closed_over_floor=t_closed / t_floor, crashed=int((first >= 0).sum()))
            if R <= a.skip_composed_above:
                t_comp, first_c = timed(lambda: composed(cars, m, fg, states, T, edge), 1)
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
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/gpu_drive_bench.py", rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
