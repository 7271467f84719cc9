#!/usr/bin/env python3
"""Closed-loop policy roll-outs and the policy network alone (rl_car_drive_policy, rl_policy_eval_device).

Per map (cfg2's 2049^2 maze, colombia) and car count R (1, 64, 4096), T ticks (200) at 2 m/s, RMGPU, 1081 beams:
  policy    CarBatch.drive_policy (steer_clip 0.4189): every tick one fan launch sequence, one policy_mlp_kernel and
            one drive_tick_kernel (policy source), no host sync
  followgap CarBatch.drive_followgap on the same starts (DESIGN section 7a's loop)
  composed  per tick: rollout(n_steps=1) of the live cars -> lidar poses in numpy -> calc_range_fan to the host ->
            the crash test on the host -> Policy.predict_many (the ranges go back to the GPU)
  floor     T serial calc_range_fan_device launches of the R start poses (the scan alone, device buffers)
Then the network alone on a cfg5-sized batch (262 144 scans x 720 beams, in_start 0) and at R = 1, 64, 4096 on
device buffers: the time per launch (HIP events over --mlp-reps back-to-back launches), scans/s and the fraction of
the 155 TFLOP/s f32 MFMA rate.  The weights are tests/golden/policy_mlp720.npz (the reference's network)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from pyracecarsimulator_amd import Policy, maps, range_libc, workloads, racecar as RC  # noqa: E402
from pyracecarsimulator_amd.followgap import PyFollowGap  # noqa: E402
import policy_statement as S  # noqa: E402

FOV, B, THRESH, D_BASE, SPEED, CLIP = workloads.SCAN_FOV, 1081, 0.001, 0.275, 2.0, 0.4189
PEAK_F32 = 155e12


def composed(cars, m, pol, states, T, edge):
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
            steer[go] = np.clip(pol.predict_many(np.ascontiguousarray(ranges[~crashed])).astype(np.float64), -CLIP, CLIP)
    return first


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


def mlp_alone(pol, n, size, reps):
    rng = np.random.default_rng(n)
    d_in = torch.from_numpy(rng.uniform(0.1, 20.0, (n, size)).astype(np.float32)).cuda()
    d_out = torch.empty(n, dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    pol.predict_device(d_in.data_ptr(), n, size, d_out.data_ptr(), stream=st.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(st):
        e0.record(st)
        for _ in range(reps):
            pol.predict_device(d_in.data_ptr(), n, size, d_out.data_ptr(), stream=st.cuda_stream)
        e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / 1e3 / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--sizes", default="1,64,4096")
    ap.add_argument("--maps", default="cfg2,colombia")
    ap.add_argument("--skip-composed-above", type=int, default=1 << 30)
    ap.add_argument("--mlp-reps", type=int, default=20)
    ap.add_argument("--only-mlp", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    T = a.ticks
    layers, relu = S.load_fixture(os.path.join(ROOT, "tests", "golden", "policy_mlp720.npz"))
    flop = 2 * sum(W.size for W, _ in layers)
    pol = Policy.from_arrays(layers, relu)
    rows, mlp_rows = [], []
    for n, size, pol_n in ((262144, 720, Policy.from_arrays(layers, relu, in_start=0)), (4096, B, pol), (64, B, pol),
                           (1, B, pol)):
        t = mlp_alone(pol_n, n, size, a.mlp_reps)
        r = dict(n=n, size=size, s_per_launch=t, us_per_launch=t * 1e6, gscans_per_s=n / t / 1e9,
                 tflops=n * flop / t / 1e12, frac_of_f32_peak=n * flop / t / PEAK_F32)
        mlp_rows.append(r)
        print("mlp n=%6d x %4d: %10.2f us/launch, %.4f Gscans/s, %.2f TFLOP/s (%.3f of 155 TF)" % (
            n, size, r["us_per_launch"], r["gscans_per_s"], r["tflops"], r["frac_of_f32_peak"]), flush=True)
    for mname in ([] if a.only_mlp else a.maps.split(",")):
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
            t_pol, res = timed(lambda: cars.drive_policy(m, pol, states, T, SPEED, FOV, B, edge, THRESH,
                                                         steer_clip=CLIP), reps)
            first = res[0]
            t_fg, _ = timed(lambda: cars.drive_followgap(m, fg, states, T, SPEED, FOV, B, edge, THRESH), reps)
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
            row = dict(map=mname, R=R, T=T, num_rays=B, method="RMGPU", policy_s=t_pol, policy_ticks_per_s=T / t_pol,
                       policy_us_per_tick=t_pol / T * 1e6, followgap_s=t_fg, followgap_us_per_tick=t_fg / T * 1e6,
                       policy_over_followgap=t_pol / t_fg, floor_s=t_floor, floor_us_per_tick=t_floor / T * 1e6,
                       policy_over_floor=t_pol / t_floor, crashed=int((first >= 0).sum()))
            if R <= a.skip_composed_above:
                t_comp, first_c = timed(lambda: composed(cars, m, pol, states, T, edge), 1)
                row.update(composed_s=t_comp, composed_ticks_per_s=T / t_comp, composed_over_policy=t_comp / t_pol,
                           same_crash_tick=int((first_c == first).sum()))
            rows.append(row)
            print("%-8s R=%5d T=%d: policy %8.1f us/tick (%7.0f ticks/s) | followgap %8.1f us/tick, policy/fg %.3f | "
                  "floor %8.1f us/tick, policy/floor %.3f | composed %s | crashed %d" % (
                      mname, R, T, row["policy_us_per_tick"], row["policy_ticks_per_s"], row["followgap_us_per_tick"],
                      row["policy_over_followgap"], row["floor_us_per_tick"], row["policy_over_floor"],
                      ("%8.1f us/tick, composed/policy %.1f, same crash tick %d/%d" % (
                          t_comp / T * 1e6, row["composed_over_policy"], row["same_crash_tick"], R))
                      if "composed_s" in row else "skipped", row["crashed"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/gpu_policy_bench.py", mlp=mlp_rows, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
