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
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from bench_common import (B, FOV, ROOT, THRESH, composed_drive, free_starts, scan_floor, timed, world,  # noqa: E402
                          write_rows)
from pyracecarsimulator_amd import Policy  # noqa: E402
import policy_statement as S  # noqa: E402

SPEED, CLIP = 2.0, 0.4189
PEAK_F32 = 155e12


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
        g, _, dt, m, fg, cars, edge = world(mname)
        for R in (int(s) for s in a.sizes.split(",")):
            states = free_starts(g, dt, R)
            reps = 10 if R <= 64 else 3
            t_pol, res = timed(lambda: cars.drive_policy(m, pol, states, T, SPEED, FOV, B, edge, THRESH,
                                                         steer_clip=CLIP), reps)
            first = res[0]
            t_fg, _ = timed(lambda: cars.drive_followgap(m, fg, states, T, SPEED, FOV, B, edge, THRESH), reps)
            floor = scan_floor(m, states, T)
            t_floor, _ = timed(floor, reps)
            row = dict(map=mname, R=R, T=T, num_rays=B, method="RMGPU", policy_s=t_pol, policy_ticks_per_s=T / t_pol,
                       policy_us_per_tick=t_pol / T * 1e6, followgap_s=t_fg, followgap_us_per_tick=t_fg / T * 1e6,
                       policy_over_followgap=t_pol / t_fg, floor_s=t_floor, floor_us_per_tick=t_floor / T * 1e6,
                       policy_over_floor=t_pol / t_floor, crashed=int((first >= 0).sum()))
            if R <= a.skip_composed_above:
                t_comp, first_c = timed(lambda: composed_drive(
                    cars, m, lambda r: np.clip(pol.predict_many(r).astype(np.float64), -CLIP, CLIP), states, T, edge,
                    SPEED), 1)
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
        write_rows(a.out, "tools/gpu_policy_bench.py", rows, mlp=mlp_rows)


if __name__ == "__main__":
    main()
