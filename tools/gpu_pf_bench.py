#!/usr/bin/env python3
"""Particle-filter weights: what the fused call costs next to the unfused pair, the parent's best and a plain fan.

Kinds RMGPU, CDDT (theta 108), GiantLUT (theta 108) on colombia; P particles x A beams (a sparse fan over the lidar's
field of view) at 4000 x 54, 4000 x 108, 65 536 x 108 and 2^20 x 54.  Per kind and shape:
  fused     rl_calc_range_repeat_angles_eval_sensor_model_device, everything device-resident
  unfused   rl_calc_range_repeat_angles_device, then rl_eval_sensor_model_device on the device buffers
  baseline  what a caller could do before these calls existed: the (x, y, theta + a_j) rows expanded on the host, the
            2-argument calc_range_many, the statement's product in NumPy (host wall time, fewer repetitions)
and, RMGPU only, rl_calc_range_fan_device of about the same number of rays as 1081-beam fans: on the one-ray-per-lane
kernel (variant 0) and as the planner launches it (variant 1).  Device times are HIP events around each call, median of
--reps calls after warm-up.  Every line is checked against tests/pf_statement.py on a 64-particle subsample before it
is printed.  --out writes the rows as JSON."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pf_statement as PS  # noqa: E402
from oracle import oracle as O  # noqa: E402
from pyracecarsimulator_amd import maps, range_libc, workloads  # noqa: E402

FOV, MRX, THETA, FAN_B = workloads.SCAN_FOV, 300, 108, 1081
SHAPES = [(4000, 54), (4000, 108), (65536, 108), (1 << 20, 54)]


def sensor_table(width, sigma=3.0, floor=0.02):
    """A plain beam model: a Gaussian around the expected bin on a uniform floor, every column summing to one."""
    o = np.arange(width, dtype=np.float64)[:, None]
    e = np.arange(width, dtype=np.float64)[None, :]
    t = np.exp(-0.5 * ((o - e) / sigma) ** 2) + floor
    return np.ascontiguousarray(t / t.sum(0, keepdims=True))


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


def check(ok, what):
    if not ok:
        raise SystemExit("gpu_pf_bench: verification failed: " + what)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kinds", default="RMGPU,CDDT,GLT")
    ap.add_argument("--max-particles", type=int, default=1 << 20)
    ap.add_argument("--baseline-max-rays", type=int, default=1 << 26, help="skip the host baseline beyond this many rays")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reps = max(args.reps, 20)
    g = maps.load_colombia()
    omap = range_libc.PyOMap(g)
    dt = omap.distance_transform()
    om = O.OracleMap.from_gridmap(g, MRX)
    inv_res = PS.inv_res_of(g.resolution)
    table = sensor_table(MRX + 1)
    stream = torch.cuda.current_stream().cuda_stream
    makers = {"RMGPU": lambda: range_libc.PyRayMarchingGPU(omap, MRX), "CDDT": lambda: range_libc.PyCDDTCast(omap, MRX, THETA),
              "GLT": lambda: range_libc.PyGiantLUTCast(omap, MRX, THETA)}
    rows = []
    all_poses = maps.sample_free_poses(g, min(args.max_particles, SHAPES[-1][0]), 17, 2.0, dt).astype(np.float32)
    for kind in args.kinds.split(","):
        m = makers[kind]()
        m.set_sensor_model(table)
        for P, A in SHAPES:
            if P > args.max_particles:
                continue
            poses = np.ascontiguousarray(all_poses[:P])
            angles = np.linspace(-FOV / 2, FOV / 2, A).astype(np.float32)
            # the observation: the scan of a pose nobody else stands on
            obs = np.empty(A, np.float32)
            m.calc_range_repeat_angles(np.ascontiguousarray(all_poses[-1:]), angles, obs)
            d_p, d_a, d_o = (torch.from_numpy(x).cuda() for x in (poses, angles, obs))
            d_r = torch.empty(P * A, dtype=torch.float32, device="cuda")
            d_wf = torch.empty(P, dtype=torch.float64, device="cuda")
            d_wu = torch.empty(P, dtype=torch.float64, device="cuda")

            def fused():
                m.calc_range_repeat_angles_eval_sensor_model_device(d_p.data_ptr(), P, d_a.data_ptr(), d_o.data_ptr(), A,
                                                                    d_wf.data_ptr(), stream=stream)

            def scan():
                m.calc_range_repeat_angles_device(d_p.data_ptr(), P, d_a.data_ptr(), A, d_r.data_ptr(), stream=stream)

            def unfused():
                scan()
                m.eval_sensor_model_device(d_o.data_ptr(), d_r.data_ptr(), d_wu.data_ptr(), A, P, stream=stream)

            for _ in range(3):
                fused()
                unfused()
            torch.cuda.synchronize()
            # verification on a 64-particle subsample: ranges against the statement / the oracle, weights against the
            # statement's ascending product, fused against unfused
            sub = np.random.default_rng(P + A).choice(P, 64, replace=False)
            r_sub = d_r.cpu().numpy().reshape(P, A)[sub]
            if kind == "RMGPU":
                want_r = PS.repeat_angles(g.occ, g.resolution, g.origin, MRX, poses[sub], angles, step_coeff=1.0, dt=om.dt)[0]
                check(want_r.tobytes() == r_sub.tobytes(), "%s %dx%d ranges" % (kind, P, A))
            elif float(g.origin[2]) == 0.0:
                ins = PS.expand_rows(poses[sub], angles)
                want_r = om.cddt_rays(THETA, ins) if kind == "CDDT" else om.lut_rays(m.table(), ins)
                check(want_r.tobytes() == r_sub.tobytes(), "%s %dx%d ranges" % (kind, P, A))
            want_w = PS.weights(table, obs, r_sub, inv_res)
            check(want_w.tobytes() == d_wu.cpu().numpy()[sub].tobytes(), "%s %dx%d unfused weights" % (kind, P, A))
            check(want_w.tobytes() == d_wf.cpu().numpy()[sub].tobytes(), "%s %dx%d fused weights" % (kind, P, A))
            t_f, t_s, t_u = device_ms(fused, reps), device_ms(scan, reps), device_ms(unfused, reps)
            row = dict(kind=kind, map="colombia", particles=P, angles=A, rays=P * A, fused_us=t_f * 1e3,
                       unfused_us=t_u * 1e3, scan_us=t_s * 1e3, fused_grays=P * A / t_f / 1e6,
                       unfused_over_fused=t_u / t_f)
            line = "%-5s %8d x %3d  fused %9.1f us (%6.2f Grays/s)  unfused %9.1f us (scan %9.1f)  unfused/fused %.2fx" % (
                kind, P, A, t_f * 1e3, P * A / t_f / 1e6, t_u * 1e3, t_s * 1e3, t_u / t_f)
            if kind == "RMGPU":
                n_f = max(1, round(P * A / FAN_B))
                fp = torch.from_numpy(np.ascontiguousarray(all_poses[:n_f])).cuda()
                fo = torch.empty(n_f * FAN_B, dtype=torch.float32, device="cuda")
                for variant, key in ((0, "fan_lane_us"), (1, "fan_planner_us")):
                    m.set_option("variant", variant)
                    for _ in range(3):
                        m.calc_range_fan_device(fp.data_ptr(), n_f, FOV, FAN_B, fo.data_ptr(), stream=stream)
                    t = device_ms(lambda: m.calc_range_fan_device(fp.data_ptr(), n_f, FOV, FAN_B, fo.data_ptr(), stream=stream), reps)
                    row[key] = t * 1e3 * (P * A) / (n_f * FAN_B)           # scaled to exactly P * A rays
                m.set_option("variant", 1)
                row["fused_over_fan_lane"] = row["fused_us"] / row["fan_lane_us"]
                line += "  | 1081-beam fan, same rays: one ray per lane %.1f us, planner %.1f us  fused/lane-fan %.2fx" % (
                    row["fan_lane_us"], row["fan_planner_us"], row["fused_over_fan_lane"])
            if P * A <= args.baseline_max_rays:
                n_base = 3 if P * A <= (1 << 23) else 1
                times = []
                for _ in range(n_base):
                    t0 = time.perf_counter()
                    ins = PS.expand_rows(poses, angles)
                    outs = np.empty(P * A, np.float32)
                    m.calc_range_many(ins, outs)
                    w_base = PS.weights(table, obs, outs, inv_res)
                    times.append(time.perf_counter() - t0)
                # (RMGPU's 2-argument form takes sin / cos of theta + a_j directly, the repeat-angle scan adds the angles
                #  by rotation: its ranges are pinned to the oracle's per-ray caster instead of to the fused weights)
                b_sub = outs.reshape(P, A)[sub]
                if kind == "RMGPU":
                    check(om.rm_rays(ins.reshape(P, A, 3)[sub], step_coeff=1.0)[0].tobytes() == b_sub.tobytes(),
                          "%s %dx%d baseline ranges" % (kind, P, A))
                elif float(g.origin[2]) == 0.0:
                    check(b_sub.tobytes() == r_sub.tobytes(), "%s %dx%d baseline ranges" % (kind, P, A))
                check(w_base[sub].tobytes() == PS.weights(table, obs, b_sub, inv_res).tobytes(), "%s %dx%d baseline weights" % (kind, P, A))
                row["baseline_ms"] = float(np.median(times)) * 1e3
                row["baseline_over_fused"] = row["baseline_ms"] * 1e3 / row["fused_us"]
                line += "  | host baseline %.1f ms (%.0fx)" % (row["baseline_ms"], row["baseline_over_fused"])
            rows.append(row)
            print(line, flush=True)
            del d_r, d_wf, d_wu
        m.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=reps, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
