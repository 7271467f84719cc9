#!/usr/bin/env python3
"""Particle-filter localisation: what a whole MCL update costs next to its likelihood alone and next to the update a
caller composes on the host.

Colombia; kinds RMGPU, CDDT (theta 108), GiantLUT (theta 108); P particles x A beams at 4000 x 54, 65 536 x 108 and
2^20 x 54.  Per kind and shape:
  mcl       rl_pf_run over --steps steps (motion noise on, resample ratio 0.5): host wall time of the synchronous call
            divided by the steps — what a caller pays per lidar frame, the upload of odometry and scans and the read-back
            of the estimates included; median of --bursts calls after a warm-up call
  floor (a) rl_calc_range_repeat_angles_eval_sensor_model_device alone on the same particles: device time (HIP events),
            median of --reps calls after warm-up.  A step cannot cost less: it contains this call
  host  (b) the update a caller writes without rl_pf: NumPy motion (same draws budget: three normals per particle), the
            host-pointer fused call, NumPy normalise / estimate / systematic resampling; host wall time per step,
            fewer steps
The first step of a line is checked against tests/mcl_statement.py (L through the public fused call) before the line is
printed.  --out writes the rows as JSON."""
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
import mcl_statement as MS  # noqa: E402
from pyracecarsimulator_amd import ParticleFilter, maps, range_libc, workloads  # noqa: E402

FOV, MRX, THETA = workloads.SCAN_FOV, 300, 108
SHAPES = [(4000, 54), (65536, 108), (1 << 20, 54)]
STD = (0.05, 0.05, 0.02)


def check(ok, what):
    if not ok:
        raise SystemExit("gpu_mcl_bench: verification failed: " + what)


def host_step(m, X, w, odom, angles, obs, rng):
    """The host-composed update: what particle_filter.py does around range_libc's fused call."""
    P = X.shape[0]
    c, s = np.cos(X[:, 2]), np.sin(X[:, 2])
    X = X + np.stack([c * odom[0] - s * odom[1], s * odom[0] + c * odom[1], np.full(P, odom[2])], 1) + rng.normal(0, STD, (P, 3))
    L = np.empty(P)
    m.calc_range_repeat_angles_eval_sensor_model(np.ascontiguousarray(X, np.float32), angles, obs, L)
    w = w * L
    w = w / w.sum()
    est = (w @ X[:, 0], w @ X[:, 1], np.arctan2(w @ np.sin(X[:, 2]), w @ np.cos(X[:, 2])))
    if 1.0 / (w @ w) < 0.5 * P:
        a = np.minimum(P - 1, np.searchsorted(np.cumsum(w), (rng.random() + np.arange(P)) / P, side="right"))
        X, w = X[a], np.full(P, 1.0 / P)
    return X, w, est


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--bursts", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--kinds", default="RMGPU,CDDT,GLT")
    ap.add_argument("--max-particles", type=int, default=1 << 20)
    ap.add_argument("--min-particles", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = maps.load_colombia()
    omap = range_libc.PyOMap(g)
    dt = omap.distance_transform()
    table = MS.gaussian_table(MRX + 1)
    stream = torch.cuda.current_stream().cuda_stream
    makers = {"RMGPU": lambda: range_libc.PyRayMarchingGPU(omap, MRX), "CDDT": lambda: range_libc.PyCDDTCast(omap, MRX, THETA),
              "GLT": lambda: range_libc.PyGiantLUTCast(omap, MRX, THETA)}
    true0 = maps.sample_free_poses(g, 1, 17, 6.0, dt)[0].astype(np.float64)
    T = args.steps
    odom = np.tile([0.5 * g.resolution, 0.0, 0.004], (T, 1))
    rows = []
    for kind in args.kinds.split(","):
        m = makers[kind]()
        m.set_sensor_model(table)
        for P, A in SHAPES:
            if P > args.max_particles or P < args.min_particles:
                continue
            rng = np.random.default_rng(P + A)
            parts = true0[None, :] + rng.normal(0, 1, (P, 3)) * np.array([10 * g.resolution, 10 * g.resolution, 0.2])
            angles = np.linspace(-FOV / 2, FOV / 2, A).astype(np.float32)
            # the observations: the scans of the car's noiseless path
            path = true0[None, :]
            truth = []
            for t in range(T):
                path = MS.motion(path, odom[t], (0, 0, 0), 0, t)
                truth.append(path[0])
            obs = np.empty(T * A, np.float32)
            m.calc_range_repeat_angles(np.ascontiguousarray(truth, np.float32), angles, obs)
            obs = obs.reshape(T, A)
            pf = ParticleFilter(m, angles, P, motion_std=STD, resample_ratio=0.5)
            # verification: one step against the statement, L through the public fused call (2^20 particles — 4096
            # chunk totals under one lane — once, on the first kind: the statement takes its time there)
            if P <= 65536 or kind == args.kinds.split(",")[0]:
                pf.reset(parts, seed=1)
                got = pf.run_raw(odom[:1], obs[:1])
                st = MS.Filter(lambda q, o, t: fused_host(m, q, angles, o), P, STD, 0.5)
                st.reset(parts, seed=1)
                want = st.run(odom[:1], obs[:1])
                check(all(x.tobytes() == y.tobytes() for x, y in zip(got, want)), "%s %dx%d step outputs" % (kind, P, A))
                rd = pf.read()
                check(rd["particles"].tobytes() == st.X.tobytes() and rd["cum"].tobytes() == st.cum.tobytes(),
                      "%s %dx%d state" % (kind, P, A))
            # mcl: whole runs of T steps
            times, resampled = [], 0
            for burst in range(args.bursts + 1):
                pf.reset(parts, seed=1)
                t0 = time.perf_counter()
                est, neff, flags = pf.run_raw(odom, obs)
                if burst:
                    times.append((time.perf_counter() - t0) / T)
                resampled = int((flags & 1).sum())
            mcl_us = float(np.median(times)) * 1e6
            err = float(np.hypot(est[-1, 0] - truth[-1][0], est[-1, 1] - truth[-1][1]))
            # (a) the likelihood alone, on the final particles
            d_p = torch.from_numpy(np.ascontiguousarray(pf.read()["particles"], np.float32)).cuda()
            d_a, d_o = torch.from_numpy(angles).cuda(), torch.from_numpy(obs[-1]).cuda()
            d_w = torch.empty(P, dtype=torch.float64, device="cuda")

            def floor():
                m.calc_range_repeat_angles_eval_sensor_model_device(d_p.data_ptr(), P, d_a.data_ptr(), d_o.data_ptr(), A,
                                                                    d_w.data_ptr(), stream=stream)

            for _ in range(3):
                floor()
            torch.cuda.synchronize()
            ts = []
            for _ in range(max(args.reps, 20)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                floor()
                b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b))
            floor_us = float(np.median(ts)) * 1e3
            # (b) the host-composed update
            X, w = parts.copy(), np.full(P, 1.0 / P)
            hrng = np.random.default_rng(1)
            X, w, _ = host_step(m, X, w, odom[0], angles, obs[0], hrng)           # warm-up
            t0 = time.perf_counter()
            for t in range(1, 1 + args.host_steps):
                X, w, _ = host_step(m, X, w, odom[t], angles, obs[t], hrng)
            host_us = (time.perf_counter() - t0) / args.host_steps * 1e6
            row = dict(kind=kind, map="colombia", particles=P, angles=A, steps=T, mcl_us_per_step=mcl_us,
                       likelihood_us=floor_us, host_us_per_step=host_us, mcl_over_likelihood=mcl_us / floor_us,
                       host_over_mcl=host_us / mcl_us, resampled_steps=resampled, final_error_m=err)
            rows.append(row)
            print("%-5s %8d x %3d  mcl %9.1f us/step  | (a) likelihood alone %9.1f us  mcl/(a) %.2fx  | (b) host-composed "
                  "%10.1f us/step  (b)/mcl %.1fx  | resampled %d of %d steps, final error %.3f m" % (
                      kind, P, A, mcl_us, floor_us, mcl_us / floor_us, host_us, host_us / mcl_us, resampled, T, err), flush=True)
            pf.close()
            del d_p, d_w
        m.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), steps=T, bursts=args.bursts, rows=rows), f, indent=1)


def fused_host(m, q, angles, obs):
    wts = np.empty(q.shape[0])
    m.calc_range_repeat_angles_eval_sensor_model(np.ascontiguousarray(q, np.float32), angles, np.ascontiguousarray(obs, np.float32), wts)
    return wts


if __name__ == "__main__":
    main()
