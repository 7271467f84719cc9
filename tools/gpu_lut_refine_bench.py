#!/usr/bin/env python3
"""The origin-corrected GiantLUT query (option lut_refine) next to the default query on cfg3's shape: 2000^2 maze,
theta_disc 1442, 65 536 poses x 1081 beams.

ONE handle and ONE table serve both sides; the option is flipped between bursts, so both rates come from the same
process, the same buffers and the same minutes of the same device:
  lone        one launch on an idle device, HIP events around it; --bursts alternating bursts of --reps launches per
              side, the median launch of every burst, then the median over the bursts
  pipelined   --streams streams with their own pose and range buffers, --depth launches queued on each, events around
              the whole batch; alternating bursts likewise
and, for both, the error against exact ray marching (RMGPU, step coefficient 1.0, on the device) on a pose subsample:
median / p90 / p99 in cells and the share of rays within one cell.  Before anything is timed a 32-pose subsample of the
refined launch is checked against tests/lut_refine_statement.py bit for bit.  --out writes the rows as JSON."""
import argparse
import sys

import numpy as np
import torch

import bench_common as BC
import lut_refine_statement as S
from pyracecarsimulator_amd import range_libc, workloads


def launch_ms(fn, reps):
    """Median device time of ``reps`` single launches."""
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def error_stats(got, exact, res):
    e = np.abs(got.astype(np.float64) - exact.astype(np.float64)) / res
    return dict(median=float(np.median(e)), p90=float(np.percentile(e, 90)), p99=float(np.percentile(e, 99)),
                within_one=float((e <= 1.0).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=0, help="poses per launch (0: cfg3's 65536)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bursts", type=int, default=5)
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--sample", type=int, default=256, help="poses of the error subsample")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    w = workloads.cfg3(args.poses) if args.poses else workloads.cfg3()
    g, P, B = w.gmap, w.n_poses, w.num_rays
    omap = range_libc.PyOMap(g)
    dt = omap.distance_transform()
    poses = workloads.make_poses(w, dt=dt)
    m = range_libc.PyGiantLUTCast(omap, w.max_range_px, w.theta_disc)
    exact_m = range_libc.PyRayMarchingGPU(omap, w.max_range_px)
    streams = [torch.cuda.Stream() for _ in range(args.streams)]
    d_poses = [torch.from_numpy(np.roll(poses, 977 * i, axis=0).copy()).cuda() for i in range(args.streams)]
    d_out = [torch.empty(P * B, dtype=torch.float32, device="cuda") for _ in range(args.streams)]
    cur = torch.cuda.current_stream().cuda_stream

    def lone():
        m.calc_range_fan_device(d_poses[0].data_ptr(), P, w.fov, B, d_out[0].data_ptr(), stream=cur)

    def pipelined():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for s in streams:
            s.wait_event(a)
        for _ in range(args.depth):
            for i, s in enumerate(streams):
                m.calc_range_fan_device(d_poses[i].data_ptr(), P, w.fov, B, d_out[i].data_ptr(), stream=s.cuda_stream)
        for s in streams:
            torch.cuda.current_stream().wait_stream(s)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / (args.depth * args.streams)

    # the error subsample and the bit check (the first launch builds the table)
    sub = np.random.default_rng(1).choice(P, args.sample, replace=False)
    sub_poses = np.ascontiguousarray(poses[sub])
    exact = np.empty(args.sample * B, np.float32)
    exact_m.calc_range_fan(sub_poses, exact, w.fov, B)
    errors = {}
    for side, flag in (("default", 0), ("refined", 1)):
        m.set_option("lut_refine", flag)
        got = np.empty(args.sample * B, np.float32)
        m.calc_range_fan(sub_poses, got, w.fov, B)
        errors[side] = error_stats(got, exact, g.resolution)
        if flag:
            lone()
            torch.cuda.synchronize()
            big = d_out[0].cpu().numpy().reshape(P, B)[sub[:32]]
            if not np.array_equal(big.ravel(), got[:32 * B]):
                sys.exit("gpu_lut_refine_bench: the 65536-pose launch and the subsample launch disagree")
            want = statement_rows(m, g, dt, w, sub_poses[:32])
            if not np.array_equal(want.view(np.uint32), got[:32 * B].view(np.uint32)):
                sys.exit("gpu_lut_refine_bench: the refined query differs from tests/lut_refine_statement.py")
    rows = []
    for mode, fn in (("lone", lambda: launch_ms(lone, args.reps)),
                     ("pipelined", lambda: float(np.median([pipelined() for _ in range(max(1, args.reps // 4))])))):
        ms = {"default": [], "refined": []}
        for _ in range(args.bursts):
            for side, flag in (("default", 0), ("refined", 1)):
                m.set_option("lut_refine", flag)
                fn()                                        # warm-up of the side within the burst
                ms[side].append(fn())
        d, r = float(np.median(ms["default"])), float(np.median(ms["refined"]))
        rows.append(dict(mode=mode, poses=P, beams=B, default_ms=d, refined_ms=r, default_grays=P * B / d / 1e6,
                         refined_grays=P * B / r / 1e6, refined_over_default=r / d,
                         default_ms_bursts=ms["default"], refined_ms_bursts=ms["refined"]))
        print("%-9s default %.4f ms (%6.1f Grays/s)   refined %.4f ms (%6.1f Grays/s)   refined/default %.3f" % (
            mode, d, P * B / d / 1e6, r, P * B / r / 1e6, r / d), flush=True)
    for side in ("default", "refined"):
        e = errors[side]
        print("vs_exact_rm %-8s median %.3f  p90 %.2f  p99 %.1f cells   within one cell %.3f   (%d poses)" % (
            side, e["median"], e["p90"], e["p99"], e["within_one"], args.sample), flush=True)
    m.set_option("lut_refine", 0)
    if args.out:
        BC.write_rows(args.out, "gpu_lut_refine_bench", rows, device=torch.cuda.get_device_name(0), workload=w.describe(),
                      vs_exact_rm=errors, reps=args.reps, bursts=args.bursts, streams=args.streams, depth=args.depth)


def statement_rows(m, g, dt, w, poses):
    """The statement on a few poses without reading the whole 11.5 GB table back: per pose the one table row its corner
    rule picks, behind a view the statement indexes like the whole table."""
    from oracle import np_statement as N
    gx, gy, _ = N._pose_grid(g.resolution, g.origin, poses)
    _, c, r, _, _, _, _ = S.corner(dt, gx, gy)
    out = np.empty(len(poses) * w.num_rays, np.float32)
    for i in range(len(poses)):                              # one row of the table per pose (2000 x 1442 x 2 B)
        view = _RowView(m.table(int(r[i]), int(r[i]) + 1), int(r[i]), dt.shape[0])
        out[i * w.num_rays:(i + 1) * w.num_rays] = S.lut_refine_fan(view, dt, g.resolution, g.origin, w.max_range_px,
                                                                    poses[i:i + 1], w.fov, w.num_rays)
    return out


class _RowView:
    """A (rows, cols, theta_disc) table of which one row is held: indexing any other row is an error."""
    def __init__(self, slab, row, rows):
        self.slab, self.row = slab, row
        self.shape = (rows, slab.shape[1], slab.shape[2])

    def __getitem__(self, key):
        r, c, b = key
        assert (np.asarray(r) == self.row).all()
        return self.slab[np.zeros_like(np.asarray(r)), c, b]


if __name__ == "__main__":
    main()
