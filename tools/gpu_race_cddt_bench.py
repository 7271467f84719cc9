#!/usr/bin/env python3
"""Batched races on CDDT (handle option race_cddt) next to what there was: 4096 cars x 1081 beams on colombia,
theta_disc 112, races of P = 1, 2 and 4.

  scan_cddt   the CDDT race scan (rl_calc_range_fan_cars_device on a CDDT handle with the option)
  scan_rm     the RMGPU race scan of the same cars: what a race scan cost before
  scan_floor  rl_calc_range_fan_device of the same poses on the same CDDT handle: the scan with nobody to see
  tick_cddt / tick_rm   a rl_car_race_followgap tick on either method (host wall time of one call over its ticks)

One figure per process: without --figure the tool computes the references on the host, then starts a fresh child per
figure, one after the other.  A child first checks its launch against the reference on the cars of the first two races
— tests/race_cddt_statement.py for the CDDT race scan, the oracle on the stamped grid for the RMGPU one,
np_statement.cddt_fan for the floor — bit for bit, then times --bursts bursts of --reps launches between two events (a
tick figure: --bursts calls of --ticks ticks) and reports the median burst per launch.  --out writes the rows as JSON."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_common import B, FOV, THRESH, lidar_poses, write_rows  # noqa: E402
import support  # noqa: E402
from pyracecarsimulator_amd import maps, range_libc, workloads  # noqa: E402
from pyracecarsimulator_amd import racecar as RC  # noqa: E402

N, TD, MRX = 4096, 112, workloads.MAX_RANGE_PX
GROUPS = (1, 2, 4)
L, W = RC.DEFAULT_CAR["length"], RC.DEFAULT_CAR["width"]
FIGURES = [("scan_%s" % k, P) for P in GROUPS for k in ("cddt", "rm", "floor")] + \
          [("tick_%s" % k, P) for P in GROUPS for k in ("cddt", "rm")]


def race_states(g, dt, n_races, group, seed, spread=1.0):
    """tools/gpu_race_bench.py's line-ups: the cars of a race within ``spread`` m of a free centre."""
    rng = np.random.default_rng(seed)
    centres = maps.sample_free_poses(g, n_races, seed, 12.0, dt).astype(np.float64)
    s = np.zeros((n_races * group, 11))
    s[:, :3] = np.repeat(centres, group, 0)
    s[:, :2] += rng.uniform(-spread, spread, (n_races * group, 2))
    s[:, 2] = rng.uniform(-np.pi, np.pi, n_races * group)
    s[:, 3] = 2.0
    return s.reshape(n_races, group, 11)


def references(path):
    """The first two races of every P by the host statements: {"cddt_P", "rm_P", "floor_P"} -> float32 (2 P B,)."""
    import race_cddt_statement as S
    import race_statement as RS
    from oracle import np_statement as NS
    from oracle import oracle as O
    g = maps.load_colombia()
    dt = O.edt(g.occ)
    table = NS.CddtTable(g.occ, TD)
    out = {}
    for P in GROUPS:
        st = race_states(g, dt, N // P, P, 5 + P).reshape(N, 11)[:2 * P]
        poses = lidar_poses(st)
        cells = RS.outline_cells(st[:, :3], L, W, g.resolution, g.origin, g.rows, g.cols, O.sincosf)
        out["cddt_%d" % P] = S.fan(table, g.resolution, g.origin, MRX, poses, cells, P, FOV, B)
        out["floor_%d" % P] = NS.cddt_fan(table, g.resolution, g.origin, MRX, poses, FOV, B)
        rm = []
        for n in range(2 * P):
            om = O.OracleMap(RS.stamped(g.occ, RS.others(cells, P, n)), g.resolution, g.origin, MRX)
            rm.append(om.rm_fan(poses[n:n + 1], FOV, B, step_coeff=1.0)[0])
        out["rm_%d" % P] = np.concatenate(rm)
    np.savez(path, **out)


def figure(name, P, refs, reps, bursts, ticks):
    import torch
    kind, which = name.split("_")
    g = maps.load_colombia()
    omap = range_libc.PyOMap(g)
    dt = omap.distance_transform()
    m = range_libc.PyRayMarchingGPU(omap, MRX) if which == "rm" else range_libc.PyCDDTCast(omap, MRX, TD, races=True)
    st = race_states(g, dt, N // P, P, 5 + P)
    flat = st.reshape(N, 11)
    cars = torch.from_numpy(np.ascontiguousarray(flat[:, :3])).cuda()
    poses = torch.from_numpy(lidar_poses(flat)).cuda()
    out = torch.empty(N * B, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def scan():
        if which == "floor":
            m.calc_range_fan_device(poses.data_ptr(), N, FOV, B, out.data_ptr(), stream=stream)
        else:
            m.calc_range_fan_cars_device(poses.data_ptr(), cars.data_ptr(), N // P, P, FOV, B, out.data_ptr(), stream=stream)

    # the launch against the statement, on the first two races
    scan()
    torch.cuda.synchronize()
    want = refs["%s_%d" % (which, P)]
    got = out[:want.size].cpu().numpy()
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    if bad:
        raise SystemExit("%s P=%d: %d of %d checked rays differ from the statement" % (name, P, bad, want.size))
    times = []
    if kind == "scan":
        for _ in range(3):
            scan()
        torch.cuda.synchronize()
        for _ in range(bursts):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                scan()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) * 1e3 / reps)
    else:
        import time
        fg, cb, edge = support.followgap(), RC.CarBatch(), support.edge(B)
        cb.race_followgap(m, fg, st, 5, 2.0, FOV, B, edge, THRESH)
        for _ in range(bursts):
            t0 = time.perf_counter()
            cb.race_followgap(m, fg, st, ticks, 2.0, FOV, B, edge, THRESH)
            times.append((time.perf_counter() - t0) * 1e6 / ticks)
    return dict(figure=name, group=P, cars=N, beams=B, theta_disc=TD, us=float(np.median(times)),
                us_min=float(np.min(times)), us_max=float(np.max(times)), checked_rays=int(want.size),
                device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bursts", type=int, default=9)
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--figure", default=None, help="(child) NAME:P")
    ap.add_argument("--refs", default=None, help="(child) the parent's reference file")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.figure:
        name, P = args.figure.split(":")
        print(json.dumps(figure(name, int(P), np.load(args.refs), args.reps, args.bursts, args.ticks)), flush=True)
        return
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        refs = os.path.join(tmp, "refs.npz")
        references(refs)
        for name, P in FIGURES:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--figure", "%s:%d" % (name, P), "--refs", refs,
                                "--reps", str(args.reps), "--bursts", str(args.bursts), "--ticks", str(args.ticks)],
                               capture_output=True, text=True, timeout=300)
            if r.returncode != 0:                  # (a child that failed ends the run: nothing more is started)
                raise SystemExit("%s P=%d failed (%d): %s" % (name, P, r.returncode, (r.stderr or r.stdout)[-800:]))
            rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print("%-10s P=%d  %8.1f us  (min %.1f max %.1f; %d rays checked)"
                  % (name, P, rows[-1]["us"], rows[-1]["us_min"], rows[-1]["us_max"], rows[-1]["checked_rays"]), flush=True)
    by = {(r["figure"], r["group"]): r["us"] for r in rows}
    for P in GROUPS:
        print("P=%d  CDDT race scan %.1f us = %.2fx the floor, %.2fx the RMGPU race scan;  tick %.1f us against %.1f us"
              % (P, by[("scan_cddt", P)], by[("scan_cddt", P)] / by[("scan_floor", P)],
                 by[("scan_cddt", P)] / by[("scan_rm", P)], by[("tick_cddt", P)], by[("tick_rm", P)]), flush=True)
    if args.out:
        write_rows(args.out, "gpu_race_cddt_bench", rows)


if __name__ == "__main__":
    main()
