"""Host wall time per call of the multi-device entry points through a three-context handle (device 0 named three times,
multi_min_poses = 64: every call is cut over three worker-thread blocks), cfg2 map, 1081 beams — what the block
scheduler itself costs.  One leg per process; A/B two builds by swapping pyracecarsimulator_amd/libscan_amd.so between legs.

    python tools/gpu_multi_host_times.py <label>                 one leg: "<label> <shape> <median us>" per line
    python tools/gpu_multi_host_times.py --table A B NEW         fold three legs' outputs (files) into the table
"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CALLS, WARMUP = 200, 20


def median_us(fn):
    for _ in range(WARMUP):
        fn()
    ts = []
    for _ in range(CALLS):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e6


def leg(label):
    import torch
    from pyracecarsimulator_amd import _lib, range_libc, workloads
    from pyracecarsimulator_amd import racecar as RC
    w = workloads.cfg2()
    B = w.num_rays
    multi = range_libc.PyOMap(w.gmap, device=[0, 0, 0])
    mm = range_libc.PyRayMarchingGPU(multi, w.max_range_px)
    mm.set_option("multi_min_poses", 64)
    rows = []
    for n in (200, 1024, 4096):
        poses = workloads.make_poses(w, n_poses=n)
        out = _lib.pinned_zeros(n * B, np.float32)
        rows.append(("calc_range_fan %d poses" % n, median_us(lambda: mm.calc_range_fan(poses, out, w.fov, B))))
    R, L = 64, workloads.ROLLOUT_STEPS
    edge = RC.edge_distances(B, -w.fov / 2.0, w.fov / B, 0.275, RC.DEFAULT_CAR["width"], RC.DEFAULT_CAR["wb"])
    states, actions = workloads.rollout_inputs(w, R, 3)
    cm = RC.CarBatch(device=[0, 0, 0])
    rposes = cm.rollout(states, actions)[0].reshape(-1, 3)
    rows.append(("check_collision_groups %d x %d" % (R, L),
                 median_us(lambda: mm.check_collision_groups(rposes, L, w.fov, B, edge, 0.001))))
    rows.append(("rollout_check %d x %d" % (R, L),
                 median_us(lambda: cm.rollout_check(mm, states, actions, w.fov, B, edge, 0.001))))
    n = 4096
    poses = workloads.make_poses(w, n_poses=n)
    d_out = torch.empty(n * B, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rows.append(("calc_range_fan_multi_device %d poses, consumer 2" % n,
                 median_us(lambda: mm.calc_range_fan_multi_device(poses, d_out.data_ptr(), w.fov, B, consumer=2))))
    for name, us in rows:
        print("%s | %s | %.1f" % (label, name, us), flush=True)


def table(paths):
    legs = []
    for p in paths:
        legs.append({ln.split(" | ")[1]: float(ln.split(" | ")[2]) for ln in open(p) if ln.count(" | ") == 2})
    a, b, new = legs
    print("median host wall time per synchronous call, us (%d calls after %d warm-up; each leg a fresh process)" % (CALLS, WARMUP))
    print("%-52s %10s %10s %10s   %s" % ("call (3 contexts of device 0, multi_min_poses 64)", "parent A", "parent B", "new", "new - slower parent <= |A - B| ?"))
    ok = True
    for name in a:
        spread, over = abs(a[name] - b[name]), new[name] - max(a[name], b[name])
        ok &= over <= spread
        print("%-52s %10.1f %10.1f %10.1f   %+.1f vs %.1f: %s" % (name, a[name], b[name], new[name], over, spread, "ok" if over <= spread else "SLOWER"))
    return 0 if ok else 1


if __name__ == "__main__":
    if sys.argv[1] == "--table":
        sys.exit(table(sys.argv[2:5]))
    leg(sys.argv[1])
