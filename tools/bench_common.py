"""What the closed-loop bench tools share: the host clock around a call, the world every tool drives in, the host-composed
drive tick and the --out writer.  The fixed values and small builders are those of the tests (tests/support.py)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import support  # noqa: E402
from support import FOV, THRESH, lidar_poses  # noqa: E402
from pyracecarsimulator_amd import maps, range_libc, workloads, racecar as RC  # noqa: E402

B = 1081


def timed(fn, reps):
    fn()                                                         # warm-up (tables, launch contexts, code objects)
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


def world(map_name):
    """(gmap, omap, distance transform, RMGPU method, FollowGap, CarBatch, edge table at B beams) on cfg2's 2049^2 maze
    or colombia."""
    g = workloads.cfg2().gmap if map_name == "cfg2" else maps.load_colombia()
    omap = range_libc.PyOMap(g)
    dt = omap.distance_transform()
    m = range_libc.PyRayMarchingGPU(omap, workloads.MAX_RANGE_PX)
    return g, omap, dt, m, support.followgap(), RC.CarBatch(), support.edge(B)


def free_starts(g, dt, n):
    """n cars at rest on free poses six cells from a wall (the seed every tool draws with)."""
    states = np.zeros((n, 11))
    states[:, :3] = maps.sample_free_poses(g, n, 17, 6.0, dt)
    return states


def composed_drive(cars, m, steer_of, states, T, edge, speed):
    """The closed loop composed on the host, the way a caller of the public calls writes it: rollout(n_steps=1) of the
    live cars, lidar poses in numpy, calc_range_fan to the host, Car::isCrashed in numpy (vectorised), then
    ``steer_of(ranges of the cars that go on)``.  Returns the crash ticks."""
    R = states.shape[0]
    cur, steer = states.copy(), np.zeros(R)
    first = np.full(R, -(T + 1), np.int32)
    alive = np.ones(R, bool)
    for t in range(T):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        _, out, _ = cars.rollout(cur[idx], np.stack([np.full(idx.size, speed), steer[idx]], -1)[:, None, :],
                                 n_steps=1, action_every=1)
        cur[idx] = out
        ranges = np.empty(idx.size * B, np.float32)
        m.calc_range_fan(lidar_poses(out), ranges, FOV, B)
        ranges = ranges.reshape(idx.size, B)
        crashed = ((ranges.astype(np.float64) - edge) < THRESH).any(1)
        first[idx[crashed]] = t
        alive[idx[crashed]] = False
        go = idx[~crashed]
        if go.size:
            steer[go] = steer_of(np.ascontiguousarray(ranges[~crashed]))
    return first


def scan_floor(m, states, T):
    """The scan floor of a closed loop: T serial calc_range_fan_device launches of the start poses on device buffers."""
    import torch
    R = states.shape[0]
    st = torch.cuda.Stream()
    d_poses = torch.from_numpy(lidar_poses(states)).cuda()
    d_out = torch.empty(R * B, dtype=torch.float32, device="cuda")

    def floor():
        for _ in range(T):
            m.calc_range_fan_device(d_poses.data_ptr(), R, FOV, B, d_out.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
    return floor


def write_rows(path, tool, rows, **head):
    """--out: {"tool": tool, **head, "rows": rows} (tool None: left out)."""
    doc = dict(tool=tool) if tool else {}
    doc.update(head, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
