"""What the tests and the bench tools share: the fixed values of the reference's set-up, the builders of the objects
every closed-loop case starts from, and the two bit-level comparisons.  No tests and no marks live here."""
import numpy as np

from pyracecarsimulator_amd import maps, range_libc, workloads
from pyracecarsimulator_amd import racecar as RC
from pyracecarsimulator_amd.followgap import PyFollowGap

FOV = workloads.SCAN_FOV                      # params.yaml scan_field_of_view
THRESH, D_BASE = 0.001, 0.275                 # ttc_thresh, scan_distance_to_base_link
MAX_STEER = RC.DEFAULT_CAR["max_steer_ang"]
FOLLOWGAP_ARGS = (10, 15.0, MAX_STEER, 0.004)  # window, max distance, max angle, angle increment (simple_driver.py)


def edge(num_rays, fov=FOV):
    """The default car's outline table at ``num_rays`` beams over ``fov``."""
    return RC.edge_distances(num_rays, -fov / 2, fov / num_rays, D_BASE, RC.DEFAULT_CAR["width"], RC.DEFAULT_CAR["wb"])


def oracle_edge(oracle_mod, num_rays, fov=FOV):
    """The same table by the oracle's restatement (tests/test_host.py holds the two equal)."""
    return oracle_mod.edge_distances(num_rays, -fov / 2, fov / num_rays, D_BASE, RC.DEFAULT_CAR["width"],
                                     RC.DEFAULT_CAR["wb"])


def followgap(max_angle=MAX_STEER, inc=FOLLOWGAP_ARGS[3], **kw):
    """simple_driver.py's FollowGap (window 10, 15 m); ``kw``: device."""
    return PyFollowGap(FOLLOWGAP_ARGS[0], FOLLOWGAP_ARGS[1], max_angle, inc, **kw)


def starts(g, dt, n, seed, clear_px, speed_hi=7.0):
    """(states (n, 11), target speeds (n,)): free poses ``clear_px`` cells from a wall, under way at a part of the target."""
    rng = np.random.default_rng(seed)
    states = np.zeros((n, 11))
    states[:, :3] = maps.sample_free_poses(g, n, seed, clear_px, dt)
    speeds = rng.uniform(1.0, speed_hi, n)
    states[:, 3] = rng.uniform(0.0, 1.0, n) * speeds
    return states, speeds


def lidar_poses(states, d=D_BASE):
    """Car::getScanPose in f64 on (..., >= 3) rows of (x, y, theta, ...), rounded to the f32 lidar pose."""
    s = np.asarray(states, np.float64)
    x, y, th = s[..., 0], s[..., 1], s[..., 2]
    return np.stack([x + d * np.cos(th), y + d * np.sin(th), th], -1).astype(np.float32)


def five_methods(omap, mrx, theta=112):
    """(name, handle, scan noise std) of the five range methods; noise on for RMGPU alone."""
    return [("RM", range_libc.PyRayMarching(omap, mrx), 0.0),
            ("RMGPU", range_libc.PyRayMarchingGPU(omap, mrx), 0.05),
            ("CDDT", range_libc.PyCDDTCast(omap, mrx, theta), 0.0),
            ("GiantLUT", range_libc.PyGiantLUTCast(omap, mrx, theta), 0.0),
            ("Bresenham", range_libc.PyBresenhamsLine(omap, mrx), 0.0)]


def within_one_ulp(a, b):
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    return bool((d <= np.spacing(np.maximum(np.abs(a), np.abs(b)))).all())


def same_bits(a, b):
    """Same dtype, same shape, same bytes."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
