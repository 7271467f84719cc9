"""``range_libc``-compatible surface for the scan path, backed by libscan_amd.so.

Mirrors the objects the reference builds and calls (same names, argument meaning
and in-place/None-returning behaviour):

* ``PyOMap(map_msg)``                      scripts/ros_interface.py:210, scripts/mcts_driver.py:278
* ``PyRayMarching(omap, max_range_px)``    scripts/scan_simulator.py:72-73
* ``PyRayMarchingGPU(omap, max_range_px)`` scripts/scan_simulator.py:74-76
* ``PyCDDTCast(omap, max_range_px, theta_disc)``   scripts/two_player/scan.py:46
* ``obj.calc_range_many(ins, outs, fov, num_rays)`` scripts/scan_simulator.py:103-106,130-133
* ``obj.calc_range_many(ins, outs)``                scripts/two_player/scan.py:69-70

plus range_libc's remaining casters (``PyBresenhamsLine``, ``PyGiantLUTCast``) and its particle-filter calls
(``calc_range_repeat_angles``, ``set_sensor_model``, ``eval_sensor_model``,
``calc_range_repeat_angles_eval_sensor_model``: what a particle filter — the odometry source
scripts/mcts_driver.py:62 keeps commented out — calls per update).
Array contract: ``ins`` float32 C-contiguous (n,3), ``outs`` float32
C-contiguous (n,); anything else raises ``ValueError`` like the Cython
``np.ndarray[float, ndim=2, mode="c"]`` signature does.

Usage as a drop-in: ``from pyracecarsimulator_amd import range_libc`` (or put
``sys.modules["range_libc"] = pyracecarsimulator_amd.range_libc`` before importing
the reference's scan_simulator).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib

__all__ = ["PyOMap", "PyRayMarching", "PyRayMarchingGPU", "PyCDDTCast", "PyBresenhamsLine",
           "PyGiantLUTCast", "USE_CUDA", "SHOULD_USE_CUDA"]

#: range_libc exports these flags; the AMD build always has its device path.
USE_CUDA = True
SHOULD_USE_CUDA = True


def _yaw_from_quaternion(q) -> float:
    """yaw of tf.transformations.euler_from_quaternion (scripts/ros_interface.py:212-216)."""
    x, y, z, w = (float(q.x), float(q.y), float(q.z), float(q.w))
    return math.atan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z))


def stamp_indices(flat_idx, n_cells):
    """The cells ``PyOMap.stamp_cells`` stamps: the indices ``0 <= idx < n_cells`` of ``flat_idx`` as C-contiguous
    int32, compared on their original integer value (an int64 ``2**32 + 5`` is skipped, not wrapped to cell 5).
    An empty input of any dtype gives no cells; a non-empty input that is not integer raises ``TypeError``."""
    a = np.asarray(flat_idx).ravel()
    if a.size == 0:
        return np.zeros(0, dtype=np.int32)
    if not np.issubdtype(a.dtype, np.integer):
        raise TypeError("stamp_cells: cell indices must be integers, got dtype %s" % a.dtype)
    return np.ascontiguousarray(a[(a >= 0) & (a < n_cells)], dtype=np.int32)


class PyOMap(_lib.Handle):
    """Occupancy grid + world transform, resident on one MI355X.

    Accepts what the reference passes — a ``nav_msgs/OccupancyGrid``-like object with
    ``.info.{width,height,resolution,origin}`` and row-major ``.data`` (occupied where
    ``data > 10``) — or, since ROS messages do not exist on the GPU
    box, a NumPy ``(H, W)`` array (nonzero = occupied) with ``resolution`` and
    ``origin=(x, y, yaw)``, or a ``maps.GridMap``.

    ``device`` may be a LIST of device indices (``rl_map_create_multi``): the map then lives on every
    one of them, and the range methods created on it cut each host-pointer batch (``calc_range_many``,
    ``calc_range_fan``, ``check_collision_*``) into contiguous pose blocks, one per device, inside the
    one calling process — the reference's ``scanMany`` / ``checkCollisionMany`` callers
    (scripts/scan_simulator.py:113-135, scripts/mcts.py:237) get all the GPUs of the node unchanged.
    """

    _destroy = "rl_map_destroy"

    def __init__(self, arg1, arg2=None, resolution=None, origin=None, device=0):
        occ, res, org = self._ingest(arg1, arg2, resolution, origin)
        self.occ = np.ascontiguousarray(occ, dtype=np.uint8)
        if self.occ.ndim != 2:
            raise ValueError("PyOMap: occupancy must be a 2-D array")
        self.height, self.width = (int(v) for v in self.occ.shape)
        self.resolution = float(res)
        self.origin = tuple(float(v) for v in org)
        self._h = C.c_void_p()
        if isinstance(device, (list, tuple)):
            self.devices = [int(d) for d in device]
            if not self.devices:
                raise ValueError("PyOMap: empty device list")
            self.device = self.devices[0]
            _lib.call("rl_map_create_multi", self.occ, self.height, self.width, self.resolution, *self.origin[:3],
                      np.array(self.devices, dtype=np.intc), len(self.devices), self._h)
            return
        self.device = int(device)
        self.devices = [self.device]
        _lib.call("rl_map_create", self.occ, self.height, self.width, self.resolution, *self.origin[:3], self.device,
                  self._h)

    @staticmethod
    def _ingest(arg1, arg2, resolution, origin):
        if hasattr(arg1, "info") and hasattr(arg1, "data"):          # OccupancyGrid duck type
            info = arg1.info
            w, h = int(info.width), int(info.height)
            data = np.asarray(arg1.data).reshape(h, w)
            pos, ori = info.origin.position, info.origin.orientation
            return (data > 10), float(info.resolution), (pos.x, pos.y, _yaw_from_quaternion(ori))
        if hasattr(arg1, "occ") and hasattr(arg1, "resolution"):     # maps.GridMap
            return arg1.occ != 0, arg1.resolution, arg1.origin
        arr = np.asarray(arg1)
        if arr.ndim == 2:
            if resolution is None and arg2 is not None and not isinstance(arg2, (tuple, list)):
                resolution = arg2
            return arr != 0, (1.0 if resolution is None else resolution), \
                ((0.0, 0.0, 0.0) if origin is None else origin)
        raise TypeError("PyOMap: expected an OccupancyGrid-like message, a GridMap or a 2-D array")

    # -- range_libc.PyOMap helpers ------------------------------------------
    def isOccupied(self, x, y):
        return bool(self.occ[int(x), int(y)])

    def update(self, occ):
        """Replace the grid (same shape) and rebuild the device tables — the per-scan
        rebuild of scripts/two_player/rcs_two_player.py:110-121."""
        occ = np.ascontiguousarray(np.asarray(occ) != 0, dtype=np.uint8)
        if occ.shape != self.occ.shape:
            raise ValueError("PyOMap.update: shape mismatch")
        self.occ = occ
        self._base_occ = None
        _lib.call("rl_map_update", self, occ)

    def stamp_cells(self, flat_idx, value=255):
        """The two-player tick without re-uploading the grid (rl_map_stamp_cells): the occupancy becomes the BASE map
        (as constructed / last ``update``d) with the cells ``flat_idx`` (row * width + col) set, tables rebuilt on the
        device.  Each stamp replaces the previous one; an empty list restores the base map.

        Indices are filtered on their integer value before they are narrowed to int32: cells with
        ``0 <= idx < rows * cols`` are stamped, every other index is skipped.  For ``idx >= rows * cols`` that is the
        reference's guard (scripts/two_player/rcs_two_player.py:113).  Negative indices are a deliberate divergence:
        the reference's guard lets them through and its numpy map wraps ``-size <= idx < 0`` to a cell from the end;
        here they are skipped.  A non-empty input that is not an integer array raises ``TypeError``."""
        idx = stamp_indices(flat_idx, self.occ.size)
        if getattr(self, "_base_occ", None) is None:
            self._base_occ = self.occ.copy()
        _lib.call("rl_map_stamp_cells", self, idx, idx.size, int(value) & 0xff)
        occ = self._base_occ.copy()
        occ.reshape(-1)[idx] = 1 if (int(value) & 0xff) else 0
        self.occ = occ

    def distance_transform(self):
        """float32 (H, W) exact EDT in cells as built on the device (test hook)."""
        out = np.empty((self.height, self.width), dtype=np.float32)
        _lib.call("rl_map_get_dt", self, out)
        return out


def _check_ins_outs(ins, outs):
    if not isinstance(ins, np.ndarray) or not isinstance(outs, np.ndarray):
        raise TypeError("calc_range_many: ins/outs must be numpy arrays")
    if ins.dtype != np.float32 or outs.dtype != np.float32:
        raise ValueError("Buffer dtype mismatch, expected 'float'")
    if ins.ndim != 2 or outs.ndim != 1:
        raise ValueError("Buffer has wrong number of dimensions (expected 2 and 1)")
    if not ins.flags.c_contiguous or not outs.flags.c_contiguous:
        raise ValueError("ndarray is not C-contiguous")
    if ins.shape[1] != 3:
        raise ValueError("ins must have shape (n, 3)")
    if outs.shape[0] < ins.shape[0]:
        raise ValueError("outs is shorter than ins")


def _check_ranges_out(ranges, n):
    """An optional ranges buffer the C side will fill with n float32 values."""
    if ranges is None:
        return
    if not isinstance(ranges, np.ndarray) or ranges.dtype != np.float32 or not ranges.flags.c_contiguous \
            or ranges.size < n:
        raise ValueError("ranges must be a C-contiguous float32 array with n_poses*num_rays elements")


def _check_aux_outs(hit_cells, steps, n, shape, exact=False):
    """The optional diagnostics of an n-ray scan: ``hit_cells`` int32 with 2 n elements, ``steps`` uint16 with n, both
    C-contiguous arrays.  ``exact``: the sizes must match; otherwise a larger buffer passes.  ``shape`` names n in the
    message."""
    for name, a, dtype, size in (("hit_cells", hit_cells, np.int32, 2 * n), ("steps", steps, np.uint16, n)):
        if a is None:
            continue
        if not isinstance(a, np.ndarray) or a.dtype != dtype or not a.flags.c_contiguous \
                or (a.size != size if exact else a.size < size):
            raise ValueError("%s must be C-contiguous %s (%s%s)" % (name, np.dtype(dtype).name, shape,
                                                                    ", 2" if name == "hit_cells" else ","))


def _prep_crash(poses, edge_distances, num_rays, group=None):
    """The crash-test wrappers' inputs: (poses float32 (n, 3), edge float64) as C-contiguous arrays, checked."""
    poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 3)
    if group is not None and poses.shape[0] % group:
        raise ValueError("number of poses is not a multiple of the group size")
    edge = np.ascontiguousarray(edge_distances, dtype=np.float64)
    if edge.size < num_rays:
        raise ValueError("edge_distances needs num_rays entries")
    return poses, edge


def _check_f32_vector(name, a, n=None):
    """A C-contiguous float32 1-D array (of n elements when n is given), as the Cython signatures take them."""
    if not isinstance(a, np.ndarray):
        raise TypeError("%s must be a numpy array" % name)
    if a.dtype != np.float32:
        raise ValueError("Buffer dtype mismatch, expected 'float' (%s)" % name)
    if a.ndim != 1:
        raise ValueError("Buffer has wrong number of dimensions (expected 1) (%s)" % name)
    if not a.flags.c_contiguous:
        raise ValueError("ndarray is not C-contiguous (%s)" % name)
    if n is not None and a.shape[0] != n:
        raise ValueError("%s must have %d elements, got %d" % (name, n, a.shape[0]))


def _check_particles(ins):
    if not isinstance(ins, np.ndarray):
        raise TypeError("ins must be a numpy array")
    if ins.dtype != np.float32:
        raise ValueError("Buffer dtype mismatch, expected 'float' (ins)")
    if ins.ndim != 2 or ins.shape[1] != 3:
        raise ValueError("ins must have shape (n, 3)")
    if not ins.flags.c_contiguous:
        raise ValueError("ndarray is not C-contiguous (ins)")


def _check_weights(weights, n):
    if not isinstance(weights, np.ndarray):
        raise TypeError("weights must be a numpy array")
    if weights.dtype != np.float64:
        raise ValueError("Buffer dtype mismatch, expected 'double' (weights)")
    if weights.ndim != 1 or not weights.flags.c_contiguous:
        raise ValueError("weights must be a C-contiguous 1-D array")
    if weights.shape[0] != n:
        raise ValueError("weights must have %d elements, got %d" % (n, weights.shape[0]))


class _RangeMethod(_lib.Handle):
    KIND = None
    _destroy = "rl_method_destroy"

    def __init__(self, omap, max_range_px, theta_disc=0):
        if not isinstance(omap, PyOMap):
            raise TypeError("expected a PyOMap")
        self.omap = omap                         # keep the map alive
        self.max_range_px = float(max_range_px)
        self.theta_disc = int(theta_disc)
        self._h = C.c_void_p()
        _lib.call("rl_method_create", omap, self.KIND, self.max_range_px, self.theta_disc, self._h)
        self._fan_raw = _lib.raw("rl_calc_range_many_fan")
        self._fan_dense_raw = _lib.raw("rl_calc_range_fan")

    # -- the reference's entry point ----------------------------------------
    def calc_range_many(self, ins, outs, fov=None, num_rays=None):
        """In-place, returns None.  2 args: one (x, y, theta) row per ray
        (scripts/two_player/scan.py:69-70).  4 args: the fork's fan form — pose p in row
        ``p*num_rays``, result ``outs[p*num_rays + j]`` (scripts/scan_simulator.py:103-106,
        130-133)."""
        _check_ins_outs(ins, outs)
        if fov is None and num_rays is None:
            _lib.call("rl_calc_range_many", self, ins, outs, ins.shape[0])
        elif fov is None or num_rays is None:
            raise TypeError("calc_range_many takes (ins, outs) or (ins, outs, fov, num_rays)")
        else:
            _lib.call("rl_calc_range_many_fan", self, ins, outs, ins.shape[0], fov, num_rays)
        return None

    def _fan_rows_ptr(self, ins_addr, outs_addr, n_rows, fov, num_rays):
        """4-argument calc_range_many on buffers whose addresses the caller keeps (ScanSimulator2D's
        cached vectors): same C entry point, no per-call ctypes pointer objects, no re-validation."""
        rc = self._fan_raw(self._h, ins_addr, outs_addr, n_rows, fov, num_rays)
        if rc:
            _lib.check(rc)

    def calc_range(self, x, y, heading):
        """Scalar query in world coordinates (upstream's RayMarchingGPU does not support
        this and returns -1; here it is one 1-ray launch)."""
        ins = np.array([[x, y, heading]], dtype=np.float32)
        outs = np.zeros(1, dtype=np.float32)
        self.calc_range_many(ins, outs)
        return float(outs[0])

    # -- dense fast paths -------------------------------------
    def calc_range_fan(self, poses, outs, fov, num_rays, hit_cells=None, steps=None):
        """poses float32 (P,3) -> outs float32 (P*num_rays,), optional diagnostics."""
        poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 3)
        n = poses.shape[0] * int(num_rays)
        if outs.dtype != np.float32 or not outs.flags.c_contiguous or outs.size < n:
            raise ValueError("outs must be C-contiguous float32 with P*num_rays elements")
        _check_aux_outs(hit_cells, steps, n, "P*num_rays")
        _lib.call("rl_calc_range_fan", self, poses, poses.shape[0], fov, num_rays, outs, hit_cells, steps)
        return None

    def calc_range_fan_cars(self, poses, car_poses, group, fov, num_rays, outs=None, length=0.4064, width=0.2032,
                            hit_cells=None, steps=None):
        """The scan of N = n_groups * group poses in races of ``group`` cars (``rl_calc_range_fan_cars``): pose i of
        group g is scanned on the grid with the outlines (length x width, the reference car by default) of the OTHER
        cars of group g stamped, car k at ``car_poses`` row g * group + k.  poses float32 (N, 3) lidar poses; car_poses
        float64 (N, 3) car states (x, y, theta).  RM and RMGPU, and CDDT with ``races=True`` (ranges only: the others'
        cells join the static buckets at query time, include/scanlib.h); GiantLUT and Bresenham are refused.  Returns
        outs float32 (N * num_rays,)."""
        poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 3)
        cars = np.ascontiguousarray(car_poses, dtype=np.float64).reshape(-1, 3)
        group = int(group)
        if cars.shape[0] != poses.shape[0]:
            raise ValueError("car_poses needs one (x, y, theta) row per pose")
        if group < 1 or poses.shape[0] % group:
            raise ValueError("the number of poses must be a multiple of group >= 1")
        n = poses.shape[0] * int(num_rays)
        if outs is None:
            outs = np.empty(n, dtype=np.float32)
        if outs.dtype != np.float32 or not outs.flags.c_contiguous or outs.size < n:
            raise ValueError("outs must be C-contiguous float32 with N*num_rays elements")
        _check_aux_outs(hit_cells, steps, n, "N*num_rays")
        _lib.call("rl_calc_range_fan_cars", self, poses, cars, poses.shape[0] // group, group, length, width, fov,
                  num_rays, outs, hit_cells, steps)
        return outs

    def calc_range_fan_cars_device(self, d_poses_ptr, d_cars_ptr, n_groups, group, fov, num_rays, d_outs_ptr,
                                   length=0.4064, width=0.2032, d_hits_ptr=0, d_steps_ptr=0, stream=0):
        """``calc_range_fan_cars`` on device pointers (ints, e.g. torch ``tensor.data_ptr()``): asynchronous."""
        _lib.call("rl_calc_range_fan_cars_device", self, d_poses_ptr, d_cars_ptr, n_groups, group, length, width, fov,
                  num_rays, d_outs_ptr, d_hits_ptr, d_steps_ptr, stream)

    def calc_range_fan_device(self, d_poses_ptr, n_poses, fov, num_rays, d_outs_ptr,
                              d_hits_ptr=0, d_steps_ptr=0, stream=0):
        """Asynchronous launch on device pointers (ints), e.g. torch ``tensor.data_ptr()``."""
        _lib.call("rl_calc_range_fan_device", self, d_poses_ptr, n_poses, fov, num_rays, d_outs_ptr, d_hits_ptr,
                  d_steps_ptr, stream)

    def calc_range_many_device(self, d_ins_ptr, d_outs_ptr, n, stream=0):
        _lib.call("rl_calc_range_many_device", self, d_ins_ptr, d_outs_ptr, n, stream)

    # -- particle-filter weights (range_libc's Monte-Carlo localisation calls) -------
    def calc_range_repeat_angles(self, ins, angles, outs, hit_cells=None, steps=None):
        """In-place, returns None: every particle ``ins[p]`` (x, y, theta) casts the same ``angles`` (float32 (A,)),
        ray j of particle p at ``theta_p + angles[j]`` lands in ``outs[p*A + j]`` (rl_calc_range_repeat_angles)."""
        _check_particles(ins)
        _check_f32_vector("angles", angles)
        n = ins.shape[0] * angles.shape[0]
        _check_f32_vector("outs", outs, n)
        _check_aux_outs(hit_cells, steps, n, "P*A", exact=True)
        _lib.call("rl_calc_range_repeat_angles", self, ins, ins.shape[0], angles, angles.shape[0], outs, hit_cells,
                  steps)
        return None

    def set_sensor_model(self, table):
        """The sensor model: a square float64 2-D table, row = observed bin, column = expected bin
        (rl_set_sensor_model; a later call replaces it)."""
        if not isinstance(table, np.ndarray):
            raise TypeError("table must be a numpy array")
        if table.dtype != np.float64 or table.ndim != 2 or table.shape[0] != table.shape[1]:
            raise ValueError("the sensor model must be a square 2-D float64 array")
        _lib.call("rl_set_sensor_model", self, np.ascontiguousarray(table), table.shape[0])
        return None

    def eval_sensor_model(self, obs, ranges, outs, num_rays, num_particles):
        """``outs[p]`` (float64) = the ascending product over j of ``table[bin(obs[j]), bin(ranges[p*num_rays + j])]``
        (rl_eval_sensor_model).  In-place, returns None."""
        num_rays, num_particles = int(num_rays), int(num_particles)
        _check_f32_vector("obs", obs, num_rays)
        _check_f32_vector("ranges", ranges, num_rays * num_particles)
        _check_weights(outs, num_particles)
        _lib.call("rl_eval_sensor_model", self, obs, ranges, num_rays, num_particles, outs)
        return None

    def calc_range_repeat_angles_eval_sensor_model(self, ins, angles, obs, weights):
        """``calc_range_repeat_angles`` and ``eval_sensor_model`` in one call; the ranges stay on the device
        (rl_calc_range_repeat_angles_eval_sensor_model).  In-place on ``weights`` (float64 (P,)), returns None."""
        _check_particles(ins)
        _check_f32_vector("angles", angles)
        _check_f32_vector("obs", obs, angles.shape[0])
        _check_weights(weights, ins.shape[0])
        _lib.call("rl_calc_range_repeat_angles_eval_sensor_model", self, ins, ins.shape[0], angles, obs,
                  angles.shape[0], weights)
        return None

    def calc_range_repeat_angles_device(self, d_ins_ptr, n_particles, d_angles_ptr, n_angles, d_outs_ptr,
                                        d_hits_ptr=0, d_steps_ptr=0, stream=0):
        """``calc_range_repeat_angles`` on device pointers (ints, e.g. torch ``tensor.data_ptr()``): asynchronous."""
        _lib.call("rl_calc_range_repeat_angles_device", self, d_ins_ptr, n_particles, d_angles_ptr, n_angles,
                  d_outs_ptr, d_hits_ptr, d_steps_ptr, stream)

    def eval_sensor_model_device(self, d_obs_ptr, d_ranges_ptr, d_outs_ptr, num_rays, num_particles, stream=0):
        """``eval_sensor_model`` on device pointers: asynchronous."""
        _lib.call("rl_eval_sensor_model_device", self, d_obs_ptr, d_ranges_ptr, num_rays, num_particles, d_outs_ptr,
                  stream)

    def calc_range_repeat_angles_eval_sensor_model_device(self, d_ins_ptr, n_particles, d_angles_ptr, d_obs_ptr,
                                                          n_angles, d_weights_ptr, stream=0):
        """``calc_range_repeat_angles_eval_sensor_model`` on device pointers: asynchronous."""
        _lib.call("rl_calc_range_repeat_angles_eval_sensor_model_device", self, d_ins_ptr, n_particles, d_angles_ptr,
                  d_obs_ptr, n_angles, d_weights_ptr, stream)

    def check_collision_many(self, poses, fov, num_rays, edge_distances, crash_thresh,
                             ranges=None):
        """Scan + Car::isCrashed fused (racecar/src/racecar.cpp:305-328): index of the first
        crashed pose, else ``-(n_poses+1)``."""
        poses, edge = _prep_crash(poses, edge_distances, num_rays)
        _check_ranges_out(ranges, poses.shape[0] * int(num_rays))
        first = C.c_int(0)
        _lib.call("rl_check_collision_many", self, poses, poses.shape[0], fov, num_rays, edge, crash_thresh, first,
                  ranges)
        return int(first.value)

    def check_collision_groups(self, poses, group, fov, num_rays, edge_distances, crash_thresh,
                               ranges=None):
        """isCrashed per roll-out of a batch: ``poses`` holds consecutive roll-outs of ``group``
        poses; returns int32[n_groups] (first crashed pose inside each roll-out, else -(group+1))."""
        poses, edge = _prep_crash(poses, edge_distances, num_rays, group)
        n_groups = poses.shape[0] // group
        _check_ranges_out(ranges, poses.shape[0] * int(num_rays))
        first = np.zeros(n_groups, dtype=np.int32)
        _lib.call("rl_check_collision_groups", self, poses, n_groups, group, fov, num_rays, edge, crash_thresh, first,
                  ranges)
        return first

    def check_collision_groups_device(self, d_poses_ptr, n_groups, group, fov, num_rays, d_edge_ptr,
                                      crash_thresh, d_first_ptr, d_ranges_ptr=0, stream=0):
        """Asynchronous grouped scan + crash test on device pointers (ints)."""
        _lib.call("rl_check_collision_groups_device", self, d_poses_ptr, n_groups, group, fov, num_rays, d_edge_ptr,
                  crash_thresh, d_first_ptr, d_ranges_ptr, stream)

    def calc_range_fan_multi_device(self, poses, d_outs_ptr, fov, num_rays, consumer=0, chunks=0):
        """Multi-device handle, results in DEVICE memory of replica ``consumer``'s GPU (rl_calc_range_fan_multi_device):
        every device marches its pose block into its own HBM and sends it to the consumer chunk by chunk
        (hipMemcpyPeerAsync: xGMI between peers) under the next chunk's march.  ``poses``: host array (n, 3);
        ``d_outs_ptr``: device address (int) of n * num_rays float32 on the consumer's device.  Synchronous."""
        poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 3)
        _lib.call("rl_calc_range_fan_multi_device", self, poses, poses.shape[0], fov, num_rays, consumer, d_outs_ptr,
                  chunks)

    def check_collision_groups_multi_device(self, poses, group, fov, num_rays, edge_distances, crash_thresh, d_first_ptr,
                                            consumer=0):
        """... the fused crash indices (int32 per roll-out of ``group`` poses) of every device's block, gathered in the
        consumer device's memory at ``d_first_ptr`` (rl_check_collision_groups_multi_device)."""
        poses, edge = _prep_crash(poses, edge_distances, num_rays, group)
        _lib.call("rl_check_collision_groups_multi_device", self, poses, poses.shape[0] // int(group), group, fov,
                  num_rays, edge, crash_thresh, consumer, d_first_ptr)

    @property
    def n_devices(self):
        """Devices behind this handle (> 1 for a method of a multi-device ``PyOMap``)."""
        return _lib.call("rl_method_n_devices", self)

    def replica(self, i):
        """The per-device method ``i`` of a multi-device handle as a borrowed object for the ``*_device``
        calls (device pointers belong to one device); the handle itself for a single-device method."""
        p = _lib.call("rl_method_replica", self, i)
        if not p:
            raise IndexError("replica %d out of range (%d devices)" % (i, self.n_devices))
        if p == self._h.value:
            return self
        r = object.__new__(type(self))
        r.__dict__.update(omap=self.omap, max_range_px=self.max_range_px, theta_disc=self.theta_disc,
                          _h=C.c_void_p(p), _fan_raw=self._fan_raw, _fan_dense_raw=self._fan_dense_raw,
                          _parent=self, _borrowed=True)          # (_parent keeps the owner alive)
        return r

    def set_noise(self, std, seed=0, ray_offset=0):
        _lib.call("rl_set_noise", self, std, seed, ray_offset)

    def set_option(self, name, value):
        _lib.call("rl_method_set_option", self, name, value)

    def get_info(self, name):
        v = C.c_int64(0)
        _lib.call("rl_method_get_info", self, name, v)
        return int(v.value)

    def plan_fan(self, n_poses, num_rays, aux=False, crash=False):
        """What a fan call of this shape would launch with the handle's current options
        (kernel with template arguments, grid, LDS, binning pass): rl_method_plan_fan."""
        pl = _lib.LaunchPlan()
        _lib.call("rl_method_plan_fan", self, n_poses, num_rays, bool(aux), bool(crash), pl)
        return pl.as_dict()

    def last_plan(self):
        """The plan the last fan launch of this handle executed (rl_method_last_plan)."""
        pl = _lib.LaunchPlan()
        _lib.call("rl_method_last_plan", self, pl)
        return pl.as_dict()

    def debug_stamps(self):
        """(n_waves, 4) uint64 diagnostics of the last stream-kernel launch (option debug_stamps)."""
        n = self.get_info("last_grid") * 4 * 4
        buf = np.zeros(max(n, 4), dtype=np.uint64)
        got = _lib.call("rl_debug_read_stamps", self, buf, n)
        if got < 0:
            _lib.check(got)
        return buf[:got].reshape(-1, 4)

    def last_kernel_ms(self):
        """Device time of the last launch; needs ``set_option("timing", 1)`` before that launch."""
        ms = C.c_float(0)
        _lib.call("rl_last_kernel_ms", self, ms)
        return float(ms.value)


class PyRayMarching(_RangeMethod):
    """range_libc.PyRayMarching(omap, mrx) — step coefficient 0.999 (CPU RayMarching)."""
    KIND = _lib.RL_RM


class PyRayMarchingGPU(_RangeMethod):
    """range_libc.PyRayMarchingGPU(omap, mrx) — step coefficient 1.0 (kernels.cu)."""
    KIND = _lib.RL_RM_GPU


class PyBresenhamsLine(_RangeMethod):
    """range_libc.PyBresenhamsLine(omap, mrx)."""
    KIND = _lib.RL_BRESENHAM


class PyCDDTCast(_RangeMethod):
    """range_libc.PyCDDTCast(omap, mrx, theta_disc) (scripts/two_player/scan.py:46).

    ``races=True`` lets the handle run batched races (option ``race_cddt``, include/scanlib.h "batched multi-car races"):
    ``calc_range_fan_cars``, ``CarBatch.race_*`` and ``RaceEnv`` then query the static table with the other cars'
    outline cells folded into each bucket, instead of refusing the kind.  It equals stamping the others, rebuilding and
    scanning wherever every outline cell is an edge cell of the stamped grid and no static edge cell stops being one."""
    KIND = _lib.RL_CDDT

    def __init__(self, omap, max_range_px, theta_disc, races=False):
        super().__init__(omap, max_range_px, theta_disc)
        if races:
            self.set_option("race_cddt", 1)

    def prune(self, max_range=None):   # upstream API; pruning is a no-op for exactness
        return None


class PyGiantLUTCast(_RangeMethod):
    """range_libc.PyGiantLUTCast(omap, mrx, theta_disc): uint16 table [row][col][theta_bin] built
    on the device at first use (rows*cols*theta_disc*2 bytes of HBM).

    ``refine=True`` turns on the origin-corrected query (option ``lut_refine``, include/scanlib.h): every query reads the
    row of the pose's nearest cell corner and takes the pose's offset from it, projected on the beam, off the entry —
    the same table and table bytes, ranges within one cell of exact ray marching for ~97 % of the rays instead of ~78 %."""
    KIND = _lib.RL_GIANT_LUT

    def __init__(self, omap, max_range_px, theta_disc, refine=False):
        super().__init__(omap, max_range_px, theta_disc)
        if refine:
            self.set_option("lut_refine", 1)

    def table(self, row0=0, row1=None):
        """(row1-row0, cols, theta_disc) uint16 slab of the device table (test hook)."""
        row1 = self.omap.height if row1 is None else row1
        out = np.empty((row1 - row0, self.omap.width, self.theta_disc), dtype=np.uint16)
        _lib.call("rl_method_read_lut", self, row0, row1, out)
        return out
