"""ctypes loader for libscan_amd.so (C ABI: include/scanlib.h) and the one call layer of the package.

The library is the product: hand-written HIP kernels for gfx950 behind a C ABI.
There is no Python/NumPy fallback — if the shared object is missing or no HIP
device is usable, the calls raise.

``SYMBOLS`` restates every prototype of the header, and one table more does the same for each feature header next to
it.  ``HEADERS`` is the one list of them: per public header its file, its table, the structures it declares with the
classes that restate them, and its handle types (the list closes this text).  tests/test_py_calls_host.py pins every
entry to its header, argument by argument, with the structures and enums below; ``declared``, ``lib`` and ``build``
read the tables through ``HEADERS`` only.
``call(name, *args)`` is how the package's wrappers enter the library: every argument is converted by the type the
tables declare for it, and a symbol that returns ``rl_status`` is checked (``ScanLibError``) and gives None.  What a
declared type takes:

* pointer to a scalar (``float *``, ``int *``, ``uint64_t *`` ...): an ``ndarray`` of exactly that dtype, C-contiguous
  (anything else is a ``TypeError`` naming symbol and position — never a silent copy, an output would be lost); None
  (NULL); a ctypes scalar of the pointee type, passed by reference (an out-parameter);
* ``void **`` (a handle out) and pointer to a ``Structure``: the instance, by reference; None (NULL);
* ``void *`` (handles, device pointers, streams): a ``Handle`` or its ``_h``; None or 0 (NULL); an int (an address).
  An ``ndarray`` is refused: a host array where a handle or device pointer is wanted;
* ``const char *``: a ``str`` (encoded) or ``bytes``;
* scalars: ``int()`` / ``float()`` of the argument (NumPy scalars and bools pass);
* ``const float *const *`` (rl_policy_create): a sequence of float32 arrays, each checked as above.

``lib()`` is the typed CDLL for direct use (tests, tools, bench.py); ``raw(name)`` the all-``void *`` form for callers
that keep the addresses of long-lived buffers.
"""
from __future__ import annotations

import collections
import ctypes as C
import operator
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
#: SCANLIB_SO: an alternative build of the library (A/B runs of two builds on one box, tools/ab_so.sh)
_SO = os.environ.get("SCANLIB_SO") or os.path.join(_HERE, "libscan_amd.so")
_LIB = None

RL_OK, RL_ERR_INVALID, RL_ERR_NO_DEVICE, RL_ERR_HIP, RL_ERR_UNSUPPORTED, RL_ERR_NOMEM = 0, -1, -2, -3, -4, -5
RL_BRESENHAM, RL_RM, RL_RM_GPU, RL_CDDT, RL_GIANT_LUT = 0, 1, 2, 3, 4

f32p = C.POINTER(C.c_float)
f64p = C.POINTER(C.c_double)
i32p = C.POINTER(C.c_int32)
u16p = C.POINTER(C.c_uint16)
u8p = C.POINTER(C.c_uint8)


class PlanOpts(C.Structure):
    """rl_plan_opts (include/scanlib.h): the options that shape a launch."""
    _fields_ = [(n, C.c_int) for n in (
        "variant", "grid_mult", "wg_threads", "low_water", "sort_poses", "xcd_bands", "slots", "tiled",
        "inline_prep", "inline_max", "inline_map_kb", "stripe_max", "order_inline", "bin_multi_min",
        "bin_generic", "run_log2", "cddt_bins", "cddt_sort", "lut_debug", "debug_stamps", "slice_log2",
        "cddt_theta_min", "cddt_search", "code_map", "code_min_rays", "tail_pct", "tail_wg_pct", "code_entries")]


class LaunchPlan(C.Structure):
    """rl_launch_plan (include/scanlib.h)."""
    _fields_ = [(n, C.c_int) for n in (
        "kernel", "grid", "block", "lds_bytes", "binning", "record_source", "slots", "bands", "run_log2",
        "k_max", "tiled", "aux", "crash", "nl", "ch", "slices", "slice_poses", "code", "code_entries", "gen1")] + [("name", C.c_char * 192)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "name"}
        d["name"] = self.name.decode()
        d["kernel"] = KERNEL_IDS.get(self.kernel, str(self.kernel))
        d["binning"] = BINNINGS.get(self.binning, str(self.binning))
        return d


class MctsParams(C.Structure):
    """rl_mcts_params (include/scanlib.h)."""
    _fields_ = [("n_trees", C.c_int), ("max_nodes", C.c_int), ("rollout_steps", C.c_int), ("action_every", C.c_int),
                ("source", C.c_int)] + [(n, C.c_double) for n in (
                    "speed", "dt", "scan_dist_to_base", "C", "crash_pen", "uni_dev", "max_steer", "max_speed")] + [
                ("fov", C.c_float), ("num_rays", C.c_int), ("crash_thresh", C.c_double), ("rollout_source", C.c_int),
                ("rollout_dev", C.c_double)]


class PfParams(C.Structure):
    """rl_pf_params (include/scanlib.h)."""
    _fields_ = [("n_particles", C.c_int), ("n_angles", C.c_int), ("motion_std", C.c_double * 3),
                ("resample_ratio", C.c_double)]


class EnvParams(C.Structure):
    """rl_env_params (include/scanlib.h)."""
    _fields_ = [(n, C.c_int) for n in ("n_envs", "substeps", "num_rays", "obs_start", "obs_count", "obs_stride")] + [
        ("obs_clip", C.c_float), ("obs_scale", C.c_float), ("max_ticks", C.c_int), ("auto_reset", C.c_int)] + [
        (n, C.c_double) for n in ("dt", "scan_dist_to_base", "crash_thresh", "steer_clip", "crash_reward")] + [
        ("fov", C.c_float)]


class RaceEnvParams(C.Structure):
    """rl_race_env_params (include/scanlib.h)."""
    _fields_ = [("env", EnvParams), ("group", C.c_int), ("min_running", C.c_int)]


class TrackParams(C.Structure):
    """rl_track_params (include/scanlib.h)."""
    _fields_ = [("window", C.c_int), ("goal_span", C.c_int), ("reward_mode", C.c_int), ("lookahead", C.c_double)]


class PlanTrackParams(C.Structure):
    """rl_plan_track_params (include/scanlib_track_plan.h)."""
    _fields_ = [("reward_mode", C.c_int), ("window", C.c_int), ("goal_span", C.c_int), ("lookahead", C.c_double)]


class DriveTrackParams(C.Structure):
    """rl_drive_track_params (include/scanlib_track_drive.h)."""
    _fields_ = [("window", C.c_int), ("goal_dist", C.c_double)]


class SeatParams(C.Structure):
    """rl_seat_params (include/scanlib_seats.h)."""
    _fields_ = [("driver", C.c_int * 8), ("speed", C.c_float * 8)]


RL_MCTS_FG, RL_MCTS_NN, RL_MCTS_RANDOM, RL_MCTS_PURSUIT = 0, 1, 2, 3
#: enum rl_seat_driver (include/scanlib_seats.h)
SEAT_DRIVERS = {"caller": 0, "followgap": 1, "policy": 2}

KERNEL_IDS = {0: "none", 1: "rm_chunk", 2: "rm_stream", 3: "occ_lds", 4: "bl_stream", 5: "bl_lds", 6: "lut_lds",
              7: "lut_fan", 8: "cddt_bins", 9: "cddt_rays", 10: "cddt_theta", 11: "rm_literal", 12: "rm_stream_literal"}
BINNINGS = {0: "none", 1: "small_keys", 2: "small_records", 3: "grid_sort", 4: "grid_unsorted", 5: "generic"}

#: every symbol include/scanlib.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "rl_version": (C.c_char_p, []),
    "rl_last_error": (C.c_char_p, []),
    "rl_device_count": (C.c_int, []),
    "rl_map_create": (C.c_int, [u8p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                                C.c_int, C.POINTER(C.c_void_p)]),
    "rl_map_create_multi": (C.c_int, [u8p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                                      C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    "rl_map_n_devices": (C.c_int, [C.c_void_p]),
    "rl_map_replica": (C.c_void_p, [C.c_void_p, C.c_int]),
    "rl_map_update": (C.c_int, [C.c_void_p, u8p]),
    "rl_map_stamp_cells": (C.c_int, [C.c_void_p, i32p, C.c_int, C.c_uint8]),
    "rl_map_destroy": (None, [C.c_void_p]),
    "rl_map_rows": (C.c_int, [C.c_void_p]),
    "rl_map_cols": (C.c_int, [C.c_void_p]),
    "rl_map_device": (C.c_int, [C.c_void_p]),
    "rl_map_get_dt": (C.c_int, [C.c_void_p, f32p]),
    "rl_map_get_occ": (C.c_int, [C.c_void_p, u8p]),
    "rl_method_create": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int,
                                   C.POINTER(C.c_void_p)]),
    "rl_method_destroy": (None, [C.c_void_p]),
    "rl_method_kind": (C.c_int, [C.c_void_p]),
    "rl_method_n_devices": (C.c_int, [C.c_void_p]),
    "rl_method_replica": (C.c_void_p, [C.c_void_p, C.c_int]),
    "rl_calc_range_many": (C.c_int, [C.c_void_p, f32p, f32p, C.c_int]),
    "rl_calc_range_many_fan": (C.c_int, [C.c_void_p, f32p, f32p, C.c_int, C.c_float, C.c_int]),
    "rl_calc_range_fan": (C.c_int, [C.c_void_p, f32p, C.c_int, C.c_float, C.c_int, f32p, i32p,
                                    u16p]),
    "rl_calc_range_fan_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rl_calc_range_many_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                            C.c_void_p]),
    "rl_calc_range_repeat_angles": (C.c_int, [C.c_void_p, f32p, C.c_int, f32p, C.c_int, f32p, i32p, u16p]),
    "rl_calc_range_repeat_angles_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "rl_set_sensor_model": (C.c_int, [C.c_void_p, f64p, C.c_int]),
    "rl_eval_sensor_model": (C.c_int, [C.c_void_p, f32p, f32p, C.c_int, C.c_int, f64p]),
    "rl_eval_sensor_model_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                              C.c_void_p]),
    "rl_calc_range_repeat_angles_eval_sensor_model": (C.c_int, [C.c_void_p, f32p, C.c_int, f32p, f32p, C.c_int, f64p]),
    "rl_calc_range_repeat_angles_eval_sensor_model_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                                       C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "rl_pf_create": (C.c_int, [C.c_void_p, C.POINTER(PfParams), f32p, C.POINTER(C.c_void_p)]),
    "rl_pf_destroy": (None, [C.c_void_p]),
    "rl_pf_reset": (C.c_int, [C.c_void_p, f64p, f64p, C.c_uint64]),
    "rl_pf_run": (C.c_int, [C.c_void_p, C.c_int, f64p, f32p, f64p, f64p, i32p]),
    "rl_pf_read": (C.c_int, [C.c_void_p, f64p, f64p, i32p, f64p, f64p]),
    "rl_set_noise": (C.c_int, [C.c_void_p, C.c_float, C.c_uint64, C.c_uint64]),
    "rl_check_collision_many": (C.c_int, [C.c_void_p, f32p, C.c_int, C.c_float, C.c_int, f64p,
                                          C.c_double, C.POINTER(C.c_int), f32p]),
    "rl_check_collision_groups": (C.c_int, [C.c_void_p, f32p, C.c_int, C.c_int, C.c_float, C.c_int, f64p,
                                            C.c_double, C.POINTER(C.c_int), f32p]),
    "rl_check_collision_groups_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float,
                                                   C.c_int, C.c_void_p, C.c_double, C.c_void_p,
                                                   C.c_void_p, C.c_void_p]),
    "rl_calc_range_fan_multi_device": (C.c_int, [C.c_void_p, f32p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "rl_check_collision_groups_multi_device": (C.c_int, [C.c_void_p, f32p, C.c_int, C.c_int, C.c_float, C.c_int, f64p,
                                                         C.c_double, C.c_int, C.c_void_p]),
    "rl_followgap_create": (C.c_int, [C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
                                      C.POINTER(C.c_void_p)]),
    "rl_followgap_destroy": (None, [C.c_void_p]),
    "rl_followgap_eval": (C.c_int, [C.c_void_p, f32p, C.c_int, C.c_int, f32p]),
    "rl_followgap_eval_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p]),
    "rl_car_create": (C.c_int, [C.c_int, f64p, C.POINTER(C.c_void_p)]),
    "rl_car_create_multi": (C.c_int, [C.POINTER(C.c_int), C.c_int, f64p, C.POINTER(C.c_void_p)]),
    "rl_car_destroy": (None, [C.c_void_p]),
    "rl_car_rollout": (C.c_int, [C.c_void_p, f64p, f64p, C.c_int, C.c_int, C.c_int, C.c_double, f32p,
                                 f64p, f64p]),
    "rl_car_rollout_check": (C.c_int, [C.c_void_p, C.c_void_p, f64p, f64p, C.c_int, C.c_int, C.c_int,
                                       C.c_double, C.c_float, C.c_int, f64p, C.c_double,
                                       C.POINTER(C.c_int), f64p, f64p]),
    "rl_car_drive_followgap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, f64p, f64p, f32p, C.c_int, C.c_int,
                                         C.c_double, C.c_double, C.c_float, C.c_int, f64p, C.c_double,
                                         C.POINTER(C.c_int), f64p, f64p, f32p, f32p, f64p]),
    "rl_car_outline_cells": (C.c_int, [C.c_void_p, C.c_void_p, f64p, C.c_int, C.c_int, i32p, C.POINTER(C.c_int)]),
    "rl_calc_range_fan_cars": (C.c_int, [C.c_void_p, f32p, f64p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_float,
                                         C.c_int, f32p, i32p, u16p]),
    "rl_calc_range_fan_cars_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double,
                                                C.c_double, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p]),
    "rl_car_race_followgap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, f64p, f64p, f32p, C.c_int, C.c_int, C.c_int,
                                        C.c_double, C.c_double, C.c_float, C.c_int, f64p, C.c_double,
                                        C.POINTER(C.c_int), f64p, f64p, f32p, f32p, f64p]),
    "rl_policy_create": (C.c_int, [C.c_int, C.c_int, i32p, C.POINTER(f32p), C.POINTER(f32p), u8p, C.c_int,
                                   C.c_float, C.c_float, C.POINTER(C.c_void_p)]),
    "rl_policy_destroy": (None, [C.c_void_p]),
    "rl_policy_eval": (C.c_int, [C.c_void_p, f32p, C.c_int, C.c_int, f32p]),
    "rl_policy_eval_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rl_car_drive_policy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, f64p, f64p, f32p, C.c_int, C.c_int,
                                      C.c_double, C.c_double, C.c_float, C.c_int, f64p, C.c_double, C.c_double,
                                      C.POINTER(C.c_int), f64p, f64p, f32p, f32p, f64p]),
    "rl_env_create": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(EnvParams), f64p, f64p, C.c_int, C.POINTER(C.c_void_p)]),
    "rl_env_destroy": (None, [C.c_void_p]),
    "rl_env_reset": (C.c_int, [C.c_void_p, C.c_uint64, i32p, f32p, f32p, i32p]),
    "rl_env_step": (C.c_int, [C.c_void_p, f32p, f32p, f32p, i32p, f32p]),
    "rl_env_reset_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rl_env_step_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rl_env_read": (C.c_int, [C.c_void_p, f64p, i32p, i32p, i32p, i32p]),
    "rl_env_create_race": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RaceEnvParams), f64p, f64p, C.c_int,
                                     C.POINTER(C.c_void_p)]),
    "rl_env_read_races": (C.c_int, [C.c_void_p, i32p, i32p, i32p, i32p]),
    "rl_track_create": (C.c_int, [C.c_int, f64p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "rl_track_destroy": (None, [C.c_void_p]),
    "rl_track_read": (C.c_int, [C.c_void_p, f64p, f64p]),
    "rl_env_attach_track": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(TrackParams)]),
    "rl_env_read_track": (C.c_int, [C.c_void_p, f32p, i32p]),
    "rl_env_read_track_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rl_mcts_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MctsParams), f64p,
                                 C.POINTER(C.c_void_p)]),
    "rl_mcts_destroy": (None, [C.c_void_p]),
    "rl_mcts_reset": (C.c_int, [C.c_void_p, f64p, f64p, C.POINTER(C.c_uint64)]),
    "rl_mcts_run": (C.c_int, [C.c_void_p, C.c_int]),
    "rl_mcts_best": (C.c_int, [C.c_void_p, f64p, i32p, i32p]),
    "rl_mcts_drive": (C.c_int, [C.c_void_p, f64p, f64p, C.POINTER(C.c_uint64), C.c_int, C.c_int, C.c_int, C.c_double,
                                i32p, f64p, f64p, f64p, i32p, f64p]),
    "rl_mcts_read_tree": (C.c_int, [C.c_void_p, C.c_int, i32p, i32p, i32p, i32p, i32p, i32p, f64p, f64p, i32p, f64p,
                                    f32p, f32p, i32p, i32p]),
    "rl_mcts_probe_ucb": (C.c_int, [C.c_int, f64p, i32p, i32p, C.c_size_t, C.c_double, f64p]),
    "rl_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    "rl_host_free": (C.c_int, [C.c_void_p]),
    "rl_car_edge_distances": (C.c_int, [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                        f64p]),
    "rl_car_is_crashed": (C.c_int, [f32p, C.c_int, C.c_int, f64p, C.c_double, C.POINTER(C.c_int)]),
    "rl_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "rl_method_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "rl_method_get_info": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]),
    "rl_method_read_lut": (C.c_int, [C.c_void_p, C.c_int, C.c_int, u16p]),
    "rl_debug_read_stamps": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]),
    "rl_probe_gather_rate": (C.c_int, [C.c_int, C.c_int, f64p, f64p, C.POINTER(C.c_int)]),
    "rl_plan_default_opts": (C.c_int, [C.POINTER(PlanOpts)]),
    "rl_plan_fan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.POINTER(PlanOpts), C.c_int,
                              C.c_int, C.c_int, C.c_int, C.POINTER(LaunchPlan)]),
    "rl_method_plan_fan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(LaunchPlan)]),
    "rl_method_last_plan": (C.c_int, [C.c_void_p, C.POINTER(LaunchPlan)]),
    "rl_launch_contexts": (C.c_int, []),
    "rl_probe_hbm": (C.c_int, [C.c_int, C.c_size_t, f64p]),
    "rl_probe_hbm_nt": (C.c_int, [C.c_int, C.c_size_t, f64p]),
    "rl_probe_literal_sincosf": (C.c_int, [C.c_int, f32p, C.c_size_t, f32p, f32p]),
    "rl_ranges_to_u16_device": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p]),
    "rl_ranges_from_u16_device": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p]),
}

#: every symbol include/scanlib_track_plan.h declares, in the shape of ``SYMBOLS``
EXT_SYMBOLS = {
    "rl_car_rollout_track": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PlanTrackParams), f64p, f64p, C.c_int, C.c_int,
                                       C.c_int, C.c_double, C.POINTER(C.c_int), f64p, f64p, f64p, C.POINTER(C.c_int),
                                       f64p]),
    "rl_mcts_attach_track": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PlanTrackParams)]),
    "rl_mcts_set_points": (C.c_int, [C.c_void_p, f64p]),
    "rl_mcts_read_track": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), f64p, C.POINTER(C.c_int), f64p]),
}


#: every symbol include/scanlib_seats.h declares, in the shape of ``SYMBOLS``
SEAT_SYMBOLS = {
    "rl_car_race_seats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_double, f64p,
                                    f64p, f32p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_float, C.c_int,
                                    f64p, C.c_double, C.POINTER(C.c_int), f64p, f64p, f32p, f32p, f64p]),
    "rl_env_attach_seats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SeatParams)]),
    "rl_env_read_seats": (C.c_int, [C.c_void_p, f32p]),
    "rl_env_read_seats_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
}


#: every symbol include/scanlib_population.h declares, in the shape of ``SYMBOLS``.  Every ``int`` is an rl_status:
#: sizes come back through pointers
POP_SYMBOLS = {
    "rl_policy_pop_create": (C.c_int, [C.c_int, C.c_int, C.c_int, i32p, u8p, C.c_int, C.c_float, C.c_float,
                                       C.POINTER(C.c_void_p)]),
    "rl_policy_pop_destroy": (None, [C.c_void_p]),
    "rl_policy_pop_layout": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rl_policy_pop_set": (C.c_int, [C.c_void_p, C.c_int, C.c_int, f32p]),
    "rl_policy_pop_set_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rl_policy_pop_get": (C.c_int, [C.c_void_p, C.c_int, f32p]),
    "rl_policy_pop_eval": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, f32p, C.c_int, f32p]),
    "rl_policy_pop_eval_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                            C.c_void_p]),
    "rl_car_drive_population": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, f64p,
                                          f64p, f32p, C.c_int, C.c_double, C.c_double, C.c_float, C.c_int, f64p,
                                          C.c_double, C.POINTER(C.c_int), f64p, f64p, f32p, f32p, f64p, f64p]),
}


#: every symbol include/scanlib_league.h declares, in the shape of ``SYMBOLS``.  Every ``int`` is an rl_status
LEAGUE_SYMBOLS = {
    "rl_policy_pop_eval_rows": (C.c_int, [C.c_void_p, C.c_int, i32p, f32p, C.c_int, f32p]),
    "rl_policy_pop_eval_rows_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                 C.c_void_p]),
    "rl_car_race_league": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, i32p, C.c_double, f64p, f64p, f32p,
                                     C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_float, C.c_int, f64p,
                                     C.c_double, C.POINTER(C.c_int), f64p, f64p, f32p, f32p, f64p, f64p]),
}


#: every symbol include/scanlib_league_env.h declares, in the shape of ``SYMBOLS``.  Every ``int`` is an rl_status
LEAGUE_ENV_SYMBOLS = {
    "rl_env_attach_league": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, i32p, f32p]),
    "rl_env_set_league_entries": (C.c_int, [C.c_void_p, i32p]),
    "rl_env_set_league_entries_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rl_env_read_league_steers": (C.c_int, [C.c_void_p, f32p]),
    "rl_env_read_league_steers_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rl_env_read_league_entries": (C.c_int, [C.c_void_p, i32p, i32p]),
    "rl_env_read_league_results": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
}


#: every symbol include/scanlib_track_drive.h declares, in the shape of ``SYMBOLS``.  Every ``int`` is an rl_status
TRACK_DRIVE_SYMBOLS = {
    "rl_car_attach_track": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(DriveTrackParams)]),
    "rl_car_read_track": (C.c_int, [C.c_void_p, C.c_int, f64p, C.POINTER(C.c_int)]),
    "rl_car_read_track_scores": (C.c_int, [C.c_void_p, C.c_int, C.c_int, f64p]),
}


#: every public header, in the order the features came: its file under include/, the table of its symbols, {structure it
#: declares: the class that restates it}, and the handle types it declares beyond those of scanlib.h
Header = collections.namedtuple("Header", "file symbols structs handles")
HEADERS = (
    Header("scanlib.h", SYMBOLS, {"rl_plan_opts": PlanOpts, "rl_launch_plan": LaunchPlan, "rl_mcts_params": MctsParams,
                                  "rl_pf_params": PfParams, "rl_env_params": EnvParams,
                                  "rl_race_env_params": RaceEnvParams, "rl_track_params": TrackParams}, ()),
    Header("scanlib_track_plan.h", EXT_SYMBOLS, {"rl_plan_track_params": PlanTrackParams}, ()),
    Header("scanlib_seats.h", SEAT_SYMBOLS, {"rl_seat_params": SeatParams}, ()),
    Header("scanlib_population.h", POP_SYMBOLS, {}, ("rl_policy_pop",)),
    Header("scanlib_league.h", LEAGUE_SYMBOLS, {}, ()),
    Header("scanlib_league_env.h", LEAGUE_ENV_SYMBOLS, {}, ()),
    Header("scanlib_track_drive.h", TRACK_DRIVE_SYMBOLS, {"rl_drive_track_params": DriveTrackParams}, ()),
)
__doc__ += "\nThe public headers: %s.\n" % ", ".join("include/%s (%d symbols)" % (h.file, len(h.symbols)) for h in HEADERS)


def _merge(headers):
    """One dictionary of every header's symbols; a name two headers declare is an error."""
    merged = {}
    for h in headers:
        if set(merged) & set(h.symbols):
            raise ValueError("include/%s declares %s again" % (h.file, ", ".join(sorted(set(merged) & set(h.symbols)))))
        merged.update(h.symbols)
    return merged


_DECLARED = _merge(HEADERS)
#: (restype, argtypes) of a name, whichever header of ``HEADERS`` declares it; KeyError for any other
declared = _DECLARED.__getitem__


#: the symbols whose ``int`` is a value; every other ``int`` function returns rl_status (``call`` checks it)
INT_VALUED = frozenset(("rl_device_count", "rl_launch_contexts", "rl_map_rows", "rl_map_cols", "rl_map_device",
                        "rl_map_n_devices", "rl_method_kind", "rl_method_n_devices", "rl_debug_read_stamps"))


def plan_fan(kind, rows, cols, n_poses, num_rays, max_range_px=300.0, theta_disc=0, n_cu=256, aux=False,
             crash=False, **opts):
    """The launch plan of a fan call (rl_plan_fan: pure host arithmetic, no device needed) as a dict.
    ``opts`` override fields of the default rl_plan_opts."""
    o = PlanOpts()
    call("rl_plan_default_opts", o)
    for k, v in opts.items():
        if not hasattr(o, k):
            raise KeyError("unknown plan option %r" % k)
        setattr(o, k, int(v))
    pl = LaunchPlan()
    call("rl_plan_fan", kind, n_cu, rows, cols, max_range_px, theta_disc, o, n_poses, num_rays, bool(aux), bool(crash),
         pl)
    return pl.as_dict()


class ScanLibError(RuntimeError):
    """A libscan_amd.so call returned a negative rl_status."""

    def __init__(self, code, msg):
        super().__init__("libscan_amd: %s (rl_status %d)" % (msg, code))
        self.code = code


def build_sources():
    """The files ``build`` compares with the library: csrc's units and kernel headers, and every header of ``HEADERS``."""
    return [os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc")) if f.endswith((".hip", ".h"))
            ] + [os.path.join(_HERE, "..", "include", h.file) for h in HEADERS]


def build(force: bool = False) -> str:
    """Compile libscan_amd.so for gfx950 with hipcc (in-tree; cross-compiles without a GPU)."""
    stale = (not os.path.exists(_SO)) or any(os.path.getmtime(s) > os.path.getmtime(_SO)
                                             for s in build_sources())
    if force or stale:
        subprocess.check_call(["make", "-j4", "-C", os.path.join(_HERE, "csrc"), "../libscan_amd.so"]
                              + (["-B"] if force else []))
    return _SO


def _share_torch_hip_runtime():
    """PyTorch wheels carry their own copy of the HIP/HSA runtime (torch/lib/libamdhip64.so, same
    SONAME as /opt/rocm's).  A process must run ONE runtime: if libscan_amd.so pulls in the system
    copy first and torch is imported later, torch's HSA runtime finds the device already taken
    ("No HIP GPUs are available").  So when torch is installed but not imported yet, its runtime is
    loaded first and libscan_amd.so binds to it — the same arrangement as importing torch before
    this package.  Without torch (or with SCANLIB_SYSTEM_HIP=1) the system runtime is used."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("SCANLIB_SYSTEM_HIP") == "1":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """Load libscan_amd.so; raises if it has not been built (no fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            raise ImportError(
                "libscan_amd.so is missing: run `python -c 'import __graft_entry__ as g; "
                "g.build()'` (or make -C pyracecarsimulator_amd/csrc). There is no CPU fallback.")
        _share_torch_hip_runtime()
        L = C.CDLL(_SO)
        for name, (res, args) in _DECLARED.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                if os.environ.get("SCANLIB_SO"):          # an older build in an A/B run: newer entry points absent
                    continue
                raise
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


_RAW = {}


def raw(name):
    """The same entry point with every pointer argument typed ``void*``: callers that keep the
    addresses of long-lived buffers (ints) skip the per-call ``ndarray.ctypes.data_as`` objects —
    a few microseconds on the 25-us scan() path."""
    fn = _RAW.get(name)
    if fn is None:
        res, args = declared(name)
        args = [C.c_void_p if (isinstance(a, type) and issubclass(a, C._Pointer)) else a for a in args]
        fn = C.CFUNCTYPE(res, *args)((name, lib()))
        _RAW[name] = fn
    return fn


def check(code: int) -> None:
    if code != RL_OK:
        raise ScanLibError(code, lib().rl_last_error().decode("utf-8", "replace"))


def _refuse(name, i, what, a):
    return TypeError("%s argument %d: %s, got %s" % (name, i, what, getattr(a, "dtype", type(a).__name__)))


def _converter(name, i, t):
    """What ``call`` does to argument ``i`` (declared type ``t``) of ``name``: see the module text."""
    import numpy as np
    if t is C.c_void_p:
        def conv(a):
            if type(a) is int:                             # (first: the device forms pass addresses, call after call)
                return a or None
            if isinstance(a, Handle):
                return a._h
            if a is None or isinstance(a, C.c_void_p):
                return a
            if isinstance(a, np.ndarray):
                raise _refuse(name, i, "a handle or device address, not a host array", a)
            return operator.index(a) or None
    elif t is C.c_char_p:
        def conv(a):
            return a.encode() if isinstance(a, str) else a
    elif not issubclass(t, C._Pointer):
        conv = float if t in (C.c_float, C.c_double) else int
    elif issubclass(t._type_, C._Pointer):                 # const float *const *
        inner = _converter(name, i, t._type_)

        def conv(a):
            return (C.c_void_p * len(a))(*[inner(x) for x in a])
    elif issubclass(t._type_, (C.Structure, C.c_void_p)):
        cls = t._type_

        def conv(a):
            if a is None:
                return None
            if not isinstance(a, cls):
                raise _refuse(name, i, "a %s" % cls.__name__, a)
            return C.addressof(a)
    else:
        cls, dt = t._type_, np.dtype(t._type_)

        def conv(a):
            if isinstance(a, np.ndarray):
                if a.dtype != dt or not a.flags.c_contiguous:
                    raise _refuse(name, i, "a C-contiguous %s array" % dt, a)
                return a.ctypes.data
            if a is None:
                return None
            if not isinstance(a, cls):
                raise _refuse(name, i, "a %s array, a %s or None" % (dt, cls.__name__), a)
            return C.addressof(a)
    return conv


_CALLS = {}


def converters(name):
    """(the all-``void *`` entry point, one converter per argument, returns rl_status?) of ``name``, built once."""
    ent = _CALLS.get(name)
    if ent is None:
        res, args = declared(name)
        ent = _CALLS[name] = (raw(name), tuple(_converter(name, i, t) for i, t in enumerate(args)),
                              res is C.c_int and name not in INT_VALUED)
    return ent


def call(name, *args):
    """Enter the library at ``name`` with ``args`` converted by their declared types (the module text says how).  A
    symbol that returns rl_status gives None or raises ``ScanLibError``; any other gives its value."""
    fn, convs, status = converters(name)
    if len(args) != len(convs):
        raise TypeError("%s takes %d arguments, got %d" % (name, len(convs), len(args)))
    rc = fn(*[cv(a) for cv, a in zip(convs, args)])
    if not status:
        return rc
    if rc:
        check(rc)


class Handle:
    """Base of every wrapper of a C handle: ``_h`` (a ``ctypes.c_void_p``) and ``_destroy``, the ``rl_*_destroy``
    symbol that gives it back.  ``close()`` may be called any number of times; a handle marked ``_borrowed`` (the
    per-device replica of a multi-device parent) is left to its owner."""
    _destroy = None
    _h = None                 # (until __init__ has made the handle)
    _borrowed = False

    def close(self):
        h = self._h
        if h is not None and h.value and not self._borrowed:
            self._h = C.c_void_p()
            getattr(lib(), self._destroy)(h)

    def __del__(self):
        try:
            self.close()
        except Exception:     # (interpreter shutdown: the module globals may be gone)
            pass


class _PinnedOwner:
    """Keeps one rl_host_alloc block alive for the NumPy array built on it."""

    def __init__(self, ptr):
        self.ptr = ptr

    def __del__(self):
        try:
            if self.ptr and _LIB is not None:
                _LIB.rl_host_free(C.c_void_p(self.ptr))
        except Exception:
            pass


def pinned_zeros(shape, dtype):
    """A zeroed NumPy array in pinned host memory of the library (rl_host_alloc): host-pointer scans
    write their ranges straight into it.  Falls back to ordinary memory when no device is usable (the
    array is then just an array; scans would fail earlier anyway)."""
    import numpy as np
    dt = np.dtype(dtype)
    n = int(np.prod(shape))
    p = C.c_void_p()
    try:
        rc = lib().rl_host_alloc(max(n, 1) * dt.itemsize, C.byref(p))
    except Exception:
        rc = -1
    if rc != RL_OK or not p.value:
        return np.zeros(shape, dtype=dt)
    nbytes = max(n, 1) * dt.itemsize

    class _Block(C.c_char * nbytes):              # (a Python subclass: instances can carry the owner)
        pass

    buf = _Block.from_address(p.value)
    buf._owner = _PinnedOwner(p.value)            # freed when the last array on the block is gone
    return np.frombuffer(buf, dtype=dt, count=n).reshape(shape)
