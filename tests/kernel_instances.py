"""The kernel instances the fan planner can name, each with the launch that reaches it, as plain data and small helpers:
no device call.  STREAM holds one row per rm_fan_stream_kernel<AUX, CRASH, NT, INLINE, TILED, SLOTS, LIT, CODE> instance the
library compiles (53), CHUNK the four rm_fan_kernel<AUX, CRASH>, OTHER every name the planner returns for the other
kernels.  tests/test_kernel_instances_host.py checks with the planner and the oracle alone that every row names its
instance and that the census inputs do what the GPU test takes them to do; tests/test_gpu_kernel_instances.py runs
every launchable row against the oracle and asserts the name the launch reports."""
import itertools

import numpy as np

import support
from pyracecarsimulator_amd import _lib, maps

UNREACHABLE = "no entry point requests diagnostics and a crash test together"
N_CU = 256                                    # the MI355X; the host test plans every row for it


# ---------------------------------------------------------------- the instance set
def _stream_instance(a, c, n, inl, t, s, lit, code):
    """csrc/launch_plan.h stream_instance, restated: the rm_fan_stream_kernel<AUX, CRASH, NT, INLINE, TILED, SLOTS, LIT,
    CODE> instances the library compiles."""
    return (n in (256, 512, 1024) and 1 <= s <= 3 and code in (0, 2)
            and (not lit or (not a and n == 1024 and inl and t and s <= 2))
            and (code == 0 or (s == 2 and not a and t and n == 1024))
            and (s == 1 or (not a and t))
            and (s != 3 or (not c and n == 1024 and code == 0))
            and (not inl or n == 1024 or (n == 512 and not c and t and s == 2 and not lit and code == 0)))


def _tf(b):
    return "true" if b else "false"


def stream_name(a, c, n, inl, t, s, lit, code):
    return "scan::rm_fan_stream_kernel<%s, %s, %d, %s, %s, %d, %s, %d>" % (_tf(a), _tf(c), n, _tf(inl), _tf(t), s, _tf(lit), code)


STREAM_KEYS = tuple((a, c, n, i, t, s, l, cd)
                    for a, c in itertools.product((0, 1), repeat=2) for n in (256, 512, 1024)
                    for i, t in itertools.product((0, 1), repeat=2) for s in (1, 2, 3) for l in (0, 1) for cd in (0, 2)
                    if _stream_instance(a, c, n, i, t, s, l, cd))


# ---------------------------------------------------------------- the census shape
MAZE = dict(cell=40, wall=3, p=0.45, seed=21, origin=(-7.0, 3.0, -0.4))       # the schedule test's map, rotated origin
MAZE_SIDE, MAX_RANGE, FOV = 400, 300, 4.71
POSES, BEAMS, GROUP = 768, 1025, 32           # 17 blocks of 64 rays per pose, the last holding one ray; 24 groups
POSE_SEED, CLEAR_PX, CLEAR_FAR_PX = 4, 2.0, 14.0
NAN_POSE, FAR_POSE, EDGE_POSE = 17, 200, 201  # the schedule test's three special poses
EDGE_WIDEN = 0.25                             # test_fused_crash_marks_poses_then_reduces' wide car
NOISE_OFFSET = 2 ** 32 - POSES * BEAMS // 2   # ray ids straddle 2^32
#: palette entries of the census map's u16 code map: its distinct positive EDT values and the two stop codes.  Read on
#: the MI355X (get_info("code_entries") after a launch); the host test restates it from the oracle's EDT, the GPU test
#: asserts it, so a drift is noticed instead of silently planning the float32 map.
PALETTE = 467


def census_map(side=MAZE_SIDE):
    """The census maze; ``side`` < 400: its lower-left cut of side x side cells (part 2's map)."""
    g = maps.make_maze(MAZE_SIDE, **MAZE)
    if side == MAZE_SIDE:
        return g
    occ = np.ascontiguousarray(g.occ[:side, :side]).copy()
    occ[0, :] = occ[-1, :] = occ[:, 0] = occ[:, -1] = 1
    return maps.GridMap(occ, g.resolution, g.origin, "maze%d" % side)


def census_poses(g, dt, n=POSES):
    """n poses in groups of GROUP: even groups CLEAR_FAR_PX cells from any wall — beyond the widened outline's reach of
    10.9 cells, a cell and a half for the pose's place within its cell and the march's last sample: none of them
    crashes —, odd groups CLEAR_PX cells; then the three special poses (all in even groups)."""
    poses = maps.sample_free_poses(g, n, POSE_SEED, CLEAR_PX, dt)
    far = maps.sample_free_poses(g, n, POSE_SEED + 1, CLEAR_FAR_PX, dt)
    even = (np.arange(n) // GROUP) % 2 == 0
    poses[even] = far[even]
    poses[NAN_POSE % n] = [np.nan, 0, 0]
    poses[FAR_POSE % n] = [1e6, 1e6, 1.0]
    # -1 < gx < 0: grid (-0.3, 20.0) through the map's rotated origin (the schedule test's pose of that name is written
    # for an unrotated origin; on this map it lies eight cells outside)
    ox, oy, yaw = g.origin
    gx, gy = -0.3, 20.0
    poses[EDGE_POSE % n] = [ox + (np.cos(yaw) * gx - np.sin(yaw) * gy) * g.resolution,
                            oy + (np.sin(yaw) * gx + np.cos(yaw) * gy) * g.resolution, yaw + 0.2]
    return poses


def census_edge(beams=BEAMS):
    return support.edge(beams, FOV) + EDGE_WIDEN


def palette_size(dt, max_range, coeff):
    """code_mark_kernel / code_scan_kernel restated: one entry per distinct positive EDT value whose step stays below
    max_range, and the two stop codes."""
    d = np.asarray(dt, np.float32).reshape(-1)
    d = d[d > 0]
    step = np.maximum(d * np.float32(coeff), np.float32(1.0))
    return int(np.unique(d[step < np.float32(max_range)]).size) + 2


# ---------------------------------------------------------------- 1. the stream instances, 2. the chunk kernel
def _stream_row(a, c, n, inl, t, s, lit, code):
    if a and c:
        return UNREACHABLE
    opts = {"grid_mult": 1, "slots": s, "wg_threads": n, "tiled": t, "inline_prep": inl, "code_map": code,
            "code_min_rays": 0}
    if not lit:
        opts = dict(variant=1, **opts)
    return ("PyRayMarching" if lit else "PyRayMarchingGPU", opts, bool(a), bool(c))


#: name -> (class, set_option dict, aux, crash) | UNREACHABLE.  PyRayMarchingGPU at variant 1 for LIT = false,
#: PyRayMarching at its default variant 3 for LIT = true.
STREAM = {stream_name(*k): _stream_row(*k) for k in STREAM_KEYS}
CHUNK = {"scan::rm_fan_kernel<%s, %s>" % (_tf(a), _tf(c)):
         UNREACHABLE if a and c else ("PyRayMarchingGPU", {"variant": 0, "grid_mult": 1}, bool(a), bool(c))
         for a, c in itertools.product((0, 1), repeat=2)}

KINDS = {"PyRayMarching": _lib.RL_RM, "PyRayMarchingGPU": _lib.RL_RM_GPU, "PyBresenhamsLine": _lib.RL_BRESENHAM,
         "PyCDDTCast": _lib.RL_CDDT, "PyGiantLUTCast": _lib.RL_GIANT_LUT}


def plan_row(row, rows, cols, n_poses, beams, theta_disc=0, max_range=MAX_RANGE):
    """rl_plan_fan of a launchable row at n_cu = 256 (code-map rows with the census palette): the plan as a dict."""
    cls, opts, aux, crash = row[:4]
    opts = dict(opts)
    if opts.get("code_map") == 2:
        opts["code_entries"] = PALETTE
    return _lib.plan_fan(KINDS[cls], rows, cols, n_poses, beams, max_range_px=max_range, theta_disc=theta_disc, n_cu=N_CU,
                         aux=aux, crash=crash, **opts)


def plan_blocks(plan, n_poses, beams):
    """The 64-ray blocks of a stream launch: per pose when the workgroups derive their records (a block never
    straddles two poses), over the whole batch behind a binning launch."""
    return n_poses * ((beams + 63) // 64) if plan["record_source"] else (n_poses * beams + 63) // 64


# ---------------------------------------------------------------- 3. the other kernels the planner can name
O_SIDE, O_POSES, O_BEAMS, O_BEAMS_17 = 120, 130, 129, 1025
#: (name, block) -> (class, set_option dict, aux, crash, theta_disc, beams, oracle) | "tests/<file>.py::<test>" (a test
#: that runs the instance and asserts its name).  ``oracle``: which OracleMap fan is the row's reference.
OTHER = {}
for _nl, _td in ((1, 112), (2, 514), (3, 1026)):          # 16-B loads per lane of one table row: ceil(td / 2 / 256)
    for _ch, _b in ((12, O_BEAMS), (17, O_BEAMS_17)):      # 64-beam chunks: up to 768 beams, up to 1088
        OTHER[("scan::lut_fan_lds_kernel<%d, %d>" % (_nl, _ch), 256)] = ("PyGiantLUTCast", {}, False, False, _td, _b, "lut_fan")
for _ch, _b in ((12, O_BEAMS), (17, O_BEAMS_17)):
    OTHER[("scan::lut_fan_kernel<%d>" % _ch, 256)] = ("PyGiantLUTCast", {"lut_debug": 4}, False, False, 112, _b, "lut_fan")
OTHER.update({
    ("scan::cddt_fan_bins_kernel", 256): ("PyCDDTCast", {}, False, False, 112, O_BEAMS, "cddt_fan"),
    ("scan::cddt_fan_bins_kernel", 1024): ("PyCDDTCast", {}, False, False, 720, O_BEAMS_17, "cddt_fan"),
    ("scan::cddt_fan_kernel", 256): ("PyCDDTCast", {"cddt_bins": 0}, False, False, 112, O_BEAMS, "cddt_fan"),
    ("scan::cddt_theta_search_kernel", 256): ("PyCDDTCast", {"cddt_theta_min": 1, "cddt_search": 0}, False, False, 112, O_BEAMS, "cddt_fan"),
    ("scan::cddt_theta_search2_kernel", 256): ("PyCDDTCast", {"cddt_theta_min": 1, "cddt_search": 1}, False, False, 112, O_BEAMS, "cddt_fan"),
    ("scan::cddt_theta_fused_kernel", 256): ("PyCDDTCast", {"cddt_theta_min": 1, "cddt_search": 2}, False, False, 112, O_BEAMS, "cddt_fan"),
    ("scan::bl_fan_stream_kernel<false, 1024>", 1024): ("PyBresenhamsLine", {}, False, False, 0, O_BEAMS, "bl_fan"),
    ("scan::bl_fan_stream_kernel<true, 1024>", 1024): ("PyBresenhamsLine", {}, True, False, 0, O_BEAMS, "bl_fan"),
    ("scan::bl_fan_kernel<false>", 256): ("PyBresenhamsLine", {"variant": 0}, False, False, 0, O_BEAMS, "bl_fan"),
    ("scan::bl_fan_kernel<true>", 256): ("PyBresenhamsLine", {"variant": 0}, True, False, 0, O_BEAMS, "bl_fan"),
    # (the occupancy-window march is approximate — within one cell of ray marching —: its own tests hold it)
    ("scan::occ_fan_lds_kernel<false>", 256): "tests/test_gpu_noise.py::test_noise_bresenham_kernels",
    ("scan::occ_fan_lds_kernel<true>", 256): "tests/test_gpu_parity.py::test_occ_fan_lds_north_star_shape_within_one_cell_of_ray_marching",
    ("scan::rm_literal_kernel<false, false>", 256): ("PyRayMarching", {"tiled": 0}, False, False, 0, O_BEAMS, "rm_fan_libm"),
    ("scan::rm_literal_kernel<true, false>", 256): ("PyRayMarching", {}, True, False, 0, O_BEAMS, "rm_fan_libm"),
})
