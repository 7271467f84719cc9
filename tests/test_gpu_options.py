"""Handle options on the MI355X: every option name of rl_method_set_option, with the clamp it applies, read back through
rl_method_get_info; and a fresh handle of every kind starts from rl_plan_default_opts (variant = the kind's default)."""
import ctypes as C

import numpy as np
import pytest

from pyracecarsimulator_amd import _lib, maps, range_libc

pytestmark = pytest.mark.gpu

VALUES = (-1000, -1, 0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 100, 256, 511, 512, 1024, 4096, 5000, 1 << 30)


def _clip(lo, hi):
    return lambda v: min(max(v, lo), hi)


def _bool(v):
    return int(v != 0)


def _at_least(lo):
    return lambda v: max(v, lo)


def _lds_sort(v):
    p = 128
    while p * 2 <= v and p * 2 <= 16384:
        p *= 2
    return p


# option -> what get_info answers after set_option(option, v) (variant < 0 is the kind's default: checked apart)
CLAMPS = {
    "variant": lambda v: v,
    "grid_mult": _at_least(1),
    "wg_threads": lambda v: 1024 if v >= 1024 else (512 if v >= 512 else 256),
    "low_water": lambda v: -1 if v < 0 else min(v, 63),
    "sort_poses": _bool,
    "xcd_bands": _at_least(1),
    "slots": _clip(0, 3),
    "tiled": _bool,
    "inline_prep": _bool,
    "inline_max": lambda v: v,
    "inline_map_kb": _at_least(0),
    "stripe_max": _at_least(0),
    "order_inline": _bool,
    "bin_multi_min": lambda v: v,
    "bin_generic": _bool,
    "run_log2": lambda v: -1 if v < 0 else min(v, 8),
    "cddt_bins": _bool,
    "cddt_sort": _bool,
    "debug_stamps": _bool,
    "slice_log2": _clip(8, 30),
    "cddt_theta_min": _at_least(0),
    "cddt_search": _clip(0, 2),
    "code_map": lambda v: 2 if v == 2 else 0,
    "code_min_rays": _at_least(0),
    "tail_pct": _clip(0, 75),
    "tail_wg_pct": _clip(10, 400),
    "timing": _clip(0, 2),
    "drain_prio": _bool,
    "spec_drain": _clip(0, 64),
    "spec_stretch": _clip(1, 4096),
    "drain_cap": _clip(1, 64),
    "drain_stretch": _clip(1, 4096),
    "group_drain": _clip(0, 16),
    "handoff": _bool,
    "handoff_cap": lambda v: 64 if v >= 64 else (32 if v >= 32 else (16 if v >= 16 else 8)),
    "handoff_wg": lambda v: 256 if v >= 256 else (128 if v >= 128 else 64),
    "nt_store": _bool,
    "bin_ppw": _clip(256, 8192),
    "tile_stripe": lambda v: -1 if v < 0 else min(v, 4096),
    "pinned_max_rays": _at_least(0),
    "direct_max_rays": _at_least(0),
    "overlap_min_rays": _at_least(0),
    "cddt_lds_sort": _lds_sort,
}
READ_ONLY = ("n_cu", "clock_khz", "code_entries", "last_grid", "map_epoch", "n_devices")
KINDS = {
    "RM": (range_libc.PyRayMarching, (), 3),
    "RMGPU": (range_libc.PyRayMarchingGPU, (), 1),
    "BL": (range_libc.PyBresenhamsLine, (), 1),
    "CDDT": (range_libc.PyCDDTCast, (108,), 1),
    "GLT": (range_libc.PyGiantLUTCast, (108,), 1),
}


@pytest.fixture(scope="module")
def grid(need_gpu):
    return maps.make_maze(128, cell=16, wall=2, p=0.4, seed=5)


@pytest.fixture(scope="module")
def omap(grid):
    return range_libc.PyOMap(grid, device=0)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_fresh_handle_options_equal_the_plan_defaults(omap, kind):
    cls, extra, variant = KINDS[kind]
    m = cls(omap, 60.0, *extra)
    d = _lib.PlanOpts()
    _lib.check(_lib.lib().rl_plan_default_opts(C.byref(d)))
    for name, _ in _lib.PlanOpts._fields_:
        if name in ("code_entries", "lut_debug"):       # (code_entries is the map's palette size: read-only)
            continue
        want = variant if name == "variant" else getattr(d, name)
        assert m.get_info(name) == want, (kind, name)
    assert m.get_info("code_entries") == 0               # (no step map built yet)


def test_every_option_clamps_as_set_option_states_it(grid, omap):
    rm, gpu = range_libc.PyRayMarching(omap, 60.0), range_libc.PyRayMarchingGPU(omap, 60.0)
    defaults = {name: gpu.get_info(name) for name in CLAMPS}
    for name, want in CLAMPS.items():
        for v in VALUES:
            gpu.set_option(name, v)
            if name == "variant" and v < 0:
                assert gpu.get_info(name) == 1
                rm.set_option(name, v)
                assert rm.get_info(name) == 3
                continue
            assert gpu.get_info(name) == want(v), (name, v, gpu.get_info(name))
    for v in VALUES:                                      # (stored as given; also the LUT / CDDT kernels' debug bits)
        gpu.set_option("lut_debug", v)
    gpu.set_option("lut_debug", 0)
    for name in READ_ONLY + ("multi_min_poses", "no_such_option"):   # (multi_min_poses: multi-device handles only)
        with pytest.raises(_lib.ScanLibError):
            gpu.set_option(name, 1)
    for name in READ_ONLY:
        assert gpu.get_info(name) >= 0
    assert gpu.get_info("n_devices") == 1 and gpu.get_info("n_cu") > 0
    for name in ("multi_min_poses", "no_such_option"):
        with pytest.raises(_lib.ScanLibError):
            gpu.get_info(name)
    # back at the defaults, the handle scans like a fresh one
    for name, v in defaults.items():
        gpu.set_option(name, v)
    fresh = range_libc.PyRayMarchingGPU(omap, 60.0)
    assert {name: gpu.get_info(name) for name in CLAMPS} == {name: fresh.get_info(name) for name in CLAMPS}
    poses = maps.sample_free_poses(grid, 4, 3)
    got, want = np.zeros(4 * 64, np.float32), np.ones(4 * 64, np.float32)
    gpu.calc_range_fan(poses, got, 4.71, 64)
    fresh.calc_range_fan(poses, want, 4.71, 64)
    assert np.array_equal(got, want) and want.max() > 0
