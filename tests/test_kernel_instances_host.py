"""tests/kernel_instances.py checked with the planner and the oracle alone (no device): every row names the instance it
stands for, the rows without a GPU run are exactly the AUX + CRASH ones, and the census inputs do what
tests/test_gpu_kernel_instances.py takes them to do."""
import itertools
import os
import re

import numpy as np
import pytest

import kernel_instances as KI
from conftest import ROOT
from pyracecarsimulator_amd import _lib
from support import THRESH


def _launchable(table):
    return {k: v for k, v in table.items() if not isinstance(v, str)}


def test_the_stream_table_is_the_instance_set():
    """53 rows, one per instance of csrc/launch_plan.h stream_instance, restated here by enumeration of the eight
    template arguments; abi_fan.hip compiles its dispatch table from the same predicate."""
    names = {KI.stream_name(a, c, n, i, t, s, l, cd)
             for a, c, i, t, l in itertools.product((0, 1), repeat=5) for n in (256, 512, 1024) for s in (1, 2, 3)
             for cd in (0, 2) if KI._stream_instance(a, c, n, i, t, s, l, cd)}
    assert len(names) == 53 and set(KI.STREAM) == names
    hdr = open(os.path.join(ROOT, "pyracecarsimulator_amd", "csrc", "launch_plan.h")).read()
    assert "constexpr bool stream_instance(const StreamKey &k)" in hdr
    assert len(KI.CHUNK) == 4


def test_only_the_aux_and_crash_instances_go_without_a_gpu_run():
    """The cap: a row holds the reason string exactly when its instance has AUX and CRASH both set — eight stream
    instances and rm_fan_kernel<true, true> — and the planner does name those nine (they are compiled and reachable
    by rl_plan_fan, but no entry point asks for hit cells and a crash test in one call)."""
    for table, pat in ((KI.STREAM, "rm_fan_stream_kernel<true, true, "), (KI.CHUNK, "rm_fan_kernel<true, true>")):
        for name, row in table.items():
            assert (row == KI.UNREACHABLE) == (pat in name), name
            assert isinstance(row, str) == (row == KI.UNREACHABLE), name
    dead = [n for t in (KI.STREAM, KI.CHUNK) for n, r in t.items() if isinstance(r, str)]
    assert len(dead) == 9
    assert len(_launchable(KI.STREAM)) == 45 and len(_launchable(KI.CHUNK)) == 3
    # the four entry-point call sites pass diagnostics pointers or crash parameters, never both
    csrc = os.path.join(ROOT, "pyracecarsimulator_amd", "csrc")
    calls = []
    for unit in ("abi_fan.hip", "abi_car.hip"):
        text = open(os.path.join(csrc, unit)).read()
        calls += [m.group(1) for m in re.finditer(r"FanCall\{([^}]*)\}", text)]
    assert len(calls) == 4
    for args in calls:
        a = [x.strip() for x in args.replace("\n", " ").split(",")]
        hits, steps, crash = a[6], a[7], a[8]
        assert (hits == "nullptr" and steps == "nullptr") or crash == "nullptr", args


@pytest.mark.parametrize("table", ["STREAM", "CHUNK"])
def test_every_launchable_row_plans_its_own_instance_on_the_census_shape(table):
    """rl_plan_fan at n_cu = 256 with the row's options (code-map rows with the census palette) returns RL_OK and names
    exactly the row's instance; every stream plan leaves each wave at least four 64-ray blocks per ray slot — so every
    wave claims, refills and drains several times — and the last block of a pose is partly filled."""
    assert KI.BEAMS % 64 == 1 and KI.POSES % KI.GROUP == 0
    worst, lds = None, 0
    for name, row in _launchable(getattr(KI, table)).items():
        cls, opts, aux, crash = row
        lit = table == "STREAM" and name.split(", ")[6] == "true"              # the seventh template argument
        assert cls == ("PyRayMarching" if lit else "PyRayMarchingGPU"), name
        assert ("variant" in opts) == (cls == "PyRayMarchingGPU")          # PyRayMarching at its default: 3
        assert opts["grid_mult"] == 1
        p = KI.plan_row(row, KI.MAZE_SIDE, KI.MAZE_SIDE, KI.POSES, KI.BEAMS)    # (raises unless RL_OK)
        assert p["name"] == name, (name, p["name"])
        assert (bool(p["aux"]), bool(p["crash"]), p["slices"]) == (aux, crash, 1), name
        assert p["lds_bytes"] <= 64 * 1024, (name, p["lds_bytes"])
        lds = max(lds, p["lds_bytes"])
        if table == "STREAM":
            assert p["code"] == opts["code_map"] and p["code_entries"] == (KI.PALETTE if p["code"] else 0), name
            blocks, waves = KI.plan_blocks(p, KI.POSES, KI.BEAMS), p["grid"] * p["block"] // 64
            assert blocks >= 4 * p["slots"] * waves, (name, blocks, p["slots"], waves)
            worst = min(worst or 1e9, blocks / (p["slots"] * waves))
    print(table, "fewest blocks per wave and ray slot:", worst, "largest dynamic LDS:", lds)


def _oracle():
    from oracle import oracle as O
    g = KI.census_map()
    return O, g, O.OracleMap.from_gridmap(g, KI.MAX_RANGE)


def test_the_census_inputs():
    """With the oracle alone: the palette size written into the table is the census map's (either step coefficient);
    the three special poses are what they are named; with the widened outline some groups of 32 poses crash and some
    do not, and the whole-batch index is neither 0 nor "none" — in the canonical and in the literal arithmetic."""
    O, g, om = _oracle()
    assert KI.palette_size(om.dt, KI.MAX_RANGE, 1.0) == KI.PALETTE == KI.palette_size(om.dt, KI.MAX_RANGE, 0.999)
    assert 2 <= KI.PALETTE <= 4096                                   # plan::CODE_MAX_ENTRIES
    poses = KI.census_poses(g, om.dt)
    assert poses.shape == (KI.POSES, 3) and np.isnan(poses[KI.NAN_POSE, 0]) and poses[KI.FAR_POSE, 0] == 1e6
    c, s = np.cos(g.origin[2]), np.sin(g.origin[2])
    dx, dy = poses[KI.EDGE_POSE, 0] - g.origin[0], poses[KI.EDGE_POSE, 1] - g.origin[1]
    assert -1.0 < (c * dx + s * dy) / g.resolution < 0.0
    assert np.isfinite(np.delete(poses, KI.NAN_POSE, 0)).all()
    edge = KI.census_edge()
    n_groups = KI.POSES // KI.GROUP
    for ranges in (om.rm_fan(poses, KI.FOV, KI.BEAMS, step_coeff=1.0, nthreads=4, want_hits=False, want_steps=False)[0],
                   om.rm_fan_libm(poses, KI.FOV, KI.BEAMS, step_coeff=0.999)[0]):
        whole = O.is_crashed(ranges, KI.BEAMS, KI.POSES, edge, THRESH)
        assert 0 < whole < KI.POSES, whole
        per = [O.is_crashed(ranges[k * KI.GROUP * KI.BEAMS:(k + 1) * KI.GROUP * KI.BEAMS], KI.BEAMS, KI.GROUP, edge,
                            THRESH) for k in range(n_groups)]
        crashed = sum(v >= 0 for v in per)
        assert 0 < crashed < n_groups, per
        assert all(v >= 0 or v == -(KI.GROUP + 1) for v in per)


# ---------------------------------------------------------------- the other kernels
def _other_sweep():
    """Every (name, block) the planner returns on part 2's shapes for a kernel that is neither the stream nor the
    chunk ray march: the sweep, in full."""
    RM, RMGPU, CDDT, GLT, BL = _lib.RL_RM, _lib.RL_RM_GPU, _lib.RL_CDDT, _lib.RL_GIANT_LUT, _lib.RL_BRESENHAM
    seen = set()

    def plan(kind, beams, td=0, aux=False, **o):
        p = _lib.plan_fan(kind, KI.O_SIDE, KI.O_SIDE, KI.O_POSES, beams, max_range_px=KI.MAX_RANGE, theta_disc=td,
                          n_cu=KI.N_CU, aux=aux, **o)
        if "rm_fan_stream_kernel" not in p["name"] and "rm_fan_kernel" not in p["name"]:
            seen.add((p["name"], p["block"]))

    for beams in (32, 129, 768, 769, 1025, 1088, 1089):
        for td in (112, 113, 514, 1026, 1536, 1538):                 # even / odd, 1 ... 3 loads per lane and beyond
            for dbg in (0, 4):
                plan(GLT, beams, td, lut_debug=dbg)
        for td in (112, 512, 514, 720):                               # table bins up to 256 and above
            for bins, tmin, search in itertools.product((0, 1), (32768, 1), (0, 1, 2)):
                plan(CDDT, beams, td, cddt_bins=bins, cddt_theta_min=tmin, cddt_search=search)
        for aux in (False, True):
            for variant in (0, 1):
                plan(BL, beams, aux=aux, variant=variant)
            plan(RMGPU, beams, aux=aux, variant=2)
            for kind in (RM, RMGPU):
                for tiled in (0, 1):
                    plan(kind, beams, aux=aux, variant=3, tiled=tiled)
    return seen


def test_the_other_table_is_what_the_planner_can_name():
    """OTHER's keys are exactly the (name, block) pairs the sweep sees; every launchable row plans its own key on its
    shape; a row that cites a test names one that exists and holds the instance's name."""
    seen = _other_sweep()
    assert seen == set(KI.OTHER), (sorted(seen - set(KI.OTHER)), sorted(set(KI.OTHER) - seen))
    for (name, block), row in KI.OTHER.items():
        if isinstance(row, str):
            path, test = row.split("::")
            text = open(os.path.join(ROOT, path)).read()
            assert "def %s(" % test in text and '"%s"' % name in text, row    # the cited test asserts this name
            continue
        cls, opts, aux, crash, td, beams, oracle = row
        assert not crash and oracle in ("lut_fan", "cddt_fan", "bl_fan", "rm_fan_libm")
        p = KI.plan_row(row, KI.O_SIDE, KI.O_SIDE, KI.O_POSES, beams, theta_disc=td)
        assert (p["name"], p["block"]) == (name, block), (name, block, p)
