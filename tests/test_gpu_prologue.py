"""The stream kernel's prologue — the tables and the per-block pose records every workgroup of an INLINE launch puts
into LDS before its first sample — against the oracle, bit for bit, at the shapes where it takes another path: every
record source the planner reaches (records derived in place, the band list compacted per workgroup, pose ids from the
keys-only tile order), batches with fewer blocks than lanes (1 and 17 poses), a band whose last run of blocks ends
inside a pose and beyond the band, a workgroup with more blocks than lanes (the rounds behind the first), each through
the canonical and the code-map march, the upstream-literal variant and the fused crash test.  The map, the poses and
their NaN / far / edge members are the census of tests/kernel_instances.py; the oracle scans them once."""
import numpy as np
import pytest

import kernel_instances as KI
from pyracecarsimulator_amd import range_libc
from support import THRESH, same_bits

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

#: record source (rl_launch_plan) -> the options that make the planner take it on the census map (640 KB of float32
#: cells: "small", so the records are derived in place unless the small-map bound is taken away)
SOURCES = {1: {}, 2: {"inline_map_kb": 0}, 3: {"inline_map_kb": 0, "stripe_max": 0}}
#: march -> (class, options, fused crash test)
MODES = {"canonical": ("PyRayMarchingGPU", {"variant": 1}, False),
         "code": ("PyRayMarchingGPU", {"variant": 1, "code_map": 2, "code_min_rays": 0}, False),
         "literal": ("PyRayMarching", {}, False),
         "crash": ("PyRayMarchingGPU", {"variant": 1}, True)}
#: pose ranges of the census batch: all of it; one pose; 17 poses (17 x 17 blocks: fewer than a workgroup's lanes) with
#: the NaN pose; 100 poses with the far and the edge pose — 8 bands of 12 or 13 poses, 204 or 221 blocks each, in runs
#: of 8 blocks: no band is a whole number of runs and a pose's 17 blocks never are
BATCHES = {"all": (0, KI.POSES), "one": (5, 6), "seventeen": (1, 18), "boundary": (120, 220)}
BOUNDARY_RUN_LOG2 = 3
#: more blocks than lanes: 64 workgroups of 1024 lanes at grid_mult 1, 65-beam fans (two blocks per pose, the second
#: holding one ray)
ROUNDS_POSES, ROUNDS_BEAMS = 33000, 65


@pytest.fixture(scope="module")
def census(oracle_mod):
    g = KI.census_map()
    om = oracle_mod.OracleMap.from_gridmap(g, KI.MAX_RANGE)
    poses = KI.census_poses(g, om.dt)
    nt = oracle_mod.max_threads()
    want = {"PyRayMarchingGPU": om.rm_fan(poses, KI.FOV, KI.BEAMS, step_coeff=1.0, nthreads=nt, want_hits=False,
                                          want_steps=False)[0],
            "PyRayMarching": om.rm_fan_libm(poses, KI.FOV, KI.BEAMS, step_coeff=0.999)[0]}
    for v in want.values():
        v.setflags(write=False)
    omap = range_libc.PyOMap(g)
    assert np.array_equal(omap.distance_transform(), om.dt)
    return dict(g=g, om=om, omap=omap, poses=poses, want=want, edge=KI.census_edge(), oracle=oracle_mod)


def _method(census, cls, opts):
    m = getattr(range_libc, cls)(census["omap"], KI.MAX_RANGE)
    for k, v in dict(grid_mult=1, slots=2, **opts).items():
        m.set_option(k, v)
        assert m.get_info(k) == v, (k, v)
    return m


def _check(census, m, cls, crash, poses, want, beams, source, edge):
    got = np.full(want.size, -7.0, np.float32)
    if crash:
        first = m.check_collision_many(poses, KI.FOV, beams, edge, THRESH, ranges=got)
        assert first == census["oracle"].is_crashed(want, beams, len(poses), edge, THRESH)
    else:
        m.calc_range_fan(poses, got, KI.FOV, beams)
    pl = m.last_plan()
    assert pl["record_source"] == source and pl["block"] == 1024 and pl["slots"] == 2, pl
    assert pl["kernel"] == ("rm_stream_literal" if cls == "PyRayMarching" else "rm_stream"), pl
    assert pl["crash"] == int(crash), pl
    assert same_bits(got, want), (pl["name"], int((got != want).sum()))
    return pl


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("source", list(SOURCES))
@pytest.mark.parametrize("batch", list(BATCHES))
def test_prologue_records_equal_the_oracle(census, batch, source, mode):
    cls, opts, crash = MODES[mode]
    lo, hi = BATCHES[batch]
    opts = dict(opts, **SOURCES[source])
    if batch == "boundary":
        opts["run_log2"] = BOUNDARY_RUN_LOG2
        if source != 1:
            opts["inline_max"] = 0                    # (below 512 poses the records are derived in place on any map)
    # (batches below 64 poses are one band: nothing to compact or to order, the records are derived in place)
    expect = source if hi - lo >= 64 else 1
    m = _method(census, cls, opts)
    pl = _check(census, m, cls, crash, census["poses"][lo:hi], census["want"][cls][lo * KI.BEAMS:hi * KI.BEAMS], KI.BEAMS,
                expect, census["edge"])
    if mode == "code":
        assert pl["code"] == 2 and pl["code_entries"] == KI.PALETTE, pl
    if batch == "boundary":
        assert pl["run_log2"] == BOUNDARY_RUN_LOG2 and pl["bands"] > 1, pl
    if batch in ("one", "seventeen"):
        assert KI.plan_blocks(pl, hi - lo, KI.BEAMS) < pl["block"]
    m.close()


@pytest.mark.parametrize("mode", ["canonical", "crash"])
def test_prologue_rounds_behind_the_first_equal_the_oracle(census, mode):
    """More blocks per workgroup than lanes: the records of the blocks past the first 1024 are made in rounds."""
    cls, opts, crash = MODES[mode]
    g, om = census["g"], census["om"]
    poses = KI.census_poses(g, om.dt, ROUNDS_POSES)
    want = om.rm_fan(poses, KI.FOV, ROUNDS_BEAMS, step_coeff=1.0, nthreads=census["oracle"].max_threads(),
                     want_hits=False, want_steps=False)[0]
    m = _method(census, cls, opts)
    pl = _check(census, m, cls, crash, poses, want, ROUNDS_BEAMS, 1, KI.census_edge(ROUNDS_BEAMS))
    assert KI.plan_blocks(pl, ROUNDS_POSES, ROUNDS_BEAMS) > pl["grid"] * pl["block"], pl
    m.close()
