"""The origin-corrected GiantLUT query (option ``lut_refine``) as tests/lut_refine_statement.py states it, on the CPU:
what it buys against exact ray marching, and the identities its contract names (include/scanlib.h).  The device is held
to the same statement bit for bit in tests/test_gpu_lut_refine.py."""
import numpy as np
import pytest

import lut_refine_statement as S
from oracle import np_statement as N
from pyracecarsimulator_amd import maps

FOV, BEAMS, TD, MRX = 4.71, 1081, 1442, 200
SEED = 3                                   # of both pose sets (the near-wall set's census below holds for it)


@pytest.fixture(scope="module")
def world(oracle_mod):
    g = maps.make_maze(192, cell=24, wall=2, seed=7)
    om = oracle_mod.OracleMap.from_gridmap(g, MRX)
    lut = om.lut_build(TD, nthreads=oracle_mod.max_threads())
    sets = {"clear": maps.sample_free_poses(g, 128, SEED, 2.0, dt=om.dt),          # clearance >= 2 cells
            "wall": S.near_wall_poses(g, om.dt, 256, SEED, 1.5)}                   # hugging a wall: dt <= 1.5
    return g, om, lut, sets


def refined_fan(g, om, lut, poses, fov=FOV, beams=BEAMS):
    return S.lut_refine_fan(lut, om.dt, g.resolution, g.origin, MRX, poses, fov, beams)


def error_stats(got, exact, res):
    e = np.abs(got.astype(np.float64) - exact.astype(np.float64)) / res
    return float(np.median(e)), float(np.percentile(e, 90)), float(np.percentile(e, 99)), float((e <= 1.0).mean())


def test_statement_against_exact_ray_marching(world):
    """Cells against exact ray marching (rm_fan, step coefficient 1.0), median / p90 / p99 / within one cell.  Measured:
        clear   default 0.633 / 1.44 / 25.3 / 0.780     refined 0.011 / 0.83 /  3.0 / 0.969
        wall    default 0.607 / 1.75 / 27.8 / 0.758     refined 0.080 / 0.94 / 15.0 / 0.924"""
    g, om, lut, sets = world
    stats = {}
    for name, poses in sets.items():
        exact = om.rm_fan(poses, FOV, BEAMS, step_coeff=1.0, want_hits=False, want_steps=False)[0]
        default = om.lut_fan(lut, poses, FOV, BEAMS)
        stats[name] = (error_stats(default, exact, g.resolution), error_stats(refined_fan(g, om, lut, poses), exact, g.resolution))
        print("%-5s default %.3f / %.2f / %.1f / %.3f   refined %.3f / %.2f / %.1f / %.3f" % ((name,) + stats[name][0] + stats[name][1]))
    for name, (d, r) in stats.items():
        assert r[3] >= d[3] + 0.10, (name, "within one cell", d[3], r[3])
        assert r[0] <= 0.3, (name, "median", r[0])
    d, r = stats["clear"]
    assert r[2] < d[2], ("clear p99", d[2], r[2])


def test_integer_poses_in_free_cells_equal_the_default(world):
    g, om, lut, _ = world
    poses = S.integer_poses(g, om.dt, 48, 11)
    gx, gy, _ = N._pose_grid(g.resolution, g.origin, poses)
    assert (gx == np.rint(gx)).all() and (gy == np.rint(gy)).all() and (om.dt[gy.astype(int), gx.astype(int)] > 0).all()
    want = N.lut_fan(lut, g.occ.shape, g.resolution, g.origin, MRX, poses, FOV, BEAMS)
    got = refined_fan(g, om, lut, poses)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_wall_and_miss_entries_pass_through_and_the_range_is_bounded(world):
    g, om, lut, sets = world
    q = np.array([0, 65535, 0, 65535, 1, 65534], np.uint16)
    f = np.array([0.9, 0.9, -0.5, -0.5, 0.9, -0.5], np.float32)
    one = np.ones(6, np.float32)
    out = S._correct(q, f, f, one, one, np.float32(MRX), np.float32(g.resolution))
    deq = np.float32(np.float32(MRX) / np.float32(65535.0))
    plain = ((q.astype(np.float32) * deq).astype(np.float32) * np.float32(g.resolution)).astype(np.float32)
    assert np.array_equal(out[:4], plain[:4])                # 0 and 65535 untouched ...
    assert out[4] == 0.0 and out[5] == np.float32(MRX) * np.float32(g.resolution)      # ... their neighbours clamped
    top = np.float32(np.float32(MRX) * np.float32(g.resolution))
    for poses in sets.values():
        r = refined_fan(g, om, lut, poses)
        assert (r >= 0).all() and (r <= top).all()
    # a fan in a table of misses and of walls alone: the default's bits wherever the pose sits in its cell
    for fill in (0, 65535):
        flat = np.full_like(lut, fill)
        p = sets["wall"][:16]
        assert np.array_equal(S.lut_refine_fan(flat, om.dt, g.resolution, g.origin, MRX, p, FOV, 64),
                              N.lut_fan(flat, g.occ.shape, g.resolution, g.origin, MRX, p, FOV, 64))


def test_corner_rule_at_the_map_border():
    """gx in [cols - 0.5, cols) rounds to the corner `cols`, which no cell owns: the last column's corner is taken and
    fx lies in [0.5, 1); the same for rows.  Ties round to even.  A free map, so that no fallback interferes."""
    dt = np.ones((8, 12), np.float32)
    gx = np.array([11.5, 11.75, 11.999, 3.0, 0.5, 1.5, 2.5, 0.0], np.float32)
    gy = np.array([7.5, 2.25, 7.999, 7.75, 0.5, 1.5, 2.5, 0.25], np.float32)
    inb, c, r, fx, fy, _, _ = S.corner(dt, gx, gy)
    assert inb.all()
    assert c.tolist() == [11, 11, 11, 3, 0, 2, 2, 0]
    assert r.tolist() == [7, 2, 7, 7, 0, 2, 2, 0]
    assert np.array_equal(fx, (gx - c.astype(np.float32)).astype(np.float32)) and fx[0] == 0.5 and fx[1] == 0.75
    assert (fx >= -0.5).all() and (fx < 1).all() and (fy >= -0.5).all() and (fy < 1).all()
    assert fx[5] == -0.5 and fx[6] == 0.5 and fx[4] == 0.5          # 1.5 -> 2, 2.5 -> 2, 0.5 -> 0
    # an occupied nearest corner: the pose keeps its own cell's
    dt[3, 5] = 0.0
    inb, c, r, fx, fy, took, fell = S.corner(dt, np.array([4.75, 4.25], np.float32), np.array([2.75, 2.75], np.float32))
    assert (c.tolist(), r.tolist()) == ([4, 4], [2, 3]) and fell.tolist() == [True, False] and took.tolist() == [False, True]
    # outside the map: no cell is read (index 0), whatever the coordinates
    inb, c, r, _, _, _, _ = S.corner(dt, np.array([-0.25, 12.0, np.nan], np.float32), np.array([1.0, 1.0, 1.0], np.float32))
    assert not inb.any() and c.tolist() == [0, 0, 0]


def test_both_corner_outcomes_occur_near_walls(world):
    g, om, _, sets = world
    took, fell = S.census(om.dt, g.resolution, g.origin, sets["wall"])
    print("near-wall set: %d poses take another cell's corner, %d fall back" % (took, fell))
    assert took >= 20 and fell >= 20
    assert S.census(om.dt, g.resolution, g.origin, sets["clear"])[1] == 0


def test_repeat_angles_of_the_fan_are_the_fan_and_rows_are_single_beams(world):
    g, om, lut, sets = world
    p = sets["wall"][:24]
    fan = S.lut_refine_fan(lut, om.dt, g.resolution, g.origin, MRX, p, FOV, 65)
    again = S.lut_refine_angles(lut, om.dt, g.resolution, g.origin, MRX, p, N._fan_alpha(FOV, 65))
    assert np.array_equal(fan, again)
    # a row (x, y, theta): the beam at angle 0 of a pose, with the direction det_sincosf(thg) itself — within an ulp of
    # the composed direction's result, and the same corner
    rows = S.lut_refine_rays(lut, om.dt, g.resolution, g.origin, MRX, p)
    zero = S.lut_refine_angles(lut, om.dt, g.resolution, g.origin, MRX, p, np.zeros(1, np.float32))
    assert np.abs(rows - zero).max() <= 1e-5 * g.resolution * MRX
