"""The inputs of tests/test_gpu_map_extents.py checked with the oracle alone (no GPU), so that a pass there means what
it claims: rays do run the length of the 16384-cell maps, hit cells reach both ends, the sample counts stay below the
uint16 ceiling, the table methods do not answer the maximum range everywhere, the two pairs of maps stand either side
of 48 KiB of dynamic LDS, and the launch planner has an answer for every map shape."""
import numpy as np
import pytest

import map_extents as X
from pyracecarsimulator_amd import _lib, maps


def _grid(name):
    return maps.GridMap(X.occupancy(name), X.RES, X.ORIGIN, name)


def test_shapes_are_what_the_table_says():
    assert X.SHAPES["wide"][:2] == (24, X.MAP_SIDE_MAX) and X.SHAPES["tall"][:2] == (X.MAP_SIDE_MAX, 24)
    assert X.SHAPES["row"][:2] == (1, X.MAP_SIDE_MAX) and X.SHAPES["column"][:2] == (X.MAP_SIDE_MAX, 1)
    # edt_rows_kernel: cols * 4 bytes of dynamic LDS
    assert X.SHAPES["lds48k"][1] * 4 == X.LDS_DEFAULT and X.SHAPES["lds48k+"][1] * 4 == X.LDS_DEFAULT + 4
    assert X.SHAPES["wide"][1] * 4 == 64 * 1024
    # edt_cols_kernel: 16 segments of ceil(rows / 16) rows; a one-row map leaves 15 of them empty
    assert -(-X.SHAPES["tall"][0] // 16) == 1024 and -(-X.SHAPES["row"][0] // 16) == 1
    # tiles of 8 columns, bit-map words of 32
    assert X.SHAPES["wide"][1] // 8 == 2048 and X.SHAPES["wide"][1] // 32 == 512
    assert X.SHAPES["odd"][1] == 8193 and X.SHAPES["odd"][1] % 8 and X.SHAPES["odd"][1] % 32
    assert set(X.EDT_MAPS) == set(X.SHAPES)
    for name, (rows, cols, kind) in X.SHAPES.items():
        occ = X.occupancy(name)
        assert occ.shape == (rows, cols) and occ.dtype == np.uint8 and occ.any() and not occ.all()
        assert np.array_equal(occ, X.occupancy(name))                              # seeded
        if kind == "corridor":
            short = min(rows, cols)
            lo, hi = X.lane(short)
            line = occ if cols >= rows else occ.T
            assert not line[lo:hi + 1, 1:-1].any() and line[:, 0].all() and line[:, -1].all()
            # the cross-walls are partial: from either side, never across the lane
            cross = np.flatnonzero(line[1:-1, 1:-1].any(axis=0))
            assert 30 <= len(cross) <= 2 * X.N_CROSS_WALLS
            assert line[1, 1:-1].any() and line[short - 2, 1:-1].any()
        # the mutations of the EDT test change cells at the far end of the long axis only
        far = np.argwhere(X.far_block(occ) != occ)
        assert len(far) and (far[:, X.long_axis(name)] >= max(rows, cols) - 40).all()
        idx = X.far_stamp(occ)
        assert ((idx >= occ.size - 100) | (idx < 0)).all() and (idx >= occ.size).sum() == 2 and (idx == occ.size - 1).any()


def test_the_column_map_needs_carries_across_many_segments():
    """edt_cols_kernel sweeps 16 row segments of 1024 rows in parallel and hands the last occupied row below / the first
    above from segment to segment: on 16384 x 1 thousands of cells have their nearest occupied cell several segments
    away, in the last segment for one group of them; after the update of the EDT test too."""
    for occ in (X.occupancy("column"), X.far_block(X.occupancy("column"))):
        rr = np.flatnonzero(occ[:, 0])
        r = np.arange(occ.shape[0])
        nxt = np.searchsorted(rr, r, side="left")
        above = np.where(nxt < len(rr), rr[np.minimum(nxt, len(rr) - 1)], 10 ** 6)
        below = np.where(nxt > 0, rr[np.maximum(nxt - 1, 0)], -10 ** 6)
        seg = r // 1024
        up = (above - r < r - below) & (above // 1024 - seg >= 2)
        down = (r - below < above - r) & (seg - below // 1024 >= 2)
        assert up.sum() > 2000 and down.sum() > 2000
        assert (up & (above // 1024 == 15)).sum() > 1500 and set(seg[up]) >= {12, 13} and set(seg[down]) >= {6, 11, 12}
    row = X.occupancy("row")                                    # the same layout along the columns
    assert row[0, :X.SPARSE_DENSE].sum() > 5 and np.flatnonzero(row[0, X.SPARSE_DENSE:]).tolist() == [
        k - X.SPARSE_DENSE for k in X.SPARSE_LONE]


def test_cddt_pairs_straddle_48_kib_and_the_long_maps_take_the_opt_in_branch(oracle_mod):
    sc = oracle_mod.sincosf
    for td in X.CDDT_THETA:
        lo = X.cddt_wmax(*X.SHAPES["cddt6100"][:2], td, sc)
        hi = X.cddt_wmax(*X.SHAPES["cddt6200"][:2], td, sc)
        assert (lo, hi) == (6101, 6201), (td, lo, hi)
        assert X.cddt_lds_fill(*X.SHAPES["cddt6100"][:2], td, sc) < X.LDS_DEFAULT < X.cddt_lds_fill(*X.SHAPES["cddt6200"][:2], td, sc)
        for name in X.CDDT_LONG:
            w = X.cddt_wmax(*X.SHAPES[name][:2], td, sc)
            assert 6144 < w <= 19200 and w >= X.MAP_SIDE_MAX, (name, td, w)
            assert X.LDS_DEFAULT < w * 8 <= X.CDDT_LDS_MAX and w * 8 >= 128 * 1024
        assert X.cddt_wmax(*X.REFUSED, td, sc) > 19200
        assert X.cddt_lds_fill(*X.REFUSED, td, sc) > X.CDDT_LDS_MAX
    # the formula against the one case worked by hand: a square map at theta_disc 4 (bins 0 and pi / 2)
    assert X.cddt_wmax(100, 100, 4, sc) == 101


@pytest.mark.parametrize("name", X.RAY_MAPS + X.CDDT_PAIR + X.LUT_MAPS)
def test_rays_run_the_length_of_the_map(oracle_mod, name):
    rows, cols, _ = X.SHAPES[name]
    length, ax = max(rows, cols), (0 if X.long_axis(name) else 1)       # hit cells are (col, row)
    g = _grid(name)
    far = oracle_mod.OracleMap.from_gridmap(g, X.MRX_FAR)
    rm_far = oracle_mod.OracleMap.from_gridmap(g, X.MRX_RM_FAR)
    p = X.poses(g, far.dt, name)
    assert len(p) == X.N_POSES + 12 and np.isnan(p[X.N_POSES]).any()
    for what, (r, h, s) in (("rm", rm_far.rm_fan(p, X.FOV, X.BEAMS, step_coeff=1.0, nthreads=8)),
                            ("rm_libm", rm_far.rm_fan_libm(p, X.FOV, X.BEAMS, step_coeff=0.999)),
                            ("bl", far.bl_fan(p, X.FOV, X.BEAMS, nthreads=8))):
        hit = h[:, 0] >= 0
        longest = float(r[hit].max()) / X.RES
        # a ray that crosses 2^13 cells where the map has them, all but the end of the lane elsewhere
        assert longest > (8192 if length == X.MAP_SIDE_MAX else length - 8), (name, what, longest)
        assert h[hit, ax].min() == 0 and h[hit, ax].max() == length - 1, (name, what)
        assert 1000 < int(s.max()) < 65535, (name, what, int(s.max()))
        assert 0.02 < hit.mean() < 1.0                                   # (the NaN and the outside pose hit nothing)
    near = oracle_mod.OracleMap.from_gridmap(g, X.MRX_NEAR)
    for what, r in (("rm", near.rm_fan(p, X.FOV, X.BEAMS, step_coeff=1.0, nthreads=8)[0]),
                    ("rm_libm", near.rm_fan_libm(p, X.FOV, X.BEAMS, step_coeff=0.999)[0]),
                    ("bl", near.bl_fan(p, X.FOV, X.BEAMS, nthreads=8)[0])):
        # nothing reaches past the 300-cell window: 15 m, and for a hit found by the window's last sample up to that
        # sample's overshoot (the oracle: 0.9 cell for the march, 2.1 cells for the walk's budget of mrx + 3 steps)
        assert 15.0 <= float(r.max()) <= 15.0 + 3 * X.RES, (name, what, float(r.max()))
        assert float(np.median(r)) < 5.0
    # the table methods do not answer the maximum range everywhere
    for om, mrx in ((near, X.MRX_NEAR), (far, X.MRX_FAR)):
        top = np.float32(mrx) * np.float32(X.RES)
        if name in X.CDDT_LONG + X.CDDT_PAIR:
            for td in X.CDDT_THETA:
                c = om.cddt_fan(td, p, X.FOV, X.BEAMS, nthreads=8)
                assert (c < top).mean() > 0.9 and len(np.unique(c)) > 1000, (name, td, mrx)
                if mrx == X.MRX_FAR:
                    # (112 has a table bin along either axis; the odd 113 has none along the rows, and its nearest bin
                    #  meets the side wall of the lane after some 1500 cells)
                    want = (8192 if length == X.MAP_SIDE_MAX else length - 8) if td == 112 else 1000
                    assert float(c[c < top].max()) / X.RES > want, (name, td)
        if name in X.LUT_MAPS:
            lut = om.lut_build(X.LUT_THETA)
            f = om.lut_fan(lut, p, X.FOV, X.BEAMS)
            assert (f < top).mean() > 0.9 and len(np.unique(f)) > 100, (name, mrx)
            assert lut.shape == (rows, cols, X.LUT_THETA)
            r_, c_ = om.lut_pose_cells(X.to_world(cols - 0.5, rows - 0.5, 0.3))
            assert (int(r_[0]), int(c_[0])) == (rows - 1, cols - 1)        # the pose of the table's last cell


def test_ray_marching_windows_either_side_of_the_step_map_limit():
    """The ray-marching handles answer RL_ERR_UNSUPPORTED for a step map of 2^30 cells or more: the far window the GPU
    tests march at fits on every map, the window the table methods and Bresenham run at does not, on any of them."""
    for name in X.RAY_MAPS + X.THIN_MAPS:
        rows, cols, _ = X.SHAPES[name]
        assert X.step_map_cells(rows, cols, X.MRX_RM_FAR) < 2 ** 30 <= X.step_map_cells(rows, cols, X.MRX_FAR), name
        assert cols + 2 * (X.MRX_FAR + 2) + 31 < 2 ** 23
    assert 8192 < 0.7 * X.MAP_SIDE_MAX < X.MRX_RM_FAR < X.MAP_SIDE_MAX
    # by hand: a 1 x 1 map at a window of 14 cells is 33 rows of 64 cells
    assert X.step_map_cells(1, 1, 14.0) == 33 * 64 and X.step_map_cells(1, 1, 13.5) == 33 * 64


def test_special_poses_land_where_they_are_meant_to(oracle_mod):
    for name in X.RAY_MAPS:
        rows, cols, _ = X.SHAPES[name]
        om = oracle_mod.OracleMap.from_gridmap(_grid(name), X.MRX_FAR)
        sp = X.special_poses(name)
        r_, c_ = om.lut_pose_cells(sp)                       # (row, col) of the cell a pose stands in, -1 outside
        assert (r_[0], c_[0]) == (-1, -1) and (r_[1], c_[1]) == (-1, -1) and (r_[2], c_[2]) == (-1, -1)
        last = (r_[3], c_[3])[X.long_axis(name)]
        assert last == max(rows, cols) - 1 and om.occ[r_[3], c_[3]]
        assert (r_[4:] >= 0).all() and not om.occ[r_[4:], c_[4:]].any()


@pytest.mark.parametrize("n", [64, 600, 9000])
def test_the_planner_answers_for_every_map_shape(n):
    kinds = {"RM": _lib.RL_RM, "RMGPU": _lib.RL_RM_GPU, "BL": _lib.RL_BRESENHAM, "CDDT": _lib.RL_CDDT,
             "GLT": _lib.RL_GIANT_LUT}
    for name, (rows, cols, _) in X.SHAPES.items():
        for mrx in (X.MRX_NEAR, X.MRX_FAR):
            for kind, k in kinds.items():
                td = {"CDDT": X.CDDT_THETA[0], "GLT": X.LUT_THETA}.get(kind, 0)
                for aux in (False, True):
                    if aux and kind in ("CDDT", "GLT"):
                        continue                                  # (the table methods have no diagnostics)
                    p = _lib.plan_fan(k, rows, cols, n, X.BEAMS, max_range_px=mrx, theta_disc=td, aux=aux)
                    what = (name, mrx, kind, n, aux, p)
                    assert p["grid"] >= 1 and p["block"] in (64, 256, 512, 1024), what
                    assert 0 <= p["lds_bytes"] <= 160 * 1024, what
                    assert p["name"].startswith("scan::"), what
                    assert p["slices"] >= 1 and p["slices"] * max(p["slice_poses"], 1) >= min(n, 1) , what
                    if kind in ("RM", "RMGPU") and p["tiled"]:
                        # tile_key keeps the tile columns in 16 bits
                        assert (cols + 7) // 8 <= 0xffff
