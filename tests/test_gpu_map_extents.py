"""Every map and range kernel at rl_map_create's limit of 16384 cells per side (run with -m gpu on the MI355X box).

What changes with the map extent and not with the pose batch — the dynamic LDS of edt_rows_kernel (cols * 4 bytes: 48 KiB
at 12288 columns, 64 KiB at 16384) and of cddt_project_kernel (8 bytes per bucket of the widest bin: the opt-in branch
above 48 KiB, the refusal above 150 KiB), edt_cols_kernel's 16 row segments, the packed (row << 16 | col) coordinates of
the edge list and the outline cells, tile_key's 16-bit tile columns, the bit map's word stride and gridDim.y, hit cells
up to 16383, sample counts in the thousands, float32 grid coordinates at 2^14 — on thin maps (tests/map_extents.py) that
keep it cheap.  Every comparison is bit for bit against the CPU oracle; tests/test_map_extents_host.py shows with the
oracle alone that the inputs reach what they are meant to reach."""
import time

import numpy as np
import pytest

import map_extents as X
import race_statement as RS
import support
from noise_checks import SEED_HI, check_noise
from support import same_bits
from pyracecarsimulator_amd import _lib, maps, range_libc
from pyracecarsimulator_amd import racecar as RC

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

RL_ERR_UNSUPPORTED = -4                       # include/scanlib.h rl_status
MRXS = (X.MRX_NEAR, X.MRX_FAR)

# the stream kernel's schedules that depend on the map's tile grid (defaults first)
SCHEDULES = [
    {},
    {"inline_map_kb": 0, "stripe_max": 0},                  # keys-only binning launch + records derived in the march
    {"inline_map_kb": 0, "inline_max": 0},                  # stripe bands compacted inside the march kernel
    {"inline_prep": 0, "bin_multi_min": 64},                # grid-wide binning kernels
    {"tiled": 0},                                           # row-major padded EDT
    {"slots": 2, "code_map": 2, "code_min_rays": 0},        # u16 palette codes
    {"tile_stripe": 0},                                     # binning tiles row-major
    {"tile_stripe": 1},
    {"tile_stripe": 4096},                                  # more rows than the map has tiles
    {"tile_stripe": 1, "inline_prep": 0},                   # ... behind the binning launch
    {"tile_stripe": 4096, "inline_prep": 0, "bin_multi_min": 64},
]


_CACHE = {}


def _grid(name):
    if ("g", name) not in _CACHE:
        _CACHE["g", name] = maps.GridMap(X.occupancy(name), X.RES, X.ORIGIN, name)
    return _CACHE["g", name]


def _oracle(oracle_mod, name, mrx):
    """(grid, OracleMap, poses) of a map and a range window, made once."""
    if ("om", name, mrx) not in _CACHE:
        g = _grid(name)
        om = oracle_mod.OracleMap.from_gridmap(g, mrx)
        _CACHE["om", name, mrx] = (g, om, X.poses(g, om.dt, name))
    return _CACHE["om", name, mrx]


def _ref(oracle_mod, name, mrx, what):
    """The oracle's (ranges, hit cells, steps) of the map's poses, computed once and shared."""
    key = ("ref", name, mrx, what)
    if key not in _CACHE:
        g, om, p = _oracle(oracle_mod, name, mrx)
        _CACHE[key] = {"rm": lambda: om.rm_fan(p, X.FOV, X.BEAMS, step_coeff=1.0, nthreads=8),
                       "rm_libm": lambda: om.rm_fan_libm(p, X.FOV, X.BEAMS, step_coeff=0.999),
                       "bl": lambda: om.bl_fan(p, X.FOV, X.BEAMS, nthreads=8)}[what]()
        for a in _CACHE[key]:
            a.setflags(write=False)
    return _CACHE[key]


def _fan(m, poses, aux):
    n = len(poses) * X.BEAMS
    out = np.full(n, -7.0, np.float32)
    if not aux:
        m.calc_range_fan(poses, out, X.FOV, X.BEAMS)
        return out, None, None
    hits = np.full((n, 2), -7, np.int32)
    steps = np.full(n, 7, np.uint16)
    m.calc_range_fan(poses, out, X.FOV, X.BEAMS, hit_cells=hits, steps=steps)
    return out, hits, steps


def _check_fan(m, poses, want, what):
    r, h, s = _fan(m, poses, True)
    r0, h0, s0 = want
    assert same_bits(r, r0), (what, "ranges", int((r != r0).sum()), m.last_plan())
    assert same_bits(h, h0), (what, "hit cells", int((h != h0).any(axis=1).sum()), m.last_plan())
    assert same_bits(s, s0), (what, "steps", int((s != s0).sum()), m.last_plan())
    r1 = _fan(m, poses, False)[0]                                   # the ranges-only launch
    assert same_bits(r1, r0), (what, "ranges only", int((r1 != r0).sum()), m.last_plan())


# ---------------------------------------------------------------- 1. EDT
@pytest.mark.parametrize("name", X.EDT_MAPS)
def test_edt_bit_equal_to_the_oracle(oracle_mod, name):
    occ = X.occupancy(name)
    omap = range_libc.PyOMap(occ, X.RES, origin=X.ORIGIN)          # (edt_rows_kernel: cols * 4 bytes of dynamic LDS)
    assert same_bits(omap.distance_transform(), oracle_mod.edt(occ)), name
    occ2 = X.far_block(occ)
    omap.update(occ2)
    assert same_bits(omap.distance_transform(), oracle_mod.edt(occ2)), (name, "update")
    idx = X.far_stamp(occ2)
    occ3 = occ2.copy()
    occ3.reshape(-1)[idx[idx < occ2.size]] = 1
    assert (occ3 != occ2).any()
    omap.stamp_cells(idx)
    assert same_bits(omap.distance_transform(), oracle_mod.edt(occ3)), (name, "stamp")
    omap.stamp_cells(np.zeros(0, np.int64))                         # back to the base map
    assert same_bits(omap.distance_transform(), oracle_mod.edt(occ2)), (name, "stamp lifted")
    omap.close()


# ---------------------------------------------------------------- 2. ray marching
@pytest.mark.parametrize("mrx", (X.MRX_NEAR, X.MRX_RM_FAR))
@pytest.mark.parametrize("name", X.RAY_MAPS + X.THIN_MAPS)
def test_ray_marching_bit_equal_to_the_oracle(oracle_mod, name, mrx):
    g, om, poses = _oracle(oracle_mod, name, mrx)
    omap = range_libc.PyOMap(g)
    m = range_libc.PyRayMarchingGPU(omap, mrx)
    m.set_option("variant", 0)                                      # the chunk kernel
    _check_fan(m, poses, _ref(oracle_mod, name, mrx, "rm"), (name, mrx, "RMGPU variant 0"))
    m.close()
    plans = set()
    fits = _lib.plan_fan(_lib.RL_RM_GPU, g.rows, g.cols, len(poses), X.BEAMS, max_range_px=mrx)["tiled"]
    assert fits or mrx == X.MRX_RM_FAR
    for cls, ref in ((range_libc.PyRayMarchingGPU, "rm"), (range_libc.PyRayMarching, "rm_libm")):
        for opts in SCHEDULES:
            m = cls(omap, mrx)                                      # RMGPU: variant 1; RM: the upstream-literal variant 3
            assert m.get_info("variant") == (1 if ref == "rm" else 3)
            for k, v in opts.items():
                m.set_option(k, v)
                assert m.get_info(k) == v
            _check_fan(m, poses, _ref(oracle_mod, name, mrx, ref), (name, mrx, cls.__name__, opts))
            pl = m.last_plan()
            if ref == "rm":
                assert pl["kernel"] == "rm_stream", pl
                # (where the tiled step map's geometry does not fit the window every schedule falls back to row-major)
                assert pl["tiled"] == (opts.get("tiled", 1) if fits else 0), pl
                plans.add((pl["binning"], pl["record_source"]))
            else:
                # (the literal arithmetic rides the stream kernel on the tiled map only; else one lane per ray)
                assert pl["kernel"] in ("rm_stream_literal", "rm_literal"), pl
                assert mrx != X.MRX_NEAR or opts or pl["kernel"] == "rm_stream_literal", pl
            m.close()
    assert len(plans) >= 4, plans                                   # the schedules did take different binning paths
    omap.close()


@pytest.mark.parametrize("cls", [range_libc.PyRayMarchingGPU, range_libc.PyRayMarching])
def test_ray_marching_refuses_a_window_whose_step_map_passes_2_30_cells(cls):
    """The step map is the EDT padded by the range window on every side, addressed in 32 bits: 17000 cells around a
    16384-cell map are 1.7e9 cells.  RL_ERR_UNSUPPORTED from every call, and the map goes on serving other handles."""
    g = _grid("wide")
    assert X.step_map_cells(g.rows, g.cols, X.MRX_FAR) >= 2 ** 30
    omap = range_libc.PyOMap(g)
    m = cls(omap, X.MRX_FAR)
    poses = X.special_poses("wide")[4:6]
    out = np.full(2 * X.BEAMS, -7.0, np.float32)
    for call in range(2):
        with pytest.raises(_lib.ScanLibError) as e:
            m.calc_range_fan(poses, out, X.FOV, X.BEAMS)
        assert e.value.code == RL_ERR_UNSUPPORTED and "too large for the step map" in str(e.value), str(e.value)
        assert (out == -7.0).all()
    m.close()
    m = cls(omap, X.MRX_NEAR)
    m.calc_range_fan(poses, out, X.FOV, X.BEAMS)
    assert (out >= 0.0).all() and (out <= 15.1).all()
    m.close()
    omap.close()


# ---------------------------------------------------------------- 3. Bresenham
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("mrx", MRXS)                               # 17000: no LDS window: the global bit map, 512-word stride
@pytest.mark.parametrize("name", X.RAY_MAPS)
def test_bresenham_bit_equal_to_the_oracle(oracle_mod, name, mrx, variant):
    g, om, poses = _oracle(oracle_mod, name, mrx)
    omap = range_libc.PyOMap(g)
    m = range_libc.PyBresenhamsLine(omap, mrx)
    m.set_option("variant", variant)
    _check_fan(m, poses, _ref(oracle_mod, name, mrx, "bl"), (name, mrx, "Bresenham", variant))
    assert m.last_plan()["kernel"] == ("bl_stream" if variant else "bl_lds"), m.last_plan()
    ins = X.ray_rows(poses, 3000, 3)
    outs = np.full(len(ins), -7.0, np.float32)
    m.calc_range_many(ins, outs)
    assert same_bits(outs, om.bl_rays(ins)[0]), (name, mrx, variant, "rays")
    m.close()
    omap.close()


# ---------------------------------------------------------------- 4. CDDT
def _cddt_paths(m, poses, want, what):
    """The per-bin and the per-ray fan kernel, and the theta-major pair with each of its searches."""
    for bins in (1, 0):
        m.set_option("cddt_bins", bins)
        out = np.full(len(poses) * X.BEAMS, -7.0, np.float32)
        m.calc_range_fan(poses, out, X.FOV, X.BEAMS)
        assert m.last_plan()["kernel"] == ("cddt_bins" if bins else "cddt_rays"), m.last_plan()
        assert same_bits(out, want), (what, "cddt_bins", bins, int((out != want).sum()))
    m.set_option("cddt_bins", 1)
    m.set_option("cddt_theta_min", 1)
    for search in (1, 0, 2):
        m.set_option("cddt_search", search)
        out = np.full(len(poses) * X.BEAMS, -7.0, np.float32)
        m.calc_range_fan(poses, out, X.FOV, X.BEAMS)
        assert m.last_plan()["kernel"] == "cddt_theta", m.last_plan()
        assert same_bits(out, want), (what, "theta-major", search, int((out != want).sum()))
    m.set_option("cddt_search", 1)
    m.set_option("cddt_theta_min", 32768)


@pytest.mark.parametrize("order", [("cddt6100", "cddt6200"), ("cddt6200", "cddt6100")])
def test_cddt_builds_either_side_of_48_kib_in_either_order(oracle_mod, order):
    """cddt_project_kernel's dynamic LDS: 49 608 bytes (the build sets the function attribute, which stays set) and
    48 808 bytes (it does not), one build after the other in one process, both orders.  6100 first: run alone, that
    build and the rebuild at the end see the attribute never set and set by another map's build."""
    td = 112
    fills = [X.cddt_lds_fill(*X.SHAPES[n][:2], td, oracle_mod.sincosf) for n in order]
    assert sorted(fills) == [48808, 49608] and min(fills) < X.LDS_DEFAULT < max(fills)
    keep = []
    for name in order:
        g, om, poses = _oracle(oracle_mod, name, X.MRX_NEAR)
        omap = range_libc.PyOMap(g)
        m = range_libc.PyCDDTCast(omap, X.MRX_NEAR, td)
        out = np.full(len(poses) * X.BEAMS, -7.0, np.float32)
        m.calc_range_fan(poses, out, X.FOV, X.BEAMS)
        assert same_bits(out, om.cddt_fan(td, poses, X.FOV, X.BEAMS, nthreads=8)), (order, name)
        keep.append((omap, m, g, om, poses))
    # a rebuild of the first one after the second has been built
    omap, m, g, om, poses = keep[0]
    occ2 = X.long_wall(g.occ)
    omap.update(occ2)
    om2 = oracle_mod.OracleMap(occ2, g.resolution, g.origin, X.MRX_NEAR)
    out = np.full(len(poses) * X.BEAMS, -7.0, np.float32)
    m.calc_range_fan(poses, out, X.FOV, X.BEAMS)
    assert same_bits(out, om2.cddt_fan(td, poses, X.FOV, X.BEAMS, nthreads=8)), (order, "rebuild")
    for omap, m, *_ in keep:
        m.close()
        omap.close()


@pytest.mark.parametrize("td", X.CDDT_THETA)
@pytest.mark.parametrize("name", X.CDDT_LONG + X.CDDT_PAIR)
def test_cddt_bit_equal_to_the_oracle(oracle_mod, name, td):
    rows, cols, _ = X.SHAPES[name]
    fill = X.cddt_lds_fill(rows, cols, td, oracle_mod.sincosf)
    if name in X.CDDT_LONG:
        assert 128 * 1024 <= fill <= X.CDDT_LDS_MAX                 # the opt-in branch, 131 KiB
    else:
        assert (fill > X.LDS_DEFAULT) == (name == "cddt6200")
    g = _grid(name)
    omap = range_libc.PyOMap(g)
    for mrx in MRXS:
        _, om, poses = _oracle(oracle_mod, name, mrx)
        m = range_libc.PyCDDTCast(omap, mrx, td)
        want = om.cddt_fan(td, poses, X.FOV, X.BEAMS, nthreads=8)
        _cddt_paths(m, poses, want, (name, td, mrx))
        ins = X.ray_rows(poses, 5000, td)
        outs = np.full(len(ins), -7.0, np.float32)
        m.calc_range_many(ins, outs)
        assert same_bits(outs, om.cddt_rays(td, ins, nthreads=8)), (name, td, mrx, "rays")
        if mrx == X.MRX_FAR:
            # after a map change with a new long wall (thousands of values in one bucket) the rebuilt table follows
            occ2 = X.long_wall(g.occ)
            omap.update(occ2)
            om2 = oracle_mod.OracleMap(occ2, g.resolution, g.origin, mrx)
            want2 = om2.cddt_fan(td, poses, X.FOV, X.BEAMS, nthreads=8)
            assert not same_bits(want2, want)
            out = np.full(len(poses) * X.BEAMS, -7.0, np.float32)
            m.calc_range_fan(poses, out, X.FOV, X.BEAMS)
            assert same_bits(out, want2), (name, td, "after update", int((out != want2).sum()))
            m.calc_range_many(ins, outs)
            assert same_bits(outs, om2.cddt_rays(td, ins, nthreads=8)), (name, td, "rays after update")
            omap.update(g.occ)
        m.close()
    omap.close()


# ---------------------------------------------------------------- 5. GiantLUT
@pytest.mark.parametrize("mrx", MRXS)
@pytest.mark.parametrize("name", X.LUT_MAPS)
def test_giant_lut_bit_equal_to_the_oracle(oracle_mod, name, mrx):
    rows, cols, _ = X.SHAPES[name]
    g, om, poses = _oracle(oracle_mod, name, mrx)
    omap = range_libc.PyOMap(g)
    m = range_libc.PyGiantLUTCast(omap, mrx, X.LUT_THETA)
    lut = om.lut_build(X.LUT_THETA, nthreads=oracle_mod.max_threads())
    assert same_bits(m.table(), lut), (name, mrx, "table")
    assert same_bits(m.table(rows - 1, rows), lut[rows - 1:]), (name, mrx, "last row of the table")
    # the table's last cell (inside the border wall) and the last free cell next to it
    poses = np.concatenate([poses, X.to_world(cols - 0.5, rows - 0.5, 0.3), X.to_world(cols - 1.5, rows - 1.5, -2.0)])
    cell = om.lut_pose_cells(poses[-2:])
    assert (int(cell[0][0]), int(cell[1][0])) == (rows - 1, cols - 1)
    out = np.full(len(poses) * X.BEAMS, -7.0, np.float32)
    m.calc_range_fan(poses, out, X.FOV, X.BEAMS)
    assert same_bits(out, om.lut_fan(lut, poses, X.FOV, X.BEAMS, nthreads=8)), (name, mrx, "fan")
    ins = X.ray_rows(poses, 5000, 5)
    ins[:2, :2] = poses[-2:, :2]
    outs = np.full(len(ins), -7.0, np.float32)
    m.calc_range_many(ins, outs)
    assert same_bits(outs, om.lut_rays(lut, ins)), (name, mrx, "rays")
    m.close()
    omap.close()


# ---------------------------------------------------------------- 6. the CDDT refusal
def test_cddt_refuses_a_map_whose_widest_bin_passes_the_lds_histogram(oracle_mod):
    """10400 x 16384: the diagonal bins are 19 400 buckets wide, 155 KiB of histogram: RL_ERR_UNSUPPORTED from the first
    call, the same from the second, a clean close and a device that still answers."""
    assert X.cddt_lds_fill(*X.REFUSED, 112, oracle_mod.sincosf) > X.CDDT_LDS_MAX
    t0 = time.time()
    omap = range_libc.PyOMap(X.refused_occupancy(), X.RES, origin=X.ORIGIN)
    m = range_libc.PyCDDTCast(omap, X.MRX_NEAR, 112)
    poses = X.to_world([100.5, 9000.25], [50.5, 7000.5], 0.4)
    out = np.full(2 * X.BEAMS, -7.0, np.float32)
    for call in range(2):
        with pytest.raises(_lib.ScanLibError) as e:
            if call == 0:
                m.calc_range_fan(poses, out, X.FOV, X.BEAMS)
            else:
                m.calc_range_many(np.ascontiguousarray(poses), out[:2])
        assert e.value.code == RL_ERR_UNSUPPORTED, (call, str(e.value))
        assert "map too large for the LDS bucket histogram" in str(e.value), (call, str(e.value))
        assert (out == -7.0).all()
    m.close()
    omap.close()
    print("\nCDDT refusal on %d x %d: %.2f s" % (X.REFUSED + (time.time() - t0,)))
    small = np.zeros((33, 65), np.uint8)
    small[5, 7] = 1
    omap = range_libc.PyOMap(small, X.RES)
    assert same_bits(omap.distance_transform(), oracle_mod.edt(small))
    omap.close()


# ---------------------------------------------------------------- 7. races
L, W = RC.DEFAULT_CAR["length"], RC.DEFAULT_CAR["width"]


def _far_end_cars(n, seed, spread_across):
    """Cars within a car length (8 cells) of the far end of the 24 x 16384 map, some of them partly off the grid."""
    rows, cols, _ = X.SHAPES["wide"]
    rng = np.random.default_rng(seed)
    lo, hi = spread_across
    cars = X.to_world(cols - rng.uniform(-4.0, 8.0, n), rng.uniform(lo, hi, n)).astype(np.float64)
    cars[:, 2] = rng.uniform(-np.pi, np.pi, n)
    return cars


def test_outline_cells_at_the_far_end_equal_the_statement(oracle_mod):
    rows, cols, _ = X.SHAPES["wide"]
    g = _grid("wide")
    omap = range_libc.PyOMap(g)
    cars = _far_end_cars(400, 1, (-4.0, rows + 4.0))
    cells, counts = RC.CarBatch().outline_cells(omap, cars)
    want = RS.outline_cells(cars, L, W, g.resolution, g.origin, rows, cols, oracle_mod.sincosf)
    n_points = sum(RS.edge_counts(L, W, g.resolution)) * 2
    partly, last_col = 0, 0
    for i in range(len(cars)):
        got = cells[i, :counts[i]]
        assert (cells[i, counts[i]:] == -1).all()
        assert set(got.tolist()) == set(want[i].tolist()), i
        partly += 0 < len(want[i]) < n_points
        last_col += bool(len(want[i])) and int((want[i] % cols).max()) == cols - 1
    assert partly > 40 and last_col > 40, (partly, last_col)
    omap.close()


@pytest.mark.parametrize("kind", ["RMGPU", "RM"])
def test_fan_cars_at_the_far_end_equal_the_oracle_on_the_stamped_grid(oracle_mod, kind):
    rows, cols, _ = X.SHAPES["wide"]
    g = _grid("wide")
    mrx, group, nb = X.MRX_RM_FAR, 2, 360
    lo, hi = X.lane(rows)
    cars = _far_end_cars(8, 5, (lo - 2.0, hi + 3.0))
    cars[:, 0:2] = X.to_world(cols - np.linspace(3.0, 14.0, 8), np.tile([lo + 0.5, hi + 0.5], 4))[:, :2]
    cars[1::2, 2] = cars[0::2, 2] + np.pi
    # car 1 looks straight back down the corridor from the middle of the lane (beam nb / 2 is the heading itself)
    cars[1] = X.to_world(cols - 6.0, 0.5 * (lo + hi + 1), np.pi)[0]
    poses = support.lidar_poses(cars)
    omap = range_libc.PyOMap(g)
    m = (range_libc.PyRayMarching if kind == "RM" else range_libc.PyRayMarchingGPU)(omap, mrx)
    N = len(poses)
    hits = np.full((N * nb, 2), -7, np.int32)
    steps = np.full(N * nb, 7, np.uint16)
    outs = m.calc_range_fan_cars(poses, cars, group, X.FOV, nb, hit_cells=hits, steps=steps)
    cells = RS.outline_cells(cars, L, W, g.resolution, g.origin, rows, cols, oracle_mod.sincosf)
    assert all(len(c) for c in cells)
    for p in range(N):
        om = oracle_mod.OracleMap(RS.stamped(g.occ, RS.others(cells, group, p)), g.resolution, g.origin, mrx)
        if kind == "RM":
            r, h, s = om.rm_fan_libm(poses[p:p + 1], X.FOV, nb, step_coeff=0.999)
        else:
            r, h, s = om.rm_fan(poses[p:p + 1], X.FOV, nb, step_coeff=1.0)
        sl = slice(p * nb, (p + 1) * nb)
        assert same_bits(outs[sl], r) and same_bits(hits[sl], h) and same_bits(steps[sl], s), (kind, p)
    plain = np.empty(N * nb, np.float32)
    m.calc_range_fan(poses, plain, X.FOV, nb)
    changed = int((plain != outs).sum())
    assert changed > 20, changed                                   # the other car is in sight
    assert float(outs[nb + nb // 2]) == np.float32(mrx) * np.float32(X.RES)    # ... and car 1's middle beam runs out the window
    m.close()
    omap.close()


# ---------------------------------------------------------------- 8. noise
@pytest.mark.parametrize("method", ["RMGPU", "RM", "BL", "CDDT", "GLT"])
def test_noise_keyed_by_the_global_ray_id_across_2_32(oracle_mod, method):
    name = "wide"
    mrx = X.MRX_RM_FAR if method in ("RMGPU", "RM") else X.MRX_FAR
    g, om, poses = _oracle(oracle_mod, name, mrx)
    sub = np.ascontiguousarray(poses[np.r_[0:52, len(poses) - 12:len(poses)]])
    n = len(sub) * X.BEAMS
    omap = range_libc.PyOMap(g)
    if method == "RMGPU":
        m, want = range_libc.PyRayMarchingGPU(omap, mrx), om.rm_fan(sub, X.FOV, X.BEAMS, step_coeff=1.0, nthreads=8)[0]
    elif method == "RM":
        m, want = range_libc.PyRayMarching(omap, mrx), om.rm_fan_libm(sub, X.FOV, X.BEAMS, step_coeff=0.999)[0]
    elif method == "BL":
        m, want = range_libc.PyBresenhamsLine(omap, mrx), om.bl_fan(sub, X.FOV, X.BEAMS, nthreads=8)[0]
    elif method == "CDDT":
        m, want = range_libc.PyCDDTCast(omap, mrx, 112), om.cddt_fan(112, sub, X.FOV, X.BEAMS, nthreads=8)
    else:
        m = range_libc.PyGiantLUTCast(omap, mrx, X.LUT_THETA)
        want = om.lut_fan(om.lut_build(X.LUT_THETA, nthreads=oracle_mod.max_threads()), sub, X.FOV, X.BEAMS, nthreads=8)
    off = 2 ** 32 - n // 2
    assert off < 2 ** 32 < off + n
    check_noise(m, sub, X.FOV, X.BEAMS, want, SEED_HI, off, what=(method, name))
    m.close()
    omap.close()
