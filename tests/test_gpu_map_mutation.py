"""Map mutations under live method handles (run with -m gpu on the MI355X box).

``rl_map_update`` uploads a new grid and ``rl_map_stamp_cells`` lays an outline over the base grid (the two-player
tick).  Both rebuild the map-level tables at once; the larger tables of every method handle are rebuilt lazily when the
handle sees ``rl_map::epoch`` move.  Every check here compares the device with the oracle built on the mutated grid,
bit for bit, and first asserts that the oracle's answer on the new grid differs from its answer on the previous grid:
a handle that served a stale table would fail.  Each probe is called twice after a mutation (the first call rebuilds,
the second takes the cached tables).

tests/coverage_tables.py TABLE_CACHES names the case that covers each site under csrc/ that asks a table's cache whether
it is still good for the map (``fresh_for``); tests/test_host.py keeps it in step with the sources."""
import threading

import numpy as np
import pytest

import support
from table_cases import all_equal as _all_equal, cddt_ranges, rm_ranges
from pyracecarsimulator_amd import _lib, maps, range_libc

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

MRX, B, FOV, TD = 120, 256, 6.2, 112


def _dev_occ(omap):
    out = np.empty((omap.height, omap.width), np.uint8)
    _lib.check(_lib.lib().rl_map_get_occ(omap._h, out.ctypes.data_as(_lib.u8p)))
    return out


def _base_grid(rows, cols, seed):
    """A maze cropped to rows x cols with gaps in its border (so a stamped border is new) and two open corners."""
    occ = maps.make_maze(max(rows, cols), cell=24, wall=2, p=0.5, seed=seed).occ[:rows, :cols].copy()
    occ[0, :] = occ[-1, :] = 1
    occ[:, 0] = occ[:, -1] = 1
    g0 = max(4, cols // 4)
    occ[:6, g0:2 * g0] = 0                      # gap in the top border, open band inside it
    occ[-6:, -6:] = 0                           # open corner
    occ[g0:2 * g0, :6] = 0                      # gap in the left border
    return occ


def _open_center(occ, min_dt, avoid=()):
    """A free cell at least ``min_dt`` from every wall, away from the border and from the cells in ``avoid``."""
    from oracle import oracle as O
    dt = O.edt(occ)
    rows, cols = occ.shape
    rr, cc = np.nonzero(dt >= min_dt)
    ok = (rr > 12) & (rr < rows - 12) & (cc > 12) & (cc < cols - 12)
    for (ar, ac) in avoid:
        ok &= np.hypot(rr - ar, cc - ac) > 3 * min_dt
    assert ok.any(), "no open area"
    k = int(np.flatnonzero(ok)[len(np.flatnonzero(ok)) // 2])
    return int(rr[k]), int(cc[k])


def _rect_outline(r, c, hh, hw, rows, cols):
    """Flat indices of the outline of the rectangle rows r-hh..r+hh, cols c-hw..c+hw."""
    cells = set()
    for dr in range(-hh, hh + 1):
        for dc in range(-hw, hw + 1):
            if abs(dr) == hh or abs(dc) == hw:
                cells.add((r + dr) * cols + (c + dc))
    return np.array(sorted(cells), np.int64)


def _script(rows, cols, seed, h):
    """The mutation script: [(label, ("stamp", idx, value) | ("update", occ), expected grid)], the base grids and
    the grid cells of the focus poses (inside each outline, next to the border gaps)."""
    rng = np.random.default_rng(seed)
    base0 = _base_grid(rows, cols, seed)
    base1 = _base_grid(rows, cols, seed + 100)
    ca = _open_center(base0, h + 2)
    cb = _open_center(base1, h + 2, avoid=[ca])
    out_a = _rect_outline(ca[0], ca[1], h, h + 1, rows, cols)                       # ~40 cells at h = 4
    out_b = _rect_outline(ca[0] + 2, ca[1] + 3, h, h + 1, rows, cols)               # overlaps A, new place
    big = rng.choice(rows * cols, 3000, replace=False).astype(np.int64)             # > 1024: stamp_cap growth
    # an erase block: around the wall cell nearest to A's centre, free cells included
    wr, wc = np.argwhere(base0 != 0)[np.argmin(np.hypot(*(np.argwhere(base0 != 0) - np.array(ca)).T))]
    er = np.arange(max(wr - 5, 1), min(wr + 6, rows - 1))
    ec = np.arange(max(wc - 5, 1), min(wc + 6, cols - 1))
    erase = (er[:, None] * cols + ec[None, :]).ravel().astype(np.int64)
    assert (base0.reshape(-1)[erase] != 0).any() and (base0.reshape(-1)[erase] == 0).any()
    border = np.flatnonzero(np.pad(np.zeros((rows - 2, cols - 2), bool), 1, constant_values=True).reshape(-1))
    out_c = _rect_outline(cb[0], cb[1], h, h + 1, rows, cols)

    def stamped(base, idx, value):
        g = base.copy()
        g.reshape(-1)[idx] = 1 if value else 0
        return g

    steps = [("outline A", ("stamp", out_a, 255), stamped(base0, out_a, 255)),
             ("outline B over A", ("stamp", out_b, 255), stamped(base0, out_b, 255)),
             ("3000 cells", ("stamp", big, 255), stamped(base0, big, 255)),
             ("erase a wall block", ("stamp", erase, 0), stamped(base0, erase, 0)),
             ("border and corners", ("stamp", border, 255), stamped(base0, border, 255)),
             ("empty list", ("stamp", np.zeros(0, np.int64), 255), base0.copy()),
             ("update", ("update", base1), base1.copy()),
             ("outline on the new base", ("stamp", out_c, 255), stamped(base1, out_c, 255))]
    focus = [ca, (ca[0] + 2, ca[1] + 3), cb, (3, cols // 4 + cols // 8), (rows - 3, cols - 3), (cols // 4 + cols // 8, 3)]
    return base0, steps, focus


def _poses(g, occs, focus, n, seed):
    """``n`` free poses of the first grid plus one pose at each focus cell (world coordinates)."""
    rng = np.random.default_rng(seed)
    free = np.argwhere(occs[0] == 0)
    cells = np.concatenate([np.array(focus, float), free[rng.choice(len(free), n, replace=False)].astype(float)])
    gy, gx = cells[:, 0] + 0.5, cells[:, 1] + 0.5
    c, s = np.cos(g.origin[2]), np.sin(g.origin[2])
    th = rng.uniform(-3.1, 3.1, len(cells))
    return np.stack([g.origin[0] + (c * gx - s * gy) * g.resolution, g.origin[1] + (s * gx + c * gy) * g.resolution,
                     th + g.origin[2]], 1).astype(np.float32)


def _fan(m, poses, aux=False):
    n = len(poses) * B
    out = np.full(n, -1.0, np.float32)
    if not aux:
        m.calc_range_fan(poses, out, FOV, B)
        return (out,)
    hits = np.full((n, 2), -7, np.int32)
    steps = np.zeros(n, np.uint16)
    m.calc_range_fan(poses, out, FOV, B, hit_cells=hits, steps=steps)
    return out, hits, steps


def _apply(omap, action):
    if action[0] == "stamp":
        omap.stamp_cells(action[1], value=action[2])
    else:
        omap.update(action[1])


def _check_map(oracle_mod, omap, grid, g, label):
    assert np.array_equal(_dev_occ(omap) != 0, grid != 0), label
    assert np.array_equal(omap.occ != 0, grid != 0), label
    om = oracle_mod.OracleMap(grid, g.resolution, g.origin, MRX)
    assert np.array_equal(omap.distance_transform(), om.dt), label
    return om


def _run_script(oracle_mod, omap, g, base0, steps, probes):
    """Warm every probe at epoch 0, then walk the script: map checks, then for each probe 'oracle differs from the
    previous grid' and two device calls equal to the oracle."""
    om = oracle_mod.OracleMap(base0, g.resolution, g.origin, MRX)
    prev = {}
    for name, dev, ora in probes:
        prev[name] = ora(om)
        assert _all_equal(dev(), prev[name]), (name, "epoch 0")
    for label, action, grid in steps:
        _apply(omap, action)
        om = _check_map(oracle_mod, omap, grid, g, label)
        for name, dev, ora in probes:
            want = ora(om)
            assert not _all_equal(want, prev[name]), (name, label, "the probe does not see this mutation")
            for call in (1, 2):
                assert _all_equal(dev(), want), (name, label, call)
            prev[name] = want


def test_warm_handles_follow_a_mutation_script(oracle_mod):
    """Every method's cached tables (step map, code map and palette, Bresenham pad, CDDT pose-/theta-major and the
    LDS-sorted table, GiantLUT) follow stamps (small, overlapping, growth past stamp_cap, erase, border, empty) and an
    update to a new base, on warm handles."""
    rows, cols = 230, 250
    base0, steps, focus = _script(rows, cols, 7, 4)
    g = maps.GridMap(base0, 0.05, (-1.3, 0.7, 0.25), "mut")
    poses = _poses(g, [base0], focus, 40, 3)
    omap = range_libc.PyOMap(g)
    edge = support.oracle_edge(oracle_mod, B, FOV)
    grp = len(poses) // 2
    probes = []

    for variant in (3, 1, 0):
        m = range_libc.PyRayMarching(omap, MRX)
        m.set_option("variant", variant)
        ref = (lambda o: o.rm_fan_libm(poses, FOV, B, step_coeff=0.999)) if variant == 3 else \
            (lambda o: o.rm_fan(poses, FOV, B, step_coeff=0.999, nthreads=8))
        probes.append(("RM v%d" % variant, lambda m=m: _fan(m, poses, aux=True), ref))
        probes.append(("RM v%d ranges" % variant, lambda m=m: _fan(m, poses), lambda o, ref=ref: ref(o)[:1]))

    code = range_libc.PyRayMarchingGPU(omap, MRX)
    code.set_option("code_map", 2)
    code.set_option("code_min_rays", 0)
    code.set_option("slots", 2)

    def code_fan():
        r = _fan(code, poses)
        pl = code.last_plan()
        assert pl["code"] == 2 and pl["code_entries"] == code.get_info("code_entries") >= 2, pl
        ranges = np.empty(len(poses) * B, np.float32)
        first_many = code.check_collision_many(poses, FOV, B, edge, 0.001, ranges=ranges)
        assert code.last_plan()["crash"] == 1 and np.array_equal(ranges, r[0])
        groups = code.check_collision_groups(poses, grp, FOV, B, edge, 0.001)
        assert code.last_plan()["code"] == 2
        return r[0], np.array([first_many]), groups

    def code_ref(o):
        r = rm_ranges(o, poses, FOV, B)
        return r, np.array([oracle_mod.is_crashed(r, B, len(poses), edge, 0.001)]), \
            np.array([oracle_mod.is_crashed(r[k * grp * B:(k + 1) * grp * B], B, grp, edge, 0.001) for k in range(2)])
    probes.append(("RMGPU code map + crash", code_fan, lambda o: code_ref(o)))

    rowmajor = range_libc.PyRayMarchingGPU(omap, MRX)
    rowmajor.set_option("tiled", 0)
    probes.append(("RMGPU tiled 0", lambda: _fan(rowmajor, poses, aux=True),
                   lambda o: o.rm_fan(poses, FOV, B, step_coeff=1.0, nthreads=8)))
    probes.append(("RMGPU tiled 0 ranges", lambda: _fan(rowmajor, poses),
                   lambda o: (rm_ranges(o, poses, FOV, B),)))
    for variant in (0, 1):
        m = range_libc.PyBresenhamsLine(omap, MRX)
        m.set_option("variant", variant)
        probes.append(("BL v%d" % variant, lambda m=m: _fan(m, poses, aux=True),
                       lambda o: o.bl_fan(poses, FOV, B, nthreads=8)))
    for label, opts in (("pose-major", {"cddt_theta_min": 0}), ("theta-major", {"cddt_theta_min": 1}),
                        ("lds_sort 128", {"cddt_lds_sort": 128})):
        m = range_libc.PyCDDTCast(omap, MRX, TD)
        for k, v in opts.items():
            m.set_option(k, v)
        probes.append(("CDDT " + label, lambda m=m: _fan(m, poses), lambda o: (cddt_ranges(o, TD, poses, FOV, B),)))
    _run_script(oracle_mod, omap, g, base0, steps, probes)
    omap.close()

    # GiantLUT on a small map: the table itself and a fan
    rows, cols = 70, 78
    base0, steps, focus = _script(rows, cols, 11, 3)
    g = maps.GridMap(base0, 0.05, (0.4, -0.9, -0.6), "mut-lut")
    lposes = _poses(g, [base0], focus, 24, 4)
    omap = range_libc.PyOMap(g)
    lut = range_libc.PyGiantLUTCast(omap, MRX, 180)

    def lut_ref(o):
        t = o.lut_build(180, nthreads=8)
        return t, o.lut_fan(t, lposes, FOV, B)
    _run_script(oracle_mod, omap, g, base0, steps, [("LUT", lambda: (lut.table(), _fan(lut, lposes)[0]), lut_ref)])
    omap.close()


def test_code_map_palette_follows_updates(oracle_mod):
    """One handle through a map whose palette fits, an open room whose palette does not, and back: code_entries, the
    plan's code map and the ranges follow each update."""
    n = 900
    maze = maps.make_maze(n, cell=40, wall=3, p=0.45, seed=21).occ.copy()
    room = np.zeros((n, n), np.uint8)
    room[0, :] = room[-1, :] = room[:, 0] = room[:, -1] = 1
    room[450, 450] = room[100, 700] = room[777, 123] = 1
    g = maps.GridMap(maze, 0.05, (-3.0, -2.0, 0.3), "palette")
    mrx, nb, fov = 300, 360, 6.0
    om = oracle_mod.OracleMap(maze, g.resolution, g.origin, mrx)
    poses = maps.sample_free_poses(g, 64, 5, dt=np.minimum(om.dt, oracle_mod.edt(room)))
    omap = range_libc.PyOMap(g)
    m = range_libc.PyRayMarchingGPU(omap, mrx)
    m.set_option("slots", 2)
    m.set_option("code_min_rays", 0)
    prev = None
    for label, grid, fits in (("maze", maze, True), ("room", room, False), ("maze again", maze, True)):
        if label != "maze":
            omap.update(grid)
        om = oracle_mod.OracleMap(grid, g.resolution, g.origin, mrx)
        want = om.rm_fan(poses, fov, nb, step_coeff=1.0, nthreads=8, want_hits=False, want_steps=False)[0]
        assert prev is None or not np.array_equal(want, prev), label
        for call in (1, 2):
            got = np.full(len(poses) * nb, -1.0, np.float32)
            m.calc_range_fan(poses, got, fov, nb)
            entries, pl = m.get_info("code_entries"), m.last_plan()
            if fits:
                assert entries >= 2 and pl["code"] == 2 and pl["code_entries"] == entries, (label, call, entries, pl)
            else:
                assert entries == 0 and pl["code"] == 0, (label, call, entries, pl)
            assert np.array_equal(got, want), (label, call)
        prev = want
    m.close()
    omap.close()


def test_entry_points_after_a_stamp(oracle_mod):
    """The 2-argument and 4-argument calc_range_many, the device-resident fan and grouped crash calls, and
    CarBatch.rollout_check, each warmed at epoch 0 and called after a stamp."""
    torch = pytest.importorskip("torch")
    from pyracecarsimulator_amd import racecar as RC
    rows, cols = 230, 250
    base0, steps, focus = _script(rows, cols, 7, 4)
    g = maps.GridMap(base0, 0.05, (-1.3, 0.7, 0.25), "mut")
    poses = _poses(g, [base0], focus, 40, 3)
    stamp, grid = steps[0][1][1], steps[0][2]
    om0 = oracle_mod.OracleMap(base0, g.resolution, g.origin, MRX)
    om1 = oracle_mod.OracleMap(grid, g.resolution, g.origin, MRX)
    omap = range_libc.PyOMap(g)
    rng = np.random.default_rng(5)
    ins = poses[rng.integers(0, len(poses), 3000)].copy()
    ins[:, 2] = rng.uniform(-7, 7, len(ins)).astype(np.float32)
    ins[:len(focus), :2] = poses[:len(focus), :2]
    sparse = np.zeros((len(poses) * B, 3), np.float32)
    sparse[::B] = poses
    rm = range_libc.PyRayMarching(omap, MRX)                    # upstream-literal arithmetic in both arities
    dev = range_libc.PyRayMarchingGPU(omap, MRX)
    edge = support.oracle_edge(oracle_mod, B, FOV)
    group = len(poses) // 4
    d_poses = torch.from_numpy(poses).cuda()
    d_edge = torch.from_numpy(edge).cuda()
    d_out = torch.zeros(len(poses) * B, dtype=torch.float32, device="cuda")
    d_first = torch.zeros(4, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    R, n_steps = 8, 200
    states = np.zeros((R, 11))
    states[:, :3] = poses[:R]                    # (the first pose sits inside the stamped outline)
    states[:, 3] = rng.uniform(1, 3, R)
    actions = np.stack([rng.uniform(0, 5, (R, 20)), rng.uniform(-0.4, 0.4, (R, 20))], -1)
    cars = RC.CarBatch()
    roll_poses = cars.rollout(states, actions)[0].reshape(-1, 3)

    def run():
        outs = np.empty(len(ins), np.float32)
        rm.calc_range_many(ins, outs)
        fan4 = np.full(len(poses) * B, -1.0, np.float32)
        rm.calc_range_many(sparse, fan4, FOV, B)
        dev.calc_range_fan_device(d_poses.data_ptr(), len(poses), FOV, B, d_out.data_ptr(), stream=st)
        d_first.fill_(-99)
        dev.check_collision_groups_device(d_poses.data_ptr(), 4, group, FOV, B, d_edge.data_ptr(), 0.001,
                                          d_first.data_ptr(), stream=st)
        torch.cuda.synchronize()
        first = cars.rollout_check(dev, states, actions, FOV, B, edge, 0.001)[0]
        return outs, fan4, d_out.cpu().numpy(), d_first.cpu().numpy(), first

    def ref(o):
        fan = rm_ranges(o, poses, FOV, B)
        rr = rm_ranges(o, roll_poses, FOV, B)
        return (o.rm_rays_libm(ins, step_coeff=0.999), o.rm_fan_libm(poses, FOV, B, step_coeff=0.999)[0], fan,
                np.array([oracle_mod.is_crashed(fan[k * group * B:(k + 1) * group * B], B, group, edge, 0.001)
                          for k in range(4)], np.int32),
                np.array([oracle_mod.is_crashed(rr[r * n_steps * B:(r + 1) * n_steps * B], B, n_steps, edge, 0.001)
                          for r in range(R)], np.int32), rr)

    w0, w1 = ref(om0), ref(om1)
    for k in (0, 1, 2, 5):                     # ranges of every form (and of the roll-out poses) see the stamp
        assert not np.array_equal(w0[k], w1[k]), k
    assert _all_equal(run(), w0[:5])
    omap.stamp_cells(stamp)
    assert np.array_equal(omap.distance_transform(), om1.dt)
    for call in (1, 2):
        got = run()
        for k, (a, b) in enumerate(zip(got, w1[:5])):
            assert np.array_equal(a, b), (k, call)
    omap.close()


def test_multi_device_map_mutations(oracle_mod):
    """A map on two devices (device 0 twice): RMGPU and CDDT handles across stamps and an update, each pose block on
    its own replica."""
    rows, cols = 230, 250
    base0, steps, focus = _script(rows, cols, 7, 4)
    g = maps.GridMap(base0, 0.05, (-1.3, 0.7, 0.25), "mut")
    poses = _poses(g, [base0], focus, 40, 3)
    omap = range_libc.PyOMap(g, device=[0, 0])
    rm = range_libc.PyRayMarchingGPU(omap, MRX)
    rm.set_option("multi_min_poses", 1)
    cd = range_libc.PyCDDTCast(omap, MRX, TD)
    cd.set_option("multi_min_poses", 1)
    assert rm.n_devices == 2 and cd.n_devices == 2
    probes = [("multi RMGPU", lambda: _fan(rm, poses),
               lambda o: (rm_ranges(o, poses, FOV, B),)),
              ("multi CDDT", lambda: _fan(cd, poses), lambda o: (cddt_ranges(o, TD, poses, FOV, B),))]
    # outline A, the growth path, the update, a stamp on the new base
    _run_script(oracle_mod, omap, g, base0, [steps[0], steps[2], steps[6], steps[7]], probes)
    omap.close()


def test_stamps_race_scan_threads(oracle_mod):
    """A thread alternates two stamps while two threads scan through methods of the map: every scan equals the oracle
    on ONE of the two grids (the stamp sibling of test_gpu_concurrency's update race)."""
    g = maps.make_maze(256, cell=32, wall=3, p=0.5, seed=8)
    rows, cols = g.occ.shape
    st_a = _rect_outline(100, 100, 12, 30, rows, cols)
    st_b = np.concatenate([_rect_outline(150, 60, 8, 8, rows, cols), np.arange(60, 200) * cols + 120])
    occ_a, occ_b = g.occ.copy(), g.occ.copy()
    occ_a.reshape(-1)[st_a] = 1
    occ_b.reshape(-1)[st_b] = 1
    mrx, nb, fov = 200, 360, 6.2
    om_a = oracle_mod.OracleMap(occ_a, g.resolution, g.origin, mrx)
    om_b = oracle_mod.OracleMap(occ_b, g.resolution, g.origin, mrx)
    omap = range_libc.PyOMap(g)
    methods = [range_libc.PyRayMarching(omap, mrx), range_libc.PyRayMarchingGPU(omap, mrx)]
    poses = maps.sample_free_poses(g, 24, 3, dt=np.minimum(om_a.dt, om_b.dt))
    want = [[om.rm_fan_libm(poses, fov, nb, step_coeff=0.999)[0] for om in (om_a, om_b)],
            [om.rm_fan(poses, fov, nb, step_coeff=1.0, nthreads=8)[0] for om in (om_a, om_b)]]
    assert not np.array_equal(want[0][0], want[0][1]) and not np.array_equal(want[1][0], want[1][1])
    omap.stamp_cells(st_a)
    stop = threading.Event()
    errors = []
    seen = [set(), set()]

    def stamper():
        k = 0
        while not stop.is_set():
            omap.stamp_cells(st_b if k % 2 == 0 else st_a)
            k += 1

    def scanner(i):
        out = np.empty(len(poses) * nb, np.float32)
        try:
            for k in range(300):
                methods[i].calc_range_fan(poses, out, fov, nb)
                if np.array_equal(out, want[i][0]):
                    seen[i].add("a")
                elif np.array_equal(out, want[i][1]):
                    seen[i].add("b")
                else:
                    errors.append((i, k))
                    return
        except Exception as e:                                  # noqa: BLE001
            errors.append((i, repr(e)))

    up = threading.Thread(target=stamper)
    sc = [threading.Thread(target=scanner, args=(i,)) for i in range(2)]
    up.start()
    for t in sc:
        t.start()
    for t in sc:
        t.join(300)
    stop.set()
    up.join(60)
    assert not errors, errors[:3]
    assert seen[0] == {"a", "b"} or seen[1] == {"a", "b"}
    omap.close()


def test_stamp_index_edge_cases(oracle_mod):
    """int64 indices are filtered on their integer value (0 <= idx < size), never wrapped by the int32 narrowing; a
    Python list works the same; an empty input of any dtype restores the base; a non-integer input raises."""
    g = maps.make_maze(64, cell=16, wall=2, p=0.5, seed=3)
    rows, cols = 50, 61
    base = g.occ[:rows, :cols].copy()
    g = maps.GridMap(base, 0.05, (0.0, 0.0, 0.0), "idx")
    size = rows * cols
    free = np.flatnonzero(base.reshape(-1) == 0)
    c0, c1, c2 = (int(v) for v in free[[5, len(free) // 2, -3]])
    w = int(free[1])                             # a free cell no index below stamps: 2**32 + w must not wrap onto it
    assert w not in (c0, c1, c2)
    vals = [-1, -size, size, 2**31, 2**32 + 5, 2**32 + w, 2**63 - 1, c0, c1, c1, c2, c0]
    omap = range_libc.PyOMap(g)
    for label, idx in (("int64", np.array(vals, np.int64)), ("list", list(vals))):
        omap.stamp_cells(idx)
        want = base.copy()
        want.reshape(-1)[[v for v in vals if 0 <= v < size]] = 1
        assert np.array_equal(_dev_occ(omap) != 0, want != 0), label
        assert np.array_equal(omap.occ != 0, want != 0), label
        om = oracle_mod.OracleMap(want, g.resolution, g.origin, MRX)
        assert np.array_equal(omap.distance_transform(), om.dt), label
        for empty in ([], np.zeros(0, np.float64), np.zeros((0, 2), np.int16), np.zeros(0, np.uint64)):
            omap.stamp_cells(idx)
            omap.stamp_cells(empty)
            assert np.array_equal(_dev_occ(omap) != 0, base != 0), (label, type(empty))
            assert np.array_equal(omap.occ != 0, base != 0), (label, type(empty))
    with pytest.raises(TypeError):
        omap.stamp_cells(np.array([1.0, 2.0]))
    omap.close()
