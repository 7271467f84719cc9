"""NumPy statement of the race scan on CDDT (include/scanlib.h, "Races on CDDT"; handle option ``race_cddt``), built on
oracle/np_statement.py's ``CddtTable`` of the STATIC grid and tests/race_statement.py's outline: car i scans the static
table with the outline cells of the other cars of its race joining the bucket it searches, each projected the way the
table build projects an edge cell.  Every operation is a separately rounded float32, as in ``CddtTable``.

Also here, because the host test and the GPU test share them: the two conditions under which the statement equals
"stamp, rebuild, scan" (``meets_conditions``), that second answer itself (``stamped_fan``), the 96-cell maze and the
two line-up recipes of docs/history/race_cddt.md."""
import numpy as np

import race_statement as RS
from oracle import np_statement as NS
from pyracecarsimulator_amd import maps

f32 = np.float32
L, W = 0.4064, 0.2032                       # the reference car (racecar.DEFAULT_CAR's length and width)


def cell_entries(table, a, cells):
    """(slx, lower, upper) of the flat ``cells`` in table bin ``a``: the rotated x a cell adds and the buckets
    [lower, upper] it covers, as ``CddtTable.__init__`` computes them for an edge cell."""
    cells = np.asarray(cells, np.int64)
    r, c = cells // table.cols, cells % table.cols
    px, py = (c.astype(f32) + f32(0.5)).astype(f32), (r.astype(f32) + f32(0.5)).astype(f32)
    cs, sn = table.cos[a], table.sin[a]
    half = f32((abs(sn) + abs(cs)) * f32(0.5))
    slx = NS.fma(px, cs, -(py * sn).astype(f32))
    sly = (NS.fma(px, sn, (py * cs).astype(f32)) + table.trans[a]).astype(f32)
    upper = NS._trunc_i(((sly + half).astype(f32) - table.EPS).astype(f32))
    lower = NS._trunc_i(((sly - half).astype(f32) + table.EPS).astype(f32))
    return slx, np.maximum(lower, 0), np.minimum(upper, table.width[a] - 1)


def query(table, gx, gy, th, max_range, cells):
    """``CddtTable.query`` with the flat ``cells`` (S_i) joining every bucket they cover: ranges in pixels."""
    out = np.full(len(gx), f32(max_range), f32)
    b = NS._theta_bin((-np.asarray(th, f32)).astype(f32), table.td)
    flipped = b >= table.nb
    b = np.where(flipped, b - table.td // 2, b)
    b = np.minimum(b, table.nb - 1)
    gx, gy = np.asarray(gx, f32), np.asarray(gy, f32)
    cs, sn = table.cos[b], table.sin[b]
    with np.errstate(invalid="ignore", over="ignore"):
        lx_all = NS.fma(gx, cs, -(gy * sn).astype(f32))
        ly_all = (NS.fma(gx, sn, (gy * cs).astype(f32)) + table.trans[b]).astype(f32)
        inside = (ly_all >= 0) & (ly_all < table.width[b].astype(f32))
    # the beams of a pose in one bin share an answer: one look-up per distinct (origin projection, bin, direction)
    keys = np.stack([lx_all.view(np.uint32), ly_all.view(np.uint32), b.astype(np.uint32), flipped.astype(np.uint32)], -1)
    rays = np.flatnonzero(inside)
    uniq, which = np.unique(keys[rays], axis=0, return_inverse=True)
    which = which.reshape(-1)
    per_bin = {}
    for u in range(len(uniq)):
        i = rays[np.flatnonzero(which == u)[0]]
        a, lx, bkt = int(b[i]), lx_all[i], int(np.trunc(ly_all[i]))
        if a not in per_bin:
            per_bin[a] = cell_entries(table, a, cells)
        slx, lower, upper = per_bin[a]
        F = np.concatenate([table.buckets[a][bkt], slx[(lower <= bkt) & (bkt <= upper)]]).astype(f32)
        r = f32(max_range)
        if not flipped[i]:
            ahead = F[F >= lx]
            if len(ahead):
                r = min(f32(ahead.min() - lx), f32(max_range))
        else:
            behind = F[F <= lx]
            if len(behind):
                r = min(f32(lx - behind.max()), f32(max_range))
        out[rays[which == u]] = r
    return out


def fan(table, resolution, origin, max_range_px, poses, cell_lists, group, fov, num_rays):
    """The race scan of ``poses`` float32 (N, 3) in races of ``group``: pose n against the cells of the other cars of its
    race (``cell_lists``: one flat-cell array per car, e.g. RS.outline_cells).  float32 (N * num_rays,) metres, no noise."""
    poses = np.asarray(poses, f32).reshape(-1, 3)
    gx, gy, thg = NS._pose_grid(resolution, origin, poses)
    alpha = NS._fan_alpha(fov, num_rays)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(poses.shape[0]):
            th = (thg[n] + alpha).astype(f32)
            r = query(table, np.repeat(gx[n], num_rays), np.repeat(gy[n], num_rays), th, max_range_px,
                      RS.others(cell_lists, group, n))
            out.append((r * f32(resolution)).astype(f32))
    return np.concatenate(out) if out else np.zeros(0, f32)


# ---------------------------------------------------------------- the relation to "stamp, rebuild, scan"
def edge_mask(occ):
    """OMap::make_edge_map's rule as ``CddtTable`` states it: occupied, and on the border or with a free 4-neighbour."""
    occ = np.asarray(occ) != 0
    pad = np.pad(occ, 1, constant_values=False)
    all4 = pad[:-2, 1:-1] & pad[2:, 1:-1] & pad[1:-1, :-2] & pad[1:-1, 2:]
    border = np.zeros_like(occ)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
    return occ & (~all4 | border)


def meets_conditions(occ, cells):
    """(i) every cell of ``cells`` is an edge cell of occ u cells; (ii) every edge cell of occ still is one there."""
    after = edge_mask(RS.stamped(occ, cells))
    flat = after.reshape(-1)
    return bool(flat[np.asarray(cells, np.int64)].all()) and bool(after[edge_mask(occ)].all())


def stamped_fan(g, theta_disc, max_range_px, pose, cells, fov, num_rays):
    """Stamp ``cells``, rebuild the table, scan ``pose``: NS.cddt_fan on ``CddtTable(stamped grid)``."""
    table = NS.CddtTable(RS.stamped(g.occ, cells), theta_disc)
    return NS.cddt_fan(table, g.resolution, g.origin, max_range_px, np.asarray(pose, f32).reshape(1, 3), fov, num_rays)


# ---------------------------------------------------------------- the measured set-up (docs/history/race_cddt.md)
MAZE_SIDE, MRX, BEAMS, OTHERS = 96, 60, 97, 3


def maze():
    return maps.make_maze(MAZE_SIDE, cell=16, wall=2, p=0.4, seed=5)


def lineup(g, dt, rng, clear):
    """One scanning pose (a free cell 3 cells off the walls) and the (x, y, theta) of OTHERS other cars.  ``clear`` 7:
    the others' centres anywhere on the map's cells whose EDT is at least 7 cells (the corridor centres: an outline
    reaches 4.6 cells); None: thrown anywhere within +-1.2 m of the scanning pose, walls and each other included."""
    res, (ox, oy, _) = g.resolution, g.origin

    def in_cell(rc):
        return ox + (rc[1] + rng.uniform()) * res, oy + (rc[0] + rng.uniform()) * res

    free = np.argwhere(dt >= 3)
    pose = np.array(in_cell(free[rng.integers(len(free))]) + (rng.uniform(-np.pi, np.pi),))
    pool = np.argwhere(dt >= clear) if clear is not None else None
    cars = np.zeros((OTHERS, 3))
    for k in range(OTHERS):
        xy = in_cell(pool[rng.integers(len(pool))]) if clear is not None else pose[:2] + rng.uniform(-1.2, 1.2, 2)
        cars[k] = (xy[0], xy[1], rng.uniform(-np.pi, np.pi))
    return pose, cars


def compare_lineups(g, dt, table, theta_disc, n, seed, clear, fov, sincosf):
    """``n`` line-ups of the recipe ``clear``: the statement against stamp-rebuild-scan on each.  Returns (line-ups that
    meet (i) and (ii), rays that differ in those, rays that differ in all of them, rays in all of them)."""
    rng = np.random.default_rng(seed)
    kept = diff_kept = diff_all = 0
    for _ in range(n):
        pose, cars = lineup(g, dt, rng, clear)
        lists = RS.outline_cells(cars, L, W, g.resolution, g.origin, g.rows, g.cols, sincosf)
        cells = np.concatenate(lists)
        # a race of OTHERS + 1 cars whose first car scans: its own outline is not in its S
        got = fan(table, g.resolution, g.origin, MRX, pose[None], [np.zeros(0, np.int64)] + lists, OTHERS + 1, fov,
                  BEAMS)[:BEAMS]
        want = stamped_fan(g, theta_disc, MRX, pose, cells, fov, BEAMS)
        d = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        diff_all += d
        if meets_conditions(g.occ, cells):
            kept += 1
            diff_kept += d
    return kept, diff_kept, diff_all, n * BEAMS
