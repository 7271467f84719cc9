"""NumPy statement of the canonical car outline of the batched races (include/scanlib.h, "batched multi-car races"):
the rectangle Car::getBound means to trace, centred on (x, y), LENGTH along the heading and WIDTH across it, at
half-cell spacing, turned into grid cells.  Every operation is a separately rounded IEEE double, as on the device;
the heading's (sin, cos) is det_sincosf((float)theta), which the oracle's sincosf reproduces."""
import math

import numpy as np


def edge_counts(length, width, resolution):
    """Points per long / short edge: max(1, ceil(len / (0.5 res))) with the map's float32 res widened."""
    spacing = 0.5 * float(np.float32(resolution))
    return max(1, math.ceil(length / spacing)), max(1, math.ceil(width / spacing))


def car_frame_points(length, width, resolution):
    """(a, b) of every outline point in the car frame, in point order (corner 0's edge first)."""
    n_l, n_w = edge_counts(length, width, resolution)
    hl, hw = length / 2.0, width / 2.0
    corners = [(hl, hw), (-hl, hw), (-hl, -hw), (hl, -hw)]
    a, b = [], []
    for e, n in enumerate((n_l, n_w, n_l, n_w)):
        (a0, b0), (a1, b1) = corners[e], corners[(e + 1) % 4]
        u = np.arange(n, dtype=np.float64) / float(n)
        a.append(a0 + (a1 - a0) * u)
        b.append(b0 + (b1 - b0) * u)
    return np.concatenate(a), np.concatenate(b)


def grid_points(cars, length, width, resolution, origin, sincosf):
    """Grid coordinates (gx, gy) float64 (n, points) of each car's outline points; cars (n, 3) as (x, y, theta)."""
    cars = np.asarray(cars, dtype=np.float64).reshape(-1, 3)
    a, b = car_frame_points(length, width, resolution)
    s32, c32 = sincosf(cars[:, 2].astype(np.float32))
    s, c = s32.astype(np.float64)[:, None], c32.astype(np.float64)[:, None]
    xw = cars[:, :1] + (c * a - s * b)
    yw = cars[:, 1:2] + (s * a + c * b)
    inv_res = 1.0 / float(np.float32(resolution))
    gx0 = (xw - float(np.float32(origin[0]))) * inv_res
    gy0 = (yw - float(np.float32(origin[1]))) * inv_res
    ws, wc = sincosf(np.array([-np.float32(origin[2])], dtype=np.float32))      # PyOMap: world_angle = -yaw
    ws, wc = float(ws[0]), float(wc[0])
    with np.errstate(invalid="ignore"):
        return wc * gx0 - ws * gy0, ws * gx0 + wc * gy0


def outline_cells(cars, length, width, resolution, origin, rows, cols, sincosf):
    """Per car the flat cells row * cols + col of its outline points inside the grid, in point order with duplicates
    (a list of int64 arrays).  Non-finite points and points off the grid are skipped."""
    gx, gy = grid_points(cars, length, width, resolution, origin, sincosf)
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(gx) & np.isfinite(gy) & (gx >= 0) & (gx < cols) & (gy >= 0) & (gy < rows)
    out = []
    for i in range(gx.shape[0]):
        k = keep[i]
        out.append(np.floor(gy[i][k]).astype(np.int64) * cols + np.floor(gx[i][k]).astype(np.int64))
    return out


def point_cells(cars, length, width, resolution, origin, rows, cols, sincosf):
    """int64 (n, points): the flat cell of every outline point, -1 where the point is off the grid or not finite."""
    gx, gy = grid_points(cars, length, width, resolution, origin, sincosf)
    with np.errstate(invalid="ignore"):
        inside = np.isfinite(gx) & np.isfinite(gy) & (gx >= 0) & (gx < cols) & (gy >= 0) & (gy < rows)
    col = np.floor(np.where(inside, gx, 0.0)).astype(np.int64)
    row = np.floor(np.where(inside, gy, 0.0)).astype(np.int64)
    return np.where(inside, row * cols + col, -1)


def kept_points(cell):
    """bool, the shape of ``cell`` (point_cells): the points rl_car_outline_cells emits.  A point is kept when it has
    a cell and that cell differs from the cell of the point immediately before it in the full point list; a point
    without a cell is no cell to repeat, point 0 has no predecessor, and the last point is not compared with the first."""
    before = np.concatenate([np.full(cell.shape[:-1] + (1,), -1, cell.dtype), cell[..., :-1]], -1)
    return (cell >= 0) & (cell != before)


def outline_sequence(cars, length, width, resolution, origin, rows, cols, sincosf):
    """Per car the cells rl_car_outline_cells emits, in its order (include/scanlib.h: "points whose cell repeats the
    point before dropped"): a list of int64 arrays, point_cells at kept_points."""
    cell = point_cells(cars, length, width, resolution, origin, rows, cols, sincosf)
    keep = kept_points(cell)
    return [cell[i][keep[i]] for i in range(cell.shape[0])]


def stamped(occ, cells):
    """occ with the flat cells set (a copy)."""
    o = np.array(occ, dtype=np.uint8, copy=True)
    flat = o.reshape(-1)
    if len(cells):
        flat[np.asarray(cells, dtype=np.int64)] = 1
    return o


def others(cell_lists, group, n):
    """The cells car n scans against: the outlines of the other cars of its group."""
    g = n // group
    parts = [cell_lists[g * group + k] for k in range(group) if g * group + k != n]
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)
