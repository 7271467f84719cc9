"""NumPy statement of the origin-corrected GiantLUT query (handle option ``lut_refine``; include/scanlib.h
"origin-corrected GiantLUT query") — TEST INFRASTRUCTURE ONLY.

The table is the oracle's (``OracleMap.lut_build``: every row cast from the integer corner of its cell) and so are the
bin rule, the world -> grid transform and the deterministic trig (oracle/np_statement.py).  What is stated here is the
query: which corner's row a pose reads and the first-order correction of the pose's offset from that corner.  Every
operation is a separately rounded float32 unless written as ``fma``.

    c0, r0 = (int)gx, (int)gy                                   the default's cell
    cn, rn = min((int)rintf(gx), cols-1), min((int)rintf(gy), rows-1)     the nearest corner (ties to even)
    (c, r) = (cn, rn) unless dt[rn, cn] == 0 (that corner's cell is occupied): then (c0, r0)
    fx, fy = gx - c, gy - r                                     exact, in [-0.5, 1)
    q      = lut[r, c, bin]                                     the default's bin of the default's angle
    t      = (float)q * dequant
    px     = t                                   if q == 0 (starts in a wall) or q == 65535 (a miss)
             min(max(t - p, 0), max_range)       otherwise, p = fma(fx, dx, fy*dy), (dx, dy) the canonical march's direction
    range  = px * res  (+ the handle's noise)
"""
from __future__ import annotations

import numpy as np

from oracle import np_statement as N

f32 = N.f32
fma = N.fma
sincosf = N.sincosf


def corner(dt, gx, gy):
    """Per pose: (inb, c, r, fx, fy, took_nearest, fell_back).  ``took_nearest``: the nearest corner is another cell
    than the default's and was taken; ``fell_back``: it is another cell, occupied, and the default's was kept."""
    dt = np.asarray(dt, f32)
    rows, cols = dt.shape
    gx, gy = np.asarray(gx, f32), np.asarray(gy, f32)
    with np.errstate(invalid="ignore"):
        inb = (gx >= 0) & (gx < cols) & (gy >= 0) & (gy < rows)
    sx, sy = np.where(inb, gx, f32(0)).astype(f32), np.where(inb, gy, f32(0)).astype(f32)
    c0, r0 = np.trunc(sx).astype(np.int64), np.trunc(sy).astype(np.int64)
    cn = np.minimum(np.rint(sx).astype(np.int64), cols - 1)          # (np.rint: ties to even, as rintf)
    rn = np.minimum(np.rint(sy).astype(np.int64), rows - 1)
    occupied = dt[rn, cn] == f32(0)
    c, r = np.where(occupied, c0, cn), np.where(occupied, r0, rn)
    fx, fy = (sx - c.astype(f32)).astype(f32), (sy - r.astype(f32)).astype(f32)
    moved = inb & ((cn != c0) | (rn != r0))
    return inb, c, r, fx, fy, moved & ~occupied, moved & occupied


def _correct(q, fx, fy, dx, dy, mr, res):
    """uint16 table entries -> metres; every argument broadcast to q's shape."""
    t = (q.astype(f32) * f32(mr / f32(65535.0))).astype(f32)
    p = fma(fx, dx, (fy * dy).astype(f32))
    px = np.minimum(np.maximum((t - p).astype(f32), f32(0)), mr).astype(f32)
    px = np.where((q == 0) | (q == 65535), t, px).astype(f32)
    return (px * res).astype(f32)


def lut_refine_angles(lut, dt, resolution, origin, max_range_px, poses, alpha):
    """The refined query of every pose at its heading + alpha[j] (an arbitrary float32 angle table): f32[P * A]."""
    td = lut.shape[2]
    mr, res = f32(max_range_px), f32(resolution)
    alpha = np.asarray(alpha, f32).ravel()
    gx, gy, thg = N._pose_grid(resolution, origin, poses)
    inb, c, r, fx, fy, _, _ = corner(dt, gx, gy)
    b = N._theta_bin((thg[:, None] + alpha[None, :]).astype(f32), td)
    q = lut[r[:, None], c[:, None], b]
    st, ct = sincosf(thg)
    sa, ca = sincosf(alpha)
    dx = fma(ct[:, None], ca[None, :], -(st[:, None] * sa[None, :]).astype(f32))
    dy = fma(st[:, None], ca[None, :], (ct[:, None] * sa[None, :]).astype(f32))
    val = _correct(q, fx[:, None], fy[:, None], dx, dy, mr, res)
    return np.where(inb[:, None], val, f32(mr * res)).astype(f32).ravel()


def lut_refine_fan(lut, dt, resolution, origin, max_range_px, poses, fov, num_rays):
    """The refined fan: beam j at fan_alpha(f, j)."""
    return lut_refine_angles(lut, dt, resolution, origin, max_range_px, poses, N._fan_alpha(fov, num_rays))


def lut_refine_rays(lut, dt, resolution, origin, max_range_px, ins):
    """The refined per-ray call on (x, y, theta) rows: the direction is det_sincosf of the grid heading itself."""
    td = lut.shape[2]
    mr, res = f32(max_range_px), f32(resolution)
    gx, gy, thg = N._pose_grid(resolution, origin, ins)
    inb, c, r, fx, fy, _, _ = corner(dt, gx, gy)
    q = lut[r, c, N._theta_bin(thg, td)]
    dy, dx = sincosf(thg)
    return np.where(inb, _correct(q, fx, fy, dx, dy, mr, res), f32(mr * res)).astype(f32)


def census(dt, resolution, origin, poses):
    """(poses that take a nearest corner other than their own cell's, poses that fall back from an occupied one)."""
    gx, gy, _ = N._pose_grid(resolution, origin, poses)
    _, _, _, _, _, took, fell = corner(dt, gx, gy)
    return int(took.sum()), int(fell.sum())


def near_wall_poses(g, dt, n, seed, max_dt=1.5):
    """Seeded world poses float32 (n, 3) in free cells hugging a wall (0 < dt <= max_dt cells): sub-cell offset
    U[0, 1)^2, heading U(-pi, pi), as maps.sample_free_poses draws them."""
    rng = np.random.default_rng(seed)
    dt = np.asarray(dt).reshape(g.occ.shape)
    rr, cc = np.nonzero((g.occ == 0) & (dt <= max_dt))
    pick = rng.integers(0, rr.size, size=n)
    off = rng.random((n, 2))
    th = rng.uniform(-np.pi, np.pi, size=n)
    ox, oy, yaw = g.origin
    gx, gy = cc[pick] + off[:, 0], rr[pick] + off[:, 1]
    c, s = np.cos(yaw), np.sin(yaw)
    xw = ox + (c * gx - s * gy) * g.resolution
    yw = oy + (s * gx + c * gy) * g.resolution
    return np.ascontiguousarray(np.stack([xw, yw, th + yaw], axis=1).astype(np.float32))


def integer_poses(g, dt, n, seed):
    """World poses float32 (n, 3) whose grid coordinates are integers of free cells: candidates on cell corners, kept
    where the float32 world -> grid transform lands on the integer exactly (about a third do at 0.05 m per cell)."""
    rng = np.random.default_rng(seed)
    dt = np.asarray(dt).reshape(g.occ.shape)
    rr, cc = np.nonzero(dt > 0)
    pick = rng.integers(0, rr.size, size=16 * n)
    ox, oy, yaw = g.origin
    c, s = np.cos(yaw), np.sin(yaw)
    cand = np.stack([ox + (c * cc[pick] - s * rr[pick]) * g.resolution, oy + (s * cc[pick] + c * rr[pick]) * g.resolution,
                     rng.uniform(-np.pi, np.pi, pick.size) + yaw], axis=1).astype(np.float32)
    gx, gy, _ = N._pose_grid(g.resolution, g.origin, cand)
    keep = (gx == cc[pick]) & (gy == rr[pick])
    assert keep.sum() >= n, "too few candidates land on integer grid coordinates"
    return np.ascontiguousarray(cand[keep][:n])
