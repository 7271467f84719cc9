"""NumPy statement of the particle-filter calls (include/scanlib.h "particle-filter weights") — TEST INFRASTRUCTURE ONLY.

(a) the canonical repeat-angle march: oracle/np_statement.rm_fan's loop with the beam angles as an argument;
(b) the sensor model: ``bin()`` and the ascending product, an explicit loop over j vectorised over particles.
Plus the row expansions the oracle's per-ray casters take and the fan-equivalent angle tables.
"""
from __future__ import annotations

import numpy as np

from oracle import np_statement as NS

f32 = np.float32


def witness_table(width=64, seed=20):
    """The seeded sensor-model table of the product-order witness: uniform in (0.5, 1.5), so that a product of a
    hundred factors neither overflows nor underflows and nearly every product rounds."""
    return np.random.default_rng(seed).uniform(0.5, 1.5, (width, width))


def fan_angles(fov, num_rays):
    """angles[j] = fma(j, inc, amin): the canonical and table kinds' fan (np_statement._fan_alpha)."""
    return NS._fan_alpha(fov, num_rays)


def fan_angles_literal(fov, num_rays):
    """angles[j] = amin + j * inc, product and sum each rounded to float32: the literal kind's fan."""
    j = np.arange(num_rays, dtype=f32)
    inc = f32(f32(fov) / f32(num_rays))
    amin = f32(f32(-0.5) * f32(fov))
    return (amin + (j * inc).astype(f32)).astype(f32)


def expand_rows(poses, angles):
    """(P*A, 3) float32 rows (x, y, f32(theta + a_j)): what the 2-argument calc_range_many takes, particle-major."""
    poses = np.asarray(poses, f32).reshape(-1, 3)
    angles = np.asarray(angles, f32)
    rows = np.empty((poses.shape[0], angles.size, 3), f32)
    rows[:, :, 0] = poses[:, None, 0]
    rows[:, :, 1] = poses[:, None, 1]
    rows[:, :, 2] = (poses[:, None, 2] + angles[None, :]).astype(f32)
    return rows.reshape(-1, 3)


def repeat_angles(occ, resolution, origin, max_range_px, poses, angles, step_coeff=0.999, dt=None):
    """(a) canonical repeat-angle scan -> (ranges f32[P*A], hits i32[P*A, 2], steps u16[P*A])."""
    occ = np.asarray(occ)
    rows, cols = occ.shape
    dt = NS.edt(occ) if dt is None else np.asarray(dt, f32)
    res = f32(resolution)
    gx, gy, thg = NS._pose_grid(resolution, origin, poses)
    alpha = np.asarray(angles, f32)
    num_rays = alpha.size
    st, ct = NS.sincosf(thg)
    sa, ca = NS.sincosf(alpha)
    dx = NS.fma(ct[:, None], ca[None, :], -(st[:, None] * sa[None, :]).astype(f32)).ravel()
    dy = NS.fma(st[:, None], ca[None, :], (ct[:, None] * sa[None, :]).astype(f32)).ravel()
    gx = np.repeat(gx, num_rays)
    gy = np.repeat(gy, num_rays)
    n = gx.size
    mr = f32(max_range_px)
    t = np.zeros(n, f32)
    out = np.full(n, mr, f32)
    hits = np.full((n, 2), -1, np.int32)
    steps = np.zeros(n, np.int64)
    live = np.ones(n, bool)
    while True:
        live &= t < mr
        idx = np.nonzero(live)[0]
        if idx.size == 0:
            break
        fx = NS.fma(dx[idx], t[idx], gx[idx])
        fy = NS.fma(dy[idx], t[idx], gy[idx])
        inb = (fx > -1) & (fx < cols) & (fy > -1) & (fy < rows)
        live[idx[~inb]] = False
        idx, fx, fy = idx[inb], fx[inb], fy[inb]
        pc = np.trunc(fx).astype(np.int64)
        pr = np.trunc(fy).astype(np.int64)
        d = dt[pr, pc]
        steps[idx] += 1
        hit = d <= 0
        hi = idx[hit]
        xd = (pc[hit].astype(f32) - gx[hi]).astype(f32)
        yd = (pr[hit].astype(f32) - gy[hi]).astype(f32)
        out[hi] = np.sqrt(NS.fma(xd, xd, (yd * yd).astype(f32))).astype(f32)
        hits[hi, 0] = pc[hit]
        hits[hi, 1] = pr[hit]
        live[hi] = False
        go = idx[~hit]
        t[go] = (t[go] + np.maximum((d[~hit] * f32(step_coeff)).astype(f32), f32(1.0))).astype(f32)
    return (out * res).astype(f32), hits, np.minimum(steps, 65535).astype(np.uint16)


def inv_res_of(resolution):
    """The map's float32 inverse resolution, as the world -> grid transform uses it."""
    return f32(1.0 / float(f32(resolution)))


def sensor_bin(v, inv_res, width):
    """bin(v) = (int) fminf(fmaxf(v * inv_res, 0), width - 1); NaN -> 0 (fmaxf returns its other argument)."""
    v = np.asarray(v, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (v * f32(inv_res)).astype(f32)
        u = np.where(np.isnan(u), f32(0.0), np.maximum(u, f32(0.0))).astype(f32)
        u = np.minimum(u, f32(width - 1)).astype(f32)
    return np.trunc(u).astype(np.int64)


def factors(table, obs, ranges, inv_res):
    """(P, A) float64 factors table[bin(obs[j]), bin(ranges[p, j])]."""
    table = np.asarray(table, np.float64)
    width = table.shape[0]
    obs = np.asarray(obs, f32)
    ranges = np.asarray(ranges, f32).reshape(-1, obs.size)
    return table[sensor_bin(obs, inv_res, width)[None, :], sensor_bin(ranges, inv_res, width)]


def product_ascending(fac):
    w = np.ones(fac.shape[0], np.float64)
    for j in range(fac.shape[1]):
        w = w * fac[:, j]
    return w


def product_descending(fac):
    w = np.ones(fac.shape[0], np.float64)
    for j in range(fac.shape[1] - 1, -1, -1):
        w = w * fac[:, j]
    return w


def product_tree(fac):
    """Halving tree: pad to a power of two with ones, multiply the two halves until one column is left."""
    n = 1
    while n < fac.shape[1]:
        n *= 2
    a = np.ones((fac.shape[0], n), np.float64)
    a[:, :fac.shape[1]] = fac
    while n > 1:
        n //= 2
        a = a[:, :n] * a[:, n:2 * n]
    return a[:, 0].copy()


def weights(table, obs, ranges, inv_res):
    """(b) weight_p = 1.0; for j ascending: weight_p *= table[bin(obs[j]), bin(ranges[p, j])]."""
    return product_ascending(factors(table, obs, ranges, inv_res))
