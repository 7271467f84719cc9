"""NumPy statement of one particle-filter update (include/scanlib.h "particle-filter localisation") — TEST
INFRASTRUCTURE ONLY.  Every operation is a float64 NumPy operation (one rounding each); sums whose order the contract
pins are ``np.cumsum`` (sequential) or explicit Python loops.  The likelihood is a callable, so that a test can plug in
tests/pf_statement.py's march or the oracle's table kinds (GPU parity) or a synthetic model (host tests).
"""
from __future__ import annotations

import numpy as np

from mcts_statement import uniform01
from oracle import np_statement as NS

f32 = np.float32
CHUNK = 256
RESAMPLED, DEGENERATE = 1, 2


# ---------------------------------------------------------------- draws
def motion_counters(t, axis):
    """The twelve counters i of axis ``axis``'s normal at step t (d is the particle)."""
    return 64 * int(t) + 1 + 12 * int(axis) + np.arange(12, dtype=np.uint64)


def resample_counter(t):
    """(d, i) of step t's resampling draw."""
    return 0, 64 * int(t)


def normal12(seed, p, t, axis):
    """g = (sum of twelve uniforms, ascending from 0.0) - 6.0 for particles ``p`` (Probabilistic Robotics, Table 5.4)."""
    p = np.asarray(p, np.uint64).ravel()
    i = motion_counters(t, axis).astype(np.uint64)
    u = uniform01(seed, np.repeat(p, 12), np.tile(i, p.size)).reshape(p.size, 12)
    s = np.zeros(p.size)
    for k in range(12):
        s = s + u[:, k]
    return s - 6.0


# ---------------------------------------------------------------- blocked sums
def chunk_totals(v):
    v = np.asarray(v, np.float64)
    return np.array([np.cumsum(v[b:b + CHUNK])[-1] for b in range(0, v.size, CHUNK)])


def bs(v):
    """The sequential sum of the sequential chunk totals."""
    return float(np.cumsum(chunk_totals(v))[-1])


def cum(v):
    """cum(v)[i] = B_b + s_i: the chunk's base (sequential sum of the totals before it, from 0.0) + the inclusive sum
    inside the chunk."""
    v = np.asarray(v, np.float64)
    tot = chunk_totals(v)
    base = np.concatenate([[0.0], np.cumsum(tot)[:-1]])
    out = np.empty_like(v)
    for k, b in enumerate(range(0, v.size, CHUNK)):
        out[b:b + CHUNK] = base[k] + np.cumsum(v[b:b + CHUNK])
    return out


# ---------------------------------------------------------------- the step
def motion(X, odom, std, seed, t):
    X = np.asarray(X, np.float64)
    dx, dy, dth = (np.float64(v) for v in odom)
    s, c = NS.sincosf(X[:, 2].astype(f32))
    s, c = s.astype(np.float64), c.astype(np.float64)
    p = np.arange(X.shape[0])
    out = np.empty_like(X)
    out[:, 0] = X[:, 0] + (c * dx - s * dy)
    out[:, 1] = X[:, 1] + (s * dx + c * dy)
    out[:, 2] = X[:, 2] + dth
    for a in range(3):
        if std[a] > 0:
            out[:, a] = out[:, a] + np.float64(std[a]) * normal12(seed, p, t, a)
    return out


def ancestors(c, u):
    """a_i = min(P - 1, #{k : c[k] <= tau_i}), tau_i = ((u + i) / P) S."""
    P = c.size
    tau = ((np.float64(u) + np.arange(P, dtype=np.float64)) / np.float64(P)) * c[-1]
    assert (np.diff(c) >= 0).all(), "cum(w) must be non-decreasing (non-negative weights)"
    return np.minimum(P - 1, np.searchsorted(c, tau, side="right")).astype(np.int32)


class Filter:
    """likelihood(q float32 (P, 3), obs float32 (A,), t) -> float64 (P,)."""

    def __init__(self, likelihood, n_particles, motion_std=(0.0, 0.0, 0.0), resample_ratio=0.5):
        self.likelihood = likelihood
        self.P = int(n_particles)
        self.std = tuple(float(v) for v in motion_std)
        self.ratio = float(resample_ratio)

    def reset(self, particles, weights=None, seed=0):
        self.X = np.array(particles, np.float64).reshape(self.P, 3)
        self.w = np.full(self.P, 1.0 / float(self.P)) if weights is None else np.array(weights, np.float64)
        self.seed, self.t = int(seed), 0

    def step(self, odom, obs):
        P, t = self.P, self.t
        Xp = motion(self.X, odom, self.std, self.seed, t)
        q = Xp.astype(f32)
        L = np.asarray(self.likelihood(q, np.asarray(obs, f32), t), np.float64)
        omega = self.w * L
        W = bs(omega)
        flags = 0
        if np.isnan(W) or W == np.inf or not W > 0:
            w = np.full(P, 1.0 / float(P))
            flags |= DEGENERATE
        else:
            w = omega / np.float64(W)
        sh, ch = NS.sincosf(Xp[:, 2].astype(f32))
        with np.errstate(divide="ignore"):
            neff = float(np.float64(1.0) / np.float64(bs(w * w)))
        est = np.array([bs(w * Xp[:, 0]), bs(w * Xp[:, 1]), bs(w * ch.astype(np.float64)), bs(w * sh.astype(np.float64))])
        c = cum(w)
        if neff < self.ratio * float(P):
            a = ancestors(c, uniform01(self.seed, *resample_counter(t)))
            self.X, self.w = Xp[a], np.full(P, 1.0 / float(P))
            flags |= RESAMPLED
        else:
            a = np.arange(P, dtype=np.int32)
            self.X, self.w = Xp, w
        self.anc, self.cum, self.L, self.omega, self.q = a, c, L, omega, q
        self.t += 1
        return est, neff, flags

    def run(self, odom, obs):
        odom = np.asarray(odom, np.float64).reshape(-1, 3)
        rows = [self.step(odom[k], obs[k]) for k in range(odom.shape[0])]
        return (np.array([r[0] for r in rows]).reshape(-1, 4), np.array([r[1] for r in rows]),
                np.array([r[2] for r in rows], np.int32))


def pose_of(est):
    est = np.asarray(est).reshape(-1, 4)
    return np.stack([est[:, 0], est[:, 1], np.arctan2(est[:, 3], est[:, 2])], axis=1)


# ---------------------------------------------------------------- synthetic models of the host tests
def gaussian_table(width, sigma=3.0, floor=0.02):
    """A beam model: a Gaussian around the diagonal on a uniform floor, every column summing to one."""
    o = np.arange(width, dtype=np.float64)[:, None]
    e = np.arange(width, dtype=np.float64)[None, :]
    t = np.exp(-0.5 * ((o - e) / sigma) ** 2) + floor
    return np.ascontiguousarray(t / t.sum(0, keepdims=True))


def peaked_table(width, sigma=1.0, floor=1e-3):
    """The GPU tests' table: so narrow that a handful of particles carry the weight (many die, some multiply)."""
    return gaussian_table(width, sigma, floor)


# ---------------------------------------------------------------- the GPU tests' input
def statement_likelihood(g, om, max_range_px, form, angles, table, theta_disc=None, lut=None):
    """The statement's L for one arithmetic — "literal" (step coefficient 0.999), "canonical" (1.0), "cddt", "lut" — as a
    Filter likelihood: the kind's ranges by the oracle map ``om`` / tests/pf_statement.py and the ascending product.
    ``lut``: the GiantLUT handle's own table (the oracle reads it; the other forms need no device)."""
    import pf_statement as PS
    inv_res = PS.inv_res_of(g.resolution)

    def lik(q, obs, t):
        if form == "canonical":
            r = PS.repeat_angles(g.occ, g.resolution, g.origin, max_range_px, q, angles, step_coeff=1.0, dt=om.dt)[0]
        else:
            rows = PS.expand_rows(q, angles)
            if form == "literal":
                r = om.rm_rays_libm(rows, step_coeff=0.999)
            elif form == "cddt":
                r = om.cddt_rays(theta_disc, rows)
            else:
                r = om.lut_rays(lut, rows)
        return PS.weights(table, obs, r, inv_res)
    return lik


def localisation_case(g, dt, max_range_px, fov, P, A, T, seed=5):
    """A car driving a gentle arc through golden map ``g`` and P particles scattered around its start (3 cells, 0.1 rad;
    particle 0 on it): (particles (P, 3) f64, angles (A,) f32, odom (T, 3) f64, obs (T, A) f32 — the canonical march from
    the car's true poses —, table).  With ``peaked_table`` most particles lose to the few near the truth."""
    import pf_statement as PS
    from pyracecarsimulator_amd import maps
    true0 = maps.sample_free_poses(g, 1, seed, 6.0, dt)[0].astype(np.float64)
    rng = np.random.default_rng(1000 * A + P + seed)
    spread = np.array([3.0 * g.resolution, 3.0 * g.resolution, 0.1])
    particles = true0[None, :] + rng.normal(0.0, 1.0, (P, 3)) * spread[None, :]
    particles[0] = true0
    angles = (np.linspace(-0.5 * fov, 0.5 * fov, A) if A > 1 else np.zeros(1)).astype(f32)
    odom = np.array([[0.8 * g.resolution, 0.1 * g.resolution, 0.02]]) * (1.0 + 0.25 * np.arange(T))[:, None]
    X, obs = true0[None, :], []
    for t in range(T):
        X = motion(X, odom[t], (0.0, 0.0, 0.0), 0, t)
        obs.append(PS.repeat_angles(g.occ, g.resolution, g.origin, max_range_px, X.astype(f32), angles, dt=dt)[0])
    return particles, angles, odom, np.array(obs, f32), peaked_table(int(max_range_px) + 1)


# ---------------------------------------------------------------- the inputs of tests/test_gpu_pf_scale.py
#: (P, A, T, kinds, ratios, dead, most): the localisation rows beyond one workgroup round.  ``dead`` / ``most``: with ratio
#: 2.0 the ancestors of the LAST step leave at least that share of the particles without a descendant and give some
#: particle at least that many.  A single beam tells few particles apart: at A = 1 the second step's resampling of the
#: already resampled cloud leaves 21-23 % dead and no particle more than two descendants, so the two-step rows at A = 1
#: take (0.20, 2); the others the (0.25, 3) of tests/test_gpu_mcl.py.  tests/test_mcl_host.py holds the statement to every bar.
SCALE_ROWS = [
    (2500, 7, 2, ("RM-3", "RMGPU-1", "CDDT", "GLT"), (2.0, 0.5, 0.0), 0.25, 3),
    (65793, 1, 2, ("RMGPU-1", "CDDT"), (2.0, 0.5), 0.20, 2),
    (131072, 1, 2, ("RM-3",), (2.0,), 0.20, 2),
    (131073, 1, 2, ("RM-3",), (2.0, 0.5), 0.20, 2),
    (140001, 1, 2, ("RM-3", "RMGPU-1", "CDDT", "GLT"), (2.0, 0.5), 0.20, 2),
    (1 << 20, 1, 1, ("RM-3",), (2.0,), 0.25, 3),
]
#: the flags of a row's steps by ratio: a peaked table always falls below 2 P, never below 0; below P / 2 at every step
#: with 7 beams, at the first step only with one (neff 0.40 P, then 0.76 P)
def scale_flags(A, T, ratio):
    if ratio == 2.0:
        return [RESAMPLED] * T
    if ratio == 0.0:
        return [0] * T
    return [RESAMPLED] * T if A > 1 else [RESAMPLED, 0][:T]


def overflow_table(table):
    """With weights of 1e308 the first step's omega overflows: W = +inf."""
    return table * 300.0


def nan_table(table):
    """NaN planted in one entry of 35: some particle meets one at every step, and W is NaN."""
    t = table.copy()
    t[::5, ::7] = np.nan
    return t


def plateau_table(table):
    """Every entry below 1e-2 exactly zero: most particles get a zero weight, cum(w) has long flat stretches."""
    t = table.copy()
    t[t < 1e-2] = 0.0
    return t
