"""Particle-filter localisation, host side: the NumPy statement (tests/mcl_statement.py) on its own — the draw counters,
the twelve-uniform normal, the witness that lets the GPU tests tell the pinned summation order from any other, the
condition of the GPU tests' input, the estimate's convergence, and the degenerate / never-resample paths."""
import numpy as np
import pytest

import mcl_statement as MS
import pf_statement as PS
from conftest import load_golden
from mcts_statement import uniform01

f32 = np.float32


def test_draw_counters_do_not_collide():
    """Step t owns counters 64 t ... 64 t + 63: the resampling draw at (0, 64 t), the motion draws of particle p at
    (p, 64 t + 1 ... 64 t + 36).  No pair (d, i) is used twice over particles, axes and steps, and 2^26 steps fit u32."""
    seen = set()
    for t in (0, 1, 2, 77, (1 << 26) - 1):
        block = [MS.resample_counter(t)]
        for p in (0, 1, 599):
            for a in range(3):
                block += [(p, int(i)) for i in MS.motion_counters(t, a)]
        assert all(64 * t <= i < 64 * (t + 1) for _, i in block)
        assert all(0 <= i < 2 ** 32 for _, i in block)
        assert not seen & set(block) and len(set(block)) == len(block)
        seen |= set(block)
    assert len(seen) == 5 * (1 + 3 * 36)


def test_host_sincosf_is_the_oracles(oracle_mod):
    x = np.random.default_rng(1).uniform(-20, 20, 500).astype(f32)
    s, c = MS.NS.sincosf(x)
    so, co = oracle_mod.sincosf(x)
    assert s.tobytes() == so.tobytes() and c.tobytes() == co.tobytes()


def test_normal_draw_moments():
    """200 000 draws of the twelve-uniform normal: mean 0 and standard deviation 1 to three standard errors
    (0.0067 and 0.0047 at this count), nothing beyond +-6, and draws of different axes / steps are different streams."""
    p = np.arange(200_000)
    g = MS.normal12(9, p, 3, 1)
    assert abs(g.mean()) < 3 / np.sqrt(g.size)
    assert abs(g.std() - 1.0) < 3 / np.sqrt(2 * g.size)
    assert np.abs(g).max() < 6.0
    assert abs(np.corrcoef(g, MS.normal12(9, p, 3, 2))[0, 1]) < 0.01
    assert abs(np.corrcoef(g, MS.normal12(9, p, 4, 1))[0, 1]) < 0.01
    # the sum is the ascending one from 0.0
    u = uniform01(9, np.full(12, 5, np.uint64), MS.motion_counters(3, 1))
    s = 0.0
    for k in range(12):
        s += float(u[k])
    assert MS.normal12(9, [5], 3, 1)[0] == s - 6.0


def test_summation_order_witness():
    """The blocked order is told apart from the plain sequential one: at P = 600 with weights
    uniform(0.5, 1.5) 10^uniform(-30, -28), cum differs from np.cumsum in >= 40 % of the elements and W differs from the
    sequential sum on every one of 20 seeds (40-57 % and 20 of 20 when this was written).  At P = 257 the two orders
    coincide (one chunk and one element), so 257 is no witness shape."""
    for seed in range(20):
        rng = np.random.default_rng(seed)
        w = rng.uniform(0.5, 1.5, 600) * 10.0 ** rng.uniform(-30, -28, 600)
        seq = np.cumsum(w)
        assert (MS.cum(w) != seq).mean() >= 0.40, seed
        assert MS.bs(w) != seq[-1], seed
        assert np.allclose(MS.cum(w), seq, rtol=1e-12)
        w = w[:257]
        assert MS.cum(w).tobytes() == np.cumsum(w).tobytes() and MS.bs(w) == np.cumsum(w)[-1]


def test_blocked_sums_spelt_out():
    """bs and cum against explicit Python loops on an odd size (three chunks, the last one short)."""
    v = np.random.default_rng(3).uniform(0, 1, 600)
    tot, base, c = [], [], []
    for b in range(0, 600, 256):
        s = 0.0
        B = 0.0
        for x in tot:
            B += x
        base.append(B)
        for x in v[b:b + 256]:
            s += float(x)
            c.append(B + s)
        tot.append(s)
    W = 0.0
    for x in tot:
        W += x
    assert MS.bs(v) == W and MS.cum(v).tolist() == c


def _march_likelihood(g, om, mrx, angles, table):
    return MS.statement_likelihood(g, om, mrx, "canonical", angles, table)


def test_gpu_input_condition(oracle_mod):
    """The peaked-table input of tests/test_gpu_mcl.py exercises the resampling: in the statement at least a quarter of
    the particles are left without a descendant and some particle gets three or more, at every step."""
    g, z = load_golden("rm_maze256")
    fov, mrx = float(z["fov"]), int(z["max_range_px"])
    om = oracle_mod.OracleMap.from_gridmap(g, mrx)
    P, A, T = 600, 54, 3
    parts, angles, odom, obs, table = MS.localisation_case(g, om.dt, mrx, fov, P, A, T)
    f = MS.Filter(_march_likelihood(g, om, mrx, angles, table), P, (0.02, 0.02, 0.01), 2.0)
    f.reset(parts, seed=3)
    for t in range(T):
        _, neff, flags = f.step(odom[t], obs[t])
        n = np.bincount(f.anc, minlength=P)
        assert flags == MS.RESAMPLED and (n == 0).mean() >= 0.25 and n.max() >= 3, (t, neff)
        assert n.sum() == P and (np.diff(f.anc) >= 0).all()
        assert f.w.tobytes() == np.full(P, 1.0 / P).tobytes()


#: the arithmetic of the kinds the host can state (GiantLUT's statement reads the device's table)
_HOST_FORMS = {"RM-3": "literal", "RMGPU-1": "canonical", "CDDT": "cddt"}
_STD = (0.02, 0.02, 0.01)


def test_gpu_scale_input_condition(oracle_mod):
    """What tests/test_gpu_pf_scale.py relies on, in the statement alone.  Every row of MS.SCALE_ROWS, for every kind
    the host can state: with ratio 2.0 every step resamples and the last step's ancestors clear the row's (dead, most)
    bar — and the first step's the (0.25, 3) bar, 54-55 % and 4 at one beam —, the flags by ratio are MS.scale_flags,
    and at 131 073, 140 001 and 2^20 particles the blocked total of omega is not the sequential one, so the pinned order
    is still told apart from np.cumsum's.  Then the three inputs of the degenerate / dead-particle tests at 600 x 7."""
    g, z = load_golden("rm_maze256")
    fov, mrx = float(z["fov"]), int(z["max_range_px"])
    om = oracle_mod.OracleMap.from_gridmap(g, mrx)

    def run(P, A, T, form, ratio, table=None, weights=None):
        parts, angles, odom, obs, tb = MS.localisation_case(g, om.dt, mrx, fov, P, A, T)
        f = MS.Filter(MS.statement_likelihood(g, om, mrx, form, angles, tb if table is None else table(tb), 112), P, _STD, ratio)
        f.reset(parts, weights=weights, seed=3)
        rows = []
        with np.errstate(over="ignore", invalid="ignore"):
            for t in range(T):
                _, neff, flags = f.step(odom[t], obs[t])
                rows.append((flags, neff, np.bincount(f.anc, minlength=P)))
        return f, rows

    for P, A, T, kinds, ratios, dead, most in MS.SCALE_ROWS:
        for i, kind in enumerate(k for k in kinds if k in _HOST_FORMS):
            f, rows = run(P, A, T, _HOST_FORMS[kind], 2.0)          # (each shape once: 2^20 takes seconds)
            assert [r[0] for r in rows] == MS.scale_flags(A, T, 2.0), (P, kind)
            n = rows[0][2]
            assert (n == 0).mean() >= 0.25 and n.max() >= 3, (P, kind, (n == 0).mean(), n.max())
            n = rows[-1][2]
            assert (n == 0).mean() >= dead and n.max() >= most and n.sum() == P, (P, kind, (n == 0).mean(), n.max())
            if P > 131072:
                assert MS.bs(f.omega) != float(np.cumsum(f.omega)[-1]), (P, kind)
            for ratio in ratios[1:] if i == 0 else ():
                _, rows = run(P, A, T, _HOST_FORMS[kind], ratio)
                assert [r[0] for r in rows] == MS.scale_flags(A, T, ratio), (P, kind, ratio, [r[1] for r in rows])
    assert {r[0] for r in MS.SCALE_ROWS} >= {131073, 140001, 1 << 20}

    P, A = 600, 7
    # W = +inf at step 0 (degenerate, uniform weights), usable afterwards
    f, rows = run(P, A, 3, "canonical", 0.0, MS.overflow_table, np.full(P, 1e308))
    assert [r[0] for r in rows] == [MS.DEGENERATE, 0, 0]
    assert abs(rows[0][1] - 600.0) < 1e-6 and abs(rows[1][1] - 3.58) < 0.01 and abs(rows[2][1] - 1.04) < 0.01
    # W = NaN at every step, whatever the ratio; about 13 % of the likelihoods are NaN
    for ratio, flag in ((0.0, MS.DEGENERATE), (2.0, MS.DEGENERATE | MS.RESAMPLED)):
        f, rows = run(P, A, 3, "canonical", ratio, MS.nan_table)
        assert [r[0] for r in rows] == [flag] * 3 and 0.05 < np.isnan(f.L).mean() < 0.5
        assert np.isnan(MS.bs(f.omega)) and f.w.tobytes() == np.full(P, 1.0 / P).tobytes()
    # plateaus: most likelihoods are exactly zero, most steps of cum(w) are flat, and no ancestor had a zero weight
    f, rows = run(P, A, 3, "canonical", 2.0, MS.plateau_table)
    assert [r[0] for r in rows] == [MS.RESAMPLED] * 3
    assert (f.L == 0).mean() >= 0.5 and (np.diff(f.cum) == 0).mean() >= 0.5
    assert (f.omega[f.anc] > 0).all()


def test_estimate_converges_for_a_stationary_car(oracle_mod):
    """A stationary car, a Gaussian-diagonal table: after 10 steps the statement's position estimate is closer to the
    truth than at step 0."""
    g, z = load_golden("rm_maze256")
    fov, mrx = float(z["fov"]), int(z["max_range_px"])
    om = oracle_mod.OracleMap.from_gridmap(g, mrx)
    P, A, T = 300, 27, 10
    parts, angles, _, obs, _ = MS.localisation_case(g, om.dt, mrx, fov, P, A, 1)
    true = parts[0].copy()
    obs0 = PS.repeat_angles(g.occ, g.resolution, g.origin, mrx, true[None, :].astype(f32), angles, step_coeff=1.0, dt=om.dt)[0]
    parts = parts + np.array([2.0 * g.resolution, -2.0 * g.resolution, 0.0])      # a biased cloud
    f = MS.Filter(_march_likelihood(g, om, mrx, angles, MS.gaussian_table(mrx + 1)), P, (0.01, 0.01, 0.005), 0.5)
    f.reset(parts, seed=11)
    est, neff, flags = f.run(np.zeros((T, 3)), np.tile(obs0, (T, 1)))
    err = np.hypot(*(MS.pose_of(est)[:, :2] - true[None, :2]).T)
    assert err[-1] < err[0], err
    assert (flags & MS.RESAMPLED).any() and (neff > 1.0).all() and (neff <= P * (1 + 1e-9)).all()


def test_degenerate_and_never_resample_paths():
    P = 600
    rng = np.random.default_rng(4)
    parts = rng.uniform(-1, 1, (P, 3))
    odom, obs = np.array([[0.1, 0.0, 0.05]] * 2), np.zeros((2, 3), f32)
    # an all-zero likelihood: the degenerate flag, uniform weights, neff = P, the estimate the plain mean
    for bad in (0.0, np.nan, np.inf):
        f = MS.Filter(lambda q, o, t, bad=bad: np.full(P, bad), P, (0.0, 0.0, 0.0), 0.5)
        f.reset(parts, seed=1)
        est, neff, flags = f.step(odom[0], obs[0])
        assert flags == MS.DEGENERATE
        assert f.w.tobytes() == np.full(P, 1.0 / P).tobytes()
        assert abs(neff - P) < 1e-6 and abs(est[0] - f.X[:, 0].mean()) < 1e-12
        assert np.array_equal(f.anc, np.arange(P))
    # ... and with ratio 2 a degenerate step still resamples (uniformly: every particle keeps one descendant)
    f = MS.Filter(lambda q, o, t: np.zeros(P), P, (0.0, 0.0, 0.0), 2.0)
    f.reset(parts, seed=1)
    _, _, flags = f.step(odom[0], obs[0])
    assert flags == MS.DEGENERATE | MS.RESAMPLED and np.bincount(f.anc, minlength=P).max() <= 2
    # ratio 0: never resampled, the weights accumulate over the steps and stay normalised
    L = rng.uniform(0.1, 1.0, P)
    f = MS.Filter(lambda q, o, t: L, P, (0.01, 0.0, 0.0), 0.0)
    f.reset(parts, seed=1)
    x0 = f.X.copy()
    _, _, flags = f.run(odom, obs)
    assert not flags.any() and np.array_equal(f.anc, np.arange(P))
    w2 = L * L
    assert np.allclose(f.w, w2 / w2.sum(), rtol=1e-12) and abs(f.w.sum() - 1.0) < 1e-12
    # std = (s, 0, 0): only x is perturbed — y and theta are the noiseless motion's
    quiet = MS.motion(MS.motion(x0, odom[0], (0, 0, 0), 1, 0), odom[1], (0, 0, 0), 1, 1)
    assert np.array_equal(f.X[:, 2], quiet[:, 2]) and not np.array_equal(f.X[:, 0], quiet[:, 0])
    # the caller's weights are taken as given
    f.reset(parts, weights=np.arange(1, P + 1, dtype=np.float64), seed=1)
    assert f.w[5] == 6.0


def test_python_layer_is_exported():
    import pyracecarsimulator_amd as pkg
    from pyracecarsimulator_amd import _lib, particle_filter
    assert pkg.ParticleFilter is particle_filter.ParticleFilter
    assert hasattr(pkg.RacecarSimulator, "particleFilter")
    for name in ("rl_pf_create", "rl_pf_destroy", "rl_pf_reset", "rl_pf_run", "rl_pf_read"):
        assert name in _lib.SYMBOLS
    assert (particle_filter.RESAMPLED, particle_filter.DEGENERATE) == (MS.RESAMPLED, MS.DEGENERATE)
