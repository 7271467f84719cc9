"""Particle-filter weights, host side: the NumPy statement (tests/pf_statement.py) against the oracle's fans, the
product-order witness that lets the GPU tests tell summation orders apart, the sensor model's bin rule on its edge
values, and the Python layer's validation (which fires before the C ABI is reached)."""
import numpy as np
import pytest

import pf_statement as PS
from conftest import load_golden
from pyracecarsimulator_amd import range_libc

f32 = np.float32


def test_canonical_statement_with_fan_angles_equals_the_oracle_fan(oracle_mod):
    g, z = load_golden("rm_maze256")
    fov, B, mrx = float(z["fov"]), int(z["num_rays"]), int(z["max_range_px"])
    om = oracle_mod.OracleMap.from_gridmap(g, mrx)
    poses = np.ascontiguousarray(z["poses"][:6], f32)
    for coeff in (0.999, 1.0):
        want_r, want_h, want_s = om.rm_fan(poses, fov, B, step_coeff=coeff)
        got_r, got_h, got_s = PS.repeat_angles(g.occ, g.resolution, g.origin, mrx, poses, PS.fan_angles(fov, B),
                                               step_coeff=coeff, dt=om.dt)
        assert got_r.tobytes() == want_r.tobytes()
        assert np.array_equal(got_h, want_h) and np.array_equal(got_s, want_s)
    assert (want_h[:, 0] >= 0).mean() > 0.5                  # (most beams hit something: the hit branch is exercised)


def test_literal_expansion_equals_the_oracle_literal_fan(oracle_mod):
    for name in ("rm_maze256", "rm_maze192_yaw"):
        g, z = load_golden(name)
        fov, B, mrx = float(z["fov"]), int(z["num_rays"]), int(z["max_range_px"])
        om = oracle_mod.OracleMap.from_gridmap(g, mrx)
        poses = np.ascontiguousarray(z["poses"][:6], f32)
        want_r, want_h, want_s = om.rm_fan_libm(poses, fov, B, step_coeff=0.999)
        rows = PS.expand_rows(poses, PS.fan_angles_literal(fov, B))
        got_r, got_h, got_s = om.rm_rays_libm(rows, step_coeff=0.999, full=True)
        assert got_r.tobytes() == want_r.tobytes(), name
        assert np.array_equal(got_h, want_h) and np.array_equal(got_s, want_s), name


@pytest.mark.parametrize("A", [54, 65, 130])
def test_product_order_witness(A):
    """The ascending product is told apart from a halving tree and from the descending order on most particles: a
    kernel that multiplied in another order would fail the bit-for-bit weight tests.  With this table and these seeds
    the ascending product differs from the tree on 84-93 % of the 257 particles and from the descending order on
    86-91 %; the assertion is "more than half"."""
    table = PS.witness_table()
    rng = np.random.default_rng(A)
    P, width = 257, table.shape[0]
    fac = table[rng.integers(0, width, A)[None, :], rng.integers(0, width, (P, A))]
    up, down, tree = PS.product_ascending(fac), PS.product_descending(fac), PS.product_tree(fac)
    assert np.allclose(up, tree, rtol=1e-12) and np.allclose(up, down, rtol=1e-12)
    assert (up != tree).sum() > P // 2, (up != tree).mean()
    assert (up != down).sum() > P // 2, (up != down).mean()
    assert PS.weights(table, np.zeros(A, f32), np.zeros((P, A), f32), f32(20.0)).tobytes() == \
        PS.product_ascending(np.full((P, A), table[0, 0])).tobytes()


def test_sensor_bin_edge_values():
    res = f32(0.05)
    inv = PS.inv_res_of(res)
    width = 120
    top = f32(width - 1) * res                                    # exactly (width - 1) * res
    assert PS.sensor_bin(f32(-3.0), inv, width) == 0
    assert PS.sensor_bin(f32(-0.0), inv, width) == 0
    assert PS.sensor_bin(top, inv, width) == width - 1
    assert PS.sensor_bin(f32(1e9), inv, width) == width - 1
    assert PS.sensor_bin(f32(np.inf), inv, width) == width - 1
    assert PS.sensor_bin(f32(-np.inf), inv, width) == 0
    assert PS.sensor_bin(f32(np.nan), inv, width) == 0
    # a value below 7 cells in real arithmetic whose float32 product v * inv_res rounds up to 7.0: the bin is the
    # float32 product's, not the real quotient's
    found = None
    for k in range(1, 4000):
        v = np.nextafter(f32(k) * res, f32(0), dtype=f32)
        if float(v) / float(res) < k and f32(v * inv) == f32(k):
            found = (k, v)
            break
    assert found is not None
    k, v = found
    assert PS.sensor_bin(v, inv, 4096) == k
    assert int(float(v) / float(res)) == k - 1
    got = PS.sensor_bin(np.array([0.0, 0.049, 0.051, 5.93, 5.96], f32), inv, width)
    assert got.tolist() == [0, 0, 1, 118, 119]


def _bare(cls=range_libc.PyRayMarchingGPU):
    """A method object without a handle: validation raises before the library is touched."""
    m = object.__new__(cls)
    m._h = None
    return m


def test_python_layer_validation_fires_before_the_abi_call():
    m = _bare()
    ins = np.zeros((5, 3), f32)
    ang = np.zeros(7, f32)
    outs = np.zeros(35, f32)
    obs = np.zeros(7, f32)
    w = np.zeros(5, np.float64)
    V, T = ValueError, TypeError
    for exc, args in [(V, (ins.astype(np.float64), ang, outs)), (V, (ins[:, :2], ang, outs)), (V, (ins.ravel(), ang, outs)),
                      (V, (np.zeros((10, 3), f32)[::2], ang, outs)), (V, (ins, ang.astype(np.float64), outs)),
                      (V, (ins, ang.reshape(1, 7), outs)), (V, (ins, np.zeros(14, f32)[::2], outs)),
                      (V, (ins, ang, outs[:34])), (V, (ins, ang, np.zeros(36, f32))), (V, (ins, ang, outs.astype(np.float64))),
                      (T, ([[0, 0, 0]], ang, outs)), (T, (ins, [0.0], outs)), (T, (ins, ang, None))]:
        with pytest.raises(exc):
            m.calc_range_repeat_angles(*args)
    with pytest.raises(V):
        m.calc_range_repeat_angles(ins, ang, outs, hit_cells=np.zeros((35, 2), np.int64))
    with pytest.raises(V):
        m.calc_range_repeat_angles(ins, ang, outs, steps=np.zeros(34, np.uint16))
    for exc, t in [(T, [[1.0, 2.0], [3.0, 4.0]]), (V, np.ones((4, 4), f32)), (V, np.ones((4, 5))), (V, np.ones(16)),
                   (V, np.ones((2, 2, 2)))]:
        with pytest.raises(exc):
            m.set_sensor_model(t)
    for exc, args in [(V, (obs[:6], np.zeros(35, f32), w, 7, 5)), (V, (obs, np.zeros(34, f32), w, 7, 5)),
                      (V, (obs, np.zeros(35, f32), w.astype(f32), 7, 5)), (V, (obs, np.zeros(35, f32), w[:4], 7, 5)),
                      (V, (obs.astype(np.float64), np.zeros(35, f32), w, 7, 5)), (T, (obs, None, w, 7, 5)),
                      (T, (obs, np.zeros(35, f32), [0.0] * 5, 7, 5))]:
        with pytest.raises(exc):
            m.eval_sensor_model(*args)
    for exc, args in [(V, (ins, ang, obs[:6], w)), (V, (ins, ang, obs, w[:4])), (V, (ins, ang, obs, w.astype(f32))),
                      (V, (ins, ang, obs, np.zeros((5, 1)))), (V, (ins.T.copy().T, ang, obs, w)), (T, (ins, ang, obs, None)),
                      (T, (None, ang, obs, w))]:
        with pytest.raises(exc):
            m.calc_range_repeat_angles_eval_sensor_model(*args)
