"""Particle-filter weights on the MI355X (rl_calc_range_repeat_angles, rl_set_sensor_model, rl_eval_sensor_model,
rl_calc_range_repeat_angles_eval_sensor_model and their Python forms): the repeat-angle scan against the handle's own
fan (the pin to the oracle) and against the oracle / tests/pf_statement.py on arbitrary angles, the weights against
the statement's ascending product bit for bit, fused against unfused, noise keyed by the global ray id, the
device-pointer forms, and every error of the contract."""
import ctypes as C
import math

import numpy as np
import pytest

import pf_statement as PS
from conftest import load_golden
from pyracecarsimulator_amd import _lib, maps, range_libc

pytestmark = pytest.mark.gpu

f32 = np.float32
RL_ERR_INVALID, RL_ERR_UNSUPPORTED = -1, -4           # include/scanlib.h rl_status
THETA = 112
#: name -> (class, extra constructor arguments, variant or None, step coefficient, arithmetic)
KINDS = {
    "RM-3": (range_libc.PyRayMarching, (), 3, 0.999, "literal"),
    "RM-1": (range_libc.PyRayMarching, (), 1, 0.999, "canonical"),
    "RMGPU-1": (range_libc.PyRayMarchingGPU, (), 1, 1.0, "canonical"),
    "RMGPU-3": (range_libc.PyRayMarchingGPU, (), 3, 1.0, "literal"),
    "CDDT": (range_libc.PyCDDTCast, (THETA,), None, None, "cddt"),
    "GLT": (range_libc.PyGiantLUTCast, (THETA,), None, None, "lut"),
}
MAPS = ("rm_maze256", "rm_maze192_yaw")              # yaw 0 / yawed origin


@pytest.fixture(scope="module", autouse=True)
def _gpu(need_gpu):
    yield


class World:
    """One fixture map: the device map, the oracle map, 257 free poses, and the handles made on it."""

    def __init__(self, oracle_mod, name):
        self.name = name
        self.g, z = load_golden(name)
        self.fov, self.mrx = float(z["fov"]), int(z["max_range_px"])
        self.om = oracle_mod.OracleMap.from_gridmap(self.g, self.mrx)
        self.omap = range_libc.PyOMap(self.g)
        self.poses = np.ascontiguousarray(maps.sample_free_poses(self.g, 257, 31, 2.0, self.om.dt), f32)
        self.inv_res = PS.inv_res_of(self.g.resolution)
        self.methods, self.expected = {}, {}

    def method(self, kind):
        if kind not in self.methods:
            cls, extra, variant, _, _ = KINDS[kind]
            m = cls(self.omap, self.mrx, *extra)
            if variant is not None:
                m.set_option("variant", variant)
            self.methods[kind] = m
        return self.methods[kind]

    def expect(self, kind, poses, angles, key):
        """Ranges of the repeat-angle scan by the oracle / the statement; computed once per (arithmetic, shape)."""
        _, _, _, coeff, form = KINDS[kind]
        key = (form, coeff, key)
        if key not in self.expected:
            rows = PS.expand_rows(poses, angles)
            if form == "literal":
                want = self.om.rm_rays_libm(rows, step_coeff=coeff)
            elif form == "canonical":
                want = PS.repeat_angles(self.g.occ, self.g.resolution, self.g.origin, self.mrx, poses, angles,
                                        step_coeff=coeff, dt=self.om.dt)[0]
            elif form == "cddt":
                want = self.om.cddt_rays(THETA, rows)
            else:
                want = self.om.lut_rays(self.method(kind).table(), rows)
            self.expected[key] = want
        return self.expected[key]


@pytest.fixture(scope="module")
def worlds(oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = World(oracle_mod, name)
        return cache[name]
    return get


def _same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _fan_equivalent(kind, fov, B):
    return PS.fan_angles_literal(fov, B) if KINDS[kind][4] == "literal" else PS.fan_angles(fov, B)


def _wild_angles(A, seed):
    """Non-monotone, with duplicates, with values beyond +-pi."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-4.0 * math.pi, 4.0 * math.pi, A).astype(f32)
    if A >= 8:
        a[A // 2] = a[1]
        a[A - 1] = a[0]
        a[2], a[3] = f32(7.5), f32(-9.25)
        a[5] = f32(0.0)
    return a


def _scan(m, poses, angles, aux=False):
    n = poses.shape[0] * angles.size
    outs = np.full(n, -7.0, f32)
    if not aux:
        m.calc_range_repeat_angles(poses, angles, outs)
        return outs
    hits, steps = np.full((n, 2), -9, np.int32), np.full(n, 9, np.uint16)
    m.calc_range_repeat_angles(poses, angles, outs, hits, steps)
    return outs, hits, steps


def _obs_of(w, A, seed):
    """An observed scan: plausible ranges with a few values off the table's ends."""
    rng = np.random.default_rng(seed)
    obs = rng.uniform(0.0, w.mrx * w.g.resolution, A).astype(f32)
    if A >= 8:
        obs[0], obs[3], obs[6] = f32(-1.0), f32(1e6), f32(np.nan)
    return obs


# ---------------------------------------------------------------- 1. fan equivalence
@pytest.mark.parametrize("name", MAPS)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_repeat_angles_of_the_fans_own_angles_equal_the_fan(worlds, kind, name):
    w = worlds(name)
    m = w.method(kind)
    aux = KINDS[kind][4] in ("literal", "canonical")
    some_hit = False
    for B in (10, 65, 1081):
        angles = _fan_equivalent(kind, w.fov, B)
        for P in (1, 7):
            poses = np.ascontiguousarray(w.poses[3:3 + P])
            want = np.empty(P * B, f32)
            if aux:
                want_h, want_s = np.empty((P * B, 2), np.int32), np.empty(P * B, np.uint16)
                m.calc_range_fan(poses, want, w.fov, B, want_h, want_s)
                got, got_h, got_s = _scan(m, poses, angles, aux=True)
                assert np.array_equal(got_h, want_h) and np.array_equal(got_s, want_s), (kind, name, B, P)
                some_hit |= bool((got_h[:, 0] >= 0).any())
            else:
                m.calc_range_fan(poses, want, w.fov, B)
                got = _scan(m, poses, angles)
            assert _same_bits(got, want), (kind, name, B, P, np.abs(got - want).max())
    assert some_hit or not aux


# ---------------------------------------------------------------- 2. arbitrary angles
SHAPES = [(A, P) for A in (1, 54, 65, 130) for P in (1, 7, 257)] + [(2048, 2)]


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_arbitrary_angles_equal_the_oracle(worlds, kind):
    form = KINDS[kind][4]
    for name in (MAPS if form in ("literal", "canonical") else MAPS[:1]):       # (table kinds: the yaw-0 map)
        w = worlds(name)
        m = w.method(kind)
        for A, P in SHAPES:
            angles = _wild_angles(A, 100 + A)
            poses = np.ascontiguousarray(w.poses[:P])
            want = w.expect(kind, poses, angles, (A, P))
            got = _scan(m, poses, angles)
            assert _same_bits(got, want), (kind, name, A, P, int((got != want).sum()))
            assert np.unique(got).size > min(A * P, 4) // 2


def test_out_of_map_and_huge_heading_particles(worlds):
    """Particles outside the map and with headings far beyond a turn: the march kinds answer as their statements do."""
    w = worlds(MAPS[1])
    poses = np.ascontiguousarray(w.poses[:9]).copy()
    span = w.g.cols * w.g.resolution
    poses[1, :2] += f32(3.0 * span)
    poses[4, 2] = f32(1234.5)
    poses[6, 0] -= f32(2.0 * span)
    angles = _wild_angles(65, 5)
    for kind in ("RM-3", "RMGPU-1"):
        got = _scan(w.method(kind), poses, angles)
        assert _same_bits(got, w.expect(kind, poses, angles, "outside")), kind


# ---------------------------------------------------------------- 3. eval_sensor_model
def _planted_ranges(w, m, A, P, seed, poses=None):
    """Ranges of a real scan (of ``poses``, else the world's first P) with planted values: negative, NaN, above the
    table, on and next to bin edges."""
    angles = _wild_angles(A, seed)
    r = _scan(m, np.ascontiguousarray(w.poses[:P] if poses is None else poses[:P]), angles).copy()
    rng = np.random.default_rng(seed)
    res = f32(w.g.resolution)
    for v in (f32(-0.3), f32(np.nan), f32(1e5), f32(np.inf), f32(-np.inf), f32(-0.0)):
        r[rng.integers(0, r.size, 5)] = v
    k = rng.integers(1, 60, 40).astype(f32)
    edges = (k * res).astype(f32)
    idx = rng.choice(r.size, 120, replace=False)
    r[idx[:40]] = edges
    r[idx[40:80]] = np.nextafter(edges, f32(0), dtype=f32)
    r[idx[80:]] = np.nextafter(edges, f32(1e9), dtype=f32)
    return r


def test_eval_sensor_model_equals_the_statement(worlds):
    w = worlds(MAPS[0])
    m = w.method("RMGPU-1")
    differs = 0
    try:
        for width in (301, 64):                           # (the second table replaces the first on the same handle)
            table = PS.witness_table(width, seed=20 + width)
            m.set_sensor_model(table)
            for (A, P), block in [((54, 257), 0), ((54, 257), 38), ((54, 257), 5), ((65, 7), 0), ((130, 257), 0),
                                  ((1, 257), 0), ((2048, 2), 0), ((2048, 2), 2)]:
                m.set_option("pf_block", block)
                ranges = _planted_ranges(w, m, A, P, 7 * A + P)
                obs = _obs_of(w, A, A)
                got = np.full(P, -1.0)
                m.eval_sensor_model(obs, ranges, got, A, P)
                fac = PS.factors(table, obs, ranges, w.inv_res)
                want = PS.product_ascending(fac)
                assert _same_bits(got, want), (width, A, P, block, int((got != want).sum()))
                assert np.isfinite(got).all() and (got > 0).all()
                if (A, P) == (54, 257):
                    differs = max(differs, int((want != PS.product_tree(fac)).sum()))
    finally:
        m.set_option("pf_block", 0)
    assert differs > 128                                  # (the order witness holds on the tested data too)


# ---------------------------------------------------------------- 4. the fused call
def _fused(m, poses, angles, obs):
    wts = np.full(poses.shape[0], -1.0)
    m.calc_range_repeat_angles_eval_sensor_model(poses, angles, obs, wts)
    return wts


def _unfused(m, poses, angles, obs):
    ranges = _scan(m, poses, angles)
    wts = np.full(poses.shape[0], -1.0)
    m.eval_sensor_model(obs, ranges, wts, angles.size, poses.shape[0])
    return ranges, wts


@pytest.mark.parametrize("name", MAPS)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_fused_equals_unfused_equals_the_statement(worlds, kind, name):
    w = worlds(name)
    m = w.method(kind)
    table = PS.witness_table(301, seed=5)
    m.set_sensor_model(table)
    try:
        for noise in (False, True):
            if noise:
                m.set_noise(0.02, seed=77, ray_offset=123457)
            for (A, P), block in [((54, 257), 0), ((54, 257), 38), ((54, 257), 5), ((65, 7), 0), ((130, 40), 0),
                                  ((1, 257), 0), ((2048, 2), 0)]:
                m.set_option("pf_block", block)
                angles = _wild_angles(A, 300 + A)
                poses = np.ascontiguousarray(w.poses[:P])
                obs = _obs_of(w, A, 3 * A)
                ranges, unfused = _unfused(m, poses, angles, obs)
                fused = _fused(m, poses, angles, obs)
                assert _same_bits(fused, unfused), (kind, name, noise, A, P, block, int((fused != unfused).sum()))
                assert _same_bits(fused, PS.weights(table, obs, ranges, w.inv_res)), (kind, name, noise, A, P, block)
                if not noise and (name == MAPS[0] or KINDS[kind][4] in ("literal", "canonical")):
                    assert _same_bits(ranges, w.expect(kind, poses, angles, ("fused", A, P)))
            if noise:
                # the ray ids: with the fan's own angles the noisy ranges are the noisy fan's
                B, P = 65, 7
                poses = np.ascontiguousarray(w.poses[:P])
                want = np.empty(P * B, f32)
                m.calc_range_fan(poses, want, w.fov, B)
                got = _scan(m, poses, _fan_equivalent(kind, w.fov, B))
                assert _same_bits(got, want), (kind, name)
                m.set_noise(0.0)
                clean = _scan(m, poses, _fan_equivalent(kind, w.fov, B))
                assert (clean != got).mean() > 0.9
    finally:
        m.set_noise(0.0)
        m.set_option("pf_block", 0)


# ---------------------------------------------------------------- 5. device-pointer forms
@pytest.mark.parametrize("kind", ["RM-3", "RMGPU-1", "CDDT", "GLT"])
def test_device_pointer_forms_equal_the_host_forms(worlds, kind):
    import torch
    w = worlds(MAPS[0])
    m = w.method(kind)
    A, P = 54, 257
    table = PS.witness_table(301, seed=9)
    m.set_sensor_model(table)
    m.set_noise(0.01, seed=5, ray_offset=999)
    try:
        angles, obs = _wild_angles(A, 41), _obs_of(w, A, 42)
        poses = np.ascontiguousarray(w.poses[:P])
        ranges, unfused = _unfused(m, poses, angles, obs)
        fused = _fused(m, poses, angles, obs)
        before = {k: m.get_info(k) for k in ("variant", "pf_block", "slots", "timing", "grid_mult")}
        plan_before = m.last_plan()
        dev = torch.device("cuda:0")
        d_poses, d_ang, d_obs = (torch.from_numpy(a).to(dev) for a in (poses, angles, obs))
        d_r = torch.full((P * A,), -3.0, dtype=torch.float32, device=dev)
        d_w = [torch.full((P,), -3.0, dtype=torch.float64, device=dev) for _ in range(3)]
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        assert s.cuda_stream != 0
        with torch.cuda.stream(s):
            m.calc_range_repeat_angles_device(d_poses.data_ptr(), P, d_ang.data_ptr(), A, d_r.data_ptr(), stream=s.cuda_stream)
            m.eval_sensor_model_device(d_obs.data_ptr(), d_r.data_ptr(), d_w[0].data_ptr(), A, P, stream=s.cuda_stream)
            for k in (1, 2):                                  # two fused calls back to back on one handle
                m.calc_range_repeat_angles_eval_sensor_model_device(d_poses.data_ptr(), P, d_ang.data_ptr(), d_obs.data_ptr(),
                                                                    A, d_w[k].data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        assert _same_bits(d_r.cpu().numpy(), ranges)
        assert _same_bits(d_w[0].cpu().numpy(), unfused)
        assert _same_bits(d_w[1].cpu().numpy(), fused) and _same_bits(d_w[2].cpu().numpy(), fused)
        assert _same_bits(fused, unfused)
        # options and the noise offset read the same afterwards: the host forms give the same bits again
        assert {k: m.get_info(k) for k in before} == before
        assert m.last_plan() == plan_before
        assert _same_bits(_fused(m, poses, angles, obs), fused)
        assert _same_bits(_scan(m, poses, angles), ranges)
    finally:
        m.set_noise(0.0)


# ---------------------------------------------------------------- 6. errors
def test_every_error_of_the_contract_and_a_correct_call_afterwards(worlds):
    w = worlds(MAPS[0])
    L = _lib.lib()
    m = range_libc.PyRayMarchingGPU(w.omap, w.mrx)          # a fresh handle: no table set yet
    A, P = 54, 7
    poses = np.ascontiguousarray(w.poses[:P])
    angles, obs = _wild_angles(A, 1), _obs_of(w, A, 2)
    outs, wts = np.zeros(P * A, f32), np.zeros(P)
    table = PS.witness_table(64)
    p_ins, p_ang, p_obs = poses.ctypes.data_as(_lib.f32p), angles.ctypes.data_as(_lib.f32p), obs.ctypes.data_as(_lib.f32p)
    p_out, p_w, p_t = outs.ctypes.data_as(_lib.f32p), wts.ctypes.data_as(_lib.f64p), table.ctypes.data_as(_lib.f64p)
    h = m._h

    def scan(h=h, ins=p_ins, n=P, ang=p_ang, a=A, out=p_out):
        return L.rl_calc_range_repeat_angles(h, ins, n, ang, a, out, None, None)

    def ev(h=h, o=p_obs, r=p_out, a=A, n=P, wt=p_w):
        return L.rl_eval_sensor_model(h, o, r, a, n, wt)

    def fused(h=h, ins=p_ins, n=P, ang=p_ang, o=p_obs, a=A, wt=p_w):
        return L.rl_calc_range_repeat_angles_eval_sensor_model(h, ins, n, ang, o, a, wt)

    # evaluating before a table is set
    assert ev() == RL_ERR_INVALID and fused() == RL_ERR_INVALID
    assert b"sensor model" in L.rl_last_error()
    assert scan() == 0                                       # (the plain scan needs none)
    # the table's width
    for width in (1, 0, -3, 2049):
        assert L.rl_set_sensor_model(h, p_t, width) == RL_ERR_INVALID
    assert L.rl_set_sensor_model(h, None, 64) == RL_ERR_INVALID
    assert L.rl_set_sensor_model(None, p_t, 64) == RL_ERR_INVALID
    assert L.rl_set_sensor_model(h, p_t, 64) == 0
    # null pointers
    assert scan(h=None) == scan(ins=None) == scan(ang=None) == scan(out=None) == RL_ERR_INVALID
    assert ev(h=None) == ev(o=None) == ev(r=None) == ev(wt=None) == RL_ERR_INVALID
    assert fused(h=None) == fused(ins=None) == fused(ang=None) == fused(o=None) == fused(wt=None) == RL_ERR_INVALID
    # shapes
    for call in (scan, ev, fused):
        assert call(n=-1) == RL_ERR_INVALID
        assert call(a=0) == call(a=-5) == call(a=2049) == RL_ERR_INVALID
        assert call(n=1 << 20, a=2048) == RL_ERR_INVALID      # 2^31 rays (refused before anything is read)
        assert call(n=0) == 0                                 # nothing to do
    # the device forms check the same things (nothing is launched)
    void = C.c_void_p
    one = void(256)
    assert L.rl_calc_range_repeat_angles_device(h, None, P, one, A, one, None, None, None) == RL_ERR_INVALID
    assert L.rl_calc_range_repeat_angles_device(h, one, P, one, 2049, one, None, None, None) == RL_ERR_INVALID
    assert L.rl_eval_sensor_model_device(h, one, None, A, P, one, None) == RL_ERR_INVALID
    assert L.rl_eval_sensor_model_device(h, one, one, A, -1, one, None) == RL_ERR_INVALID
    assert L.rl_calc_range_repeat_angles_eval_sensor_model_device(h, one, P, one, one, A, None, None) == RL_ERR_INVALID
    assert L.rl_calc_range_repeat_angles_eval_sensor_model_device(h, one, 1 << 20, one, one, 2048, one, None) == RL_ERR_INVALID
    # kinds and variants without a repeat-angle form
    bl = range_libc.PyBresenhamsLine(w.omap, w.mrx)
    assert scan(h=bl._h) == RL_ERR_UNSUPPORTED and fused(h=bl._h) == RL_ERR_UNSUPPORTED
    m.set_option("variant", 2)
    assert scan() == RL_ERR_UNSUPPORTED and fused() == RL_ERR_UNSUPPORTED
    m.set_option("variant", 1)
    cd = w.method("CDDT")
    hits = np.zeros((P * A, 2), np.int32)
    assert L.rl_calc_range_repeat_angles(cd._h, p_ins, P, p_ang, A, p_out, hits.ctypes.data_as(_lib.i32p), None) == RL_ERR_UNSUPPORTED
    # multi-device handles
    momap = range_libc.PyOMap(w.g, device=[0, 0])
    mm = range_libc.PyRayMarchingGPU(momap, w.mrx)
    assert L.rl_set_sensor_model(mm._h, p_t, 64) == RL_ERR_INVALID
    assert scan(h=mm._h) == ev(h=mm._h) == fused(h=mm._h) == RL_ERR_INVALID
    assert b"multi-device" in L.rl_last_error()
    rep = mm.replica(1)                                       # ... whose replicas are ordinary handles
    rep.set_sensor_model(table)
    # a correct call on the same handle afterwards succeeds, with the right answer
    good = _fused(m, poses, angles, obs)
    ranges = _scan(m, poses, angles)
    assert _same_bits(good, PS.weights(table, obs, ranges, w.inv_res))
    assert _same_bits(_fused(rep, poses, angles, obs), good)
    with pytest.raises(_lib.ScanLibError) as e:
        m.calc_range_repeat_angles(poses, np.zeros(2049, f32), np.zeros(P * 2049, f32))
    assert e.value.code == RL_ERR_INVALID
