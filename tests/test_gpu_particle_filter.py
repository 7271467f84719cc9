"""Particle-filter weights on the MI355X (rl_calc_range_repeat_angles, rl_set_sensor_model, rl_eval_sensor_model,
rl_calc_range_repeat_angles_eval_sensor_model and their Python forms): the repeat-angle scan against the handle's own
fan (the pin to the oracle) and against the oracle / tests/pf_statement.py on arbitrary angles, the weights against
the statement's ascending product bit for bit, fused against unfused, noise keyed by the global ray id, the
device-pointer forms, and every error of the contract."""
import ctypes as C

import numpy as np
import pytest

import pf_statement as PS
import pf_cases as PF
from pf_cases import MAPS, WEIGHT_KINDS as KINDS, WeightWorld as World
from support import same_bits
from pyracecarsimulator_amd import _lib, range_libc

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

f32 = np.float32
RL_ERR_INVALID, RL_ERR_UNSUPPORTED = -1, -4           # include/scanlib.h rl_status


@pytest.fixture(scope="module")
def worlds(oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = World(oracle_mod, name)
        return cache[name]
    return get


def _fan_equivalent(kind, fov, B):
    return PS.fan_angles_literal(fov, B) if KINDS[kind][4] == "literal" else PS.fan_angles(fov, B)


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
                got, got_h, got_s = PF.scan(m, poses, angles, aux=True)
                assert np.array_equal(got_h, want_h) and np.array_equal(got_s, want_s), (kind, name, B, P)
                some_hit |= bool((got_h[:, 0] >= 0).any())
            else:
                m.calc_range_fan(poses, want, w.fov, B)
                got = PF.scan(m, poses, angles)
            assert same_bits(got, want), (kind, name, B, P, np.abs(got - want).max())
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
            angles = PF.wild_angles(A, 100 + A)
            poses = np.ascontiguousarray(w.poses[:P])
            want = w.expect(kind, poses, angles, (A, P))
            got = PF.scan(m, poses, angles)
            assert same_bits(got, want), (kind, name, A, P, int((got != want).sum()))
            assert np.unique(got).size > min(A * P, 4) // 2


def test_out_of_map_and_huge_heading_particles(worlds):
    """Particles outside the map and with headings far beyond a turn: the march kinds answer as their statements do."""
    w = worlds(MAPS[1])
    poses = np.ascontiguousarray(w.poses[:9]).copy()
    span = w.g.cols * w.g.resolution
    poses[1, :2] += f32(3.0 * span)
    poses[4, 2] = f32(1234.5)
    poses[6, 0] -= f32(2.0 * span)
    angles = PF.wild_angles(65, 5)
    for kind in ("RM-3", "RMGPU-1"):
        got = PF.scan(w.method(kind), poses, angles)
        assert same_bits(got, w.expect(kind, poses, angles, "outside")), kind


# ---------------------------------------------------------------- 3. eval_sensor_model
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
                ranges = PF.planted_ranges(w, m, A, P, 7 * A + P)
                obs = PF.obs_of(w, A, A)
                got = np.full(P, -1.0)
                m.eval_sensor_model(obs, ranges, got, A, P)
                fac = PS.factors(table, obs, ranges, w.inv_res)
                want = PS.product_ascending(fac)
                assert same_bits(got, want), (width, A, P, block, int((got != want).sum()))
                assert np.isfinite(got).all() and (got > 0).all()
                if (A, P) == (54, 257):
                    differs = max(differs, int((want != PS.product_tree(fac)).sum()))
    finally:
        m.set_option("pf_block", 0)
    assert differs > 128                                  # (the order witness holds on the tested data too)


# ---------------------------------------------------------------- 4. the fused call
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
                angles = PF.wild_angles(A, 300 + A)
                poses = np.ascontiguousarray(w.poses[:P])
                obs = PF.obs_of(w, A, 3 * A)
                ranges, unfused = PF.unfused(m, poses, angles, obs)
                fused = PF.fused(m, poses, angles, obs)
                assert same_bits(fused, unfused), (kind, name, noise, A, P, block, int((fused != unfused).sum()))
                assert same_bits(fused, PS.weights(table, obs, ranges, w.inv_res)), (kind, name, noise, A, P, block)
                if not noise and (name == MAPS[0] or KINDS[kind][4] in ("literal", "canonical")):
                    assert same_bits(ranges, w.expect(kind, poses, angles, ("fused", A, P)))
            if noise:
                # the ray ids: with the fan's own angles the noisy ranges are the noisy fan's
                B, P = 65, 7
                poses = np.ascontiguousarray(w.poses[:P])
                want = np.empty(P * B, f32)
                m.calc_range_fan(poses, want, w.fov, B)
                got = PF.scan(m, poses, _fan_equivalent(kind, w.fov, B))
                assert same_bits(got, want), (kind, name)
                m.set_noise(0.0)
                clean = PF.scan(m, poses, _fan_equivalent(kind, w.fov, B))
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
        angles, obs = PF.wild_angles(A, 41), PF.obs_of(w, A, 42)
        poses = np.ascontiguousarray(w.poses[:P])
        ranges, unfused = PF.unfused(m, poses, angles, obs)
        fused = PF.fused(m, poses, angles, obs)
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
        assert same_bits(d_r.cpu().numpy(), ranges)
        assert same_bits(d_w[0].cpu().numpy(), unfused)
        assert same_bits(d_w[1].cpu().numpy(), fused) and same_bits(d_w[2].cpu().numpy(), fused)
        assert same_bits(fused, unfused)
        # options and the noise offset read the same afterwards: the host forms give the same bits again
        assert {k: m.get_info(k) for k in before} == before
        assert m.last_plan() == plan_before
        assert same_bits(PF.fused(m, poses, angles, obs), fused)
        assert same_bits(PF.scan(m, poses, angles), ranges)
    finally:
        m.set_noise(0.0)


# ---------------------------------------------------------------- 6. errors
def test_every_error_of_the_contract_and_a_correct_call_afterwards(worlds):
    w = worlds(MAPS[0])
    L = _lib.lib()
    m = range_libc.PyRayMarchingGPU(w.omap, w.mrx)          # a fresh handle: no table set yet
    A, P = 54, 7
    poses = np.ascontiguousarray(w.poses[:P])
    angles, obs = PF.wild_angles(A, 1), PF.obs_of(w, A, 2)
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
    good = PF.fused(m, poses, angles, obs)
    ranges = PF.scan(m, poses, angles)
    assert same_bits(good, PS.weights(table, obs, ranges, w.inv_res))
    assert same_bits(PF.fused(rep, poses, angles, obs), good)
    with pytest.raises(_lib.ScanLibError) as e:
        m.calc_range_repeat_angles(poses, np.zeros(2049, f32), np.zeros(P * 2049, f32))
    assert e.value.code == RL_ERR_INVALID
