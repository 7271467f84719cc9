"""Particle-filter localisation on the MI355X (rl_pf_*, pyracecarsimulator_amd.ParticleFilter) against the NumPy statement
tests/mcl_statement.py, bit for bit: the per-step estimate, neff and flags, and the final particles, weights, ancestors,
cumulative weights and likelihoods, for every kind the fused weight call serves, always / never / sometimes resampling;
run(3) against run(1) + run(2); the likelihood against the public fused call, scan noise included; motion noise on, off
and per axis; the degenerate step; reset; and every error of the contract."""
import ctypes as C

import numpy as np
import pytest

import mcl_statement as MS
from pf_cases import MAPS, MCL_KINDS as KINDS, STD, T, MclWorld as World, assert_equal_to_statement, both, mcl_fused
from support import same_bits
from pyracecarsimulator_amd import ParticleFilter, _lib, range_libc

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

f32 = np.float32
RL_ERR_INVALID, RL_ERR_UNSUPPORTED = -1, -4           # include/scanlib.h rl_status
#: (P, A, resample ratio): every P of {1, 256, 600} and A of {1, 7, 54}; ratio 2 always resamples, 0 never, 0.5 as neff says
RUNS = [(600, 54, 2.0), (256, 7, 2.0), (1, 1, 2.0), (600, 7, 0.0), (256, 1, 0.5), (1, 54, 0.5)]


@pytest.fixture(scope="module")
def worlds(oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = World(oracle_mod, name)
        return cache[name]
    return get


# ---------------------------------------------------------------- 1. the statement, bit for bit
@pytest.mark.parametrize("name", MAPS)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_runs_equal_the_statement(worlds, kind, name):
    w = worlds(name)
    seen = 0
    for P, A, ratio in RUNS:
        pf, out, st, want = both(w, kind, P, A, ratio)
        assert_equal_to_statement(pf, out, st, want, (kind, name, P, A, ratio))
        seen |= 1 << int(out[2][-1])
        if ratio == 2.0:
            assert (out[2] & MS.RESAMPLED).all()
            if P == 600:                                  # the resampling did something: particles died and multiplied
                n = np.bincount(pf.read()["ancestors"], minlength=P)
                assert (n == 0).mean() >= 0.25 and n.max() >= 3
        if ratio == 0.0:
            assert not out[2].any() and same_bits(pf.read()["ancestors"], np.arange(P, dtype=np.int32))
        pf.close()
    assert seen & 0b11 == 0b11                            # runs ended both on a resampled and on a kept step


def test_multi_pass_tiles_and_given_weights(worlds):
    """pf_block forced to 2 (the weight launch has several tiles: 128 at P = 256, on a grid of min(128, 8 n_cu), so on a
    part of 16 CUs or more every workgroup still takes one; tests/test_gpu_pf_scale.py has workgroups take a second and a
    third), and a reset with the caller's weights, taken as given (they need not sum to one)."""
    w = worlds(MAPS[0])
    m = w.method("RMGPU-1")
    m.set_option("pf_block", 2)
    try:
        given = np.random.default_rng(8).uniform(0.5, 1.5, 256) * 1e-29
        pf, out, st, want = both(w, "RMGPU-1", 256, 7, 0.5, weights=given)
        assert_equal_to_statement(pf, out, st, want, "pf_block 2")
        assert m.get_info("pf_block") == 2
    finally:
        m.set_option("pf_block", 0)


def test_motion_noise_off_and_per_axis(worlds):
    w = worlds(MAPS[1])
    got = {}
    for std in ((0.0, 0.0, 0.0), (0.03, 0.0, 0.0), (0.0, 0.0, 0.02)):
        pf, out, st, want = both(w, "RM-3", 600, 7, 0.0, std=std)
        assert_equal_to_statement(pf, out, st, want, std)
        got[std] = pf.read()["particles"]
    # an axis with std 0 draws nothing and adds nothing: with noise on x alone, y and theta are the quiet run's
    quiet, x_only, th_only = (got[k] for k in ((0.0, 0.0, 0.0), (0.03, 0.0, 0.0), (0.0, 0.0, 0.02)))
    assert same_bits(x_only[:, 1:], quiet[:, 1:]) and (x_only[:, 0] != quiet[:, 0]).mean() > 0.9
    assert (th_only[:, 2] != quiet[:, 2]).mean() > 0.9


# ---------------------------------------------------------------- 2. composition
@pytest.mark.parametrize("kind", ["RMGPU-1", "CDDT"])
def test_run_three_equals_run_one_then_two(worlds, kind):
    w = worlds(MAPS[0])
    P, A = 600, 54
    parts, angles, odom, obs, table = w.case(P, A)
    m = w.method(kind)
    m.set_sensor_model(table)
    m.set_noise(0.02, seed=7, ray_offset=1000)               # (the scan noise's offset follows t, not the call)
    try:
        a = ParticleFilter(m, angles, P, motion_std=STD, resample_ratio=0.5)
        b = ParticleFilter(m, angles, P, motion_std=STD, resample_ratio=0.5)
        a.reset(parts, seed=5)
        b.reset(parts, seed=5)
        whole = a.run_raw(odom, obs)
        first = b.run_raw(odom[:1], obs[:1])
        rest = b.run_raw(odom[1:], obs[1:])
        for x, y, z in zip(whole, first, rest):
            assert same_bits(x, np.concatenate([y, z]))
        ra, rb = a.read(), b.read()
        assert all(same_bits(ra[k], rb[k]) for k in ra)
        # the poses of run() are the raw sums' (x, y, atan2(sin, cos))
        a.reset(parts, seed=5)
        poses, neff, flags = a.run(odom, obs)
        assert same_bits(poses, MS.pose_of(whole[0])) and same_bits(neff, whole[1]) and same_bits(flags, whole[2])
        # step() is run() of one row
        b.reset(parts, seed=5)
        pose, ne, fl = b.step(odom[0], obs[0])
        assert same_bits(pose, poses[0]) and ne == neff[0] and fl == flags[0]
    finally:
        m.set_noise(0.0)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_likelihood_is_the_public_fused_call_scan_noise_included(worlds, kind):
    """Never resampling, read()'s particles are X' of the last step: L is the public fused call of their float32 cast
    at ray offset (entry offset + t P A), the weights are omega / W of it, and the handle's offset and options read the
    same afterwards."""
    w = worlds(MAPS[0])
    P, A = 600, 54
    parts, angles, odom, obs, table = w.case(P, A)
    m = w.method(kind)
    m.set_sensor_model(table)
    R0 = 123457
    try:
        for noise in (0.0, 0.02):
            m.set_noise(noise, seed=77, ray_offset=R0)
            before = {k: m.get_info(k) for k in ("variant", "pf_block", "slots", "timing", "grid_mult")}
            pf = ParticleFilter(m, angles, P, motion_std=STD, resample_ratio=0.0)
            Ls = []
            for n_steps in (1, 3):
                pf.reset(parts, seed=2)
                pf.run_raw(odom[:n_steps], obs[:n_steps])
                rd = pf.read()
                q = rd["particles"].astype(f32)
                # the handle's offset is back at R0: the public call at the handle's own offset ...
                at_entry = mcl_fused(m, q, angles, obs[n_steps - 1])
                m.set_noise(noise, seed=77, ray_offset=R0)
                assert same_bits(at_entry, mcl_fused(m, q, angles, obs[n_steps - 1]))
                # ... and L at the step's
                m.set_noise(noise, seed=77, ray_offset=R0 + (n_steps - 1) * P * A)
                L = mcl_fused(m, q, angles, obs[n_steps - 1])
                m.set_noise(noise, seed=77, ray_offset=R0)
                assert same_bits(rd["likelihood"], L), (kind, noise, n_steps)
                if n_steps == 1:
                    omega = np.full(P, 1.0 / P) * L
                    assert same_bits(rd["weights"], omega / np.float64(MS.bs(omega)))
                    if noise:
                        assert (at_entry == L).all()          # (step 0's offset is the entry offset)
                elif noise:
                    assert (at_entry != L).mean() > 0.5       # (step 2's is not)
                Ls.append(L)
            assert {k: m.get_info(k) for k in before} == before
            pf.close()
    finally:
        m.set_noise(0.0)


# ---------------------------------------------------------------- 3. degenerate, reset
def test_all_zero_table_is_degenerate(worlds):
    w = worlds(MAPS[0])
    P, A = 600, 7
    parts, angles, odom, obs, table = w.case(P, A)
    m = w.method("RMGPU-1")
    m.set_sensor_model(np.zeros_like(table))
    for ratio, flag in ((0.5, MS.DEGENERATE), (2.0, MS.DEGENERATE | MS.RESAMPLED)):
        pf = ParticleFilter(m, angles, P, motion_std=STD, resample_ratio=ratio)
        pf.reset(parts, seed=1)
        est, neff, flags = pf.run_raw(odom, obs)
        st = MS.Filter(lambda q, o, t: np.zeros(P), P, STD, ratio)
        st.reset(parts, seed=1)
        assert_equal_to_statement(pf, (est, neff, flags), st, st.run(odom, obs), ("zero table", ratio))
        assert (flags == flag).all()
        assert same_bits(pf.read()["weights"], np.full(P, 1.0 / P)) and not pf.read()["likelihood"].any()
        assert np.isfinite(est).all()


def test_reset_is_idempotent(worlds):
    w = worlds(MAPS[0])
    P, A = 256, 7
    parts, angles, odom, obs, table = w.case(P, A)
    m = w.method("GLT")
    m.set_sensor_model(table)
    pf = ParticleFilter(m, angles, P, motion_std=STD, resample_ratio=0.5)
    pf.reset(parts, seed=4)
    rd = pf.read()
    assert same_bits(rd["particles"], parts) and same_bits(rd["weights"], np.full(P, 1.0 / P))
    one = pf.run_raw(odom, obs), pf.read()
    pf.reset(parts, seed=4)
    pf.reset(parts, seed=4)
    two = pf.run_raw(odom, obs), pf.read()
    assert all(same_bits(x, y) for x, y in zip(one[0], two[0])) and all(same_bits(one[1][k], two[1][k]) for k in one[1])
    pf.reset(parts, seed=5)                                   # (another seed: other draws)
    assert not same_bits(pf.run_raw(odom, obs)[0], one[0][0])


# ---------------------------------------------------------------- 4. errors
def test_every_error_of_the_contract_and_a_correct_run_afterwards(worlds):
    w = worlds(MAPS[0])
    L = _lib.lib()
    P, A = 256, 7
    parts, angles, odom, obs, table = w.case(P, A)
    m = range_libc.PyRayMarchingGPU(w.omap, w.mrx)            # a fresh handle: no table set yet
    p_ang = angles.ctypes.data_as(_lib.f32p)

    def create(h=m._h, n=P, a=A, std=STD, ratio=0.5, ang=p_ang, par=True, out=True):
        f = C.c_void_p()
        p = _lib.PfParams(n, a, (C.c_double * 3)(*std), ratio)
        rc = L.rl_pf_create(h, C.byref(p) if par else None, ang, C.byref(f) if out else None)
        assert rc != 0 or f.value
        if f.value:
            L.rl_pf_destroy(f)
        return rc

    assert create() == RL_ERR_INVALID and b"sensor model" in L.rl_last_error()
    m.set_sensor_model(table)
    assert create() == 0
    assert create(h=None) == create(par=False) == create(ang=None) == create(out=False) == RL_ERR_INVALID
    assert create(n=0) == create(n=-1) == create(n=(1 << 20) + 1) == RL_ERR_INVALID
    assert create(a=0) == create(a=2049) == create(n=1 << 20, a=2048) == RL_ERR_INVALID
    for bad in (-0.1, float("nan")):
        assert create(std=(bad, 0.0, 0.0)) == create(std=(0.0, 0.0, bad)) == create(ratio=bad) == RL_ERR_INVALID
    bl = range_libc.PyBresenhamsLine(w.omap, w.mrx)
    bl.set_sensor_model(table)
    assert create(h=bl._h) == RL_ERR_UNSUPPORTED
    m.set_option("variant", 2)
    assert create() == RL_ERR_UNSUPPORTED
    m.set_option("variant", 1)
    momap = range_libc.PyOMap(w.g, device=[0, 0])
    mm = range_libc.PyRayMarchingGPU(momap, w.mrx)
    assert create(h=mm._h) == RL_ERR_INVALID and b"multi-device" in L.rl_last_error()

    pf = ParticleFilter(m, angles, P, motion_std=STD, resample_ratio=0.5)
    est, neff, flags = np.zeros((T, 4)), np.zeros(T), np.zeros(T, np.int32)
    p_od, p_ob = odom.ctypes.data_as(_lib.f64p), obs.ctypes.data_as(_lib.f32p)
    p_e, p_n, p_f = est.ctypes.data_as(_lib.f64p), neff.ctypes.data_as(_lib.f64p), flags.ctypes.data_as(_lib.i32p)

    def run(f=pf._h, n=T, od=p_od, ob=p_ob, e=p_e, ne=p_n, fl=p_f):
        return L.rl_pf_run(f, n, od, ob, e, ne, fl)

    assert run() == RL_ERR_INVALID and b"reset" in L.rl_last_error()          # before a reset
    assert L.rl_pf_read(pf._h, None, None, None, None, None) == RL_ERR_INVALID
    assert L.rl_pf_reset(None, parts.ctypes.data_as(_lib.f64p), None, 1) == RL_ERR_INVALID
    assert L.rl_pf_reset(pf._h, None, None, 1) == RL_ERR_INVALID
    pf.reset(parts, seed=3)
    assert run(f=None) == run(od=None) == run(ob=None) == run(e=None) == run(ne=None) == run(fl=None) == RL_ERR_INVALID
    assert run(n=-1) == RL_ERR_INVALID
    assert run(n=(1 << 26) + 1) == RL_ERR_INVALID
    assert L.rl_pf_read(None, None, None, None, None, None) == RL_ERR_INVALID
    assert run(n=0) == 0 and run(n=0, od=None, ob=None, e=None, ne=None, fl=None) == 0      # nothing to do
    assert L.rl_pf_read(pf._h, None, None, None, None, None) == 0                         # every output may be null
    with pytest.raises(_lib.ScanLibError) as e:
        ParticleFilter(m, angles, 0)
    assert e.value.code == RL_ERR_INVALID
    with pytest.raises(ValueError):
        pf.reset(parts[:5])
    # the filter and the method are usable afterwards, with the right answer (n_steps = 0 did not advance t)
    assert run() == 0
    st = MS.Filter(w.likelihood("RMGPU-1", angles, table), P, STD, 0.5)
    st.reset(parts, seed=3)
    assert_equal_to_statement(pf, (est, neff, flags), st, st.run(odom, obs), "after the errors")
