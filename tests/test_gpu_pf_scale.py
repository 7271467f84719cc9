"""The particle-filter kernels beyond one round of their grids (csrc/pf_kernels.h, csrc/mcl_kernels.h), bit for bit
against tests/pf_statement.py, the oracle and tests/mcl_statement.py: a second and a third tile per workgroup of the
weight kernels, the production tile sizes, the second round of the repeat-angle scan, the LDS cap of a tile, and
localisation at sizes with several workgroups, staging rounds and base tiles up to the contract's 2^20 particles; the
+inf and NaN forms of a degenerate total and dead particles.  The weight shapes are derived from the device's CU count
and every test first asserts the inequality that puts it on its path; tests/test_mcl_host.py
(test_gpu_scale_input_condition) holds the statement to what the localisation inputs are taken to do."""
import numpy as np
import pytest

import mcl_statement as MS
import pf_statement as PS
import pf_cases as PF
from support import same_bits
from pyracecarsimulator_amd import ParticleFilter, maps

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

f32 = np.float32
KINDS = sorted(PF.MCL_KINDS)                     # RM-3 literal, RMGPU-1 canonical, CDDT, GLT
MARCH = ("RM-3", "RMGPU-1")
MAPS = PF.MAPS
STD = PF.STD
WG, TILE_RAYS, CHUNK = 256, 2048, MS.CHUNK   # pf_kernels.h PF_WG, PF_TILE_RAYS; the contract's chunk
NOISE = dict(seed=77, ray_offset=123457)


class Weights(PF.WeightWorld):
    """The weight tests' world: as many free poses as a shape asks for, drawn once per P."""

    def poses_of(self, P):
        drawn = self.__dict__.setdefault("drawn", {})
        if P not in drawn:
            drawn[P] = np.ascontiguousarray(maps.sample_free_poses(self.g, P, 31, 2.0, self.om.dt), f32)
        return drawn[P]


@pytest.fixture(scope="module")
def pf_worlds(oracle_mod):
    cache = {}
    return lambda name: cache[name] if name in cache else cache.setdefault(name, Weights(oracle_mod, name))


@pytest.fixture(scope="module")
def mcl_worlds(oracle_mod):
    cache = {}
    return lambda name: cache[name] if name in cache else cache.setdefault(name, PF.MclWorld(oracle_mod, name))


def _lds_bytes(block, A):
    return block * (A | 1) * 8 + block * 16 + A * 12


def _tile_block(n_cu, P, A, forced=0):
    """make_pf's arithmetic: particles per tile of the weight kernels."""
    block = max(1, min(-(-TILE_RAYS // A), WG, P))
    spread = -(-P // (4 * n_cu))
    block = max(max(1, WG // A), min(block, spread))
    if forced > 0:
        block = forced
    block = max(1, min(block, WG, max(P, 1)))
    while block > 1 and _lds_bytes(block, A) > 65536:
        block -= 1
    return block


def _maps_of(kind):
    """The marching kinds are stated on the yawed map too; the oracle's table kinds for a yaw-0 origin."""
    return MAPS if kind in MARCH else MAPS[:1]


# ---------------------------------------------------------------- A1. a second and a third tile per workgroup
def _later_tile_shapes(n_cu):
    """(pf_block, A, P): every workgroup takes two tiles and 77 a third; some take two, the rest one, the last tile short."""
    return [(1, 7, 2 * 8 * n_cu + 77), (3, 7, 3 * 8 * n_cu + 100)]


def _assert_later_tiles(n_cu, block, P):
    tiles, grid = -(-P // block), 8 * n_cu
    assert tiles > grid, "no workgroup takes a second tile on this part: %d tiles, a grid of %d" % (tiles, grid)
    if block == 1:
        assert 2 * grid < tiles < 3 * grid              # every workgroup a second tile, some a third
    else:
        assert tiles < 2 * grid and P - (tiles - 1) * block == 1      # some a second; the last tile holds one particle
    return tiles


@pytest.mark.parametrize("kind", KINDS)
def test_later_tiles_of_the_fused_call(pf_worlds, kind):
    for name in _maps_of(kind):
        w = pf_worlds(name)
        m = w.method(kind)
        n_cu = m.get_info("n_cu")
        table = PS.witness_table(301, seed=5)
        m.set_sensor_model(table)
        try:
            for block, A, P in _later_tile_shapes(n_cu):
                _assert_later_tiles(n_cu, block, P)
                m.set_option("pf_block", block)
                assert m.get_info("pf_block") == block == _tile_block(n_cu, P, A, block)
                angles, obs, poses = PF.wild_angles(A, 300 + A), PF.obs_of(w, A, 3 * A), w.poses_of(P)
                fused = PF.fused(m, poses, angles, obs)
                want = PS.weights(table, obs, w.expect(kind, poses, angles, ("scale", A, P)), w.inv_res)
                bad = np.nonzero(fused != want)[0]
                assert same_bits(fused, want), (kind, name, block, P, bad.size, bad[:4], bad[:4] // block)
                assert np.unique(fused).size > P // 4
                # scan noise is keyed by the global ray id: (p0 + p) A + j of a later tile is the plain scan's p A + j
                m.set_noise(0.02, **NOISE)
                ranges, unfused = PF.unfused(m, poses, angles, obs)
                fused = PF.fused(m, poses, angles, obs)
                m.set_noise(0.0)
                bad = np.nonzero(fused != unfused)[0]
                assert same_bits(fused, unfused), (kind, name, block, P, "noise", bad.size, bad[:4], bad[:4] // block)
                assert same_bits(fused, PS.weights(table, obs, ranges, w.inv_res)), (kind, name, block, P, "noise")
                assert (ranges != w.expect(kind, poses, angles, ("scale", A, P))).mean() > 0.9
        finally:
            m.set_noise(0.0)
            m.set_option("pf_block", 0)


def test_later_tiles_of_eval_sensor_model(pf_worlds):
    w = pf_worlds(MAPS[0])
    m = w.method("RMGPU-1")
    n_cu = m.get_info("n_cu")
    table = PS.witness_table(301, seed=21)
    m.set_sensor_model(table)
    try:
        for block, A, P in _later_tile_shapes(n_cu):
            _assert_later_tiles(n_cu, block, P)
            m.set_option("pf_block", block)
            ranges = PF.planted_ranges(w, m, A, P, 7 * A + P, poses=w.poses_of(P))
            assert ranges.size == P * A
            obs = PF.obs_of(w, A, A)
            got = np.full(P, -1.0)
            m.eval_sensor_model(obs, ranges, got, A, P)
            want = PS.weights(table, obs, ranges, w.inv_res)
            bad = np.nonzero(got != want)[0]
            assert same_bits(got, want), (block, P, bad.size, bad[:4], bad[:4] // block)
            assert np.isfinite(got).all() and (got > 0).all()
    finally:
        m.set_option("pf_block", 0)


# ---------------------------------------------------------------- A2. the production tile sizes
@pytest.mark.parametrize("kind", MARCH)
def test_production_tile_sizes(pf_worlds, kind):
    """pf_block 0 and more than four particles per CU: make_pf sizes the tile from the spread (6 particles) and, with
    enough particles, at PF_TILE_RAYS rays (38 particles of 54 beams)."""
    w = pf_worlds(MAPS[0])
    m = w.method(kind)
    n_cu = m.get_info("n_cu")
    table = PS.witness_table(301, seed=5)
    m.set_sensor_model(table)
    assert m.get_info("pf_block") == 0
    A = 54
    for P, block in ((4 * n_cu * 5 + 3, 6), (4 * n_cu * 40 + 5, 38)):
        assert P > 4 * n_cu and -(-P // (4 * n_cu)) > WG // A            # the spread, not the floor, sizes the tile
        assert _tile_block(n_cu, P, A) == block
        assert P % block != 0                                            # (a short last tile)
        angles, obs, poses = PF.wild_angles(A, 300 + A), PF.obs_of(w, A, 3 * A), w.poses_of(P)
        fused = PF.fused(m, poses, angles, obs)
        want = PS.weights(table, obs, w.expect(kind, poses, angles, ("scale", A, P)), w.inv_res)
        bad = np.nonzero(fused != want)[0]
        assert same_bits(fused, want), (kind, P, block, bad.size, bad[:4], bad[:4] // block)


# ---------------------------------------------------------------- A3. the scan's second grid-stride round
@pytest.mark.parametrize("kind", KINDS)
def test_second_round_of_the_repeat_angle_scan(pf_worlds, kind):
    w = pf_worlds(MAPS[0])
    m = w.method(kind)
    n_cu = m.get_info("n_cu")
    A, P = 2048, 2 * n_cu + 9
    assert P * A > 16 * n_cu * WG, "the scan's grid covers every ray in one round on this part"
    angles, poses = PF.wild_angles(A, 100 + A), w.poses_of(P)
    if kind == "RMGPU-1":                                   # the AUX instantiation: hit cells and step counts too
        want, want_h, want_s = PS.repeat_angles(w.g.occ, w.g.resolution, w.g.origin, w.mrx, poses, angles,
                                                step_coeff=1.0, dt=w.om.dt)
        got, got_h, got_s = PF.scan(m, poses, angles, aux=True)
        assert np.array_equal(got_h, want_h), int((got_h != want_h).any(1).sum())
        assert np.array_equal(got_s, want_s), int((got_s != want_s).sum())
        assert (got_h[16 * n_cu * WG:, 0] >= 0).any()
        assert same_bits(got, want)
    else:
        want = w.expect(kind, poses, angles, ("scale", A, P))
    got = PF.scan(m, poses, angles)
    bad = np.nonzero(got != want)[0]
    assert same_bits(got, want), (kind, bad.size, bad[:4])
    assert np.unique(got[16 * n_cu * WG:]).size > 100


# ---------------------------------------------------------------- A4. the LDS cap of a tile
def test_tile_shrinks_to_the_lds_cap(pf_worlds):
    """2048 beams: three particles' factor rows pass 64 KiB, so a forced pf_block of 4 or 256 is cut to 2 and five
    particles make tiles of 2, 2 and 1."""
    w = pf_worlds(MAPS[0])
    A, P = 2048, 5
    table = PS.witness_table(301, seed=5)
    angles, obs, poses = PF.wild_angles(A, 300 + A), PF.obs_of(w, A, 3 * A), w.poses_of(P)
    for kind in MARCH:
        m = w.method(kind)
        n_cu = m.get_info("n_cu")
        m.set_sensor_model(table)
        try:
            for forced in (4, 256):
                assert _lds_bytes(3, A) > 65536 >= _lds_bytes(2, A) and _tile_block(n_cu, P, A, forced) == 2
                m.set_option("pf_block", forced)
                fused = PF.fused(m, poses, angles, obs)
                want = PS.weights(table, obs, w.expect(kind, poses, angles, ("scale", A, P)), w.inv_res)
                assert same_bits(fused, want), (kind, forced, np.nonzero(fused != want)[0])
                ranges = PF.planted_ranges(w, m, A, P, 7 * A + P, poses=poses)
                got = np.full(P, -1.0)
                m.eval_sensor_model(obs, ranges, got, A, P)
                want = PS.weights(table, obs, ranges, w.inv_res)
                assert same_bits(got, want), (kind, forced, "eval", np.nonzero(got != want)[0])
        finally:
            m.set_option("pf_block", 0)


# ---------------------------------------------------------------- B. localisation beyond one workgroup and one tile
def _assert_path(P, T):
    """What a row reaches in mcl_kernels.h, from its number of chunks."""
    NB = -(-P // CHUNK)
    assert NB > 8 and NB > 4                                # mcl_weight_kernel and mcl_norm_kernel: several workgroups
    assert P.bit_length() > 11                              # the bisection probes more than ten times
    if P == 2500:
        assert P % CHUNK not in (0, 1)                      # a short last chunk
    if P == 65793:
        assert NB > 256 and P % CHUNK == 1                  # a second staging round; the last chunk holds one particle
    if P == 131072:
        assert NB == 512 and P % CHUNK == 0                 # exactly one full base tile
    if P in (131073, 140001):
        assert NB > 512                                     # a second base tile (of one total at 131 073)
    if P == 131073:
        assert NB == 513
    if P == 1 << 20:
        assert NB == 4096 and T == 1                        # the contract's maximum: every staging array full
    return NB


def _first_difference(pf, st):
    """Where the device leaves the statement: the first differing index of each read-back array, its chunk, its base tile."""
    rd, out = pf.read(), {}
    for key, want in (("likelihood", st.L), ("cum", st.cum), ("ancestors", st.anc), ("weights", st.w)):
        bad = np.nonzero(rd[key] != want)[0]
        if bad.size:
            out[key] = dict(n=int(bad.size), first=int(bad[0]), chunk=int(bad[0]) // CHUNK, tile=int(bad[0]) // CHUNK // 512)
    return out


ROW_CASES = [(P, A, T, kind, ratios, dead, most) for P, A, T, kinds, ratios, dead, most in MS.SCALE_ROWS for kind in kinds]


@pytest.mark.parametrize("P,A,T,kind,ratios,dead,most", ROW_CASES, ids=["%d-%s" % (c[0], c[3]) for c in ROW_CASES])
def test_localisation_rows_equal_the_statement(mcl_worlds, P, A, T, kind, ratios, dead, most):
    _assert_path(P, T)
    for name in (_maps_of(kind) if P == 2500 else MAPS[:1]):
        w = mcl_worlds(name)
        for ratio in ratios:
            pf, out, st, want = PF.both(w, kind, P, A, ratio, n_steps=T)
            what = (kind, name, P, A, ratio)
            if not same_bits(pf.read()["cum"], st.cum) or not same_bits(out[1], want[1]):
                print(what, _first_difference(pf, st))
            PF.assert_equal_to_statement(pf, out, st, want, what)
            if name == MAPS[0]:
                assert out[2].tolist() == MS.scale_flags(A, T, ratio), (what, out[1])
            if ratio == 2.0:
                assert (out[2] & MS.RESAMPLED).all()
                n = np.bincount(pf.read()["ancestors"], minlength=P)
                assert (n == 0).mean() >= dead and n.max() >= most, (what, (n == 0).mean(), n.max())
            if ratio == 0.0:
                assert not out[2].any() and same_bits(pf.read()["ancestors"], np.arange(P, dtype=np.int32))
            pf.close()


def test_run_two_equals_run_one_twice_at_scale(mcl_worlds):
    """140 001 particles, ratio 0.5: step 0 resamples, step 1 keeps."""
    w = mcl_worlds(MAPS[0])
    P, A = 140001, 1
    assert _assert_path(P, 2) > 512
    parts, angles, odom, obs, table = w.case(P, A, 2)
    m = w.method("RMGPU-1")
    m.set_sensor_model(table)
    a = ParticleFilter(m, angles, P, motion_std=STD, resample_ratio=0.5)
    b = ParticleFilter(m, angles, P, motion_std=STD, resample_ratio=0.5)
    a.reset(parts, seed=5)
    b.reset(parts, seed=5)
    whole = a.run_raw(odom, obs)
    first = b.run_raw(odom[:1], obs[:1])
    n = np.bincount(b.read()["ancestors"], minlength=P)
    assert (n == 0).mean() >= 0.25 and n.max() >= 3
    rest = b.run_raw(odom[1:], obs[1:])
    for x, y, z in zip(whole, first, rest):
        assert same_bits(x, np.concatenate([y, z]))
    assert whole[2].tolist() == MS.scale_flags(A, 2, 0.5)
    ra, rb = a.read(), b.read()
    assert all(same_bits(ra[k], rb[k]) for k in ra)
    a.close()
    b.close()


# ---------------------------------------------------------------- C. the other degenerate totals, dead particles
def _small(w, ratio, table, weights=None):
    """600 x 7 on RMGPU-1 with the case's table rewritten by ``table``."""
    P, A = 600, 7
    tb = table(w.case(P, A)[4])
    with np.errstate(over="ignore", invalid="ignore"):
        return PF.both(w, "RMGPU-1", P, A, ratio, weights=weights, table=tb)


def test_infinite_total_is_degenerate(mcl_worlds):
    w = mcl_worlds(MAPS[0])
    P = 600
    pf, out, st, want = _small(w, 0.0, MS.overflow_table, weights=np.full(P, 1e308))
    PF.assert_equal_to_statement(pf, out, st, want, "W = +inf")
    assert out[2].tolist() == [MS.DEGENERATE, 0, 0]
    # step 0 alone: omega overflows, the weights are reset to 1 / P
    pf.reset(w.case(P, 7)[0], weights=np.full(P, 1e308), seed=3)
    _, neff, flags = pf.run_raw(w.case(P, 7)[2][:1], w.case(P, 7)[3][:1])
    rd = pf.read()
    assert flags[0] == MS.DEGENERATE and same_bits(rd["weights"], np.full(P, 1.0 / P))
    with np.errstate(over="ignore"):
        assert np.isinf(1e308 * rd["likelihood"]).any() and abs(neff[0] - P) < 1e-6
    pf.close()


def test_nan_total_is_degenerate(mcl_worlds):
    w = mcl_worlds(MAPS[0])
    P = 600
    for ratio, flag in ((0.0, MS.DEGENERATE), (2.0, MS.DEGENERATE | MS.RESAMPLED)):
        pf, out, st, want = _small(w, ratio, MS.nan_table)
        PF.assert_equal_to_statement(pf, out, st, want, ("W = NaN", ratio))
        assert (out[2] == flag).all()
        assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all()
        rd = pf.read()
        assert 0.05 < np.isnan(rd["likelihood"]).mean() < 0.5 and same_bits(rd["weights"], np.full(P, 1.0 / P))
        pf.close()


def test_zero_weight_plateaus(mcl_worlds):
    w = mcl_worlds(MAPS[0])
    pf, out, st, want = _small(w, 2.0, MS.plateau_table)
    PF.assert_equal_to_statement(pf, out, st, want, "plateaus")
    rd = pf.read()
    assert (rd["likelihood"] == 0).mean() >= 0.5 and (np.diff(rd["cum"]) == 0).mean() >= 0.5
    assert (out[2] == MS.RESAMPLED).all()
    assert (st.omega[rd["ancestors"]] > 0).all()             # no ancestor had a zero weight before the resampling
    pf.close()
