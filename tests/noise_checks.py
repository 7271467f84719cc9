"""check_noise: a handle's Gaussian range noise on one launch shape against the independent statement of the generator
(oracle/np_statement.py gauss_noise_ref), as tests/test_gpu_noise.py describes it."""
import numpy as np

from oracle import np_statement as N

#: bound on |g_device - g_ref| (the hardware log2 / cos estimates in Box-Muller): the MI355X was observed at
#: 2.0e-6 over this module, the schedules and the fuzz (``max_dg``); a ray keyed by a wrong id is off by ~1
EPS_G = 2e-5


SEED_HI = 0x9E3779B97F4A7C15           # a seed whose high word matters (the fold)
_MAX_DG = [0.0]


def max_dg():
    """The largest |g_device - g_ref| seen so far (beyond the rounding of range + std g), over every check_noise."""
    return _MAX_DG[0]


def noise_mismatch(noisy, clean, std, g_ref, eps_g=EPS_G):
    """Indices of rays whose noise is not std * g_ref (NaN positions must match, finite ones agree to
    ulp(noisy) + std * eps_g); records the observed excess in units of g."""
    noisy = np.asarray(noisy, np.float32)
    clean = np.asarray(clean, np.float32)
    nan = np.isnan(noisy)
    bad = np.flatnonzero(nan != np.isnan(clean))
    if bad.size:
        return bad
    ok = ~nan
    d = np.abs(noisy[ok].astype(np.float64) - clean[ok].astype(np.float64) - std * g_ref[ok])
    ulp = np.spacing(np.abs(noisy[ok])).astype(np.float64)
    if d.size:
        _MAX_DG[0] = max(_MAX_DG[0], float(np.max(np.maximum(d - ulp, 0.0)) / std))
    return np.flatnonzero(ok)[d > ulp + std * eps_g]


def check_noise(m, poses, fov, num_rays, want, seed, offset, stds=(1.0, 0.01), scan=None, ids=None,
                kernel=None, name=None, what=""):
    """Noise of handle ``m`` on one launch shape against the reference.

    ``scan()`` launches with the handle's current noise and returns the float32 ranges (default: calc_range_fan of
    ``poses``); ``want`` the oracle's clean ranges (None: only for the approximate occ_lds kernel); ``ids`` the global
    ray id of every output (default ``offset + arange``); ``kernel`` / ``name`` what last_plan() must report after
    each launch.  Returns the clean ranges."""
    if scan is None:
        P = len(poses)

        def scan():
            out = np.full(P * num_rays, -7.0, np.float32)
            m.calc_range_fan(poses, out, fov, num_rays)
            return out

    def ran(tag):
        if kernel is None and name is None:
            return
        pl = m.last_plan()
        assert kernel is None or pl["kernel"] == kernel, (what, tag, pl["kernel"], pl["name"])
        assert name is None or name in pl["name"], (what, tag, pl["name"])

    m.set_noise(0.0, seed, offset)
    clean = scan()
    ran("clean")
    if want is not None:
        assert np.array_equal(clean.view(np.uint32), np.asarray(want, np.float32).view(np.uint32)), \
            (what, "clean ranges differ from the oracle", int((clean != want).sum()))
    if ids is None:
        ids = N.fan_ray_ids(offset, clean.size, 1)
    g = N.gauss_noise_ref(seed, ids)
    try:
        for std in stds:
            m.set_noise(std, seed, offset)
            noisy = scan()
            ran("std %g" % std)
            bad = noise_mismatch(noisy, clean, std, g)
            assert bad.size == 0, (what, "std %g seed %#x offset %#x: %d rays off, first %s: got %r clean %r ref %r"
                                   % (std, seed, offset, bad.size, bad[:4].tolist(), noisy[bad[:4]].tolist(),
                                      clean[bad[:4]].tolist(), (std * g[bad[:4]]).tolist()))
    finally:
        m.set_noise(0.0, 0, 0)
    return clean
