"""Particle-filter localisation on the device (rl_pf_*, include/scanlib.h "particle-filter localisation").

``ParticleFilter`` keeps P particles on the GPU of a range method and runs whole Monte-Carlo-localisation updates there:
odometry motion with noise, the fused repeat-angle scan + sensor model, weight normalisation, the pose estimate and
systematic resampling.  ``run`` takes the odometry and the observed scans of T steps at once; nothing crosses to the
host between the steps.  tests/mcl_statement.py is the same update in NumPy, bit for bit.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

RESAMPLED, DEGENERATE = 1, 2        # bits of a step's flags


class ParticleFilter(_lib.Handle):
    """A filter of ``n_particles`` particles casting the beams ``angles`` (radians, float32, relative to the heading) on
    ``method`` (a ``range_libc`` RayMarching, RayMarchingGPU, CDDTCast or GiantLUTCast object on one device whose sensor
    model has been set with ``set_sensor_model``; it must outlive the filter).

    ``motion_std``: the standard deviations of the noise added to (x, y, theta) after the odometry step; 0 switches an
    axis' draws off.  ``resample_ratio``: resample when the effective sample size falls below ``ratio * n_particles``
    (0: never, >= 2: always).

    The sensor-model table is used as it is set: a squash exponent (particle_filter.py's ``squash_factor``) is applied by
    the caller to the table, ``table ** (1 / squash)``, before ``set_sensor_model`` — no ``pow`` runs on the device.
    """

    _destroy = "rl_pf_destroy"

    def __init__(self, method, angles, n_particles, motion_std=(0.0, 0.0, 0.0), resample_ratio=0.5):
        self._h = C.c_void_p()
        self.method = method
        self.angles = np.ascontiguousarray(angles, dtype=np.float32).ravel()
        self.n_particles = int(n_particles)
        std = np.asarray(motion_std, dtype=np.float64).ravel()
        if std.size != 3:
            raise ValueError("motion_std needs three values (x, y, theta)")
        par = _lib.PfParams(self.n_particles, int(self.angles.size), (C.c_double * 3)(*std), float(resample_ratio))
        _lib.call("rl_pf_create", method, par, self.angles, self._h)

    def reset(self, particles, weights=None, seed=0):
        """Start from ``particles`` (P, 3) float64 (x, y, theta) with uniform weights, or ``weights`` taken as given;
        the step counter returns to 0 and every draw is keyed by ``seed``."""
        particles = np.ascontiguousarray(particles, dtype=np.float64)
        if particles.shape != (self.n_particles, 3):
            raise ValueError("particles must be (%d, 3)" % self.n_particles)
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.float64).ravel()
            if weights.size != self.n_particles:
                raise ValueError("weights must have %d values" % self.n_particles)
        _lib.call("rl_pf_reset", self, particles, weights, seed)

    def run_raw(self, odom, obs):
        """T updates: ``odom`` (T, 3) float64 (dx, dy, dtheta) in the car frame, ``obs`` (T, A) float32 observed ranges
        in metres.  Returns (est (T, 4) = weighted sums of x, y, cos, sin; neff (T,); flags (T,) int32)."""
        odom = np.ascontiguousarray(odom, dtype=np.float64).reshape(-1, 3)
        obs = np.ascontiguousarray(obs, dtype=np.float32).reshape(-1, self.angles.size)
        T = odom.shape[0]
        if obs.shape[0] != T:
            raise ValueError("odom has %d rows, obs %d" % (T, obs.shape[0]))
        est, neff, flags = np.zeros((T, 4)), np.zeros(T), np.zeros(T, np.int32)
        _lib.call("rl_pf_run", self, T, odom, obs, est, neff, flags)
        return est, neff, flags

    def run(self, odom, obs):
        """T updates (see ``run_raw``).  Returns (poses (T, 3) = the weighted mean x, y and the heading
        ``atan2`` of the weighted sin and cos sums, taken before resampling; neff (T,); flags (T,): bit 0 resampled,
        bit 1 degenerate — the weights summed to nothing usable and were reset to uniform)."""
        est, neff, flags = self.run_raw(odom, obs)
        poses = np.stack([est[:, 0], est[:, 1], np.arctan2(est[:, 3], est[:, 2])], axis=1)
        return poses, neff, flags

    def step(self, odom, obs):
        """One update: (pose (3,), neff, flags)."""
        poses, neff, flags = self.run(np.asarray(odom, np.float64).reshape(1, 3), np.asarray(obs, np.float32).reshape(1, -1))
        return poses[0], float(neff[0]), int(flags[0])

    def read(self):
        """The state after the last step as a dict: particles (P, 3), weights (P,), and the last step's ancestors
        (P,) int32, cum (P,) — the cumulative weights the ancestors were searched in — and likelihood (P,)."""
        P = self.n_particles
        out = dict(particles=np.zeros((P, 3)), weights=np.zeros(P), ancestors=np.zeros(P, np.int32), cum=np.zeros(P),
                   likelihood=np.zeros(P))
        _lib.call("rl_pf_read", self, *out.values())
        return out
