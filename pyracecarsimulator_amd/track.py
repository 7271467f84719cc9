"""``Track`` — a closed or open polyline of waypoints on the device (``rl_track_*``, include/scanlib.h "track
progress"): the global path of the reference's driver (``paths/wp-u.csv``).  Attached to a ``DriveEnv`` or ``RaceEnv``
(``track=``) it gives every env, at every reset and step and without leaving the GPU, its arc length, lateral offset and
heading error on the track, the progress of the step, its laps, a lookahead waypoint in the car's frame and, in a race,
its position (``env.track_state()``), and optionally the progress as the reward."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

MAX_POINTS = 65536

#: the columns of ``track_state()['rows']``
ROW_NAMES = ("delta", "s", "lateral", "heading_err", "gx", "gy", "progress", "race_dist")


def track_args(xy, closed=True):
    """``Track``'s arguments checked and laid out for ``rl_track_create`` (no library call): float64 (W, 2)."""
    p = np.asarray(xy, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError("xy must be (W, 2)")
    W = p.shape[0]
    if W < (3 if closed else 2):
        raise ValueError("a closed track needs at least 3 points, an open one 2")
    if W > MAX_POINTS:
        raise ValueError("a track holds at most %d points" % MAX_POINTS)
    if not np.isfinite(p).all():
        raise ValueError("xy must be finite")
    nxt = np.roll(p, -1, 0) if closed else p[1:]
    d = nxt - (p if closed else p[:-1])
    q = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    if (q == 0).any() or not np.isfinite(q).all():
        raise ValueError("segment %d has no length (or overflows)" % int(np.nonzero((q == 0) | ~np.isfinite(q))[0][0]))
    return np.ascontiguousarray(p)


def track_env_args(track_window=0, lookahead=1.5, goal_span=0, progress_reward=False):
    """The track keywords of ``DriveEnv`` / ``RaceEnv`` checked and laid out as ``rl_track_params`` (no library call)."""
    for name, v in (("track_window", track_window), ("goal_span", goal_span)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("%s must be an integer" % name)
        if not 0 <= int(v) <= MAX_POINTS:
            raise ValueError("%s must lie in [0, %d]" % (name, MAX_POINTS))
    la = float(lookahead)
    if not np.isfinite(la) or la <= 0:
        raise ValueError("lookahead must be finite and > 0")
    if progress_reward not in (False, True, 0, 1):
        raise ValueError("progress_reward must be a bool")
    p = _lib.TrackParams()
    p.window, p.goal_span, p.reward_mode, p.lookahead = int(track_window), int(goal_span), int(bool(progress_reward)), la
    return p


class Track(_lib.Handle):
    """``xy`` (W, 2) waypoints in map metres; ``closed``: the last point joins the first."""
    _destroy = "rl_track_destroy"

    def __init__(self, xy, closed=True, device=0):
        p = track_args(xy, closed)
        self.xy, self.closed, self.device = p, bool(closed), int(device)
        self.n_points = p.shape[0]
        self.n_segments = self.n_points if self.closed else self.n_points - 1
        self._h = C.c_void_p()
        _lib.call("rl_track_create", self.device, p, self.n_points, self.closed, self._h)

    @staticmethod
    def read_csv(path):
        """The reference's waypoint file: comma-separated numbers per line, the first two columns x and y."""
        rows = []
        with open(path) as f:
            for line in f:
                cols = line.split(",")
                if len(cols) >= 2 and line.strip():
                    rows.append((float(cols[0]), float(cols[1])))
        return np.array(rows, dtype=np.float64).reshape(-1, 2)

    @classmethod
    def from_csv(cls, path, closed=True, device=0):
        return cls(cls.read_csv(path), closed, device)

    @property
    def cum(self):
        """Arc length at every point, float64 (S + 1,): cum[0] = 0, cum[S] = length."""
        out = np.empty(self.n_segments + 1)
        _lib.call("rl_track_read", self, out, None)
        return out

    @property
    def length(self):
        L = C.c_double()
        _lib.call("rl_track_read", self, None, L)
        return L.value
