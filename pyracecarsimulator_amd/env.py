"""``DriveEnv`` — a batched, device-resident driving environment (``rl_env_*``, include/scanlib.h).

The closed loops of ``racecar.CarBatch`` (``drive_followgap``, ``drive_policy``, ``drive_mcts``) have their steering
source compiled in.  ``DriveEnv`` is the same loop opened at that point: every ``step`` takes one (speed, steer) pair
per env from the caller — a PyTorch policy being trained, another planner, a heuristic — and, for ``n_envs`` cars at
once on the GPU, steps the cars, scans them, tests them for a crash, computes a reward and writes the observation.
Episode ends, truncation after ``max_ticks`` steps and re-spawning from a pool of start states happen on the device.

Two forms, picked by what ``step`` is given:

* a NumPy ``(n_envs, 2)`` float32 array takes the host form: synchronous, returns NumPy arrays;
* a torch tensor on the env's device takes the device form: the launches are enqueued on
  ``torch.cuda.current_stream()`` and nothing waits for the GPU.  It returns torch tensors that the env allocated
  once: THE NEXT CALL OVERWRITES THEM (clone what must be kept).

The interface follows the usual vectorised-environment shape (``reset`` -> obs, ``step`` -> obs, reward, done) but
depends on no environment toolkit.  ``done`` codes: 0 running, 1 crashed, 2 truncated, 3 invalid (non-finite) action.
The reward of a step is the distance travelled (float32), ``crash_reward`` for a step that crashes or an invalid
action, 0 for an env that was re-spawned by this call or that stands frozen.

``RaceEnv`` is the same environment with a race of P cars as the episode (``rl_env_create_race``): the cars of a race
see each other in every scan, a finished car stays in the map as a wreck, and the race spawns and re-spawns as a whole
once fewer than ``min_running`` of its cars run or ``max_ticks`` is reached.

Both take a ``track`` (``track.Track``): every reset and step then also places each car on the track, on the device,
and ``track_state()`` reads the result; ``progress_reward=True`` pays the progress along the track instead of the
distance travelled.

``RaceEnv`` also takes ``seats``: a driver per seat of the race (``seats.py``, include/scanlib_seats.h).  A car in a seat
with a ``PyFollowGap`` or a ``Policy`` is steered on the device by that driver's answer to its own full scan of the call
before, at ``seat_speed``; only the seats left None read the caller's actions.

``RaceEnv`` takes ``league`` instead: a ``PolicyPopulation`` and one entry per car (``league.py``,
include/scanlib_league_env.h), so that every race has its own line-up of members, FollowGap and caller's cars.
``set_entries`` hands over new line-ups at any time (a race adopts them when it spawns), and ``league_results`` reads
the running tally of who beat whom.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .track import Track, track_env_args


def env_args(n_envs, num_rays, starts, edge, substeps=1, obs_window=None, obs_clip=0, obs_scale=0, max_ticks=0,
             steer_clip=0, crash_reward=0, dt=0.01):
    """``DriveEnv``'s arguments checked and laid out for ``rl_env_create`` (no library call): returns (starts float64
    (M, 11), edge float64 (num_rays,), (obs_start, obs_count, obs_stride)).  ``obs_window`` None: every beam."""
    N, B = int(n_envs), int(num_rays)
    if (N, B) != (n_envs, num_rays) or int(substeps) != substeps or int(max_ticks) != max_ticks:
        raise ValueError("n_envs, num_rays, substeps and max_ticks must be integers")
    if N < 1:
        raise ValueError("n_envs must be >= 1")
    if not 1 <= int(substeps) <= 512:
        raise ValueError("substeps must lie in [1, 512]")
    if not 10 <= B <= 1280:
        raise ValueError("num_rays must lie in [10, 1280]")
    if N * B >= 1 << 31:
        raise ValueError("n_envs * num_rays must stay below 2^31")
    if int(max_ticks) < 0:
        raise ValueError("max_ticks must be >= 0")
    st = np.asarray(starts)
    if st.dtype != np.float64 or st.ndim != 2 or st.shape[1] != 11 or st.shape[0] < 1:
        raise ValueError("starts must be float64 (M, 11) with M >= 1")
    if not np.isfinite(st).all():
        raise ValueError("starts must be finite")
    ed = np.asarray(edge)
    if ed.dtype != np.float64 or ed.shape != (B,):
        raise ValueError("edge must be float64 (num_rays,)")
    win = (0, B, 1) if obs_window is None else tuple(obs_window)
    if len(win) != 3 or any(int(v) != v for v in win):
        raise ValueError("obs_window must be None or three integers (start, count, stride)")
    start, count, stride = (int(v) for v in win)
    if count < 1 or stride < 1 or start < 0 or start + (count - 1) * stride >= B:
        raise ValueError("obs_window (start, count, stride) must lie in [0, num_rays) with count and stride >= 1")
    for name, v in (("steer_clip", steer_clip), ("obs_clip", obs_clip), ("obs_scale", obs_scale)):
        if not float(v) >= 0:
            raise ValueError("%s must be >= 0" % name)
    if float(crash_reward) != float(crash_reward):
        raise ValueError("crash_reward must not be NaN")
    if not np.isfinite(float(dt)):
        raise ValueError("dt must be finite")
    return np.ascontiguousarray(st), np.ascontiguousarray(ed), (start, count, stride)


def race_env_args(n_races, num_rays, starts, edge, min_running=1, **kw):
    """``RaceEnv``'s arguments checked and laid out for ``rl_env_create_race`` (no library call): returns (starts
    float64 (M, P, 11), edge, the observation window, P).  ``kw``: what ``env_args`` takes after ``edge``."""
    R = int(n_races)
    if R != n_races or int(min_running) != min_running:
        raise ValueError("n_races and min_running must be integers")
    if R < 1:
        raise ValueError("n_races must be >= 1")
    st = np.asarray(starts)
    if st.dtype != np.float64 or st.ndim != 3 or st.shape[2] != 11 or st.shape[0] < 1:
        raise ValueError("starts must be float64 (M, P, 11) with M >= 1")
    P = st.shape[1]
    if not 1 <= P <= 8:
        raise ValueError("a race holds 1 to 8 cars (starts is (M, P, 11))")
    if not 1 <= int(min_running) <= P:
        raise ValueError("min_running must lie in [1, P]")
    flat, ed, win = env_args(R * P, num_rays, st.reshape(-1, 11), edge, **kw)
    return flat.reshape(-1, P, 11), ed, win, P


class DriveEnv(_lib.Handle):
    """``n_envs`` cars on one device, driven by the caller's actions.  ``method`` scans (any kind, with its options and
    noise), ``starts`` float64 (M, 11) is the pool of start states (getState layout), ``edge`` the car-outline table
    (``racecar.edge_distances``).  ``obs_window`` (start, count, stride) picks the beams of the observation (None:
    all); ``obs_scale`` > 0 gives them in the policy network's input form, (r <= obs_clip) ? r / obs_scale : 1.
    ``car``: a ``CarBatch`` on the method's device (None: one with the default parameters).  The handles are
    borrowed: the env keeps them alive.

    ``track``: a ``Track`` on the method's device (None: no track work at all).  ``track_window`` > 0 searches the
    nearest segment only within that many segments of the last one (0: all, every step), ``lookahead`` (m) and
    ``goal_span`` pick the goal waypoint (0: among all waypoints, the reference's rule; > 0: among that many forward of
    the car), ``progress_reward`` pays the step's progress along the track where the env pays the distance travelled."""
    _destroy = "rl_env_destroy"

    def __init__(self, method, starts, n_envs, num_rays, fov, edge, crash_thresh, *, substeps=1, obs_window=None,
                 obs_clip=0, obs_scale=0, max_ticks=0, auto_reset=True, steer_clip=0, crash_reward=0, car=None,
                 dt=0.01, scan_dist_to_base=0.275, track=None, track_window=0, lookahead=1.5, goal_span=0,
                 progress_reward=False):
        st, ed, win = env_args(n_envs, num_rays, starts, edge, substeps, obs_window, obs_clip, obs_scale, max_ticks,
                               steer_clip, crash_reward, dt)
        tp = track_env_args(track_window, lookahead, goal_span, progress_reward)
        if track is not None and not isinstance(track, Track):
            raise ValueError("track must be a Track (or None)")
        if car is None:
            from .racecar import CarBatch
            car = CarBatch(device=self._method_device(method))
        p = _lib.EnvParams()
        p.n_envs, p.substeps, p.num_rays = int(n_envs), int(substeps), int(num_rays)
        p.obs_start, p.obs_count, p.obs_stride = win
        p.obs_clip, p.obs_scale = float(obs_clip), float(obs_scale)
        p.max_ticks, p.auto_reset = int(max_ticks), int(bool(auto_reset))
        p.dt, p.scan_dist_to_base, p.crash_thresh = float(dt), float(scan_dist_to_base), float(crash_thresh)
        p.steer_clip, p.crash_reward, p.fov = float(steer_clip), float(crash_reward), float(fov)
        self.params = p
        self.n_starts = st.shape[0]
        self._keep = (car, method)
        self._n, self._count = int(n_envs), win[1]
        self._n_idx = self._n         # start indices a reset takes
        self._torch = None            # the device form's tensors, made at its first call
        self._h = C.c_void_p()
        self._create(car, method, p, ed, st)
        self.device = self._method_device(method)
        self.track = None
        if track is not None:
            self.attach_track(track, tp)

    def _create(self, car, method, p, ed, st):
        _lib.call("rl_env_create", car, method, p, ed, st, st.shape[0], self._h)

    @staticmethod
    def _method_device(method):
        omap = getattr(method, "omap", None)
        dev = getattr(omap, "device", 0)
        return dev if isinstance(dev, int) else 0

    @property
    def n_envs(self):
        return self._n

    @property
    def obs_shape(self):
        return (self._n, self._count)

    # -- track progress -----------------------------------------------------------------
    def attach_track(self, track, params=None, **kw):
        """Attach ``track`` (None: detach) with ``params`` (``track_env_args``'s result) or its keywords.  The env needs
        a ``reset`` afterwards."""
        tp = params if params is not None else track_env_args(**kw)
        _lib.call("rl_env_attach_track", self, track, tp)
        self.track = track            # (borrowed by the library: kept alive here)
        self._track_torch = None

    def track_state(self, on_device=False):
        """Where every env is on its track after the last reset or step: a dict of ``rows`` (n_envs, 8) float32 =
        (delta, s, lateral, heading_err, gx, gy, progress, race_dist) and ``segment``, ``goal``, ``laps``, ``rank`` int32
        (n_envs,).  NumPy by default (waits for the device); ``on_device=True``: the env's own torch tensors, filled on
        the current stream and overwritten by the next call."""
        if on_device:
            import torch
            if getattr(self, "_track_torch", None) is None:
                dev = torch.device("cuda", self.device)
                self._track_torch = (torch.empty((self._n, 8), dtype=torch.float32, device=dev),
                                     torch.empty((self._n, 4), dtype=torch.int32, device=dev))
            rows, ints = self._track_torch
            _lib.call("rl_env_read_track_device", self, rows.data_ptr(), ints.data_ptr(), self._stream())
        else:
            rows, ints = np.empty((self._n, 8), np.float32), np.empty((self._n, 4), np.int32)
            _lib.call("rl_env_read_track", self, rows, ints)
        return self._track_dict(rows, ints)

    @staticmethod
    def _track_dict(rows, ints):
        return dict(rows=rows, segment=ints[:, 0], goal=ints[:, 1], laps=ints[:, 2], rank=ints[:, 3])

    # -- the device form's buffers ----------------------------------------------------
    def _tensors(self):
        if self._torch is None:
            import torch
            dev = torch.device("cuda", self.device)
            self._torch = dict(obs=torch.empty(self.obs_shape, dtype=torch.float32, device=dev),
                               reward=torch.zeros(self._n, dtype=torch.float32, device=dev),
                               done=torch.zeros(self._n, dtype=torch.int32, device=dev),
                               aux=torch.empty((self._n, 4), dtype=torch.float32, device=dev))
        return self._torch

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def _is_tensor(self, x):
        return x is not None and not isinstance(x, np.ndarray) and type(x).__module__.split(".")[0] == "torch"

    def _check_tensor(self, x, shape, dtype_name, what):
        import torch
        if (not x.is_cuda or x.device.index != self.device or x.dtype != getattr(torch, dtype_name)
                or tuple(x.shape) != shape or not x.is_contiguous()):
            raise ValueError("%s must be a contiguous %s tensor of shape %s on cuda:%d" % (what, dtype_name, shape,
                                                                                           self.device))

    # -- calls ------------------------------------------------------------------------
    def reset(self, seed=0, start_index=None, *, aux=False, on_device=False):
        """Spawn every env (episode 0) and scan it: returns the observation (n_envs, obs_count) float32, plus the aux
        rows with ``aux=True``.  ``start_index`` None: each env draws its start from the pool with the counter-based
        uniform of ``seed``; int32 (n_envs,): the given pool rows.  A torch ``start_index`` or ``on_device=True``
        takes the device form (see the module text: its tensors are overwritten by the next call).  ``read()['done']``
        shows the starts that lie inside the crash margin."""
        seed = int(seed)
        if seed < 0 or seed >= 1 << 64:
            raise ValueError("seed must lie in [0, 2^64)")
        if self._is_tensor(start_index) or on_device:
            t = self._tensors()
            sidx = None
            if start_index is not None:
                if not self._is_tensor(start_index):
                    raise ValueError("on_device=True takes start_index as a torch tensor (or None)")
                self._check_tensor(start_index, (self._n_idx,), "int32", "start_index")
                sidx = start_index.data_ptr()
            _lib.call("rl_env_reset_device", self, seed, sidx, t["obs"].data_ptr(),
                      t["aux"].data_ptr() if aux else None, t["done"].data_ptr(), self._stream())
            return (t["obs"], t["aux"]) if aux else t["obs"]
        sidx = None
        if start_index is not None:
            sidx = np.asarray(start_index)
            if sidx.dtype.kind not in "iu" or sidx.shape != (self._n_idx,):
                raise ValueError("start_index must be integers (%d,)" % self._n_idx)
            if ((sidx < 0) | (sidx >= self.n_starts)).any():
                raise ValueError("start_index must lie in [0, %d)" % self.n_starts)
            sidx = np.ascontiguousarray(sidx, dtype=np.int32)
        obs = np.empty(self.obs_shape, np.float32)
        done = np.empty(self._n, np.int32)
        ax = np.empty((self._n, 4), np.float32) if aux else None
        _lib.call("rl_env_reset", self, seed, sidx, obs, ax, done)
        return (obs, ax) if aux else obs

    def step(self, actions, aux=False):
        """One call of the state machine with ``actions`` (n_envs, 2) float32 as (speed, steer): returns (obs
        (n_envs, obs_count) float32, reward (n_envs,) float32, done (n_envs,) int32) and with ``aux=True`` also
        (n_envs, 4) float32 = (velocity, steer_angle, angular_velocity, slip_angle).  NumPy in, NumPy out
        (synchronous); a torch tensor on the env's device in, the env's own torch tensors out (enqueued on the
        current stream; overwritten by the next call)."""
        if self._is_tensor(actions):
            self._check_tensor(actions, (self._n, 2), "float32", "actions")
            t = self._tensors()
            _lib.call("rl_env_step_device", self, actions.data_ptr(), t["obs"].data_ptr(), t["reward"].data_ptr(),
                      t["done"].data_ptr(), t["aux"].data_ptr() if aux else None, self._stream())
            return (t["obs"], t["reward"], t["done"]) + ((t["aux"],) if aux else ())
        a = np.asarray(actions)
        if a.dtype != np.float32 or a.shape != (self._n, 2):
            raise ValueError("actions must be float32 (n_envs, 2)")
        a = np.ascontiguousarray(a)
        obs = np.empty(self.obs_shape, np.float32)
        reward = np.empty(self._n, np.float32)
        done = np.empty(self._n, np.int32)
        ax = np.empty((self._n, 4), np.float32) if aux else None
        _lib.call("rl_env_step", self, a, obs, reward, done, ax)
        return (obs, reward, done) + ((ax,) if aux else ())

    def read(self):
        """The envs as they stand (waits for the device): a dict of ``states`` float64 (n_envs, 11) and ``ticks``,
        ``episodes``, ``start_index``, ``done`` int32 (n_envs,)."""
        out = dict(states=np.empty((self._n, 11)), ticks=np.empty(self._n, np.int32),
                   episodes=np.empty(self._n, np.int32), start_index=np.empty(self._n, np.int32),
                   done=np.empty(self._n, np.int32))
        _lib.call("rl_env_read", self, *out.values())
        return out


class RaceEnv(DriveEnv):
    """``n_races`` races of P cars on one device, every car driven by the caller's actions.  ``starts`` float64
    (M, P, 11) is the pool of line-ups: a race spawns all its cars from one of them.  ``method``: RM, RMGPU, or
    ``PyCDDTCast(..., races=True)`` (the two-player simulator's method; GiantLUT and Bresenham cannot race).  The race
    is over once fewer than ``min_running`` of its cars run (``race_over`` 1; the cars still running read done = 2) or
    at ``max_ticks`` steps (``race_over`` 2); until then a finished car stays where it is and the others see it.  The
    other arguments are ``DriveEnv``'s.  ``reset`` takes one start index per race; ``reset``, ``step`` and ``read`` give
    the per-car rows as (n_races, P, ...) views, car k of race r at [r, k]; ``step`` takes (n_races, P, 2) actions.

    ``seats``: one driver per seat, ``[None, fg, pol, ...]`` — None is the caller's seat, a ``PyFollowGap`` or a
    ``Policy`` (at most one object of each kind) drives car k of every race itself: at each step such a car takes
    (``seat_speed``, its driver's answer to the car's own scan of the call before: all ``num_rays`` beams, whatever
    ``obs_window`` shows the caller) in place of its row of ``actions``, which is not read.  ``seat_speed``: a scalar or
    one value per seat.  ``seat_steers()`` reads the answers.

    ``league``: ``(pop, entries)`` instead of ``seats`` — a ``PolicyPopulation`` and one entry per car, int
    (n_races, P): ``league.CALLER`` (-2), ``league.FOLLOWGAP`` (-1: ``followgap``) or member m >= 0 of ``pop``;
    ``seat_speed`` is the speed of the scripted cars of a seat.  See ``attach_league``, ``set_entries``, ``entries``,
    ``league_steers`` and ``league_results``."""
    league = None                 # (pop, followgap, seat speeds) while a league is attached

    def __init__(self, method, starts, n_races, num_rays, fov, edge, crash_thresh, *, min_running=1, seats=None,
                 seat_speed=2.0, league=None, followgap=None, **kw):
        checks = {k: kw[k] for k in ("substeps", "obs_window", "obs_clip", "obs_scale", "max_ticks", "steer_clip",
                                     "crash_reward", "dt") if k in kw}
        if seats is not None and league is not None:
            raise ValueError("seats and league exclude each other: a league names every car's driver")
        st, _, _, P = race_env_args(n_races, num_rays, starts, edge, min_running, **checks)
        self._group, self._min_running, self._races = P, int(min_running), int(n_races)
        super().__init__(method, st.reshape(-1, 11), self._races * P, num_rays, fov, edge, crash_thresh, **kw)
        self.n_starts = st.shape[0]
        self._n_idx = self._races
        self.seats = None
        if seats is not None:
            self.attach_seats(seats, seat_speed)
        if league is not None:
            self.attach_league(league[0], league[1], followgap, seat_speed)

    def _create(self, car, method, p, ed, st):
        rp = _lib.RaceEnvParams()
        rp.env, rp.group, rp.min_running = p, self._group, self._min_running
        _lib.call("rl_env_create_race", car, method, rp, ed, st, st.shape[0] // self._group, self._h)

    @property
    def n_races(self):
        return self._races

    @property
    def group(self):
        return self._group

    def _rows(self, x):
        """Per-car rows (n_envs, ...) as (n_races, P, ...), a view in both forms."""
        return x.reshape((self._races, self._group) + tuple(x.shape[1:]))

    def reset(self, seed=0, start_index=None, *, aux=False, on_device=False):
        """``DriveEnv.reset`` with ``start_index`` (n_races,): the line-up of every race.  Returns the observation
        (n_races, P, obs_count), plus aux (n_races, P, 4) with ``aux=True``."""
        out = super().reset(seed, start_index, aux=aux, on_device=on_device)
        return tuple(self._rows(x) for x in out) if aux else self._rows(out)

    def step(self, actions, aux=False):
        """``DriveEnv.step`` with ``actions`` (n_races, P, 2) (or the per-car rows (n_envs, 2)): returns obs
        (n_races, P, obs_count), reward and done (n_races, P), and aux (n_races, P, 4) with ``aux=True``."""
        if tuple(actions.shape) == (self._races, self._group, 2):
            actions = actions.reshape(self._n, 2)
        return tuple(self._rows(x) for x in super().step(actions, aux))

    # -- per-seat drivers ---------------------------------------------------------------
    def attach_seats(self, seats, seat_speed=2.0):
        """Give the seats their drivers (``seats`` and ``seat_speed`` as the constructor takes them; None: detach, every
        seat is the caller's again).  The env needs a ``reset`` afterwards."""
        from .seats import seat_env_args
        if seats is not None and self.league is not None:
            raise ValueError("a league is attached (attach_league(None) first)")
        if seats is None:
            _lib.call("rl_env_attach_seats", self, None, None, None)
            self.seats = None
            return
        sp, fg, pol = seat_env_args(seats, seat_speed, self._group, self.params.num_rays)
        _lib.call("rl_env_attach_seats", self, fg, pol, sp)
        self.seats = (tuple(seats), fg, pol)      # (borrowed by the library: kept alive here)

    def seat_steers(self, on_device=False):
        """Each car's seat driver's answer to its latest scan, float32 (n_races, P): the steer it takes at the next
        step.  NaN for a car in the caller's seat and for one that is not running after that scan.  NumPy by default
        (waits for the device); ``on_device=True``: the env's own torch tensor, filled on the current stream and
        overwritten by the next call."""
        if self.seats is None:
            raise ValueError("no seats attached (attach_seats)")
        if on_device:
            import torch
            if getattr(self, "_seat_torch", None) is None:
                self._seat_torch = torch.empty(self._n, dtype=torch.float32, device=torch.device("cuda", self.device))
            out = self._seat_torch
            _lib.call("rl_env_read_seats_device", self, out.data_ptr(), self._stream())
        else:
            out = np.empty(self._n, np.float32)
            _lib.call("rl_env_read_seats", self, out)
        return self._rows(out)

    # -- league line-ups ----------------------------------------------------------------
    def attach_league(self, pop, entries=None, followgap=None, seat_speed=2.0):
        """Give every car its driver: ``entries`` int (n_races, P) with ``league.CALLER`` (-2, the caller's actions),
        ``league.FOLLOWGAP`` (-1, ``followgap``) or m >= 0, member m of ``pop`` (a ``PolicyPopulation``).  A scripted
        car (an entry >= -1) takes (``seat_speed`` of its seat, its driver's answer to the car's own full scan of the
        call before) in place of its row of ``actions``.  ``pop`` None (or ``entries`` None) detaches the league.  The
        env needs a ``reset`` afterwards; the results start at zero."""
        from . import league as LG
        if pop is None or entries is None:
            _lib.call("rl_env_attach_league", self, None, None, None, None)
            self.league = None
            return
        if self.seats is not None:
            raise ValueError("seats are attached (attach_seats(None) first)")
        spd = LG.seat_speeds(seat_speed, self._group)
        ent = LG.league_env_args(entries, self._races, self._group, pop, followgap, self.params.num_rays, spd)
        _lib.call("rl_env_attach_league", self, followgap, pop, ent, np.where(np.isfinite(spd), spd, np.float32(0)))
        self.league = (pop, followgap, spd)       # (borrowed by the library: kept alive here)
        self._league_torch = None

    def _need_league(self):
        if self.league is None:
            raise ValueError("no league attached (attach_league)")
        return self.league

    def set_entries(self, entries):
        """Replace the pending line-ups: every race adopts its cars' entries when it next spawns (a reset or an
        auto-reset re-spawn), and a running race keeps the line-up it has.  A NumPy array (n_races, P) takes the host
        form (checked, synchronous); a torch int32 tensor (n_races, P) or (n_envs,) on the env's device takes the
        enqueued form on the current stream, where an entry the checks would refuse behaves as ``league.CALLER``."""
        from . import league as LG
        pop, fg, spd = self._need_league()
        if self._is_tensor(entries):
            if tuple(entries.shape) == (self._races, self._group):
                entries = entries.reshape(self._n)
            self._check_tensor(entries, (self._n,), "int32", "entries")
            _lib.call("rl_env_set_league_entries_device", self, entries.data_ptr(), self._stream())
            return
        ent = LG.league_env_args(entries, self._races, self._group, pop, fg, self.params.num_rays, spd)
        _lib.call("rl_env_set_league_entries", self, ent)

    def entries(self):
        """The line-ups as a dict of ``live`` (what every race runs with) and ``pending`` (what it adopts at its next
        spawn), int32 (n_races, P).  Waits for the device."""
        self._need_league()
        live, pending = np.empty(self._n, np.int32), np.empty(self._n, np.int32)
        _lib.call("rl_env_read_league_entries", self, live, pending)
        return dict(live=self._rows(live), pending=self._rows(pending))

    def league_steers(self, on_device=False):
        """``seat_steers`` for a league: each scripted car's driver's answer to its latest scan, float32 (n_races, P); NaN
        for a caller's car and for one that is not running after that scan."""
        self._need_league()
        if on_device:
            import torch
            if getattr(self, "_league_torch", None) is None:
                self._league_torch = torch.empty(self._n, dtype=torch.float32, device=torch.device("cuda", self.device))
            out = self._league_torch
            _lib.call("rl_env_read_league_steers_device", self, out.data_ptr(), self._stream())
        else:
            out = np.empty(self._n, np.float32)
            _lib.call("rl_env_read_league_steers", self, out)
        return self._rows(out)

    def league_results(self, clear=False):
        """The tally of the races that finished since the attach (or the last ``clear=True``): a dict with one int64
        (n_members,) array per column of ``league.RESULT_COLUMNS`` — ``entered`` (cars in finished races), ``out`` (of
        them, done 1 or 3), ``ticks`` (their summed ticks), ``faced`` / ``beaten`` (cars of their own races),
        ``callers_faced`` / ``callers_beaten`` / ``callers_won`` (the caller's cars among them, and those that beat the
        driver's car) — and the same columns for FollowGap's cars (``followgap``) and the caller's (``caller``) as dicts
        of ints.  A reset does not clear it."""
        from . import league as LG
        pop = self._need_league()[0]
        raw = np.zeros((pop.n_members + 2, 8), np.int64)
        _lib.call("rl_env_read_league_results", self, raw, 1 if clear else 0)
        return LG.results_dict(raw, pop.n_members)

    def track_state(self, on_device=False):
        """``DriveEnv.track_state`` as (n_races, P, ...); ``rank`` 0 leads its race."""
        return {k: self._rows(v) for k, v in super().track_state(on_device).items()}

    def read(self):
        """``DriveEnv.read``'s per-car arrays as (n_races, P, ...), and the races' counters ``race_ticks``,
        ``race_episodes``, ``race_start_index`` and ``race_over`` (0 running, 1 too few cars run, 2 truncated), int32
        (n_races,)."""
        out = {k: self._rows(v) for k, v in super().read().items()}
        names = ("race_ticks", "race_episodes", "race_start_index", "race_over")
        out.update((k, np.empty(self._races, np.int32)) for k in names)
        _lib.call("rl_env_read_races", self, *(out[k] for k in names))
        return out
