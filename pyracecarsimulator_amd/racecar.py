"""Batched vehicle roll-outs for the scan path.

The reference's ``racecar`` package is a C++ ``Car`` behind a Cython ``PyCar``
(/root/reference/racecar/src/racecar.cpp, racecar/pywrapper/racecar.pyx:75-114).  Only the two
pieces of it that sit directly on either side of the batched scan are provided here, batched and
on the GPU:

* before the scan — the roll-out pose generator: ``MCTS.rollout`` calls ``control`` +
  ``updatePosition(0.01)`` 200 times per roll-out (scripts/mcts.py:214-231).  ``CarBatch.rollout``
  integrates any number of roll-outs at once, one GPU lane each, in float64;
* after the scan — the crash test ``isCrashed`` over ``setCarEdgeDistances``' table
  (racecar.cpp:239-292, 305-328; scripts/racecar_simulator_v2.py:47-50, 146-167):
  ``edge_distances`` (host table, same quirks) + the fused device test in ``range_libc``.

``CarBatch.rollout_check`` chains roll-outs -> poses -> scan -> per-roll-out crash index on the
device (poses and ranges never cross PCIe).  ``CarBatch.drive_followgap`` closes the loop: each tick's
steering angle is FollowGap's answer to that tick's scan, all on the device.  ``CarBatch.plan_mcts`` runs
scripts/mcts.py's tree search for many trees at once on the device (``mcts.MCTSPlanner``), ``CarBatch.drive_mcts``
scripts/mcts_driver.py's closed loop of it: every car replans at every decision.
``CarBatch.race_followgap`` runs many races of up to 8 cars at once, each car's scan seeing the other cars of its
race (scripts/two_player/); ``CarBatch.outline_cells`` gives the canonical outline cells of the cars.
``CarBatch.attach_track`` places the cars of every closed-loop roll-out on a ``Track`` after each step they take
(include/scanlib_track_drive.h): ``track_state`` and ``track_scores`` read progress, laps, goal ticks, places and the
population's and league's scores built on them.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

#: constructor order of Car (racecar/include/racecar.hpp:32-36) with the reference's values
#: (params.yaml:3-21,47)
CAR_PARAM_ORDER = ("wb", "fc", "h_cg", "l_f", "l_r", "cs_f", "cs_r", "mass", "I_z", "ttc_thresh",
                   "width", "length", "max_steer_vel", "max_steer_ang", "max_speed", "max_accel",
                   "max_decel")
DEFAULT_CAR = dict(wb=0.3302, fc=1.0, h_cg=0.08255, l_f=0.15875, l_r=0.17145, cs_f=2.3, cs_r=2.3,
                   mass=3.17, I_z=0.0398378, ttc_thresh=0.001, width=0.2032, length=0.4064,
                   max_steer_vel=5.0, max_steer_ang=0.4189, max_speed=7.0, max_accel=3.0,
                   max_decel=20.0)


def edge_distances(num_rays, min_ang, scan_ang_inc, scan_dist_to_base, width, wheelbase):
    """Car::setCarEdgeDistances (racecar.cpp:239-292) as float64[num_rays]: distance from the lidar
    to the car's outline along each beam — native (``rl_car_edge_distances``, host C++ of
    libscan_amd.so; needs no GPU).  Kept as the reference computes it: the angle is incremented BEFORE
    use (table shifted by one beam, :256), ``PI = 3.145`` (racecar.hpp:117), and a beam at exactly
    0 rad gets ``side / sin(-0.0001)`` (a large negative number, :277-283)."""
    out = np.empty(int(num_rays), dtype=np.float64)
    _lib.call("rl_car_edge_distances", num_rays, min_ang, scan_ang_inc, scan_dist_to_base, width, wheelbase, out)
    return out


def is_crashed(rays, num_rays, poses, edge, crash_thresh):
    """Car::isCrashed (racecar.cpp:305-328) over host ranges (``rl_car_is_crashed``): index of the
    first crashed scan, else ``-(poses+1)``."""
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    edge = np.ascontiguousarray(edge, dtype=np.float64)
    if rays.size < num_rays * poses or edge.size < num_rays:
        raise ValueError("is_crashed: rays needs poses*num_rays values, edge num_rays")
    first = C.c_int(0)
    _lib.call("rl_car_is_crashed", rays, num_rays, poses, edge, crash_thresh, first)
    return int(first.value)


class CarBatch(_lib.Handle):
    """Many ``Car`` objects stepped together on one MI355X, or on several (``device=[...]``) (no CPU path)."""
    _destroy = "rl_car_destroy"

    def __init__(self, params=None, device=0):
        p = dict(DEFAULT_CAR)
        p.update(params or {})
        self.params = p
        arr = np.array([p[k] for k in CAR_PARAM_ORDER], dtype=np.float64)
        self._h = C.c_void_p()
        if isinstance(device, (list, tuple)):
            # several devices (pair with a method of PyOMap(device=[...]) on the same list): roll-outs are cut
            # into contiguous blocks, one per device, inside this one process
            devs = np.array([int(d) for d in device], dtype=np.intc)
            _lib.call("rl_car_create_multi", devs, len(devs), arr, self._h)
        else:
            _lib.call("rl_car_create", device, arr, self._h)

    @staticmethod
    def _prep(states, actions, n_steps, action_every):
        states = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 11)
        n_act = (n_steps + action_every - 1) // action_every
        actions = np.ascontiguousarray(actions, dtype=np.float64).reshape(states.shape[0], n_act, 2)
        return states, actions

    def rollout(self, states, actions, n_steps=200, action_every=10, dt=0.01):
        """states float64 (R, 11) in getState layout; actions float64 (R, ceil(n_steps/every), 2) as
        (speed, steer).  Returns (poses float32 (R, n_steps, 3), final states (R, 11), velocities
        (R, n_steps)) — the arrays MCTS.rollout builds (all_sim_states, rewards)."""
        states, actions = self._prep(states, actions, n_steps, action_every)
        R = states.shape[0]
        poses = np.empty((R, n_steps, 3), dtype=np.float32)
        out = np.empty((R, 11), dtype=np.float64)
        vel = np.empty((R, n_steps), dtype=np.float64)
        _lib.call("rl_car_rollout", self, states, actions, R, n_steps, action_every, dt, poses, out, vel)
        return poses, out, vel

    def rollout_check(self, method, states, actions, fov, num_rays, edge, crash_thresh, n_steps=200,
                      action_every=10, dt=0.01):
        """MCTS.rollout + checkCollisionMany for R roll-outs in one call; returns (first crashed
        pose per roll-out int32 (R,), final states (R, 11), velocities (R, n_steps))."""
        states, actions = self._prep(states, actions, n_steps, action_every)
        R = states.shape[0]
        edge = np.ascontiguousarray(edge, dtype=np.float64)
        first = np.zeros(R, dtype=np.int32)
        out = np.empty((R, 11), dtype=np.float64)
        vel = np.empty((R, n_steps), dtype=np.float64)
        _lib.call("rl_car_rollout_check", self, method, states, actions, R, n_steps, action_every, dt, fov, num_rays,
                  edge, crash_thresh, first, out, vel)
        return first, out, vel

    def rollout_track(self, track, states, actions, reward="progress", lookahead=1.5, window=0, goal_span=0,
                      anchors=None, points=None, n_steps=200, action_every=10, dt=0.01):
        """``rollout``'s roll-outs with the per-step reward terms of the track-guided planner
        (``rl_car_rollout_track``, include/scanlib_track_plan.h) on ``track`` (a ``Track``; None for "velocity", and
        for "waypoint" with ``points``).  ``reward`` and the keywords as ``MCTSPlanner.attach_track``; ``anchors``
        int32 (R,): the segments the "progress" windows are centred on (None: the nearest segment of each start);
        ``points`` float64 (R, 2) or (2,): the "waypoint" points (None: the goal rule at each start).  Returns a dict:
        terms float64 (R, n_steps) and, for "progress", s (R, n_steps), segment int32 (R, n_steps), start_s (R,)."""
        from .mcts import plan_track_args, points_args
        states, actions = self._prep(states, actions, n_steps, action_every)
        R = states.shape[0]
        p = plan_track_args(reward, lookahead, window, goal_span, points=points is not None)
        if track is None and (reward == "progress" or (reward == "waypoint" and points is None)):
            raise ValueError("reward %r needs a track" % reward)
        if not 1 <= int(n_steps) <= 512:
            raise ValueError("n_steps must lie in [1, 512]")
        anc = pts = None
        if anchors is not None:
            anc = np.asarray(anchors)
            if anc.dtype.kind not in "iu" or anc.shape != (R,):
                raise ValueError("anchors must be integers (%d,)" % R)
            if track is not None and ((anc < 0) | (anc >= track.n_segments)).any():
                raise ValueError("anchors must lie in [0, %d)" % track.n_segments)
            anc = np.ascontiguousarray(anc, np.int32)
        if points is not None:
            pts = points_args(points, R)
        progress = reward == "progress"
        out = dict(terms=np.empty((R, n_steps)))
        if progress:
            out.update(s=np.empty((R, n_steps)), segment=np.empty((R, n_steps), np.int32), start_s=np.empty(R))
        _lib.call("rl_car_rollout_track", self, track, p, states, actions, R, n_steps, action_every, dt, anc, pts,
                  out["terms"], out.get("s"), out.get("segment"), out.get("start_s"))
        return out

    def drive_followgap(self, method, followgap, states, n_ticks, speed, fov, num_rays, edge, crash_thresh,
                        scan_dist_to_base=0.275, dt=0.01, steer0=None, trace=False):
        """Closed-loop Follow-the-Gap roll-outs (``rl_car_drive_followgap``): every tick steps each live car,
        scans from its lidar pose with ``method``, tests the scan for a crash (a crashed car freezes) and
        steers the next tick with ``followgap``'s answer to that scan — the reference's simulator tick
        (scripts/ros_interface.py:119-148) driven by scripts/two_player/simple_driver.py, for R cars at once.

        states float64 (R, 11) in getState layout; speed a scalar or float64 (R,); steer0 None (0) or
        float32 (R,); edge float64 (num_rays,).  Returns (first crash tick int32 (R,) or -(n_ticks+1),
        final states (R, 11), velocities float64 (R, n_ticks), steers float32 (R, n_ticks)) and with
        ``trace=True`` also (lidar poses float32 (R, n_ticks, 3), states float64 (R, n_ticks, 11)).  Trace
        rows after a car's crash tick, and its steer at that tick, are NaN."""
        return self._drive("rl_car_drive_followgap", (method, followgap), None, (), (), states, n_ticks, speed, fov,
                           num_rays, edge, crash_thresh, scan_dist_to_base, dt, steer0, trace)

    def outline_cells(self, omap, car_poses):
        """The canonical outline cells of each car (``rl_car_outline_cells``, include/scanlib.h) on ``omap`` (a
        ``range_libc.PyOMap``) with this batch's length and width.  car_poses float64 (n, 3) as (x, y, theta).
        Returns (cells int32 (n, max count) as row * cols + col, -1 padded; counts int32 (n,))."""
        cars = np.ascontiguousarray(car_poses, dtype=np.float64).reshape(-1, 3)
        n = cars.shape[0]
        cells = np.empty((n, 512), dtype=np.int32)
        counts = np.zeros(n, dtype=np.int32)
        _lib.call("rl_car_outline_cells", self, omap, cars, n, 512, cells, counts)
        width = int(counts.max()) if n else 0
        return np.ascontiguousarray(cells[:, :width]), counts

    def race_followgap(self, method, followgap, states, n_ticks, speed, fov, num_rays, edge, crash_thresh,
                       steer0=None, dt=0.01, trace=False, scan_dist_to_base=0.275):
        """Batched closed-loop races (``rl_car_race_followgap``): ``drive_followgap``'s loop in which every car's scan
        sees the other cars of its race (scripts/two_player/: ros_interface_two_player.py's tick, simple_driver.py's
        FollowGap).  states float64 (R, P, 11) — R races of P <= 8 cars —; speed a scalar or float64 (R, P); steer0
        None (0) or float32 (R, P).  Returns ``drive_followgap``'s tuple with R P reshaped to (R, P): first crash tick
        (R, P), final states (R, P, 11), velocities and steers (R, P, n_ticks), with ``trace=True`` also lidar poses
        (R, P, n_ticks, 3) and states (R, P, n_ticks, 11).  A crashed car stays in its race as a wreck.  ``method``: RM,
        RMGPU, or ``PyCDDTCast(..., races=True)``; GiantLUT and Bresenham are refused (so in ``race_seats`` and
        ``race_league``)."""
        st, counts = self._race_states(states)
        return self._drive("rl_car_race_followgap", (method, followgap), counts, (), (), st, n_ticks, speed, fov,
                           num_rays, edge, crash_thresh, scan_dist_to_base, dt, steer0, trace)

    def race_seats(self, method, drivers, states, n_ticks, speed, fov, num_rays, edge, crash_thresh, steer_clip=None,
                   steer0=None, dt=0.01, trace=False, scan_dist_to_base=0.275):
        """``race_followgap`` with a driver per seat (``rl_car_race_seats``, include/scanlib_seats.h): ``drivers`` holds
        one ``PyFollowGap`` or ``Policy`` per car of a race (at most one distinct object of each kind), and car k of
        every race is steered by ``drivers[k]``'s answer to its scan — scripts/two_player/ with simple_driver.py in some
        seats and policy_driver.py in others.  ``steer_clip`` as ``drive_policy`` takes it: it clamps the network's
        seats only.  The steers returned are each driver's raw answers.  Arguments (the kinds of ``method`` that race
        included) and results as ``race_followgap``; with FollowGap in every seat it returns that call's bits."""
        from .seats import seat_args
        st, counts = self._race_states(states)
        codes, fg, pol = seat_args(drivers, counts[1], num_rays, caller_ok=False)
        front = (method, fg, pol, codes, self._clip(steer_clip))
        return self._drive("rl_car_race_seats", front, counts, (), (), st, n_ticks, speed, fov, num_rays, edge,
                           crash_thresh, scan_dist_to_base, dt, steer0, trace)

    def drive_policy(self, method, policy, states, n_ticks, speed, fov, num_rays, edge, crash_thresh,
                     scan_dist_to_base=0.275, dt=0.01, steer0=None, steer_clip=None, trace=False):
        """Closed-loop policy roll-outs (``rl_car_drive_policy``): ``drive_followgap``'s loop with the steer of
        every tick from ``policy`` (a ``policy.Policy``) — scripts/policy_driver.py's driver for R cars at once.
        ``steer_clip`` None: the car gets the raw output (as scripts/mcts.py passes it to drive()); a value: the
        output clamped to +-steer_clip (policy_driver.py uses 0.4189).  The steers returned are the raw network
        outputs.  Arguments and results as ``drive_followgap``."""
        return self._drive("rl_car_drive_policy", (method, policy), None, (self._clip(steer_clip),), (), states,
                           n_ticks, speed, fov, num_rays, edge, crash_thresh, scan_dist_to_base, dt, steer0, trace)

    def drive_population(self, method, pop, states, n_ticks, speed, fov, num_rays, edge, crash_thresh, cars_per_member,
                         first=0, steer_clip=None, scan_dist_to_base=0.275, dt=0.01, steer0=None, trace=False):
        """``drive_policy`` for a population (``rl_car_drive_population``, include/scanlib_population.h): ``pop`` a
        ``population.PolicyPopulation``, states float64 (n E, 11) with E = ``cars_per_member``; car r is steered by
        member ``first + r // E`` at every tick, every member's network in one launch.  Returns ``drive_policy``'s
        tuple plus ``fitness`` float64 (n, 2): per member the sum over its cars (ascending, each addition rounded) of
        travel_dist gained (state index 8), and the number of its cars that crashed."""
        clip = self._clip(steer_clip)
        E, first = int(cars_per_member), int(first)
        if E < 1:
            raise ValueError("cars_per_member must be >= 1")

        def members(R):                                    # (the members are known once the cars are counted)
            if R % E:
                raise ValueError("states must hold a whole number of members: %d cars, %d per member" % (R, E))
            n = R // E
            if first < 0 or first + n > pop.n_members:
                raise ValueError("members [%d, %d) do not lie in [0, %d)" % (first, first + n, pop.n_members))
            if int(num_rays) < pop.in_start + pop.dims[0]:
                raise ValueError("scans of %d beams do not hold the policy's window [%d, %d)"
                                 % (num_rays, pop.in_start, pop.in_start + pop.dims[0]))
            return (method, pop, first, n, E, clip), (np.zeros((n, 2), dtype=np.float64), (n, 3))
        return self._drive("rl_car_drive_population", members, (), (), (), states, n_ticks, speed, fov, num_rays, edge,
                           crash_thresh, scan_dist_to_base, dt, steer0, trace)

    def race_league(self, method, pop, entries, states, n_ticks, speed, fov, num_rays, edge, crash_thresh,
                    followgap=None, steer_clip=None, steer0=None, dt=0.01, trace=False, scan_dist_to_base=0.275):
        """``race_seats`` with a line-up per race drawn from a population (``rl_car_race_league``,
        include/scanlib_league.h): ``entries`` int (R, P) names the driver of every car, member m >= 0 of ``pop`` (a
        ``population.PolicyPopulation``) or -1 for ``followgap``; states float64 (R, P, 11).  ``steer_clip`` clamps the
        members' cars only.  Returns ``race_seats``'s tuple plus ``standings`` float64 (n_members, 4): per member the
        cars it entered, the sum of their travel_dist gains (ascending car index, each addition rounded), how many
        crashed, and how many cars of their own races they beat (alive longer, or as long with the larger gain).
        ``method`` as ``race_followgap``: RM, RMGPU or a CDDT handle made with ``races=True``."""
        from .league import league_args
        st, counts = self._race_states(states)
        entry = league_args(entries, counts[0], counts[1], pop, followgap, num_rays)
        front = (method, followgap, pop, entry, self._clip(steer_clip))
        scores = (np.zeros((pop.n_members, 4), dtype=np.float64), (pop.n_members, 4))
        return self._drive("rl_car_race_league", front, counts, (), scores, st, n_ticks, speed, fov, num_rays, edge,
                           crash_thresh, scan_dist_to_base, dt, steer0, trace)

    # -- track progress of the roll-outs (include/scanlib_track_drive.h) -----------------------------------
    _track = None             # the attached ``Track``, kept referenced: the library only borrows it
    _track_shape = None       # the car shape of the last roll-out made with it: (R,) or (n_races, P)
    _score_shape = None       # the shape of the track scores that roll-out left, if any

    def attach_track(self, track, window=0, goal_dist=None):
        """Place the cars of every later roll-out (``drive_*``, ``race_*``) on ``track`` (a ``Track``) after each step
        they take (``rl_car_attach_track``): read the result with ``track_state`` and ``track_scores``.  ``window``: 0
        searches every segment at every tick, w > 0 the segments within w of the previous one; ``goal_dist`` metres of
        progress for ``goal_tick`` (None: one track length).  The roll-outs' own results keep their bits."""
        from .track import Track
        if not isinstance(track, Track):
            raise ValueError("track must be a Track")
        if isinstance(window, (bool, np.bool_)) or not isinstance(window, (int, np.integer)) or not 0 <= window <= 65536:
            raise ValueError("window must be an integer in [0, 65536]")
        if goal_dist is not None and not (isinstance(goal_dist, (int, float, np.integer, np.floating))
                                          and np.isfinite(goal_dist) and goal_dist > 0):
            raise ValueError("goal_dist must be None or finite and > 0")
        goal = 0.0 if goal_dist is None else float(goal_dist)
        _lib.call("rl_car_attach_track", self, track, _lib.DriveTrackParams(int(window), goal))
        self._track, self._track_shape, self._score_shape = track, None, None

    def detach_track(self):
        """Later roll-outs run without a track again (``rl_car_attach_track`` with no track)."""
        _lib.call("rl_car_attach_track", self, None, None)
        self._track = self._track_shape = self._score_shape = None

    def _tracked(self, shape, scores=None):
        """After a roll-out's library call: what ``track_state`` and ``track_scores`` may ask for."""
        if self._track is not None:
            self._track_shape, self._score_shape = tuple(int(v) for v in shape), scores

    def track_state(self):
        """Where the last roll-out's cars are on the attached track (``rl_car_read_track``): a dict of s0, s, progress
        and race_dist (float64), segment, laps, goal_tick and rank (int32), each shaped (R,) or, after a race,
        (n_races, P)."""
        if self._track is None or self._track_shape is None:
            raise ValueError("track_state needs an attached track and a roll-out made with it")
        shape = self._track_shape
        R = int(np.prod(shape))
        rows, ints = np.empty((R, 4), dtype=np.float64), np.empty((R, 4), dtype=np.intc)
        _lib.call("rl_car_read_track", self, R, rows, ints)
        out = {k: np.ascontiguousarray(rows[:, i]).reshape(shape) for i, k in enumerate(("s0", "s", "progress", "race_dist"))}
        out.update({k: np.ascontiguousarray(ints[:, i]).astype(np.int32).reshape(shape)
                    for i, k in enumerate(("segment", "laps", "goal_tick", "rank"))})
        return out

    def track_scores(self):
        """The track scores the last roll-out left (``rl_car_read_track_scores``): float64 (n, 3) after
        ``drive_population`` — per member the sum of its cars' progress (ascending, each addition rounded), how many
        reached ``goal_dist`` and the sum of their goal ticks —, (n_members, 4) after ``race_league`` — cars entered,
        the sum of their progress, how many reached the goal, and how many cars of their own races they are ahead of."""
        shape = self._score_shape
        if self._track is None or self._track_shape is None or shape is None:
            raise ValueError("track_scores needs an attached track and a drive_population or race_league made with it")
        out = np.empty(shape, dtype=np.float64)
        _lib.call("rl_car_read_track_scores", self, shape[0], shape[1], out)
        return out

    def plan_mcts(self, method, followgap_or_policy, root_states, n_iterations, seeds, fov, num_rays, edge,
                  crash_thresh, root_actions=0.0, source=None, rollout_steps=200, action_every=10, speed=2.0,
                  dt=0.01, scan_dist_to_base=0.275, C_ucb=0.5, crash_pen=-10.0, uni_dev=0.05, max_nodes=None,
                  trees=False, track=None, track_reward="progress", lookahead=1.5, track_window=0, goal_span=0,
                  rollout="random", rollout_dev=0.1):
        """scripts/mcts.py's search for K trees at once (``rl_mcts_*``, one tree per root state): ``n_iterations``
        iterations each, every tree adding one node per iteration.  ``followgap_or_policy``: a ``PyFollowGap``
        (source "fg"), a ``Policy`` ("nn") or None ("random"); ``source`` overrides the choice.  root_states float64
        (K, 11), root_actions scalar or (K,), seeds uint64 (K,).  Returns (best root action float64 (K,), its visits
        int32 (K,), nodes per tree int32 (K,)) and with ``trees=True`` also the K node-array dicts of
        ``MCTSPlanner.read_tree``.  ``track`` (a ``Track``): the roll-outs are rewarded along it, ``track_reward``,
        ``lookahead``, ``track_window`` and ``goal_span`` as ``MCTSPlanner.attach_track`` takes them
        (``track_reward="velocity"`` attaches it for the steering alone).  ``source="track"`` (no handle:
        ``followgap_or_policy`` None) expands with the pure pursuit of the track's goal waypoint, ``rollout="pursuit"``
        steers the roll-outs along it with a deviation of +-``rollout_dev``; both need ``track``."""
        from .mcts import rollout_args, steering_args
        rollout_args(rollout, rollout_dev)
        steering_args(source, rollout, track, False)
        root_states = np.asarray(root_states, np.float64).reshape(-1, 11)
        K = root_states.shape[0]
        n_iterations = int(n_iterations)
        pl = self._planner(method, followgap_or_policy, source, K, max_nodes or n_iterations + 1, fov, num_rays, edge,
                           crash_thresh, rollout_steps=rollout_steps, action_every=action_every, speed=speed, dt=dt,
                           scan_dist_to_base=scan_dist_to_base, C_ucb=C_ucb, crash_pen=crash_pen, uni_dev=uni_dev,
                           rollout=rollout, rollout_dev=rollout_dev)
        try:
            if track is not None:
                pl.attach_track(track, track_reward, lookahead, track_window, goal_span)
            pl.reset(root_states, root_actions, seeds)
            pl.run(n_iterations)
            res = pl.best()
            if trees:
                res = res + ([pl.read_tree(k) for k in range(K)],)
        finally:
            pl.close()
        return res

    def drive_mcts(self, method, followgap_or_policy, states, n_decisions, n_iterations, seeds, fov, num_rays, edge,
                   crash_thresh, recent_actions=0.0, source=None, steps_per_decision=1, steer_clip=None,
                   rollout_steps=200, action_every=10, speed=2.0, dt=0.01, scan_dist_to_base=0.275, C_ucb=0.5,
                   crash_pen=-10.0, uni_dev=0.05, trace=False, track=None, track_reward="progress", lookahead=1.5,
                   track_window=0, goal_span=0, rollout="random", rollout_dev=0.1):
        """scripts/mcts_driver.py's closed loop for K cars at once (``rl_mcts_drive``): every car replans at each of
        ``n_decisions`` decisions (a fresh tree of ``n_iterations`` iterations from its state) and takes
        ``steps_per_decision`` steps with the most visited root action.  Source and handles as ``plan_mcts``; states
        float64 (K, 11), recent_actions scalar or (K,), seeds integers (K,).  Returns ``MCTSPlanner.drive``'s tuple.
        ``track`` and its keywords as ``plan_mcts``: the roots are placed on it anew at every decision, on the device;
        ``source="track"``, ``rollout`` and ``rollout_dev`` as ``plan_mcts``."""
        from .mcts import rollout_args, steering_args
        rollout_args(rollout, rollout_dev)
        steering_args(source, rollout, track, False)
        states = np.asarray(states)
        if states.dtype != np.float64 or states.ndim != 2 or states.shape[1] != 11:
            raise ValueError("states must be float64 (K, 11)")
        pl = self._planner(method, followgap_or_policy, source, states.shape[0], int(n_iterations) + 1, fov, num_rays,
                           edge, crash_thresh, rollout_steps=rollout_steps, action_every=action_every, speed=speed,
                           dt=dt, scan_dist_to_base=scan_dist_to_base, C_ucb=C_ucb, crash_pen=crash_pen, uni_dev=uni_dev,
                           rollout=rollout, rollout_dev=rollout_dev)
        try:
            if track is not None:
                pl.attach_track(track, track_reward, lookahead, track_window, goal_span)
            return pl.drive(states, recent_actions, seeds, n_decisions, n_iterations,
                            steps_per_decision=steps_per_decision, steer_clip=steer_clip, trace=trace)
        finally:
            pl.close()

    def _planner(self, method, followgap_or_policy, source, n_trees, max_nodes, *args, **kw):
        """The ``MCTSPlanner`` of ``plan_mcts`` and ``drive_mcts``: ``source`` None picks "random" for no handle, "nn"
        for a ``Policy``, "fg" otherwise; the handle goes to the planner as the source's."""
        from .mcts import MCTSPlanner
        from .policy import Policy
        if source is None:
            source = "random" if followgap_or_policy is None else ("nn" if isinstance(followgap_or_policy, Policy)
                                                                   else "fg")
        return MCTSPlanner(self, method, n_trees, max_nodes, *args, source=source,
                           followgap=followgap_or_policy if source == "fg" else None,
                           policy=followgap_or_policy if source == "nn" else None, **kw)

    @staticmethod
    def _clip(steer_clip):
        """``steer_clip`` as the library takes it: 0 for None (the raw output), else a value > 0."""
        if steer_clip is not None and not float(steer_clip) > 0:
            raise ValueError("steer_clip must be None or > 0")
        return 0.0 if steer_clip is None else float(steer_clip)

    @staticmethod
    def _race_states(states):
        """A race's states float64 (R, P, 11) as an array, and (R, P): the car-count arguments of its roll-out."""
        st = np.asarray(states)
        if st.dtype != np.float64 or st.ndim != 3 or st.shape[2] != 11:
            raise ValueError("states must be float64 (R, P, 11)")
        return st, (st.shape[0], st.shape[1])

    def _drive(self, fn, front, counts, after_thresh, scores, states, n_ticks, speed, fov, num_rays, edge, crash_thresh,
               scan_dist_to_base, dt, steer0, trace):
        """The one library call of the closed-loop roll-outs, ``fn``.  ``front``: what stands between the cars and
        ``states_in`` (the method, the steering source's handles and arguments).  ``counts``: the car-count arguments,
        None for (R,), () for none (a population), (n_races, group) for a race, whose states, speed and steer0 come
        shaped (R, P, ...) and whose results go back that way.  ``after_thresh`` goes after crash_thresh (the policy's
        steer_clip).  ``scores``: (), or the score array that goes last and the shape of the track scores of such a
        roll-out.  Where these depend on the number of cars, ``front`` is a function of it that gives (front, scores)."""
        race = counts is not None and len(counts) == 2
        if race:
            states = states.reshape(-1, 11)
            speed = np.asarray(speed, dtype=np.float64)
            speed = float(speed) if speed.ndim == 0 else speed.reshape(-1)
            steer0 = None if steer0 is None else np.asarray(steer0).reshape(-1)
        R, n_ticks, states, speeds, st0, edge, first, out, vel, steers, poses, trace_st = self._drive_args(
            states, n_ticks, speed, num_rays, edge, steer0, trace)
        if callable(front):
            front, scores = front(R)
        _lib.call(fn, self, *front, states, speeds, st0, *((R,) if counts is None else counts), n_ticks, dt,
                  scan_dist_to_base, fov, num_rays, edge, crash_thresh, *after_thresh, first, out, vel, steers, poses,
                  trace_st, *scores[:1])
        self._tracked(counts if race else (R,), *scores[1:])
        res = (first, out, vel, steers) + ((poses, trace_st) if trace else ())
        if race:                                           # every array's leading R P becomes (R, P)
            res = tuple(a.reshape(counts + a.shape[1:]) for a in res)
        return res + scores[:1]

    @staticmethod
    def _drive_args(states, n_ticks, speed, num_rays, edge, steer0, trace):
        states = np.asarray(states)
        if states.dtype != np.float64 or states.ndim != 2 or states.shape[1] != 11:
            raise ValueError("states must be float64 (R, 11)")
        states = np.ascontiguousarray(states)
        R, n_ticks = states.shape[0], int(n_ticks)
        speeds = np.asarray(speed, dtype=np.float64)
        if speeds.ndim == 0:
            speeds = np.full(R, float(speeds))
        if speeds.shape != (R,):
            raise ValueError("speed must be a scalar or float64 (R,)")
        speeds = np.ascontiguousarray(speeds)
        st0 = None
        if steer0 is not None:
            st0 = np.asarray(steer0)
            if st0.dtype != np.float32 or st0.shape != (R,):
                raise ValueError("steer0 must be float32 (R,)")
            st0 = np.ascontiguousarray(st0)
        edge = np.asarray(edge)
        if edge.dtype != np.float64 or edge.shape != (int(num_rays),):
            raise ValueError("edge must be float64 (num_rays,)")
        edge = np.ascontiguousarray(edge)
        T = max(n_ticks, 0)
        first = np.zeros(R, dtype=np.int32)
        out = np.empty((R, 11), dtype=np.float64)
        vel = np.empty((R, T), dtype=np.float64)
        steers = np.empty((R, T), dtype=np.float32)
        poses = np.empty((R, T, 3), dtype=np.float32) if trace else None
        trace_st = np.empty((R, T, 11), dtype=np.float64) if trace else None
        return R, n_ticks, states, speeds, st0, edge, first, out, vel, steers, poses, trace_st
