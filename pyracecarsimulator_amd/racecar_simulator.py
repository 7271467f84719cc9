"""``RacecarSimulator`` — the reference's simulator façade over the MI355X scan path.

Same constructor config and methods as /root/reference/scripts/racecar_simulator_v2.py
(``__init__`` :7-66, ``setState``/``getState`` :68-83, ``getMeanVelocity`` :85-90,
``getTravelDistance`` :92-97, ``getScan`` :99-105, ``runScan`` :108-116, ``drive`` :118-124,
``updatePose`` :126-132, ``checkCollision`` :134-144, ``checkCollisionMany`` :146-167, ``stop``
:169-188, ``setMap`` :190-197, ``setRaytracingMethod`` :199-204), so ``scripts/mcts.py`` can drive
it unchanged.  The two native pieces behind it are on the GPU:

* the vehicle (``racecar.PyCar``) -> ``racecar.CarBatch`` with one roll-out (float64 dynamics);
* ``car.isCrashed(scanMany(poses))`` -> the crash test fused into the scan kernel, so
  ``checkCollisionMany`` moves 12 B per pose down and one int back.

``rolloutMany`` is the batched form of ``MCTS.rollout`` + ``checkCollisionMany``
(scripts/mcts.py:202-245) for any number of roll-outs per call; ``driveFollowGapMany`` the closed
loop of the simulator tick and simple_driver.py's FollowGap answer to every scan; ``drivePolicyMany`` the same loop
steered by the policy network (scripts/policy_driver.py); ``planMCTSMany`` scripts/mcts.py's tree search from many
start states at once; ``raceFollowGapMany`` many races of up to 8 cars that see each other (scripts/two_player/);
``driveEnv`` the same tick with the steering left to the caller (``env.DriveEnv``), ``raceEnv`` the race's
(``env.RaceEnv``).
"""
from __future__ import annotations

import math

import numpy as np

from . import racecar as RC
from .scan_simulator import ScanSimulator2D


class RacecarSimulator:

    def __init__(self, config, verbose=False, device=0):
        self.verbose = verbose
        self.map_frame = "map"
        self.base_frame = "base_link"
        self.scan_frame = "laser"
        self.config = config

        self.scan_dist_to_base = config["scan_dist_to_base"]
        self.max_speed = config["max_speed"]
        self.max_accel = config["max_accel"]
        self.max_steer_ang = config["max_steer_ang"]
        self.max_steer_vel = config["max_steer_vel"]
        self.max_decel = config["max_decel"]
        self.width = config["width"]
        self.length = config["length"]
        self.batch_size = config["batch_size"]
        self.num_rays = config["scan_beams"]
        self.scan_fov = config["scan_fov"]
        self.scan_std = config["scan_std"]
        self.scan_max_range = config["scan_max_range"]
        self.free_thresh = config["free_thresh"]
        self.ttc_thresh = config["ttc_thresh"]

        # car object: racecar.PyCar(...) in the reference (:37-44)
        self.car_params = {k: config[k] for k in RC.CAR_PARAM_ORDER}
        self.car = RC.CarBatch(self.car_params, device=device)
        self._device = device
        self._followgap = None      # driveFollowGapMany's driver, built at its first call
        self._state = np.zeros(11, dtype=np.float64)
        # where the lidar beams leave the car body: setCarEdgeDistances (:47-50)
        self.edge_distances = RC.edge_distances(self.num_rays, -self.scan_fov / 2.0,
                                                self.scan_fov / self.num_rays,
                                                self.scan_dist_to_base, config["width"], config["wb"])
        self.scan_simulator = ScanSimulator2D(self.num_rays, self.scan_fov, self.scan_std,
                                              self.batch_size)
        self.scan = np.zeros(self.num_rays, dtype=np.float32)
        self.desired_speed = 0.0
        self.desired_steer_ang = 0.0
        if self.verbose:
            print("Simulator constructed")

    # -- state ---------------------------------------------------------------------
    def setState(self, state):
        self._state = np.array(state, dtype=np.float64)
        self._state[7] = 1.0 if self._state[7] > 0.0 else 0.0      # racecar.cpp:345-352

    def getState(self):
        return self._state.copy()

    def getMeanVelocity(self):
        return self._state[9] / self._state[10]                    # racecar.cpp:100-107

    def getTravelDistance(self):
        return self._state[8]

    def getScan(self):
        return self.scan

    def laserScanFields(self, stamp=None, frame_id="laser"):
        """The fields RunSimulationViz.lidarPub puts into sensor_msgs/LaserScan
        (scripts/ros_interface.py:332-348) as a plain dict (there is no ROS on the GPU box): the fan
        convention every consumer of the scan relies on.  ``ranges`` and ``intensities`` alias the
        current scan, as the reference's message does."""
        return {
            "header": {"stamp": stamp, "frame_id": frame_id},
            "angle_min": -self.scan_fov / 2.0,
            "angle_max": self.scan_fov / 2.0,
            "angle_increment": self.scan_fov / self.num_rays,
            "range_max": self.config["scan_max_range"],
            "ranges": self.scan,
            "intensities": self.scan,
        }

    # -- one tick -------------------------------------------------------------------
    def getScanPose(self):
        """Car::getScanPose (racecar.cpp:378-387): the lidar sits scan_dist_to_base ahead."""
        x, y, th = self._state[0], self._state[1], self._state[2]
        return (x + self.scan_dist_to_base * math.cos(th), y + self.scan_dist_to_base * math.sin(th), th)

    def runScan(self):
        """One scan from the lidar pose (:108-116); the ranges land in the simulator's cached output vector
        (same alias semantics as ``scan()``)."""
        self.scan = self.scan_simulator.scan(*self.getScanPose())

    def drive(self, desired_speed, desired_steer_ang):
        self.desired_speed = desired_speed
        self.desired_steer_ang = desired_steer_ang

    def updatePose(self, dt=0.01):
        """car.control(...) + car.updatePosition(dt) (:126-132)."""
        _, out, _ = self.car.rollout(self._state[None, :],
                                     np.array([[[self.desired_speed, self.desired_steer_ang]]]),
                                     n_steps=1, action_every=1, dt=dt)
        self._state = out[0]

    def checkCollision(self):
        """isCrashed(scan, num_rays, 1) on the scan array's CURRENT contents, as the reference evaluates it
        (:134-144): 0 when the scan touches the car outline, else -2.  ``self.scan`` aliases the simulator's
        cached vector — a later ``scan()`` or an in-place edit changes what is tested, exactly as in the
        reference — so nothing is cached here: the native host test is one pass over num_rays floats."""
        return RC.is_crashed(self.scan, self.num_rays, 1, self.edge_distances, self.ttc_thresh)

    def checkCollisionMany(self, poses):
        """scanMany + isCrashed fused on the device: index of the first crashed pose of the first
        ``batch_size`` poses, else -(batch_size+1)."""
        b = self.batch_size
        p = np.ascontiguousarray(np.asarray(poses, dtype=np.float32)[:b, :3])
        if p.shape[0] < b:
            raise IndexError("checkCollisionMany needs batch_size poses")     # scan_simulator.py:119
        return self.scan_simulator.scan_method.check_collision_many(
            p, self.scan_fov, self.num_rays, self.edge_distances, self.ttc_thresh)

    def rolloutMany(self, states, actions, n_steps=None, action_every=10, dt=0.01):
        """R roll-outs at once: (first crashed pose per roll-out or -(n_steps+1), final states,
        per-step velocities) — poses and ranges stay on the GPU."""
        n_steps = self.batch_size if n_steps is None else n_steps
        return self.car.rollout_check(self.scan_simulator.scan_method, states, actions, self.scan_fov,
                                      self.num_rays, self.edge_distances, self.ttc_thresh,
                                      n_steps=n_steps, action_every=action_every, dt=dt)

    def driveFollowGapMany(self, states, n_ticks, speed=2.0, track=None, track_window=0, goal_dist=None):
        """R closed-loop roll-outs of the reference's tick (scripts/ros_interface.py:119-148: updatePose, runScan,
        checkCollision() >= 0) steered by ``PyFollowGap(10, 15.0, max_steer_ang, 0.004)`` as
        scripts/two_player/simple_driver.py:31 builds it, on this simulator's range method, edge table and
        ttc_thresh.  Returns ``CarBatch.drive_followgap``'s (first crash tick or -(n_ticks+1), final states,
        velocities, steers); ranges never leave the GPU.  ``track`` (a ``Track``): the cars are placed on it
        (``CarBatch.attach_track`` for the call, ``track_window`` and ``goal_dist`` as it takes them) and
        ``CarBatch.track_state``'s dict is appended to the tuple."""
        if self._followgap is None:
            from .followgap import PyFollowGap
            self._followgap = PyFollowGap(10, 15.0, self.max_steer_ang, 0.004, device=self._device)
        return self._tracked(track, track_window, goal_dist, False, self.car.drive_followgap,
                             self.scan_simulator.scan_method, self._followgap,
                                        np.asarray(states, dtype=np.float64).reshape(-1, 11), n_ticks, speed,
                                        self.scan_fov, self.num_rays, self.edge_distances, self.ttc_thresh,
                                        scan_dist_to_base=self.scan_dist_to_base)

    def raceFollowGapMany(self, states, n_ticks, speed=2.0, track=None, track_window=0, goal_dist=None):
        """R batched races of P cars (states float64 (R, P, 11)) under ``driveFollowGapMany``'s driver, method, edge
        table and ttc_thresh: scripts/two_player/'s tick (every car steps, then every car scans with the others in the
        map) for many races at once.  Returns ``CarBatch.race_followgap``'s (first crash tick or -(n_ticks+1) (R, P),
        final states, velocities, steers); ranges never leave the GPU.  ``track`` (a ``Track``): the cars are placed
        on it (``CarBatch.attach_track`` for the call, ``track_window`` and ``goal_dist`` as it takes them) and
        ``CarBatch.track_state``'s dict is appended to the tuple."""
        if self._followgap is None:
            from .followgap import PyFollowGap
            self._followgap = PyFollowGap(10, 15.0, self.max_steer_ang, 0.004, device=self._device)
        return self._tracked(track, track_window, goal_dist, False, self.car.race_followgap,
                             self.scan_simulator.scan_method, self._followgap,
                                       np.asarray(states, dtype=np.float64), n_ticks, speed, self.scan_fov,
                                       self.num_rays, self.edge_distances, self.ttc_thresh,
                                       scan_dist_to_base=self.scan_dist_to_base)

    def raceSeatsMany(self, states, n_ticks, drivers, speed=2.0, steer_clip=None, track=None, track_window=0,
                      goal_dist=None):
        """``raceFollowGapMany`` with a driver per seat: ``drivers`` holds, for each of the P cars of a race, a
        ``policy.Policy``, a ``PyFollowGap`` or the string "fg" (this simulator's own FollowGap driver, as
        ``raceFollowGapMany`` builds it) — scripts/two_player/ with the network in some seats and simple_driver.py in
        the others.  ``steer_clip`` clamps the network's seats only (scripts/policy_driver.py uses 0.4189).  Returns
        ``CarBatch.race_seats``'s tuple.  ``track`` (a ``Track``): the cars are placed on it
        (``CarBatch.attach_track`` for the call, ``track_window`` and ``goal_dist`` as it takes them) and
        ``CarBatch.track_state``'s dict is appended to the tuple."""
        drivers = [self._mcts_source("fg", None) if isinstance(d, str) and d == "fg" else d for d in drivers]
        return self._tracked(track, track_window, goal_dist, False, self.car.race_seats,
                             self.scan_simulator.scan_method, drivers, np.asarray(states, dtype=np.float64),
                                   n_ticks, speed, self.scan_fov, self.num_rays, self.edge_distances, self.ttc_thresh,
                                   steer_clip=steer_clip, scan_dist_to_base=self.scan_dist_to_base)

    def drivePolicyMany(self, states, n_ticks, policy, speed=2.0, steer_clip=None, track=None, track_window=0,
                        goal_dist=None):
        """``driveFollowGapMany`` with the steer of every tick from ``policy`` (a ``policy.Policy``, e.g.
        ``Policy('model/frozen_model.pb')``): scripts/policy_driver.py's driver with ``steer_clip=0.4189``, MCTS's
        roll-out policy (scripts/mcts.py:252-256, the raw output) with None.  Returns
        ``CarBatch.drive_policy``'s tuple.  ``track`` (a ``Track``): the cars are placed on it
        (``CarBatch.attach_track`` for the call, ``track_window`` and ``goal_dist`` as it takes them) and
        ``CarBatch.track_state``'s dict is appended to the tuple."""
        return self._tracked(track, track_window, goal_dist, False, self.car.drive_policy,
                             self.scan_simulator.scan_method, policy,
                                     np.asarray(states, dtype=np.float64).reshape(-1, 11), n_ticks, speed,
                                     self.scan_fov, self.num_rays, self.edge_distances, self.ttc_thresh,
                                     scan_dist_to_base=self.scan_dist_to_base, steer_clip=steer_clip)

    def drivePopulationMany(self, states, n_ticks, pop, cars_per_member, speed=2.0, first=0, steer_clip=None, track=None,
                            track_window=0, goal_dist=None):
        """``drivePolicyMany`` for a ``population.PolicyPopulation``: states (n E, 11), car r steered by member
        ``first + r // E`` (E = ``cars_per_member``), every member's network in one launch per tick.  Returns
        ``CarBatch.drive_population``'s tuple, the (n, 2) ``fitness`` last.  ``track`` (a ``Track``): the cars are placed
        on it (``CarBatch.attach_track`` for the call, ``track_window`` and ``goal_dist`` as it takes them) and
        ``CarBatch.track_state``'s dict is appended to the tuple, then ``CarBatch.track_scores``'s (n, 3)."""
        return self._tracked(track, track_window, goal_dist, True, self.car.drive_population,
                             self.scan_simulator.scan_method, pop,
                                         np.asarray(states, dtype=np.float64).reshape(-1, 11), n_ticks, speed,
                                         self.scan_fov, self.num_rays, self.edge_distances, self.ttc_thresh,
                                         cars_per_member, first=first, steer_clip=steer_clip,
                                         scan_dist_to_base=self.scan_dist_to_base)

    def raceLeagueMany(self, states, n_ticks, pop, entries, speed=2.0, steer_clip=None, track=None, track_window=0,
                       goal_dist=None):
        """``raceSeatsMany`` with a line-up per race drawn from a ``population.PolicyPopulation``: ``entries`` int
        (R, P) names every car's driver, member m >= 0 of ``pop`` or -1 for this simulator's own FollowGap driver (as
        ``raceFollowGapMany`` builds it).  ``steer_clip`` clamps the members' cars only.  Returns
        ``CarBatch.race_league``'s tuple, the (n_members, 4) ``standings`` last.  ``track`` (a ``Track``): the cars are
        placed on it (``CarBatch.attach_track`` for the call, ``track_window`` and ``goal_dist`` as it takes them) and
        ``CarBatch.track_state``'s dict is appended to the tuple, then ``CarBatch.track_scores``'s
        (n_members, 4)."""
        fg = self._mcts_source("fg", None) if (np.asarray(entries) < 0).any() else None
        return self._tracked(track, track_window, goal_dist, True, self.car.race_league,
                             self.scan_simulator.scan_method, pop, entries, np.asarray(states, dtype=np.float64),
                                    n_ticks, speed, self.scan_fov, self.num_rays, self.edge_distances, self.ttc_thresh,
                                    followgap=fg, steer_clip=steer_clip, scan_dist_to_base=self.scan_dist_to_base)

    def _tracked(self, track, track_window, goal_dist, scores, rollout, *args, **kw):
        """``rollout(*args, **kw)`` of ``self.car``; with a ``track`` it is attached for the call and detached
        afterwards, and ``track_state`` (``scores``: then ``track_scores``) is appended to the result."""
        if track is None:
            return rollout(*args, **kw)
        self.car.attach_track(track, track_window, goal_dist)
        try:
            res = rollout(*args, **kw)
            extra = (self.car.track_state(),) + ((self.car.track_scores(),) if scores else ())
        finally:
            self.car.detach_track()
        return tuple(res) + extra

    def _mcts_source(self, source, policy):
        if source == "fg":
            if self._followgap is None:
                from .followgap import PyFollowGap
                self._followgap = PyFollowGap(10, 15.0, self.max_steer_ang, 0.004, device=self._device)
            return self._followgap
        if source == "nn":
            if policy is None:
                raise ValueError("source 'nn' needs a policy")
            return policy
        return None

    def planMCTSMany(self, states, n_iterations, seeds=None, source="fg", policy=None, root_actions=0.0, track=None,
                     track_reward="progress", lookahead=1.5, track_window=0, goal_span=0, rollout="random",
                     rollout_dev=0.1):
        """scripts/mcts.py's search from each of R start states at once (one tree each, ``n_iterations`` iterations,
        roll-outs of ``batch_size`` steps) on this simulator's range method, edge table and ttc_thresh; ``source``
        "fg" (PyFollowGap(10, 15.0, max_steer_ang, 0.004)), "nn" (``policy``) or "random".  seeds: one per tree
        (default 0 ... R-1).  ``track`` (a ``Track``) and its keywords as ``CarBatch.plan_mcts``: the roll-outs are
        rewarded along the track; ``source="track"`` and ``rollout="pursuit"`` (with ``rollout_dev``) let it steer the
        search as well.  Returns ``CarBatch.plan_mcts``'s (best actions, their visits, nodes per tree)."""
        from .mcts import rollout_args, steering_args
        rollout_args(rollout, rollout_dev)
        steering_args(source, rollout, track, False)
        states = np.asarray(states, dtype=np.float64).reshape(-1, 11)
        R = states.shape[0]
        seeds = np.arange(R, dtype=np.uint64) if seeds is None else np.asarray(seeds, np.uint64)
        handle = self._mcts_source(source, policy)
        return self.car.plan_mcts(self.scan_simulator.scan_method, handle, states, n_iterations, seeds,
                                  self.scan_fov, self.num_rays, self.edge_distances, self.ttc_thresh,
                                  root_actions=root_actions, source=source, rollout_steps=self.batch_size,
                                  scan_dist_to_base=self.scan_dist_to_base, track=track, track_reward=track_reward,
                                  lookahead=lookahead, track_window=track_window, goal_span=goal_span, rollout=rollout,
                                  rollout_dev=rollout_dev)

    def driveMCTSMany(self, states, n_decisions, n_iterations, seeds=None, source="fg", policy=None, steer_clip=0.4189,
                      steps_per_decision=1, recent_actions=0.0, track=None, track_reward="progress", lookahead=1.5,
                      track_window=0, goal_span=0, rollout="random", rollout_dev=0.1):
        """scripts/mcts_driver.py's action callback (:207-264) for R cars at once: at each of ``n_decisions``
        decisions every car plans a fresh tree from its state (``planMCTSMany``'s search and source, seed
        ``seeds + d``), then takes ``steps_per_decision`` steps with the most visited root action; the recent action
        at the next root is that action clamped to +-``steer_clip`` (the driver's 0.4189; None: raw).  Returns
        ``CarBatch.drive_mcts``'s (first crash decision or -(n_decisions+1), final states, recent actions, actions
        (R, n_decisions), visits (R, n_decisions)); nothing leaves the GPU between decisions, with a ``track`` (keywords
        as ``planMCTSMany``, ``source="track"`` and ``rollout="pursuit"`` included) neither: every decision's roots are
        placed on it on the device."""
        from .mcts import rollout_args, steering_args
        rollout_args(rollout, rollout_dev)
        steering_args(source, rollout, track, False)
        states = np.asarray(states, dtype=np.float64).reshape(-1, 11)
        R = states.shape[0]
        seeds = np.arange(R, dtype=np.uint64) if seeds is None else np.asarray(seeds, np.uint64)
        handle = self._mcts_source(source, policy)
        return self.car.drive_mcts(self.scan_simulator.scan_method, handle, states, n_decisions, n_iterations, seeds,
                                   self.scan_fov, self.num_rays, self.edge_distances, self.ttc_thresh,
                                   recent_actions=recent_actions, source=source, steps_per_decision=steps_per_decision,
                                   steer_clip=steer_clip, rollout_steps=self.batch_size,
                                   scan_dist_to_base=self.scan_dist_to_base, track=track, track_reward=track_reward,
                                   lookahead=lookahead, track_window=track_window, goal_span=goal_span, rollout=rollout,
                                  rollout_dev=rollout_dev)

    def particleFilter(self, n_particles, angles=None, motion_std=(0.05, 0.05, 0.02), resample_ratio=0.5,
                       sensor_model=None):
        """A ``ParticleFilter`` on this simulator's range method: ``n_particles`` particles casting ``angles`` (default:
        every 20th beam of this simulator's fan, the sparse scan mit-racecar's particle_filter.py localises with).
        ``sensor_model``: a (W, W) table for ``set_sensor_model`` (None: the method's table as already set).  Run it with
        ``reset(particles)`` and ``run(odom, obs)``; nothing leaves the GPU between the steps of a run."""
        from .particle_filter import ParticleFilter
        if angles is None:
            j = np.arange(0, self.num_rays, 20, dtype=np.float32)
            angles = (np.float32(-0.5 * self.scan_fov) + j * np.float32(self.scan_fov / self.num_rays)).astype(np.float32)
        method = self.scan_simulator.scan_method
        if sensor_model is not None:
            method.set_sensor_model(sensor_model)
        return ParticleFilter(method, angles, n_particles, motion_std=motion_std, resample_ratio=resample_ratio)

    def driveEnv(self, n_envs, starts, **kw):
        """A ``DriveEnv`` of ``n_envs`` cars on this simulator's range method, car, fan, edge table, ttc_thresh and
        scan_dist_to_base, spawning from ``starts`` float64 (M, 11): the tick of ``driveFollowGapMany`` with the (speed,
        steer) of every step supplied by the caller.  ``kw``: ``DriveEnv``'s keyword arguments (substeps, obs_window,
        obs_clip, obs_scale, max_ticks, auto_reset, steer_clip, crash_reward, dt, and the track keywords track,
        track_window, lookahead, goal_span, progress_reward)."""
        from .env import DriveEnv
        kw.setdefault("car", self.car)
        kw.setdefault("scan_dist_to_base", self.scan_dist_to_base)
        return DriveEnv(self.scan_simulator.scan_method, np.asarray(starts, dtype=np.float64).reshape(-1, 11), n_envs,
                        self.num_rays, self.scan_fov, self.edge_distances, self.ttc_thresh, **kw)

    def raceEnv(self, n_races, starts, **kw):
        """A ``RaceEnv`` of ``n_races`` races on this simulator's range method (RM, RMGPU or "CDDT" set with
        ``races=True``), car, fan, edge table, ttc_thresh and scan_dist_to_base, spawning from the line-ups ``starts``
        float64 (M, P, 11): the tick of ``raceFollowGapMany`` with the (speed, steer) of every car supplied by the caller.  ``kw``: ``RaceEnv``'s keyword
        arguments (min_running and ``DriveEnv``'s, the track keywords included; ``seats`` and ``seat_speed`` put a
        driver into a seat, "fg" standing for this simulator's own FollowGap driver; ``league=(pop, entries)`` gives
        every car its own driver, -1 entries going to ``followgap`` or, without one, to the simulator's own)."""
        from .env import RaceEnv
        if kw.get("league") is not None and kw.get("followgap") is None and (np.asarray(kw["league"][1]) == -1).any():
            kw["followgap"] = self._mcts_source("fg", None)
        if kw.get("seats") is not None:
            kw["seats"] = [self._mcts_source("fg", None) if isinstance(d, str) and d == "fg" else d for d in kw["seats"]]
        kw.setdefault("car", self.car)
        kw.setdefault("scan_dist_to_base", self.scan_dist_to_base)
        return RaceEnv(self.scan_simulator.scan_method, starts, n_races, self.num_rays, self.scan_fov,
                       self.edge_distances, self.ttc_thresh, **kw)

    def stop(self):
        state = self.getState()
        state[:11] = 0.0
        self.setState(state)
        self.desired_speed = 0.0
        self.desired_steer_ang = 0.0

    # -- map / method -----------------------------------------------------------------
    def setMap(self, ros_map, resolution, origin):
        max_range_px = int(self.scan_max_range / resolution)        # :196
        self.scan_simulator.setMap(ros_map, max_range_px, resolution, origin)

    def setRaytracingMethod(self, method="RMGPU", **kw):
        # (theta_disc=, lut_refine= for "GLT"; theta_disc=, races= for "CDDT")
        self.scan_simulator.setRaytracingMethod(method, **kw)
