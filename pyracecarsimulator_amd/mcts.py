"""The MCTS planner on the GPU (``rl_mcts_*``, include/scanlib.h; kernels csrc/mcts_kernels.h).

``MCTSPlanner`` advances K independent trees of scripts/mcts.py's search in lock step: one node per tree per
iteration, each iteration one batched act (step, scan, crash test, expansion answer) and one batched roll-out,
nothing leaving the device between iterations.  The trees are the reference's bit for bit (tests/mcts_statement.py).

``MCTSPlanner.drive`` closes the loop of scripts/mcts_driver.py:207-264 for the K cars (``rl_mcts_drive``): at every
decision a fresh tree from the car's state, the search, the most visited root action, the car's steps with it — all
decisions enqueued at once, nothing leaving the device in between.

``MCTSPlanner.attach_track`` gives the planner a ``Track`` (include/scanlib_track_plan.h; kernels
csrc/plan_track_kernels.h): every roll-out step's reward term becomes the reference's waypoint reward (mcts.py:233-234)
or the track progress of the step, for ``run`` and for ``drive`` alike, with nothing new crossing to the host.  The track
can also steer the search (kernels csrc/plan_pursuit_kernels.h): ``source="track"`` expands every node with the pure
pursuit of the tree's track point, ``rollout="pursuit"`` steers every roll-out along the track's goal waypoints.

``MCTS`` is a drop-in for the reference class (scripts/mcts.py:83-148) on a ``RacecarSimulator``: ``mcts()`` plans
from the simulator's state and returns the most visited root action; ``root`` holds the tree read back from the
device as ``Node`` objects.
"""
from __future__ import annotations

import ctypes as C
import time

import numpy as np

from . import _lib

SOURCES = {"fg": _lib.RL_MCTS_FG, "nn": _lib.RL_MCTS_NN, "random": _lib.RL_MCTS_RANDOM, "track": _lib.RL_MCTS_PURSUIT}
#: who steers a roll-out (rl_mcts_params.rollout_source)
ROLLOUTS = {"random": 0, "pursuit": 1}
#: the reward term of a roll-out step (rl_plan_track_params.reward_mode)
REWARDS = {"velocity": 0, "waypoint": 1, "progress": 2}
MAX_TRACK_POINTS = 65536
TREE_FIELDS = ("parent", "first_child", "next_sibling", "n_children", "visits", "child_visits", "reward", "action",
               "terminal", "state", "scan_pose", "answer", "crash")


# ---------------------------------------------------------------- the decision loop's host-side definitions
def drive_seeds(seeds, d):
    """The seeds of decision ``d``: (seeds + d) mod 2^64 (the tree's Philox key is ``noise_key`` of it)."""
    s = np.asarray(seeds, np.uint64)
    return (np.atleast_1d(s) + np.uint64(int(d) % (1 << 64))).reshape(s.shape)      # (uint64 array addition wraps)


def drive_stride(n_trees, num_rays, n_iterations, rollout_steps):
    """Rays one decision consumes, K B (1 + I (1 + L)): the root scans, then per iteration the act scans and the
    roll-out scans of every tree.  Decision d's ray offset is the handle's offset at entry + d * stride."""
    return int(n_trees) * int(num_rays) * (1 + int(n_iterations) * (1 + int(rollout_steps)))


def drive_recent(action, steer_clip):
    """The recent action after a decision (mcts_driver.py:254): the raw best action clamped to +-steer_clip, or
    the raw action when steer_clip is None.  The car itself is driven with the raw action (:249)."""
    a = np.asarray(action, np.float64)
    return a.copy() if steer_clip is None else np.clip(a, -float(steer_clip), float(steer_clip))


def drive_dead_rows(first, n_decisions):
    """Which (car, decision) rows of ``drive``'s outputs a crash blanks, bool (K, D): a car with crash decision
    ``first`` >= 0 has actions NaN, visits -1 and trace rows NaN from that decision on; ``first`` = -(D+1): never."""
    first = np.asarray(first)
    return (first[:, None] >= 0) & (np.arange(int(n_decisions))[None, :] >= first[:, None])


def drive_args(n_trees, states, recent_actions, seeds, n_decisions, n_iterations, steps_per_decision, steer_clip):
    """``MCTSPlanner.drive``'s arguments checked and laid out for ``rl_mcts_drive`` (no library call): states float64
    (K, 11), recent actions scalar or (K,), seeds integers >= 0 scalar or (K,); returns (states, recent, seeds, D, I,
    S, clip) with clip = 0.0 for ``steer_clip=None``."""
    K = int(n_trees)
    st = np.asarray(states)
    if st.dtype != np.float64 or st.shape != (K, 11):
        raise ValueError("states must be float64 (%d, 11)" % K)
    ac = np.asarray(recent_actions)
    if ac.dtype.kind not in "fiu" or ac.shape not in ((), (K,)):
        raise ValueError("recent_actions must be a real scalar or (%d,)" % K)
    sd = np.asarray(seeds)
    if sd.dtype.kind not in "iu" or sd.shape not in ((), (K,)):
        raise ValueError("seeds must be an integer scalar or (%d,)" % K)
    if sd.dtype.kind == "i" and (sd < 0).any():
        raise ValueError("seeds must be >= 0")
    D, I, S = int(n_decisions), int(n_iterations), int(steps_per_decision)
    if (D, I, S) != (n_decisions, n_iterations, steps_per_decision):
        raise ValueError("n_decisions, n_iterations and steps_per_decision must be integers")
    if D < 0 or I < 1 or S < 1:
        raise ValueError("n_decisions >= 0, n_iterations >= 1 and steps_per_decision >= 1 required")
    clip = 0.0 if steer_clip is None else float(steer_clip)
    if steer_clip is not None and not clip > 0:
        raise ValueError("steer_clip must be None or > 0")
    return (np.ascontiguousarray(st), np.ascontiguousarray(np.broadcast_to(ac.astype(np.float64), (K,))),
            np.ascontiguousarray(np.broadcast_to(sd.astype(np.uint64), (K,))), D, I, S, clip)


def plan_track_args(reward="progress", lookahead=1.5, window=0, goal_span=0, points=False):
    """The track keywords of the planner and of ``CarBatch.rollout_track`` checked and laid out as
    ``rl_plan_track_params`` (no library call).  ``points``: explicit points stand in for the goal rule, so the
    lookahead is not read."""
    if reward not in REWARDS:
        raise ValueError("reward must be one of %s" % sorted(REWARDS))
    for name, v in (("window", window), ("goal_span", goal_span)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("%s must be an integer" % name)
        if not 0 <= int(v) <= MAX_TRACK_POINTS:
            raise ValueError("%s must lie in [0, %d]" % (name, MAX_TRACK_POINTS))
    la = float(lookahead)
    if reward == "waypoint" and not points and (not np.isfinite(la) or la <= 0):
        raise ValueError("lookahead must be finite and > 0")
    p = _lib.PlanTrackParams()
    p.reward_mode, p.window, p.goal_span, p.lookahead = REWARDS[reward], int(window), int(goal_span), la
    return p


def rollout_args(rollout="random", rollout_dev=0.1):
    """The roll-out keywords of the planner checked (no library call): (rollout_source, rollout_dev)."""
    if rollout not in ROLLOUTS:
        raise ValueError("rollout must be one of %s" % sorted(ROLLOUTS))
    dev = float(rollout_dev)
    if not np.isfinite(dev) or dev < 0:
        raise ValueError("rollout_dev must be finite and >= 0")
    return ROLLOUTS[rollout], dev


def steering_args(source, rollout, track, points):
    """What a planner steered by the track needs before it searches (no library call): ``source="track"`` a track or
    explicit points, ``rollout="pursuit"`` a track (a roll-out travels metres: one point does not help it)."""
    if source == "track" and track is None and not points:
        raise ValueError("source 'track' needs a track or a track point")
    if rollout == "pursuit" and track is None:
        raise ValueError("rollout 'pursuit' needs a track")


def points_args(xy, n):
    """Explicit track points checked and laid out (no library call): float64 (n, 2), or one point for all."""
    p = np.asarray(xy, np.float64)
    if p.shape == (2,):
        p = np.broadcast_to(p, (int(n), 2))
    if p.shape != (int(n), 2):
        raise ValueError("points must be (2,) or (%d, 2)" % int(n))
    return np.ascontiguousarray(p)


class MCTSPlanner(_lib.Handle):
    """K trees of at most ``max_nodes`` nodes on one device.  ``method`` scans, ``source`` ("fg", "nn", "random" or
    "track") picks the expansion answer: ``followgap`` (a ``PyFollowGap``) for "fg", ``policy`` (a ``Policy``) for "nn",
    the pure pursuit of the tree's track point for "track" (``attach_track`` or ``set_points`` before the reset).
    ``rollout``: "random" (the reference's uniform steer) or "pursuit" (every roll-out action steers for the attached
    track's goal waypoint, plus a uniform deviation of +-``rollout_dev`` rad).  The handles are borrowed: keep them
    alive as long as the planner."""
    _destroy = "rl_mcts_destroy"
    _track, _points = None, False       # (the attached Track, kept alive here; are explicit points set)
    _velocity_points = False            # (explicit points alone run the velocity reward, not the waypoint reward)
    source, rollout = "fg", "random"

    def __init__(self, car, method, n_trees, max_nodes, fov, num_rays, edge, crash_thresh, source="fg",
                 followgap=None, policy=None, rollout_steps=200, action_every=10, speed=2.0, dt=0.01,
                 scan_dist_to_base=0.275, C_ucb=0.5, crash_pen=-10.0, uni_dev=0.05, max_steer=None, max_speed=None,
                 rollout="random", rollout_dev=0.1):
        if source not in SOURCES:
            raise ValueError("source must be one of %s" % sorted(SOURCES))
        rollout_source, rollout_dev = rollout_args(rollout, rollout_dev)
        edge = np.asarray(edge)
        if edge.dtype != np.float64 or edge.shape != (int(num_rays),):
            raise ValueError("edge must be float64 (num_rays,)")
        self._edge = np.ascontiguousarray(edge)
        p = _lib.MctsParams()
        p.n_trees, p.max_nodes, p.rollout_steps = int(n_trees), int(max_nodes), int(rollout_steps)
        p.action_every, p.source = int(action_every), SOURCES[source]
        p.speed, p.dt, p.scan_dist_to_base, p.C = float(speed), float(dt), float(scan_dist_to_base), float(C_ucb)
        p.crash_pen, p.uni_dev = float(crash_pen), float(uni_dev)
        p.max_steer = float(car.params["max_steer_ang"] if max_steer is None else max_steer)
        p.max_speed = float(car.params["max_speed"] if max_speed is None else max_speed)
        p.fov, p.num_rays, p.crash_thresh = float(fov), int(num_rays), float(crash_thresh)
        p.rollout_source, p.rollout_dev = rollout_source, rollout_dev
        self.params = p
        self.n_trees, self.max_nodes, self.source, self.rollout = int(n_trees), int(max_nodes), source, rollout
        self._keep = (car, method, followgap, policy)
        self._h = C.c_void_p()
        _lib.call("rl_mcts_create", car, method, followgap, policy, p, self._edge, self._h)

    def attach_track(self, track, reward="progress", lookahead=1.5, window=0, goal_span=0):
        """Give the planner ``track`` (a ``Track``, borrowed: kept alive here while attached).  ``reward``: "progress"
        (per step the arc length gained, searched within ``window`` segments of the root's nearest segment; 0: all),
        "waypoint" (velocity over the distance to the tree's track point: the waypoint ``lookahead`` away from the
        root, findBestPoint's rule, looking ``goal_span`` waypoints ahead; 0: all) or "velocity" (today's reward).
        Takes effect at the next ``reset`` or ``drive``.  A planner with ``source="track"`` (without explicit points) or
        ``rollout="pursuit"`` reads ``lookahead``, ``goal_span`` and ``window`` for its steering whatever the reward."""
        p = plan_track_args(reward, lookahead, window, goal_span, points=self._points)
        if track is None:
            raise ValueError("track must be a Track (detach_track() removes it)")
        steers = (self.source == "track" and not self._points) or self.rollout == "pursuit"
        if steers and (not np.isfinite(p.lookahead) or p.lookahead <= 0):
            raise ValueError("lookahead must be finite and > 0")
        _lib.call("rl_mcts_attach_track", self, track, p)
        self._track = track

    def detach_track(self):
        _lib.call("rl_mcts_attach_track", self, None, None)
        self._track, self._velocity_points = None, False

    def set_points(self, xy, reward="waypoint"):
        """One explicit track point per tree, float64 (K, 2) or (2,) for all (None removes them): the waypoint reward's
        point, as the reference's constructor takes it, and what ``source="track"`` pursues.  Without a track the planner
        then runs the waypoint reward, or with ``reward="velocity"`` (no track attached) the velocity reward."""
        if reward not in ("waypoint", "velocity"):
            raise ValueError("reward of explicit points must be 'waypoint' or 'velocity'")
        p = None if xy is None else points_args(xy, self.n_trees)
        _lib.call("rl_mcts_set_points", self, p)
        self._points = p is not None
        velocity = p is not None and reward == "velocity"
        if self._track is None and velocity != self._velocity_points:
            _lib.call("rl_mcts_attach_track", self, None, plan_track_args("velocity", points=True) if velocity else None)
            self._velocity_points = velocity

    def read_track(self):
        """The current roots on the track, a dict: segment int32 (K,), s float64 (K,), goal int32 (K,) (-1: none), point
        float64 (K, 2).  After ``drive``: those of the last decision."""
        K = self.n_trees
        out = dict(segment=np.empty(K, np.int32), s=np.empty(K), goal=np.empty(K, np.int32), point=np.empty((K, 2)))
        _lib.call("rl_mcts_read_track", self, out["segment"], out["s"], out["goal"], out["point"])
        return out

    def reset(self, root_states, root_actions, seeds):
        """The K roots: states float64 (K, 11) in getState layout, recent actions (K,), one 64-bit seed per tree."""
        K = self.n_trees
        st = np.ascontiguousarray(np.asarray(root_states, np.float64).reshape(K, 11))
        ac = np.ascontiguousarray(np.broadcast_to(np.asarray(root_actions, np.float64), (K,)))
        sd = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, np.uint64), (K,)))
        steering_args(self.source, self.rollout, self._track, self._points)
        _lib.call("rl_mcts_reset", self, st, ac, sd)

    def run(self, n_iterations):
        steering_args(self.source, self.rollout, self._track, self._points)
        _lib.call("rl_mcts_run", self, n_iterations)

    def best(self):
        """(best root action float64 (K,), its visits int32 (K,), nodes per tree int32 (K,))."""
        K = self.n_trees
        a, v, n = np.empty(K), np.empty(K, np.int32), np.empty(K, np.int32)
        _lib.call("rl_mcts_best", self, a, v, n)
        return a, v, n

    def read_tree(self, tree):
        """Tree ``tree``'s node arrays in creation order, a dict keyed by TREE_FIELDS (state (n, 11), scan_pose (n, 3))."""
        N = self.max_nodes
        out = {f: np.empty(N, np.int32) for f in ("parent", "first_child", "next_sibling", "n_children", "visits",
                                                  "child_visits", "terminal", "crash")}
        out.update(reward=np.empty(N), action=np.empty(N), state=np.empty((N, 11)),
                   scan_pose=np.empty((N, 3), np.float32), answer=np.empty(N, np.float32))
        n = C.c_int(0)
        _lib.call("rl_mcts_read_tree", self, tree, *(out[f] for f in TREE_FIELDS), n)
        return {f: a[:n.value] for f, a in out.items()}

    def drive(self, states, recent_actions, seeds, n_decisions, n_iterations, steps_per_decision=1, steer_clip=None,
              trace=False):
        """The closed loop of scripts/mcts_driver.py:207-264 for the K cars (``rl_mcts_drive``): ``n_decisions``
        times a fresh tree from the car's state with its recent action at the root and seed ``seeds + d``,
        ``n_iterations`` iterations, the most visited root action, ``steps_per_decision`` car steps at the planner's
        speed with it; the next recent action is that action clamped to +-``steer_clip`` (None: raw).  A car whose
        root scan crashes at decision d freezes there.  Returns (first crash decision or -(D+1) int32 (K,), final
        states (K, 11), recent actions (K,), best actions float64 (K, D) — NaN from the crash on —, their visits
        int32 (K, D) — -1 from the crash on) and with ``trace=True`` also the states every decision was planned
        from, (K, D, 11).  The planner keeps the last decision's trees (``read_tree``, ``best``)."""
        K = self.n_trees
        if self._points:
            raise ValueError("a planner with explicit points cannot drive: attach a track instead")
        steering_args(self.source, self.rollout, self._track, self._points)
        st, ac, sd, D, I, S, clip = drive_args(K, states, recent_actions, seeds, n_decisions, n_iterations,
                                               steps_per_decision, steer_clip)
        first, out, recent = np.empty(K, np.int32), np.empty((K, 11)), np.empty(K)
        actions, visits = np.empty((K, D)), np.empty((K, D), np.int32)
        tr = np.empty((K, D, 11)) if trace else None
        _lib.call("rl_mcts_drive", self, st, ac, sd, D, I, S, clip, first, out, recent, actions, visits, tr)
        return (first, out, recent, actions, visits) + ((tr,) if trace else ())


class Node:
    """A node of a tree read back from the device, with the reference Node's fields (scripts/mcts.py:16-31)."""

    def __init__(self, state, action, terminal, parent, visits, reward, scan_pose, answer, index):
        self.state, self.action, self.terminal, self.parent = state, action, terminal, parent
        self.visits, self.reward, self.scan_pose, self.answer, self.index = visits, reward, scan_pose, answer, index
        self.children = []

    def isTerminal(self):
        return self.terminal

    def hasChildren(self):
        return len(self.children) > 0

    def size(self):
        return len(self.children)

    def getState(self):
        return self.state


def build_nodes(arrays):
    """The Node tree of one ``read_tree`` dict (children in insertion order); returns the root."""
    n = len(arrays["parent"])
    nodes = []
    for i in range(n):
        par = int(arrays["parent"][i])
        node = Node(arrays["state"][i].copy(), float(arrays["action"][i]), bool(arrays["terminal"][i]),
                    nodes[par] if par >= 0 else None, int(arrays["visits"][i]), float(arrays["reward"][i]),
                    arrays["scan_pose"][i].copy(), float(arrays["answer"][i]), i)
        nodes.append(node)
        if par >= 0:
            nodes[par].children.append(node)      # nodes are created in order: siblings append in insertion order
    return nodes[0] if nodes else None


class MCTS:
    """Drop-in for scripts/mcts.py's MCTS on a ``RacecarSimulator``: ``mcts()`` searches from the simulator's state
    with ``recent_action`` at the root and returns (and keeps in ``self.action``) the most visited root child's
    action; ``root`` is the searched tree (``Node`` objects read back from the device).

    ``budget`` seconds of wall clock run chunks of iterations until the time is spent or ``max_nodes`` is reached,
    at least one iteration; ``n_iterations`` runs exactly that many instead (deterministic).  ``seed`` keys the
    draws.  ``source``: "fg" (the reference's live generateActionFromFG, PyFollowGap(10, 15.0, max_steer, 0.004)),
    "nn" (``policy_session``, a ``Policy``), "random" or "track" (the pure pursuit of ``track_point``, or of the goal
    waypoint of ``track``, whether or not ``with_global`` asks for the waypoint reward).  ``track`` (a ``Track``) is
    attached with the velocity reward (the waypoint reward with ``with_global=True``) and ``lookahead``, ``track_window``
    and ``goal_span``; ``rollout="pursuit"`` needs it (``rollout_dev`` as ``MCTSPlanner``).  ``with_global=True`` with a ``track_point`` (x, y) is the
    reference's global-planner call (mcts_driver.py:224-227): every roll-out step is rewarded with its velocity over the
    distance to that point (mcts.py:233-234, 247-250, commented out upstream).  ``with_global=False``, the default,
    is the velocity reward, whatever ``track_point`` holds."""

    def __init__(self, simulator, policy_session, recent_action, roll_out_itr, budget=1.0, track_point=None,
                 with_global=False, *, seed=0, n_iterations=None, source="fg", max_nodes=4097, track=None, rollout="random",
                 rollout_dev=0.1, lookahead=1.5, track_window=0, goal_span=0):
        if with_global and track_point is None and track is None:
            raise ValueError("with_global=True needs a track_point")
        if source not in SOURCES:
            raise ValueError("source must be one of %s" % sorted(SOURCES))
        rollout_args(rollout, rollout_dev)
        steering_args(source, rollout, track, track_point is not None)
        self.track, self.rollout, self.rollout_dev = track, rollout, rollout_dev
        self.track_args = (lookahead, track_window, goal_span)
        self.point_to_follow = track_point
        self.with_global = with_global
        self.simulator = simulator
        self.policy_session = policy_session
        self.budget = budget
        self.max_iterations = int(roll_out_itr)
        self.action = recent_action
        self.root = None
        self.C = 0.5
        self.crash_pen = -10.0
        self.speed = 2.0
        self.seed = seed
        self.n_iterations = n_iterations
        self.source = source
        self.max_nodes = int(max_nodes if n_iterations is None else max(max_nodes, int(n_iterations) + 1))
        self.iterations = 0
        self.fg = None
        if source == "fg":
            from .followgap import PyFollowGap
            self.fg = PyFollowGap(10, 15.0, simulator.config["max_steer_ang"], 0.004, device=simulator._device)
        self._planner = None

    def _make_planner(self):
        sim = self.simulator
        return MCTSPlanner(sim.car, sim.scan_simulator.scan_method, 1, self.max_nodes, sim.scan_fov, sim.num_rays,
                           sim.edge_distances, sim.ttc_thresh, source=self.source, followgap=self.fg,
                           policy=self.policy_session if self.source == "nn" else None,
                           rollout_steps=self.max_iterations, speed=self.speed, C_ucb=self.C, crash_pen=self.crash_pen,
                           scan_dist_to_base=sim.scan_dist_to_base, max_steer=sim.config["max_steer_ang"],
                           max_speed=sim.config["max_speed"], rollout=self.rollout, rollout_dev=self.rollout_dev)

    def mcts(self):
        if self._planner is None:
            self._planner = self._make_planner()
            reward = "waypoint" if self.with_global else "velocity"
            if self.point_to_follow is not None and (self.with_global or self.source == "track"):
                self._planner.set_points(self.point_to_follow, reward=reward)
            if self.track is not None:
                self._planner.attach_track(self.track, reward, *self.track_args)
        pl = self._planner
        pl.reset(self.simulator.getState()[None, :], [self.action], [self.seed])
        cap = self.max_nodes - 1
        if self.n_iterations is not None:
            pl.run(int(self.n_iterations))
            done = int(self.n_iterations)
        else:
            t_start = time.time()
            pl.run(1)
            done = 1
            per_it = max(time.time() - t_start, 1e-6)
            while done < cap:
                left = t_start + self.budget - time.time()
                n = min(cap - done, int(0.5 * left / per_it))
                if n < 1:
                    break
                t0 = time.time()
                pl.run(n)
                done += n
                per_it = max((time.time() - t0) / n, 1e-6)
        self.iterations = done
        a, _, _ = pl.best()
        self.root = build_nodes(pl.read_tree(0))
        self.action = None if np.isnan(a[0]) else float(a[0])
        return self.action
