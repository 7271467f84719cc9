"""Host statement of scripts/mcts.py's search as the planner computes it (include/scanlib.h, rl_mcts_*), restated
literally from the reference (line numbers of scripts/mcts.py) with its draws and reward sum pinned.

The recursion of mctsIteration is kept as written; its two calls into the simulator (act, rollout) are yields, so
that a driver can advance many trees in lock step and answer each phase with one batched call:
  ("act", node, action)      -> (new_state, scan_pose, answer, terminal)
  ("rollout", node)          -> (crash index, velocities float64 (L,))
``run_lockstep`` is such a driver over plain callbacks; ``Tree.arrays`` gives a tree as the device's node arrays."""
import math

import numpy as np

from oracle.np_statement import noise_key, philox2x32_10

RANDOM_DEV = 0.41                                   # generateActionFromRandom (:259-260)


# ---------------------------------------------------------------- draws
def uniform01(seed, d, i):
    """Philox-2x32-10, key noise_key(seed), counter (d, i): ((out0 << 32 | out1) >> 11) 2^-53 (float64 array)."""
    c0, c1 = philox2x32_10(np.asarray(d, np.uint64), np.asarray(i, np.uint64), noise_key(seed))
    w = (c0 << np.uint64(32)) | c1
    return (w >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def uniform(lo, hi, u):
    """numpy's uniform(lo, hi) = lo + (hi - lo) u, each operation rounded."""
    return float(np.float64(lo) + (np.float64(hi) - np.float64(lo)) * np.float64(u))


def rollout_actions(seed, i, n_act, max_steer, max_speed):
    """(n_act, 2) (speed, steer) of iteration i's roll-out: steer (d = 1 + 2m) drawn before speed (d = 2 + 2m)."""
    m = np.arange(n_act, dtype=np.uint64)
    us = uniform01(seed, 1 + 2 * m, np.full(n_act, i, np.uint64))
    uv = uniform01(seed, 2 + 2 * m, np.full(n_act, i, np.uint64))
    out = np.empty((n_act, 2))
    for j in range(n_act):
        out[j, 1] = uniform(-max_steer, max_steer, us[j])
        out[j, 0] = uniform(0, max_speed, uv[j])
    return out


# ---------------------------------------------------------------- the reward sum
def pairwise_sum(v):
    """numpy.add.reduce of a contiguous float64 vector: 0.0 + P(v) with NumPy's pairwise_sum P."""
    v = [float(x) for x in v]

    def P(a, lo, n):
        if n < 8:
            res = 0.0
            for i in range(n):
                res += a[lo + i]
            return res
        if n <= 128:
            r = a[lo:lo + 8]
            i = 8
            while i < n - (n % 8):
                for j in range(8):
                    r[j] += a[lo + i + j]
                i += 8
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
            while i < n:
                res += a[lo + i]
                i += 1
            return res
        n2 = n // 2
        n2 -= n2 % 8
        return P(a, lo, n2) + P(a, lo + n2, n - n2)

    return 0.0 + P(v, 0, len(v))


def reward_of(index, vel, action):
    """rollout's value (:240-245): sum(vel[:index] or all) / abs(action), IEEE inf / NaN as NumPy gives them."""
    v = vel if index < 0 else vel[:index]
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(pairwise_sum(v)) / np.float64(abs(action)))


# ---------------------------------------------------------------- the tree
class Node:
    """scripts/mcts.py:16-81 (the fields the search reads); ``answer`` is the node's own expansion answer."""

    def __init__(self, state, pose, answer, action, terminal=False, parent=None):
        self.state = state
        self.pose = pose
        self.answer = answer
        self.parent = parent
        self.terminal = terminal
        self.action = action
        self.visits = 1
        self.reward = 0.0
        self.children = []
        self.crash = -1
        self.index = 0

    def isTerminal(self):
        return self.terminal

    def hasChildren(self):
        return len(self.children) > 0

    def size(self):
        return len(self.children)

    def visit(self):
        self.visits += 1

    @staticmethod
    def propagate(obj, reward):                      # :71-81
        if not obj.parent:
            return
        else:
            obj.reward += reward
            obj = obj.parent
            Node.propagate(obj, reward)


class Tree:
    """One tree of MCTS (:83-185) with the planner's draws; ``source`` "fg", "nn" or "random"."""

    def __init__(self, root_state, root_pose, root_answer, root_action, seed, source="fg", C=0.5, crash_pen=-10.0,
                 uni_dev=0.05):
        self.root = Node(root_state, root_pose, root_answer, root_action)
        self.nodes = [self.root]
        self.seed, self.source, self.C, self.crash_pen, self.uni_dev = seed, source, C, crash_pen, uni_dev
        self.i = 0

    def uniSample(self, prediction, dev):           # :269-270
        return uniform(prediction - dev, prediction + dev, uniform01(self.seed, 0, self.i))

    def generateAction(self, node):                  # :252-267
        if self.source == "random":
            return self.uniSample(0, RANDOM_DEV)
        if node.hasChildren():
            return self.uniSample(node.children[0].action, self.uni_dev)
        return float(node.answer)

    def iteration(self):
        """One mctsIteration from the root (a generator: yields the act and roll-out requests)."""
        yield from self.mctsIteration(self.root)
        self.i += 1

    def mctsIteration(self, node, expanded=False):   # :150-185
        if node.isTerminal():
            return 0, False
        node.visit()
        sum_of_visits = sum([x.visits for x in node.children])
        if node.hasChildren():
            action = max(node.children, key=lambda x: (x.reward / x.visits +
                                                      self.C * math.sqrt(math.log(sum_of_visits) / x.visits)))
        if math.sqrt(sum_of_visits) < node.size():
            node = action
            rv, expanded = yield from self.mctsIteration(node, expanded=False)
        if not expanded:
            new_action = self.generateAction(node)
            new_state, new_pose, answer, terminal = yield ("act", node, new_action)
            new_child = Node(new_state, new_pose, answer, new_action, terminal, parent=node)
            new_child.index = len(self.nodes)
            self.nodes.append(new_child)
            node.children.append(new_child)
            if not terminal:
                index, vel = yield ("rollout", new_child)
                new_child.crash = int(index)
                rv = reward_of(index, vel, new_child.action)
            else:
                rv = self.crash_pen
            node = new_child
        Node.propagate(node, rv)
        return rv, True

    def best(self):
        """MCTS.mcts's answer (:125-131): the first root child with the most visits (None, -1 without children)."""
        action, visits = None, -1
        for child in self.root.children:
            if child.visits > visits:
                action, visits = child.action, child.visits
        return action, visits

    def arrays(self):
        """The device's node arrays (rl_mcts_read_tree) of this tree."""
        n = len(self.nodes)
        out = {f: np.full(n, -1, np.int32) for f in ("parent", "first_child", "next_sibling", "crash")}
        for f in ("n_children", "visits", "child_visits", "terminal"):
            out[f] = np.zeros(n, np.int32)
        out.update(reward=np.zeros(n), action=np.zeros(n), state=np.zeros((n, 11)),
                   scan_pose=np.zeros((n, 3), np.float32), answer=np.zeros(n, np.float32))
        for nd in self.nodes:
            k = nd.index
            out["parent"][k] = nd.parent.index if nd.parent is not None else -1
            out["first_child"][k] = nd.children[0].index if nd.children else -1
            out["n_children"][k] = len(nd.children)
            for a, b in zip(nd.children, nd.children[1:]):
                out["next_sibling"][a.index] = b.index
            out["visits"][k] = nd.visits
            out["child_visits"][k] = sum(c.visits for c in nd.children)
            out["terminal"][k] = int(bool(nd.terminal))
            out["crash"][k] = nd.crash
            out["reward"][k] = nd.reward
            out["action"][k] = nd.action
            out["state"][k] = nd.state
            out["scan_pose"][k] = nd.pose
            out["answer"][k] = np.float32(nd.answer)
        return out


def run_lockstep(trees, n_iterations, act_many, rollout_many, snapshots=()):
    """Advance every tree n_iterations in lock step.  act_many(i, [(tree k, node, action)]) -> [(state, pose, answer,
    terminal)]; rollout_many(i, [(tree k, child)], acts) -> [(index, vel)] for the non-terminal children (acts: the
    act requests of the iteration, for drivers that roll every child out densely).  Returns {n: [arrays of each tree]}
    for the iteration counts in ``snapshots``."""
    snaps = {}
    for it in range(n_iterations):
        gens = [t.iteration() for t in trees]
        reqs = [next(g) for g in gens]
        assert all(r[0] == "act" for r in reqs)
        acts = [(k, r[1], r[2]) for k, r in enumerate(reqs)]
        results = act_many(it, acts)
        nxt = {}
        for k, g in enumerate(gens):
            try:
                nxt[k] = g.send(results[k])
            except StopIteration:
                pass
        ro = [(k, r[1]) for k, r in nxt.items()]
        if ro:
            answers = rollout_many(it, ro, acts)
            for (k, _), ans in zip(ro, answers):
                try:
                    gens[k].send(ans)
                    raise AssertionError("one roll-out per iteration")
                except StopIteration:
                    pass
        if it + 1 in snapshots:
            snaps[it + 1] = [t.arrays() for t in trees]
    return snaps
