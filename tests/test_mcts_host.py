"""The MCTS statement (tests/mcts_statement.py) on a fake simulator, against hand-worked trees of scripts/mcts.py's
mctsIteration, and the two exactness definitions of include/scanlib.h that need no GPU: the reward sum in NumPy's
pairwise order and the Philox uniform draws."""
import math

import numpy as np
import pytest

import mcts_statement as S
from oracle.np_statement import noise_key, philox2x32_10


def _tree(source="fg", answer=0.2, seed=5):
    return S.Tree(np.zeros(11), np.zeros(3, np.float32), answer, 0.1, seed, source=source)


def _drive(tree, n, terminal_of=lambda k, node, a: False, rollout_of=lambda k, child: (-1, np.ones(4))):
    """n iterations of one tree on a fake simulator: the act keeps the state, terminal_of decides the crash,
    rollout_of gives (crash index, velocities)."""
    def act(i, reqs):
        return [(node.state, node.pose, 0.3, terminal_of(i, node, a)) for _, node, a in reqs]

    def ro(i, reqs, acts):
        return [rollout_of(i, child) for _, child in reqs]
    return S.run_lockstep([tree], n, act, ro, snapshots=(n,))[n][0]


def test_first_iterations_by_hand():
    """Iteration 0 expands the root with the FG answer; iteration 1 widens children[0].action (sqrt(1) < 1 is false:
    no descent); iteration 2 descends (sqrt(2) < 2) into the better child and expands it."""
    t = _tree()
    vel = np.array([1.0, 2.0, 3.0, 4.0])
    arr = _drive(t, 1, rollout_of=lambda i, c: (-1, vel))
    assert arr["parent"].tolist() == [-1, 0]
    assert arr["action"][1] == 0.2                                  # the root's stored answer, widened to double
    rv0 = 10.0 / 0.2
    assert arr["reward"].tolist() == [0.0, rv0] and arr["visits"].tolist() == [2, 1]
    t = _tree()
    arr = _drive(t, 2, rollout_of=lambda i, c: (2 if i == 1 else -1, vel))
    u = S.uniform01(5, 0, 1)
    assert arr["action"][2] == S.uniform(0.2 - 0.05, 0.2 + 0.05, u)
    assert arr["crash"].tolist() == [-1, -1, 2]
    assert arr["reward"][2] == 3.0 / abs(arr["action"][2])          # vel[:2]
    assert arr["visits"].tolist() == [3, 1, 1] and arr["child_visits"][0] == 2
    assert arr["next_sibling"].tolist() == [-1, 2, -1] and arr["first_child"][0] == 1
    # iteration 2: sum 2, sqrt(2) < 2: descend into the max of reward/1 + 0.5 sqrt(log 2 / 1); child 1 (50) wins
    t = _tree()
    arr = _drive(t, 3, rollout_of=lambda i, c: (2 if i == 1 else -1, vel))
    assert arr["parent"].tolist() == [-1, 0, 0, 1]
    assert arr["visits"].tolist() == [4, 2, 1, 1]
    rv2 = 10.0 / abs(arr["action"][3])
    # propagate multiplicities: the new child once, the node it was added under twice (two recursion levels)
    assert arr["reward"][3] == rv2
    assert arr["reward"][1] == (rv0 + rv2) + rv2


def test_propagate_multiplicities_deep_chain():
    """A chain forced by one child per level: at depth D the j-th ancestor of the new child gets rv j + 1 times."""
    t = _tree(source="fg")

    def ro(i, child):
        return -1, np.full(3, 1.0)
    arr = _drive(t, 6, rollout_of=ro)
    # rebuild the expected rewards with a direct walk of the statement's own recursion counts
    n = len(arr["parent"])
    want = np.zeros(n)
    for c in range(1, n):
        rv = 3.0 / abs(arr["action"][c])
        want[c] += rv
        node, j = arr["parent"][c], 1
        while node > 0:
            for _ in range(j + 1):
                want[node] += rv
            node, j = arr["parent"][node], j + 1
    # the order of the adds per node is the order of creation here (one per iteration): same bits
    assert arr["reward"].tobytes() == want.tobytes()


def test_terminal_child_gets_expanded():
    """The root's only child is terminal; the next iteration descends into it (sqrt(1) < 1 is false, so the root
    expands again first: child 2); with both terminal and sqrt(2) < 2 the search descends into the UCB maximum,
    which returns "not expanded": the terminal node gets a child and is not visited."""
    t = _tree(source="random")
    arr = _drive(t, 3, terminal_of=lambda i, node, a: i < 2)
    assert arr["terminal"].tolist() == [0, 1, 1, 0]
    assert arr["reward"][2] == -10.0
    # both terminal children have reward -10 and visits 1: equal keys, the first wins (Python max)
    assert arr["parent"][3] == 1
    assert arr["visits"].tolist() == [4, 1, 1, 1]                   # the terminal node 1 was not visited
    rv = 4.0 / abs(arr["action"][3])
    assert arr["reward"][3] == rv
    assert arr["reward"][1] == -10.0 + rv                           # j = 1 under a terminal node: once
    assert arr["child_visits"][0] == 2 and arr["child_visits"][1] == 1


def test_first_maximum_wins_ties():
    """Two root children with equal UCB keys: the search descends into the first (Python's max)."""
    t = _tree(source="random")
    t.root.children = []
    a = S.Node(np.zeros(11), np.zeros(3, np.float32), 0.0, 0.3, parent=t.root)
    b = S.Node(np.zeros(11), np.zeros(3, np.float32), 0.0, -0.3, parent=t.root)
    a.index, b.index = 1, 2
    a.reward = b.reward = 5.0
    t.root.children = [a, b]
    t.nodes += [a, b]
    arr = _drive(t, 1)
    assert arr["parent"][3] == 1                                    # descended into the first of the equals
    assert arr["visits"].tolist() == [2, 2, 1, 1]


def test_inf_and_nan_rewards_propagate():
    """A zero action gives sum / 0: inf (or NaN for a zero sum); both propagate by IEEE rules."""
    t = S.Tree(np.zeros(11), np.zeros(3, np.float32), 0.0, 0.1, 1, source="fg")
    arr = _drive(t, 1, rollout_of=lambda i, c: (-1, np.ones(3)))
    assert arr["action"][1] == 0.0 and math.isinf(arr["reward"][1]) and arr["reward"][1] > 0
    t = S.Tree(np.zeros(11), np.zeros(3, np.float32), 0.0, 0.1, 1, source="fg")
    arr = _drive(t, 1, rollout_of=lambda i, c: (0, np.ones(3)))
    assert math.isnan(arr["reward"][1])
    assert S.reward_of(-1, np.array([-1.0]), 0.0) == -math.inf


def _adversarial(n, rng):
    """Vectors whose sum depends on the summation order: huge values that cancel, mixed with small ones."""
    out = []
    big = 2.0 ** 60
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-10, 10, n)
    out.append(v)
    w = rng.standard_normal(n)
    if n:
        idx = rng.permutation(n)
        w[idx[: n // 3]] = big * rng.choice([-1, 1], len(idx[: n // 3]))
    out.append(w)
    out.append(np.where(rng.uniform(size=n) < 0.5, 1.0, 2.0 ** -53) * rng.choice([-1, 1], n))
    z = np.full(n, -0.0)
    out.append(z)
    return out


def test_pairwise_sum_equals_numpy_bitwise():
    rng = np.random.default_rng(3)
    for n in range(0, 201):
        for v in _adversarial(n, rng):
            v = np.ascontiguousarray(v, np.float64)
            assert np.float64(S.pairwise_sum(v)).tobytes() == np.sum(v).tobytes(), n
    # and the orders differ: a sequential sum disagrees on some of these
    differs = 0
    for n in (9, 17, 64, 129, 200):
        for v in _adversarial(n, rng):
            seq = 0.0
            for x in v:
                seq += float(x)
            differs += np.float64(seq).tobytes() != np.sum(v).tobytes()
    assert differs > 0
    # up to the planner's roll-out cap of 512 steps
    for n in range(201, 513, 7):
        v = _adversarial(n, rng)[1]
        assert np.float64(S.pairwise_sum(v)).tobytes() == np.sum(v).tobytes(), n
    # special values
    for v in ([np.inf, -np.inf] * 5, [np.nan] + [1.0] * 20, [1e308] * 10):
        v = np.array(v)
        with np.errstate(over="ignore", invalid="ignore"):
            a, b = S.pairwise_sum(v), np.sum(v)
        assert (math.isnan(a) and math.isnan(b)) or np.float64(a).tobytes() == b.tobytes()


def test_philox_uniform_draws_known_answers():
    # Random123's known-answer vectors of Philox-2x32-10
    for (c0, c1, k), want in [((0, 0, 0), (0xff1dae59, 0x6cd10df2)),
                              ((0xffffffff, 0xffffffff, 0xffffffff), (0x2c3f628b, 0xab4fd7ad)),
                              ((0x243f6a88, 0x85a308d3, 0x13198a2e), (0xdd7ce038, 0xf62a4c12))]:
        a, b = philox2x32_10(np.array([c0], np.uint64), np.array([c1], np.uint64), k)
        assert (int(a[0]), int(b[0])) == want
    # the draw of seed 0 at counter (0, 0): key noise_key(0) = 0, the words above
    u = S.uniform01(0, 0, 0)
    assert u == ((0xff1dae59 << 32 | 0x6cd10df2) >> 11) * 2.0 ** -53
    assert noise_key(1 << 32) == 0x85EBCA6B
    # draws lie in [0, 1) and use all 53 bits
    us = S.uniform01(7, np.arange(4096, dtype=np.uint64), np.full(4096, 3, np.uint64))
    assert (us >= 0).all() and (us < 1).all() and len(np.unique(us)) == 4096
    assert ((us * 2.0 ** 53) % 1 == 0).all()
    # uniform(lo, hi): NumPy's formula, two rounded operations
    assert S.uniform(-0.4189, 0.4189, 0.5) == -0.4189 + (0.4189 - -0.4189) * 0.5
    acts = S.rollout_actions(7, 3, 20, 0.4189, 7.0)
    assert acts.shape == (20, 2) and (np.abs(acts[:, 1]) <= 0.4189).all() and (acts[:, 0] >= 0).all()
    assert acts[4, 1] == S.uniform(-0.4189, 0.4189, S.uniform01(7, 9, 3))


@pytest.mark.parametrize("source", ["fg", "nn", "random"])
def test_one_node_per_iteration(source):
    rng = np.random.default_rng(1)
    t = S.Tree(np.zeros(11), np.zeros(3, np.float32), 0.05, 0.1, 11, source=source)
    arr = _drive(t, 40, terminal_of=lambda i, node, a: rng.uniform() < 0.3,
                 rollout_of=lambda i, c: (int(rng.integers(-201, 200)) if rng.uniform() < 0.5 else -201,
                                          rng.uniform(0, 7, 200)))
    assert len(arr["parent"]) == 41
    assert (arr["n_children"].sum() == 40) and (arr["child_visits"] >= arr["n_children"]).all()
