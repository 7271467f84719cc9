"""The shapes tests/test_gpu_consumer_shapes.py runs the closed-loop kernels at (drive_tick_kernel<ROWS, *>,
mcts_act_kernel<ROWS>, the one-lane-per-tree planner kernels, the roll-out reward sum, the fused crash test), as plain
data and NumPy (the fixed values are tests/support.py's): no library call.  tests/test_consumer_shapes_host.py checks
with the references alone that these inputs do what the GPU tests take them to do."""
import math

import numpy as np

from support import D_BASE, FOV, THRESH  # noqa: F401  (the cases' fixed values, read as CS.FOV ...)

FG_ROWS = 20                                  # consumer_kernels.h: one instantiation per ROWS = 1 ... FG_ROWS
MIN_RAYS, MAX_RAYS = 10, 64 * FG_ROWS         # loop_args (every closed loop): num_rays in [10, 1280]
DRIVE_CARS = 8                                # drive_kernels.h: cars (waves) per workgroup of drive_tick_kernel


def rows_of(n):
    """ROWS = ceil(num_rays / 64): the instantiation a closed loop of n beams runs."""
    return (n + 63) // 64


# one size per row count: odd r one beam in the last row, even r a full last row.  (r = 1: the odd form is one beam,
# below MIN_RAYS; the edges 10, 11, 63 and 64 stand for that row.)
ROW_SIZES = {r: (64 * (r - 1) + 1 if r % 2 else 64 * r) for r in range(2, FG_ROWS + 1)}
EDGE_SIZES = (10, 11, 63, 64, 65, 1080, 1088, 1217, 1280)
SIZES = tuple(sorted(set(ROW_SIZES.values()) | set(EDGE_SIZES)))

# beam counts the fixture network (tests/golden/policy_mlp720.npz, 720 inputs) accepts: (num_rays, in_start)
NN_SIZES = ((720, 0), (769, 0), (1024, 0), (1280, 0), (900, 180), (1217, 180))
NN_CLIPPED = (720, 900, 1280)                 # part B: steer_clip set at these, None at the others

R_CARS = 19                                   # three workgroups of DRIVE_CARS, the last one partial


def one_hot_beams(n):
    """The beams j* that decide a crash alone: both ends of the first row, the last beam of the last full row, the
    first and the last beam of the last row."""
    rows = rows_of(n)
    js = {0, min(63, n - 1), 64 * (rows - 1), n - 1}
    if rows > 1:
        js.add(64 * (rows - 1) - 1)
    return tuple(sorted(js))


def one_hot_edge(n, j):
    """An outline table no beam can reach (-100 m) except beam j (+100 m: any range is inside it); j None: no beam."""
    edge = np.full(n, -100.0)
    if j is not None:
        edge[j] = 100.0
    return edge


# ---------------------------------------------------------------- part A / B: 19 cars in an empty 10 m room
ROOM = 200                                    # maps.make_room(200): 0.05 m cells, one-cell walls, origin (0, 0, 0)
WALL_CARS = (1, 6, 8, 12, 17, 18)             # side-on within 4 cm of a wall; one of them in every workgroup


def room_starts(n):
    """(states (19, 11), speeds (19,), steer0 f32 (19,)) of part B at n beams: 13 cars in free space, the WALL_CARS
    side-on between 1 and 4 cm from the inner face of a wall (x or y = 0.05 / 9.95), round the four walls."""
    rng = np.random.default_rng(1000 + n)
    states = np.zeros((R_CARS, 11))
    states[:, 0] = rng.uniform(2.5, 7.5, R_CARS)
    states[:, 1] = rng.uniform(2.5, 7.5, R_CARS)
    states[:, 2] = rng.uniform(-math.pi, math.pi, R_CARS)
    speeds = rng.uniform(1.0, 7.0, R_CARS)
    states[:, 3] = rng.uniform(0.0, 1.0, R_CARS) * speeds
    lo, hi = 0.05, ROOM * 0.05 - 0.05
    for i, r in enumerate(WALL_CARS):
        gap, along = rng.uniform(0.01, 0.04), rng.uniform(2.0, 8.0)
        wall = i % 4
        if wall == 0:
            states[r, :3] = (lo + gap, along, math.pi / 2)
        elif wall == 1:
            states[r, :3] = (hi - gap, along, -math.pi / 2)
        elif wall == 2:
            states[r, :3] = (along, lo + gap, 0.0)
        else:
            states[r, :3] = (along, hi - gap, math.pi)
        states[r, 3], speeds[r] = 0.0, 1.0
    steer0 = rng.uniform(-0.3, 0.3, R_CARS).astype(np.float32)
    return states, speeds, steer0


def room_method(n):
    """Part B's range method at n beams: ("RMGPU", noise 0.05) for odd row counts, ("RM", 0.0) — PyRayMarching's
    default, the upstream-literal arithmetic — for even ones."""
    return ("RMGPU", 0.05) if rows_of(n) % 2 else ("RM", 0.0)


# ---------------------------------------------------------------- part D: roll-out lengths
ROLLOUT_SHAPES = ((1, 1), (7, 3), (128, 10), (129, 10), (257, 16), (300, 7), (512, 64))      # (L, action_every)
ROLLOUT_K, ROLLOUT_ITERS, ROLLOUT_RAYS = 5, 8, 65
BIG_ROOM = 2000                               # a 100 m room: 512 steps at the car's top speed stay inside it


def big_room_roots(K=ROLLOUT_K, seed=3):
    """(states, recent actions, seeds) of part D: cars within 3 m of the big room's centre."""
    rng = np.random.default_rng(seed)
    states = np.zeros((K, 11))
    c = BIG_ROOM * 0.05 / 2
    states[:, 0] = c + rng.uniform(-3.0, 3.0, K)
    states[:, 1] = c + rng.uniform(-3.0, 3.0, K)
    states[:, 2] = rng.uniform(-math.pi, math.pi, K)
    states[:, 3] = rng.uniform(0.0, 3.0, K)
    seeds = rng.integers(0, 2 ** 63, K, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    return states, rng.uniform(-0.3, 0.3, K), seeds


def pairwise_sum_capped(v, depth):
    """mcts_statement.pairwise_sum with the recursion cut after `depth` splits (the device's mcts_pairwise<depth>):
    depth 3 is NumPy's order up to 512 elements, depth 1 leaves the second-level split out, which
    every n > 256 takes (and 249 ... 255, whose larger half exceeds 128)."""
    v = [float(x) for x in v]

    def block(lo, n):
        if n < 8:
            res = 0.0
            for i in range(n):
                res += v[lo + i]
            return res
        r = v[lo:lo + 8]
        i = 8
        while i < n - (n % 8):
            for j in range(8):
                r[j] += v[lo + i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            res += v[lo + i]
            i += 1
        return res

    def P(lo, n, d):
        if d == 0 or n <= 128:
            return block(lo, n)
        n2 = n // 2
        n2 -= n2 % 8
        return P(lo, n2, d - 1) + P(lo + n2, n - n2, d - 1)

    return 0.0 + P(0, len(v), depth)


def assert_rollout_regime(L, every, rollouts):
    """rollouts: the statement's record [(crash index, velocities (L,))] of a run at (L, every).  Some node's summed
    length n is L itself; for L > 256 some node's NumPy sum differs in its bits from the sum without the second-level
    split (otherwise the depth-2 path of mcts_pairwise would be invisible)."""
    import mcts_statement as S
    lengths = [len(v) if idx < 0 else min(idx, len(v)) for idx, v in rollouts]
    assert L in lengths, ("no roll-out of (%d, %d) survives to n = L" % (L, every), sorted(set(lengths)))
    for idx, v in rollouts:
        vv = v if idx < 0 else v[:idx]
        assert pairwise_sum_capped(vv, 3) == S.pairwise_sum(vv)
    if L > 256:
        differ = [n for (idx, v), n in zip(rollouts, lengths)
                  if n > 256 and pairwise_sum_capped(v[:n], 1) != S.pairwise_sum(v[:n])]
        assert differ, "the second-level split changes no sum at L = %d" % L


# ---------------------------------------------------------------- part C / E
TREE_COUNTS = (65, 130)                       # one lane per tree in 64-lane workgroups: blockIdx.x = 1 and 2
ALONE_TREES = (64, 65, 129)
CRASH_BEAMS = (10, 63, 64, 65, 129, 720, 1080, 1280)
CRASH_POSES = (200, 513)                      # the two sides of the per-pose-mark switch (512 poses)
CRASH_CDDT_BEAMS = (10, 65, 1280)
