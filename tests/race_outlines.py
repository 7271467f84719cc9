"""Car outlines beyond one 64-lane pass of outline_wave (csrc/race_kernels.h): the size ladder, the three maps, the
seeded cars of the outline test with the census its sample must reach, and the seeded races of the scan test with
theirs.  Plain data and NumPy over tests/race_statement.py and the oracle: the host tests check it without a GPU, the
GPU tests (tests/test_gpu_race_outlines.py) assert the same censuses before they compare."""
import functools
import math

import numpy as np

import race_statement as RS
import support
from drive_cases import RACE_MRX, race_oracle_fan
from support import FOV
from pyracecarsimulator_amd import maps

# (length m, width m, m per cell, outline points 2 (n_l + n_w)); none of the sizes sits on a ceil boundary
LADDER = ((0.4064, 0.2032, 0.05, 52),        # the default car: one partial round
          (0.49, 0.29, 0.05, 64),            # one full round
          (0.49, 0.31, 0.05, 66),            # a second round of 2 lanes
          (1.06, 0.51, 0.05, 128),           # two full rounds
          (1.06, 0.53, 0.05, 130),           # a third round
          (0.4064, 0.2032, 0.01, 246),       # the default car on a fine map
          (4.49, 1.89, 0.05, 512),           # the cap: eight full rounds
          (4.49, 1.91, 0.05, 514))           # refused
MAX_POINTS = 512
ACCEPTED = tuple(row for row in LADDER if row[3] <= MAX_POINTS)
BY_POINTS = {row[3]: row for row in LADDER}
WAVE = 64


@functools.lru_cache(maxsize=None)
def room():
    """20 m at 0.05 m per cell: the big cars."""
    return maps.make_room(400)


@functools.lru_cache(maxsize=None)
def yawed_room():
    g = room()
    return maps.GridMap(g.occ, g.resolution, (3.1, -2.7, 0.61), "yawed")


@functools.lru_cache(maxsize=None)
def fine_room():
    """6 m at 0.01 m per cell: the default car takes 246 points."""
    return maps.make_room(600, resolution=0.01)


def map_of(resolution):
    return fine_room() if resolution < 0.05 else room()


def to_world(g, u, v):
    """Metres along the grid's axes from its corner -> world (the inverse of the map's world -> grid turn)."""
    c, s = math.cos(g.origin[2]), math.sin(g.origin[2])
    return g.origin[0] + c * u - s * v, g.origin[1] + s * u + c * v


def most_cells(length, width, resolution):
    """An upper bound of the cells one outline can emit: a straight run of d cells changes cell at most
    d (|cos| + |sin|) <= d sqrt 2 times, and each of the four edges starts with one more."""
    return int(math.sqrt(2.0) * 2.0 * (length + width) / resolution) + 4


# ---------------------------------------------------------------- a. rl_car_outline_cells
OUTLINE_CARS, OUTLINE_SEED = 1500, 20


def outline_cars(g, length, seed=OUTLINE_SEED, n=OUTLINE_CARS):
    """float64 (n, 3): positions over the map and a margin of twice the car length on every side (many cars partly off
    the grid, some wholly), the last fifth of them within a car length of one of the four borders (a uniform draw
    leaves some 13 of 1500 cars of 1 m with only their later rounds off the grid), theta in +-7, and twelve rows with
    a NaN, an infinity or 1e300 in them."""
    rng = np.random.default_rng(seed)
    side_u, side_v, margin = g.cols * g.resolution, g.rows * g.resolution, 2.0 * length
    u, v = rng.uniform(-margin, side_u + margin, n), rng.uniform(-margin, side_v + margin, n)
    near = np.arange(n - n // 5, n)
    border, off = rng.integers(0, 4, near.size), rng.uniform(-length, length, near.size)
    u[near] = np.where(border == 0, off, np.where(border == 1, side_u + off, u[near]))
    v[near] = np.where(border == 2, off, np.where(border == 3, side_v + off, v[near]))
    x, y = to_world(g, u, v)
    cars = np.stack([x, y, rng.uniform(-7.0, 7.0, n)], -1)
    bad = (np.nan, np.inf, -np.inf, 1e300, -1e300, np.nan, np.inf, 1e300, np.nan, -np.inf, -1e300, np.inf)
    for j, v in enumerate(bad):
        cars[(7 + 113 * j) % n, j % 3] = v
    return cars


def outline_census(cell):
    """What a sample of cars (RS.point_cells) holds of the paths only a later round takes: counts of cars."""
    keep = RS.kept_points(cell)
    n_pts = cell.shape[1]
    lane0 = np.arange(WAVE, n_pts, WAVE)                       # lane 0 of every later round
    before = cell[:, lane0 - 1]
    later_off = (cell[:, WAVE:] < 0).any(1) if n_pts > WAVE else np.zeros(len(cell), bool)
    return dict(beyond_64=int((keep.sum(1) > WAVE).sum()),
                kept_at_lane0=int(keep[:, lane0].any(1).sum()),
                dropped_at_lane0=int(((cell[:, lane0] >= 0) & (cell[:, lane0] == before)).any(1).sum()),
                off_grid_later_only=int((later_off & (cell[:, :WAVE] >= 0).all(1)).sum()),
                wholly_off=int((cell < 0).all(1).sum()),
                partly_off=int(((cell < 0).any(1) & (cell >= 0).any(1)).sum()))


def outline_census_floor(length, width, resolution, points, n=OUTLINE_CARS):
    """The least each census entry must reach at this size.  Two entries cannot be met by every size: an outline of
    most_cells(...) <= 64 cells never fills slot 64, and later rounds that hold only inner points of the last edge
    (fewer than n_w points, as at 66) cannot leave the grid alone: they lie on one straight line between a point of
    the first round and corner 0, which is point 0, and the grid is convex."""
    if points <= WAVE:
        return {}
    floor = dict(kept_at_lane0=20, dropped_at_lane0=20)
    if most_cells(length, width, resolution) > WAVE:
        floor["beyond_64"] = n // 10
    n_w = RS.edge_counts(length, width, resolution)[1]
    if points - WAVE >= n_w:
        floor["off_grid_later_only"] = 20
    return floor


# ---------------------------------------------------------------- b. the race scan
# (points, group, n_groups, beams) -> the seed of the race; "special": what the case carries beside its races
FAN_BEAMS = 360
FAN_CASES = {(66, 2, 3, 360): dict(seed=1), (66, 8, 2, 360): dict(seed=2),
             (130, 2, 3, 360): dict(seed=3), (130, 8, 2, 360): dict(seed=4, special="off_grid"),
             (246, 2, 3, 360): dict(seed=5), (246, 8, 2, 360): dict(seed=6, special="nan"),
             (512, 2, 3, 360): dict(seed=7), (512, 8, 2, 360): dict(seed=8),
             (512, 8, 2, 1280): dict(seed=9)}
YAWED_CASE = (130, 4, 2, 360)
YAWED_SEED = 10


def fan_race(g, points, group, n_groups, seed, special=None):
    """(cars float64 (N, 3), lidar poses float32 (N, 3)): the cars of a race within a car length of the race's centre,
    so within about two of each other; the centres far enough inside the map that every lidar stands in it.
    ``special``: "off_grid" moves car 1 of race 0 wholly off the grid, "nan" gives it a NaN x; both keep a lidar pose
    inside the map (the pose is an argument of its own)."""
    length, width, res, _ = BY_POINTS[points]
    rng = np.random.default_rng(seed)
    side = g.cols * g.resolution
    reach = length + 0.5 * math.hypot(length, width) + 0.4
    cu, cv = rng.uniform(reach, side - reach, n_groups), rng.uniform(reach, side - reach, n_groups)
    u = np.repeat(cu, group) + rng.uniform(-length, length, n_groups * group)
    v = np.repeat(cv, group) + rng.uniform(-length, length, n_groups * group)
    x, y = to_world(g, u, v)
    cars = np.stack([x, y, g.origin[2] + rng.uniform(-math.pi, math.pi, n_groups * group)], -1)
    poses = support.lidar_poses(cars)
    if special == "off_grid":
        cars[1, :2] = to_world(g, -3.0 * length - 1.0, 0.5 * side)
    elif special == "nan":
        cars[1, 0] = np.nan
    elif special is not None:
        raise ValueError(special)
    return cars, poses


def first_round_only(seqs):
    """Each car's cells in slots 0 ... 63 of its sequence: what a kernel that loses the later rounds keeps."""
    return [s[:WAVE] for s in seqs]


def fan_census(oracle_mod, g, cars, poses, points, group, num_rays, literal, step_coeff, want=None):
    """From the oracle alone: rays of the scan on the stamped grid (``want``: its ranges, if the caller has them) that
    differ from the plain scan, and rays that differ from the scan on the grid stamped with first_round_only."""
    length, width = BY_POINTS[points][:2]
    args = (length, width, g.resolution, g.origin, g.rows, g.cols, oracle_mod.sincosf)
    if want is None:
        want = race_oracle_fan(oracle_mod, g, RS.outline_cells(cars, *args), group, poses, num_rays, literal, step_coeff)[0]
    om = oracle_mod.OracleMap(g.occ, g.resolution, g.origin, RACE_MRX)
    plain = (om.rm_fan_libm if literal else om.rm_fan)(poses, FOV, num_rays, step_coeff=step_coeff)[0]
    seqs = RS.outline_sequence(cars, *args)
    short = race_oracle_fan(oracle_mod, g, first_round_only(seqs), group, poses, num_rays, literal, step_coeff)[0]
    return dict(seen=int((want != plain).sum()), later_rounds=int((want != short).sum()),
                empty_cars=int(sum(s.size == 0 for s in seqs)))


def fan_census_floor(points):
    """Condition 1 everywhere; condition 2 where an outline can fill slot 64 at all (not at 66 points: at most 49)."""
    length, width, res, _ = BY_POINTS[points]
    return dict(seen=100, later_rounds=30 if most_cells(length, width, res) > WAVE else 0)
