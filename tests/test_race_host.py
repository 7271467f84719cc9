"""Batched multi-car races, host side: the NumPy outline statement (tests/race_statement.py) against hand-worked
cases and its geometric invariants, and the union identity that makes the race scan exact without a per-race
table: the EDT of a grid with extra cells stamped is the elementwise min of the two EDTs, bit for bit."""
import math

import numpy as np
import pytest

import race_outlines as RO
import race_statement as RS


@pytest.fixture(scope="module")
def sincosf(oracle_mod):
    return oracle_mod.sincosf


def _cells(sincosf, car, length=4.0, width=2.0, res=1.0, origin=(0.0, 0.0, 0.0), rows=20, cols=20):
    flat = RS.outline_cells([car], length, width, res, origin, rows, cols, sincosf)[0]
    return {(int(c) // cols, int(c) % cols) for c in flat}


def _ring(r0, r1, c0, c1):
    return {(r, c) for r in range(r0, r1 + 1) for c in range(c0, c1 + 1) if r in (r0, r1) or c in (c0, c1)}


def test_edge_counts():
    assert RS.edge_counts(4.0, 2.0, 1.0) == (8, 4)
    assert RS.edge_counts(0.4064, 0.2032, 0.05) == (17, 9)           # the reference car: 52 points
    assert RS.edge_counts(1e-9, 1e-9, 0.05) == (1, 1)
    a, b = RS.car_frame_points(4.0, 2.0, 1.0)
    assert a.size == b.size == 24
    assert (a[0], b[0]) == (2.0, 1.0) and (a[8], b[8]) == (-2.0, 1.0) and (a[12], b[12]) == (-2.0, -1.0)
    assert (a[20], b[20]) == (2.0, -1.0)


@pytest.mark.parametrize("theta,ring", [(0.0, (9, 11, 8, 12)), (math.pi / 2, (8, 12, 9, 11)),
                                        (math.pi, (9, 11, 8, 12)), (-math.pi / 2, (8, 12, 9, 11))])
def test_axis_aligned_headings(sincosf, theta, ring):
    """A 4 x 2 cell car whose points sit a quarter cell inside the cells: the ring of cells around it."""
    assert _cells(sincosf, (10.25, 10.25, theta)) == _ring(*ring)


def test_points_on_cell_borders(sincosf):
    """Centred on a cell centre at heading 0 (sin 0, cos 1 exactly): points land on integer coordinates and floor
    puts them in the cell above / to the right of the border."""
    s, c = sincosf(np.float32(0.0))
    assert (float(s[0]), float(c[0])) == (0.0, 1.0)
    assert _cells(sincosf, (10.5, 10.5, 0.0)) == _ring(9, 11, 8, 12)
    gx, gy = RS.grid_points([(10.5, 10.5, 0.0)], 4.0, 2.0, 1.0, (0.0, 0.0, 0.0), sincosf)
    assert 9.0 in gx[0] and 10.0 in gy[0]


def test_yawed_map(sincosf):
    """Origin yaw pi/2: world (x, y) lands at col ~ y, row ~ -x."""
    got = _cells(sincosf, (-10.25, 10.25, 0.0), origin=(0.0, 0.0, math.pi / 2))
    assert got == _ring(8, 12, 9, 11)


def test_points_off_the_grid(sincosf):
    assert _cells(sincosf, (0.25, 0.25, 0.0)) == {(1, 0), (1, 1), (1, 2), (0, 2)}
    assert _cells(sincosf, (-30.0, 5.0, 0.3)) == set()
    flat = RS.outline_cells([(float("nan"), 5.0, 0.0), (5.0, float("inf"), 0.0)], 4.0, 2.0, 1.0, (0, 0, 0), 20, 20,
                            sincosf)
    assert all(f.size == 0 for f in flat)


def _sequence(sincosf, car, cols=20):
    seq = RS.outline_sequence([car], 4.0, 2.0, 1.0, (0.0, 0.0, 0.0), 20, cols, sincosf)[0]
    return [(int(c) // cols, int(c) % cols) for c in seq]


def test_outline_sequence_known_answers(sincosf):
    """outline_sequence on the 4 x 2 cell car, 24 points half a cell apart, worked by hand from the points."""
    # heading 0, a quarter cell inside the cells: along row 11 the columns 12 11 11 10 10 9 9 8, the corner (11, 8)
    # again, down column 8, (9, 8) again, along row 9, up column 12; the last point (10, 12) meets no first point
    assert _sequence(sincosf, (10.25, 10.25, 0.0)) == [(11, 12), (11, 11), (11, 10), (11, 9), (11, 8), (10, 8), (9, 8),
                                                       (9, 9), (9, 10), (9, 11), (9, 12), (10, 12)]
    # across the grid's corner: points 5 ... 21 lie off it, point 22 has no cell before it, point 23 repeats it
    assert _sequence(sincosf, (0.25, 0.25, 0.0)) == [(1, 2), (1, 1), (1, 0), (0, 2)]
    # heading pi / 4, corner 1 at x = -0.07 off the grid between point 7 at (0.28, 5.85) and point 9 at (0.28, 5.14),
    # both in cell (5, 0) and both kept: a point without a cell is no cell to repeat
    gx, gy = RS.grid_points([(2.05, 6.2, math.pi / 4)], 4.0, 2.0, 1.0, (0.0, 0.0, 0.0), sincosf)
    assert gx[0, 8] < 0.0 and (int(gx[0, 7]), int(gy[0, 7])) == (int(gx[0, 9]), int(gy[0, 9])) == (0, 5)
    assert _sequence(sincosf, (2.05, 6.2, math.pi / 4)) == [(8, 2), (7, 2), (7, 1), (6, 1), (6, 0), (5, 0), (5, 0),
                                                            (4, 0), (4, 1), (4, 2), (5, 2), (5, 3), (6, 3), (6, 4),
                                                            (7, 3)]
    # wholly off the grid, and not finite
    assert _sequence(sincosf, (-30.0, 5.0, 0.3)) == []
    assert _sequence(sincosf, (float("nan"), 5.0, 0.0)) == [] and _sequence(sincosf, (5.0, float("inf"), 0.0)) == []
    assert _sequence(sincosf, (1e300, 5.0, 0.0)) == []


def test_size_ladder():
    """The ladder of tests/race_outlines.py holds the point counts it names, from one full round to the cap and one
    size beyond it."""
    assert [row[3] for row in RO.LADDER] == [52, 64, 66, 128, 130, 246, 512, 514]
    for length, width, res, points in RO.LADDER:
        n_l, n_w = RS.edge_counts(length, width, res)
        assert 2 * (n_l + n_w) == points, (length, width, res)
        a, _ = RS.car_frame_points(length, width, res)
        assert a.size == points
    assert [row[3] for row in RO.ACCEPTED] == [52, 64, 66, 128, 130, 246, 512]
    # what the census floors rest on: 66 points emit at most 49 cells and their second round is two inner points of
    # the last edge; every larger size can fill slot 64 and has later rounds that reach beyond that edge
    assert RO.most_cells(*RO.BY_POINTS[66][:3]) == 49
    assert set(RO.outline_census_floor(*RO.BY_POINTS[66])) == {"kept_at_lane0", "dropped_at_lane0"}
    for points in (128, 130, 246, 512):
        assert set(RO.outline_census_floor(*RO.BY_POINTS[points])) == {"kept_at_lane0", "dropped_at_lane0", "beyond_64",
                                                                      "off_grid_later_only"}


def test_sequence_against_set(sincosf):
    """Every accepted row of the ladder and 300 random cars each, many across the border: the sequence holds the
    cells of outline_cells, no more of them than points, and no cell twice in a row unless a point without a cell
    lies between."""
    for length, width, res, points in RO.ACCEPTED:
        g = RO.map_of(res)
        cars = RO.outline_cars(g, length, seed=4, n=300)
        args = (length, width, g.resolution, g.origin, g.rows, g.cols, sincosf)
        seqs, flat = RS.outline_sequence(cars, *args), RS.outline_cells(cars, *args)
        cell = RS.point_cells(cars, *args)
        assert cell.shape == (300, points)
        n_some = 0
        for i in range(300):
            assert set(seqs[i].tolist()) == set(flat[i].tolist()), (points, i)
            assert len(seqs[i]) <= points
            assert np.array_equal(cell[i][cell[i] >= 0], flat[i])
            n_some += len(seqs[i]) > 0
            # the sequence by a loop over the points, as the header words it
            want, before = [], -1
            for c in cell[i].tolist():
                if c >= 0 and c != before:
                    want.append(c)
                before = c
            assert seqs[i].tolist() == want, (points, i)
        assert 100 < n_some < 300, points


def test_outline_samples_reach_the_later_rounds(sincosf):
    """The seeded cars of the GPU outline test hold what only a later round of the raster does, at every size."""
    for length, width, res, points in RO.ACCEPTED:
        g = RO.map_of(res)
        cell = RS.point_cells(RO.outline_cars(g, length), length, width, g.resolution, g.origin, g.rows, g.cols, sincosf)
        census, floor = RO.outline_census(cell), RO.outline_census_floor(length, width, res, points)
        assert all(census[k] >= v for k, v in floor.items()), (points, census, floor)
        assert census["wholly_off"] >= 100 and census["partly_off"] >= 100, (points, census)


def test_fan_races_reach_the_later_rounds(oracle_mod):
    """The seeded races of the GPU scan test, by the oracle alone (the literal march at 0.999 and the canonical one at
    1.0): the other cars change at least 100 rays of every case, the cells in slots 64 and beyond at least 30 wherever
    an outline can hold that many, and the two special cases hold their car without a cell."""
    cases = [(RO.map_of(RO.BY_POINTS[c[0]][2]), c, spec) for c, spec in RO.FAN_CASES.items()]
    cases.append((RO.yawed_room(), RO.YAWED_CASE, dict(seed=RO.YAWED_SEED)))
    for g, (points, group, n_groups, nb), spec in cases:
        cars, poses = RO.fan_race(g, points, group, n_groups, **spec)
        assert np.isfinite(poses).all()
        floor = RO.fan_census_floor(points)
        assert floor["later_rounds"] == (30 if points > 66 else 0)
        for literal, coeff in ((True, 0.999), (False, 1.0)):
            census = RO.fan_census(oracle_mod, g, cars, poses, points, group, nb, literal, coeff)
            assert all(census[k] >= v for k, v in floor.items()), (points, group, nb, literal, census)
            assert census["empty_cars"] == ("special" in spec)


def test_closed_loop_and_spacing(sincosf):
    """Cars fully inside the grid: consecutive points (the last back to the first) at most half a cell apart, so
    their cells form a closed 8-connected loop."""
    rng = np.random.default_rng(3)
    n, res = 300, 0.05
    cars = np.stack([rng.uniform(2.0, 8.0, n), rng.uniform(2.0, 8.0, n), rng.uniform(-4.0, 4.0, n)], -1)
    origin = (0.3, -0.2, 0.4)
    gx, gy = RS.grid_points(cars, 0.4064, 0.2032, res, origin, sincosf)
    flat = RS.outline_cells(cars, 0.4064, 0.2032, res, origin, 400, 400, sincosf)
    inside = ((gx >= 0) & (gx < 400) & (gy >= 0) & (gy < 400)).all(1)
    assert inside.sum() > n // 2
    for i in np.nonzero(inside)[0]:
        step = np.hypot(np.diff(np.r_[gx[i], gx[i][:1]]), np.diff(np.r_[gy[i], gy[i][:1]]))
        assert step.max() <= 0.5 + 1e-9
        assert flat[i].size == gx.shape[1]
        r, c = flat[i] // 400, flat[i] % 400
        dr, dc = np.abs(np.diff(np.r_[r, r[:1]])), np.abs(np.diff(np.r_[c, c[:1]]))
        assert dr.max() <= 1 and dc.max() <= 1


def test_union_identity(oracle_mod):
    """oracle.edt(occ | S) == min(oracle.edt(occ), oracle.edt(S)) bit for bit, empty grid and empty set included."""
    rng = np.random.default_rng(7)
    for trial in range(12):
        rows, cols = int(rng.integers(1, 90)), int(rng.integers(1, 90))
        occ = (rng.random((rows, cols)) < [0.0, 0.002, 0.05, 0.3][trial % 4]).astype(np.uint8)
        s = np.zeros_like(occ)
        if trial % 3:
            s.reshape(-1)[rng.integers(0, rows * cols, int(rng.integers(1, 40)))] = 1
        want = oracle_mod.edt(occ | s)
        got = np.minimum(oracle_mod.edt(occ), oracle_mod.edt(s))
        assert want.tobytes() == got.tobytes(), trial
    # a real-size case with a car outline as the set
    occ = np.zeros((200, 300), np.uint8)
    occ[0, :] = occ[-1, :] = occ[:, 0] = occ[:, -1] = 1
    cells = RS.outline_cells([(7.1, 4.3, 0.7)], 0.4064, 0.2032, 0.05, (0.0, 0.0, 0.0), 200, 300,
                             oracle_mod.sincosf)[0]
    s = RS.stamped(np.zeros_like(occ), cells)
    assert oracle_mod.edt(occ | s).tobytes() == np.minimum(oracle_mod.edt(occ), oracle_mod.edt(s)).tobytes()
