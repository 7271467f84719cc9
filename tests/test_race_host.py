"""Batched multi-car races, host side: the NumPy outline statement (tests/race_statement.py) against hand-worked
cases and its geometric invariants, and the union identity that makes the race scan exact without a per-race
table: the EDT of a grid with extra cells stamped is the elementwise min of the two EDTs, bit for bit."""
import math

import numpy as np
import pytest

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
