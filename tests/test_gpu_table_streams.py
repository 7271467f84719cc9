"""A derived table whose first reader is on another stream than its builder (run with -m gpu on the MI355X box).

A method handle builds its tables lazily on the stream of the call that needs them first (csrc/abi_internal.h
TableCache: fresh? wait : begin a rebuild, build, mark built).  A call on a second stream, enqueued at once behind the
first, finds the table marked fresh while its build is still running on the other stream: it has to wait for the
build's event.  After a map update the rebuild happens while the other stream's launch context is warm.  Every method
goes through the same protocol; each is checked here, bit for bit against the oracle, as are the four beam-direction
tables of a handle called with five fans from two streams."""
import numpy as np
import pytest

from table_cases import bl_ranges, cddt_ranges, lut_ranges, rm_ranges
from pyracecarsimulator_amd import maps, pipeline, range_libc

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

ROWS, COLS, MRX, TD, B, FOV, N = 128, 160, 60, 112, 65, 4.71, 96


def _rm(**opts):
    def make(omap):
        m = range_libc.PyRayMarchingGPU(omap, MRX)
        for k, v in opts.items():
            m.set_option(k, v)
        return m
    return make


def _cddt(theta_min):
    def make(omap):
        m = range_libc.PyCDDTCast(omap, MRX, TD)
        m.set_option("cddt_theta_min", theta_min)
        return m
    return make


def _bl(omap):
    m = range_libc.PyBresenhamsLine(omap, MRX)
    m.set_option("variant", 1)
    return m


# label: (handle, the oracle's ranges, what the plan of its launches has to say)
HANDLES = {
    "RMGPU tiled code map": (_rm(slots=2, code_min_rays=0), "rm", {"kernel": "rm_stream", "tiled": 1, "code": 2}),
    "RMGPU row-major": (_rm(tiled=0), "rm", {"kernel": "rm_stream", "tiled": 0, "code": 0}),
    "Bresenham variant 1": (_bl, "bl", {"kernel": "bl_stream"}),
    "CDDT theta_min 0": (_cddt(0), "cddt", {}),
    "CDDT theta_min 1": (_cddt(1), "cddt", {}),
    "GiantLUT": (lambda omap: range_libc.PyGiantLUTCast(omap, MRX, TD), "lut", {}),
}
RANGES = {"rm": rm_ranges, "bl": bl_ranges, "cddt": lambda o, *a: cddt_ranges(o, TD, *a),
          "lut": lambda o, *a: lut_ranges(o, TD, *a)}


@pytest.fixture(scope="module")
def streams():
    pytest.importorskip("torch")
    st = pipeline.concurrent_streams(2)
    if len(st) < 2:
        pytest.skip("this box runs no two streams concurrently")
    return st


@pytest.fixture(scope="module")
def case(oracle_mod):
    """Two mazes of one shape, their oracle maps, and 96 poses free in both."""
    grids = [maps.make_maze(COLS, cell=24, wall=2, p=0.5, seed=s).occ[:ROWS, :COLS].copy() for s in (17, 18)]
    for occ in grids:
        occ[0, :] = occ[-1, :] = occ[:, 0] = occ[:, -1] = 1
    g = maps.GridMap(grids[0], 0.05, (-1.3, 0.7, 0.25), "streams")
    oms = [oracle_mod.OracleMap(occ, g.resolution, g.origin, MRX) for occ in grids]
    poses = maps.sample_free_poses(g, N, 5, 2.0, dt=np.minimum(oms[0].dt, oms[1].dt))
    want = {}

    def ranges(kind, k):                       # of both halves, on grid k; computed once per kind and grid
        if (kind, k) not in want:
            want[(kind, k)] = RANGES[kind](oms[k], poses, FOV, B)
            want[(kind, k)].setflags(write=False)
        return want[(kind, k)]
    return g, grids, oms, poses, ranges


@pytest.mark.parametrize("label", list(HANDLES))
def test_the_first_reader_of_a_table_is_on_another_stream(case, streams, label):
    """Cold handle: half A on stream 1 and at once half B on stream 2 (B reads the table A's call is building).  Then
    the map is updated and the halves go out with the streams swapped: the rebuild is enqueued on stream 2 while stream
    1's context is warm, and stream 1 reads it.  Both halves equal the oracle on the grid in place, each time."""
    import torch
    g, grids, oms, poses, ranges = case
    make, kind, plan = HANDLES[label]
    omap = range_libc.PyOMap(g)
    m = make(omap)
    half = N // 2
    d_poses = [torch.from_numpy(poses[:half]).cuda(), torch.from_numpy(poses[half:]).cuda()]
    d_out = [torch.empty(half * B, dtype=torch.float32, device="cuda") for _ in range(2)]
    assert not np.array_equal(ranges(kind, 0)[:half * B], ranges(kind, 1)[:half * B])      # both halves see the update
    assert not np.array_equal(ranges(kind, 0)[half * B:], ranges(kind, 1)[half * B:])
    for k, order in ((0, (0, 1)), (1, (1, 0))):
        if k:
            omap.update(grids[1])
        for o in d_out:
            o.fill_(-1.0)
        torch.cuda.synchronize()
        for h, s in zip((0, 1), order):
            m.calc_range_fan_device(d_poses[h].data_ptr(), half, FOV, B, d_out[h].data_ptr(), stream=streams[s].cuda_stream)
            pl = m.last_plan()
            assert all(pl[key] == v for key, v in plan.items()), (label, pl)
        torch.cuda.synchronize()
        got = np.concatenate([o.cpu().numpy() for o in d_out])
        for h in (0, 1):
            assert np.array_equal(got[h * half * B:(h + 1) * half * B], ranges(kind, k)[h * half * B:(h + 1) * half * B]), \
                (label, "grid %d" % k, "half %d on stream %d" % (h, order[h]))
    m.close()
    omap.close()


def test_five_fans_share_four_beam_tables_across_two_streams(case, streams):
    """One ray-marching handle called with five (fov, num_rays) pairs, alternating between two streams, then with the
    first pair again: the fifth fan takes the least recently used of the four beam-direction tables, and the first
    pair's table is built a second time.  Every result equals the oracle."""
    import torch
    g, grids, oms, poses, ranges = case
    fans = [(4.71, 65), (6.2, 33), (3.0, 120), (4.71, 64), (2.0, 17)]
    calls = fans + fans[:1]
    omap = range_libc.PyOMap(g)
    m = range_libc.PyRayMarchingGPU(omap, MRX)
    d_poses = torch.from_numpy(poses).cuda()
    d_out = [torch.full((N * nb,), -1.0, dtype=torch.float32, device="cuda") for _, nb in calls]
    torch.cuda.synchronize()
    for i, (fov, nb) in enumerate(calls):
        m.calc_range_fan_device(d_poses.data_ptr(), N, fov, nb, d_out[i].data_ptr(), stream=streams[i % 2].cuda_stream)
    torch.cuda.synchronize()
    for i, (fov, nb) in enumerate(calls):
        want = ranges("rm", 0) if (fov, nb) == (FOV, B) else rm_ranges(oms[0], poses, fov, nb)
        assert np.array_equal(d_out[i].cpu().numpy(), want), (i, fov, nb)
    m.close()
    omap.close()
