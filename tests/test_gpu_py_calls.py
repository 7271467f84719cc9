"""The wrappers no other test runs (docs/history/py_calls.md), at the smallest shape that uses every pointer they take:
a 64 x 64 room, 4 poses, 16 beams, each against its host-pointer sibling, which the oracle pins elsewhere."""
import ctypes as C
import math

import numpy as np
import pytest

import support
from support import FOV, same_bits
from pyracecarsimulator_amd import _lib, range_libc

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("need_gpu")]

NB, GROUP = 16, 4


@pytest.fixture(scope="module")
def room():
    import torch
    occ = np.zeros((64, 64), np.uint8)
    occ[0, :] = occ[-1, :] = occ[:, 0] = occ[:, -1] = 1
    m = range_libc.PyRayMarchingGPU(range_libc.PyOMap(occ, 0.05), 60)
    # four cars around the middle of the 3.2 m room, nose to nose: every lidar has another car in front of it
    cars = np.array([[1.2, 1.6, 0.0], [2.0, 1.6, math.pi], [1.6, 1.2, math.pi / 2], [1.6, 2.0, -math.pi / 2]])
    return {"m": m, "cars": cars, "poses": support.lidar_poses(cars), "dev": torch.device("cuda:0"), "torch": torch}


def _to_device(room, *arrays):
    return [room["torch"].from_numpy(np.ascontiguousarray(a)).to(room["dev"]) for a in arrays]


def test_calc_range_many_device_equals_the_host_form(room):
    torch, m = room["torch"], room["m"]
    ang = room["poses"][:, None, 2] - FOV / 2 + (FOV / NB) * np.arange(NB, dtype=np.float32)[None, :]
    ins = np.empty((4 * NB, 3), np.float32)                       # one (x, y, theta) row per ray
    ins[:, :2] = np.repeat(room["poses"][:, :2], NB, axis=0)
    ins[:, 2] = ang.reshape(-1)
    want = np.full(4 * NB, -1.0, np.float32)
    m.calc_range_many(ins, want)
    assert (want > 0).all()
    d_ins, = _to_device(room, ins)
    for stream in (None, torch.cuda.Stream()):
        d_out = torch.full((4 * NB,), -3.0, dtype=torch.float32, device=room["dev"])
        torch.cuda.synchronize()
        if stream is None:
            m.calc_range_many_device(d_ins.data_ptr(), d_out.data_ptr(), 4 * NB)
        else:
            m.calc_range_many_device(d_ins.data_ptr(), d_out.data_ptr(), 4 * NB, stream=stream.cuda_stream)
        torch.cuda.synchronize()
        assert same_bits(d_out.cpu().numpy(), want)


@pytest.mark.parametrize("aux", [False, True])
def test_calc_range_fan_cars_device_equals_the_host_form(room, aux):
    torch, m, poses, cars = room["torch"], room["m"], room["poses"], room["cars"]
    n = 4 * NB
    hits, steps = (np.empty((n, 2), np.int32), np.empty(n, np.uint16)) if aux else (None, None)
    want = m.calc_range_fan_cars(poses, cars, GROUP, FOV, NB, hit_cells=hits, steps=steps)
    plain = np.empty(n, np.float32)
    m.calc_range_fan(poses, plain, FOV, NB)
    assert (want < plain).any() and (want <= plain).all()             # the other cars are seen
    d_poses, d_cars = _to_device(room, poses, cars)
    d_out = torch.full((n,), -3.0, dtype=torch.float32, device=room["dev"])
    d_hits = torch.full((n, 2), -3, dtype=torch.int32, device=room["dev"])
    d_steps = torch.full((n,), -3, dtype=torch.int16, device=room["dev"])        # (uint16 words)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    kw = dict(d_hits_ptr=d_hits.data_ptr(), d_steps_ptr=d_steps.data_ptr()) if aux else {}
    m.calc_range_fan_cars_device(d_poses.data_ptr(), d_cars.data_ptr(), 4 // GROUP, GROUP, FOV, NB, d_out.data_ptr(),
                                 stream=stream.cuda_stream, **kw)
    stream.synchronize()
    assert same_bits(d_out.cpu().numpy(), want)
    if aux:
        assert same_bits(d_hits.cpu().numpy(), hits) and same_bits(d_steps.cpu().numpy().view(np.uint16), steps)
    else:
        assert (d_hits.cpu().numpy() == -3).all() and (d_steps.cpu().numpy() == -3).all()      # omitted: untouched


def test_debug_stamps_reads_what_the_library_recorded(room):
    m, poses, nb = room["m"], room["poses"], 64
    plain, out = np.empty(4 * nb, np.float32), np.empty(4 * nb, np.float32)
    m.calc_range_fan(poses, plain, FOV, nb)
    m.set_option("debug_stamps", 1)
    try:
        m.calc_range_fan(poses, out, FOV, nb)
        assert m.last_plan()["kernel"] == "rm_stream"                  # (the kernel that stamps)
        s = m.debug_stamps()
        waves = m.get_info("last_grid") * 4
        assert s.dtype == np.uint64 and s.shape == (waves, 4) and waves > 0
        direct = np.zeros(waves * 4, np.uint64)                        # the same read through the typed entry point
        got = _lib.lib().rl_debug_read_stamps(m._h, direct.ctypes.data_as(C.POINTER(C.c_uint64)), direct.size)
        assert got == direct.size and same_bits(s.reshape(-1), direct)
    finally:
        m.set_option("debug_stamps", 0)
    assert same_bits(out, plain)                                       # the option changes no range
