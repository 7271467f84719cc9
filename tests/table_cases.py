"""What the tests of the per-handle derived tables share (test_gpu_map_mutation.py, test_gpu_table_streams.py): the
oracle's ranges of a fan for each table kind and the comparison of result tuples.  No tests and no marks live here."""
import numpy as np


def all_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def rm_ranges(o, poses, fov, num_rays):
    """PyRayMarchingGPU's ranges (canonical arithmetic, step coefficient 1)."""
    return o.rm_fan(poses, fov, num_rays, step_coeff=1.0, nthreads=8, want_hits=False, want_steps=False)[0]


def bl_ranges(o, poses, fov, num_rays):
    return o.bl_fan(poses, fov, num_rays, nthreads=8)[0]


def cddt_ranges(o, theta_disc, poses, fov, num_rays):
    return o.cddt_fan(theta_disc, poses, fov, num_rays, nthreads=8)


def lut_ranges(o, theta_disc, poses, fov, num_rays):
    return o.lut_fan(o.lut_build(theta_disc, nthreads=8), poses, fov, num_rays)
