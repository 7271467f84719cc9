// pursuit_device.h — the pure-pursuit steer towards a world point (include/scanlib.h, "the pursuit steer"): the one
// statement the track expansion source (RL_MCTS_PURSUIT) and the pursuit roll-outs of the MCTS planner share.
#pragma once
#include <hip/hip_runtime.h>

namespace scan {

// The steer of a car at (x, y, th) with wheelbase WB towards (X, Y), clamped to +-max_steer: the point in the car's frame
// as track_kernel's (gx, gy), the arc through it, every f64 operation rounded on its own, the answer rounded to f32 as
// FollowGap's and the network's are.  0.0f when the point is the car or something is NaN.
__device__ inline float pursuit_steer(double WB, double max_steer, double x, double y, double th, double X, double Y)
{
    const double rx = X - x, ry = Y - y;
    const double hx = cos(th), hy = sin(th);
    const double gx = hx * rx + hy * ry;
    const double gy = hx * ry - hy * rx;
    const double d2 = gx * gx + gy * gy;
    if (!(d2 > 0.0)) return 0.0f;
    double a = atan(((2.0 * WB) * gy) / d2);
    a = fmin(fmax(a, -max_steer), max_steer);
    return (float)a;
}

}  // namespace scan
