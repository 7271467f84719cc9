// outline_device.h — the canonical outline of a car of a batched race (include/scanlib.h, "batched multi-car races"), as
// device functions and launch constants only: what the race kernels of race_kernels.h (abi_car.hip) and the CDDT race
// kernel of cddt_kernels.h (abi_fan.hip) share.  No kernels in here, so both units can include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_device.h"

namespace scan {

constexpr int RACE_MAX_GROUP = 8;          // cars per race
constexpr int RACE_MAX_POINTS = 512;       // outline points per car
constexpr int RACE_MAX_RAYS = 1280;        // beams per scan (FollowGap's one-bit-per-beam kernel)
constexpr int RACE_WG = 256;
// the CDDT race kernel parks group x theta_disc per-bin ranges in LDS next to the outlines' 16 KiB: at most this many floats
constexpr int RACE_CDDT_MAX_BINS = 8192;

// The canonical outline of a car (include/scanlib.h): the rectangle LENGTH x WIDTH centred on (x, y), traced at
// half-cell spacing.  Every field is computed on the host: n_l / n_w = max(1, ceil(len / (0.5 res))) in double,
// inv_res = 1.0 / res in double, the rest the map's float32 parameters widened.
struct OutlineParams {
    double half_l, half_w;              // LENGTH / 2, WIDTH / 2
    int n_l, n_w;                       // points on a long (corners 0 -> 1, 2 -> 3) / a short edge
    double ox, oy, inv_res, wa_cos, wa_sin;
    int rows, cols;                     // < 32768 (cells are packed as row << 16 | col)
};

__device__ __forceinline__ int outline_points(const OutlineParams &o) { return 2 * (o.n_l + o.n_w); }

// point k of the outline of the car at (x, y) with heading (s, c) -> its cell as row << 16 | col, or -1 when it lies
// off the grid or is not finite.  Every operation a separately rounded double (the unit is built with -ffp-contract=off).
__device__ __forceinline__ int outline_cell(const OutlineParams &o, double x, double y, double s, double c, int k)
{
    // edge e runs from corner e to corner e + 1 mod 4: (L/2, W/2), (-L/2, W/2), (-L/2, -W/2), (L/2, -W/2)
    int e = 0, n = o.n_l;
    if (k >= n) { k -= n; e = 1; n = o.n_w; }
    if (e == 1 && k >= n) { k -= n; e = 2; n = o.n_l; }
    if (e == 2 && k >= n) { k -= n; e = 3; n = o.n_w; }
    const double a0 = (e == 0 || e == 3) ? o.half_l : -o.half_l, b0 = e < 2 ? o.half_w : -o.half_w;
    const double a1 = e < 2 ? -o.half_l : o.half_l, b1 = (e == 0 || e == 3) ? o.half_w : -o.half_w;
    const double u = (double)k / (double)n;
    const double a = a0 + (a1 - a0) * u, b = b0 + (b1 - b0) * u;
    const double xw = x + (c * a - s * b), yw = y + (s * a + c * b);
    const double gx0 = (xw - o.ox) * o.inv_res, gy0 = (yw - o.oy) * o.inv_res;
    const double gx = o.wa_cos * gx0 - o.wa_sin * gy0, gy = o.wa_sin * gx0 + o.wa_cos * gy0;
    // (floor(g) in [0, n) <=> g in [0, n); NaN fails both)
    if (!(gx >= 0.0 && gx < (double)o.cols && gy >= 0.0 && gy < (double)o.rows)) return -1;
    return ((int)gy << 16) | (int)gx;
}

struct CellBox {
    int r0, r1, c0, c1;                 // inclusive; meaningful when the car has a cell
};

// One wave rasterises one car: the cells of its outline points in point order, a point whose cell repeats the point
// before it dropped, each handed to emit(slot, cell).  Returns the cell count (wave-uniform); box: their bounding box.
template <class EMIT>
__device__ inline int outline_wave(const OutlineParams &o, double x, double y, double theta, int lane, EMIT emit,
                                   CellBox &box)
{
    float sf, cf;
    det_sincosf((float)theta, sf, cf);
    const double s = sf, c = cf;
    const int n_pts = outline_points(o);
    int count = 0, prev = -1;
    int r0 = INT_MAX, r1 = -1, c0 = INT_MAX, c1 = -1;
    for (int base = 0; base < n_pts; base += 64) {
        const int k = base + lane;
        const int cell = k < n_pts ? outline_cell(o, x, y, s, c, k) : -1;
        int before = __shfl(cell, (lane + 63) & 63);
        if (lane == 0) before = prev;
        const bool keep = cell >= 0 && cell != before;
        const uint64_t mask = __ballot(keep);
        if (keep) {
            emit(count + __popcll(mask & ((1ull << lane) - 1ull)), cell);
            const int r = cell >> 16, cc = cell & 0xffff;
            r0 = min(r0, r); r1 = max(r1, r);
            c0 = min(c0, cc); c1 = max(c1, cc);
        }
        count += __popcll(mask);
        prev = __shfl(cell, 63);
    }
    for (int w = 32; w >= 1; w >>= 1) {
        r0 = min(r0, __shfl_xor(r0, w)); r1 = max(r1, __shfl_xor(r1, w));
        c0 = min(c0, __shfl_xor(c0, w)); c1 = max(c1, __shfl_xor(c1, w));
    }
    box = CellBox{r0, r1, c0, c1};
    return count;
}

struct RaceParams {
    OutlineParams o;
    const double *cars;                 // car n's (x, y, theta) at cars[n * car_stride + 0, 1, 2]
    int car_stride;                     // 3: rl_calc_range_fan_cars' rows; 11: the getState rows of a race
    int group, n_groups;
};

}  // namespace scan
