// race_kernels.h — batched multi-car races (rl_calc_range_fan_cars, rl_car_race_followgap, rl_car_outline_cells;
// include/scanlib.h): every car's scan sees the other cars of its race.  The reference's two-player tick writes the
// other car's outline into a copy of the grid, rebuilds the tables and scans (scripts/two_player/rcs_two_player.py:
// 99-126); a batch of races cannot share one map that way.  The march reads the map only through dt[row, col], and
// the EDT of the grid with extra cells S stamped is, bit for bit,
//     dt_{grid u S}(q) = min(dt_grid(q), sqrtf((float)min_{c in S} |q - c|^2))
// (the EDT is sqrtf of the integer squared distance, and sqrtf and the int -> float conversion are monotone).  So
// race_fan_kernel marches on the static EDT and folds the other cars' cells in at each sample: exact, and no per-race
// table.  One workgroup per race: its cars' outline cells sit in LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "literal_kernels.h"
#include "scan_device.h"
#include "outline_device.h"      // the outline itself: OutlineParams, outline_wave, RaceParams, the RACE_ constants

namespace scan {

// rl_car_outline_cells: one wave per car, flat cells row * cols + col, -1 past the count
__global__ __launch_bounds__(256) void outline_cells_kernel(OutlineParams o, const double *__restrict__ cars, int n,
                                                            int max_cells, int32_t *__restrict__ cells,
                                                            int *__restrict__ counts)
{
    const int car = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (car >= n) return;                                   // (wave-uniform)
    int32_t *dst = cells + (size_t)car * max_cells;
    CellBox box;
    const int cnt = outline_wave(o, cars[3 * (size_t)car], cars[3 * (size_t)car + 1], cars[3 * (size_t)car + 2], lane,
                                 [&](int q, int cell) { dst[q] = (cell >> 16) * o.cols + (cell & 0xffff); }, box);
    for (int q = cnt + lane; q < max_cells; q += 64) dst[q] = -1;
    if (lane == 0) counts[car] = cnt;
}

// The scan of every car of race g = blockIdx.x with the other cars of the race in the map.  Pose i of the race is
// scanned as RM / RMGPU scans it (LIT: rm_literal_kernel's upstream-literal arithmetic, else rm_fan_kernel's canonical
// one) with dt(row, col) = min(static EDT, every other car's exact cell distance).  A car's cells are scanned only
// where its bounding box could beat the static value: sqrtf((float)lb^2) >= dt already leaves dt the minimum.
template <bool LIT, bool AUX>
__global__ __launch_bounds__(RACE_WG) void race_fan_kernel(MapParams m, FanParams f, LiteralParams lp, RaceParams rp,
                                                           const float *__restrict__ poses, float *__restrict__ out,
                                                           int32_t *__restrict__ hits, uint16_t *__restrict__ steps)
{
    __shared__ uint32_t cells[RACE_MAX_GROUP][RACE_MAX_POINTS];
    __shared__ CellBox box[RACE_MAX_GROUP];
    __shared__ int n_cells[RACE_MAX_GROUP];
    __shared__ float2 fan_cs[LIT ? 1 : RACE_MAX_RAYS];      // canonical: per-beam (cos a_j, sin a_j)
    const int g = blockIdx.x, group = rp.group;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k = wave; k < group; k += RACE_WG / 64) {
        const double *s = rp.cars + (size_t)(g * group + k) * rp.car_stride;
        CellBox b;
        const int cnt = outline_wave(rp.o, s[0], s[1], s[2], lane, [&](int q, int cell) { cells[k][q] = (uint32_t)cell; }, b);
        if (lane == 0) {
            n_cells[k] = cnt;
            box[k] = b;
        }
    }
    if (!LIT) {
        for (int j = threadIdx.x; j < f.num_rays; j += RACE_WG) {
            float s, c;
            det_sincosf(fan_alpha(f, j), s, c);
            fan_cs[j] = make_float2(c, s);
        }
    }
    __syncthreads();

    const int total = group * f.num_rays;
    for (int r = threadIdx.x; r < total; r += RACE_WG) {
        const int i = r / f.num_rays, j = r - i * f.num_rays;
        const size_t p = (size_t)g * group + i;
        auto dist = [&](int pr, int pc) {
            float d = m.dt[(size_t)pr * m.cols + pc];
            for (int k = 0; k < group; ++k) {
                const int n = n_cells[k];
                if (k == i || n == 0) continue;
                const CellBox b = box[k];
                const int dr = max(max(b.r0 - pr, pr - b.r1), 0), dc = max(max(b.c0 - pc, pc - b.c1), 0);
                if (__builtin_sqrtf((float)(dr * dr + dc * dc)) >= d) continue;
                int best = INT_MAX;
                for (int q = 0; q < n; ++q) {
                    const uint32_t cell = cells[k][q];
                    const int a = (int)(cell >> 16) - pr, bb = (int)(cell & 0xffffu) - pc;
                    best = min(best, a * a + bb * bb);
                }
                const float dk = __builtin_sqrtf((float)best);
                d = dk < d ? dk : d;
            }
            return d;
        };
        const float xw = poses[3 * p], yw = poses[3 * p + 1], th = poses[3 * p + 2];
        RayResult rr;
        if (LIT) {
            const float aj = (float)j * f.inc;
            rr = literal_cast_dist(m, lp, f.max_range, f.step_coeff, xw, yw, th + (f.amin + aj), dist);
        } else {
            float gx, gy, thg, st, ct;
            world_to_grid(m, xw, yw, th, gx, gy, thg);
            det_sincosf(thg, st, ct);
            const float2 cs = fan_cs[j];
            const float dx = __builtin_fmaf(ct, cs.x, -(st * cs.y));
            const float dy = __builtin_fmaf(st, cs.x, ct * cs.y);
            rr = rm_march_dist(m, f.max_range, f.step_coeff, gx, gy, dx, dy, dist);
        }
        const size_t idx = p * f.num_rays + j;
        float v = rr.range_px * m.res;
        if (f.noise_std > 0.0f) v += fan_noise(f, idx);
        out[idx] = v;
        if (AUX) {
            if (hits) { hits[2 * idx] = rr.hit_c; hits[2 * idx + 1] = rr.hit_r; }
            if (steps) steps[idx] = (uint16_t)(rr.steps > 65535u ? 65535u : rr.steps);
        }
    }
}

}  // namespace scan
