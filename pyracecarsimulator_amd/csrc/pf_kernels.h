// pf_kernels.h — particle-filter weights (include/scanlib.h "particle-filter weights"): range_libc's
// calc_range_repeat_angles / eval_sensor_model / calc_range_repeat_angles_eval_sensor_model, the calls of a Monte-Carlo
// localisation update.  Every particle casts the SAME A beam angles (an arbitrary float32 table, not a fan), and what the
// caller wants back is one float64 weight per particle: the ordered product of A sensor-model entries.
//   pf_angles_kernel<KIND, AUX>   the plain repeat-angle scan, one ray per lane
//   pf_weight_kernel<LIT>         march + sensor-model lookup + ordered product in one launch: ranges, hit cells and
//                                 factors never reach global memory, the only global write is 8 B per particle
//   pf_eval_kernel                the same staging and product on ranges already in memory
// Each kind keeps the arithmetic of its fan kernel with fan_alpha(f, j) replaced by angles[j] (rm_fan_kernel,
// rm_literal_kernel, cddt_fan_kernel, lut_fan_kernel), so a repeat-angle scan of the fan's own angles is the fan,
// bit for bit.
#pragma once
#include "scan_device.h"
#include "scan_params.h"
#include "rm_kernels.h"
#include "lut_kernels.h"
#include "cddt_kernels.h"
#include "literal_kernels.h"

namespace scan {

constexpr int PF_WG = 256;                 // lanes per workgroup of the three kernels
constexpr int PF_MAX_ANGLES = 2048;        // beams per particle: tables + one particle's factors stay below 64 KiB of LDS
constexpr int PF_MAX_WIDTH = 2048;         // sensor-model table side
constexpr int PF_TILE_RAYS = 2048;         // rays a workgroup marches between two barriers (8 per lane)

enum { PF_RM = 0, PF_RM_LITERAL = 1, PF_CDDT = 2, PF_LUT = 3, PF_LUT_REFINE = 4 };      // (4: handle option lut_refine)
static inline bool pf_table_kind(int kind) { return kind == PF_CDDT || kind == PF_LUT || kind == PF_LUT_REFINE; }

struct PfParams {
    int n_particles, n_angles;
    int block;                 // particles per tile (pf_block)
    const double *table;       // sensor model, width x width, row = observed bin, column = expected bin
    int width;
    float top;                 // (float)(width - 1)
};

// particles per tile: about PF_TILE_RAYS rays, at most one product lane per particle
static inline int pf_block(int n_particles, int n_angles)
{
    int b = (PF_TILE_RAYS + n_angles - 1) / n_angles;
    if (b > PF_WG) b = PF_WG;
    if (b > n_particles) b = n_particles;
    return b < 1 ? 1 : b;
}
// factor rows are padded to an odd number of doubles: the product lanes walk their rows side by side
static inline __host__ __device__ int pf_row_stride(int n_angles) { return n_angles | 1; }
static inline size_t pf_lds_bytes(int block, int n_angles)
{
    return (size_t)block * pf_row_stride(n_angles) * sizeof(double) + (size_t)block * sizeof(float4) +
           (size_t)n_angles * (sizeof(float2) + sizeof(int));
}

// the sensor model's bin of a range in metres.  NaN -> bin 0 (fmaxf returns its other argument)
__device__ __forceinline__ int pf_bin(float v, float inv_res, float top)
{
    return (int)__builtin_fminf(__builtin_fmaxf(v * inv_res, 0.0f), top);
}

// one ray of a particle by kind; (px, py, pth): the world pose for PF_RM_LITERAL, else (gx, gy, thg).  The marching kinds
// return cells in range_px, the table kinds their finished metres (cddt_query and the GiantLUT entry are scaled by the
// resolution where they are read, as in their fan kernels): pf_value tells them apart
template <int KIND>
__device__ __forceinline__ RayResult pf_cast(const MapParams &m, const FanParams &f, const LiteralParams &lt,
                                             const CddtParams &cp, const LutParams &lp, float px, float py, float pth,
                                             float a)
{
    RayResult rr;
    rr.hit_c = -1;
    rr.hit_r = -1;
    rr.steps = 0;
    if (KIND == PF_RM) {
        float sa, ca, st, ct;
        det_sincosf(a, sa, ca);
        det_sincosf(pth, st, ct);
        const float dx = __builtin_fmaf(ct, ca, -(st * sa));
        const float dy = __builtin_fmaf(st, ca, ct * sa);
        return rm_march(m, f.max_range, f.step_coeff, px, py, dx, dy);
    } else if (KIND == PF_RM_LITERAL) {
        return literal_cast(m, lt, f.max_range, f.step_coeff, px, py, pth + a);
    } else if (KIND == PF_CDDT) {
        rr.range_px = cddt_query(m, cp, f.max_range, px, py, pth + a);
        return rr;
    } else if (KIND == PF_LUT) {
        const float td_f = (float)lp.theta_disc, inv_td = 1.0f / (float)lp.theta_disc;
        rr.range_px = f.max_range * m.res;
        if (px >= 0.0f && px < m.fcols && py >= 0.0f && py < m.frows)
            rr.range_px = (float)lp.lut[((size_t)(int)py * m.cols + (int)px) * lp.theta_disc +
                                        lut_bin_fast(pth + a, lp, td_f, inv_td)] * lp.dequant * m.res;
        return rr;
    } else {
        // the origin-corrected query (lut_kernels.h): the refined fan's arithmetic with angles[j] for fan_alpha(f, j)
        const float td_f = (float)lp.theta_disc, inv_td = 1.0f / (float)lp.theta_disc;
        rr.range_px = f.max_range * m.res;
        if (px >= 0.0f && px < m.fcols && py >= 0.0f && py < m.frows) {
            LutOrigin o;
            float sa, ca;
            const int cell = lut_origin_cell(m, px, py, m.dt[lut_nearest_cell(m, px, py)], o.fx, o.fy);
            det_sincosf(pth, o.st, o.ct);
            det_sincosf(a, sa, ca);
            rr.range_px = lut_refined_px(lp.lut[(size_t)cell * lp.theta_disc + lut_bin_fast(pth + a, lp, td_f, inv_td)],
                                         lp.dequant, f.max_range, o, sa, ca) * m.res;
        }
        return rr;
    }
}

// the float32 value a scan stores for global ray i: metres, plus the handle's noise
template <int KIND>
__device__ __forceinline__ float pf_value(const MapParams &m, const FanParams &f, const RayResult &rr, uint64_t i)
{
    float v = (KIND == PF_RM || KIND == PF_RM_LITERAL) ? rr.range_px * m.res : rr.range_px;
    if (f.noise_std > 0.0f) v += fan_noise(f, i);      // (the generator call the literal and race kernels share)
    return v;
}

// ------------------------------------------------------------------------------
// the plain repeat-angle scan: out[p * A + j] = range of particle p at theta_p + angles[j]
// ------------------------------------------------------------------------------
template <int KIND, bool AUX>
__global__ __launch_bounds__(PF_WG) void pf_angles_kernel(MapParams m, FanParams f, LiteralParams lt, CddtParams cp,
                                                          LutParams lp, const float *__restrict__ poses,
                                                          const float *__restrict__ angles, long n_rays,
                                                          float *__restrict__ out, int32_t *__restrict__ hits,
                                                          uint16_t *__restrict__ steps)
{
    const long stride = (long)gridDim.x * PF_WG;
    for (long i = (long)blockIdx.x * PF_WG + threadIdx.x; i < n_rays; i += stride) {
        const long p = i / f.num_rays;
        const int j = (int)(i - p * f.num_rays);
        float px = poses[3 * p], py = poses[3 * p + 1], pth = poses[3 * p + 2];
        if (KIND != PF_RM_LITERAL) world_to_grid(m, px, py, pth, px, py, pth);
        const RayResult rr = pf_cast<KIND>(m, f, lt, cp, lp, px, py, pth, angles[j]);
        out[i] = pf_value<KIND>(m, f, rr, (uint64_t)i);
        if (AUX) {
            if (hits) { hits[2 * i] = rr.hit_c; hits[2 * i + 1] = rr.hit_r; }
            if (steps) steps[i] = (uint16_t)(rr.steps > 65535u ? 65535u : rr.steps);
        }
    }
}

// ------------------------------------------------------------------------------
// weights.  A workgroup stages the beam table — (cos, sin) of angles[j], or the raw angle for the literal form — and the
// observed-row offsets bin(obs[j]) * width once, then takes tiles of `block` particles: one ray per lane over the
// tile's block * A rays, the factor T[obs row + bin(range)] parked as a double at [particle][j]; after a barrier one
// lane per particle multiplies its row in ascending j, every product its own IEEE rounding.
// SRC 0: march canonically, 1: march literally, 2: read the range from `ranges`.
// ------------------------------------------------------------------------------
template <int SRC>
__device__ __forceinline__ void pf_weights_body(const MapParams &m, const FanParams &f, const LiteralParams &lt,
                                                const PfParams &pp, const float *__restrict__ poses,
                                                const float *__restrict__ angles, const float *__restrict__ obs,
                                                const float *__restrict__ ranges, double *__restrict__ weights)
{
    extern __shared__ float4 pf_lds[];
    const int A = pp.n_angles, AS = pf_row_stride(A), PB = pp.block;
    float4 *pose = pf_lds;                                          // [PB]  (16-B records first: every part stays aligned)
    double *fac = reinterpret_cast<double *>(pose + PB);            // [PB][AS]
    float2 *beam = reinterpret_cast<float2 *>(fac + (size_t)PB * AS);   // [A]
    int *orow = reinterpret_cast<int *>(beam + A);                  // [A]
    for (int j = threadIdx.x; j < A; j += PF_WG) {
        if (SRC == 0) {
            float s, c;
            det_sincosf(angles[j], s, c);
            beam[j] = make_float2(c, s);
        } else if (SRC == 1) {
            beam[j] = make_float2(angles[j], 0.0f);
        }
        orow[j] = pf_bin(obs[j], m.inv_res, pp.top) * pp.width;
    }
    const int n_tiles = (pp.n_particles + PB - 1) / PB;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int p0 = tile * PB;
        const int np = min(PB, pp.n_particles - p0);
        if (SRC != 2 && (int)threadIdx.x < np) {
            const size_t p = (size_t)(p0 + threadIdx.x);
            float px = poses[3 * p], py = poses[3 * p + 1], pth = poses[3 * p + 2], st = 0.0f, ct = 0.0f;
            if (SRC == 0) {
                world_to_grid(m, px, py, pth, px, py, pth);
                det_sincosf(pth, st, ct);
                pose[threadIdx.x] = make_float4(px, py, ct, st);
            } else {
                pose[threadIdx.x] = make_float4(px, py, pth, 0.0f);
            }
        }
        __syncthreads();          // tables and this tile's poses are in place; the last tile's products have been formed
        const int n_tile_rays = np * A;
        for (int i = threadIdx.x; i < n_tile_rays; i += PF_WG) {
            const int p = i / A, j = i - p * A;
            const uint64_t ray = (uint64_t)(p0 + p) * (uint64_t)A + (uint64_t)j;
            float v;
            if (SRC == 2) {
                v = ranges[ray];
            } else {
                const float4 q = pose[p];
                const float2 b = beam[j];
                RayResult rr;
                if (SRC == 0) {
                    const float dx = __builtin_fmaf(q.z, b.x, -(q.w * b.y));
                    const float dy = __builtin_fmaf(q.w, b.x, q.z * b.y);
                    rr = rm_march(m, f.max_range, f.step_coeff, q.x, q.y, dx, dy);
                } else {
                    rr = literal_cast(m, lt, f.max_range, f.step_coeff, q.x, q.y, q.z + b.x);
                }
                v = pf_value<PF_RM>(m, f, rr, ray);
            }
            fac[(size_t)p * AS + j] = pp.table[orow[j] + pf_bin(v, m.inv_res, pp.top)];
        }
        __syncthreads();
        if ((int)threadIdx.x < np) {
            const double *row = fac + (size_t)threadIdx.x * AS;
            double w = 1.0;
            for (int j = 0; j < A; ++j) w *= row[j];
            weights[p0 + threadIdx.x] = w;
        }
    }
}

template <bool LIT>
__global__ __launch_bounds__(PF_WG) void pf_weight_kernel(MapParams m, FanParams f, LiteralParams lt, PfParams pp,
                                                          const float *__restrict__ poses,
                                                          const float *__restrict__ angles,
                                                          const float *__restrict__ obs, double *__restrict__ weights)
{
    pf_weights_body<LIT ? 1 : 0>(m, f, lt, pp, poses, angles, obs, nullptr, weights);
}

__global__ __launch_bounds__(PF_WG) void pf_eval_kernel(MapParams m, PfParams pp, const float *__restrict__ obs,
                                                        const float *__restrict__ ranges, double *__restrict__ weights)
{
    const FanParams no_f{};
    const LiteralParams no_lt{};
    pf_weights_body<2>(m, no_f, no_lt, pp, nullptr, nullptr, obs, ranges, weights);
}

}  // namespace scan
