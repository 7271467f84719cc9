// mcl_kernels.h — particle-filter localisation (include/scanlib.h "particle-filter localisation"): what one
// Monte-Carlo-localisation update does around the fused weight call of pf_kernels.h, so that T updates run back to back
// on one stream with nothing read on the host in between.  Per step:
//   mcl_motion_kernel     odometry in the car frame + the twelve-uniform normal per axis -> X' (f64) and q = (float) X'
//   (launch_pf_weights)   L[p], the fused repeat-angle scan + sensor model of q
//   mcl_weight_kernel     omega = w L and the sequential total of every chunk of 256
//   mcl_norm_kernel       W = the sequential sum of the chunk totals, w = omega / W (or 1 / P: degenerate), the six chunk
//                         totals of the estimate (w, w^2, w x', w y', w c, w s) and the inclusive in-chunk sums of w
//   mcl_base_kernel       six waves: the chunk bases of cum(w), neff, the estimate, the resample decision (a device flag)
//   mcl_resample_kernel   cum = base + in-chunk sum, the systematic-resampling ancestor by binary search, the gather
// Every sum is taken in the order the contract pins (a chunk ascending, then the chunk totals ascending) by ONE lane per
// sum: any other order gives other bits (tests/test_mcl_host.py's order witness).  Every operation is a separately
// rounded IEEE double (the library is built with -ffp-contract=off).
#pragma once
#include "scan_device.h"

namespace scan {

constexpr int MCL_WG = 256;                    // lanes per workgroup of the per-particle kernels
constexpr int MCL_CHUNK = 256;                 // particles per chunk of the blocked sums (the contract's)
constexpr int MCL_MAX_PARTICLES = 1 << 20;
constexpr int MCL_MAX_CHUNKS = MCL_MAX_PARTICLES / MCL_CHUNK;      // totals one lane sums: at most 4096
constexpr int MCL_GROUP = 8;                   // chunks per workgroup of mcl_weight_kernel
constexpr int MCL_NGROUP = 4;                  // chunks per workgroup of mcl_norm_kernel (six LDS rows per chunk: 48 KiB)
constexpr int MCL_SUMS = 6;                    // w, w^2, w x', w y', w c, w s
static_assert(5 * MCL_NGROUP * (MCL_CHUNK + 1) >= MCL_MAX_CHUNKS, "mcl_norm_kernel stages the chunk totals in its value rows");
constexpr int MCL_BASE_TILE = 512;             // chunk totals a wave of mcl_base_kernel stages per round
constexpr int MCL_LDS_ROW = MCL_CHUNK + 1;     // odd row stride: the summing lanes walk their rows side by side

enum { MCL_RESAMPLED = 1, MCL_DEGENERATE = 2 };     // bits of a step's flags

struct MclParams {
    int n_particles, n_chunks;
    double inv_p;                  // 1.0 / (double)P
    double std[3];                 // motion noise per axis; 0: the axis draws nothing
    double resample_below;         // resample_ratio * (double)P
    uint32_t key;                  // noise_key(seed)
};

// Probabilistic Robotics, Table 5.4: twelve uniforms summed ascending from 0.0, minus 6.0 — a unit normal (to +-6) whose
// bits the host reproduces, which a log / cos Box-Muller on hardware estimates does not give
__device__ __forceinline__ double mcl_normal12(uint32_t key, uint32_t p, uint32_t first)
{
    double s = 0.0;
    for (uint32_t k = 0; k < 12u; ++k) s += mcts_uniform01(key, p, first + k);
    return s - 6.0;
}

// ---- 1. motion and pose cast.  odom: this step's (dx, dy, dtheta) in the car frame; draws at counter (p, 64 t + 1 + 12 a + k)
__global__ __launch_bounds__(MCL_WG) void mcl_motion_kernel(MclParams mp, const double *__restrict__ odom, uint32_t t,
                                                            const double *__restrict__ cur, double *__restrict__ prop,
                                                            float *__restrict__ q)
{
    const int p = blockIdx.x * MCL_WG + threadIdx.x;
    if (p >= mp.n_particles) return;
    const double x = cur[3 * (size_t)p], y = cur[3 * (size_t)p + 1], th = cur[3 * (size_t)p + 2];
    const double dx = odom[0], dy = odom[1], dth = odom[2];
    float sf, cf;
    det_sincosf((float)th, sf, cf);
    const double s = (double)sf, c = (double)cf;
    double nx = x + (c * dx - s * dy);
    double ny = y + (s * dx + c * dy);
    double nth = th + dth;
    const uint32_t first = 64u * t + 1u;
    if (mp.std[0] > 0.0) nx = nx + mp.std[0] * mcl_normal12(mp.key, (uint32_t)p, first);
    if (mp.std[1] > 0.0) ny = ny + mp.std[1] * mcl_normal12(mp.key, (uint32_t)p, first + 12u);
    if (mp.std[2] > 0.0) nth = nth + mp.std[2] * mcl_normal12(mp.key, (uint32_t)p, first + 24u);
    prop[3 * (size_t)p] = nx;
    prop[3 * (size_t)p + 1] = ny;
    prop[3 * (size_t)p + 2] = nth;
    q[3 * (size_t)p] = (float)nx;
    q[3 * (size_t)p + 1] = (float)ny;
    q[3 * (size_t)p + 2] = (float)nth;
}

// particles of chunk b
__device__ __forceinline__ int mcl_chunk_len(int n_particles, int b)
{
    const int left = n_particles - b * MCL_CHUNK;
    return left < MCL_CHUNK ? left : MCL_CHUNK;
}

// ---- 3. omega = w L, and T_b(omega): a workgroup stages MCL_GROUP chunks in LDS, one lane per chunk sums it ascending
__global__ __launch_bounds__(MCL_WG) void mcl_weight_kernel(MclParams mp, const double *__restrict__ w,
                                                            const double *__restrict__ lik, double *__restrict__ omega,
                                                            double *__restrict__ tot)
{
    __shared__ double row[MCL_GROUP][MCL_LDS_ROW];
    const int b0 = blockIdx.x * MCL_GROUP;
    for (int e = 0; e < MCL_GROUP; ++e) {
        const long i = (long)(b0 + e) * MCL_CHUNK + threadIdx.x;
        double v = 0.0;
        if (i < mp.n_particles) {
            v = w[i] * lik[i];
            omega[i] = v;
        }
        row[e][threadIdx.x] = v;
    }
    __syncthreads();
    const int b = b0 + (int)threadIdx.x;
    if ((int)threadIdx.x < MCL_GROUP && b < mp.n_chunks) {
        const int n = mcl_chunk_len(mp.n_particles, b);
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += row[threadIdx.x][i];
        tot[b] = s;
    }
}

// ---- 4. normalise, the estimate's chunk totals, the in-chunk sums of w.
// Lane 0 of every workgroup sums the chunk totals of omega (at most 4096 adds, the same in every workgroup: one fewer
// launch and grid-wide wait than a kernel of its own).  Then 6 lanes per chunk, one per sum, walk the chunk in LDS.
// scal[0] = W (block 0 writes it for mcl_base_kernel).  tot6: [MCL_SUMS][n_chunks].
__global__ __launch_bounds__(MCL_WG) void mcl_norm_kernel(MclParams mp, const double *__restrict__ tot_omega,
                                                          const double *__restrict__ omega,
                                                          const double *__restrict__ prop, double *__restrict__ w,
                                                          double *__restrict__ part, double *__restrict__ tot6,
                                                          double *__restrict__ scal)
{
    __shared__ double val[5][MCL_NGROUP][MCL_LDS_ROW];        // w, x', y', c, s
    __shared__ double inc[MCL_NGROUP][MCL_LDS_ROW];           // inclusive sums of w inside the chunk
    __shared__ double w_total;
    double *stage = &val[0][0][0];                            // (the totals pass through LDS: one lane's 4096 dependent
    for (int b = threadIdx.x; b < mp.n_chunks; b += MCL_WG)   //  adds then wait on LDS, not on a global load each)
        stage[b] = tot_omega[b];
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < mp.n_chunks; ++b) s += stage[b];
        w_total = s;
        if (blockIdx.x == 0) scal[0] = s;
    }
    __syncthreads();
    const double W = w_total;
    const bool degenerate = !(W > 0.0) || W == __builtin_huge_val();
    const int b0 = blockIdx.x * MCL_NGROUP;
    for (int e = 0; e < MCL_NGROUP; ++e) {
        const long i = (long)(b0 + e) * MCL_CHUNK + threadIdx.x;
        if (i < mp.n_particles) {
            const double wn = degenerate ? mp.inv_p : omega[i] / W;
            w[i] = wn;
            float sf, cf;
            det_sincosf((float)prop[3 * i + 2], sf, cf);
            val[0][e][threadIdx.x] = wn;
            val[1][e][threadIdx.x] = prop[3 * i];
            val[2][e][threadIdx.x] = prop[3 * i + 1];
            val[3][e][threadIdx.x] = (double)cf;
            val[4][e][threadIdx.x] = (double)sf;
        }
    }
    __syncthreads();
    const int e = (int)threadIdx.x / MCL_SUMS, k = (int)threadIdx.x % MCL_SUMS, b = b0 + e;
    if ((int)threadIdx.x < MCL_NGROUP * MCL_SUMS && b < mp.n_chunks) {
        const int n = mcl_chunk_len(mp.n_particles, b);
        const double *other = val[k >= 2 ? k - 1 : 0][e];
        double s = 0.0;
        for (int i = 0; i < n; ++i) {
            const double wn = val[0][e][i];
            s += k == 0 ? wn : wn * other[i];
            if (k == 0) inc[e][i] = s;
        }
        tot6[(size_t)k * mp.n_chunks + b] = s;
    }
    __syncthreads();
    for (int e2 = 0; e2 < MCL_NGROUP; ++e2) {
        const long i = (long)(b0 + e2) * MCL_CHUNK + threadIdx.x;
        if (i < mp.n_particles) part[i] = inc[e2][threadIdx.x];
    }
}

// ---- 5. six waves, one per sequence of chunk totals: waves 0..4 sum those of w^2, w x', w y', w c, w s, wave 5 turns
// the totals of w into the chunk bases of cum(w).  A wave stages MCL_BASE_TILE totals in LDS, its lane 0 adds them in
// order.  Thread 0 then writes the step's neff, estimate and flags: the resample decision stays on the device
__global__ __launch_bounds__(64 * MCL_SUMS) void mcl_base_kernel(MclParams mp, const double *__restrict__ tot6,
                                                                 const double *__restrict__ scal, double *__restrict__ base,
                                                                 double *__restrict__ est, double *__restrict__ neff,
                                                                 int *__restrict__ flags)
{
    __shared__ double tile[MCL_SUMS][MCL_BASE_TILE];
    __shared__ double r[MCL_SUMS];
    const int k = (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
    const double *v = tot6 + (size_t)(k == MCL_SUMS - 1 ? 0 : k + 1) * mp.n_chunks;
    double s = 0.0;
    for (int b0 = 0; b0 < mp.n_chunks; b0 += MCL_BASE_TILE) {
        const int n = mp.n_chunks - b0 < MCL_BASE_TILE ? mp.n_chunks - b0 : MCL_BASE_TILE;
        for (int i = lane; i < n; i += 64) tile[k][i] = v[b0 + i];
        __syncthreads();
        if (lane == 0) {
            for (int i = 0; i < n; ++i) {
                const double x = tile[k][i];
                if (k == MCL_SUMS - 1) tile[k][i] = s;
                s += x;
            }
        }
        __syncthreads();
        if (k == MCL_SUMS - 1)
            for (int i = lane; i < n; i += 64) base[b0 + i] = tile[k][i];
        __syncthreads();
    }
    if (lane == 0) r[k] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double W = scal[0];
        const double ne = 1.0 / r[0];
        neff[0] = ne;
        est[0] = r[1];
        est[1] = r[2];
        est[2] = r[3];
        est[3] = r[4];
        int fl = (!(W > 0.0) || W == __builtin_huge_val()) ? MCL_DEGENERATE : 0;
        if (ne < mp.resample_below) fl |= MCL_RESAMPLED;
        flags[0] = fl;
    }
}

// cum(w)[i] = B_b + s_i
__device__ __forceinline__ double mcl_cum_at(const double *__restrict__ base, const double *__restrict__ part, int i)
{
    return base[i / MCL_CHUNK] + part[i];
}

// ---- 6. cum, the ancestor and the gather.  flags: this step's (bit 0 decides); the draw is U(0, 64 t).
// a_i = min(P - 1, #{k : c[k] <= tau_i}), tau_i = ((u + i) / P) S — c is non-decreasing for non-negative weights, so the
// count is an upper bound found by bisection
__global__ __launch_bounds__(MCL_WG) void mcl_resample_kernel(MclParams mp, uint32_t t, const int *__restrict__ flags,
                                                              const double *__restrict__ base,
                                                              const double *__restrict__ part,
                                                              const double *__restrict__ prop, double *__restrict__ cur,
                                                              double *__restrict__ w, int32_t *__restrict__ anc,
                                                              double *__restrict__ cum)
{
    const int i = blockIdx.x * MCL_WG + threadIdx.x;
    const int P = mp.n_particles;
    if (i >= P) return;
    cum[i] = mcl_cum_at(base, part, i);
    int a = i;
    if (flags[0] & MCL_RESAMPLED) {
        const double S = mcl_cum_at(base, part, P - 1);
        const double u = mcts_uniform01(mp.key, 0u, 64u * t);
        const double tau = ((u + (double)i) / (double)P) * S;
        int lo = 0, hi = P;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (mcl_cum_at(base, part, mid) <= tau) lo = mid + 1;
            else hi = mid;
        }
        a = lo < P - 1 ? lo : P - 1;
        w[i] = mp.inv_p;
    }
    anc[i] = a;
    cur[3 * (size_t)i] = prop[3 * (size_t)a];
    cur[3 * (size_t)i + 1] = prop[3 * (size_t)a + 1];
    cur[3 * (size_t)i + 2] = prop[3 * (size_t)a + 2];
}

}  // namespace scan
