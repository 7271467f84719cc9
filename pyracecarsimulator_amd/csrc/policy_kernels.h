// policy_kernels.h — the steering policy network (rl_policy_*, rl_car_drive_policy; include/scanlib.h): a dense ReLU
// chain over a window of each scan, the MLP of the reference's scripts/policy.py (720 -> 64 -> 128 -> 128 -> 64 -> 1),
// for R scans in one launch, in the project's canonical float32 form (scanlib.h):
//   x_k   = (r <= clip) ? r / scale : 1.0f,  r = scan[in_start + k]        (correctly rounded division)
//   acc_j = +0.0f;  acc_j = fmaf(x_k, W[k][j], acc_j) for k = 0, 1, ..., K-1 in ascending order
//   y_j   = acc_j + b_j;  ReLU: y_j > 0 ? y_j : 0.0f
// No split-K, no tree sums: every output is one k-ordered fmaf chain, so any tiling of cars x neurons gives the same
// bits.
//
// Shape: one wave per workgroup owns PM_CARS cars and runs the whole chain for them.  Each lane holds micro-tiles of
// PM_MC cars x 4 neurons in registers (PM_MC * 4 v_fma_f32 per k for one ds_read of PM_MC activations and one
// 16-byte weight load).  The activations stay in LDS (k-major, [K][PM_CARS], one buffer: a layer's outputs wait in
// registers until every lane has read its inputs); only the steers are written.  Layer 1's 184 KB of weights exceed
// LDS, so every layer's weights are staged in k-blocks of PM_KB rows (at most 16 KB): each lane issues its share of a
// block's loads before its first store, served by L2 (every workgroup reads the same 313 KB in the same order), and
// the k-steps then read LDS.  (Reading the rows straight from L1/L2 inside the k loop, one dependent load per k-step,
// measured ~230 us per launch at any R; staging with a load-wait-store loop ~180 us: latency-bound both.)  Layer 1's inputs come in the same k-blocks straight from the range
// buffer, the input transform fused in.  Zero padding (neurons to a multiple
// of 4, cars to PM_CARS) never enters a kept output's chain.
// policy_mlp_rows_kernel is the same body over a list of scan rows (per-seat drivers, include/scanlib_seats.h: the
// network for the cars it drives); policy_mlp_kernel is the dense form, every row; policy_mlp_pop_kernel the population
// form (include/scanlib_population.h): every workgroup's cars belong to ONE member, whose weight block it reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace scan {

constexpr int PM_MAX_LAYERS = 8;       // caps of rl_policy_create (RL_ERR_UNSUPPORTED beyond them)
constexpr int PM_MAX_IN = 1024;
constexpr int PM_MAX_W = 256;
constexpr int PM_CARS = 8;             // cars per workgroup (one wave)
constexpr int PM_MC = 2;               // cars per lane micro-tile
constexpr int PM_KB = 16;              // k-block: weight rows (every layer) and inputs (layer 1) staged in LDS
constexpr int PM_MT = (PM_CARS / PM_MC) * (PM_MAX_W / 4) / 64;   // micro-tiles per lane at the widest layer

struct PolicyParams {
    int n_layers;
    int dims[PM_MAX_LAYERS + 1];       // dims[0] = input width, dims[n_layers] = 1
    const float *W[PM_MAX_LAYERS];     // [dims[l]][ceil4(dims[l+1])] row-major, zero-padded columns
    const float *b[PM_MAX_LAYERS];     // [ceil4(dims[l+1])], zero-padded
    uint32_t relu;                     // bit l: layer l ends in a ReLU
    int in_start;
    float clip, scale;
};

__device__ inline float policy_input(float r, float clip, float scale)
{
    return (r <= clip) ? r / scale : 1.0f;      // NaN and +inf: 1.0 (scripts/policy.py's `x if x <= 15.0 else 15.0`)
}

// The chain for the workgroup's cars car0 ... car0 + PM_CARS - 1 of a segment of n cars.  ROWS_FORM false: car i is scan
// row row0 + i.  ROWS_FORM true: car i is scan row rows[i] (any order, each row once) and its answer goes to
// out[rows[i]]: the network for the cars it drives and no others.  A car's chain reads its own scan row and the weights
// only, so the forms give a row the same bits.  The dense and the rows form have one segment, the launch (row0 = 0,
// w_off = 0); the population form one per member: its E cars, rows first at row0, weights w_off floats into the block.
// The padding clamp and the store guard stay inside the segment: a padding lane never touches the next member's row.
template <bool ROWS_FORM>
__device__ __forceinline__ void policy_mlp_body(const PolicyParams &p, size_t w_off, const float *__restrict__ scans,
                                                const int *__restrict__ rows, int row0, int car0, int n, int size,
                                                float *__restrict__ out)
{
    __shared__ float xin[PM_KB * PM_CARS];
    __shared__ float act[PM_MAX_W * PM_CARS];
    __shared__ float4 wl[PM_KB * (PM_MAX_W / 4)];
    const int lane = threadIdx.x;
    constexpr int CG = PM_CARS / PM_MC;
    int srow[PM_CARS];                         // the scan row of each of the workgroup's cars (padding: the last car's)
#pragma unroll
    for (int c = 0; c < PM_CARS; ++c) {
        const int i = min(car0 + c, n - 1);
        srow[c] = ROWS_FORM ? rows[i] : row0 + i;
    }
    for (int l = 0; l < p.n_layers; ++l) {
        const int K = p.dims[l], N = p.dims[l + 1], ng = (N + 3) >> 2, n_mt = CG * ng;
        const float4 *__restrict__ W4 = reinterpret_cast<const float4 *>(p.W[l] + w_off);
        int jg[PM_MT], cg[PM_MT];
        float acc[PM_MT][PM_MC][4];
#pragma unroll
        for (int m = 0; m < PM_MT; ++m) {
            const int mt = lane + 64 * m;
            jg[m] = mt % ng;                   // neighbouring lanes: neighbouring neuron groups (conflict-free LDS rows)
            cg[m] = mt / ng;
#pragma unroll
            for (int i = 0; i < PM_MC; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[m][i][j] = 0.0f;
        }
        for (int kb = 0; kb < K; kb += PM_KB) {
            const int kn = min(PM_KB, K - kb);
            __syncthreads();                   // (every lane is done with the previous block's wl / xin)
            // the block's weight rows and inputs: every load issued before the first store (one latency per block)
            // (indices clamped into the block, not branched on: the loads stay unconditional and back to back)
            const int ne = kn * ng;
            float4 wv[PM_KB];
#pragma unroll
            for (int u = 0; u < PM_KB; ++u) wv[u] = W4[(size_t)kb * ng + min(lane + 64 * u, ne - 1)];
            float xv[PM_CARS];
            if (l == 0) {
                const int kk = p.in_start + kb + min(lane, kn - 1);
#pragma unroll
                for (int c = 0; c < PM_CARS; ++c) xv[c] = scans[(size_t)srow[c] * size + kk];
            }
#pragma unroll
            for (int u = 0; u < PM_KB; ++u) wl[lane + 64 * u] = wv[u];    // (entries past ne: never read)
            if (l == 0 && lane < kn) {
#pragma unroll
                for (int c = 0; c < PM_CARS; ++c)
                    xin[lane * PM_CARS + c] = car0 + c < n ? policy_input(xv[c], p.clip, p.scale) : 0.0f;
            }
            __syncthreads();
            const float *src = l == 0 ? xin : act + kb * PM_CARS;
            for (int k = 0; k < kn; ++k) {
#pragma unroll
                for (int m = 0; m < PM_MT; ++m) {
                    if (lane + 64 * m < n_mt) {
                        const float *a = src + k * PM_CARS + cg[m] * PM_MC;
                        const float4 w = wl[k * ng + jg[m]];
#pragma unroll
                        for (int i = 0; i < PM_MC; ++i) {
                            const float x = a[i];
                            acc[m][i][0] = fmaf(x, w.x, acc[m][i][0]);
                            acc[m][i][1] = fmaf(x, w.y, acc[m][i][1]);
                            acc[m][i][2] = fmaf(x, w.z, acc[m][i][2]);
                            acc[m][i][3] = fmaf(x, w.w, acc[m][i][3]);
                        }
                    }
                }
            }
        }
        const bool relu = (p.relu >> l) & 1u, last = l == p.n_layers - 1;
        const float4 *B4 = reinterpret_cast<const float4 *>(p.b[l] + w_off);
        if (!last) __syncthreads();            // every lane is done reading act: the outputs overwrite it in place
#pragma unroll
        for (int m = 0; m < PM_MT; ++m) {
            if (lane + 64 * m >= n_mt) continue;
            const float4 bv = B4[jg[m]];
            const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
            for (int i = 0; i < PM_MC; ++i) {
                const int c = cg[m] * PM_MC + i;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float y = acc[m][i][j] + bb[j];
                    if (relu) y = y > 0.0f ? y : 0.0f;
                    if (last) {
                        if (jg[m] == 0 && j == 0 && car0 + c < n) out[ROWS_FORM ? srow[c] : row0 + car0 + c] = y;
                    } else {
                        act[(4 * jg[m] + j) * PM_CARS + c] = y;
                    }
                }
            }
        }
        if (!last) __syncthreads();
    }
}

// scans [n][size] (row stride `size`) -> out [n]
__global__ __launch_bounds__(64) void policy_mlp_kernel(PolicyParams p, const float *__restrict__ scans, int n, int size,
                                                        float *__restrict__ out)
{
    policy_mlp_body<false>(p, 0, scans, nullptr, 0, blockIdx.x * PM_CARS, n, size, out);
}

// the row-indexed form: rows [n] names the scan rows (of stride `size`) the network answers -> out [rows[i]]; the
// other rows of out are left alone
__global__ __launch_bounds__(64) void policy_mlp_rows_kernel(PolicyParams p, const float *__restrict__ scans,
                                                             const int *__restrict__ rows, int n, int size,
                                                             float *__restrict__ out)
{
    policy_mlp_body<true>(p, 0, scans, rows, 0, blockIdx.x * PM_CARS, n, size, out);
}

// ---------------------------------------------------------------- populations (include/scanlib_population.h)
// the flat parameter vector theta of a member against the padded block: per layer, where W starts in theta (b follows
// its K N values) and where W and b start in the block
struct PopLayout {
    int n_layers;
    int dims[PM_MAX_LAYERS + 1];
    int theta_off[PM_MAX_LAYERS + 1];  // theta_off[n_layers] = P
    int w_off[PM_MAX_LAYERS], b_off[PM_MAX_LAYERS];
};

// the population form: scans [n E][size] -> out [n E]; workgroup (m, chunk) of the n x wg_per_member grid answers cars
// chunk PM_CARS ... of member first + m, rows m E + ..., with the weights at `stride` floats a member (a multiple of 4:
// every float4 load stays 16-byte aligned)
__global__ __launch_bounds__(64) void policy_mlp_pop_kernel(PolicyParams p, size_t stride, int first, int wg_per_member,
                                                            int E, const float *__restrict__ scans, int size,
                                                            float *__restrict__ out)
{
    const int m = blockIdx.x / wg_per_member, chunk = blockIdx.x - m * wg_per_member;
    policy_mlp_body<false>(p, (size_t)(first + m) * stride, scans, nullptr, m * E, chunk * PM_CARS, E, size, out);
}

// theta [n][P] -> the padded blocks of members first ... first + n - 1: one thread per parameter; the padding columns
// (zeroed by create) are never written
__global__ __launch_bounds__(256) void policy_pop_pack_kernel(PopLayout L, const float *__restrict__ theta, int first, int n,
                                                              size_t stride, float *__restrict__ weights)
{
    const int P = L.theta_off[L.n_layers];
    const size_t total = (size_t)n * P;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int m = (int)(e / P), q = (int)(e - (size_t)m * P);
        int l = 0;
#pragma unroll
        for (int i = 1; i < PM_MAX_LAYERS; ++i)
            if (i < L.n_layers && q >= L.theta_off[i]) l = i;
        int K = L.dims[0], N = L.dims[1], t0 = L.theta_off[0], wo = L.w_off[0], bo = L.b_off[0];
#pragma unroll
        for (int i = 1; i < PM_MAX_LAYERS; ++i)        // (a select chain: no lane-indexed read of the argument arrays)
            if (l == i) K = L.dims[i], N = L.dims[i + 1], t0 = L.theta_off[i], wo = L.w_off[i], bo = L.b_off[i];
        const int idx = q - t0, Np = (N + 3) & ~3;
        const int dst = idx < K * N ? wo + (idx / N) * Np + idx % N : bo + idx - K * N;
        weights[(size_t)(first + m) * stride + dst] = theta[e];
    }
}

// fitness [n][2] of a population roll-out: one lane per member, a serial f64 sum over its E cars in ascending order
// (travel_dist now less travel_dist at the start) and the count of its crashed cars
__global__ __launch_bounds__(64) void policy_pop_fitness_kernel(const double *__restrict__ states, const double *__restrict__ states0,
                                                                const int *__restrict__ first_crashed, int n, int E,
                                                                double *__restrict__ fitness)
{
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= n) return;
    double sum = 0.0;
    int crashed = 0;
    for (int e = 0; e < E; ++e) {
        const size_t r = (size_t)m * E + e;
        sum = sum + (states[r * 11 + 8] - states0[r * 11 + 8]);
        crashed += first_crashed[r] >= 0;
    }
    fitness[2 * (size_t)m] = sum;
    fitness[2 * (size_t)m + 1] = (double)crashed;
}

}  // namespace scan
