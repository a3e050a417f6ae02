// Importance-sampling error (include/plnerf_hip_sampleerr.h): test_images_samples of
// depth_supervised_exps/run_nerf_sample_based_depth.py:396-411 -- per ray the mean over the N hypotheses of
// |pred_hyp - depth_map|, summed over the valid rays with their count -- one launch over groups of rays, one over the
// groups.
//
// Group: PLNERF_SAMPLEERR_RAYS_PER_GROUP rays per workgroup of 4 waves.  The group's depths and valid flags go to LDS;
// its hypotheses are the contiguous span pred_hyp[r0*N .. (r0+64)*N), which the 256 lanes sweep in order, 16 B per lane
// when N % 4 == 0 and the pointer is 16-B aligned (4 B otherwise), 4 loads in flight per lane.  A lane's element moves by
// 256*VEC floats per step, so its ray and column advance by fixed amounts (one carry) with no division in the loop.
// Every counted (r, k) adds |h - d| in fp64 (the difference of two fp32 values is exact there); N is the same for every
// ray, so the 1/N of the per-ray mean is applied once, to the total.  Lanes by a fixed butterfly, waves in order, the
// groups in order in sample_error_reduce_kernel: no atomics, the row's bits do not depend on timing.
#include "common.h"
#include "../../include/plnerf_hip_sampleerr.h"

namespace {

constexpr int G = PLNERF_SAMPLEERR_RAYS_PER_GROUP, K = PLNERF_SAMPLEERR_ROW;
constexpr int THREADS = 256, WAVES = THREADS / 64, UNROLL = 4;
static_assert(G <= THREADS, "one thread per ray stages the group");

__device__ __forceinline__ double wave_sum(double v) {      // butterfly: every lane ends with the same, fixed-order sum
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

template <int VEC> struct Vec;
template <> struct Vec<1> {
    using T = float;
    __device__ static float at(const float& x, int) { return x; }
};
template <> struct Vec<4> {
    using T = float4;
    __device__ static float at(const float4& x, int q) { return q == 0 ? x.x : q == 1 ? x.y : q == 2 ? x.z : x.w; }
};

template <int VEC>
__global__ __launch_bounds__(THREADS) void sample_error_kernel(const int R, const int N, const float* __restrict__ hyp,
                                                               const float* __restrict__ depth,
                                                               const uint8_t* __restrict__ valid,
                                                               double* __restrict__ partial) {
    using VT = typename Vec<VEC>::T;
    __shared__ float sd[G];
    __shared__ int sv[G];
    __shared__ double red[WAVES][K];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = blockIdx.x * G;
    const int nr = min(G, R - r0);      // rays of this group (the last one may be short)
    double count = 0.0;
    if (tid < G) {
        float d = 0.0f;
        int v = 0;
        if (tid < nr) {
            d = depth[r0 + tid];
            v = valid ? (valid[r0 + tid] != 0) : 1;
        }
        sd[tid] = d;
        sv[tid] = v;
        count = (double)v;
    }
    __syncthreads();

    // the group's span in VT units; VEC = 4 only when N % 4 == 0, so a vector never straddles two rays
    const VT* h = reinterpret_cast<const VT*>(hyp + (size_t)r0 * N);
    const int span = nr * N / VEC;
    constexpr int STEP = THREADS * VEC;      // floats a lane's element moves per step
    const int dq = STEP / N, dr = STEP - dq * N;
    int ray = tid * VEC / N, k = tid * VEC - ray * N;
    double sum = 0.0;
    for (int i = tid; i < span; i += UNROLL * THREADS) {
        VT x[UNROLL];
        int rr[UNROLL];
        bool on[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {      // all loads first: UNROLL requests in flight per lane
            rr[u] = ray;
            on[u] = (i + u * THREADS < span) && sv[ray];      // (ray < nr whenever the element is inside the span)
            if (on[u]) x[u] = h[i + u * THREADS];
            ray += dq;
            k += dr;
            if (k >= N) {
                k -= N;
                ++ray;
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            if (on[u]) {
                const double d = (double)sd[rr[u]];
#pragma unroll
                for (int q = 0; q < VEC; ++q) sum += fabs((double)Vec<VEC>::at(x[u], q) - d);
            }
        }
    }

    const double v[K] = {sum, count};
#pragma unroll
    for (int q = 0; q < K; ++q) {
        const double s = wave_sum(v[q]);
        if (lane == 0) red[wave][q] = s;
    }
    __syncthreads();
    if (tid < K) {
        double s = red[0][tid];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) s += red[w][tid];
        partial[(size_t)blockIdx.x * K + tid] = s;
    }
}

// One workgroup: lane-strided sums over the groups, then waves in order; 1/N on the sum; written or added to the row.
__global__ __launch_bounds__(THREADS) void sample_error_reduce_kernel(const int groups, const int N, const int accumulate,
                                                                      const double* __restrict__ partial,
                                                                      double* __restrict__ row) {
    __shared__ double red[WAVES][K];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double v[K] = {0.0, 0.0};
    for (int t = tid; t < groups; t += THREADS)
#pragma unroll
        for (int q = 0; q < K; ++q) v[q] += partial[(size_t)t * K + q];
#pragma unroll
    for (int q = 0; q < K; ++q) {
        const double s = wave_sum(v[q]);
        if (lane == 0) red[wave][q] = s;
    }
    __syncthreads();
    if (tid < K) {
        double s = red[0][tid];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) s += red[w][tid];
        if (tid == PLNERF_SAMPLEERR_SUM) s /= (double)N;
        row[tid] = accumulate ? row[tid] + s : s;
    }
}

int groups_of(int R) { return (R + G - 1) / G; }

}  // namespace

extern "C" size_t plnerf_sample_error_workspace_bytes(int R) {
    return R > 0 ? (size_t)groups_of(R) * K * sizeof(double) : 0;
}

extern "C" int plnerf_sample_error(int R, int N, const float* pred_hyp, const float* depth, const uint8_t* valid,
                                   int accumulate, void* workspace, double* row, plnerf_stream_t stream) {
    if (!row) return PLNERF_EINVAL;
    if (R < 0 || N < 1 || N > PLNERF_SAMPLEERR_MAX_N) return PLNERF_ERANGE;
    if (R > 0 && (!pred_hyp || !depth || !workspace)) return PLNERF_EINVAL;
    if (R == 0 && accumulate) return PLNERF_OK;      // nothing to add
    const int groups = groups_of(R);
    if (R > 0) {
        const bool vec4 = N % 4 == 0 && ((uintptr_t)pred_hyp & 15) == 0;
        if (vec4)
            hipLaunchKernelGGL(sample_error_kernel<4>, dim3(groups), dim3(THREADS), 0, (hipStream_t)stream, R, N, pred_hyp,
                               depth, valid, (double*)workspace);
        else
            hipLaunchKernelGGL(sample_error_kernel<1>, dim3(groups), dim3(THREADS), 0, (hipStream_t)stream, R, N, pred_hyp,
                               depth, valid, (double*)workspace);
        PLNERF_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(sample_error_reduce_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, groups, N,
                       accumulate ? 1 : 0, (const double*)workspace, row);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}
