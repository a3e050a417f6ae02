// Held-out view metrics (include/plnerf_hip_eval.h): run_plnerf.py:318-340's img2mse on rgb and rgb0, skimage 0.19's
// structural_similarity(clamp(rgb, 0, 1), target, data_range=1, channel_axis=-1), and run_nerf_helpers.py:537's
// compute_rmse over the valid depth pixels -- one launch over every tile of every frame, one over the frames.
//
// Tile: PLNERF_EVAL_TILE_H x PLNERF_EVAL_TILE_W output pixels per workgroup of 4 waves; lane = tile column, wave w the
// tile rows [8w, 8w+8).  The tile's clamped pred and target, with a 3-pixel halo, go to LDS as fp32 planes (64,000 B:
// two workgroups per CU).  Per channel each lane forms, for the 14 halo rows its 8 output rows need, the horizontal
// 7-sums of x, y, x^2, y^2, xy in fp64 (products of fp32 values are exact in fp64) and adds each into the vertical sums
// of the output rows whose window contains it, in row order; then S per interior pixel.  The SSE and depth sums cover
// the tile's own pixels (halo excluded), so the tiles together cover the border that SSIM skips.  Partial rows go to
// the workspace; eval_reduce_kernel adds a frame's tiles in tile order.  No atomics: the bits do not depend on timing,
// on n or on the other frames.
#include "common.h"
#include "../../include/plnerf_hip_eval.h"

namespace {

constexpr int TH = PLNERF_EVAL_TILE_H, TW = PLNERF_EVAL_TILE_W, K = PLNERF_EVAL_ROW;
constexpr int THREADS = 256, WAVES = THREADS / 64, ROWS = TH / WAVES;      // ROWS output rows per wave
constexpr int HR = TH + 6, HC = TW + 6;                                     // halo tile
constexpr int WIN = 7;
static_assert(TW == 64 && TH % WAVES == 0, "lane = tile column");

__device__ __forceinline__ double wave_sum(double v) {      // butterfly: every lane ends with the same, fixed-order sum
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(THREADS) void eval_tiles_kernel(const int H, const int W, const int tiles_x, const int tiles,
                                                             const float* __restrict__ pred,
                                                             const float* __restrict__ target,
                                                             const float* __restrict__ pred0,
                                                             const float* __restrict__ depth,
                                                             const float* __restrict__ target_depth,
                                                             const uint8_t* __restrict__ valid,
                                                             double* __restrict__ partial) {
    __shared__ float X[3][HR][HC];     // clamp(pred, 0, 1)
    __shared__ float Y[3][HR][HC];     // target
    __shared__ double red[WAVES][K];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x, frame = blockIdx.y;
    const int r0 = (tile / tiles_x) * TH, c0 = (tile % tiles_x) * TW;
    const size_t plane = (size_t)H * W;
    const float* P = pred + (size_t)frame * plane * 3;
    const float* T = target + (size_t)frame * plane * 3;
    const float* P0 = pred0 ? pred0 + (size_t)frame * plane * 3 : nullptr;

    // ---- halo load (row-contiguous, coalesced); out-of-image entries are 0 and feed only pixels outside the interior
    double sse = 0.0, sse0 = 0.0;
    for (int e = tid; e < HR * HC * 3; e += THREADS) {
        const int hr = e / (HC * 3), rem = e - hr * (HC * 3);
        const int hc = rem / 3, ch = rem - hc * 3;
        const int gr = r0 - 3 + hr, gc = c0 - 3 + hc;
        float x = 0.0f, y = 0.0f;
        if (gr >= 0 && gr < H && gc >= 0 && gc < W) {
            const size_t i = ((size_t)gr * W + gc) * 3 + ch;
            const float p = P[i];
            y = T[i];
            x = plnerf::tmin(plnerf::tmax(p, 0.0f), 1.0f);      // torch.clamp: NaN stays NaN
            if (hr >= 3 && hr < 3 + TH && hc >= 3 && hc < 3 + TW) {      // this tile's own pixel
                const double d = (double)p - (double)y;
                sse += d * d;
                if (P0) {
                    const double d0 = (double)P0[i] - (double)y;
                    sse0 += d0 * d0;
                }
            }
        }
        X[ch][hr][hc] = x;
        Y[ch][hr][hc] = y;
    }

    double dsse = 0.0, dcount = 0.0;
    if (depth) {
        const float* D = depth + (size_t)frame * plane;
        const float* TD = target_depth + (size_t)frame * plane;
        const uint8_t* V = valid + (size_t)frame * plane;
        for (int e = tid; e < TH * TW; e += THREADS) {
            const int gr = r0 + e / TW, gc = c0 + e % TW;
            if (gr < H && gc < W) {
                const size_t i = (size_t)gr * W + gc;
                if (V[i]) {
                    const double d = (double)D[i] - (double)TD[i];
                    dsse += d * d;
                    dcount += 1.0;
                }
            }
        }
    }
    __syncthreads();

    // ---- SSIM over the interior [3, H-3) x [3, W-3)
    constexpr double inv_np = 1.0 / 49.0, cov_norm = 49.0 / 48.0;
    constexpr double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    const int gc = c0 + lane;
    const bool col_in = gc >= 3 && gc < W - 3;
    double ssim = 0.0;
    for (int ch = 0; ch < 3; ++ch) {
        double acc[ROWS][5];
#pragma unroll
        for (int j = 0; j < ROWS; ++j)
#pragma unroll
            for (int q = 0; q < 5; ++q) acc[j][q] = 0.0;
#pragma unroll
        for (int i = 0; i < ROWS + WIN - 1; ++i) {
            const int hr = wave * ROWS + i;
            double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
            for (int k = 0; k < WIN; ++k) {
                const double x = X[ch][hr][lane + k], y = Y[ch][hr][lane + k];
                sx += x;
                sy += y;
                sxx += x * x;
                syy += y * y;
                sxy += x * y;
            }
#pragma unroll
            for (int j = 0; j < ROWS; ++j) {
                if (i >= j && i < j + WIN) {      // (compile-time after unrolling)
                    acc[j][0] += sx;
                    acc[j][1] += sy;
                    acc[j][2] += sxx;
                    acc[j][3] += syy;
                    acc[j][4] += sxy;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            const int gr = r0 + wave * ROWS + j;
            if (col_in && gr >= 3 && gr < H - 3) {
                const double ux = acc[j][0] * inv_np, uy = acc[j][1] * inv_np;
                const double uxx = acc[j][2] * inv_np, uyy = acc[j][3] * inv_np, uxy = acc[j][4] * inv_np;
                const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy);
                const double vxy = cov_norm * (uxy - ux * uy);
                const double a1 = 2.0 * ux * uy + C1, a2 = 2.0 * vxy + C2;
                const double b1 = ux * ux + uy * uy + C1, b2 = vx + vy + C2;
                ssim += (a1 * a2) / (b1 * b2);
            }
        }
    }

    // ---- the tile's partial row: waves in order, lanes by a fixed butterfly
    const double v[K] = {sse, sse0, ssim, dsse, dcount};
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
        partial[((size_t)frame * tiles + tile) * K + tid] = s;
    }
}

// One workgroup per frame: lane-strided sums over the frame's tiles, then waves in order.
__global__ __launch_bounds__(THREADS) void eval_reduce_kernel(const int H, const int W, const int tiles,
                                                              const int has_pred0, const double* __restrict__ partial,
                                                              double* __restrict__ rows) {
    __shared__ double red[WAVES][K];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, frame = blockIdx.x;
    const double* p = partial + (size_t)frame * tiles * K;
    double v[K];
#pragma unroll
    for (int q = 0; q < K; ++q) v[q] = 0.0;
    for (int t = tid; t < tiles; t += THREADS)
#pragma unroll
        for (int q = 0; q < K; ++q) v[q] += p[(size_t)t * K + q];
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
        if (tid == PLNERF_EVAL_SSE_RGB0 && !has_pred0) s = __builtin_nan("");
        if (tid == PLNERF_EVAL_SSIM) s /= 3.0 * (double)(H - 6) * (double)(W - 6);
        rows[(size_t)frame * K + tid] = s;
    }
}

}  // namespace

extern "C" int plnerf_eval_metrics(int n, int H, int W, const float* pred, const float* target, const float* pred0,
                                   const float* depth, const float* target_depth, const uint8_t* valid, void* workspace,
                                   double* rows, plnerf_stream_t stream) {
    if (n < 1 || H < WIN || W < WIN || !pred || !target || !workspace || !rows) return PLNERF_EINVAL;
    const bool any_depth = depth || target_depth || valid, all_depth = depth && target_depth && valid;
    if (any_depth && !all_depth) return PLNERF_EINVAL;
    if (n > 65535 || (int64_t)H * W > (int64_t(1) << 28)) return PLNERF_ERANGE;
    const int tiles_x = (W + TW - 1) / TW, tiles = ((H + TH - 1) / TH) * tiles_x;
    hipLaunchKernelGGL(eval_tiles_kernel, dim3(tiles, n), dim3(THREADS), 0, (hipStream_t)stream, H, W, tiles_x, tiles,
                       pred, target, pred0, depth, target_depth, valid, (double*)workspace);
    PLNERF_CHECK_LAUNCH();
    hipLaunchKernelGGL(eval_reduce_kernel, dim3(n), dim3(THREADS), 0, (hipStream_t)stream, H, W, tiles,
                       pred0 != nullptr ? 1 : 0, (const double*)workspace, rows);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}
