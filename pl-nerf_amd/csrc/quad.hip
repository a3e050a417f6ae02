// Quadrature kernels: raw2outputs forward and its backward with respect to `raw`.
//
// Reference semantics: run_plnerf.py:553-624 (raw2outputs), :516-550
// (compute_weights_piecewise_linear), :504-513 (compute_weights).  HBM-bound streaming
// scan: one 64-lane wavefront owns one ray, reads its (z, raw) rows with coalesced
// 16-byte loads, keeps the ray's knots in LDS, and does the transmittance prefix product
// as a wave scan (fp64 carry, like the reference's CPU cumprod) -- nothing is re-read
// from HBM.  Algorithmic bytes per ray (linear): 32*S+64.
#include "common.h"
#include "ray_bwd_dev.h"

using namespace plnerf;

namespace {

constexpr int WAVES = RAY_WAVES;  // rays per 256-thread workgroup

template <int MODE>
__global__ __launch_bounds__(256) void quad_fwd_kernel(QuadArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const RayWave rw(a.R);
    const int lane = rw.lane, ray = rw.ray, S = a.S;
    const bool live = rw.live;
    float* zk = smem + rw.wave * a.lds_stride;
    float* tau = zk + (S + 2);
    float* col = tau + (S + 2);
    float dnorm;
    load_ray(RayIn{a.raw, a.z, a.near, a.far, a.rays_d, a.noise, a.S}, ray, lane, zk, tau, col, dnorm);
    __syncthreads();

    // the scan, its element rule and the map write: ray_fwd_dev.h
    QuadSums sums;
    quad_scan<MODE>(S, zk, tau, dnorm, lane, [&](const int i, const bool valid, const float e, float, const float Ti, const float Tn) {
        if (valid) quad_element<MODE>(sums, a.out, ray, live, i, e, Ti, Tn, S, zk, col, a.color_mode, a.farcolorfix);
    });
    quad_write_maps<MODE>(sums, a.out, ray, live, lane, S, tau, a.white_bkgd);
}

// Backward: quad_bwd_rows (ray_bwd_dev.h).
template <int MODE>
__global__ __launch_bounds__(256) void quad_bwd_kernel(QuadArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ unsigned wave_max_bits[WAVES];
    const RayWave rw(a.R);
    quad_bwd_rows<MODE>(a, rw.ray, rw.live, rw.wave, rw.lane, smem + rw.wave * a.lds_stride, wave_max_bits, nullptr);
}

int check_common(const float* raw, const float* z, const float* near, const float* far,
                 const float* rays_d, int R, int S, int mode, int color_mode) {
    if (R < 0 || S < 2) return PLNERF_EINVAL;
    if (R > 0 && (!raw || !z || !near || !far || !rays_d)) return PLNERF_EINVAL;
    if (!plnerf::aligned16(raw)) return PLNERF_EINVAL;      // read as float4
    if (S > PLNERF_MAX_SAMPLES) return PLNERF_ERANGE;
    if (mode != PLNERF_MODE_LINEAR && mode != PLNERF_MODE_CONSTANT) return PLNERF_EINVAL;
    if (color_mode != PLNERF_COLOR_MIDPOINT && color_mode != PLNERF_COLOR_LEFT) return PLNERF_EINVAL;
    return PLNERF_OK;
}

}  // namespace

extern "C" int plnerf_quad_fwd(const float* raw, const float* z, const float* near, const float* far,
                               const float* rays_d, const float* noise, int R, int S, int mode,
                               int color_mode, int white_bkgd, int farcolorfix, float* rgb_map,
                               float* disp_map, float* acc_map, float* depth_map, float* weights,
                               float* tau, float* T, plnerf_stream_t stream) {
    int rc = check_common(raw, z, near, far, rays_d, R, S, mode, color_mode);
    if (rc) return rc;
    if (R == 0) return PLNERF_OK;
    if (!rgb_map || !disp_map || !acc_map || !depth_map) return PLNERF_EINVAL;
    QuadArgs a{};
    a.raw = raw; a.z = z; a.near = near; a.far = far; a.rays_d = rays_d; a.noise = noise;
    a.R = R; a.S = S; a.color_mode = color_mode; a.white_bkgd = white_bkgd; a.farcolorfix = farcolorfix;
    a.out = QuadOut{rgb_map, disp_map, acc_map, depth_map, weights, tau, T};
    a.lds_stride = ((5 * S + 4) + 3) & ~3;
    const size_t lds = (size_t)WAVES * a.lds_stride * sizeof(float);
    dim3 grid((R + WAVES - 1) / WAVES), block(WAVES * 64);
    hipStream_t st = (hipStream_t)stream;
    if (lds > 160 * 1024) return PLNERF_ERANGE;
    if (lds > 64 * 1024) {
        if (mode == PLNERF_MODE_LINEAR)
            (void)hipFuncSetAttribute((const void*)quad_fwd_kernel<PLNERF_MODE_LINEAR>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        else
            (void)hipFuncSetAttribute((const void*)quad_fwd_kernel<PLNERF_MODE_CONSTANT>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }
    if (mode == PLNERF_MODE_LINEAR)
        hipLaunchKernelGGL(quad_fwd_kernel<PLNERF_MODE_LINEAR>, grid, block, lds, st, a);
    else
        hipLaunchKernelGGL(quad_fwd_kernel<PLNERF_MODE_CONSTANT>, grid, block, lds, st, a);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}

namespace {
int quad_bwd_launch(const float* raw, const float* z, const float* near, const float* far, const float* rays_d,
                    const float* noise, int R, int S, int mode, int color_mode, int white_bkgd, int farcolorfix,
                    const float* g_rgb, const float* g_depth, const float* g_acc, const float* g_weights,
                    const float* g_tau, const float* g_T, float* g_raw, uint32_t* absmax_out, float* g_z, float* g_near,
                    float* g_far, float* g_dnorm, plnerf_stream_t stream) {
    int rc = check_common(raw, z, near, far, rays_d, R, S, mode, color_mode);
    if (rc) return rc;
    if (R == 0) return PLNERF_OK;
    if (!g_rgb || !g_raw || !plnerf::aligned16(g_raw)) return PLNERF_EINVAL;      // (g_raw is stored as float4)
    if ((g_tau || g_T) && mode != PLNERF_MODE_LINEAR) return PLNERF_EINVAL;
    QuadArgs a{};
    a.raw = raw; a.z = z; a.near = near; a.far = far; a.rays_d = rays_d; a.noise = noise;
    a.R = R; a.S = S; a.color_mode = color_mode; a.white_bkgd = white_bkgd; a.farcolorfix = farcolorfix;
    a.g_rgb = g_rgb; a.g_depth = g_depth; a.g_acc = g_acc; a.g_weights = g_weights; a.g_tau = g_tau; a.g_T = g_T; a.g_raw = g_raw;
    a.absmax_out = absmax_out;
    a.g_z = g_z; a.g_near = g_near; a.g_far = g_far; a.g_dnorm = g_dnorm;
    a.lds_stride = ((5 * S + 4 + (g_z ? 5 : 4) * (S + 2)) + 3) & ~3;
    const size_t lds = (size_t)WAVES * a.lds_stride * sizeof(float);
    dim3 grid((R + WAVES - 1) / WAVES), block(WAVES * 64);
    hipStream_t st = (hipStream_t)stream;
    if (lds > 160 * 1024) return PLNERF_ERANGE;
    if (lds > 64 * 1024) {
        // opt in to the large dynamic-LDS carve-out (S > ~400)
        if (mode == PLNERF_MODE_LINEAR)
            (void)hipFuncSetAttribute((const void*)quad_bwd_kernel<PLNERF_MODE_LINEAR>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        else
            (void)hipFuncSetAttribute((const void*)quad_bwd_kernel<PLNERF_MODE_CONSTANT>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }
    if (mode == PLNERF_MODE_LINEAR)
        hipLaunchKernelGGL(quad_bwd_kernel<PLNERF_MODE_LINEAR>, grid, block, lds, st, a);
    else
        hipLaunchKernelGGL(quad_bwd_kernel<PLNERF_MODE_CONSTANT>, grid, block, lds, st, a);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}
}  // namespace

extern "C" int plnerf_quad_bwd(const float* raw, const float* z, const float* near, const float* far,
                               const float* rays_d, const float* noise, int R, int S, int mode,
                               int color_mode, int white_bkgd, int farcolorfix, const float* g_rgb,
                               const float* g_depth, const float* g_acc, const float* g_weights,
                               const float* g_tau, const float* g_T, float* g_raw, uint32_t* absmax_out,
                               plnerf_stream_t stream) {
    return quad_bwd_launch(raw, z, near, far, rays_d, noise, R, S, mode, color_mode, white_bkgd, farcolorfix, g_rgb, g_depth,
                           g_acc, g_weights, g_tau, g_T, g_raw, absmax_out, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int plnerf_quad_bwd_rays(const float* raw, const float* z, const float* near, const float* far,
                                    const float* rays_d, const float* noise, int R, int S, int mode,
                                    int color_mode, int white_bkgd, int farcolorfix, const float* g_rgb,
                                    const float* g_depth, const float* g_acc, const float* g_weights,
                                    const float* g_tau, const float* g_T, float* g_raw, float* g_z, float* g_near,
                                    float* g_far, float* g_dnorm, plnerf_stream_t stream) {
    if (R > 0 && (!g_z || !g_near || !g_far || !g_dnorm)) return PLNERF_EINVAL;
    return quad_bwd_launch(raw, z, near, far, rays_d, noise, R, S, mode, color_mode, white_bkgd, farcolorfix, g_rgb, g_depth,
                           g_acc, g_weights, g_tau, g_T, g_raw, nullptr, g_z, g_near, g_far, g_dnorm, stream);
}
