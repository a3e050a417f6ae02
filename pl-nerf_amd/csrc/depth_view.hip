// The two kernels a rendered view of the depth-supervised variant needs beyond render_rays' own
// (include/experimental/plnerf_hip_depthview.h):
//   plnerf_depth_view_rays    depth_supervised_exps/model/run_nerf_helpers.py:243-263 for a full view: the rays of
//                             consecutive pixels, without the H x W grids
//   plnerf_frame_export_u16   run_nerf_sample_based_depth.py:277-295: (depth * 1000).astype(np.uint16), clamped
#include "common.h"
#include "pixel_select.h"
#include "../../include/experimental/plnerf_hip_depthview.h"

using namespace plnerf;

namespace {

struct DepthViewRayArgs {
    int H, W;
    float fx, fy, cx, cy;
    float c2w[12];          // rows of the 3x4 camera-to-world matrix
    int pix0, R;
    float near, far;
    float* rays_o;
    float* rays_d;
    float* viewdirs;        // or null
    float* near_out;
    float* far_out;
};

// pixel_ray_centred (pixel_select.h): the expressions of select_depth_rays_kernel (depthfeed.hip), which are torch's device
// kernels' for depth.get_rays with the intrinsics as device tensors; here for consecutive pixels and a pose from the host.
// One lane per pixel.
__global__ __launch_bounds__(256) void depth_view_rays_kernel(const DepthViewRayArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.R) return;
    const int p = a.pix0 + i;
    const int row = p / a.W, col = p - row * a.W;
    float d[3];
    const float nrm = pixel_ray_centred(row, col, a.H, a.fx, a.fy, a.cx, a.cy, a.c2w, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.rays_o[3 * (size_t)i + k] = a.c2w[4 * k + 3];
        a.rays_d[3 * (size_t)i + k] = d[k];
        if (a.viewdirs) a.viewdirs[3 * (size_t)i + k] = d[k] / nrm;
    }
    a.near_out[i] = a.near;
    a.far_out[i] = a.far;
}

// clamp to [0, 65535], truncate.  NaN -> 0 (no comparison holds), +inf -> 65535.
__device__ __forceinline__ uint32_t code_u16(const float g, const float mult) {
    const float x = g * mult;
    return (uint32_t)(x > 0.0f ? (x < 65535.0f ? x : 65535.0f) : 0.0f);
}

// One thread = one 32-bit word of output, two codes.  The last value of an odd n, or every value when the output is not
// word-aligned, leaves value by value: never a byte past 2 n.
__global__ __launch_bounds__(256) void frame_export_u16_kernel(const float* __restrict__ gray, const float mult,
                                                               uint16_t* __restrict__ out16, const size_t n, const int words) {
    const size_t e = 2 * ((size_t)blockIdx.x * 256 + threadIdx.x);
    if (e >= n) return;
    if (words && e + 2 <= n) {
        reinterpret_cast<uint32_t*>(out16)[e / 2] = code_u16(gray[e], mult) | (code_u16(gray[e + 1], mult) << 16);
    } else {
        for (size_t k = e; k < n && k < e + 2; ++k) out16[k] = (uint16_t)code_u16(gray[k], mult);
    }
}

}  // namespace

extern "C" int plnerf_depth_view_rays(int H, int W, float fx, float fy, float cx, float cy, const float* c2w_host, int pix0,
                                      int R, float near, float far, float* rays_o, float* rays_d, float* viewdirs,
                                      float* near_out, float* far_out, plnerf_stream_t stream) {
    if (H < 1 || W < 1 || R < 0 || pix0 < 0 || !c2w_host || !(fx != 0.0f) || !(fy != 0.0f)) return PLNERF_EINVAL;
    const uint64_t M = (uint64_t)H * (uint64_t)W;
    if (M > (1ull << 30) || (uint64_t)pix0 + (uint64_t)R > M) return PLNERF_ERANGE;
    if (R == 0) return PLNERF_OK;
    if (!rays_o || !rays_d || !near_out || !far_out) return PLNERF_EINVAL;
    DepthViewRayArgs a{};
    a.H = H; a.W = W; a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
    for (int i = 0; i < 12; ++i) a.c2w[i] = c2w_host[i];
    a.pix0 = pix0; a.R = R; a.near = near; a.far = far;
    a.rays_o = rays_o; a.rays_d = rays_d; a.viewdirs = viewdirs; a.near_out = near_out; a.far_out = far_out;
    hipLaunchKernelGGL(depth_view_rays_kernel, dim3((R + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}

extern "C" int plnerf_frame_export_u16(const float* gray, float mult, uint16_t* out16, int n, plnerf_stream_t stream) {
    if (n < 0) return PLNERF_EINVAL;
    if (n > (1 << 30)) return PLNERF_ERANGE;
    if (n == 0) return PLNERF_OK;
    if (!gray || !out16 || ((uintptr_t)out16 % 2) != 0) return PLNERF_EINVAL;
    const int words = ((uintptr_t)out16 % 4) == 0;
    const size_t threads = ((size_t)n + 1) / 2;
    hipLaunchKernelGGL(frame_export_u16_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gray,
                       mult, out16, (size_t)n, words);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}
