// The two kernels a rendered view needs beyond render_rays' own (include/plnerf_hip_view.h):
//   plnerf_view_rays      run_plnerf.py:130-150 for a full view: the rays of consecutive pixels, without the H x W grids
//   plnerf_frame_export   run_nerf_helpers.py:19-20: to8b of a colour plane and to16b of a scaled depth plane, one launch
#include "common.h"
#include "pixel_select.h"
#include "../../include/plnerf_hip_view.h"

using namespace plnerf;

namespace {

struct ViewRayArgs {
    int W;
    float inv_fx, inv_fy, cx, cy;
    float c2w[12];          // rows of the 3x4 camera-to-world matrix
    int pix0, R;
    float near, far;
    float* rays_o;
    float* rays_d;
    float* viewdirs;        // or null
    float* near_out;
    float* far_out;
};

// pixel_ray_device (pixel_select.h): pixel_ray's convention in the arithmetic of torch's device kernels, which is what render()
// evaluates for a full view.  (plnerf_select_rays keeps pixel_ray: the host's get_rays, which the training ray sources are held to.)
__global__ __launch_bounds__(256) void view_rays_kernel(const ViewRayArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.R) return;
    const int p = a.pix0 + i;
    const int row = p / a.W, col = p - row * a.W;
    float d[3];
    const float nrm = pixel_ray_device(row, col, a.inv_fx, a.inv_fy, a.cx, a.cy, a.c2w, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.rays_o[3 * (size_t)i + k] = a.c2w[4 * k + 3];
        a.rays_d[3 * (size_t)i + k] = d[k];
        if (a.viewdirs) a.viewdirs[3 * (size_t)i + k] = d[k] / nrm;
    }
    a.near_out[i] = a.near;
    a.far_out[i] = a.far;
}

// ---- export: clip to [0, 1], scale, truncate.  NaN -> 0 (no comparison holds), +inf -> the top code.
__device__ __forceinline__ float clip01(const float x) { return x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f; }
__device__ __forceinline__ uint32_t code8(const float x) { return (uint32_t)(255.0f * clip01(x)); }
__device__ __forceinline__ uint32_t code16(const float g, const float scale) { return (uint32_t)(65535.0f * clip01(g * scale)); }

struct ExportArgs {
    const float* rgb;       // [n8] = 3 n values, or null
    uint8_t* rgb8;
    const float* gray;      // [n] or null
    uint16_t* gray16;
    float gray_scale;
    size_t n8, n16;         // values of either plane (0: absent)
    size_t t8;              // threads of the colour plane: ceil(n8 / 4); the rest serve the grey plane, two values each
    int words8, words16;    // the output is 4-byte aligned: whole groups leave as one 32-bit store
};

// One thread = one 32-bit word of output: 4 colour codes or 2 grey codes.  A group that would reach past the plane's end
// (n8 % 4 != 0, n16 odd), or a plane whose output is not word-aligned, leaves value by value: never a byte past 3 n / 2 n.
__global__ __launch_bounds__(256) void frame_export_kernel(const ExportArgs a) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < a.t8) {
        const size_t e = 4 * t;
        if (a.words8 && e + 4 <= a.n8) {
            const uint32_t c0 = code8(a.rgb[e]), c1 = code8(a.rgb[e + 1]), c2 = code8(a.rgb[e + 2]), c3 = code8(a.rgb[e + 3]);
            reinterpret_cast<uint32_t*>(a.rgb8)[t] = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
        } else {
            for (size_t k = e; k < a.n8 && k < e + 4; ++k) a.rgb8[k] = (uint8_t)code8(a.rgb[k]);
        }
        return;
    }
    const size_t e = 2 * (t - a.t8);
    if (e >= a.n16) return;
    if (a.words16 && e + 2 <= a.n16) {
        reinterpret_cast<uint32_t*>(a.gray16)[t - a.t8] = code16(a.gray[e], a.gray_scale) | (code16(a.gray[e + 1], a.gray_scale) << 16);
    } else {
        for (size_t k = e; k < a.n16 && k < e + 2; ++k) a.gray16[k] = (uint16_t)code16(a.gray[k], a.gray_scale);
    }
}

}  // namespace

extern "C" int plnerf_view_rays(int H, int W, float fx, float fy, float cx, float cy, const float* c2w_host, int pix0, int R,
                                float near, float far, float* rays_o, float* rays_d, float* viewdirs, float* near_out,
                                float* far_out, plnerf_stream_t stream) {
    if (H < 1 || W < 1 || R < 0 || pix0 < 0 || !c2w_host || !(fx != 0.0f) || !(fy != 0.0f)) return PLNERF_EINVAL;
    const uint64_t M = (uint64_t)H * (uint64_t)W;
    if (M > (1ull << 30) || (uint64_t)pix0 + (uint64_t)R > M) return PLNERF_ERANGE;
    if (R == 0) return PLNERF_OK;
    if (!rays_o || !rays_d || !near_out || !far_out) return PLNERF_EINVAL;
    ViewRayArgs a{};
    a.W = W; a.inv_fx = 1.0f / fx; a.inv_fy = 1.0f / fy; a.cx = cx; a.cy = cy;
    for (int i = 0; i < 12; ++i) a.c2w[i] = c2w_host[i];
    a.pix0 = pix0; a.R = R; a.near = near; a.far = far;
    a.rays_o = rays_o; a.rays_d = rays_d; a.viewdirs = viewdirs; a.near_out = near_out; a.far_out = far_out;
    hipLaunchKernelGGL(view_rays_kernel, dim3((R + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}

extern "C" int plnerf_frame_export(const float* rgb, uint8_t* rgb8, const float* gray, float gray_scale, uint16_t* gray16,
                                   int n, plnerf_stream_t stream) {
    if (n < 0 || (rgb == nullptr) != (rgb8 == nullptr) || (gray == nullptr) != (gray16 == nullptr)) return PLNERF_EINVAL;
    if (n > (1 << 30)) return PLNERF_ERANGE;
    if (n == 0 || (!rgb && !gray)) return PLNERF_OK;
    ExportArgs a{};
    a.rgb = rgb; a.rgb8 = rgb8; a.gray = gray; a.gray16 = gray16; a.gray_scale = gray_scale;
    a.n8 = rgb ? 3 * (size_t)n : 0;
    a.n16 = gray ? (size_t)n : 0;
    a.t8 = (a.n8 + 3) / 4;
    a.words8 = ((uintptr_t)rgb8 % 4) == 0;
    a.words16 = ((uintptr_t)gray16 % 4) == 0;
    const size_t threads = a.t8 + (a.n16 + 1) / 2;
    hipLaunchKernelGGL(frame_export_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}
