// The data feed of the depth-supervised training loop (depth_supervised_exps/run_nerf_sample_based_depth.py:1102-1167)
// as kernels:
//
//   plnerf_select_depth_rays       :1111-1120 and get_ray_batch_from_one_image_hypothesis_idx (:960-1001): a step's
//                                  distinct random pixels of one device-resident view -> their rays in the depth
//                                  script's camera convention, targets, scaled depth hypotheses and space-carving mask
//   plnerf_depth_scale_shift_grad  the space-carving term's gradient with respect to the view's depth scale and shift
//                                  (what loss.backward() leaves in DEPTH_SCALES / DEPTH_SHIFTS, :1071-1082)
//
// Built with -ffp-contract=off like the other per-ray kernels: products and sums are rounded separately, in the
// reference's order.
#include "common.h"
#include "pixel_select.h"
#include "../../include/plnerf_hip_depthfeed.h"

using namespace plnerf;

namespace {

struct DepthFeedArgs {
    int H, W, n_hyp;
    const float* image;      // [H, W, 3] of the view
    const float* hyp;        // [n_hyp, H, W] of the view
    const uint8_t* valid;    // [H, W] of the view, or null
    const float* pose;       // rows of the view's camera-to-world matrix (12 floats used)
    const float* intr;       // (fx, fy, cx, cy) of the view
    const float* scale;      // the view's scale, or null (1)
    const float* shift;      // the view's shift, or null (0)
    PixelPerm perm;
    int ray_id0, R;
    float near, far;
    float* rays_o;
    float* rays_d;
    float* viewdirs;
    float* near_out;
    float* far_out;
    float* target;
    float* target_h;         // [n_hyp, R]
    float* mask;             // [R]
    float* hyp_raw;          // [n_hyp, R] or null
    int* pixels;             // [R, 2] or null
};

// one lane per ray: a gather of scattered pixels, bound by load latency
__global__ __launch_bounds__(256) void select_depth_rays_kernel(const DepthFeedArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.R) return;
    const uint32_t pix = perm_index(a.perm, (uint32_t)(a.ray_id0 + i));
    const int row = (int)(pix / (uint32_t)a.W), col = (int)(pix % (uint32_t)a.W);
    float c[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) c[k] = a.pose[k];
    float d[3];
    const float nrm = pixel_ray_centred(row, col, a.H, a.intr[0], a.intr[1], a.intr[2], a.intr[3], c, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.rays_o[3 * (size_t)i + k] = c[4 * k + 3];
        a.rays_d[3 * (size_t)i + k] = d[k];
        if (a.viewdirs) a.viewdirs[3 * (size_t)i + k] = d[k] / nrm;
    }
    a.near_out[i] = a.near;
    a.far_out[i] = a.far;
    const float* px = a.image + (size_t)pix * 3;
    a.target[3 * (size_t)i + 0] = px[0];
    a.target[3 * (size_t)i + 1] = px[1];
    a.target[3 * (size_t)i + 2] = px[2];
    // target_h * curr_scale + curr_shift (:1120): two roundings, never an FMA
    const float s = a.scale ? *a.scale : 1.0f, t = a.shift ? *a.shift : 0.0f;
    const size_t hw = (size_t)a.H * a.W;
    for (int h = 0; h < a.n_hyp; ++h) {
        const float raw = a.hyp[(size_t)h * hw + pix];
        a.target_h[(size_t)h * a.R + i] = __fadd_rn(__fmul_rn(raw, s), t);
        if (a.hyp_raw) a.hyp_raw[(size_t)h * a.R + i] = raw;
    }
    a.mask[i] = (a.valid == nullptr || a.valid[pix] != 0) ? 1.0f : 0.0f;
    if (a.pixels) { a.pixels[2 * (size_t)i] = row; a.pixels[2 * (size_t)i + 1] = col; }
}

// ---- d total / d (scale, shift): SS_BLOCKS workgroups, fp64 partial sums per workgroup in a fixed order, then one
// workgroup adds them in workgroup order and writes the dense [n_views] rows.  The choice of hypothesis, the tie rule,
// the mask, the threshold and the normaliser are those of depth_loss_kernel (step.hip), restated.
struct ScaleShiftArgs {
    const float* hyp;          // pred_hyp [R, P]
    const float* target_h;     // [H, R, PT] (scaled)
    const float* hyp_raw;      // [H, R, PT] (unscaled)
    const float* mask;         // [R] or nullptr
    int R, P, H, PT;
    int is_joint;
    const int* joint_choice;   // [P] or nullptr
    float weight, threshold;
    double* partial;           // [SS_BLOCKS][2]: sum g_t * hyp_raw, sum g_t
};
constexpr int SS_BLOCKS = 64, SS_THREADS = 256;

__global__ __launch_bounds__(SS_THREADS) void depth_scale_shift_kernel(const ScaleShiftArgs a) {
    __shared__ double part[2][SS_THREADS / 64];
    __shared__ double jred[SS_THREADS / 64];
    __shared__ double jbest;
    __shared__ int jarg;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    double s_scale = 0.0, s_shift = 0.0;
    if (a.is_joint) {
        // one hypothesis per point column, chosen from the column's mean over the rays (model/run_nerf_helpers.py:72-77)
        const float gs = a.weight / ((float)a.R * (float)a.P);
        for (int p = b; p < a.P; p += SS_BLOCKS) {
            int hs;
            if (a.joint_choice) {
                hs = min(max(a.joint_choice[p], 0), a.H - 1);      // (an index of the caller's: kept in bounds)
            } else {
                for (int h = 0; h < a.H; ++h) {
                    double sum = 0.0;
                    for (int r = tid; r < a.R; r += SS_THREADS) {
                        const float m = a.mask ? a.mask[r] : 1.0f;
                        const float t = a.target_h[((size_t)h * a.R + r) * a.PT + (a.PT == 1 ? 0 : p)];
                        float d = fabsf(a.hyp[(size_t)r * a.P + p] - t) * m;
                        if (a.threshold > 0.0f && d < a.threshold) d = 0.0f;
                        sum += (double)d;
                    }
                    sum = wave_sum(sum);
                    if (lane == 0) jred[wave] = sum;
                    __syncthreads();
                    if (tid == 0) {
                        double tot = 0.0;
                        for (int w = 0; w < SS_THREADS / 64; ++w) tot += jred[w];
                        const float mean = (float)(tot / (double)a.R);
                        if (h == 0 || mean < (float)(jbest / (double)a.R)) { jbest = tot; jarg = h; }
                    }
                    __syncthreads();
                }
                hs = jarg;
            }
            for (int r = tid; r < a.R; r += SS_THREADS) {
                const float m = a.mask ? a.mask[r] : 1.0f;
                const size_t k = ((size_t)hs * a.R + r) * a.PT + (a.PT == 1 ? 0 : p);
                const float diff = a.hyp[(size_t)r * a.P + p] - a.target_h[k];
                float gd = diff > 0.0f ? m : (diff < 0.0f ? -m : 0.0f);
                if (a.threshold > 0.0f && fabsf(diff) * m < a.threshold) gd = 0.0f;
                const float gt = -(gd * gs);      // d / d target = -(d / d pred)
                s_shift += (double)gt;
                s_scale += (double)gt * (double)a.hyp_raw[k];
            }
            __syncthreads();      // (jarg / jbest are rewritten for the next column)
        }
    } else {
        // per (ray, point): the first minimum over the hypotheses of the masked, thresholded distance
        const int np = a.R * a.P;
        const float gs = a.weight / (float)np;
        const int per = (np + SS_BLOCKS - 1) / SS_BLOCKS, lo = b * per, hi = min(np, lo + per);
        for (int i = lo + tid; i < hi; i += SS_THREADS) {
            const int r = i / a.P, p = i - r * a.P;
            const float x = a.hyp[i];
            const float m = a.mask ? a.mask[r] : 1.0f;
            float best = 0.0f, gbest = 0.0f;
            int hbest = 0;
            for (int h = 0; h < a.H; ++h) {
                const float t = a.target_h[((size_t)h * a.R + r) * a.PT + (a.PT == 1 ? 0 : p)];
                const float diff = x - t;
                float d = fabsf(diff) * m;
                float gd = diff > 0.0f ? m : (diff < 0.0f ? -m : 0.0f);
                if (a.threshold > 0.0f && d < a.threshold) { d = 0.0f; gd = 0.0f; }
                if (h == 0 || d < best) { best = d; gbest = gd; hbest = h; }
            }
            const float gt = -(gbest * gs);
            s_shift += (double)gt;
            s_scale += (double)gt * (double)a.hyp_raw[((size_t)hbest * a.R + r) * a.PT + (a.PT == 1 ? 0 : p)];
        }
    }
    s_scale = wave_sum(s_scale);
    s_shift = wave_sum(s_shift);
    if (lane == 0) { part[0][wave] = s_scale; part[1][wave] = s_shift; }
    __syncthreads();
    if (tid == 0) {
        double v0 = 0.0, v1 = 0.0;
        for (int w = 0; w < SS_THREADS / 64; ++w) { v0 += part[0][w]; v1 += part[1][w]; }
        a.partial[2 * b + 0] = v0;
        a.partial[2 * b + 1] = v1;
    }
}

__global__ __launch_bounds__(256) void depth_scale_shift_finish_kernel(const double* __restrict__ partial, const int n_views,
                                                                       const int view, float* __restrict__ g_scale,
                                                                       float* __restrict__ g_shift) {
    const int tid = threadIdx.x;
    for (int v = tid; v < n_views; v += blockDim.x) {
        if (v != view) { g_scale[v] = 0.0f; g_shift[v] = 0.0f; }
    }
    if (tid == 0) {
        double s0 = 0.0, s1 = 0.0;
        for (int w = 0; w < SS_BLOCKS; ++w) { s0 += partial[2 * w + 0]; s1 += partial[2 * w + 1]; }      // workgroup order
        g_scale[view] = (float)s0;
        g_shift[view] = (float)s1;
    }
}

}  // namespace

extern "C" int plnerf_select_depth_rays(int n_views, int view, int H, int W, int n_hyp, const float* images, const float* hyp,
                                        const uint8_t* valid, const float* poses, int pose_rows, const float* intrinsics,
                                        const float* scale, const float* shift, float near, float far, uint64_t seed,
                                        uint32_t step, int ray_id0, int R, float* rays_o, float* rays_d, float* viewdirs,
                                        float* near_out, float* far_out, float* target, float* target_h, float* mask,
                                        float* hyp_raw, int* pixels, plnerf_stream_t stream) {
    if (n_views < 1 || view < 0 || view >= n_views || H < 1 || W < 1 || n_hyp < 1 || R < 0 || ray_id0 < 0 ||
        (pose_rows != 3 && pose_rows != 4) || !images || !hyp || !poses || !intrinsics)
        return PLNERF_EINVAL;
    const uint64_t M = (uint64_t)H * (uint64_t)W;
    if (M > (1ull << 30) || (uint64_t)ray_id0 + (uint64_t)R > M) return PLNERF_ERANGE;     // distinct pixels only
    if (R == 0) return PLNERF_OK;
    if (!rays_o || !rays_d || !near_out || !far_out || !target || !target_h || !mask) return PLNERF_EINVAL;
    DepthFeedArgs a{};
    a.H = H; a.W = W; a.n_hyp = n_hyp;
    // (pointer arithmetic only: the host reads nothing of the views)
    a.image = images + (size_t)view * M * 3;
    a.hyp = hyp + (size_t)view * n_hyp * M;
    a.valid = valid ? valid + (size_t)view * M : nullptr;
    a.pose = poses + (size_t)view * pose_rows * 4;
    a.intr = intrinsics + (size_t)view * 4;
    a.scale = scale ? scale + view : nullptr;
    a.shift = shift ? shift + view : nullptr;
    a.perm = make_perm(M, 0x5e1ec7u, seed, step);      // plnerf_select_rays' bijection: the same pixels for (seed, step)
    a.ray_id0 = ray_id0; a.R = R; a.near = near; a.far = far;
    a.rays_o = rays_o; a.rays_d = rays_d; a.viewdirs = viewdirs; a.near_out = near_out; a.far_out = far_out;
    a.target = target; a.target_h = target_h; a.mask = mask; a.hyp_raw = hyp_raw; a.pixels = pixels;
    hipLaunchKernelGGL(select_depth_rays_kernel, dim3((R + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}

extern "C" int plnerf_depth_scale_shift_grad(const float* pred_hyp, const float* target_h, const float* hyp_raw,
                                             const float* mask, int R, int n_points, int n_hyp, int target_points,
                                             int is_joint, const int* joint_choice, float space_carving_weight,
                                             float threshold, int n_views, int view, float* g_scale, float* g_shift,
                                             void* workspace, plnerf_stream_t stream) {
    static_assert(SS_BLOCKS * 2 * sizeof(double) <= PLNERF_DEPTH_SS_WORKSPACE_BYTES, "workspace");
    if (R < 1 || n_points < 1 || n_hyp < 1 || n_views < 1 || view < 0 || view >= n_views ||
        (target_points != 1 && target_points != n_points) || !pred_hyp || !target_h || !hyp_raw || !g_scale ||
        !g_shift || !workspace)
        return PLNERF_EINVAL;
    if ((uint64_t)R * (uint64_t)n_points > (1ull << 30)) return PLNERF_ERANGE;
    ScaleShiftArgs a{pred_hyp, target_h, hyp_raw, mask, R, n_points, n_hyp, target_points, is_joint ? 1 : 0,
                     is_joint ? joint_choice : nullptr, space_carving_weight, threshold, (double*)workspace};
    hipLaunchKernelGGL(depth_scale_shift_kernel, dim3(SS_BLOCKS), dim3(SS_THREADS), 0, (hipStream_t)stream, a);
    PLNERF_CHECK_LAUNCH();
    hipLaunchKernelGGL(depth_scale_shift_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream,
                       (const double*)workspace, n_views, view, g_scale, g_shift);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}
