// Test-time optimisation of a view's camera code on a cached colour head (include/experimental/plnerf_hip_camcode.h):
// optimize_camera_embedding of depth_supervised_exps/run_nerf_sample_based_depth.py:311-347 with everything that does not
// depend on the code -- sample depths, weights, the trunk, the view layer's pre-activation A -- held constant.
//
// camcode_sweep_kernel: one workgroup of 4 waves per ray, rays dealt round-robin over at most PLNERF_CAMCODE_MAX_GROUPS
// workgroups.  A row of A goes to a group of 32 lanes, each holding four columns (one 16-byte load when the row allows it,
// four 4-byte loads a stride of 32 apart otherwise); the 8 row groups of a workgroup take rows g, g + 8, ...
//   pass one (the only read of A): z = A + W_cam cam (the product once per workgroup, in registers), y = W_rgb relu(z) + b
//     by a butterfly over the 32 lanes, rgb = sigmoid(y) (lanes 0..2 of the group take one channel each); the ray's colour
//     accumulates c_s rgb_s; LDS keeps relu's mask (4 dwords per row: bit l of dword q = lane l's column q) and
//     e_sk = c_s rgb_sk (1 - rgb_sk): 40 B per row;
//   the ray's residual: the 8 partial colours in order, + bkgd - target; its loss term, added to the workgroup's sum;
//   pass two (LDS only): g_z[j] += mask_sj sum_k W_rgb[k, j] r_k e_sk with r_k = 2 ray_weight (rgb_ik - t_ik), in the
//     lane's registers across all rays of the workgroup.
// Each workgroup leaves one partial row (g_z[128] and its loss); camcode_reduce_kernel sums the rows in order and takes
// g_cam = W_cam^T g_z once.  No atomics: the outputs' bits do not depend on timing.
//
// Arithmetic: what is read is fp32; everything computed from it -- z, y, the sigmoid, every sum -- is fp64 on the vector
// ALU (no MFMA, no LDS-DMA), and g_cam is rounded to fp32 once, at the end.  The reason is the contract of
// tests/test_gpu_camcode.py: the outputs may be no farther from fp64 autograd than 4 x what torch's fp32 evaluation of the
// same expression is, case by case.  Two fp32 evaluations in different orders differ from the exact value by independent
// sums of roundings, and one of them is often a small fraction of the other by chance; only a result that is (to double
// rounding) the correctly rounded value is never farther away than ANY fp32 number, torch's included.  The cost is ~1 fp64
// operation per byte of A, which the CDNA vector ALU runs at its fp32 rate; the kernel stays bound by the read of A and the
// per-row butterfly (tools/bench_camopt.py).
//
// camcode_update_kernel: Adam, mse2psnr, ReduceLROnPlateau and the reference's best-code tracking for one iteration, on a
// state struct in device memory, so that all iterations are enqueued back to back.
#include <math.h>

#include "common.h"
#include "../../include/experimental/plnerf_hip_camcode.h"

namespace {

constexpr int MAXW = PLNERF_CAMCODE_MAX_WIDTH, MAXC = PLNERF_CAMCODE_MAX_CAM, MAXG = PLNERF_CAMCODE_MAX_GROUPS;
constexpr int THREADS = 256, LPR = 32, ROW_GROUPS = THREADS / LPR, Q = MAXW / LPR, UNROLL = 4;
static_assert(Q == 4, "a lane holds four columns: one float4, or four floats a stride of 32 apart");
constexpr size_t PARTIAL_GZ_BYTES = (size_t)MAXG * MAXW * sizeof(double);      // then MAXG doubles

struct RowSave {      // what pass two needs of a row
    uint32_t mask[Q];
    double e[3];
};
static_assert(sizeof(RowSave) == 40, "40 B per row: 40 KB of LDS at PLNERF_CAMCODE_MAX_ROWS");

template <bool VEC>
__device__ __forceinline__ int col_of(const int lig, const int q) { return VEC ? 4 * lig + q : lig + LPR * q; }

// sum over the 32 lanes of a row group (the xor distances stay inside the group): every lane ends with the same value
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int d = LPR / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(THREADS) void camcode_sweep_kernel(
    const float* __restrict__ A, const float* __restrict__ coef, const int n_rays, const int rows_per_ray, const int width,
    const float* __restrict__ cam, const int n_cam, const float* __restrict__ w_cam, const int w_cam_stride,
    const float* __restrict__ w_rgb, const float* __restrict__ b_rgb, const float* __restrict__ target,
    const float* __restrict__ bkgd, const float* __restrict__ ray_weight, double* __restrict__ partial_gz,
    double* __restrict__ partial_loss) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    RowSave* saved = reinterpret_cast<RowSave*>(lds_raw);      // [rows_per_ray]
    __shared__ double red[2][ROW_GROUPS][3];
    __shared__ double gz_red[ROW_GROUPS][MAXW];

    const int tid = threadIdx.x, lig = tid & (LPR - 1), grp = tid / LPR;
    const int half = (tid & 63) / LPR;      // which half of its wave this row group is (the ballot's 32 bits)

    // this lane's four columns: W_cam cam, W_rgb and whether the column exists
    double wc[Q], wr[3][Q];
    bool live[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int j = col_of<VEC>(lig, q);
        live[q] = j < width;
        double s = 0.0;
        if (live[q])
            for (int c = 0; c < n_cam; ++c) s = fma((double)w_cam[(size_t)j * w_cam_stride + c], (double)cam[c], s);
        wc[q] = s;
#pragma unroll
        for (int k = 0; k < 3; ++k) wr[k][q] = live[q] ? (double)w_rgb[k * width + j] : 0.0;
    }
    const double b0 = b_rgb[0], b1 = b_rgb[1], b2 = b_rgb[2];

    double gz[Q] = {0.0, 0.0, 0.0, 0.0};
    double loss = 0.0;      // (thread 0's is the workgroup's)
    int parity = 0;
    for (int ray = blockIdx.x; ray < n_rays; ray += gridDim.x) {
        const double lambda = (double)ray_weight[ray];
        if (lambda == 0.0) continue;      // (uniform over the workgroup)
        const size_t row0 = (size_t)ray * rows_per_ray;
        double acc = 0.0;      // lanes 0..2 of the group: channel `lig` of the group's share of the ray's colour

        // ---- pass one: the trip count is the same for every lane of the workgroup (the ballots need whole waves)
        for (int base = 0; base < rows_per_ray; base += ROW_GROUPS * UNROLL) {
            float a[UNROLL][Q], c[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {      // all loads first: UNROLL rows in flight per lane
                const int r = base + u * ROW_GROUPS + grp;
                c[u] = r < rows_per_ray ? coef[row0 + r] : 0.0f;
#pragma unroll
                for (int q = 0; q < Q; ++q) a[u][q] = 0.0f;
                if (c[u] != 0.0f) {
                    const float* row = A + (row0 + r) * (size_t)width;
                    if (VEC) {
                        if (live[0]) {      // (width % 4 == 0: the four columns exist together)
                            const float4 x = *reinterpret_cast<const float4*>(row + 4 * lig);
                            a[u][0] = x.x, a[u][1] = x.y, a[u][2] = x.z, a[u][3] = x.w;
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < Q; ++q)
                            if (live[q]) a[u][q] = row[lig + LPR * q];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int r = base + u * ROW_GROUPS + grp;
                const bool on = c[u] != 0.0f;
                double y0 = 0.0, y1 = 0.0, y2 = 0.0;
                uint32_t m[Q];
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const double z = (double)a[u][q] + wc[q];
                    const bool pos = on && live[q] && z > 0.0;
                    m[q] = (uint32_t)(__ballot(pos) >> (32 * half));
                    const double h = pos ? z : 0.0;
                    y0 = fma(wr[0][q], h, y0), y1 = fma(wr[1][q], h, y1), y2 = fma(wr[2][q], h, y2);
                }
                y0 = group_sum(y0) + b0, y1 = group_sum(y1) + b1, y2 = group_sum(y2) + b2;
                if (r < rows_per_ray) {
                    if (lig == 0) {
#pragma unroll
                        for (int q = 0; q < Q; ++q) saved[r].mask[q] = on ? m[q] : 0u;
                    }
                    if (lig < 3) {      // one channel per lane
                        double e = 0.0;
                        if (on) {
                            const double y = lig == 0 ? y0 : (lig == 1 ? y1 : y2);
                            const double s = 1.0 / (1.0 + exp(-y)), cs = (double)c[u];
                            acc = fma(cs, s, acc);
                            e = cs * (s * (1.0 - s));
                        }
                        saved[r].e[lig] = e;
                    }
                }
            }
        }
        if (lig < 3) red[parity][grp][lig] = acc;
        __syncthreads();      // (the rows a group reads back below are its own; the barrier is for `red`)

        // ---- the ray's residual, by every thread alike (the buffer alternates: one barrier per ray)
        double r_k[3], term = 0.0;
        const double bk = bkgd ? (double)bkgd[ray] : 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double s = red[parity][0][k];
#pragma unroll
            for (int g2 = 1; g2 < ROW_GROUPS; ++g2) s += red[parity][g2][k];
            const double d = (s + bk) - (double)target[(size_t)ray * 3 + k];
            term = fma(d, d, term);
            r_k[k] = 2.0 * lambda * d;
        }
        if (tid == 0) loss += lambda * term;
        parity ^= 1;

        // ---- pass two: LDS only
        for (int r = grp; r < rows_per_ray; r += ROW_GROUPS) {
            const RowSave s = saved[r];
            const double d0 = r_k[0] * s.e[0], d1 = r_k[1] * s.e[1], d2 = r_k[2] * s.e[2];
#pragma unroll
            for (int q = 0; q < Q; ++q)
                if ((s.mask[q] >> lig) & 1u) gz[q] += fma(wr[2][q], d2, fma(wr[1][q], d1, wr[0][q] * d0));
        }
    }

    // ---- the workgroup's partial row: the 8 row groups in order
#pragma unroll
    for (int q = 0; q < Q; ++q) gz_red[grp][col_of<VEC>(lig, q)] = gz[q];
    __syncthreads();
    if (tid < MAXW) {
        double s = gz_red[0][tid];
#pragma unroll
        for (int g2 = 1; g2 < ROW_GROUPS; ++g2) s += gz_red[g2][tid];
        partial_gz[(size_t)blockIdx.x * MAXW + tid] = s;
    }
    if (tid == 0) partial_loss[blockIdx.x] = loss;
}

// One workgroup: column j's partials in two strided halves, each in order; the loss by wave 0 (lane-strided, then a fixed
// butterfly); g_cam = W_cam^T g_z, rounded to fp32 once.
__global__ __launch_bounds__(THREADS) void camcode_reduce_kernel(const int groups, const int width, const int n_cam,
                                                                 const float* __restrict__ w_cam, const int w_cam_stride,
                                                                 const double* __restrict__ partial_gz,
                                                                 const double* __restrict__ partial_loss,
                                                                 double* __restrict__ loss_sum, float* __restrict__ g_cam) {
    __shared__ double part[2][MAXW];
    __shared__ double gz[MAXW];
    const int tid = threadIdx.x, j = tid & (MAXW - 1), h = tid / MAXW;
    double s = 0.0;
    if (j < width)
        for (int b = h; b < groups; b += 2) s += partial_gz[(size_t)b * MAXW + j];
    part[h][j] = s;
    if (tid < 64) {
        double l = 0.0;
        for (int b = tid; b < groups; b += 64) l += partial_loss[b];
        l = plnerf::wave_sum(l);
        if (tid == 0) *loss_sum = l;
    }
    __syncthreads();
    if (tid < MAXW) gz[tid] = part[0][tid] + part[1][tid];
    __syncthreads();
    if (tid < n_cam) {
        double g = 0.0;
        for (int jj = 0; jj < width; ++jj) g = fma((double)w_cam[(size_t)jj * w_cam_stride + tid], gz[jj], g);
        g_cam[tid] = (float)g;
    }
}

__global__ void camcode_update_kernel(plnerf_camcode_state* __restrict__ st, const int n_cam,
                                      const double* __restrict__ loss_sum, const float* __restrict__ g_cam,
                                      const int n_batches, const float b1, const float b2, const float eps,
                                      const float factor, const int patience, float* __restrict__ psnr_history,
                                      float* __restrict__ lr_history, const int n_history) {
    const int i = threadIdx.x;
    const int it = st->step;
    const float lr = st->lr;
    // 1. torch.optim.Adam (single-tensor path), as adam.hip: m = lerp(m, g, 1 - b1); v = b2 v + (1 - b2) g^2;
    //    denom = sqrt(v) / sqrt(bc2) + eps; p -= (lr / bc1) m / denom
    float p = 0.0f;
    if (i < n_cam) {
        const double bc1 = 1.0 - pow((double)b1, (double)(it + 1)), bc2 = 1.0 - pow((double)b2, (double)(it + 1));
        const float step_size = (float)((double)lr / bc1), bc2_sqrt = (float)sqrt(bc2);
        const float g = g_cam[i];
        const float m = st->exp_avg[i] + (g - st->exp_avg[i]) * (1.0f - b1);
        const float v = st->exp_avg_sq[i] * b2 + (1.0f - b2) * g * g;
        st->exp_avg[i] = m;
        st->exp_avg_sq[i] = v;
        p = st->cam[i] - step_size * (m / (sqrtf(v) / bc2_sqrt + eps));
        st->cam[i] = p;
    }
    // 2. mse2psnr(sum_img_loss / len(batches)), fp32 as there
    const float mse = (float)(*loss_sum) / (float)n_batches;
    const float psnr = -10.0f * logf(mse) / logf(10.0f);
    // 4. the reference's own tracking (:343-345).  Its quirk is kept: the code stored is the one AFTER this iteration's Adam
    //    step, i.e. one step ahead of the code whose PSNR selected it.
    const bool better = psnr > st->max_psnr;      // (read by every thread before thread 0 writes it: one wave)
    if (better && i < n_cam) st->best_cam[i] = p;
    if (i == 0) {
        if (it < n_history) {
            if (psnr_history) psnr_history[it] = psnr;
            if (lr_history) lr_history[it] = lr;
        }
        // 3. ReduceLROnPlateau('max', threshold 1e-4 'rel', cooldown 0, min_lr 0, eps 1e-8), in double as Python's floats
        const double current = (double)psnr, best = (double)st->best;
        int bad = st->num_bad_epochs;
        if (current > best * (1e-4 + 1.0)) {
            st->best = psnr;
            bad = 0;
        } else {
            ++bad;
        }
        if (bad > patience) {
            const double old_lr = (double)lr, new_lr = fmax(old_lr * (double)factor, 0.0);
            if (old_lr - new_lr > 1e-8) st->lr = (float)new_lr;
            bad = 0;
        }
        st->num_bad_epochs = bad;
        if (better) {
            st->max_psnr = psnr;
            st->best_iter = it;
        }
        st->step = it + 1;
    }
}

int groups_of(int n_rays) { return n_rays < MAXG ? n_rays : MAXG; }

}  // namespace

extern "C" size_t plnerf_camcode_sweep_workspace_bytes(int n_rays) {
    if (n_rays < 1) return 0;
    const size_t bytes = PARTIAL_GZ_BYTES + (size_t)MAXG * sizeof(double);
    return (bytes + 255) / 256 * 256;
}

extern "C" int plnerf_camcode_sweep(const float* A, const float* coef, int n_rows, int rows_per_ray, int width,
                                    const float* cam, int n_cam, const float* w_cam, int w_cam_stride, const float* w_rgb,
                                    const float* b_rgb, const float* target, const float* bkgd, const float* ray_weight,
                                    void* workspace, size_t workspace_bytes, double* loss_sum, float* g_cam,
                                    plnerf_stream_t stream) {
    if (!loss_sum || !g_cam || ((uintptr_t)loss_sum & 7)) return PLNERF_EINVAL;
    if (width < 1 || width > MAXW || n_cam < 1 || n_cam > MAXC || rows_per_ray < 1 || rows_per_ray > PLNERF_CAMCODE_MAX_ROWS)
        return PLNERF_EINVAL;
    if (n_rows < 0 || w_cam_stride < n_cam) return PLNERF_EINVAL;
    if (n_rows > (1 << 30)) return PLNERF_ERANGE;
    if (n_rows % rows_per_ray != 0) return PLNERF_EINVAL;
    if (n_rows == 0) return PLNERF_OK;
    if (!A || !coef || !cam || !w_cam || !w_rgb || !b_rgb || !target || !ray_weight || !workspace) return PLNERF_EINVAL;
    const int n_rays = n_rows / rows_per_ray;
    if (((uintptr_t)workspace & 255) || workspace_bytes < plnerf_camcode_sweep_workspace_bytes(n_rays)) return PLNERF_EINVAL;
    const int groups = groups_of(n_rays);
    double* partial_gz = (double*)workspace;
    double* partial_loss = (double*)((char*)workspace + PARTIAL_GZ_BYTES);
    const size_t lds = (size_t)rows_per_ray * sizeof(RowSave);
    const bool vec = width % 4 == 0 && plnerf::aligned16(A);
    if (vec)
        hipLaunchKernelGGL(camcode_sweep_kernel<true>, dim3(groups), dim3(THREADS), lds, (hipStream_t)stream, A, coef, n_rays,
                           rows_per_ray, width, cam, n_cam, w_cam, w_cam_stride, w_rgb, b_rgb, target, bkgd, ray_weight,
                           partial_gz, partial_loss);
    else
        hipLaunchKernelGGL(camcode_sweep_kernel<false>, dim3(groups), dim3(THREADS), lds, (hipStream_t)stream, A, coef, n_rays,
                           rows_per_ray, width, cam, n_cam, w_cam, w_cam_stride, w_rgb, b_rgb, target, bkgd, ray_weight,
                           partial_gz, partial_loss);
    PLNERF_CHECK_LAUNCH();
    hipLaunchKernelGGL(camcode_reduce_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, groups, width, n_cam, w_cam,
                       w_cam_stride, (const double*)partial_gz, (const double*)partial_loss, loss_sum, g_cam);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}

extern "C" int plnerf_camcode_update(plnerf_camcode_state* state, int n_cam, const double* loss_sum, const float* g_cam,
                                     int n_batches, float beta1, float beta2, float eps, float factor, int patience,
                                     float* psnr_history, float* lr_history, int n_history, plnerf_stream_t stream) {
    if (!state || !loss_sum || !g_cam || ((uintptr_t)state & 3) || ((uintptr_t)loss_sum & 7)) return PLNERF_EINVAL;
    if (n_cam < 1 || n_cam > MAXC || n_batches < 1 || n_history < 0 || patience < 0) return PLNERF_EINVAL;
    if (!(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f) || !(eps >= 0.0f)) return PLNERF_EINVAL;
    if (!(factor > 0.0f && factor < 1.0f)) return PLNERF_EINVAL;
    hipLaunchKernelGGL(camcode_update_kernel, dim3(1), dim3(PLNERF_WAVE), 0, (hipStream_t)stream, state, n_cam, loss_sum, g_cam,
                       n_batches, beta1, beta2, eps, factor, patience, psnr_history, lr_history, n_history);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}
