// The backward of the constant-mode final stage (plnerf_fine_epilogue_const, epilogue.hip) with respect to `raw` as ONE per-ray
// kernel: plnerf_fine_epilogue_const_bwd (include/plnerf_hip_conststep.h).
//
//     plnerf_sample_const_bwd(bins, weights[:, 1:-1], u, inds, g_hyp)   -> g_in [R,S-2]
//     g_w = g_weights + pad(g_in, 1, 1)                                   (torch: zeros, slice assignment, add)
//     plnerf_quad_bwd(PLNERF_MODE_CONSTANT, ..., g_w)                    -> g_raw, max |g_raw| per workgroup
//
// One wavefront owns one ray.  Both phases are the device functions the separate kernels run (ray_bwd_dev.h), in their order,
// so the result is theirs bit for bit; the interior weights are read in place from the [R,S] rows (no contiguous copy) and g_in
// never reaches HBM.  The wave's LDS row:
//
//     [ g_in, padded to S entries | sampler rows (6 (S-1) + 4 N floats)  OVERLAID BY  quadrature rows (9 S + 12 floats) ]
//
// The sampler's rows are dead once g_in exists, so the quadrature's take their place; g_in is read by both of the quadrature's
// passes and stays apart.  At the depth step's shape (S = 192, N = 128) that is 7.7 KB per wave, 31 KB per workgroup.
#include "common.h"
#include "ray_bwd_dev.h"
#include "../../include/plnerf_hip_conststep.h"

using namespace plnerf;

namespace {

struct FineConstBwdArgs {
    QuadArgs q;               // (lds_stride: floats of the whole row, g_in included)
    SampleConstBwdIn s;
    int gin_floats;           // S rounded up to 4: the quadrature's rows start 16-byte aligned
};

__global__ __launch_bounds__(256) void fine_epilogue_const_bwd_kernel(const FineConstBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ unsigned wave_max_bits[RAY_WAVES];
    const RayWave rw(a.q.R);
    const int lane = rw.lane, ray = rw.ray, S = a.q.S, n = S - 2;
    float* gin = smem + (size_t)rw.wave * a.q.lds_stride;
    float* row = gin + a.gin_floats;
    float total, dot;
    sample_const_bwd_rows(a.s, ray, lane, row, total, dot);
    // sample_const_bwd_kernel's last line, into the interior of a zero row
    for (int i = lane; i < n; i += 64) gin[i + 1] = (row[i] - dot) / total;
    if (lane == 0) { gin[0] = 0.0f; gin[S - 1] = 0.0f; }
    __syncthreads();      // the sampler's rows are read: the quadrature's may overwrite them
    quad_bwd_rows<PLNERF_MODE_CONSTANT>(a.q, ray, rw.live, rw.wave, lane, row, wave_max_bits, gin);
}

}  // namespace

extern "C" int plnerf_fine_epilogue_const_bwd(const float* raw, const float* z, const float* near, const float* far,
                                              const float* rays_d, const float* noise, const float* weights,
                                              const float* bins, const float* u, int u_row_stride, const int64_t* inds, int R,
                                              int S, int N, int white_bkgd, const float* g_rgb, const float* g_depth,
                                              const float* g_acc, const float* g_weights, const float* g_hyp, float* g_raw,
                                              uint32_t* absmax_out, plnerf_stream_t stream) {
    if (R < 0 || S < 3 || N < 1) return PLNERF_EINVAL;      // (S >= 3: the sampler needs one interior weight)
    if (u_row_stride != 0 && u_row_stride != N) return PLNERF_EINVAL;
    if (g_hyp && (!weights || !bins || !u || !inds)) return PLNERF_EINVAL;
    if (S > PLNERF_MAX_SAMPLES || N > 1024) return PLNERF_ERANGE;
    const int stride = fine_const_bwd_row_floats(S, N);
    const size_t lds = (size_t)RAY_WAVES * stride * sizeof(float);
    if (lds > 160 * 1024) return PLNERF_ERANGE;
    if (R == 0) return PLNERF_OK;
    if (!raw || !z || !near || !far || !rays_d || !g_rgb || !g_raw) return PLNERF_EINVAL;
    if (!plnerf::aligned16(raw) || !plnerf::aligned16(g_raw)) return PLNERF_EINVAL;      // read / stored as float4
    if (!g_hyp)      // nothing comes through the sampler: the quadrature's backward alone
        return plnerf_quad_bwd(raw, z, near, far, rays_d, noise, R, S, PLNERF_MODE_CONSTANT, PLNERF_COLOR_MIDPOINT, white_bkgd, 0,
                               g_rgb, g_depth, g_acc, g_weights, nullptr, nullptr, g_raw, absmax_out, stream);
    FineConstBwdArgs a{};
    a.q.raw = raw; a.q.z = z; a.q.near = near; a.q.far = far; a.q.rays_d = rays_d; a.q.noise = noise;
    a.q.R = R; a.q.S = S; a.q.color_mode = PLNERF_COLOR_MIDPOINT; a.q.white_bkgd = white_bkgd;
    a.q.g_rgb = g_rgb; a.q.g_depth = g_depth; a.q.g_acc = g_acc; a.q.g_weights = g_weights; a.q.g_raw = g_raw;
    a.q.absmax_out = absmax_out;
    a.q.lds_stride = stride;
    a.s = SampleConstBwdIn{bins, weights + 1, S, u, u_row_stride, inds, g_hyp, S - 1, N};
    a.gin_floats = (S + 3) & ~3;
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute((const void*)fine_epilogue_const_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds);
    hipLaunchKernelGGL(fine_epilogue_const_bwd_kernel, dim3((R + RAY_WAVES - 1) / RAY_WAVES), dim3(RAY_WAVES * 64), lds,
                       (hipStream_t)stream, a);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}
