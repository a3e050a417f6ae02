// What the one-call step entries (train_step.hip: plnerf_train_step; depth_train_step.hip: plnerf_depth_train_step) share:
// the workspace carver, the check of a plnerf_step_net and the small scaling kernel that stands for torch's
// `tensor * python_float` between two launches of the Python route.
#pragma once
#include "common.h"
#include "../../include/plnerf_hip_step.h"

namespace plnerf_step {

constexpr size_t ALIGN = 256;
constexpr uint32_t NOISE_STREAM = 2;      // functional.DrawSource.NOISE: the coarse pass's density noise; the fine pass's is + 1

// x[i] *= s over two buffers in one launch (torch: `t * python_float`, the scalar rounded to fp32 first)
static __global__ __launch_bounds__(256) void scale2_kernel(float* __restrict__ a, const size_t na, float* __restrict__ b,
                                                            const size_t nb, const float s) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < na) a[i] = a[i] * s;
    else if (i < na + nb) b[i - na] = b[i - na] * s;
}

static inline int scale2(float* a, size_t na, float* b, size_t nb, float s, hipStream_t st) {
    const size_t n = na + nb;
    if (n == 0) return PLNERF_OK;
    hipLaunchKernelGGL(scale2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, na, b, nb, s);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}

struct Carver {
    unsigned char* base;
    size_t off;
    template <typename T>
    T* take(size_t nbytes) {
        T* p = (T*)(base + off);      // (base may be NULL: the size query only adds up)
        off += (nbytes + ALIGN - 1) / ALIGN * ALIGN;
        return p;
    }
    float* floats(size_t n) { return take<float>(n * sizeof(float)); }
};

static inline int check_net(const plnerf_step_net* n) {
    if (!n->param_flat || !n->grad_flat || !n->exp_avg || !n->exp_avg_sq || !n->packed || n->n_params < 1) return PLNERF_EINVAL;
    for (int i = 0; i < PLNERF_N_PARAM_TENSORS; ++i)
        if (!n->params[i] || n->params[i] < n->param_flat || n->params[i] >= n->param_flat + n->n_params) return PLNERF_EINVAL;
    return PLNERF_OK;
}

// feature_linear.weight / .bias (params[18], [19]) are copied as float4 by plnerf_mlp_pack_weights, which refuses them
// unless they are 16-byte aligned: the one-call entries look BEFORE their first launch (a refused call enqueues nothing),
// as the last of their argument checks, so that every other refusal keeps the code it had
static inline int check_params_aligned(const float* const* params) {
    return (plnerf::aligned16(params[18]) && plnerf::aligned16(params[19])) ? PLNERF_OK : PLNERF_EINVAL;
}

}  // namespace plnerf_step
