// A torch-free training host of the depth-supervised one-call step (include/plnerf_hip_depthstep.h): device memory from the
// HIP runtime, weights, views and hypotheses from a fixed integer hash, then nothing but plnerf_depth_train_step, once per
// optimisation step.  Test infrastructure (tests/test_gpu_depth_one_call.py builds it with g++ and compares its parameter
// checksums with DepthTrainStep(one_call=True).step_view started from the same inputs); not part of the product.
//
//   c_abi_depth_step_gpu <precision> <R> <N_samples> <N_importance> <steps> <fwd_kernel> <n_hyp> tables.bin
//
// The scene: 3 views of 24 x 32 (hashed colours, hypotheses in [2, 6), about 70 % of the pixels valid) seen from
// (0.1 v, 0, 4) down -z with intrinsics (40 + v, 42 - v, 16, 12), near 2, far 6, white background, jitter on, the
// space-carving term on from the first step (weight 0.007) and the depth scales / shifts (1.02, -0.03) stepped at 1e-3;
// one Adam at 5e-4 over both networks, clipped at 0.1, guarded by both range status words.  Step k trains on view k % 3.
// tables.bin (fp32): t_vals [N_samples] then u_vals [N_importance] -- torch.linspace(0, 1, n) to the bit.
// stdout: one line per step "step <k> loss <8 hex digits of the fp32 total> carve <8 hex digits>", then
// "params <sum of the coarse network's parameter bit patterns> <the fine network's>" and "ss <the scales'> <the shifts'>"
// (uint64, decimal).
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "plnerf_hip_depthstep.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 10; } } while (0)
#define PL_OK(x) do { int rc_ = (x); if (rc_ != PLNERF_OK) { std::fprintf(stderr, "%s: %s\n", #x, plnerf_error_string(rc_)); return 11; } } while (0)

namespace {
constexpr int W = 256, XYZ = 57, DIR = 3, IMG_H = 24, IMG_W = 32, V = 3;      // (multires 9, multires_views 0)

// value i of sequence k, uniform in [0, 1): two rounds of the Numerical Recipes LCG over a counter (tests/test_gpu_depth_one_call.py
// restates it in numpy)
inline float hashed(uint32_t k, uint32_t i) {
    uint32_t x = i * 2654435761u + k * 0x9e3779b9u + 12345u;
    x = x * 1664525u + 1013904223u;
    x ^= x >> 15;
    x = x * 1664525u + 1013904223u;
    return (float)(x >> 8) * (1.0f / 16777216.0f);
}

struct Tensor { size_t n; int fan_in; };

std::vector<Tensor> param_tensors() {      // state_dict order (run_nerf_helpers.py:87-101): weight [out, in], bias [out]
    std::vector<Tensor> t;
    for (int i = 0; i < 8; ++i) {
        const int fan_in = i == 0 ? XYZ : (i == 5 ? W + XYZ : W);
        t.push_back({(size_t)W * fan_in, fan_in});
        t.push_back({(size_t)W, fan_in});
    }
    t.push_back({(size_t)(W / 2) * (W + DIR), W + DIR}); t.push_back({(size_t)(W / 2), W + DIR});      // views_linears.0
    t.push_back({(size_t)W * W, W}); t.push_back({(size_t)W, W});                                      // feature_linear
    t.push_back({(size_t)W, W}); t.push_back({1, W});                                                  // alpha_linear
    t.push_back({(size_t)3 * (W / 2), W / 2}); t.push_back({3, W / 2});                                // rgb_linear
    return t;
}

// one network: its flat parameter buffer filled from the hash (nn.Linear's uniform(-1 / sqrt(fan_in), 1 / sqrt(fan_in))), flat
// gradient (+ 4 floats of tail) and moments, packed buffer with its status word zeroed
int make_net(int which, int prec, plnerf_step_net* net, float** flat_out, size_t* n_out) {
    const std::vector<Tensor> ts = param_tensors();
    size_t n = 0;
    for (const Tensor& t : ts) n += t.n;
    std::vector<float> h(n);
    size_t off = 0;
    std::vector<size_t> offs;
    for (size_t k = 0; k < ts.size(); ++k) {
        const float bound = 1.0f / std::sqrt((float)ts[k].fan_in);
        for (size_t i = 0; i < ts[k].n; ++i) h[off + i] = (2.0f * hashed((uint32_t)(100 * which + k), (uint32_t)i) - 1.0f) * bound;
        offs.push_back(off);
        off += ts[k].n;
    }
    float *flat, *grad, *m, *v;
    HIP_OK(hipMalloc((void**)&flat, n * 4));
    HIP_OK(hipMalloc((void**)&grad, (n + 4) * 4));
    HIP_OK(hipMalloc((void**)&m, n * 4));
    HIP_OK(hipMalloc((void**)&v, n * 4));
    HIP_OK(hipMemcpy(flat, h.data(), n * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(grad, 0, (n + 4) * 4));
    HIP_OK(hipMemset(m, 0, n * 4));
    HIP_OK(hipMemset(v, 0, n * 4));
    const size_t packed_bytes = plnerf_mlp_packed_bytes(prec);
    if (packed_bytes == 0) { std::fprintf(stderr, "precision mode %d is not built\n", prec); return 7; }
    void* packed;
    HIP_OK(hipMalloc(&packed, packed_bytes));
    HIP_OK(hipMemset(packed, 0, packed_bytes));
    for (int k = 0; k < PLNERF_N_PARAM_TENSORS; ++k) net->params[k] = flat + offs[k];
    net->param_flat = flat; net->grad_flat = grad; net->exp_avg = m; net->exp_avg_sq = v;
    net->n_params = (int64_t)n;
    net->packed = packed;
    *flat_out = flat;
    *n_out = n;
    return 0;
}

const uint32_t* status_word(const plnerf_step_net& net, int prec) {
    return (const uint32_t*)((const unsigned char*)net.packed + plnerf_mlp_status_offset(prec));
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 9) { std::fprintf(stderr, "usage: %s precision R N_samples N_importance steps fwd_kernel n_hyp tables.bin\n", argv[0]); return 2; }
    const int prec = std::atoi(argv[1]), R = std::atoi(argv[2]), Ns = std::atoi(argv[3]), Ni = std::atoi(argv[4]),
              steps = std::atoi(argv[5]), fwd_kernel = std::atoi(argv[6]), n_hyp = std::atoi(argv[7]);
    if (plnerf_version() != PLNERF_VERSION) { std::fprintf(stderr, "library / header version mismatch\n"); return 3; }
    if (Ns < 2 || Ni < 1 || steps < 1 || n_hyp < 1) return 2;

    plnerf_depth_step_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.max_rays = R; cfg.n_samples = Ns; cfg.n_importance = Ni; cfg.color_mode = PLNERF_COLOR_MIDPOINT;
    cfg.perturb = 1; cfg.white_bkgd = 1; cfg.zero_tol = 1e-4f; cfg.epsilon = 1e-3f;
    cfg.n_views = V; cfg.H = IMG_H; cfg.W = IMG_W; cfg.n_hyp = n_hyp; cfg.pose_rows = 4;
    cfg.near = 2.0f; cfg.far = 6.0f;
    cfg.precision = prec; cfg.fwd_kernel = fwd_kernel; cfg.input_ch = XYZ; cfg.input_ch_views = DIR;
    cfg.input_scale = (float)3.141592653589793; cfg.density_beta = 10.0f;
    cfg.space_carving_weight = 0.007f; cfg.clip_value = 0.1f;
    cfg.beta1 = 0.9f; cfg.beta2 = 0.999f; cfg.adam_eps = 1e-8f;
    cfg.ss_beta1 = 0.9f; cfg.ss_beta2 = 0.999f; cfg.ss_adam_eps = 1e-8f;
    cfg.seed = 11;

    plnerf_depth_step_io io;
    std::memset(&io, 0, sizeof io);
    float *flat_c, *flat_f;
    size_t n_c, n_f;
    int rc = make_net(0, prec, &io.coarse, &flat_c, &n_c);
    if (rc) return rc;
    rc = make_net(1, prec, &io.fine, &flat_f, &n_f);
    if (rc) return rc;
    // one optimizer over both networks: both runs guarded by both words, one counter (depth.create_nerf)
    uint32_t* withheld;
    HIP_OK(hipMalloc((void**)&withheld, 4));
    HIP_OK(hipMemset(withheld, 0, 4));
    io.coarse.skip_if_set = io.fine.skip_if_set = status_word(io.coarse, prec);
    io.coarse.skip_if_set2 = io.fine.skip_if_set2 = status_word(io.fine, prec);
    io.coarse.withheld = io.fine.withheld = withheld;

    std::vector<float> tables((size_t)Ns + Ni);
    {
        std::FILE* f = std::fopen(argv[8], "rb");
        if (!f || std::fread(tables.data(), 4, tables.size(), f) != tables.size()) return 4;
        std::fclose(f);
    }
    float* d_tables;
    HIP_OK(hipMalloc((void**)&d_tables, tables.size() * 4));
    HIP_OK(hipMemcpy(d_tables, tables.data(), tables.size() * 4, hipMemcpyHostToDevice));
    io.t_vals = d_tables; io.u_vals = d_tables + Ns;

    // the views: images, hypotheses, validity, poses, intrinsics
    const size_t px = (size_t)V * IMG_H * IMG_W;
    std::vector<float> images(px * 3), hyp(px * n_hyp), poses((size_t)V * 16, 0.0f), intr((size_t)V * 4);
    std::vector<uint8_t> valid(px);
    for (size_t i = 0; i < images.size(); ++i) images[i] = hashed(999u, (uint32_t)i);
    for (size_t i = 0; i < hyp.size(); ++i) hyp[i] = 2.0f + 4.0f * hashed(998u, (uint32_t)i);
    for (size_t i = 0; i < px; ++i) valid[i] = hashed(997u, (uint32_t)i) > 0.3f ? 1 : 0;
    for (int v = 0; v < V; ++v) {
        float* p = &poses[(size_t)v * 16];
        p[0] = p[5] = p[10] = p[15] = 1.0f;
        p[3] = 0.1f * (float)v; p[11] = 4.0f;
        intr[4 * v] = 40.0f + (float)v; intr[4 * v + 1] = 42.0f - (float)v; intr[4 * v + 2] = 16.0f; intr[4 * v + 3] = 12.0f;
    }
    float *d_images, *d_hyp, *d_poses, *d_intr, *d_ss;
    uint8_t* d_valid;
    HIP_OK(hipMalloc((void**)&d_images, images.size() * 4));
    HIP_OK(hipMemcpy(d_images, images.data(), images.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMalloc((void**)&d_hyp, hyp.size() * 4));
    HIP_OK(hipMemcpy(d_hyp, hyp.data(), hyp.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMalloc((void**)&d_valid, valid.size()));
    HIP_OK(hipMemcpy(d_valid, valid.data(), valid.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMalloc((void**)&d_poses, poses.size() * 4));
    HIP_OK(hipMemcpy(d_poses, poses.data(), poses.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMalloc((void**)&d_intr, intr.size() * 4));
    HIP_OK(hipMemcpy(d_intr, intr.data(), intr.size() * 4, hipMemcpyHostToDevice));
    io.images = d_images; io.hyp = d_hyp; io.valid = d_valid; io.poses = d_poses; io.intrinsics = d_intr;
    // scales [V], shifts [V], their gradient [2, V] and moments [2, V] x 2 in one allocation
    std::vector<float> ss((size_t)8 * V, 0.0f);
    for (int v = 0; v < V; ++v) { ss[v] = 1.02f; ss[V + v] = -0.03f; }
    HIP_OK(hipMalloc((void**)&d_ss, ss.size() * 4));
    HIP_OK(hipMemcpy(d_ss, ss.data(), ss.size() * 4, hipMemcpyHostToDevice));
    io.scale = d_ss; io.shift = d_ss + V; io.ss_grad = d_ss + 2 * V; io.ss_exp_avg = d_ss + 4 * V; io.ss_exp_avg_sq = d_ss + 6 * V;

    float* d_loss;      // one loss5 per step, read back after the last one
    HIP_OK(hipMalloc((void**)&d_loss, (size_t)steps * 5 * 4));
    HIP_OK(hipMemset(d_loss, 0, (size_t)steps * 5 * 4));

    const size_t ws_bytes = plnerf_depth_train_step_workspace_bytes(&cfg);
    if (ws_bytes == 0) { std::fprintf(stderr, "the configuration was refused\n"); return 8; }
    void* ws;
    HIP_OK(hipMalloc(&ws, ws_bytes));      // (hipMalloc's alignment is at least 256 bytes)
    HIP_OK(hipMemset(ws, 0, ws_bytes));

    plnerf_depth_step_args a;
    std::memset(&a, 0, sizeof a);
    a.rays = R; a.lr = 5e-4f; a.carve = 1; a.ss_step = 1; a.ss_lr = 1e-3f;
    for (int k = 0; k < steps; ++k) {
        a.view = k % V;
        a.step = (uint32_t)k;
        a.adam_step = a.ss_adam_step = k + 1;
        io.loss5 = d_loss + 5 * k;
        PL_OK(plnerf_depth_train_step(&cfg, &io, &a, ws, ws_bytes, nullptr));
    }
    HIP_OK(hipDeviceSynchronize());

    std::vector<float> loss((size_t)steps * 5);
    HIP_OK(hipMemcpy(loss.data(), d_loss, loss.size() * 4, hipMemcpyDeviceToHost));
    for (int k = 0; k < steps; ++k) {
        uint32_t bits[2];
        std::memcpy(&bits[0], &loss[5 * k], 4);
        std::memcpy(&bits[1], &loss[5 * k + 3], 4);
        std::printf("step %d loss %08x carve %08x\n", k, bits[0], bits[1]);
    }
    unsigned long long sums[2];
    float* flats[2] = {flat_c, flat_f};
    const size_t ns[2] = {n_c, n_f};
    for (int j = 0; j < 2; ++j) {
        std::vector<uint32_t> h(ns[j]);
        HIP_OK(hipMemcpy(h.data(), flats[j], ns[j] * 4, hipMemcpyDeviceToHost));
        sums[j] = 0;
        for (uint32_t x : h) sums[j] += x;
    }
    std::printf("params %llu %llu\n", sums[0], sums[1]);
    std::vector<uint32_t> hs((size_t)2 * V);
    HIP_OK(hipMemcpy(hs.data(), d_ss, hs.size() * 4, hipMemcpyDeviceToHost));
    unsigned long long s_scale = 0, s_shift = 0;
    for (int v = 0; v < V; ++v) { s_scale += hs[v]; s_shift += hs[V + v]; }
    std::printf("ss %llu %llu\n", s_scale, s_shift);
    uint32_t w;
    HIP_OK(hipMemcpy(&w, withheld, 4, hipMemcpyDeviceToHost));
    if (w) { std::fprintf(stderr, "steps were withheld (%u)\n", w); return 12; }
    return 0;
}
