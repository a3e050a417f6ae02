// A torch-free training host of the C ABI that starts a PL-NeRF run the way the reference does (include/plnerf_hip_conststep.h):
// K warm-up steps in piecewise-constant mode through plnerf_train_step_const, then piecewise-linear steps through
// plnerf_train_step, on ONE workspace of max(const, linear) bytes zeroed once -- device memory from the HIP runtime, weights
// from a fixed integer hash (tests/c_abi_step_gpu.cpp's).  Test infrastructure (tests/test_gpu_const_one_call.py builds it with
// g++ and compares the parameters it writes with TrainStep(constant_init = K + 1) on the Python route); not part of the product.
//
//   c_abi_const_step_gpu <precision> <R> <N_samples> <N_importance> <const steps> <linear steps> <fwd_kernel> <tables.bin> <params.bin>
//
// params.bin (written): the coarse network's flat parameters, then the fine network's, fp32, tensors in state_dict order.
// The scene: one 40 x 48 view (hashed colours) seen from (0, 0, 4) down -z, near 2, far 6, white background, jitter on; Adam
// at the reference's rates (5e-4, decay 250k steps), both optimizers guarded by the networks' range status words.
// tables.bin (fp32): t_vals [N_samples] then u_vals [N_importance] -- torch.linspace(0, 1, n) to the bit.
// stdout: one line per step "step <k> loss <8 hex digits of the fp32 total> psnr <8 hex digits>", then
// "params <floats of the coarse network> <of the fine network>".
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "plnerf_hip_conststep.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 10; } } while (0)
#define PL_OK(x) do { int rc_ = (x); if (rc_ != PLNERF_OK) { std::fprintf(stderr, "%s: %s\n", #x, plnerf_error_string(rc_)); return 11; } } while (0)

namespace {
constexpr int W = 256, XYZ = 63, DIR = 27, IMG_H = 40, IMG_W = 48;

// value i of sequence k, uniform in [0, 1): two rounds of the Numerical Recipes LCG over a counter (tests/test_gpu_one_call.py
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
    uint32_t* withheld;
    HIP_OK(hipMalloc((void**)&withheld, 4));
    HIP_OK(hipMemset(withheld, 0, 4));
    net->withheld = withheld;
    *flat_out = flat;
    *n_out = n;
    return 0;
}

const uint32_t* status_word(const plnerf_step_net& net, int prec) {
    return (const uint32_t*)((const unsigned char*)net.packed + plnerf_mlp_status_offset(prec));
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 10) {
        std::fprintf(stderr, "usage: %s precision R N_samples N_importance const_steps linear_steps fwd_kernel tables.bin params.bin\n", argv[0]);
        return 2;
    }
    const int prec = std::atoi(argv[1]), R = std::atoi(argv[2]), Ns = std::atoi(argv[3]), Ni = std::atoi(argv[4]),
              const_steps = std::atoi(argv[5]), steps = const_steps + std::atoi(argv[6]), fwd_kernel = std::atoi(argv[7]);
    if (plnerf_version() != PLNERF_VERSION) { std::fprintf(stderr, "library / header version mismatch\n"); return 3; }
    if (Ns < 3 || Ni < 1 || const_steps < 0 || steps < 1) return 2;

    plnerf_step_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.max_rays = R; cfg.n_samples = Ns; cfg.n_importance = Ni;
    cfg.mode = PLNERF_MODE_LINEAR; cfg.color_mode = PLNERF_COLOR_MIDPOINT;
    cfg.perturb = 1; cfg.white_bkgd = 1; cfg.zero_tol = 1e-4f; cfg.epsilon = 1e-3f;
    cfg.H = IMG_H; cfg.W = IMG_W; cfg.fx = 60.0f; cfg.fy = 60.0f; cfg.cx = 0.5f * IMG_W; cfg.cy = 0.5f * IMG_H;
    cfg.near = 2.0f; cfg.far = 6.0f;
    cfg.precision = prec; cfg.fwd_kernel = fwd_kernel; cfg.input_ch = XYZ; cfg.input_ch_views = DIR;
    cfg.ray_source = PLNERF_STEP_RAYS_VIEW;
    cfg.beta1 = 0.9f; cfg.beta2 = 0.999f; cfg.adam_eps = 1e-8f;
    cfg.seed = 11;

    plnerf_step_io io;
    std::memset(&io, 0, sizeof io);
    float *flat_c, *flat_f;
    size_t n_c, n_f;
    int rc = make_net(0, prec, &io.coarse, &flat_c, &n_c);
    if (rc) return rc;
    rc = make_net(1, prec, &io.fine, &flat_f, &n_f);
    if (rc) return rc;
    // the fine optimizer is guarded by both networks' words, the coarse one by its own (render.create_nerf)
    io.fine.skip_if_set = status_word(io.fine, prec); io.fine.skip_if_set2 = status_word(io.coarse, prec);
    io.coarse.skip_if_set = status_word(io.coarse, prec);

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

    std::vector<float> image((size_t)IMG_H * IMG_W * 3);
    for (size_t i = 0; i < image.size(); ++i) image[i] = hashed(999u, (uint32_t)i);
    float* d_image;
    HIP_OK(hipMalloc((void**)&d_image, image.size() * 4));
    HIP_OK(hipMemcpy(d_image, image.data(), image.size() * 4, hipMemcpyHostToDevice));
    float* d_loss;      // one loss4 per step, read back after the last one
    HIP_OK(hipMalloc((void**)&d_loss, (size_t)steps * 4 * 4));
    HIP_OK(hipMemset(d_loss, 0, (size_t)steps * 4 * 4));

    // one workspace for both entries: the larger of the two queries (each entry wants its own mode in the config)
    plnerf_step_config cfg_const = cfg;
    cfg_const.mode = PLNERF_MODE_CONSTANT;
    const size_t linear_bytes = plnerf_train_step_workspace_bytes(&cfg), const_bytes = plnerf_train_step_const_workspace_bytes(&cfg_const);
    if (linear_bytes == 0 || const_bytes == 0) { std::fprintf(stderr, "the configuration was refused\n"); return 8; }
    const size_t ws_bytes = linear_bytes > const_bytes ? linear_bytes : const_bytes;
    void* ws;
    HIP_OK(hipMalloc(&ws, ws_bytes));      // (hipMalloc's alignment is at least 256 bytes)
    HIP_OK(hipMemset(ws, 0, ws_bytes));

    plnerf_step_args a;
    std::memset(&a, 0, sizeof a);
    const float c2w[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 4};
    std::memcpy(a.c2w, c2w, sizeof c2w);
    a.rays = R; a.image = d_image; a.crop_rows = IMG_H; a.crop_cols = IMG_W; a.loss_scale = 1.0f;
    const double lrate = 5e-4, decay_steps = 250.0 * 1000.0;
    for (int k = 0; k < steps; ++k) {
        // (the reference sets the rate for the NEXT iteration after each step, run_plnerf.py:1309-1315)
        const double lr = k == 0 ? lrate : lrate * std::pow(0.1, (double)(k - 1) / decay_steps);
        a.step = (uint32_t)k;
        a.lr_fine = a.lr_coarse = (float)lr;
        a.adam_step_fine = a.adam_step_coarse = k + 1;
        io.loss4 = d_loss + 4 * k;
        if (k < const_steps) PL_OK(plnerf_train_step_const(&cfg_const, &io, &a, ws, ws_bytes, nullptr));
        else PL_OK(plnerf_train_step(&cfg, &io, &a, ws, ws_bytes, nullptr));
    }
    HIP_OK(hipDeviceSynchronize());

    std::vector<float> loss((size_t)steps * 4);
    HIP_OK(hipMemcpy(loss.data(), d_loss, loss.size() * 4, hipMemcpyDeviceToHost));
    for (int k = 0; k < steps; ++k) {
        uint32_t bits[2];
        std::memcpy(&bits[0], &loss[4 * k], 4);
        std::memcpy(&bits[1], &loss[4 * k + 3], 4);
        std::printf("step %d loss %08x psnr %08x\n", k, bits[0], bits[1]);
    }
    float* flats[2] = {flat_c, flat_f};
    const size_t ns[2] = {n_c, n_f};
    std::FILE* out = std::fopen(argv[9], "wb");
    if (!out) return 5;
    for (int j = 0; j < 2; ++j) {
        std::vector<float> h(ns[j]);
        HIP_OK(hipMemcpy(h.data(), flats[j], ns[j] * 4, hipMemcpyDeviceToHost));
        if (std::fwrite(h.data(), 4, h.size(), out) != h.size()) return 5;
    }
    if (std::fclose(out) != 0) return 5;
    std::printf("params %zu %zu\n", n_c, n_f);
    uint32_t withheld[2];
    HIP_OK(hipMemcpy(&withheld[0], io.coarse.withheld, 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(&withheld[1], io.fine.withheld, 4, hipMemcpyDeviceToHost));
    if (withheld[0] || withheld[1]) { std::fprintf(stderr, "steps were withheld (%u, %u)\n", withheld[0], withheld[1]); return 12; }
    return 0;
}
