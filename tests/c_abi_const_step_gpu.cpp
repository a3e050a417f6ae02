// A torch-free training host of the C ABI that starts a PL-NeRF run the way the reference does (include/plnerf_hip_conststep.h):
// K warm-up steps in piecewise-constant mode through plnerf_train_step_const, then piecewise-linear steps through
// plnerf_train_step, on ONE workspace of max(const, linear) bytes zeroed once -- device memory from the HIP runtime, weights
// from the fixed integer hash of tests/c_abi_host.h.  Test infrastructure (tests/test_gpu_const_one_call.py builds it with
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
#include <cmath>
#include <cstdlib>

#include "plnerf_hip_conststep.h"
#include "c_abi_host.h"      // HIP_OK / PL_OK and the scene's weights, tables and loss lines

using namespace c_abi_host;

namespace {
constexpr int XYZ = 63, DIR = 27, IMG_H = 40, IMG_W = 48;
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
    // each network: parameters from the hash in one flat buffer, packed buffer, flat gradient and moments, a counter of its own
    plnerf_step_net* nets[2] = {&io.coarse, &io.fine};
    const size_t n_params = param_count(XYZ, DIR);
    for (int j = 0; j < 2; ++j) {
        int rc = make_net(hashed_net_values(j, XYZ, DIR), XYZ, DIR, prec, nets[j]);
        if (!rc) rc = add_training_state(nets[j], n_params);
        if (!rc) rc = zeroed(&nets[j]->withheld, 4);
        if (rc) return rc;
    }
    // the fine optimizer is guarded by both networks' words, the coarse one by its own (render.create_nerf)
    io.fine.skip_if_set = status_word(io.fine, prec); io.fine.skip_if_set2 = status_word(io.coarse, prec);
    io.coarse.skip_if_set = status_word(io.coarse, prec);

    std::vector<float> tables;
    if (!load_tables(argv[8], Ns, Ni, &tables)) return 4;
    const float* d_tables = upload(tables);
    if (!d_tables) return 10;
    io.t_vals = d_tables; io.u_vals = d_tables + Ns;

    std::vector<float> image((size_t)IMG_H * IMG_W * 3);
    for (size_t i = 0; i < image.size(); ++i) image[i] = hashed(999u, (uint32_t)i);
    const float* d_image = upload(image);
    if (!d_image) return 10;
    float* d_loss;      // one loss4 per step, read back after the last one
    if (zeroed(&d_loss, (size_t)steps * 4 * 4)) return 10;

    // one workspace for both entries: the larger of the two queries (each entry wants its own mode in the config)
    plnerf_step_config cfg_const = cfg;
    cfg_const.mode = PLNERF_MODE_CONSTANT;
    const size_t linear_bytes = plnerf_train_step_workspace_bytes(&cfg), const_bytes = plnerf_train_step_const_workspace_bytes(&cfg_const);
    if (linear_bytes == 0 || const_bytes == 0) { std::fprintf(stderr, "the configuration was refused\n"); return 8; }
    const size_t ws_bytes = linear_bytes > const_bytes ? linear_bytes : const_bytes;
    void* ws;      // (hipMalloc's alignment is at least 256 bytes)
    if (zeroed(&ws, ws_bytes)) return 10;

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

    if (print_step_losses(d_loss, steps, 4, "psnr")) return 10;
    std::FILE* out = std::fopen(argv[9], "wb");
    if (!out) return 5;
    for (int j = 0; j < 2; ++j) {
        std::vector<float> h(n_params);
        HIP_OK(hipMemcpy(h.data(), nets[j]->param_flat, n_params * 4, hipMemcpyDeviceToHost));
        if (std::fwrite(h.data(), 4, h.size(), out) != h.size()) return 5;
    }
    if (std::fclose(out) != 0) return 5;
    std::printf("params %zu %zu\n", n_params, n_params);
    uint32_t withheld[2];
    HIP_OK(hipMemcpy(&withheld[0], io.coarse.withheld, 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(&withheld[1], io.fine.withheld, 4, hipMemcpyDeviceToHost));
    if (withheld[0] || withheld[1]) { std::fprintf(stderr, "steps were withheld (%u, %u)\n", withheld[0], withheld[1]); return 12; }
    return 0;
}
