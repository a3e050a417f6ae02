// A torch-free training host of the C ABI (include/plnerf_hip_step.h): what a C, cgo or ctypes caller writes to TRAIN with
// libplnerf_hip.so -- device memory from the HIP runtime, weights from a fixed integer hash (tests/c_abi_host.h, with the
// error macros and what else the hosts share), then nothing but plnerf_train_step, once per optimisation step.  Test infrastructure (tests/test_gpu_one_call.py builds it with g++ and
// compares its per-step losses with the Python one-call route started from the same weights); not part of the product.
//
//   c_abi_step_gpu <precision> <R> <N_samples> <N_importance> <steps> <fwd_kernel> [tables.bin]
//
// The scene: one 40 x 48 view (hashed colours) seen from (0, 0, 4) down -z, near 2, far 6, white background, jitter on; Adam
// at the reference's rates (5e-4, decay 250k steps), both optimizers guarded by the networks' range status words.
// tables.bin (optional, fp32): t_vals [N_samples] then u_vals [N_importance] -- torch.linspace(0, 1, n) to the bit, which a
// caller comparing against the Python route supplies; without it the host computes start + i * step itself.
// stdout: one line per step "step <k> loss <8 hex digits of the fp32 total> psnr <8 hex digits>", then
// "params <sum of the coarse network's parameter bit patterns> <the fine network's>" (uint64, decimal).
#include <cmath>
#include <cstdlib>

#include "plnerf_hip_step.h"
#include "c_abi_host.h"      // HIP_OK / PL_OK and the scene's weights, tables and checksums

using namespace c_abi_host;

namespace {
constexpr int XYZ = 63, DIR = 27, IMG_H = 40, IMG_W = 48;
}  // namespace

int main(int argc, char** argv) {
    if (argc != 7 && argc != 8) { std::fprintf(stderr, "usage: %s precision R N_samples N_importance steps fwd_kernel [tables.bin]\n", argv[0]); return 2; }
    const int prec = std::atoi(argv[1]), R = std::atoi(argv[2]), Ns = std::atoi(argv[3]), Ni = std::atoi(argv[4]),
              steps = std::atoi(argv[5]), fwd_kernel = std::atoi(argv[6]);
    if (plnerf_version() != PLNERF_VERSION) { std::fprintf(stderr, "library / header version mismatch\n"); return 3; }
    if (Ns < 2 || Ni < 1 || steps < 1) return 2;

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
    for (int j = 0; j < 2; ++j) {
        int rc = make_net(hashed_net_values(j, XYZ, DIR), XYZ, DIR, prec, nets[j]);
        if (!rc) rc = add_training_state(nets[j], param_count(XYZ, DIR));
        if (!rc) rc = zeroed(&nets[j]->withheld, 4);
        if (rc) return rc;
    }
    // the fine optimizer is guarded by both networks' words, the coarse one by its own (render.create_nerf)
    io.fine.skip_if_set = status_word(io.fine, prec); io.fine.skip_if_set2 = status_word(io.coarse, prec);
    io.coarse.skip_if_set = status_word(io.coarse, prec);

    std::vector<float> tables;
    if (!load_tables(argc == 8 ? argv[7] : nullptr, Ns, Ni, &tables)) return 4;
    const float* d_tables = upload(tables);
    if (!d_tables) return 10;
    io.t_vals = d_tables; io.u_vals = d_tables + Ns;

    std::vector<float> image((size_t)IMG_H * IMG_W * 3);
    for (size_t i = 0; i < image.size(); ++i) image[i] = hashed(999u, (uint32_t)i);
    const float* d_image = upload(image);
    if (!d_image) return 10;
    float* d_loss;      // one loss4 per step, read back after the last one
    if (zeroed(&d_loss, (size_t)steps * 4 * 4)) return 10;

    const size_t ws_bytes = plnerf_train_step_workspace_bytes(&cfg);
    if (ws_bytes == 0) { std::fprintf(stderr, "the configuration was refused\n"); return 8; }
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
        PL_OK(plnerf_train_step(&cfg, &io, &a, ws, ws_bytes, nullptr));
    }
    HIP_OK(hipDeviceSynchronize());

    if (print_step_losses(d_loss, steps, 4, "psnr") || print_param_checksums(io.coarse, io.fine)) return 10;
    uint32_t withheld[2];
    HIP_OK(hipMemcpy(&withheld[0], io.coarse.withheld, 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(&withheld[1], io.fine.withheld, 4, hipMemcpyDeviceToHost));
    if (withheld[0] || withheld[1]) { std::fprintf(stderr, "steps were withheld (%u, %u)\n", withheld[0], withheld[1]); return 12; }
    return 0;
}
