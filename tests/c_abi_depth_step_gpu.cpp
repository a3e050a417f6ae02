// A torch-free training host of the depth-supervised one-call step (include/plnerf_hip_depthstep.h): device memory from the
// HIP runtime, weights, views and hypotheses from the fixed integer hash of tests/c_abi_host.h, then nothing but
// plnerf_depth_train_step, once per optimisation step.  Test infrastructure (tests/test_gpu_depth_one_call.py builds it with
// g++ and compares its parameter checksums with DepthTrainStep(one_call=True).step_view started from the same inputs); not
// part of the product.
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
#include <cstdlib>

#include "plnerf_hip_depthstep.h"
#include "c_abi_host.h"      // HIP_OK / PL_OK and the scene's hash, weights, tables and checksums

using namespace c_abi_host;

namespace {
constexpr int XYZ = 57, DIR = 3, IMG_H = 24, IMG_W = 32, V = 3;      // (multires 9, multires_views 0)
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
    // each network: parameters from the hash in one flat buffer, packed buffer, flat gradient and moments
    plnerf_step_net* nets[2] = {&io.coarse, &io.fine};
    for (int j = 0; j < 2; ++j) {
        int rc = make_net(hashed_net_values(j, XYZ, DIR), XYZ, DIR, prec, nets[j]);
        if (!rc) rc = add_training_state(nets[j], param_count(XYZ, DIR));
        if (rc) return rc;
    }
    // one optimizer over both networks: both runs guarded by both words, one counter (depth.create_nerf)
    uint32_t* withheld;
    if (zeroed(&withheld, 4)) return 10;
    io.coarse.skip_if_set = io.fine.skip_if_set = status_word(io.coarse, prec);
    io.coarse.skip_if_set2 = io.fine.skip_if_set2 = status_word(io.fine, prec);
    io.coarse.withheld = io.fine.withheld = withheld;

    std::vector<float> tables;
    if (!load_tables(argv[8], Ns, Ni, &tables)) return 4;
    const float* d_tables = upload(tables);
    if (!d_tables) return 10;
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
    io.images = upload(images); io.hyp = upload(hyp); io.valid = upload(valid); io.poses = upload(poses); io.intrinsics = upload(intr);
    if (!io.images || !io.hyp || !io.valid || !io.poses || !io.intrinsics) return 10;
    // scales [V], shifts [V], their gradient [2, V] and moments [2, V] x 2 in one allocation
    std::vector<float> ss((size_t)8 * V, 0.0f);
    for (int v = 0; v < V; ++v) { ss[v] = 1.02f; ss[V + v] = -0.03f; }
    float* d_ss = upload(ss);
    if (!d_ss) return 10;
    io.scale = d_ss; io.shift = d_ss + V; io.ss_grad = d_ss + 2 * V; io.ss_exp_avg = d_ss + 4 * V; io.ss_exp_avg_sq = d_ss + 6 * V;

    float* d_loss;      // one loss5 per step, read back after the last one
    if (zeroed(&d_loss, (size_t)steps * 5 * 4)) return 10;

    const size_t ws_bytes = plnerf_depth_train_step_workspace_bytes(&cfg);
    if (ws_bytes == 0) { std::fprintf(stderr, "the configuration was refused\n"); return 8; }
    void* ws;      // (hipMalloc's alignment is at least 256 bytes)
    if (zeroed(&ws, ws_bytes)) return 10;

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

    if (print_step_losses(d_loss, steps, 5, "carve") || print_param_checksums(io.coarse, io.fine)) return 10;
    unsigned long long s_scale, s_shift;
    if (bit_sum(io.scale, V, &s_scale) || bit_sum(io.shift, V, &s_shift)) return 10;
    std::printf("ss %llu %llu\n", s_scale, s_shift);
    uint32_t w;
    HIP_OK(hipMemcpy(&w, withheld, 4, hipMemcpyDeviceToHost));
    if (w) { std::fprintf(stderr, "steps were withheld (%u)\n", w); return 12; }
    return 0;
}
