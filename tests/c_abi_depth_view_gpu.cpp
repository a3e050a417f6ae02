// A torch-free rendering host of the experimental C ABI (include/experimental/plnerf_hip_depthview.h): what a C, cgo or
// ctypes caller writes to evaluate a trained model of the depth-supervised variant with libplnerf_hip.so -- device memory
// from the HIP runtime, then nothing but plnerf_depth_render_view, once per frame (tests/c_abi_host.h holds the error macros,
// the tensor table and the network builder that the hosts share).  Test infrastructure (tests/test_gpu_depth_view.py builds
// it with g++, writes its input tables and compares its hashes with DepthViewRenderer on the same inputs); not part of the
// product.
//
//   c_abi_depth_view_gpu <precision> <fwd_kernel> <inputs.bin>
//
// inputs.bin, back to back: the coarse network's 24 parameter tensors (fp32, state_dict order, the depth script's widths
// 57 | 3), the fine network's, t_vals [6], u_vals [5] (fp32) and valid [9 * 13] (uint8).
// The scene: one 9 x 13 view, intrinsics (11.3, 9.7, 6.1, 4.3), near 2, far 6, white background, jitter on, 6 + 5 samples,
// encoder scale pi, softplus beta 10, draws keyed by seed 11 and step 3, blocks of 32 pixels, every plane, the hypotheses,
// valid + error_row and the three exports.
// stdout: "<plane> <FNV-1a 64 of its bytes, hex>" for rgb, disp, acc, depth, rgb0, disp0, acc0, depth0, z_std, pred_hyp, rgb8,
// depth16, depth_mm16, error_row.
#include <cstdlib>

#include "experimental/plnerf_hip_depthview.h"
#include "c_abi_host.h"      // HIP_OK / PL_OK, the network builder and FNV-1a

using namespace c_abi_host;

namespace {
constexpr int XYZ = 57, DIR = 3, IMG_H = 9, IMG_W = 13, NS = 6, NI = 5, N_PIX = IMG_H * IMG_W, BLOCK = 32;

// one network: its parameters from the file in one device buffer, and its packed buffer with the status word zeroed
int read_net(std::FILE* f, int prec, plnerf_view_net* net) {
    std::vector<float> h(param_count(XYZ, DIR));
    if (std::fread(h.data(), 4, h.size(), f) != h.size()) { std::fprintf(stderr, "inputs.bin is too short for a network\n"); return 4; }
    return make_net(h, XYZ, DIR, prec, net);
}

struct Plane { const char* name; size_t bytes; void* dev; };
}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: %s precision fwd_kernel inputs.bin\n", argv[0]); return 2; }
    const int prec = std::atoi(argv[1]), fwd_kernel = std::atoi(argv[2]);
    if (plnerf_version() != PLNERF_VERSION) { std::fprintf(stderr, "library / header version mismatch\n"); return 3; }
    std::FILE* f = std::fopen(argv[3], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[3]); return 4; }

    plnerf_depth_view_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.max_rays = BLOCK; cfg.n_samples = NS; cfg.n_importance = NI;
    cfg.mode = PLNERF_MODE_LINEAR; cfg.color_mode = PLNERF_COLOR_MIDPOINT;
    cfg.perturb = 1; cfg.white_bkgd = 1; cfg.zero_tol = 1e-4f; cfg.epsilon = 1e-3f;
    cfg.H = IMG_H; cfg.W = IMG_W; cfg.near = 2.0f; cfg.far = 6.0f;
    cfg.precision = prec; cfg.fwd_kernel = fwd_kernel; cfg.input_ch = XYZ; cfg.input_ch_views = DIR;
    cfg.input_scale = 3.14159265358979323846f; cfg.density_beta = 10.0f;
    cfg.seed = 11;

    plnerf_depth_view_io io;
    std::memset(&io, 0, sizeof io);
    int rc = read_net(f, prec, &io.coarse);
    if (!rc) rc = read_net(f, prec, &io.fine);
    if (rc) return rc;
    std::vector<float> tables((size_t)NS + NI);
    std::vector<uint8_t> valid(N_PIX);
    if (std::fread(tables.data(), 4, tables.size(), f) != tables.size() || std::fread(valid.data(), 1, valid.size(), f) != valid.size()) {
        std::fprintf(stderr, "inputs.bin is too short for the tables\n");
        return 4;
    }
    std::fclose(f);
    const float* d_tables = upload(tables);
    io.valid = upload(valid);
    if (!d_tables || !io.valid) return 10;
    double* d_row;      // the caller zeroes the row before a frame's first call
    if (zeroed(&d_row, 2 * sizeof(double))) return 10;
    io.t_vals = d_tables; io.u_vals = d_tables + NS;
    io.error_row = d_row;

    Plane planes[] = {
        {"rgb", (size_t)N_PIX * 12, nullptr}, {"disp", (size_t)N_PIX * 4, nullptr}, {"acc", (size_t)N_PIX * 4, nullptr},
        {"depth", (size_t)N_PIX * 4, nullptr}, {"rgb0", (size_t)N_PIX * 12, nullptr}, {"disp0", (size_t)N_PIX * 4, nullptr},
        {"acc0", (size_t)N_PIX * 4, nullptr}, {"depth0", (size_t)N_PIX * 4, nullptr}, {"z_std", (size_t)N_PIX * 4, nullptr},
        {"pred_hyp", (size_t)N_PIX * NI * 4, nullptr}, {"rgb8", (size_t)N_PIX * 3, nullptr}, {"depth16", (size_t)N_PIX * 2, nullptr},
        {"depth_mm16", (size_t)N_PIX * 2, nullptr}, {"error_row", 2 * sizeof(double), d_row},
    };
    constexpr int N_PLANES = sizeof planes / sizeof planes[0];
    for (int k = 0; k < N_PLANES - 1; ++k) {
        HIP_OK(hipMalloc(&planes[k].dev, planes[k].bytes));
        HIP_OK(hipMemset(planes[k].dev, 0xa5, planes[k].bytes));
    }
    io.rgb = (float*)planes[0].dev; io.disp = (float*)planes[1].dev; io.acc = (float*)planes[2].dev;
    io.depth = (float*)planes[3].dev; io.rgb0 = (float*)planes[4].dev; io.disp0 = (float*)planes[5].dev;
    io.acc0 = (float*)planes[6].dev; io.depth0 = (float*)planes[7].dev; io.z_std = (float*)planes[8].dev;
    io.pred_hyp = (float*)planes[9].dev; io.rgb8 = (uint8_t*)planes[10].dev; io.depth16 = (uint16_t*)planes[11].dev;
    io.depth_mm16 = (uint16_t*)planes[12].dev;

    plnerf_depth_view_args a;
    std::memset(&a, 0, sizeof a);
    const float c2w[12] = {0.8f, -0.6f, 0.0f, 0.1f, 0.6f, 0.8f, 0.0f, -0.2f, 0.0f, 0.0f, 1.0f, 4.0f};
    std::memcpy(a.c2w, c2w, sizeof c2w);
    a.fx = 11.3f; a.fy = 9.7f; a.cx = 6.1f; a.cy = 4.3f;
    a.step = 3; a.pix0 = 0; a.n_pix = N_PIX; a.pack_weights = 1; a.depth16_scale = 1.0f / cfg.far; a.depth_mm_mult = 1000.0f;

    const size_t ws_bytes = plnerf_depth_render_view_workspace_bytes(&cfg);
    if (ws_bytes == 0) { std::fprintf(stderr, "the configuration was refused\n"); return 8; }
    void* ws;
    HIP_OK(hipMalloc(&ws, ws_bytes));      // (hipMalloc's alignment is at least 256 bytes)
    PL_OK(plnerf_depth_render_view(&cfg, &io, &a, ws, ws_bytes, nullptr));
    HIP_OK(hipDeviceSynchronize());

    const plnerf_view_net* nets[2] = {&io.coarse, &io.fine};
    for (int j = 0; j < 2; ++j) {
        uint32_t status;
        HIP_OK(hipMemcpy(&status, status_word(*nets[j], prec), 4, hipMemcpyDeviceToHost));
        if (status) { std::fprintf(stderr, "network %d left the half range (status %u)\n", j, status); return 14; }
    }
    for (int k = 0; k < N_PLANES; ++k) {
        std::vector<unsigned char> h(planes[k].bytes);
        HIP_OK(hipMemcpy(h.data(), planes[k].dev, planes[k].bytes, hipMemcpyDeviceToHost));
        std::printf("%s %016llx\n", planes[k].name, fnv1a(h.data(), h.size()));
    }
    return 0;
}
