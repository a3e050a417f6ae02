// A torch-free rendering host of the experimental C ABI (include/experimental/plnerf_hip_depthview.h): what a C, cgo or
// ctypes caller writes to evaluate a trained model of the depth-supervised variant with libplnerf_hip.so -- device memory
// from the HIP runtime, then nothing but plnerf_depth_render_view, once per frame.  Test infrastructure
// (tests/test_gpu_depth_view.py builds it with g++, writes its input tables and compares its hashes with DepthViewRenderer on
// the same inputs); not part of the product.
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
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "experimental/plnerf_hip_depthview.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 10; } } while (0)
#define PL_OK(x) do { int rc_ = (x); if (rc_ != PLNERF_OK) { std::fprintf(stderr, "%s: %s\n", #x, plnerf_error_string(rc_)); return 11; } } while (0)

namespace {
constexpr int W = 256, XYZ = 57, DIR = 3, IMG_H = 9, IMG_W = 13, NS = 6, NI = 5, N_PIX = IMG_H * IMG_W, BLOCK = 32;

std::vector<size_t> param_sizes() {      // state_dict order: weight [out, in], bias [out]
    std::vector<size_t> t;
    for (int i = 0; i < 8; ++i) {
        const int fan_in = i == 0 ? XYZ : (i == 5 ? W + XYZ : W);
        t.push_back((size_t)W * fan_in);
        t.push_back((size_t)W);
    }
    t.push_back((size_t)(W / 2) * (W + DIR)); t.push_back((size_t)(W / 2));      // views_linears.0
    t.push_back((size_t)W * W); t.push_back((size_t)W);                          // feature_linear
    t.push_back((size_t)W); t.push_back(1);                                      // alpha_linear
    t.push_back((size_t)3 * (W / 2)); t.push_back(3);                            // rgb_linear
    return t;
}

// one network: its parameters from the file in one device buffer, and its packed buffer with the status word zeroed
int make_net(std::FILE* f, int prec, plnerf_view_net* net) {
    const std::vector<size_t> sizes = param_sizes();
    size_t n = 0;
    for (size_t s : sizes) n += s;
    std::vector<float> h(n);
    if (std::fread(h.data(), 4, n, f) != n) { std::fprintf(stderr, "inputs.bin is too short for a network\n"); return 4; }
    float* flat;
    HIP_OK(hipMalloc((void**)&flat, n * 4));
    HIP_OK(hipMemcpy(flat, h.data(), n * 4, hipMemcpyHostToDevice));
    const size_t packed_bytes = plnerf_mlp_packed_bytes(prec);
    if (packed_bytes == 0) { std::fprintf(stderr, "precision mode %d is not built\n", prec); return 7; }
    void* packed;
    HIP_OK(hipMalloc(&packed, packed_bytes));
    HIP_OK(hipMemset(packed, 0, packed_bytes));
    size_t off = 0;
    for (int k = 0; k < PLNERF_N_PARAM_TENSORS; ++k) { net->params[k] = flat + off; off += sizes[k]; }
    net->packed = packed;
    return 0;
}

unsigned long long fnv1a(const void* data, size_t n) {
    const unsigned char* p = (const unsigned char*)data;
    unsigned long long h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
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
    int rc = make_net(f, prec, &io.coarse);
    if (rc) return rc;
    rc = make_net(f, prec, &io.fine);
    if (rc) return rc;
    std::vector<float> tables((size_t)NS + NI);
    std::vector<uint8_t> valid(N_PIX);
    if (std::fread(tables.data(), 4, tables.size(), f) != tables.size() || std::fread(valid.data(), 1, valid.size(), f) != valid.size()) {
        std::fprintf(stderr, "inputs.bin is too short for the tables\n");
        return 4;
    }
    std::fclose(f);
    float* d_tables;
    uint8_t* d_valid;
    double* d_row;
    HIP_OK(hipMalloc((void**)&d_tables, tables.size() * 4));
    HIP_OK(hipMemcpy(d_tables, tables.data(), tables.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMalloc((void**)&d_valid, valid.size()));
    HIP_OK(hipMemcpy(d_valid, valid.data(), valid.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMalloc((void**)&d_row, 2 * sizeof(double)));
    HIP_OK(hipMemset(d_row, 0, 2 * sizeof(double)));      // the caller zeroes the row before a frame's first call
    io.t_vals = d_tables; io.u_vals = d_tables + NS;
    io.valid = d_valid; io.error_row = d_row;

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
        HIP_OK(hipMemcpy(&status, (const unsigned char*)nets[j]->packed + plnerf_mlp_status_offset(prec), 4, hipMemcpyDeviceToHost));
        if (status) { std::fprintf(stderr, "network %d left the half range (status %u)\n", j, status); return 14; }
    }
    for (int k = 0; k < N_PLANES; ++k) {
        std::vector<unsigned char> h(planes[k].bytes);
        HIP_OK(hipMemcpy(h.data(), planes[k].dev, planes[k].bytes, hipMemcpyDeviceToHost));
        std::printf("%s %016llx\n", planes[k].name, fnv1a(h.data(), h.size()));
    }
    return 0;
}
