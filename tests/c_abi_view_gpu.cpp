// A torch-free rendering host of the C ABI (include/plnerf_hip_view.h): what a C, cgo or ctypes caller writes to turn two
// trained networks into a frame with libplnerf_hip.so -- device memory from the HIP runtime, weights from the fixed integer
// hash of tests/c_abi_step_gpu.cpp, then nothing but plnerf_render_view, once per frame.  Test infrastructure
// (tests/test_gpu_view.py builds it with g++ and compares its hashes with ViewRenderer on the same weights and pose); not
// part of the product.
//
//   c_abi_view_gpu <precision> <fwd_kernel> [tables.bin]
//
// The scene: one 16 x 12 view seen from (0.1, -0.2, 4) down -z, near 2, far 6, white background, jitter on, 64 + 128 samples,
// draws keyed by seed 11 and step 3.  The frame is rendered twice, in blocks of 64 and of 192 pixels: the two must agree byte
// for byte in every plane and be finite (but for the disparity of a ray that met nothing).
// tables.bin (optional, fp32): t_vals [64] then u_vals [128] -- torch.linspace(0, 1, n) to the bit.
// stdout: "rgb8 <FNV-1a 64 of the 8-bit frame, hex>", "rgb <FNV-1a 64 of the fp32 colour plane>", "depth16 <...>".
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "plnerf_hip_view.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 10; } } while (0)
#define PL_OK(x) do { int rc_ = (x); if (rc_ != PLNERF_OK) { std::fprintf(stderr, "%s: %s\n", #x, plnerf_error_string(rc_)); return 11; } } while (0)

namespace {
constexpr int W = 256, XYZ = 63, DIR = 27, IMG_H = 16, IMG_W = 12, NS = 64, NI = 128, N_PIX = IMG_H * IMG_W;

// value i of sequence k, uniform in [0, 1): tests/c_abi_step_gpu.cpp's hash (tests/test_gpu_one_call.py restates it in numpy)
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

// one network: its parameters from the hash (nn.Linear's uniform(-1 / sqrt(fan_in), 1 / sqrt(fan_in))) in one device buffer,
// and its packed buffer with the status word zeroed
int make_net(int which, int prec, plnerf_view_net* net) {
    const std::vector<Tensor> ts = param_tensors();
    size_t n = 0;
    for (const Tensor& t : ts) n += t.n;
    std::vector<float> h(n);
    std::vector<size_t> offs;
    size_t off = 0;
    for (size_t k = 0; k < ts.size(); ++k) {
        const float bound = 1.0f / std::sqrt((float)ts[k].fan_in);
        for (size_t i = 0; i < ts[k].n; ++i) h[off + i] = (2.0f * hashed((uint32_t)(100 * which + k), (uint32_t)i) - 1.0f) * bound;
        offs.push_back(off);
        off += ts[k].n;
    }
    float* flat;
    HIP_OK(hipMalloc((void**)&flat, n * 4));
    HIP_OK(hipMemcpy(flat, h.data(), n * 4, hipMemcpyHostToDevice));
    const size_t packed_bytes = plnerf_mlp_packed_bytes(prec);
    if (packed_bytes == 0) { std::fprintf(stderr, "precision mode %d is not built\n", prec); return 7; }
    void* packed;
    HIP_OK(hipMalloc(&packed, packed_bytes));
    HIP_OK(hipMemset(packed, 0, packed_bytes));
    for (int k = 0; k < PLNERF_N_PARAM_TENSORS; ++k) net->params[k] = flat + offs[k];
    net->packed = packed;
    return 0;
}

unsigned long long fnv1a(const void* data, size_t n) {
    const unsigned char* p = (const unsigned char*)data;
    unsigned long long h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}

// every plane of a frame, back to back on the host: rgb, disp, acc, depth, rgb0, disp0, acc0, depth0, z_std (fp32), rgb8, depth16
constexpr size_t F32_FLOATS = (size_t)N_PIX * (3 + 1 + 1 + 1 + 3 + 1 + 1 + 1 + 1);
constexpr size_t FRAME_BYTES = F32_FLOATS * 4 + (size_t)N_PIX * 3 + (size_t)N_PIX * 2;
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3 && argc != 4) { std::fprintf(stderr, "usage: %s precision fwd_kernel [tables.bin]\n", argv[0]); return 2; }
    const int prec = std::atoi(argv[1]), fwd_kernel = std::atoi(argv[2]);
    if (plnerf_version() != PLNERF_VERSION) { std::fprintf(stderr, "library / header version mismatch\n"); return 3; }

    plnerf_step_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.n_samples = NS; cfg.n_importance = NI;
    cfg.mode = PLNERF_MODE_LINEAR; cfg.color_mode = PLNERF_COLOR_MIDPOINT;
    cfg.perturb = 1; cfg.white_bkgd = 1; cfg.zero_tol = 1e-4f; cfg.epsilon = 1e-3f;
    cfg.H = IMG_H; cfg.W = IMG_W; cfg.fx = 20.0f; cfg.fy = 21.0f; cfg.cx = 0.5f * IMG_W; cfg.cy = 0.5f * IMG_H;
    cfg.near = 2.0f; cfg.far = 6.0f;
    cfg.precision = prec; cfg.fwd_kernel = fwd_kernel; cfg.input_ch = XYZ; cfg.input_ch_views = DIR;
    cfg.seed = 11;

    plnerf_view_io io;
    std::memset(&io, 0, sizeof io);
    int rc = make_net(0, prec, &io.coarse);
    if (rc) return rc;
    rc = make_net(1, prec, &io.fine);
    if (rc) return rc;

    std::vector<float> tables((size_t)NS + NI);
    if (argc == 4) {
        std::FILE* f = std::fopen(argv[3], "rb");
        if (!f || std::fread(tables.data(), 4, tables.size(), f) != tables.size()) return 4;
        std::fclose(f);
    } else {
        for (int i = 0; i < NS; ++i) tables[i] = (float)i * (1.0f / (float)(NS - 1));
        for (int i = 0; i < NI; ++i) tables[NS + i] = (float)i * (1.0f / (float)(NI - 1));
    }
    float* d_tables;
    HIP_OK(hipMalloc((void**)&d_tables, tables.size() * 4));
    HIP_OK(hipMemcpy(d_tables, tables.data(), tables.size() * 4, hipMemcpyHostToDevice));
    io.t_vals = d_tables; io.u_vals = d_tables + NS;

    // the frame: every plane in one allocation (each offset a multiple of 4 bytes)
    unsigned char* d_frame;
    HIP_OK(hipMalloc((void**)&d_frame, FRAME_BYTES));
    float* f32 = (float*)d_frame;
    io.rgb = f32; f32 += 3 * N_PIX;
    io.disp = f32; f32 += N_PIX;
    io.acc = f32; f32 += N_PIX;
    io.depth = f32; f32 += N_PIX;
    io.rgb0 = f32; f32 += 3 * N_PIX;
    io.disp0 = f32; f32 += N_PIX;
    io.acc0 = f32; f32 += N_PIX;
    io.depth0 = f32; f32 += N_PIX;
    io.z_std = f32; f32 += N_PIX;
    io.rgb8 = (uint8_t*)f32;
    io.depth16 = (uint16_t*)(io.rgb8 + 3 * N_PIX);

    plnerf_view_args a;
    std::memset(&a, 0, sizeof a);
    const float c2w[12] = {1, 0, 0, 0.1f, 0, 1, 0, -0.2f, 0, 0, 1, 4};
    std::memcpy(a.c2w, c2w, sizeof c2w);
    a.step = 3; a.pix0 = 0; a.n_pix = N_PIX; a.pack_weights = 1; a.depth16_scale = 1.0f / cfg.far;

    std::vector<unsigned char> frames[2];
    const int blocks[2] = {64, N_PIX};
    for (int k = 0; k < 2; ++k) {
        cfg.max_rays = blocks[k];
        const size_t ws_bytes = plnerf_render_view_workspace_bytes(&cfg);
        if (ws_bytes == 0) { std::fprintf(stderr, "the configuration was refused\n"); return 8; }
        void* ws;
        HIP_OK(hipMalloc(&ws, ws_bytes));      // (hipMalloc's alignment is at least 256 bytes)
        HIP_OK(hipMemset(d_frame, 0xa5, FRAME_BYTES));
        PL_OK(plnerf_render_view(&cfg, &io, &a, ws, ws_bytes, nullptr));
        HIP_OK(hipDeviceSynchronize());
        frames[k].resize(FRAME_BYTES);
        HIP_OK(hipMemcpy(frames[k].data(), d_frame, FRAME_BYTES, hipMemcpyDeviceToHost));
        HIP_OK(hipFree(ws));
    }
    if (std::memcmp(frames[0].data(), frames[1].data(), FRAME_BYTES) != 0) {
        std::fprintf(stderr, "the frame depends on max_rays\n");
        return 12;
    }
    // finite: every plane but the two disparities, which are 1 / max(1e-10, depth / acc) = NaN where a ray met nothing
    // (acc = 0), in the reference as here (run_plnerf.py:612)
    const float* host_f32 = (const float*)frames[0].data();
    for (size_t i = 0; i < F32_FLOATS; ++i) {
        const size_t p = i / N_PIX;      // the plane's position in units of N_PIX floats: rgb 0-2, disp 3, ..., rgb0 6-8, disp0 9
        if (p == 3 || p == 9) continue;
        if (!std::isfinite(host_f32[i])) { std::fprintf(stderr, "value %zu of the fp32 planes is not finite\n", i); return 13; }
    }
    const plnerf_view_net* nets[2] = {&io.coarse, &io.fine};
    for (int j = 0; j < 2; ++j) {
        uint32_t status;
        HIP_OK(hipMemcpy(&status, (const unsigned char*)nets[j]->packed + plnerf_mlp_status_offset(prec), 4, hipMemcpyDeviceToHost));
        if (status) { std::fprintf(stderr, "network %d left the half range (status %u)\n", j, status); return 14; }
    }
    const unsigned char* bytes = frames[0].data();
    std::printf("rgb8 %016llx\n", fnv1a(bytes + F32_FLOATS * 4, (size_t)N_PIX * 3));
    std::printf("rgb %016llx\n", fnv1a(bytes, (size_t)N_PIX * 3 * 4));
    std::printf("depth16 %016llx\n", fnv1a(bytes + F32_FLOATS * 4 + (size_t)N_PIX * 3, (size_t)N_PIX * 2));
    return 0;
}
