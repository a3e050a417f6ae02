// A torch-free rendering host of the experimental entry plnerf_render_view_any (include/experimental/plnerf_hip_anyview.h):
// what a C, cgo or ctypes caller writes to turn a MIXED pair of trained networks into a frame -- a coarse network on the
// compiled 8 x 256 trunk (a FUSED slot) and a fine network outside it, netdepth 9 at netwidth 72 with its skip behind layer 4
// (a LAYERS32 slot: exact fp32, layer by layer inside the library).  Device memory from the HIP runtime, weights from the
// fixed integer hash of tests/c_abi_host.h, then nothing but the one call per frame.  Test infrastructure
// (tests/test_gpu_anyview.py builds it with g++ and compares its hashes with AnyViewRenderer on the same weights and pose); not
// part of the product.
//
//   c_abi_anyview_gpu <precision> <fwd_kernel> [tables.bin]
//
// The scene: one 6 x 10 view seen from (0.1, -0.2, 4) down -z, near 2, far 6, white background, jitter on, 8 + 8 samples,
// draws keyed by seed 11 and step 3.  The frame is rendered three times -- blocks of 16 pixels with network calls of at most
// 100 rows (which cut rays), blocks of 16 with unbounded network calls, one block of 60 --: the three must agree byte for byte.
// tables.bin (optional, fp32): t_vals [8] then u_vals [8] -- torch.linspace(0, 1, n) to the bit.
// stdout: "rgb8 <FNV-1a 64 of the 8-bit frame, hex>", "rgb <FNV-1a 64 of the fp32 colour plane>", "depth16 <...>".
#include <cmath>
#include <cstdlib>

#include "experimental/plnerf_hip_anyview.h"
#include "c_abi_host.h"      // HIP_OK / PL_OK and the scene's weights, tables and FNV-1a

using namespace c_abi_host;

namespace {
constexpr int XYZ = 63, DIR = 27, IMG_H = 6, IMG_W = 10, NS = 8, NI = 8, N_PIX = IMG_H * IMG_W;
constexpr int FINE_D = 9, FINE_W = 72, FINE_SKIP = 4;

// every plane of a frame, back to back on the host: rgb, disp, acc, depth, rgb0, disp0, acc0, depth0, z_std (fp32), rgb8, depth16
constexpr size_t F32_FLOATS = (size_t)N_PIX * (3 + 1 + 1 + 1 + 3 + 1 + 1 + 1 + 1);
constexpr size_t FRAME_BYTES = F32_FLOATS * 4 + (size_t)N_PIX * 3 + (size_t)N_PIX * 2;

// the fine network's tensors in state_dict order (run_nerf_helpers.py:87-101): weight [out, in], bias [out]
std::vector<Tensor> fine_tensors() {
    std::vector<Tensor> t;
    const auto layer = [&t](int out, int in) { t.push_back({(size_t)out * in, in}); t.push_back({(size_t)out, in}); };
    for (int i = 0; i < FINE_D; ++i) layer(FINE_W, i == 0 ? XYZ : (i == FINE_SKIP + 1 ? FINE_W + XYZ : FINE_W));
    layer(FINE_W / 2, FINE_W + DIR);      // views_linears.0
    layer(FINE_W, FINE_W);                // feature_linear
    layer(1, FINE_W);                     // alpha_linear
    layer(3, FINE_W / 2);                 // rgb_linear
    return t;
}

// hashed_net_values' fill over another tensor list: tensor k of network `which` is sequence 100 * which + k scaled to
// nn.Linear's uniform(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
std::vector<float> hashed_values(int which, const std::vector<Tensor>& ts) {
    std::vector<float> h;
    for (size_t k = 0; k < ts.size(); ++k) {
        const float bound = 1.0f / std::sqrt((float)ts[k].fan_in);
        for (size_t i = 0; i < ts[k].n; ++i) h.push_back((2.0f * hashed((uint32_t)(100 * which + k), (uint32_t)i) - 1.0f) * bound);
    }
    return h;
}
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

    plnerf_anyview_io io;
    std::memset(&io, 0, sizeof io);
    // the coarse network: on the trunk, as plnerf_render_view takes it
    io.coarse.route = PLNERF_ANYVIEW_FUSED;
    int rc = make_net(hashed_net_values(0, XYZ, DIR), XYZ, DIR, prec, &io.coarse.fused);
    if (rc) return rc;
    // the fine network: its shape, and a HOST table of device pointers into one flat buffer
    io.fine.route = PLNERF_ANYVIEW_LAYERS32;
    plnerf_generic_shape& s = io.fine.shape;
    s.D = FINE_D; s.W = FINE_W; s.input_ch = XYZ; s.view_ch = DIR; s.use_viewdirs = 1; s.n_view_layers = 1;
    s.n_skips = 1; s.skips[0] = FINE_SKIP;
    const std::vector<Tensor> ts = fine_tensors();
    const float* flat = upload(hashed_values(1, ts));
    if (!flat) return 10;
    std::vector<const float*> table;
    size_t off = 0;
    for (const Tensor& t : ts) { table.push_back(flat + off); off += t.n; }
    io.fine.params = table.data();

    std::vector<float> tables;
    if (!load_tables(argc == 4 ? argv[3] : nullptr, NS, NI, &tables)) return 4;
    const float* d_tables = upload(tables);
    if (!d_tables) return 10;
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

    std::vector<unsigned char> frames[3];
    const int blocks[3] = {16, 16, N_PIX}, net_rows[3] = {100, 1 << 21, 1 << 21};
    for (int k = 0; k < 3; ++k) {
        cfg.max_rays = blocks[k];
        io.max_net_rows = net_rows[k];
        const size_t ws_bytes = plnerf_render_view_any_workspace_bytes(&cfg, &io);
        if (ws_bytes == 0) { std::fprintf(stderr, "the configuration was refused\n"); return 8; }
        void* ws;
        HIP_OK(hipMalloc(&ws, ws_bytes));      // (hipMalloc's alignment is at least 256 bytes)
        HIP_OK(hipMemset(d_frame, 0xa5, FRAME_BYTES));
        PL_OK(plnerf_render_view_any(&cfg, &io, &a, ws, ws_bytes, nullptr));
        HIP_OK(hipDeviceSynchronize());
        frames[k].resize(FRAME_BYTES);
        HIP_OK(hipMemcpy(frames[k].data(), d_frame, FRAME_BYTES, hipMemcpyDeviceToHost));
        HIP_OK(hipFree(ws));
    }
    for (int k = 1; k < 3; ++k)
        if (std::memcmp(frames[0].data(), frames[k].data(), FRAME_BYTES) != 0) {
            std::fprintf(stderr, "the frame depends on max_rays or max_net_rows (rendering %d)\n", k);
            return 12;
        }
    // finite: every plane but the two disparities, which are 1 / max(1e-10, depth / acc) = NaN where a ray met nothing
    const float* host_f32 = (const float*)frames[0].data();
    for (size_t i = 0; i < F32_FLOATS; ++i) {
        const size_t p = i / N_PIX;      // the plane's position in units of N_PIX floats: rgb 0-2, disp 3, ..., rgb0 6-8, disp0 9
        if (p == 3 || p == 9) continue;
        if (!std::isfinite(host_f32[i])) { std::fprintf(stderr, "value %zu of the fp32 planes is not finite\n", i); return 13; }
    }
    uint32_t status;
    HIP_OK(hipMemcpy(&status, status_word(io.coarse.fused, prec), 4, hipMemcpyDeviceToHost));
    if (status) { std::fprintf(stderr, "the coarse network left the half range (status %u)\n", status); return 14; }
    const unsigned char* bytes = frames[0].data();
    std::printf("rgb8 %016llx\n", fnv1a(bytes + F32_FLOATS * 4, (size_t)N_PIX * 3));
    std::printf("rgb %016llx\n", fnv1a(bytes, (size_t)N_PIX * 3 * 4));
    std::printf("depth16 %016llx\n", fnv1a(bytes + F32_FLOATS * 4 + (size_t)N_PIX * 3, (size_t)N_PIX * 2));
    return 0;
}
