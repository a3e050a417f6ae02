// What the torch-free hosts of the C ABI (tests/c_abi_*_gpu.cpp) share: the error macros, the fixed integer hash their scenes
// and weights come from, the network's tensor table, one network builder over either net struct, the sample tables, and the
// checksums they print.  Header-only C++17, test infrastructure; tests/c_hosts.py restates the hash and the weight fill in
// numpy, and tests/test_c_hosts_host.py holds the two to the same bits without a device.
#ifndef PLNERF_TESTS_C_ABI_HOST_H
#define PLNERF_TESTS_C_ABI_HOST_H
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "plnerf_hip.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 10; } } while (0)
#define PL_OK(x) do { int rc_ = (x); if (rc_ != PLNERF_OK) { std::fprintf(stderr, "%s: %s\n", #x, plnerf_error_string(rc_)); return 11; } } while (0)

namespace c_abi_host {
constexpr int W = 256;      // the networks' width (netwidth = netwidth_fine, 8 layers, skip at 4)

// value i of sequence k, uniform in [0, 1): two rounds of the Numerical Recipes LCG over a counter
inline float hashed(uint32_t k, uint32_t i) {
    uint32_t x = i * 2654435761u + k * 0x9e3779b9u + 12345u;
    x = x * 1664525u + 1013904223u;
    x ^= x >> 15;
    x = x * 1664525u + 1013904223u;
    return (float)(x >> 8) * (1.0f / 16777216.0f);
}

struct Tensor { size_t n; int fan_in; };

// the 24 parameter tensors in state_dict order (run_nerf_helpers.py:87-101): weight [out, in], bias [out]; xyz | dir are the
// encoded input widths (63 | 27, or the depth script's 57 | 3)
inline std::vector<Tensor> param_tensors(int xyz, int dir) {
    std::vector<Tensor> t;
    for (int i = 0; i < 8; ++i) {
        const int fan_in = i == 0 ? xyz : (i == 5 ? W + xyz : W);
        t.push_back({(size_t)W * fan_in, fan_in});
        t.push_back({(size_t)W, fan_in});
    }
    t.push_back({(size_t)(W / 2) * (W + dir), W + dir}); t.push_back({(size_t)(W / 2), W + dir});      // views_linears.0
    t.push_back({(size_t)W * W, W}); t.push_back({(size_t)W, W});                                      // feature_linear
    t.push_back({(size_t)W, W}); t.push_back({1, W});                                                  // alpha_linear
    t.push_back({(size_t)3 * (W / 2), W / 2}); t.push_back({3, W / 2});                                // rgb_linear
    return t;
}

inline size_t param_count(int xyz, int dir) {
    size_t n = 0;
    for (const Tensor& t : param_tensors(xyz, dir)) n += t.n;
    return n;
}

// network `which` (0 coarse, 1 fine) flat on the host: tensor k is sequence 100 * which + k scaled to nn.Linear's
// uniform(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
inline std::vector<float> hashed_net_values(int which, int xyz, int dir) {
    std::vector<float> h;
    h.reserve(param_count(xyz, dir));
    const std::vector<Tensor> ts = param_tensors(xyz, dir);
    for (size_t k = 0; k < ts.size(); ++k) {
        const float bound = 1.0f / std::sqrt((float)ts[k].fan_in);
        for (size_t i = 0; i < ts[k].n; ++i) h.push_back((2.0f * hashed((uint32_t)(100 * which + k), (uint32_t)i) - 1.0f) * bound);
    }
    return h;
}

// a host vector in device memory of its own (+ spare_bytes behind it); nullptr, with the runtime's message, where that failed
template <class T>
T* upload(const std::vector<T>& h, size_t spare_bytes = 0) {
    T* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, h.size() * sizeof(T) + spare_bytes);
    if (e == hipSuccess) e = hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) { std::fprintf(stderr, "upload of %zu bytes: %s\n", h.size() * sizeof(T), hipGetErrorString(e)); return nullptr; }
    return d;
}

// n bytes of device memory, zeroed
template <class T>
int zeroed(T** out, size_t bytes) {
    HIP_OK(hipMalloc((void**)out, bytes));
    HIP_OK(hipMemset(*out, 0, bytes));
    return 0;
}

// one network (plnerf_step_net or plnerf_view_net): the flat parameters `values` (param_count(xyz, dir) floats) in one device
// buffer, params[k] pointing into it, and the packed buffer with its status word zeroed (the library only ORs into it)
template <class Net>
int make_net(const std::vector<float>& values, int xyz, int dir, int prec, Net* net) {
    const size_t packed_bytes = plnerf_mlp_packed_bytes(prec);
    if (packed_bytes == 0) { std::fprintf(stderr, "precision mode %d is not built\n", prec); return 7; }
    float* flat = upload(values);
    if (!flat) return 10;
    int rc = zeroed(&net->packed, packed_bytes);
    if (rc) return rc;
    const std::vector<Tensor> ts = param_tensors(xyz, dir);
    size_t off = 0;
    for (int k = 0; k < PLNERF_N_PARAM_TENSORS; ++k) { net->params[k] = flat + off; off += ts[k].n; }
    return 0;
}

// what only training adds to a network made by make_net: the flat view of its n parameters, the flat gradient (+ 4 floats of
// tail) and both moments, zeroed.  (The withheld counter stays with the program: who owns it differs.)
template <class Net>
int add_training_state(Net* net, size_t n) {
    net->param_flat = (float*)net->params[0];
    net->n_params = (int64_t)n;
    int rc = zeroed(&net->grad_flat, (n + 4) * 4);
    if (!rc) rc = zeroed(&net->exp_avg, n * 4);
    if (!rc) rc = zeroed(&net->exp_avg_sq, n * 4);
    return rc;
}

// the range status word behind a network's packed weights
template <class Net>
const uint32_t* status_word(const Net& net, int prec) {
    return (const uint32_t*)((const unsigned char*)net.packed + plnerf_mlp_status_offset(prec));
}

// t_vals [Ns] then u_vals [Ni] from the file -- torch.linspace(0, 1, n) to the bit, which a caller comparing against the
// Python route supplies -- or, for a null path, start + i * step computed here; false where the file cannot be read in full
inline bool load_tables(const char* path, int Ns, int Ni, std::vector<float>* out) {
    out->assign((size_t)Ns + Ni, 0.0f);
    if (path) {
        std::FILE* f = std::fopen(path, "rb");
        if (!f || std::fread(out->data(), 4, out->size(), f) != out->size()) return false;
        std::fclose(f);
        return true;
    }
    for (int i = 0; i < Ns; ++i) (*out)[i] = (float)i * (1.0f / (float)(Ns - 1));
    for (int i = 0; i < Ni; ++i) (*out)[Ns + i] = Ni > 1 ? (float)i * (1.0f / (float)(Ni - 1)) : 0.0f;
    return true;
}

inline unsigned long long fnv1a(const void* data, size_t n) {      // FNV-1a, 64 bits
    const unsigned char* p = (const unsigned char*)data;
    unsigned long long h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}

// the sum of n device words' bit patterns
inline int bit_sum(const void* dev, size_t n, unsigned long long* sum) {
    std::vector<uint32_t> h(n);
    HIP_OK(hipMemcpy(h.data(), dev, n * 4, hipMemcpyDeviceToHost));
    *sum = 0;
    for (uint32_t x : h) *sum += x;
    return 0;
}

// "params <sum of the coarse network's parameter bit patterns> <the fine network's>"
template <class Net>
int print_param_checksums(const Net& coarse, const Net& fine) {
    unsigned long long sums[2];
    int rc = bit_sum(coarse.param_flat, (size_t)coarse.n_params, &sums[0]);
    if (!rc) rc = bit_sum(fine.param_flat, (size_t)fine.n_params, &sums[1]);
    if (!rc) std::printf("params %llu %llu\n", sums[0], sums[1]);
    return rc;
}

// one line per step, "step <k> loss <8 hex digits of the fp32 total> <label> <8 hex digits>", from the device's [steps, width]
// loss rows: the total is value 0 of a row, the labelled one value 3
inline int print_step_losses(const float* d_loss, int steps, int width, const char* label) {
    std::vector<float> loss((size_t)steps * width);
    HIP_OK(hipMemcpy(loss.data(), d_loss, loss.size() * 4, hipMemcpyDeviceToHost));
    for (int k = 0; k < steps; ++k) {
        uint32_t bits[2];
        std::memcpy(&bits[0], &loss[(size_t)width * k], 4);
        std::memcpy(&bits[1], &loss[(size_t)width * k + 3], 4);
        std::printf("step %d loss %08x %s %08x\n", k, bits[0], label, bits[1]);
    }
    return 0;
}
}  // namespace c_abi_host

#endif
