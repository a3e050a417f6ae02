// Pixel choice and camera rays shared by the ray sources (step.hip: plnerf_select_rays, plnerf_select_bank_rays;
// depthfeed.hip: plnerf_select_depth_rays).
#pragma once
#include <stdint.h>

#include "common.h"
#include "philox.h"

namespace plnerf {

// ---- pixel choice: a keyed bijection of [0, M) (4-round Feistel network on 2 hb bits, cycle-walked into the
// domain), evaluated at the global ray ids: distinct ids -> distinct pixels, i.e. a draw WITHOUT replacement like the
// reference's np.random.choice(..., replace=False), with no H x W permutation to build.
struct PixelPerm {
    uint32_t key[4];
    uint32_t M;
    int hb;
};

__device__ __forceinline__ uint32_t mix32(uint32_t h) {
    h *= 0x9E3779B1u; h ^= h >> 15; h *= 0x85EBCA77u; h ^= h >> 13; h *= 0xC2B2AE3Du; h ^= h >> 16;
    return h;
}

__device__ __forceinline__ uint32_t perm_index(const PixelPerm& p, uint32_t x) {
    const uint32_t mask = (1u << p.hb) - 1u;
    do {
        uint32_t L = x >> p.hb, Rr = x & mask;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t F = mix32(Rr + p.key[r]) & mask;
            const uint32_t nl = Rr;
            Rr = L ^ F;
            L = nl;
        }
        x = (L << p.hb) | Rr;
    } while (x >= p.M);
    return x;
}

// the keyed bijection of [0, M) (M <= 2^30): 2 hb >= log2 M bits, round keys from one Philox block on (seed, ctr)
// under a per-use domain constant
static inline PixelPerm make_perm(uint64_t M, uint32_t domain, uint64_t seed, uint32_t ctr) {
    PixelPerm p{};
    int bits = 1;
    while ((1ull << bits) < M) ++bits;
    p.hb = (bits + 1) / 2;
    if (p.hb < 1) p.hb = 1;
    p.M = (uint32_t)M;
    uint32_t c[4] = {domain, 0u, 0xffffffffu, ctr};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    for (int i = 0; i < 4; ++i) p.key[i] = c[i];
    return p;
}

// camera-frame direction (d0, d1, -1) -> world direction d and |d|: rays_d[k] = sum_j dirs[j] * c2w[k][j] (c2w: rows of
// the 3x4 camera-to-world matrix), and |d| from the squares in the same order.  Two summation orders of the 3 terms:
//   ThreeTermOrder::left_to_right  (t0 + t1) + t2: torch's CPU sum / norm over a trailing axis of 3 -- what the NVS ray
//                                  sources are held to (the CPU oracle's get_rays);
//   ThreeTermOrder::device         (t0 + t2) + t1: the same torch reductions on the GPU (ROCm; measured on the MI355X for
//                                  640,000 and 1,961 rays: every element of depth.get_rays' rays_d and of torch.norm on
//                                  them, none under the other two orders) -- what the depth script's training loop runs.
enum class ThreeTermOrder { left_to_right, device };

template <ThreeTermOrder O>
__device__ __forceinline__ float sum3(const float t0, const float t1, const float t2) {
    return O == ThreeTermOrder::left_to_right ? (t0 + t1) + t2 : (t0 + t2) + t1;
}

template <ThreeTermOrder O = ThreeTermOrder::left_to_right>
__device__ __forceinline__ float rotate_ray(const float d0, const float d1, const float* c2w, float d[3]) {
    const float d2 = -1.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = sum3<O>(d0 * c2w[4 * k + 0], d1 * c2w[4 * k + 1], d2 * c2w[4 * k + 2]);
    return sqrtf(sum3<O>(d[0] * d[0], d[1] * d[1], d[2] * d[2]));
}

// pixel (row, col) -> camera ray direction d and |d| (run_nerf_helpers.py:166-169):
// dirs = ((i - cx) / fx, -(j - cy) / fy, -1)
__device__ __forceinline__ float pixel_ray(const int row, const int col, const float fx, const float fy, const float cx,
                                           const float cy, const float* c2w, float d[3]) {
    return rotate_ray(((float)col - cx) / fx, -((float)row - cy) / fy, c2w, d);
}

// pixel_ray's convention in the arithmetic torch's DEVICE kernels give rays.get_rays (which render() evaluates on the GPU for a
// full view whose pose lives there): `x / python_float` is a multiply by the fp32 reciprocal there (inv_fx = 1.0f / fx, computed
// by the caller), and a reduction over a trailing axis of 3 associates as ThreeTermOrder::device.  One ulp from pixel_ray.
__device__ __forceinline__ float pixel_ray_device(const int row, const int col, const float inv_fx, const float inv_fy,
                                                  const float cx, const float cy, const float* c2w, float d[3]) {
    return rotate_ray<ThreeTermOrder::device>(((float)col - cx) * inv_fx, -((float)row - cy) * inv_fy, c2w, d);
}

// the depth script's convention (depth_supervised_exps/model/run_nerf_helpers.py:243-257): pixel CENTRES and a
// flipped row, dirs = (((i + 0.5) - cx) / fx, ((H - (j + 0.5)) - cy) / fy, -1); summed as torch sums on the GPU, where
// that script builds its rays
__device__ __forceinline__ float pixel_ray_centred(const int row, const int col, const int H, const float fx,
                                                   const float fy, const float cx, const float cy, const float* c2w,
                                                   float d[3]) {
    return rotate_ray<ThreeTermOrder::device>(((float)col + 0.5f - cx) / fx, ((float)H - ((float)row + 0.5f) - cy) / fy,
                                              c2w, d);
}

}  // namespace plnerf
