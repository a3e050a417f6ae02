// The per-ray forward bodies that more than one kernel runs, each as a device function over one wave's LDS rows: the separate
// launches (quad.hip, sampler.hip, step.hip) and the fused ones (epilogue.hip, and pass 1 of ray_bwd_dev.h's quad_bwd_rows) call
// the same code, so "bit-equal to the separate launches" holds by construction.  No function here knows its caller, chooses
// an LDS layout, holds a barrier or returns for a dead wave: those stay with each kernel.
// Everything that includes this is built with -ffp-contract=off.
#pragma once
#include "common.h"
#include "ray_dev.h"

namespace plnerf {

constexpr int RAY_WAVES = 4;      // rays (= wavefronts) per 256-thread workgroup of every per-ray kernel

// The wave's place in a per-ray launch.  A dead wave (past the last ray) works on the last ray, so that it meets every
// barrier and wave operation, and stores nothing.
struct RayWave {
    int wave, lane, ray;
    bool live;
    __device__ __forceinline__ explicit RayWave(const int R) : wave(threadIdx.x >> 6), lane(threadIdx.x & 63) {
        ray = blockIdx.x * RAY_WAVES + wave;
        live = ray < R;
        if (!live) ray = R - 1;
    }
};

// The chunked transmittance scan (fp64 carry, like the reference's CPU cumprod) over the n = S + 1 (linear) / S (constant)
// elements of a ray.  Every lane calls body(i, valid, e, f, Ti, Tn) once per chunk, valid or not (e = f = 1 when not), so
// the body may use wave operations: Ti = prod_{j<i} f_j, Tn = Ti f_i.
template <int MODE, class Body>
__device__ __forceinline__ void quad_scan(const int S, const float* zk, const float* tau, const float dnorm, const int lane,
                                          Body body) {
    const int n = (MODE == PLNERF_MODE_LINEAR) ? S + 1 : S;
    double carry = 1.0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool valid = i < n;
        float seg = 0.f, e = 1.f, f = 1.f;
        if (valid) interval<MODE>(i, S, zk, tau, dnorm, seg, e, f);
        const double incl = wave_incl_prod((double)f);
        double excl = __shfl_up(incl, 1);
        if (lane == 0) excl = 1.0;
        const float Ti = (float)(carry * excl);
        const float Tn = (float)(carry * incl);
        carry = carry * __shfl(incl, 63);
        body(i, valid, e, f, Ti, Tn);
    }
}

struct QuadOut {          // the quadrature's outputs (device pointers; weights, tau and T may be null)
    float* rgb_map;
    float* disp_map;
    float* acc_map;
    float* depth_map;
    float* weights;       // [R, n]
    float* tau;           // linear mode: [R, S+2]
    float* T;             // linear mode: [R, S+2]
};

struct QuadSums { double r = 0, g = 0, b = 0, d = 0, a = 0; };      // one lane's share of the maps

// A valid element of the scan joins the sums, and a live wave stores its weight and transmittance.  Returns the weight.
template <int MODE>
__device__ __forceinline__ float quad_element(QuadSums& s, const QuadOut& o, const int ray, const bool live, const int i,
                                              const float e, const float Ti, const float Tn, const int S, const float* zk,
                                              const float* col, const int color_mode, const int farcolorfix) {
    const int n = (MODE == PLNERF_MODE_LINEAR) ? S + 1 : S;
    const float w = (1.0f - e) * Ti;
    s.r += (double)(w * elem_colour<MODE>(i, 0, S, col, color_mode, farcolorfix));
    s.g += (double)(w * elem_colour<MODE>(i, 1, S, col, color_mode, farcolorfix));
    s.b += (double)(w * elem_colour<MODE>(i, 2, S, col, color_mode, farcolorfix));
    s.d += (double)(w * elem_depth<MODE>(i, zk));
    s.a += (double)w;
    if (live) {
        if (o.weights) o.weights[(size_t)ray * n + i] = w;
        if (MODE == PLNERF_MODE_LINEAR && o.T) o.T[(size_t)ray * (S + 2) + i + 1] = Tn;
    }
    return w;
}

// After the scan: the returned tau row and T[0] = 1 (linear mode), then the wave's sums as the ray's maps.
template <int MODE>
__device__ __forceinline__ void quad_write_maps(QuadSums s, const QuadOut& o, const int ray, const bool live, const int lane,
                                                const int S, const float* tau, const int white_bkgd) {
    if (MODE == PLNERF_MODE_LINEAR && live) {
        if (o.T && lane == 0) o.T[(size_t)ray * (S + 2)] = 1.0f;
        if (o.tau)
            for (int k = lane; k < S + 2; k += 64) o.tau[(size_t)ray * (S + 2) + k] = tau[k];
    }
    s.r = wave_sum(s.r); s.g = wave_sum(s.g); s.b = wave_sum(s.b); s.d = wave_sum(s.d); s.a = wave_sum(s.a);
    if (live && lane == 0) {
        const float acc = (float)s.a, depth = (float)s.d;
        float r = (float)s.r, g = (float)s.g, b = (float)s.b;
        if (white_bkgd) {
            const float bg = 1.0f - acc;
            r += bg; g += bg; b += bg;
        }
        o.rgb_map[3 * ray + 0] = r;
        o.rgb_map[3 * ray + 1] = g;
        o.rgb_map[3 * ray + 2] = b;
        o.depth_map[ray] = depth;
        o.acc_map[ray] = acc;
        o.disp_map[ray] = 1.0f / tmax(1e-10f, depth / acc);
    }
}

// One chunk of cdf = [0, cumsum(v)]: fp64 running sum, each entry rounded to fp32.  Every lane calls it (v = 0 when !valid).
__device__ __forceinline__ void cdf_scan_step(const int j, const bool valid, const float v, double& carry, float* cdf) {
    const double incl = wave_incl_sum((double)v);
    if (valid) cdf[j + 1] = (float)(carry + incl);
    carry = carry + __shfl(incl, 63);
}

// The piecewise-linear sampler's cdf over n weights w_of(j): entries 1 .. n; the ends are cdf_linear_ends', past a barrier.
template <class WeightOf>
__device__ __forceinline__ void cdf_linear_rows(const int n, const int lane, float* cdf, WeightOf w_of) {
    double carry = 0.0;
    for (int base = 0; base < n; base += 64) {
        const int j = base + lane;
        cdf_scan_step(j, j < n, (j < n) ? w_of(j) : 0.0f, carry, cdf);
    }
}
__device__ __forceinline__ void cdf_linear_ends(float* cdf, const int K, const int lane) {
    if (lane == 0) { cdf[0] = 0.0f; cdf[K - 1] = 1.0f; }      // (the last entry is forced to 1)
}

// sample_pdf's cdf over the LDS row wv[0 .. n) (weights + 1e-5): pdf = wv / sum(wv) with torch.sum's order and IEEE division;
// the last entry is what the sum gives, not forced to 1.
__device__ __forceinline__ void cdf_const_rows(const float* wv, const int n, const int lane, float* cdf) {
    const float total = torch_row_sum(wv, n, lane);
    double carry = 0.0;
    for (int base = 0; base < n; base += 64) {
        const int j = base + lane;
        cdf_scan_step(j, j < n, (j < n) ? wv[j] / total : 0.0f, carry, cdf);
    }
    if (lane == 0) cdf[0] = 0.0f;
}

// One draw of sample_pdf_reformulation (run_nerf_helpers.py:364-445) through the K = S + 2 entries of cdf / knots / tau / Tr.
__device__ __forceinline__ float invert_pl(const float* cdf, const float* knots, const float* tau, const float* Tr, const int S,
                                           const float u, const float zero_tol, const float eps, int& ind, float& T0,
                                           float& tau0, float& s0) {
    const int K = S + 2;
    ind = upper_bound(cdf, K, u);
    const int below = ind - 1 > 0 ? ind - 1 : 0;
    const int above = ind < K - 1 ? ind : K - 1;
    s0 = knots[below];
    const float s1 = knots[above];
    T0 = Tr[below];
    tau0 = tau[below];
    const float tau1 = tau[above];
    const int di = below < S ? below : S;               // H4: reference reads out of bounds at u == 1
    const float d = tau[di + 1] - tau[di];
    float out = (d < zero_tol && d > -zero_tol) ? s0 : -1.0f;
    const bool rising = d >= zero_tol;
    if (rising || d <= -zero_tol) out = invert_segment(s0, s1, T0, tau0, tau1, u, eps, rising);      // (one evaluation, operands selected per lane)
    if (out != out) out = s0;
    return out;
}

// One draw of sample_pdf (run_nerf_helpers.py:241-284) through the B entries of cdf; bin_of(j) is bin j.
template <class BinOf>
__device__ __forceinline__ float invert_const(const float* cdf, const int B, const float u, BinOf bin_of, int& ind) {
    ind = upper_bound(cdf, B, u);
    const int below = ind - 1 > 0 ? ind - 1 : 0;
    const int above = ind < B - 1 ? ind : B - 1;
    const float c0 = cdf[below], c1 = cdf[above];
    float denom = c1 - c0;
    if (denom < 1e-5f) denom = 1.0f;
    const float t = (u - c0) / denom;
    const float b0 = bin_of(below), b1 = bin_of(above);
    return b0 + t * (b1 - b0);
}

// sort(row) as torch.sort orders values, in registers (bitonic_sort_regs): position p = 64 r + lane of the n <= 64 KPL values
// value_of(p), then store(p, value) of the sorted row.  Two halves, because a kernel's barrier or its dead wave's return
// stands between them.
template <int KPL, class ValueOf>
__device__ __forceinline__ void sort_row_regs(uint32_t (&x)[KPL], const int n, const int lane, ValueOf value_of) {
#pragma unroll
    for (int r = 0; r < KPL; ++r) {
        const int p = 64 * r + lane;
        x[r] = p < n ? sort_key(value_of(p)) : 0xFFFFFFFFu;
    }
    bitonic_sort_regs<KPL>(x, lane);
}
template <int KPL, class Store>
__device__ __forceinline__ void store_row_regs(const uint32_t (&x)[KPL], const int n, const int lane, Store store) {
#pragma unroll
    for (int r = 0; r < KPL; ++r) {
        const int p = 64 * r + lane;
        if (p < n) store(p, sort_unkey(x[r]));
    }
}

// Four consecutive floats, from element e0 on, of the n x 3 block o + d z of one ray.
__device__ __forceinline__ float4 ray_positions4(const float3 o, const float3 d, const float* zs, const int e0) {
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int e = e0 + k, si = e / 3, c = e - 3 * si;
        const float oc = c == 0 ? o.x : (c == 1 ? o.y : o.z);
        const float dc = c == 0 ? d.x : (c == 1 ? d.y : d.z);
        v[k] = oc + dc * zs[si];
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}

// Positions o + d zs[0 .. n) of ray `ray` (o, d: rows of rays_o, rays_d [R, 3]) into its row prow [n, 3]: 16-byte stores
// where the row allows them.
__device__ __forceinline__ void ray_positions(const float* rays_o, const float* rays_d, const int ray, const float* zs,
                                              const int n, float* prow, const int lane) {
    const float3 o = make_float3(rays_o[3 * (size_t)ray], rays_o[3 * (size_t)ray + 1], rays_o[3 * (size_t)ray + 2]);
    const float3 d = make_float3(rays_d[3 * (size_t)ray], rays_d[3 * (size_t)ray + 1], rays_d[3 * (size_t)ray + 2]);
    if ((3 * n) % 4 == 0 && ((uintptr_t)prow & 15) == 0) {
        for (int q = lane; q < 3 * n / 4; q += 64) reinterpret_cast<float4*>(prow)[q] = ray_positions4(o, d, zs, 4 * q);
    } else {
        for (int e = lane; e < 3 * n; e += 64) {
            const int si = e / 3, c = e - 3 * si;
            prow[e] = (c == 0 ? o.x : (c == 1 ? o.y : o.z)) + (c == 0 ? d.x : (c == 1 ? d.y : d.z)) * zs[si];
        }
    }
}

// Coarse depths (run_plnerf.py:683-705): sample s of linspace t between near and far, in depth or in disparity ...
__device__ __forceinline__ float coarse_depth(const float nr, const float fr, const float t, const int lindisp) {
    const float omt = 1.0f - t;
    if (!lindisp) return nr * omt + fr * t;                 // near * (1 - t) + far * t
    return 1.0f / (1.0f / nr * omt + 1.0f / fr * t);        // 1 / (1/near * (1 - t) + 1/far * t)
}

// ... and jittered by t within its stratum:
// mids = .5 * (z[1:] + z[:-1]); upper = [mids, z[-1]]; lower = [z[0], mids]; z = lower + (upper - lower) * t_rand
__device__ __forceinline__ float stratified_depth(const float nr, const float fr, const float* t_vals, const int s, const int S,
                                                  const int lindisp, const float t) {
    const float z = coarse_depth(nr, fr, t_vals[s], lindisp);
    const float zl = s > 0 ? coarse_depth(nr, fr, t_vals[s - 1], lindisp) : z;
    const float zu = s + 1 < S ? coarse_depth(nr, fr, t_vals[s + 1], lindisp) : z;
    const float lower = s > 0 ? 0.5f * (z + zl) : z;
    const float upper = s + 1 < S ? 0.5f * (zu + z) : z;
    return lower + (upper - lower) * t;
}

}  // namespace plnerf
