// The per-ray backward bodies that more than one kernel runs: the quadrature's backward (quad.hip's quad_bwd_kernel) and the
// constant-mode sampler's (sampler.hip's sample_const_bwd_kernel), each as a device function over one wave's LDS row, so that
// the fused backward of the constant-mode final stage (epilogue_bwd.hip) computes bit for bit what the two launches compute.
// Everything that includes this is built with -ffp-contract=off.
#pragma once
#include "common.h"
#include "ray_fwd_dev.h"

namespace plnerf {

struct QuadArgs {
    const float* raw;
    const float* z;
    const float* near;
    const float* far;
    const float* rays_d;
    const float* noise;
    int R, S;
    int color_mode, white_bkgd, farcolorfix;
    int lds_stride;  // floats per wave
    QuadOut out;     // forward outputs
    // backward inputs / output
    const float* g_rgb;
    const float* g_depth;
    const float* g_acc;
    const float* g_weights;
    const float* g_tau;   // linear mode: upstream gradient of the returned tau [R,S+2] (or nullptr)
    const float* g_T;     // linear mode: upstream gradient of the returned T   [R,S+2] (or nullptr)
    float* g_raw;
    // backward by-product (may be null): max |g_raw| of each workgroup's rays as fp32 bits, [ceil(R / WAVES)] -- the
    // candidates of the half dz planes' launch scale, which plnerf_mlp_bwd otherwise finds with a pass of its own over g_raw
    unsigned* absmax_out;
    // backward, the ray geometry's gradient (all four or none; plnerf_quad_bwd_rays): what autograd gives the reference
    // for z_vals [R,S], near, far [R] (the outer knots of the piecewise-linear rule; zero in constant mode) and for
    // |rays_d| [R], which scales every interval
    float* g_z;
    float* g_near;
    float* g_far;
    float* g_dnorm;
};

// The weights' upstream gradient of element i joins G: the caller's g_weights [R,n] (HBM), an LDS row g_in [n] (the sampler's
// backward, padded), or their sum -- one fp32 add, as torch's `g_weights + g_in` before the separate launch.
__device__ __forceinline__ float add_upstream_weights(const QuadArgs& a, const float* g_in, const int ray, const int n,
                                                      const int i, const float G) {
    if (g_in) return G + (a.g_weights ? a.g_weights[(size_t)ray * n + i] + g_in[i] : g_in[i]);
    if (a.g_weights) return G + a.g_weights[(size_t)ray * n + i];
    return G;
}

// Backward.  With w_i = (1-e_i) T_i and T_i = prod_{j<i} f_j:
//   dL/de_k = T_k (X_k - G_k),  X_k = sum_{i>k} G_i (1-e_i) prod_{k<j<i} f_j
// (division-free, so exact even when some e_k underflows to 0, like autograd's cumprod
// backward).  X obeys the reverse recurrence X_k = G_{k+1}(1-e_{k+1}) + f_{k+1} X_{k+1},
// evaluated as a wave scan over affine maps.
// The returned transmittances T_m = prod_{j<m} f_j (m = 1..S+1) can carry their own upstream
// gradient H_m (the depth-supervised variant differentiates through the sampler,
// depth_supervised_exps/run_nerf_sample_based_depth.py:923-934): that adds T_k Y_k to dL/de_k with
// Y_k = H_{k+1} + f_{k+1} Y_{k+1}, the same recurrence -- so H_m simply joins the additive term.
// The returned tau[s+1] = relu(sigma_s + noise_s) passes its upstream gradient straight to sigma_s.
// (The body of quad_bwd_kernel (quad.hip) and of the second phase of fine_epilogue_const_bwd_kernel (epilogue_bwd.hip): `row` is
// the wave's LDS row; g_in, when given, is an LDS row of n entries that joins the weights' upstream gradient.)
template <int MODE>
__device__ __forceinline__ void quad_bwd_rows(const QuadArgs& a, const int ray, const bool live, const int wave, const int lane,
                                              float* row, unsigned* wave_max_bits, const float* g_in) {
    const int S = a.S;
    const int n = (MODE == PLNERF_MODE_LINEAR) ? S + 1 : S;
    float* zk = row;
    float* tau = zk + (S + 2);
    float* col = tau + (S + 2);
    float* fv = col + 3 * S;     // f_i (fv[n] = 1)
    float* av = fv + (n + 1);    // G_i (1 - e_i)  (av[n] = 0)
    float* wv = av + (n + 1);    // w_i
    float* qv = wv + (n + 1);    // T_i, then Q_i = dL/de_i * seg_i * e_i
    float* sv = qv + (n + 1);    // (only with g_z) dL/dseg_i = dL/de_i * e_i * (-density of the interval)
    float dnorm;
    load_ray(RayIn{a.raw, a.z, a.near, a.far, a.rays_d, a.noise, a.S}, ray, lane, zk, tau, col, dnorm);
    const float gr = a.g_rgb[3 * ray + 0], gg = a.g_rgb[3 * ray + 1], gb = a.g_rgb[3 * ray + 2];
    const float gdep = a.g_depth ? a.g_depth[ray] : 0.0f;
    float gacc = a.g_acc ? a.g_acc[ray] : 0.0f;
    if (a.white_bkgd) gacc -= (gr + gg + gb);
    __syncthreads();

    // pass 1: forward scan, stash per-element terms
    quad_scan<MODE>(S, zk, tau, dnorm, lane, [&](const int i, const bool valid, const float e, const float f, const float Ti, float) {
        if (valid) {
            float G = gr * elem_colour<MODE>(i, 0, S, col, a.color_mode, a.farcolorfix) +
                      gg * elem_colour<MODE>(i, 1, S, col, a.color_mode, a.farcolorfix) +
                      gb * elem_colour<MODE>(i, 2, S, col, a.color_mode, a.farcolorfix) +
                      gdep * elem_depth<MODE>(i, zk) + gacc;
            G = add_upstream_weights(a, g_in, ray, n, i, G);
            fv[i] = f;
            av[i] = G * (1.0f - e) + ((MODE == PLNERF_MODE_LINEAR && a.g_T) ? a.g_T[(size_t)ray * (S + 2) + i] : 0.0f);
            wv[i] = (1.0f - e) * Ti;
            qv[i] = Ti;   // G_i and seg_i are recomputed in pass 2 (cheaper than two more LDS rows)
        }
    });
    if (lane == 0) {
        fv[n] = 1.0f;
        av[n] = (MODE == PLNERF_MODE_LINEAR && a.g_T) ? a.g_T[(size_t)ray * (S + 2) + n] : 0.0f;
    }
    __syncthreads();

    // pass 2: reverse affine scan.  Position p = n-1-i ascending <=> i descending;
    // y_p = A_p + F_p y_{p-1} with A_p = av[i+1], F_p = fv[i+1], y_{-1} = 0.
    float ycarry = 0.0f;
    for (int base = 0; base < n; base += 64) {
        const int p = base + lane;
        const bool valid = p < n;
        const int i = n - 1 - p;
        float A = 0.0f, F = 1.0f;
        if (valid) { A = av[i + 1]; F = fv[i + 1]; }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float Alo = __shfl_up(A, d), Flo = __shfl_up(F, d);
            if (lane >= d) { A = A + F * Alo; F = F * Flo; }
        }
        const float X = A + F * ycarry;            // X_i
        ycarry = __shfl(X, 63);
        if (valid) {
            float seg, e, f;
            interval<MODE>(i, S, zk, tau, dnorm, seg, e, f);
            // (G_i = av[i] / (1-e_i) would divide by zero when e_i == 1: recompute it)
            float G = gr * elem_colour<MODE>(i, 0, S, col, a.color_mode, a.farcolorfix) +
                      gg * elem_colour<MODE>(i, 1, S, col, a.color_mode, a.farcolorfix) +
                      gb * elem_colour<MODE>(i, 2, S, col, a.color_mode, a.farcolorfix) +
                      gdep * elem_depth<MODE>(i, zk) + gacc;
            G = add_upstream_weights(a, g_in, ray, n, i, G);
            const float Ti = qv[i];
            const float dLde = Ti * (X - G);
            qv[i] = dLde * seg * e;                // Q_i
            if (a.g_z) {                           // e_i = exp(-dens_i seg_i)
                const float dens = (MODE == PLNERF_MODE_LINEAR) ? 0.5f * (tau[i + 1] + tau[i]) : tau[i + 1];
                sv[i] = (dLde * e) * (-dens);
            }
        }
    }
    __syncthreads();

    // pass 3: per-sample gradients
    if (live) {
        float4* out = reinterpret_cast<float4*>(a.g_raw) + (size_t)ray * S;
        float gmax = 0.0f;
        for (int s = lane; s < S; s += 64) {
            float gtau, coef;
            if (MODE == PLNERF_MODE_LINEAR) {
                gtau = -0.5f * (qv[s + 1] + qv[s]);
                if (a.g_tau) gtau += a.g_tau[(size_t)ray * (S + 2) + s + 1];
                if (a.color_mode == PLNERF_COLOR_MIDPOINT) {
                    coef = 0.5f * (wv[s] + wv[s + 1]);
                    if (s == 0) coef += 0.5f * wv[0];
                    if (s == S - 1 && !a.farcolorfix) coef += 0.5f * wv[S];
                } else {
                    coef = wv[s + 1];
                    if (s == 0) coef += wv[0];
                }
            } else {
                gtau = -qv[s];
                coef = wv[s];
            }
            const float c0 = col[3 * s + 0], c1 = col[3 * s + 1], c2 = col[3 * s + 2];
            float4 g;
            g.x = gr * coef * (c0 * (1.0f - c0));
            g.y = gg * coef * (c1 * (1.0f - c1));
            g.z = gb * coef * (c2 * (1.0f - c2));
            g.w = (tau[s + 1] > 0.0f) ? gtau : 0.0f;
            out[s] = g;
            const float c[4] = {fabsf(g.x), fabsf(g.y), fabsf(g.z), fabsf(g.w)};
#pragma unroll
            for (int k = 0; k < 4; ++k) gmax = (c[k] > gmax || c[k] != c[k]) ? c[k] : gmax;   // a NaN sticks (and orders above every float as bits)
        }
        if (a.absmax_out) {      // (uniform)
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const float o = __shfl_xor(gmax, d);
                gmax = (o > gmax || o != o) ? o : gmax;
            }
            if (lane == 0) wave_max_bits[wave] = __float_as_uint(gmax);
        }
    }
    if (a.g_z && live) {
        // seg_i = (knot_{i+1} - knot_i) |d|, the depth map weighs the elements' depths: a knot collects from the two
        // elements it bounds.  Linear: knots [near, z, far], element i between knots i and i + 1, depth = their mean.
        // Constant: element i from z_i to z_{i+1} (the last one is 1e10 |d| long), depth = z_i.
        double gdn = 0.0;      // (up to 1023 terms that cancel: fp64, rounded once -- off every training path)
        if (MODE == PLNERF_MODE_LINEAR) {
            for (int k = lane; k < S + 2; k += 64) {
                const float s_lo = k > 0 ? sv[k - 1] : 0.0f, s_hi = k <= S ? sv[k] : 0.0f;
                const float w_lo = k > 0 ? wv[k - 1] : 0.0f, w_hi = k <= S ? wv[k] : 0.0f;
                const float g = dnorm * (s_lo - s_hi) + gdep * (0.5f * (w_lo + w_hi));
                if (k == 0) a.g_near[ray] = g;
                else if (k == S + 1) a.g_far[ray] = g;
                else a.g_z[(size_t)ray * S + k - 1] = g;
                if (k <= S) gdn += (double)sv[k] * (double)(zk[k + 1] - zk[k]);
            }
        } else {
            for (int k = lane; k < S; k += 64) {
                const float s_lo = k > 0 ? sv[k - 1] : 0.0f, s_hi = k < S - 1 ? sv[k] : 0.0f;
                a.g_z[(size_t)ray * S + k] = dnorm * (s_lo - s_hi) + gdep * wv[k];
                gdn += (double)sv[k] * (double)(k < S - 1 ? zk[k + 2] - zk[k + 1] : 1e10f);
            }
            if (lane == 0) { a.g_near[ray] = 0.0f; a.g_far[ray] = 0.0f; }
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) gdn += __shfl_xor(gdn, d);
        if (lane == 0) a.g_dnorm[ray] = (float)gdn;
    }
    if (a.absmax_out) {
        // One plain store per workgroup, no atomic: 4096 atomicMax on one address cost the launch 46 us of serialised L2
        // round trips (14 -> 60 us, round 5) -- every workgroup of this grid is resident at once, so "skip if the word
        // already holds more" skips nothing.  The consumer (the dgrad kernel's prologue) takes the maximum of the array.
        if (!live && lane == 0) wave_max_bits[wave] = 0u;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned m = wave_max_bits[0];      // (non-negative floats and NaNs order as unsigned integers; a NaN sticks)
#pragma unroll
            for (int w = 1; w < RAY_WAVES; ++w) m = wave_max_bits[w] > m ? wave_max_bits[w] : m;
            a.absmax_out[blockIdx.x] = m;
        }
    }
}

struct SampleConstBwdIn {      // the sampler's saved operands (device pointers) of one launch
    const float* bins;         // [R,B]
    const float* weights;      // row r at weights + r * w_row_stride, n = B - 1 entries (a slice of a wider row is read in place)
    int w_row_stride;
    const float* u;
    int u_row_stride;
    const int64_t* inds;
    const float* g_samples;    // [R,N]
    int B, N;
};

// floats of the wave's LDS row of sample_const_bwd_rows (the fp64 cdf included)
__host__ __device__ inline int sample_const_bwd_row_floats(int B, int N) { return 6 * B + 4 * N; }

// floats of the wave's LDS row of fine_epilogue_const_bwd_kernel (epilogue_bwd.hip): the padded g_in row of S entries, then the
// sampler's rows (B = S - 1) overlaid by the constant-mode quadrature's (plnerf_quad_bwd's 5 S + 4 + 4 (S + 2))
__host__ __device__ inline int fine_const_bwd_row_floats(int S, int N) {
    const int sampler = sample_const_bwd_row_floats(S - 1, N), quad = 5 * S + 4 + 4 * (S + 2);
    return ((S + 3) & ~3) + (((sampler > quad ? sampler : quad) + 3) & ~3);
}

// Backward of sample_const_kernel with respect to `weights` (what autograd derives for sample_pdf_return_u,
// depth_supervised_exps/model/run_nerf_helpers.py:343-394, when pred_hyp carries a loss in constant mode):
//   sample = b0 + t (b1 - b0),  t = (u - c0) / denom,  denom = c1 - c0 (or 1 where that is < 1e-5)
//   cdf[j] = sum_{i<j} pdf[i],  pdf = w' / sum(w'),  w' = w + 1e-5
// Per-knot sums run in sample order and the suffix sums are wave scans: deterministic, no atomics.
// Leaves g_pdf in row[0 .. n) (n = B - 1), the fp32 row total and sum_k g_pdf[k] pdf[k]: the gradient of weight i is
// (row[i] - dot) / total.  Ends on a barrier; every wave of the workgroup calls it (a dead wave on a clamped ray).
__device__ __forceinline__ void sample_const_bwd_rows(const SampleConstBwdIn& a, const int ray, const int lane, float* row,
                                                      float& total_out, float& dot_out) {
    const int B = a.B, n = a.B - 1, N = a.N;
    float* cdf = row;                            // B
    float* bins = cdf + B;                      // B
    float* wv = bins + B;                       // n  (weights + 1e-5), later g_pdf
    float* g0 = wv + B;                         // N: gradient landing on cdf[below]
    float* g1 = g0 + N;                         // N: on cdf[above]
    int* lo = reinterpret_cast<int*>(g1 + N);   // N
    int* hi = lo + N;                           // N
    float* gc = reinterpret_cast<float*>(hi + N);   // B: g_cdf
    // the cdf before its rounding to fp32 (round 6): c1 - c0 of two fp32 roundings carries 6e-8 / (c1 - c0) -- 1e-3 of the gradient
    // on a narrow bin, in the reference's fp32 autograd and in this kernel until then; the derivative's VALUE now comes from these,
    // which bins count as empty (c1 - c0 < 1e-5) stays the forward's fp32 decision (as plnerf_sample_pl_bwd: LABNOTES R6-13)
    double* cdf64 = reinterpret_cast<double*>(gc + B);      // B  (4 B + 4 N floats precede it: 8-byte aligned)
    for (int j = lane; j < B; j += 64) bins[j] = a.bins[(size_t)ray * B + j];
    for (int j = lane; j < n; j += 64) wv[j] = a.weights[(size_t)ray * a.w_row_stride + j] + 1e-5f;
    __syncthreads();
    const float total = torch_row_sum(wv, n, lane);
    double total64 = 0.0;      // (the same row in fp64, from the fp32 weights: w + 1e-5 and its sum before any rounding)
    for (int j = lane; j < n; j += 64) total64 += (double)a.weights[(size_t)ray * a.w_row_stride + j] + 1e-5;
    total64 = wave_sum(total64);
    double carry = 0.0, carry64 = 0.0;
    for (int base = 0; base < n; base += 64) {
        const int j = base + lane;
        const float pdf = (j < n) ? wv[j] / total : 0.0f;
        const double incl = wave_incl_sum((double)pdf);
        const double incl64 = wave_incl_sum((j < n) ? ((double)a.weights[(size_t)ray * a.w_row_stride + j] + 1e-5) / total64 : 0.0);
        if (j < n) { cdf[j + 1] = (float)(carry + incl); cdf64[j + 1] = carry64 + incl64; }
        carry = carry + __shfl(incl, 63);
        carry64 = carry64 + __shfl(incl64, 63);
    }
    if (lane == 0) { cdf[0] = 0.0f; cdf64[0] = 0.0; }
    __syncthreads();
    const float* urow = a.u + (size_t)ray * a.u_row_stride;
    for (int k = lane; k < N; k += 64) {
        const size_t o = (size_t)ray * N + k;
        const float u = urow[k];
        const int ind = (int)a.inds[o];
        const int below = ind - 1 > 0 ? ind - 1 : 0;
        const int above = ind < B - 1 ? ind : B - 1;
        const float c0 = cdf[below], c1 = cdf[above];
        const float d = c1 - c0;
        const bool active = !(d < 1e-5f);
        const double c0d = cdf64[below];
        const double denom = active ? cdf64[above] - c0d : 1.0;
        const double gt = (double)a.g_samples[o] * ((double)bins[above] - (double)bins[below]);
        const double q = ((double)u - c0d) / denom;            // = t
        // dt/dc0 = -1/denom + [active] t/denom ;  dt/dc1 = -[active] t/denom
        g0[k] = (float)(gt * ((-1.0 / denom) + (active ? q / denom : 0.0)));
        g1[k] = active ? (float)(gt * (-(q / denom))) : 0.0f;
        lo[k] = below; hi[k] = above;
    }
    __syncthreads();
    for (int j = lane; j < B; j += 64) {
        float sacc = 0.0f;
        for (int k = 0; k < N; ++k) {
            if (lo[k] == j) sacc += g0[k];
            if (hi[k] == j) sacc += g1[k];
        }
        gc[j] = sacc;
    }
    __syncthreads();
    // g_pdf[i] = sum_{j > i} g_cdf[j]  (i = 0..n-1): suffix sums, scanned from the top in fp64
    double tail = 0.0, dot = 0.0;
    for (int base = 0; base < n; base += 64) {
        const int p = base + lane;                  // position from the top: i = n - 1 - p, adds g_cdf[i + 1]
        const int i = n - 1 - p;
        const double v = (p < n) ? (double)gc[i + 1] : 0.0;
        const double incl = wave_incl_sum(v);
        if (p < n) {
            const float gp = (float)(tail + incl);
            dot += (double)gp * (double)(wv[i] / total);   // sum_k g_pdf[k] pdf[k]
            cdf[i] = gp;                                      // g_pdf (the cdf row is no longer needed)
        }
        tail = tail + __shfl(incl, 63);
    }
    dot_out = (float)wave_sum(dot);
    total_out = total;
    __syncthreads();
}

}  // namespace plnerf
