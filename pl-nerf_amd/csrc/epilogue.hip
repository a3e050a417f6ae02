// The coarse pass's epilogue as ONE per-ray kernel (run_plnerf.py:714-735, piecewise-linear mode):
//
//     raw2outputs(raw, z)                       -> rgb0, disp0, acc0, depth0        (:553-624, weights :516-550)
//     sample_pdf_reformulation(z, w, tau, T, u) -> z_samples                        (run_nerf_helpers.py:364-445)
//     clamp(z_samples, near, far); z_std                                            (:731, :752)
//     sort(cat(z, z_samples))                   -> z_fine                            (:733-734)
//     pts = o + d * z_fine                                                          (:735)
//
// One wavefront owns one ray.  weights, tau, T and the cdf never leave the CU: they are LDS rows of the wave (the
// separate launches write them to HBM for the next launch to read back).  HBM sees raw, z and u in, the coarse maps,
// z_fine, pts and z_std out: algorithmic bytes per ray 20 S + 4 N (+44) in, 16 (S + N) + 32 out.  The scan, the
// element rule and map write, the cdfs, each draw's inversion, the general sort arm and the positions are the bodies
// the separate kernels run (ray_fwd_dev.h, over ray_dev.h's leaves), so the results are bit-identical to
// plnerf_quad_fwd -> plnerf_sample_pl -> plnerf_merge_sort -> plnerf_ray_points by construction
// (guarded by tests/test_gpu_step.py::test_fused_coarse_epilogue_equals_separate_launches).  This kernel's own: the
// LDS layout, z_std, and the rank merge of two ascending runs, which no separate launch has.
//
// Piecewise-constant mode (MODE = PLNERF_MODE_CONSTANT: the vanilla-NeRF baseline, `constant_init`, the depth script's
// constant configuration) is the same kernel with compute_weights (run_plnerf.py:504-513) as the quadrature and sample_pdf
// (run_nerf_helpers.py:241-284) on z_mid / weights[1:-1] as the sampler -- bit-identical to
// plnerf_quad_fwd -> torch z_mid -> plnerf_sample_const -> plnerf_merge_sort -> plnerf_ray_points
// (tests/test_gpu_const_epilogue.py); entry points in include/plnerf_hip_constepi.h.
#include "common.h"
#include "philox.h"
#include "ray_fwd_dev.h"
#include "../../include/plnerf_hip_constepi.h"

using namespace plnerf;

namespace {

constexpr int WAVES = RAY_WAVES;

struct EpiArgs {
    RayIn in;
    const float* rays_o;
    const float* u;          // [R, N] (stride N), one shared row [N] (stride 0), or null = drawn here (rng)
    int u_row_stride;
    RngArgs rng;
    int R, S, N;
    int color_mode, white_bkgd, farcolorfix;
    float zero_tol, eps;
    int lds_stride;
    QuadOut out;             // the coarse maps; optional weights [R, S+1] (constant mode: [R, S]), tau, T [R, S+2]
    float* z_fine;           // [R, S+N]
    float* pts;              // [R, S+N, 3]
    float* z_std;            // [R]
    // hypothesis mode (HYP: the depth-supervised variant's final stage, plnerf_fine_epilogue): the samples themselves
    float* samples;          // [R, N], NOT clamped
    int64_t* inds;           // [R, N] searchsorted indices (plnerf_sample_pl_bwd wants them)
    float* u_out;            // [R, N] the draws used (the variant's render_rays returns them)
    float* bins_out;         // constant mode, optional [R, S-1]: the sampler's bins z_mid (plnerf_sample_const_bwd wants them)
};

// HYP = false: the coarse pass's epilogue (samples clamped, merged, sorted, turned into positions).
// HYP = true: raw2outputs + the *_return_u sampler of the depth-supervised variant's LAST stage
// (run_nerf_sample_based_depth.py:923-934): the samples are the depth hypotheses pred_hyp -- not clamped, kept with their
// indices and draws for the sampler's backward -- and z_std is theirs (:934); nothing is sorted or positioned.
// KPL: registers per lane of the general sort network (64 KPL >= S + N); KS: of the samples' own network (64 KS >= N)
// MODE: the quadrature rule and its sampler.  Constant mode keeps the row layout: Tr holds the sampler's weights
// w[1:-1] + 1e-5, cdf the S - 1 entries of [0, cumsum(pdf)]; the bins z_mid are formed from zk where they are read.
template <int KPL, bool HYP, int KS = KPL, int MODE = PLNERF_MODE_LINEAR>
__global__ __launch_bounds__(256) void coarse_epilogue_kernel(const EpiArgs a) {
    constexpr bool LINEAR = MODE == PLNERF_MODE_LINEAR;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const RayWave rw(a.R);
    const int lane = rw.lane, ray = rw.ray;
    const bool live = rw.live;
    const int S = a.S, K = S + 2, N = a.N, NF = S + N;
    float* zk = smem + (size_t)rw.wave * a.lds_stride;   // K knots [near, z, far]
    float* tau = zk + K;                               // K
    float* col = tau + K;                              // 3 S
    float* Tr = col + 3 * S;                           // K  (constant mode: the sampler's S - 2 weights)
    float* cdf = Tr + K;                               // K  (constant mode: S - 1 entries)
    float* smp = cdf + K;                              // N clamped samples; later the sorted row (NF, aliases col..)
    float dnorm;
    load_ray(a.in, ray, lane, zk, tau, col, dnorm);
    __syncthreads();

    // ---- quadrature (quad_scan, as quad_fwd_kernel runs it) with the linear cdf's running sum riding along ----
    QuadSums sums;
    [[maybe_unused]] double ccarry = 0.0;
    quad_scan<MODE>(S, zk, tau, dnorm, lane, [&](const int i, const bool valid, const float e, float, const float Ti, const float Tn) {
        float w = 0.0f;
        if (valid) {
            w = quad_element<MODE>(sums, a.out, ray, live, i, e, Ti, Tn, S, zk, col, a.color_mode, a.farcolorfix);
            if constexpr (LINEAR) Tr[i + 1] = Tn;
            else if (i >= 1 && i < S - 1) Tr[i - 1] = w + 1e-5f;      // sample_pdf's weights[..., 1:-1] + 1e-5
        }
        if constexpr (LINEAR) cdf_scan_step(i, valid, w, ccarry, cdf);      // (cdf_linear_rows' step: w is in a register here)
    });
    quad_write_maps<MODE>(sums, a.out, ray, live, lane, S, tau, a.white_bkgd);
    __syncthreads();
    const int B = S - 1;          // (constant mode) bins z_mid = cdf entries
    if constexpr (LINEAR) {
        if (lane == 0) Tr[0] = 1.0f;
        cdf_linear_ends(cdf, K, lane);
    } else {
        cdf_const_rows(Tr, B - 1, lane, cdf);
        if constexpr (HYP) {
            if (live && a.bins_out)
                for (int j = lane; j < B; j += 64) a.bins_out[(size_t)ray * B + j] = 0.5f * (zk[j + 2] + zk[j + 1]);
        }
    }
    __syncthreads();

    // ---- importance samples (invert_pl / invert_const, as sample_pl_kernel / sample_const_kernel run them), clamped to
    // [near, far]; unlike the separate samplers a dead wave draws too: barriers follow ----
    const float lo = zk[0], hi = zk[K - 1];
    double ssum = 0.0;
    for (int k = lane; k < N; k += 64) {
        const float u = a.u ? a.u[(size_t)ray * a.u_row_stride + k] : rng_uniform(a.rng, a.rng.ray_id0 + ray, k);
        int ind;
        float out;
        if constexpr (LINEAR) {
            [[maybe_unused]] float T0, tau0, s0;
            out = invert_pl(cdf, zk, tau, Tr, S, u, a.zero_tol, a.eps, ind, T0, tau0, s0);
        } else {
            // z_mid = .5 * (z[1:] + z[:-1])
            out = invert_const(cdf, B, u, [&](const int j) { return 0.5f * (zk[j + 2] + zk[j + 1]); }, ind);
        }
        if constexpr (HYP) {
            if (live) {
                a.samples[(size_t)ray * N + k] = out;
                a.inds[(size_t)ray * N + k] = ind;
                if (a.u_out) a.u_out[(size_t)ray * N + k] = u;
            }
        } else {
            out = tmin(tmax(out, lo), hi);        // torch.clamp(z_samples, near, far)
        }
        smp[k] = out;
        ssum += (double)out;
    }
    // z_std = std(z_samples, unbiased=False) over the clamped samples
    ssum = wave_sum(ssum);
    const double mean = ssum / (double)N;
    __syncthreads();
    double sq = 0.0;
    for (int k = lane; k < N; k += 64) {
        const double dv = (double)smp[k] - mean;
        sq += dv * dv;
    }
    sq = wave_sum(sq);
    if (live && lane == 0) a.z_std[ray] = (float)sqrt(sq / (double)N);
    if constexpr (HYP) return;

    // ---- sort(cat(z, samples)) ----
    // The coarse depths are ascending in every reference call (stratified bins, run_plnerf.py:683-705) -- checked per ray,
    // else the general network below.  Then only the N samples need sorting (the bitonic network on KS registers: 28 stages
    // for 128 keys instead of 36 over 256), and the two ascending runs merge by rank: two binary searches per element in
    // place of the network's last eight stages.  Same multiset, same order: the same bits as sort(cat()) (round 5; the
    // launch was VALU-issue bound, profiles/r05_pmc_stream_kernels_262144rays.txt).
    uint32_t xs[KS];
#pragma unroll
    for (int r = 0; r < KS; ++r) {
        const int q = 64 * r + lane;
        xs[r] = q < N ? sort_key(smp[q]) : 0xFFFFFFFFu;
    }
    bitonic_sort_regs<KS>(xs, lane);
    bool asc = true;
    for (int p = lane; p + 1 < S; p += 64) asc = asc && (sort_key(zk[p + 1]) <= sort_key(zk[p + 2]));
    const bool merge = __all(asc) != 0;           // (per wave = per ray; every path below meets the same barriers)
    __syncthreads();                              // the sampler's and z_std's reads of tau / smp are done
    uint32_t* zkey = reinterpret_cast<uint32_t*>(tau);
    uint32_t* skey = reinterpret_cast<uint32_t*>(smp);
    if (merge) {
        for (int p = lane; p < S; p += 64) zkey[p] = sort_key(zk[p + 1]);
#pragma unroll
        for (int r = 0; r < KS; ++r) {
            const int q = 64 * r + lane;
            if (q < N) skey[q] = xs[r];
        }
    }
    __syncthreads();
    int rank_s[KS], rank_z[KPL];
    uint32_t x[KPL];
    if (merge) {
#pragma unroll
        for (int r = 0; r < KS; ++r) rank_s[r] = 64 * r + lane + count_le(zkey, S, xs[r]);
        // (the z elements' ranks read skey, which the sorted row may overwrite: all of them before the barrier)
#pragma unroll
        for (int r = 0; r < KPL; ++r) {
            const int p = 64 * r + lane;
            rank_z[r] = p < S ? p + count_lt(skey, N, zkey[p]) : -1;
        }
    } else {      // merge_sort_kernel's network (the samples are clamped already)
        sort_row_regs<KPL>(x, NF, lane, [&](const int p) { return p < S ? zk[p + 1] : smp[p - S]; });
    }
    float* zs = col;                  // NF <= 3 S + K + K + N floats from col on (col, Tr, cdf, smp are contiguous)
    // ONE barrier for both arms (`merge` is decided per wave = per ray: a barrier inside each arm was reached at different
    // program points by the waves of one workgroup -- the counts matched, the HIP programming model calls it undefined):
    // every read of col / smp / tau is done, the sorted row may overwrite them
    __syncthreads();
    if (merge) {
#pragma unroll
        for (int r = 0; r < KPL; ++r)
            if (rank_z[r] >= 0) zs[rank_z[r]] = zk[64 * r + lane + 1];
#pragma unroll
        for (int r = 0; r < KS; ++r)
            if (64 * r + lane < N) zs[rank_s[r]] = sort_unkey(xs[r]);
    } else {
        store_row_regs<KPL>(x, NF, lane, [&](const int p, const float v) { zs[p] = v; });
    }
    __syncthreads();
    if (live)
        for (int p = lane; p < NF; p += 64) a.z_fine[(size_t)ray * NF + p] = zs[p];
    if (!live) return;
    // ---- positions of the merged samples ----
    ray_positions(a.rays_o, a.in.rays_d, ray, zs, NF, a.pts + (size_t)ray * 3 * NF, lane);
}

template <int KPL, bool HYP = false, int KS = KPL, int MODE = PLNERF_MODE_LINEAR>
int launch(const EpiArgs& a, size_t lds, hipStream_t st) {
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute((const void*)coarse_epilogue_kernel<KPL, HYP, KS, MODE>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((coarse_epilogue_kernel<KPL, HYP, KS, MODE>), dim3((a.R + WAVES - 1) / WAVES), dim3(WAVES * 64), lds, st,
                       a);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}

// The coarse form's tiers.  (KS: the samples' own network; the small shapes get every size, the large ones sort their
// samples on the full width)
template <int MODE>
int launch_coarse(const EpiArgs& a, size_t lds, hipStream_t st) {
    const int nf = a.S + a.N, N = a.N;
    if (nf <= 64) return launch<1, false, 1, MODE>(a, lds, st);
    if (nf <= 128) return N <= 64 ? launch<2, false, 1, MODE>(a, lds, st) : launch<2, false, 2, MODE>(a, lds, st);
    if (nf <= 256)
        return N <= 64 ? launch<4, false, 1, MODE>(a, lds, st)
                       : (N <= 128 ? launch<4, false, 2, MODE>(a, lds, st) : launch<4, false, 4, MODE>(a, lds, st));
    if (nf <= 512) return launch<8, false, 8, MODE>(a, lds, st);
    return launch<16, false, 16, MODE>(a, lds, st);
}

// zk, tau, Tr, cdf: 4 (S+2); col 3 S; samples N   (the sorted row of S + N <= 3 S + 2 (S+2) + N reuses col onwards)
inline int lds_row(int S, int N) { return ((4 * (S + 2) + 3 * S + N) + 3) & ~3; }

}  // namespace

extern "C" int plnerf_coarse_epilogue(const float* raw, const float* z, const float* near, const float* far,
                                      const float* rays_o, const float* rays_d, const float* noise, const float* u,
                                      int u_row_stride, uint64_t seed, uint32_t step, int ray_id0, int R, int S, int N,
                                      int color_mode, int white_bkgd, int farcolorfix, float zero_tol, float epsilon,
                                      float* rgb_map, float* disp_map, float* acc_map, float* depth_map, float* weights,
                                      float* tau, float* T, float* z_fine, float* pts, float* z_std,
                                      plnerf_stream_t stream) {
    if (R < 0 || S < 2 || N < 1) return PLNERF_EINVAL;
    if (u && u_row_stride != 0 && u_row_stride != N) return PLNERF_EINVAL;
    if (color_mode != PLNERF_COLOR_MIDPOINT && color_mode != PLNERF_COLOR_LEFT) return PLNERF_EINVAL;
    if (S > PLNERF_MAX_SAMPLES || S + N > 1024) return PLNERF_ERANGE;
    if (R == 0) return PLNERF_OK;
    if (!raw || !z || !near || !far || !rays_o || !rays_d || !rgb_map || !disp_map || !acc_map || !depth_map ||
        !z_fine || !pts || !z_std)
        return PLNERF_EINVAL;
    if (!plnerf::aligned16(raw)) return PLNERF_EINVAL;      // read as float4
    EpiArgs a{};
    a.in = RayIn{raw, z, near, far, rays_d, noise, S};
    a.rays_o = rays_o; a.u = u; a.u_row_stride = u_row_stride;
    a.rng = RngArgs{(uint32_t)seed, (uint32_t)(seed >> 32), 1u, step, ray_id0, u ? 0 : 1};
    a.R = R; a.S = S; a.N = N; a.color_mode = color_mode; a.white_bkgd = white_bkgd; a.farcolorfix = farcolorfix;
    a.zero_tol = zero_tol; a.eps = epsilon;
    a.out = QuadOut{rgb_map, disp_map, acc_map, depth_map, weights, tau, T};
    a.z_fine = z_fine; a.pts = pts; a.z_std = z_std;
    a.lds_stride = lds_row(S, N);
    const size_t lds = (size_t)WAVES * a.lds_stride * sizeof(float);
    if (lds > 160 * 1024) return PLNERF_ERANGE;
    return launch_coarse<PLNERF_MODE_LINEAR>(a, lds, (hipStream_t)stream);
}


extern "C" int plnerf_fine_epilogue(const float* raw, const float* z, const float* near, const float* far,
                                    const float* rays_d, const float* noise, const float* u, int u_row_stride,
                                    uint64_t seed, uint32_t step, int ray_id0, int R, int S, int N, int color_mode,
                                    int white_bkgd, int farcolorfix, float zero_tol, float epsilon, float* rgb_map,
                                    float* disp_map, float* acc_map, float* depth_map, float* weights, float* tau,
                                    float* T, float* samples, int64_t* inds, float* u_out, float* z_std,
                                    plnerf_stream_t stream) {
    if (R < 0 || S < 2 || N < 1) return PLNERF_EINVAL;
    if (u && u_row_stride != 0 && u_row_stride != N) return PLNERF_EINVAL;
    if (color_mode != PLNERF_COLOR_MIDPOINT && color_mode != PLNERF_COLOR_LEFT) return PLNERF_EINVAL;
    if (S > PLNERF_MAX_SAMPLES || N > 1024) return PLNERF_ERANGE;
    if (R == 0) return PLNERF_OK;
    if (!raw || !z || !near || !far || !rays_d || !rgb_map || !disp_map || !acc_map || !depth_map || !weights || !tau ||
        !T || !samples || !inds || !z_std)
        return PLNERF_EINVAL;
    if (!plnerf::aligned16(raw)) return PLNERF_EINVAL;      // read as float4
    EpiArgs a{};
    a.in = RayIn{raw, z, near, far, rays_d, noise, S};
    a.u = u; a.u_row_stride = u_row_stride;
    // (stream id 4: the hypotheses' draw is not the coarse pass's importance draw, stream 1)
    a.rng = RngArgs{(uint32_t)seed, (uint32_t)(seed >> 32), 4u, step, ray_id0, u ? 0 : 1};
    a.R = R; a.S = S; a.N = N; a.color_mode = color_mode; a.white_bkgd = white_bkgd; a.farcolorfix = farcolorfix;
    a.zero_tol = zero_tol; a.eps = epsilon;
    a.out = QuadOut{rgb_map, disp_map, acc_map, depth_map, weights, tau, T};
    a.z_std = z_std;
    a.samples = samples; a.inds = inds; a.u_out = u_out;
    a.lds_stride = lds_row(S, N);
    const size_t lds = (size_t)WAVES * a.lds_stride * sizeof(float);
    if (lds > 160 * 1024) return PLNERF_ERANGE;
    return launch<1, true>(a, lds, (hipStream_t)stream);      // (KPL sizes the sort network only: unused here)
}


// ---- piecewise-constant mode (include/plnerf_hip_constepi.h) ----
extern "C" int plnerf_coarse_epilogue_const(const float* raw, const float* z, const float* near, const float* far,
                                            const float* rays_o, const float* rays_d, const float* noise, const float* u,
                                            int u_row_stride, uint64_t seed, uint32_t step, int ray_id0, int R, int S, int N,
                                            int white_bkgd, float* rgb_map, float* disp_map, float* acc_map,
                                            float* depth_map, float* weights, float* z_fine, float* pts, float* z_std,
                                            plnerf_stream_t stream) {
    if (R < 0 || S < 3 || N < 1) return PLNERF_EINVAL;      // (S >= 3: the sampler needs one interior weight)
    if (u && u_row_stride != 0 && u_row_stride != N) return PLNERF_EINVAL;
    if (S > PLNERF_MAX_SAMPLES || S + N > 1024) return PLNERF_ERANGE;
    if (R == 0) return PLNERF_OK;
    if (!raw || !z || !near || !far || !rays_o || !rays_d || !rgb_map || !disp_map || !acc_map || !depth_map ||
        !z_fine || !pts || !z_std)
        return PLNERF_EINVAL;
    if (!plnerf::aligned16(raw)) return PLNERF_EINVAL;      // read as float4
    EpiArgs a{};
    a.in = RayIn{raw, z, near, far, rays_d, noise, S};
    a.rays_o = rays_o; a.u = u; a.u_row_stride = u_row_stride;
    a.rng = RngArgs{(uint32_t)seed, (uint32_t)(seed >> 32), 1u, step, ray_id0, u ? 0 : 1};
    a.R = R; a.S = S; a.N = N; a.white_bkgd = white_bkgd;
    a.out = QuadOut{rgb_map, disp_map, acc_map, depth_map, weights, nullptr, nullptr};
    a.z_fine = z_fine; a.pts = pts; a.z_std = z_std;
    a.lds_stride = lds_row(S, N);
    const size_t lds = (size_t)WAVES * a.lds_stride * sizeof(float);
    if (lds > 160 * 1024) return PLNERF_ERANGE;
    return launch_coarse<PLNERF_MODE_CONSTANT>(a, lds, (hipStream_t)stream);
}

extern "C" int plnerf_fine_epilogue_const(const float* raw, const float* z, const float* near, const float* far,
                                          const float* rays_d, const float* noise, const float* u, int u_row_stride,
                                          uint64_t seed, uint32_t step, int ray_id0, int R, int S, int N, int white_bkgd,
                                          float* rgb_map, float* disp_map, float* acc_map, float* depth_map, float* weights,
                                          float* bins_out, float* samples, int64_t* inds, float* u_out, float* z_std,
                                          plnerf_stream_t stream) {
    if (R < 0 || S < 3 || N < 1) return PLNERF_EINVAL;
    if (u && u_row_stride != 0 && u_row_stride != N) return PLNERF_EINVAL;
    if (S > PLNERF_MAX_SAMPLES || N > 1024) return PLNERF_ERANGE;
    if (R == 0) return PLNERF_OK;
    if (!raw || !z || !near || !far || !rays_d || !rgb_map || !disp_map || !acc_map || !depth_map || !weights ||
        !samples || !inds || !z_std)
        return PLNERF_EINVAL;
    if (!plnerf::aligned16(raw)) return PLNERF_EINVAL;      // read as float4
    EpiArgs a{};
    a.in = RayIn{raw, z, near, far, rays_d, noise, S};
    a.u = u; a.u_row_stride = u_row_stride;
    a.rng = RngArgs{(uint32_t)seed, (uint32_t)(seed >> 32), 4u, step, ray_id0, u ? 0 : 1};      // (stream 4: as plnerf_fine_epilogue)
    a.R = R; a.S = S; a.N = N; a.white_bkgd = white_bkgd;
    a.out = QuadOut{rgb_map, disp_map, acc_map, depth_map, weights, nullptr, nullptr};
    a.z_std = z_std;
    a.samples = samples; a.inds = inds; a.u_out = u_out; a.bins_out = bins_out;
    a.lds_stride = lds_row(S, N);
    const size_t lds = (size_t)WAVES * a.lds_stride * sizeof(float);
    if (lds > 160 * 1024) return PLNERF_ERANGE;
    return launch<1, true, 1, PLNERF_MODE_CONSTANT>(a, lds, (hipStream_t)stream);
}
