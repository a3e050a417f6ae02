// What the one-call entries share (train_step.hip, depth_train_step.hip, render_view.hip, depth_render_view.hip): what a pass
// over R rays needs as plain data (Pass, Rays, Samples, ...), the checks every configuration gets, the workspace carver and
// its common blocks, the stages (forward, depth_last_stage, backward_nets, block_maps: each a sequence of this library's own
// entry points) and the small scaling kernel that stands for torch's `tensor * python_float` between two launches.
// No function here knows which entry calls it: what differs between the entries arrives as data (a NULL `saved`, a
// farcolorfix of 0, input_scale / density_beta of 1 / 0, output pointers, the configuration's mode).
#pragma once
#include "common.h"
#include "../../include/plnerf_hip_step.h"
#include "../../include/plnerf_hip_view.h"      // (plnerf_view_net; brings plnerf_hip_constepi.h)
#include "../../include/experimental/plnerf_hip_unique.h"

namespace plnerf_step {

constexpr size_t ALIGN = 256;
constexpr uint32_t NOISE_STREAM = 2;      // functional.DrawSource.NOISE: the coarse pass's density noise; the fine pass's is + 1

#define STEP_OK(call) do { rc = (call); if (rc) return rc; } while (0)

// x[i] *= s over two buffers in one launch (torch: `t * python_float`, the scalar rounded to fp32 first)
static __global__ __launch_bounds__(256) void scale2_kernel(float* __restrict__ a, const size_t na, float* __restrict__ b,
                                                            const size_t nb, const float s) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < na) a[i] = a[i] * s;
    else if (i < na + nb) b[i - na] = b[i - na] * s;
}

static inline int scale2(float* a, size_t na, float* b, size_t nb, float s, hipStream_t st) {
    const size_t n = na + nb;
    if (n == 0) return PLNERF_OK;
    hipLaunchKernelGGL(scale2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, na, b, nb, s);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}

// ---- what a pass needs ----

// The scalars plnerf_step_config, plnerf_depth_step_config and plnerf_depth_view_config carry under the same names, and the
// per-call ones.  Flags are 0 / 1.
struct Pass {
    uint64_t seed;
    uint32_t step;
    int ray_id0;      // global id of the first ray
    int R, S, N;      // rays, coarse samples and importance samples per ray
    int mode, color_mode, white_bkgd, farcolorfix;
    float zero_tol, epsilon;
    int lindisp, perturb;
    float raw_noise_std;
    int precision, input_ch, input_ch_views;
    float input_scale, density_beta;
    int fwd_kernel;
    const float *t_vals, *u_vals;
};

// mode, farcolorfix, input_scale, density_beta: not every configuration has them (the NVS entries pass 1 / 0 for the last
// two, the depth entries 0 for farcolorfix, which that script's raw2outputs ignores)
template <typename Config>
static inline Pass make_pass(const Config& c, int mode, int farcolorfix, float input_scale, float density_beta, int R, int ray_id0,
                             uint32_t step, const float* t_vals, const float* u_vals) {
    Pass ps{};
    ps.seed = c.seed; ps.step = step; ps.ray_id0 = ray_id0;
    ps.R = R; ps.S = c.n_samples; ps.N = c.n_importance;
    ps.mode = mode; ps.color_mode = c.color_mode; ps.white_bkgd = c.white_bkgd ? 1 : 0; ps.farcolorfix = farcolorfix ? 1 : 0;
    ps.zero_tol = c.zero_tol; ps.epsilon = c.epsilon;
    ps.lindisp = c.lindisp ? 1 : 0; ps.perturb = c.perturb ? 1 : 0;
    ps.raw_noise_std = c.raw_noise_std;
    ps.precision = c.precision; ps.input_ch = c.input_ch; ps.input_ch_views = c.input_ch_views;
    ps.input_scale = input_scale; ps.density_beta = density_beta;
    ps.fwd_kernel = c.fwd_kernel;
    ps.t_vals = t_vals; ps.u_vals = u_vals;
    return ps;
}

struct Rays { float *o, *d, *viewdirs, *near, *far; };
// one pass's samples; noise: NULL without density noise; saved: NULL when no backward follows
struct Samples { float *z, *pts, *raw, *noise; void* saved; };
struct CoarseMaps { float *rgb0, *disp0, *acc0, *depth0, *z_std; };
struct FineMaps { float *rgb, *disp, *acc, *depth; };
// what the depth variant's last stage writes besides the maps: see depth_last_stage
struct HypPlanes { float *w, *tau, *T, *hyp; int64_t* inds; float *u_used, *z_std; };
// what the backward of both networks writes and works in
// (uniq_f: the fine pass's unique-row workspace, include/experimental/plnerf_hip_unique.h; NULL where the entry carves none
// and, in the Backward an entry hands to backward_nets(), where this step's fine pass took the plain forward)
struct Backward { float *g_raw_c, *g_raw_f; uint32_t *absmax_c, *absmax_f; void *bwd_c, *bwd_f; void* uniq_f; };
// a block's planes of a view entry
struct ViewMaps { FineMaps fine; CoarseMaps coarse; };

// ---- the checks ----

// the piecewise-constant sampler needs one interior weight
static inline int min_samples(int mode) { return mode == PLNERF_MODE_LINEAR ? 2 : 3; }

// What every configuration is checked for, ps.R being its max_rays.  max_total: the cap on S + N (the last stage's limit);
// extra_cols: the columns beyond S + N of the widest plane with R rows.  Sums and products in 64 bits: no count can overflow.
static inline int check_pass(const Pass& ps, int min_s, int max_total, int extra_cols) {
    if (ps.mode != PLNERF_MODE_LINEAR && ps.mode != PLNERF_MODE_CONSTANT) return PLNERF_EINVAL;
    if (ps.R < 1 || ps.S < min_s || ps.N < 1) return PLNERF_EINVAL;
    if (ps.color_mode != PLNERF_COLOR_MIDPOINT && ps.color_mode != PLNERF_COLOR_LEFT) return PLNERF_EINVAL;
    if (ps.fwd_kernel != PLNERF_FWD_KERNEL_AUTO && ps.fwd_kernel != PLNERF_FWD_KERNEL_RR && ps.fwd_kernel != PLNERF_FWD_KERNEL_PP)
        return PLNERF_EINVAL;
    if (!(ps.raw_noise_std >= 0.0f) || !(ps.density_beta >= 0.0f) || !(ps.input_scale > 0.0f)) return PLNERF_EINVAL;
    // the in-kernel encoding's widths (plnerf_mlp_fwd without `embedded`)
    if (ps.input_ch < 3 || ps.input_ch > 63 || (ps.input_ch - 3) % 6 != 0 || ps.input_ch_views < 3 || ps.input_ch_views > 27 ||
        (ps.input_ch_views - 3) % 6 != 0)
        return PLNERF_EINVAL;
    if (plnerf_mlp_packed_bytes(ps.precision) == 0) return PLNERF_ENOSYS;
    const int64_t total = (int64_t)ps.S + (int64_t)ps.N;
    if (ps.S > PLNERF_MAX_SAMPLES || total > max_total) return PLNERF_ERANGE;
    // (row counts are ints throughout the ABI)
    if ((uint64_t)ps.R * (uint64_t)(total + extra_cols) > (uint64_t)INT32_MAX / 4) return PLNERF_ERANGE;
    return PLNERF_OK;
}

static inline int check_net(const plnerf_step_net* n) {
    if (!n->param_flat || !n->grad_flat || !n->exp_avg || !n->exp_avg_sq || !n->packed || n->n_params < 1) return PLNERF_EINVAL;
    for (int i = 0; i < PLNERF_N_PARAM_TENSORS; ++i)
        if (!n->params[i] || n->params[i] < n->param_flat || n->params[i] >= n->param_flat + n->n_params) return PLNERF_EINVAL;
    return PLNERF_OK;
}

static inline int check_net(const plnerf_view_net* n) {
    if (!n->packed) return PLNERF_EINVAL;
    for (int i = 0; i < PLNERF_N_PARAM_TENSORS; ++i)
        if (!n->params[i]) return PLNERF_EINVAL;
    return PLNERF_OK;
}

// feature_linear.weight / .bias (params[18], [19]) are copied as float4 by plnerf_mlp_pack_weights, which refuses them
// unless they are 16-byte aligned: the one-call entries look BEFORE their first launch (a refused call enqueues nothing),
// as the last of their argument checks, so that every other refusal keeps the code it had
static inline int check_params_aligned(const float* const* params) {
    return (plnerf::aligned16(params[18]) && plnerf::aligned16(params[19])) ? PLNERF_OK : PLNERF_EINVAL;
}

// ---- the workspace ----

struct Carver {
    unsigned char* base;
    size_t off;
    template <typename T>
    T* take(size_t nbytes) {
        T* p = (T*)(base + off);      // (base may be NULL: the size query only adds up)
        off += (nbytes + ALIGN - 1) / ALIGN * ALIGN;
        return p;
    }
    float* floats(size_t n) { return take<float>(n * sizeof(float)); }

    // The blocks the entries have in common, each taken in its struct's order of fields (a braced list is evaluated from
    // left to right).  Each entry takes the blocks in an order of its own, which is what fixes its offsets.
    Rays rays(size_t R) { return Rays{floats(3 * R), floats(3 * R), floats(3 * R), floats(R), floats(R)}; }
    // one pass of K samples per ray (saved: carved by backward(), behind everything else)
    Samples samples(size_t R, size_t K, bool noise) {
        return Samples{floats(R * K), floats(3 * R * K), floats(4 * R * K), noise ? floats(R * K) : nullptr, nullptr};
    }
    CoarseMaps coarse_maps(size_t R) { return CoarseMaps{floats(3 * R), floats(R), floats(R), floats(R), floats(R)}; }
    FineMaps fine_maps(size_t R) { return FineMaps{floats(3 * R), floats(R), floats(R), floats(R)}; }
    // a block of every plane a view's caller may leave out (the colour is the caller's always)
    ViewMaps view_maps(size_t R) { return ViewMaps{FineMaps{nullptr, floats(R), floats(R), floats(R)}, coarse_maps(R)}; }
    // the steps' tail: d loss / d raw of either pass, max |g_raw| per group of rays, then both passes' saved activations
    // and the backward's scratch
    // (unique: the block of the fine pass's unique-row forward behind everything else -- the NVS steps)
    Backward backward(size_t R, size_t S, size_t F, int precision, Samples* coarse, Samples* fine, bool unique = false) {
        Backward b{};
        b.g_raw_c = floats(4 * R * S); b.g_raw_f = floats(4 * R * F);
        const size_t groups = (R + PLNERF_QUAD_RAYS_PER_GROUP - 1) / PLNERF_QUAD_RAYS_PER_GROUP;
        b.absmax_c = take<uint32_t>(groups * sizeof(uint32_t)); b.absmax_f = take<uint32_t>(groups * sizeof(uint32_t));
        coarse->saved = take<void>(plnerf_mlp_saved_bytes((int)(R * S), precision));
        fine->saved = take<void>(plnerf_mlp_saved_bytes((int)(R * F), precision));
        b.bwd_c = take<void>(plnerf_mlp_bwd_workspace_bytes((int)(R * S), precision));
        b.bwd_f = take<void>(plnerf_mlp_bwd_workspace_bytes((int)(R * F), precision));
        b.uniq_f = unique ? take<void>(plnerf_mlp_unique_workspace_bytes((int)(R * F))) : nullptr;
        return b;
    }
};

// ---- the stages ----

// a pass's density noise over its K samples per ray (counter stream `noise_stream`): behind the network, whichever ran
static inline int density_noise(const Pass& ps, const Samples& s, int K, uint32_t noise_stream, plnerf_stream_t stream) {
    int rc;
    if (s.noise) {
        STEP_OK(plnerf_normal(ps.seed, noise_stream, ps.step, ps.ray_id0, ps.R, K, s.noise, stream));
        if (ps.raw_noise_std != 1.0f)
            STEP_OK(scale2(s.noise, (size_t)ps.R * K, nullptr, 0, ps.raw_noise_std, (hipStream_t)stream));
    }
    return PLNERF_OK;
}

// Does a pass of K samples per ray take the unique-row forward (uniq_ws: its workspace, NULL = the entry has none)?  The
// library's host-side predicate, and no density activation (the backward would want the activated output in compact order).
// An entry asks ONCE per step, ahead of the forward, and hands forward() and backward_nets() the answer as the workspace
// pointer -- given: the route, NULL: the plain forward -- so that the forward and the backward's fold cannot disagree (the
// predicate reads the environment's switches at every call).
static inline bool unique_pass(const Pass& ps, int K, bool training, const void* uniq_ws) {
    return uniq_ws && !(ps.density_beta > 0.0f) &&
           plnerf_mlp_fwd_unique_served(ps.precision, 0, ps.fwd_kernel, K, ps.R * K, training ? 1 : 0) != 0;
}

// one network of the compiled trunk over a pass's K samples per ray, then that pass's density noise
// (uniq_ws: not NULL for a fine pass that takes the unique-row forward, as unique_pass() decided -- runs of bit-identical rows
// are evaluated at their ends)
static inline int network(const Pass& ps, const Rays& r, const void* packed, const Samples& s, int K, uint32_t noise_stream,
                          plnerf_stream_t stream, void* uniq_ws = nullptr) {
    int rc;
    if (uniq_ws)
        STEP_OK(plnerf_mlp_fwd_unique(packed, ps.precision, s.pts, r.viewdirs, ps.input_ch, ps.input_ch_views, ps.R * K, K,
                                      ps.input_scale, ps.density_beta, s.raw, s.saved, ps.fwd_kernel, uniq_ws, stream));
    else
        STEP_OK(plnerf_mlp_fwd(packed, ps.precision, s.pts, r.viewdirs, nullptr, ps.input_ch, ps.input_ch_views, ps.R * K, K,
                               ps.input_scale, ps.density_beta, s.raw, s.saved, ps.fwd_kernel, stream));
    return density_noise(ps, s, K, noise_stream, stream);
}

// The forward up to the fine network's raw output and noise: coarse samples -> coarse network -> coarse epilogue (the coarse
// maps, the fine pass's depths and points) -> fine network.  r.o / r.d: the rays the samples lie on (the NDC ones under
// ndc; r.viewdirs stay the camera-space rays').  net_c, net_f: the network stage of either pass, (samples, K, noise stream)
// -> code: network() for the compiled trunk (forward() below), another body for a network outside it.
template <class NetC, class NetF>
static inline int forward_with(const Pass& ps, const Rays& r, NetC&& net_c, NetF&& net_f, const Samples& c, const Samples& f,
                               const CoarseMaps& m, plnerf_stream_t stream) {
    const int R = ps.R, S = ps.S, N = ps.N;
    const float* u = ps.perturb ? nullptr : ps.u_vals;
    int rc;
    STEP_OK(plnerf_coarse_samples(r.o, r.d, r.near, r.far, ps.t_vals, nullptr, ps.seed, ps.step, ps.ray_id0, R, S, ps.lindisp,
                                  ps.perturb, c.z, c.pts, stream));
    STEP_OK(net_c(c, S, NOISE_STREAM));
    if (ps.mode == PLNERF_MODE_LINEAR)
        STEP_OK(plnerf_coarse_epilogue(c.raw, c.z, r.near, r.far, r.o, r.d, c.noise, u, 0, ps.seed, ps.step, ps.ray_id0, R, S, N,
                                       ps.color_mode, ps.white_bkgd, ps.farcolorfix, ps.zero_tol, ps.epsilon, m.rgb0, m.disp0,
                                       m.acc0, m.depth0, nullptr, nullptr, nullptr, f.z, f.pts, m.z_std, stream));
    else
        STEP_OK(plnerf_coarse_epilogue_const(c.raw, c.z, r.near, r.far, r.o, r.d, c.noise, u, 0, ps.seed, ps.step, ps.ray_id0, R, S,
                                             N, ps.white_bkgd, m.rgb0, m.disp0, m.acc0, m.depth0, nullptr, f.z, f.pts, m.z_std,
                                             stream));
    return net_f(f, S + N, NOISE_STREAM + 1);
}

// ... with both networks on the compiled trunk
// (uniq_f: the fine pass's unique-row workspace where unique_pass() said yes, else NULL; the coarse pass's jittered depths
// never repeat)
static inline int forward(const Pass& ps, const Rays& r, const void* packed_c, const void* packed_f, const Samples& c,
                          const Samples& f, const CoarseMaps& m, plnerf_stream_t stream, void* uniq_f = nullptr) {
    const auto trunk = [&](const void* packed, void* uniq_ws) {
        return [&ps, &r, packed, stream, uniq_ws](const Samples& s, int K, uint32_t noise_stream) {
            return network(ps, r, packed, s, K, noise_stream, stream, uniq_ws);
        };
    };
    return forward_with(ps, r, trunk(packed_c, nullptr), trunk(packed_f, uniq_f), c, f, m, stream);
}

// The depth variant's last stage: the fine maps, and N depth hypotheses per ray drawn from the final weights with their
// spread h.z_std.  u_in: the hypotheses' draws (a table or one row), NULL: drawn in the kernel; h.u_used: NULL unless a
// backward wants the draws.  Linear mode leaves weights [R,F+1] in h.w and the knots in h.tau / h.T [R,F+2]; constant mode
// leaves its weights [R,F] in the tau plane and its bins [R,F-1] in the T plane, and h.w untouched.
static inline int depth_last_stage(const Pass& ps, const Rays& r, const Samples& f, const float* u_in, const FineMaps& m,
                                   const HypPlanes& h, plnerf_stream_t stream) {
    const int F = ps.S + ps.N;
    if (ps.mode == PLNERF_MODE_LINEAR)
        return plnerf_fine_epilogue(f.raw, f.z, r.near, r.far, r.d, f.noise, u_in, 0, ps.seed, ps.step, ps.ray_id0, ps.R, F, ps.N,
                                    ps.color_mode, ps.white_bkgd, ps.farcolorfix, ps.zero_tol, ps.epsilon, m.rgb, m.disp, m.acc,
                                    m.depth, h.w, h.tau, h.T, h.hyp, h.inds, h.u_used, h.z_std, stream);
    return plnerf_fine_epilogue_const(f.raw, f.z, r.near, r.far, r.d, f.noise, u_in, 0, ps.seed, ps.step, ps.ray_id0, ps.R, F, ps.N,
                                      ps.white_bkgd, m.rgb, m.disp, m.acc, m.depth, h.tau, h.T, h.hyp, h.inds, h.u_used, h.z_std,
                                      stream);
}

// The backward of both networks, behind the last stage's own (which left d loss / d raw of the fine pass in b.g_raw_f and
// its max |g_raw| in b.absmax_f): d loss / d raw of the coarse pass from g_rgb0, then both networks at once.  Gradient k of
// a network goes to the offset of grad_flat its parameter k has in param_flat, the range status to grad_flat[n_params].
static inline int backward_nets(const Pass& ps, const Rays& r, const Samples& c, const Samples& f, const float* g_rgb0,
                                const Backward& b, int layout, const plnerf_step_net* coarse, const plnerf_step_net* fine,
                                plnerf_stream_t stream) {
    const int R = ps.R, S = ps.S, F = ps.S + ps.N;
    int rc;
    STEP_OK(plnerf_quad_bwd(c.raw, c.z, r.near, r.far, r.d, c.noise, R, S, ps.mode, ps.color_mode, ps.white_bkgd, ps.farcolorfix,
                            g_rgb0, nullptr, nullptr, nullptr, nullptr, nullptr, b.g_raw_c, b.absmax_c, stream));
    const plnerf_step_net* nets[2] = {coarse, fine};
    float* grads[2 * PLNERF_N_PARAM_TENSORS];
    for (int j = 0; j < 2; ++j)
        for (int i = 0; i < PLNERF_N_PARAM_TENSORS; ++i)
            grads[j * PLNERF_N_PARAM_TENSORS + i] = nets[j]->grad_flat + (nets[j]->params[i] - nets[j]->param_flat);
    const int groups = (R + PLNERF_QUAD_RAYS_PER_GROUP - 1) / PLNERF_QUAD_RAYS_PER_GROUP;
    // (max |g_raw| as the quadrature's by-product serves networks WITHOUT a density activation only: with one, the
    // backward scales by the maximum behind the activation's derivative and takes its own pass over raw_out, which it
    // does not look at otherwise)
    const bool by_product = !(ps.density_beta > 0.0f);
    const void* packed[2] = {coarse->packed, fine->packed};
    const float* g_raw[2] = {b.g_raw_c, b.g_raw_f};
    const uint32_t* absmax[2] = {by_product ? b.absmax_c : nullptr, by_product ? b.absmax_f : nullptr};
    int n_absmax[2] = {by_product ? groups : 0, by_product ? groups : 0};
    if (b.uniq_f) {
        // the fine forward ran over its needed rows (the entry's one unique_pass() decision: b.uniq_f is what forward() was
        // given): its saved planes are in compact order, and so must the gradient be -- folded, with the launch scale's
        // candidates taken from the FOLDED gradient in place of the quadrature's (unique_pass() admits no density
        // activation, so by_product holds here)
        plnerf_unique_layout lo;
        STEP_OK(plnerf_mlp_unique_layout(R * F, &lo));
        STEP_OK(plnerf_mlp_unique_fold(b.g_raw_f, R * F, b.uniq_f, stream));
        g_raw[1] = (const float*)((const unsigned char*)b.uniq_f + lo.g_raw_u);
        absmax[1] = (const uint32_t*)((const unsigned char*)b.uniq_f + lo.absmax);
        n_absmax[1] = (int)lo.n_absmax;
    }
    const int n_rows[2] = {R * S, R * F};
    const void* saved[2] = {c.saved, f.saved};
    const int layouts[2] = {layout, layout};
    const float* raw_out[2] = {by_product ? nullptr : c.raw, by_product ? nullptr : f.raw};
    void* bwd_ws[2] = {b.bwd_c, b.bwd_f};
    float* status_out[2] = {coarse->grad_flat + coarse->n_params, fine->grad_flat + fine->n_params};
    return plnerf_mlp_bwd_multi(2, packed, ps.precision, g_raw, absmax, n_absmax, ps.input_ch, ps.input_ch_views, n_rows, saved,
                                layouts, raw_out, ps.density_beta, bwd_ws, grads, status_out, stream);
}

// Where the block of a view that starts at pixel `at` writes its maps: into the caller's frame planes at the block's offset;
// a plane the caller left out: this block's values go to the workspace (ws)
template <typename Io>
static inline ViewMaps block_maps(const Io* io, size_t at, const ViewMaps& ws) {
    const auto plane = [at](float* given, size_t width, float* left_out) { return given ? given + width * at : left_out; };
    ViewMaps m{};
    m.fine.rgb = io->rgb + 3 * at;
    m.fine.disp = plane(io->disp, 1, ws.fine.disp);
    m.fine.acc = plane(io->acc, 1, ws.fine.acc);
    m.fine.depth = plane(io->depth, 1, ws.fine.depth);
    m.coarse.rgb0 = plane(io->rgb0, 3, ws.coarse.rgb0);
    m.coarse.disp0 = plane(io->disp0, 1, ws.coarse.disp0);
    m.coarse.acc0 = plane(io->acc0, 1, ws.coarse.acc0);
    m.coarse.depth0 = plane(io->depth0, 1, ws.coarse.depth0);
    m.coarse.z_std = plane(io->z_std, 1, ws.coarse.z_std);
    return m;
}

}  // namespace plnerf_step
